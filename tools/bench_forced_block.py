#!/usr/bin/env python
"""Known tokens fed four at a time (decode_n_tokens' forced_block) against the token-by-token loop, at the benchmark's shape:
Llama-3-8B (bf16, random weights), heavy_hitter, cache 4096.  Behind a prefill and a settling run, 256 forced tokens are fed with

    forced_block = 1, eager launches      (the loop as it is without forced_block)
    forced_block = 1, hipGraph decoder    (what generate() callers run today)
    forced_block = 4                      (blocks are eager launches; status word read behind each block)
    forced_block = 4, recover=False       (no status read: the host runs ahead of the device)
    forced_block = 4, captured blocks     (block_decoder=GraphedBlockDecoder: each block one hipGraph replay)

in alternating order, `--rounds` times each; tokens/s is the median.  Then the HIP-event time of cc_gemv_fused_multi (T = 4) against
cc_gemv_fused per matrix (wqkv, wo, w1/w3, w2 over the 32 layers' own weights, so every launch streams cold weights; the LM head).
Prints one JSON object; profiles/forced_block.md and profiles/forced_block_graph.md are written from it.  --no_gemv leaves the
per-matrix part out.

--weights int8 / mxfp4 quantises the random model with the weight-only handler (harness/quantize.py, as tools/run_configs.py
--weights does) and sets Transformer.block_weight_only: the blocks and the per-matrix table then run cc_gemv_fused_w8_multi /
cc_gemv_fused_mx4_multi against cc_gemv_fused_w8 / cc_gemv_fused_mx4 (profiles/forced_block_weight_only.md).  --weights int4
--groupsize G does the same with the int4 handler and Transformer.block_int4: cc_gemv_fused_w4_multi against cc_gemv_fused_w4
(profiles/w4_multi.md).  Default bf16: as it was.

    python tools/bench_forced_block.py [--n_layer 32] [--tokens 256] [--rounds 5] [--weights bf16|int8|mxfp4|int4] [--groupsize G] [--no_gemv] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build(n_layer, dev, weights="bf16", groupsize=128):
    from cold_compress_amd.harness import CONFIGS, ModelArgs, Transformer

    cfg = dict(CONFIGS["Meta-Llama-3-8B-Instruct"], n_layer=n_layer, block_size=16384)
    torch.manual_seed(1234)
    with torch.device("meta"):
        model = Transformer(ModelArgs(**cfg))
    model = model.to_empty(device=dev).to(torch.bfloat16)
    g = torch.Generator(device=dev).manual_seed(1234)
    with torch.no_grad():
        for name, p in model.named_parameters():
            p.fill_(1.0) if "norm" in name else p.normal_(0.0, 0.02, generator=g)
    model.eval()
    if weights != "bf16":
        from cold_compress_amd.harness.quantize import WeightOnlyInt4QuantHandler, WeightOnlyInt8QuantHandler, WeightOnlyMxfp4QuantHandler

        handler = {"int8": WeightOnlyInt8QuantHandler, "mxfp4": WeightOnlyMxfp4QuantHandler,
                   "int4": lambda m: WeightOnlyInt4QuantHandler(m, groupsize)}[weights]
        sd = handler(model).create_quantized_state_dict()
        del model
        with torch.device("meta"):
            model = handler(Transformer(ModelArgs(**cfg))).convert_for_runtime()
        model.load_state_dict(sd, assign=True)
        model = model.to(device=dev, dtype=torch.bfloat16).eval()
        del sd
        torch.cuda.empty_cache()
        if weights == "int4":
            model.block_int4 = True  # (callers that want the per-token route clear it)
        else:
            model.block_weight_only = True
    return model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n_layer", type=int, default=32)
    ap.add_argument("--cache_len", type=int, default=4096)
    ap.add_argument("--prompt_len", type=int, default=4095)
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--settle", type=int, default=160)
    ap.add_argument("--weights", default="bf16", choices=["bf16", "int8", "mxfp4", "int4"])
    ap.add_argument("--groupsize", type=int, default=128, choices=[32, 64, 128, 256], help="--weights int4: columns per group")
    ap.add_argument("--no_gemv", action="store_true", help="the loop modes only: no per-matrix GEMV table")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from cold_compress_amd.harness import GraphedBlockDecoder, GraphedDecoder, decode_n_tokens, decode_one_token, glue, prefill, setup_caches
    from cold_compress_amd.harness.model import _gemv_multi, _quant

    dev = torch.device("cuda", 0)
    model = build(args.n_layer, dev, args.weights, args.groupsize)
    ck = dict(max_cache_length=[float(args.cache_len)], cache_bits=None, cache_length_pattern="tile", cache_strategy=["heavy_hitter"],
              cache_strategy_pattern="tile", feed_long_prompts=False, prompt_compression_strategy=["heavy_hitter"], global_tokens=4,
              recent_window=10, history_window_size=1, attn_thresholding=False, min_recovery_frac=0.9)
    setup_caches(model, None, dev, 16384, ck)
    assert model.block_eligible()
    gen = torch.Generator().manual_seed(7)
    V = model.config.vocab_size
    prompt = torch.randint(0, V, (args.prompt_len,), generator=gen, dtype=torch.int32).to(dev)
    with torch.no_grad():
        tok, _ = prefill(model, prompt.view(1, -1), torch.arange(args.prompt_len, device=dev))
        pos = torch.tensor([args.prompt_len], dtype=torch.int32, device=dev)
        cur = tok.view(1, 1).to(torch.int32)
        graphed = GraphedDecoder(model)
        blocks = GraphedBlockDecoder(model)

        def feed(n, dec, **kw):
            nonlocal cur
            forced = torch.randint(0, V, (n,), generator=gen, dtype=torch.int32).to(dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            toks, _ = decode_n_tokens(model, cur, pos, dec, n, prefix=forced, **kw)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            cur = toks[-1].view(1, 1)
            return n / dt

        feed(args.settle, graphed)  # clocks settle, the graph is captured (bench.py does the same ahead of its timed region)
        modes = {"eager_1": (decode_one_token, {}), "graphed_1": (graphed, {}), "block_4": (decode_one_token, {"forced_block": 4}),
                 "block_4_norecover": (decode_one_token, {"forced_block": 4, "recover": False}),
                 "block_4_graph": (decode_one_token, {"forced_block": 4, "block_decoder": blocks})}
        names = list(modes)
        for m in names:  # one untimed pass of every mode
            feed(16, modes[m][0], **modes[m][1])
        tps = {m: [] for m in names}
        for r in range(args.rounds):
            for m in names[r % len(names):] + names[:r % len(names)]:  # alternating order
                tps[m].append(feed(args.tokens, modes[m][0], **modes[m][1]))

        # ---- per matrix: multi (T = 4) against single, HIP events over the layers' own (cold) weights
        def ev_us(fn, n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            return a.elapsed_time(b) * 1e3 / n

        L, cfg = model.layers, model.config
        HQ, H, D = cfg.n_head, cfg.n_local_heads, cfg.head_dim
        x4 = torch.randn(4, cfg.dim, device=dev).to(torch.bfloat16)
        d4 = torch.randn(4, cfg.dim, device=dev).to(torch.bfloat16)
        g4 = torch.randn(4, cfg.intermediate_size, device=dev).to(torch.bfloat16)
        fr4 = model.freqs_cis[torch.arange(4000, 4004, device=dev)]
        h4 = torch.empty_like(x4)
        rope = dict(rope_rows=(HQ + H) * D, head_dim=D)
        mats = {
            "wqkv": (len(L), lambda i, T: _gemv_multi(L[i].attention.wqkv, x4[:T], delta=d4[:T], norm_weight=L[i].attention_norm.weight,
                                                      h_out=h4[:T], freqs=fr4[:T], **rope),
                     lambda i: glue.gemv_fused(L[i].attention.wqkv.weight, x4[0], delta=d4[0], norm_weight=L[i].attention_norm.weight, h_out=h4[0],
                                               freqs=fr4[0], **rope, **_quant(L[i].attention.wqkv))),
            "wo": (len(L), lambda i, T: _gemv_multi(L[i].attention.wo, x4[:T]),
                   lambda i: glue.gemv_fused(L[i].attention.wo.weight, x4[0], **_quant(L[i].attention.wo))),
            "w1/w3": (len(L), lambda i, T: _gemv_multi(L[i].feed_forward.w1, x4[:T], w3=L[i].feed_forward.w3, delta=d4[:T],
                                                       norm_weight=L[i].ffn_norm.weight, h_out=h4[:T]),
                      lambda i: glue.gemv_fused(L[i].feed_forward.w1.weight, x4[0], w3=L[i].feed_forward.w3.weight, delta=d4[0],
                                                norm_weight=L[i].ffn_norm.weight, h_out=h4[0],
                                                **{**_quant(L[i].feed_forward.w1), **_quant(L[i].feed_forward.w3, "3")})),
            "w2": (len(L), lambda i, T: _gemv_multi(L[i].feed_forward.w2, g4[:T]),
                   lambda i: glue.gemv_fused(L[i].feed_forward.w2.weight, g4[0], **_quant(L[i].feed_forward.w2))),
            "lm_head": (1, lambda i, T: _gemv_multi(model.output, x4[:T], delta=d4[:T], norm_weight=model.norm.weight),
                        lambda i: glue.gemv_fused(model.output.weight, x4[0], delta=d4[0], norm_weight=model.norm.weight, **_quant(model.output))),
        }
        gemv = {}
        for name, (n, multi, single) in ({} if args.no_gemv else mats).items():
            reps = 4 if n > 1 else 8
            runs = {"single": lambda: [single(i) for _ in range(reps) for i in range(n)]}
            for T in (2, 3, 4):
                runs[f"multi_T{T}"] = (lambda T: lambda: [multi(i, T) for _ in range(reps) for i in range(n)])(T)
            for fn in runs.values():
                fn()
            us = {k: [] for k in runs}
            order = list(runs)
            for r in range(args.rounds):
                for k in order[r % len(order):] + order[:r % len(order)]:
                    us[k].append(ev_us(runs[k], reps * n))
            gemv[name] = {k: round(statistics.median(v), 2) for k, v in us.items()}
    out = {"shape": "Meta-Llama-3-8B-Instruct", "weights": args.weights, **({"groupsize": args.groupsize} if args.weights == "int4" else {}), "n_layer": args.n_layer, "cache_len": args.cache_len, "tokens": args.tokens, "rounds": args.rounds,
           "device": torch.cuda.get_device_name(0),
           "tokens_per_s": {m: {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)} for m, v in tps.items()},
           "ms_per_token": {m: round(1e3 / statistics.median(v), 3) for m, v in tps.items()},
           "captured_blocks": {"captures": blocks.captures, "replays": blocks.replays, "keys": sorted(blocks.keys())}, "gemv_us": gemv}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
