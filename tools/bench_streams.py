#!/usr/bin/env python
"""Up to four sequences decoded in lock-step (harness/streams.py) against the one-token loop, at the benchmark's shape: Llama-3-8B
(bf16, random weights), heavy_hitter, cache 4096.  Behind one prefill, a fork into four cache sets and a settling run, free tokens
are decoded with

    graphed_1          the hipGraph one-token loop with the 12-bit packed weights on (what generate() callers run today)
    eager_N            N = 2, 3, 4 streams, eager joint steps       (one cc_gemv_fused_multi pass per matrix, N cache steps per layer)
    graphed_N          N = 2, 3, 4 streams, the captured joint step (GraphedStreamsDecoder)

in alternating order, `--rounds` times each, on one device in one process; tokens/s is the AGGREGATE over the streams, median
(min - max).  Every streams mode reads the single-launch status word behind every joint step, as generate_streams does.  The
one-token loop runs on stream 0, which the streams modes step too: every mode continues each sequence where the last run left it.
Prints one JSON object; profiles/streams.md is written from it.

--weights int8 / mxfp4 / int4 (--groupsize G) quantises the random model with the weight-only handler and sets the matching opt-in
attribute (Transformer.block_weight_only / block_int4).  Such runs add

    serial_N           N = 2, 3, 4 streams, one stream at a time per step (decode_one_token on each stream's caches): the route these
                       models take with the attribute off

Default bf16: as it was.

    python tools/bench_streams.py [--n_layer 32] [--tokens 128] [--rounds 5] [--temperature T --top_k K --top_p P]
                                  [--weights bf16|int8|mxfp4|int4] [--groupsize G] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_forced_block import build  # noqa: E402  (the same model, built the same way)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n_layer", type=int, default=32)
    ap.add_argument("--cache_len", type=int, default=4096)
    ap.add_argument("--prompt_len", type=int, default=4095)
    ap.add_argument("--tokens", type=int, default=128, help="decode steps per timed run (a streams run yields N times as many tokens)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--settle", type=int, default=160)
    ap.add_argument("--temperature", type=float, default=None, help="default: greedy, as bench.py decodes")
    ap.add_argument("--top_k", type=int, default=None)
    ap.add_argument("--top_p", type=float, default=None)
    ap.add_argument("--weights", default="bf16", choices=["bf16", "int8", "mxfp4", "int4"])
    ap.add_argument("--groupsize", type=int, default=128, choices=[32, 64, 128, 256], help="--weights int4: columns per group")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from cold_compress_amd.harness import DecodeStreams, GraphedDecoder, GraphedStreamsDecoder, decode_n_tokens, glue, prefill, setup_caches
    from cold_compress_amd.harness.streams import decode_streams

    dev = torch.device("cuda", 0)
    model = build(args.n_layer, dev, args.weights, args.groupsize)  # (sets the opt-in attribute of a weight-only model)
    ck = dict(max_cache_length=[float(args.cache_len)], cache_bits=None, cache_length_pattern="tile", cache_strategy=["heavy_hitter"],
              cache_strategy_pattern="tile", feed_long_prompts=False, prompt_compression_strategy=["heavy_hitter"], global_tokens=4,
              recent_window=10, history_window_size=1, attn_thresholding=False, min_recovery_frac=0.9)
    setup_caches(model, None, dev, 16384, ck)
    streams4 = DecodeStreams(model, 4)
    assert model.streams_eligible(streams4) and (args.weights != "bf16" or glue.w12_enabled())
    gen = torch.Generator().manual_seed(7)
    V = model.config.vocab_size
    prompt = torch.randint(0, V, (args.prompt_len,), generator=gen, dtype=torch.int32).to(dev)
    skw = dict(temperature=args.temperature, top_k=args.top_k, top_p=args.top_p)
    with torch.no_grad():
        first, _ = prefill(model, prompt.view(1, -1), torch.arange(args.prompt_len, device=dev))
        streams4.fork()
        tok = first.view(1, 1).to(torch.int32).expand(1, 4).contiguous()  # every stream's next input token ...
        pos = torch.full((4,), args.prompt_len, dtype=torch.int32, device=dev)  # ... and its position
        graphed = GraphedDecoder(model, seed=0, **skw)
        decs = {n: GraphedStreamsDecoder(model, streams4.first(n), range(n), args.temperature, args.top_k, args.top_p) for n in (2, 3, 4)}

        def one_token(steps):
            p = pos[:1].clone()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            toks, _ = decode_n_tokens(model, tok[:, :1].clone(), p, graphed, steps, seed=0, **skw)  # (advances p in place)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            tok[0, :1] = toks[-1].view(1)
            pos[:1] = p
            return steps / dt

        def joint(n, graph_it, steps, serial=False):
            dec = decs[n] if graph_it else None
            settings = (tuple(range(n)), args.temperature, args.top_k, args.top_p, None, False)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            toks, _, _, dec2 = decode_streams(model, streams4.first(n), tok[:, :n].contiguous(), pos[:n].clone(), steps, settings, dec=dec,
                                                  joint=not serial)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert dec2 is dec, "the capture of the joint step was refused"
            tok[0, :n] = toks[-1]
            pos[:n] += steps
            return n * steps / dt

        one_token(args.settle)  # clocks settle, the graph is captured, the packed copies exist (bench.py does the same)
        modes = {"graphed_1": lambda steps: one_token(steps)}
        for n in (2, 3, 4):
            modes[f"eager_{n}"] = (lambda n: lambda steps: joint(n, False, steps))(n)
            modes[f"graphed_{n}"] = (lambda n: lambda steps: joint(n, True, steps))(n)
        if args.weights != "bf16":
            for n in (2, 3, 4):
                modes[f"serial_{n}"] = (lambda n: lambda steps: joint(n, False, steps, serial=True))(n)
        names = list(modes)
        for m in names:  # one untimed pass of every mode (captures included)
            modes[m](16)
        tps = {m: [] for m in names}
        for r in range(args.rounds):
            for m in names[r % len(names):] + names[:r % len(names)]:  # alternating order
                tps[m].append(modes[m](args.tokens))
    width = {m: 1 if m == "graphed_1" else int(m.split("_")[1]) for m in names}
    out = {"shape": "Meta-Llama-3-8B-Instruct", "weights": args.weights, **({"groupsize": args.groupsize} if args.weights == "int4" else {}),
           "n_layer": args.n_layer, "cache_len": args.cache_len, "steps_per_run": args.tokens,
           "rounds": args.rounds, "sampling": skw, "device": torch.cuda.get_device_name(0),
           "cache_set_gb": round(sum(b.numel() * b.element_size() for c in streams4.sets[1] for b in c._buffers.values() if b is not None) / 1e9, 3),
           "aggregate_tokens_per_s": {m: {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}
                                      for m, v in tps.items()},
           "ms_per_step": {m: round(1e3 * width[m] / statistics.median(v), 3) for m, v in tps.items()}}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
