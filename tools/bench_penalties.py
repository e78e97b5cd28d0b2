"""What the token-history penalties (cc_logits_penalize, one launch per decode step) cost -> profiles/logit_penalties.md.

    python tools/bench_penalties.py

Kernel rows: HIP events around `--launches` back-to-back calls on one stream after a warm-up, bf16, T = 1 and 4 rows at
V = 32000 and 128256, eager and under hipGraph replay; the rows, the counts and the bias stay resident in L2 between the calls, as
the logits are behind the LM head of a decode step.
Generation: the Llama-3-8B shape with random weights (bf16), a 512-token prompt, heavy_hitter at 4096 slots, `--tokens` free greedy
tokens through generate() with the hipGraph decoder, with all three penalties and a bias on against `penalties=None`, in alternating
order, `--rounds` times after one untimed pass of each; the decode phase is closed by a device synchronise and the median is kept."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cold_compress_amd.harness import (CONFIGS, GraphedDecoder, LogitPenalties, ModelArgs, Transformer, generate, glue,  # noqa: E402
                                       prefill, setup_caches)


def timed(fn, launches, warmup=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / launches  # us


def kernels(dev, launches, out):
    for V in (32000, 128256):
        for T in (1, 4):
            g = torch.Generator().manual_seed(V + T)
            logits = (torch.randn(T, V, generator=g) * 3).to(torch.bfloat16).to(dev)
            pc = torch.randint(0, 3, (V,), generator=g, dtype=torch.int32).to(dev)
            gc = torch.randint(0, 3, (V,), generator=g, dtype=torch.int32).to(dev)
            gs = torch.tensor([100], dtype=torch.int32, device=dev)
            toks = torch.randint(0, V, (T,), generator=g, dtype=torch.int32).to(dev)
            pos = torch.arange(200, 200 + T, dtype=torch.int32).to(dev)
            bias = torch.randn(V, generator=g).to(dev)

            def fn():
                return glue.logits_penalize(logits, pc, gc, gs, toks, pos, 1.2, 0.3, 0.5, bias)

            us = timed(fn, launches)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                fn()
            us_graph = timed(graph.replay, launches)
            nbytes = V * (2 * T * 2 + 8 + 4)
            out({"what": "kernel", "V": V, "T": T, "dtype": "bf16", "launches": launches, "bytes": nbytes,
                 "us_per_call_eager": round(us, 2), "us_per_call_graph": round(us_graph, 2)})


def generation(dev, tokens, rounds, out):
    cfg = dict(CONFIGS["Meta-Llama-3-8B-Instruct"])
    cfg["block_size"] = 8192
    with torch.device("meta"):
        model = Transformer(ModelArgs(**cfg))
    model = model.to_empty(device=dev).to(torch.bfloat16)
    g = torch.Generator(device=dev).manual_seed(1234)
    for n, p in model.named_parameters():
        p.fill_(1.0) if "norm" in n else p.normal_(0.0, 0.02, generator=g)
    model.eval()
    kw = dict(max_cache_length=[4096.0], cache_bits=None, cache_length_pattern="tile", cache_strategy=["heavy_hitter"],
              cache_strategy_pattern="tile", feed_long_prompts=False, prompt_compression_strategy=["heavy_hitter"], global_tokens=4,
              recent_window=10, history_window_size=1, attn_thresholding=False, min_recovery_frac=0.9)
    setup_caches(model, None, dev, 4096, dict(kw))
    V = cfg["vocab_size"]
    prompt = torch.randint(0, V, (512,), generator=torch.Generator().manual_seed(1), dtype=torch.int32).to(dev)
    pen = LogitPenalties(V, dev, 1.2, 0.3, 0.5, {7: -float("inf"), 11: 1.5})
    runs = {False: (GraphedDecoder(model), None), True: (GraphedDecoder(model, penalties=pen), pen)}
    res = {False: [], True: []}

    def one(on):
        dec, p = runs[on]
        for l in model.layers:
            l.attention.kv_cache.reset()
        torch.cuda.synchronize()
        seq, _, stats = generate(model, prompt, prefill, dec, max_new_tokens=tokens, penalties=p)
        torch.cuda.synchronize()
        if on:  # the state the captured steps advanced is the histogram of what was fed
            assert int(p.prompt_count.sum()) == 512 and int(p.gen_count.sum()) == tokens - 1 and 7 not in seq[512:].tolist()
        return stats["decode_seconds"] / stats["decode_tokens"] * 1e3  # ms per token

    for on in (False, True):  # one untimed pass of each: the captures, the workspaces, the clocks
        one(on)
    for k in range(rounds):
        for on in ((False, True) if k % 2 == 0 else (True, False)):
            res[on].append(one(on))
    off, on = statistics.median(res[False]), statistics.median(res[True])
    out({"what": "generate", "shape": "Meta-Llama-3-8B-Instruct", "prompt": 512, "tokens": tokens, "loop": "graphed", "rounds": rounds,
         "ms_per_token_off": {"median": round(off, 4), "min": round(min(res[False]), 4), "max": round(max(res[False]), 4)},
         "ms_per_token_on": {"median": round(on, 4), "min": round(min(res[True]), 4), "max": round(max(res[True]), 4)},
         "added_us_per_token": round((on - off) * 1e3, 2), "on_over_off": round(on / off, 4)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=400)
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no_generate", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "logit_penalties.md"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    rows = []

    def out(row):
        print(json.dumps(row), flush=True)
        rows.append(row)

    with torch.no_grad():
        out({"what": "device", "name": torch.cuda.get_device_name(0)})
        kernels(dev, a.launches, out)
        if not a.no_generate:
            generation(dev, a.tokens, a.rounds, out)
    with open(a.out, "w") as fh:
        fh.write("# Logit penalties: what the one launch per step costs\n\n`python tools/bench_penalties.py` on one MI355X, bf16; one JSON "
                 "row per measurement (the tool's docstring says what each is).\n\n```\n")
        fh.writelines(json.dumps(r) + "\n" for r in rows)
        fh.write("```\n")


if __name__ == "__main__":
    main()
