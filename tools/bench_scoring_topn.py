"""Time of top-N scoring (cc_logprob_topn) beside cc_logprob_rows of the same build, and of a teacher-forced generation with
`logprobs=True, top_logprobs=20` against `logprobs=True` alone -> profiles/scoring_topn.jsonl (one JSON row per line).

    python tools/bench_scoring_topn.py                 # the kernel rows + the 256-token teacher-forced generation
    python tools/bench_scoring_topn.py --no_generate   # the kernel rows alone

Kernel rows: as tools/bench_scoring.py times them (HIP events around `--launches` back-to-back calls on one stream, after a warm-up,
eager and under hipGraph replay), T = 1 and 4 rows at V = 32000 and 128256 (bf16): cc_logprob_rows, then cc_logprob_topn at N = 1, 5
and 20, with the extra time over cc_logprob_rows.  The baseline of every difference and ratio is cc_logprob_rows.
Generation: bench_scoring.py's set-up (the Llama-3-8B shape with random weights, bf16, a 512-token prompt, heavy_hitter at 4096
slots, 256 forced tokens) in its three loops — eager one-token steps, the hipGraph decoder, forced_block = 4 — each with
`top_logprobs=20` and without, in alternating order, `--rounds` times; tokens/s is the median over the decode phase, and the
microseconds per token that the alternatives cost are 1e6 / on - 1e6 / off of the medians.  The baseline is the `logprobs=True` loop."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cold_compress_amd.harness import (CONFIGS, GraphedDecoder, ModelArgs, Transformer, decode_one_token, generate, glue,  # noqa: E402
                                       prefill, setup_caches)

NS = (1, 5, 20)


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
            logits = (torch.randn(T, V, generator=torch.Generator().manual_seed(V)) * 3).to(torch.bfloat16).to(dev)
            targets = torch.randint(0, V, (T,), generator=torch.Generator().manual_seed(T), dtype=torch.int32).to(dev)
            rows = [("cc_logprob_rows", None, lambda: glue.logprob_rows(logits, targets))]
            rows += [("cc_logprob_topn", n, lambda n=n: glue.logprob_topn(logits, n, targets)) for n in NS]
            base = None
            for name, n, fn in rows:
                us = timed(fn, launches)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    fn()
                us_graph = timed(g.replay, launches)
                row = {"what": "kernel", "V": V, "T": T, "dtype": "bf16", "path": name, "N": n, "launches": launches,
                       "us_per_call_eager": round(us, 2), "us_per_call_graph": round(us_graph, 2)}
                if base is None:
                    base = (us, us_graph)
                else:
                    row["extra_us_over_logprob_rows"] = {"eager": round(us - base[0], 2), "graph": round(us_graph - base[1], 2)}
                out(row)


def generation(dev, tokens, rounds, top_n, out):
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
    assert model.block_eligible()
    V = cfg["vocab_size"]
    prompt = torch.randint(0, V, (512,), generator=torch.Generator().manual_seed(1), dtype=torch.int32).to(dev)
    forced = torch.randint(0, V, (tokens,), generator=torch.Generator().manual_seed(2), dtype=torch.int32).to(dev)
    decoders = {None: GraphedDecoder(model, logprobs=True), top_n: GraphedDecoder(model, logprobs=True, top_logprobs=top_n)}
    loops = {"eager_1": lambda n: (decode_one_token, {}), "graphed_1": lambda n: (decoders[n], {}),
             "block_4": lambda n: (decode_one_token, {"forced_block": 4})}
    runs = [(loop, n) for loop in loops for n in (None, top_n)]
    res = {r: [] for r in runs}
    same = {}

    def one(loop, n):
        dec, extra = loops[loop](n)
        for l in model.layers:
            l.attention.kv_cache.reset()
        torch.cuda.synchronize()
        seq, second, stats = generate(model, prompt, prefill, dec, max_new_tokens=tokens, next_tokens=forced, logprobs=True,
                                      top_logprobs=n, **extra)
        torch.cuda.synchronize()
        same.setdefault(loop, {})[n] = second.logprob.clone()
        return stats["decode_toks_per_sec"]

    for r in runs:  # one untimed pass of every run: captures, workspaces, clocks
        one(*r)
    for k in range(rounds):
        for r in runs[k % len(runs):] + runs[:k % len(runs)]:  # alternating order
            res[r].append(one(*r))
    for loop in loops:
        off, on = res[(loop, None)], res[(loop, top_n)]
        m_off, m_on = statistics.median(off), statistics.median(on)
        out({"what": "generate", "shape": "Meta-Llama-3-8B-Instruct", "prompt": 512, "forced_tokens": tokens, "loop": loop, "rounds": rounds,
             "top_logprobs": top_n,
             "decode_tok_s_logprobs_only": {"median": round(m_off, 1), "min": round(min(off), 1), "max": round(max(off), 1)},
             "decode_tok_s_top_logprobs": {"median": round(m_on, 1), "min": round(min(on), 1), "max": round(max(on), 1)},
             "top_over_logprobs_only": round(m_on / m_off, 4), "extra_us_per_token": round(1e6 / m_on - 1e6 / m_off, 2),
             "logprob_bits_equal": bool(torch.equal(same[loop][None].view(torch.int32), same[loop][top_n].view(torch.int32)))})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=400)
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--top_logprobs", type=int, default=20)
    ap.add_argument("--no_generate", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scoring_topn.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    fh = open(a.out, "w")

    def out(row):
        line = json.dumps(row)
        print(line, flush=True)
        fh.write(line + "\n")
        fh.flush()

    with torch.no_grad():
        out({"what": "device", "name": torch.cuda.get_device_name(0)})
        kernels(dev, a.launches, out)
        if not a.no_generate:
            generation(dev, a.tokens, a.rounds, a.top_logprobs, out)
    fh.close()


if __name__ == "__main__":
    main()
