"""What the sequence rules (cc_logits_constrain: a copy of the rows and a ban pass per decode step) cost -> profiles/logit_constraints.md.

    python tools/bench_constraints.py

Kernel rows: HIP events around `--launches` back-to-back calls on one stream after a warm-up, V = 128256, bf16, T = 1 and 4 rows,
history lengths 512 / 8192 / 65536 over an alphabet of 50, with no_repeat_ngram_size = 3, 8 banned sequences and a minimum length
on, into a new tensor (the copy pass runs), eager and under hipGraph replay; rows and history stay resident in L2 between the calls,
as the logits are behind the LM head of a decode step.  `model_us` is the project's cost model of stand-alone launches:
5.5 us + bytes / 6.5 TB/s for each of the two.
Generation: the Llama-3-8B shape with random weights (bf16), a 512-token prompt, heavy_hitter at 4096 slots, `--tokens` free greedy
tokens through generate() with the hipGraph decoder, with the same rules on against `constraints=None`, in alternating order,
`--rounds` times after one untimed pass of each; the decode phase is closed by a device synchronise and the median is kept."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cold_compress_amd.harness import (CONFIGS, GraphedDecoder, LogitConstraints, ModelArgs, Transformer, generate, glue,  # noqa: E402
                                       prefill, setup_caches)

BAD_WORDS = [[11, 12], [13, 14, 15], [16], [17, 18, 19, 20], [21, 22], [23, 24, 25], [26, 27], [28, 29, 30, 31, 32]]


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
    V = 128256
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)  # noqa: E731
    bw_tokens = i32([t for w in BAD_WORDS for t in w])
    offs = [0]
    for w in BAD_WORDS:
        offs.append(offs[-1] + len(w))
    bw_offsets, terms = i32(offs), i32([1, 2])
    for L in (512, 8192, 65536):
        for T in (1, 4):
            g = torch.Generator().manual_seed(L + T)
            logits = (torch.randn(T, V, generator=g) * 3).to(torch.bfloat16).to(dev)
            hist = torch.zeros(L + 64, dtype=torch.int32)
            hist[:L] = torch.randint(0, 50, (L,), generator=g, dtype=torch.int32) * 2565
            hist = hist.to(dev)
            gs = i32([100])
            toks = (torch.randint(0, 50, (T,), generator=g, dtype=torch.int32) * 2565).to(dev)
            pos = i32([L])

            def fn():
                return glue.logits_constrain(logits, hist, gs, toks, pos, 3, False, L + 64, terms, bw_tokens, bw_offsets)

            us = timed(fn, launches)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                fn()
            us_graph = timed(graph.replay, launches)
            copy_bytes, ban_bytes = 2 * T * V * 2, T * 4 * L
            model = 2 * 5.5 + (copy_bytes + ban_bytes) / 6.5e6
            out({"what": "kernel", "V": V, "T": T, "history": L, "dtype": "bf16", "launches": launches, "copy_bytes": copy_bytes,
                 "ban_bytes": ban_bytes, "model_us": round(model, 2), "us_per_call_eager": round(us, 2), "us_per_call_graph": round(us_graph, 2)})


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
    con = LogitConstraints(V, dev, 512 + tokens, no_repeat_ngram_size=3, min_new_tokens=tokens, terminator_ids=[1, 2], bad_words_ids=BAD_WORDS)
    runs = {False: (GraphedDecoder(model), None), True: (GraphedDecoder(model, constraints=con), con)}
    res = {False: [], True: []}

    def one(on):
        dec, c = runs[on]
        for l in model.layers:
            l.attention.kv_cache.reset()
        torch.cuda.synchronize()
        seq, _, stats = generate(model, prompt, prefill, dec, max_new_tokens=tokens, constraints=c)
        torch.cuda.synchronize()
        if on:  # the history the captured steps advanced is what was fed, and the rules held
            s = seq.tolist()
            assert c.hist[:len(s) - 1].tolist() == s[:-1] and not {1, 2, 16} & set(s[512:])
            assert len({tuple(s[i:i + 3]) for i in range(len(s) - 2)}) == len(s) - 2
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "logit_constraints.md"))
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
        fh.write("# Logit constraints: what the copy and the ban pass per step cost\n\n`python tools/bench_constraints.py` on one MI355X, bf16; "
                 "one JSON row per measurement (the tool's docstring says what each is).\n\n```\n")
        fh.writelines(json.dumps(r) + "\n" for r in rows)
        fh.write("```\n")


if __name__ == "__main__":
    main()
