"""Time of per-token scoring (cc_logprob_rows) beside the greedy tail, and of a teacher-forced generation with `logprobs=True`
against `logprobs=False` -> profiles/scoring.jsonl (one JSON row per line).

    python tools/bench_scoring.py                 # the kernel rows + the 256-token teacher-forced generation
    python tools/bench_scoring.py --no_generate   # the kernel rows alone

Kernel rows: HIP events around `--launches` back-to-back calls on one stream, after a warm-up, T = 1 and 4 rows at V = 32000 and
128256 (bf16), eager and under hipGraph replay, beside cc_softmax_argmax of the same run (T = 4: four calls of it, what four greedy
steps pay); the logits stay resident in L2 between the calls, as they are behind the LM head of a decode step.
Generation: the Llama-3-8B shape with random weights (bf16), a 512-token prompt, heavy_hitter at 4096 slots, 256 forced tokens
through generate(next_tokens=...) in three loops — eager one-token steps, the hipGraph decoder, forced_block = 4 — each with
logprobs on and off in alternating order, `--rounds` times; tokens/s is the median over the decode phase (closed by a device
synchronise).  Memory: the allocator's peak statistics are reset before each run; the peak above the run's start (at this prompt it is
the prefill's own [1, 512, V] logits, in both modes), what generate()'s second result keeps allocated when the run returns (the
V-sized rows against the scores), and generate()'s own `memory_used_gb` (peak reserved)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cold_compress_amd.harness import (CONFIGS, GraphedDecoder, ModelArgs, Transformer, decode_one_token, generate, glue,  # noqa: E402
                                       perplexity, prefill, setup_caches)


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
            rows = [("cc_logprob_rows", lambda: glue.logprob_rows(logits, targets)),
                    ("cc_softmax_argmax", lambda: [glue.softmax_argmax(logits[t]) for t in range(T)])]
            for name, fn in rows:
                us = timed(fn, launches)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    fn()
                us_graph = timed(g.replay, launches)
                out({"what": "kernel", "V": V, "T": T, "dtype": "bf16", "path": name, "launches": launches,
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
    assert model.block_eligible()
    V = cfg["vocab_size"]
    prompt = torch.randint(0, V, (512,), generator=torch.Generator().manual_seed(1), dtype=torch.int32).to(dev)
    forced = torch.randint(0, V, (tokens,), generator=torch.Generator().manual_seed(2), dtype=torch.int32).to(dev)
    decoders = {False: GraphedDecoder(model), True: GraphedDecoder(model, logprobs=True)}
    loops = {"eager_1": lambda lp: (decode_one_token, {}), "graphed_1": lambda lp: (decoders[lp], {}),
             "block_4": lambda lp: (decode_one_token, {"forced_block": 4})}
    runs = [(loop, lp) for loop in loops for lp in (False, True)]
    res = {r: dict(tps=[], peak=[], reserved=[], held=[]) for r in runs}
    ppl = {}

    def one(loop, lp):
        dec, extra = loops[loop](lp)
        for l in model.layers:
            l.attention.kv_cache.reset()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        seq, second, stats = generate(model, prompt, prefill, dec, max_new_tokens=tokens, next_tokens=forced, logprobs=lp, **extra)
        torch.cuda.synchronize()
        peak = (torch.cuda.max_memory_allocated() - base) / 1e9
        held = (torch.cuda.memory_allocated() - base) / 1e9  # what the returned rows / scores keep alive
        if lp:
            ppl[loop] = perplexity(second.logprob, every=None)["ppl"]
        del second
        return stats["decode_toks_per_sec"], peak, stats["memory_used_gb"], held

    for r in runs:  # one untimed pass of every run: captures, workspaces, clocks
        one(*r)
    for k in range(rounds):
        for r in runs[k % len(runs):] + runs[:k % len(runs)]:  # alternating order
            tps, peak, reserved, held = one(*r)
            res[r]["held"].append(held)
            res[r]["tps"].append(tps)
            res[r]["peak"].append(peak)
            res[r]["reserved"].append(reserved)
    for loop in loops:
        off, on = res[(loop, False)], res[(loop, True)]
        m_off, m_on = statistics.median(off["tps"]), statistics.median(on["tps"])
        out({"what": "generate", "shape": "Meta-Llama-3-8B-Instruct", "prompt": 512, "forced_tokens": tokens, "loop": loop, "rounds": rounds,
             "decode_tok_s_logprobs_off": {"median": round(m_off, 1), "min": round(min(off["tps"]), 1), "max": round(max(off["tps"]), 1)},
             "decode_tok_s_logprobs_on": {"median": round(m_on, 1), "min": round(min(on["tps"]), 1), "max": round(max(on["tps"]), 1)},
             "on_over_off": round(m_on / m_off, 4),
             "peak_allocated_above_start_gb": {"off": round(max(off["peak"]), 4), "on": round(max(on["peak"]), 4)},
             "held_by_second_result_gb": {"off": round(max(off["held"]), 6), "on": round(max(on["held"]), 6)},
             "memory_used_gb": {"off": round(max(off["reserved"]), 3), "on": round(max(on["reserved"]), 3)},
             "ppl_logprobs_on": ppl.get(loop)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=400)
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no_generate", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scoring.jsonl"))
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
            generation(dev, a.tokens, a.rounds, out)
    fh.close()


if __name__ == "__main__":
    main()
