#!/usr/bin/env python
"""What the per-stream logit processors cost in the captured joint step (harness/streams.py), at the benchmark's shape:
Llama-3-8B (bf16, random weights), heavy_hitter, cache 4096.  Behind one prefill, a fork into four cache sets and a settling run,
free tokens are decoded by captured joint steps of N = 4 and N = 2 streams with

    plain_N            no processors (tools/bench_streams.py's graphed_N)
    streams_N          a LogitPenalties and a LogitConstraints on every stream, through ONE cc_logits_penalize_streams and ONE
                       cc_logits_constrain_streams launch per step
    percall_N          the same objects through the single-sequence entry points, once per stream: a copy of the rows, then N
                       cc_logits_penalize and N cc_logits_constrain launches in place per step (what a caller could do before)
    baseline_N         (--baseline_streams FILE) plain_N run by ANOTHER revision's harness/streams.py, loaded beside the package's:
                       shows whether the path without processors changed

in alternating order, `--rounds` times each, on one device in one process; tokens/s is the AGGREGATE over the streams, median
(min - max).  Every mode continues each sequence where the last run left it; the processors' histories hold the prompt and what the
modes WITH processors fed (the others do not store their tokens), which is immaterial to the time: the ban pass walks the history
whatever it holds.  Prints one JSON object; profiles/streams_logits.md is written from it.

    python tools/bench_streams_logits.py [--n_layer 32] [--tokens 128] [--rounds 5] [--baseline_streams FILE] [--out FILE]"""
import argparse
import importlib.util
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
    ap.add_argument("--tokens", type=int, default=128, help="decode steps per timed run (a run yields N times as many tokens)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--settle", type=int, default=160)
    ap.add_argument("--max_positions", type=int, default=16384, help="the constraints' history: every mode's steps must fit")
    ap.add_argument("--baseline_streams", default=None, help="a harness/streams.py of another revision, timed as baseline_N")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from cold_compress_amd.harness import (DecodeStreams, GraphedStreamsDecoder, LogitConstraints, LogitPenalties, glue, prefill,
                                           setup_caches)
    from cold_compress_amd.harness import streams as S

    base = None
    if args.baseline_streams:
        spec = importlib.util.spec_from_file_location("cold_compress_amd.harness._streams_baseline", args.baseline_streams)
        base = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = base
        spec.loader.exec_module(base)

    dev = torch.device("cuda", 0)
    model = build(args.n_layer, dev, "bf16", 128)
    ck = dict(max_cache_length=[float(args.cache_len)], cache_bits=None, cache_length_pattern="tile", cache_strategy=["heavy_hitter"],
              cache_strategy_pattern="tile", feed_long_prompts=False, prompt_compression_strategy=["heavy_hitter"], global_tokens=4,
              recent_window=10, history_window_size=1, attn_thresholding=False, min_recovery_frac=0.9)
    setup_caches(model, None, dev, 16384, ck)
    streams4 = DecodeStreams(model, 4)
    assert model.streams_eligible(streams4) and glue.w12_enabled()
    gen = torch.Generator().manual_seed(7)
    V = model.config.vocab_size
    prompt = torch.randint(0, V, (args.prompt_len,), generator=gen, dtype=torch.int32).to(dev)
    pens = [LogitPenalties(V, dev, repetition_penalty=1.3, frequency_penalty=0.4, presence_penalty=0.2, logit_bias={9: -float("inf"), 17: 2.0})
            for _ in range(4)]
    cons = [LogitConstraints(V, dev, args.max_positions, no_repeat_ngram_size=2, min_new_tokens=6, terminator_ids=[2],
                             bad_words_ids=[[11, 12], [13]]) for _ in range(4)]
    for o in pens + cons:
        o.reset(prompt, args.prompt_len)

    def processed_per_call(logits, tok, pos, proc):
        """streams._processed through the single-sequence entry points: a copy of the rows, then every stream's two launches in place"""
        rows = logits[0].clone()
        tokens = tok.reshape(-1)
        for t, (p, c) in enumerate(zip(proc.pens, proc.cons)):
            row, tk, ps = rows[t:t + 1], tokens[t:t + 1], pos[t:t + 1]
            glue.logits_penalize(row, *p.record()[:3], tk, ps, *p.record()[3:], out=row)
            hist, gen_start, *rules = c.record()
            glue.logits_constrain(row, hist, gen_start, tk, ps, *rules, out=row)
        return rows.unsqueeze(0)

    with torch.no_grad():
        first, _ = prefill(model, prompt.view(1, -1), torch.arange(args.prompt_len, device=dev))
        streams4.fork()
        tok = first.view(1, 1).to(torch.int32).expand(1, 4).contiguous()  # every stream's next input token ...
        pos = torch.full((4,), args.prompt_len, dtype=torch.int32, device=dev)  # ... and its position
        decs, kinds = {}, ["plain", "streams", "percall"] + (["baseline"] if base is not None else [])
        for n in (4, 2):
            view = streams4.first(n)
            decs["plain", n] = GraphedStreamsDecoder(model, view, range(n))
            decs["streams", n] = GraphedStreamsDecoder(model, view, range(n), penalties=pens[:n], constraints=cons[:n])
            decs["percall", n] = GraphedStreamsDecoder(model, view, range(n), penalties=pens[:n], constraints=cons[:n])
            if base is not None:
                decs["baseline", n] = base.GraphedStreamsDecoder(model, view, range(n))

        def joint(kind, n, steps):
            dec, mod = decs[kind, n], base if kind == "baseline" else S
            assert pos.max().item() + steps < args.max_positions, "raise --max_positions"
            real = S._processed
            if kind == "percall":
                S._processed = processed_per_call
            try:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                toks, _, _, dec2 = mod.decode_streams(model, dec.streams, tok[:, :n].contiguous(), pos[:n].clone(), steps, dec.settings, dec=dec)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
            finally:
                S._processed = real
            assert dec2 is dec, "the capture of the joint step was refused"
            tok[0, :n] = toks[-1]
            pos[:n] += steps
            return n * steps / dt

        modes = {f"{kind}_{n}": (lambda kind, n: lambda steps: joint(kind, n, steps))(kind, n) for n in (4, 2) for kind in kinds}
        names = list(modes)
        modes[names[0]](args.settle)  # clocks settle, the packed copies exist (bench.py does the same)
        for m in names:  # one untimed pass of every mode (captures included)
            modes[m](16)
        captures = {m: decs[m.split("_")[0], int(m.split("_")[1])].captures if not m.startswith("baseline") else None for m in names}
        tps = {m: [] for m in names}
        for r in range(args.rounds):
            for m in names[r % len(names):] + names[:r % len(names)]:  # alternating order
                tps[m].append(modes[m](args.tokens))
        recaptured = {m: decs[m.split("_")[0], int(m.split("_")[1])].captures - captures[m] for m in names if captures[m] is not None}
    width = {m: int(m.split("_")[1]) for m in names}
    ms = {m: 1e3 * width[m] / statistics.median(v) for m, v in tps.items()}
    out = {"shape": "Meta-Llama-3-8B-Instruct", "weights": "bf16", "n_layer": args.n_layer, "cache_len": args.cache_len,
           "steps_per_run": args.tokens, "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "final_positions": pos.tolist(),
           "captures_during_timed_runs": recaptured,
           "aggregate_tokens_per_s": {m: {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}
                                      for m, v in tps.items()},
           "ms_per_step": {m: round(v, 4) for m, v in ms.items()},
           "us_per_step_over_plain": {m: round(1e3 * (ms[m] - ms[f"plain_{width[m]}"]), 1) for m in names if not m.startswith("plain")}}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
