"""Time of the sampling tail against the greedy tail and the torch composition, and tokens/s of a graphed generation with sampling on
and off -> profiles/sampling_tail.jsonl (one JSON row per line).

    python tools/bench_sampling.py                 # tails at V = 32000 and 128256 (bf16), top_p / min_p rows included, + the 128-token generation
    python tools/bench_sampling.py --no_generate   # the tails alone (what a rocprofv3 --kernel-trace --stats run wraps)

Tails: HIP events around `--launches` back-to-back calls on one stream, after a warm-up; the logits stay resident in L2 between the
calls, as they are behind the LM head of a decode step.  The torch composition is topk + softmax + multinomial (scaling included), the
launches the reference's logits_to_probs and a multinomial draw would cost.  Generation: the Llama-3-8B shape with random weights, a
512-token prompt, heavy_hitter at 4096 slots, 128 tokens through generate() with a GraphedDecoder."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cold_compress_amd.harness import CONFIGS, GraphedDecoder, ModelArgs, Transformer, generate, glue, prefill, setup_caches  # noqa: E402


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


def tails(dev, launches, out):
    for V in (32000, 128256):
        logits = (torch.randn(V, generator=torch.Generator().manual_seed(V)) * 3).to(torch.bfloat16).to(dev)
        pos = torch.tensor([7], dtype=torch.int32, device=dev)

        def torch_comp(k=50):
            x = logits / 0.8
            v, _ = torch.topk(x, k)
            x = torch.where(x < v[-1], -float("inf"), x)
            return torch.multinomial(torch.softmax(x, dim=-1).float(), 1)

        rows = [("cc_softmax_argmax", None, lambda: glue.softmax_argmax(logits)),
                ("cc_sample_topk", None, lambda: glue.sample_topk(logits, 0.8, None, 1, pos)),
                ("cc_sample_topk", 50, lambda: glue.sample_topk(logits, 0.8, 50, 1, pos)),
                ("torch topk+softmax+multinomial", 50, torch_comp)]
        # cc_sample_nucleus beside the cc_sample_topk rows of the same run (the only numbers its cost is compared against)
        rows += [("cc_sample_nucleus", k, lambda k=k, p=p, mp=mp: glue.sample_nucleus(logits, 0.8, k, p, mp, 1, pos), p, mp)
                 for k, p, mp in ((None, 0.9, None), (50, 0.9, None), (None, None, 0.05), (50, 0.9, 0.05))]
        for name, k, fn, *filters in rows:
            # under hipGraph replay as well: what the decode step pays (no per-launch host work)
            us = timed(fn, launches)
            try:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    fn()
                us_graph = round(timed(g.replay, launches), 2)
            except RuntimeError:  # (a composition this runtime cannot capture)
                us_graph = None
            row = {"what": "tail", "V": V, "dtype": "bf16", "path": name, "top_k": k}
            if filters:
                row.update(top_p=filters[0], min_p=filters[1])
            out({**row, "launches": launches, "us_per_call_eager": round(us, 2), "us_per_call_graph": us_graph})


def generation(dev, out):
    cfg = dict(CONFIGS["Meta-Llama-3-8B-Instruct"])
    cfg["block_size"] = 8192
    with torch.device("meta"):
        model = Transformer(ModelArgs(**cfg))
    model = model.to_empty(device=dev).to(torch.bfloat16)
    g = torch.Generator(device=dev).manual_seed(1234)
    with torch.no_grad():
        for n, p in model.named_parameters():
            p.fill_(1.0) if "norm" in n else p.normal_(0.0, 0.02, generator=g)
    model.eval()
    kw = dict(max_cache_length=[4096.0], cache_bits=None, cache_length_pattern="tile", cache_strategy=["heavy_hitter"],
              cache_strategy_pattern="tile", feed_long_prompts=False, prompt_compression_strategy=["heavy_hitter"], global_tokens=4,
              recent_window=10, history_window_size=1, attn_thresholding=False)
    setup_caches(model, None, dev, 4096, dict(kw))
    prompt = torch.randint(0, cfg["vocab_size"], (512,), generator=torch.Generator().manual_seed(1), dtype=torch.int32).to(dev)
    for name, skw in (("greedy", {}), ("sampling", dict(temperature=0.8, top_k=50, seed=1)),
                      ("sampling top_p", dict(temperature=0.8, top_k=50, top_p=0.9, seed=1))):
        dec = GraphedDecoder(model, **skw)
        best = None
        for r in range(3):  # the first run captures; best of the next two
            for l in model.layers:
                l.attention.kv_cache.reset()
            t0 = time.perf_counter()
            seq, _, stats = generate(model, prompt, prefill, dec, max_new_tokens=128, **skw)
            torch.cuda.synchronize()
            if r > 0:
                best = max(best or 0.0, stats["decode_toks_per_sec"])
        out({"what": "generate", "shape": "Meta-Llama-3-8B-Instruct", "prompt": 512, "new_tokens": 128, "decoder": "hipGraph", "mode": name,
             **skw, "decode_tok_s": round(best, 1), "wall_s_last": round(time.perf_counter() - t0, 3)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=400)
    ap.add_argument("--no_generate", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampling_tail.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    fh = open(a.out, "w")

    def out(row):
        line = json.dumps(row)
        print(line, flush=True)
        fh.write(line + "\n")
        fh.flush()

    with torch.no_grad():
        tails(dev, a.launches, out)
        if not a.no_generate:
            generation(dev, out)
    fh.close()


if __name__ == "__main__":
    main()
