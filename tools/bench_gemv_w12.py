#!/usr/bin/env python3
"""cc_gemv_fused_w12 (the lossless 12-bit packed copy of dense bf16 weights) in its three layouts — the first one ("w12"), the
planar one and, where it serves the shape (plain, 4096 < K <= 16384), the long-row launch over planar codes ("long", layout id 2) —
against cc_gemv_fused on the same weights in ONE session, at the Llama-3-8B decode shapes and the LM head, in the fused
forms the decode loop launches (wqkv: norm + RoPE; w1/w3: norm + SwiGLU pair; LM head: final norm).  Rotates over enough distinct
weight copies to exceed the 256 MB Infinity Cache; hipGraph replays, HIP events, median of 10, the kernels alternating three
times.  Outputs are compared bit for bit.  One JSON line per shape.  The packed kernels are forced for every shape here; the
harness uses one only where `on_by_default` / `planar_on_by_default` / `long_on_by_default` say it measured faster.  `long_wins`:
the same rule for layout 2, against the dense kernel and planar.  `planar_wins`: the rule those defaults
follow — planar's best beats the best of the dense kernel AND of the first layout by more than `bf16_spread_us`, the dense kernel's
own min-to-max spread over this session's repeats.
    python tools/bench_gemv_w12.py [shape ...]      (CC_GEMV_W12_CFG="RB,CU[,workgroups]" overrides the packed launch geometry;
                                                     the K = 8192 shapes w1w3_70b, lm_head_70b and square_8k run only when named)"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from cold_compress_amd.harness import glue  # noqa: E402
from bench_gemv import timed  # noqa: E402

dev = "cuda"
REPEATS = 3
MODES = {"bf16": False, "w12": "force", "planar": "force-planar", "long": "force-long"}
LAYOUTS = (("w12", 0), ("planar", glue.W12_PLANAR), ("long", glue.W12_LONG))


def main():
    torch.manual_seed(0)
    shapes = {"wqkv": (6144, 4096), "wo": (4096, 4096), "w1w3": (14336, 4096), "w2": (4096, 14336), "lm_head": (128256, 4096),
              "w1w3_70b": (28672, 8192), "lm_head_70b": (128256, 8192), "square_8k": (8192, 8192)}
    only = sys.argv[1:]
    bf = torch.bfloat16
    for name, (N, K) in shapes.items():
        if (only and name not in only) or (not only and name.endswith(("_70b", "_8k"))):
            continue
        pair = name.startswith("w1w3")
        nmat = 2 if pair else 1
        nbytes16 = nmat * N * K * 2
        ncopy = max(2, (600 << 20) // (nbytes16 * 3 // 4) + 1)  # the packed set alone exceeds the Infinity Cache
        x = torch.randn(K, device=dev).to(bf)
        delta = torch.randn(K, device=dev).to(bf)
        nw = torch.ones(K, device=dev, dtype=bf)
        h = torch.empty(K, device=dev, dtype=bf)
        fr = torch.rand(64, 2, device=dev).to(bf)
        kw = {}
        if name == "wqkv":
            kw = dict(delta=delta, norm_weight=nw, h_out=h, freqs=fr, rope_rows=5120, head_dim=128)
        elif pair or name.startswith("lm_head"):
            kw = dict(delta=delta, norm_weight=nw, h_out=h)
        W = [[torch.randn(N, K, device=dev).mul_(0.02).to(bf) for _ in range(nmat)] for _ in range(ncopy)]

        def run(i, mode):
            return glue.gemv_fused(W[i % ncopy][0], x, w3=W[i % ncopy][1] if pair else None, w12=MODES[mode], **kw)

        pk = {m: glue._w12_get(W[0][0], pair, True, lay) for m, lay in LAYOUTS}
        same = {m: pk[m] is not None for m in pk}
        for i in range(ncopy):  # packs every copy eagerly (nothing is packed under capture) and checks the bits
            ref = run(i, "bf16").view(torch.int16)
            for m in pk:
                same[m] = same[m] and torch.equal(run(i, m).view(torch.int16), ref)
        ts = {m: [] for m in MODES}
        for _ in range(REPEATS):
            for m in MODES:
                if m == "bf16" or pk[m] is not None:  # (a geometry not built in a layout is not timed: it would run the dense kernel)
                    ts[m].append(timed(lambda i: run(i, m), max(ncopy, 8)))
        best = {m: (min(t) if t else None) for m, t in ts.items()}
        spread = max(ts["bf16"]) - min(ts["bf16"])
        geo = {m: glue.w12_geometry(N, K, pair, lay) for m, lay in LAYOUTS}
        res = {"shape": name, "N": N, "K": K, "matrices": nmat, "MB_bf16": round(nbytes16 / 1e6, 1), "MB_w12": round(nbytes16 * 0.75 / 1e6, 1),
               "copies": ncopy, "bf16_spread_us": round(spread, 3), "cfg_env": os.environ.get("CC_GEMV_W12_CFG")}
        for m in MODES:
            res[m + "_us"] = round(best[m], 2) if best[m] is not None else None
            res[m + "_us_runs"] = [round(t, 2) for t in ts[m]]
        res["bf16_TBps"] = round(nbytes16 / best["bf16"] / 1e6, 2)
        for m in pk:
            if best[m] is not None:
                res[m + "_ratio"] = round(best[m] / best["bf16"], 3)
                res[m + "_TBps"] = round(nbytes16 * 0.75 / best[m] / 1e6, 2)
                res[m + "_bit_identical"] = same[m]
                res[m + "_geometry"] = [pk[m].rb, pk[m].cu, pk[m].cap]
                res[m + "_pack"] = dict(base=pk[m].base, records=pk[m].n_records, overflow=pk[m].n_overflow, escapes=pk[m].n_escapes)
        others = [best[m] for m in ("bf16", "w12") if best[m] is not None]
        res["planar_wins"] = bool(best["planar"] is not None and best["planar"] < min(others) - spread)
        others = [best[m] for m in ("bf16", "planar") if best[m] is not None]
        res["long_wins"] = bool(best["long"] is not None and best["long"] < min(others) - spread)
        res["on_by_default"] = bool(geo["w12"] and geo["w12"][4])
        res["planar_on_by_default"] = bool(geo["planar"] and geo["planar"][4])
        res["long_on_by_default"] = bool(geo["long"] and geo["long"][4])
        print(json.dumps(res), flush=True)
        del W
        glue.w12_cache_clear()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
