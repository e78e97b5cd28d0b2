#!/usr/bin/env python3
"""cc_gemv_fused_w12 (the lossless 12-bit packed copy of dense bf16 weights) against cc_gemv_fused on the same weights, at the
Llama-3-8B decode shapes and the LM head, in the fused forms the decode loop launches (wqkv: norm + RoPE; w1/w3: norm + SwiGLU
pair; LM head: final norm).  Rotates over enough distinct weight copies to exceed the 256 MB Infinity Cache; hipGraph replays, HIP
events, median of 10, the two kernels alternating twice.  Outputs are compared bit for bit.  One JSON line per shape.  The packed
kernel is forced for every shape here; the harness uses it only where `on_by_default` says it measured faster.
    python tools/bench_gemv_w12.py [shape ...]      (CC_GEMV_W12_CFG="RB,CU[,workgroups]" overrides the packed launch geometry)"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from cold_compress_amd.harness import glue  # noqa: E402
from bench_gemv import timed  # noqa: E402

dev = "cuda"


def main():
    torch.manual_seed(0)
    shapes = {"wqkv": (6144, 4096), "wo": (4096, 4096), "w1w3": (14336, 4096), "w2": (4096, 14336), "lm_head": (128256, 4096)}
    only = sys.argv[1:]
    bf = torch.bfloat16
    for name, (N, K) in shapes.items():
        if only and name not in only:
            continue
        pair = name == "w1w3"
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
        elif pair or name == "lm_head":
            kw = dict(delta=delta, norm_weight=nw, h_out=h)
        W = [[torch.randn(N, K, device=dev).mul_(0.02).to(bf) for _ in range(nmat)] for _ in range(ncopy)]

        def run(i, w12):
            return glue.gemv_fused(W[i % ncopy][0], x, w3=W[i % ncopy][1] if pair else None, w12="force" if w12 else False, **kw)

        same = True
        for i in range(ncopy):  # packs every copy eagerly (nothing is packed under capture) and checks the bits
            same = same and torch.equal(run(i, True).view(torch.int16), run(i, False).view(torch.int16))
        pk = glue._w12_get(W[0][0], pair, True)
        t16, t12 = [], []
        for _ in range(2):
            t16.append(timed(lambda i: run(i, False), max(ncopy, 8)))
            t12.append(timed(lambda i: run(i, True), max(ncopy, 8)))
        b16, b12 = min(t16), min(t12)
        res = {"shape": name, "N": N, "K": K, "matrices": nmat, "MB_bf16": round(nbytes16 / 1e6, 1), "MB_w12": round(nbytes16 * 0.75 / 1e6, 1),
               "copies": ncopy, "bf16_us": round(b16, 2), "w12_us": round(b12, 2), "ratio": round(b12 / b16, 3),
               "bf16_us_runs": [round(t, 2) for t in t16], "w12_us_runs": [round(t, 2) for t in t12],
               "bf16_TBps": round(nbytes16 / b16 / 1e6, 2), "w12_TBps": round(nbytes16 * 0.75 / b12 / 1e6, 2), "bit_identical": same,
               "packed": pk is not None, "on_by_default": bool(glue.w12_geometry(N, K, pair)[4])}
        if pk is not None:
            res.update(rb=pk.rb, cu=pk.cu, base=pk.base, records=pk.n_records, overflow=pk.n_overflow, escapes=pk.n_escapes)
        print(json.dumps(res), flush=True)
        del W
        glue.w12_cache_clear()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
