#!/usr/bin/env python3
"""cc_gemv_fused_w8 (int8 weight-only) against cc_gemv_fused (bf16) at the Llama-3-8B decode shapes and the LM head, in the fused
forms the decode loop launches (wqkv: norm + RoPE; w1/w3: norm + SwiGLU pair; LM head: final norm).  Rotates over enough distinct
weight copies to exceed the 256 MB Infinity Cache; hipGraph replays, HIP events, median of 10.  One JSON line per shape.
    python tools/bench_gemv_w8.py [shape ...]      (CC_GEMV_W8_CFG="RB,CU[,workgroups]" overrides the int8 launch geometry)"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from cold_compress_amd.harness import glue  # noqa: E402
from cold_compress_amd.harness.quantize import quantize_per_channel_int8  # noqa: E402
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
        ncopy = max(2, (600 << 20) // (nbytes16 // 2) + 1)  # the int8 set alone exceeds the Infinity Cache
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
        res = {"shape": name, "N": N, "K": K, "matrices": nmat, "MB_bf16": round(nbytes16 / 1e6, 1), "MB_int8": round(nbytes16 / 2e6, 1),
               "copies": ncopy}
        # 16-bit
        W16 = [[torch.randn(N, K, device=dev).mul_(0.02).to(bf) for _ in range(nmat)] for _ in range(min(ncopy, max(2, (600 << 20) // nbytes16 + 1)))]
        n16 = len(W16)
        t16 = timed(lambda i: glue.gemv_fused(W16[i % n16][0], x, w3=W16[i % n16][1] if pair else None, **kw), max(n16, 8))
        del W16
        torch.cuda.empty_cache()
        # int8
        Q = []
        for _ in range(ncopy):
            qs = [quantize_per_channel_int8(torch.randn(N, K, device=dev).mul_(0.02)) for _ in range(nmat)]
            Q.append([(q, s.to(bf)) for q, s in qs])
        t8 = timed(lambda i: glue.gemv_fused(Q[i % ncopy][0][0], x, w3=Q[i % ncopy][1][0] if pair else None, scales=Q[i % ncopy][0][1],
                                             scales3=Q[i % ncopy][1][1] if pair else None, **kw), max(ncopy, 8))
        res.update(bf16_us=round(t16, 2), int8_us=round(t8, 2), ratio=round(t8 / t16, 3), bf16_TBps=round(nbytes16 / t16 / 1e6, 2),
                   int8_TBps=round(nbytes16 / 2 / t8 / 1e6, 2))
        print(json.dumps(res), flush=True)
        del Q
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
