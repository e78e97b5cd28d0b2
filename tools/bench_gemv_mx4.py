#!/usr/bin/env python3
"""cc_gemv_fused_mx4 (MXFP4 weight-only) against cc_gemv_fused_w4 (int4, G = 32 and 128), cc_gemv_fused_w8 (int8) and cc_gemv_fused
(bf16) at the Llama-3-8B decode shapes and the LM head, in the fused forms the decode loop launches (wqkv: norm + RoPE; w1/w3:
norm + SwiGLU pair; LM head: final norm).  Each format rotates over enough distinct weight copies to exceed the 256 MB Infinity
Cache; hipGraph replays, HIP events, median of 10.  One JSON line per shape; TB/s counts the bytes each format streams (MXFP4:
codes + scale bytes; int4: codes + pairs).
    python tools/bench_gemv_mx4.py [shape ...] [--mx4-only]   (CC_GEMV_MX4_CFG="RB,CU[,workgroups]" overrides the MXFP4 geometry)"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from cold_compress_amd.harness import glue  # noqa: E402
from cold_compress_amd.harness.quantize import group_quantize_int4, pack_int4, quantize_mxfp4, quantize_per_channel_int8  # noqa: E402
from bench_gemv import timed  # noqa: E402

dev = "cuda"
SET = 600 << 20  # bytes per format in rotation


def _int4(N, K, G):
    w = torch.randn(N, K, device=dev).mul_(0.02).to(torch.bfloat16)
    q, s, z = group_quantize_int4(w, G)
    return pack_int4(q).contiguous(), torch.stack([s, z], -1).contiguous()


def _mx4(N, K):
    return quantize_mxfp4(torch.randn(N, K, device=dev).mul_(0.02).to(torch.bfloat16))


def main():
    torch.manual_seed(0)
    shapes = {"wqkv": (6144, 4096), "wo": (4096, 4096), "w1w3": (14336, 4096), "w2": (4096, 14336), "lm_head": (128256, 4096)}
    mx4_only = "--mx4-only" in sys.argv[1:]
    only = [a for a in sys.argv[1:] if a != "--mx4-only"]
    bf = torch.bfloat16
    for name, (N, K) in shapes.items():
        if only and name not in only:
            continue
        pair = name == "w1w3"
        nmat = 2 if pair else 1
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
        b16 = nmat * N * K * 2
        b8 = nmat * N * (K + 2)
        res = {"shape": name, "N": N, "K": K, "matrices": nmat, "MB_bf16": round(b16 / 1e6, 1)}
        ncopy = lambda b: max(2, SET // b + 1)  # noqa: E731
        t16 = t8 = None
        if not mx4_only:
            # 16-bit
            W16 = [[torch.randn(N, K, device=dev).mul_(0.02).to(bf) for _ in range(nmat)] for _ in range(ncopy(b16))]
            n = len(W16)
            t16 = timed(lambda i: glue.gemv_fused(W16[i % n][0], x, w3=W16[i % n][1] if pair else None, **kw), max(n, 8))
            del W16
            torch.cuda.empty_cache()
            # int8
            Q = []
            for _ in range(ncopy(b8)):
                qs = [quantize_per_channel_int8(torch.randn(N, K, device=dev).mul_(0.02)) for _ in range(nmat)]
                Q.append([(q, s.to(bf)) for q, s in qs])
            n = len(Q)
            t8 = timed(lambda i: glue.gemv_fused(Q[i % n][0][0], x, w3=Q[i % n][1][0] if pair else None, scales=Q[i % n][0][1],
                                                 scales3=Q[i % n][1][1] if pair else None, **kw), max(n, 8))
            del Q
            torch.cuda.empty_cache()
            res.update(bf16_us=round(t16, 2), int8_us=round(t8, 2), bf16_TBps=round(b16 / t16 / 1e6, 2), int8_TBps=round(b8 / t8 / 1e6, 2))
        # MXFP4
        bm = nmat * N * (K // 2 + K // 32)
        QM = [[_mx4(N, K) for _ in range(nmat)] for _ in range(ncopy(bm))]
        n = len(QM)
        tm = timed(lambda i: glue.gemv_fused(QM[i % n][0][0], x, w3=QM[i % n][1][0] if pair else None, scales=QM[i % n][0][1],
                                             scales3=QM[i % n][1][1] if pair else None, **kw), max(n, 8))
        del QM
        torch.cuda.empty_cache()
        res.update(mxfp4_us=round(tm, 2), mxfp4_TBps=round(bm / tm / 1e6, 2))
        if t8 is not None:
            res.update(mxfp4_vs_int8=round(tm / t8, 3), mxfp4_vs_bf16=round(tm / t16, 3))
        # int4
        for G in (() if mx4_only else (32, 128)):
            b4 = nmat * N * (K // 2 + 4 * (K // G))
            Q4 = [[_int4(N, K, G) for _ in range(nmat)] for _ in range(ncopy(b4))]
            n = len(Q4)
            t4 = timed(lambda i: glue.gemv_fused(Q4[i % n][0][0], x, w3=Q4[i % n][1][0] if pair else None, scales=Q4[i % n][0][1],
                                                 scales3=Q4[i % n][1][1] if pair else None, groupsize=G, **kw), max(n, 8))
            del Q4
            torch.cuda.empty_cache()
            res.update({f"int4_g{G}_us": round(t4, 2), f"int4_g{G}_TBps": round(b4 / t4 / 1e6, 2)})
            res.update({f"mxfp4_vs_int4_g{G}": round(tm / t4, 3)})
        cfg = os.environ.get("CC_GEMV_MX4_CFG")
        if cfg:
            res["mx4_cfg"] = cfg
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
