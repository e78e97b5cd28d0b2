#!/usr/bin/env python3
"""cc_gemv_fused_w4 (int4 group-wise weight-only, G = 32 and 128) against cc_gemv_fused_w8 (int8) and cc_gemv_fused (bf16) at the
Llama-3-8B decode shapes and the LM head, in the fused forms the decode loop launches (wqkv: norm + RoPE; w1/w3: norm + SwiGLU
pair; LM head: final norm).  Each format rotates over enough distinct weight copies to exceed the 256 MB Infinity Cache; hipGraph
replays, HIP events, median of 10.  One JSON line per shape; TB/s counts the bytes each format streams (int4: codes + pairs).
    python tools/bench_gemv_w4.py [shape ...] [--int4-only]   (CC_GEMV_W4_CFG="RB,CU[,workgroups]" overrides the int4 geometry)
    python tools/bench_gemv_w4.py [shape ...] --tokens T      cc_gemv_fused_w4_multi at 1 .. T input rows (T <= 4) against as many
        single-vector launches, G = 32 and 128, the same rotation and timing; five passes in alternating order, the median of the
        passes' medians.  us per launch; "x_singles" is t(T) / (T * t(single)): below 1 the one pass over the weights wins."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from cold_compress_amd.harness import glue  # noqa: E402
from cold_compress_amd.harness.quantize import group_quantize_int4, pack_int4, quantize_per_channel_int8  # noqa: E402
from bench_gemv import timed  # noqa: E402

dev = "cuda"
SET = 600 << 20  # bytes per format in rotation


def _int4(N, K, G):
    w = torch.randn(N, K, device=dev).mul_(0.02).to(torch.bfloat16)
    q, s, z = group_quantize_int4(w, G)
    return pack_int4(q).contiguous(), torch.stack([s, z], -1).contiguous()


SHAPES = {"wqkv": (6144, 4096), "wo": (4096, 4096), "w1w3": (14336, 4096), "w2": (4096, 14336), "lm_head": (128256, 4096)}


def main_tokens(tmax, only, passes=5):
    torch.manual_seed(0)
    bf = torch.bfloat16
    for name, (N, K) in SHAPES.items():
        if only and name not in only:
            continue
        pair = name == "w1w3"
        nmat = 2 if pair else 1
        x = torch.randn(tmax, K, device=dev).to(bf)
        delta = torch.randn(tmax, K, device=dev).to(bf)
        nw = torch.ones(K, device=dev, dtype=bf)
        h = torch.empty(tmax, K, device=dev, dtype=bf)
        fr = torch.rand(tmax, 64, 2, device=dev).to(bf)
        for G in (32, 128):
            b4 = nmat * N * (K // 2 + 4 * (K // G))
            Q4 = [[_int4(N, K, G) for _ in range(nmat)] for _ in range(max(2, SET // b4 + 1))]
            n = len(Q4)

            def kw(T, one):
                r = slice(0, 1) if one else slice(0, T)
                if name == "wqkv":
                    k = dict(delta=delta[r], norm_weight=nw, h_out=h[r], freqs=fr[r], rope_rows=5120, head_dim=128)
                elif pair or name == "lm_head":
                    k = dict(delta=delta[r], norm_weight=nw, h_out=h[r])
                else:
                    k = {}
                return {a: (b[0] if one and torch.is_tensor(b) and a != "norm_weight" else b) for a, b in k.items()}

            def single(i):
                m = Q4[i % n]
                return glue.gemv_fused(m[0][0], x[0], w3=m[1][0] if pair else None, scales=m[0][1], scales3=m[1][1] if pair else None,
                                       groupsize=G, **kw(1, True))

            def multi(T):
                def run(i):
                    m = Q4[i % n]
                    return glue.gemv_fused_w4_multi(m[0][0], x[:T], m[0][1], G, w3=m[1][0] if pair else None,
                                                    scales3=m[1][1] if pair else None, **kw(T, False))
                return run

            runs = [("single", single)] + [(f"T{T}", multi(T)) for T in range(1, tmax + 1)]
            ts = {k: [] for k, _ in runs}
            for ps in range(passes):  # alternating order
                for k, fn in (runs if ps % 2 == 0 else runs[::-1]):
                    ts[k].append(timed(fn, max(n, 8)))
            med = {k: sorted(v)[len(v) // 2] for k, v in ts.items()}
            res = {"shape": name, "N": N, "K": K, "matrices": nmat, "G": G, "MB_int4": round(b4 / 1e6, 1), "single_us": round(med["single"], 2)}
            for T in range(1, tmax + 1):
                t = med[f"T{T}"]
                res.update({f"T{T}_us": round(t, 2), f"T{T}_x_singles": round(t / (T * med["single"]), 3), f"T{T}_TBps": round(b4 / t / 1e6, 2)})
            cfg = os.environ.get("CC_GEMV_W4_CFG")
            if cfg:
                res["w4_cfg"] = cfg
            print(json.dumps(res), flush=True)
            del Q4
            torch.cuda.empty_cache()


def main():
    torch.manual_seed(0)
    shapes = SHAPES
    if "--tokens" in sys.argv[1:]:
        i = sys.argv.index("--tokens")
        tmax = int(sys.argv[i + 1])
        if not 1 <= tmax <= glue.GEMV_MULTI_MAX_T:
            sys.exit(f"--tokens: 1 .. {glue.GEMV_MULTI_MAX_T}")
        return main_tokens(tmax, [a for a in sys.argv[1:i] + sys.argv[i + 2:] if not a.startswith("--")])
    int4_only = "--int4-only" in sys.argv[1:]
    only = [a for a in sys.argv[1:] if a != "--int4-only"]
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
        if not int4_only:
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
        # int4
        for G in (32, 128):
            b4 = nmat * N * (K // 2 + 4 * (K // G))
            Q4 = [[_int4(N, K, G) for _ in range(nmat)] for _ in range(ncopy(b4))]
            n = len(Q4)
            t4 = timed(lambda i: glue.gemv_fused(Q4[i % n][0][0], x, w3=Q4[i % n][1][0] if pair else None, scales=Q4[i % n][0][1],
                                                 scales3=Q4[i % n][1][1] if pair else None, groupsize=G, **kw), max(n, 8))
            del Q4
            torch.cuda.empty_cache()
            res.update({f"int4_g{G}_us": round(t4, 2), f"int4_g{G}_TBps": round(b4 / t4 / 1e6, 2)})
            if t8 is not None:
                res.update({f"int4_g{G}_vs_int8": round(t4 / t8, 3), f"int4_g{G}_vs_bf16": round(t4 / t16, 3)})
        cfg = os.environ.get("CC_GEMV_W4_CFG")
        if cfg:
            res["w4_cfg"] = cfg
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
