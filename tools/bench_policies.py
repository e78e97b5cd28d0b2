#!/usr/bin/env python3
"""Layer-step time (update_kv + attention + update_state, hipGraph-replayed, rotating over > 512 MB of distinct K/V)
of every cache policy at the SURVEY §8(d) configurations: C2 (S = 2560), C3 (S = 4096), C4 (hybrid S = 18432),
C5 (Llama-3-70B at TP = 8: one kv head, 8 query heads per rank, S = 3488).  Llama-3 head geometry, bf16."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

from cold_compress_amd import _abi  # noqa: E402
from cold_compress_amd.attention_utils import scaled_dot_product_attention as sdpa  # noqa: E402
from cold_compress_amd.cache import get_cache_constructor  # noqa: E402

dev = "cuda"
HYBRID = [{"strategy": "special"}, {"strategy": "special_punc"}, {"strategy": "special_punc_heavy_hitter", "heavy_hitter_frac": 0.3},
          {"strategy": "special_punc_window", "recent_window": 0.3}, {"strategy": "full"}]


def timed(fn, n, iters=8, after=None):
    """Median device time per call of fn over `iters` replays of a hipGraph of n calls.  `after` (optional) runs once per replay
    behind the calls — the fused steps pass `pos.add_(1)`: positions must ADVANCE between replays, or the recoverable heavy-hitter
    step finds its position committed already and only replays the attention (no insert, no state stores)."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn(0)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(n):
            fn(i)
        if after is not None:
            after()
    g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / n)
    ts.sort()
    return ts[len(ts) // 2]


QBITS = {"fused": 8, "fp8": 8, "uint4": 4, "mxfp4": 4}  # cache_quant_mode -> the cache_bits it serves


def make(strategy, H, S, D, extra=None):
    cls, rk = get_cache_constructor(strategy)
    kw = dict(max_cache_length=S, global_tokens=4, max_seq_length=4 * S, cache_bits=None, recent_window=10, history_window_size=1,
              attn_thresholding=False, token_ids={"special": [[1], [2, 3]], "punctuation": [5, 6, 7]}, min_recovery_frac=0.9,
              hybrid_strategies=HYBRID)
    kw.update(extra or {})
    lk = {k: kw[k] for k in rk}
    if kw.get("cache_quant_mode"):
        lk["cache_quant_mode"] = kw["cache_quant_mode"]
    with torch.device(dev):
        kv = cls(1, H, D, torch.bfloat16, **lk)
    T = S
    if getattr(kv, "fused_quant", False) and kv.quant_format == _abi.CC_QUANT_UINT4:  # 4-bit images of N(0, 1) rows: 15 steps over [-3.2, 3.2]
        kv.k_cache_q.copy_(torch.randint(0, 256, kv.k_cache_q.shape, device=dev, dtype=torch.int32).to(torch.uint8))
        kv.v_cache_q.copy_(torch.randint(0, 256, kv.v_cache_q.shape, device=dev, dtype=torch.int32).to(torch.uint8))
        kv.kv_qparams[..., 0::2] = 6.4 / 15
        kv.kv_qparams[..., 1::2] = -3.2
    elif getattr(kv, "fused_quant", False) and kv.quant_format == _abi.CC_QUANT_MXFP4:  # MXFP4 images: any code, block scales 2^-1
        kv.k_cache_q.copy_(torch.randint(0, 256, kv.k_cache_q.shape, device=dev, dtype=torch.int32).to(torch.uint8))
        kv.v_cache_q.copy_(torch.randint(0, 256, kv.v_cache_q.shape, device=dev, dtype=torch.int32).to(torch.uint8))
        kv.kv_qparams.view(torch.int32)[..., 0::2] = 0x7E7E7E7E  # (bit patterns: four e8m0 bytes per row)
    elif getattr(kv, "fused_quant", False) and kv.quant_format != 8:  # FP8 images of N(0, 1) rows, scale 2^0
        kv.k_cache_q.copy_(torch.randn(kv.cache_shape, device=dev).to(torch.float8_e4m3fn).view(torch.uint8))
        kv.v_cache_q.copy_(torch.randn(kv.cache_shape, device=dev).to(torch.float8_e4m3fn).view(torch.uint8))
        kv.kv_qparams[..., 0::2] = 1.0
        kv.kv_qparams[..., 1::2] = 0.0
    elif getattr(kv, "fused_quant", False):  # uint8 images of N(0, 1) rows: 255 steps over [-3.2, 3.2]
        kv.k_cache_q.copy_((torch.randn(kv.cache_shape, device=dev) * 40 + 128).clamp_(0, 255).to(torch.uint8))
        kv.v_cache_q.copy_((torch.randn(kv.cache_shape, device=dev) * 40 + 128).clamp_(0, 255).to(torch.uint8))
        kv.kv_qparams[..., 0::2] = 6.4 / 255
        kv.kv_qparams[..., 1::2] = -3.2
    else:
        kv.k_cache.normal_()
        kv.v_cache.normal_()
    kv.pos[0] = torch.stack([torch.randperm(S + 64, device=dev)[:S] for _ in range(kv.pos.shape[1])]).int()
    kv.mask.fill_(True)
    kv.cache_cts.fill_(S)
    if hasattr(kv, "attn_history_num"):
        kv.attn_history_num.uniform_()
        kv.attn_history_denom.fill_(3)
    if hasattr(kv, "key_norm"):
        kv.key_norm.uniform_(8, 12)
    if strategy == "hybrid":  # a decode-ready state: head h runs policy h % 5
        kv.cache_strategies = (torch.arange(H, device=dev) % len(HYBRID)).to(torch.int64).contiguous()
        kv.requires_heavy_hitter = kv.requires_punc = kv.requires_special = True
    return kv


def main():
    cfgs = [("C2", 8, 32, 2560), ("C3", 8, 32, 4096), ("C4", 8, 32, 18432), ("C5", 1, 8, 3488)]
    D = 128
    only = os.environ.get("CC_POLICIES_ONLY")  # e.g. "C4:hybrid" — one configuration, for profiling
    for tag, H, HQ, S in cfgs:
        n_buf = max(4, min(32, (600 << 20) // (2 * H * S * D * 2) + 1))
        for strategy in (["hybrid"] if tag == "C4" else ["heavy_hitter", "l2", "random", "recent_global", "full"]) + (["heavy_hitter"] if tag == "C4" else []):
            if only and only != f"{tag}:{strategy}":
                continue
            try:
                caches = [make(strategy, H, S, D) for _ in range(n_buf)]
            except Exception as e:
                print(json.dumps({"cfg": tag, "strategy": strategy, "error": f"{type(e).__name__}: {e}"[:160]}), flush=True)
                continue
            q = torch.randn(1, HQ, 1, D, device=dev).to(torch.bfloat16)
            k1 = torch.randn(1, H, 1, D, device=dev).to(torch.bfloat16)
            pos = torch.tensor([S + 100], dtype=torch.int32, device=dev)
            ids = torch.tensor([[11]], device=dev)

            def three_call(i):
                kv = caches[i % n_buf]
                k, v, m = kv.update_kv(pos, k1, k1, False, input_ids=ids)
                fuse = strategy in ("heavy_hitter", "hybrid")
                y, a = sdpa(q, k, v, attn_mask=m, return_attn=kv.return_attn() and not fuse, group_mean=True,
                            history=kv.fused_history() if fuse else None)
                if fuse:
                    kv._state_fused = True
                kv.update_state(pos, k1, k1, False, a, input_ids=ids)

            for i in range(n_buf):  # lazily built per-cache tables / scratch must exist before graph capture
                three_call(i)
            res = {"cfg": tag, "strategy": strategy, "H": H, "HQ": HQ, "S": S, "three_call_us": round(timed(three_call, n_buf), 2)}
            if strategy in ("heavy_hitter", "recent_global", "full", "random", "l2"):
                for kv in caches:
                    kv.prepare_decode(pos)
                res["fused_step_us"] = round(timed(lambda i: caches[i % n_buf].decode_step(q, k1, k1, pos), n_buf, after=lambda: pos.add_(1)), 2)
            if strategy in ("heavy_hitter", "recent_global", "full", "random"):
                # the opt-in fused quantised cache (cache_bits=8, cache_quant_mode="fused" / "fp8"; cache_bits=4, "uint4" / "mxfp4"):
                # uint8, FP8, 4-bit or MXFP4 images streamed, dequantised in registers
                for key, mode in (("fused_quant8_step_us", "fused"), ("fused_fp8_step_us", "fp8"), ("fused_uint4_step_us", "uint4"),
                                  ("fused_mxfp4_step_us", "mxfp4")):
                    del caches
                    torch.cuda.empty_cache()
                    caches = [make(strategy, H, S, D, {"cache_bits": QBITS[mode], "cache_quant_mode": mode}) for _ in range(n_buf)]
                    for kv in caches:
                        kv.prepare_decode(pos)
                    for i in range(n_buf):
                        caches[i].decode_step(q, k1, k1, pos)
                    res[key] = round(timed(lambda i: caches[i % n_buf].decode_step(q, k1, k1, pos), n_buf, after=lambda: pos.add_(1)), 2)
            if strategy == "hybrid" and caches[0].supports_fused_step():
                for kv in caches:
                    kv.prepare_decode(pos)
                res["fused_step_us"] = round(timed(lambda i: caches[i % n_buf].decode_step(q, k1, k1, pos, input_ids=ids), n_buf, after=lambda: pos.add_(1)), 2)
                res["fused_one_launch"] = caches[0].single_launch_active(HQ)
                # the hybrid step over uint8 images (cache_quant_mode="fused"), FP8 images ("fp8"), 4-bit images ("uint4") and MXFP4
                # images ("mxfp4")
                for key, mode in (("fused_quant8", "fused"), ("fused_fp8", "fp8"), ("fused_uint4", "uint4"), ("fused_mxfp4", "mxfp4")):
                    del caches
                    torch.cuda.empty_cache()
                    caches = [make(strategy, H, S, D, {"cache_bits": QBITS[mode], "cache_quant_mode": mode}) for _ in range(n_buf)]
                    for kv in caches:
                        kv.prepare_decode(pos)
                    for i in range(n_buf):
                        caches[i].decode_step(q, k1, k1, pos, input_ids=ids)
                    res[key + "_step_us"] = round(timed(lambda i: caches[i % n_buf].decode_step(q, k1, k1, pos, input_ids=ids), n_buf,
                                                        after=lambda: pos.add_(1)), 2)
                    res[key + "_one_launch"] = caches[0].single_launch_active(HQ)
            b = 2 * H * S * D * 2
            res["kv_MB"] = round(b / 1e6, 1)
            best = res.get("fused_step_us", res["three_call_us"])
            res["kv_GBps"] = round(b / best / 1e3)
            print(json.dumps(res), flush=True)
            del caches
            torch.cuda.empty_cache()
        # heavy hitter with a finite history window (the two-launch ring step): 16-bit and over uint8 / FP8 images
        for W in ((8, 400) if tag in ("C2", "C3") else ()):
            strategy = f"heavy_hitter_w{W}"
            if only and only != f"{tag}:{strategy}":
                continue
            res = {"cfg": tag, "strategy": strategy, "H": H, "HQ": HQ, "S": S, "W": W}
            q = torch.randn(1, HQ, 1, D, device=dev).to(torch.bfloat16)
            k1 = torch.randn(1, H, 1, D, device=dev).to(torch.bfloat16)
            pos = torch.tensor([S + 100], dtype=torch.int32, device=dev)
            n_w = max(4, min(n_buf, (900 << 20) // (H * S * (W * 2 + 2 * D * 2)) + 1))
            for key, extra in (("fused_step_us", {}), ("fused_quant8_step_us", {"cache_bits": 8, "cache_quant_mode": "fused"}),
                               ("fused_fp8_step_us", {"cache_bits": 8, "cache_quant_mode": "fp8"}),
                               ("fused_uint4_step_us", {"cache_bits": 4, "cache_quant_mode": "uint4"}),
                               ("fused_mxfp4_step_us", {"cache_bits": 4, "cache_quant_mode": "mxfp4"})):
                caches = [make("heavy_hitter", H, S, D, dict(extra, history_window_size=W)) for _ in range(n_w)]
                for kv in caches:
                    kv.prepare_decode(pos)
                for i in range(n_w):
                    caches[i].decode_step(q, k1, k1, pos)
                res[key] = round(timed(lambda i: caches[i % n_w].decode_step(q, k1, k1, pos), n_w, after=lambda: pos.add_(1)), 2)
                del caches
                torch.cuda.empty_cache()
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
