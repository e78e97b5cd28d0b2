"""CPU checks of the float64 attention reference (tests/attn_ref.py) that the GPU tests at odd query-group ratios lean on
(tests/test_gpu_gqa_ratios.py): it must reproduce the reference's own attention captured in the f7 fixtures — at 4 query heads
per kv head (f7_attn_<dtype>) and at 7 and 3 (f7_attn_gqa_<dtype>) — and the CPU oracle must agree with it at 3 and 7 query heads
per kv head, prefill, decode and the heavy-hitter pipeline.  Also: the harness refuses a fused quantised cache at a ratio the
decode kernels do not serve before any prefill, and the step fuzzer's seeded draws are unchanged by its ratio option."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

import attn_ref as AR
from helpers import DT_CODE, from_np, load_golden, to_np


def _close_mostly_exact(mine, ref, dtype, what, atol):
    """Every entry within `atol`; for 16-bit dtypes at least 99 % of them bit-equal to the reference's (what only the same
    rounding points give: fp32 matrix products differ from float64 ones in the last bits)."""
    mine, ref = mine.double(), ref.double()
    assert float((mine - ref).abs().max()) < atol, f"{what}: max |diff| {float((mine - ref).abs().max())}"
    if dtype == torch.float32:
        return
    same = float((mine == ref).double().mean())
    assert same >= 0.99, f"{what}: only {same:.4f} of the entries equal the reference's {dtype} values"


def _dec_check(f, pre, dtype, y_tol):
    q, k, v, mask = (f[pre + n] for n in ("q", "k", "v", "mask"))
    y, p, gm = AR.decode_ref(q, k, v, mask)
    _close_mostly_exact(y, f[pre + "y"][0, :, 0], dtype, pre + "y", y_tol)
    _close_mostly_exact(p, f[pre + "probs"][0, :, 0], dtype, pre + "probs", 1e-3)
    _close_mostly_exact(gm, f[pre + "attn_gm"][0, :, 0], dtype, pre + "attn_gm", 1e-3)


def _pre_check(f, pre, dtype, y_tol, cs_tol, ob_tol):
    q, k, v = (f[pre + n] for n in ("q", "k", "v"))
    out = AR.prefill_ref(q, k, v, obs_len=16, chunk=7)  # (a chunk that does not divide L)
    _close_mostly_exact(out["y"], f[pre + "y"][0], dtype, pre + "y", y_tol)
    assert float((out["colsum"] - f[pre + "colsum"][0].double()).abs().max()) < cs_tol
    assert float((out["obs"] - f[pre + "obs_mean"][0].double()).abs().max()) < ob_tol
    # the group-mean probabilities themselves: the column sums of the fixture's, row by row
    gm = f[pre + "attn_gm"][0].double()
    full = AR.prefill_ref(q, k, v, obs_len=q.shape[2])
    assert float((full["colsum"] - gm.sum(dim=1)).abs().max()) < 1e-2 * max(1.0, float(gm.sum(dim=1).abs().max()))


@pytest.mark.parametrize("tag", ["f32", "bf16"])
def test_attn_ref_reproduces_reference_attention(tag):
    """f7_attn_<tag> (4 query heads per kv head), within the tolerances tests/test_gpu_parity.py holds the kernels to."""
    f = load_golden(f"f7_attn_{tag}.npz")
    dtype = f["dec.q"].dtype
    tol = 8e-3 if tag == "bf16" else 1e-3
    for case in ("dec", "dec8b"):
        _dec_check(f, case + ".", dtype, tol)
    _pre_check(f, "pre.", dtype, tol, 6e-2 if tag == "bf16" else 1e-3, 4e-3 if tag == "bf16" else 1e-3)


@pytest.mark.parametrize("tag", ["bf16", "f16"])
@pytest.mark.parametrize("ratio", ["r7", "r3"])
def test_attn_ref_reproduces_reference_attention_at_odd_ratios(tag, ratio):
    """f7_attn_gqa_<tag>: the reference's attention at 7 query heads per kv head (H = 4, D = 128) and 3 (H = 2, D = 64)."""
    f = load_golden(f"f7_attn_gqa_{tag}.npz")
    pre = ratio + "."
    dtype = f[pre + "dec.q"].dtype
    R = {"r7": 7, "r3": 3}[ratio]
    assert f[pre + "dec.q"].shape[1] == R * f[pre + "dec.k"].shape[1]
    ulp = AR.ulp_of(dtype)
    _dec_check(f, pre + "dec.", dtype, 1e-3 + 2 * ulp * float(f[pre + "dec.y"].float().abs().max()))
    _pre_check(f, pre + "pre.", dtype, 1e-3 + 2 * ulp * float(f[pre + "pre.y"].float().abs().max()), 5e-2, 4e-3)


# ------------------------------------------------------------------------------------ the oracle at odd ratios


def _oracle_decode(o, q, k, v, mask, dtype, hist=None):
    HQ, D = q.shape[1], q.shape[3]
    H, S = k.shape[1], k.shape[2]
    code = DT_CODE[dtype]
    es = np.float32 if code == 0 else np.uint16
    y, attn, probs = np.zeros((HQ, D), es), np.zeros((H, S), es), np.zeros((HQ, S), es)
    o.call("cc_decode_attn_gqa", o.ptr(to_np(q[0, :, 0])), o.ptr(to_np(k[0])), o.ptr(to_np(v[0])), o.ptr(to_np(mask[0, :, 0])),
           HQ, H, S, D, code, 1.0 / math.sqrt(D), o.ptr(y), o.ptr(attn), o.ptr(probs), None, None, None, None, 0, None)
    return from_np(y, dtype), from_np(probs, dtype), from_np(attn, dtype)


@pytest.mark.parametrize("dtype,H,R,S,D", [(torch.bfloat16, 4, 7, 300, 128), (torch.float16, 2, 3, 1000, 64),
                                           (torch.float32, 2, 3, 77, 64), (torch.bfloat16, 1, 7, 13, 128),
                                           (torch.float16, 4, 7, 513, 128)])
def test_oracle_decode_attention_at_odd_ratios(oracle, dtype, H, R, S, D):
    gen = torch.Generator().manual_seed(S + R)
    HQ = H * R
    q = torch.randn(1, HQ, 1, D, generator=gen).to(dtype)
    k = torch.randn(1, H, S, D, generator=gen).to(dtype)
    v = torch.randn(1, H, S, D, generator=gen).to(dtype)
    mask = torch.rand(1, H, 1, S, generator=gen) > 0.3
    mask[..., -1] = True
    y, p, gm = _oracle_decode(oracle, q, k, v, mask, dtype)
    yr, pr, gr = AR.decode_ref(q, k, v, mask)
    ulp = AR.ulp_of(dtype)
    assert float((y.double() - yr).abs().max()) <= 1e-3 + 2 * ulp * float(yr.abs().max())
    assert float((p.double() - pr).abs().max()) < 1e-3 + 2 * ulp
    assert float((gm.double() - gr).abs().max()) < 1e-3 + 2 * ulp


@pytest.mark.parametrize("dtype,H,R,L,D", [(torch.bfloat16, 4, 7, 100, 128), (torch.float16, 2, 3, 130, 64),
                                           (torch.float32, 1, 7, 45, 64), (torch.bfloat16, 2, 3, 33, 128)])
def test_oracle_prefill_attention_at_odd_ratios(oracle, dtype, H, R, L, D):
    gen = torch.Generator().manual_seed(L + R)
    HQ = H * R
    q = torch.randn(1, HQ, L, D, generator=gen).to(dtype)
    k = torch.randn(1, H, L, D, generator=gen).to(dtype)
    v = torch.randn(1, H, L, D, generator=gen).to(dtype)
    code = DT_CODE[dtype]
    es = np.float32 if code == 0 else np.uint16
    y, cs, ob = np.zeros((HQ, L, D), es), np.zeros((H, L), np.float32), np.zeros((H, L), np.float32)
    bands = (3, 17)
    bo = np.zeros((len(bands), H, L), np.float32)
    barr = (C.c_int32 * len(bands))(*bands)
    oracle.call("cc_prefill_attn_bands", oracle.ptr(to_np(q[0])), oracle.ptr(to_np(k[0])), oracle.ptr(to_np(v[0])), HQ, H, L, D, code,
                1.0 / math.sqrt(D), oracle.ptr(y), oracle.ptr(cs), oracle.ptr(ob), 16, barr, len(bands), oracle.ptr(bo), None, 0, None)
    ref = AR.prefill_ref(q, k, v, obs_len=16, bands=bands)
    ulp = AR.ulp_of(dtype)
    yr = ref["y"]
    assert float((from_np(y, dtype).double() - yr).abs().max()) <= 1e-3 + 2 * ulp * float(yr.abs().max())
    tight = code == 0
    assert float((torch.from_numpy(cs).double() - ref["colsum"]).abs().max()) < (1e-3 if tight else 5e-2)
    assert float((torch.from_numpy(ob).double() - ref["obs"]).abs().max()) < (1e-3 if tight else 4e-3)
    for i, b in enumerate(bands):
        assert float((torch.from_numpy(bo[i]).double() - ref["bands"][b]).abs().max()) < (1e-3 if tight else 5e-2), b


@pytest.mark.parametrize("H,R", [(4, 7), (2, 3)])
def test_oracle_heavy_hitter_pipeline_at_odd_ratios(oracle, H, R):
    """The oracle's update -> attention (history fused) pipeline, the checker of the GPU step tests at these ratios: every
    step's y and group mean against attn_ref on the oracle's own cache, the history grown by exactly that group mean, and the
    evicted slot the arg-min of the heavy-hitter scores (cache.py:727-749)."""
    o = oracle
    dtype, S, D, g, w, T = torch.bfloat16, 96, 128, 4, 10, 90
    HQ, code = H * R, 1
    gen = torch.Generator().manual_seed(100 + R)
    k0 = torch.randn(H, S, D, generator=gen).to(dtype)
    v0 = torch.randn(H, S, D, generator=gen).to(dtype)
    st = dict(k=to_np(k0), v=to_np(v0), pos=np.full((H, S), -1, np.int32), mask=np.zeros((H, S), np.uint8),
              cts=np.full(H, T, np.int32), num=np.zeros((H, S), np.float64), denom=np.zeros((H, S), np.int32), ctr=np.zeros(1, np.int64))
    st["pos"][:, :T] = np.arange(T)
    st["mask"][:, :T] = 1
    st["num"][:, :T] = torch.rand(H, T, generator=gen, dtype=torch.float64).numpy()
    st["denom"][:, :T] = 1
    ulp = 2.0 ** -8
    for t in range(24):
        p = T + t
        pt = np.array([p], np.int32)
        k1 = torch.randn(H, D, generator=gen).to(dtype)
        v1 = torch.randn(H, D, generator=gen).to(dtype)
        q1 = (1.5 * torch.randn(HQ, D, generator=gen)).to(dtype)
        dn = np.maximum(st["denom"], 1).astype(np.float32)
        sc = (st["num"].astype(np.float32) / dn).astype(np.float32)
        sc[(st["pos"] < g) | (st["pos"] >= p - w)] = 1.0
        sc[st["pos"] == -1] = 0.0
        view = o.view(st["k"], st["v"], st["pos"], st["mask"], st["cts"], code)
        idx = np.zeros(H, np.int64)
        o.call("cc_decode_update_heavy_hitter", C.byref(view), o.ptr(to_np(k1)), o.ptr(to_np(v1)), o.ptr(pt), o.ptr(st["num"]),
               o.ptr(st["denom"]), g, w, o.ptr(idx), None)
        assert np.array_equal(idx, sc.argmin(axis=1)), f"step {t}"
        num_before = st["num"].copy()
        yo, ao = np.zeros((HQ, D), np.uint16), np.zeros((H, S), np.uint16)
        o.call("cc_decode_attn_gqa", o.ptr(to_np(q1)), o.ptr(st["k"]), o.ptr(st["v"]), o.ptr(st["mask"]), HQ, H, S, D, code,
               1.0 / math.sqrt(D), o.ptr(yo), o.ptr(ao), None, o.ptr(st["num"]), o.ptr(st["denom"]), o.ptr(st["ctr"]), None, 0, None)
        kk, vv = from_np(st["k"], dtype), from_np(st["v"], dtype)
        yr, _, gr = AR.decode_ref(q1, kk.unsqueeze(0), vv.unsqueeze(0), torch.from_numpy(st["mask"].astype(bool)).view(1, H, 1, S))
        y, gm = from_np(yo, dtype).double(), from_np(ao, dtype).double()
        assert float((y - yr).abs().max()) <= 1e-3 + 2 * ulp * float(yr.abs().max()), f"step {t}: y"
        assert float((gm - gr).abs().max()) < 1e-3 + 2 * ulp, f"step {t}: group mean"
        assert np.array_equal(st["num"], num_before + gm.numpy()), f"step {t}: history"
    assert int(st["ctr"][0]) == 24


# ------------------------------------------------------------------------------------ setup-time refusal


@pytest.mark.parametrize("mode,bits", [("fused", 8), ("fp8", 8), ("uint4", 4)])
@pytest.mark.parametrize("n_head,n_kv", [(28, 4), (6, 2)])
def test_fused_quant_cache_refused_at_setup_for_unserved_ratios(mode, bits, n_head, n_kv):
    """A Qwen2-shaped model (7 query heads per kv head) or one with 3 per kv head asks for a fused quantised cache: the harness
    raises before any cache exists, naming the ratio — not at the first decode token after a whole prefill."""
    from cold_compress_amd._abi import ColdCompressError
    from cold_compress_amd.harness import ModelArgs, Transformer, setup_caches
    from cold_compress_amd.harness.model import CONFIGS

    cfg = dict(CONFIGS["Qwen2-7B-Instruct"], n_layer=1, block_size=256, vocab_size=64, intermediate_size=64)
    cfg.update(n_head=n_head, n_local_heads=n_kv, dim=n_head * 128)
    model = Transformer(ModelArgs(**cfg)).to(torch.bfloat16)
    kw = dict(max_cache_length=[64], cache_bits=bits, cache_quant_mode=mode, cache_length_pattern="tile", cache_strategy=["heavy_hitter"],
              cache_strategy_pattern="tile", prompt_compression_strategy=["heavy_hitter"], global_tokens=4, recent_window=10,
              history_window_size=1, attn_thresholding=False)
    with pytest.raises(ColdCompressError, match=f"{n_head // n_kv} per kv head"):
        setup_caches(model, None, "cpu", 128, kw)
    assert model.layers[0].attention.kv_cache is None


# ------------------------------------------------------------------------------------ the step fuzzer's draws


class _Stop(Exception):
    pass


class _LoggedRandom:
    """random.Random that records every value it hands out."""

    def __init__(self, seed):
        import random

        self.r, self.log = random.Random(seed), []

    def __getattr__(self, name):
        fn = getattr(self.r, name)

        def wrapped(*a, **k):
            v = fn(*a, **k)
            self.log.append(v)
            return v

        return wrapped


def _fuzz_draws(monkeypatch, n, **kw):
    """The draws of tools/fuzz_step.py's step (even cases) and hybrid-step (odd cases) families from seed 3, up to the first cache."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import fuzz_step as F

    def stop(*a, **k):
        raise _Stop

    monkeypatch.setattr(F.cache, "get_cache_constructor", stop)
    rng, out = _LoggedRandom(3), []
    for i in range(n):
        with pytest.raises(_Stop):
            (F.one_hybrid_step if i % 2 else F.one)(rng, i, **kw)
        out.append(tuple("HYB" if v is F.HYB else "HYB_YAML" if v is F.HYB_YAML else v for v in rng.log))
        rng.log.clear()
    return out


def test_fuzzer_default_draws_unchanged(monkeypatch):
    """Recorded from the fuzzer before it had a ratio option: without the option the same seed names the same cases (the
    differential fuzz test and the small-grid stress test keep their cases); with it only the ratio draw changes."""
    bf, f16, f32 = torch.bfloat16, torch.float16, torch.float32
    want = [("recent_global", f32, 128, 2, 4, 36, 74, 2781, 4096, 3961, 2781, 2256, 2781, 1, 8, 4),
            (f16, 8, 4, 67, 2801, 3311, 9000, 9000, "HYB", 0.6714114753695926, 0),
            ("recent_global", f32, 16, 3, 1, 23, 283, 2737, 9000, 3794, 9000, 6471, 6471, 1, 6, None),
            (bf, 2, 8, 63, 1257, 3894, 9000, 3894, "HYB_YAML", 0.5072429838290595, 3)]
    assert _fuzz_draws(monkeypatch, 4) == want
    assert _fuzz_draws(monkeypatch, 4, ratios=None) == want
    odd = _fuzz_draws(monkeypatch, 12, ratios=[3, 5, 6, 7, 12])
    assert all(c[4] in (3, 5, 6, 7, 12) for c in odd[0::2]) and all(c[2] in (3, 5, 6, 7, 12) for c in odd[1::2])
