"""The MXFP4 fused KV cache (cache_bits=4, cache_quant_mode="mxfp4"; include/coldcompress.h): OCP e2m1 codes, two per byte, one e8m0
scale byte per block of 32 channels, decoded in the decode kernels by v_cvt_scalef32_pk_{bf16,f16}_fp4.  Pinned as the other formats:
  * the hardware decode, exhaustively: all 256 bytes in every byte position under every scale byte, bf16 and f16, through
    cc_kv_dequant_rows against the numpy twin of the contract (tests/kv_mxfp4_twin.py, itself checked against exact fractions by
    tests/test_kv_mxfp4_host.py), bit for bit — f16 overflow (+-inf), underflow (rounded subnormals, +-0) and the NaN of the scale byte
    0xff included: the twin states what the instruction returns;
  * cc_kv_quant_rows against the twin: images and scale words equal;
  * every served policy's MXFP4 step against the SAME policy's 16-bit step fed the dequantised values: every buffer and y bit for bit;
  * the graphed harness loop against the unquantised run, with bounds measured on this format.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from helpers import DT_CODE

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_mxfp4_twin as tw  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = __import__("helpers").TEST_DEVICE
D = 128
MX4 = 0x300 | 4  # CC_QUANT_MXFP4
HYB5 = [{"strategy": "special"}, {"strategy": "special_punc"}, {"strategy": "special_punc_heavy_hitter", "heavy_hitter_frac": 0.3},
        {"strategy": "special_punc_window", "recent_window": 0.3}, {"strategy": "full"}]
HYB_YAML = [{"strategy": "window", "recent_window": 0.1},
            {"strategy": "window_heavy_hitter", "heavy_hitter_frac": 0.25, "recent_window": 0.1},
            {"strategy": "window_heavy_hitter", "heavy_hitter_frac": 0.5, "recent_window": 0.1}, {"strategy": "full"}]
TOKEN_IDS = {"special": [[1], [2, 3]], "punctuation": [5, 6, 7]}
NAME = {torch.bfloat16: "bf16", torch.float16: "f16"}


def _abi():
    from cold_compress_amd import _abi

    return _abi


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _words(par):
    """kv_qparams-like float32 storage [..., 4] -> its int32 bit patterns (the scale words are never floats)."""
    return par.contiguous().view(torch.int32)


def _quant_rows(x):
    """[N, Dx] rows -> (images [N, Dx / 2] uint8, K words [N, 2] int32, round trip [N, Dx]) by cc_kv_quant_rows / cc_kv_dequant_rows."""
    N, Dx = x.shape
    kq, vq = torch.empty((N, Dx // 2), dtype=torch.uint8, device=DEV), torch.empty((N, Dx // 2), dtype=torch.uint8, device=DEV)
    par = torch.empty((N, 4), dtype=torch.float32, device=DEV)
    out, out2 = torch.empty_like(x), torch.empty_like(x)
    _abi().call("cc_kv_quant_rows", _p(x), _p(x), 1, N, Dx, DT_CODE[x.dtype], MX4, _p(kq), _p(vq), _p(par), _st())
    _abi().call("cc_kv_dequant_rows", _p(kq), _p(vq), _p(par), 1, N, Dx, DT_CODE[x.dtype], MX4, _p(out), _p(out2), _st())
    return kq, _words(par)[:, 0:2], out


def _twin_rows(x):
    """The twin's (images, K words [N, 2] int32) of rows x (a CPU tensor of a 16-bit dtype)."""
    img, sb = tw.quant_rows(x.float().numpy())
    w = np.stack([tw.scale_word(sb), np.zeros(len(sb), np.uint32)], axis=-1)
    return img, w.view(np.int32)


# ---------------------------------------------------------------------------------------------------------- the converters
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_every_code_under_every_scale_decodes_as_the_twin(dtype):
    """Exhaustive: row (s, i), i = 0 .. 15, holds the scale byte (s + 64 * ((b + i) & 3)) & 255 in block b and, at byte j, the codes
    (i + j) & 15 (low nibble) and (3 * i + j + 5) & 15 (high nibble): over the 4096 rows every one of the 128 positions of a row
    decodes every code under every scale byte 0 .. 255 exactly once (the contract uses 7 .. 247 and 0xff) — all four byte selects of
    all 16 words, both nibbles, the four blocks' scale bytes all different within a row.  bf16 is exact in 7 .. 247; f16 overflows to
    +-inf and underflows through rounded subnormals to +-0 — the twin says exactly that, and so does the header."""
    n = 256 * 16
    s_, i_ = np.divmod(np.arange(n), 16)
    j = np.arange(D // 2)
    img = (((i_[:, None] + j) & 15) | (((3 * i_[:, None] + j + 5) & 15) << 4)).astype(np.uint8)
    sb = ((s_[:, None] + 64 * ((np.arange(4) + i_[:, None]) & 3)) & 255).astype(np.uint8)
    combos = (sb.astype(np.int64).repeat(32, axis=1) * 16 + tw.unpack(img)) * D + np.arange(D)
    assert len(np.unique(combos)) == 256 * 16 * D == n * D  # every (scale byte, code, position in the row), once
    par = np.zeros((n, 4), np.uint32)
    par[:, 0] = tw.scale_word(sb)
    par[:, 2] = tw.scale_word(sb[::-1])
    kq, vq = torch.from_numpy(img).to(DEV), torch.from_numpy(img[::-1].copy()).to(DEV)
    k = torch.empty((n, D), dtype=dtype, device=DEV)
    v = torch.empty_like(k)
    part = torch.from_numpy(par.view(np.float32)).to(DEV)
    _abi().call("cc_kv_dequant_rows", _p(kq), _p(vq), _p(part), 1, n, D, DT_CODE[dtype], MX4, _p(k), _p(v), _st())
    torch.cuda.synchronize()
    for got, im, sc in ((_bits(k), img, sb), (_bits(v), img[::-1], sb[::-1])):
        want = tw.dequant_bits(im, sc, NAME[dtype])
        if not np.array_equal(got, want):
            r, c = np.argwhere(got != want)[0]
            raise AssertionError(f"{(got != want).sum()} values differ; first: row {r} col {c} (scale byte {sc[r, c // 32]}, code "
                                 f"{tw.unpack(im)[r, c]}): {got[r, c]:#06x} vs {want[r, c]:#06x}")
    # the scale byte 0xff: every element of the block is the pinned NaN
    nan = np.repeat(sb == 0xFF, 32, axis=1)
    assert nan.sum() == 16 * D and np.all(_bits(k)[nan] == tw.NAN_BITS[NAME[dtype]])


def _edge_rows(dtype):
    g = np.random.default_rng(5)
    big = 65504.0 if dtype == torch.float16 else 3.0e38
    rows = [g.standard_normal(D) * 2, g.standard_normal(D) * 1e-3 + 7]
    out = g.standard_normal(D)
    out[17] *= 50  # one outlier channel
    rows.append(out)
    ties = np.zeros(D)
    ties[0:16] = [6, 0.25, -0.25, 0.75, -0.75, 1.25, -1.25, 1.75, -1.75, 2.5, -2.5, 3.5, -3.5, 5, -5, -0.0]  # e_b = 0: every tie
    ties[32:48] = np.array([6, 0.25, -0.25, 0.75, -0.75, 1.25, -1.25, 1.75, -1.75, 2.5, -2.5, 3.5, -3.5, 5, -5, 0.5]) * 2.0 ** -9
    ties[64:70] = [6 * 2.0 ** 5, 6 * 2.0 ** 5 * (1 - 2.0 ** -8), 3 * 2.0 ** 5, 1, 2, 3]  # a block maximum on the exponent boundary
    ties[96:100] = [6 * 2.0 ** 5 * (1 + 2.0 ** -7), 100, -100, 50]  # ... and one bf16 / f16 step above it
    rows.append(ties)
    rows.append(np.zeros(D))  # all-zero blocks
    z = np.zeros(D)
    z[40], z[41] = -0.0, 1e-3
    rows.append(z)
    rows.append(np.linspace(-big, big, D))  # the dtype's extremes (bf16: the clamp at e = 120)
    rows.append(np.where(np.arange(D) % 2 == 0, big, -big))
    rows.append(g.standard_normal(D) * (1e-39 if dtype == torch.bfloat16 else 1e-6))  # subnormals (bf16: below 6 * 2^-120)
    nf = g.standard_normal(D)
    nf[3], nf[70], nf[71] = np.inf, -np.inf, np.nan  # blocks 0 and 2 hold non-finite values
    rows.append(nf)
    return torch.tensor(np.stack(rows), dtype=torch.float32).to(dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("rows", ["random", "edge"])
def test_row_conversion_matches_the_twin(dtype, rows):
    if rows == "random":
        g = torch.Generator().manual_seed(13)
        x = (torch.randn(300, 4, 32, generator=g) * torch.exp2(torch.randint(-12, 12, (300, 4, 1), generator=g).float())).reshape(300, D)
        x = (x + torch.randn(300, 1, generator=g) * 0.5).to(dtype)
    else:
        x = _edge_rows(dtype)
    kq, kw, rt = _quant_rows(x.to(DEV))
    torch.cuda.synchronize()
    img, w = _twin_rows(x)
    got = kq.cpu().numpy()
    assert np.array_equal(got, img), np.argwhere(got != img)[:5]
    assert np.array_equal(kw.cpu().numpy(), w), np.argwhere(kw.cpu().numpy() != w)[:5]
    want = tw.dequant_bits(img, tw.quant_rows(x.float().numpy())[1], NAME[dtype])
    assert np.array_equal(_bits(rt), want), np.argwhere(_bits(rt) != want)[:5]
    if rows == "edge":
        sb = tw.quant_rows(x.float().numpy())[1]
        assert list(sb[4]) == [7, 7, 7, 7] and list(sb[9][[0, 2]]) == [0xFF, 0xFF] and sb[9][1] != 0xFF
        assert np.all(_bits(rt)[9, :32] == tw.NAN_BITS[NAME[dtype]]) and np.all(_bits(rt)[9, 64:96] == tw.NAN_BITS[NAME[dtype]])


def test_other_formats_stay_unsupported():
    lib = _abi().lib()
    x = torch.ones(4, D, dtype=torch.bfloat16, device=DEV)
    q = torch.zeros(4, D, dtype=torch.uint8, device=DEV)
    par = torch.zeros(4, 4, device=DEV)
    for fmt in (0x300 | 8, 0x300 | 2, 0x100 | 4, 2, 4):
        assert lib["cc_kv_quant_rows"](_p(x), _p(x), 1, 4, D, 1, fmt, _p(q), _p(q), _p(par), _st()) == -2
        assert lib["cc_kv_dequant_rows"](_p(q), _p(q), _p(par), 1, 4, D, 1, fmt, _p(x), _p(x), _st()) == -2
        assert lib["cc_decode_step_quant_single_launch"](32, 8, 4096, D, 1, fmt) == 0
        assert lib["cc_decode_step_hybrid_quant_single_launch"](32, 8, 4096, D, 1, fmt) == 0
    xf = x.float()
    assert lib["cc_kv_quant_rows"](_p(xf), _p(xf), 1, 4, D, 0, MX4, _p(q), _p(q), _p(par), _st()) == -2  # 16-bit model dtypes only
    torch.cuda.synchronize()
    assert bool((q == 0).all()) and bool((par == 0).all())
    U4 = 0x200 | 4
    for HQ, H, S in ((32, 8, 4096), (32, 8, 18432), (16, 2, 300), (64, 8, 4096), (32, 8, 65536), (28, 4, 4096)):
        for dt in (1, 2):
            assert lib["cc_decode_step_quant_single_launch"](HQ, H, S, D, dt, MX4) == lib["cc_decode_step_quant_single_launch"](HQ, H, S, D, dt, U4)
            assert lib["cc_decode_step_hybrid_quant_single_launch"](HQ, H, S, D, dt, MX4) == \
                lib["cc_decode_step_hybrid_quant_single_launch"](HQ, H, S, D, dt, U4)


# ---------------------------------------------------------------------------------------------------------- the steps
def _mk(strategy, H, S, dtype, mx4, W=1, g=4, w=10):
    import cold_compress_amd.cache as cache

    cls, rk = cache.get_cache_constructor(strategy)
    kw = dict(max_cache_length=S, max_seq_length=4 * S, cache_bits=4 if mx4 else None, global_tokens=g, recent_window=w,
              history_window_size=W, attn_thresholding=False)
    lk = {k: kw[k] for k in rk}
    if W != 1:
        lk["history_window_size"] = W
    if mx4:
        lk["cache_quant_mode"] = "mxfp4"
    with torch.device(DEV):
        return cls(1, H, D, dtype, **lk)


def _twin_round_trip(r, H, dtype):
    bits = tw.round_trip_bits(r.reshape(H, D).float().numpy(), NAME[dtype])
    return torch.from_numpy(bits.view(np.int16)).view(dtype).view(1, H, 1, D).to(DEV)


@pytest.mark.parametrize("strategy", ["heavy_hitter", "recent_global", "full", "random"])
@pytest.mark.parametrize("dtype,H,HQ,S,T", [(torch.bfloat16, 8, 32, 4096, 4090), (torch.float16, 2, 16, 300, 290)])
@pytest.mark.parametrize("single", [False, True])
def test_mxfp4_step_equals_16bit_step_on_dequantised_values(strategy, dtype, H, HQ, S, T, single):
    """`b` = the MXFP4 cache, `a` = the same policy's 16-bit cache holding b's DEQUANTISED values and fed the twin's round trip of every
    new token: y, the cache contents, pos, mask, cache_cts and the history agree bit for bit, 12 steps, in both launch forms; the step
    writes exactly the inserted token's rows, which are cc_kv_quant_rows of that token."""
    abi = _abi()
    abi.lib()["cc_decode_step_set_single_launch"](1 if single else 0)
    try:
        a, b = _mk(strategy, H, S, dtype, False), _mk(strategy, H, S, dtype, True)
        for kv in (a, b):
            if hasattr(kv, "single_launch"):
                kv.single_launch = single
        gen = torch.Generator().manual_seed(41)
        k0 = torch.randn(1, H, T, D, generator=gen).to(dtype).to(DEV)
        v0 = (2.0 * torch.randn(1, H, T, D, generator=gen)).to(dtype).to(DEV)
        for kv in (a, b):
            kv.update_kv(torch.arange(T, device=DEV), k0, v0, True)
            if strategy == "heavy_hitter":
                g2 = torch.Generator().manual_seed(42)
                kv.attn_history_num[0, :, :T, 0] = torch.rand(H, T, generator=g2, dtype=torch.float64).to(DEV)
                kv.attn_history_denom[0, :, :T] = torch.randint(1, 5, (H, T), generator=g2, dtype=torch.int32).to(DEV)
        kd, vd = b.dequantized_kv()
        a.k_cache.copy_(kd)
        a.v_cache.copy_(vd)
        if strategy == "random":
            draws = [torch.rand(S, generator=gen).to(DEV) for _ in range(20)]
            for kv in (a, b):
                it = iter(list(draws))
                kv._rand = lambda it=it: next(it)
        hs = torch.arange(H, device=DEV)
        for t in range(12):
            p = torch.tensor([T + 5 + t], dtype=torch.int32, device=DEV)
            k1 = torch.randn(1, H, 1, D, generator=gen).to(dtype)
            v1 = (2.0 * torch.randn(1, H, 1, D, generator=gen)).to(dtype)
            q = torch.randn(1, HQ, 1, D, generator=gen).to(dtype).to(DEV)
            kq_new, kpar_new, _ = _quant_rows(k1.reshape(H, D).to(DEV))
            vq_new, vpar_new, _ = _quant_rows(v1.reshape(H, D).to(DEV))
            for im, wd, src in ((kq_new, kpar_new, k1), (vq_new, vpar_new, v1)):  # ... which are the twin's
                ti, tw_ = _twin_rows(src.reshape(H, D))
                assert np.array_equal(im.cpu().numpy(), ti) and np.array_equal(wd.cpu().numpy(), tw_)
            kimg0, vimg0, par0 = b.k_cache_q.clone(), b.v_cache_q.clone(), b.kv_qparams.clone()
            ya = a.decode_step(q, _twin_round_trip(k1, H, dtype), _twin_round_trip(v1, H, dtype), p)
            yb = b.decode_step(q, k1.to(DEV), v1.to(DEV), p)
            torch.cuda.synchronize()
            if not torch.equal(ya, yb):
                d = (ya.float() - yb.float()).abs()[0, :, 0]
                kd, vd = b.dequantized_kv()
                raise AssertionError(f"step {t}: attention output: max |dy| {float(d.max()):.3e}; K rows differing "
                                     f"{(kd != a.k_cache).any(-1).nonzero().tolist()[:6]}; V rows {(vd != a.v_cache).any(-1).nonzero().tolist()[:6]}")
            kd, vd = b.dequantized_kv()
            assert torch.equal(kd, a.k_cache) and torch.equal(vd, a.v_cache), f"step {t}: cache contents"
            for name in ("pos", "mask", "cache_cts", "attn_history_num", "attn_history_denom", "attn_counter"):
                if hasattr(a, name):
                    assert torch.equal(getattr(a, name), getattr(b, name)), f"step {t}: {name}"
            here = b.pos[0] == int(p)  # [Hp, S]: the slot the token went to (every head's, or the shared one)
            if not bool(here.any(dim=1).all()):
                continue
            slot = here.int().argmax(dim=1).expand(H)
            assert torch.equal(b.k_cache_q[0, hs, slot], kq_new) and torch.equal(b.v_cache_q[0, hs, slot], vq_new), f"step {t}: image"
            assert torch.equal(_words(b.kv_qparams)[0, hs, slot, 0:2], kpar_new) and torch.equal(_words(b.kv_qparams)[0, hs, slot, 2:4], vpar_new)
            keep = torch.ones(H, S, dtype=torch.bool, device=DEV)
            keep[hs, slot] = False
            for now, before in ((b.k_cache_q, kimg0), (b.v_cache_q, vimg0), (_words(b.kv_qparams), _words(par0))):
                assert torch.equal(now[0][keep], before[0][keep]), f"step {t}: rows other than the inserted one changed"
        if strategy == "heavy_hitter":
            assert b.step_status(HQ) == 0
        if single and S == 4096:
            if strategy == "heavy_hitter":
                assert b.single_launch_active(HQ)
            assert abi.lib()["cc_decode_step_quant_single_launch"](HQ, H, S, D, DT_CODE[dtype], MX4) == 1
    finally:
        abi.lib()["cc_decode_step_set_single_launch"](1)


def _mk_hyb(strategies, H, S, dtype, mx4):
    import cold_compress_amd.cache as cache

    kw = dict(max_cache_length=S, max_seq_length=S, cache_bits=4 if mx4 else None, global_tokens=4, token_ids=TOKEN_IDS,
              min_recovery_frac=0.9, hybrid_strategies=strategies)
    if mx4:
        kw["cache_quant_mode"] = "mxfp4"
    with torch.device(DEV):
        return cache.KVCacheHybrid(1, H, D, dtype, **kw)


def _pair(kind, W, strategies, H, S, T, dtype, seed):
    """Twin caches in the same decode-ready state: a (16-bit, holding b's dequantised K / V) and b (MXFP4)."""
    gen = torch.Generator().manual_seed(seed)
    if kind == "hh":
        a, b = _mk("heavy_hitter", H, S, dtype, False, W=W), _mk("heavy_hitter", H, S, dtype, True, W=W)
    else:
        a, b = _mk_hyb(strategies, H, S, dtype, False), _mk_hyb(strategies, H, S, dtype, True)
    k0 = torch.randn(1, H, T, D, generator=gen).to(dtype).to(DEV)
    v0 = (2.0 * torch.randn(1, H, T, D, generator=gen)).to(dtype).to(DEV)
    ring0 = (torch.rand(H, S, a.attn_history_num.shape[-1], generator=gen) * 1e-2).to(dtype)
    den0 = torch.randint(1, 500, (H, S), generator=gen, dtype=torch.int32)
    fill = torch.tensor([T if h % 2 == 0 else max(4, T // 2) for h in range(H)], dtype=torch.int32)
    sp0 = torch.rand(H, S, generator=gen) < 0.02
    pu0 = torch.rand(H, S, generator=gen) < 0.02
    for kv in (a, b):
        if kind == "hh":
            kv.update_kv(torch.arange(T, device=DEV), k0, v0, True)
        else:
            kv.update_kv(torch.arange(T, device=DEV), k0, v0, True, input_ids=torch.zeros(T, dtype=torch.int64, device=DEV))
            kv.cache_strategies = (torch.arange(H, device=DEV) % len(strategies)).to(torch.int64).contiguous()
            kv.requires_heavy_hitter = any("heavy_hitter" in s["strategy"] for s in strategies)
            kv.cache_cts.copy_(fill.to(DEV))
            live = torch.arange(S, device=DEV).view(1, S) < fill.to(DEV).view(H, 1)
            kv.mask[0, :, 0, :] = live
            kv.pos[0] = torch.where(live, torch.arange(S, device=DEV, dtype=kv.pos.dtype).view(1, S).expand(H, S),
                                    torch.full_like(kv.pos[0], -1))
            if hasattr(kv, "special_mask"):
                kv.special_mask[0] = sp0.to(DEV) & live
                kv.num_special.fill_(int(sp0[0, : int(fill[0])].sum()))
            if hasattr(kv, "punc_mask"):
                kv.punc_mask[0] = pu0.to(DEV) & live
                kv.num_punc.fill_(3)
        kv.attn_history_num.copy_(ring0.to(DEV).unsqueeze(0))
        kv.attn_history_denom.copy_(den0.to(DEV).unsqueeze(0))
    kd, vd = b.dequantized_kv()
    a.k_cache.copy_(kd)
    a.v_cache.copy_(vd)
    return a, b, gen


def _run_lockstep(kind, W, strategies, H, HQ, S, T, steps, dtype, seed, check_rows=True):
    a, b, gen = _pair(kind, W, strategies, H, S, T, dtype, seed)
    for t in range(steps):
        p = torch.tensor([T + 3 + t], dtype=torch.int32, device=DEV)
        k1 = torch.randn(1, H, 1, D, generator=gen).to(dtype).to(DEV)
        v1 = (2.0 * torch.randn(1, H, 1, D, generator=gen)).to(dtype).to(DEV)
        q = torch.randn(1, HQ, 1, D, generator=gen).to(dtype).to(DEV)
        kq_new, kpar_new, kh = _quant_rows(k1.reshape(H, D))
        vq_new, vpar_new, vh = _quant_rows(v1.reshape(H, D))
        kimg0, vimg0, par0 = (b.k_cache_q.clone(), b.v_cache_q.clone(), b.kv_qparams.clone()) if check_rows else (None, None, None)
        if kind == "hh":
            ya = a.decode_step(q, kh.view(1, H, 1, D), vh.view(1, H, 1, D), p)
            yb = b.decode_step(q, k1, v1, p)
        else:
            ids = torch.tensor([[6 if t % 5 == 2 else 11]], dtype=torch.int64, device=DEV)  # every fifth token is punctuation
            ya = a.decode_step(q, kh.view(1, H, 1, D), vh.view(1, H, 1, D), p, input_ids=ids)
            yb = b.decode_step(q, k1, v1, p, input_ids=ids)
        torch.cuda.synchronize()
        assert torch.equal(ya, yb), f"step {t}: attention output, max |dy| {float((ya.float() - yb.float()).abs().max()):.3e}"
        kd, vd = b.dequantized_kv()
        assert torch.equal(kd, a.k_cache) and torch.equal(vd, a.v_cache), f"step {t}: cache contents"
        bb = dict(b.named_buffers())
        for name, ta in a.named_buffers():
            if name not in ("k_cache", "v_cache"):
                assert torch.equal(ta, bb[name]), f"step {t}: {name}"
        if check_rows:  # the step writes the inserted token's rows (cc_kv_quant_rows of them) and nothing else
            slot = (b.pos[0] == int(p)).int().argmax(dim=1)
            hs = torch.arange(H, device=DEV)
            assert torch.equal(b.k_cache_q[0, hs, slot], kq_new) and torch.equal(b.v_cache_q[0, hs, slot], vq_new), f"step {t}: image"
            assert torch.equal(_words(b.kv_qparams)[0, hs, slot, 0:2], kpar_new) and torch.equal(_words(b.kv_qparams)[0, hs, slot, 2:4], vpar_new)
            keep = torch.ones(H, b.max_cache_length, dtype=torch.bool, device=DEV)
            keep[hs, slot] = False
            for now, before in ((b.k_cache_q, kimg0), (b.v_cache_q, vimg0), (_words(b.kv_qparams), _words(par0))):
                assert torch.equal(now[0][keep], before[0][keep]), f"step {t}: rows other than the inserted one changed"
    return a, b


@pytest.mark.parametrize("W", [8, 400])
def test_ring_lockstep_64_steps(W):
    """The windowed heavy hitter at C3 size (8 kv heads, 32 query heads, S = 4096): 64 steps of the MXFP4 ring step (two launches)."""
    a, b = _run_lockstep("hh", W, None, 8, 32, 4096, 4090, 64, torch.bfloat16, 51 + W, check_rows=(W == 8))
    assert not b.single_launch_active(32) and b.step_status(32) == 0


def test_hybrid_c4_lockstep_64_steps_one_launch():
    """C4 size (8 kv heads, 32 query heads, S = 18432): 64 steps of the MXFP4 hybrid step, as one launch."""
    H, HQ, S = 8, 32, 18432
    assert _abi().lib()["cc_decode_step_hybrid_quant_single_launch"](HQ, H, S, D, 1, MX4) == 1
    a, b = _run_lockstep("hyb", 400, HYB_YAML, H, HQ, S, 18300, 64, torch.bfloat16, 61, check_rows=False)
    assert b.single_launch_active(HQ) and a.single_launch_active(HQ)
    assert b.step_status(HQ) == 0


@pytest.mark.parametrize("two", [False, True])
def test_hybrid_small_both_forms(two):
    """A small f16 hybrid cache (appends, evictions, dropped and punctuation tokens) in the single- and the two-launch form."""
    fn = _abi().lib()["cc_decode_step_device_single_launch"]
    if two:
        fn(0)
    try:
        a, b = _run_lockstep("hyb", 400, HYB5, 2, 16, 1000, 20, 14, torch.float16, 71)
        assert b.single_launch_active(16) == a.single_launch_active(16)
        assert b.step_status(16) == 0
    finally:
        if two:
            fn(1)


def test_step_replays_in_a_hip_graph():
    """The MXFP4 heavy-hitter step captured once and replayed: the replays equal eager steps of a twin cache bit for bit."""
    H, HQ, S, T, dtype = 8, 32, 4096, 4000, torch.bfloat16
    gen = torch.Generator().manual_seed(91)
    a, b = _mk("heavy_hitter", H, S, dtype, True), _mk("heavy_hitter", H, S, dtype, True)
    k0 = torch.randn(1, H, T, D, generator=gen).to(dtype).to(DEV)
    v0 = (2.0 * torch.randn(1, H, T, D, generator=gen)).to(dtype).to(DEV)
    for kv in (a, b):
        kv.update_kv(torch.arange(T, device=DEV), k0, v0, True)
    q, k1, v1 = (torch.zeros(1, n, 1, D, dtype=dtype, device=DEV) for n in (HQ, H, H))
    p = torch.tensor([T], dtype=torch.int32, device=DEV)
    ins = [(torch.randn(1, HQ, 1, D, generator=gen).to(dtype).to(DEV), torch.randn(1, H, 1, D, generator=gen).to(dtype).to(DEV),
            torch.randn(1, H, 1, D, generator=gen).to(dtype).to(DEV)) for _ in range(9)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up outside the capture (workspaces), on both caches alike
        for kv in (a, b):
            q.copy_(ins[0][0]), k1.copy_(ins[0][1]), v1.copy_(ins[0][2])
            kv.decode_step(q, k1, v1, p)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    p.add_(1)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        yb = b.decode_step(q, k1, v1, p)
    for t in range(1, 9):
        q.copy_(ins[t][0]), k1.copy_(ins[t][1]), v1.copy_(ins[t][2])
        graph.replay()
        torch.cuda.synchronize()
        ya = a.decode_step(q, k1, v1, p)
        torch.cuda.synchronize()
        assert torch.equal(ya, yb), f"replay {t}"
        for name, ta in a.named_buffers():
            assert torch.equal(ta.view(torch.uint8) if ta.dtype == torch.float32 else ta, (dict(b.named_buffers())[name].view(torch.uint8)
                               if ta.dtype == torch.float32 else dict(b.named_buffers())[name])), f"replay {t}: {name}"
        p.add_(1)
    assert b.step_status(HQ) == 0


# ---------------------------------------------------------------------------------------------------------- the harness
def test_mxfp4_end_to_end_in_the_harness():
    """The tiny-Llama loop of tests/test_gpu_kv_fp8.py::test_fp8_end_to_end_in_the_harness with cache_quant_mode="mxfp4": prefill through
    the HIP path, row quantisation of the compacted prompt, hipGraph decode over the MXFP4 images, teacher-forced against the
    unquantised run."""
    from cold_compress_amd.harness import GraphedDecoder, ModelArgs, Transformer, decode_one_token, prefill, setup_caches

    dev = torch.device(DEV)
    cfg = dict(block_size=1024, vocab_size=512, n_layer=2, n_head=8, n_local_heads=2, dim=1024, intermediate_size=2048)
    torch.manual_seed(5)
    model = Transformer(ModelArgs(**cfg)).to(torch.bfloat16).eval()
    with torch.no_grad():
        g = torch.Generator().manual_seed(5)
        for n, p in model.named_parameters():
            p.fill_(1.0) if "norm" in n else p.normal_(0.0, 0.05, generator=g)
    model = model.to(dev)
    prompt = torch.randint(0, cfg["vocab_size"], (300,), generator=torch.Generator().manual_seed(3), dtype=torch.int32).to(dev)
    runs = {}
    for name, extra in (("bf16", {}), ("mxfp4", {"cache_bits": 4, "cache_quant_mode": "mxfp4"})):
        kw = dict(max_cache_length=[128.0], cache_bits=None, cache_length_pattern="tile", cache_strategy=["heavy_hitter"],
                  cache_strategy_pattern="tile", feed_long_prompts=False, prompt_compression_strategy=["heavy_hitter"], global_tokens=4,
                  recent_window=10, history_window_size=1, attn_thresholding=False, min_recovery_frac=0.9)
        kw.update(extra)
        setup_caches(model, None, dev, 400, kw)
        with torch.no_grad():
            tok, probs = prefill(model, prompt.view(1, -1), torch.arange(300, device=dev))
            pos = torch.tensor([300], dtype=torch.int32, device=dev)
            plist, toks = [probs.float().clone()], [int(tok)]
            cur = tok.view(1, 1).to(torch.int32)
            step = GraphedDecoder(model) if name != "bf16" else decode_one_token
            for i in range(16):
                nt, pr = step(model, cur, pos)
                plist.append(pr.float().clone())
                toks.append(int(nt))
                cur = (nt if name == "bf16" else torch.tensor(runs["bf16"][0][len(toks) - 1], device=dev)).view(1, 1).to(torch.int32)
                pos += 1
        torch.cuda.synchronize()
        kv = model.layers[0].attention.kv_cache
        runs[name] = (toks, plist, kv.memory_usage(), kv)
    assert torch.equal(runs["bf16"][1][0], runs["mxfp4"][1][0])  # prefill attends to the prompt's own k / v: identical
    worst = max(float((a - b).abs().max() / a.abs().max()) for a, b in zip(runs["bf16"][1], runs["mxfp4"][1]))
    agree = sum(int(a == b) for a, b in zip(runs["bf16"][0], runs["mxfp4"][0]))
    print(f"end to end, worst relative probability drift / tokens agreeing: {worst:.3f} / {agree} of {len(runs['bf16'][0])}")
    # Bounds from a measured run on MI355X: worst drift 4.98, 9 of 17 tokens agreeing, against uint4's 1.71 and 8 / 17,
    # FP8's 0.48 and 16 / 17 and uint8's 0.12 and 17 / 17 on the same model.  e2m1 is coarsest where the values are largest (one step
    # from 4 to 6 at the top of a block), and the largest K entries move a logit most: the worst probability row of this random-weight,
    # near-flat model moves three times as far as under the even 15-step grid, while as many tokens agree.  The bit-exact checks of
    # the step are the tests above; this one bounds the format's effect on a model (margins as the uint4 test's: 1.3 x, two tokens).
    assert worst < 6.5 and agree >= 7, (worst, agree)
    assert runs["mxfp4"][2] < 0.35 * runs["bf16"][2]
    kv = runs["mxfp4"][3]
    assert kv.fused_quant and kv.quant_format == MX4 and kv.k_cache.numel() == 0 and kv.step_status(cfg["n_head"]) == 0
    assert tuple(kv.k_cache_q.shape) == (1, cfg["n_local_heads"], kv.max_cache_length, D // 2)
