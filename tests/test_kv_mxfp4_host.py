"""CPU tests of the MXFP4 fused KV cache (cache_bits=4, cache_quant_mode="mxfp4"): the numpy twin of its numerical contract
(tests/kv_mxfp4_twin.py) against exact arithmetic in fractions, block independence, where the format is finer and where coarser than
the uint4 grid, construction of every served policy with the uint4 mode's buffers, memory, the refusals, the flag and the ABI
constant.  The kernels are checked against the twin on the GPU: tests/test_gpu_kv_mxfp4.py.

Round-trip RMS error on 4096 bf16 rows of N(0, 1), mxfp4 / uint4 (seeds 0, 1, 2; the twin's numbers):
  Gaussian rows                      0.116 / 0.100   1.15 - 1.16 x   coarser: 8 magnitudes per sign against 15 even steps
  one channel x 50                   0.61  / 1.12    0.54 - 0.55 x   finer: the outlier stretches its own block only
  per-channel log-normal spread      0.32  / 0.37    0.83 - 0.90 x   finer
  rows shifted by +3                 0.321 / 0.100   3.21 - 3.22 x   coarser: a symmetric format has no zero point
The two structural directions are asserted (outlier < 0.7 x, shifted > 2.5 x: margins of a quarter of what is seen); the other two
are stated in DESIGN §2.5."""
import argparse
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_mxfp4_twin as tw  # noqa: E402
import kv_uint4_twin as u4  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HYBRID = [{"strategy": "special"}, {"strategy": "special_punc"}, {"strategy": "special_punc_heavy_hitter", "heavy_hitter_frac": 0.3},
          {"strategy": "special_punc_window", "recent_window": 0.3}, {"strategy": "full"}]
GRID = [Fraction(0), Fraction(1, 2), Fraction(1), Fraction(3, 2), Fraction(2), Fraction(3), Fraction(4), Fraction(6)]


# ---------------------------------------------------------------------------------------------------------- the twin
def _exact_code(y):
    """e2m1 magnitude code of the exact y >= 0 (a Fraction): nearest grid point, ties to the even code (the even mantissa)."""
    if y >= 6:
        return 7
    best = min(range(8), key=lambda c: (abs(GRID[c] - y), c & 1))
    return best


def _exact_exp(amax):
    """The smallest integer e with amax <= 6 * 2^e (amax > 0, a Fraction), clamped to [-120, 120]."""
    e = -200
    while amax > 6 * Fraction(2) ** e:
        e += 1
    return max(-120, min(120, e))


def _bf16(x):
    return (tw.bf16_bits_from_f32(np.asarray(x, np.float32)).astype(np.uint32) << 16).view(np.float32)


def _rows(n=256, seed=7):
    g = np.random.default_rng(seed)
    x = g.standard_normal((n, 128)) * np.exp2(g.integers(-30, 30, (n, 4, 1))).repeat(32, axis=1).reshape(n, 128)
    return _bf16(x.astype(np.float32))


def test_twin_matches_exact_arithmetic():
    x = _rows(64)
    codes, sb = tw.quant_codes(x)
    for r in range(x.shape[0]):
        for b in range(4):
            blk = [Fraction(float(v)) for v in x[r, 32 * b:32 * b + 32]]
            e = _exact_exp(max(abs(v) for v in blk))
            assert sb[r, b] == e + 127
            for i, v in enumerate(blk):
                c = int(codes[r, 32 * b + i])
                assert (c & 7) == _exact_code(abs(v) / Fraction(2) ** e), (r, b, i)
                assert (c >> 3) == int(v < 0)
    val = tw.dequant_f64(codes, sb)
    for r in range(0, x.shape[0], 7):
        for d in range(128):
            c = int(codes[r, d])
            assert Fraction(float(val[r, d])) == (-1 if c & 8 else 1) * GRID[c & 7] * Fraction(2) ** (int(sb[r, d // 32]) - 127)


def test_every_tie_goes_to_the_even_mantissa():
    ties = {0.25: 0, 0.75: 2, 1.25: 2, 1.75: 4, 2.5: 4, 3.5: 6, 5.0: 6}
    for e in (-120, -14, 0, 3, 120):
        x = np.zeros((1, 128), np.float32)
        x[0, 0] = np.ldexp(np.float32(6), e)  # the block's amax: e_b = e
        for i, t in enumerate(ties):
            x[0, 1 + 2 * i] = np.ldexp(np.float32(t), e)
            x[0, 2 + 2 * i] = -np.ldexp(np.float32(t), e)
        codes, sb = tw.quant_codes(x)
        assert sb[0, 0] == e + 127 and codes[0, 0] == 7
        for i, (t, c) in enumerate(ties.items()):
            assert codes[0, 1 + 2 * i] == c and codes[0, 2 + 2 * i] == (c | 8), (e, t)
            # one float32 ulp to either side leaves the tie
            up, dn = np.nextafter(np.float32(t), np.float32(9)), np.nextafter(np.float32(t), np.float32(0))
            cu, _ = tw.quant_codes(np.r_[np.float32(6), up, dn, np.zeros(29, np.float32)][None])
            assert cu[0, 1] == _exact_code(Fraction(float(up))) and cu[0, 2] == _exact_code(Fraction(float(dn)))
            assert cu[0, 1] != cu[0, 2]


def test_block_maximum_on_an_exponent_boundary():
    """amax exactly 6 * 2^e keeps e (code 7, nothing saturates); one ulp above steps to e + 1 (code 5 = 3 * 2^(e + 1) after rounding)."""
    for e in (-119, -20, 0, 7, 119):
        top = np.ldexp(np.float32(6), e)
        x = np.zeros((2, 32), np.float32)
        x[0, 3], x[1, 3] = top, np.nextafter(top, np.float32(np.inf))
        codes, sb = tw.quant_codes(x)
        assert sb[0, 0] == e + 127 and codes[0, 3] == 7
        assert sb[1, 0] == e + 128 and codes[1, 3] == 5
        assert tw.dequant_f64(codes, sb)[0, 3] == float(top)
    # float32 values of 16-bit dtypes: the largest scaled magnitude is never above 6
    x = _rows(128, 3)
    codes, sb = tw.quant_codes(x)
    y = np.abs(x.astype(np.float64)).reshape(-1, 4, 32) * np.exp2(127.0 - sb)[..., None]
    assert y.max() <= 6.0 and np.all(y.max(axis=-1) > 3.0)


def test_zero_blocks_signed_zero_and_the_clamp_ends():
    x = np.zeros((1, 128), np.float32)
    x[0, 5] = -0.0
    x[0, 32:64] = np.float32(2.0 ** -140)  # below 6 * 2^-120: clamped to -120, codes 0
    x[0, 64] = np.float32(2.0 ** -120) * 3  # e = -121 -> clamped to -120: 3 * 2^-120 is code 5
    x[0, 96] = np.float32(3.0e38)  # bf16's top: e clamped at 120; 3e38 / 2^120 > 6 -> code 7
    x[0, 97] = -np.float32(2.0 ** 122)  # 4 * 2^120: code 6 under the clamped scale
    codes, sb = tw.quant_codes(x)
    assert list(sb[0]) == [7, 7, 7, 247]
    assert codes[0, 5] == 8 and np.all(np.delete(codes[0, :32], 5) == 0)
    assert np.all(codes[0, 32:64] == 0)
    assert codes[0, 64] == 5 and codes[0, 96] == 7 and codes[0, 97] == (6 | 8)
    bits = tw.dequant_bits(tw.pack(codes), sb, "bf16")
    assert bits[0, 5] == 0x8000 and bits[0, 0] == 0


def test_non_finite_block():
    x = np.ones((1, 128), np.float32)
    x[0, 40], x[0, 41], x[0, 42] = np.inf, -np.inf, np.nan
    x[0, 43] = 5.5
    codes, sb = tw.quant_codes(x)
    assert list(sb[0]) == [125, 0xFF, 125, 125]  # 1.0 <= 6 * 2^-2; the block's exponent comes from its finite values (5.5 -> 0)
    assert codes[0, 40] == 7 and codes[0, 41] == 15 and (codes[0, 42] & 7) == 0 and codes[0, 43] == 7
    for dt in ("bf16", "f16"):
        bits = tw.dequant_bits(tw.pack(codes), sb, dt)
        assert np.all(bits[0, 32:64] == tw.NAN_BITS[dt])
        assert np.all(bits[0, :32] == bits[0, 0]) and bits[0, 0] == (0x3F80 if dt == "bf16" else 0x3C00)
    # the NaN patterns are NaNs of their dtypes
    assert np.isnan(np.uint16(tw.NAN_BITS["f16"]).view(np.float16))
    assert np.isnan((np.uint32(tw.NAN_BITS["bf16"]) << 16).view(np.float32))


def test_f16_overflow_and_underflow_follow_one_rounding():
    img = np.full((1, 16), 0x17, np.uint8)  # codes 7 (6.0) and 1 (0.5)
    assert list(tw.dequant_bits(img, np.uint8([[127 + 13]]), "f16")[0, :2]) == [0x7A00, 0x6C00]  # 49152, 4096
    assert list(tw.dequant_bits(img, np.uint8([[127 + 14]]), "f16")[0, :2]) == [0x7C00, 0x7000]  # 98304 -> inf
    assert list(tw.dequant_bits(img, np.uint8([[127 - 24]]), "f16")[0, :2]) == [0x0006, 0x0000]  # 6 * 2^-24; 2^-25: the tie to 0
    assert list(tw.dequant_bits(img, np.uint8([[127 - 27]]), "f16")[0, :2]) == [0x0001, 0x0000]  # 1.5 * 2^-25 -> 2^-24
    torch_fp4 = getattr(torch, "float4_e2m1fn_x2", None)  # a second opinion on the grid, where this torch has the dtype
    if torch_fp4 is not None:
        assert torch.empty(1, dtype=torch.uint8).view(torch_fp4).element_size() == 1


def test_packing_is_low_nibble_first_and_words_are_little_end_first():
    codes = np.arange(16, dtype=np.uint8)[None].repeat(2, 0)
    img = tw.pack(codes)
    assert img.shape == (2, 8) and list(img[0]) == [0x10, 0x32, 0x54, 0x76, 0x98, 0xBA, 0xDC, 0xFE]
    assert np.array_equal(tw.unpack(img), codes)
    assert tw.scale_word(np.uint8([[1, 2, 3, 0xFF]]))[0] == 0xFF030201
    assert list(tw.scale_bytes(np.uint32([0xFF030201]))[0]) == [1, 2, 3, 0xFF]
    q = tw.qparams(np.uint8([[1, 2, 3, 4]]), np.uint8([[5, 6, 7, 8]]))
    assert list(q[0]) == [0x04030201, 0, 0x08070605, 0]


def test_blocks_are_independent_bit_for_bit():
    x = _rows(64, 5)
    codes, sb = tw.quant_codes(x)
    g = np.random.default_rng(9)
    for r in range(x.shape[0]):
        d = int(g.integers(0, 128))
        y = x[r:r + 1].copy()
        y[0, d] = _bf16(np.float32(y[0, d] * 300 + 1))
        c2, s2 = tw.quant_codes(y)
        b = d // 32
        other = np.ones(128, bool)
        other[32 * b:32 * b + 32] = False
        assert np.array_equal(c2[0, other], codes[r, other]) and np.array_equal(np.delete(s2[0], b), np.delete(sb[r], b))
        assert s2[0, b] != sb[r, b]  # its own block moved to the new range


def _rms(a):
    return float(np.sqrt(np.mean(np.square(np.asarray(a, np.float64)))))


def _errors(x):
    em = _rms(tw.round_trip_f64(x) - x)
    img, sc, mn = u4.quant_rows(x)
    return em, _rms(u4.dequant_f32(u4.unpack(img), sc, mn).astype(np.float64) - x)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_finer_than_uint4_on_outlier_rows_coarser_on_shifted_rows(seed):
    g = np.random.default_rng(seed)
    base = g.standard_normal((4096, 128)).astype(np.float32)
    out = base.copy()
    out[:, 77] *= 50
    em, eu = _errors(_bf16(out))
    print(f"one channel x50: mxfp4 {em:.4f} uint4 {eu:.4f} ratio {em / eu:.3f}")
    assert em < 0.7 * eu  # three of four blocks keep their own range (seen: 0.54 - 0.55)
    em, eu = _errors(_bf16(base + 3))
    print(f"rows shifted by +3: mxfp4 {em:.4f} uint4 {eu:.4f} ratio {em / eu:.3f}")
    assert em > 2.5 * eu  # no zero point: the codes are spent on [-6, 6] * 2^e around a mean of 3 (seen: 3.21 - 3.22)
    em, eu = _errors(_bf16(base))
    print(f"Gaussian rows: mxfp4 {em:.4f} uint4 {eu:.4f} ratio {em / eu:.3f}")
    em, eu = _errors(_bf16(base * np.exp(g.standard_normal((1, 128))).astype(np.float32)))
    print(f"per-channel log-normal spread: mxfp4 {em:.4f} uint4 {eu:.4f} ratio {em / eu:.3f}")


def test_round_trip_error_is_half_a_grid_step():
    x = _rows(256, 11)
    codes, sb = tw.quant_codes(x)
    val = tw.dequant_f64(codes, sb)
    sc = np.exp2(sb.astype(np.float64) - 127).repeat(32, axis=-1)
    assert np.all(np.abs(val - x) <= sc)  # the widest gap of the grid is 2 (4 .. 6): half of it
    small = np.abs(x) <= 2 * sc
    assert np.all(np.abs(val - x)[small] <= 0.25 * sc[small])
    assert np.array_equal(tw.round_trip_bits(x, "bf16"), tw.bf16_bits_from_f32(val.astype(np.float32)))


# ---------------------------------------------------------------------------------------------------------- the caches
def _kw(mode, bits, **extra):
    kw = dict(max_cache_length=64, max_seq_length=256, cache_bits=bits, global_tokens=4, recent_window=10, history_window_size=1,
              attn_thresholding=False, min_recovery_frac=0.9, hybrid_strategies=HYBRID,
              token_ids={"special": [[1], [2, 3]], "punctuation": [5, 6, 7]}, cache_quant_mode=mode)
    kw.update(extra)
    return kw


def _make(strategy, mode, bits=4, H=2, dtype=torch.bfloat16, head_dim=128, **extra):
    from cold_compress_amd.cache import get_cache_constructor

    cls, rk = get_cache_constructor(strategy)
    kw = _kw(mode, bits, **extra)
    keys = set(rk) | {"cache_quant_mode"} | ({"history_window_size"} & set(extra))
    return cls(1, H, head_dim, dtype, **{k: kw[k] for k in keys if k in kw})


SERVED = [("heavy_hitter", {}), ("heavy_hitter", {"history_window_size": 8}), ("recent_global", {}), ("full", {}), ("random", {}),
          ("hybrid", {})]


@pytest.mark.parametrize("strategy,extra", SERVED, ids=[s + ("_w8" if e else "") for s, e in SERVED])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_mxfp4_caches_are_the_uint4_caches(strategy, extra, dtype):
    from cold_compress_amd import _abi

    a = _make(strategy, "uint4", 4, dtype=dtype, **extra)
    b = _make(strategy, "mxfp4", 4, dtype=dtype, **extra)
    f8 = _make(strategy, "fused", 8, dtype=dtype, **extra)
    assert b.fused_quant and not b.quantize
    assert b.quant_format == _abi.CC_QUANT_MXFP4 == 0x304
    assert b._fused_quant_policy() == f8._fused_quant_policy() != 0
    ba, bb = dict(a.named_buffers()), dict(b.named_buffers())
    assert set(ba) == set(bb)
    for name in ba:
        assert ba[name].dtype == bb[name].dtype and ba[name].shape == bb[name].shape, name
    for name in ("k_cache_q", "v_cache_q"):
        assert bb[name].dtype == torch.uint8 and tuple(bb[name].shape) == (1, 2, 64, 64), name
    assert tuple(bb["kv_qparams"].shape) == (1, 2, 64, 4) and bb["kv_qparams"].dtype == torch.float32
    assert b.k_cache.numel() == 0 and b.k_cache.dtype == dtype
    assert b.memory_usage() == a.memory_usage()
    if strategy == "hybrid":  # (its statistics report the profiled heads' policies)
        b.cache_strategies = torch.zeros(2, dtype=torch.int64)
    stats = b.compute_statistics(torch.tensor(10))
    assert "working_cache_gb" not in stats and stats["cache_memory_gb"] == b.memory_usage()


def test_mxfp4_three_call_decode_path_refused():
    from cold_compress_amd._abi import ColdCompressError

    z = torch.zeros(1, 2, 1, 128, dtype=torch.bfloat16)
    for strategy, extra in SERVED:
        kv = _make(strategy, "mxfp4", **extra)
        if strategy == "hybrid":
            kv.cache_strategies = torch.zeros(2, dtype=torch.int64)
            with pytest.raises(ColdCompressError, match="mxfp4"):
                kv._decoding_update(torch.tensor([70]), z, z, input_ids=torch.tensor([[9]]))
        else:
            with pytest.raises(ColdCompressError, match="mxfp4"):
                kv._decoding_update(torch.tensor([70]), z, z)


def test_mxfp4_refusals():
    from cold_compress_amd._abi import ColdCompressError

    for bits in (8, 2):  # cache_bits=4 only
        for strategy, extra in SERVED:
            with pytest.raises(ColdCompressError, match="mxfp4"):
                _make(strategy, "mxfp4", bits, **extra)
    kv = _make("heavy_hitter", "mxfp4", None)  # no cache_bits: the mode has nothing to do
    assert not kv.fused_quant and kv.quant_format is None
    with pytest.raises(ColdCompressError, match="mxfp4"):  # l2 is not served
        _make("l2", "mxfp4")
    with pytest.raises(ColdCompressError, match="mxfp4"):  # a 16-bit model only
        _make("heavy_hitter", "mxfp4", dtype=torch.float32)
    with pytest.raises(ColdCompressError, match="mxfp4"):
        _make("hybrid", "mxfp4", dtype=torch.float32)
    with pytest.raises(ColdCompressError, match="mxfp4"):  # head_dim 128 only
        _make("recent_global", "mxfp4", head_dim=64)
    with pytest.raises(ColdCompressError, match="mxfp4"):
        _make("hybrid", "mxfp4", hybrid_strategies=HYBRID * 5)  # more policies than the step's table holds
    with pytest.raises(ColdCompressError, match="mxfp4"):  # the message of an unknown mode names this one
        _make("heavy_hitter", "mxfp6", 4)


def test_mxfp4_flag_parses():
    from cold_compress_amd.cache import add_extension_arguments

    ap = argparse.ArgumentParser()
    add_extension_arguments(ap)
    assert ap.parse_args(["--cache_quant_mode", "mxfp4"]).cache_quant_mode == "mxfp4"
    assert ap.parse_args([]).cache_quant_mode == "reference"
    with pytest.raises(SystemExit):
        ap.parse_args(["--cache_quant_mode", "mxfp6"])


def test_header_defines_the_format():
    from cold_compress_amd import _abi

    with open(os.path.join(ROOT, "include", "coldcompress.h")) as fh:
        header = fh.read()
    assert re.search(r"#define\s+CC_QUANT_MXFP4\s+\(0x300\s*\|\s*4\)", header), "CC_QUANT_MXFP4"
    assert _abi.CC_QUANT_MXFP4 == 0x300 | 4
    for pinned in ("0xffc0", "0xfe00"):  # the decode's NaN patterns are part of the contract
        assert pinned in header


def test_mxfp4_setup_caches_refuses_an_unserved_ratio():
    """7 query heads per kv head (Qwen2's ratio): refused where the query heads are known, naming the mode."""
    from cold_compress_amd import cache
    from cold_compress_amd._abi import ColdCompressError
    from cold_compress_amd.harness import ModelArgs, Transformer, setup_caches

    model = Transformer(ModelArgs(block_size=256, vocab_size=64, n_layer=1, n_head=7, n_local_heads=1, dim=896, intermediate_size=256))
    model = model.to(torch.bfloat16).eval()
    ap = argparse.ArgumentParser()
    cache.add_cache_arguments(ap)
    kw = vars(ap.parse_args([]))
    kw.update(cache_strategy=["heavy_hitter"], prompt_compression_strategy=["heavy_hitter"], max_cache_length=[64], global_tokens=4,
              recent_window=10, history_window_size=1, cache_bits=4, cache_quant_mode="mxfp4")
    with pytest.raises(ColdCompressError, match="mxfp4.*multiple of 4"):
        setup_caches(model, None, "cpu", 128, dict(kw))
