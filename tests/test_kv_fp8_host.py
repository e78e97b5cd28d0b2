"""CPU tests of the FP8 fused KV cache (cache_bits=8, cache_quant_mode="fp8"): the numpy twin of its numerical contract
(tests/kv_fp8_twin.py) against torch.float8_e4m3fn, the row exponent at its edges, construction of every served policy with the
uint8 mode's buffers and memory, the refusals, the flag and the ABI constant.  The kernels are checked against the twin on the GPU:
tests/test_gpu_kv_fp8.py."""
import argparse
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_fp8_twin as tw  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HYBRID = [{"strategy": "special"}, {"strategy": "special_punc"}, {"strategy": "special_punc_heavy_hitter", "heavy_hitter_frac": 0.3},
          {"strategy": "special_punc_window", "recent_window": 0.3}, {"strategy": "full"}]


def _torch_codes(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


# ---------------------------------------------------------------------------------------------------------- the twin
def test_twin_decodes_all_codes_as_torch():
    ref = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float().numpy()
    got = tw.e4m3_table()
    assert np.array_equal(np.isnan(ref), np.isnan(got))
    assert np.isnan(got).sum() == 2 and np.isnan(got[0x7F]) and np.isnan(got[0xFF])  # e4m3fn: no infinities, NaN = S.1111.111
    fin = ~np.isnan(ref)
    assert np.array_equal(ref[fin].view(np.uint32), got[fin].view(np.uint32))  # bit for bit, the sign of zero included
    assert np.nanmax(got) == 448.0 and got[1] == 2.0 ** -9


def test_twin_encodes_as_torch():
    rng = np.random.default_rng(7)
    n = 100_000
    x = (rng.standard_normal(n) * np.exp2(rng.integers(-12, 8, n))).astype(np.float32)
    x = np.clip(x, -448, 448)
    pos = tw.e4m3_table()[:127].astype(np.float64)
    mids = ((pos[1:] + pos[:-1]) / 2).astype(np.float32)  # every tie between neighbouring codes (exact in float32)
    assert np.array_equal(mids.astype(np.float64), (pos[1:] + pos[:-1]) / 2)
    x = np.concatenate([x, mids, -mids, pos.astype(np.float32), -pos.astype(np.float32), np.float32([0.0, -0.0, 1e-30, -1e-30])])
    assert np.array_equal(tw.e4m3_rne(x), _torch_codes(x))


def test_twin_non_finite_encode_to_signed_nan():
    x = np.float32([np.inf, -np.inf, np.nan, -np.nan])
    assert list(tw.e4m3_rne(x)) == [0x7F, 0xFF, 0x7F, 0xFF]
    # a row with one NaN: the other values keep the scale of the finite maximum
    row = np.float32([1.0, -3.0, np.nan, 0.5])
    codes, e = tw.quant_rows(row[None])
    assert e[0] == tw.row_exponent(np.float32([[1.0, -3.0, 0.5]]))[0]
    assert codes[0, 2] == 0x7F and np.array_equal(codes[0, [0, 1, 3]], tw.quant_rows(np.float32([[1.0, -3.0, 0.5]]))[0][0])


@pytest.mark.parametrize("amax,e", [(448.0, 0), (449.0, 1), (224.0, -1), (0.0, 0), (896.0, 1), (897.0, 2), (1.0, -8), (0.875, -9),
                                    (0.8751, -8), (3.3895313892515355e38, 120), (65504.0, 8), (2.0 ** -133, -120),
                                    (2.0 ** -24, -32), (6.103515625e-05, -22)])
def test_row_exponent_edges(amax, e):
    row = np.float32([[amax, -amax / 2, 0.0]])
    assert tw.row_exponent(row)[0] == e
    # the rule is the smallest e with amax <= 448 * 2^e (inside the clamp)
    if amax > 0 and -120 < e < 120:
        assert np.float64(np.float32(amax)) <= 448.0 * 2.0 ** e and np.float64(np.float32(amax)) > 448.0 * 2.0 ** (e - 1)
    codes, ee = tw.quant_rows(row)
    assert tw._TAB[codes].max() <= 448.0  # never saturates


def test_row_exponent_sign_and_clamp():
    assert tw.row_exponent(np.float32([[-448.0, 1.0]]))[0] == 0
    assert tw.row_exponent(np.float32([[1e-40, 0.0]]))[0] == -120  # f32 subnormal: clamped
    assert tw.row_exponent(np.float32([[np.inf, 2.0]]))[0] == tw.row_exponent(np.float32([[2.0]]))[0]


def test_round_trip_bf16_is_exact_and_f16_overflow_defined():
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((16, 128)) * 3).astype(np.float32)
    codes, e = tw.quant_rows(x)
    f = tw.dequant_f32(codes, e)
    bits = tw.dequant_bits(codes, e, "bf16")
    assert np.array_equal(tw.bf16_bits_from_f32(f), bits)
    assert np.array_equal(bits.astype(np.uint32) << 16, f.view(np.uint32))  # exact in bf16: no rounding happened
    # f16: inf from 65520 up (nearest even), as numpy's float32 -> float16
    big = tw.dequant_bits(np.uint8([0x7E, 0x7E]), np.int32(8), "f16")  # 448 * 256 = 114688
    assert np.all(big == 0x7C00)
    assert tw.dequant_bits(np.uint8([0x77]), np.int32(0), "f16")[0] == np.float16(240.0).view(np.uint16)


def test_fp8_is_finer_than_uint8_on_outlier_rows():
    """The property the mode exists for: one outlier channel coarsens a uint8 row, not an e4m3 row."""
    rng = np.random.default_rng(11)
    x = rng.standard_normal((64, 128)).astype(np.float32)
    x[:, 5] *= 50
    codes, e = tw.quant_rows(x)
    fp8 = tw.dequant_f32(codes, e)
    mn, mx = x.min(1, keepdims=True), x.max(1, keepdims=True)
    sc = np.maximum(mx - mn, 1e-6) / 255
    u8 = np.clip(np.rint((x - mn) / sc), 0, 255) * sc + mn
    rest = np.ones(128, bool)
    rest[5] = False
    rms = lambda a: float(np.sqrt(np.mean((a[:, rest] - x[:, rest]) ** 2)))  # noqa: E731
    assert rms(fp8) < rms(u8)


# ---------------------------------------------------------------------------------------------------------- the caches
def _kw(mode, **extra):
    kw = dict(max_cache_length=64, max_seq_length=256, cache_bits=8, global_tokens=4, recent_window=10, history_window_size=1,
              attn_thresholding=False, min_recovery_frac=0.9, hybrid_strategies=HYBRID,
              token_ids={"special": [[1], [2, 3]], "punctuation": [5, 6, 7]}, cache_quant_mode=mode)
    kw.update(extra)
    return kw


def _make(strategy, mode, H=2, dtype=torch.bfloat16, head_dim=128, **extra):
    from cold_compress_amd.cache import get_cache_constructor

    cls, rk = get_cache_constructor(strategy)
    kw = _kw(mode, **extra)
    keys = set(rk) | {"cache_quant_mode"} | ({"history_window_size"} & set(extra))
    return cls(1, H, head_dim, dtype, **{k: kw[k] for k in keys if k in kw})


SERVED = [("heavy_hitter", {}), ("heavy_hitter", {"history_window_size": 8}), ("recent_global", {}), ("full", {}), ("random", {}),
          ("hybrid", {})]


@pytest.mark.parametrize("strategy,extra", SERVED, ids=[s + ("_w8" if e else "") for s, e in SERVED])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_fp8_caches_match_the_uint8_buffers_and_memory(strategy, extra, dtype):
    from cold_compress_amd import _abi

    a = _make(strategy, "fused", dtype=dtype, **extra)
    b = _make(strategy, "fp8", dtype=dtype, **extra)
    assert b.fused_quant and not b.quantize
    assert a.quant_format == 8 and b.quant_format == _abi.CC_QUANT_FP8_E4M3 == 0x108
    assert b._fused_quant_policy() == a._fused_quant_policy() != 0
    ba, bb = dict(a.named_buffers()), dict(b.named_buffers())
    assert set(ba) == set(bb)
    for name in ba:
        assert ba[name].dtype == bb[name].dtype and ba[name].shape == bb[name].shape, name
    assert bb["k_cache_q"].dtype == torch.uint8 and tuple(bb["k_cache_q"].shape) == (1, 2, 64, 128)
    assert tuple(bb["kv_qparams"].shape) == (1, 2, 64, 4) and bb["kv_qparams"].dtype == torch.float32
    assert b.k_cache.numel() == 0 and b.k_cache.dtype == dtype
    assert b.memory_usage() == a.memory_usage()
    if strategy == "hybrid":  # (its statistics report the profiled heads' policies)
        b.cache_strategies = torch.zeros(2, dtype=torch.int64)
    stats = b.compute_statistics(torch.tensor(10))
    assert "working_cache_gb" not in stats and stats["cache_memory_gb"] == b.memory_usage()


def test_fp8_three_call_decode_path_refused():
    from cold_compress_amd._abi import ColdCompressError

    z = torch.zeros(1, 2, 1, 128, dtype=torch.bfloat16)
    for strategy, extra in SERVED:
        kv = _make(strategy, "fp8", **extra)
        if strategy == "hybrid":
            kv.cache_strategies = torch.zeros(2, dtype=torch.int64)
            with pytest.raises(ColdCompressError, match="fp8"):
                kv._decoding_update(torch.tensor([70]), z, z, input_ids=torch.tensor([[9]]))
        else:
            with pytest.raises(ColdCompressError, match="fp8"):
                kv._decoding_update(torch.tensor([70]), z, z)


def test_fp8_refusals():
    from cold_compress_amd._abi import ColdCompressError

    with pytest.raises(ColdCompressError, match="fp8"):  # l2 is not served
        _make("l2", "fp8")
    for bits in (4, 2):
        for strategy, extra in SERVED:
            with pytest.raises(ColdCompressError, match="fp8"):
                _make(strategy, "fp8", cache_bits=bits, **extra)
    with pytest.raises(ColdCompressError, match="fp8"):  # a 16-bit model only
        _make("heavy_hitter", "fp8", dtype=torch.float32)
    with pytest.raises(ColdCompressError, match="fp8"):
        _make("hybrid", "fp8", dtype=torch.float32)
    with pytest.raises(ColdCompressError, match="fp8"):  # head_dim 128 only
        _make("recent_global", "fp8", head_dim=64)
    with pytest.raises(ColdCompressError, match="fp8"):
        _make("hybrid", "fp8", hybrid_strategies=HYBRID * 5)  # more policies than the step's table holds
    with pytest.raises(ColdCompressError):
        _make("heavy_hitter", "e5m2")
    kv = _make("heavy_hitter", "fp8", cache_bits=None)  # no cache_bits: the mode has nothing to do, as "fused"
    assert not kv.fused_quant and kv.quant_format is None


def test_fp8_flag_parses():
    from cold_compress_amd.cache import add_extension_arguments

    ap = argparse.ArgumentParser()
    add_extension_arguments(ap)
    assert ap.parse_args(["--cache_quant_mode", "fp8"]).cache_quant_mode == "fp8"
    assert ap.parse_args([]).cache_quant_mode == "reference"
    with pytest.raises(SystemExit):
        ap.parse_args(["--cache_quant_mode", "e5m2"])


def test_header_defines_the_format():
    from cold_compress_amd import _abi

    with open(os.path.join(ROOT, "include", "coldcompress.h")) as fh:
        header = fh.read()
    m = re.search(r"#define\s+CC_QUANT_FP8_E4M3\s+\(0x100\s*\|\s*8\)", header)
    assert m, "CC_QUANT_FP8_E4M3"
    assert _abi.CC_QUANT_FP8_E4M3 == 0x100 | 8
