"""CPU tests of the 4-bit fused KV cache (cache_bits=4, cache_quant_mode="uint4"): the numpy twin of its numerical contract
(tests/kv_uint4_twin.py) against an independent torch formulation and exact fractions, construction of every served policy with
half-size images and the uint8 mode's row parameters, memory, the refusals, the flag and the ABI constant.  The kernels are checked
against the twin on the GPU: tests/test_gpu_kv_uint4.py."""
import argparse
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_uint4_twin as tw  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HYBRID = [{"strategy": "special"}, {"strategy": "special_punc"}, {"strategy": "special_punc_heavy_hitter", "heavy_hitter_frac": 0.3},
          {"strategy": "special_punc_window", "recent_window": 0.3}, {"strategy": "full"}]


# ---------------------------------------------------------------------------------------------------------- the twin
def _torch_contract(x):
    """The contract in torch (float32 tensor ops; the fma emulated in float64): (images, scale, mn, float32 values)."""
    x = torch.from_numpy(np.ascontiguousarray(x, np.float32))
    mn, mx = x.min(dim=-1).values, x.max(dim=-1).values
    rng = torch.clamp_min(mx - mn, torch.tensor(1e-6, dtype=torch.float32))
    scale, inv = rng / 15.0, 15.0 / rng
    q = torch.round((x - mn[:, None]) * inv[:, None]).clamp(0, 15).to(torch.uint8)  # torch.round: half to even
    img = q[:, 0::2] | (q[:, 1::2] << 4)
    val = (q.double() * scale.double()[:, None] + mn.double()[:, None]).float()  # may round twice: compared where it cannot
    return img.numpy(), scale.numpy(), mn.numpy(), val.numpy()


def _rows(n=512, seed=7):
    g = np.random.default_rng(seed)
    x = g.standard_normal((n, 128)) * np.exp2(g.integers(-10, 10, (n, 1))) + g.standard_normal((n, 1)) * 4
    return x.astype(np.float32)


def test_twin_matches_torch():
    x = _rows()
    img, scale, mn = tw.quant_rows(x)
    t_img, t_scale, t_mn, t_val = _torch_contract(x)
    assert np.array_equal(img, t_img)
    assert np.array_equal(scale.view(np.uint32), t_scale.view(np.uint32)) and np.array_equal(mn.view(np.uint32), t_mn.view(np.uint32))
    val = tw.dequant_f32(tw.unpack(img), scale, mn)
    a = tw.unpack(img).astype(np.float64) * scale.astype(np.float64)[:, None]
    b = np.broadcast_to(mn.astype(np.float64)[:, None], a.shape)
    s = a + b
    bb = s - a
    exact = ((a - (s - bb)) + (b - bb)) == 0  # where float64 held the sum, torch's conversion is the one rounding
    assert exact.mean() > 0.5
    assert np.array_equal(val[exact].view(np.uint32), t_val[exact].view(np.uint32))
    ulp = np.abs(val.view(np.int32).astype(np.int64) - t_val.view(np.int32).astype(np.int64))
    assert ulp.max() <= 1  # elsewhere at most the double rounding torch's float64 path may add


def test_twin_fma_is_one_rounding():
    """dequant_f32 is the float32 nearest to q * scale + mn, ties to even, on sums chosen to land on float32 midpoints."""
    g = np.random.default_rng(3)
    scale = (g.random(400) * 2.0 ** g.integers(-20, 4, 400)).astype(np.float32)
    mn = (g.standard_normal(400) * 2.0 ** g.integers(-4, 12, 400)).astype(np.float32)
    codes = g.integers(0, 16, (400, 16)).astype(np.uint8)
    got = tw.dequant_f32(codes, scale, mn)
    for i in range(400):
        for j in range(16):
            ex = Fraction(int(codes[i, j])) * Fraction(float(scale[i])) + Fraction(float(mn[i]))
            r = got[i, j]
            lo, hi = np.nextafter(r, np.float32(-np.inf)), np.nextafter(r, np.float32(np.inf))
            d = abs(ex - Fraction(float(r)))
            assert d <= abs(ex - Fraction(float(lo))) and d <= abs(ex - Fraction(float(hi)))
            if d == abs(ex - Fraction(float(lo))) or d == abs(ex - Fraction(float(hi))):
                assert int(r.view(np.uint32)) & 1 == 0  # a tie went to the even neighbour
    # q * scale on a float32 midpoint and a tiny minimum: float64 drops the minimum, a plain float64 -> float32 conversion then
    # breaks the false tie to even (3 + 2^-21); the exact sum lies below the midpoint (3 + 2^-22)
    q, sc, m = np.uint8([[3]]), np.float32([1.0 + 2.0 ** -23]), np.float32([-(2.0 ** -80)])
    assert np.float32(3.0 * (1.0 + 2.0 ** -23) - 2.0 ** -80) == np.float32(3.0 + 2.0 ** -21)
    assert tw.dequant_f32(q, sc, m)[0, 0] == np.float32(3.0 + 2.0 ** -22)


def test_packing_is_low_nibble_first():
    codes = np.arange(16, dtype=np.uint8)[None].repeat(2, 0)
    img = tw.pack(codes)
    assert img.shape == (2, 8) and list(img[0]) == [0x10, 0x32, 0x54, 0x76, 0x98, 0xBA, 0xDC, 0xFE]
    assert np.array_equal(tw.unpack(img), codes)


def test_edge_rows():
    x = np.zeros((4, 128), np.float32)
    x[0] = 3.25  # a constant row: range = 1e-6, every code 0, value = mn
    x[1] = 1.0
    x[1, 7] = 1.0 + 2.0 ** -23  # a range below 1e-6
    x[2] = np.linspace(-65504, 65504, 128)
    x[3] = np.float32(0.5)
    x[3, 100] = 40.0  # one outlier channel
    img, scale, mn = tw.quant_rows(x)
    codes = tw.unpack(img)
    assert np.all(codes[0] == 0) and scale[0] == np.float32(np.float32(1e-6) / np.float32(15))
    assert np.all(tw.dequant_f32(codes, scale, mn)[0] == np.float32(3.25))
    assert codes[1, 7] == 2 and np.all(np.delete(codes[1], 7) == 0)  # 2^-23 * (15 / 1e-6) = 1.79: the 1e-6 floor, not the range
    assert codes[2, 0] == 0 and codes[2, -1] == 15 and np.all(np.diff(codes[2].astype(int)) >= 0)
    assert codes[3, 100] == 15 and np.all(np.delete(codes[3], 100) == 0)
    bits = tw.round_trip_bits(x, "f16")
    assert bits[2, -1] == np.float16(65504).view(np.uint16) and bits[2, 0] == np.float16(-65504).view(np.uint16)


def test_round_trip_error_is_half_a_step():
    x = _rows(256, 11)
    img, scale, mn = tw.quant_rows(x)
    val = tw.dequant_f32(tw.unpack(img), scale, mn)
    assert np.all(np.abs(val - x) <= scale[:, None] * (0.5 + 1e-4) + np.abs(x) * 2.0 ** -22)


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
def test_uint4_caches_halve_the_uint8_images(strategy, extra, dtype):
    from cold_compress_amd import _abi

    a = _make(strategy, "fused", 8, dtype=dtype, **extra)
    b = _make(strategy, "uint4", 4, dtype=dtype, **extra)
    assert b.fused_quant and not b.quantize
    assert b.quant_format == _abi.CC_QUANT_UINT4 == 0x204
    assert b._fused_quant_policy() == a._fused_quant_policy() != 0
    ba, bb = dict(a.named_buffers()), dict(b.named_buffers())
    assert set(ba) == set(bb)
    for name in ba:
        if name not in ("k_cache_q", "v_cache_q"):
            assert ba[name].dtype == bb[name].dtype and ba[name].shape == bb[name].shape, name
    for name in ("k_cache_q", "v_cache_q"):
        assert bb[name].dtype == torch.uint8 and tuple(bb[name].shape) == (1, 2, 64, 64), name
    assert tuple(bb["kv_qparams"].shape) == (1, 2, 64, 4) and bb["kv_qparams"].dtype == torch.float32
    assert b.k_cache.numel() == 0 and b.k_cache.dtype == dtype
    img8 = sum(ba[n].numel() * ba[n].element_size() for n in ("k_cache_q", "v_cache_q"))
    assert b.memory_usage() == (a.memory_usage() * 1024 ** 3 - img8 // 2) / 1024 ** 3
    if strategy == "hybrid":  # (its statistics report the profiled heads' policies)
        b.cache_strategies = torch.zeros(2, dtype=torch.int64)
    stats = b.compute_statistics(torch.tensor(10))
    assert "working_cache_gb" not in stats and stats["cache_memory_gb"] == b.memory_usage()


def test_uint4_three_call_decode_path_refused():
    from cold_compress_amd._abi import ColdCompressError

    z = torch.zeros(1, 2, 1, 128, dtype=torch.bfloat16)
    for strategy, extra in SERVED:
        kv = _make(strategy, "uint4", **extra)
        if strategy == "hybrid":
            kv.cache_strategies = torch.zeros(2, dtype=torch.int64)
            with pytest.raises(ColdCompressError, match="uint4"):
                kv._decoding_update(torch.tensor([70]), z, z, input_ids=torch.tensor([[9]]))
        else:
            with pytest.raises(ColdCompressError, match="uint4"):
                kv._decoding_update(torch.tensor([70]), z, z)


def test_uint4_refusals():
    from cold_compress_amd._abi import ColdCompressError

    for bits in (8, 2):  # cache_bits=4 only, as "fused" takes cache_bits=8 only
        for strategy, extra in SERVED:
            with pytest.raises(ColdCompressError, match="uint4"):
                _make(strategy, "uint4", bits, **extra)
            if bits == 2:
                with pytest.raises(ColdCompressError, match="fused"):
                    _make(strategy, "fused", bits, **extra)
    for mode in ("uint4", "fused"):  # no cache_bits: the mode has nothing to do
        kv = _make("heavy_hitter", mode, None)
        assert not kv.fused_quant and kv.quant_format is None
    with pytest.raises(ColdCompressError, match="uint4"):  # l2 is not served
        _make("l2", "uint4")
    with pytest.raises(ColdCompressError, match="uint4"):  # a 16-bit model only
        _make("heavy_hitter", "uint4", dtype=torch.float32)
    with pytest.raises(ColdCompressError, match="uint4"):
        _make("hybrid", "uint4", dtype=torch.float32)
    with pytest.raises(ColdCompressError, match="uint4"):  # head_dim 128 only
        _make("recent_global", "uint4", head_dim=64)
    with pytest.raises(ColdCompressError, match="uint4"):
        _make("hybrid", "uint4", hybrid_strategies=HYBRID * 5)  # more policies than the step's table holds
    with pytest.raises(ColdCompressError):
        _make("heavy_hitter", "uint2", 2)


def test_uint4_flag_parses():
    from cold_compress_amd.cache import add_extension_arguments

    ap = argparse.ArgumentParser()
    add_extension_arguments(ap)
    assert ap.parse_args(["--cache_quant_mode", "uint4"]).cache_quant_mode == "uint4"
    assert ap.parse_args([]).cache_quant_mode == "reference"
    with pytest.raises(SystemExit):
        ap.parse_args(["--cache_quant_mode", "uint2"])


def test_header_defines_the_format():
    from cold_compress_amd import _abi

    with open(os.path.join(ROOT, "include", "coldcompress.h")) as fh:
        header = fh.read()
    assert re.search(r"#define\s+CC_QUANT_UINT4\s+\(0x200\s*\|\s*4\)", header), "CC_QUANT_UINT4"
    assert _abi.CC_QUANT_UINT4 == 0x200 | 4
