"""numpy twin of the FP8 (OCP e4m3fn) fused KV cache: cache_quant_mode="fp8" (include/coldcompress.h).

One power-of-two scale 2^e per (head, slot) row of K and of V:
  amax  = max |x| over the row's finite values;  amax = m * 2^k, m in [0.5, 1) (frexp)
  e     = k - 9 if m <= 0.875 else k - 8  (the smallest e with amax <= 448 * 2^e), clamped to [-120, 120]; 0 for amax == 0
  code  = e4m3_rne(f32(x) * 2^-e)  (never above 448: no saturation); non-finite x -> the e4m3 NaN with x's sign (0x7f | sign)
  value = dtype(f32(e4m3(code)) * 2^e)  (f32 product, then one round to nearest even into bf16 / f16; f16 overflow -> inf)
"""
import numpy as np

E4M3_MAX = 448.0
EXP_MIN, EXP_MAX = -120, 120


def e4m3_table():
    """float32 value of each of the 256 e4m3fn codes (0x7f / 0xff: NaN)."""
    c = np.arange(256)
    s = np.where(c >> 7, -1.0, 1.0)
    E, M = (c >> 3) & 15, c & 7
    mag = np.where(E == 0, M * 2.0 ** -9, (1.0 + M / 8.0) * np.exp2(E - 7.0))
    v = (s * mag).astype(np.float32)
    v[(E == 15) & (M == 7)] = np.nan
    return v


_TAB = e4m3_table()
_POS = _TAB[:127].astype(np.float64)  # codes 0x00 .. 0x7e: the non-negative finite values, increasing


def e4m3_rne(y):
    """Codes of float32 values |y| <= 448 (round to nearest, ties to even); non-finite -> 0x7f | sign."""
    y = np.asarray(y, np.float32)
    a = np.abs(y.astype(np.float64))
    fin = np.isfinite(a)
    a = np.where(fin, a, 0.0)
    assert np.all(a <= E4M3_MAX), "e4m3_rne: the row scale keeps every value within +-448"
    ex = np.floor(np.log2(np.maximum(a, 2.0 ** -6)))  # binade; the subnormals share the quantum of the first normal binade
    quantum = np.exp2(ex - 3)
    r = np.rint(a / quantum) * quantum  # exact: a power-of-two quantum, np.rint ties to even
    code = np.searchsorted(_POS, r).astype(np.int64)
    assert np.array_equal(_POS[code], r)
    sign = (np.signbit(y)).astype(np.int64) << 7
    code = np.where(fin, code, 0x7F) | sign
    return code.astype(np.uint8)


def row_exponent(x):
    """e of each row of x (last axis), per the rule above."""
    x = np.asarray(x, np.float32)
    a = np.where(np.isfinite(x), np.abs(x), np.float32(0)).max(axis=-1)
    m, k = np.frexp(a)
    e = np.where(m <= 0.875, k - 9, k - 8)
    e = np.clip(e, EXP_MIN, EXP_MAX)
    return np.where(a == 0, 0, e).astype(np.int32)


def quant_rows(x):
    """(codes uint8 like x, e int32 per row)."""
    x = np.asarray(x, np.float32)
    e = row_exponent(x)
    y = np.ldexp(x, -e[..., None]).astype(np.float32)
    return e4m3_rne(y), e


def bf16_bits_from_f32(f):
    """Round float32 to bf16 (nearest even), as uint16 bits; NaN -> 0x7fc0 with the sign."""
    f = np.ascontiguousarray(f, np.float32)
    u = f.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = np.isnan(f)
    return np.where(nan, (np.signbit(f).astype(np.uint16) << 15) | np.uint16(0x7FC0), r).astype(np.uint16)


def dequant_f32(codes, e):
    """f32(e4m3(code)) * 2^e, float32 (inf where the product overflows)."""
    v = _TAB[np.asarray(codes, np.uint8)]
    with np.errstate(over="ignore"):
        return np.ldexp(v, np.asarray(e, np.int32)[..., None] if np.ndim(e) == np.ndim(codes) - 1 else e).astype(np.float32)


def dequant_bits(codes, e, dtype):
    """uint16 bits of the decoded values in `dtype` ("bf16" or "f16")."""
    f = dequant_f32(codes, e)
    if dtype == "bf16":
        return bf16_bits_from_f32(f)
    with np.errstate(over="ignore"):
        return f.astype(np.float16).view(np.uint16)


def bits_equal(a, b, dtype):
    """Bit equality of 16-bit images, every NaN equal to every NaN."""
    a = np.asarray(a, np.uint16)
    b = np.asarray(b, np.uint16)
    if dtype == "bf16":
        na = ((a & 0x7F80) == 0x7F80) & ((a & 0x7F) != 0)
        nb = ((b & 0x7F80) == 0x7F80) & ((b & 0x7F) != 0)
    else:
        na = ((a & 0x7C00) == 0x7C00) & ((a & 0x3FF) != 0)
        nb = ((b & 0x7C00) == 0x7C00) & ((b & 0x3FF) != 0)
    return (na == nb) & (na | (a == b))
