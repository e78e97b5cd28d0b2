"""numpy twin of the 4-bit fused KV cache: cache_quant_mode="uint4", cache_bits=4 (include/coldcompress.h).

The uint8 grid with 15 steps, one (scale, min) pair per (head, slot) row of K and of V:
  mn, mx = min / max over the row;  range = max(mx - mn, 1e-6f);  scale = range / 15.f
  q[d]   = clamp(rintf((x[d] - mn) * (15.f / range)), 0, 15)   (IEEE fp32 ops, round-half-even, no contraction)
  value  = T(fmaf((float)q[d], scale, mn))                     (one fp32 rounding of the exact q * scale + mn, then one into T)
  byte j of a row's image = q[2j] | q[2j + 1] << 4             (low nibble first)

numpy has no fma: q * scale is exact in float64 (4 + 24 significant bits), q * scale + mn in float64 is exact up to a TwoSum error
term, and where that term is non-zero the two float32 neighbours of the float64 sum are compared with the exact sum in fractions.
"""
from fractions import Fraction

import numpy as np

LEVELS = 15


def row_params(x, levels=LEVELS):
    """(scale, mn, inv) float32 per row of x (last axis): the contract's row grid.  levels: 15 (this format) or 255 (the uint8
    grid of cache_quant_mode="fused": the same arithmetic, one code per byte; tests/kv_quant_twin.py)."""
    x = np.asarray(x, np.float32)
    mn, mx = x.min(axis=-1), x.max(axis=-1)
    rng = np.maximum(np.float32(mx - mn), np.float32(1e-6)).astype(np.float32)
    with np.errstate(over="ignore", divide="ignore"):
        scale = (rng / np.float32(levels)).astype(np.float32)
        inv = (np.float32(levels) / rng).astype(np.float32)
    return scale, mn.astype(np.float32), inv


def quant_codes(x, levels=LEVELS):
    """(codes uint8 in [0, levels] like x, scale [rows], mn [rows])."""
    x = np.asarray(x, np.float32)
    scale, mn, inv = row_params(x, levels)
    t = ((x - mn[..., None]).astype(np.float32) * inv[..., None]).astype(np.float32)
    q = np.clip(np.rint(t), 0, levels)
    return q.astype(np.uint8), scale, mn


def pack(codes):
    """[..., D] codes -> [..., D / 2] bytes, byte j = q[2j] | q[2j + 1] << 4."""
    codes = np.asarray(codes, np.uint8)
    assert codes.shape[-1] % 2 == 0
    return (codes[..., 0::2] | (codes[..., 1::2] << 4)).astype(np.uint8)


def unpack(img):
    """[..., D / 2] bytes -> [..., D] codes."""
    img = np.asarray(img, np.uint8)
    out = np.empty(img.shape[:-1] + (2 * img.shape[-1],), np.uint8)
    out[..., 0::2] = img & 15
    out[..., 1::2] = img >> 4
    return out


def quant_rows(x):
    """Rows [..., D] -> (images [..., D / 2] uint8, scale, mn): what cc_kv_quant_rows writes."""
    q, scale, mn = quant_codes(x)
    return pack(q), scale, mn


def _f32_nearest(s, err, a, b):
    """float32 nearest to the exact a + b (float64 s = fl(a + b), err = the TwoSum error; ties to even)."""
    r = s.astype(np.float32)
    for i in np.flatnonzero(err != 0):
        ex = Fraction(float(a.flat[i])) + Fraction(float(b.flat[i]))
        r0 = r.flat[i]
        lo = np.nextafter(r0, np.float32(-np.inf)) if Fraction(float(r0)) > ex else r0
        hi = np.nextafter(lo, np.float32(np.inf))
        dlo, dhi = ex - Fraction(float(lo)), Fraction(float(hi)) - ex
        if dlo < dhi:
            r.flat[i] = lo
        elif dhi < dlo:
            r.flat[i] = hi
        else:
            r.flat[i] = lo if (int(np.float32(lo).view(np.uint32)) & 1) == 0 else hi
    return r


def dequant_f32(codes, scale, mn):
    """fmaf(q, scale, mn) in float32, exactly (one rounding)."""
    a = np.asarray(codes, np.float64) * np.asarray(scale, np.float64)[..., None]  # exact
    b = np.broadcast_to(np.asarray(mn, np.float64)[..., None], a.shape)
    s = a + b
    bb = s - a
    err = (a - (s - bb)) + (b - bb)  # TwoSum: a + b = s + err exactly
    return _f32_nearest(s, err, a, b)


def bf16_bits_from_f32(f):
    """float32 -> bf16 bits, round to nearest even (finite inputs)."""
    u = np.asarray(f, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def to_bits(f, dt):
    """float32 values -> 16-bit patterns of dt ('bf16' or 'f16'), one round to nearest even."""
    if dt == "bf16":
        return bf16_bits_from_f32(f)
    return np.asarray(f, np.float32).astype(np.float16).view(np.uint16)


def dequant_bits(img, scale, mn, dt):
    """Images [..., D / 2] + row params -> the model-dtype bit patterns [..., D] (what the decode kernels see)."""
    return to_bits(dequant_f32(unpack(img), scale, mn), dt)


def round_trip_bits(x, dt):
    """The contract's round trip of rows x (float32 values of a 16-bit dtype) -> dt bit patterns."""
    img, scale, mn = quant_rows(x)
    return dequant_bits(img, scale, mn, dt)
