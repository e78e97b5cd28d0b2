"""numpy twin of the MXFP4 fused KV cache: cache_quant_mode="mxfp4", cache_bits=4 (include/coldcompress.h).

A row's D values are blocks of 32 consecutive channels, each with its own power-of-two scale, stored as an e8m0 byte:
  amax_b = max |x| over the block's finite values;  e_b = the smallest integer with amax_b <= 6 * 2^e_b, clamped to [-120, 120];
           -120 for an all-zero block;  scale byte = e_b + 127, or 0xff when the block holds a non-finite value
  code   = sign << 3 | e2m1 magnitude of |x * 2^-e_b| on {0, 0.5, 1, 1.5, 2, 3, 4, 6}, round to nearest, ties to the even mantissa;
           above 6 (clamped e_b, +-inf): 6;  NaN: 0 under its sign;  -0 keeps its sign
  value  = T(e2m1(code) * 2^e_b), one rounding;  every element of a block with scale byte 0xff: the conversion's NaN
  byte j of a row's image = code[2j] | code[2j + 1] << 4   (low nibble first)
  qparams word 0 = K's scale bytes (byte b = block b), word 2 = V's, words 1 and 3 zero: bit patterns in float32 storage

x * 2^-e_b is formed in float64 here (exact); where the float32 product of the kernels would round (a float32 subnormal) or
overflow, it is far below 0.25 or above 6 and the code is the same.
"""
import numpy as np

BLOCK = 32
E2M1 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
NAN_BITS = {"bf16": 0xFFC0, "f16": 0xFE00}  # what v_cvt_scalef32_pk_{bf16,f16}_fp4 return under the scale byte 0xff


def block_exp(amax):
    """e_b per block from its float32 amax (finite, >= 0)."""
    amax = np.asarray(amax, np.float32)
    m, k = np.frexp(amax)  # amax = m * 2^k, m in [0.5, 1)
    e = np.where(m <= np.float32(0.75), k - 3, k - 2)
    e = np.clip(e, -120, 120)
    return np.where(amax > 0, e, -120).astype(np.int32)


def magnitude_code(y):
    """e2m1 magnitude code 0..7 of y >= 0: nearest, ties to the even mantissa (the even codes); NaN -> 0."""
    y = np.asarray(y, np.float64)
    with np.errstate(invalid="ignore"):
        return ((y > 0.25).astype(np.uint8) + (y >= 0.75) + (y > 1.25) + (y >= 1.75) + (y > 2.5) + (y >= 3.5) + (y > 5.0)).astype(np.uint8)


def quant_codes(x):
    """Rows [..., D] (float32 values of a 16-bit dtype) -> (codes uint8 [..., D] in [0, 15], scale bytes uint8 [..., D / 32])."""
    x = np.asarray(x, np.float32)
    assert x.shape[-1] % BLOCK == 0
    xb = x.reshape(x.shape[:-1] + (x.shape[-1] // BLOCK, BLOCK))
    fin = np.isfinite(xb)
    amax = np.where(fin, np.abs(xb), np.float32(0)).max(axis=-1).astype(np.float32)
    e = block_exp(amax)
    with np.errstate(invalid="ignore", over="ignore"):
        y = np.abs(xb.astype(np.float64)) * np.exp2(-e.astype(np.float64))[..., None]
    codes = magnitude_code(y) | (np.signbit(xb).astype(np.uint8) << 3)
    sb = np.where(fin.all(axis=-1), e + 127, 0xFF).astype(np.uint8)
    return codes.reshape(x.shape).astype(np.uint8), sb


def pack(codes):
    """[..., D] codes -> [..., D / 2] bytes, byte j = code[2j] | code[2j + 1] << 4."""
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


def scale_word(sb):
    """Scale bytes [..., nb <= 4] -> the row's qparams word (uint32; byte b = block b)."""
    sb = np.asarray(sb, np.uint8).astype(np.uint32)
    w = np.zeros(sb.shape[:-1], np.uint32)
    for b in range(sb.shape[-1]):
        w |= sb[..., b] << np.uint32(8 * b)
    return w


def scale_bytes(word, nb=4):
    """The inverse of scale_word."""
    word = np.asarray(word, np.uint32)
    return np.stack([(word >> np.uint32(8 * b)) & np.uint32(0xFF) for b in range(nb)], axis=-1).astype(np.uint8)


def qparams(k_sb, v_sb):
    """[..., 4] uint32 words of a row: (K word, 0, V word, 0) — what kv_qparams holds, viewed as int32 / uint32."""
    kw, vw = scale_word(k_sb), scale_word(v_sb)
    z = np.zeros_like(kw)
    return np.stack([kw, z, vw, z], axis=-1)


def quant_rows(x):
    """Rows [..., D] -> (images [..., D / 2] uint8, scale bytes [..., D / 32] uint8): what cc_kv_quant_rows writes."""
    codes, sb = quant_codes(x)
    return pack(codes), sb


def dequant_f64(codes, sb):
    """The exact value e2m1(code) * 2^(sb - 127) in float64 (NaN where sb == 0xff)."""
    codes = np.asarray(codes, np.uint8)
    sb = np.asarray(sb, np.uint8)
    mag = E2M1[codes & 7] * np.where(codes & 8, -1.0, 1.0)
    sc = np.exp2(sb.astype(np.float64) - 127.0)
    sc = np.repeat(sc, BLOCK, axis=-1)
    bad = np.repeat(sb == 0xFF, BLOCK, axis=-1)
    return np.where(bad, np.nan, mag * sc)


def bf16_bits_from_f32(f):
    """float32 -> bf16 bits, round to nearest even (finite inputs)."""
    u = np.asarray(f, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def dequant_bits(img, sb, dt):
    """Images [..., D / 2] + scale bytes [..., D / 32] -> the model-dtype bit patterns [..., D] (what the decode kernels see).
    bf16: exact for scale bytes 7 .. 247 (every e_b in range).  f16: one round to nearest even of the exact product — +-inf from
    65520 up, subnormals rounded, +-0 below; that is what the conversion instruction returns (tests/test_gpu_kv_mxfp4.py)."""
    v = dequant_f64(unpack(img), sb)
    bad = np.isnan(v)
    v = np.where(bad, 0.0, v)
    if dt == "bf16":
        with np.errstate(over="ignore"):  # (scale bytes past 247, outside the contract: inf, as the instruction)
            bits = bf16_bits_from_f32(v.astype(np.float32))  # (the product is a float32 value: 3 significant bits)
    else:
        with np.errstate(over="ignore"):
            bits = v.astype(np.float16).view(np.uint16)
    return np.where(bad, np.uint16(NAN_BITS[dt]), bits).astype(np.uint16)


def round_trip_bits(x, dt):
    """The contract's round trip of rows x (float32 values of a 16-bit dtype) -> dt bit patterns."""
    img, sb = quant_rows(x)
    return dequant_bits(img, sb, dt)


def round_trip_f64(x):
    """The round trip's exact values (before the rounding into T; equal to it in bf16)."""
    codes, sb = quant_codes(x)
    return dequant_f64(codes, sb)
