"""One interface over the numpy twins of the four fused KV-cache image formats (include/coldcompress.h):
  "fused"  the uint8 grid          tests/kv_uint4_twin.py with 255 levels, one code per byte
  "fp8"    OCP e4m3fn, 2^e per row  tests/kv_fp8_twin.py
  "uint4"  the grid with 15 levels tests/kv_uint4_twin.py, two codes per byte
  "mxfp4"  OCP e2m1, e8m0 per 32   tests/kv_mxfp4_twin.py
A helper, not a test.  numpy only; rows are torch tensors of the model dtype (bf16 / f16) or float32 arrays holding such values.

A row of K and a row of V share one [4]-word entry of kv_qparams: words 0, 1 are K's, words 2, 3 are V's.  round_trip() serves ONE
row kind and returns its PAIR of words; qparams() puts a K pair and a V pair together into the entry's four words.
  fused / uint4   (scale, minimum) as float32 bit patterns
  fp8             (2^e as a float32 bit pattern, 0)
  mxfp4           (the scale bytes, byte b = block b, 0)
tests/test_step_exact_quant_host.py holds the 255-level form to the oracle's cc_kv_quant_rows / cc_kv_dequant_rows bit for bit."""
import numpy as np
import torch

import kv_fp8_twin as F8
import kv_mxfp4_twin as MX
import kv_uint4_twin as U4

FORMATS = ("fused", "fp8", "uint4", "mxfp4")
LEVELS = {"fused": 255, "uint4": 15}
FOUR_BIT = ("uint4", "mxfp4")
DT_NAME = {torch.bfloat16: "bf16", torch.float16: "f16", "bf16": "bf16", "f16": "f16"}


def cache_bits(fmt):
    """The cache_bits argument the cache classes take with cache_quant_mode=fmt."""
    return 4 if fmt in FOUR_BIT else 8


def image_width(D, fmt):
    return D // 2 if fmt in FOUR_BIT else D


def _f32(rows):
    if torch.is_tensor(rows):
        return rows.detach().cpu().to(torch.float32).numpy()
    return np.asarray(rows, np.float32)


def _u32(f):
    return np.ascontiguousarray(f, np.float32).view(np.uint32)


def encode(rows, fmt):
    """Rows [..., D] -> (images uint8 [..., D or D / 2], words uint32 [..., 2])."""
    assert fmt in FORMATS, fmt
    x = _f32(rows)
    if fmt in LEVELS:
        q, scale, mn = U4.quant_codes(x, LEVELS[fmt])
        img = q if fmt == "fused" else U4.pack(q)
        return img, np.stack([_u32(scale), _u32(mn)], axis=-1)
    if fmt == "fp8":
        codes, e = F8.quant_rows(x)
        w = _u32(np.ldexp(np.float32(1), e).astype(np.float32))
        return codes, np.stack([w, np.zeros_like(w)], axis=-1)
    img, sb = MX.quant_rows(x)
    w = MX.scale_word(sb)
    return img, np.stack([w, np.zeros_like(w)], axis=-1)


def decode(img, words, dt, fmt, block0=False):
    """Images + their pairs of words -> the dt bit patterns [..., D] the decode kernels see.  block0 (a mutant of the MXFP4 decode,
    tests/step_exact.py): every block is decoded with block 0's scale."""
    assert fmt in FORMATS, fmt
    name = DT_NAME[dt]
    img = np.asarray(img, np.uint8)
    words = np.ascontiguousarray(words, np.uint32)
    if fmt in LEVELS:
        codes = img if fmt == "fused" else U4.unpack(img)
        scale, mn = words[..., 0].view(np.float32), words[..., 1].view(np.float32)
        return U4.to_bits(U4.dequant_f32(codes, scale, mn), name)
    if fmt == "fp8":
        m, k = np.frexp(words[..., 0].view(np.float32))
        assert np.all(m == 0.5), "fp8: word 0 is a power of two"
        return F8.dequant_bits(img, (k - 1).astype(np.int32), name)
    sb = MX.scale_bytes(words[..., 0], img.shape[-1] * 2 // MX.BLOCK)
    if block0:
        sb = np.repeat(sb[..., :1], sb.shape[-1], axis=-1)
    return MX.dequant_bits(img, sb, name)


def round_trip(rows, dt, fmt):
    """-> (images uint8, the rows' pairs of kv_qparams words uint32 [..., 2], dt bit patterns of the decoded values uint16 [..., D])."""
    img, words = encode(rows, fmt)
    return img, words, decode(img, words, dt, fmt)


def qparams(k_words, v_words):
    """A K pair and a V pair -> the four words of the (head, slot) entry of kv_qparams."""
    return np.concatenate([np.asarray(k_words, np.uint32), np.asarray(v_words, np.uint32)], axis=-1)


def swap_nibbles(img):
    """(a mutant of the 4-bit inserts: high nibble first)"""
    img = np.asarray(img, np.uint8)
    return ((img >> 4) | (img << 4)).astype(np.uint8)


def to_tensor(bits16, dt):
    """uint16 bit patterns -> a torch tensor of dt."""
    return torch.from_numpy(np.ascontiguousarray(bits16, np.uint16).view(np.int16).copy()).view(dt)
