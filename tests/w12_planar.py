"""The planar layout of the 12-bit packed weight copy (include/coldcompress.h, cc_gemv_w12.hip) in numpy: a packer, a field-by-field
decoder of the format, a decoder of whole packed tensors with their patch records, and the kernel's nine-operation decode emulated
in uint32.  Shares no code with the library.  The emulation takes its constants as arguments so that the host test can hand it
one-fault mutants.

A chunk is 8 bf16 weights -> 3 dwords.  With e the 8-bit exponent, s the sign, base even and B = base / 2:
  dword 0 / 1, byte k : low byte of weight k / 4 + k  (e & 1 in bit 7, the mantissa below)
  dword 2,     byte k : s(k) << 7 | ((e(4 + k) >> 1) - B) << 4 | s(4 + ((k + 3) & 3)) << 3 | ((e(k) >> 1) - B)
In-window: base <= e < base + 16; every other weight is an escape (its code is arbitrary: zero here)."""
import numpy as np

MASK = 0x87878787
SEL_LO, SEL_HI = 0x05010400, 0x07030602
ROT = 4


def in_window(bits, base):
    e = (bits.astype(np.int64) >> 7) & 0xFF
    return (e >= base) & (e < base + 16)


def pack_chunks(bits, base, check_even=True, sign_byte=lambda k: (k + 1) & 3):
    """bits uint16 [..., 8] -> (codes uint32 [..., 3], escape mask bool [..., 8]).  `sign_byte(k)`: the byte of dword 2 whose bit 3
    holds the sign of weight 4 + k."""
    if check_even and base % 2:
        raise ValueError("planar: base must be even")
    if not 0 <= base <= 240:
        raise ValueError("planar: base out of range")
    b = bits.astype(np.uint32)
    ok = in_window(bits, base)
    hi = ((((b >> 7) & 0xFF) >> 1) - np.uint32(base // 2)) & np.uint32(0xFFFFFFFF)
    sg = b >> 15
    codes = np.zeros(bits.shape[:-1] + (3,), dtype=np.uint32)
    for k in range(8):
        j = k & 3
        m = ok[..., k]
        codes[..., k >> 2] |= np.where(m, (b[..., k] & 0xFF) << (8 * j), 0).astype(np.uint32)
        if k < 4:
            x = ((sg[..., k] << 7) | hi[..., k]) << (8 * j)
        else:
            x = (hi[..., k] << (8 * j + 4)) | (sg[..., k] << (8 * sign_byte(j) + 3))
        codes[..., 2] |= np.where(m, x, 0).astype(np.uint32)
    return codes, ~ok


def decode_fields(codes, base):
    """The format read field by field: codes uint32 [..., 3] -> bits uint16 [..., 8]."""
    c = codes.astype(np.uint32)
    out = np.zeros(codes.shape[:-1] + (8,), dtype=np.uint32)
    B = base // 2
    for k in range(8):
        j = k & 3
        low = (c[..., k >> 2] >> (8 * j)) & 0xFF
        xb = (c[..., 2] >> (8 * j)) & 0xFF
        if k < 4:
            s, h = xb >> 7, xb & 7
        else:
            s, h = (c[..., 2] >> (8 * ((j + 1) & 3) + 3)) & 1, (xb >> 4) & 7
        out[..., k] = (s << 15) | ((h + B) << 8) | low
    return out.astype(np.uint16)


def _perm(s0, s1, sel):
    """v_perm_b32: selector bytes 0 .. 3 take bytes of the second source, 4 .. 7 of the first."""
    out = np.zeros_like(s0)
    for i in range(4):
        n = (sel >> (8 * i)) & 0xFF
        src = s1 if n < 4 else s0
        out |= ((src >> np.uint32(8 * (n & 3))) & np.uint32(0xFF)) << np.uint32(8 * i)
    return out


def _rotr(x, n):
    n &= 31
    return x if n == 0 else ((x >> np.uint32(n)) | (x << np.uint32(32 - n))) & np.uint32(0xFFFFFFFF)


def decode9(codes, base, inside=True, rot=ROT, mask=MASK, sel_lo=SEL_LO, sel_hi=SEL_HI):
    """The kernel's decode, operation by operation in uint32: two v_and, two v_add, one v_alignbit, four v_perm.  codes uint32
    [..., 3] -> the four dwords of the dense chunk, as bits uint16 [..., 8].  `inside` False: outside the matrix, no base added."""
    q0, q1, X = (codes[..., i].astype(np.uint32) for i in range(3))
    Bx = np.uint32((base // 2) * 0x01010101 if inside else 0)
    m = np.uint32(mask)
    ha = ((X & m) + Bx) & np.uint32(0xFFFFFFFF)
    hb = ((_rotr(X, rot) & m) + Bx) & np.uint32(0xFFFFFFFF)
    d = [_perm(ha, q0, sel_lo), _perm(ha, q0, sel_hi), _perm(hb, q1, sel_lo), _perm(hb, q1, sel_hi)]
    out = np.zeros(codes.shape[:-1] + (8,), dtype=np.uint16)
    for w in range(4):
        out[..., 2 * w] = (d[w] & 0xFFFF).astype(np.uint16)
        out[..., 2 * w + 1] = (d[w] >> 16).astype(np.uint16)
    return out


def decode_tensor(codes, records, base, rb, cu, N, K):
    """A packed tensor with its patch records (the record format is layout 0's): codes uint32 [N, K / 8, 3], records uint32
    [records, 8] -> (bits uint16 [N, K], overflowing records).  An overflowing record is counted, not decoded."""
    nch = K // 8
    bits = decode_fields(codes.reshape(N, nch, 3), base).reshape(N, K)
    nstep = -(-(-(-nch // 64)) // 4)
    nph = -(-nstep // cu)
    overflow = 0
    for rid in np.nonzero(records[:, 0])[0]:
        cnt = int(records[rid, 0])
        if cnt == 0xFFFFFFFF:
            overflow += 1
            continue
        assert 1 <= cnt <= 7
        wave, ph, rg = rid % 4, (rid // 4) % nph, rid // (4 * nph)
        for en in records[rid, 1:1 + cnt]:
            en = int(en)
            t, lane, k = en >> 25, (en >> 19) & 63, (en >> 16) & 7
            row, c = rg * rb + t // cu, ((ph * cu + t % cu) * 4 + wave) * 64 + lane
            bits[row, c * 8 + k] = en & 0xFFFF
    return bits, overflow
