"""The planar layout of the 12-bit packed weight copy, on the host: tests/w12_planar.py states the format a second time (numpy packer
and field decoder) and emulates the kernel's nine-operation decode in uint32 (mask, add, rotate right by 4, four byte permutes).
pack -> decode must be exact over every (sign, exponent in window, low byte) at each of the 8 chunk positions, over random full
chunks, at base 0 and base 240, and zero codes without the base must give zeros (the fill outside the matrix).  Five one-fault
mutants — wrong rotate, swapped selectors, mask 0x8f8f8f8f, the sign of weight 4 + k read from byte k, an odd base accepted — must
each be caught by that same comparison."""
import numpy as np
import pytest

import w12_planar as WP


def _window_chunks(base, rng, n):
    """n random chunks whose 8 weights all lie in [base, base + 16)."""
    e = rng.integers(base, base + 16, size=(n, 8), dtype=np.int64)
    return ((rng.integers(0, 2, size=(n, 8)) << 15) | (e << 7) | rng.integers(0, 128, size=(n, 8))).astype(np.uint16)


def _exhaustive(base, rng):
    """[8 positions, 2 * 16 * 128 patterns, 8]: every (sign, exponent in window, mantissa) — every (sign, high-byte field, low byte) —
    at each chunk position, the other seven weights random in-window fillers."""
    s, e, m = np.meshgrid(np.arange(2), np.arange(base, base + 16), np.arange(128), indexing="ij")
    pat = ((s << 15) | (e << 7) | m).reshape(-1).astype(np.uint16)
    out = np.stack([_window_chunks(base, rng, pat.size) for _ in range(8)])
    for k in range(8):
        out[k, :, k] = pat
    return out


def _exact(bits, base, pack_kw=None, dec_kw=None):
    codes, esc = WP.pack_chunks(bits, base, **(pack_kw or {}))
    assert not esc.any()
    return bool(np.array_equal(WP.decode9(codes, base, **(dec_kw or {})), bits))


@pytest.mark.parametrize("base", [0, 108, 240])
def test_planar_decode_is_exact(base):
    rng = np.random.default_rng(base)
    ex = _exhaustive(base, rng)
    assert ex.shape == (8, 4096, 8)
    assert _exact(ex, base)
    rnd = _window_chunks(base, rng, 65536)
    assert _exact(rnd, base)
    codes, _ = WP.pack_chunks(rnd, base)
    assert np.array_equal(WP.decode_fields(codes, base), rnd)  # the format's field decoder agrees with the nine operations
    assert (codes[..., 2] & 0x08080808).any() and (codes[..., 2] & 0x80808080).any()  # both sign positions occur


def test_planar_zero_codes_without_base_give_zeros():
    z = np.zeros((4, 3), dtype=np.uint32)
    assert not WP.decode9(z, 108, inside=False).any()
    assert WP.decode9(z, 108, inside=True).any()  # (with the base they would not: the kernel must drop it outside the matrix)


def test_planar_escapes_are_marked_and_leave_zero_codes():
    bits = np.array([[0x0000, 0x8000, 0x0001, 0x7F80, 0xFF80, 0x7FC1, 0x3CA0, 0xBCA0]], dtype=np.uint16)  # 0x3CA0: exponent 121
    codes, esc = WP.pack_chunks(bits, 108)
    assert esc.tolist() == [[True] * 6 + [False] * 2]
    back = WP.decode9(codes, 108)
    assert np.array_equal(back[0, 6:], bits[0, 6:])
    assert WP.in_window(bits, 108).tolist() == [[False] * 6 + [True] * 2]


MUTANTS = {
    "wrong_rotate": dict(dec_kw=dict(rot=28)),
    "swapped_selectors": dict(dec_kw=dict(sel_lo=WP.SEL_HI, sel_hi=WP.SEL_LO)),
    "mask_8f": dict(dec_kw=dict(mask=0x8F8F8F8F)),
    "sign_of_4_plus_k_in_byte_k": dict(pack_kw=dict(sign_byte=lambda k: k)),
}


@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_planar_mutant_is_rejected(name):
    rng = np.random.default_rng(1)
    assert _exact(_exhaustive(108, rng), 108)
    assert not _exact(_exhaustive(108, rng), 108, **MUTANTS[name]), name


def test_planar_odd_base_is_refused_and_would_be_wrong():
    rng = np.random.default_rng(2)
    bits = _window_chunks(109, rng, 4096)
    with pytest.raises(ValueError):
        WP.pack_chunks(bits, 109)
    codes, esc = WP.pack_chunks(bits, 109, check_even=False)  # the mutant: an odd base accepted
    assert not esc.any()
    assert not np.array_equal(WP.decode9(codes, 109), bits)
