"""Known-answer inputs for the prefill attention (cc_prefill_attn_bands: the VALU kernels of csrc/cc_attn_prefill.hip, the two-pass,
single-pass and K-stationary matrix-core kernels of csrc/cc_attn_prefill_mfma.hip) and its side sums.  A helper, not a test:
tests/test_prefill_exact_host.py holds tests/attn_ref.prefill_ref and the oracle to these answers on the CPU and shows that the
comparisons have teeth (the mutants below), tests/test_gpu_prefill_exact.py holds the kernels to them on the device.

A. SELECTOR inputs.  Key row s is a +-1 code word: bit b of s (of s ^ flip[h] where the kv heads differ), b < nbits = ceil(log2 L),
   repeated rep = D // nbits times, the remaining dimensions +1.  Query row i of query head j is amp * code(sel[j][i]), sel <= i, amp
   a power of two.  q . k = amp * (D - 2 rep hamming(sel, s)): every product and partial sum is an integer below 2^24 — the fp32
   dot product is exact in any order — and amp * n is exact in every dtype for n <= 256.  The selected key's score exceeds every other
   live key's by `gap` (measured on the dtype-rounded scores, >= 40), so in every dtype the selected probability rounds to 1 and
   every other is <= exp(-gap):
     y[j, i]  = v[j // R, sel[j][i]] bit for bit (|v| >= 2^-6: a contribution of exp(-40) |v| cannot move the last bit — also in
                the single pass, whose O / l carries the selected weight exactly 1 in O and in l);
     gm[q, k] = dtype(n / R), n = how many of the group's R heads select k at q — formed as dtype(n / R), which is what a kernel
                that sums n ones and divides makes (fp32 and float64 quotients round alike: asserted by the host test);
     colsum, obs, band are plain sums of those — exact in fp32 in any order (asserted per case: every gm is a multiple of 2^-k with
     L 2^k <= 2^24).  Accepted within fig = R L exp(-gap) absolute (< 1e-12 everywhere).  obs is an f32 QUOTIENT sum / obs_len: where
     obs_len is no power of two the f32 output carries one rounding, 2^-24 |obs|, which is added to fig for that plane only.

B. RAMP inputs.  Entries of magnitude <= 8 plus one "position" dimension (s // 4, reversed, or a spike), scale 2^-3: every q . k is an
   integer below 2^24, so dtype(dtype(q . k) * scale) is ONE value on the device, in prefill_ref and in the oracle — the score-rounding
   ambiguity that forces wide limits on Gaussian inputs does not arise.  y: the contract, 1e-3 + 2 ulp_of(dtype) max|y_ref|.  Side
   planes per element: sum over the plane's queries of [mean over the group's heads of step(p_ref) + step(gm_ref)] + L 2^-24 |ref|
   (step = the dtype's spacing there, the smallest subnormal at 0): one step per probability (v_exp_f32 and the reciprocal may land on
   the neighbouring value), one for the rounding of the mean, sequential fp32 accumulation.  No element is left out.
   ONE derived widening, on the matrix-core paths only: their probabilities are exp2 results of v_exp_f32, which returns 0 for a result
   below the smallest normal fp32, where the reference keeps a bf16 subnormal.  A probability p_ref < 2^-126 may therefore be off by
   its whole value: its term is max(step(p_ref), p_ref) there.  (Measured without the term on bf16 "down", L = 400 — the only case
   with such probabilities, in the columns behind key 345: 12.5 x the bound for a band, 5.9 x for a column sum, 6.0 x for the window.)"""
import ctypes as C
import math

import numpy as np
import torch

import attn_ref as A
import compact_ref as R
from helpers import DT_CODE, to_np, from_np

F32, BF, HF = R.F32, R.BF, R.HF
DT_NAME = R.DT_NAME
KV_MARGIN_ROWS = 32  # NaN rows on both sides of q, k, v and y
WS_GUARD = 256       # guard bytes on both sides of the workspace
K_LAZY = 6.0         # csrc/cc_attn_prefill_mfma.hip kLazy
WANTS = ("none", "all", "colsum", "obs")


class PCase:
    """One call: q [HQ, L, D], k / v [H, L, D] CPU tensors of `dt`, the scalar arguments, and for selector cases sel [HQ, L], gap."""

    def __init__(self, cid, family, dt, HQ, H, L, D, scale, q, k, v, obs_len=16, bands=(), sel=None, gap=None, amp=None):
        self.id, self.family, self.dt, self.HQ, self.H, self.L, self.D = cid, family, dt, HQ, H, L, D
        self.R = HQ // H
        self.scale, self.q, self.k, self.v, self.obs_len, self.bands = float(scale), q, k, v, int(obs_len), tuple(int(b) for b in bands)
        self.sel, self.gap, self.amp = sel, gap, amp
        self._cache = {}

    @property
    def ol(self):
        return max(0, min(self.obs_len, self.L))

    def with_side(self, obs_len, bands):
        c = PCase(self.id + f"-obs{obs_len}-b{'.'.join(map(str, bands)) or 'none'}", self.family, self.dt, self.HQ, self.H, self.L, self.D,
                  self.scale, self.q, self.k, self.v, obs_len, bands, self.sel, self.gap, self.amp)
        return c


def default_scale(D):
    return float(np.float32(1.0 / math.sqrt(D)))  # what travels through the C ABI's float argument


# ------------------------------------------------------------------------------------------------ A. selector inputs
def nbits_for(L):
    return max(1, (L - 1).bit_length())


def code_words(L, D, flip=0):
    """[L, D] of +-1: bit b of (s ^ flip) repeated rep times, the rest +1.  -> (codes, rep)"""
    nb = nbits_for(L)
    rep = D // nb
    assert rep >= 1, (L, D)
    s = np.arange(L, dtype=np.int64) ^ int(flip)
    bit = (s[:, None] >> np.arange(nb)[None, :]) & 1
    c = np.ones((L, D), np.float64)
    c[:, : nb * rep] = np.repeat(2.0 * bit - 1.0, rep, axis=1)
    return c, rep


def selector(name, L, j, arg=0, seed=0):
    """sel[i] <= i for query head j."""
    i = np.arange(L, dtype=np.int64)
    if name == "diag":
        return i
    if name == "sink":
        return np.zeros(L, np.int64)
    if name == "back":  # the heads of a group alternate between c and c + 1
        return np.maximum(0, i - (arg + (j & 1)))
    if name == "tile_edge":  # the last key of the previous tile / the first key of the query's own tile, alternating over the heads
        prev = np.maximum(0, 32 * (i // 32) - 1)
        own = 32 * (i // 32)
        return prev if (j + arg) % 2 == 0 else own
    if name == "uniform":
        rng = np.random.default_rng(1000003 * seed + 7919 * j + L)
        return (rng.random(L) * (i + 1)).astype(np.int64)
    raise ValueError(name)


def rounded_scores(n, amp, scale, dt):
    """dtype(dtype(amp * n) * scale) for integer n, float64."""
    x = torch.as_tensor(np.asarray(n, np.float64) * amp)
    return A.rnd(A.rnd(x, dt) * scale, dt).numpy()


def pick_amp(D, L, scale):
    rep = D // nbits_for(L)
    amp = 1
    while 2 * rep * amp * scale < 44.0:
        amp *= 2
    return amp


def selector_case(cid, dt, HQ, H, L, D, sel_name, arg=0, seed=0, scale=None, obs_len=16, bands=(), vary_heads=True):
    scale = default_scale(D) if scale is None else scale
    Rg = HQ // H
    assert Rg * H == HQ
    amp = pick_amp(D, L, scale)
    nb = nbits_for(L)
    codes, rep = zip(*[code_words(L, D, flip=(h * 5 + 1) % (1 << nb) if (vary_heads and h) else 0) for h in range(H)])
    rep = rep[0]
    assert amp * D < (1 << 24) and amp <= 256 and D <= 256
    ham = np.arange(0, nb + 1)
    sc = rounded_scores(D - 2 * rep * ham, amp, scale, dt)
    gap = float(sc[0] - sc[1:].max()) if nb >= 1 and L > 1 else float("inf")
    assert np.isfinite(sc).all()
    sel = np.stack([selector(sel_name, L, j, arg, seed) for j in range(HQ)])
    assert (sel <= np.arange(L)[None, :]).all() and (sel >= 0).all()
    k = torch.from_numpy(np.stack(codes)).to(dt)
    q = torch.from_numpy(np.stack([amp * codes[j // Rg][sel[j]] for j in range(HQ)])).to(dt)
    g = torch.Generator().manual_seed(seed * 131 + L)
    v = torch.randn(H, L, D, generator=g, dtype=torch.float64)
    v = torch.where(v.abs() < 2.0 ** -6, torch.copysign(torch.tensor(2.0 ** -6, dtype=torch.float64), v), v).to(dt)
    return PCase(cid, "sel", dt, HQ, H, L, D, scale, q, k, v, obs_len, bands, sel=sel, gap=gap, amp=amp)


def gm_value(n, Rg, dt, via=torch.float64):
    """dtype(n / R) as float64."""
    return float(torch.tensor(n / Rg if via == torch.float64 else float(np.float32(n) / np.float32(Rg)), dtype=via).to(dt).double())


def selector_fig(c):
    return c.R * c.L * math.exp(-c.gap)


def expected_selector(c):
    """-> dict(y [HQ, L, D] dtype, colsum [H, L], obs [H, L], bands [nb, H, L]) float64 planes: the counts of the module docstring."""
    key = ("exp", c.obs_len, c.bands)
    if key in c._cache:
        return c._cache[key]
    H, Rg, L = c.H, c.R, c.L
    y = torch.stack([c.v[j // Rg][torch.from_numpy(c.sel[j])] for j in range(c.HQ)])
    qi = np.tile(np.arange(L, dtype=np.int64), Rg)
    colsum = np.zeros((H, L))
    osum = np.zeros((H, L))
    band = np.zeros((len(c.bands), H, L))
    table = np.array([gm_value(n, Rg, c.dt) for n in range(Rg + 1)])
    k_pow = 0
    while not np.array_equal(table * 2.0 ** k_pow, np.rint(table * 2.0 ** k_pow)):
        k_pow += 1
    assert L * 2 ** k_pow <= 1 << 24, f"{c.id}: fp32 sums of dtype(n / {Rg}) are not exact at L = {L}"
    ol = c.ol
    for h in range(H):
        lin = qi * L + c.sel[h * Rg:(h + 1) * Rg].reshape(-1)  # (query, key) pairs the group's heads select
        u, n = np.unique(lin, return_counts=True)
        qq, kk, gm = u // L, u % L, table[n]
        np.add.at(colsum[h], kk, gm)
        w = qq >= L - ol
        np.add.at(osum[h], kk[w], gm[w])
        for b, width in enumerate(c.bands):
            w = (qq - kk) < width
            np.add.at(band[b, h], kk[w], gm[w])
    out = dict(y=y, colsum=colsum, obs=osum / ol if ol > 0 else osum * 0.0, bands=band)
    c._cache[key] = out
    return out


def _pow2(n):
    return n > 0 and n & (n - 1) == 0


def check_selector(c, got):
    """got: dict(y=tensor of dt, colsum / obs = [H, L] or None, bands = [nb, H, L] or None).  -> list of failures (empty: accepted)."""
    exp = expected_selector(c)
    fig = selector_fig(c)
    bad = []
    y = got["y"].reshape(exp["y"].shape).to(c.dt) if got["y"].dtype != c.dt else got["y"].reshape(exp["y"].shape)
    if not R.same(y, exp["y"]):
        bad.append(f"{c.id}: y {R.first_diffs(y, exp['y'])}")
    for name in ("colsum", "obs", "bands"):
        g = got.get(name)
        if g is None:
            continue
        g = np.asarray(g, np.float64).reshape(exp[name].shape)
        tol = fig + (2.0 ** -24 * np.abs(exp[name]) if name == "obs" and not _pow2(c.ol) else 0.0)
        err = np.abs(g - exp[name])
        if not bool((err <= tol).all()):  # (NaN fails)
            w = np.unravel_index(int(np.nanargmax(np.where(np.isnan(err), np.inf, err - tol))), err.shape)
            bad.append(f"{c.id}: {name}{list(w)} = {g[w]!r}, expected {exp[name][w]!r} (limit {fig:.3g})")
    return bad


# ------------------------------------------------------------------------------------------------ B. ramp inputs
RAMP_SCALE = 2.0 ** -3


def ramp_case(cid, dt, HQ, H, L, D, variant, seed=0, obs_len=16, bands=()):
    rng = np.random.default_rng(4241 * seed + 17 * L + D + {"up": 0, "down": 1, "spike": 2}[variant])
    q = rng.integers(-1, 2, (HQ, L, D)).astype(np.float64)
    k = rng.integers(-1, 2, (H, L, D)).astype(np.float64)
    s = np.arange(L)
    q[:, :, 0] = 8.0
    if variant == "up":
        k[:, :, 0] = s // 4
    elif variant == "down":
        k[:, :, 0] = (L - 1 - s) // 4
    else:
        k[:, :, 0] = 0.0
        for h in range(H):
            k[h, int(rng.integers((3 * L) // 4, L)), 0] = 30.0
    assert np.abs(q).max() <= 8 and np.abs(k[:, :, 1:]).max() <= 8 and k[:, :, 0].max() <= 256
    g = torch.Generator().manual_seed(seed * 977 + L)
    v = torch.randn(H, L, D, generator=g).to(dt)
    c = PCase(cid, "ramp", dt, HQ, H, L, D, RAMP_SCALE, torch.from_numpy(q).to(dt), torch.from_numpy(k).to(dt), v, obs_len, bands)
    c.variant = variant
    return c


def matrix_core(c):
    """Does the launcher serve this case on the matrix cores (mfma_eligible and the L >= 64 threshold of cc_prefill_attn_bands)?"""
    return c.D == 128 and c.R == 4 and c.dt in (BF, HF) and c.L >= 64


def step_of(x, dt):
    """The dtype's spacing at |x| (float64 array); the smallest subnormal at 0."""
    p, qmin = R.FMT[dt]
    _, e = np.frexp(np.abs(x))  # |x| = m 2^e, m in [0.5, 1)
    return np.ldexp(1.0, np.maximum(e - p, qmin).astype(np.int32))


# ------------------------------------------------------------------------------------------------ the dense float64 reference and its mutants
FAULTS = ("causal_lt", "band_le", "band_wrong_end", "window_long", "window_short", "window_first", "pad_live", "head_mod", "v_unpermuted",
          "serpentine_forward", "no_rescale", "l_only_rescale")


def c_row_perm():
    """position pp = kb * 16 + 8 * hi + i of a 32-key block holds key c_row(kb * 8 + i, hi) (vt_perm_kernel)."""
    out = np.zeros(32, np.int64)
    for pp in range(32):
        kb, hi, i = pp >> 4, (pp >> 3) & 1, pp & 7
        reg = kb * 8 + i
        out[pp] = (reg & 3) + 8 * (reg >> 2) + 4 * hi
    return out


def dense_ref(c, fault=None, nwg=64, want_p=False):
    """prefill_ref with the [H, R, L, L] probabilities materialised (small L only) and, with `fault`, ONE deliberate error.
    fault None is held bit for bit to prefill_ref by the host test.  -> dict(y [HQ, L, D], colsum, obs, bands [nb, H, L]) float64
    (+ p [H, R, L, L], gm [H, L, L] with want_p)."""
    assert fault is None or fault in FAULTS, fault
    dt, H, Rg, L, D = c.dt, c.H, c.R, c.L, c.D
    qd = c.q.double().view(H, Rg, L, D)
    kd, vd = c.k.double(), c.v.double()
    if fault == "head_mod":  # query head j reads kv head j % H
        hm = (torch.arange(H * Rg) % H).view(H, Rg)
        kq, vq = kd[hm], vd[hm]  # [H, R, L, D]
    else:
        kq, vq = kd[:, None].expand(H, Rg, L, D), vd[:, None].expand(H, Rg, L, D)
    npad = (-L) % 32 if fault == "pad_live" else 0
    if npad:  # the padded keys read the clamped last row; their V is the zero padding of the permuted image
        kq = torch.cat([kq, kq[:, :, L - 1:L].expand(H, Rg, npad, D)], dim=2)
        vq = torch.cat([vq, torch.zeros(H, Rg, npad, D, dtype=torch.float64)], dim=2)
    Lk = L + npad
    rows, cols = torch.arange(L).view(-1, 1), torch.arange(Lk).view(1, -1)
    colc = cols.clamp(max=L - 1)  # (a mask made from the clamped row index lets query L - 1 see the padding)
    live = (colc < rows) if fault == "causal_lt" else (colc <= rows)
    sc = A.rnd(A.rnd(torch.einsum("hrid,hrsd->hris", qd, kq), dt) * c.scale, dt).masked_fill(~live, float("-inf"))
    if fault in ("no_rescale", "l_only_rescale"):
        y = _flash_y(c, sc, vq, fault)
        p = A.rnd(torch.nan_to_num(torch.softmax(sc, dim=-1)), dt)
    else:
        p = A.rnd(torch.nan_to_num(torch.softmax(sc, dim=-1)), dt)
        vu = vq
        if fault == "v_unpermuted":  # P in the c_row order against V in the natural one
            Lp = (L + 31) // 32 * 32
            idx = (torch.arange(Lp) // 32) * 32 + torch.from_numpy(c_row_perm())[torch.arange(Lp) % 32]
            vpad = torch.cat([vq, torch.zeros(H, Rg, Lp + 32 - L, D, dtype=torch.float64)], dim=2)
            vu = vpad[:, :, idx[:L]]
        y = A.rnd(torch.einsum("hris,hrsd->hrid", p, vu), dt)
    if fault == "serpentine_forward":  # the second round's query tiles land on the mirrored workgroup's rows
        nqt = (L + 31) // 32
        ys = y.clone()
        for qt in range(nwg, min(2 * nwg, nqt)):
            mt = nwg + (2 * nwg - 1 - qt)
            if mt < nqt and min(L, 32 * mt + 32) - 32 * mt == min(L, 32 * qt + 32) - 32 * qt:
                ys[:, :, 32 * qt:32 * qt + 32] = y[:, :, 32 * mt:32 * mt + 32]
        y = ys
    gm = A.rnd(p.mean(dim=1), dt)[:, :, :L]  # [H, L, L]
    ol = c.ol
    r1 = torch.arange(L)
    win = {"window_long": r1 >= L - ol - 1, "window_short": r1 >= L - ol + 1, "window_first": r1 < ol}.get(fault, r1 >= L - ol)
    n_win = int(win.sum())  # (a window of the wrong length is a mean over its own rows)
    obs = gm[:, win].sum(dim=1) / n_win if ol > 0 and n_win > 0 else torch.zeros(H, L, dtype=torch.float64)
    bands = []
    dist = rows - cols[:, :L]
    for b in c.bands:
        near = dist <= b if fault == "band_le" else (rows >= L - b).expand(L, L) if fault == "band_wrong_end" else dist < b
        bands.append((gm * near).sum(dim=1))
    out = dict(y=y.reshape(H * Rg, L, D), colsum=gm.sum(dim=1).numpy(), obs=obs.numpy(),
               bands=torch.stack(bands).numpy() if bands else np.zeros((0, H, L)))
    if want_p:
        out.update(p=p[..., :L], gm=gm)
    return out


def _flash_y(c, sc, vq, fault=None):
    """The single pass in float64: 32-key tiles, the lazy reference maximum (raised when a tile's maximum exceeds it by more than
    K_LAZY), weights rounded to the dtype UNNORMALISED, l the sum of the rounded weights, y = O / l.  fault: the raise leaves O
    (l_only_rescale) or O and l (no_rescale) unscaled."""
    H, Rg, L, Lk = sc.shape
    D = vq.shape[-1]
    m_ref = torch.full((H, Rg, L), float("-inf"), dtype=torch.float64)
    l = torch.zeros((H, Rg, L), dtype=torch.float64)
    O = torch.zeros((H, Rg, L, D), dtype=torch.float64)
    for k0 in range(0, Lk, 32):
        x = sc[..., k0:k0 + 32]
        mx = x.max(dim=-1).values
        raise_ = (mx > m_ref + K_LAZY) | (torch.isinf(m_ref) & ~torch.isinf(mx))
        m_new = torch.where(raise_, mx, m_ref)
        alpha = torch.where(raise_ & ~torch.isinf(m_ref), torch.exp(m_ref - m_new), torch.ones_like(mx))
        alpha = torch.where(raise_ & torch.isinf(m_ref), torch.zeros_like(mx), alpha)
        w = A.rnd(torch.nan_to_num(torch.exp(x - m_new.unsqueeze(-1))), c.dt)
        w = torch.where(torch.isinf(m_new).unsqueeze(-1), torch.zeros_like(w), w)
        l = (l if fault == "no_rescale" else l * alpha) + w.sum(dim=-1)
        O = (O if fault in ("no_rescale", "l_only_rescale") else O * alpha.unsqueeze(-1)) + torch.einsum("hris,hrsd->hrid", w, vq[:, :, k0:k0 + 32])
        m_ref = m_new
    return A.rnd(O / l.unsqueeze(-1), c.dt)


def flash_ref_y(c):
    """y of the single pass (no fault), [HQ, L, D] float64."""
    H, Rg, L, D = c.H, c.R, c.L, c.D
    rows, cols = torch.arange(L).view(-1, 1), torch.arange(L).view(1, -1)
    kq, vq = c.k.double()[:, None].expand(H, Rg, L, D), c.v.double()[:, None].expand(H, Rg, L, D)
    sc = A.rnd(A.rnd(torch.einsum("hrid,hrsd->hris", c.q.double().view(H, Rg, L, D), kq), c.dt) * c.scale, c.dt)
    return _flash_y(c, sc.masked_fill(cols > rows, float("-inf")), vq).reshape(H * Rg, L, D)


def lazy_raises(c):
    """[HQ, L] int: at how many key-tile boundaries (after the first live tile) a row's maximum rises by more than K_LAZY."""
    H, Rg, L, D = c.H, c.R, c.L, c.D
    rows, cols = torch.arange(L).view(-1, 1), torch.arange(L).view(1, -1)
    sc = A.rnd(A.rnd(torch.einsum("hrid,hsd->hris", c.q.double().view(H, Rg, L, D), c.k.double()), c.dt) * c.scale, c.dt)
    sc = sc.masked_fill(cols > rows, float("-inf"))
    m_ref = sc[..., :32].max(dim=-1).values
    n = torch.zeros_like(m_ref)
    for k0 in range(32, L, 32):
        mx = sc[..., k0:k0 + 32].max(dim=-1).values
        up = mx > m_ref + K_LAZY
        n += up
        m_ref = torch.where(up, mx, m_ref)
    return n.reshape(H * Rg, L)


def ramp_reference(c):
    """-> (ref, bound): ref = prefill_ref's outputs as numpy (y a float64 tensor), bound = the per-element side-plane bounds of the
    module docstring, and bound['y'] the contract's scalar."""
    key = ("ramp", c.obs_len, c.bands)
    if key in c._cache:
        return c._cache[key]
    L, dt = c.L, c.dt
    d = dense_ref(c, want_p=True)
    ref = A.prefill_ref(c.q[None], c.k[None], c.v[None], scale=c.scale, dtype=dt, obs_len=c.ol, bands=c.bands)
    ref = dict(y=ref["y"], colsum=ref["colsum"].numpy(), obs=ref["obs"].numpy(),
               bands=np.stack([ref["bands"][b].numpy() for b in c.bands]) if c.bands else np.zeros((0, c.H, L)))
    assert torch.equal(ref["y"], d["y"].double()) and np.array_equal(ref["colsum"], d["colsum"])
    sp = step_of(d["p"].numpy(), dt)
    if matrix_core(c):  # v_exp_f32 flushes a result below the smallest normal fp32: such a probability may come out 0, off by itself
        pn = d["p"].numpy()
        sp = np.where(pn < 2.0 ** -126, np.maximum(sp, pn), sp)
    per = torch.from_numpy(sp).mean(dim=1) + torch.from_numpy(step_of(d["gm"].numpy(), dt))  # [H, q, k]
    rows, cols = torch.arange(L).view(-1, 1), torch.arange(L).view(1, -1)
    per = per * (cols <= rows)  # (a masked slot is an exact zero on every path)
    acc = L * 2.0 ** -24
    ol = c.ol
    bound = dict(y=1e-3 + 2 * A.ulp_of(dt) * float(ref["y"].abs().max()),
                 colsum=per.sum(dim=1).numpy() + acc * np.abs(ref["colsum"]),
                 obs=(per[:, L - ol:].sum(dim=1).numpy() / ol if ol > 0 else np.zeros((c.H, L))) + acc * np.abs(ref["obs"]),
                 bands=np.stack([(per * ((rows - cols) < b)).sum(dim=1).numpy() for b in c.bands]) + acc * np.abs(ref["bands"])
                 if c.bands else np.zeros((0, c.H, L)))
    c._cache[key] = (ref, bound)
    return ref, bound


def check_ramp(c, got):
    """-> (failures, {name: worst error / bound})."""
    ref, bound = ramp_reference(c)
    bad, ratio = [], {}
    err = float((got["y"].double().reshape(ref["y"].shape) - ref["y"]).abs().max())
    ratio["y"] = err / bound["y"]
    if not err <= bound["y"]:
        bad.append(f"{c.id}: y differs by {err:.4g} (limit {bound['y']:.4g})")
    for name in ("colsum", "obs", "bands"):
        g = got.get(name)
        if g is None or ref[name].size == 0:
            continue
        e = np.abs(np.asarray(g, np.float64).reshape(ref[name].shape) - ref[name])
        ok = e <= bound[name]
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(e == 0, 0.0, e / bound[name])
        ratio[name] = float(np.nanmax(np.where(np.isnan(r), np.inf, r)))
        if not bool(ok.all()):
            w = np.unravel_index(int(np.argmax(np.where(np.isnan(r), np.inf, r))), e.shape)
            bad.append(f"{c.id}: {name}{list(w)} differs by {e[w]:.4g}, {ratio[name]:.3g} of its bound {bound[name][w]:.4g}")
    return bad, ratio


def check(c, got):
    """-> list of failures for either family."""
    return check_selector(c, got) if c.family == "sel" else check_ramp(c, got)[0]


def old_limits_accept(c, got, ref):
    """The limits of test_gpu_parity / test_gpu_fullsize / test_gpu_hybrid: y the contract, column and band sums 5e-2, window mean 4e-3."""
    ok = float((got["y"].double() - ref["y"].double()).abs().max()) <= 1e-3 + 2 * A.ulp_of(c.dt) * float(ref["y"].double().abs().max())
    ok = ok and float(np.abs(got["colsum"] - ref["colsum"]).max()) <= 5e-2 and float(np.abs(got["obs"] - ref["obs"]).max()) <= 4e-3
    return ok and (ref["bands"].size == 0 or float(np.abs(got["bands"] - ref["bands"]).max()) <= 5e-2)


def gaussian_case(L, seed=0, dt=BF, obs_len=16, bands=(32,), sigma=1.0):
    """The inputs of the older suites (test_gpu_parity: q, k, v ~ N(0, 1); the full-size tests: sigma = 1.5); HQ = 4, H = 1, D = 128."""
    g = torch.Generator().manual_seed(seed * 7 + L)
    q = (sigma * torch.randn(4, L, 128, generator=g)).to(dt)
    k = (sigma * torch.randn(1, L, 128, generator=g)).to(dt)
    v = torch.randn(1, L, 128, generator=g).to(dt)
    return PCase(f"gauss-L{L}", "gauss", dt, 4, 1, L, 128, default_scale(128), q, k, v, obs_len, bands)


# ------------------------------------------------------------------------------------------------ marshalling
def _side_shapes(c, want):
    return dict(colsum=(c.H, c.L) if want in ("all", "colsum") else None, obs=(c.H, c.L) if want in ("all", "obs") else None,
                bands=(len(c.bands), c.H, c.L) if want == "all" and c.bands else None)


def run_oracle(o, c, want="all"):
    """-> (return code, got) of the oracle's cc_prefill_attn_bands on host copies."""
    sh = _side_shapes(c, want)
    q, k, v = to_np(c.q), to_np(c.k), to_np(c.v)
    y = to_np(torch.zeros(c.HQ, c.L, c.D, dtype=c.dt))
    side = {n: (None if s is None else np.full(s, np.nan, np.float32)) for n, s in sh.items()}
    nb = len(c.bands) if side["bands"] is not None else 0
    barr = (C.c_int32 * nb)(*c.bands[:nb]) if nb else None
    rc = o.fns()["cc_prefill_attn_bands"](o.ptr(q), o.ptr(k), o.ptr(v), c.HQ, c.H, c.L, c.D, DT_CODE[c.dt], c.scale, o.ptr(y), o.ptr(side["colsum"]),
                                          o.ptr(side["obs"]), c.obs_len, barr, nb, o.ptr(side["bands"]), None, 0, None)
    return rc, dict(y=from_np(y, c.dt), **side)


def workspace_bytes(c):
    from cold_compress_amd import _abi

    return int(_abi.lib()["cc_prefill_attn_workspace_bytes"](c.HQ, c.H, c.L, c.D, DT_CODE[c.dt]))


def new_workspace(nbytes, device="cuda"):
    """NaN-filled (0xFF bytes) workspace between two guards of 0xAB bytes."""
    ws = torch.full((nbytes + 2 * WS_GUARD,), 0xFF, dtype=torch.uint8, device=device)
    ws[:WS_GUARD] = 0xAB
    ws[WS_GUARD + nbytes:] = 0xAB
    return ws


def run_device(c, want="all", ws=None, device="cuda"):
    """-> (return code, got) of the device's cc_prefill_attn_bands.  q, k, v, y sit inside NaN-filled buffers with KV_MARGIN_ROWS rows
    of margin on both sides (so K and V have 32 NaN rows behind row L - 1), the side outputs with 64 floats; the workspace (the
    caller's new_workspace(), or a fresh NaN-filled one of exactly cc_prefill_attn_workspace_bytes) between guard bytes.  Afterwards: margins and
    guards intact, inputs unchanged."""
    from cold_compress_amd import _abi

    sh = _side_shapes(c, want)
    if ws is None:
        ws = new_workspace(workspace_bytes(c), device)
    nbytes = ws.numel() - 2 * WS_GUARD  # (a caller's larger workspace is handed over whole)
    assert nbytes >= workspace_bytes(c)
    bufs, margin = {}, {}

    def place(name, t, m):
        b = torch.full((t.numel() + 2 * m,), float("nan"), dtype=t.dtype, device=device)
        b[m:m + t.numel()] = t.reshape(-1).to(device)
        bufs[name], margin[name] = b, m

    for n in ("q", "k", "v"):
        place(n, getattr(c, n), KV_MARGIN_ROWS * c.D)
    place("y", torch.full((c.HQ, c.L, c.D), float("nan"), dtype=c.dt), KV_MARGIN_ROWS * c.D)
    for n, s in sh.items():
        if s is not None:
            place(n, torch.full(s, float("nan"), dtype=F32), R.MARGIN)

    def ptr(n):
        b = bufs.get(n)
        return None if b is None else C.c_void_p(b.data_ptr() + margin[n] * b.element_size())

    nb = len(c.bands) if sh["bands"] is not None else 0
    barr = (C.c_int32 * nb)(*c.bands[:nb]) if nb else None
    torch.cuda.synchronize()
    rc = _abi.lib()["cc_prefill_attn_bands"](ptr("q"), ptr("k"), ptr("v"), c.HQ, c.H, c.L, c.D, DT_CODE[c.dt], c.scale, ptr("y"), ptr("colsum"),
                                             ptr("obs"), c.obs_len, barr, nb, ptr("bands"), C.c_void_p(ws.data_ptr() + WS_GUARD), nbytes, None)
    torch.cuda.synchronize()
    got = dict(colsum=None, obs=None, bands=None)
    for n, b in bufs.items():
        h, m = b.cpu(), margin[n]
        assert R.holds_sentinel(h[:m]) and R.holds_sentinel(h[h.numel() - m:]), f"{c.id}: margin of '{n}' overwritten"
        body = h[m:h.numel() - m]
        if n in ("q", "k", "v"):
            assert R.same(body.view(getattr(c, n).shape), getattr(c, n)), f"{c.id}: input '{n}' modified"
        elif n == "y":
            got["y"] = body.view(c.HQ, c.L, c.D)
        else:
            got[n] = body.view(sh[n]).numpy()
    g = ws.cpu()
    assert bool((g[:WS_GUARD] == 0xAB).all()) and bool((g[WS_GUARD + nbytes:] == 0xAB).all()), f"{c.id}: wrote outside the workspace"
    return rc, got


# ------------------------------------------------------------------------------------------------ case lists
MFMA_SHORT_L = (64, 65, 79, 80, 81, 95, 96, 97, 127, 128, 129)
BAND_SETS = ((), (32,), (1, 33), (2, 31, 100, "L"), ("L+5",), (100, "L"))
OBS_LENS = (0, 1, 16, 32, 33, 47, "L", "L+3")
SELECTORS = (("diag", 0), ("sink", 0), ("uniform", 0), ("tile_edge", 0), ("tile_edge", 1))


def _resolve(x, L):
    return L if x == "L" else L + int(x[2:]) if isinstance(x, str) else x


def side_variants(i, L):
    """The i-th (obs_len, bands) pair of a rotation through OBS_LENS x BAND_SETS."""
    bands = tuple(_resolve(b, L) for b in BAND_SETS[i % len(BAND_SETS)])
    return _resolve(OBS_LENS[(i * 5 + i // len(OBS_LENS)) % len(OBS_LENS)], L), bands


def back_args(obs_len, bands):
    """c for back(c): b - 1 (inside) and b (just outside) for every band width and for the window."""
    out = []
    for b in tuple(bands) + (obs_len,):
        out += [a for a in (b - 1, b) if a >= 0]
    return sorted(set(out))


def mfma_short_cases(dt):
    """D = 128, HQ = 4 H; every short L with H in {1, 3}, selectors and side variants rotating; the back(c) selectors at the band and
    window edges of each variant; the xcd_remap branch (H % 8 == 0) at L = 97."""
    out, i = [], 0
    for L in MFMA_SHORT_L:
        for H in (1, 3):
            name, arg = SELECTORS[i % len(SELECTORS)]
            ol, bands = side_variants(i, L)
            out.append(selector_case(f"sel-{DT_NAME[dt]}-H{H}-L{L}-{name}{arg}", dt, 4 * H, H, L, 128, name, arg, seed=i, obs_len=ol, bands=bands))
            a = back_args(ol, bands)
            cb = a[i % len(a)] if a else 7
            out.append(selector_case(f"sel-{DT_NAME[dt]}-H{H}-L{L}-back{cb}", dt, 4 * H, H, L, 128, "back", min(cb, L), seed=i, obs_len=ol, bands=bands))
            i += 1
    for H in (8, 16):
        out.append(selector_case(f"sel-{DT_NAME[dt]}-H{H}-L97-uniform", dt, 4 * H, H, 97, 128, "uniform", seed=H, obs_len=33, bands=(2, 31, 100, 97)))
    return out


def mfma_band_obs_cases(dt, L=97):
    """Every band set and every obs_len at one ragged length, with back(c) at each edge."""
    out = []
    for i in range(max(len(BAND_SETS), len(OBS_LENS))):
        bands = tuple(_resolve(b, L) for b in BAND_SETS[i % len(BAND_SETS)])
        ol = _resolve(OBS_LENS[i % len(OBS_LENS)], L)
        for cb in back_args(min(ol, L), [min(b, L) for b in bands])[:4] or [7]:
            out.append(selector_case(f"sel-{DT_NAME[dt]}-L{L}-back{cb}", dt, 4, 1, L, 128, "back", cb, seed=i, obs_len=ol, bands=bands))
    return [c.with_side(c.obs_len, c.bands) for c in out]


def mfma_long_cases(dt, L, H=1):
    """diag, uniform and back at a length whose query tiles need a further round of the persistent loops."""
    ol, bands = (47, (33, 100)) if L != 4133 else (16, (1, 32, 100, L))
    return [selector_case(f"sel-{DT_NAME[dt]}-H{H}-L{L}-{n}{a}", dt, 4 * H, H, L, 128, n, a, seed=L, obs_len=ol, bands=bands)
            for n, a in (("diag", 0), ("uniform", 0), ("back", bands[-1] - 1 if bands[-1] < L else 99))]


def mfma_ramp_cases(dt):
    return [ramp_case(f"ramp-{DT_NAME[dt]}-{var}-L{L}", dt, 4, 1, L, 128, var, seed=L, obs_len=(16, 33, 47)[n % 3], bands=((32,), (1, 33), (2, 31, 100, L))[n % 3])
            for n, (L, var) in enumerate((L, var) for L in (97, 160, 400) for var in ("up", "down", "spike"))]


def valu_cases():
    """Below the matrix-core threshold in its geometry, and the other geometries."""
    out, i = [], 0
    for dt in (BF, HF):
        for L in (1, 2, 31, 32, 33, 63):
            name, arg = SELECTORS[i % len(SELECTORS)]
            ol, bands = side_variants(i, L)
            out.append(selector_case(f"valu-{DT_NAME[dt]}-D128-R4-L{L}-{name}{arg}", dt, 4, 1, L, 128, name, arg, seed=i, obs_len=ol, bands=bands))
            i += 1
    geo = [(F32, 128, 4, 1, 70), (F32, 128, 4, 2, 33), (BF, 64, 4, 1, 9), (BF, 64, 4, 2, 257), (BF, 64, 4, 1, 263), (BF, 64, 1, 2, 1031),
           (HF, 128, 2, 2, 100), (BF, 128, 3, 2, 100), (HF, 64, 3, 1, 70), (BF, 128, 7, 1, 130), (HF, 128, 8, 1, 70), (BF, 256, 2, 1, 70),
           (HF, 256, 2, 2, 45), (BF, 16, 4, 1, 200), (HF, 16, 2, 1, 37), (BF, 80, 4, 1, 200), (F32, 80, 2, 1, 97), (F32, 64, 1, 3, 65)]
    for dt, D, Rg, H, L in geo:
        for name, arg in (SELECTORS[i % len(SELECTORS)], ("back", None)):
            ol, bands = side_variants(i, L)
            if arg is None:
                a = back_args(min(ol, L), [min(b, L) for b in bands]) or [7]
                arg = a[i % len(a)]
            out.append(selector_case(f"valu-{DT_NAME[dt]}-D{D}-R{Rg}-H{H}-L{L}-{name}{arg}", dt, Rg * H, H, L, D, name, arg, seed=i, obs_len=ol, bands=bands))
            i += 1
    return out


def valu_ramp_cases():
    out = []
    for n, (dt, D, L) in enumerate(((BF, 64, 97), (HF, 64, 160), (BF, 64, 400), (F32, 128, 97), (F32, 128, 160))):
        for var in ("up", "down", "spike"):
            out.append(ramp_case(f"ramp-valu-{DT_NAME[dt]}-D{D}-{var}-L{L}", dt, 4, 1, L, D, var, seed=L + n, obs_len=(16, 33)[n % 2], bands=((32,), (1, 33, 100))[n % 2]))
    return out


def kstat_cases(dt):
    """The K-stationary form: query-segment (512) and 128-key-block edges."""
    out = []
    for L in (513, 640, 1153):
        for n, a in (("uniform", 0), ("back", 32), ("tile_edge", 0)):
            out.append(selector_case(f"sel-{DT_NAME[dt]}-L{L}-{n}{a}", dt, 4, 1, L, 128, n, a, seed=L, obs_len=33, bands=(1, 33) if L != 640 else (32,)))
    return out


def host_selector_cases():
    """Every selector case with L <= 512."""
    out = []
    for dt in (BF, HF):
        out += mfma_short_cases(dt) + mfma_band_obs_cases(dt)
    return out + [c for c in valu_cases() if c.L <= 512]


def mutant_cases():
    """The (short) list every mutant is run against."""
    out = [selector_case("m-diag-L130", BF, 4, 1, 130, 128, "diag", obs_len=16, bands=(32,)),
           selector_case("m-back15-L130", BF, 4, 1, 130, 128, "back", 15, obs_len=16, bands=(32,)),
           selector_case("m-back31-L130", HF, 4, 1, 130, 128, "back", 31, obs_len=16, bands=(32,)),
           selector_case("m-uniform-L300", BF, 8, 2, 300, 128, "uniform", seed=3, obs_len=16, bands=(32, 100)),
           selector_case("m-tile-L97", HF, 4, 1, 97, 128, "tile_edge", obs_len=33, bands=(1, 33)),
           ramp_case("m-ramp-up-L160", BF, 4, 1, 160, 128, "up", seed=1, obs_len=16, bands=(32,)),
           ramp_case("m-ramp-spike-L160", BF, 4, 1, 160, 128, "spike", seed=1, obs_len=16, bands=(32,))]
    return out
