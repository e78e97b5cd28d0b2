"""References for cc_logprob_topn (include/coldcompress.h): the float64 reference — the ids by the contract's total order (larger
value first, +0 and -0 equal, equal values by lower index, NaN never listed), the values from logprob_twin.ref64 — and the input
families: those of logprob_twin that bear on an order, and the ones a sliced top-N can get wrong.

The ids carry no tolerance: the order compares the row's own values, which every dtype converts to fp32 exactly.  The values keep
logprob_twin.TOL by class: each is cc_logprob_rows' (x - M) - log S for that id.

Slices: the kernel cuts the row into logprob_twin.SLICES slices of `per(V)` elements (the last may be shorter or missing)."""
import functools

import numpy as np
import torch

import logprob_twin as L

N_MAX = 20
SHARED = ("outlier", "equal", "tie4", "some_ninf", "all_ninf", "pinf", "two_nan")
OWN = ("one_slice_mid", "one_slice_last", "across", "ramp_up", "ramp_down", "zeros", "few_finite")
FAMILIES = SHARED + OWN


def per(V):
    return (-(-V // L.SLICES) + 7) & ~7


def _dtype_values(dtype):
    """every value of a 16-bit dtype in [-8, 8], ascending, one zero."""
    v = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dtype).float()
    v = v[torch.isfinite(v) & (v.abs() <= 8)]
    return torch.unique(v)  # (sorted; -0 == +0 collapse)


def _ramp(dtype, V):
    """an increasing row: strictly where the dtype has V values in [-8, 8] (always in fp32; up to about 32000 elements in the 16-bit
    formats), otherwise in runs of equal values, which the order breaks by index."""
    if dtype == torch.float32:
        return torch.linspace(-8.0, 8.0, V, dtype=torch.float64).float() if V > 1 else torch.tensor([0.5])
    vals = _dtype_values(dtype)
    return vals[(torch.arange(V, dtype=torch.int64) * len(vals)) // V] if V > 1 else torch.tensor([0.5])


@functools.lru_cache(maxsize=None)
def family(name, dtype, V):
    """-> (row [V] of `dtype`, targets: a tuple of indices) or None where the family needs a larger V."""
    if name in SHARED:
        return L.family(name, dtype, V)
    g = torch.Generator().manual_seed(7000003 * OWN.index(name) + 31 * V + L.DTYPES.index(dtype))
    base = torch.randn(V, generator=g).clamp(-2, 2)
    p = per(V)
    n_slices = -(-V // p)
    if name in ("one_slice_mid", "one_slice_last"):
        # the N + 3 largest values (as many of them as the slice holds), all distinct, at shuffled places of ONE slice: an interior
        # one, or the last, which is partial
        g_ = n_slices // 2 if name == "one_slice_mid" else n_slices - 1
        lo, hi = g_ * p, min(V, (g_ + 1) * p)
        if n_slices < 3 or (name == "one_slice_last" and hi - lo == p):
            return None
        c = min(N_MAX + 3, hi - lo)
        x = base
        x[lo + torch.randperm(hi - lo, generator=g)[:c]] = 10 + 0.25 * torch.arange(c, dtype=torch.float32)
    elif name == "across":  # equal maxima on both sides of a slice boundary and at both ends of the row
        if n_slices < 3:
            return None
        x = base
        b = (n_slices // 2) * p
        x[torch.tensor([0, b - 1, b, V - 1])] = 6.0
    elif name == "ramp_up":
        x = _ramp(dtype, V)
    elif name == "ramp_down":
        x = _ramp(dtype, V).flip(0)
    elif name == "zeros":  # +0 and -0 alternating above a negative background
        if V < 2:
            return None
        x = -1 - base.abs()
        at = torch.sort(torch.randperm(V, generator=g)[:min(V, 30)]).values
        x[at] = torch.where(torch.arange(len(at)) % 2 == 0, torch.tensor(0.0), torch.tensor(-0.0))
    elif name == "few_finite":  # three non-NaN elements (or V), the rest NaN
        x = torch.full((V,), float("nan"))
        at = torch.randperm(V, generator=g)[:min(V, 3)]
        x[at] = base[at] * 3
    else:
        raise KeyError(name)
    x = x.to(dtype)
    xf = x.float()
    top = int(torch.argmax(torch.where(torch.isnan(xf), torch.full_like(xf, -float("inf")), xf)))
    return x, tuple(dict.fromkeys((0, V - 1, top, V // 2)))


def ref_ids(x, n):
    """-> the n first ids of the row in the total order (a list of python ints), padded with -1."""
    v = x.double().numpy()
    keep = np.flatnonzero(~np.isnan(v))
    with np.errstate(all="ignore"):
        order = keep[np.argsort(-v[keep], kind="stable")]  # (-0 and +0 compare equal; stable: equal values stay in index order)
    ids = [int(i) for i in order[:n]]
    return ids + [-1] * (n - len(ids))


def ref_values(x, ids):
    """-> float64 log-probabilities of the listed ids (NaN behind an id of -1)."""
    lsm, _ = L.ref64(x)
    return [float(lsm[i]) if i >= 0 else float("nan") for i in ids]


def check(x, n, top_ids, top_lp, what=""):
    """one row's results against the reference: ids exact, values within TOL by class; -> the worst error over (1 + |ref|)."""
    ids = ref_ids(x, n)
    got = [int(i) for i in top_ids]
    assert got == ids, f"{what}: ids {got}, reference {ids}"
    worst = 0.0
    for j, ref in enumerate(ref_values(x, ids)):
        e = L.error(top_lp[j], ref)
        assert e <= L.TOL, f"{what}: position {j} (id {ids[j]}): error {e:.3e} * (1 + |ref|)"
        worst = max(worst, e)
    return worst
