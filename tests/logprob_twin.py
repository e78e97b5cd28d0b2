"""References for cc_logprob_rows (include/coldcompress.h): the float64 reference (torch.log_softmax / torch.logsumexp of the row in
double precision, the rank by comparison), an fp32 twin of the contract (sliced (m_g, s_g) partials folded in order), the input
families and the tolerance.

Tolerance: |logprob - ref64| <= 2^-18 * (1 + |ref64|), the same for lse.  At most about 32 fp32 roundings lie on any path of the sum
(a lane's serial adds, the shuffles, the waves, the fold): at most 2^-19 on log S; exp and log add a few ulp; (x_t - M) and log S are
each at most |ref64| in magnitude.  The fp32 twin's own worst error over three dtypes, V from 1 to 128256 and scales 0.01 to 30 is
1.03e-7 * (1 + |ref|): the bound leaves a factor of about 37 for a device's own exp, log and order.  A 16-bit slip anywhere is 2^-9.

Classes: the results are fp32, so the class of a reference value (finite, -inf, +inf, NaN) is taken after rounding it to fp32 — a
float64 log-probability of -6e38 (an fp32 row that spans both ends of the format) is -inf in the only format the result has."""
import functools
import math

import numpy as np
import torch

DTYPES = (torch.float32, torch.bfloat16, torch.float16)
TOL = 2.0 ** -18
SLICES = 128
FAMILIES = ("outlier", "ramp", "equal", "extreme", "tie4", "some_ninf", "all_ninf", "pinf", "two_nan")


def _below(v, dtype):
    """the largest value of `dtype` below v (v > 0, a value of the dtype)."""
    t = torch.tensor([v], dtype=dtype)
    bits = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}[dtype]
    return float((t.view(bits) - 1).view(dtype)[0])


@functools.lru_cache(maxsize=None)
def family(name, dtype, V):
    """-> (row [V] of `dtype`, targets: a tuple of indices) or None where the family needs a larger V.  Every row's targets hold the
    first, the last, a maximum and a middle element, and what the family is about."""
    g = torch.Generator().manual_seed(1000003 * FAMILIES.index(name) + 31 * V + DTYPES.index(dtype))
    base = torch.randn(V, generator=g)
    extra = ()
    if name == "outlier":  # normal * 4 with one element raised 20 above the maximum
        x = base * 4
        j = int(torch.randint(0, V, (1,), generator=g))
        x[j] = x.max() + 20
    elif name == "ramp":
        x = torch.linspace(-8.0, 8.0, V) if V > 1 else torch.tensor([0.5])
    elif name == "equal":  # logprob = -log V and rank 0 for every target
        x = torch.full((V,), 1.5)
    elif name == "extreme":  # magnitudes near the dtype's largest finite value in both signs
        big = 0.9 * torch.finfo(dtype).max
        x = torch.where(torch.arange(V) % 2 == 0, torch.tensor(big), torch.tensor(-big)) * (1 - 0.01 * torch.rand(V, generator=g))
    elif name == "tie4":  # a tie of four at the top; targets among them and just below them
        if V < 5:
            return None
        x = base.clamp(-2, 2)
        idx = torch.randperm(V, generator=g)[:5]
        x[idx[:4]] = 5.0
        x[idx[4]] = _below(5.0, dtype)
        extra = (int(idx[1]), int(idx[3]), int(idx[4]))
    elif name == "some_ninf":
        x = base * 3
        x[1::3] = -float("inf")
        extra = (1,) if V > 1 else ()
    elif name == "all_ninf":
        x = torch.full((V,), -float("inf"))
    elif name == "pinf":
        x = base * 3
        j = int(torch.randint(0, V, (1,), generator=g))
        x[j] = float("inf")
        extra = (j,)
    elif name == "two_nan":
        x = base * 3
        idx = torch.randperm(V, generator=g)[:2]
        x[idx] = float("nan")
        extra = (int(idx[0]),)
    else:
        raise KeyError(name)
    x = x.to(dtype)
    xf = x.float()
    top = int(torch.argmax(torch.where(torch.isnan(xf), torch.full_like(xf, -float("inf")), xf)))
    targets = tuple(dict.fromkeys((0, V - 1, top, V // 2) + extra))
    return x, targets


def ref64(x):
    """-> (log_softmax [V] float64, lse float64 scalar tensor) of one row."""
    xd = x.double()
    return torch.log_softmax(xd, dim=-1), torch.logsumexp(xd, dim=-1)


def rank_ref(x, t):
    xd = x.double()
    return -1 if bool(torch.isnan(xd[t])) else int((xd > xd[t]).sum())


def twin32(x, t, slices=SLICES):
    """The contract in fp32 numpy: slices of ceil(V / slices) elements rounded up to 8, per slice (m_g, s_g), one fold in slice order.
    -> (logprob, lse, rank) as np.float32 / int."""
    f32 = np.float32
    v = x.float().numpy()
    V = v.shape[0]
    per = (-(-V // slices) + 7) & ~7
    with np.errstate(all="ignore"):
        parts = []
        for lo in range(0, V, per):
            s = v[lo:lo + per]
            m = np.fmax.reduce(s, initial=f32(-np.inf))  # (NaN never counts)
            e = np.where(s == m, f32(1), np.exp((s - m).astype(f32))).astype(f32)
            parts.append((f32(m), e.sum(dtype=f32)))
        M = np.fmax.reduce(np.array([m for m, _ in parts], dtype=f32), initial=f32(-np.inf))
        S = f32(0)
        for m, s in parts:
            if s != 0:
                S = f32(S + f32(s * (f32(1) if m == M else np.exp(f32(m - M)))))
        logS = np.log(S).astype(f32)
        lse = f32(M + logS)
        xt = v[t]
        lp = f32(np.nan) if M == np.inf else f32(f32(xt - M) - logS)
        rank = -1 if xt != xt else int((v > xt).sum())
    return lp, lse, rank


def cls(v):
    """the class of a value once it is an fp32: "nan", "-inf", "+inf" or "finite"."""
    with np.errstate(over="ignore"):
        v = float(np.float32(float(v)))
    if math.isnan(v):
        return "nan"
    if math.isinf(v):
        return "-inf" if v < 0 else "+inf"
    return "finite"


def error(got, ref):
    """-> |got - ref| / (1 + |ref|) where the reference is finite as an fp32 (to be held under TOL); asserts equal classes."""
    got, ref = float(got), float(ref)
    assert cls(got) == cls(ref), f"class {cls(got)} ({got}), reference {cls(ref)} ({ref})"
    if cls(ref) != "finite":
        return 0.0
    return abs(got - ref) / (1.0 + abs(ref))
