"""numpy twin of cc_sample_nucleus's two filters (include/coldcompress.h), on top of tests/sample_twin.py.  A helper, not a test.
Everything is float64.  The device's masses go through an fp32 exponential, so its nucleus level is held to a BAND around the exact
one (DELTA below, derived from that exponential's error, not from a run); where the exact level's margin exceeds the band, the band
admits the exact level alone.  The level a run chose is read from its number of kept elements."""
import numpy as np
import torch

import sample_twin as S

# The band.  16-bit path: the exponent argument t = d * log2(e) is one fp32 product, off by |t| * 2^-24; for |t| <= 24 that is a
# relative error of at most 1.0e-6 in e, plus 2 ulp (2.4e-7) for the exponential.  Terms with |t| > 24 hold at most V * 2^-24 of the
# mass and err by at most 6.2e-6 relative: under 5e-8 of the total.  The floor to 2^-40 adds at most V * 2^-40 (1.2e-7 at V = 2^17).
# Numerator and denominator of c both err: about 2.5e-6.  (fp32 path: libm's expf, 1 ulp: well inside.)  DELTA = 2^-18 = 3.8e-6.
DELTA = 2.0 ** -18

TOP_PS = (0.5, 0.9, 0.95, 0.999)
MIN_PS = (0.01, 0.1, 0.5, 1.0)
VS = (1, 7, 1000, 32013, 128256)  # 1, 7: most workgroups' slices are empty; 32013: no multiple of 8; 128256: Llama-3's vocabulary
TEMPS = (0.7, 1.0)
TOP_KS = (None, 50)


def table():
    """The 240 cases: (dtype, V, temperature, top_k, top_p)."""
    return [(dt, V, T, k, p) for dt in S.DTYPES for V in VS for T in TEMPS for k in TOP_KS for p in TOP_PS]


def levels(x, K):
    """The distinct values of x in K, descending, with c(v) = mass(x >= v) / mass(K) and the number of elements of K at or above
    each -> (values [L], c [L], counts [L])."""
    xk = x[K]
    m = xk.max()
    vals, cnt = np.unique(xk, return_counts=True)
    vals, cnt = vals[::-1], cnt[::-1]
    mass = np.cumsum(np.exp(vals - m) * cnt)
    return vals, mass / mass[-1], np.cumsum(cnt)


def nucleus(x, K, top_p):
    """-> dict(vals, c, counts, p, j = the exact level j* (first with c >= float32(top_p)), margin = min(c[j*] - p, p - c[j* - 1]))."""
    vals, c, counts = levels(x, K)
    p = float(np.float32(top_p))  # what the entry point receives: 0.999 as a float and as a double differ by 1e-8
    j = int(np.argmax(c >= p)) if p < 1 else len(c) - 1
    margin = c[j] - p
    if j > 0:
        margin = min(margin, p - c[j - 1])
    return dict(vals=vals, c=c, counts=counts, p=p, j=j, margin=float(margin))


def level_of(nuc, n_kept):
    """The level whose set {x >= v} has n_kept elements, or None if none has."""
    hit = np.flatnonzero(nuc["counts"] == int(n_kept))
    return int(hit[0]) if hit.size else None


def in_band(nuc, j):
    """The band rule: c[j] >= p - DELTA and (j == 0 or c[j - 1] < p + DELTA).  With margin > DELTA only j* passes."""
    if j is None:
        return False
    c, p = nuc["c"], nuc["p"]
    return bool(c[j] >= p - DELTA and (j == 0 or c[j - 1] < p + DELTA))


def min_p_set(x, min_p):
    """Exact: x - m >= fp32(log(min_p)) with the subtraction rounded to fp32 (x and m are values of the model dtype)."""
    if min_p is None or min_p <= 0:
        return np.ones(x.shape[0], dtype=bool)
    dmin = np.float32(np.log(np.float64(np.float32(min_p))))
    with np.errstate(invalid="ignore"):
        return (x.astype(np.float32) - np.float32(x[~np.isnan(x)].max())) >= dmin


def twin(logits, temperature, top_k, seed, pos, kept):
    """sample_twin.twin restricted to `kept` (a bool [V] inside the top-k set): probabilities renormalised over it, keys -inf outside."""
    x = S.scaled(logits, temperature)
    m = x[kept].max()
    e = np.where(kept, np.exp(x - m), 0.0)
    u = S.uniforms(seed, pos, x.shape[0])
    with np.errstate(divide="ignore"):
        key = np.where(kept, (x - m) - np.log(-np.log(u)), -np.inf)
    return dict(x=x, kept=kept, probs=e / e.sum(), key=key, token=int(np.argmax(key)))


def check_case(logits, temperature, top_k, top_p, seed, pos, probs, token, n_kept, dtype):
    """One table case: the band rule on the level read from n_kept, zeros exact outside the kept set, check_probs, the token rule.
    -> (how the token was accepted, whether the margin exceeds DELTA)."""
    x = S.scaled(logits, temperature)
    nuc = nucleus(x, S.kept_set(x, top_k), top_p)
    j = level_of(nuc, n_kept)
    what = f"V={x.shape[0]} T={temperature} top_k={top_k} top_p={top_p}"
    assert in_band(nuc, j), (f"{what}: n_kept {int(n_kept)} is level {j}, outside the band around level {nuc['j']} "
                             f"(c = {nuc['c'][max(nuc['j'] - 1, 0):nuc['j'] + 2]}, margin {nuc['margin']:.3g})")
    if nuc["margin"] > DELTA:
        assert j == nuc["j"]
    kept = x >= nuc["vals"][j]
    tw = twin(logits, temperature, top_k, seed, pos, kept)
    S.check_probs(probs, tw, dtype)
    how = S.accepts(token, tw)
    assert how is not None, f"{what}: token {int(token)}, twin {tw['token']}"
    return how, nuc["margin"] > DELTA


def tie_logits(dtype, V=64):
    """Logits whose 0.9 mass point falls inside a run of four equal values (V >= 8): masses 0.5, 0.2, 0.1 above
    four of 0.04 each, the rest sharing 0.04 -> c = 0.5, 0.7, 0.8, 0.96: the level of the four, 7 elements, margin 0.06."""
    g = torch.Generator().manual_seed(5)
    order = torch.randperm(V, generator=g)
    p = torch.full((V,), 0.04 / (V - 7), dtype=torch.float64)
    p[order[:3]] = torch.tensor([0.5, 0.2, 0.1], dtype=torch.float64)
    p[order[3:7]] = 0.04
    logits = torch.log(p).to(dtype)
    x = S.scaled(logits, 1.0)
    nuc = nucleus(x, np.ones(V, dtype=bool), 0.9)
    assert nuc["margin"] > DELTA and nuc["counts"][nuc["j"]] == 7 and nuc["c"][nuc["j"] - 1] < 0.9
    return logits, 7
