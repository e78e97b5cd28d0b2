"""numpy twin of the sampling tail's contract (include/coldcompress.h, cc_sample_topk).  A helper, not a test.
Steps 1 and 2 (scaling, kept set) are EXACT in the model dtype's arithmetic (torch CPU does the rounding); probabilities and Gumbel
keys are float64.  `accepts` is the acceptance rule of the token, defined once for the host and the GPU tests."""
import numpy as np
import torch

M64 = np.uint64(0xFFFFFFFFFFFFFFFF)
SALT = 0x53414D504C45
GOLD = 0x9E3779B97F4A7C15
# A token agrees with the twin if it is the twin's arg-max, or if the twin's own key of it is within G of the winner's.  Winning keys
# are below 17 in magnitude, where an fp32 ulp is 1.9e-6; two 2-ulp logarithms and the final subtraction put an fp32 key within 8e-6
# of its float64 value, and both contenders err, so the gap allows twice that: 1.6e-5, G = 2^-16 being the power of two just below.
# It is an escape, not a tolerance: over a test's cases at most 1 % may pass by it.
G = 2.0 ** -16


def mix64(x):
    with np.errstate(over="ignore"):
        x = x ^ (x >> np.uint64(33))
        x = x * np.uint64(0xFF51AFD7ED558CCD)
        x = x ^ (x >> np.uint64(33))
        x = x * np.uint64(0xC4CEB9FE1A85EC53)
        return x ^ (x >> np.uint64(33))


def uniforms(seed, pos, V):
    """u_i of step 4 for i in [0, V), as float64 (exact: odd multiples of 2^-24).  pos: an int or an array [P] -> [V] or [P, V]."""
    pos = np.asarray(pos, dtype=np.int64)
    base = np.array([((int(seed) ^ SALT) + (int(p) & 0xFFFFFFFF) * GOLD) & int(M64) for p in pos.reshape(-1)], dtype=np.uint64)
    with np.errstate(over="ignore"):
        h = mix64(mix64(base[:, None] + np.arange(V, dtype=np.uint64)[None, :]))
    u = (2.0 * (h >> np.uint64(41)).astype(np.float64) + 1.0) * 2.0 ** -24
    return u.reshape(pos.shape + (V,))


def scaled(logits, temperature):
    """step 1 -> x as float64 (values of the model dtype): one fp32 division, rounded to the dtype."""
    tmax = np.maximum(np.float32(temperature), np.float32(1e-5))
    x = (logits.detach().cpu().float() / torch.tensor(tmax, dtype=torch.float32)).to(logits.dtype)
    return x.double().numpy()


def kept_set(x, top_k):
    """step 2 -> bool [V]: everything not below the k-th largest value counted with multiplicity."""
    V = x.shape[0]
    if top_k is None or top_k <= 0:
        return np.ones(V, dtype=bool)
    k = min(int(top_k), V)
    return x >= np.sort(x)[V - k]


def twin(logits, temperature, top_k, seed, pos):
    """-> dict(x, kept, probs, key, token): probs and key float64 (key = -inf outside the kept set)."""
    x = scaled(logits, temperature)
    kept = kept_set(x, top_k)
    m = x[kept].max()
    e = np.where(kept, np.exp(x - m), 0.0)
    probs = e / e.sum()
    u = uniforms(seed, pos, x.shape[0])
    with np.errstate(divide="ignore"):
        key = np.where(kept, (x - m) - np.log(-np.log(u)), -np.inf)
    return dict(x=x, kept=kept, probs=probs, key=key, token=int(np.argmax(key)))


def tokens(logits, temperature, top_k, seed, positions):
    """The twin's tokens at many positions at once -> int64 [P]."""
    x = scaled(logits, temperature)
    kept = kept_set(x, top_k)
    m = x[kept].max()
    u = uniforms(seed, np.asarray(positions), x.shape[0])
    key = np.where(kept[None, :], (x - m)[None, :] - np.log(-np.log(u)), -np.inf)
    return np.argmax(key, axis=1)


def accepts(token, tw):
    """-> "equal", "gap" (inside the kept set, the twin's key within G of the winner's) or None (refused)."""
    token = int(token)
    if token == tw["token"]:
        return "equal"
    if 0 <= token < tw["key"].shape[0] and tw["kept"][token] and tw["key"][tw["token"]] - tw["key"][token] < G:
        return "gap"
    return None


def top_two_gap(tw):
    k = np.sort(tw["key"][tw["kept"]])
    return np.inf if k.shape[0] < 2 else float(k[-1] - k[-2])


# ---- the cases the host and the GPU tests share
TEMPS = (0.7, 1.0, 1e-7)  # (the last one is clamped to 1e-5)
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
PROB_ULP = {torch.float32: 1.2e-7, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}  # tests/test_gpu_glue.py's bound on the greedy tail


# smallest positive values the probabilities are held to: the dtype's, but no subnormal of the fp32 exp behind them (not promised)
TINY = {torch.float32: 2.0 ** -126, torch.bfloat16: 2.0 ** -126, torch.float16: 2.0 ** -24}


def top_ks(V):
    return (None, 1, 2, 50, V, V + 5)


def case_logits(dtype, V, temperature):
    """Seeded normal logits, sigma 3; under the clamped temperature sigma 0.1, so that x = logits / 1e-5 stays finite in f16."""
    g = torch.Generator().manual_seed(7919 * V + int(1e3 * min(temperature, 10.0)))
    return (torch.randn(V, generator=g) * (0.1 if temperature < 1e-5 else 3.0)).to(dtype)


def check_probs(probs, tw, dtype):
    """probs (a tensor of the model dtype) against the twin: exactly 0 outside the kept set, inside it within the greedy tail's bound."""
    p = probs.detach().cpu().double().numpy()
    assert np.all(p[~tw["kept"]] == 0.0), "a probability outside the kept set is not exactly 0"
    assert np.all(p[tw["kept"]] >= 0.0)
    # the kept set, as far as the dtype can show it: a kept element whose probability the dtype can represent is not 0
    assert np.all(p[tw["kept"] & (tw["probs"] > 4 * TINY[dtype])] > 0.0), "a kept element has probability 0"
    err = np.abs(p - tw["probs"])[tw["kept"]].max()
    assert err <= 2 * PROB_ULP[dtype] * tw["probs"].max() + 1e-12, f"probabilities differ from the twin by {err}"
