"""Plain references of the caller-glue kernels and the greedy tail of csrc/cc_glue.hip (cc_add_rmsnorm, cc_qkv_rope, cc_silu_mul,
cc_softmax_argmax), written from the contracts of include/coldcompress.h.  A helper, not a test: tests/test_glue_ref_host.py holds
the references to the oracle's twins on the CPU and shows that the case list rejects wrong variants of every kernel,
tests/test_gpu_glue_shapes.py holds the kernels to the references on the device.  The comparison helpers, the sentinel buffers and
the marshalling are tests/compact_ref.py's.

Every reference returns, per output, a pair (lo, hi) of tensors of the model dtype; the device value must lie inside (inside()).
Where lo and hi have the same bit pattern that is equality of bit patterns.

EXACT parts (lo is hi) — numpy float32 arithmetic, one IEEE operation at a time (numpy does not contract a product into an add):
  cc_add_rmsnorm   h = dtype(fp32(x) + fp32(delta)); without delta nothing is written to h_out.
  cc_qkv_rope      every output: four fp32 products, one fp32 add or subtract, one rounding to the dtype; V is a copy; outputs are
                   head-major [heads, T, D].
  cc_silu_mul      at the special points of SILU_SPECIAL (the band below collapses there: no finite error moves 0, inf or NaN).
  cc_softmax_argmax  exp(-inf) = 0 and exp(0) = 1 exactly: a row of one finite logit among -inf is exactly (1.0, 0, ...); a row that
                   holds a NaN, a +inf, or nothing but -inf is all NaN with token 0 (CPU torch.softmax / torch.argmax say the same:
                   restated in the host test).  The token is the first index of the largest of the device's OWN rounded
                   probabilities, the first NaN if there is one (token_of).

BANDED parts.  The device evaluates rsqrtf / expf / v_exp_f32 and sums in an order of its own, so the reference computes the
quantity q behind them in float64 (error ~1e-16, ignored), allows the device's fp32 value any fp32 number in [q(1 - d), q(1 + d)]
and pushes both ends through the operations that follow, which are exact and monotone; lo / hi are the per-element minimum / maximum
(signs of h, w, b flip the direction).  u = 2^-24 is the relative error of one rounded fp32 operation.  Function accuracy: the HIP
math API documentation is not part of this ROCm install, so these are ASSUMPTIONS, taken from the published HIP math tables and the
CDNA ISA guide: expf <= 1 ulp, rsqrtf <= 1 ulp, v_exp_f32 <= 1 ulp — each <= 2u relative.  First-order counts, then doubled for the
second-order terms a first-order count drops:

  rmsnorm  q = rs = 1 / sqrt(mean(h^2) + eps).  The sum of squares (all terms >= 0, so relative errors do not amplify): a per-thread
           chain of up to kNormMaxVec * 8 = 32 fmaf, 6 shuffle adds, 3 adds over the four waves: 41u; the divide by dim and the add of
           eps: 2u -> 43u on the argument; rsqrt halves that: 21.5u; rsqrtf itself: 2u.  23.5u = 2^-19.4; DELTA_NORM = 47u = 2^-18.4.
           Then fp32 h * rs, round to the dtype, fp32 * w, round to the dtype.
  silu     q = s = a / (1 + exp(-a)).  expf: 2u on e, which reaches 1 + e with weight e / (1 + e) <= 1; the add: u; the divide: u.
           4u = 2^-22; DELTA_SILU = 8u = 2^-21.  fp32 overflow of exp(-a) (a < -88.72) is modelled: s = a / inf = -0.  Then round to
           the dtype, fp32 * b, round to the dtype.
  softmax  q = p_i = exp(d_i) / S, d_i = fp32(x_i - M) — ONE IEEE subtraction from the exact global maximum, taken as the device
           takes it, not banded.
           The numerator: exp: 2u; 16-bit types only (v_exp_f32 path): the rounding of d_i * log2(e) and of the fp32 constant
           itself, an absolute error (1 + 1/4) u |d_i| log2(e) on the exponent of two, i.e. 1.25 u |d_i| relative: PER ELEMENT.
           The sum S, folded from 128 per-slice (m_g, s_g) pairs: each term carries the roundings of x - m_g and m_g - M
           (<= u |x - M| together, m_g lies between), for 16-bit also the two products (2.25 u |x - M| in all), weighted by its
           share p_i: c E u with E = sum p_i |d_i| (computed from the reference; E <= ln V), c = 1 (fp32) or 2.25 (16-bit); exp: 2u;
           the per-slice chain of n_t = ceil(slice / 256) adds per thread, 6 shuffle adds, 2 adds: (n_t + 8) u; the rescale by
           exp(m_g - M): 2u and its product u; the fold of 2 + 6 adds: 8u.  The divide: u.
           delta_i = 2 (24 + n_t + c E + [16-bit] 1.25 |d_i|) u — at V = 128256, fp32, E = 3: 62u = 2^-18.  Then round to the dtype.
           Absolute term: an exp result in fp32's subnormal range is 1 ulp ABSOLUTE, and the divide rounds once more: 2^-148 on p.
           16-bit types: v_exp_f32 returns +0 where its result would be subnormal (exp(d_i) < 2^-126), so +0 is a SECOND allowed
           answer there, beside the band (it matters to bf16 only, whose subnormals start at 2^-126; not counted as an open band).
           An element of -inf is exactly 0 whatever the band.

CONDITION on the band: for bf16 and fp16 at most OPEN_SHARE_MAX = 2 % of the elements of any case may have lo != hi (asserted on
every case by the host test from the reference alone); fp32 outputs are a tolerance test by nature.

OUTSIDE the contract, and kept out of the cases: a sum of squares near fp32's maximum (torch.mean and the device overflow in fp32
there, the oracle's twin sums in double and does not), and silu inputs near the overflow threshold of fp32 exp (88.72) other than
the two special points."""
import math

import numpy as np
import torch

import compact_ref as R
from compact_ref import BF, DT_NAME, DTYPES, F32, HF, Case, Op, filled
from helpers import DT_CODE

U = 2.0 ** -24
DELTA_NORM = 47 * U
DELTA_SILU = 8 * U
OPEN_SHARE_MAX = 0.02
LN_F32_MAX = 88.7228391  # exp overflows fp32 above
OK, BAD_ARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -4

# the launchers' constants ...
NORM_THREADS, NORM_MAX_VEC = 256, 4
CAP_ROPE = 8192 * 256  # (token, head, pair) items per grid-stride pass
CAP_SILU = 4096 * 256  # 16-byte vectors per grid-stride pass
SM_BLOCKS, SM_THREADS, SM_REGS = 128, 256, 4  # slices, threads per slice, logits a thread keeps in registers
WS_BYTES = SM_BLOCKS * 8 + 16  # cc_softmax_argmax_workspace_bytes(): 128 float2, one 64-bit key, one ticket, padded
# ... and the source lines they are: the host test fails when one changes
MIRRORED_LINES = {"cc_glue.hip": ["constexpr int kNormThreads = 256;", "constexpr int kNormMaxVec = 4;", "if (nb > 8192) nb = 8192;",
                                  "dim3 grid((unsigned)nb), block(256);", "if (nb > 4096) nb = 4096;", "constexpr int kSmThreads = 256;",
                                  "constexpr int kSmBlocks = 128;", "float x[4];",
                                  "const int per = ((V + kSmBlocks - 1) / kSmBlocks + 7) & ~7;",
                                  "if (dim % vec || dim / vec > kNormThreads * kNormMaxVec) return CC_ERR_UNSUPPORTED;"]}


def vec(dt):
    return 4 if dt == F32 else 8


def slice_len(V):
    return ((V + SM_BLOCKS - 1) // SM_BLOCKS + 7) & ~7


# ------------------------------------------------------------------------------------------------ number formats
def f32(t):
    return t.float().numpy()  # widening is exact


def rnd(a, dt):
    """float32 ndarray -> the values of dt nearest (even) to it, as a float32 ndarray."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a if dt == F32 else torch.from_numpy(a).to(dt).float().numpy()


def tens(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dt)


def ceil32(x):
    """float64 ndarray -> the smallest fp32 >= x."""
    with np.errstate(over="ignore", invalid="ignore"):
        f = x.astype(np.float32)
        low = f.astype(np.float64) < x
        f[low] = np.nextafter(f[low], np.float32(np.inf))
    return f


def floor32(x):
    with np.errstate(over="ignore", invalid="ignore"):
        f = x.astype(np.float32)
        high = f.astype(np.float64) > x
        f[high] = np.nextafter(f[high], np.float32(-np.inf))
    return f


def _band(ends, dt):
    """the outputs of the two ends -> (lo, hi) tensors of dt."""
    with np.errstate(invalid="ignore"):
        return tens(np.minimum(*ends), dt), tens(np.maximum(*ends), dt)


def inside(got, lo, hi):
    """elementwise: got has lo's or hi's bit pattern, or lies strictly between two different ones; NaN only where the band is NaN."""
    g, l, h = R.bits(got), R.bits(lo), R.bits(hi)
    nan = torch.isnan(lo) | torch.isnan(hi)
    between = (lo.double() <= got.double()) & (got.double() <= hi.double()) & (l != h)
    return torch.where(nan, torch.isnan(got), (g == l) | (g == h) | between)


def open_share(lo, hi):
    return float((R.bits(lo) != R.bits(hi)).double().mean()) if lo.numel() else 0.0


def describe(got, lo, hi, n=4):
    bad = (~inside(got, lo, hi)).reshape(-1).nonzero().reshape(-1)
    g, l, h = got.reshape(-1), lo.reshape(-1), hi.reshape(-1)
    return f"{bad.numel()} of {got.numel()} outside, first {[(int(i), float(g[i]), float(l[i]), float(h[i])) for i in bad[:n]]} (index, got, lo, hi)"


# ------------------------------------------------------------------------------------------------ references
def ref_add_rmsnorm(c, scale=1.0):
    dt = c.dtype
    h = f32(c.t["x"])
    out = {}
    if c.t["delta"] is not None:
        h = rnd(h + f32(c.t["delta"]), dt)
        if c.t["h_out"] is not None:
            out["h_out"] = (tens(h, dt),) * 2
    elif c.t["h_out"] is not None:
        out["h_out"] = (c.t["h_out"],) * 2  # not written
    h64 = h.astype(np.float64)
    rs = 1.0 / np.sqrt((h64 * h64).mean(axis=1, keepdims=True) + np.float64(np.float32(c.eps)))
    d = DELTA_NORM * scale
    w = f32(c.t["w"])[None]
    ends = [rnd(rnd(h * r, dt) * w, dt) for r in (ceil32(rs * (1 - d)), floor32(rs * (1 + d)))]
    out["out"] = _band(ends, dt)
    return out


def ref_qkv_rope(c, scale=1.0):
    dt, T, HQ, H, D = c.dtype, c.T, c.HQ, c.H, c.D
    heads = HQ + 2 * H
    x = f32(c.t["qkv"]).reshape(T, heads, D // 2, 2)
    f = f32(c.t["freqs"]).reshape(T, 1, D // 2, 2)
    x0, x1, cs, sn = x[..., 0], x[..., 1], f[..., 0], f[..., 1]
    a0, a1, b0, b1 = x0 * cs, x1 * sn, x1 * cs, x0 * sn  # four rounded fp32 products
    rot = tens(np.stack([a0 - a1, b0 + b1], axis=-1).reshape(T, heads, D), dt)
    raw = c.t["qkv"].view(T, heads, D)
    q, k, v = rot[:, :HQ], rot[:, HQ:HQ + H], raw[:, HQ + H:]
    return {n: (t.transpose(0, 1).contiguous(),) * 2 for n, t in (("q", q), ("k", k), ("v", v))}


def silu64(a):
    """a / (1 + exp(-a)) in float64, the fp32 overflow of exp modelled."""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        e = np.exp(-a)
        e[-a > LN_F32_MAX] = np.inf
        return a / (1.0 + e)


def ref_silu_mul(c, scale=1.0):
    dt = c.dtype
    s = silu64(f32(c.t["a"]).astype(np.float64))
    d = DELTA_SILU * scale
    with np.errstate(invalid="ignore"):
        lo, hi = np.minimum(s * (1 - d), s * (1 + d)), np.maximum(s * (1 - d), s * (1 + d))
        b = f32(c.t["b"])
        ends = [rnd(rnd(e, dt) * b, dt) for e in (ceil32(lo), floor32(hi))]
    return dict(out=_band(ends, dt))


def poisoned(x):
    """a NaN, a +inf, or nothing but -inf: torch.softmax gives an all-NaN row."""
    return bool(np.isnan(x).any() or (x == np.inf).any() or (x == -np.inf).all())


def softmax64(x):
    """-> (d = fp32(x - max) as float64, p) of a row that is not poisoned."""
    with np.errstate(invalid="ignore"):
        d = (x - x.max()).astype(np.float64)
    e = np.exp(d)
    return d, e / e.sum()


def softmax_delta(d, p, V, dt, scale=1.0):
    absd = np.where(np.isfinite(d), -d, 0.0)
    E = float((p * absd).sum())
    n_t = math.ceil(slice_len(V) / SM_THREADS)
    k = 24 + n_t + (1.0 if dt == F32 else 2.25) * E + (0.0 if dt == F32 else 1.25) * absd
    return 2 * k * U * scale


def ref_softmax_argmax(c, scale=1.0):
    dt, V = c.dtype, c.V
    x = f32(c.t["logits"])
    if poisoned(x):
        nan = torch.full((V,), float("nan"), dtype=dt)
        return dict(probs=(nan, nan))
    d, p = softmax64(x)
    delta = softmax_delta(d, p, V, dt, scale)
    A = 2.0 ** -148
    banned = d == -np.inf
    lo = np.where(banned, 0.0, np.maximum(p * (1 - delta) - A, 0.0))
    hi = np.where(banned, 0.0, p * (1 + delta) + A)
    out = dict(probs=(tens(ceil32(lo), dt), tens(floor32(hi), dt)))
    if dt != F32:  # v_exp_f32 returns +0 where exp's result would be subnormal: +0 is a second allowed answer there
        out["probs"] += (torch.from_numpy(np.exp(d) * (1 + delta) < 2.0 ** -126),)
    return out


def token_of(probs):
    """torch.argmax's rule on a row of rounded probabilities: the first NaN, else the first index of the maximum."""
    p = probs.float().numpy()
    nan = np.isnan(p)
    return int(nan.argmax()) if nan.any() else int(p.argmax())


OPS = {
    "add_rmsnorm": Op("cc_add_rmsnorm", ("h_out", "out"),
                      lambda c, p: (p("x"), p("delta"), p("w"), c.T, c.dim, c.eps, c.code, p("h_out"), p("out"), None), ref_add_rmsnorm),
    "qkv_rope": Op("cc_qkv_rope", ("q", "k", "v"),
                   lambda c, p: (p("qkv"), p("freqs"), c.T, c.HQ, c.H, c.D, c.code, p("q"), p("k"), p("v"), None), ref_qkv_rope),
    "silu_mul": Op("cc_silu_mul", ("out",), lambda c, p: (p("a"), p("b"), c.n, c.code, p("out"), None), ref_silu_mul),
    "softmax_argmax": Op("cc_softmax_argmax", ("probs", "idx", "ws"),
                         lambda c, p: (p("logits"), c.V, c.code, p("probs"), p("idx"), p("ws"), c.ws_bytes, None), ref_softmax_argmax),
}


def reference(c, scale=1.0):
    return OPS[c.op].ref(c, scale)


def run_oracle(o, c):
    return R.run_oracle(o, c, OPS)


def run_device(c):
    return R.run_device(c, ops=OPS)


def verdict(c, got, scale=1.0):
    """-> None when every output of the call lies inside the reference (and equals the case's known answer, and the token follows
    the row), else what does not."""
    want = reference(c, scale)
    for n, (lo, hi, *zero_ok) in want.items():
        if n not in got:
            return f"{c.id}: no '{n}'"
        g = got[n]
        if g.shape != lo.shape or g.dtype != lo.dtype:
            return f"{c.id}: '{n}' {tuple(g.shape)} {g.dtype}"
        ok = inside(g, lo, hi)
        if zero_ok:
            ok |= zero_ok[0] & (R.bits(g) == 0)
        if not bool(ok.all()):
            return f"{c.id}: '{n}' {describe(g, lo, hi)}"
    for n, w in getattr(c, "exact", {}).items():
        ok = bool(torch.isnan(got[n]).all()) if bool(torch.isnan(w).all()) else R.same(w, got[n])
        if not ok:
            return f"{c.id}: '{n}' known answer: {R.first_diffs(got[n], w)}"
    if hasattr(c, "exact_np") and not special_ok(c, got["out"]):
        return f"{c.id}: special points: {got['out'].float().tolist()[:9]} for {c.exact_np.tolist()[:9]}"
    if c.op == "softmax_argmax":
        tok = int(got["idx"][0])
        if tok != token_of(got["probs"]):
            return f"{c.id}: token {tok}, the row's first maximum is at {token_of(got['probs'])}"
        if getattr(c, "token", None) is not None and tok != c.token:
            return f"{c.id}: token {tok}, expected {c.token}"
    return None


LADDER = (0.0, 1 / 32, 1 / 16, 1 / 8, 1 / 4, 1 / 2, 1.0)


def fraction_of_delta(c, got):
    """the smallest rung of LADDER at which the band scaled by it still holds the device's outputs (2.0: none)."""
    for s in LADDER:
        if verdict(c, got, s) is None:
            return s
    return 2.0


# ------------------------------------------------------------------------------------------------ cases
def _gen(*key):
    seed = sum((i + 1) * 1000003 * (ord(ch) + 7) for i, ch in enumerate("|".join(map(str, key)))) % (1 << 31)  # (hash() is salted per process)
    return np.random.default_rng(seed), torch.Generator().manual_seed(seed)


NORM_DIMS = (1, 3, 63, 256, 257, 773, 1024)  # in vectors: one; a few; part of a wave idle; one per thread; second register vector; ragged; the cap
NORM_T = (1, 3, 70)


def norm_case(dt, nv, T, with_delta, pass_h=None):
    dim = nv * vec(dt)
    _, gen = _gen("norm", DT_NAME[dt], nv, T, with_delta)
    x = torch.randn(T, dim, generator=gen)
    if T > 1:
        x = x * (2.0 ** ((torch.arange(T) % 16) - 8)).view(T, 1)  # row r scaled by 2^(r % 16 - 8): a row mix-up shows
        x[1] = 0.75  # a constant row
        x[T - 1] = 0.01 * x[T - 1]
        x[T - 1, dim // 2] = 1000.0  # one large element among small ones
    x = x.to(dt)
    delta = None
    if with_delta:
        delta = (0.5 * torch.randn(T, dim, generator=gen)).to(dt)
        if T > 1:
            delta[0] = -x[0]  # h = +0 everywhere
    elif T > 1:
        x[0] = 0.0
    w = torch.randn(dim, generator=gen).to(dt)  # both signs
    pass_h = with_delta if pass_h is None else pass_h
    t = dict(x=x, delta=delta, w=w, h_out=filled((T, dim), dt) if pass_h else None, out=filled((T, dim), dt))
    return Case("add_rmsnorm", f"add_rmsnorm-{DT_NAME[dt]}-T{T}-dim{dim}-{'delta' if with_delta else 'plain'}{'' if pass_h == with_delta else '-h' + str(int(pass_h))}",
                t, T=T, dim=dim, eps=1e-5, dtype=dt, code=DT_CODE[dt])


def cases_add_rmsnorm():
    for dt in DTYPES:
        for nv in NORM_DIMS:
            for T in NORM_T:
                for with_delta in (False, True):
                    yield norm_case(dt, nv, T, with_delta)
        yield norm_case(dt, 3, 3, False, pass_h=True)  # h_out handed in without delta: stays as it was
        yield norm_case(dt, 3, 3, True, pass_h=False)  # delta without h_out


ROPE_SHAPES = ((1, 1, 1, 2), (3, 6, 3, 6), (5, 28, 4, 128), (2, 8, 8, 64), (7, 4, 2, 256))
ROPE_SECOND_PASS = (4097, 4, 2, 128)


def rope_case(dt, T, HQ, H, D, table, tag=""):
    from cold_compress_amd.harness.model import precompute_freqs_cis

    rng, gen = _gen("rope", DT_NAME[dt], T, HQ, H, D, table)
    heads = HQ + 2 * H
    qkv = torch.randn(T, heads * D, generator=gen).to(dt)
    if table == "rope":
        freqs = precompute_freqs_cis(4096, D, 500000, dt)[torch.from_numpy(rng.integers(0, 4096, T))]
    elif table == "random":  # non-unit (c, s): a unit or zero-angle table hides swaps
        freqs = (torch.rand(T, D // 2, 2, generator=gen) * 3 - 1.5).to(dt)
    else:  # "identity": c = 1, s = 0
        freqs = torch.tensor([1.0, 0.0]).repeat(T, D // 2, 1).to(dt)
        qkv = torch.arange(T * heads * D, dtype=torch.float32).view(T, heads * D).to(dt)
        assert torch.equal(qkv.float().reshape(-1), torch.arange(T * heads * D, dtype=torch.float32))  # exactly representable
    t = dict(qkv=qkv, freqs=freqs.contiguous(), q=filled((HQ, T, D), dt), k=filled((H, T, D), dt), v=filled((H, T, D), dt))
    return Case("qkv_rope", f"qkv_rope-{DT_NAME[dt]}-T{T}-HQ{HQ}-H{H}-D{D}-{table}{tag}", t, T=T, HQ=HQ, H=H, D=D, dtype=dt, code=DT_CODE[dt])


def rope_layout_case(dt):
    """every input element holds its flat index, c = 1, s = 0: the outputs are a pure permutation (stated here by indexing)."""
    T, HQ, H, D = 3, 2, 1, 8
    c = rope_case(dt, T, HQ, H, D, "identity")
    src = c.t["qkv"].view(T, HQ + 2 * H, D)
    c.exact = dict(q=src[:, :HQ].transpose(0, 1).contiguous(), k=src[:, HQ:HQ + H].transpose(0, 1).contiguous(),
                   v=src[:, HQ + H:].transpose(0, 1).contiguous())
    return c


def cases_qkv_rope():
    for dt in DTYPES:
        for shape in ROPE_SHAPES:
            for table in ("rope", "random"):
                yield rope_case(dt, *shape, table)
        yield rope_layout_case(dt)
        yield rope_case(dt, *ROPE_SECOND_PASS, "random", tag="-second-pass")


SILU_SPECIAL = ((0.0, 1.5, "+0 * b"), (0.0, -1.5, "+0 * b"), (-100.0, 1.5, "-0 * b"), (-100.0, -1.5, "-0 * b"), (np.inf, 1.5, "+inf * b"),
                (np.inf, -1.5, "+inf * b"), (-np.inf, 1.5, "NaN"), (np.nan, 1.5, "NaN"), (np.inf, 0.0, "NaN"))


def silu_special_answer(a, b):
    """the known answers of SILU_SPECIAL, stated without the silu formula."""
    b = np.float32(b)
    with np.errstate(invalid="ignore"):
        if a == 0.0:
            return np.float32(0.0) * b
        if a == -100.0:
            return np.float32(-0.0) * b
        if a == np.inf and b != 0:
            return np.float32(np.inf) * b
    return np.float32(np.nan)


def silu_case(dt, n, kind="normal", tag=""):
    _, gen = _gen("silu", DT_NAME[dt], n, kind)
    if kind == "special":
        reps = -(-n // len(SILU_SPECIAL))
        a = torch.tensor([s[0] for s in SILU_SPECIAL] * reps, dtype=torch.float32)[:n].to(dt)
        b = torch.tensor([s[1] for s in SILU_SPECIAL] * reps, dtype=torch.float32)[:n].to(dt)
    else:
        a = ((torch.rand(n, generator=gen) * 160 - 80) if kind == "wide" else 3 * torch.randn(n, generator=gen)).to(dt)
        b = torch.randn(n, generator=gen).to(dt)
    c = Case("silu_mul", f"silu_mul-{DT_NAME[dt]}-n{n}-{kind}{tag}", dict(a=a, b=b, out=filled((n,), dt)), n=n, dtype=dt, code=DT_CODE[dt])
    if kind == "special":
        want = np.array([silu_special_answer(s[0], s[1]) for s in SILU_SPECIAL] * reps, dtype=np.float32)[:n]
        c.exact_np = want  # NaN where NaN, else the bit pattern: checked by special_ok
    return c


def special_ok(c, out):
    w, g = tens(c.exact_np, c.dtype), out
    nan = torch.isnan(w)
    return bool((torch.isnan(g) == nan).all()) and bool((R.bits(g)[~nan] == R.bits(w)[~nan]).all())


def silu_sizes(dt):
    v = vec(dt)
    return (1, v - 1, v, v + 1, 256 * v + 3)


def silu_second_pass_n(dt):
    return (CAP_SILU + 1) * vec(dt) + vec(dt) - 1


def cases_silu_mul():
    for dt in DTYPES:
        for n in silu_sizes(dt):
            for kind in ("normal", "wide"):
                yield silu_case(dt, n, kind)
        yield silu_case(dt, len(SILU_SPECIAL), "special")  # the scalar tail (f32: two vectors and a tail)
        yield silu_case(dt, 4 * len(SILU_SPECIAL), "special")  # ... and the vector loop
        yield silu_case(dt, silu_second_pass_n(dt), "wide", tag="-second-pass")


SM_V = (1, 7, 8, 9, 128, 1023, 1024, 1025, 32000, 128256, 131072, 131080, 151936, 262144)
NINF = -float("inf")


def sm_case(dt, V, logits, tag, token=None, exact=None):
    t = dict(logits=logits.to(dt), probs=filled((V,), dt), idx=filled((1,), torch.int32), ws=filled((WS_BYTES,), torch.uint8))
    c = Case("softmax_argmax", f"softmax_argmax-{DT_NAME[dt]}-V{V}-{tag}", t, V=V, ws_bytes=WS_BYTES, dtype=dt, code=DT_CODE[dt], token=token)
    if exact is not None:
        c.exact = dict(probs=exact.to(dt))
    return c


def _logits(V, sigma, *key):
    _, gen = _gen("sm", V, sigma, *key)
    return torch.randn(V, generator=gen) * sigma


def sm_positions(V):
    """{name: index} of the places a dominated maximum is put at."""
    per = slice_len(V)
    n = -(-V // per)  # slices that hold anything
    mid = n // 2
    pos = {"first": 0, "last": V - 1}
    if n > 2:
        pos["slice-first"] = mid * per
        pos["slice-last"] = min(V, (mid + 1) * per) - 1
    if per > SM_REGS * SM_THREADS:
        pos["reload-first"] = mid * per + SM_REGS * SM_THREADS  # the first id a thread reads again instead of keeping
        pos["reload-last"] = min(V, (mid + 1) * per) - 1
    return pos


def cases_softmax_random():
    for V in SM_V:
        for dt in DTYPES:
            for sigma in (3, 12):
                yield sm_case(dt, V, _logits(V, sigma, "random"), f"sigma{sigma}")


def cases_softmax_maxima():
    for i, V in enumerate(SM_V):
        per = slice_len(V)
        n = -(-V // per)
        dts = DTYPES if V in (128, 128256, 151936) else (DTYPES[i % 3],)
        for dt in dts:
            for name, at in sm_positions(V).items():
                x = _logits(V, 3, "dominated").to(dt).float()
                x[at] = float(x.max()) + 20.0
                yield sm_case(dt, V, x, f"max-at-{name}-{at}", token=at)
            if n > 4:  # equal maxima in two different slices: the lower index wins, whichever workgroup arrives first
                x = _logits(V, 3, "tie2").to(dt).float()
                a, b = 1 * per + per // 2, (n - 2) * per + 1
                x[a] = x[b] = float(x.max()) + 20.0
                yield sm_case(dt, V, x, f"tie-slices-{a}-{b}", token=a)
            if per > 261:  # equal maxima 256 apart inside one slice: the same thread sees both
                x = _logits(V, 3, "tie256").to(dt).float()
                a = (n // 2) * per + 5
                x[a] = x[a + 256] = float(x.max()) + 20.0
                yield sm_case(dt, V, x, f"tie-256-apart-{a}", token=a)
    # two logits one bf16 step apart: their probabilities round to one value, the FIRST index wins although the second is larger
    x = torch.full((1024,), -5.0)
    x[10], x[500] = 2.0 ** -10, 2.0 ** -10 + 2.0 ** -17
    yield sm_case(BF, 1024, x, "near-tie-rounds-equal", token=10)


def cases_softmax_inf():
    nan = float("nan")
    for dt, V in ((F32, 128), (BF, 128256)):
        per = slice_len(V)
        n = -(-V // per)
        base = _logits(V, 3, "inf").to(dt).float()

        def banned(lo, hi, tag):
            x = base.clone()
            x[lo:hi] = NINF
            return sm_case(dt, V, x, tag)

        yield banned(V // 3, V // 3 + 1, "one-inf")
        yield banned(0, per, "first-slice-inf")
        yield banned((n // 2) * per, (n // 2 + 1) * per, "middle-slice-inf")
        yield banned((n - 1) * per, V, "last-slice-inf")
        if V == 128256:
            yield banned(128000, V, "special-tokens-inf")  # Llama-3's reserved ids: the whole last slice and more
        x = base.clone()
        for g in range(0, n, 2):
            x[g * per:(g + 1) * per] = NINF
        yield sm_case(dt, V, x, "every-second-slice-inf")
        # known answers
        at = (n // 2) * per + 3
        one = torch.full((V,), NINF)
        one[at] = -3.25
        want = torch.zeros(V)
        want[at] = 1.0
        yield sm_case(dt, V, one, "one-finite", token=at, exact=want)
        all_nan = torch.full((V,), nan)
        yield sm_case(dt, V, torch.full((V,), NINF), "all-inf", token=0, exact=all_nan)
        x = base.clone()
        x[V - 2] = float("inf")
        yield sm_case(dt, V, x, "plus-inf", token=0, exact=all_nan)
        x = base.clone()
        x[V // 2] = nan
        yield sm_case(dt, V, x, "nan", token=0, exact=all_nan)
        x = base.clone()
        x[per:2 * per] = NINF
        x[per + 2] = nan
        yield sm_case(dt, V, x, "nan-in-inf-slice", token=0, exact=all_nan)


def cases_softmax_argmax():
    yield from cases_softmax_random()
    yield from cases_softmax_maxima()
    yield from cases_softmax_inf()


CASES = dict(add_rmsnorm=cases_add_rmsnorm, qkv_rope=cases_qkv_rope, silu_mul=cases_silu_mul, softmax_argmax=cases_softmax_argmax)
BANDED = dict(add_rmsnorm="out", silu_mul="out", softmax_argmax="probs")  # the output a band applies to


# ------------------------------------------------------------------------------------------------ refusals
def refusals():
    """[(what, case, the device's answer, the oracle twin's answer)].  Every buffer is large enough for the refused shape.  The
    twin knows neither vector widths, nor the register cap, nor a workspace: it answers CC_OK (and computes) where the device
    refuses for one of those."""
    out = []
    for dt in DTYPES:
        v, name = vec(dt), DT_NAME[dt]
        nc = norm_case(dt, 3, 2, True)
        ragged = norm_case(dt, 3, 2, True).replace(dim=3 * v - 1)
        over = norm_case(dt, NORM_THREADS * NORM_MAX_VEC + 1, 1, True)
        assert over.dim == NORM_THREADS * NORM_MAX_VEC * v + v
        out += [(f"cc_add_rmsnorm {name} dim % VEC != 0", ragged, UNSUPPORTED, OK), (f"cc_add_rmsnorm {name} dim = cap + VEC", over, UNSUPPORTED, OK)]
        if dt == BF:
            out += [("cc_add_rmsnorm x = NULL", nc.replace(t=dict(x=None)), BAD_ARG, BAD_ARG),
                    ("cc_add_rmsnorm weight = NULL", nc.replace(t=dict(w=None)), BAD_ARG, BAD_ARG),
                    ("cc_add_rmsnorm out = NULL", nc.replace(t=dict(out=None)), BAD_ARG, BAD_ARG),
                    ("cc_add_rmsnorm T = 0", nc.replace(T=0), BAD_ARG, BAD_ARG), ("cc_add_rmsnorm T < 0", nc.replace(T=-2), BAD_ARG, BAD_ARG),
                    ("cc_add_rmsnorm dim = 0", nc.replace(dim=0), BAD_ARG, BAD_ARG), ("cc_add_rmsnorm dtype 3", nc.replace(code=3), BAD_ARG, BAD_ARG)]
    rc = rope_case(HF, 3, 2, 1, 8, "random")
    out += [(f"cc_qkv_rope {n} = NULL", rc.replace(t={n: None}), BAD_ARG, BAD_ARG) for n in ("qkv", "freqs", "q", "k", "v")]
    out += [("cc_qkv_rope T = 0", rc.replace(T=0), BAD_ARG, BAD_ARG), ("cc_qkv_rope HQ = 0", rc.replace(HQ=0), BAD_ARG, BAD_ARG),
            ("cc_qkv_rope H < 0", rc.replace(H=-1), BAD_ARG, BAD_ARG), ("cc_qkv_rope odd D", rc.replace(D=7), BAD_ARG, BAD_ARG),
            ("cc_qkv_rope D = 0", rc.replace(D=0), BAD_ARG, BAD_ARG), ("cc_qkv_rope dtype -1", rc.replace(code=-1), BAD_ARG, BAD_ARG)]
    sc = silu_case(F32, 9)
    out += [(f"cc_silu_mul {n} = NULL", sc.replace(t={n: None}), BAD_ARG, BAD_ARG) for n in ("a", "b", "out")]
    out += [("cc_silu_mul n = 0", sc.replace(n=0), BAD_ARG, BAD_ARG), ("cc_silu_mul n < 0", sc.replace(n=-9), BAD_ARG, BAD_ARG),
            ("cc_silu_mul dtype 7", sc.replace(code=7), BAD_ARG, BAD_ARG)]
    mc = sm_case(BF, 300, _logits(300, 3, "refusal"), "refusal")
    out += [(f"cc_softmax_argmax {n} = NULL", mc.replace(t={n: None}), BAD_ARG, BAD_ARG) for n in ("logits", "probs", "idx")]
    out += [("cc_softmax_argmax workspace = NULL", mc.replace(t=dict(ws=None)), BAD_ARG, OK),
            ("cc_softmax_argmax V = 0", mc.replace(V=0), BAD_ARG, BAD_ARG), ("cc_softmax_argmax V < 0", mc.replace(V=-300), BAD_ARG, BAD_ARG),
            ("cc_softmax_argmax dtype 3", mc.replace(code=3), BAD_ARG, BAD_ARG),
            ("cc_softmax_argmax short workspace", mc.replace(ws_bytes=WS_BYTES - 24), WORKSPACE, OK),
            ("cc_softmax_argmax no workspace bytes", mc.replace(ws_bytes=0), WORKSPACE, OK)]
    return out
