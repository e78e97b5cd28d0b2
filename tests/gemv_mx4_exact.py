"""Known-answer inputs for the MXFP4 decode GEMV (cc_gemv_fused_mx4), in the spirit of tests/gemv_exact.py: CPU tensors only.

The kernel chooses its own summation order, so on random data only a tolerance can be asserted.  The inputs made here have an answer
that does NOT depend on the order:

  * the input vector, norm weights and biases are small integers; every scale byte is >= 128 (scale 2, 4 or 8), so every weight
    e2m1(code) * scale is an integer (0.5 * 2 = 1, 1.5 * 2 = 3) and every product and partial sum, in any order, is an integer.  The
    generator asserts sum_k |term_k| < 2^24 per row: exact in fp32;
  * a repair pass nudges a few codes of every row, in blocks of scale 2 and on columns of unit input, until the row's exact result
    is an integer with |y| < 256 (bf16 holds it exactly; strictly inside: at 256 a result off by one would round back);
  * RMSNorm prologue: x + delta = +-1 element-wise, eps = 0, so the normalised input is the integer +-norm_w (tests/gemv_exact.py);
  * SwiGLU: the gate value t comes from gemv_exact.gate_values (silu(t) at least 2^-18 relative away from every bf16 rounding
    midpoint), t3 is never 0, and rnd(silu(t)) * t3 is an exact fp32 product;
  * RoPE rows stay below 64 in magnitude and the table holds integers in [-2, 2], so the rotated value is an exact integer < 256.

The expected output is therefore ONE bit pattern, computed here in int64 / float64; the device must equal it bit for bit.

Also here: a Python mirror of the launcher's choice of template instantiation (cc_gemv_mx4.hip launch_gemv_mx4 / pick_mx4_cfg), the
default-reachable instantiations and the case list tests/test_gpu_gemv_mx4_exact.py runs (tests/test_mx4_host.py checks on the CPU
that the list reaches every one of them and that the mirrored source lines are still there)."""
import types

import numpy as np
import torch

from gemv_exact import BF, EXACT_RANGE, GATE_MARGIN, bits, gate_values, midpoint_margin, round_to, silu64, to_dt  # noqa: F401

E2M1 = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
R = EXACT_RANGE[BF]  # 256


# ------------------------------------------------------------------------------------------------ the launcher's choice, mirrored
def geometry(pair, N, K):
    """(form, N, K) -> the switch key of launch_gemv_mx4 and the numbers the row loop depends on: a copy of MIRRORED_LINES."""
    nseg = (K // 32 + 63) // 64
    ws = 4 if nseg >= 3 else nseg
    nstep = (nseg + ws - 1) // ws
    if nstep <= 1:
        rb, cu, cap = (4, 1, 512) if pair else (4, 1, 1024)
    else:
        rb, cu, cap = (2, 2, 512) if pair else (4, 2, 512)
    xs = 1 if nstep <= 1 else 2 if nstep <= 2 else 4
    assert nstep <= 4 and cu <= xs
    key = (100000 if pair else 0) + ws * 10000 + xs * 1000 + rb * 10 + cu
    return types.SimpleNamespace(key=key, rows=rb * (4 // ws), cap=cap, cu=cu, xs=xs, ws=ws, nstep=nstep)


MIRRORED_LINES = [
    "const int nseg = (a.K / 32 + 63) / 64;", "const int ws = nseg >= 3 ? 4 : nseg;", "const int nstep = (nseg + ws - 1) / ws;",
    "if (nstep <= 1) return a.W3 != nullptr ? Mx4Cfg{4, 1, 512} : Mx4Cfg{4, 1, 1024};",
    "return a.W3 != nullptr ? Mx4Cfg{2, 2, 512} : Mx4Cfg{4, 2, 512};", "const int xs = nstep <= 1 ? 1 : nstep <= 2 ? 2 : 4;",
    "const int key = (a.W3 ? 100000 : 0) + ws * 10000 + xs * 1000 + c.rb * 10 + c.cu;", "constexpr int RW = RB * (kMx4Waves / WS);",
    "constexpr int kMx4Threads = 256;",
]

# the instantiations a default launch (no CC_GEMV_MX4_CFG) can select
DEFAULT_KEYS = {11041, 21041, 41041, 42042, 44042, 111041, 121041, 141041, 142022, 144022}


# ------------------------------------------------------------------------------------------------ the integer reference
def weights_int(codes, sbytes):
    """int64 [N, K]: e2m1(code) * 2^(byte - 127), an integer for every byte >= 128."""
    mag = E2M1[(codes & 7).astype(np.int64)]
    val = np.where(codes & 8, -mag, mag)
    w = val * np.ldexp(1.0, sbytes.astype(np.int64) - 127).repeat(32, axis=1)
    assert np.array_equal(w, np.rint(w))
    return w.astype(np.int64)


def dot_exact(codes, sbytes, xin, block=512):
    """-> (acc int64 [N], abs_sum int64 [N]): every row's exact dot product with xin and the sum of the magnitudes of its terms, in
    float64 on integers far below 2^53."""
    xt = torch.from_numpy(xin.astype(np.float64))
    N = codes.shape[0]
    acc, tot = np.empty(N, np.int64), np.empty(N, np.int64)
    for r0 in range(0, N, block):
        w = torch.from_numpy(weights_int(codes[r0:r0 + block], sbytes[r0:r0 + block]).astype(np.float64))
        acc[r0:r0 + block] = (w @ xt).numpy().astype(np.int64)
        tot[r0:r0 + block] = (w.abs() @ xt.abs()).numpy().astype(np.int64)
    return acc, tot


def _value_to_code(v2):
    """integer weight value at scale 2 (in +-{0, 1, 2, 3, 4, 6, 8, 12}) -> e2m1 code."""
    return _CODE_OF[np.abs(v2)] | ((v2 < 0).astype(np.uint8) << 3)


_CODE_OF = np.zeros(13, np.uint8)
_CODE_OF[[0, 1, 2, 3, 4, 6, 8, 12]] = np.arange(8, dtype=np.uint8)
_GRID2 = np.array(sorted({s * v for v in (0, 1, 2, 3, 4, 6, 8, 12) for s in (-1, 1)}), np.int64)


def reserve_columns(xin):
    """the columns of block 0 with unit input: their codes start at 0 and finish the repair in unit steps (block 0 has scale 2 in
    every row)."""
    return np.nonzero(np.abs(xin[:32]) == 1)[0]


def _repair(codes, sbytes, xin, cur, tgt, rng):
    """move codes of every row, on columns of unit input inside blocks of scale 2, until its dot product with xin is tgt: a coarse
    pass over random columns (any value of the grid, leaving |r| <= 2), then unit steps in [-4, 4] on the reserve columns."""
    N, K = codes.shape
    res = reserve_columns(xin)
    colmask = (np.abs(xin) == 1)[None, :] & (sbytes == 128).repeat(32, axis=1)  # [N, K]
    colmask[:, :32] = False
    r = (tgt - cur).astype(np.int64)
    for k in rng.permutation(K):
        live = np.nonzero((np.abs(r) > 2) & colmask[:, k])[0]
        if not len(live):
            if (np.abs(r) <= 2).all():
                break
            continue
        c = codes[live, k]
        mag = (E2M1[(c & 7).astype(np.int64)] * 2).astype(np.int64)
        v = np.where(c & 8, -mag, mag)
        want = v + r[live] * int(xin[k])  # x = +-1: 1 / x = x
        new = _GRID2[np.abs(_GRID2[None, :] - want[:, None]).argmin(1)]
        codes[live, k] = _value_to_code(new)
        r[live] -= (new - v) * int(xin[k])
    for k in res:  # (their codes are 0)
        step = np.clip(r * int(xin[k]), -4, 4)
        codes[:, k] = np.where(step != 0, _value_to_code(step), codes[:, k])
        r -= step * int(xin[k])
    assert not r.any(), "the repair pass could not bring every row to its target"


def make_case(N, K, form="plain", seed=0):
    """One exact case: CPU tensors in the layout glue.gemv_fused takes and the expected output `y` (and `h`).  form: '+'-joined subset
    of norm, delta, pair, rope, bias ('plain' = none)."""
    f = set(form.split("+")) - {"plain"}
    assert f <= {"norm", "delta", "pair", "rope", "bias"} and K % 32 == 0 and K * 2 <= 65536
    c = types.SimpleNamespace(N=N, K=K, form=form, norm="norm" in f, delta="delta" in f, pair="pair" in f, rope="rope" in f,
                              has_bias="bias" in f)
    assert not (c.delta and not c.norm) and not (c.pair and (c.rope or c.has_bias))
    rng = np.random.default_rng([seed, N, K, sum(map(ord, "mx4" + form))])
    # ---- the input vector
    c.h_i = c.delta_i = c.nw_i = None
    if c.norm:
        c.h_i = rng.choice(np.array([-1, 1]), K)
        c.x_i = rng.integers(-3, 4, K) if c.delta else c.h_i.copy()
        if c.delta:
            c.delta_i = c.h_i - c.x_i
        c.nw_i = rng.choice(np.array([1, -1, 2, -2, 3, -3]), K, p=[.35, .35, .1, .1, .05, .05] if K >= 256 else [.5, .5, 0, 0, 0, 0])
        c.nw_i[0], c.nw_i[K - 1] = 1, -1
        c.xin = c.h_i * c.nw_i
    else:
        c.x_i = rng.choice(np.array([-1, 0, 1]), K, p=[7 / 16, 1 / 8, 7 / 16])
        c.x_i[0], c.x_i[K - 1] = 1, -1
        c.xin = c.x_i.copy()
    c.bias_i = rng.integers(-8, 9, N) if c.has_bias else None
    c.freqs_i, c.rope_rows, c.hd = None, 0, 0
    if c.rope:
        g = geometry(False, N, K)
        c.hd = 2 if N < g.rows + 2 or seed % 2 else g.rows + 2
        c.rope_rows = c.hd * max(1, min(N // c.hd, 3) - (1 if N // c.hd > 1 and N % c.hd == 0 else 0))
        assert c.rope_rows <= N, "RoPE needs two rows at least"
        c.freqs_i = rng.integers(-2, 3, (c.hd // 2, 2))
        c.freqs_i[0] = (1, 2)
        c.freqs_i[(c.freqs_i == 0).all(1), 0] = -1  # (0, 0) would hide a row pair
    # ---- codes and scale bytes
    mats = []
    for which in range(2 if c.pair else 1):
        codes = rng.integers(0, 16, (N, K)).astype(np.uint8)  # every code, -0 (8) included
        sbytes = rng.choice(np.array([128, 129, 130], np.uint8), (N, K // 32), p=[.5, .3, .2])
        sbytes[:, 0] = sbytes[:, -1] = 128  # the first and last block carry repairable columns (xin = +-1 at columns 0 and K - 1)
        res = reserve_columns(c.xin)
        codes[:, res] = 0
        cur, _ = dot_exact(codes, sbytes, c.xin)
        limit = np.full(N, R - 1, np.int64)
        if c.rope:
            limit = np.where(np.arange(N) < c.rope_rows, R // 4 - 1, limit)
        if c.has_bias:
            limit -= np.abs(c.bias_i)
        if K < 256:  # one block: the reserve columns are all there is
            assert K == 32 and not cur.any() and len(res) >= 16
            limit = np.minimum(limit, 4 * len(res))
        if c.pair and which == 0:
            gv = gate_values(BF)
            gv = gv[np.abs(gv) <= limit.min()]
            tgt = gv[rng.integers(0, len(gv), N)]
        else:
            tgt = np.sign(cur + (cur == 0)) * (limit - rng.integers(0, np.maximum(limit // 4, 1) + 1, N))
            edge = np.arange(N) % 5 == 0  # some rows sit exactly on the edge of the range handed out
            tgt = np.where(edge, np.where(cur < 0, -limit, limit), tgt)
            if c.pair:
                tgt = np.where(tgt == 0, 1, tgt)
        _repair(codes, sbytes, c.xin, cur, tgt, rng)
        mats.append((codes, sbytes))
    c.codes, c.sbytes = mats[0]
    c.codes3, c.sbytes3 = mats[1] if c.pair else (None, None)
    c.y = to_dt(BF, exact_output(c, check=True))
    c.h = to_dt(BF, c.h_i) if c.norm else None
    _tensors(c)
    return c


def exact_output(c, check=True):
    """The unique correct output of case c from its integer fields -> float64 [N]; with check every guarantee is asserted."""
    rnd = (lambda v: round_to(BF, v)) if check else (lambda v: torch.from_numpy(np.asarray(v, np.float64)).to(BF).double().numpy())
    acc, tot = dot_exact(c.codes, c.sbytes, c.xin)
    c.acc, c.abs_sum = acc, tot
    if check:
        assert (tot < 2 ** 24).all(), "a partial sum could leave fp32's exact integers"
        assert (np.abs(acc) < R).all(), "a row's dot product left the exact range"
    v = rnd(acc.astype(np.float64))
    if c.bias_i is not None:
        v = v + c.bias_i
        assert not check or (np.abs(v) < R).all()
        v = rnd(v)
    if c.pair:
        acc3, tot3 = dot_exact(c.codes3, c.sbytes3, c.xin)
        c.acc3 = acc3
        if check:
            assert (tot3 < 2 ** 24).all() and (np.abs(acc3) < R).all() and (acc3 != 0).all()
            assert np.isin(v, gate_values(BF)).all() and (midpoint_margin(BF, silu64(v)) >= GATE_MARGIN).all()
        v = rnd(rnd(silu64(v)) * rnd(acc3.astype(np.float64)))
    if c.freqs_i is not None:
        rr, hd = c.rope_rows, c.hd
        fq = c.freqs_i.astype(np.float64)
        pr = (np.arange(rr) % hd) >> 1
        cs, sn = fq[pr, 0], fq[pr, 1]
        part = v[:rr].reshape(-1, 2)[:, ::-1].reshape(-1)  # the pair partner
        sign = np.where(np.arange(rr) & 1, 1.0, -1.0)
        rot = v[:rr] * cs + sign * part * sn
        assert not check or (np.abs(rot) < R).all()
        v = np.concatenate([rnd(rot), v[rr:]])
    return v


def pack(codes):
    return torch.from_numpy(np.ascontiguousarray(codes[:, 0::2] | (codes[:, 1::2] << 4)))


def _tensors(c):
    iv = lambda a: to_dt(BF, a) if a is not None else None  # noqa: E731
    c.x, c.delta_t, c.nw, c.bias, c.freqs = iv(c.x_i), iv(c.delta_i), iv(c.nw_i), iv(c.bias_i), iv(c.freqs_i)
    c.W, c.scales = pack(c.codes), torch.from_numpy(np.ascontiguousarray(c.sbytes))
    c.W3 = pack(c.codes3) if c.pair else None
    c.scales3 = torch.from_numpy(np.ascontiguousarray(c.sbytes3)) if c.pair else None


# ------------------------------------------------------------------------------------------------ the cases the GPU file runs
# one block; one segment -+ a chunk; WS = 2; the WS = 2 / 4 boundary + a chunk; WS = 4 full; + a chunk (two steps); the 8B w2; two
# full steps; + a chunk (three steps, XS = 4); the 70B w2 (four steps); the limit
K_VALUES = (32, 2016, 2048, 2080, 4096, 4128, 6144, 8192, 8224, 14336, 16384, 16416, 28672, 32768)
PLAIN_FORMS = ("plain", "norm+delta", "rope+bias", "norm+delta+rope+bias")
PAIR_FORMS = ("pair", "norm+delta+pair")


def gpu_cases():
    """[(id, N, K, form, seed)]: every K edge x form with 1, rows-per-round -+ 1, 38 (no multiple of any rows-per-round) and
    2 rounds + 1 rows, and one count past cap x rows-per-round at each instantiation's smallest K (two rounds of the row loop)."""
    out, seen, n = [], set(), 0
    for K in K_VALUES:
        for form in PLAIN_FORMS + PAIR_FORMS:
            pair = "pair" in form
            g = geometry(pair, 1, K)
            N = 2 * g.rows + 3 if "rope" in form else (1, g.rows - 1, g.rows + 1, 38, 2 * g.rows + 1)[n % 5]
            n += 1
            out.append((N, K, form))
            if g.key not in seen and form in ("norm+delta+rope+bias", "norm+delta+pair"):
                seen.add(g.key)  # K ascends: this is the instantiation's smallest K
                out.append((g.cap * g.rows + 1, K, form))
    return [(f"mx4-N{N}-K{K}-{form}", N, K, form, 300 + i) for i, (N, K, form) in enumerate(out)]


def case_keys():
    return {geometry("pair" in form, N, K).key for (_, N, K, form, _) in gpu_cases()}
