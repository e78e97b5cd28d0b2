"""Known-answer inputs for the three decode GEMVs (cc_gemv_fused, cc_gemv_fused_w8, cc_gemv_fused_w4): CPU tensors only.

The kernels choose their own summation order, so on random data only a tolerance can be asserted, and at K = 4096 in bf16 that
tolerance (2 ulp of the largest output, about 0.09) is wider than one dropped weight (about 0.05).  The inputs made here have an
answer that does NOT depend on the order:

  * weights (codes) and the input vector are small integers, so every product and every partial sum, in any order, is an integer
    (int4: an integer multiple of the smallest group scale, which is >= 1) of magnitude < 2^24: exact in fp32.  The generator
    asserts sum_k |term_k| < 2^24 per row; for int4 it asserts it for the kernel's factored form
    s (sum x (128 + q) - 136 Sx) + z Sx, whose terms are far larger than those of the plain dot product;
  * a repair pass moves a few codes of every row until the row's exact result is an integer the model dtype holds exactly:
    |y| < 256 (bf16), < 2048 (fp16), < 2^24 (fp32).  Strictly inside: at |y| = 256 a bf16 result that is off by one (257) would
    round back to 256;
  * RMSNorm prologue: x + delta = +-1 element-wise, eps = 0, so the mean square is exactly 1, h * rsqrt(1) lies within an fp32 ulp
    of +-1 and rounds to +-1 in bf16 / fp16, and the normalised input is the integer +-norm_w.  (fp32 keeps rsqrtf's ulp: see `tol`);
  * SwiGLU: the gate value t is an integer whose float64 silu(t) is at least 2^-18 (relative) away from every rounding midpoint of
    the dtype (16 x an fp32 expf / divide error of 4 ulp) and normal in fp16, so rnd(silu(t)) is unique; rnd(silu) * t3 is an exact
    fp32 product of two <= 11-bit significands, so the output rounding is unique too.  t and t3 are never 0 (a zero factor would
    hide the other matrix);
  * int8: per-row scales are powers of two; int4: group scales are powers of two >= 1 and zeros integer multiples of the scale.

The expected output is therefore ONE bit pattern, computed here in int64 / float64; a dropped, doubled or misaddressed weight moves
an integer by at least 1 and changes the pattern.

Also here: a Python mirror of the three launchers' choice of template instantiation, the default-reachable instantiations per
kernel file, and the case list tests/test_gpu_gemv_exact.py runs (tests/test_gemv_exact_host.py checks, on the CPU, that the list
reaches every one of them)."""
import types

import numpy as np
import torch

BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32
DT_NAME = {BF: "bf16", HF: "f16", F32: "f32"}
EXACT_RANGE = {BF: 256, HF: 2048, F32: 1 << 24}  # |integer| <= this is held exactly; generated rows stay strictly inside
SIG_BITS = {BF: 8, HF: 11, F32: 24}
MIN_NORMAL = {BF: 2.0 ** -126, HF: 2.0 ** -14, F32: 2.0 ** -126}
MAX_FINITE = {BF: 3.38e38, HF: 65504.0, F32: 3.4e38}
ELEM = {BF: 2, HF: 2, F32: 4}
GATE_MARGIN = 2.0 ** -18
KERNELS = ("16", "w8", "w4")
DTYPES = {"16": (BF, HF, F32), "w8": (BF, HF), "w4": (BF,)}


# ------------------------------------------------------------------------------------------------ the launchers' choices, mirrored
def geometry(kernel, pair, N, K, dt=BF):
    """(form, dtype, N, K) -> the switch key of the launcher and the numbers the row loop depends on.  Copies, line for line:
    cc_gemv.hip pick_cfg (the `const int nseg = ...` line to `return c;`) and launch_gemv (`const int xs = ...`, `const int key = ...`);
    cc_gemv_w8.hip pick_w8_cfg (`if (nstep <= 1) {` to the last return) and launch_gemv_w8 (nseg / nstep, xs, key);
    cc_gemv_w4.hip pick_w4_cfg (its two returns) and launch_gemv_w4 (nseg, ws, nstep, xs, key), launch_w4_cfg (RW).
    MIRRORED_LINES below pins those source lines: tests/test_gemv_exact_host.py fails when one of them changes."""
    if kernel == "16":
        vec = 16 // ELEM[dt]
        nseg = (K // vec + 63) // 64
        nstep = (nseg + 3) // 4
        cap = 2048
        if nstep <= 2 and not pair:
            rb, cu = (2, 2) if N >= 32768 else (4, 2)
            cap = 1024
        elif nstep <= 2:
            rb, cu = 2, 2
        elif pair:
            rb, cu = 2, (4 if (nstep <= 4 or nstep > 8) else 8)
        else:
            rb, cu, cap = 4, 4, 512
        xs = 2 if nstep <= 2 else 8 if nstep <= 8 else 16
        assert nstep <= 16 and cu <= xs
        key, rows, ws, chunk = (100000 if pair else 0) + xs * 1000 + rb * 10 + cu, rb, 4, vec
    elif kernel == "w8":
        nseg = (K // 16 + 63) // 64
        nstep = (nseg + 3) // 4
        if nstep <= 1:
            rb, cu, cap = (4, 1, 2048) if pair else (4, 1, 1024) if N >= 32768 else (8, 1, 1024)
        elif nstep <= 2:
            rb, cu, cap = (2, 2, 2048) if pair else (4, 2, 1024)
        elif nstep <= 4:
            rb, cu, cap = (2, 4, 2048) if pair else (4, 4, 512)
        else:
            rb, cu, cap = (2, 2, 2048) if pair else (4, 2, 512)
        xs = 1 if nstep <= 1 else 2 if nstep <= 2 else 4 if nstep <= 4 else 8
        assert nstep <= 8 and cu <= xs
        key, rows, ws, chunk = (100000 if pair else 0) + xs * 1000 + rb * 10 + cu, rb, 4, 16
    else:
        nseg = (K // 32 + 63) // 64
        ws = 4 if nseg >= 3 else nseg
        nstep = (nseg + ws - 1) // ws
        if nstep <= 1:
            rb, cu, cap = (4, 1, 512) if pair else (4, 1, 1024)
        else:
            rb, cu, cap = (2, 2, 512) if pair else (4, 2, 512)
        xs = 1 if nstep <= 1 else 2 if nstep <= 2 else 4
        assert nstep <= 4 and cu <= xs
        key, rows, chunk = (100000 if pair else 0) + ws * 10000 + xs * 1000 + rb * 10 + cu, rb * (4 // ws), 32
    return types.SimpleNamespace(key=key, rows=rows, cap=cap, cu=cu, xs=xs, ws=ws, nstep=nstep, chunk=chunk)


MIRRORED_LINES = {
    "cc_gemv.hip": [
        "const int nseg = (a.K / vec + 63) / 64, nstep = (nseg + kGvWaves - 1) / kGvWaves;",
        "c.cap = 2048;", "if (nstep <= 2 && a.W3 == nullptr) {", "if (a.N >= 32768) {", "c.rb = 2; c.cu = 2;", "c.rb = 4; c.cu = 2;",
        "c.cap = 1024;", "} else if (nstep <= 2) {", "} else if (a.W3 != nullptr) {", "c.rb = 2; c.cu = (nstep <= 4 || nstep > 8) ? 4 : 8;",
        "c.rb = 4; c.cu = 4;", "c.cap = 512;", "const int xs = nstep <= 2 ? 2 : nstep <= 8 ? 8 : 16;",
        "if (nstep > 16 || c.cu > xs) return CC_ERR_UNSUPPORTED;", "const int key = (a.W3 ? 100000 : 0) + xs * 1000 + c.rb * 10 + c.cu;",
        "constexpr int kGvThreads = 256;",
    ],
    "cc_gemv_w8.hip": [
        "const int nseg = (a.K / 16 + 63) / 64, nstep = (nseg + kW8Waves - 1) / kW8Waves;",
        "if (a.W3 != nullptr) return {4, 1, 2048};", "return a.N >= 32768 ? W8Cfg{4, 1, 1024} : W8Cfg{8, 1, 1024};",
        "if (nstep <= 2) return a.W3 != nullptr ? W8Cfg{2, 2, 2048} : W8Cfg{4, 2, 1024};",
        "if (nstep <= 4) return a.W3 != nullptr ? W8Cfg{2, 4, 2048} : W8Cfg{4, 4, 512};",
        "return a.W3 != nullptr ? W8Cfg{2, 2, 2048} : W8Cfg{4, 2, 512};",
        "const int xs = nstep <= 1 ? 1 : nstep <= 2 ? 2 : nstep <= 4 ? 4 : 8;",
        "const int key = (a.W3 ? 100000 : 0) + xs * 1000 + c.rb * 10 + c.cu;", "constexpr int kW8Threads = 256;",
    ],
    "cc_gemv_w4.hip": [
        "const int nseg = (a.K / 32 + 63) / 64;", "const int ws = nseg >= 3 ? 4 : nseg;", "const int nstep = (nseg + ws - 1) / ws;",
        "if (nstep <= 1) return a.W3 != nullptr ? W4Cfg{4, 1, 512} : W4Cfg{4, 1, 1024};",
        "return a.W3 != nullptr ? W4Cfg{2, 2, 512} : W4Cfg{4, 2, 512};", "const int xs = nstep <= 1 ? 1 : nstep <= 2 ? 2 : 4;",
        "const int key = (a.W3 ? 100000 : 0) + ws * 10000 + xs * 1000 + c.rb * 10 + c.cu;", "constexpr int RW = RB * (kW4Waves / WS);",
        "constexpr int kW4Threads = 256;",
    ],
}

# the instantiations a default launch (no CC_GEMV*_CFG) can select, per kernel file
DEFAULT_KEYS = {
    "16": {2022, 2042, 8044, 16044, 102022, 108024, 108028, 116024},
    "w8": {1041, 1081, 2042, 4044, 8042, 101041, 102022, 104024, 108022},
    "w4": {11041, 21041, 41041, 42042, 44042, 111041, 121041, 141041, 142022, 144022},
}


# ------------------------------------------------------------------------------------------------ rounding in float64
def round_to(dt, v):
    """float64 -> the nearest value of dt (ties to even), as float64.  Zeros keep their sign; a non-zero value must be normal in dt
    and finite after rounding (asserted)."""
    v = np.asarray(v, np.float64)
    out = v.copy()
    nz = v != 0
    a = np.abs(v[nz])
    assert (a >= MIN_NORMAL[dt]).all(), "subnormal in the model dtype"
    _, ex = np.frexp(a)  # a = m * 2^ex, m in [0.5, 1)
    ulp = np.ldexp(1.0, ex - SIG_BITS[dt])
    r = np.rint(a / ulp) * ulp
    assert (r <= MAX_FINITE[dt]).all(), "overflows the model dtype"
    out[nz] = np.copysign(r, v[nz])
    return out


def midpoint_margin(dt, v):
    """relative distance of each float64 v (non-zero) from the nearest rounding midpoint of dt."""
    a = np.abs(np.asarray(v, np.float64))
    _, ex = np.frexp(a)
    ulp = np.ldexp(1.0, ex - SIG_BITS[dt])
    f = a / ulp
    return np.abs(f - np.floor(f) - 0.5) * ulp / a


def silu64(t):
    t = np.asarray(t, np.float64)
    with np.errstate(over="ignore"):
        return t / (1.0 + np.exp(-t))


def gate_values(dt):
    """the integer gate values t the generator may hand out: silu(t) normal in dt (fp16: and half of it, the smallest |t3| being
    1/2), clear of every rounding midpoint, t != 0."""
    ts = np.array([t for t in range(-10 if dt == HF else -32, 33) if t != 0], np.int64)
    s = silu64(ts)
    ok = (np.abs(s) >= MIN_NORMAL[dt]) & (midpoint_margin(dt, s) >= GATE_MARGIN)
    return ts[ok]


def to_dt(dt, v):
    """float64 values that dt holds exactly -> a tensor of dt (asserted exact)."""
    t = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(dt)
    assert np.array_equal(t.double().numpy(), np.asarray(v, np.float64)), "value is not exactly representable in the model dtype"
    return t


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)


# ------------------------------------------------------------------------------------------------ the integer reference
def _dequant_block(c, which, r0, r1):
    """float64 [r1 - r0, K]: the weight the contract multiplies, before any per-row scale (int8: the codes)."""
    codes = (c.codes if which == 0 else c.codes3)[r0:r1].double()
    if c.kernel != "w4":
        return codes
    S, M = (c.gs, c.gm) if which == 0 else (c.gs3, c.gm3)
    s = S[r0:r1].double().repeat_interleave(c.G, 1)
    m = M[r0:r1].double().repeat_interleave(c.G, 1)
    return (codes - 8.0 + m) * s


def dot_exact(c, which=0, block=256):
    """-> (acc int64 [N], abs_sum float64 [N]): the exact dot product of every row with the kernel's input vector and the sum of the
    magnitudes of its terms (int4: of the terms of the kernel's factored form), in float64 on integers far below 2^53."""
    xin = torch.from_numpy(c.xin.astype(np.float64))
    ax = xin.abs()
    acc = torch.empty(c.N, dtype=torch.float64)
    tot = torch.empty(c.N, dtype=torch.float64)
    if c.kernel == "w4":
        sxc = xin.view(-1, 32).sum(1).abs().view(-1, c.G // 32).sum(1)  # sum over a group's chunks of |Sx|
    for r0 in range(0, c.N, block):
        r1 = min(c.N, r0 + block)
        w = _dequant_block(c, which, r0, r1)
        acc[r0:r1] = w @ xin
        if c.kernel != "w4":
            tot[r0:r1] = w.abs() @ ax
        else:
            S, M = (c.gs, c.gm) if which == 0 else (c.gs3, c.gm3)
            s = S[r0:r1].double()
            q = (c.codes if which == 0 else c.codes3)[r0:r1].double()
            tot[r0:r1] = ((q + 128.0) * s.repeat_interleave(c.G, 1)) @ ax + ((136.0 * s + (M[r0:r1].double() * s).abs()) @ sxc)
    a = acc.numpy()
    assert np.array_equal(a, np.rint(a))
    return a.astype(np.int64), tot.numpy()


def exact_output(c, check=True):
    """The unique correct output of case c from its integer fields -> (y float64 [N], tol float64 [N] or None).  With check, every
    guarantee of the module docstring is asserted; without (the sensitivity tests corrupt the inputs) the roundings go through
    torch's conversions instead."""
    dt, R = c.dt, EXACT_RANGE[c.dt]
    rnd = (lambda v: round_to(dt, v)) if check else (lambda v: torch.from_numpy(np.asarray(v, np.float64)).to(dt).double().numpy())
    acc, tot = dot_exact(c, 0)
    c.acc, c.abs_sum = acc, tot
    if check:
        assert (tot < 2.0 ** 24).all(), "a partial sum could leave fp32's exact integers"
        assert (np.abs(acc) < R).all(), "a row's dot product left the exact range"
    v = acc.astype(np.float64)
    if c.kernel == "w8":
        v = rnd(rnd(v) * c.scale_f)
    if c.bias_i is not None:
        v = rnd(v) + c.bias_i if c.kernel != "16" else v + c.bias_i
    if check:
        to_dt(dt, v)
        assert (np.abs(v) < R).all()
    v = rnd(v)
    tol = None
    if dt == F32 and c.norm:  # one ulp of rs carried linearly, factor 2 of margin
        assert not check or (tot < 2.0 ** 22).all()
        tol = 2.0 ** -22 * tot
    if c.pair:
        acc3, tot3 = dot_exact(c, 1)
        c.acc3 = acc3
        v3 = acc3.astype(np.float64)
        if c.kernel == "w8":
            v3 = rnd(rnd(v3) * c.scale3_f)
        if check:
            assert (tot3 < 2.0 ** 24).all() and (np.abs(acc3) < R).all() and (v3 != 0).all()
            to_dt(dt, v3)
            assert np.isin(v, gate_values(dt)).all(), "a gate value is too close to a rounding midpoint of silu"
            assert (midpoint_margin(dt, silu64(v)) >= GATE_MARGIN).all()
        v = rnd(rnd(silu64(v)) * rnd(v3))
    if c.freqs_i is not None:
        rr, hd = c.rope_rows, c.hd
        f = c.freqs_i.astype(np.float64)
        pr = (np.arange(rr) % hd) >> 1
        cs, sn = f[pr, 0], f[pr, 1]
        part = v[:rr].reshape(-1, 2)[:, ::-1].reshape(-1)  # the pair partner
        sign = np.where(np.arange(rr) & 1, 1.0, -1.0)
        rot = v[:rr] * cs + sign * part * sn
        if tol is not None:
            tol = tol.copy()
            tol[:rr] = np.abs(cs) * tol[:rr] + np.abs(sn) * tol[:rr].reshape(-1, 2)[:, ::-1].reshape(-1)
        v = np.concatenate([rot, v[rr:]])
        if check:
            to_dt(dt, v)
            assert (np.abs(v) <= R).all()
        v = rnd(v)
    return v, tol


# ------------------------------------------------------------------------------------------------ the generator
def _targets(cur, limit, mod, allowed, rng, nearest, nonzero, reach):
    """per row: the dot product to repair to.  limit: |target| <= limit; mod: the target stays congruent to cur (int4: every term is
    a multiple of the row's smallest scale); allowed: per row a sorted int array of permitted values (gate rows) or None."""
    N = len(cur)
    if allowed is None:
        edge = (np.arange(N) % 5 == 0) & (mod == 1) & (limit <= reach)  # some rows sit exactly on the edge of the range handed out
        want = np.sign(cur) * (limit - rng.integers(0, np.maximum(limit // 4, 1) + 1, N))
        want = np.where(edge, np.where(cur < 0, -limit, limit), want)
        t = cur - mod * np.rint((cur - want) / mod).astype(np.int64)
        t = np.where(np.abs(t) > limit, t - np.sign(t) * mod, t)
        tgt = np.where((np.abs(cur) > limit) | edge, t, cur)
        if nonzero:
            tgt = np.where(tgt == 0, mod, tgt)
        assert (np.abs(tgt) <= limit).all() and ((tgt - cur) % mod == 0).all()
        return tgt
    tgt = cur.copy()
    for i in range(N):
        cand = allowed[i]
        cand = cand[((cand - cur[i]) % mod[i] == 0) & (np.abs(cand) <= limit[i])]
        assert len(cand), "no permitted gate value is reachable"
        tgt[i] = cand[np.argmin(np.abs(cand - cur[i]))] if nearest else cand[rng.integers(len(cand))]
    return tgt


def _repair(codes, xin, lo, hi, mult, cur, tgt, rng, frozen=None):
    """move codes of every row, a few columns each, until its dot product with xin is tgt.  mult [N, K] or None: the factor a code
    step carries besides xin (int4: the group scale).  frozen: bool [N, K] of codes that stay (int8: the placed extremes)."""
    N, K = codes.shape
    cols = np.nonzero(xin)[0]
    d = (cur - tgt).astype(np.int64)
    start = rng.integers(0, len(cols), N)
    xt = torch.from_numpy(xin.astype(np.int64))
    for it in range(2 * len(cols)):
        live = np.nonzero(d)[0]
        if not len(live):
            break
        k = cols[(start[live] + it) % len(cols)]
        lt, kt = torch.from_numpy(live), torch.from_numpy(k)
        cv = codes[lt, kt].to(torch.int64)
        m = xt[kt] * (mult[lt, kt].to(torch.int64) if mult is not None else 1)
        dl = torch.from_numpy(d[live])
        step = -torch.div(dl, m, rounding_mode="trunc")  # the change of the code that takes d towards 0 without passing it
        new = torch.clamp(cv + step, lo, hi)
        if frozen is not None:
            new = torch.where(frozen[lt, kt], cv, new)
        codes[lt, kt] = new.to(codes.dtype)
        d[live] = (dl + (new - cv) * m).numpy()
    assert not d.any(), "the repair pass could not bring every row into range"


def _pack4(q):
    q = q.to(torch.uint8)
    return (q[:, 0::2] | (q[:, 1::2] << 4)).contiguous()


def make_case(kernel, dt, N, K, form="plain", seed=0, G=32):
    """One exact case: CPU tensors in the layout glue.gemv_fused takes, the expected output `y` (and `h`, `tol`), and the integer
    fields they were computed from.  form: '+'-joined subset of norm, delta, pair, rope, bias ('plain' = none)."""
    f = set(form.split("+")) - {"plain"}
    assert f <= {"norm", "delta", "pair", "rope", "bias"} and dt in DTYPES[kernel]
    c = types.SimpleNamespace(kernel=kernel, dt=dt, N=N, K=K, G=G, form=form, norm="norm" in f, delta="delta" in f, pair="pair" in f,
                              rope="rope" in f, has_bias="bias" in f)
    assert not (c.delta and not c.norm) and not (c.pair and (c.rope or c.has_bias)) and not (c.pair and dt == F32)
    assert K % {"16": 16 // ELEM[dt], "w8": 16, "w4": G}[kernel] == 0 and K * ELEM[dt] <= 65536
    rng = np.random.default_rng([seed, N, K, sum(map(ord, kernel + form))])
    tg = torch.Generator().manual_seed(int(rng.integers(1 << 31)))
    R = EXACT_RANGE[dt]
    # ---- the input vector
    c.h_i = c.delta_i = c.nw_i = None
    if c.norm:
        c.h_i = rng.choice(np.array([-1, 1]), K)
        c.x_i = rng.integers(-3, 4, K) if c.delta else c.h_i.copy()
        if c.delta:
            c.delta_i = c.h_i - c.x_i
        wide = not (kernel == "w4" and K > 8192)  # the factored form's 2^24 bound at long int4 rows
        c.nw_i = rng.choice(np.array([1, -1, 2, -2, 3, -3]), K, p=[.35, .35, .1, .1, .05, .05] if wide else [.45, .45, .05, .05, 0, 0])
        c.xin = c.h_i * c.nw_i
    else:
        c.x_i = rng.choice(np.array([-1, 0, 1]), K, p=[7 / 16, 1 / 8, 7 / 16])
        c.x_i[0], c.x_i[K - 1] = 1, -1
        c.xin = c.x_i.copy()
    # ---- bias, RoPE
    c.bias_i = rng.integers(-8, 9, N).astype(np.float64) if c.has_bias else None
    c.freqs_i, c.rope_rows, c.hd = None, 0, 0
    if c.rope:
        g = geometry(kernel, False, N, K, dt)
        c.hd = 2 if N < g.rows + 2 or seed % 2 else g.rows + 2
        c.rope_rows = c.hd * max(1, min(N // c.hd, 3) - (1 if N // c.hd > 1 and N % c.hd == 0 else 0))
        assert c.rope_rows <= N, "RoPE needs two rows at least"
        c.freqs_i = rng.integers(-2, 3, (c.hd // 2, 2))
        c.freqs_i[0] = (1, 2)
        c.freqs_i[(c.freqs_i == 0).all(1), 0] = -1  # (0, 0) would hide a row pair
    # ---- codes
    mats = 2 if c.pair else 1
    c.codes3 = c.gs3 = c.gm3 = c.scale3_f = None
    c.scale_f = None
    for which in range(mats):
        frozen = mult = None
        if kernel == "w4":
            codes = torch.randint(0, 16, (N, K), generator=tg, dtype=torch.int8)
            ng = K // G
            sset = [1, 2, 4] if K <= 8192 else [1, 2]
            gs = torch.from_numpy(rng.choice(np.array(sset), (N, ng)).astype(np.int16))
            gm = torch.from_numpy(rng.integers(-4, 5, (N, ng)).astype(np.int16))
            mult = gs.repeat_interleave(G, 1)
            lo, hi = 0, 15
            mod = gs.min(1).values.numpy().astype(np.int64)
            scale = np.ones(N)
            if which == 0:
                c.codes, c.gs, c.gm = codes, gs, gm
            else:
                c.codes3, c.gs3, c.gm3 = codes, gs, gm
        else:
            codes = torch.randint(-8, 9, (N, K), generator=tg, dtype=torch.int8)
            lo, hi = -8, 8
            mod = np.ones(N, np.int64)
            scale = np.ones(N)
            if kernel == "w8":
                scale = np.ldexp(1.0, rng.integers(-1, 3, N))
                # the extreme codes, in every third row, on two columns of equal input (they all but cancel: -128 v + 127 v)
                ext = np.arange(0, N, 3)
                for val in (1, -1):
                    same = np.nonzero(c.xin == val)[0]
                    if len(same) >= 2:
                        break
                assert len(same) >= 2 or K < 64, "no two columns of equal unit input"
                if len(same) >= 2:
                    codes[torch.from_numpy(ext), torch.from_numpy(same[(5 * ext) % len(same)])] = -128
                    codes[torch.from_numpy(ext), torch.from_numpy(same[(5 * ext + 1) % len(same)])] = 127
                frozen = codes.to(torch.int16).abs() > 8
                if which == 0:
                    c.scale_f = scale
                else:
                    c.scale3_f = scale
            if which == 0:
                c.codes = codes
            else:
                c.codes3 = codes
        cur, _ = dot_exact(c, which)
        # the largest dot product every rounding point after it holds exactly
        Rv = R - 1
        babs = np.abs(c.bias_i) if c.bias_i is not None else np.zeros(N)
        if c.rope:
            Rv = np.where(np.arange(N) < c.rope_rows, R // (8 if kernel == "w8" else 4) - 1, Rv)
        if c.pair and which == 1:
            Rv = min(R - 1, 1023)  # fp16: rnd(silu) * t3 must stay finite
        limit = np.floor((Rv * np.minimum(scale, 1.0) - babs) / scale).astype(np.int64)
        allowed = None
        if c.pair and which == 0:
            gv = gate_values(dt)
            allowed = []
            for i in range(N):
                a = gv / scale[i]
                allowed.append(a[a == np.rint(a)].astype(np.int64))
        few = int(np.count_nonzero(c.xin)) * 6 < 400
        tgt = _targets(cur, limit, mod, allowed, rng, nearest=few, nonzero=c.pair and which == 1, reach=4 * int(np.count_nonzero(c.xin)))
        _repair(codes, c.xin, lo, hi, mult, cur, tgt, rng, frozen)
    # ---- the expected output (asserts every guarantee)
    y, tol = exact_output(c, check=True)
    c.y = to_dt(dt, y)
    c.tol = torch.from_numpy(tol) if tol is not None else None
    c.h = to_dt(dt, c.h_i) if c.norm else None
    _tensors(c)
    return c


def _tensors(c):
    """the kernel-side tensors of c's integer fields."""
    dt = c.dt
    iv = lambda a: to_dt(dt, a) if a is not None else None  # noqa: E731
    c.x, c.delta_t, c.nw, c.bias = iv(c.x_i), iv(c.delta_i), iv(c.nw_i), iv(c.bias_i)
    c.freqs = iv(c.freqs_i)
    c.W3 = c.scales = c.scales3 = None
    if c.kernel == "16":
        c.W = c.codes.to(dt)
        c.W3 = c.codes3.to(dt) if c.pair else None
    elif c.kernel == "w8":
        c.W, c.scales = c.codes.contiguous(), to_dt(dt, c.scale_f)
        if c.pair:
            c.W3, c.scales3 = c.codes3.contiguous(), to_dt(dt, c.scale3_f)
    else:
        c.W = _pack4(c.codes)
        c.scales = torch.stack([c.gs.to(BF), (c.gm * c.gs).to(BF)], -1).contiguous()
        if c.pair:
            c.W3 = _pack4(c.codes3)
            c.scales3 = torch.stack([c.gs3.to(BF), (c.gm3 * c.gs3).to(BF)], -1).contiguous()


# ------------------------------------------------------------------------------------------------ one-hot address probes
def probe_matrix(kernel, dt, N, K, pair=False, G=32, seed=0):
    """Inputs whose product with the unit vector e_j is column j itself: W[i][k] an integer pattern in [-127, 127] of (i, k) (int4:
    every code 0..15, scales and zeros varying per group; pair: W holds permitted gate values, W3 the pattern) -> a case without x
    and y, and `column(j)` -> the exact output for x = e_j as a tensor of dt."""
    c = types.SimpleNamespace(kernel=kernel, dt=dt, N=N, K=K, G=G, form="pair" if pair else "plain", norm=False, delta=False, pair=pair,
                              rope=False, has_bias=False, x_i=np.zeros(K, np.int64), delta_i=None, nw_i=None, bias_i=None, freqs_i=None,
                              rope_rows=0, hd=0, h_i=None, codes3=None, gs3=None, gm3=None, scale_f=None, scale3_f=None)
    i = torch.arange(N, dtype=torch.int64).view(-1, 1)
    k = torch.arange(K, dtype=torch.int64).view(1, -1)
    pat = (i * 89 + k * 37 + (k // 8) * 11 + (k // 512) * 5 + (k // 4096) + seed) % 255 - 127
    if kernel == "w4":
        ng = K // G
        gi = torch.arange(ng, dtype=torch.int64).view(1, -1)

        def groups(o):
            return (2 ** ((i + gi + o) % 3)).to(torch.int16), ((i * 3 + gi * 5 + o) % 9 - 4).to(torch.int16)

        if pair:  # gate: one group value (s = 1, m picks it), W3: the code pattern
            gv = torch.from_numpy(gate_values(dt))
            gv = gv[(gv >= -8) & (gv <= 7)]  # q - 8
            want = gv[(i * 7 + k * 3 + k // 32) % len(gv)]
            c.gs = torch.ones(N, ng, dtype=torch.int16)
            c.gm = torch.zeros(N, ng, dtype=torch.int16)
            c.codes = (want + 8).clamp(0, 15).to(torch.int8)
            c.codes3 = ((pat + 127) % 16).to(torch.int8)
            c.gs3, c.gm3 = groups(1)
        else:
            c.codes = ((pat + 127) % 16).to(torch.int8)
            c.gs, c.gm = groups(0)
    elif pair:
        gv = torch.from_numpy(gate_values(dt))
        c.codes = gv[(i * 7 + k * 3 + k // 8) % len(gv)].to(torch.int8)
        c.codes3 = torch.where(pat == 0, torch.ones_like(pat), pat).to(torch.int8)
    else:
        c.codes = pat.to(torch.int8)
    if kernel == "w8":
        c.scale_f = np.ones(N)
        c.scale3_f = np.ones(N) if pair else None
    _tensors(c)
    w = _dequant_block(c, 0, 0, N).numpy()
    w3 = _dequant_block(c, 1, 0, N).numpy() if pair else None

    def column(j):
        v = w[:, j]
        if pair:
            v = round_to(dt, round_to(dt, silu64(v)) * w3[:, j])
        return to_dt(dt, v)

    c.column = column
    return c


def probe_columns(kernel, dt, K, G=32):
    """the columns at the edges of every index the kernels compute: first / last element of a 16-byte chunk, last lane of a wave and
    first of the next, last chunk of a wave's segment group and first of the next step (for every waves-per-row split), both nibbles
    of a byte, either side of a group boundary, the last column."""
    ce = {"16": 16 // ELEM[dt], "w8": 16, "w4": 32}[kernel]
    js = {0, 1, ce - 1, ce, 2 * ce - 1, K - 1, K - 2, K - ce, K - ce - 1, G - 1, G, K - G, K - G - 1}
    for m in (63, 64, 65, 128, 192, 256, 512, 1024, 2048):
        js |= {m * ce - 1, m * ce, m * ce + 1}
    return sorted(j for j in js if 0 <= j < K)


# ------------------------------------------------------------------------------------------------ the cases the GPU file runs
def k_values(kernel, dt):
    """one chunk, one chunk either side of every segment-count / nstep (int4: and waves-per-row) boundary, exactly 64 KiB of input."""
    ce = {"16": 16 // ELEM[dt], "w8": 16, "w4": 32}[kernel]
    seg = 64 * ce
    top = 65536 // ELEM[dt]
    ks = {ce, seg - ce, seg, seg + ce, top - ce, top}
    b = {"16": 8, "w8": 4, "w4": 1}[kernel] * seg  # the first boundary between two instantiations
    while b < top:
        ks |= {b, b + ce}
        b *= 2
    return sorted(ks)


PLAIN_FORMS = ("plain", "norm", "norm+delta", "rope", "bias", "rope+bias", "norm+delta+rope+bias")
PAIR_FORMS = ("pair", "norm+pair", "norm+delta+pair")


def gpu_cases(kernel):
    """[(id, dt, N, K, form, G, seed)]: every dtype x K edge x form, the row counts 1, rows-per-round - 1, + 1, an odd count whose RoPE
    rows end inside a workgroup's round, one count past cap x rows-per-round at each instantiation's smallest K (two rounds of the
    row loop), and 32768 / 32771 rows at K <= 512 for the many-rows branch of the plain one- and two-segment kernels."""
    out = []
    seen_two_rounds = set()
    n = 0
    for dt in DTYPES[kernel]:
        for K in k_values(kernel, dt):
            for form in PLAIN_FORMS + (PAIR_FORMS if dt != F32 else ()):
                pair = "pair" in form
                G = 32 if kernel != "w4" else (256 if K % 256 == 0 and n % 2 else 128 if K % 128 == 0 and n % 5 == 0 else 32)
                g = geometry(kernel, pair, 1, K, dt)
                if "rope" in form:
                    N = 2 * g.rows + 3
                else:
                    N = (1, g.rows - 1, g.rows + 1, 2 * g.rows + 1)[n % 4]
                n += 1
                out.append((dt, N, K, form, G))
                if (dt, g.key) not in seen_two_rounds and (form in ("norm+delta+rope+bias", "norm+delta+pair")):
                    seen_two_rounds.add((dt, g.key))  # K ascends: this is the instantiation's smallest K
                    out.append((dt, g.cap * g.rows + 1, K, form, G))
        if kernel != "w4":
            ce = 16 // ELEM[dt] if kernel == "16" else 16
            for K in (ce, 512):
                for N, form in ((32768, "plain"), (32771, "norm+delta+rope+bias"), (32771, "bias")):
                    out.append((dt, N, K, form, 32))
    return [(f"{kernel}-{DT_NAME[dt]}-N{N}-K{K}-G{G}-{form}", dt, N, K, form, G, 100 + i) for i, (dt, N, K, form, G) in enumerate(out)]


def case_keys(kernel):
    return {geometry(kernel, "pair" in form, N, K, dt).key for (_, dt, N, K, form, _, _) in gpu_cases(kernel)}
