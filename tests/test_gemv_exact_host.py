"""CPU checks of tests/gemv_exact.py, the known-answer inputs of tests/test_gpu_gemv_exact.py: the integer reference against the
oracle's double-precision twin (16-bit kernel) and against the torch contract formula in float64 on harness/quantize.py's dequantised
weights (int8, int4); the generator's guarantees for every case the GPU file runs; the sensitivity the random-data tests lack
(shown by corrupting the REFERENCE's inputs, never a kernel); and that the GPU cases reach every instantiation a default launch
can select."""
import copy
import os

import numpy as np
import pytest
import torch

import gemv_exact as E
from helpers import DT_CODE, from_np, to_np

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cold_compress_amd", "csrc")


# ------------------------------------------------------------------------------------------------ the launcher mirror
@pytest.mark.parametrize("fname", sorted(E.MIRRORED_LINES))
def test_mirrored_launcher_lines_are_the_source(fname):
    """geometry() copies these lines of the launchers: when one changes, update the mirror (and DEFAULT_KEYS, and the cases)."""
    src = " ".join(open(os.path.join(CSRC, fname)).read().split())
    for line in E.MIRRORED_LINES[fname]:
        assert " ".join(line.split()) in src, f"{fname} no longer contains: {line}"


@pytest.mark.parametrize("kernel", E.KERNELS)
def test_default_keys_are_what_the_mirror_can_select(kernel):
    got = set()
    for dt in E.DTYPES[kernel]:
        step = {"16": 16 // E.ELEM[dt], "w8": 16, "w4": 32}[kernel]
        for K in range(step, 65536 // E.ELEM[dt] + 1, step):
            for pair in (False, True):
                for N in (1, 32768):
                    got.add(E.geometry(kernel, pair, N, K, dt).key)
    assert got == E.DEFAULT_KEYS[kernel]
    if kernel != "w4":  # every one of them is a case of the launcher's switch
        src = open(os.path.join(CSRC, {"16": "cc_gemv.hip", "w8": "cc_gemv_w8.hip"}[kernel])).read()
        for key in got:
            assert f"case {key}:" in src, key


@pytest.mark.parametrize("kernel", E.KERNELS)
def test_gpu_cases_reach_every_default_instantiation(kernel):
    assert E.case_keys(kernel) == E.DEFAULT_KEYS[kernel]
    # ... each with two rounds of the row loop, and the many-rows branch at both row counts
    two = {E.geometry(kernel, "pair" in f, N, K, dt).key for (_, dt, N, K, f, _, _) in E.gpu_cases(kernel)
           if N == (lambda g: g.cap * g.rows + 1)(E.geometry(kernel, "pair" in f, 1, K, dt))}
    many = {2022} if kernel == "16" else {1041} if kernel == "w8" else set()
    assert two == E.DEFAULT_KEYS[kernel] - many
    assert {N for (_, _, N, _, _, _, _) in E.gpu_cases(kernel)} >= ({32768, 32771} if many else set())


# ------------------------------------------------------------------------------------------------ references
def _contract_f64(c):
    """the contract of include/coldcompress.h as a float64 torch composition with the model dtype's rounding points."""
    from cold_compress_amd.harness.quantize import dequantize_int4

    dt = c.dt
    r = lambda t: t.to(dt).double()  # noqa: E731
    xf = c.x.double()
    h = None
    if c.norm:
        h = r(xf + c.delta_t.double()) if c.delta else xf
        n = r(h * torch.rsqrt((h * h).mean()))
        xin = r(n * c.nw.double())
    else:
        xin = xf

    def lin(W, s):
        if c.kernel == "16":
            return W.double() @ xin
        if c.kernel == "w8":
            return r(r(W.double() @ xin) * s.double())
        return r(dequantize_int4(W, s, c.G).double() @ xin)

    t = lin(c.W, c.scales)
    if c.bias is not None:
        t = t + c.bias.double()
    t = r(t)
    if c.pair:
        t3 = lin(c.W3, c.scales3)
        t = r(r(torch.nn.functional.silu(t)) * (r(t3) if c.kernel == "16" else t3))
    if c.freqs is not None:
        f = c.freqs.double().view(-1, 2)
        rr = t[:c.rope_rows].view(-1, c.hd // 2, 2)
        cs, sn = f[:, 0].view(1, -1), f[:, 1].view(1, -1)
        out = torch.stack([rr[..., 0] * cs - rr[..., 1] * sn, rr[..., 1] * cs + rr[..., 0] * sn], -1).reshape(-1)
        t = torch.cat([r(out), t[c.rope_rows:]])
    return t.to(dt), (h.to(dt) if h is not None else None)


def _oracle_twin(o, c):
    es = np.float32 if c.dt == E.F32 else np.uint16
    yo = np.zeros(c.N, es)
    ho = np.zeros(c.K, es) if c.norm else None
    pp = lambda t: o.ptr(to_np(t)) if t is not None else None  # noqa: E731
    o.call("cc_gemv_fused", pp(c.W), pp(c.W3), pp(c.x), pp(c.delta_t), pp(c.nw), 0.0, o.ptr(ho) if ho is not None else None, pp(c.bias),
           pp(c.freqs), c.rope_rows, c.hd, o.ptr(yo), c.N, c.K, DT_CODE[c.dt], None)
    return from_np(yo, c.dt), (from_np(ho, c.dt) if ho is not None else None)


def _groups():
    out = []
    for kernel in E.KERNELS:
        by = {}
        for case in E.gpu_cases(kernel):
            by.setdefault((kernel, E.DT_NAME[case[1]], case[3]), []).append(case)
        out += [pytest.param(kernel, cases, id=f"{kernel}-{d}-K{K}") for (kernel, d, K), cases in by.items()]
    return out


@pytest.mark.parametrize("kernel,cases", _groups())
def test_every_gpu_case_keeps_the_guarantees_and_matches_the_twin(oracle, kernel, cases):
    """make_case asserts, for every row it hands out: the row inside the exact range, sum |terms| < 2^24 (int4: of the factored form),
    every gate value clear of silu's rounding midpoints, every rounding point an identity.  Here each case of the GPU file is
    generated, and its expected y / h_out compared bit for bit with an independent evaluation: the oracle's double-accumulating twin
    of cc_gemv_fused (16-bit kernel; rsqrt(1) is exactly 1 there, so fp32 norm forms too), the float64 contract formula (int8, int4)."""
    for (cid, dt, N, K, form, G, seed) in cases:
        c = E.make_case(kernel, dt, N, K, form, seed, G)
        assert (np.abs(c.acc) < E.EXACT_RANGE[dt]).all() and (c.abs_sum < 2.0 ** 24).all(), cid
        assert (np.abs(c.y.double().numpy()) <= E.EXACT_RANGE[dt]).all() or c.pair, cid
        if c.pair:
            t = c.acc * (c.scale_f if kernel == "w8" else 1.0)
            assert np.isin(t, E.gate_values(dt)).all() and (E.midpoint_margin(dt, E.silu64(t)) >= E.GATE_MARGIN).all(), cid
            assert (c.acc3 != 0).all(), cid
        if c.tol is not None:
            assert (c.abs_sum < 2.0 ** 22).all(), cid
        y, h = _oracle_twin(oracle, c) if kernel == "16" else _contract_f64(c)
        assert torch.equal(E.bits(y), E.bits(c.y)), f"{cid}: rows {(E.bits(y) != E.bits(c.y)).nonzero().flatten()[:8].tolist()}"
        if c.norm:
            assert torch.equal(E.bits(h), E.bits(c.h)), f"{cid}: h_out"


def test_gate_values_are_clear_of_midpoints():
    for dt in (E.BF, E.HF):
        gv = E.gate_values(dt)
        assert len(gv) >= 24 and 0 not in gv
        s = E.silu64(gv)
        assert (E.midpoint_margin(dt, s) >= E.GATE_MARGIN).all() and (np.abs(s) * 0.5 >= E.MIN_NORMAL[dt]).all()
        # the fp32 evaluation of the kernels, rounded, is the float64 one, rounded
        t = torch.from_numpy(gv.astype(np.float32))
        assert torch.equal((t / (1.0 + torch.exp(-t))).to(dt).double(), torch.from_numpy(E.round_to(dt, s)))


@pytest.mark.parametrize("kernel", E.KERNELS)
def test_probe_columns_are_the_matrix_columns(kernel):
    for pair in (False, True):
        c = E.probe_matrix(kernel, E.BF, 9, 4096, pair, 32)
        for j in E.probe_columns(kernel, E.BF, 4096, 32):
            c.x_i[:] = 0
            c.x_i[j] = 1
            c.xin = c.x_i
            y, _ = E.exact_output(c, check=False)
            assert np.array_equal(y, c.column(j).double().numpy()), (pair, j)
    js = E.probe_columns("w4", E.BF, 8192, 256)
    assert {0, 1, 31, 32, 255, 256, 2047, 2048, 4095, 4096, 8191} <= set(js)


# ------------------------------------------------------------------------------------------------ sensitivity
def _corruptions(c):
    """[(name, corrupted copy of c, rows it touches)]: each changes the reference's INPUTS the way a wrong kernel would read them.
    A candidate that changes no term (equal chunks, a zero input) is no corruption: the first one that does is taken."""
    ce = {"16": 16 // E.ELEM[c.dt], "w8": 16, "w4": 32}[c.kernel]
    base, _ = E.dot_exact(c, 0)
    out = []

    def attempt(name, edits):
        for edit in edits:
            k = copy.copy(c)
            k.codes, k.xin = c.codes.clone(), c.xin.copy()
            if c.kernel == "w4":
                k.gs = c.gs.clone()
            edit(k)
            acc, _ = E.dot_exact(k, 0)
            rows = np.nonzero(acc != base)[0]
            if len(rows):
                out.append((name, k, rows))
                return
        raise AssertionError(f"no candidate for '{name}' changed a term")

    def zero(i, j):
        def f(k):
            k.codes[i, j] = 0 if c.kernel != "w4" else 8 - int(c.gm[i, j // c.G])
        return f

    def dup(i, a, b):
        def f(k):
            k.codes[i, b * ce:(b + 1) * ce] = c.codes[i, a * ce:(a + 1) * ce]
        return f

    def swap(i, a):
        def f(k):
            k.codes[i, a * ce:(a + 1) * ce] = c.codes[i + 1, a * ce:(a + 1) * ce]
            k.codes[i + 1, a * ce:(a + 1) * ce] = c.codes[i, a * ce:(a + 1) * ce]
        return f

    def skip(k):
        k.xin[-64 * ce:] = 0

    nch = c.K // ce
    attempt("zero one weight", [zero(3, j) for j in range(c.K - 1, c.K - 40, -1)])
    attempt("duplicate one 16-byte chunk", [dup(2, a, a + 1) for a in range(nch - 2, nch - 8, -1)])
    attempt("swap two rows' chunks", [swap(4, a) for a in range(nch - 1, nch - 8, -1)])
    attempt("skip the last segment", [skip])
    if c.kernel == "w4":
        def nibble(i, j):
            def f(k):
                k.codes[i, 2 * j], k.codes[i, 2 * j + 1] = c.codes[i, 2 * j + 1], c.codes[i, 2 * j]
            return f

        def scale(i, g):
            def f(k):
                k.gs[i, g] = c.gs[i, g + 1]
            return f

        attempt("use the wrong nibble", [nibble(5, j) for j in range(7, 40)])
        attempt("use the neighbouring group's scale", [scale(6, g) for g in range(0, c.K // c.G - 1)])
    return out


@pytest.mark.parametrize("kernel,form", [(k, f) for k in E.KERNELS for f in ("plain", "norm+delta+rope+bias", "norm+delta+pair")])
def test_every_corruption_changes_every_row_it_touches(kernel, form):
    c = E.make_case(kernel, E.BF, 16, 4096, form, seed=31, G=32)
    y0, _ = E.exact_output(c, check=True)
    for name, k, rows in _corruptions(c):
        y1, _ = E.exact_output(k, check=False)
        y1 = torch.from_numpy(y1).to(c.dt)
        if c.rope:  # a rotated row carries its partner
            rows = np.unique(np.concatenate([rows, rows[rows < c.rope_rows] ^ 1]))
        same = [int(i) for i in rows if E.bits(y1)[i] == E.bits(c.y)[i] and not (c.rope and i < c.rope_rows)]
        assert not same, f"{kernel} {form}: '{name}' left rows {same} unchanged"
        if name == "skip the last segment":
            assert len(rows) >= 12, name  # (a row whose last segment sums to exactly 0 is not touched)
        if c.rope:  # of a rotated pair at least one row moves
            for i in rows[rows < c.rope_rows]:
                assert E.bits(y1)[i] != E.bits(c.y)[i] or E.bits(y1)[i ^ 1] != E.bits(c.y)[i ^ 1], (name, int(i))


def test_the_same_corruptions_hide_inside_the_random_data_tolerance(capsys):
    """tests/test_gpu_gemv.py's 'wo' case (Gaussian bf16 4096 x 4096, its seed): the corruptions above, applied to a float64
    evaluation, against that file's tolerance 2 ulp x max(1, max |ref|).  The figures are printed; a single zeroed weight, at
    least, stays inside the tolerance, which is why the exact cases exist."""
    N = K = 4096
    g = torch.Generator().manual_seed(N * 7 + K)
    W = (torch.randn(N, K, generator=g) * 0.05).to(E.BF).double()
    x = torch.randn(K, generator=g).to(E.BF).double()
    ref = (W @ x).to(E.BF).double()
    tol = 2 * 2.0 ** -8 * max(1.0, float(ref.abs().max()))
    rows = []

    def report(name, Wc, xc=x):
        err = float(((Wc @ xc).to(E.BF).double() - ref).abs().max())
        rows.append((name, err, err <= tol))

    Wc = W.clone(); Wc[3, K - 1] = 0; report("zero one weight", Wc)
    Wc = W.clone(); Wc[2, K - 8:] = W[2, K - 16:K - 8]; report("duplicate one 16-byte chunk", Wc)
    Wc = W.clone(); Wc[4, K - 8:], Wc[5, K - 8:] = W[5, K - 8:], W[4, K - 8:]; report("swap two rows' chunks", Wc)
    xc = x.clone(); xc[-512:] = 0; report("skip the last segment", W, xc)
    with capsys.disabled():
        print(f"\nrandom-data tolerance {tol:.4f} (2 ulp x max|ref|), largest output error per corruption:")
        for name, err, inside in rows:
            print(f"  {name:<32} {err:.4f}  {'NOT DETECTED' if inside else 'detected'}")
    assert any(inside for _, _, inside in rows) and rows[0][2]
