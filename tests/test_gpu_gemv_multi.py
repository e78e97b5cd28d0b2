"""cc_gemv_fused_multi: cc_gemv_fused for up to four input vectors from one pass over the weights.  The contract is bit identity, row
by row, with cc_gemv_fused — for every dtype, form and shape that kernel serves — so the cases are tests/gemv_exact.py's list for the
dense kernel, unchanged (every instantiation's smallest and largest K, one chunk either side of each class boundary, odd row counts,
RoPE rows ending inside a round, two rounds of the row loop, the many-rows branch), each with T = 1, 2, 3 and 4 input rows.

Row t's inputs are gemv_exact.make_case's for T different seeds; W, W3, norm_w and bias are the FIRST case's, so that one matrix
serves all rows.  What is required of row t of y and h_out:
  * bit-equal to cc_gemv_fused run on row t alone (every form, every row);
  * bit-equal to the exact integer answer (within the existing fp32-norm bound where `tol` is set).  Row 0 is the first case itself:
    its `y` / `h`.  Rows t > 0 multiply the first case's matrix with ANOTHER case's input, which make_case's repair pass never saw:
    their integer answer is recomputed here by gemv_exact.exact_output(check=False) from the first case's codes and row t's input
    — still a unique bit pattern for the plain / norm / RoPE / bias forms (all sums are integers below 2^24, exact in fp32 in any
    order; only the final rounding is no longer an identity).  For the SwiGLU forms an unrepaired gate value may sit on a rounding
    midpoint of silu, where the fp32 expf decides: there rows t > 0 have no unique answer and are held to cc_gemv_fused alone
    (which tests/test_gpu_gemv_exact.py pins to the integer answers);
  * 64 guard elements behind y and h_out untouched.
Also: T = 0 and T = 5 are CC_ERR_BAD_ARG and write nothing; graph replay equals eager; one-hot probes per dtype where token t carries
x = e_(j+t) and must return column j + t (names a token / column mix-up)."""
import copy
import ctypes as C

import pytest
import torch

import gemv_exact as E

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
SENTINEL = 1536.0
MAX_T = 4


def _call(name, *a):
    from cold_compress_amd import _abi

    _abi.call(name, *a)


def _ptrs():
    from cold_compress_amd.harness.glue import _DT, _p, _stream

    return _DT, _p, _stream


def _rows(dt, N, K, form, G, seed):
    """-> [case 0, composite rows 1..3]: each with .x / .delta_t / .freqs (CPU tensors of this row) and the expected .y (None: no
    unique answer) / .tol / .h for the FIRST case's matrix."""
    c0 = E.make_case("16", dt, N, K, form, seed, G)
    g = E.geometry("16", c0.pair, N, K, dt)
    # rows t > 0 only lend their input vectors: a small matrix makes the same ones, with the same head_dim (make_case derives it from
    # the rows per round, which the many-rows branch changes: those cases keep their N)
    n_small = N if N >= 32768 else min(N, 2 * g.rows + 3)
    rows = [c0]
    for t in range(1, MAX_T):
        ct = E.make_case("16", dt, n_small, K, form, seed + 2 * t, G)  # (same parity: make_case derives head_dim from it)
        assert ct.hd == c0.hd and (ct.freqs_i is None) == (c0.freqs_i is None)
        k = copy.copy(c0)
        k.x_i, k.delta_i, k.h_i, k.freqs_i = ct.x_i, ct.delta_i, ct.h_i, ct.freqs_i
        k.xin = ct.h_i * c0.nw_i if c0.norm else ct.x_i.copy()
        k.x, k.delta_t, k.freqs, k.h = ct.x, ct.delta_t, ct.freqs, ct.h
        k.y = k.tol = None
        if not c0.pair:
            y, tol = E.exact_output(k, check=False)
            k.y = torch.from_numpy(y).to(dt)
            k.tol = torch.from_numpy(tol) if tol is not None else None
        rows.append(k)
    return rows


def _stack(rows, key):
    ts = [getattr(r, key) for r in rows]
    return None if ts[0] is None else torch.stack(ts).to(DEV).contiguous()


def _dev0(c):
    return {k: (getattr(c, k).to(DEV).contiguous() if getattr(c, k, None) is not None else None) for k in ("W", "W3", "nw", "bias")}


def _buf(n, dt):
    return torch.full((n + GUARD,), SENTINEL, dtype=dt, device=DEV)


def _launch_multi(c, d, X, D, F, T, ybuf, hbuf):
    _DT, _p, _stream = _ptrs()
    _call("cc_gemv_fused_multi", _p(d["W"]), _p(d["W3"]), _p(X), _p(D), _p(d["nw"]), 0.0, _p(hbuf), _p(d["bias"]), _p(F), int(c.rope_rows),
          int(c.hd), _p(ybuf), c.N, c.K, T, _DT[c.dt], _stream())


def _launch_single(c, d, x, dl, fr, ybuf, hbuf):
    _DT, _p, _stream = _ptrs()
    _call("cc_gemv_fused", _p(d["W"]), _p(d["W3"]), _p(x), _p(dl), _p(d["nw"]), 0.0, _p(hbuf), _p(d["bias"]), _p(fr), int(c.rope_rows),
          int(c.hd), _p(ybuf), c.N, c.K, _DT[c.dt], _stream())


def _singles(c, d, X, D, F):
    """cc_gemv_fused on every row alone -> [(y [N], h [K] or None)] on the CPU."""
    out = []
    for t in range(X.shape[0]):
        yb, hb = _buf(c.N, c.dt), (_buf(c.K, c.dt) if c.norm else None)
        _launch_single(c, d, X[t], None if D is None else D[t], None if F is None else F[t], yb, hb)
        out.append((yb[:c.N].cpu(), hb[:c.K].cpu() if hb is not None else None))
    return out


def _check(what, rows, singles, T, ybuf, hbuf):
    c = rows[0]
    N, K = c.N, c.K
    assert (ybuf[T * N:].float() == SENTINEL).all(), f"{what}: wrote behind y"
    if c.norm:
        assert (hbuf[T * K:].float() == SENTINEL).all(), f"{what}: wrote behind h_out"
    y = ybuf[:T * N].view(T, N).cpu()
    h = hbuf[:T * K].view(T, K).cpu() if c.norm else None
    for t in range(T):
        ys, hs = singles[t]
        if not torch.equal(E.bits(y[t]), E.bits(ys)):
            bad = (E.bits(y[t]) != E.bits(ys)).nonzero().flatten()
            r = int(bad[0])
            raise AssertionError(f"{what} token {t}: {len(bad)} of {N} rows differ from cc_gemv_fused, first row {r}: {float(y[t][r])} vs {float(ys[r])}")
        k = rows[t]
        if k.y is not None:
            if k.tol is None:
                if not torch.equal(E.bits(y[t]), E.bits(k.y)):
                    bad = (E.bits(y[t]) != E.bits(k.y)).nonzero().flatten()
                    r = int(bad[0])
                    raise AssertionError(f"{what} token {t}: {len(bad)} of {N} rows differ from the integer answer, first row {r}: "
                                         f"{float(y[t][r])} vs {float(k.y[r])}")
            else:
                err = (y[t].double() - k.y.double()).abs()
                assert (err <= k.tol).all(), f"{what} token {t}: row {int((err - k.tol).argmax())} beyond the fp32 norm bound by {float((err - k.tol).max())}"
        if c.norm:
            assert torch.equal(E.bits(h[t]), E.bits(hs)), f"{what} token {t}: h_out differs from cc_gemv_fused"
            assert torch.equal(E.bits(h[t]), E.bits(k.h)), f"{what} token {t}: h_out differs from the exact x + delta"


@pytest.mark.parametrize("dt,N,K,form,G,seed", [pytest.param(dt, N, K, form, G, seed, id=i) for (i, dt, N, K, form, G, seed) in E.gpu_cases("16")])
def test_gemv_multi_exact(dt, N, K, form, G, seed):
    rows = _rows(dt, N, K, form, G, seed)
    c = rows[0]
    d = _dev0(c)
    X, D, F = _stack(rows, "x"), _stack(rows, "delta_t"), _stack(rows, "freqs")
    singles = _singles(c, d, X, D, F)
    key = E.geometry("16", c.pair, N, K, dt).key
    for T in (1, 2, 3, 4):
        ybuf, hbuf = _buf(T * N, dt), (_buf(T * K, dt) if c.norm else None)
        _launch_multi(c, d, X, D, F, T, ybuf, hbuf)
        torch.cuda.synchronize()
        _check(f"{E.DT_NAME[dt]} N={N} K={K} {form} key {key} T={T}", rows, singles, T, ybuf, hbuf)


def test_token_count_outside_1_to_4_is_a_bad_argument():
    from cold_compress_amd import _abi

    _DT, _p, _stream = _ptrs()
    rows = _rows(E.BF, 9, 512, "norm+delta+rope+bias", 32, 300)
    c, d = rows[0], _dev0(rows[0])
    X, D, F = _stack(rows, "x"), _stack(rows, "delta_t"), _stack(rows, "freqs")
    f = _abi.lib()["cc_gemv_fused_multi"]
    for T in (0, 5, -1):
        ybuf, hbuf = _buf(4 * c.N, c.dt), _buf(4 * c.K, c.dt)
        rc = f(_p(d["W"]), None, _p(X), _p(D), _p(d["nw"]), 0.0, _p(hbuf), _p(d["bias"]), _p(F), int(c.rope_rows), int(c.hd), _p(ybuf), c.N, c.K, T,
               _DT[c.dt], _stream())
        assert rc == -1, (T, rc)  # CC_ERR_BAD_ARG
        torch.cuda.synchronize()
        assert (ybuf.float() == SENTINEL).all() and (hbuf.float() == SENTINEL).all(), f"T={T}: an error wrote something"
    # the checks it shares with cc_gemv_fused
    ybuf = _buf(4 * c.N, c.dt)
    assert f(_p(d["W"]), None, _p(X), _p(D), None, 0.0, None, None, None, 0, 0, _p(ybuf), c.N, c.K, 2, _DT[c.dt], _stream()) == -1  # delta without norm_w
    assert f(_p(d["W"]), None, _p(X), None, None, 0.0, None, None, None, 0, 0, _p(ybuf), c.N, 12, 2, _DT[c.dt], _stream()) == -2  # K % 8: unsupported
    torch.cuda.synchronize()
    assert (ybuf.float() == SENTINEL).all()


def test_graph_replay_bit_equal():
    dt = E.BF
    ks = E.k_values("16", dt)
    for n, (N, K, form) in enumerate([(37, ks[3], "norm+delta+rope+bias"), (29, ks[-3], "norm+delta+pair")]):
        rows = _rows(dt, N, K, form, 32, 900 + n)
        c, d = rows[0], _dev0(rows[0])
        X, D, F = _stack(rows, "x"), _stack(rows, "delta_t"), _stack(rows, "freqs")
        singles = _singles(c, d, X, D, F)
        ybuf, hbuf = _buf(4 * N, dt), _buf(4 * K, dt)
        _launch_multi(c, d, X, D, F, 4, ybuf, hbuf)
        torch.cuda.synchronize()
        _check(f"eager {form} K={K}", rows, singles, 4, ybuf, hbuf)
        yg, hg = _buf(4 * N, dt), _buf(4 * K, dt)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            _launch_multi(c, d, X, D, F, 4, yg, hg)
        torch.cuda.current_stream().wait_stream(s)
        yg.fill_(SENTINEL)
        hg.fill_(SENTINEL)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            _launch_multi(c, d, X, D, F, 4, yg, hg)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(E.bits(yg), E.bits(ybuf)) and torch.equal(E.bits(hg), E.bits(hbuf)), f"{form} K={K}: graph replay != eager"
        _check(f"graph {form} K={K}", rows, singles, 4, yg, hg)


@pytest.mark.parametrize("dt,pair", [pytest.param(dt, pair, id=f"{E.DT_NAME[dt]}-{'pair' if pair else 'plain'}")
                                     for dt in (E.BF, E.HF, E.F32) for pair in (False, True) if not (pair and dt == E.F32)])
def test_one_hot_probes_name_the_token_and_the_column(dt, pair):
    """token t carries x = e_(j+t): row t of y must be column j + t of W, exactly (pair: rnd(silu(W[:, j+t])) * W3[:, j+t]) — a
    token whose output came from another token's input, or from a neighbouring column, shows as the wrong column."""
    _DT, _p, _stream = _ptrs()
    K = E.k_values("16", dt)[-3]  # 16 chunks per lane
    g = E.geometry("16", pair, 1, K, dt)
    N = 2 * g.rows + 1
    c = E.probe_matrix("16", dt, N, K, pair, 32)
    d = _dev0(c)
    X = torch.zeros((MAX_T, K), dtype=dt, device=DEV)
    for j in E.probe_columns("16", dt, K, 32):
        if j + MAX_T > K:
            continue
        X.zero_()
        for t in range(MAX_T):
            X[t, j + t] = 1.0
        ybuf = _buf(MAX_T * N, dt)
        _call("cc_gemv_fused_multi", _p(d["W"]), _p(d["W3"]), _p(X), None, None, 0.0, None, None, None, 0, 0, _p(ybuf), N, K, MAX_T, _DT[dt], _stream())
        y = ybuf[:MAX_T * N].view(MAX_T, N).cpu()
        assert (ybuf[MAX_T * N:].float() == SENTINEL).all(), f"column {j}: wrote behind y"
        for t in range(MAX_T):
            want = c.column(j + t)
            assert torch.equal(E.bits(y[t]), E.bits(want)), f"token {t}, column {j + t}: rows {(E.bits(y[t]) != E.bits(want)).nonzero().flatten().tolist()} " \
                                                            f"got {y[t].float().tolist()} want {want.float().tolist()}"
