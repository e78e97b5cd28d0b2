"""cc_gemv_fused_w8_multi / cc_gemv_fused_mx4_multi: the int8 and MXFP4 weight-only GEMVs for up to four input vectors from one pass
over the weights.  tests/test_gpu_gemv_multi.py for these two kernels: the contract is bit identity, row by row, with the
single-vector entry point (cc_gemv_fused_w8 / cc_gemv_fused_mx4) — for every dtype, form and shape it serves — so the cases are
gemv_exact.gpu_cases("w8") and gemv_mx4_exact.gpu_cases(), unchanged (every default instantiation's smallest and largest K, one chunk
either side of each class boundary, 64 KiB of input with the norm prologue, row counts 1, rows-per-round -+ 1, odd counts whose RoPE
rows end inside a round, two rounds of the row loop, the 32768-row branch), each with T = 1, 2, 3 and 4 input rows.

Row t's inputs are the generator's for T different seeds; W, W3, the scales, norm_w and bias are the FIRST case's, so that one matrix
serves all rows.  What is required of row t of y and h_out:
  * bit-equal to the single-vector entry point run on row t alone (every form, every row);
  * row 0 bit-equal to the case's integer answer; rows t > 0 bit-equal to the integer answer recomputed from the first case's codes
    and row t's input (exact_output(check=False)) for the non-pair forms — all sums are integers below 2^24, exact in fp32 in any
    order.  For the SwiGLU forms an unrepaired gate value may sit on a rounding midpoint of silu: there rows t > 0 are held to the
    single kernel alone (which tests/test_gpu_gemv_exact.py / test_gpu_gemv_mx4_exact.py pin to the integer answers);
  * 64 guard elements behind y and h_out untouched.
Also: T = 0, 5, -1 are CC_ERR_BAD_ARG and write nothing, the shared checks return what the single entry point returns; one-hot probes
per kernel and dtype where token t carries x = e_(j+t) and must return column j + t; graph replay of a T = 4 launch equals eager."""
import copy
import types

import numpy as np
import pytest
import torch

import gemv_exact as E
import gemv_mx4_exact as X

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
SENTINEL = 1536.0
MAX_T = 4
BF = torch.bfloat16
ENTRY = {"w8": ("cc_gemv_fused_w8", "cc_gemv_fused_w8_multi"), "mx4": ("cc_gemv_fused_mx4", "cc_gemv_fused_mx4_multi")}


def _ptrs():
    from cold_compress_amd.harness.glue import _DT, _p, _stream

    return _DT, _p, _stream


def _make(kernel, dt, N, K, form, seed):
    if kernel == "w8":
        return E.make_case("w8", dt, N, K, form, seed, 32)
    c = X.make_case(N, K, form, seed)
    c.dt, c.tol = BF, None
    return c


def _geometry(kernel, pair, N, K, dt):
    return E.geometry("w8", pair, N, K, dt) if kernel == "w8" else X.geometry(pair, N, K)


def _rows(kernel, dt, N, K, form, seed):
    """-> [case 0, composite rows 1..3]: each with .x / .delta_t / .freqs (CPU tensors of this row) and the expected .y (None: no
    unique answer) / .h for the FIRST case's matrix."""
    c0 = _make(kernel, dt, N, K, form, seed)
    g = _geometry(kernel, c0.pair, N, K, dt)
    # rows t > 0 only lend their input vectors: a small matrix makes the same ones, with the same head_dim (the generators derive it
    # from the rows per round, which the many-rows branch changes: those cases keep their N)
    n_small = N if N >= 32768 else min(N, 2 * g.rows + 3)
    rows = [c0]
    for t in range(1, MAX_T):
        ct = _make(kernel, dt, n_small, K, form, seed + 2 * t)  # (same parity: the generators derive head_dim from it)
        assert ct.hd == c0.hd and (ct.freqs_i is None) == (c0.freqs_i is None)
        k = copy.copy(c0)
        k.x_i, k.delta_i, k.h_i, k.freqs_i = ct.x_i, ct.delta_i, ct.h_i, ct.freqs_i
        k.xin = ct.h_i * c0.nw_i if c0.norm else ct.x_i.copy()
        k.x, k.delta_t, k.freqs, k.h = ct.x, ct.delta_t, ct.freqs, ct.h
        k.y = None
        if not c0.pair:
            if kernel == "w8":
                y, tol = E.exact_output(k, check=False)
                assert tol is None
            else:
                y = X.exact_output(k, check=False)
            k.y = torch.from_numpy(y).to(dt)
        rows.append(k)
    return rows


def _stack(rows, key):
    ts = [getattr(r, key) for r in rows]
    return None if ts[0] is None else torch.stack(ts).to(DEV).contiguous()


def _dev0(c):
    return {k: (getattr(c, k).to(DEV).contiguous() if getattr(c, k, None) is not None else None)
            for k in ("W", "W3", "scales", "scales3", "nw", "bias")}


def _buf(n, dt):
    return torch.full((n + GUARD,), SENTINEL, dtype=dt, device=DEV)


def _args(c, d, x, dl, fr, ybuf, hbuf):
    _DT, _p, _stream = _ptrs()
    return (_p(d["W"]), _p(d["scales"]), _p(d["W3"]), _p(d["scales3"]), _p(x), _p(dl), _p(d["nw"]), 0.0, _p(hbuf), _p(d["bias"]), _p(fr),
            int(c.rope_rows), int(c.hd), _p(ybuf), c.N, c.K)


def _launch_multi(kernel, c, d, X_, D, F, T, ybuf, hbuf):
    from cold_compress_amd import _abi

    _DT, _p, _stream = _ptrs()
    _abi.call(ENTRY[kernel][1], *_args(c, d, X_, D, F, ybuf, hbuf), T, _DT[c.dt], _stream())


def _launch_single(kernel, c, d, x, dl, fr, ybuf, hbuf):
    from cold_compress_amd import _abi

    _DT, _p, _stream = _ptrs()
    _abi.call(ENTRY[kernel][0], *_args(c, d, x, dl, fr, ybuf, hbuf), _DT[c.dt], _stream())


def _singles(kernel, c, d, X_, D, F):
    """the single-vector entry point on every row alone -> [(y [N], h [K] or None)] on the CPU."""
    out = []
    for t in range(X_.shape[0]):
        yb, hb = _buf(c.N, c.dt), (_buf(c.K, c.dt) if c.norm else None)
        _launch_single(kernel, c, d, X_[t], None if D is None else D[t], None if F is None else F[t], yb, hb)
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
            raise AssertionError(f"{what} token {t}: {len(bad)} of {N} rows differ from the single-vector kernel, first row {r}: "
                                 f"{float(y[t][r])} vs {float(ys[r])}")
        k = rows[t]
        if k.y is not None and not torch.equal(E.bits(y[t]), E.bits(k.y)):
            bad = (E.bits(y[t]) != E.bits(k.y)).nonzero().flatten()
            r = int(bad[0])
            raise AssertionError(f"{what} token {t}: {len(bad)} of {N} rows differ from the integer answer, first row {r}: "
                                 f"{float(y[t][r])} vs {float(k.y[r])}")
        if c.norm:
            assert torch.equal(E.bits(h[t]), E.bits(hs)), f"{what} token {t}: h_out differs from the single-vector kernel"
            assert torch.equal(E.bits(h[t]), E.bits(k.h)), f"{what} token {t}: h_out differs from the exact x + delta"


def _params():
    out = [pytest.param("w8", dt, N, K, form, seed, id=i) for (i, dt, N, K, form, _, seed) in E.gpu_cases("w8")]
    return out + [pytest.param("mx4", BF, N, K, form, seed, id=i) for (i, N, K, form, seed) in X.gpu_cases()]


@pytest.mark.parametrize("kernel,dt,N,K,form,seed", _params())
def test_gemv_wo_multi_exact(kernel, dt, N, K, form, seed):
    rows = _rows(kernel, dt, N, K, form, seed)
    c = rows[0]
    d = _dev0(c)
    X_, D, F = _stack(rows, "x"), _stack(rows, "delta_t"), _stack(rows, "freqs")
    singles = _singles(kernel, c, d, X_, D, F)
    key = _geometry(kernel, c.pair, N, K, dt).key
    for T in (1, 2, 3, 4):
        ybuf, hbuf = _buf(T * N, dt), (_buf(T * K, dt) if c.norm else None)
        _launch_multi(kernel, c, d, X_, D, F, T, ybuf, hbuf)
        torch.cuda.synchronize()
        _check(f"{kernel} {E.DT_NAME[dt]} N={N} K={K} {form} key {key} T={T}", rows, singles, T, ybuf, hbuf)


@pytest.mark.parametrize("kernel", ["w8", "mx4"])
def test_token_count_outside_1_to_4_is_a_bad_argument(kernel):
    from cold_compress_amd import _abi

    _DT, _p, _stream = _ptrs()
    rows = _rows(kernel, BF, 9, 512, "norm+delta+rope+bias", 300)
    c, d = rows[0], _dev0(rows[0])
    X_, D, F = _stack(rows, "x"), _stack(rows, "delta_t"), _stack(rows, "freqs")
    f, f1 = _abi.lib()[ENTRY[kernel][1]], _abi.lib()[ENTRY[kernel][0]]
    for T in (0, 5, -1):
        ybuf, hbuf = _buf(4 * c.N, c.dt), _buf(4 * c.K, c.dt)
        rc = f(*_args(c, d, X_, D, F, ybuf, hbuf), T, _DT[c.dt], _stream())
        assert rc == -1, (T, rc)  # CC_ERR_BAD_ARG
        torch.cuda.synchronize()
        assert (ybuf.float() == SENTINEL).all() and (hbuf.float() == SENTINEL).all(), f"T={T}: an error wrote something"
    # the checks it shares with the single-vector entry point: the same return code, and nothing written
    ybuf = _buf(4 * c.N, c.dt)
    W, sc = _p(d["W"]), _p(d["scales"])
    tail = (None, None, None, 0, 0, _p(ybuf), c.N)  # h_out, bias, freqs, rope_rows, head_dim, y, N
    shared = [((W, sc, None, None, _p(X_), _p(D), None, 0.0, *tail, c.K), _DT[BF], -1),          # delta without norm_w
              ((W, sc, None, None, _p(X_), None, None, 0.0, *tail, 40), _DT[BF], -2),            # K % 16 / K % 32: unsupported
              ((W, sc, None, None, _p(X_), None, None, 0.0, *tail, c.K), _DT[torch.float32], -2)]  # an f32 dtype: unsupported
    for head, dtc, want in shared:
        assert f(*head, 2, dtc, _stream()) == want == f1(*head, dtc, _stream()), (head[-1], dtc)
    torch.cuda.synchronize()
    assert (ybuf.float() == SENTINEL).all()


def _graph_forms(kernel):
    if kernel == "w8":
        ks = E.k_values("w8", BF)
        return [(37, ks[3], "norm+delta+rope+bias"), (29, ks[-3], "norm+delta+pair")]
    return [(37, 2080, "norm+delta+rope+bias"), (29, 14336, "norm+delta+pair")]


@pytest.mark.parametrize("kernel", ["w8", "mx4"])
def test_graph_replay_bit_equal(kernel):
    """one kernel node, no parallel branches"""
    dt = BF
    for n, (N, K, form) in enumerate(_graph_forms(kernel)):
        rows = _rows(kernel, dt, N, K, form, 900 + n)
        c, d = rows[0], _dev0(rows[0])
        X_, D, F = _stack(rows, "x"), _stack(rows, "delta_t"), _stack(rows, "freqs")
        singles = _singles(kernel, c, d, X_, D, F)
        ybuf, hbuf = _buf(4 * N, dt), _buf(4 * K, dt)
        _launch_multi(kernel, c, d, X_, D, F, 4, ybuf, hbuf)
        torch.cuda.synchronize()
        _check(f"{kernel} eager {form} K={K}", rows, singles, 4, ybuf, hbuf)
        yg, hg = _buf(4 * N, dt), _buf(4 * K, dt)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            _launch_multi(kernel, c, d, X_, D, F, 4, yg, hg)
        torch.cuda.current_stream().wait_stream(s)
        yg.fill_(SENTINEL)
        hg.fill_(SENTINEL)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            _launch_multi(kernel, c, d, X_, D, F, 4, yg, hg)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(E.bits(yg), E.bits(ybuf)) and torch.equal(E.bits(hg), E.bits(hbuf)), f"{kernel} {form} K={K}: graph replay != eager"
        _check(f"{kernel} graph {form} K={K}", rows, singles, 4, yg, hg)


# ------------------------------------------------------------------------------------------------ one-hot probes
def _mx4_probe_matrix(N, K, pair):
    """gemv_exact.probe_matrix for the MXFP4 layout: every code and three scale bytes in a pattern of (row, column), so that the
    product with e_j is column j itself, an integer bf16 holds (pair: W holds permitted gate values, W3 the pattern)."""
    i = np.arange(N, dtype=np.int64).reshape(-1, 1)
    k = np.arange(K, dtype=np.int64).reshape(1, -1)
    kb = np.arange(K // 32, dtype=np.int64).reshape(1, -1)
    pat = ((i * 7 + k * 5 + (k // 8) * 3 + (k // 32) + (k // 2048) * 11) % 16).astype(np.uint8)
    sb = (128 + (i * 2 + kb) % 3).astype(np.uint8)
    c = types.SimpleNamespace(N=N, K=K, dt=BF, pair=pair, norm=False, rope_rows=0, hd=0)
    if pair:
        # gate values that are e2m1 magnitudes at scale 2 (1, 2, 3, 4, 6, 8, 12), either sign
        gv = np.array([v for v in E.gate_values(BF) if abs(int(v)) in (1, 2, 3, 4, 6, 8, 12)], np.int64)
        assert len(gv) >= 4
        want = gv[(i * 3 + k + k // 32) % len(gv)]
        codes, sbytes = X._value_to_code(want), np.full((N, K // 32), 128, np.uint8)
        codes3 = np.where((pat & 7) == 0, pat | 1, pat).astype(np.uint8)  # never +-0: a zero factor would hide the gate
        w3 = X.weights_int(codes3, sb).astype(np.float64)
        c.W3, c.scales3 = X.pack(codes3), torch.from_numpy(np.ascontiguousarray(sb))
    else:
        codes, sbytes = pat, sb
        c.W3 = c.scales3 = None
    w = X.weights_int(codes, sbytes).astype(np.float64)
    c.W, c.scales = X.pack(codes), torch.from_numpy(np.ascontiguousarray(sbytes))
    c.nw = c.bias = None

    def column(j):
        v = w[:, j]
        if pair:
            v = E.round_to(BF, E.round_to(BF, E.silu64(v)) * w3[:, j])
        return E.to_dt(BF, v)

    c.column = column
    return c


def _probe_params():
    out = []
    for kernel, dts in (("w8", E.DTYPES["w8"]), ("mx4", (BF,))):
        for dt in dts:
            for pair in (False, True):
                out.append(pytest.param(kernel, dt, pair, id=f"{kernel}-{E.DT_NAME[dt]}-{'pair' if pair else 'plain'}"))
    return out


@pytest.mark.parametrize("kernel,dt,pair", _probe_params())
def test_one_hot_probes_name_the_token_and_the_column(kernel, dt, pair):
    """token t carries x = e_(j+t): row t of y must be column j + t of W, exactly (pair: rnd(silu(W[:, j+t])) * W3[:, j+t]) — a
    token whose output came from another token's input, or from a neighbouring column, shows as the wrong column.  K: the largest of
    the instantiation with the most input chunks per lane."""
    from cold_compress_amd import _abi

    _DT, _p, _stream = _ptrs()
    K = 32768  # 64 KiB of input: 8 (int8) / 4 (MXFP4) chunks per lane
    g = _geometry(kernel, pair, 1, K, dt)
    N = 2 * g.rows + 1
    if kernel == "w8":
        c = E.probe_matrix("w8", dt, N, K, pair, 32)
        cols = E.probe_columns("w8", dt, K, 32)
    else:
        c = _mx4_probe_matrix(N, K, pair)
        cols = E.probe_columns("w4", dt, K, 32)  # (the int4 kernel's chunking: 32 codes per 16-byte load)
    c.rope_rows, c.hd = 0, 0
    d = _dev0(c)
    X_ = torch.zeros((MAX_T, K), dtype=dt, device=DEV)
    for j in cols:
        if j + MAX_T > K:
            continue
        X_.zero_()
        for t in range(MAX_T):
            X_[t, j + t] = 1.0
        ybuf = _buf(MAX_T * N, dt)
        _abi.call(ENTRY[kernel][1], *_args(c, d, X_, None, None, ybuf, None), MAX_T, _DT[dt], _stream())
        y = ybuf[:MAX_T * N].view(MAX_T, N).cpu()
        assert (ybuf[MAX_T * N:].float() == SENTINEL).all(), f"column {j}: wrote behind y"
        for t in range(MAX_T):
            want = c.column(j + t)
            assert torch.equal(E.bits(y[t]), E.bits(want)), f"token {t}, column {j + t}: rows {(E.bits(y[t]) != E.bits(want)).nonzero().flatten().tolist()} " \
                                                            f"got {y[t].float().tolist()} want {want.float().tolist()}"


# ------------------------------------------------------------------------------------------------ the tuning hooks
def _hook_child():
    """run in a child process whose CC_GEMV_W8_CFG / CC_GEMV_MX4_CFG name a geometry the launchers read once: T = 4 against the
    single-vector entry point under the same setting, bit for bit, and the same return code where the setting is not served."""
    import os

    from cold_compress_amd import _abi

    _DT, _p, _stream = _ptrs()
    want_rc = int(os.environ["WO_MULTI_EXPECT_RC"])
    for kernel, K in (("w8", 16384), ("mx4", 2048)):
        rows = _rows(kernel, BF, 37, K, "norm+delta+rope+bias", 41)
        c, d = rows[0], _dev0(rows[0])
        X_, D, F = _stack(rows, "x"), _stack(rows, "delta_t"), _stack(rows, "freqs")
        ybuf, hbuf = _buf(4 * c.N, BF), _buf(4 * c.K, BF)
        y1, h1 = _buf(c.N, BF), _buf(c.K, BF)
        rc1 = _abi.lib()[ENTRY[kernel][0]](*_args(c, d, X_[0], D[0], F[0], y1, h1), _DT[BF], _stream())
        rc4 = _abi.lib()[ENTRY[kernel][1]](*_args(c, d, X_, D, F, ybuf, hbuf), 4, _DT[BF], _stream())
        torch.cuda.synchronize()
        assert rc1 == rc4 == want_rc, (kernel, rc1, rc4, want_rc)
        if want_rc == 0:
            _check(f"{kernel} under the tuning hook", rows, _singles(kernel, c, d, X_, D, F), 4, ybuf, hbuf)
        else:
            assert (ybuf.float() == SENTINEL).all() and (hbuf.float() == SENTINEL).all(), f"{kernel}: an error wrote something"
    print("hook child ok")


@pytest.mark.parametrize("w8_cfg,mx4_cfg,rc", [("2,4,300", "8,1,300", 0), ("4,8", "4,2", -2), ("3,1", "3,1", -2)],
                         ids=["served", "more-column-steps-than-chunks", "no-such-instantiation"])
def test_tuning_hook_geometries_give_the_same_bits_and_the_same_refusals(w8_cfg, mx4_cfg, rc):
    """CC_GEMV_W8_CFG / CC_GEMV_MX4_CFG are read once per process, so each setting runs in a child.  Int8: K = 16384 keeps 4 chunk
    pairs per lane, 2 x 4 is an instantiation of both launchers.  MXFP4: K = 2048 is one segment on one wave; 8 x 1 is served by the
    single-vector launcher only, and the multi launcher runs the shape's default geometry (results do not depend on it).  Settings
    the single-vector entry point refuses are refused alike (CC_ERR_UNSUPPORTED), and nothing is written."""
    import os
    import subprocess
    import sys

    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, CC_GEMV_W8_CFG=w8_cfg, CC_GEMV_MX4_CFG=mx4_cfg, WO_MULTI_EXPECT_RC=str(rc))
    code = f"import sys; sys.path[:0] = [{here!r}, {os.path.dirname(here)!r}]; import test_gpu_gemv_wo_multi as M; M._hook_child()"
    r = subprocess.run([sys.executable, *(["-s"] if sys.flags.no_user_site else []), "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "hook child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
