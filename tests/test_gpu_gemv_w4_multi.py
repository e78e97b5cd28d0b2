"""cc_gemv_fused_w4_multi: the int4 group-wise weight-only GEMV for up to four input vectors from one pass over the weights.
tests/test_gpu_gemv_wo_multi.py for this kernel: the contract is bit identity, row by row, with cc_gemv_fused_w4 — for every form and
shape it serves — so the cases are gemv_exact.gpu_cases("w4"), unchanged (every default instantiation's smallest and largest K, one
chunk either side of each class boundary K = 2048 / 4096 / 8192 / 16384 / 32768, 64 KiB of input with the norm prologue, row counts 1,
rows-per-round -+ 1, odd counts whose RoPE rows end inside a round, two rounds of the row loop, the G = 32 / 128 / 256 picks of that
list), plus a G = 64 case pair per waves-per-row class, each with T = 1, 2, 3 and 4 input rows.

Row t's inputs are the generator's for T different seeds; W, W3, the (scale, zero) words, norm_w and bias are the FIRST case's, so that
one matrix serves all rows.  What is required of row t of y and h_out:
  * bit-equal to cc_gemv_fused_w4 run on row t alone (every form, every row);
  * row 0 bit-equal to the case's integer answer; rows t > 0 of the non-pair forms bit-equal to the integer answer recomputed from the
    first case's codes and row t's input (exact_output(check=False)) WHERE the twin's own bound for the factored int4 form holds for
    that row — the sum of the magnitudes of the factored form's terms (dot_exact's abs_sum) below 2^24, so that every partial sum is
    an integer fp32 holds in any order; a RoPE row needs its pair partner's bound too.  An unrepaired row elsewhere, and every
    pair-form row t > 0 (a gate value may sit on a rounding midpoint of silu), is held to the single kernel alone, which
    tests/test_gpu_gemv_exact.py pins to the integer answers;
  * 64 guard elements behind y and h_out untouched.
Also: T = 0, 5, -1 are CC_ERR_BAD_ARG and write nothing, the shared checks return what the single entry point returns; one-hot probes
where token t carries x = e_(j+t) and must return column j + t; graph replay of a T = 4 launch equals eager; the CC_GEMV_W4_CFG hook in
child processes."""
import copy

import numpy as np
import pytest
import torch

import gemv_exact as E

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
SENTINEL = 1536.0
MAX_T = 4
BF = torch.bfloat16
SINGLE, MULTI = "cc_gemv_fused_w4", "cc_gemv_fused_w4_multi"


def _ptrs():
    from cold_compress_amd.harness.glue import _DT, _p, _stream

    return _DT, _p, _stream


def _rows(N, K, form, seed, G):
    """-> [case 0, composite rows 1..3]: each with .x / .delta_t / .freqs (CPU tensors of this row), the expected .y (None: no
    answer of the twin's) with .y_ok (bool [N]: the rows the twin's 2^24 bound covers) and .h, for the FIRST case's matrix."""
    c0 = E.make_case("w4", BF, N, K, form, seed, G)
    c0.y_ok = torch.ones(N, dtype=torch.bool)
    g = E.geometry("w4", c0.pair, N, K, BF)
    # rows t > 0 only lend their input vectors: a small matrix makes the same ones, with the same head_dim (the generator derives it
    # from the rows per round and the seed's parity)
    n_small = min(N, 2 * g.rows + 3)
    rows = [c0]
    for t in range(1, MAX_T):
        ct = E.make_case("w4", BF, n_small, K, form, seed + 2 * t, G)
        assert ct.hd == c0.hd and (ct.freqs_i is None) == (c0.freqs_i is None)
        k = copy.copy(c0)
        k.x_i, k.delta_i, k.h_i, k.freqs_i = ct.x_i, ct.delta_i, ct.h_i, ct.freqs_i
        k.xin = ct.h_i * c0.nw_i if c0.norm else ct.x_i.copy()
        k.x, k.delta_t, k.freqs, k.h = ct.x, ct.delta_t, ct.freqs, ct.h
        k.y = None
        if not c0.pair:
            y, tol = E.exact_output(k, check=False)  # (leaves the factored form's abs_sum on k)
            assert tol is None
            ok = k.abs_sum < 2.0 ** 24
            if k.freqs_i is not None:
                rr = k.rope_rows
                ok[:rr] &= ok[:rr].reshape(-1, 2)[:, ::-1].reshape(-1)
            k.y, k.y_ok = torch.from_numpy(y).to(BF), torch.from_numpy(ok)
        rows.append(k)
    return rows


def _stack(rows, key):
    ts = [getattr(r, key) for r in rows]
    return None if ts[0] is None else torch.stack(ts).to(DEV).contiguous()


def _dev0(c):
    return {k: (getattr(c, k).to(DEV).contiguous() if getattr(c, k, None) is not None else None)
            for k in ("W", "W3", "scales", "scales3", "nw", "bias")}


def _buf(n):
    return torch.full((n + GUARD,), SENTINEL, dtype=BF, device=DEV)


def _args(c, d, x, dl, fr, ybuf, hbuf):
    _DT, _p, _stream = _ptrs()
    return (_p(d["W"]), _p(d["scales"]), _p(d["W3"]), _p(d["scales3"]), _p(x), _p(dl), _p(d["nw"]), 0.0, _p(hbuf), _p(d["bias"]), _p(fr),
            int(c.rope_rows), int(c.hd), _p(ybuf), c.N, c.K, c.G)


def _launch_multi(c, d, X_, D, F, T, ybuf, hbuf):
    from cold_compress_amd import _abi

    _DT, _p, _stream = _ptrs()
    _abi.call(MULTI, *_args(c, d, X_, D, F, ybuf, hbuf), T, _DT[BF], _stream())


def _singles(c, d, X_, D, F):
    """cc_gemv_fused_w4 on every row alone -> [(y [N], h [K] or None)] on the CPU."""
    from cold_compress_amd import _abi

    _DT, _p, _stream = _ptrs()
    out = []
    for t in range(X_.shape[0]):
        yb, hb = _buf(c.N), (_buf(c.K) if c.norm else None)
        _abi.call(SINGLE, *_args(c, d, X_[t], None if D is None else D[t], None if F is None else F[t], yb, hb), _DT[BF], _stream())
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
        if k.y is not None:
            ne = (E.bits(y[t]) != E.bits(k.y)) & k.y_ok
            if ne.any():
                bad = ne.nonzero().flatten()
                r = int(bad[0])
                raise AssertionError(f"{what} token {t}: {len(bad)} of {int(k.y_ok.sum())} rows inside the twin's bound differ from the "
                                     f"integer answer, first row {r}: {float(y[t][r])} vs {float(k.y[r])}")
        if c.norm:
            assert torch.equal(E.bits(h[t]), E.bits(hs)), f"{what} token {t}: h_out differs from the single-vector kernel"
            assert torch.equal(E.bits(h[t]), E.bits(k.h)), f"{what} token {t}: h_out differs from the exact x + delta"


# a G = 64 pair of cases per waves-per-row class (WS = 1: K <= 2048; WS = 2: K <= 4096; WS = 4 with 1, 2 and 4 segments per wave)
G64_K = (2048, 4096, 8192, 16384, 32768)


def _params():
    out = [pytest.param(N, K, form, seed, G, id=i) for (i, _, N, K, form, G, seed) in E.gpu_cases("w4")]
    for n, K in enumerate(G64_K):
        for form in ("norm+delta+rope+bias", "norm+delta+pair"):
            N = 2 * E.geometry("w4", "pair" in form, 1, K, BF).rows + 3
            out.append(pytest.param(N, K, form, 700 + n, 64, id=f"w4-bf16-N{N}-K{K}-G64-{form}"))
    return out


@pytest.mark.parametrize("N,K,form,seed,G", _params())
def test_gemv_w4_multi_exact(N, K, form, seed, G):
    rows = _rows(N, K, form, seed, G)
    c = rows[0]
    d = _dev0(c)
    X_, D, F = _stack(rows, "x"), _stack(rows, "delta_t"), _stack(rows, "freqs")
    singles = _singles(c, d, X_, D, F)
    key = E.geometry("w4", c.pair, N, K, BF).key
    for T in (1, 2, 3, 4):
        ybuf, hbuf = _buf(T * N), (_buf(T * K) if c.norm else None)
        _launch_multi(c, d, X_, D, F, T, ybuf, hbuf)
        torch.cuda.synchronize()
        _check(f"w4 N={N} K={K} G={G} {form} key {key} T={T}", rows, singles, T, ybuf, hbuf)


def test_the_g64_cases_cover_every_waves_per_row_class():
    assert {E.geometry("w4", False, 1, K, BF).ws for K in G64_K} == {1, 2, 4}
    assert {E.geometry("w4", False, 1, K, BF).xs for K in G64_K} == {1, 2, 4}


def test_token_count_outside_1_to_4_is_a_bad_argument():
    from cold_compress_amd import _abi

    _DT, _p, _stream = _ptrs()
    rows = _rows(9, 512, "norm+delta+rope+bias", 300, 32)
    c, d = rows[0], _dev0(rows[0])
    X_, D, F = _stack(rows, "x"), _stack(rows, "delta_t"), _stack(rows, "freqs")
    f, f1 = _abi.lib()[MULTI], _abi.lib()[SINGLE]
    for T in (0, 5, -1):
        ybuf, hbuf = _buf(4 * c.N), _buf(4 * c.K)
        rc = f(*_args(c, d, X_, D, F, ybuf, hbuf), T, _DT[BF], _stream())
        assert rc == -1, (T, rc)  # CC_ERR_BAD_ARG
        torch.cuda.synchronize()
        assert (ybuf.float() == SENTINEL).all() and (hbuf.float() == SENTINEL).all(), f"T={T}: an error wrote something"
    # the checks it shares with the single-vector entry point: the same return code, and nothing written
    ybuf = _buf(4 * c.N)
    W, sc = _p(d["W"]), _p(d["scales"])
    tail = (None, None, None, 0, 0, _p(ybuf), c.N)  # h_out, bias, freqs, rope_rows, head_dim, y, N
    shared = [((W, sc, None, None, _p(X_), _p(D), None, 0.0, *tail, c.K, 32), _DT[BF], -1),              # delta without norm_w
              ((W, sc, None, None, _p(X_), None, None, 0.0, *tail, 480, 64), _DT[BF], -2),               # K not a multiple of G
              ((W, sc, None, None, _p(X_), None, None, 0.0, *tail, c.K, 48), _DT[BF], -1),               # G = 48
              ((W, sc, None, None, _p(X_), None, None, 0.0, *tail, c.K, 32), _DT[torch.float16], -2),    # an f16 dtype
              ((W, None, None, None, _p(X_), None, None, 0.0, *tail, c.K, 32), _DT[BF], -1),             # no (scale, zero) words
              ((W, sc, None, sc, _p(X_), None, None, 0.0, *tail, c.K, 32), _DT[BF], -1)]                 # qparams3 without W3
    for head, dtc, want in shared:
        assert f(*head, 2, dtc, _stream()) == want == f1(*head, dtc, _stream()), (head[-2:], dtc)
    torch.cuda.synchronize()
    assert (ybuf.float() == SENTINEL).all()


def test_misaligned_pointers_are_a_bad_argument():
    """the multi entry point's own check: 16-byte alignment of W, x, delta, norm_w and h_out, 4 bytes for the (scale, zero) words"""
    from cold_compress_amd import _abi
    import ctypes as C

    _DT, _p, _stream = _ptrs()
    rows = _rows(9, 512, "norm+delta", 301, 32)
    c, d = rows[0], _dev0(rows[0])
    X_, D = _stack(rows, "x"), _stack(rows, "delta_t")
    f = _abi.lib()[MULTI]
    ybuf, hbuf = _buf(4 * c.N), _buf(4 * c.K)
    base = list(_args(c, d, X_, D, None, ybuf, hbuf))
    assert f(*base, 2, _DT[BF], _stream()) == 0
    torch.cuda.synchronize()
    ybuf.fill_(SENTINEL)
    hbuf.fill_(SENTINEL)
    for idx, off in ((0, 8), (1, 2), (4, 2), (5, 8), (6, 4), (8, 2)):  # W, qparams, x, delta, norm_w, h_out
        a = list(base)
        a[idx] = C.c_void_p(a[idx].value + off)
        assert f(*a, 2, _DT[BF], _stream()) == -1, idx
    torch.cuda.synchronize()
    assert (ybuf.float() == SENTINEL).all() and (hbuf.float() == SENTINEL).all()


def test_graph_replay_bit_equal():
    """one kernel node, no parallel branches"""
    for n, (N, K, form) in enumerate([(37, 2080, "norm+delta+rope+bias"), (29, 14336, "norm+delta+pair")]):
        rows = _rows(N, K, form, 900 + n, 32)
        c, d = rows[0], _dev0(rows[0])
        X_, D, F = _stack(rows, "x"), _stack(rows, "delta_t"), _stack(rows, "freqs")
        singles = _singles(c, d, X_, D, F)
        ybuf, hbuf = _buf(4 * N), _buf(4 * K)
        _launch_multi(c, d, X_, D, F, 4, ybuf, hbuf)
        torch.cuda.synchronize()
        _check(f"w4 eager {form} K={K}", rows, singles, 4, ybuf, hbuf)
        yg, hg = _buf(4 * N), _buf(4 * K)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            _launch_multi(c, d, X_, D, F, 4, yg, hg)
        torch.cuda.current_stream().wait_stream(s)
        yg.fill_(SENTINEL)
        hg.fill_(SENTINEL)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            _launch_multi(c, d, X_, D, F, 4, yg, hg)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(E.bits(yg), E.bits(ybuf)) and torch.equal(E.bits(hg), E.bits(hbuf)), f"w4 {form} K={K}: graph replay != eager"
        _check(f"w4 graph {form} K={K}", rows, singles, 4, yg, hg)


# ------------------------------------------------------------------------------------------------ one-hot probes
@pytest.mark.parametrize("pair", [False, True], ids=["plain", "pair"])
def test_one_hot_probes_name_the_token_and_the_column(pair):
    """token t carries x = e_(j+t): row t of y must be column j + t of the dequantised W, exactly (pair: rnd(silu(W[:, j+t])) *
    W3[:, j+t]) — a token whose output came from another token's input, or from a neighbouring column, shows as the wrong column.
    K = 32768: four input chunks per lane and token."""
    from cold_compress_amd import _abi

    _DT, _p, _stream = _ptrs()
    K, G = 32768, 32
    N = 2 * E.geometry("w4", pair, 1, K, BF).rows + 1
    c = E.probe_matrix("w4", BF, N, K, pair, G)
    c.rope_rows, c.hd = 0, 0
    d = _dev0(c)
    X_ = torch.zeros((MAX_T, K), dtype=BF, device=DEV)
    for j in E.probe_columns("w4", BF, K, G):
        if j + MAX_T > K:
            continue
        X_.zero_()
        for t in range(MAX_T):
            X_[t, j + t] = 1.0
        ybuf = _buf(MAX_T * N)
        _abi.call(MULTI, *_args(c, d, X_, None, None, ybuf, None), MAX_T, _DT[BF], _stream())
        y = ybuf[:MAX_T * N].view(MAX_T, N).cpu()
        assert (ybuf[MAX_T * N:].float() == SENTINEL).all(), f"column {j}: wrote behind y"
        for t in range(MAX_T):
            want = c.column(j + t)
            assert torch.equal(E.bits(y[t]), E.bits(want)), f"token {t}, column {j + t}: rows {(E.bits(y[t]) != E.bits(want)).nonzero().flatten().tolist()} " \
                                                            f"got {y[t].float().tolist()} want {want.float().tolist()}"


# ------------------------------------------------------------------------------------------------ the tuning hook
def _hook_child():
    """run in a child process whose CC_GEMV_W4_CFG names a geometry the launcher reads once: T = 4 against the single-vector entry
    point under the same setting, bit for bit, and the same return code where the setting is not served."""
    import os

    from cold_compress_amd import _abi

    _DT, _p, _stream = _ptrs()
    want_rc = int(os.environ["W4_MULTI_EXPECT_RC"])
    for K, form in ((2048, "norm+delta+rope+bias"), (2048, "norm+delta+pair")):
        rows = _rows(37, K, form, 41, 32)
        c, d = rows[0], _dev0(rows[0])
        X_, D, F = _stack(rows, "x"), _stack(rows, "delta_t"), _stack(rows, "freqs")
        ybuf, hbuf = _buf(4 * c.N), _buf(4 * c.K)
        y1, h1 = _buf(c.N), _buf(c.K)
        rc1 = _abi.lib()[SINGLE](*_args(c, d, X_[0], D[0], None if F is None else F[0], y1, h1), _DT[BF], _stream())
        rc4 = _abi.lib()[MULTI](*_args(c, d, X_, D, F, ybuf, hbuf), 4, _DT[BF], _stream())
        torch.cuda.synchronize()
        assert rc1 == rc4 == want_rc, (form, rc1, rc4, want_rc)
        if want_rc == 0:
            _check(f"w4 {form} under the tuning hook", rows, _singles(c, d, X_, D, F), 4, ybuf, hbuf)
        else:
            assert (ybuf.float() == SENTINEL).all() and (hbuf.float() == SENTINEL).all(), f"{form}: an error wrote something"
    print("hook child ok")


@pytest.mark.parametrize("cfg,rc", [("4,1,2", 0), ("8,1,2", 0), ("4,2", -2), ("3,1", -2)],
                         ids=["served", "mapped-to-the-default", "more-column-steps-than-chunks", "no-such-instantiation"])
def test_tuning_hook_geometries_give_the_same_bits_and_the_same_refusals(cfg, rc):
    """CC_GEMV_W4_CFG is read once per process, so each setting runs in a child.  K = 2048 is one segment on one wave: 4 x 1 is the
    class's default and an instantiation of both kernels — its cap of 2 workgroups makes 37 rows two rounds of the row loop; 8 x 1 is
    served by the single-vector kernel only, and the multi launcher runs the default geometry under the same cap (results do not
    depend on it).  Settings the single-vector entry point refuses are refused alike (CC_ERR_UNSUPPORTED), and nothing is written."""
    import os
    import subprocess
    import sys

    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, CC_GEMV_W4_CFG=cfg, W4_MULTI_EXPECT_RC=str(rc))
    code = f"import sys; sys.path[:0] = [{here!r}, {os.path.dirname(here)!r}]; import test_gpu_gemv_w4_multi as M; M._hook_child()"
    r = subprocess.run([sys.executable, *(["-s"] if sys.flags.no_user_site else []), "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "hook child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
