"""cc_gemv_fused / cc_gemv_fused_w8 / cc_gemv_fused_w4 on inputs whose answer does not depend on the summation order
(tests/gemv_exact.py): every instantiation a default launch can select, at the smallest and largest K of its class and one chunk
either side of every class boundary, K * sizeof = 64 KiB included (for int8 / int4 with the RMSNorm prologue that is 64 KiB of
dynamic LDS on top of the static arrays), with 1, rows-per-round -+ 1 rows, odd counts whose RoPE rows end inside a round, two rounds
of the row loop at each instantiation's smallest K, and 32768 / 32771 rows for the many-rows branch.

y and h_out are compared BIT FOR BIT with the integer reference, and the 64 elements behind each must be untouched.  The only
tolerance is the fp32 RMSNorm forms': |y - exact| <= 2^-22 sum_k |W_ik in_k| (rsqrtf's ulp is not rounded away in fp32).
One-hot probes (x = e_j, y must be column j) name the (row, column) of an addressing mistake; graph replay equals eager."""
import functools

import pytest
import torch

import gemv_exact as E

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64


def _sentinel(dt):
    return 1536.0


def _dev(c):
    d = {}
    for k in ("W", "W3", "scales", "scales3", "x", "delta_t", "nw", "bias", "freqs"):
        t = getattr(c, k, None)
        d[k] = t.to(DEV).contiguous() if t is not None else None
    return d


def _launch(c, d, ybuf, hbuf):
    """the C entry point itself (glue.gemv_fused's argument order), writing into caller buffers that carry a guard region."""
    from cold_compress_amd import _abi
    from cold_compress_amd.harness.glue import _DT, _p, _stream

    common = (_p(d["x"]), _p(d["delta_t"]), _p(d["nw"]), 0.0, _p(hbuf), _p(d["bias"]), _p(d["freqs"]), int(c.rope_rows), int(c.hd),
              _p(ybuf), c.N, c.K)
    if c.kernel == "16":
        _abi.call("cc_gemv_fused", _p(d["W"]), _p(d["W3"]), *common, _DT[c.dt], _stream())
    elif c.kernel == "w8":
        _abi.call("cc_gemv_fused_w8", _p(d["W"]), _p(d["scales"]), _p(d["W3"]), _p(d["scales3"]), *common, _DT[c.dt], _stream())
    else:
        _abi.call("cc_gemv_fused_w4", _p(d["W"]), _p(d["scales"]), _p(d["W3"]), _p(d["scales3"]), *common, int(c.G), _DT[c.dt], _stream())


def _buffers(c):
    ybuf = torch.full((c.N + GUARD,), _sentinel(c.dt), dtype=c.dt, device=DEV)
    hbuf = torch.full((c.K + GUARD,), _sentinel(c.dt), dtype=c.dt, device=DEV) if c.norm else None
    return ybuf, hbuf


def _assert_exact(c, ybuf, hbuf, what):
    y = ybuf[:c.N].cpu()
    assert (ybuf[c.N:].float() == _sentinel(c.dt)).all(), f"{what}: wrote behind y"
    if c.tol is None:
        if not torch.equal(E.bits(y), E.bits(c.y)):
            bad = (E.bits(y) != E.bits(c.y)).nonzero().flatten()
            r = int(bad[0])
            raise AssertionError(f"{what}: {len(bad)} of {c.N} rows differ, first row {r}: got {float(y[r])}, exact {float(c.y[r])}")
    else:
        err = (y.double() - c.y.double()).abs()
        assert (err <= c.tol).all(), f"{what}: row {int((err - c.tol).argmax())} off by {float((err - c.tol).max())} beyond the fp32 norm bound"
    if c.norm:
        assert torch.equal(E.bits(hbuf[:c.K].cpu()), E.bits(c.h)), f"{what}: h_out"
        assert (hbuf[c.K:].float() == _sentinel(c.dt)).all(), f"{what}: wrote behind h_out"


def _params(kernel):
    return [pytest.param(kernel, dt, N, K, form, G, seed, id=i) for (i, dt, N, K, form, G, seed) in E.gpu_cases(kernel)]


@pytest.mark.parametrize("kernel,dt,N,K,form,G,seed", _params("16") + _params("w8") + _params("w4"))
def test_gemv_exact(kernel, dt, N, K, form, G, seed):
    c = E.make_case(kernel, dt, N, K, form, seed, G)
    ybuf, hbuf = _buffers(c)
    _launch(c, _dev(c), ybuf, hbuf)
    torch.cuda.synchronize()
    _assert_exact(c, ybuf, hbuf, f"{kernel} {E.DT_NAME[dt]} N={N} K={K} {form} key {E.geometry(kernel, c.pair, N, K, dt).key}")


def _probe_params():
    out = []
    for kernel in E.KERNELS:
        for dt in E.DTYPES[kernel]:
            seen = set()
            for K in reversed(E.k_values(kernel, dt)):  # the largest K of every instantiation
                for pair in (False, True):
                    key = E.geometry(kernel, pair, 1, K, dt).key
                    if key in seen or (pair and dt == E.F32):
                        continue
                    seen.add(key)
                    out.append(pytest.param(kernel, dt, K, pair, id=f"{kernel}-{E.DT_NAME[dt]}-K{K}-{'pair' if pair else 'plain'}-key{key}"))
    return out


@pytest.mark.parametrize("kernel,dt,K,pair", _probe_params())
def test_one_hot_probes(kernel, dt, K, pair):
    """x = e_j for j at the edges of every index the kernel computes: y must be column j of W, exactly (pair: rnd(silu(W[:, j])) *
    W3[:, j]).  A failure names the row and the column."""
    g = E.geometry(kernel, pair, 1, K, dt)
    N = 2 * g.rows + 1
    G = 256 if kernel == "w4" and K % 256 == 0 else 32
    c = E.probe_matrix(kernel, dt, N, K, pair, G)
    d = _dev(c)
    for j in E.probe_columns(kernel, dt, K, G):
        d["x"].zero_()
        d["x"][j] = 1.0
        ybuf, _ = _buffers(c)
        _launch(c, d, ybuf, None)
        y = ybuf[:N].cpu()
        want = c.column(j)
        assert torch.equal(E.bits(y), E.bits(want)), f"column {j}: rows {(E.bits(y) != E.bits(want)).nonzero().flatten().tolist()} got " \
                                                      f"{y.float().tolist()} want {want.float().tolist()}"
        assert (ybuf[N:].float() == _sentinel(dt)).all(), f"column {j}: wrote behind y"


@functools.lru_cache(maxsize=None)
def _graph_cases(kernel):
    dt = E.BF
    ks = E.k_values(kernel, dt)
    return [(dt, 37, ks[3], "norm+delta+rope+bias"), (dt, 29, ks[-3], "norm+delta+pair"), (dt, 21, ks[-1], "plain")]


@pytest.mark.parametrize("kernel", E.KERNELS)
def test_graph_replay_bit_equal(kernel):
    for n, (dt, N, K, form) in enumerate(_graph_cases(kernel)):
        c = E.make_case(kernel, dt, N, K, form, seed=900 + n, G=32)
        d = _dev(c)
        ybuf, hbuf = _buffers(c)
        _launch(c, d, ybuf, hbuf)
        torch.cuda.synchronize()
        _assert_exact(c, ybuf, hbuf, f"{kernel} eager {form} K={K}")
        yg, hg = _buffers(c)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            _launch(c, d, yg, hg)
        torch.cuda.current_stream().wait_stream(s)
        yg.fill_(_sentinel(dt))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            _launch(c, d, yg, hg)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(E.bits(yg), E.bits(ybuf)), f"{kernel} {form} K={K}: graph replay != eager"
        _assert_exact(c, yg, hg, f"{kernel} graph {form} K={K}")


@pytest.mark.parametrize("kernel", ["w8", "w4"])
def test_norm_prologue_at_64k_of_input(kernel):
    """K = 32768: the int8 / int4 norm forms ask for K * 2 = 64 KiB of dynamic LDS beside their static arrays, and
    glue.gemv_supported admits the shape.  The launch must succeed and be exact (plain rows and the SwiGLU pair)."""
    from cold_compress_amd.harness import glue

    for form in ("norm+delta", "norm+delta+pair", "norm+delta+rope+bias"):
        c = E.make_case(kernel, E.BF, 19, 32768, form, seed=77, G=256 if kernel == "w4" else 32)
        d = _dev(c)
        assert glue.gemv_supported(d["W"])
        ybuf, hbuf = _buffers(c)
        _launch(c, d, ybuf, hbuf)
        torch.cuda.synchronize()
        _assert_exact(c, ybuf, hbuf, f"{kernel} K=32768 {form}")
