"""cc_gemv_fused_mx4 on inputs whose answer does not depend on the summation order (tests/gemv_mx4_exact.py): every instantiation a
default launch can select, at one block, one chunk either side of every segment-count / waves-per-row / step boundary, the 8B and
70B w2 lengths and K * 2 = 64 KiB (with the RMSNorm prologue that is 64 KiB of dynamic LDS beside the static arrays), with 1,
rows-per-round -+ 1, 38 rows, odd counts whose RoPE rows end inside a round, and two rounds of the row loop at each instantiation's
smallest K.  y and h_out are compared BIT FOR BIT with the integer reference, and the 64 elements behind each must be untouched;
graph replay equals eager."""
import pytest
import torch

import gemv_mx4_exact as X

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
SENTINEL = 1536.0
BF = torch.bfloat16


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

    _abi.call("cc_gemv_fused_mx4", _p(d["W"]), _p(d["scales"]), _p(d["W3"]), _p(d["scales3"]), _p(d["x"]), _p(d["delta_t"]), _p(d["nw"]),
              0.0, _p(hbuf), _p(d["bias"]), _p(d["freqs"]), int(c.rope_rows), int(c.hd), _p(ybuf), c.N, c.K, _DT[BF], _stream())


def _buffers(c):
    ybuf = torch.full((c.N + GUARD,), SENTINEL, dtype=BF, device=DEV)
    hbuf = torch.full((c.K + GUARD,), SENTINEL, dtype=BF, device=DEV) if c.norm else None
    return ybuf, hbuf


def _assert_exact(c, ybuf, hbuf, what):
    y = ybuf[:c.N].cpu()
    assert (ybuf[c.N:].float() == SENTINEL).all(), f"{what}: wrote behind y"
    if not torch.equal(X.bits(y), X.bits(c.y)):
        bad = (X.bits(y) != X.bits(c.y)).nonzero().flatten()
        r = int(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {c.N} rows differ, first row {r}: got {float(y[r])}, exact {float(c.y[r])}")
    if c.norm:
        assert torch.equal(X.bits(hbuf[:c.K].cpu()), X.bits(c.h)), f"{what}: h_out"
        assert (hbuf[c.K:].float() == SENTINEL).all(), f"{what}: wrote behind h_out"


@pytest.mark.parametrize("N,K,form,seed", [pytest.param(N, K, form, seed, id=i) for (i, N, K, form, seed) in X.gpu_cases()])
def test_gemv_mx4_exact(N, K, form, seed):
    c = X.make_case(N, K, form, seed)
    ybuf, hbuf = _buffers(c)
    _launch(c, _dev(c), ybuf, hbuf)
    torch.cuda.synchronize()
    _assert_exact(c, ybuf, hbuf, f"mx4 N={N} K={K} {form} key {X.geometry(c.pair, N, K).key}")


def test_graph_replay_bit_equal():
    for n, (N, K, form) in enumerate([(37, 2080, "norm+delta+rope+bias"), (29, 14336, "norm+delta+pair"), (21, 32768, "plain")]):
        c = X.make_case(N, K, form, seed=900 + n)
        d = _dev(c)
        ybuf, hbuf = _buffers(c)
        _launch(c, d, ybuf, hbuf)
        torch.cuda.synchronize()
        _assert_exact(c, ybuf, hbuf, f"eager {form} K={K}")
        yg, hg = _buffers(c)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            _launch(c, d, yg, hg)
        torch.cuda.current_stream().wait_stream(s)
        yg.fill_(SENTINEL)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            _launch(c, d, yg, hg)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(X.bits(yg), X.bits(ybuf)), f"{form} K={K}: graph replay != eager"
        _assert_exact(c, yg, hg, f"graph {form} K={K}")


def test_norm_prologue_at_64k_of_input():
    """K = 32768: the norm forms ask for K * 2 = 64 KiB of dynamic LDS beside their static arrays, and glue.gemv_supported admits the
    shape.  The launch must succeed and be exact (plain rows and the SwiGLU pair)."""
    from cold_compress_amd.harness import glue

    for form in ("norm+delta", "norm+delta+pair", "norm+delta+rope+bias"):
        c = X.make_case(19, 32768, form, seed=77)
        d = _dev(c)
        assert glue.gemv_supported(d["W"])
        ybuf, hbuf = _buffers(c)
        _launch(c, d, ybuf, hbuf)
        torch.cuda.synchronize()
        _assert_exact(c, ybuf, hbuf, f"K=32768 {form}")
