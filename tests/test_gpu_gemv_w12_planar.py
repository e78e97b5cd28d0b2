"""cc_gemv_fused_w12 over the PLANAR layout of the packed copy (layout id 1 in bits 8 .. 15 of the rb word) against cc_gemv_fused
itself: y and h_out equal BIT FOR BIT in every form, at the six shapes, four weight kinds and four forms of test_gpu_gemv_w12.py
(whose weight builders this file imports and leaves alone), plus one small shape per planar instantiation, asserted through
cc_w12_geometry to be the one launched.  Also: the numpy decoder of tests/w12_planar.py brings all 65536 bf16 patterns back; a
tensor whose fullest window of 16 exponents starts at an odd exponent gets an even base and patched escapes; ±0, a subnormal, ±inf
and a NaN payload planted at chunk positions 3, 4 and 7 (the weights whose sign bit lives in a neighbouring byte) in lanes 0 and
63; a copy handed in under the other layout's id is refused before anything is launched; the tiny harness model with the planar
path forced on every linear decodes the tokens and probability rows of CC_W12=0, eager and graphed; and the default rule."""
import argparse

import numpy as np
import pytest
import torch

import test_gpu_gemv_w12 as T12
import w12_planar as WP

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
PLANAR = 1
_bits, _p, _stream = T12._bits, T12._p, T12._stream


def _pack(w, pair, layout=PLANAR):
    from cold_compress_amd.harness import glue

    return glue.w12_pack(w, pair, refuse=False, layout=layout)


def _call12(pk, pk3, W, W3, x, form, N, K, layout=None):
    from cold_compress_amd import _abi

    layout = pk.layout if layout is None else layout
    y = torch.full((N,), 7.0, dtype=BF, device=DEV)
    h = torch.full((K,), 7.0, dtype=BF, device=DEV) if form.get("h_out") else None
    _abi.call("cc_gemv_fused_w12", _p(pk.codes), _p(pk.records), pk.base, _p(pk3.codes) if pk3 else None, _p(pk3.records) if pk3 else None,
              pk3.base if pk3 else 0, pk.rb | layout << 8, pk.cu, _p(W), _p(W3), _p(x), _p(form.get("delta")), _p(form.get("norm_weight")),
              1e-5, _p(h), _p(form.get("bias")), _p(form.get("freqs")), form.get("rope_rows", 0), form.get("head_dim", 0), _p(y), N, K,
              _abi.CC_DT_BF16, _stream())
    return y, h


def _check_forms(N, K, gen, make, forms=None, after_pack=None):
    """For every form: pack what `make(geo)` builds in the planar layout and compare the packed launch with the dense one."""
    from cold_compress_amd.harness import glue

    x = torch.randn(K, generator=gen, device=DEV).to(BF)
    for fname, form in T12._forms(N, K, gen).items():
        if forms is not None and fname not in forms:
            continue
        pair = bool(form.get("swiglu"))
        geo = glue.w12_geometry(N, K, pair, PLANAR)
        assert geo is not None
        W = make(geo)
        W3 = make(geo) if pair else None
        pk = _pack(W, pair)
        pk3 = _pack(W3, pair) if pair else None
        for p in (pk, pk3):
            if p is not None:
                assert p.layout == PLANAR and p.base % 2 == 0, p.base
                if after_pack:
                    after_pack(p)
        y0, h0 = T12._call("cc_gemv_fused", None, None, W, W3, x, form, N, K)
        y1, h1 = _call12(pk, pk3, W, W3, x, form, N, K)
        assert torch.equal(_bits(y0), _bits(y1)), (fname, int((_bits(y0) != _bits(y1)).sum()))
        if h0 is not None:
            assert torch.equal(_bits(h0), _bits(h1)), fname


@pytest.mark.parametrize("kind", ["normal", "zeros", "esc7", "esc8"])
@pytest.mark.parametrize("shape", range(6), ids=T12.SHAPES)
def test_planar_equals_dense_bit_for_bit(shape, kind):
    N, K = T12._shapes()[shape]
    gen = torch.Generator(device=DEV).manual_seed(100 * shape + len(kind))

    def after_pack(p):
        first = p.records[:, 0]
        if kind == "esc7":
            assert p.n_overflow == 0 and int(first.max()) == 7 and int(first[0]) == 7, (p.n_overflow, first[:8].tolist())
        if kind == "esc8":
            assert p.n_overflow == 1 and int(first[0]) == T12.OVERFLOW, (p.n_overflow, first[:8].tolist())

    _check_forms(N, K, gen, lambda geo: T12._weights(kind, N, K, geo, gen), after_pack=after_pack)


# one small shape per planar instantiation of gemv_w12_kernel: (N, K, form, (RB, CU, XS)).  (9, 4104): three column steps per wave.
INSTANCES = [(7, 520, "plain", (4, 2, 2)), (32768 + 5, 64, "plain", (2, 2, 2)), (9, 4104, "plain", (4, 4, 8)),
             (7, 520, "swiglu", (2, 2, 2)), (9, 4104, "swiglu", (2, 4, 8))]


@pytest.mark.parametrize("case", INSTANCES, ids=lambda c: f"{c[2]}-{c[3][0]}x{c[3][1]}x{c[3][2]}")
def test_planar_every_instantiation_is_launched_and_exact(case):
    from cold_compress_amd.harness import glue

    N, K, fname, inst = case
    assert glue.w12_geometry(N, K, fname == "swiglu", PLANAR)[:3] == inst
    gen = torch.Generator(device=DEV).manual_seed(N + K)
    for kind in ("normal", "zeros"):
        _check_forms(N, K, gen, lambda geo: T12._weights(kind, N, K, geo, gen), forms=("plain", "norm", "bias_rope") if fname == "plain" else (fname,))


def _round_trip(pk, w):
    N, K = w.shape
    back, overflow = WP.decode_tensor(pk.codes.cpu().numpy().view(np.uint32), pk.records.cpu().numpy().view(np.uint32), pk.base, pk.rb,
                                      pk.cu, N, K)
    return np.array_equal(back, w.view(torch.int16).cpu().numpy().view(np.uint16)), overflow


def test_planar_round_trip_of_all_65536_patterns():
    """Row i carries pattern i at column (37 i) mod K among in-window fillers: every record holds at most RB <= 4 escapes."""
    N, K = 65536, 256
    w = torch.full((N, K), 0.0234375, dtype=BF, device=DEV)
    rows = torch.arange(N, device=DEV)
    w.view(torch.int16)[rows, (rows * 37) % K] = (rows - 65536 * (rows >= 32768)).to(torch.int16)
    pk = _pack(w, False)
    assert pk.base % 2 == 0
    assert pk.n_overflow == 0 and pk.n_escapes == 65536 - 16 * 256, (pk.n_overflow, pk.n_escapes)
    same, overflow = _round_trip(pk, w)
    assert overflow == 0 and same


def test_planar_fullest_window_at_an_odd_exponent_gets_an_even_base():
    """Exponents 110 .. 123 everywhere, 20 weights at 109 and 10 at 124 (one per row): the fullest window of 16 starts at 109, which
    the first layout takes; planar has to choose between 108 (10 escapes) and 110 (20) and patches the ten."""
    N, K = 64, 1024
    gen = torch.Generator(device=DEV).manual_seed(5)
    e = torch.randint(110, 124, (N, K), generator=gen, device=DEV)
    sm = torch.randint(0, 256, (N, K), generator=gen, device=DEV)
    for r in range(20):
        e[r, (r * 53) % K] = 109
    for r in range(32, 42):
        e[r, (r * 29 + 4) % K] = 124
    v = ((sm >> 7) << 15) | (e << 7) | (sm & 127)
    w = (v - 65536 * (v >= 32768)).to(torch.int16).view(BF).contiguous()
    assert _pack(w, False, layout=0).base == 109
    pk = _pack(w, False)
    assert pk.base == 108 and pk.n_escapes == 10 and pk.n_overflow == 0, (pk.base, pk.n_escapes, pk.n_overflow)
    same, overflow = _round_trip(pk, w)
    assert overflow == 0 and same
    _check_forms(N, K, gen, lambda geo: w, forms=("plain", "norm"))


def test_planar_planted_patterns_at_the_neighbour_sign_positions():
    """±0, a subnormal, ±inf and a NaN payload at chunk positions 3, 4 and 7 of lanes 0 and 63 (chunks 0 and 63 of a row: wave 0's
    first request), pattern p in row 4 p: six escapes in each of six records, none overflowing, in both launch forms."""
    N, K = 24, 4096
    pats = [0x0000, 0x8000, 0x0001, 0x7F80, 0xFF80, 0x7FC1]
    where = [(4 * p, chunk * 8 + pos) for p in range(6) for chunk in (0, 63) for pos in (3, 4, 7)]
    gen = torch.Generator(device=DEV).manual_seed(9)

    def make(geo):
        return T12._plant(T12._windowed(N, K, gen), where, [pats[r // 4] for r, _ in where])

    def after_pack(p):
        assert p.n_escapes == 36 and p.n_overflow == 0 and int(p.records[:, 0].max()) == 6, (p.n_escapes, p.n_overflow)

    _check_forms(N, K, gen, make, after_pack=after_pack)
    w = make(None)
    pk = _pack(w, False)
    same, overflow = _round_trip(pk, w)
    assert overflow == 0 and same


def test_planar_copy_under_the_other_layout_id_is_refused():
    from cold_compress_amd import _abi

    N, K = 10, 4096
    gen = torch.Generator(device=DEV).manual_seed(4)
    W = T12._normal(N, K, gen)
    x = torch.randn(K, generator=gen, device=DEV).to(BF)
    for layout in (PLANAR, 0):
        pk = _pack(W, False, layout=layout)
        assert pk.layout == layout
        with pytest.raises(_abi.ColdCompressError):
            _call12(pk, None, W, None, x, {}, N, K, layout=1 - layout)
        y, _ = _call12(pk, None, W, None, x, {}, N, K)  # under its own id it runs
        y0, _ = T12._call("cc_gemv_fused", None, None, W, None, x, {}, N, K)
        assert torch.equal(_bits(y), _bits(y0))
    # nothing is launched by a refused call: y keeps its fill
    from cold_compress_amd.harness import glue

    y = torch.full((N,), 7.0, dtype=BF, device=DEV)
    rc = _abi.lib()["cc_gemv_fused_w12"](_p(pk.codes), _p(pk.records), pk.base, None, None, 0, pk.rb | PLANAR << 8, pk.cu, _p(W), None,
                                         _p(x), None, None, 1e-5, None, None, None, 0, 0, _p(y), N, K, _abi.CC_DT_BF16, _stream())
    torch.cuda.synchronize()
    assert rc != _abi.CC_OK and bool((y == 7.0).all())
    with pytest.raises(_abi.ColdCompressError):  # an unknown layout id
        _abi.call("cc_w12_pack", _p(W), N, K, pk.rb | 2 << 8, pk.cu, _p(pk.codes), _p(pk.records), _p(pk.records), _stream())
    glue.w12_cache_clear()


def test_planar_tiny_model_decodes_the_same_forced_on_every_linear(monkeypatch):
    """8 greedy tokens of the tiny harness model, eager and graphed: the planar path forced on wqkv, wo, the w1/w3 pair, w2 and the
    LM head gives the tokens and probability rows of CC_W12=0, bit for bit, and no dense GEMV is launched in the forced eager run."""
    import cold_compress_amd.cache as cache
    from cold_compress_amd import _abi
    from cold_compress_amd.harness import CONFIGS, GraphedDecoder, ModelArgs, Transformer, decode_one_token, glue, prefill, setup_caches

    torch.manual_seed(11)
    cfg = dict(CONFIGS["tiny"])
    model = Transformer(ModelArgs(**cfg)).to(BF).eval().to(DEV)
    ap = argparse.ArgumentParser()
    cache.add_cache_arguments(ap)
    kw = vars(ap.parse_args([]))
    kw.update(dict(cache_strategy=["full"], prompt_compression_strategy=["full"], max_cache_length=[1.0]))
    P, T = 20, 8
    setup_caches(model, None, DEV, P + T + 8, dict(kw))
    prompt = torch.randint(0, cfg["vocab_size"], (P,), generator=torch.Generator().manual_seed(1), dtype=torch.int32).to(DEV)
    calls = []
    real_call, real_gemv = _abi.call, glue.gemv_fused
    monkeypatch.setattr(_abi, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])
    monkeypatch.setattr(glue, "gemv_fused", lambda *a, **k: real_gemv(*a, **{**k, "w12": "force-planar" if k.get("w12") else False}))

    def run(w12, graphed):
        monkeypatch.setenv("CC_W12", "1" if w12 else "0")
        calls.clear()
        model.reset_caches()
        dec = GraphedDecoder(model) if graphed else None
        toks, probs = [], []
        with torch.no_grad():
            cur, _ = prefill(model, prompt.view(1, -1), torch.arange(P, device=DEV))
            cur = cur.view(1, 1).to(torch.int32)
            pos = torch.tensor([P], dtype=torch.int32, device=DEV)
            for _ in range(T):
                nt, pr = (dec or decode_one_token)(model, cur, pos)
                toks.append(int(nt.view(-1)[0]))
                probs.append(pr.clone())
                cur = nt.view(1, 1).to(torch.int32).clone()
                pos += 1
        torch.cuda.synchronize()
        return toks, torch.stack([p.view(-1) for p in probs])

    ref = run(False, False)
    assert "cc_gemv_fused_w12" not in calls
    for graphed in (False, True):
        toks, probs = run(True, graphed)
        if not graphed:
            n12 = calls.count("cc_gemv_fused_w12")
            assert "cc_gemv_fused" not in calls and n12 >= T * (3 * cfg["n_layer"] + 1), (n12, set(calls))
        assert toks == ref[0], graphed
        assert torch.equal(probs.view(torch.int32) if probs.dtype == torch.float32 else _bits(probs),
                           ref[1].view(torch.int32) if ref[1].dtype == torch.float32 else _bits(ref[1])), graphed
    assert all(k[5] == PLANAR for k, (p, _) in glue._w12_cache.items() if p is not None)
    glue.w12_cache_clear()


def test_planar_is_on_by_default_only_where_it_measured_faster(monkeypatch):
    """cc_w12_geometry's fifth word for the planar layout: the SwiGLU pair and plain matrices of 32768 rows or more at K <= 4096 —
    the two launch classes in which planar beat the dense kernel and the first layout by more than the dense kernel's own spread
     — and only with a full grid, N >= RB x workgroups, the regime measured.  wqkv, wo and w2 lost to the dense
    kernel and answer 0; K = 8192 is not enabled.  gemv_fused(w12=True) takes planar where it answers 1, the first layout where
    only that one answers 1 (a small pair), and packs nothing elsewhere."""
    from cold_compress_amd import _abi
    from cold_compress_amd.harness import glue

    monkeypatch.delenv("CC_W12", raising=False)
    on = lambda N, K, pair=False: glue.w12_geometry(N, K, pair, PLANAR)[4]  # noqa: E731
    assert on(14336, 4096, True) == 1 and on(128256, 4096) == 1 and on(32768, 512) == 1 and on(4096, 512, True) == 1
    assert on(4096, 4096) == 0 and on(6144, 4096) == 0 and on(4096, 14336) == 0
    assert on(28672, 8192, True) == 0 and on(128256, 8192) == 0
    assert on(4095, 512, True) == 0 and on(128, 64, True) == 0 and on(128, 64) == 0  # the grid is not full
    assert glue.w12_geometry(8, 16384 + 8, False, PLANAR) is None
    calls = []
    real_call = _abi.call
    monkeypatch.setattr(_abi, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])
    gen = torch.Generator(device=DEV).manual_seed(3)
    for (N, K), pair, layout in (((4096, 512), True, PLANAR), ((8, 4096), True, 0), ((4096, 1024), False, None)):
        W, W3 = T12._normal(N, K, gen), (T12._normal(N, K, gen) if pair else None)
        x = torch.randn(K, generator=gen, device=DEV).to(BF)
        y0 = glue.gemv_fused(W, x, w3=W3)
        calls.clear()
        y1 = glue.gemv_fused(W, x, w3=W3, w12=True)
        packed = layout is not None
        assert ("cc_gemv_fused_w12" in calls) == packed and ("cc_w12_pack" in calls) == packed, ((N, K), calls)
        assert sorted({k[5] for k, (p, _) in glue._w12_cache.items() if p is not None}) == ([layout] if packed else [])
        assert torch.equal(_bits(y0), _bits(y1))
        glue.w12_cache_clear()
