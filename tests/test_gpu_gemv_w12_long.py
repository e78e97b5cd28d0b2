"""cc_gemv_fused_w12 under layout id 2 — planar codes behind the pipelined long-row launch, plain matrices with 3 .. 8 column steps per
wave (4096 < K <= 16384) — against cc_gemv_fused itself: y and h_out equal BIT FOR BIT in the plain, norm (delta, h_out) and
bias + RoPE forms, on the four weight kinds of test_gpu_gemv_w12.py (whose builders this file imports and leaves alone), at
  (9, 4104)     three steps, the smallest long row, N no multiple of RB      (8, 14336)    seven steps, the last tile half exists
  (5, 12296)    seven steps, one chunk in the last segment                   (6, 16384)    eight steps, every tile full
  (7, 10248)    21 segments: six steps, the sixth in wave 0 alone            (7, 9224)     five steps, (4, 8192) four
  (2 * RB * cap + 3, 4104)   several row groups per workgroup: the request carried across the end of a row group, and a last,
                             partial row group
Also: ±0, a subnormal, ±inf and a NaN payload planted at chunk positions 3, 4 and 7 of lanes 0 and 63 come back through the numpy
decoder of tests/w12_planar.py with layout 2's (RB, CU); the contract of the id (ids 0 and 1 answer as before, id 2 refuses
K <= 4096 and the pair form before anything is launched, a copy packed under one of ids 1 and 2 is refused under the other, the
default word); and a harness model whose w2 is 64 x 4104, forced through id 2, decodes the tokens and probability rows of CC_W12=0,
eager and graphed, also after a w2 weight changed in place."""
import argparse

import numpy as np
import pytest
import torch

import test_gpu_gemv_w12 as T12
import test_gpu_gemv_w12_planar as TP
import w12_planar as WP

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
PLANAR, LONG = 1, 2
UNSUPPORTED = -2  # CC_ERR_UNSUPPORTED (include/coldcompress.h)
_bits, _p, _stream = T12._bits, T12._p, T12._stream
FORMS = ("plain", "norm", "bias_rope")


def _geo(N, K, pair=False, layout=LONG):
    from cold_compress_amd.harness import glue

    return glue.w12_geometry(N, K, pair, layout)


def _shapes():
    rb, _, _, cap, _ = _geo(4096, 4104)
    return [(9, 4104), (8, 14336), (5, 12296), (6, 16384), (7, 10248), (7, 9224), (4, 8192), (2 * rb * cap + 3, 4104)]


SHAPES = ["three_steps", "seven_steps_half_tile", "one_chunk_last_segment", "eight_steps", "six_steps_one_wave", "five_steps", "four_steps",
          "row_groups_per_workgroup"]
STEPS = [3, 7, 7, 8, 6, 5, 4, 3]


@pytest.mark.parametrize("kind", ["normal", "zeros", "esc7", "esc8"])
@pytest.mark.parametrize("shape", range(8), ids=SHAPES)
def test_long_equals_dense_bit_for_bit(shape, kind):
    N, K = _shapes()[shape]
    assert -(-(-(-K // 512)) // 4) == STEPS[shape]
    gen = torch.Generator(device=DEV).manual_seed(100 * shape + len(kind))
    x = torch.randn(K, generator=gen, device=DEV).to(BF)
    geo = _geo(N, K)
    assert geo is not None
    W = T12._weights(kind, N, K, geo, gen)
    pk = TP._pack(W, False, layout=LONG)
    assert pk.layout == LONG and pk.base % 2 == 0 and (pk.rb, pk.cu) == geo[:2]
    first = pk.records[:, 0]
    if kind == "esc7":
        assert pk.n_overflow == 0 and int(first.max()) == 7 and int(first[0]) == 7, (pk.n_overflow, first[:8].tolist())
    if kind == "esc8":
        assert pk.n_overflow == 1 and int(first[0]) == T12.OVERFLOW, (pk.n_overflow, first[:8].tolist())
    forms = T12._forms(N, K, gen)
    for fname in FORMS:
        form = forms[fname]
        y0, h0 = T12._call("cc_gemv_fused", None, None, W, None, x, form, N, K)
        y1, h1 = TP._call12(pk, None, W, None, x, form, N, K)
        assert torch.equal(_bits(y0), _bits(y1)), (fname, int((_bits(y0) != _bits(y1)).sum()))
        if h0 is not None:
            assert torch.equal(_bits(h0), _bits(h1)), fname


def test_long_round_trip_of_planted_patterns_at_the_neighbour_sign_positions():
    """±0, a subnormal, ±inf and a NaN payload at chunk positions 3, 4 and 7 of lanes 0 and 63 (chunks 0 and 63 of a row: wave 0's
    first tile), pattern p in row 4 p: six escapes in each of six records, none overflowing; decoded by tests/w12_planar.py with
    layout 2's (RB, CU), and the launch agrees with the dense kernel."""
    N, K = 24, 4104
    pats = [0x0000, 0x8000, 0x0001, 0x7F80, 0xFF80, 0x7FC1]
    where = [(4 * p, chunk * 8 + pos) for p in range(6) for chunk in (0, 63) for pos in (3, 4, 7)]
    gen = torch.Generator(device=DEV).manual_seed(9)
    w = T12._plant(T12._windowed(N, K, gen), where, [pats[r // 4] for r, _ in where])
    pk = TP._pack(w, False, layout=LONG)
    assert (pk.rb, pk.cu) == _geo(N, K)[:2]
    assert pk.n_escapes == 36 and pk.n_overflow == 0 and int(pk.records[:, 0].max()) == 6, (pk.n_escapes, pk.n_overflow)
    back, overflow = WP.decode_tensor(pk.codes.cpu().numpy().view(np.uint32), pk.records.cpu().numpy().view(np.uint32), pk.base, pk.rb,
                                      pk.cu, N, K)
    assert overflow == 0 and np.array_equal(back, w.view(torch.int16).cpu().numpy().view(np.uint16))
    x = torch.randn(K, generator=gen, device=DEV).to(BF)
    y0, _ = T12._call("cc_gemv_fused", None, None, w, None, x, {}, N, K)
    y1, _ = TP._call12(pk, None, w, None, x, {}, N, K)
    assert torch.equal(_bits(y0), _bits(y1))


def test_long_ids_0_and_1_answer_as_before():
    for layout in (0, PLANAR):
        assert _geo(4096, 14336, False, layout) == (4, 4, 8, 512, 0)
        assert _geo(9, 4104, False, layout) == (4, 4, 8, 512, 0)
        assert _geo(4096, 4096, False, layout) == (4, 2, 2, 1024, 0)
        assert _geo(14336, 4096, True, layout) == (2, 2, 2, 2048, 1)
        assert _geo(9, 4104, True, layout) == (2, 4, 8, 2048, 0)


def test_long_id_refuses_short_rows_and_the_pair_before_any_launch():
    from cold_compress_amd import _abi

    lib = _abi.lib()
    out = (T12.C.c_int32 * 5)()
    for N, K, pair in ((4096, 4096, False), (10, 4096, False), (64, 512, False), (9, 4104, True), (14336, 8192, True), (8, 16392, False)):
        assert lib["cc_w12_geometry"](N, K, int(pair) | LONG << 8, out) == UNSUPPORTED, (N, K, pair)
    assert lib["cc_w12_geometry"](9, 4104, LONG << 8, out) == _abi.CC_OK
    rb, cu = out[0], out[1]
    gen = torch.Generator(device=DEV).manual_seed(2)
    for N, K, pair in ((10, 4096, False), (9, 4104, True)):
        W = T12._normal(N, K, gen)
        x = torch.randn(K, generator=gen, device=DEV).to(BF)
        codes = torch.zeros((N, K // 8 * 3), dtype=torch.int32, device=DEV)  # (never packed: the library knows no layout for them)
        records = torch.zeros((-(-N // rb) * 4 * 4, 8), dtype=torch.int32, device=DEV)
        meta = torch.zeros((int(lib["cc_w12_meta_words"]()),), dtype=torch.int32, device=DEV)
        if not pair:
            assert lib["cc_w12_pack"](_p(W), N, K, rb | LONG << 8, cu, _p(codes), _p(records), _p(meta), _stream()) == UNSUPPORTED
            torch.cuda.synchronize()
            assert not bool(codes.any()) and not bool(records.any())
        y = torch.full((N,), 7.0, dtype=BF, device=DEV)
        rc = lib["cc_gemv_fused_w12"](_p(codes), _p(records), 108, _p(codes) if pair else None, _p(records) if pair else None, 108,
                                      rb | LONG << 8, cu, _p(W), _p(W) if pair else None, _p(x), None, None, 1e-5, None, None, None, 0, 0,
                                      _p(y), N, K, _abi.CC_DT_BF16, _stream())
        torch.cuda.synchronize()
        assert rc == UNSUPPORTED and bool((y == 7.0).all()), (N, K, pair, rc)


def test_long_copy_under_the_planar_id_is_refused_and_the_other_way_round():
    from cold_compress_amd import _abi
    from cold_compress_amd.harness import glue

    N, K = 9, 4104
    gen = torch.Generator(device=DEV).manual_seed(4)
    W = T12._normal(N, K, gen)
    x = torch.randn(K, generator=gen, device=DEV).to(BF)
    y0, _ = T12._call("cc_gemv_fused", None, None, W, None, x, {}, N, K)
    for layout, other in ((PLANAR, LONG), (LONG, PLANAR)):
        pk = TP._pack(W, False, layout=layout)
        assert pk.layout == layout
        for rb, cu in ((pk.rb, pk.cu), _geo(N, K, False, other)[:2]):  # under the other id, with either geometry
            y = torch.full((N,), 7.0, dtype=BF, device=DEV)
            rc = _abi.lib()["cc_gemv_fused_w12"](_p(pk.codes), _p(pk.records), pk.base, None, None, 0, rb | other << 8, cu, _p(W), None, _p(x),
                                                 None, None, 1e-5, None, None, None, 0, 0, _p(y), N, K, _abi.CC_DT_BF16, _stream())
            torch.cuda.synchronize()
            assert rc != _abi.CC_OK and bool((y == 7.0).all())
        y, _ = TP._call12(pk, None, W, None, x, {}, N, K)  # under its own id it runs
        assert torch.equal(_bits(y), _bits(y0))
    glue.w12_cache_clear()


def test_long_default_word_is_what_was_measured(monkeypatch):
    """DESIGN §2.17's table for layout 2: LONG_ON lists the measured classes (column steps per wave) that beat both the dense kernel
    and the planar 4 x 4 x 8 launch by more than the dense kernel's spread; each is on only with a full grid, N >= RB x workgroups."""
    from cold_compress_amd import _abi
    from cold_compress_amd.harness import glue

    monkeypatch.delenv("CC_W12", raising=False)
    LONG_ON = {7: True, 4: True}  # w2 (4096 x 14336); the K = 8192 shapes (128256 x 8192, 8192 x 8192)
    rb, _, _, cap, _ = _geo(4096, 14336)
    assert _geo(4096, 14336)[4] == int(LONG_ON[7]) and _geo(8192, 8192)[4] == int(LONG_ON[4]) and _geo(128256, 8192)[4] == int(LONG_ON[4])
    assert _geo(rb * cap - 1, 14336)[4] == 0 and _geo(64, 14336)[4] == 0 and _geo(9, 4104)[4] == 0  # the grid is not full
    assert _geo(rb * cap, 14336)[4] == int(LONG_ON[7])
    calls = []
    real_call = _abi.call
    monkeypatch.setattr(_abi, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])
    gen = torch.Generator(device=DEV).manual_seed(3)
    N, K = rb * cap, 14336
    W = T12._normal(N, K, gen)
    x = torch.randn(K, generator=gen, device=DEV).to(BF)
    y0 = glue.gemv_fused(W, x)
    calls.clear()
    y1 = glue.gemv_fused(W, x, w12=True)
    assert ("cc_gemv_fused_w12" in calls) == LONG_ON[7] and ("cc_w12_pack" in calls) == LONG_ON[7], calls
    assert sorted({k[5] for k, (p, _) in glue._w12_cache.items() if p is not None}) == ([LONG] if LONG_ON[7] else [])
    assert torch.equal(_bits(y0), _bits(y1))
    glue.w12_cache_clear()


def test_long_harness_model_decodes_the_same_with_w2_forced_through_id_2(monkeypatch):
    """dim 64, intermediate size 4104 (w2 is 64 x 4104: three steps), 2 layers, the tiny vocabulary: 8 greedy tokens, eager and
    graphed, with w2 forced through layout id 2, give the tokens and probability rows of CC_W12=0 bit for bit; the eager run
    launches cc_gemv_fused_w12 for w2 in every layer and token; after an in-place change of a w2 weight both still agree, on
    other values (the same graphed decoder is reused, so it has to notice)."""
    import cold_compress_amd.cache as cache
    from cold_compress_amd import _abi
    from cold_compress_amd.harness import CONFIGS, GraphedDecoder, ModelArgs, Transformer, decode_one_token, glue, prefill, setup_caches

    torch.manual_seed(11)
    cfg = dict(CONFIGS["tiny"], intermediate_size=4104)
    model = Transformer(ModelArgs(**cfg)).to(BF).eval().to(DEV)
    ap = argparse.ArgumentParser()
    cache.add_cache_arguments(ap)
    kw = vars(ap.parse_args([]))
    kw.update(dict(cache_strategy=["full"], prompt_compression_strategy=["full"], max_cache_length=[1.0]))
    P, T = 20, 8
    setup_caches(model, None, DEV, P + T + 8, dict(kw))
    prompt = torch.randint(0, cfg["vocab_size"], (P,), generator=torch.Generator().manual_seed(1), dtype=torch.int32).to(DEV)
    w2_calls = []
    real_call, real_gemv = _abi.call, glue.gemv_fused

    def call(name, *a):
        if name == "cc_gemv_fused_w12" and (a[-4], a[-3]) == (64, 4104):
            w2_calls.append(a[6] >> 8)  # the layout id in the rb word
        return real_call(name, *a)

    def gemv(weight, *a, **k):
        if tuple(weight.shape) == (64, 4104) and k.get("w12"):
            k = {**k, "w12": "force-long"}
        return real_gemv(weight, *a, **k)

    monkeypatch.setattr(_abi, "call", call)
    monkeypatch.setattr(glue, "gemv_fused", gemv)
    decs = {}

    def run(w12, graphed):
        monkeypatch.setenv("CC_W12", "1" if w12 else "0")
        w2_calls.clear()
        model.reset_caches()
        dec = decs.setdefault(w12, GraphedDecoder(model)) if graphed else None
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

    def all_four():
        out = {}
        for graphed in (False, True):
            for w12 in (False, True):
                out[(w12, graphed)] = run(w12, graphed)
                if not graphed:
                    assert w2_calls == ([LONG] * (T * cfg["n_layer"]) if w12 else []), w2_calls
        ref = out[(False, False)]
        for k, (toks, probs) in out.items():
            assert toks == ref[0], k
            assert torch.equal(probs.view(torch.int32) if probs.dtype == torch.float32 else _bits(probs),
                               ref[1].view(torch.int32) if ref[1].dtype == torch.float32 else _bits(ref[1])), k
        return ref

    before = all_four()
    with torch.no_grad():
        model.layers[1].feed_forward.w2.weight.mul_(-1.0)  # in place: the version counter moves
        model.layers[0].feed_forward.w2.weight.mul_(0.5)
    after = all_four()
    assert not torch.equal(before[1], after[1])
    glue.w12_cache_clear()
