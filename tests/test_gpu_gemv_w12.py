"""cc_gemv_fused_w12 (the lossless 12-bit packed copy of dense bf16 weights) against cc_gemv_fused itself: y and h_out must be equal
BIT FOR BIT (torch.equal on the int16 views) in every form — plain, norm + delta + h_out, bias + RoPE, the SwiGLU pair — at
  (6, 512)            three idle waves            (10, 4096)   two column steps
  (8, 14336)          seven steps in two issue phases          (5, 1792)    partial last segment, N no multiple of RB
  (2 * RB * cap + 3, 512)   a third, ragged round of the grid           (32768 + 3, 512)   the LM head's launch class (2 rows, 1024 groups)
on N(0, 0.02), on a tensor with zeros and subnormals sprinkled in, on tensors with exactly 7 and exactly 8 escapes in one record
(the last slot, and the reload of the tile from the dense tensor), and on a tensor with an escape in every chunk, which the packer
must refuse while the call still succeeds through the plain kernel.  Also: a numpy decoder of the format (its second statement)
brings a tensor with all 65536 bf16 patterns back bit for bit; no record of N(0, 0.02) at (14336, 4096) overflows; and the tiny
harness model decodes the same tokens and probability rows with CC_W12 on and off, eager and graphed, also after a weight changed
in place."""
import argparse
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
OVERFLOW = -1  # 0xFFFFFFFF in the int32 view of a record's first word


def _bits(t):
    return t.view(torch.int16)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _normal(N, K, gen):
    return (torch.randn(N, K, generator=gen, device=DEV) * 0.02).to(BF)


def _windowed(N, K, gen):
    """N(0, 0.02) with every magnitude moved into eight binades, [2^-12, 2^-4): whichever window of 16 exponents the packer
    chooses holds all of them, so the tensor has no escape but the ones planted afterwards."""
    w = torch.randn(N, K, generator=gen, device=DEV) * 0.02
    return (torch.sign(w) + (w == 0)) .mul(w.abs().clamp(2.0 ** -12, 2.0 ** -4 * 0.99)).to(BF)


def _plant(w, where, patterns):
    v = w.view(torch.int16)
    for (r, c), b in zip(where, patterns):
        v[r, c] = b - 65536 if b >= 32768 else b
    return w


ODD = [0x7F80, 0x8000, 0x7FC1, 0x0001, 0xFF80, 0x807F, 0x4B00, 0x0000]  # inf, -0, a NaN payload, subnormals, -inf, 2^23, +0


def _weights(kind, N, K, geo, gen):
    rb, cu = geo[0], geo[1]
    if kind == "normal":
        return _normal(N, K, gen)
    if kind == "zeros":
        w = _normal(N, K, gen)
        idx = torch.randperm(N * K, generator=torch.Generator().manual_seed(N + K))[: max(3, N * K // 1000)].to(DEV)
        pat = torch.tensor([0x0000, -32768, 0x0001, 0x007F, -32767], dtype=torch.int16, device=DEV)  # ±0 and subnormals
        w.view(torch.int16).view(-1)[idx] = pat[torch.arange(idx.numel(), device=DEV) % 5]
        return w
    if kind in ("esc7", "esc8"):
        # record 0 is wave 0's first tile: chunk (u * 4) * 64 + lane of rows 0 .. RB - 1, u < CU.  Four escapes in lane 0 of element
        # (0, 0), three in lane 2 of the tile's LAST element where there is one, else in lane 1 of (0, 0); the eighth beside the four.
        w = _windowed(N, K, gen)
        where = [(0, 0), (0, 1), (0, 5), (0, 7)]
        r_last = min(rb, N) - 1
        u_last = min(cu, -(-(K // 8) // 256)) - 1
        if (r_last, u_last) != (0, 0):
            c0 = (u_last * 4 * 64 + 2) * 8
            where += [(r_last, c0), (r_last, c0 + 3), (r_last, c0 + 6)]
        else:
            where += [(0, 8), (0, 11), (0, 14)]
        if kind == "esc8":
            where.append((0, 2))
        _plant(w, where, ODD)
        _plant(w, [(N - 1, K - 1), (N - 1, K - 8), (N - 1, K // 2)], [0x7F80, 0x8000, 0x0000])  # another row group's records: edges
        return w
    assert kind == "every_chunk"
    w = _normal(N, K, gen)
    w.view(torch.int16).view(N, K // 8, 8)[:, :, 3] = 0  # +0 in every 16-byte chunk
    return w


def _pack(w, swiglu):
    from cold_compress_amd.harness import glue

    return glue.w12_pack(w, swiglu, refuse=False)


def _call(name, pk, pk3, W, W3, x, form, N, K):
    from cold_compress_amd import _abi

    y = torch.full((N,), 7.0, dtype=BF, device=DEV)
    h = torch.full((K,), 7.0, dtype=BF, device=DEV) if form.get("h_out") else None
    tail = (_p(W), _p(W3), _p(x), _p(form.get("delta")), _p(form.get("norm_weight")), 1e-5, _p(h), _p(form.get("bias")),
            _p(form.get("freqs")), form.get("rope_rows", 0), form.get("head_dim", 0), _p(y), N, K, _abi.CC_DT_BF16, _stream())
    if name == "cc_gemv_fused":
        _abi.call(name, *tail)
    else:
        _abi.call(name, _p(pk.codes), _p(pk.records), pk.base, _p(pk3.codes) if pk3 else None, _p(pk3.records) if pk3 else None,
                  pk3.base if pk3 else 0, pk.rb, pk.cu, *tail)
    return y, h


def _forms(N, K, gen):
    r = lambda *s: torch.randn(*s, generator=gen, device=DEV).to(BF)  # noqa: E731
    norm = dict(delta=r(K), norm_weight=(1 + 0.1 * torch.randn(K, generator=gen, device=DEV)).to(BF), h_out=True)
    return {"plain": {}, "norm": norm, "bias_rope": dict(bias=r(N), freqs=r(2, 2), rope_rows=(N // 4) * 4, head_dim=4),
            "swiglu": dict(norm, swiglu=True)}


def _shapes():
    from cold_compress_amd.harness import glue

    geo = glue.w12_geometry(1 << 13, 512)
    return [(6, 512), (10, 4096), (8, 14336), (5, 1792), (2 * geo[0] * geo[3] + 3, 512), (32768 + 3, 512)]


SHAPES = ["idle_waves", "two_steps", "two_phases", "partial_segment", "ragged_round", "head_class"]


@pytest.mark.parametrize("kind", ["normal", "zeros", "esc7", "esc8"])
@pytest.mark.parametrize("shape", range(6), ids=SHAPES)
def test_w12_equals_dense_bit_for_bit(shape, kind):
    from cold_compress_amd.harness import glue

    N, K = _shapes()[shape]
    gen = torch.Generator(device=DEV).manual_seed(100 * shape + len(kind))
    x = torch.randn(K, generator=gen, device=DEV).to(BF)
    for fname, form in _forms(N, K, gen).items():
        pair = bool(form.get("swiglu"))
        geo = glue.w12_geometry(N, K, pair)
        assert geo is not None
        if shape == 5 and not pair:
            assert geo[:2] == (2, 2) and geo[3] == 1024 and geo[4] == 1, geo  # the LM head's instantiation and grid
        W = _weights(kind, N, K, geo, gen)
        W3 = _weights(kind, N, K, geo, gen) if pair else None
        pk = _pack(W, pair)
        pk3 = _pack(W3, pair) if pair else None
        for p in (pk, pk3):
            if p is None:
                continue
            first = p.records[:, 0]
            if kind == "esc7":
                assert p.n_overflow == 0 and int(first.max()) == 7 and int(first[0]) == 7, (p.n_overflow, first[:8].tolist())
            if kind == "esc8":
                assert p.n_overflow == 1 and int(first[0]) == OVERFLOW, (p.n_overflow, first[:8].tolist())
        y0, h0 = _call("cc_gemv_fused", None, None, W, W3, x, form, N, K)
        y1, h1 = _call("cc_gemv_fused_w12", pk, pk3, W, W3, x, form, N, K)
        assert torch.equal(_bits(y0), _bits(y1)), (fname, int((_bits(y0) != _bits(y1)).sum()))
        if h0 is not None:
            assert torch.equal(_bits(h0), _bits(h1)), fname


@pytest.mark.parametrize("shape", range(5), ids=SHAPES[:5])
def test_w12_refused_tensor_takes_the_plain_kernel(shape, monkeypatch):
    from cold_compress_amd import _abi
    from cold_compress_amd.harness import glue

    monkeypatch.delenv("CC_W12", raising=False)
    N, K = _shapes()[shape]
    gen = torch.Generator(device=DEV).manual_seed(7 + shape)
    x = torch.randn(K, generator=gen, device=DEV).to(BF)
    calls = []
    real_call = _abi.call
    monkeypatch.setattr(_abi, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])
    for fname, form in _forms(N, K, gen).items():
        pair = bool(form.pop("swiglu", False))
        geo = glue.w12_geometry(N, K, pair)
        W = _weights("every_chunk", N, K, geo, gen)
        W3 = _weights("every_chunk", N, K, geo, gen) if pair else None
        assert glue.w12_pack(W, pair) is None  # refused: every record overflows
        kw = {k: v for k, v in form.items() if k != "h_out"}
        h0 = torch.empty(K, dtype=BF, device=DEV) if form.get("h_out") else None
        h1 = torch.empty(K, dtype=BF, device=DEV) if form.get("h_out") else None
        y0 = glue.gemv_fused(W, x, w3=W3, h_out=h0, **kw)
        calls.clear()
        y1 = glue.gemv_fused(W, x, w3=W3, h_out=h1, w12="force", **kw)
        assert "cc_gemv_fused" in calls and "cc_gemv_fused_w12" not in calls, calls
        assert torch.equal(_bits(y0), _bits(y1)), fname
        if h0 is not None:
            assert torch.equal(_bits(h0), _bits(h1)), fname
        # and a tensor the packer accepts does go through the packed kernel, with the same bits
        Wn = _normal(N, K, gen)
        Wn3 = _normal(N, K, gen) if pair else None
        y0 = glue.gemv_fused(Wn, x, w3=Wn3, h_out=h0, **kw)
        calls.clear()
        y1 = glue.gemv_fused(Wn, x, w3=Wn3, h_out=h1, w12="force", **kw)
        assert "cc_gemv_fused_w12" in calls and "cc_gemv_fused" not in calls, calls
        assert torch.equal(_bits(y0), _bits(y1)), fname
    glue.w12_cache_clear()


def test_w12_is_on_by_default_only_where_it_measured_faster(monkeypatch):
    """cc_w12_geometry's fifth word: the SwiGLU pair and plain matrices of 32768 rows or more, at K <= 4096 (the launch classes
    that measured faster on MI355X: DESIGN §2.17).  gemv_fused(w12=True) keeps every other weight on the dense kernel and packs
    nothing for it; w12="force" is the explicit way in."""
    from cold_compress_amd import _abi
    from cold_compress_amd.harness import glue

    monkeypatch.delenv("CC_W12", raising=False)
    on = lambda N, K, pair=False: glue.w12_geometry(N, K, pair)[4]  # noqa: E731
    assert on(14336, 4096, True) == 1 and on(128256, 4096) == 1 and on(128, 64, True) == 1
    assert on(4096, 4096) == 0 and on(6144, 4096) == 0 and on(4096, 14336) == 0 and on(128, 64) == 0
    assert on(28672, 8192, True) == 0 and on(128256, 8192) == 0  # the 70B shapes: four steps per wave, not measured faster
    assert glue.w12_geometry(8, 16384 + 8) is None
    calls = []
    real_call = _abi.call
    monkeypatch.setattr(_abi, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])
    gen = torch.Generator(device=DEV).manual_seed(3)
    for (N, K), pair, packed in (((64, 4096), False, False), ((8, 8192), True, False), ((8, 4096), True, True)):
        W, W3 = _normal(N, K, gen), (_normal(N, K, gen) if pair else None)
        x = torch.randn(K, generator=gen, device=DEV).to(BF)
        y0 = glue.gemv_fused(W, x, w3=W3)
        calls.clear()
        y1 = glue.gemv_fused(W, x, w3=W3, w12=True)
        assert ("cc_gemv_fused_w12" in calls) == packed and ("cc_w12_pack" in calls) == packed, ((N, K), calls)
        assert torch.equal(_bits(y0), _bits(y1))
    glue.w12_cache_clear()


def w12_decode_numpy(codes, records, base, rb, cu, N, K):
    """The format, once more: codes uint32 [N, K / 8, 3], records uint32 [records, 8] -> the bf16 bit patterns uint16 [N, K].
    An overflowing record is reported, not decoded (its tile is read from the dense tensor)."""
    nch = K // 8
    codes = codes.reshape(N, nch, 3).astype(np.uint32)
    sm = np.stack([(codes[:, :, k >> 2] >> (8 * (k & 3))) & 0xFF for k in range(8)], axis=-1)
    idx = np.stack([(codes[:, :, 2] >> ((k & 1) * 16 + (k >> 1) * 4)) & 0xF for k in range(8)], axis=-1)
    bits = (((sm & 0x80) << 8) | (sm & 0x7F) | ((base + idx) << 7)).astype(np.uint16).reshape(N, K)
    nstep = -(-(-(-nch // 64)) // 4)
    nph = -(-nstep // cu)
    overflow = 0
    for rid in np.nonzero(records[:, 0])[0]:
        cnt = int(records[rid, 0])
        if cnt == 0xFFFFFFFF:
            overflow += 1
            continue
        assert 1 <= cnt <= 7
        wave, ph, rg = rid % 4, (rid // 4) % nph, rid // (4 * nph)
        for en in records[rid, 1:1 + cnt]:
            en = int(en)
            t, lane, k = en >> 25, (en >> 19) & 63, (en >> 16) & 7
            row, c = rg * rb + t // cu, ((ph * cu + t % cu) * 4 + wave) * 64 + lane
            bits[row, c * 8 + k] = en & 0xFFFF
    return bits, overflow


def test_w12_round_trip_of_all_65536_patterns():
    """Row i carries pattern i at column (37 i) mod K among in-window fillers: every record holds at most RB <= 4 escapes."""
    N, K = 65536, 256
    w = torch.full((N, K), 0.0234375, dtype=BF, device=DEV)
    rows = torch.arange(N, device=DEV)
    w.view(torch.int16)[rows, (rows * 37) % K] = (rows - 65536 * (rows >= 32768)).to(torch.int16)
    pk = _pack(w, False)
    assert pk.n_overflow == 0 and pk.n_escapes == 65536 - 16 * 256, (pk.n_overflow, pk.n_escapes)
    back, overflow = w12_decode_numpy(pk.codes.cpu().numpy().view(np.uint32), pk.records.cpu().numpy().view(np.uint32), pk.base, pk.rb,
                                      pk.cu, N, K)
    assert overflow == 0
    assert np.array_equal(back, w.view(torch.int16).cpu().numpy().view(np.uint16))


def test_w12_no_overflow_on_normal_weights_at_the_ffn_shape():
    w = (torch.randn(14336, 4096, generator=torch.Generator(device=DEV).manual_seed(1234), device=DEV) * 0.02).to(BF)
    pk = _pack(w, True)
    assert pk.n_overflow == 0, (pk.n_overflow, pk.n_records, pk.n_escapes)
    assert 100 <= pk.base <= 116 and 0 < pk.n_escapes < 3e-4 * w.numel(), (pk.base, pk.n_escapes)


def test_w12_tiny_model_decodes_the_same_with_and_without(monkeypatch):
    """8 greedy tokens of the tiny harness model, eager and graphed: CC_W12 on and off give identical tokens and probability rows;
    after a weight changed in place both still agree, on other values than before (the packed copy was rebuilt; the same graphed
    decoder is reused, so it has to notice).  With CC_W12 on, the w1/w3 pair of every layer goes through the packed kernel; the tiny
    model's 128-row LM head, like wo, w2 and wqkv, is no launch class that measured faster and stays dense."""
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
    real_call = _abi.call
    monkeypatch.setattr(_abi, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])
    decs = {}

    def run(w12, graphed):
        monkeypatch.setenv("CC_W12", "1" if w12 else "0")
        calls.clear()
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
                    n12 = calls.count("cc_gemv_fused_w12")
                    assert n12 == (T * cfg["n_layer"] if w12 else 0), n12
        ref = out[(False, False)]
        for k, (toks, probs) in out.items():
            assert toks == ref[0], k
            assert torch.equal(probs.view(torch.int32) if probs.dtype == torch.float32 else _bits(probs),
                               ref[1].view(torch.int32) if ref[1].dtype == torch.float32 else _bits(ref[1])), k
        return ref

    before = all_four()
    with torch.no_grad():
        model.layers[1].feed_forward.w3.weight.mul_(-1.0)  # in place: the version counter moves
        model.layers[0].feed_forward.w1.weight.mul_(0.5)
    after = all_four()
    assert not torch.equal(before[1], after[1])
    glue.w12_cache_clear()
