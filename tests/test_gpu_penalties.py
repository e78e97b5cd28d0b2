"""cc_logits_penalize and cc_token_counts_add on the device (include/coldcompress.h) against the torch twin of their contract
(tests/penalty_twin.py), bit for bit with NaNs as a class: every input family over dtype x V x T x row stride, tokens that repeat, sit
at both ends of the vocabulary, fall outside it and straddle gen_start, no tokens, no bias, in place; the counts against
torch.bincount; the full vocabulary; hipGraph replay with the tokens rewritten; and generate(penalties=...) on the tiny model: eager,
graphed and in forced blocks."""
import argparse

import pytest
import torch

import penalty_twin as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
VS = (1, 7, 8, 9, 255, 2049, 4099)
_ID = lambda d: str(d).split(".")[-1]  # noqa: E731
GUARD = 0x5A5A5A5A


def _strided(rows, stride, offset):
    """rows [T, V] on the device as a view of a [T, stride] buffer that starts `offset` elements into an allocation (the gaps hold
    NaN: reading them into a result would show)."""
    T, V = rows.shape
    buf = torch.full((offset + T * stride + 8,), float("nan"), dtype=rows.dtype, device=DEV)
    view = buf[offset:offset + T * stride].view(T, stride)[:, :V]
    view.copy_(rows)
    return view, buf


def _guarded(t, offset, fill):
    """t [V] on the device inside a buffer with `offset` + 4 guard words in front of it and 8 behind."""
    V = t.numel()
    buf = torch.full((4 + offset + V + 8,), fill, dtype=t.dtype, device=DEV)
    view = buf[4 + offset:4 + offset + V]
    view.copy_(t)
    return view, buf


def _guards_intact(buf, view_len, offset, fill):
    b = buf.cpu()
    return bool((b[:4 + offset] == fill).all()) and bool((b[4 + offset + view_len:] == fill).all())


def _one(dtype, V, T, stride, name, setting, with_bias, with_tokens, alias):
    from cold_compress_amd.harness import glue

    r, f, p = setting
    off = 0 if stride == V else 1  # (the padded stride also moves every base off its 16-byte boundary: the element-wise loads)
    rows = P.family(name, dtype, V)[:T]
    pc, gc = P.counts(V)
    toks, pos = P.block_inputs(V, T) if with_tokens else (None, None)
    bias = P.bias_vec(V) if with_bias else None
    want, cp, cg = P.twin(rows, pc, gc, P.GEN_START, toks, pos, r, f, p, bias)
    x, xbuf = _strided(rows, stride, off)
    dpc, pbuf = _guarded(pc, off, GUARD)
    dgc, gbuf = _guarded(gc, off, GUARD)
    dbias = _guarded(bias, off, 0.25)[0] if with_bias else None
    gs = torch.tensor([P.GEN_START], dtype=torch.int32, device=DEV)
    dt = torch.tensor(toks, dtype=torch.int32, device=DEV) if with_tokens else None
    dp = torch.tensor(pos, dtype=torch.int32, device=DEV) if with_tokens else None
    got = glue.logits_penalize(x, dpc, dgc, gs, dt, dp, r, f, p, dbias, out=x if alias else None)
    what = (_ID(dtype), V, T, stride, name, setting, with_bias, with_tokens, alias)
    assert (got is x) == alias and got.shape == (T, V)
    assert P.same_bits(got.cpu(), want), what
    if not alias:
        assert P.same_bits(x.cpu(), rows), what  # the input is left as it was
    # the counts are the exact integers, whole arrays: an element whose count did not change keeps its word
    assert torch.equal(dpc.cpu(), cp) and torch.equal(dgc.cpu(), cg), what
    assert _guards_intact(pbuf, V, off, GUARD) and _guards_intact(gbuf, V, off, GUARD), what
    gaps = xbuf.cpu()
    assert bool(torch.isnan(gaps[:off]).all()) and bool(torch.isnan(gaps[off + T * stride:]).all()), what
    if stride > V:
        assert bool(torch.isnan(gaps[off:off + T * stride].view(T, stride)[:, V:]).all()), what


@pytest.mark.parametrize("dtype", P.DTYPES, ids=_ID)
def test_kernel_is_the_twin(dtype):
    """Every family at every V x T x row stride with all three penalties on: once with tokens and a bias (holding -inf) into a new
    tensor, once without either and in place.  Then each penalty alone at T = 4."""
    for V in VS:
        for stride in (V, V + 3):
            for T in (1, 2, 3, 4):
                for name in P.FAMILIES:
                    _one(dtype, V, T, stride, name, P.ALL_ON, True, True, False)
                    _one(dtype, V, T, stride, name, P.ALL_ON, False, False, True)
            for k, setting in enumerate(P.SETTINGS[:-1]):
                for name in ("normal", "zeros", "inf"):
                    _one(dtype, V, 4, stride, name, setting, False, True, bool(k % 2))


def test_token_counts_add_is_bincount():
    from cold_compress_amd.harness import glue

    V = 1000
    g = torch.Generator().manual_seed(9)
    many = torch.randint(-3, V + 3, (8193,), generator=g, dtype=torch.int32)  # (out-of-range tokens included)
    many[:4] = torch.tensor([-1, V, 0, V - 1], dtype=torch.int32)
    cases = [(many[:0], 0, 5), (many[:1], 7, 5), (many[2:3], 3, 5), (many, 10, 10 + 4000), (torch.full((8193,), 17, dtype=torch.int32), 0, 100)]
    for tokens, first_pos, gen_start in cases:
        pc0, gc0 = P.counts(V, seed=1)
        dpc, pbuf = _guarded(pc0, 0, GUARD)
        dgc, gbuf = _guarded(gc0, 1, GUARD)
        gs = torch.tensor([gen_start], dtype=torch.int32, device=DEV)
        glue.token_counts_add(dpc, dgc, tokens.to(DEV), first_pos, gs)
        t = tokens.long()
        ok = (t >= 0) & (t < V)
        gen = (first_pos + torch.arange(len(t))) >= gen_start
        assert torch.equal(dpc.cpu(), pc0 + torch.bincount(t[ok & ~gen], minlength=V).to(torch.int32)), (len(t), first_pos)
        assert torch.equal(dgc.cpu(), gc0 + torch.bincount(t[ok & gen], minlength=V).to(torch.int32)), (len(t), first_pos)
        assert _guards_intact(pbuf, V, 0, GUARD) and _guards_intact(gbuf, V, 1, GUARD)


def test_full_vocabulary_twice():
    """bf16, V = 128256, T = 4: the twin's bits, and the same bits from a second run on the same inputs."""
    from cold_compress_amd.harness import glue

    V, T, dtype = 128256, 4, torch.bfloat16
    rows = P.family("peaked", dtype, V)
    pc, gc = P.counts(V)
    toks, pos = P.block_inputs(V, T)
    bias = P.bias_vec(V)
    r, f, p = P.ALL_ON
    want, cp, cg = P.twin(rows, pc, gc, P.GEN_START, toks, pos, r, f, p, bias)
    x, dbias = rows.to(DEV), bias.to(DEV)
    gs = torch.tensor([P.GEN_START], dtype=torch.int32, device=DEV)
    dt, dp = torch.tensor(toks, dtype=torch.int32, device=DEV), torch.tensor(pos, dtype=torch.int32, device=DEV)
    outs = []
    for _ in range(2):
        dpc, dgc = pc.to(DEV), gc.to(DEV)
        outs.append(glue.logits_penalize(x, dpc, dgc, gs, dt, dp, r, f, p, dbias).cpu())
        assert torch.equal(dpc.cpu(), cp) and torch.equal(dgc.cpu(), cg)
    assert P.same_bits(outs[0], want) and P.same_bits(outs[1], outs[0])


def test_replay_advances_through_device_memory():
    """One LogitPenalties.apply captured with tokens / pos in static tensors and replayed three times with other contents: rows and
    counts equal three eager calls."""
    from cold_compress_amd.harness import LogitPenalties

    V, T, dtype = 2049, 3, torch.float16
    g = torch.Generator().manual_seed(2)
    prompt = torch.randint(0, V, (50,), generator=g, dtype=torch.int32).to(DEV)
    rows = [(torch.randn(1, T, V, generator=g) * 3).to(dtype).to(DEV) for _ in range(3)]
    toks = [torch.randint(0, V, (T,), generator=g, dtype=torch.int32).to(DEV) for _ in range(3)]
    toks[1][2] = toks[1][0]
    poss = [torch.arange(48 + 3 * k, 51 + 3 * k, dtype=torch.int32).to(DEV) for k in range(3)]  # (the first block straddles gen_start)
    eager = LogitPenalties(V, DEV, 1.3, 0.2, 0.4, {5: -float("inf")})
    eager.reset(prompt, 50)
    want = []
    for k in range(3):
        out = eager.apply(rows[k], toks[k], poss[k])
        want.append((out.cpu(), eager.prompt_count.cpu(), eager.gen_count.cpu()))
    pen = LogitPenalties(V, DEV, 1.3, 0.2, 0.4, {5: -float("inf")})
    pen.reset(prompt, 50)
    x, tk, ps = rows[0].clone(), toks[0].clone(), poss[0].clone()
    snap = pen.snapshot()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = pen.apply(x, tk, ps)
    pen.restore(snap)  # (nothing ran during capture; put back all the same, as GraphedDecoder.capture does)
    for k in range(3):
        x.copy_(rows[k])
        tk.copy_(toks[k])
        ps.copy_(poss[k])
        graph.replay()
        assert P.same_bits(out.cpu(), want[k][0]), k
        assert torch.equal(pen.prompt_count.cpu(), want[k][1]) and torch.equal(pen.gen_count.cpu(), want[k][2]), k
    assert int(want[2][1].sum()) == 52 and int(want[2][2].sum()) == 7


def _tiny(dtype):
    import cold_compress_amd.cache as cache
    from cold_compress_amd.harness import CONFIGS, ModelArgs, Transformer, setup_caches

    torch.manual_seed(3)
    model = Transformer(ModelArgs(**CONFIGS["tiny"])).to(dtype).eval().to(DEV)
    ap = argparse.ArgumentParser()
    cache.add_cache_arguments(ap)
    kw = vars(ap.parse_args([]))
    kw.update(cache_strategy=["recent_global"], prompt_compression_strategy=["recent_global"], max_cache_length=[32], global_tokens=4)
    setup_caches(model, None, DEV, 64, dict(kw))
    return model


def test_generate_with_penalties_eager_graphed_and_blocks():
    """The tiny model at temperature 0.8, top_k 50, with all three penalties and a ban.  Free-running and teacher-forced: the eager
    loop, the captured step (and forced_block = 4 where tokens are forced) give the same sequence and probability rows bit for bit, and
    the counts at the end are the bincount of the inputs — which is what shows that capture() put the state back.  A second
    generation through the same decoder and the same LogitPenalties object does not capture again and matches a fresh eager run.
    logprobs=True with penalties returns the TokenScores the same committed tokens get when scored without penalties."""
    from cold_compress_amd.harness import GraphedDecoder, LogitPenalties, decode_one_token, generate, prefill

    model = _tiny(torch.bfloat16)
    V = model.config.vocab_size
    prompt = torch.randint(0, 128, (20,), generator=torch.Generator().manual_seed(1), dtype=torch.int32).to(DEV)
    forced = torch.randint(0, 128, (13,), generator=torch.Generator().manual_seed(2), dtype=torch.int32).to(DEV)
    sampling = dict(temperature=0.8, top_k=50, seed=1)

    def run(dec, **kw):
        for l in model.layers:
            l.attention.kv_cache.reset()
        seq, second, _ = generate(model, prompt, prefill, dec, max_new_tokens=16, **kw)
        torch.cuda.synchronize()
        return seq.cpu(), second

    def same(a, b):
        return torch.equal(a[0], b[0]) and len(a[1]) == len(b[1]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))

    def counts_ok(pen, seq):
        n = len(prompt)
        return (pen.prompt_count.cpu().tolist() == torch.bincount(seq[:n].long(), minlength=V).tolist()
                and pen.gen_count.cpu().tolist() == torch.bincount(seq[n:-1].long(), minlength=V).tolist())

    plain = run(decode_one_token, **sampling)
    gen = plain[0][len(prompt):]
    ban = int(torch.bincount(gen.long(), minlength=V).argmax())

    def mk():
        return LogitPenalties(V, DEV, 1.3, 0.2, 0.4, {ban: -float("inf")})

    pe = mk()
    eager = run(decode_one_token, penalties=pe, **sampling)
    assert ban not in eager[0][len(prompt):].tolist() and not torch.equal(eager[0], plain[0])
    assert all(float(r[ban]) == 0.0 for r in eager[1]) and counts_ok(pe, eager[0])
    pg = mk()
    dec = GraphedDecoder(model, penalties=pg, **sampling)
    graphed = run(dec, penalties=pg, **sampling)
    assert same(graphed, eager) and counts_ok(pg, graphed[0])
    graph1 = dec.graph
    assert graph1 is not None
    # teacher-forced, through the same decoder and the same object: no new capture; blocks of 4 give the same
    e_forced = run(decode_one_token, penalties=pe, next_tokens=forced, **sampling)
    g_forced = run(dec, penalties=pg, next_tokens=forced, **sampling)
    assert dec.graph is graph1 and same(g_forced, e_forced) and counts_ok(pg, g_forced[0]) and counts_ok(pe, e_forced[0])
    pb = mk()
    b_forced = run(decode_one_token, penalties=pb, next_tokens=forced, forced_block=4, **sampling)
    assert same(b_forced, e_forced) and counts_ok(pb, b_forced[0])
    fresh = run(decode_one_token, penalties=mk(), **sampling)
    again = run(dec, penalties=pg, **sampling)
    assert dec.graph is graph1 and same(again, fresh) and same(again, eager)
    # the scores stay the model's own: the penalised run's committed tokens, forced through a run without penalties
    seq_s, scores = run(decode_one_token, penalties=mk(), logprobs=True, **sampling)
    assert torch.equal(seq_s, eager[0])
    seq_f, own = run(decode_one_token, next_tokens=seq_s[len(prompt):].to(DEV), logprobs=True, **sampling)
    assert torch.equal(seq_f, seq_s)
    assert torch.equal(scores.logprob.view(torch.int32), own.logprob.view(torch.int32)) and torch.equal(scores.rank, own.rank)
    pl = mk()
    dec_l = GraphedDecoder(model, penalties=pl, logprobs=True, **sampling)
    seq_g, scores_g = run(dec_l, penalties=pl, logprobs=True, **sampling)
    assert torch.equal(seq_g, seq_s) and torch.equal(scores_g.logprob.view(torch.int32), scores.logprob.view(torch.int32))
