"""cc_logits_constrain and cc_token_history_write on the device (include/coldcompress.h) against the plain-Python twin of their
contract (tests/constraint_twin.py), bit for bit with NaNs as a class and every untouched element's bits kept: every input family
over dtype x V x T x row stride, histories with many matches and with none, single matches planted at the edges of the ban pass's
workgroup slices, ids outside the vocabulary, each rule alone, in place and out of place, positions at and past the end of the
history; the full vocabulary; hipGraph replay with the tokens rewritten; and generate(constraints=...) on the tiny model: eager,
graphed and in forced blocks."""
import argparse

import pytest
import torch

import constraint_twin as CT
import penalty_twin as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
VS = (1, 7, 8, 9, 255, 2049, 4099)
_ID = lambda d: str(d).split(".")[-1]  # noqa: E731
GUARD = 0x5A5A5A5A
NINF = -float("inf")
RULES = dict(n=3, scope="all", m=40, terminators=[1, 5, -0x7FFFFFFF, 0x7FFFFFFF], bad_words=[[2], [1, 6], [0, 1, 2], [2, 0, 1, 3], [1, 2, 0, 1, 2]])
EACH = (dict(n=1), dict(n=2), dict(n=3, scope="generated"), dict(n=32), dict(m=40, terminators=[0, 4]),
        dict(bad_words=[[1, 2], [0, 0, 0], [6], [2, 1, 0, 2, 1, 0, 2, 1]]), RULES)


def _strided(rows, stride, offset):
    """rows [T, V] on the device as a view of a [T, stride] buffer that starts `offset` elements into an allocation (the gaps hold
    NaN: reading them into a result would show)."""
    T, V = rows.shape
    buf = torch.full((offset + T * stride + 8,), float("nan"), dtype=rows.dtype, device=DEV)
    view = buf[offset:offset + T * stride].view(T, stride)[:, :V]
    view.copy_(rows)
    return view, buf


def _guarded(values, fill=GUARD):
    """int32 values on the device inside a buffer with 4 guard words in front of them and 8 behind."""
    t = torch.tensor(values, dtype=torch.int32)
    buf = torch.full((4 + t.numel() + 8,), fill, dtype=torch.int32, device=DEV)
    view = buf[4:4 + t.numel()]
    view.copy_(t)
    return view, buf


def _guards_intact(buf, n, fill=GUARD):
    b = buf.cpu()
    return bool((b[:4] == fill).all()) and bool((b[4 + n:] == fill).all())


def _dev_rules(n=0, scope="all", m=0, terminators=(), bad_words=()):
    """the rules as cc_logits_constrain's arguments (device tensors)."""
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)  # noqa: E731
    offs = [0]
    for w in bad_words:
        offs.append(offs[-1] + len(w))
    return dict(ngram=n, ngram_from_gen=scope == "generated", min_new_tokens=m, term_ids=i32(list(terminators)) if terminators else None,
                bw_tokens=i32([v for w in bad_words for v in w]) if bad_words else None, bw_offsets=i32(offs) if bad_words else None)


def _one(dtype, V, T, stride, name, rules, hist, pos0, gen_start, tokens, alias):
    """One launch against the twin: rows, the input left alone, the whole history, the guards and the gaps."""
    from cold_compress_amd.harness import glue

    off = 0 if stride == V else 1  # (the padded stride also moves every base off its 16-byte boundary: the element-wise copies)
    rows = P.family(name, dtype, V)[:T]
    want, hist1 = CT.twin(rows, hist, tokens, pos0, gen_start, **rules)
    x, xbuf = _strided(rows, stride, off)
    dh, hbuf = _guarded(hist)
    gs = torch.tensor([gen_start], dtype=torch.int32, device=DEV)
    dt = torch.tensor(tokens, dtype=torch.int32, device=DEV) if tokens is not None else None
    dp = torch.tensor([pos0 + t for t in range(T)], dtype=torch.int32, device=DEV)
    got = glue.logits_constrain(x, dh, gs, dt, dp, out=x if alias else None, **_dev_rules(**rules))
    what = (_ID(dtype), V, T, stride, name, rules, len(hist), pos0, gen_start, tokens, alias)
    assert (got is x) == alias and got.shape == (T, V)
    assert P.same_bits(got.cpu(), want), what
    if not alias:
        assert P.same_bits(x.cpu(), rows), what  # the input is left as it was
    assert dh.cpu().tolist() == hist1 and _guards_intact(hbuf, len(hist)), what  # exactly hist[pos0 .. pos0+T-1] was written
    gaps = xbuf.cpu()
    assert bool(torch.isnan(gaps[:off]).all()) and bool(torch.isnan(gaps[off + T * stride:]).all()), what
    if stride > V:
        assert bool(torch.isnan(gaps[off:off + T * stride].view(T, stride)[:, V:]).all()), what
    return got


def _history(L, alphabet, seed):
    g = torch.Generator().manual_seed(seed)
    return [alphabet[i] for i in torch.randint(0, len(alphabet), (L,), generator=g).tolist()]


@pytest.mark.parametrize("dtype", P.DTYPES, ids=_ID)
def test_kernel_is_the_twin(dtype):
    """Every family at every V x T x row stride with all rules on: a history over an alphabet of 3 (many matches) into a new tensor,
    and one over three ids of which two lie outside the vocabulary, in place.  Then each rule alone at T = 4, and the prefill's row
    (no tokens)."""
    for V in VS:
        for stride in (V, V + 3):
            for T in (1, 2, 3, 4):
                a = _history(41 + T, (0, 1, 2), V + T)
                b = _history(41 + T, (-1, V + 5, 2), V + T + 1)
                for name in P.FAMILIES:
                    _one(dtype, V, T, stride, name, RULES, a[:37] + [GUARD] * 11, 37, 30, a[37:37 + T], False)
                    _one(dtype, V, T, stride, name, RULES, b[:37] + [GUARD] * 11, 37, 30, b[37:37 + T], True)
            a = _history(45, (0, 1, 2), V)
            for k, rules in enumerate(EACH[:-1]):
                for name in ("normal", "inf", "nan"):
                    _one(dtype, V, 4, stride, name, rules, a[:37] + [GUARD] * 11, 37, 30, a[37:41], bool(k % 2))
            _one(dtype, V, 1, stride, "normal", RULES, a[:37] + [GUARD] * 11, 36, 30, None, False)
            _one(dtype, V, 1, stride, "nan", RULES, a[:37] + [GUARD] * 11, 36, 30, None, True)


def test_history_lengths_and_slice_edges():
    """n in (1, 2, 3, 32) x history lengths 0, 1, n - 2, n - 1, n and the lengths at which the number of candidate starts is one below
    / at / above CC_CONSTRAIN_SLICE and twice it: over an alphabet of 3, and over DISTINCT tokens (no match) with single matches
    planted at the first and last candidate of the first slice, the first of the second and the very last one — each bans its own
    marker, so a candidate that is skipped or read twice over a slice edge shows."""
    from cold_compress_amd.harness import glue

    V, dtype, S = 4099, torch.bfloat16, CT.SLICE
    assert S == glue.CONSTRAIN_SLICE
    for n in (1, 2, 3, 32):
        edges = [S + n - 2 + d for d in (-1, 0, 1)] + [2 * S + n - 2 + d for d in (-1, 0, 1)]  # (row 0 has pos0 - n + 2 candidates)
        for L in sorted({0, 1, max(n - 2, 0), max(n - 1, 0), n, *edges}):
            for T in (1, 4):
                for scope, gs in (("all", 0), ("generated", 5)):
                    h = _history(L + T, (0, 1, 2), 31 * L + n)
                    _one(dtype, V, T, V, "normal", dict(n=n, scope=scope), h[:L] + [GUARD] * (T + 3), L, gs, h[L:], False)
        planted = 0
        for L in edges:  # distinct tokens: hist[j] = j + 1, the block's inputs 4000 ..; ONE match is planted for row 0
            for gs, scope in ((0, "all"), (5, "generated")):
                tokens = [4000, 4001, 4002, 4003]
                last = L - n + 1  # row 0's last candidate start; the last one whose n-gram stays clear of the tail is n further in front
                for c in (gs, gs + S - 1, gs + S, last - n):
                    if not (gs <= c and c + n - 1 < L - n + 1):
                        continue
                    hist = list(range(1, L + 1))
                    hist[c:c + n - 1] = (hist + tokens[:1])[L + 1 - (n - 1):] if n > 1 else []
                    hist[c + n - 1] = 3000
                    rules = dict(n=n, scope=scope)
                    ban = CT.banned(hist + tokens[:1], gs, **rules)
                    assert 3000 in ban and (n == 1 or ban == {3000})
                    got = _one(dtype, V, 1, V, "normal", rules, hist + [GUARD] * 4, L, gs, tokens[:1], True)
                    assert float(got[0, 3000]) == NINF and int((got[0].float() == NINF).sum()) == len(ban)
                    _one(dtype, V, 4, V, "nan", rules, hist + [GUARD] * 4, L, gs, tokens, False)
                    planted += 1
        assert planted >= 16, (n, planted)


def test_positions_at_and_past_the_end():
    """Rows at positions outside [0, cap) are copied and store nothing: a block that crosses the end, one that starts at it, one far
    past it, and one that starts in front of position 0."""
    for dtype in P.DTYPES:
        for V in (9, 255):
            h = _history(40, (0, 1, 2), V)
            for pos0 in (38, 39, 40, 47, -2, -4, -9):
                for alias in (False, True):
                    got = _one(dtype, V, 4, V + 3, "normal", RULES, list(h), pos0, 30, [0, 1, 2, 0], alias)
                    rows = P.family("normal", dtype, V)
                    for t in range(4):
                        if not 0 <= pos0 + t < 40:
                            assert P.same_bits(got[t].cpu(), rows[t])


def test_token_history_write_is_a_slice_assignment():
    from cold_compress_amd.harness import glue

    g = torch.Generator().manual_seed(9)
    many = torch.randint(-3, 200000, (8193,), generator=g, dtype=torch.int32)
    for cap, n, first_pos in ((16, 0, 3), (16, 1, 0), (16, 1, 15), (16, 1, 16), (9000, 8193, 0), (9000, 8193, 807), (9000, 8193, 900),
                              (9000, 8193, -5), (100, 8193, -8100)):
        want = [GUARD - 1] * cap
        for i in range(n):
            if 0 <= first_pos + i < cap:
                want[first_pos + i] = int(many[i])
        dh, hbuf = _guarded([GUARD - 1] * cap)
        glue.token_history_write(dh, many[:n].to(DEV), first_pos)
        assert dh.cpu().tolist() == want and _guards_intact(hbuf, cap), (cap, n, first_pos)


def test_full_vocabulary_twice():
    """bf16, V = 128256, T = 4, a history of 8192 over an alphabet of 50, n = 3: the twin's bits, and the same bits from a second run
    on the same inputs."""
    from cold_compress_amd.harness import glue

    V, T, L, dtype = 128256, 4, 8192, torch.bfloat16
    rows = P.family("peaked", dtype, V)
    h = _history(L + T, tuple(range(0, 50 * 2565, 2565)), 11)
    hist, tokens = h[:L] + [0] * 8, h[L:]
    rules = dict(n=3)
    want, hist1 = CT.twin(rows, hist, tokens, L, 100, **rules)
    assert all(int((want[t].float() == NINF).sum()) > 0 for t in range(T))  # (about 8192 / 2500 matches per row)
    x = rows.to(DEV)
    gs = torch.tensor([100], dtype=torch.int32, device=DEV)
    dt, dp = torch.tensor(tokens, dtype=torch.int32, device=DEV), torch.tensor([L], dtype=torch.int32, device=DEV)
    outs = []
    for _ in range(2):
        dh = torch.tensor(hist, dtype=torch.int32, device=DEV)
        outs.append(glue.logits_constrain(x, dh, gs, dt, dp, **_dev_rules(**rules)).cpu())
        assert dh.cpu().tolist() == hist1
    assert P.same_bits(outs[0], want) and P.same_bits(outs[1], outs[0]) and P.same_bits(x.cpu(), rows)


def _make(V, cap, n=0, scope="all", m=0, terminators=(), bad_words=()):
    from cold_compress_amd.harness import LogitConstraints

    return LogitConstraints(V, DEV, cap, no_repeat_ngram_size=n, ngram_scope=scope, min_new_tokens=m, terminator_ids=list(terminators) or None,
                            bad_words_ids=list(bad_words) or None)


def test_replay_advances_through_device_memory():
    """One LogitConstraints.apply captured with tokens / pos in static tensors and replayed three times with other contents: rows and
    history equal three eager calls (the first block straddles gen_start)."""
    V, T, dtype = 2049, 3, torch.float16
    g = torch.Generator().manual_seed(2)
    prompt = torch.randint(0, 3, (50,), generator=g, dtype=torch.int32).to(DEV)
    rows = [(torch.randn(1, T, V, generator=g) * 3).to(dtype).to(DEV) for _ in range(3)]
    toks = [torch.randint(0, 3, (T,), generator=g, dtype=torch.int32).to(DEV) for _ in range(3)]
    poss = [torch.arange(48 + 3 * k, 51 + 3 * k, dtype=torch.int32).to(DEV) for k in range(3)]
    rules = dict(n=3, scope="generated", m=55, terminators=[7, 8], bad_words=[[1, 2], [0]])
    eager = _make(V, 64, **rules)
    eager.reset(prompt, 50)
    want = []
    for k in range(3):
        out = eager.apply(rows[k], toks[k], poss[k])
        want.append((out.cpu(), eager.hist.cpu()))
    con = _make(V, 64, **rules)
    con.reset(prompt, 50)
    x, tk, ps = rows[0].clone(), toks[0].clone(), poss[0].clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = con.apply(x, tk, ps)
    for k in range(3):
        x.copy_(rows[k])
        tk.copy_(toks[k])
        ps.copy_(poss[k])
        graph.replay()
        assert P.same_bits(out.cpu(), want[k][0]), k
        assert torch.equal(con.hist.cpu()[:51 + 3 * k], want[k][1][:51 + 3 * k]), k
    h = want[2][1].tolist()
    assert h[:48] == prompt.cpu().tolist()[:48] and h[48:57] == torch.cat(toks).cpu().tolist()
    # ... and the three rows are the twin's
    hist = prompt.cpu().tolist() + [0] * 14
    for k in range(3):
        w, hist = CT.twin(rows[k][0].cpu(), hist, toks[k].cpu().tolist(), 48 + 3 * k, 50, **rules)
        assert P.same_bits(want[k][0][0], w), k


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


def _bigrams(s):
    return [tuple(s[i:i + 2]) for i in range(len(s) - 1)]


def test_generate_with_constraints_eager_graphed_and_blocks():
    """The tiny model at temperature 0.8, top_k 50, with n = 2, a banned bigram and a minimum length.  Free-running and teacher-forced:
    the eager loop, the captured step (and forced_block = 4 where tokens are forced) give the same sequence and probability rows bit for
    bit, the history at the end is the inputs by position, and no bigram repeats.  A second generation through the same decoder and the
    same LogitConstraints object does not capture again and matches a fresh eager run — the capture's warm-up steps stored into the
    history and nothing put it back: that is what shows that no snapshot is needed.  With penalties as well: the same three-way equality.
    logprobs=True returns the TokenScores the same committed tokens get when scored without constraints."""
    from cold_compress_amd.harness import GraphedDecoder, LogitPenalties, decode_one_token, generate, prefill

    model = _tiny(torch.bfloat16)
    V = model.config.vocab_size
    prompt = torch.randint(0, 128, (20,), generator=torch.Generator().manual_seed(1), dtype=torch.int32).to(DEV)
    forced = torch.randint(0, 128, (13,), generator=torch.Generator().manual_seed(2), dtype=torch.int32).to(DEV)
    forced[4:8] = forced[0:4].clone()
    sampling = dict(temperature=0.8, top_k=50, seed=1)
    n0 = len(prompt)

    def run(dec, **kw):
        for l in model.layers:
            l.attention.kv_cache.reset()
        seq, second, _ = generate(model, prompt, prefill, dec, max_new_tokens=16, **kw)
        torch.cuda.synchronize()
        return seq.cpu(), second

    def same(a, b):
        return torch.equal(a[0], b[0]) and len(a[1]) == len(b[1]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))

    def hist_ok(con, seq):
        return con.hist.cpu()[:len(seq) - 1].tolist() == seq[:-1].tolist() and int(con.gen_start) == n0

    plain = run(decode_one_token, **sampling)
    gen = plain[0][n0:].tolist()
    term, bigram = gen[1], [gen[2], gen[3]]

    def mk():
        return _make(V, 64, n=2, m=6, terminators=[term], bad_words=[bigram])

    ce = mk()
    eager = run(decode_one_token, constraints=ce, **sampling)
    s = eager[0].tolist()
    assert not torch.equal(eager[0], plain[0]) and hist_ok(ce, eager[0])
    assert len(set(_bigrams(s))) == len(s) - 1 and tuple(bigram) not in _bigrams(s) and term not in s[n0:n0 + 6]
    for k, row in enumerate(eager[1]):  # row k was computed at position n0 - 1 + k: probability 0 exactly where the twin bans
        ban = CT.banned(s[:n0 + k], n0, n=2, m=6, terminators=[term], bad_words=[bigram])
        assert all(float(row[w]) == 0.0 for w in ban) and s[n0 + k] not in ban, k
    cg = mk()
    dec = GraphedDecoder(model, constraints=cg, **sampling)
    graphed = run(dec, constraints=cg, **sampling)
    assert same(graphed, eager) and hist_ok(cg, graphed[0])
    graph1 = dec.graph
    assert graph1 is not None
    # teacher-forced, through the same decoder and the same object: no new capture; blocks of 4 give the same
    e_forced = run(decode_one_token, constraints=ce, next_tokens=forced, **sampling)
    g_forced = run(dec, constraints=cg, next_tokens=forced, **sampling)
    assert dec.graph is graph1 and same(g_forced, e_forced) and hist_ok(cg, g_forced[0]) and hist_ok(ce, e_forced[0])
    cb = mk()
    b_forced = run(decode_one_token, constraints=cb, next_tokens=forced, forced_block=4, **sampling)
    assert same(b_forced, e_forced) and hist_ok(cb, b_forced[0])
    fresh = run(decode_one_token, constraints=mk(), **sampling)
    again = run(dec, constraints=cg, **sampling)
    assert dec.graph is graph1 and same(again, fresh) and same(again, eager)
    # with penalties as well
    def pen():
        return LogitPenalties(V, DEV, 1.3, 0.2, 0.4, {gen[0]: NINF})

    both_e = run(decode_one_token, constraints=mk(), penalties=pen(), **sampling)
    cp, pp = mk(), pen()
    dec_p = GraphedDecoder(model, constraints=cp, penalties=pp, **sampling)
    both_g = run(dec_p, constraints=cp, penalties=pp, **sampling)
    sb = both_e[0].tolist()
    assert same(both_g, both_e) and len(set(_bigrams(sb))) == len(sb) - 1 and gen[0] not in sb[n0:]
    bf_e = run(decode_one_token, constraints=mk(), penalties=pen(), next_tokens=forced, **sampling)
    bf_g = run(dec_p, constraints=cp, penalties=pp, next_tokens=forced, **sampling)
    bf_b = run(decode_one_token, constraints=mk(), penalties=pen(), next_tokens=forced, forced_block=4, **sampling)
    assert same(bf_g, bf_e) and same(bf_b, bf_e)
    # the scores stay the model's own: the constrained run's committed tokens, forced through a run without constraints
    seq_s, scores = run(decode_one_token, constraints=mk(), logprobs=True, **sampling)
    assert torch.equal(seq_s, eager[0])
    seq_f, own = run(decode_one_token, next_tokens=seq_s[n0:].to(DEV), logprobs=True, **sampling)
    assert torch.equal(seq_f, seq_s)
    assert torch.equal(scores.logprob.view(torch.int32), own.logprob.view(torch.int32)) and torch.equal(scores.rank, own.rank)
    cl = mk()
    dec_l = GraphedDecoder(model, constraints=cl, logprobs=True, **sampling)
    seq_g, scores_g = run(dec_l, constraints=cl, logprobs=True, **sampling)
    assert torch.equal(seq_g, seq_s) and torch.equal(scores_g.logprob.view(torch.int32), scores.logprob.view(torch.int32))
