"""n-gram blocking, banned sequences and a minimum length on the host side (no GPU): the plain-Python twin of cc_logits_constrain's
contract (tests/constraint_twin.py) against transformers' three processors, the harness's CPU path of `LogitConstraints` against the
twin, the ABI rows and the refusals, and the generation loop with `constraints=` on the tiny model over tests/cpu_twin.py (repeats,
scope, a banned bigram, a minimum length, the positional history, forced blocks, neutral settings, penalties as well, the rewind,
validation)."""
import argparse
import ctypes as C
import os
import random
import re

import pytest
import torch

import constraint_twin as CT
import penalty_twin as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ID = lambda d: str(d).split(".")[-1]  # noqa: E731
NINF = -float("inf")


def _hf_banned(proc, s, V):
    out = proc(torch.tensor([s], dtype=torch.long), torch.zeros(1, V))
    return {j for j in range(V) if float(out[0, j]) == NINF}


def _banned(s, V, gen_start=0, **rules):
    """The twin's banned set for the history s — after checking that LogitConstraints, reset with s, bans exactly those ids on a row of
    zeros at position len(s) - 1 (the prefill's row)."""
    want = CT.banned(s, gen_start, **rules)
    con = _make(V, len(s), **rules)
    con.reset(torch.tensor(s, dtype=torch.int32), gen_start)
    out = con.apply(torch.zeros(1, 1, V), None, torch.tensor([len(s) - 1], dtype=torch.int32))
    assert {j for j in range(V) if float(out[0, 0, j]) == NINF} == want, (s, gen_start, rules)
    return want


def test_the_twin_is_transformers():
    """The twin's three formulas (and with them LogitConstraints' CPU path, `_banned`) against NoRepeatNGramLogitsProcessor, MinNewTokensLengthLogitsProcessor and
    NoBadWordsLogitsProcessor on random histories over an alphabet of 5.  ngram_scope="generated" is the n-gram processor on the
    generated slice alone.  Banned sequences: only where the history is at least as long as the longest sequence (for shorter ones
    transformers applies none of them, which the contract does not follow); at least 80 % of the cases drawn qualify."""
    pytest.importorskip("transformers")
    from transformers.generation.logits_process import (MinNewTokensLengthLogitsProcessor, NoBadWordsLogitsProcessor,
                                                        NoRepeatNGramLogitsProcessor)

    V, rng = 5, random.Random(0)
    for _ in range(400):
        s = [rng.randrange(V) for _ in range(rng.randint(1, 40))]
        n, g = rng.randint(1, 5), rng.randint(0, 41)
        proc = NoRepeatNGramLogitsProcessor(n)
        assert _banned(s, V, n=n) == _hf_banned(proc, s, V), (s, n)
        want = _hf_banned(proc, s[g:], V) if g < len(s) else set()
        assert _banned(s, V, gen_start=g, n=n, scope="generated") == want, (s, n, g)
    for _ in range(300):
        s = [rng.randrange(V) for _ in range(rng.randint(1, 40))]
        g, m = rng.randint(0, len(s)), rng.randint(1, 12)
        terms = rng.sample(range(V), rng.randint(1, 3))
        proc = MinNewTokensLengthLogitsProcessor(g, m, terms)
        assert _banned(s, V, gen_start=g, m=m, terminators=terms) == _hf_banned(proc, s, V), (s, g, m, terms)
    drawn = qualified = 0
    for _ in range(400):
        s = [rng.randrange(V) for _ in range(rng.randint(1, 14))]
        words = []
        for _ in range(rng.randint(1, 4)):
            w = [rng.randrange(V) for _ in range(rng.randint(1, 4))]
            if w not in words:
                words.append(w)
        drawn += 1
        if len(s) < max(len(w) for w in words):
            continue
        qualified += 1
        assert _banned(s, V, bad_words=words) == _hf_banned(NoBadWordsLogitsProcessor(words), s, V), (s, words)
    assert qualified >= 0.8 * drawn, (qualified, drawn)


def test_the_twin_on_known_cases():
    """Hand-worked cases of each rule, for the twin and LogitConstraints alike (these hold whether or not transformers is installed)."""
    assert _banned([1, 2, 3, 1, 2], 10, n=3) == {3}
    assert _banned([1, 2, 3, 1, 2], 10, n=1) == {1, 2, 3}
    assert _banned([7], 10, n=3) == set() and _banned([7, 7], 10, n=3) == set() and _banned([7, 7, 7], 10, n=3) == {7}
    assert _banned([1, 2, 3, 1, 2], 10, gen_start=1, n=3, scope="generated") == set()  # (1, 2, 3) starts in the prompt
    assert _banned([0, 1, 2, 3, 1, 2], 10, gen_start=1, n=3, scope="generated") == {3}
    assert _banned([4, 4], 10, gen_start=1, m=2, terminators=[9]) == {9} and _banned([4, 4, 4], 10, gen_start=1, m=2, terminators=[9]) == set()
    assert _banned([5], 10, bad_words=[[8], [5, 6], [4, 5, 6], [6, 5, 7]]) == {8, 6}
    assert _banned([4, 5], 10, bad_words=[[4, 5, 6], [5, 4, 6]]) == {6}


RULES = dict(n=3, scope="all", m=40, terminators=[1, 5], bad_words=[[2], [1, 6], [0, 1, 2], [2, 0, 1, 3]])
EACH = (dict(n=1), dict(n=2), dict(n=3, scope="generated"), dict(m=40, terminators=[0, 4]), dict(bad_words=[[1, 2], [0, 0, 0], [6]]), RULES)


def _make(V, cap, device="cpu", n=0, scope="all", m=0, terminators=(), bad_words=()):
    from cold_compress_amd.harness import LogitConstraints

    return LogitConstraints(V, device, cap, no_repeat_ngram_size=n, ngram_scope=scope, min_new_tokens=m,
                            terminator_ids=[t for t in terminators if t < V] or None, bad_words_ids=[w for w in bad_words if max(w) < V] or None)


def _rules_for(V, rules):
    r = dict(rules)
    if "terminators" in r:
        r["terminators"] = [t for t in r["terminators"] if t < V]
    if "bad_words" in r:
        r["bad_words"] = [w for w in r["bad_words"] if max(w) < V]
    return r


@pytest.mark.parametrize("dtype", P.DTYPES, ids=_ID)
def test_logit_constraints_on_cpu_tensors(dtype):
    """LogitConstraints.apply on CPU tensors is the twin bit for bit — rows and history — over every family: each rule alone and all
    together, T = 1 .. 4, histories over an alphabet of 3, into a new tensor (the input left as it was) and in place; the prefill's
    row (no tokens); positions at and past the end of the history.  A block equals its rows taken one by one."""
    cap, GS = 48, 30
    for V in (7, 9, 255):
        g = torch.Generator().manual_seed(V)
        fed = torch.randint(0, 3, (36,), generator=g, dtype=torch.int32)
        for rules in EACH:
            rules = _rules_for(V, rules)
            for T in (1, 2, 3, 4):
                toks = torch.randint(0, 3, (T,), generator=g, dtype=torch.int32)
                for name in P.FAMILIES:
                    rows = P.family(name, dtype, V)[:T]
                    con = _make(V, cap, **rules)
                    con.reset(fed, GS)
                    assert con.hist[:36].tolist() == fed.tolist() and int(con.gen_start) == GS
                    hist0 = con.hist.tolist()
                    keep = rows.clone()
                    got = con.apply(rows.unsqueeze(0), toks, torch.tensor([36], dtype=torch.int32))
                    want, hist1 = CT.twin(rows, hist0, toks.tolist(), 36, GS, **rules)
                    assert got.shape == (1, T, V) and P.same_bits(got[0], want), (name, V, T, rules)
                    assert con.hist.tolist() == hist1 and P.same_bits(rows, keep)
                    one = _make(V, cap, **rules)  # the same block, row by row
                    one.reset(fed, GS)
                    for t in range(T):
                        r = one.apply(rows[t:t + 1].unsqueeze(0), toks[t:t + 1], torch.tensor([36 + t], dtype=torch.int32))
                        assert P.same_bits(r[0, 0], got[0, t]), (name, V, T, t)
                    assert one.hist.tolist() == con.hist.tolist()
                    x = rows.clone().unsqueeze(0)  # in place, from the same start
                    con.hist.copy_(torch.tensor(hist0, dtype=torch.int32))
                    assert con.apply(x, toks, torch.tensor([36], dtype=torch.int32), out=x) is x and P.same_bits(x[0], want)
            # the prefill's row: no tokens, the history is hist[0 .. p]; nothing is stored
            con = _make(V, cap, **rules)
            con.reset(fed, GS)
            rows = P.family("normal", dtype, V)[:1]
            got = con.apply(rows.unsqueeze(0), None, torch.tensor([35], dtype=torch.int32))
            assert P.same_bits(got[0], CT.twin(rows, con.hist.tolist(), None, 35, GS, **rules)[0]) and con.hist[:36].tolist() == fed.tolist()
            # positions cap - 2 .. cap + 1: the last two rows are copied, nothing is stored for them
            rows, toks = P.family("normal", dtype, V), torch.tensor([0, 1, 2, 0], dtype=torch.int32)
            hist0 = con.hist.tolist()
            got = con.apply(rows.unsqueeze(0), toks, torch.tensor([cap - 2], dtype=torch.int32))
            want, hist1 = CT.twin(rows, hist0, toks.tolist(), cap - 2, GS, **rules)
            assert P.same_bits(got[0], want) and con.hist.tolist() == hist1 and P.same_bits(got[0, 2:], rows[2:])
            got = con.apply(rows.unsqueeze(0), toks, torch.tensor([cap + 5], dtype=torch.int32))
            assert P.same_bits(got[0], rows) and con.hist.tolist() == hist1


def test_an_ngram_may_straddle_the_block_or_lie_inside_it():
    """n = 3 at T = 4: a prefix made of the last token in front of the block and the block's first token, and an n-gram that lies
    wholly inside the block, both ban — in the twin and in LogitConstraints alike; tokens outside the vocabulary ban nothing."""
    V, cap = 9, 32
    hist = [1, 2, 0, 1, 2, 0, 1, 2, 0, 1]
    rows = torch.zeros(4, V)
    for toks, expect in (([2, 0, 1, 2], [{0}, {1}, {2}, {0}]),      # row 0: the tail (1, 2) = hist[9], tokens[0]
                         ([3, 4, 3, 4], [set(), set(), set(), {3}]),  # row 3: (3, 4) -> 3 lies at positions 10 .. 12
                         ([3, 40, 3, 40], [set(), set(), set(), {3}]),  # an out-of-range token inside the PREFIX compares as an integer
                         ([40, 3, 40, 3], [set(), set(), set(), set()])):  # (40, 3) -> 40: outside the vocabulary, bans nothing
        con = _make(V, cap, n=3)
        con.reset(torch.tensor(hist, dtype=torch.int32), 4)
        got = con.apply(rows.unsqueeze(0), torch.tensor(toks, dtype=torch.int32), torch.tensor([10], dtype=torch.int32))
        want, hist1 = CT.twin(rows, hist + [0] * (cap - 10), toks, 10, 4, n=3)
        assert P.same_bits(got[0], want) and con.hist.tolist() == hist1, toks
        bans = [{j for j in range(V) if float(got[0, t, j]) == NINF} for t in range(4)]
        assert bans == expect, (toks, bans)


def test_abi_surface_and_refusals():
    """Both symbols are in the header and in _abi.py with matching argument counts, device-only and exported; every refusal comes
    before any launch (this machine has no device: a launch would fail with another code), and a bad argument is named before the
    dtype."""
    from cold_compress_amd import _abi, _build

    header = open(os.path.join(ROOT, "include", "coldcompress.h")).read()
    for name, n in (("cc_token_history_write", 6), ("cc_logits_constrain", 20)):
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", header, re.M | re.S)
        assert m and len(m.group(1).split(",")) == len(_abi.SIGNATURES[name][1]) == n, name
        assert name in _abi.DEVICE_ONLY
    assert "cc_constrain.hip" in _build.SOURCES
    fns = _abi.bind(C.CDLL(_build.build()))
    buf = (C.c_char * 512)()
    p = (C.addressof(buf) + 15) & ~15
    OK, BAD, UNSUPPORTED = 0, -1, -2

    wr = fns["cc_token_history_write"]
    ok = dict(hist=p, cap=8, tokens=p + 64, n=4, first_pos=0, stream=None)
    for kw in (dict(hist=None), dict(tokens=None), dict(cap=0), dict(cap=-1), dict(n=-1), dict(hist=p + 2), dict(tokens=p + 66)):
        assert wr(*{**ok, **kw}.values()) == BAD, kw
    assert wr(*{**ok, "n": 0}.values()) == OK and wr(*{**ok, "n": 0, "tokens": None}.values()) == OK  # (no launch)

    f = fns["cc_logits_constrain"]
    ok = dict(logits=p, out=p, T=1, V=8, row_stride=8, dtype=0, hist=p + 64, cap=8, tokens=p + 128, pos=p + 144, gen_start=p + 160, ngram=3,
              ngram_from_gen=0, min_new_tokens=2, term_ids=p + 176, n_term=2, bw_tokens=p + 192, bw_offsets=p + 256, n_bw=2, stream=None)

    def call(**kw):
        return f(*{**ok, **kw}.values())

    bad = (dict(T=0), dict(T=-1), dict(T=5), dict(V=0), dict(V=-8), dict(row_stride=7), dict(row_stride=-8), dict(logits=None), dict(out=None),
           dict(hist=None), dict(pos=None), dict(gen_start=None), dict(cap=0), dict(cap=-4), dict(ngram=-1), dict(ngram=33),
           dict(min_new_tokens=-1), dict(n_term=-1), dict(n_term=65), dict(term_ids=None), dict(n_bw=-1), dict(n_bw=1025), dict(bw_tokens=None),
           dict(bw_offsets=None),
           dict(out=p + 4), dict(out=p + 300, T=2, row_stride=80, dtype=0),  # partial overlaps
           dict(logits=p + 2, out=p + 2, dtype=0), dict(logits=p + 1, out=p + 1, dtype=1), dict(hist=p + 66), dict(tokens=p + 130), dict(pos=p + 146),
           dict(gen_start=p + 162), dict(term_ids=p + 178), dict(bw_tokens=p + 194), dict(bw_offsets=p + 258))  # misaligned
    for kw in bad:
        assert call(**kw) == BAD, kw
    for dt in (3, -1, 17):
        assert call(dtype=dt) == UNSUPPORTED, dt
        for kw in bad:
            if "dtype" not in kw:
                assert call(**{**kw, "dtype": dt}) == BAD, (kw, dt)  # a bad argument is named before the dtype


class Tok:  # (the ids the block-eligible tiny model's caches ask for)
    def special_ids(self):
        return [[1], [2, 3]]

    def punctuation_ids(self):
        return [5, 6, 7]


V_TINY = 128
CAP = 64


def _tiny(strategy="heavy_hitter"):
    import cold_compress_amd.cache as cache
    from cold_compress_amd.harness import ModelArgs, Transformer, setup_caches

    torch.manual_seed(3)
    cfg = dict(block_size=256, vocab_size=V_TINY, n_layer=2, n_head=4, n_local_heads=2, dim=64, intermediate_size=128)
    model = Transformer(ModelArgs(**cfg)).to(torch.float32).eval()
    ap = argparse.ArgumentParser()
    cache.add_cache_arguments(ap)
    kw = vars(ap.parse_args([]))
    kw.update(cache_strategy=[strategy], prompt_compression_strategy=["recent_global"], max_cache_length=[32.0], global_tokens=4, recent_window=8)
    setup_caches(model, Tok(), "cpu", 64, dict(kw))
    return model


def _runner(model, prompt, max_new_tokens=16):
    from cold_compress_amd.harness import decode_one_token, generate, prefill

    def run(prompt=prompt, **kw):
        for l in model.layers:
            l.attention.kv_cache.reset()
        seq, rows, _ = generate(model, prompt, prefill, decode_one_token, max_new_tokens=max_new_tokens, **kw)
        return seq, rows

    return run


def _same_rows(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _prompt(n=20, seed=1):
    return torch.randint(0, V_TINY, (n,), generator=torch.Generator().manual_seed(seed), dtype=torch.int32)


def _bigrams(s):
    return [tuple(s[i:i + 2]) for i in range(len(s) - 1)]


def _con(**kw):
    from cold_compress_amd.harness import LogitConstraints

    return LogitConstraints(V_TINY, "cpu", CAP, **kw)


def test_no_bigram_repeats(monkeypatch, oracle):
    """The unconstrained greedy run (prompt seed 1) does repeat a bigram; with no_repeat_ngram_size = 2 no bigram of the whole
    sequence occurs twice, the run differs, and every returned row has probability 0 exactly where the twin bans."""
    from cpu_twin import cpu_twin

    model = _tiny()
    prompt = _prompt()
    run = _runner(model, prompt, max_new_tokens=24)
    with cpu_twin(monkeypatch, oracle):
        seq0, _ = run()
        seq1, rows1 = run(constraints=_con(no_repeat_ngram_size=2))
    b0, b1 = _bigrams(seq0.tolist()), _bigrams(seq1.tolist())
    assert len(set(_bigrams(prompt.tolist()))) == len(prompt) - 1  # (the prompt itself repeats none)
    assert len(seq0) == len(seq1) == len(prompt) + 24
    assert len(set(b0)) < len(b0) and len(set(b1)) == len(b1) and not torch.equal(seq0, seq1)
    s = seq1.tolist()
    for k, row in enumerate(rows1):  # row k was computed at position len(prompt) - 1 + k
        ban = CT.banned(s[:len(prompt) + k], n=2)
        assert {j for j in range(V_TINY) if float(row[j]) == 0.0} >= ban and s[len(prompt) + k] not in ban


def test_scope_generated_lets_a_prompt_bigram_through(monkeypatch, oracle):
    """The prompt holds the bigram (x, c), ends on x, and the plain run continues with c.  ngram_scope = "all" forbids that c;
    "generated" emits it (the bigram then starts in the prompt and does not count), and still lets no bigram that lies wholly in the
    generated part occur twice."""
    from cpu_twin import cpu_twin

    model = _tiny()
    base = _prompt()
    with cpu_twin(monkeypatch, oracle):
        c = int(_runner(model, base, max_new_tokens=1)()[0][-1])
        prompt = base.clone()
        prompt[5], prompt[6] = base[-1], c
        run = _runner(model, prompt, max_new_tokens=24)
        seq0, _ = run()
        seq_all, _ = run(constraints=_con(no_repeat_ngram_size=2))
        seq_gen, _ = run(constraints=_con(no_repeat_ngram_size=2, ngram_scope="generated"))
    n = len(prompt)
    assert int(seq0[n]) == c  # (the plain run does emit the prompt's bigram)
    assert int(seq_all[n]) != c and int(seq_gen[n]) == c
    inside = _bigrams(seq_gen.tolist()[n:])
    assert len(set(inside)) == len(inside) and len(inside) == 23


def test_a_banned_bigram_never_appears(monkeypatch, oracle):
    """A bigram the plain run emits, given as a banned sequence, never appears, while its first token still does."""
    from cpu_twin import cpu_twin

    model = _tiny()
    prompt = _prompt()
    run = _runner(model, prompt, max_new_tokens=24)
    with cpu_twin(monkeypatch, oracle):
        seq0, _ = run()
        a, b = _bigrams(seq0.tolist()[len(prompt):])[2]
        seq1, _ = run(constraints=_con(bad_words_ids=[[a, b]]))
    gen1 = seq1.tolist()[len(prompt):]
    assert (a, b) in _bigrams(seq0.tolist()) and (a, b) not in _bigrams(seq1.tolist()) and a in gen1 and len(gen1) == 24


def test_min_new_tokens_keeps_the_terminator_away(monkeypatch, oracle):
    """With terminator_ids = [tok], tok among the plain run's first 4 new tokens, the plain run stops early; min_new_tokens = 8 yields
    at least 8 new tokens with no tok among the first 8."""
    from cpu_twin import cpu_twin

    model = _tiny()
    prompt = _prompt()
    run = _runner(model, prompt, max_new_tokens=16)
    with cpu_twin(monkeypatch, oracle):
        seq0, _ = run()
        tok = int(seq0[len(prompt) + 2])
        first = seq0.tolist()[len(prompt):].index(tok)
        seq1, _ = run(terminator_ids=[tok])
        seq2, _ = run(terminator_ids=[tok], constraints=_con(min_new_tokens=8, terminator_ids=[tok]))
    assert first <= 2 and len(seq1) == len(prompt) + first + 1 and int(seq1[-1]) == tok
    gen2 = seq2.tolist()[len(prompt):]
    assert len(gen2) >= 8 and tok not in gen2[:8]


@pytest.mark.parametrize("mode", ["plain", "feed_long_prompts", "decode_first_token", "next_tokens"])
def test_the_history_is_the_inputs_by_position(monkeypatch, oracle, mode):
    """After generate, hist[:len(seq) - 1] is every input the run fed (all of the returned sequence but its last token) and gen_start
    the ORIGINAL prompt length: a prompt tail fed through decode steps is prompt, a forced continuation generated."""
    from cpu_twin import cpu_twin

    model = _tiny()
    n = 40 if mode == "feed_long_prompts" else 20
    prompt = _prompt(n, seed=5)
    kw = {"plain": {}, "feed_long_prompts": dict(feed_long_prompts=True), "decode_first_token": dict(decode_first_token=True),
          "next_tokens": dict(next_tokens=_prompt(13, seed=2))}[mode]
    con = _con(no_repeat_ngram_size=2, ngram_scope="generated", min_new_tokens=3, terminator_ids=[0], bad_words_ids=[[4, 40]])
    with cpu_twin(monkeypatch, oracle):
        assert n < model.min_cache_length() or mode == "feed_long_prompts"
        seq, _ = _runner(model, prompt, max_new_tokens=8)(constraints=con, temperature=0.8, top_k=20, seed=3, **kw)
    assert torch.equal(seq[:n], prompt) and len(seq) == n + (13 if mode == "next_tokens" else 8)
    assert con.hist[:len(seq) - 1].tolist() == seq[:-1].tolist() and int(con.gen_start) == n


def test_forced_blocks_are_the_token_loop(monkeypatch, oracle):
    """forced_block = 4 gives the token-by-token loop's tokens, probability rows and history bit for bit, with sampling and every
    rule on — and did run blocks of 4, each with one apply call."""
    from cpu_twin import cpu_twin

    model = _tiny()
    forced = _prompt(13, seed=2)
    forced[4:8] = forced[0:4]  # (bigrams that repeat inside the forced part: the n-gram rule bans along the way)
    blocks, applies = [], []
    real = model.forward_block

    def counted(idx, input_pos, **kw):
        blocks.append(int(idx.shape[1]))
        return real(idx, input_pos, **kw)

    model.forward_block = counted
    run = _runner(model, _prompt())
    cons = [_con(no_repeat_ngram_size=2, min_new_tokens=20, terminator_ids=[3, 9], bad_words_ids=[[7], [int(forced[1]), 11]]) for _ in range(2)]
    real_apply = cons[1].apply
    cons[1].apply = lambda logits, *a, **k: (applies.append(int(logits.shape[1])), real_apply(logits, *a, **k))[1]
    sampling = dict(temperature=0.8, top_k=20, seed=1)
    with cpu_twin(monkeypatch, oracle):
        assert model.block_eligible()
        seq0, rows0 = run(next_tokens=forced, constraints=cons[0], **sampling)
        assert not blocks
        seq1, rows1 = run(next_tokens=forced, constraints=cons[1], forced_block=4, **sampling)
    assert blocks and max(blocks) == 4 and [a for a in applies if a > 1] == blocks
    assert torch.equal(seq0, seq1) and _same_rows(rows0, rows1)
    assert cons[0].hist.tolist() == cons[1].hist.tolist() and cons[0].hist[:len(seq0) - 1].tolist() == seq0[:-1].tolist()
    assert any(float(r[7]) == 0.0 and float(r[3]) == 0.0 for r in rows0)


def test_neutral_settings_are_no_constraints(monkeypatch, oracle):
    from cpu_twin import cpu_twin

    model = _tiny()
    run = _runner(model, _prompt())
    neutral = _con(terminator_ids=[3], ngram_scope="generated")
    assert neutral.neutral and not _con(no_repeat_ngram_size=1).neutral and not _con(bad_words_ids=[[1]]).neutral
    assert not _con(min_new_tokens=1, terminator_ids=[3]).neutral
    neutral.hist.fill_(-7)
    with cpu_twin(monkeypatch, oracle):
        for sampling in (dict(), dict(temperature=0.8, top_k=20, seed=1)):
            seq0, rows0 = run(**sampling)
            seq1, rows1 = run(constraints=neutral, **sampling)
            assert torch.equal(seq0, seq1) and _same_rows(rows0, rows1)
    assert bool((neutral.hist == -7).all()) and int(neutral.gen_start) == 0  # (nothing ran)
    x = torch.randn(1, 2, V_TINY)
    assert neutral.apply(x, torch.tensor([1, 2]), torch.tensor([0, 1])) is x


def test_constraints_and_penalties_commute(monkeypatch, oracle):
    """generate with penalties= and constraints=: every returned row is the softmax of the twins' two maps applied to the model's own
    row in either order (the run without either, forced along the same tokens, supplies those rows through the probabilities' support:
    here the maps are applied to random rows directly), and the sequence obeys both."""
    from cpu_twin import cpu_twin

    from cold_compress_amd.harness import LogitPenalties

    # the two maps on the same rows, either order, bit for bit (penalties map -inf to -inf; a banned NaN becomes -inf either way)
    V, GS = 255, 6
    hist = [3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5]
    toks, pos = [1, 4, 1, 5], [11, 12, 13, 14]
    pc = torch.bincount(torch.tensor(hist[:GS]), minlength=V).to(torch.int32)
    gc = torch.bincount(torch.tensor(hist[GS:]), minlength=V).to(torch.int32)
    rules = dict(n=2, m=40, terminators=[0, 7], bad_words=[[2], [5, 8]])
    r, f, p = P.ALL_ON
    for dtype in P.DTYPES:
        for name in P.FAMILIES:
            rows = P.family(name, dtype, V)
            a = CT.twin(P.twin(rows, pc, gc, GS, toks, pos, r, f, p, None)[0], hist + [0] * 21, toks, 11, GS, **rules)[0]
            b = P.twin(CT.twin(rows, hist + [0] * 21, toks, 11, GS, **rules)[0], pc, gc, GS, toks, pos, r, f, p, None)[0]
            assert P.same_bits(a, b), (name, dtype)
            pen, con = LogitPenalties(V, "cpu", r, f, p), _make(V, 32, **rules)
            pen.reset(torch.tensor(hist, dtype=torch.int32), GS)
            con.reset(torch.tensor(hist, dtype=torch.int32), GS)
            tk, ps = torch.tensor(toks, dtype=torch.int32), torch.tensor(pos, dtype=torch.int32)
            y = pen.apply(rows.unsqueeze(0), tk, ps)
            assert P.same_bits(con.apply(y, tk, ps, out=y)[0], a), (name, dtype)
    # through generate: the run with both equals the run with the constraints and the penalties' ban folded into the banned sequences
    model = _tiny()
    run = _runner(model, _prompt(), max_new_tokens=24)
    with cpu_twin(monkeypatch, oracle):
        seq0, rows0 = run(constraints=_con(no_repeat_ngram_size=2, bad_words_ids=[[117]]))
        seq1, rows1 = run(constraints=_con(no_repeat_ngram_size=2), penalties=LogitPenalties(V_TINY, "cpu", logit_bias={117: NINF}))
        seq2, _ = run(constraints=_con(no_repeat_ngram_size=2), penalties=LogitPenalties(V_TINY, "cpu", 1.3, 0.2, 0.4))
    assert torch.equal(seq0, seq1) and _same_rows(rows0, rows1) and 117 not in seq0.tolist()[20:]
    b2 = _bigrams(seq2.tolist())
    assert len(set(b2)) == len(b2)


def test_rewind_needs_no_rebuild(monkeypatch):
    """The decode loop over a stand-in device (the watch of test_penalties_host.py's rewind test): a token whose single-launch step
    fails is seen `lag` tokens late; its own launch and every launch behind it chose garbage and STORED garbage inputs — at positions
    past the failed one.  The rewound run ends with the fault-free run's sequence and the same history, and no rebuild hook exists
    for constraints: `_recover_token` is handed none."""
    from cold_compress_amd.harness import LogitConstraints
    from cold_compress_amd.harness import generation as G

    V, P0 = 1024, 40
    real_watch = G._StatusWatch
    live = {"state": None, "fail_at": None}
    prompt = torch.randint(0, V, (P0,), generator=torch.Generator().manual_seed(4), dtype=torch.int32)
    assert not hasattr(LogitConstraints, "rebuild") and not hasattr(LogitConstraints, "snapshot")

    def step(model, x, pos, next_token=None, attn_top_k=1.0, constraints=None, **kw):
        # (a row that depends on the position alone and has few distinct maxima: the n-gram rule decides most steps)
        logits = torch.randn(1, 1, V, generator=torch.Generator().manual_seed(int(pos[0]) % 3))
        t = torch.argmax(constraints.apply(logits, x, pos)[0, -1]).view(1).to(torch.int32)
        st = live["state"]
        k = int(pos[0]) - P0
        if st is not None and (st["set"] or (k == live["fail_at"] and not st["failed_once"])):
            t = torch.tensor([977], dtype=torch.int32)  # the launch did nothing: garbage, which the next step stores
        return (next_token if next_token is not None else t), torch.ones(1)

    def run(fail_at, lag, n=12):
        state = {"set": False, "failed_once": False}
        live["state"], live["fail_at"] = state, fail_at

        class Watch(real_watch):
            def __init__(self, dev):
                super().__init__(dev, depth=64)

            def _open(self, dev):
                self.values, self.started, self.n_posted = {}, {}, 0

            def _start(self, slot):
                i = self.n_posted
                if i == fail_at and not state["failed_once"]:
                    state["set"], state["failed_once"] = True, True
                self.values[slot] = int(state["set"])
                self.started[slot] = i
                self.n_posted += 1

            def post(self, token_index):
                self.n_posted = token_index
                super().post(token_index)

            def _is_done(self, slot):
                return self.n_posted - 1 - self.started[slot] >= lag

            def _wait_done(self, slot):
                pass

            def _status(self, slot):
                return self.values[slot]

        def recover(model, cur, pos, fn, nt, npb, forced, top_k, kw, max_retries=6, rebuild=None):
            assert state["set"] and rebuild is None  # (nothing to rebuild)
            state["set"] = False
            return fn(model, cur, pos, next_token=forced, attn_top_k=top_k, **kw)

        monkeypatch.setattr(G, "_StatusWatch", Watch)
        monkeypatch.setattr(G, "_recover_token", recover)
        con = LogitConstraints(V, "cpu", P0 + n + 24, no_repeat_ngram_size=2, bad_words_ids=[[3, 5]])
        con.hist.fill_(-5)
        con.reset(prompt, P0)
        pos = torch.tensor([P0], dtype=torch.int32)
        toks, _ = G.decode_n_tokens(None, torch.tensor([[3]], dtype=torch.int32), pos, step, n, recover=fail_at is not None or None,
                                    constraints=con)
        return [int(t) for t in toks], int(pos[0]), con

    clean, end, con0 = run(None, 0)
    assert end == P0 + 12 and len(clean) == 12 and 977 not in clean
    assert con0.hist[:end].tolist() == prompt.tolist() + [3] + clean[:-1]
    assert len(set(_bigrams([3] + clean))) == 12 and len(set(clean)) < 12  # (the rule did decide: three rows, twelve distinct bigrams)
    for fail_at in (0, 1, 5):
        for lag in (0, 3, 20):
            got, e, con = run(fail_at, lag)
            assert got == clean and e == end, (fail_at, lag, got, clean)
            assert con.hist[:end].tolist() == con0.hist[:end].tolist(), (fail_at, lag)


def test_invalid_settings_raise(monkeypatch, oracle):
    from cpu_twin import cpu_twin

    from cold_compress_amd.harness import LogitConstraints

    for kw in (dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=33), dict(no_repeat_ngram_size=1.5), dict(ngram_scope="prompt"),
               dict(min_new_tokens=-1), dict(min_new_tokens=2), dict(min_new_tokens=2, terminator_ids=[]),
               dict(min_new_tokens=2, terminator_ids=[V_TINY]), dict(terminator_ids=[-1]), dict(terminator_ids=list(range(65))),
               dict(bad_words_ids=[[]]), dict(bad_words_ids=[[1, V_TINY]]), dict(bad_words_ids=[[-1]]), dict(bad_words_ids=[[1] * 33]),
               dict(bad_words_ids=[[1]] * 1025), dict(bad_words_ids=[[1] * 32] * 129), dict(bad_words_ids=[[1.5]])):
        with pytest.raises(ValueError):
            LogitConstraints(V_TINY, "cpu", CAP, **kw)
    for cap in (0, -1, 1.5):
        with pytest.raises(ValueError):
            LogitConstraints(V_TINY, "cpu", cap, no_repeat_ngram_size=2)
    with pytest.raises(ValueError):
        LogitConstraints(0, "cpu", CAP)
    ok = LogitConstraints(V_TINY, "cpu", CAP, no_repeat_ngram_size=32, min_new_tokens=1, terminator_ids=list(range(64)),
                          bad_words_ids=[[1] * 32] * 128)
    assert not ok.neutral
    with pytest.raises(ValueError):
        ok.apply(torch.zeros(1, 1, V_TINY + 1), torch.tensor([1]), torch.tensor([0]))
    with pytest.raises(ValueError):
        ok.apply(torch.zeros(1, 2, V_TINY), torch.tensor([1]), torch.tensor([0]))
    with pytest.raises(ValueError):
        ok.apply(torch.zeros(1, 1, V_TINY), torch.tensor([1]))
    with pytest.raises(ValueError):
        ok.reset(torch.zeros(CAP + 1, dtype=torch.int32), 0)
    # generate refuses a run that cannot fit the history — before the prefill: the model is never called
    model = _tiny()
    calls = []
    real = model.forward
    model.forward = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    with cpu_twin(monkeypatch, oracle):
        small = LogitConstraints(V_TINY, "cpu", 27, no_repeat_ngram_size=2)
        with pytest.raises(ValueError):
            _runner(model, _prompt(), max_new_tokens=8)(constraints=small)
        assert not calls
        seq, _ = _runner(model, _prompt(), max_new_tokens=7)(constraints=small)
    assert calls and len(seq) == 27
