"""Shared by tests/test_streams_logits_host.py and tests/test_gpu_streams_logits.py.  A helper, not a test: per-stream settings of
LogitPenalties / LogitConstraints that are known to bite, fresh objects of them, recorded lone generate() runs with and without
them, and the comparison of a stream of generate_streams with its lone run — tokens, rows or scores, every cache buffer and the
objects' own state afterwards, bit for bit."""
import functools

import torch

import streams_common as SC

V = SC.TINY["vocab_size"]
CAP = 64  # the constraints' max_positions: 40 prompt tokens and 10 new ones fit
SEEDS = [11, 5, 7, 3]
MODES = {"greedy": {}, "greedy-logprobs": dict(logprobs=True), "sampled": dict(SC.SAMPLED), "sampled-logprobs": dict(SC.SAMPLED, logprobs=True)}
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
BUILDERS = {}  # name -> callable returning a fresh model: models that are not SC.tiny (a build key is then (name, None, device))

# settings are kept as sorted tuples of (name, value) pairs so that recorded runs can be cached by them
PEN_A = (("frequency_penalty", 0.4), ("logit_bias", ((9, -float("inf")), (17, 2.0))), ("presence_penalty", 0.2), ("repetition_penalty", 1.3))
PEN_B = (("repetition_penalty", 1.7),)


def build(bk):
    """bk = (dtype name, cache strategy, device) -> a callable building a fresh model"""
    if bk[0] in BUILDERS:
        return BUILDERS[bk[0]]
    return lambda: SC.tiny(DTYPES[bk[0]], bk[1], bk[2])


def make(pen, con, dev):
    """fresh objects of the settings (or None)"""
    from cold_compress_amd.harness import LogitConstraints, LogitPenalties

    def thaw(t):
        return {k: dict(v) if k == "logit_bias" else [list(w) for w in v] if k == "bad_words_ids" else list(v) if isinstance(v, tuple) else v
                for k, v in t}

    return (None if pen is None else LogitPenalties(V, dev, **thaw(pen)), None if con is None else LogitConstraints(V, dev, CAP, **thaw(con)))


@functools.lru_cache(maxsize=None)
def lone(bk, prompt_key, seed, mode, pen, con):
    """-> (SC.lone's result, (prompt_count, gen_count) or None, hist or None) of a lone generate() with fresh objects, on the CPU"""
    p, c = make(pen, con, bk[2])
    res = SC.lone(build(bk), SC.prompt(*prompt_key), seed, penalties=p, constraints=c, **MODES[mode])
    return res, None if p is None else (p.prompt_count.cpu(), p.gen_count.cpu()), None if c is None else c.hist.cpu()


def specs(bk, prompt_key, seeds, mode):
    """Per stream the settings of its penalties and of its constraints: mixed across the streams, stream 1 without penalties, stream 2
    without anything.  The terminator of min_new_tokens and the banned sequences are read from the stream's recorded lone run
    WITHOUT processors, so that they bite: tokens which that run emits among its first new ones."""
    out = []
    for s, seed in enumerate(seeds):
        new = lone(bk, prompt_key, seed, mode, None, None)[0][0][prompt_key[0]:].tolist()
        out.append([
            (PEN_A, (("no_repeat_ngram_size", 2),)),
            (None, (("bad_words_ids", ((new[0], new[1]),)), ("min_new_tokens", 6), ("terminator_ids", (new[2], 1)))),
            (None, None),
            (PEN_B, (("bad_words_ids", ((new[1],), (new[4], new[5]))), ("ngram_scope", "generated"), ("no_repeat_ngram_size", 3))),
        ][s])
    return out


def check(what, bk, prompt_keys, seeds, mode, got, objs, sp):
    for s, (pen, con) in enumerate(sp):
        key = prompt_keys[s]
        want, counts, hist = lone(bk, key, seeds[s], mode, pen, con)
        SC.assert_same(f"{what} stream {s}", got[s], want)
        if pen is not None or con is not None:  # the processors changed this stream's run: the comparison above is about them
            plain = lone(bk, key, seeds[s], mode, None, None)[0]
            assert not torch.equal(want[0], plain[0]), f"{what} stream {s}: the processors changed no token of the lone run"
        p, c = objs[s]
        if p is not None:
            assert torch.equal(p.prompt_count.cpu(), counts[0]) and torch.equal(p.gen_count.cpu(), counts[1]), f"{what} stream {s}: counts"
            assert int(p.prompt_count.sum()) == key[0] and int(p.gen_count.sum()) == SC.NEW_TOKENS - 1
        if c is not None:
            fed = len(want[0]) - 1  # (the last token was chosen, not fed)
            assert torch.equal(c.hist[:fed].cpu(), hist[:fed]), f"{what} stream {s}: history"
            assert torch.equal(c.hist[:fed].cpu().to(want[0].dtype), want[0][:fed]), f"{what} stream {s}: the history is not the sequence"


def fork_case(bk, n, mode, builder=None, **gk):
    """generate_streams of n continuations of the 40-token prompt, every stream with fresh objects of its settings (`builder`: the
    streams' model where it is not the lone runs' build(bk))
    -> (prompt key, settings, objects, per-stream results, stats, model, streams)"""
    key = (40, bk[2])
    sp = specs(bk, key, SEEDS[:n], mode)
    objs = [make(p, c, bk[2]) for p, c in sp]
    model, streams, got, stats = SC.run_streams(builder or build(bk), SC.prompt(*key), n=n, seeds=SEEDS[:n], penalties=[o[0] for o in objs],
                                                constraints=[o[1] for o in objs], **MODES[mode], **gk)
    assert stats["decode_tokens"] == [SC.NEW_TOKENS] * n
    return key, sp, objs, got, stats, model, streams


def batch_case(bk, mode, lengths=(12, 25, 31), **gk):
    """prompts of different lengths (default 12, 25 and 31): every object is reset with its own prompt and its own gen_start"""
    keys = [(L, bk[2], 20 + L) for L in lengths]
    seeds = list(range(len(lengths)))
    sp = [specs(bk, k, [sd] * (s + 1), mode)[s] for s, (k, sd) in enumerate(zip(keys, seeds))]
    objs = [make(p, c, bk[2]) for p, c in sp]
    _, _, got, stats = SC.run_streams(build(bk), [SC.prompt(*k) for k in keys], seeds=seeds, penalties=[o[0] for o in objs],
                                      constraints=[o[1] for o in objs], **MODES[mode], **gk)
    return keys, seeds, sp, objs, got, stats
