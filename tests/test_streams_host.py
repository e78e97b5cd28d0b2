"""Decode streams without a GPU (harness/streams.py over tests/cpu_twin.py: Transformer.forward_streams' row-by-row twin): every
stream of generate_streams — fork and batch — equals a lone generate() of that stream on a fresh model in its sequence, every
step's probability row or scores and every cache buffer of every layer, bit for bit; terminators trim a stream where its lone run
stops; DecodeStreams.fork copies everything a continued decode needs; what is not served raises before anything runs; and a plain
generate() behind the call behaves as on a fresh model."""
import functools

import pytest
import torch

import streams_common as SC
from cpu_twin import cpu_twin

DEV = "cpu"
DT = torch.float32


@pytest.fixture()
def twin(monkeypatch, oracle):
    with cpu_twin(monkeypatch, oracle) as fns:
        yield fns


def _build(strategy, extra=()):
    return lambda: SC.tiny(DT, strategy, DEV, **dict(extra))


@functools.lru_cache(maxsize=None)
def _lone(strategy, extra, seed, mode):
    gk = dict(SC.SAMPLED, logprobs=(mode == "logprobs"))
    return SC.lone(_build(strategy, extra), SC.prompt(40, DEV), seed, **gk)


@pytest.mark.parametrize("mode", ["sampled", "logprobs"])
@pytest.mark.parametrize("n", [2, 3, 4])
@pytest.mark.parametrize("strategy,extra", SC.POLICIES, ids=SC.POLICY_IDS)
def test_fork_streams_equal_their_lone_runs(twin, strategy, extra, n, mode):
    ex = tuple(sorted(extra.items()))
    seeds = [11, 5, 7, 3][:n]
    gk = dict(SC.SAMPLED, logprobs=(mode == "logprobs"))
    _, _, got, stats = SC.run_streams(_build(strategy, ex), SC.prompt(40, DEV), n=n, seeds=seeds, **gk)
    assert stats["streams"] == n and stats["decode_tokens"] == [SC.NEW_TOKENS] * n and stats["prefill_tokens"] == 40
    for s in range(n):
        SC.assert_same(f"{strategy} n={n} {mode} stream {s}", got[s], _lone(strategy, ex, seeds[s], mode))
    assert len({tuple(g[0].tolist()) for g in got}) > 1, "the seeds gave one continuation: the comparison shows nothing about seeds"


def test_batch_streams_equal_their_lone_runs(twin):
    """three prompts of different lengths, greedy: per-stream positions, all below the cache (nothing is evicted at first)"""
    prompts = [SC.prompt(L, DEV, seed=20 + L) for L in (12, 25, 31)]
    _, _, got, stats = SC.run_streams(_build("heavy_hitter"), prompts)
    assert stats["prefill_tokens"] == 12 + 25 + 31
    for s, p in enumerate(prompts):
        SC.assert_same(f"batch stream {s}", got[s], SC.lone(_build("heavy_hitter"), p, s))


def test_a_terminator_trims_one_stream_and_not_the_others(twin):
    """the terminator is read from recorded lone runs: a token one stream emits by decode step 4 and another never emits"""
    seeds = [11, 5, 7]
    ex = ()
    lone = [_lone("heavy_hitter", ex, s, "sampled") for s in seeds]
    new = [l[0][41:].tolist() for l in lone]  # (behind the prefill's token, which does not stop a run)
    pick = None
    for a in range(3):
        for k in range(4):
            if any(new[a][k] not in new[b] for b in range(3) if b != a) and new[a][k] not in new[a][:k]:
                pick = pick or (a, new[a][k])
    assert pick is not None, new
    a, term = pick
    _, _, got, stats = SC.run_streams(_build("heavy_hitter"), SC.prompt(40, DEV), n=3, seeds=seeds, terminator_ids=[term], **SC.SAMPLED)
    stopped = 0
    for s in range(3):
        want = SC.lone(_build("heavy_hitter"), SC.prompt(40, DEV), seeds[s], terminator_ids=[term], **SC.SAMPLED)
        early = len(want[0]) < 40 + SC.NEW_TOKENS
        stopped += early
        assert not early or int(want[0][-1]) == term
        # (a finished stream keeps stepping with its results discarded: its caches are past where the lone run stopped)
        SC.assert_same(f"terminator stream {s}", got[s], want, state=not early)
        assert stats["decode_tokens"][s] == len(want[1])
    assert len(got[a][0]) <= 40 + 1 + 4 and 1 <= stopped < 3


def test_fork_copies_everything_a_continued_decode_needs(twin):
    """after fork(), five single steps on stream 1 leave what the same steps leave on stream 0 of an identically built model"""
    from cold_compress_amd.harness import DecodeStreams, decode_one_token

    for strategy, extra in SC.POLICIES:
        if strategy == "random":  # (its streams evict independently by design)
            continue
        outs = []
        for which in (1, 0):
            model = SC.tiny(DT, strategy, DEV, **extra)
            streams = DecodeStreams(model, 2)
            p = SC.prompt(40, DEV)
            tok, _ = SC.prefill_fn()(model, p.view(1, -1), torch.arange(40))
            streams.fork()
            streams.activate(which)
            toks = []
            for i in range(5):
                tok, _ = decode_one_token(model, tok.view(1, 1), torch.tensor([40 + i], dtype=torch.int32))
                tok = tok.clone()
                toks.append(int(tok))
            outs.append((toks, SC.state_of(streams.sets[which])))
            streams.activate(0)
        assert outs[0][0] == outs[1][0], strategy
        for name in outs[0][1]:
            assert torch.equal(outs[0][1][name], outs[1][1][name]), (strategy, name)


def test_what_is_not_served_raises_before_anything_runs(twin):
    from cold_compress_amd.harness import DecodeStreams, LogitConstraints, LogitPenalties, generate_streams

    model = SC.tiny(DT, "heavy_hitter", DEV)
    p = SC.prompt(20, DEV)
    ran = []

    def pf(*a, **k):
        ran.append(1)
        raise AssertionError("the prefill ran")

    for kw in (dict(penalties=LogitPenalties(128, DEV, 1.2, 0.0, 0.0)), dict(constraints=LogitConstraints(128, DEV, 64, no_repeat_ngram_size=2)),
               dict(top_logprobs=3, logprobs=True), dict(next_tokens=torch.tensor([1, 2], dtype=torch.int32)), dict(feed_long_prompts=True),
               dict(decode_first_token=True)):
        with pytest.raises(ValueError):
            generate_streams(model, p, pf, 4, n_streams=2, **kw)
    with pytest.raises(ValueError):  # a prompt generate() would split
        generate_streams(model, SC.prompt(32, DEV), pf, 4, n_streams=2)
    with pytest.raises(ValueError):
        generate_streams(model, [p, SC.prompt(32, DEV)], pf, 4)
    for bad in (dict(n_streams=5), dict(n_streams=0), dict(n_streams=None), dict(n_streams=2, seeds=[1])):
        with pytest.raises(ValueError):
            generate_streams(model, p, pf, 4, **bad)
    with pytest.raises(ValueError):
        generate_streams(model, [p] * 5, pf, 4)
    for n in (0, 5, -1):
        with pytest.raises(ValueError):
            DecodeStreams(model, n)
    assert not ran and DecodeStreams(model, 4).n == 4


def test_a_plain_generate_behind_the_call_equals_a_fresh_models(twin):
    from cold_compress_amd.harness import decode_one_token, generate

    model, streams, _, _ = SC.run_streams(_build("heavy_hitter"), SC.prompt(40, DEV), n=3, **SC.SAMPLED)
    model.reset_caches()
    seq, probs, _ = generate(model, SC.prompt(40, DEV), SC.prefill_fn(), decode_one_token, max_new_tokens=SC.NEW_TOKENS, seed=11, **SC.SAMPLED)
    got = (seq, SC.cpu(probs), SC.state_of([l.attention.kv_cache for l in model.layers]))
    SC.assert_same("generate() behind generate_streams", got, _lone("heavy_hitter", (), 11, "sampled"))
