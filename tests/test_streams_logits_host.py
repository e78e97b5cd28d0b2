"""Logit processors per stream in generate_streams, without a GPU (harness/streams.py over tests/cpu_twin.py): every stream carries
its OWN LogitPenalties / LogitConstraints (or None) and equals a lone generate() of that stream with fresh objects of the same
settings — tokens, rows or scores, every cache buffer, and afterwards the objects' own state (prompt_count, gen_count, the history
up to the last position fed) — bit for bit.  A comparison cannot pass by the processors doing nothing: for every stream that carries
some, its lone run WITH them differs from its lone run WITHOUT them, which is asserted (streams_logits_common.check).  What stays
refused raises before the prefill."""
import pytest
import torch

import streams_common as SC
import streams_logits_common as SL
from cpu_twin import cpu_twin

DEV = "cpu"
V = SL.V


@pytest.fixture()
def twin(monkeypatch, oracle):
    with cpu_twin(monkeypatch, oracle) as fns:
        yield fns


@pytest.mark.parametrize("mode", list(SL.MODES))
@pytest.mark.parametrize("n", [2, 3, 4])
@pytest.mark.parametrize("strategy", ["heavy_hitter", "full", "l2", "hybrid"])
def test_fork_streams_with_their_own_processors_equal_their_lone_runs(twin, strategy, n, mode):
    bk = ("fp32", strategy, DEV)
    key, sp, objs, got, _, _, _ = SL.fork_case(bk, n, mode)
    SL.check(f"{strategy} n={n} {mode}", bk, [key] * n, SL.SEEDS[:n], mode, got, objs, sp)


@pytest.mark.parametrize("mode", ["greedy", "sampled-logprobs"])
def test_batch_streams_with_their_own_processors_equal_their_lone_runs(twin, mode):
    bk = ("fp32", "heavy_hitter", DEV)
    keys, seeds, sp, objs, got, stats = SL.batch_case(bk, mode)
    assert stats["prefill_tokens"] == 12 + 25 + 31
    SL.check(f"batch {mode}", bk, keys, seeds, mode, got, objs, sp)


def test_neutral_objects_behave_as_none(twin):
    from cold_compress_amd.harness import LogitConstraints, LogitPenalties

    bk = ("fp32", "heavy_hitter", DEV)
    pens = [LogitPenalties(V, DEV), None]
    cons = [None, LogitConstraints(V, DEV, 4)]  # (neutral: its max_positions is not looked at)
    _, _, got, _ = SC.run_streams(SL.build(bk), SC.prompt(40, DEV), n=2, seeds=SL.SEEDS[:2], penalties=pens, constraints=cons, **SC.SAMPLED)
    for s in range(2):
        SC.assert_same(f"neutral stream {s}", got[s], SL.lone(bk, (40, DEV), SL.SEEDS[s], "sampled", None, None)[0])
    assert int(pens[0].prompt_count.sum()) == 0


def test_a_finished_stream_keeps_its_tokens_and_the_others_their_state(twin):
    """a terminator that stream 0's lone run (with its processors) emits early and stream 1's never: stream 0 is trimmed where its lone
    run stops — its objects' state runs on past the terminator and is not compared — stream 1 is whole, state included"""
    bk, key, mode = ("fp32", "heavy_hitter", DEV), (40, DEV), "sampled"
    sp = SL.specs(bk, key, SL.SEEDS[:2], mode)
    new = [SL.lone(bk, key, SL.SEEDS[s], mode, *sp[s])[0][0][41:].tolist() for s in range(2)]
    term = next(t for t in new[0][:6] if t not in new[1])
    objs = [SL.make(p, c, DEV) for p, c in sp]
    _, _, got, _ = SC.run_streams(SL.build(bk), SC.prompt(*key), n=2, seeds=SL.SEEDS[:2], terminator_ids=[term],
                                  penalties=[o[0] for o in objs], constraints=[o[1] for o in objs], **SL.MODES[mode])
    for s in range(2):
        p, c = SL.make(*sp[s], DEV)
        want = SC.lone(SL.build(bk), SC.prompt(*key), SL.SEEDS[s], terminator_ids=[term], penalties=p, constraints=c, **SL.MODES[mode])
        early = len(want[0]) < 40 + SC.NEW_TOKENS
        assert early == (s == 0)
        SC.assert_same(f"terminator stream {s}", got[s], want, state=not early)
        if not early:
            fed = len(want[0]) - 1
            assert torch.equal(objs[s][1].hist[:fed], c.hist[:fed])


def test_what_stays_refused_raises_before_the_prefill(twin):
    from cold_compress_amd.harness import LogitConstraints, LogitPenalties, generate_streams

    model = SC.tiny(torch.float32, "heavy_hitter", DEV)
    p = SC.prompt(20, DEV)
    ran = []

    def pf(*a, **k):
        ran.append(1)
        raise AssertionError("the prefill ran")

    pen = lambda v=V: LogitPenalties(v, DEV, 1.2)  # noqa: E731
    con = lambda cap=64, v=V: LogitConstraints(v, DEV, cap, no_repeat_ngram_size=2)  # noqa: E731
    one = pen()
    with pytest.raises(ValueError, match="list"):  # a single object: the message points to the list form
        generate_streams(model, p, pf, 4, n_streams=2, penalties=one)
    with pytest.raises(ValueError, match="list"):
        generate_streams(model, p, pf, 4, n_streams=2, constraints=con())
    for kw in (dict(penalties=[pen()]), dict(penalties=[pen(), pen(), pen()]), dict(constraints=[con()]),  # a wrong length
               dict(penalties=[one, one]), dict(constraints=[con()] * 2),  # one object twice
               dict(penalties=[pen(V + 1), None]), dict(constraints=[None, con(64, V - 1)]),  # another vocabulary
               dict(constraints=[con(23), None]),  # 20 + 4 positions do not fit 23
               dict(penalties=[pen(), "x"]), dict(penalties={0: pen()}), dict(constraints=[pen(), None]),  # not the objects
               dict(penalties=[pen(), None], top_logprobs=3, logprobs=True), dict(penalties=[pen(), None], next_tokens=torch.tensor([1, 2])),
               dict(constraints=[con(), None], feed_long_prompts=True), dict(constraints=[con(), None], decode_first_token=True)):
        with pytest.raises(ValueError):
            generate_streams(model, p, pf, 4, n_streams=2, **kw)
    with pytest.raises(ValueError):  # batch: every stream's own prompt length counts
        generate_streams(model, [p, SC.prompt(25, DEV)], pf, 4, constraints=[con(24), con(28)])
    generate_streams_ok = dict(constraints=[con(24), None])  # 20 + 4 fit 24: this one reaches the prefill
    with pytest.raises(AssertionError, match="the prefill ran"):
        generate_streams(model, p, pf, 4, n_streams=2, **generate_streams_ok)
    assert ran == [1]
