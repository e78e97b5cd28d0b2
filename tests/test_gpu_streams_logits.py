"""Logit processors per stream in generate_streams on the device (harness/streams.py): tests/test_streams_logits_host.py's
comparisons — every stream with its own LogitPenalties / LogitConstraints equals a lone generate() with fresh objects of the same
settings in tokens, rows or scores, every cache buffer and the objects' own state, bit for bit — for bf16 and fp32, captured and
eager joint steps, fork and batch, the int4 joint route and the one-at-a-time route.  Counters on the glue functions show that a
joint step makes ONE cc_logits_penalize_streams and ONE cc_logits_constrain_streams call whatever n is and none of the
single-sequence ones, and that a decoder reused with other settings of the same objects captures again."""
import gc

import pytest
import torch

import streams_common as SC
import streams_logits_common as SL

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODE = {2: "greedy-logprobs", 4: "sampled"}  # greedy and sampled, with and without logprobs, over the two stream counts
BATCH_MODE = {2: "sampled-logprobs", 4: "greedy"}
LENGTHS = {2: (12, 25), 4: (12, 25, 31, 18)}


def _counted(fn):
    """fn() with the four logit-processor glue functions counted -> (result, {name: [T per call]})"""
    from cold_compress_amd.harness import glue

    names = ("logits_penalize_streams", "logits_constrain_streams", "logits_penalize", "logits_constrain")
    real = {k: getattr(glue, k) for k in names}
    calls = {k: [] for k in names}

    def counted(k):
        def f(x, *a, **kw):
            calls[k].append(1 if x.dim() == 1 else x.shape[0])
            return real[k](x, *a, **kw)

        return f

    for k in names:
        setattr(glue, k, counted(k))
    try:
        out = fn()
    finally:
        for k in names:
            setattr(glue, k, real[k])
    return out, calls


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("n", [2, 4])
@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_fork_streams_with_their_own_processors_equal_their_lone_runs(dt, n, graph):
    bk, mode = (dt, "heavy_hitter", DEV), MODE[n]
    (key, sp, objs, got, stats, _, _), calls = _counted(lambda: SL.fork_case(bk, n, mode, graph=graph))
    assert stats["joint_steps"] and bool(stats["graphed"]) == graph, stats
    SL.check(f"fork {dt} n={n} {mode} graph={graph}", bk, [key] * n, SL.SEEDS[:n], mode, got, objs, sp)
    # the prefill's row and every joint step that ran eagerly (graph: two warm-up steps and the captured one): one call each, of n rows
    steps = 1 + (3 if graph else SC.NEW_TOKENS - 1)
    assert calls["logits_penalize_streams"] == [n] * steps and calls["logits_constrain_streams"] == [n] * steps, calls
    assert not calls["logits_penalize"] and not calls["logits_constrain"], calls


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("n", [2, 4])
@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_batch_streams_with_their_own_processors_equal_their_lone_runs(dt, n, graph):
    bk, mode = (dt, "heavy_hitter", DEV), BATCH_MODE[n]
    (keys, seeds, sp, objs, got, stats), calls = _counted(lambda: SL.batch_case(bk, mode, LENGTHS[n], graph=graph))
    assert stats["joint_steps"] and bool(stats["graphed"]) == graph, stats
    SL.check(f"batch {dt} n={n} {mode} graph={graph}", bk, keys, seeds, mode, got, objs, sp)
    steps = 3 if graph else SC.NEW_TOKENS - 1  # (the prefills go through the single-sequence entry points, as prefill() serves them)
    assert calls["logits_penalize_streams"] == [n] * steps and calls["logits_constrain_streams"] == [n] * steps, calls


def test_constraints_without_penalties_and_penalties_without_constraints():
    """one stage alone: the constraints then write a new tensor (the model's rows stay what the scores read)"""
    bk, mode = ("bf16", "heavy_hitter", DEV), "sampled-logprobs"
    for which in ("constraints", "penalties"):
        con = (("no_repeat_ngram_size", 1),) if which == "constraints" else None
        pen = SL.PEN_A if which == "penalties" else None
        objs = [SL.make(pen, con, DEV) for _ in range(2)]
        kw = {which: [o[0 if which == "penalties" else 1] for o in objs]}
        (_, _, got, stats), calls = _counted(lambda: SC.run_streams(SL.build(bk), SC.prompt(40, DEV), n=2, seeds=SL.SEEDS[:2], **kw, **SL.MODES[mode]))
        assert stats["graphed"] and not calls["logits_constrain_streams" if which == "penalties" else "logits_penalize_streams"], calls
        for s in range(2):
            want = SL.lone(bk, (40, DEV), SL.SEEDS[s], mode, pen, con)[0]
            SC.assert_same(f"{which} alone, stream {s}", got[s], want)
            assert not torch.equal(want[0], SL.lone(bk, (40, DEV), SL.SEEDS[s], mode, None, None)[0][0])


def test_the_int4_joint_route_and_the_one_at_a_time_route():
    """an int4 model with `block_int4` decodes its streams jointly (cc_gemv_fused_w4_multi) and puts the rows through the two streams
    launches; without the attribute it is not eligible and every stream takes decode_one_token with its own objects"""
    import test_gpu_int4_blocks_streams as I4

    SL.BUILDERS["int4"] = lambda: I4._model(block_int4=False)  # the lone runs: the per-token route
    bk, mode, n = ("int4", None, DEV), "sampled", 3
    for joint in (True, False):
        (key, sp, objs, got, stats, model, streams), calls = _counted(
            lambda: SL.fork_case(bk, n, mode, builder=lambda: I4._model(block_int4=joint)))
        assert bool(stats["joint_steps"]) == joint and bool(stats["graphed"]) == joint, stats
        assert bool(model.streams_eligible(streams)) == joint
        SL.check(f"int4 joint={joint}", bk, [key] * n, SL.SEEDS[:n], mode, got, objs, sp)
        if joint:
            assert calls["logits_penalize_streams"] == [n] * 4 and not calls["logits_penalize"], calls
        else:  # the prefill's row through the streams form, every step through the single-sequence entry points, per stream
            assert calls["logits_penalize_streams"] == [n] and calls["logits_constrain_streams"] == [n], calls
            assert len(calls["logits_penalize"]) == SC.NEW_TOKENS - 1, calls  # (stream 0 alone has penalties)
            assert len(calls["logits_constrain"]) == 2 * (SC.NEW_TOKENS - 1), calls  # (streams 0 and 1 have constraints)


def test_a_decoder_reused_with_other_settings_of_its_objects_captures_again():
    """the objects' identities AND their settings are part of the captured step's settings: the same objects again replay the graph,
    the same objects with another penalty capture again, and both runs equal lone runs with those settings"""
    from cold_compress_amd.harness import DecodeStreams, GraphedStreamsDecoder, generate_streams

    bk, mode, n = ("bf16", "heavy_hitter", DEV), "sampled", 2
    other = (("repetition_penalty", 0.5),)
    sp = [(SL.PEN_A, (("no_repeat_ngram_size", 2),)), (SL.PEN_B, None)]
    # the lone runs first: a model that is freed moves glue.w12_epoch(), which (rightly) makes every holder of a graph capture again
    want = [SL.lone(bk, (40, DEV), SL.SEEDS[s], mode, *sp[s])[0] for s in range(n)]
    want_other = SL.lone(bk, (40, DEV), SL.SEEDS[1], mode, other, None)[0]
    gc.collect()
    objs = [SL.make(p, c, DEV) for p, c in sp]
    model = SL.build(bk)()
    streams = DecodeStreams(model, n)
    dec = GraphedStreamsDecoder(model, streams, SL.SEEDS[:n], **SC.SAMPLED, penalties=[o[0] for o in objs], constraints=[o[1] for o in objs])

    def run():
        model.reset_caches()
        streams.reset()
        seqs, probs, stats = generate_streams(model, SC.prompt(40, DEV), SC.prefill_fn(), SC.NEW_TOKENS, n_streams=n, seeds=SL.SEEDS[:n],
                                              streams=streams, decoder=dec, penalties=[o[0] for o in objs], constraints=[o[1] for o in objs],
                                              **SL.MODES[mode])
        torch.cuda.synchronize()
        return [(seqs[s].cpu(), SC.cpu(probs[s]), SC.state_of(streams.sets[s])) for s in range(n)], stats

    first, stats = run()
    assert stats["graphed"] and stats["captures"] == dec.captures == 1
    again, stats = run()
    assert stats["graphed"] and dec.captures == 1, "the same objects and settings captured again"
    objs[1][0].repetition_penalty = 0.5  # (exact in fp32, as the constructor would store it)
    changed, stats = run()
    assert stats["graphed"] and dec.captures == 2, "other settings of the same objects did not capture again"
    for s in range(n):
        SC.assert_same(f"first run, stream {s}", first[s], want[s])
        SC.assert_same(f"replayed run, stream {s}", again[s], want[s])
    SC.assert_same("other settings, stream 0", changed[0], want[0])
    SC.assert_same("other settings, stream 1", changed[1], want_other)
    assert not torch.equal(want_other[0], want[1][0]), "the other setting changed nothing"
