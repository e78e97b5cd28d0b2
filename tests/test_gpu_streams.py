"""Decode streams on the device (harness/streams.py): every stream of generate_streams — fork and batch, bf16 and fp32, every cache
policy and the fused uint8 heavy-hitter cache — equals a lone generate() of that stream on a fresh model in its sequence, every
step's probability row or scores and every cache buffer of every layer, bit for bit.  A counter on glue.gemv_fused_multi shows that
the joint route ran with T = n (4 * n_layer + 1 calls per step); the captured joint step gives what eager joint steps give and is
replayed, not re-run; a cache quantising in reference mode takes the one-at-a-time route and still equals its lone runs."""
import functools

import pytest
import torch

import streams_common as SC

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}
SEEDS = [11, 5, 7, 3]


def _build(dt, strategy, extra=()):
    return lambda: SC.tiny(DTYPES[dt], strategy, DEV, **dict(extra))


@functools.lru_cache(maxsize=None)
def _lone(dt, strategy, extra, seed, mode):
    gk = dict(SC.SAMPLED, logprobs=(mode == "logprobs"))
    return SC.lone(_build(dt, strategy, extra), SC.prompt(40, DEV), seed, **gk)


def _counted(fn):
    """fn() with glue.gemv_fused_multi and Transformer.forward_streams counted -> (result, [T per multi call], eager joint steps)"""
    from cold_compress_amd.harness import Transformer, glue

    multi, joint = [], []
    real, real_fs = glue.gemv_fused_multi, Transformer.forward_streams

    def counted(*a, **k):
        multi.append(a[1].shape[0])
        return real(*a, **k)

    def counted_fs(self, *a, **k):
        joint.append(1)
        return real_fs(self, *a, **k)

    glue.gemv_fused_multi, Transformer.forward_streams = counted, counted_fs
    try:
        out = fn()
    finally:
        glue.gemv_fused_multi, Transformer.forward_streams = real, real_fs
    return out, multi, len(joint)


@pytest.mark.parametrize("mode", ["sampled", "logprobs"])
@pytest.mark.parametrize("n", [2, 3, 4])
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("strategy,extra", SC.POLICIES, ids=SC.POLICY_IDS)
def test_fork_streams_equal_their_lone_runs(strategy, extra, dt, n, mode):
    ex = tuple(sorted(extra.items()))
    gk = dict(SC.SAMPLED, logprobs=(mode == "logprobs"))
    (_, _, got, stats), multi, _ = _counted(lambda: SC.run_streams(_build(dt, strategy, ex), SC.prompt(40, DEV), n=n, seeds=SEEDS[:n], **gk))
    assert stats["joint_steps"] and stats["graphed"] and set(multi) == {n}, (stats, multi)
    for s in range(n):
        SC.assert_same(f"{strategy} {dt} n={n} {mode} stream {s}", got[s], _lone(dt, strategy, ex, SEEDS[s], mode))
    assert len({tuple(g[0].tolist()) for g in got}) > 1


@pytest.mark.parametrize("dt", list(DTYPES))
def test_batch_streams_equal_their_lone_runs_and_take_the_joint_route(dt):
    """three prompts of lengths 12, 25 and 31, greedy, eager joint steps: 4 * n_layer + 1 multi GEMVs of T = 3 per step"""
    prompts = [SC.prompt(L, DEV, seed=20 + L) for L in (12, 25, 31)]
    (_, _, got, stats), multi, joint = _counted(lambda: SC.run_streams(_build(dt, "heavy_hitter"), prompts, graph=False))
    steps = SC.NEW_TOKENS - 1
    assert joint == steps and multi == [3] * (steps * (4 * SC.TINY["n_layer"] + 1)), (joint, multi)
    for s, p in enumerate(prompts):
        SC.assert_same(f"batch {dt} stream {s}", got[s], SC.lone(_build(dt, "heavy_hitter"), p, s))


@pytest.mark.parametrize("strategy", ["heavy_hitter", "random", "hybrid"])
def test_the_captured_joint_step_is_replayed_and_equals_eager_joint_steps(strategy):
    build = _build("bf16", strategy)
    (_, _, eager, se), _, joint_e = _counted(lambda: SC.run_streams(build, SC.prompt(40, DEV), n=4, seeds=SEEDS, graph=False, **SC.SAMPLED))
    (_, _, graphed, sg), _, joint_g = _counted(lambda: SC.run_streams(build, SC.prompt(40, DEV), n=4, seeds=SEEDS, graph=True, **SC.SAMPLED))
    assert not se["graphed"] and sg["graphed"]
    assert joint_e == SC.NEW_TOKENS - 1
    assert joint_g == 3, f"{joint_g} eager joint steps in the graphed run (two warm-up steps and the captured one)"
    for s in range(4):
        SC.assert_same(f"{strategy} graph vs eager stream {s}", graphed[s], eager[s])


def test_a_reference_mode_quantised_cache_runs_one_stream_at_a_time():
    build = lambda: SC.tiny(torch.bfloat16, "heavy_hitter", DEV, cache_bits=8)  # noqa: E731
    (model, streams, got, stats), multi, joint = _counted(lambda: SC.run_streams(build, SC.prompt(40, DEV), n=3, seeds=SEEDS[:3], **SC.SAMPLED))
    assert not model.streams_eligible(streams) and not stats["joint_steps"] and not multi and joint == 0
    for s in range(3):
        SC.assert_same(f"cache_bits 8 stream {s}", got[s], SC.lone(build, SC.prompt(40, DEV), SEEDS[s], **SC.SAMPLED))


def test_the_fused_uint8_heavy_hitter_cache_is_served():
    """the fused quantised modes serve 16-bit models at head_dim 128 with a multiple of 4 query heads per kv head: a two-layer model
    of that shape with random weights (tests/test_gpu_forced_block.py's)"""
    from cold_compress_amd.harness import ModelArgs, Transformer

    def build():
        torch.manual_seed(5)
        cfg = dict(block_size=512, vocab_size=256, n_layer=2, n_head=8, n_local_heads=2, dim=1024, intermediate_size=512)
        model = SC.caches(Transformer(ModelArgs(**cfg)).to(torch.bfloat16).eval().to(DEV), "heavy_hitter", DEV, 64, cache_bits=8,
                          cache_quant_mode="fused")
        assert all(l.attention.kv_cache.fused_quant for l in model.layers)
        return model

    (model, streams, got, stats), multi, _ = _counted(lambda: SC.run_streams(build, SC.prompt(40, DEV), n=3, seeds=SEEDS[:3], **SC.SAMPLED))
    assert model.streams_eligible(streams) and stats["graphed"] and set(multi) == {3}
    for s in range(3):
        SC.assert_same(f"fused uint8 stream {s}", got[s], SC.lone(build, SC.prompt(40, DEV), SEEDS[s], **SC.SAMPLED))


def test_more_streams_than_the_multi_gemv_takes_are_refused():
    from cold_compress_amd.harness import DecodeStreams, glue

    model = SC.tiny(torch.bfloat16, "heavy_hitter", DEV)
    assert glue.GEMV_MULTI_MAX_T == 4
    with pytest.raises(ValueError):
        DecodeStreams(model, 5)
    assert DecodeStreams(model, 4).n == 4
