"""`forced_block` and `generate_streams` on the device for int4 group-wise weight-only models (Transformer.block_int4 = True): every
multi product runs through glue.gemv_fused_w4_multi (cc_gemv_fused_w4_multi, one pass over the codes for up to four rows) and must
leave EXACTLY what the token-by-token route leaves — sequences, every step's probability row bit for bit, every cache buffer of every
layer bit for bit.  The `tiny` model of tests/streams_common.py (2 layers, dim 64, the fixture's weights) converted by the int4
handler at G = 32, bf16, a 40-token prompt over a cache of 32 so that every step evicts.  A counter on glue.gemv_fused_w4_multi tells
the routes apart; with the attribute left at its default the same model makes no multi call and gives the same results."""
import functools

import pytest
import torch

import streams_common as SC

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
G = 32
SEEDS = [11, 5, 7, 3]
LENGTHS = (12, 25, 31, 18)
NEXT = torch.tensor([9, 21, 6, 33, 47, 5, 60, 72, 7, 85, 99, 110, 14, 27], dtype=torch.int32)  # the prefill's token + 13 forced steps
PER_STEP = 4 * SC.TINY["n_layer"] + 1  # wqkv, wo, w1/w3, w2 per layer + the LM head


@functools.lru_cache(maxsize=None)
def _quantised():
    """the fixture's weights quantised once by the int4 handler -> its state dict on the device (never modified)."""
    from cold_compress_amd.harness import ModelArgs, Transformer
    from cold_compress_amd.harness.quantize import WeightOnlyInt4QuantHandler

    dense = Transformer(ModelArgs(**SC.TINY)).to(torch.float32).eval()
    dense.load_state_dict(SC.weights(), strict=True)
    return WeightOnlyInt4QuantHandler(dense.to(BF).to(DEV), groupsize=G).create_quantized_state_dict()


def _model(strategy="heavy_hitter", block_int4=True, **extra):
    from cold_compress_amd.harness import ModelArgs, Transformer
    from cold_compress_amd.harness.quantize import WeightOnlyInt4QuantHandler, is_int4_linear

    with torch.device("meta"):
        model = WeightOnlyInt4QuantHandler(Transformer(ModelArgs(**SC.TINY)), groupsize=G).convert_for_runtime()
    model.load_state_dict({k: v.clone() for k, v in _quantised().items()}, assign=True)
    model = SC.caches(model.to(device=DEV, dtype=BF).eval(), strategy, DEV, **extra)
    assert is_int4_linear(model.output) and model.output.groupsize == G
    assert not model.block_eligible(), "int4 models are opt-in"
    model.block_weight_only = True
    assert not model.block_eligible(), "block_weight_only does not cover int4"
    model.block_weight_only = False
    model.block_int4 = block_int4
    assert model.block_eligible() == block_int4
    return model


def _counted(fn):
    """fn() with both multi glue functions counted -> (result, [T per int4 multi call], [T per other multi call])"""
    from cold_compress_amd.harness import glue

    w4, other = [], []
    real4, real = glue.gemv_fused_w4_multi, glue.gemv_fused_multi

    def counted4(*a, **k):
        w4.append(a[1].shape[0])
        return real4(*a, **k)

    def counted(*a, **k):
        other.append(a[1].shape[0])
        return real(*a, **k)

    glue.gemv_fused_w4_multi, glue.gemv_fused_multi = counted4, counted
    try:
        out = fn()
    finally:
        glue.gemv_fused_w4_multi, glue.gemv_fused_multi = real4, real
    return out, w4, other


# ------------------------------------------------------------------------------------------------ forced blocks
def _forced(model, forced_block, prompt, new_tokens=0, **gk):
    from cold_compress_amd.harness import decode_one_token, generate, prefill

    torch.manual_seed(1234)
    (seq, probs, _), w4, other = _counted(lambda: generate(model, prompt, prefill, decode_one_token, max_new_tokens=new_tokens,
                                                           forced_block=forced_block, **gk))
    torch.cuda.synchronize()
    assert not other, "an int4 model reached gemv_fused_multi"
    return (seq.cpu(), [p.cpu() for p in probs], SC.state_of([l.attention.kv_cache for l in model.layers])), w4


@pytest.mark.parametrize("strategy", ["heavy_hitter", "recent_global"])
def test_teacher_forced_blocks_equal_single_steps(strategy):
    """13 forced decode steps: three blocks of four and a tail of one."""
    r4, c4 = _forced(_model(strategy), 4, SC.prompt(40, DEV), next_tokens=NEXT.to(DEV))
    r1, c1 = _forced(_model(strategy), 1, SC.prompt(40, DEV), next_tokens=NEXT.to(DEV))
    assert not c1, "forced_block=1 reached the multi kernel"
    assert c4 == [4] * (3 * PER_STEP), c4
    assert r4[0][40:].tolist() == NEXT.tolist() and len(r4[1]) == 14
    SC.assert_same(f"int4 {strategy} blocks of four vs single steps", r4, r1)


def test_long_prompt_fed_in_blocks_then_free_tokens():
    """feed_long_prompts: 11 tokens beyond the cache (blocks of 4, 4, 4), then 6 free greedy tokens through the single step."""
    r4, c4 = _forced(_model(), 4, SC.prompt(32 + 11, DEV), new_tokens=6, feed_long_prompts=True)
    r1, c1 = _forced(_model(), 1, SC.prompt(32 + 11, DEV), new_tokens=6, feed_long_prompts=True)
    assert not c1 and c4 == [4] * (3 * PER_STEP), (c1, c4)
    assert len(r4[0]) == 43 + 6 and len(r4[1]) == 12 + 6
    SC.assert_same("int4 feed_long_prompts", r4, r1)


def test_without_the_attribute_blocks_take_the_per_token_route():
    r4, c4 = _forced(_model(block_int4=False), 4, SC.prompt(40, DEV), next_tokens=NEXT.to(DEV))
    r1, _ = _forced(_model(block_int4=True), 4, SC.prompt(40, DEV), next_tokens=NEXT.to(DEV))
    assert not c4
    SC.assert_same("int4 with block_int4 off vs on", r4, r1)


# ------------------------------------------------------------------------------------------------ streams
@functools.lru_cache(maxsize=None)
def _lone(length, pseed, seed, sampled, strategy="heavy_hitter"):
    """a stream's lone generate() on a fresh model, on the per-token route (block_int4 off: the parent's route for these models)"""
    gk = dict(SC.SAMPLED) if sampled else {}
    return SC.lone(lambda: _model(strategy, block_int4=False), SC.prompt(length, DEV, seed=pseed), seed, **gk)


def _streams(n, kind, sampled, graph, block_int4=True, strategy="heavy_hitter"):
    """-> ([(got, lone) per stream], stats, int4 multi calls)"""
    gk = dict(SC.SAMPLED) if sampled else {}
    seeds = SEEDS[:n]
    if kind == "fork":
        prompts, kw = SC.prompt(40, DEV), dict(n=n)
        lone = [_lone(40, 3, s, sampled, strategy) for s in seeds]
    else:
        prompts, kw = [SC.prompt(L, DEV, seed=20 + L) for L in LENGTHS[:n]], {}
        lone = [_lone(L, 20 + L, s, sampled, strategy) for L, s in zip(LENGTHS[:n], seeds)]
    (_, _, got, stats), w4, other = _counted(lambda: SC.run_streams(lambda: _model(strategy, block_int4=block_int4), prompts, seeds=seeds,
                                                                    graph=graph, **kw, **gk))
    assert not other, "an int4 model reached gemv_fused_multi"
    return list(zip(got, lone)), stats, w4


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
@pytest.mark.parametrize("kind", ["fork", "batch"])
@pytest.mark.parametrize("n", [2, 3, 4])
def test_streams_equal_their_lone_runs_on_the_joint_route(n, kind, sampled, graph):
    pairs, stats, w4 = _streams(n, kind, sampled, graph)
    assert stats["joint_steps"] is True or stats["joint_steps"] == 1, stats
    assert bool(stats["graphed"]) == graph and w4 and set(w4) == {n}, (stats, w4)
    if not graph:
        assert w4 == [n] * ((SC.NEW_TOKENS - 1) * PER_STEP), w4
    for s, (got, lone) in enumerate(pairs):
        SC.assert_same(f"int4 {kind} n={n} {'sampled' if sampled else 'greedy'} {'graph' if graph else 'eager'} stream {s}", got, lone)
    if sampled and kind == "fork":
        assert len({tuple(g[0].tolist()) for g, _ in pairs}) > 1, "the seeds gave one continuation"


def test_streams_of_another_policy_equal_their_lone_runs():
    pairs, stats, w4 = _streams(4, "fork", True, True, strategy="recent_global")
    assert stats["joint_steps"] and stats["graphed"] and set(w4) == {4}
    for s, (got, lone) in enumerate(pairs):
        SC.assert_same(f"int4 recent_global stream {s}", got, lone)


@pytest.mark.parametrize("kind", ["fork", "batch"])
def test_without_the_attribute_streams_run_one_at_a_time_with_the_same_results(kind):
    pairs, stats, w4 = _streams(3, kind, True, True, block_int4=False)
    assert not stats["joint_steps"] and not w4, (stats, w4)
    for s, (got, lone) in enumerate(pairs):
        SC.assert_same(f"int4 {kind} with block_int4 off, stream {s}", got, lone)
