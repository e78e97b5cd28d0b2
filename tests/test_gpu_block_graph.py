"""`block_decoder=GraphedBlockDecoder(model)` on the device: the forced blocks of `forced_block` replayed from captured hipGraphs
(Transformer.forward_block and the whole per-block tail, one graph per (T, last step free)) must leave EXACTLY what the eager blocks
and the token-by-token loop leave — the sequence, every step's probability row or scores bit for bit, every cache buffer of every
layer bit for bit.  Every case is three runs on fresh models: forced_block=4 with the decoder, eager forced_block=4, forced_block=1.
The `tiny` model and helpers of tests/test_gpu_forced_block.py; the decoder's counters (`captures`, `replays`, `keys()`) tell a
replayed block from a passed-through one."""
import pytest
import torch

import test_gpu_forced_block as FB

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
NEXT = FB.NEXT
SAMPLED = dict(temperature=0.8, top_k=5, top_p=0.9, seed=7)
FEED = dict(new_tokens=6, feed_long_prompts=True)  # with a 32 + 11 token prompt: blocks (4, forced), (4, forced), (4, last free)

_REFS = {}  # eager blocks' and single steps' results shared between tests, by key; never modified


def _refs(key, build, prompt, forced_block, gk):
    """(eager blocks' result, single steps' result) on fresh models; `gk`: a factory of generate()'s keywords (fresh state objects)."""
    if key is None or key not in _REFS:
        r = (FB._generate(build(), forced_block, prompt, **gk()), FB._generate(build(), 1, prompt, **gk()))
        if key is None:
            return r
        _REFS[key] = r
    return _REFS[key]


def _triple(build, prompt, what, gk=None, forced_block=4, key=None, log=None):
    """-> (the decoder, the captured run's result, its model): asserts captured == eager blocks == single steps"""
    from cold_compress_amd.harness import GraphedBlockDecoder

    gk = (lambda: {}) if gk is None else gk
    model = build()
    dec = GraphedBlockDecoder(model, log=log)
    got = FB._generate(model, forced_block, prompt, block_decoder=dec, **gk())
    eager, single = _refs(key, build, prompt, forced_block, gk)
    FB._assert_same(f"{what}: captured blocks vs eager blocks", got, eager)
    FB._assert_same(f"{what}: captured blocks vs single steps", got, single)
    return dec, got, model


def _forced(n=14):
    return lambda: dict(next_tokens=NEXT[:n].to(DEV))


# ------------------------------------------------------------------------------------------------ 1. every policy
@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("strategy,extra", FB.POLICIES, ids=[s + ("-w8" if e else "") for s, e in FB.POLICIES])
def test_teacher_forced_blocks_replay_and_equal(strategy, extra, dtype):
    """13 forced decode steps: three replays of ONE graph of four forced rows, and a tail of one single step."""
    dec, (seq, probs, _), _ = _triple(lambda: FB._tiny(dtype, strategy, **extra), FB._prompt(40), f"{strategy} {dtype}", _forced(),
                                      key=("forced", strategy, bool(extra), dtype))
    assert seq[40:].tolist() == NEXT.tolist() and len(probs) == 14
    assert dec.replays == 3 and dec.keys() == {(4, False)} and dec.captures == 1, (dec.replays, dec.keys(), dec.captures)


# ------------------------------------------------------------------------------------------------ 2. feed_long_prompts
@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
def test_long_prompt_fed_in_captured_blocks_then_free_tokens(dtype, sampled):
    """a 32 + 11 token prompt, 6 free tokens: the third block's last step is the first free one — its token comes from the graph."""
    gk = dict(FEED, **(SAMPLED if sampled else {}))
    dec, (seq, probs, _), _ = _triple(lambda: FB._tiny(dtype, "heavy_hitter"), FB._prompt(32 + 11), f"feed_long {dtype} {gk}", lambda: dict(gk),
                                      key=("feed", dtype, sampled))
    assert len(seq) == 43 + 6 and len(probs) == 12 + 6
    assert dec.keys() == {(4, False), (4, True)} and dec.captures == 2 and dec.replays == 3, (dec.keys(), dec.captures, dec.replays)


# ------------------------------------------------------------------------------------------------ 3. partial blocks
@pytest.mark.parametrize("steps,forced_block,keys,replays", [(7, 4, {(4, False), (3, False)}, 2), (6, 4, {(4, False), (2, False)}, 2),
                                                             (13, 3, {(3, False)}, 4), (13, 2, {(2, False)}, 6)],
                         ids=["4+3", "4+2", "threes", "twos"])
def test_partial_blocks(steps, forced_block, keys, replays):
    dec, (seq, _, _), _ = _triple(lambda: FB._tiny(BF, "heavy_hitter"), FB._prompt(40), f"{steps} steps in blocks of {forced_block}",
                                  _forced(steps + 1), forced_block=forced_block)
    assert seq[40:].tolist() == NEXT[:steps + 1].tolist()
    assert dec.keys() == keys and dec.captures == len(keys) and dec.replays == replays, (dec.keys(), dec.captures, dec.replays)


# ------------------------------------------------------------------------------------------------ 4. scores
@pytest.mark.parametrize("free_last", [False, True], ids=["all-forced", "free-last-row"])
@pytest.mark.parametrize("top", [None, 3], ids=["logprobs", "top3"])
def test_scores_from_captured_blocks(top, free_last):
    """TokenScores / TokenTopScores of one cc_logprob_rows / cc_logprob_topn call per block, captured; a free last row's token is
    drawn inside the graph and scored through `fallback`."""
    gk = dict(logprobs=True, top_logprobs=top)
    if free_last:
        gk.update(FEED, **SAMPLED)
        prompt = FB._prompt(32 + 11)
    else:
        gk.update(next_tokens=NEXT.to(DEV))
        prompt = FB._prompt(40)
    dec, (_, scores, _), _ = _triple(lambda: FB._tiny(BF, "heavy_hitter"), prompt, f"scores top={top} free={free_last}", lambda: dict(gk))
    assert len(scores) == (2 if top is None else 4) and scores[0].dtype == torch.float32 and bool(torch.isfinite(scores[0]).all())
    if top is not None:
        assert scores[2].shape[1] == 3
    assert dec.replays == 3 and ((4, True) in dec.keys()) == free_last


# ------------------------------------------------------------------------------------------------ 5. penalties and constraints
@pytest.mark.parametrize("free_last", [False, True], ids=["all-forced", "free-last-row"])
def test_penalties_and_constraints_state_is_put_back(free_last):
    from cold_compress_amd.harness import LogitConstraints, LogitPenalties

    made = []

    def gk():
        pen = LogitPenalties(128, DEV, 1.2, 0.1, 0.1)
        con = LogitConstraints(128, DEV, 64, no_repeat_ngram_size=2)
        made.append((pen, con))
        extra = dict(FEED) if free_last else dict(next_tokens=NEXT.to(DEV))
        return dict(penalties=pen, constraints=con, **extra)

    dec, (seq, _, _), _ = _triple(lambda: FB._tiny(BF, "heavy_hitter"), FB._prompt(32 + 11 if free_last else 40), f"penalties free={free_last}", gk)
    assert dec.replays == 3 and dec.captures == (2 if free_last else 1)
    torch.cuda.synchronize()
    (pen_g, con_g), (pen_e, con_e), (pen_1, con_1) = made
    n_inputs = len(seq) - 1  # positions 0 .. len - 2 were a step's input
    for what, pen, con in (("eager blocks", pen_e, con_e), ("single steps", pen_1, con_1)):
        for name in ("prompt_count", "gen_count", "gen_start"):
            assert torch.equal(getattr(pen_g, name), getattr(pen, name)), f"penalties.{name} differs from the {what}' (the capture's warm-up was counted?)"
        assert int(pen_g.prompt_count.sum() + pen_g.gen_count.sum()) == n_inputs
        assert torch.equal(con_g.hist[:n_inputs], con.hist[:n_inputs]) and torch.equal(con_g.gen_start, con.gen_start), f"constraints vs {what}"


# ------------------------------------------------------------------------------------------------ 6. one decoder, several generations
def test_one_decoder_serves_consecutive_generations():
    from cold_compress_amd.harness import GraphedBlockDecoder

    gk = dict(FEED, **SAMPLED)
    model = FB._tiny(BF, "heavy_hitter")
    dec = GraphedBlockDecoder(model)
    first = FB._generate(model, 4, FB._prompt(43), block_decoder=dec, **gk)
    FB._assert_same("first generation", first, FB._generate(FB._tiny(BF, "heavy_hitter"), 4, FB._prompt(43), **gk))
    assert dec.captures == 2 and dec.replays == 3
    model.reset_caches()
    second = FB._generate(model, 4, FB._prompt(43, seed=11), block_decoder=dec, **gk)
    FB._assert_same("second generation, another prompt", second, FB._generate(FB._tiny(BF, "heavy_hitter"), 4, FB._prompt(43, seed=11), **gk))
    assert dec.captures == 2 and dec.replays == 6, "the second generation captured again"
    assert not torch.equal(first[0], second[0])
    model.reset_caches()
    gk["seed"] = 9  # carried by value: capture again
    third = FB._generate(model, 4, FB._prompt(43, seed=11), block_decoder=dec, **gk)
    FB._assert_same("third generation, another seed", third, FB._generate(FB._tiny(BF, "heavy_hitter"), 4, FB._prompt(43, seed=11), **gk))
    assert dec.captures == 4 and dec.replays == 9 and dec.keys() == {(4, False), (4, True)}


def test_random_cache_captures_again_through_the_epoch():
    """KVCacheRandom draws a seed per generation that its steps carry by value: `_graph_epoch` moves and the graphs are dropped."""
    from cold_compress_amd.harness import GraphedBlockDecoder

    gk = dict(next_tokens=NEXT.to(DEV))
    model = FB._tiny(BF, "random")
    dec = GraphedBlockDecoder(model)
    first = FB._generate(model, 4, FB._prompt(40), block_decoder=dec, **gk)
    assert dec.captures == 1 and dec.replays == 3
    model.reset_caches()
    second = FB._generate(model, 4, FB._prompt(40, seed=11), block_decoder=dec, **gk)
    assert dec.captures == 2 and dec.replays == 6 and dec.keys() == {(4, False)}
    FB._assert_same("random, first generation", first, FB._generate(FB._tiny(BF, "random"), 1, FB._prompt(40), **gk))
    FB._assert_same("random, second generation", second, FB._generate(FB._tiny(BF, "random"), 1, FB._prompt(40, seed=11), **gk))


def test_rebuilt_caches_capture_again():
    from cold_compress_amd.harness import GraphedBlockDecoder

    gk = dict(next_tokens=NEXT.to(DEV))
    model = FB._tiny(BF, "heavy_hitter")
    dec = GraphedBlockDecoder(model)
    FB._generate(model, 4, FB._prompt(40), block_decoder=dec, **gk)
    FB._caches(model, "recent_global", 64)  # setup_caches again: other cache objects
    got = FB._generate(model, 4, FB._prompt(40), block_decoder=dec, **gk)
    assert dec.captures == 2 and dec.replays == 6
    FB._assert_same("rebuilt caches", got, FB._generate(FB._tiny(BF, "recent_global"), 1, FB._prompt(40), **gk))


# ------------------------------------------------------------------------------------------------ 7. weight-only models
@pytest.mark.parametrize("mode", ["int8", "mxfp4"])
def test_weight_only_models(mode):
    import test_gpu_forced_block_weight_only as WO

    dec, _, model = _triple(lambda: WO._model(mode, BF, "heavy_hitter"), FB._prompt(40), mode, _forced())
    assert model.block_weight_only and dec.replays == 3 and dec.captures == 1


def test_int4_model():
    import test_gpu_int4_blocks_streams as W4

    dec, _, model = _triple(lambda: W4._model("heavy_hitter"), FB._prompt(40), "int4 G=32", _forced())
    assert model.block_int4 and dec.replays == 3 and dec.captures == 1


# ------------------------------------------------------------------------------------------------ 8. the fused uint8 cache
def test_fused_uint8_heavy_hitter_cache():
    from cold_compress_amd.harness import ModelArgs, Transformer

    def build():
        torch.manual_seed(5)
        cfg = dict(block_size=512, vocab_size=256, n_layer=2, n_head=8, n_local_heads=2, dim=1024, intermediate_size=512)
        model = FB._caches(Transformer(ModelArgs(**cfg)).to(BF).eval().to(DEV), "heavy_hitter", 64, cache_bits=8, cache_quant_mode="fused")
        assert all(l.attention.kv_cache.fused_quant for l in model.layers) and model.block_eligible()
        return model

    dec, _, _ = _triple(build, FB._prompt(40), "fused uint8 heavy_hitter", _forced())
    assert dec.replays == 3 and dec.captures == 1


# ------------------------------------------------------------------------------------------------ 9. a refused capture
def test_refused_capture_falls_back_to_eager_blocks(monkeypatch):
    """torch.cuda.graph raising (a Python exception: nothing on the device fails) -> one log line, eager blocks, equal results and
    caches; the decoder captures in a later call."""
    lines = []

    def refuse(*a, **k):
        raise RuntimeError("capture refused (injected)")

    with monkeypatch.context() as mp:
        mp.setattr(torch.cuda, "graph", refuse)
        dec, _, model = _triple(lambda: FB._tiny(BF, "heavy_hitter"), FB._prompt(40), "refused capture", _forced(),
                                key=("forced", "heavy_hitter", False, BF), log=lines.append)
    assert len(lines) == 1 and "capture refused (injected)" in lines[0], lines
    assert dec.captures == 0 and dec.replays == 0 and dec.keys() == set()
    model.reset_caches()
    again = FB._generate(model, 4, FB._prompt(40), block_decoder=dec, next_tokens=NEXT.to(DEV))
    assert dec.captures == 1 and dec.replays == 3 and len(lines) == 1
    FB._assert_same("the call after a refused one", again, _REFS[("forced", "heavy_hitter", False, BF)][0])


# ------------------------------------------------------------------------------------------------ 10. an ineligible model
def test_ineligible_model_takes_the_per_token_route():
    def build():
        model = FB._tiny(BF, "heavy_hitter", cache_bits=8)  # reference-mode quantisation
        assert not model.block_eligible()
        return model

    dec, _, _ = _triple(build, FB._prompt(40), "cache_bits 8 (reference mode)", _forced())
    assert dec.captures == 0 and dec.replays == 0
