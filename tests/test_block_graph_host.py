"""`block_decoder=` without a GPU (tests/cpu_twin.py): on CPU tensors GraphedBlockDecoder has no graph and passes every block through
to the eager Transformer.forward_block twin and the shared per-block tail — so a run with it equals the run without it, bit for bit;
a decoder built for another model is refused before anything runs; and the default call launches exactly what it launched before."""
import pytest
import torch

import streams_common as SC
from cpu_twin import cpu_twin

DEV, DT = "cpu", torch.float32
NEXT = torch.tensor([9, 21, 6, 33, 47, 5, 60, 72, 7, 85, 99, 110, 14, 27], dtype=torch.int32)  # the prefill's token + 13 forced steps


@pytest.fixture()
def twin(monkeypatch, oracle):
    with cpu_twin(monkeypatch, oracle) as fns:
        yield fns


def _run(strategy, prompt, with_decoder, forced_block=4, new_tokens=0, **gk):
    """-> ((sequence, probabilities or scores, cache state), T of every forward_block call, the decoder or None)"""
    from cold_compress_amd.harness import GraphedBlockDecoder, decode_one_token, generate

    model = SC.tiny(DT, strategy, DEV)
    SC.fix_rng_seeds([[l.attention.kv_cache for l in model.layers]])
    calls, real = [], model.forward_block

    def counted(idx, input_pos, **k2):
        calls.append(int(idx.shape[1]))
        return real(idx, input_pos, **k2)

    model.forward_block = counted
    dec = GraphedBlockDecoder(model) if with_decoder else None
    extra = {} if forced_block is None else {"forced_block": forced_block}
    if with_decoder:
        extra["block_decoder"] = dec
    seq, probs, _ = generate(model, prompt, SC.prefill_fn(), decode_one_token, max_new_tokens=new_tokens, **gk, **extra)
    return (seq, SC.cpu(probs), SC.state_of([l.attention.kv_cache for l in model.layers])), calls, dec


FORCED, TOP3 = dict(next_tokens=NEXT), dict(next_tokens=NEXT, logprobs=True, top_logprobs=3)
FEED = dict(new_tokens=6, feed_long_prompts=True, temperature=0.8, top_k=5, seed=7)  # (a cache of 32: hybrid's holds the whole 64)


@pytest.mark.parametrize("strategy,gk", [("heavy_hitter", FORCED), ("heavy_hitter", FEED), ("heavy_hitter", TOP3), ("hybrid", FORCED), ("hybrid", TOP3)],
                         ids=["heavy_hitter-forced", "heavy_hitter-feed_long-sampled", "heavy_hitter-top3", "hybrid-forced", "hybrid-top3"])
def test_block_decoder_on_cpu_tensors_equals_the_run_without_it(twin, strategy, gk):
    prompt = SC.prompt(43 if "feed_long_prompts" in gk else 40, DEV)
    with_dec, calls_dec, dec = _run(strategy, prompt, True, **gk)
    without, calls, _ = _run(strategy, prompt, False, **gk)
    single, calls_1, _ = _run(strategy, prompt, False, forced_block=1, **gk)
    SC.assert_same(f"{strategy}: with the decoder vs without", with_dec, without)
    SC.assert_same(f"{strategy}: with the decoder vs single steps", with_dec, single)
    assert calls_dec == calls == [4, 4, 4] and not calls_1
    assert dec.captures == 0 and dec.replays == 0 and dec.keys() == set(), "a graph on CPU tensors"


def test_a_decoder_built_for_another_model_is_refused_before_anything_runs(twin):
    from cold_compress_amd.harness import GraphedBlockDecoder, decode_n_tokens, decode_one_token, generate

    model, other = SC.tiny(DT, "heavy_hitter", DEV), SC.tiny(DT, "heavy_hitter", DEV)
    ran = []
    model.register_forward_hook(lambda *a: ran.append(1))
    dec = GraphedBlockDecoder(other)
    with pytest.raises(ValueError, match="another model"):
        generate(model, SC.prompt(40, DEV), SC.prefill_fn(), decode_one_token, max_new_tokens=0, next_tokens=NEXT, forced_block=4, block_decoder=dec)
    with pytest.raises(ValueError, match="another model"):
        decode_n_tokens(model, torch.tensor([[9]], dtype=torch.int32), torch.tensor([40], dtype=torch.int32), decode_one_token, 13, prefix=NEXT[1:],
                        forced_block=4, block_decoder=dec)
    assert not ran


def test_the_default_call_launches_what_it_launched(twin):
    """no keyword: no block and no decoder; forced_block alone: the eager blocks; block_decoder without forced_block > 1: no block."""
    prompt = SC.prompt(40, DEV)
    base, calls_default, _ = _run("heavy_hitter", prompt, False, forced_block=None, next_tokens=NEXT)
    _, calls_blocks, _ = _run("heavy_hitter", prompt, False, next_tokens=NEXT)
    got, calls_dec_only, dec = _run("heavy_hitter", prompt, True, forced_block=None, next_tokens=NEXT)
    assert calls_default == [] and calls_blocks == [4, 4, 4] and calls_dec_only == []
    SC.assert_same("block_decoder without forced_block", got, base)
    assert dec.replays == 0 and dec.captures == 0
