"""`forced_block` on the device for weight-only int8 and MXFP4 models (Transformer.block_weight_only = True): blocks of up to four
known tokens run through Transformer.forward_block with every weight matrix streamed once per block (cc_gemv_fused_w8_multi /
cc_gemv_fused_mx4_multi) and must leave EXACTLY what the token-by-token loop leaves — the sequence, every step's probabilities bit
for bit, every cache buffer of every layer bit for bit.  tests/test_gpu_forced_block.py's scheme, on the same `tiny` model and
fixture weights, converted by the int8 handler (bf16 and f16) and by the MXFP4 handler (bf16); a counter on glue.gemv_fused_multi
tells the routes apart.  With the attribute left at its default the same int8 model makes no multi call."""
import argparse
import functools

import pytest
import torch

from helpers import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
TINY = dict(block_size=256, vocab_size=128, n_layer=2, n_head=4, n_local_heads=2, dim=64, intermediate_size=128)
MODELS = [("int8", torch.bfloat16), ("int8", torch.float16), ("mxfp4", torch.bfloat16)]
IDS = ["int8-bf16", "int8-f16", "mxfp4-bf16"]


class Tok:
    def special_ids(self):
        return [[1], [2, 3]]

    def punctuation_ids(self):
        return [5, 6, 7]


@functools.lru_cache(maxsize=None)
def _weights():
    f = load_golden("f1_e2e_heavy_hitter.npz")
    assert int(f["n_layer"]) == TINY["n_layer"]
    return {k[3:]: v for k, v in f.items() if k.startswith("sd.")}


@functools.lru_cache(maxsize=None)
def _quantised(mode, dtype):
    """the fixture's weights quantised once per (mode, dtype) by the handler -> its state dict on the device (never modified)."""
    from cold_compress_amd.harness import ModelArgs, Transformer
    from cold_compress_amd.harness.quantize import WeightOnlyInt8QuantHandler, WeightOnlyMxfp4QuantHandler

    dense = Transformer(ModelArgs(**TINY)).to(torch.float32).eval()
    dense.load_state_dict(_weights(), strict=True)
    handler = {"int8": WeightOnlyInt8QuantHandler, "mxfp4": WeightOnlyMxfp4QuantHandler}[mode]
    return handler(dense.to(dtype).to(DEV)).create_quantized_state_dict()


def _model(mode, dtype, strategy, weight_only=True, max_seq=64, **extra):
    import cold_compress_amd.cache as cache
    from cold_compress_amd.harness import ModelArgs, Transformer, setup_caches
    from cold_compress_amd.harness.quantize import WeightOnlyInt8QuantHandler, WeightOnlyMxfp4QuantHandler

    handler = {"int8": WeightOnlyInt8QuantHandler, "mxfp4": WeightOnlyMxfp4QuantHandler}[mode]
    with torch.device("meta"):
        model = handler(Transformer(ModelArgs(**TINY))).convert_for_runtime()
    model.load_state_dict({k: v.clone() for k, v in _quantised(mode, dtype).items()}, assign=True)
    model = model.to(device=DEV, dtype=dtype).eval()
    ap = argparse.ArgumentParser()
    cache.add_cache_arguments(ap)
    kw = vars(ap.parse_args([]))
    whole = strategy == "full"
    kw.update(dict(cache_strategy=[strategy], prompt_compression_strategy=["full" if whole else strategy],
                   max_cache_length=[1.0 if whole else 32.0], global_tokens=4, recent_window=8))
    kw.update(extra)
    setup_caches(model, Tok(), DEV, max_seq, dict(kw))
    assert not model.block_eligible(), "weight-only models are opt-in"
    model.block_weight_only = weight_only
    assert model.block_eligible() == weight_only
    return model


def _prompt(n, seed=3):
    g = torch.Generator().manual_seed(seed)
    p = torch.randint(8, 128, (n,), generator=g, dtype=torch.int32)
    p[::9] = 6
    return p.to(DEV)


def _generate(model, forced_block, prompt, new_tokens=0, counter=None, **gk):
    """one generation -> (sequence, probabilities, {layer.buffer: tensor}) on the CPU; `counter`: gemv_fused_multi calls."""
    from cold_compress_amd.harness import decode_one_token, generate, glue, prefill

    torch.manual_seed(1234)
    real = glue.gemv_fused_multi

    def counted(*a, **k):
        if counter is not None:
            counter.append(a[1].shape[0])
        return real(*a, **k)

    glue.gemv_fused_multi = counted
    try:
        seq, probs, _ = generate(model, prompt, prefill, decode_one_token, max_new_tokens=new_tokens, forced_block=forced_block, **gk)
    finally:
        glue.gemv_fused_multi = real
    torch.cuda.synchronize()
    state = {f"{li}.{n}": b.detach().cpu().clone() for li, layer in enumerate(model.layers)
             for n, b in layer.attention.kv_cache._buffers.items() if b is not None}
    return seq.cpu(), [p.cpu() for p in probs], state


def _bits(t):
    return t.contiguous().view(torch.int16) if t.dtype in (torch.bfloat16, torch.float16) else t


def _assert_same(what, a, b):
    (seq_a, probs_a, st_a), (seq_b, probs_b, st_b) = a, b
    assert torch.equal(seq_a, seq_b), f"{what}: sequence {seq_a.tolist()} vs {seq_b.tolist()}"
    assert len(probs_a) == len(probs_b)
    for i, (pa, pb) in enumerate(zip(probs_a, probs_b)):
        assert torch.equal(_bits(pa), _bits(pb)), f"{what}: probabilities of step {i} differ (max {float((pa.float() - pb.float()).abs().max())})"
    assert st_a.keys() == st_b.keys() and st_a
    for n in st_a:
        assert torch.equal(_bits(st_a[n]), _bits(st_b[n])), f"{what}: cache buffer {n}"


def _pair(build, prompt, what, expect_blocks=True, **gk):
    """the same generation with forced_block 4 and 1 on two fresh models -> the block run's result and its multi calls."""
    c4, c1 = [], []
    r4 = _generate(build(), 4, prompt, counter=c4, **gk)
    r1 = _generate(build(), 1, prompt, counter=c1, **gk)
    assert not c1, f"{what}: forced_block=1 reached the multi kernels"
    assert bool(c4) == expect_blocks, f"{what}: gemv_fused_multi calls {c4}"
    _assert_same(what, r4, r1)
    return r4, c4


NEXT = torch.tensor([9, 21, 6, 33, 47, 5, 60, 72, 7, 85, 99, 110, 14, 27], dtype=torch.int32)  # the prefill's token + 13 forced steps


@pytest.mark.parametrize("strategy", ["heavy_hitter", "recent_global"])
@pytest.mark.parametrize("mode,dtype", MODELS, ids=IDS)
def test_teacher_forced_blocks_equal_single_steps(mode, dtype, strategy):
    """13 forced decode steps: three blocks of four and a tail of one."""
    (seq, probs, _), calls = _pair(lambda: _model(mode, dtype, strategy), _prompt(40), f"{mode} {dtype} {strategy}", next_tokens=NEXT.to(DEV))
    assert seq[40:].tolist() == NEXT.tolist() and len(probs) == 14
    # per block: wqkv, wo, w1/w3, w2 in each of the two layers + the LM head; three blocks of four tokens
    assert calls == [4] * (3 * (4 * TINY["n_layer"] + 1)), calls


@pytest.mark.parametrize("mode,dtype", MODELS, ids=IDS)
def test_long_prompt_fed_in_blocks_then_free_tokens(mode, dtype):
    """feed_long_prompts: 11 tokens beyond the cache (12 known inputs with the split's own: blocks of 4, 4, 4 whose last step is the
    first free one), then 6 free greedy tokens through the single step."""
    (seq, probs, _), calls = _pair(lambda: _model(mode, dtype, "heavy_hitter"), _prompt(32 + 11), f"feed_long {mode} {dtype}", new_tokens=6,
                                   feed_long_prompts=True)
    assert len(seq) == 43 + 6 and len(probs) == 12 + 6
    assert set(calls) == {4} and len(calls) == 3 * (4 * TINY["n_layer"] + 1), calls


def test_int8_model_without_the_attribute_makes_no_multi_call():
    _pair(lambda: _model("int8", torch.bfloat16, "heavy_hitter", weight_only=False), _prompt(40), "int8, block_weight_only left off",
          expect_blocks=False, next_tokens=NEXT.to(DEV))
