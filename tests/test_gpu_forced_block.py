"""`forced_block` on the device: decode steps whose input tokens are known run in blocks of up to four through
Transformer.forward_block (one pass over every weight matrix per block, cc_gemv_fused_multi; the layer's cache steps in order) and
must leave EXACTLY what the token-by-token loop leaves — the sequence, every step's probabilities bit for bit, every cache buffer
of every layer bit for bit — for every cache policy, in bf16 and fp32, greedy and seeded sampling, on the `tiny` model that
tests/test_gpu_e2e.py builds (its fixture's weights).  Models the block path does not serve (weight-only int8 weights, a cache
quantising in reference mode) take the per-token route and give the same results; a counter on glue.gemv_fused_multi tells the
routes apart."""
import argparse
import functools

import pytest
import torch

from helpers import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
TINY = dict(block_size=256, vocab_size=128, n_layer=2, n_head=4, n_local_heads=2, dim=64, intermediate_size=128)
HYB = [{"strategy": "special"}, {"strategy": "special_punc"}, {"strategy": "special_punc_heavy_hitter", "heavy_hitter_frac": 0.3},
       {"strategy": "special_punc_window", "recent_window": 0.3}, {"strategy": "full"}]


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


def _caches(model, strategy, max_seq, **extra):
    import cold_compress_amd.cache as cache
    from cold_compress_amd.harness import setup_caches

    ap = argparse.ArgumentParser()
    cache.add_cache_arguments(ap)
    kw = vars(ap.parse_args([]))
    whole = strategy in ("full", "hybrid")
    kw.update(dict(cache_strategy=[strategy], prompt_compression_strategy=["full" if whole else strategy if strategy != "random" else "recent_global"],
                   max_cache_length=[1.0 if whole else 32.0], global_tokens=4, recent_window=8))
    if strategy == "hybrid":
        kw.update(hybrid_strategies=HYB, min_recovery_frac=0.9)
    kw.update(extra)
    setup_caches(model, Tok(), DEV, max_seq, dict(kw))
    return model


def _tiny(dtype, strategy, max_seq=64, **extra):
    from cold_compress_amd.harness import ModelArgs, Transformer

    model = Transformer(ModelArgs(**TINY)).to(torch.float32).eval()
    model.load_state_dict(_weights(), strict=True)
    return _caches(model.to(dtype).to(DEV), strategy, max_seq, **extra)


def _prompt(n, seed=3):
    g = torch.Generator().manual_seed(seed)
    p = torch.randint(8, 128, (n,), generator=g, dtype=torch.int32)
    p[::9] = 6  # some punctuation for the hybrid policies
    return p.to(DEV)


def _generate(model, forced_block, prompt, new_tokens=0, counter=None, **gk):
    """one generation -> (sequence, probabilities, {layer.buffer: tensor}) on the CPU; `counter`: gemv_fused_multi calls."""
    from cold_compress_amd.harness import decode_one_token, generate, glue, prefill

    torch.manual_seed(1234)  # (KVCacheRandom draws its per-generation seed from torch's CPU generator)
    hybrid = type(model.layers[0].attention.kv_cache).__name__ == "KVCacheHybrid"

    def pf(m, x, input_pos, **k2):
        r = prefill(m, x, input_pos, **k2)
        if hybrid:  # the fixture's weights profile every head alike: force the reference's policy mix (tests/test_gpu_e2e.py does the same)
            for layer in m.layers:
                kv = layer.attention.kv_cache
                kv.cache_strategies = (torch.arange(kv.n_heads, device=DEV) % len(HYB)).to(torch.int64).contiguous()
                kv.requires_heavy_hitter = kv.requires_punc = kv.requires_special = True
        return r

    real = glue.gemv_fused_multi

    def counted(*a, **k):
        if counter is not None:
            counter.append(a[1].shape[0])
        return real(*a, **k)

    glue.gemv_fused_multi = counted
    try:
        extra = {} if forced_block is None else {"forced_block": forced_block}
        seq, probs, _ = generate(model, prompt, pf, decode_one_token, max_new_tokens=new_tokens, **gk, **extra)
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
    assert st_a.keys() == st_b.keys()
    for n in st_a:
        assert torch.equal(_bits(st_a[n]), _bits(st_b[n])), f"{what}: cache buffer {n}"


def _pair(build, prompt, what, expect_blocks=True, **gk):
    """the same generation with forced_block 4 and 1 on two fresh models -> both results; asserts equality and the route taken."""
    c4, c1 = [], []
    r4 = _generate(build(), 4, prompt, counter=c4, **gk)
    r1 = _generate(build(), 1, prompt, counter=c1, **gk)
    assert not c1, f"{what}: forced_block=1 reached the multi kernel"
    assert bool(c4) == expect_blocks, f"{what}: gemv_fused_multi calls {c4}"
    _assert_same(what, r4, r1)
    return r4, c4


NEXT = torch.tensor([9, 21, 6, 33, 47, 5, 60, 72, 7, 85, 99, 110, 14, 27], dtype=torch.int32)  # the prefill's token + 13 forced steps

POLICIES = [("full", {}), ("recent_global", {}), ("heavy_hitter", {}), ("l2", {}), ("random", {}), ("hybrid", {}),
            ("heavy_hitter", {"history_window_size": 8})]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("strategy,extra", POLICIES, ids=[s + ("-w8" if e else "") for s, e in POLICIES])
def test_teacher_forced_blocks_equal_single_steps(strategy, extra, dtype):
    """13 forced decode steps: three blocks of four and a tail of one."""
    (seq, probs, _), calls = _pair(lambda: _tiny(dtype, strategy, **extra), _prompt(40), f"{strategy} {dtype}", next_tokens=NEXT.to(DEV))
    assert seq[40:].tolist() == NEXT.tolist() and len(probs) == 14
    # per block: wqkv, wo, w1/w3, w2 in each of the two layers + the LM head; three blocks of four tokens
    assert calls == [4] * (3 * (4 * TINY["n_layer"] + 1)), calls


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_long_prompt_fed_in_blocks_then_free_tokens(dtype):
    """feed_long_prompts: 11 tokens beyond the smallest cache (12 known inputs with the split's own: blocks of 4, 4, 4 whose last
    step is the first free one), then free greedy tokens through the single step."""
    (seq, probs, _), calls = _pair(lambda: _tiny(dtype, "heavy_hitter"), _prompt(32 + 11), f"feed_long {dtype}", new_tokens=6, feed_long_prompts=True)
    assert len(seq) == 43 + 6 and len(probs) == 12 + 6
    assert set(calls) == {4} and len(calls) == 3 * (4 * TINY["n_layer"] + 1), calls


def test_seeded_sampling_blocks_equal_single_steps():
    _pair(lambda: _tiny(torch.bfloat16, "heavy_hitter"), _prompt(32 + 11), "sampled", new_tokens=6, feed_long_prompts=True, temperature=0.8,
          top_k=5, seed=7)


def test_int8_weights_take_the_per_token_route():
    from cold_compress_amd.harness import ModelArgs, Transformer
    from cold_compress_amd.harness.quantize import WeightOnlyInt8QuantHandler

    def build():
        dense = Transformer(ModelArgs(**TINY)).to(torch.float32).eval()
        dense.load_state_dict(_weights(), strict=True)
        sd = WeightOnlyInt8QuantHandler(dense.to(torch.bfloat16).to(DEV)).create_quantized_state_dict()
        with torch.device("meta"):
            model = WeightOnlyInt8QuantHandler(Transformer(ModelArgs(**TINY))).convert_for_runtime()
        model.load_state_dict(sd, assign=True)
        model = _caches(model.to(device=DEV, dtype=torch.bfloat16).eval(), "heavy_hitter", 64)
        assert not model.block_eligible()
        return model

    _pair(build, _prompt(40), "int8 weights", expect_blocks=False, next_tokens=NEXT.to(DEV))


def test_reference_mode_quantised_cache_takes_the_per_token_route():
    def build():
        model = _tiny(torch.bfloat16, "heavy_hitter", cache_bits=8)
        assert not model.block_eligible()
        return model

    _pair(build, _prompt(40), "cache_bits 8 (reference mode)", expect_blocks=False, next_tokens=NEXT.to(DEV))


def test_fused_uint8_heavy_hitter_cache_is_eligible_and_equal():
    """the fused quantised modes serve 16-bit models at head_dim 128 with a multiple of 4 query heads per kv head: a two-layer model
    of that shape with random weights."""
    from cold_compress_amd.harness import ModelArgs, Transformer

    def build():
        torch.manual_seed(5)
        cfg = dict(block_size=512, vocab_size=256, n_layer=2, n_head=8, n_local_heads=2, dim=1024, intermediate_size=512)
        model = _caches(Transformer(ModelArgs(**cfg)).to(torch.bfloat16).eval().to(DEV), "heavy_hitter", 64, cache_bits=8, cache_quant_mode="fused")
        assert all(l.attention.kv_cache.fused_quant for l in model.layers) and model.block_eligible()
        return model

    _pair(build, _prompt(40), "fused uint8 heavy_hitter", next_tokens=NEXT.to(DEV))
