"""Shared by tests/test_streams_host.py and tests/test_gpu_streams.py.  A helper, not a test: the `tiny` model of
tests/test_gpu_forced_block.py (2 layers, dim 64, vocabulary 128, the weights of f1_e2e_heavy_hitter.npz), a 40-token prompt over a
cache of 32 so that every step evicts, lone generate() runs and the comparison of a stream with its lone run, bit for bit."""
import argparse
import functools

import torch

from helpers import load_golden

TINY = dict(block_size=256, vocab_size=128, n_layer=2, n_head=4, n_local_heads=2, dim=64, intermediate_size=128)
HYB = [{"strategy": "special"}, {"strategy": "special_punc"}, {"strategy": "special_punc_heavy_hitter", "heavy_hitter_frac": 0.3},
       {"strategy": "special_punc_window", "recent_window": 0.3}, {"strategy": "full"}]
POLICIES = [("full", {}), ("recent_global", {}), ("heavy_hitter", {}), ("l2", {}), ("random", {}), ("hybrid", {}),
            ("heavy_hitter", {"history_window_size": 8})]
POLICY_IDS = [s + ("-w8" if e else "") for s, e in POLICIES]
SAMPLED = dict(temperature=0.8, top_k=5, top_p=0.9)
NEW_TOKENS = 10
RNG_SEED = 0x5EED5EED  # KVCacheRandom's per-generation seed, fixed on both sides of a comparison


class Tok:
    def special_ids(self):
        return [[1], [2, 3]]

    def punctuation_ids(self):
        return [5, 6, 7]


@functools.lru_cache(maxsize=None)
def weights():
    f = load_golden("f1_e2e_heavy_hitter.npz")
    assert int(f["n_layer"]) == TINY["n_layer"]
    return {k[3:]: v for k, v in f.items() if k.startswith("sd.")}


def caches(model, strategy, dev, max_seq=64, **extra):
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
    setup_caches(model, Tok(), dev, max_seq, dict(kw))
    return model


def tiny(dtype, strategy, dev, max_seq=64, **extra):
    from cold_compress_amd.harness import ModelArgs, Transformer

    model = Transformer(ModelArgs(**TINY)).to(torch.float32).eval()
    model.load_state_dict(weights(), strict=True)
    return caches(model.to(dtype).to(dev), strategy, dev, max_seq, **extra)


def prompt(n, dev, seed=3):
    g = torch.Generator().manual_seed(seed)
    p = torch.randint(8, 128, (n,), generator=g, dtype=torch.int32)
    p[::9] = 6  # some punctuation for the hybrid policies
    return p.to(dev)


def fix_rng_seeds(cache_sets):
    for cs in cache_sets:
        for c in cs:
            if hasattr(c, "_rng_seed"):
                c._rng_seed = RNG_SEED


def prefill_fn():
    """harness.prefill, followed for hybrid caches by the reference's policy mix (the fixture's weights profile every head alike:
    tests/test_gpu_e2e.py does the same) — on whichever stream is active."""
    from cold_compress_amd.harness import prefill

    def pf(m, x, input_pos, **kw):
        r = prefill(m, x, input_pos, **kw)
        for layer in m.layers:
            kv = layer.attention.kv_cache
            if type(kv).__name__ == "KVCacheHybrid":
                kv.cache_strategies = (torch.arange(kv.n_heads, device=x.device) % len(HYB)).to(torch.int64).contiguous()
                kv.requires_heavy_hitter = kv.requires_punc = kv.requires_special = True
        return r

    return pf


def state_of(cache_set):
    return {f"{li}.{n}": b.detach().cpu().clone() for li, c in enumerate(cache_set) for n, b in c._buffers.items() if b is not None}


def cpu(probs):
    if isinstance(probs, list):
        return [p.detach().cpu() for p in probs]
    return type(probs)(*(p.detach().cpu() for p in probs))


def lone(build, prompt_, seed, new_tokens=NEW_TOKENS, terminator_ids=None, **gk):
    """generate() on a fresh model -> (sequence, probabilities or scores, {layer.buffer: tensor}), on the CPU"""
    from cold_compress_amd.harness import decode_one_token, generate

    model = build()
    fix_rng_seeds([[l.attention.kv_cache for l in model.layers]])
    seq, probs, _ = generate(model, prompt_, prefill_fn(), decode_one_token, max_new_tokens=new_tokens, seed=seed,
                             terminator_ids=terminator_ids, **gk)
    if prompt_.is_cuda:
        torch.cuda.synchronize()
    return seq.cpu(), cpu(probs), state_of([l.attention.kv_cache for l in model.layers])


def run_streams(build, prompts, n=None, seeds=None, new_tokens=NEW_TOKENS, **gk):
    """generate_streams on a fresh model -> (model, streams, [(sequence, probabilities or scores, state) per stream], stats)"""
    from cold_compress_amd.harness import DecodeStreams, generate_streams

    model = build()
    n = len(prompts) if isinstance(prompts, list) else n
    streams = DecodeStreams(model, n)
    fix_rng_seeds(streams.sets)
    seqs, probs, stats = generate_streams(model, prompts, prefill_fn(), new_tokens, n_streams=None if isinstance(prompts, list) else n,
                                          seeds=seeds, streams=streams, **gk)
    if model.output.weight.is_cuda:
        torch.cuda.synchronize()
    assert streams.active == 0 and all(l.attention.kv_cache is c for l, c in zip(model.layers, streams.sets[0]))
    return model, streams, [(seqs[s].cpu(), cpu(probs[s]), state_of(streams.sets[s])) for s in range(n)], stats


def bits(t):
    return t.contiguous().view(torch.int16) if t.dtype in (torch.bfloat16, torch.float16) else t


def assert_same(what, a, b, state=True):
    (seq_a, probs_a, st_a), (seq_b, probs_b, st_b) = a, b
    assert torch.equal(seq_a, seq_b), f"{what}: sequence {seq_a.tolist()} vs {seq_b.tolist()}"
    assert type(probs_a) is type(probs_b) and len(probs_a) == len(probs_b), f"{what}: {len(probs_a)} vs {len(probs_b)} rows"
    for i, (pa, pb) in enumerate(zip(probs_a, probs_b)):
        assert pa.shape == pb.shape and torch.equal(bits(pa), bits(pb)), f"{what}: probabilities / scores {i} differ"
    if state:
        assert st_a.keys() == st_b.keys()
        for n in st_a:
            assert torch.equal(bits(st_a[n]), bits(st_b[n])), f"{what}: cache buffer {n}"
