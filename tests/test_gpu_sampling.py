"""cc_sample_topk on the device (include/coldcompress.h) against the numpy twin of the contract (tests/sample_twin.py): kept set,
probabilities and token over V x top_k x temperature x dtype, statelessness (any order of positions, and one captured graph replayed
over a device position), the properties the contract names, and the harness's generate() with sampling, eager and graphed."""
import argparse

import numpy as np
import pytest
import torch

import sample_twin as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
VS = (1, 7, 1000, 32013, 128256)  # 32013: not a multiple of 8; 128256: Llama-3's vocabulary


def _pos(p):
    return torch.tensor([p], dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_kernel_against_the_twin(dtype):
    """Kept set and zeros exact, probabilities within the greedy tail's bound, the token under the acceptance rule
    (sample_twin.accepts: at most 1 % of the cases by the gap rule; the count is printed)."""
    from cold_compress_amd.harness import glue

    n = by_gap = 0
    for V in VS:
        for temperature in S.TEMPS:
            logits = S.case_logits(dtype, V, temperature)
            dl = logits.to(DEV)
            for top_k in S.top_ks(V):
                seed, pos = 1234 + V, 17 + n
                probs, idx = glue.sample_topk(dl, temperature, top_k, seed, _pos(pos))
                tw = S.twin(logits, temperature, top_k, seed, pos)
                tok = int(idx)
                how = S.accepts(tok, tw)
                assert how is not None, f"V={V} T={temperature} top_k={top_k}: token {tok}, twin {tw['token']}"
                n += 1
                by_gap += how == "gap"
                S.check_probs(probs, tw, dtype)
                if top_k is not None and tw["kept"].sum() == 1:
                    assert tok == int(np.argmax(tw["kept"]))
    print(f"{n} cases, {by_gap} accepted by the gap rule")
    assert by_gap <= 0.01 * n


@pytest.mark.parametrize("dtype", S.DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_ties_at_the_pivot_are_all_kept(dtype):
    from cold_compress_amd.harness import glue

    g = torch.Generator().manual_seed(5)
    logits = torch.randn(3000, generator=g).clamp(-2, 2)
    order = torch.randperm(3000, generator=g)
    logits[order[:3]] = torch.tensor([5.0, 4.5, 4.0])
    logits[order[3:7]] = 3.0  # four equal values at ranks 4 to 7: top_k = 5 keeps all of them
    logits = logits.to(dtype)
    tw = S.twin(logits, 1.0, 5, 9, 3)
    assert tw["kept"].sum() == 7
    probs, idx = glue.sample_topk(logits.to(DEV), 1.0, 5, 9, _pos(3))
    assert np.array_equal(probs.float().cpu().numpy() != 0, tw["kept"])
    S.check_probs(probs, tw, dtype)
    assert S.accepts(int(idx), tw) is not None
    z = torch.tensor([0.0, -0.0, -1.0, -2.0], dtype=dtype, device=DEV)  # -0.0 == +0.0: a pivot of either sign keeps both
    for k in (1, 2):
        probs, _ = glue.sample_topk(z, 1.0, k, 1, _pos(0))
        assert (probs.float().cpu().numpy() != 0).tolist() == [True, True, False, False]


def test_a_whole_slice_of_banned_tokens():
    """ids 128000..128255 at -inf (LogitPenalties' ban of Llama-3's reserved tokens): the last of the 128 slices of the vocabulary
    (ids 128016..) holds nothing else, the first is banned as well.  The sampler subtracts the global maximum, so the row keeps its
    distribution: exact zeros on the banned ids, no NaN, the twin's probabilities and an accepted token."""
    from cold_compress_amd.harness import glue

    V = 128256
    logits = (torch.randn(V, generator=torch.Generator().manual_seed(11)) * 3).to(torch.bfloat16)
    logits[128000:] = -float("inf")
    logits[:1008] = -float("inf")
    dl = logits.to(DEV)
    for top_k in (None, 50):
        probs, idx = glue.sample_topk(dl, 0.8, top_k, 7, _pos(3))
        tw = S.twin(logits, 0.8, top_k, 7, 3)
        assert not bool(torch.isnan(probs).any()) and bool((probs[128000:] == 0).all()) and bool((probs[:1008] == 0).all())
        S.check_probs(probs, tw, torch.bfloat16)
        assert S.accepts(int(idx), tw) is not None and 1008 <= int(idx) < 128000


def test_stateless_in_any_order_and_under_graph_replay():
    """64 positions at V = 32000: ascending, shuffled, and inside ONE captured graph replayed while the host only rewrites the device
    position — the same token per position, and the twin's."""
    from cold_compress_amd.harness import glue

    V, seed, top_k, temperature = 32000, 77, 50, 0.9
    logits = S.case_logits(torch.bfloat16, V, temperature)
    dl = logits.to(DEV)
    positions = list(range(100, 164))
    asc = {p: int(glue.sample_topk(dl, temperature, top_k, seed, _pos(p))[1]) for p in positions}
    perm = [positions[i] for i in torch.randperm(64, generator=torch.Generator().manual_seed(1)).tolist()]
    shuf = {p: int(glue.sample_topk(dl, temperature, top_k, seed, _pos(p))[1]) for p in perm}
    assert asc == shuf
    how = [S.accepts(asc[p], S.twin(logits, temperature, top_k, seed, p)) for p in positions]
    assert None not in how and how.count("gap") <= 0.01 * len(how), how
    assert len(set(asc.values())) > 8
    pos = _pos(0)
    glue.sample_topk(dl, temperature, top_k, seed, pos)  # (the workspace exists before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        probs, idx = glue.sample_topk(dl, temperature, top_k, seed, pos)
    replayed = {}
    for p in positions:
        pos.fill_(p)
        graph.replay()
        replayed[p] = int(idx)
    assert replayed == asc


@pytest.mark.parametrize("dtype,V", [(torch.bfloat16, 128256), (torch.float32, 300), (torch.float16, 32000)], ids=["bf16", "f32", "f16"])
def test_properties(dtype, V):
    """top_k = 1, and the clamped temperature on logits whose top-two gap is at least 0.5, give the greedy tail's token; a NaN returns
    the first NaN's index; V = 1 returns 0."""
    from cold_compress_amd.harness import glue

    logits = S.case_logits(dtype, V, 1.0)
    top = int(torch.argmax(logits.float()))
    logits[top] = logits.float().max() + 0.5
    dl = logits.to(DEV)
    greedy_tok = int(glue.softmax_argmax(dl)[1])
    assert greedy_tok == top
    # sigma 0.02 and the largest logit at least 0.5 above the rest after rounding: logits / 1e-5 stays finite in f16 (< 65504)
    small = (S.case_logits(dtype, V, 1.0).float() * (0.02 / 3.0)).to(dtype)
    small[top] = small.float().max() + 0.51
    assert float(small.float().max()) < 0.65 and float(small.float().topk(2).values.diff().abs()) >= 0.5
    ds = small.to(DEV)
    assert int(glue.softmax_argmax(ds)[1]) == top
    for p in range(8):
        assert int(glue.sample_topk(dl, 0.8, 1, 3, _pos(p))[1]) == greedy_tok
        assert int(glue.sample_topk(ds, 1e-7, None, 3, _pos(p))[1]) == top
    nan = logits.clone()
    nan[V // 2] = nan[V - 1] = float("nan")
    for top_k in (None, 50):
        idx = int(glue.sample_topk(nan.to(DEV), 0.8, top_k, 3, _pos(0))[1])
        assert idx == V // 2
    one = torch.tensor([-2.5], dtype=dtype, device=DEV)
    for top_k in (None, 1, 5):
        probs, idx = glue.sample_topk(one, 0.8, top_k, 3, _pos(0))
        assert int(idx) == 0 and float(probs[0]) == 1.0


def _tiny(dtype):
    import cold_compress_amd.cache as cache
    from cold_compress_amd.harness import CONFIGS, ModelArgs, Transformer, setup_caches

    torch.manual_seed(3)
    model = Transformer(ModelArgs(**CONFIGS["tiny"])).to(dtype).eval().to(DEV)
    ap = argparse.ArgumentParser()
    cache.add_cache_arguments(ap)
    kw = vars(ap.parse_args([]))
    kw.update(cache_strategy=["recent_global"], prompt_compression_strategy=["recent_global"], max_cache_length=[32], global_tokens=4)
    setup_caches(model, None, DEV, 64, dict(kw))
    return model


def test_generate_with_sampling_graphed_equals_eager():
    """generate() on the tiny model with temperature 0.8, top_k 20: the captured step equals the eager run token for token at the
    same seed and differs from another seed; a decoder captured at one seed and called with another captures again and matches the
    eager run; without a temperature the decoder is the greedy one."""
    from cold_compress_amd.harness import GraphedDecoder, decode_one_token, generate, prefill

    model = _tiny(torch.bfloat16)
    prompt = torch.randint(0, 128, (20,), generator=torch.Generator().manual_seed(1), dtype=torch.int32).to(DEV)

    def run(dec, **kw):
        for l in model.layers:
            l.attention.kv_cache.reset()
        seq, probs, _ = generate(model, prompt, prefill, dec, max_new_tokens=24, **kw)
        torch.cuda.synchronize()
        return seq.cpu(), [p.cpu() for p in probs]

    kw1 = dict(temperature=0.8, top_k=20, seed=1)
    kw2 = dict(temperature=0.8, top_k=20, seed=2)
    e1, pe1 = run(decode_one_token, **kw1)
    e2, _ = run(decode_one_token, **kw2)
    greedy_seq, _ = run(decode_one_token)
    assert not torch.equal(e1, e2) and not torch.equal(e1, greedy_seq)
    dec = GraphedDecoder(model, **kw1)
    g1, pg1 = run(dec, **kw1)
    assert torch.equal(g1, e1) and all(torch.equal(a, b) for a, b in zip(pg1, pe1))
    graph1 = dec.graph
    g1b, _ = run(dec, **kw1)
    assert dec.graph is graph1 and torch.equal(g1b, e1)  # same settings: the captured step is reused
    g2, _ = run(dec, **kw2)
    assert dec.graph is not graph1 and torch.equal(g2, e2)  # another seed: captured again
    g0, _ = run(dec, temperature=None)
    assert torch.equal(g0, greedy_seq)
    forced = torch.randint(0, 128, (9,), generator=torch.Generator().manual_seed(2), dtype=torch.int32).to(DEV)
    f, pf = run(dec, next_tokens=forced, **kw1)
    assert torch.equal(f[20:], forced.cpu()) and all(int((p != 0).sum()) <= 24 for p in pf)
