"""cc_sample_nucleus on the device (include/coldcompress.h) against the twin of its contract (tests/sample_nucleus_twin.py): the nucleus
level (read from the number of kept elements) under the band rule over the 240-case table, min-p sets exactly, identity with
cc_sample_topk when both filters are off, ties, NaN and V = 1, statelessness (any order of positions, and one captured graph replayed
over a device position), and the harness's generate() with top_p, eager and graphed."""
import argparse

import numpy as np
import pytest
import torch

import sample_nucleus_twin as N
import sample_twin as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
_ID = lambda d: str(d).split(".")[-1]  # noqa: E731


def _pos(p):
    return torch.tensor([p], dtype=torch.int32, device=DEV)


def _run(logits, temperature, top_k, top_p, min_p, seed, pos):
    from cold_compress_amd.harness import glue

    probs, idx, n_kept = glue.sample_nucleus(logits.to(DEV), temperature, top_k, top_p, min_p, seed, _pos(pos), return_n_kept=True)
    return probs, int(idx), int(n_kept)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_ID)
def test_kernel_against_the_twin(dtype, audit):
    """The table's 80 cases of this dtype: the level inside the band (the exact level wherever its margin exceeds the band), zeros
    exact outside the kept set, probabilities within the greedy tail's bound, the token under the acceptance rule (at most 1 % of the
    cases by the gap rule)."""
    n = by_gap = exact = 0
    for dt, V, temperature, top_k, top_p in N.table():
        if dt is not dtype:
            continue
        logits = S.case_logits(dtype, V, temperature)
        seed, pos = 4321 + V, 5 + n
        probs, tok, n_kept = _run(logits, temperature, top_k, top_p, None, seed, pos)
        how, wide = N.check_case(logits, temperature, top_k, top_p, seed, pos, probs, tok, n_kept, dtype)
        n += 1
        by_gap += how == "gap"
        exact += wide
    audit(f"{by_gap} of {n} tokens accepted by the gap rule (limit 1 %); {exact} of {n} nucleus levels held to equality")
    assert n == 80 and by_gap <= 0.01 * n


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_ID)
def test_min_p_keeps_the_exact_set(dtype):
    """min_p in (0.01, 0.1, 0.5, 1.0), alone, with top_k, and with top_k and top_p: the size of the kept set and the zeros are the
    twin's exactly; ties at the maximum under min_p = 1; +0 and -0 at the threshold."""
    n = 0
    for V in (7, 1000, 32013):
        logits = S.case_logits(dtype, V, 1.0)
        x = S.scaled(logits, 0.9)
        for top_k in (None, 50):
            for min_p in N.MIN_PS:
                kept = S.kept_set(x, top_k) & N.min_p_set(x, min_p)
                probs, tok, n_kept = _run(logits, 0.9, top_k, None, min_p, 3, n)
                assert n_kept == kept.sum(), (V, top_k, min_p)
                tw = N.twin(logits, 0.9, top_k, 3, n, kept)
                S.check_probs(probs, tw, dtype)
                assert S.accepts(tok, tw) is not None
                n += 1
        nuc = N.nucleus(x, S.kept_set(x, 50), 0.9)
        assert nuc["margin"] > N.DELTA
        kept = (x >= nuc["vals"][nuc["j"]]) & N.min_p_set(x, 0.1)
        probs, tok, n_kept = _run(logits, 0.9, 50, 0.9, 0.1, 3, 1)
        assert n_kept == kept.sum()
        S.check_probs(probs, N.twin(logits, 0.9, 50, 3, 1, kept), dtype)
    tied = S.case_logits(dtype, 3000, 1.0)
    top = float(tied.float().max())
    tied[torch.tensor([5, 1500, 2999])] = top  # (with the maximum itself: at least four elements at it, in three workgroups)
    want = S.scaled(tied, 1.0) == S.scaled(tied, 1.0).max()
    probs, tok, n_kept = _run(tied, 1.0, None, None, 1.0, 2, 0)
    assert n_kept == want.sum() >= 4 and np.array_equal(probs.float().cpu().numpy() != 0, want) and want[tok]
    z = torch.tensor([0.0, -0.0, -1.0, 0.0], dtype=dtype)  # -0.0 == +0.0: the maximum of either sign keeps both
    probs, _, n_kept = _run(z, 1.0, None, None, 1.0, 1, 0)
    assert n_kept == 3 and (probs.float().cpu().numpy() != 0).tolist() == [True, True, False, True]
    # the threshold itself: x - m == dmin exactly survives, the next value below does not (log(0.5) rounded to fp32, as the entry point does)
    dmin = float(np.float32(np.log(0.5)))
    edge = torch.tensor([0.0, dmin, np.nextafter(np.float32(dmin), np.float32(-1.0)), -0.0], dtype=torch.float32)
    probs, _, n_kept = _run(edge, 1.0, None, None, 0.5, 1, 0)
    assert n_kept == 3 and (probs.cpu().numpy() != 0).tolist() == [True, True, False, True]


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_ID)
def test_both_filters_off_is_cc_sample_topk_bit_for_bit(dtype):
    """probs and token equal sample_topk's at V in (7, 32013, 128256), with and without top_k, whether the filters are None or at
    their off values, and whether or not the number of kept elements is asked for (that one runs the counting launches)."""
    from cold_compress_amd.harness import glue

    for V in (7, 32013, 128256):
        dl = S.case_logits(dtype, V, 0.7).to(DEV)
        for top_k in (None, 50):
            want_p, want_i = glue.sample_topk(dl, 0.7, top_k, 11, _pos(9))
            for top_p, min_p in ((None, None), (1.0, 0.0), (2.0, -1.0)):
                p, i = glue.sample_nucleus(dl, 0.7, top_k, top_p, min_p, 11, _pos(9))
                assert torch.equal(p, want_p) and torch.equal(i, want_i), (V, top_k, top_p)
            p, i, n = glue.sample_nucleus(dl, 0.7, top_k, None, None, 11, _pos(9), return_n_kept=True)
            assert torch.equal(p, want_p) and torch.equal(i, want_i)
            x = S.scaled(dl.cpu(), 0.7)
            assert int(n) == S.kept_set(x, top_k).sum()


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_ID)
def test_ties_at_the_nucleus_level_are_all_kept(dtype):
    """Four equal values straddling the 0.9 mass point (the twin checks their margin against the band): all four are kept, 7 elements
    survive, with and without a top_k that cuts below them."""
    logits, n_want = N.tie_logits(dtype, 3000)
    x = S.scaled(logits, 1.0)
    kept = x >= np.sort(x)[-n_want]
    assert kept.sum() == n_want
    for top_k in (None, 50):
        nuc = N.nucleus(x, S.kept_set(x, top_k), 0.9)
        assert nuc["margin"] > N.DELTA and nuc["counts"][nuc["j"]] == n_want
        probs, tok, n_kept = _run(logits, 1.0, top_k, 0.9, None, 9, 3)
        assert n_kept == n_want and np.array_equal(probs.float().cpu().numpy() != 0, kept)
        tw = N.twin(logits, 1.0, top_k, 9, 3, kept)
        S.check_probs(probs, tw, dtype)
        assert S.accepts(tok, tw) is not None


@pytest.mark.parametrize("dtype,V", [(torch.bfloat16, 128256), (torch.float32, 300), (torch.float16, 32000)], ids=["bf16", "f32", "f16"])
def test_properties(dtype, V):
    """top_p = 1e-6 with a unique maximum returns the greedy token and keeps one element; a NaN returns the first NaN's index; V = 1
    returns token 0 with probability 1; invalid settings raise."""
    from cold_compress_amd import _abi
    from cold_compress_amd.harness import glue

    logits = S.case_logits(dtype, V, 1.0)
    top = int(torch.argmax(logits.float()))
    logits[top] = logits.float().max() + 0.5
    for top_k in (None, 50):
        for p in range(4):
            probs, tok, n_kept = _run(logits, 0.8, top_k, 1e-6, None, 3, p)
            assert tok == top and n_kept == 1 and float(probs[top]) == 1.0 and int((probs != 0).sum()) == 1
    nan = logits.clone()
    nan[V // 2] = nan[V - 1] = float("nan")
    for top_k in (None, 50):
        assert _run(nan, 0.8, top_k, 0.9, 0.05, 3, 0)[1] == V // 2
        assert _run(nan, 0.8, top_k, None, 0.05, 3, 0)[1] == V // 2
    one = torch.tensor([-2.5], dtype=dtype)
    for top_k in (None, 1, 5):
        probs, tok, n_kept = _run(one, 0.8, top_k, 0.5, 0.5, 3, 0)
        assert tok == 0 and float(probs[0]) == 1.0 and n_kept == 1
    for top_p, min_p in ((0.0, None), (-1.0, None), (float("nan"), None), (None, 1.5), (None, float("nan"))):
        with pytest.raises(_abi.ColdCompressError):
            glue.sample_nucleus(one.to(DEV), 0.8, None, top_p, min_p, 3, _pos(0))


def test_stateless_in_any_order_and_under_graph_replay():
    """64 positions at V = 32000 in bf16 with top_k = 50, top_p = 0.9, min_p = 0.02: ascending, shuffled, and inside ONE captured
    graph replayed while the host only rewrites the device position — the same token per position, and the twin's."""
    from cold_compress_amd.harness import glue

    V, seed, top_k, top_p, min_p, temperature = 32000, 77, 50, 0.9, 0.02, 0.9
    logits = S.case_logits(torch.bfloat16, V, temperature)
    dl = logits.to(DEV)
    positions = list(range(100, 164))

    def one(p):
        return int(glue.sample_nucleus(dl, temperature, top_k, top_p, min_p, seed, _pos(p))[1])

    asc = {p: one(p) for p in positions}
    perm = [positions[i] for i in torch.randperm(64, generator=torch.Generator().manual_seed(1)).tolist()]
    shuf = {p: one(p) for p in perm}
    assert asc == shuf
    x = S.scaled(logits, temperature)
    nuc = N.nucleus(x, S.kept_set(x, top_k), top_p)
    assert nuc["margin"] > N.DELTA
    kept = (x >= nuc["vals"][nuc["j"]]) & N.min_p_set(x, min_p)
    n_kept = int(glue.sample_nucleus(dl, temperature, top_k, top_p, min_p, seed, _pos(0), return_n_kept=True)[2])
    assert n_kept == kept.sum() < 50
    how = [S.accepts(asc[p], N.twin(logits, temperature, top_k, seed, p, kept)) for p in positions]
    assert None not in how and how.count("gap") <= 0.01 * len(how), how
    assert len(set(asc.values())) > 4
    pos = _pos(0)
    glue.sample_nucleus(dl, temperature, top_k, top_p, min_p, seed, pos)  # (the workspace exists before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        probs, idx = glue.sample_nucleus(dl, temperature, top_k, top_p, min_p, seed, pos)
    replayed = {}
    for p in positions:
        pos.fill_(p)
        graph.replay()
        replayed[p] = int(idx)
    assert replayed == asc


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


def test_generate_with_top_p_graphed_equals_eager():
    """generate() on the tiny model at temperature 1: the captured step equals the eager run token for token with top_p = 0.3; a
    decoder captured with one top_p and called with another (or with a min_p) captures again and matches the eager run; top_p = 0.3
    gives another continuation than no top_p at the same seed, with fewer non-zero probabilities at every step."""
    from cold_compress_amd.harness import GraphedDecoder, decode_one_token, generate, prefill

    model = _tiny(torch.bfloat16)
    prompt = torch.randint(0, 128, (20,), generator=torch.Generator().manual_seed(1), dtype=torch.int32).to(DEV)

    def run(dec, **kw):
        for l in model.layers:
            l.attention.kv_cache.reset()
        seq, probs, _ = generate(model, prompt, prefill, dec, max_new_tokens=24, **kw)
        torch.cuda.synchronize()
        return seq.cpu(), [p.cpu() for p in probs]

    kw0 = dict(temperature=1.0, seed=1)
    kw1 = dict(temperature=1.0, seed=1, top_p=0.3)
    kw2 = dict(temperature=1.0, seed=1, top_p=0.6)
    kw3 = dict(temperature=1.0, seed=1, top_p=0.6, min_p=0.1)
    e0, pe0 = run(decode_one_token, **kw0)
    e1, pe1 = run(decode_one_token, **kw1)
    e2, _ = run(decode_one_token, **kw2)
    e3, pe3 = run(decode_one_token, **kw3)
    assert not torch.equal(e0, e1)
    assert all(int((q != 0).sum()) < int((p != 0).sum()) for p, q in zip(pe0, pe1))
    dec = GraphedDecoder(model, **kw1)
    g1, pg1 = run(dec, **kw1)
    assert torch.equal(g1, e1) and all(torch.equal(a, b) for a, b in zip(pg1, pe1))
    graph1 = dec.graph
    g1b, _ = run(dec, **kw1)
    assert dec.graph is graph1 and torch.equal(g1b, e1)  # same settings: the captured step is reused
    g2, _ = run(dec, **kw2)
    assert dec.graph is not graph1 and torch.equal(g2, e2)  # another top_p: captured again
    graph2 = dec.graph
    g3, pg3 = run(dec, **kw3)
    assert dec.graph is not graph2 and torch.equal(g3, e3) and all(torch.equal(a, b) for a, b in zip(pg3, pe3))  # a min_p: again
    g0, _ = run(dec, **kw0, top_p=None, min_p=None)  # (a setting the call leaves out keeps the decoder's)
    assert torch.equal(g0, e0)
