"""Seeded temperature / top-k sampling on the host side (no GPU): the harness's CPU path of `sample()` against the numpy twin of the
contract (tests/sample_twin.py; include/coldcompress.h, cc_sample_topk), the kept set and the probabilities, the generator's quality
on the twin alone (Pearson's chi-square), the generation loop end to end on the tiny model over tests/cpu_twin.py, and the ABI rows."""
import argparse
import os
import re

import numpy as np
import pytest
import torch

import sample_twin as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VS = (1, 7, 1000, 32013)


def _harness(logits, temperature, top_k, seed, pos):
    from cold_compress_amd.harness import sample

    idx, probs = sample(logits.view(1, 1, -1), None, temperature, top_k, seed, torch.tensor([pos], dtype=torch.int32))
    assert idx.dtype == torch.int32 and tuple(idx.shape) == (1,) and probs.dtype == logits.dtype
    return int(idx), probs


@pytest.mark.parametrize("dtype", S.DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_harness_path_against_the_twin(dtype):
    """The CPU `sample()` against the twin under the acceptance rule (sample_twin.accepts), over V x top_k x temperature; the kept
    set is the twin's exactly, probabilities are 0 outside it and within the greedy tail's bound inside.  At most 1 % of the cases
    may pass by the gap rule, and the twin's own top-two gap exceeds G on at least 99 % of them."""
    n = by_gap = close = 0
    for V in VS:
        for temperature in S.TEMPS:
            logits = S.case_logits(dtype, V, temperature)
            for top_k in S.top_ks(V):
                seed, pos = 1234 + V, 17 + n
                tw = S.twin(logits, temperature, top_k, seed, pos)
                tok, probs = _harness(logits, temperature, top_k, seed, pos)
                how = S.accepts(tok, tw)
                assert how is not None, f"V={V} T={temperature} top_k={top_k}: token {tok}, twin {tw['token']}"
                n += 1
                by_gap += how == "gap"
                close += S.top_two_gap(tw) <= S.G
                S.check_probs(probs, tw, dtype)
                if top_k is not None and tw["kept"].sum() == 1:
                    assert tok == int(np.argmax(tw["kept"]))
    print(f"{n} cases, {by_gap} accepted by the gap rule, {close} with a top-two gap of the twin within G")
    assert by_gap <= 0.01 * n and close <= 0.01 * n


@pytest.mark.parametrize("dtype", S.DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_ties_at_the_pivot_are_all_kept(dtype):
    """Four equal values straddling the pivot (ranks 4 to 7 of 64, top_k = 5): all of them are kept, so 7 elements survive; the
    probabilities outside are exactly 0."""
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(64, generator=g).clamp(-2, 2)
    order = torch.randperm(64, generator=g)
    logits[order[:3]] = torch.tensor([5.0, 4.5, 4.0])
    logits[order[3:7]] = 3.0
    logits = logits.to(dtype)
    tw = S.twin(logits, 1.0, 5, 9, 3)
    assert tw["kept"].sum() == 7 and set(np.flatnonzero(tw["kept"])) == set(order[:7].tolist())
    tok, probs = _harness(logits, 1.0, 5, 9, 3)
    assert np.array_equal(probs.float().numpy() != 0, tw["kept"])
    S.check_probs(probs, tw, dtype)
    assert S.accepts(tok, tw) == "equal"
    # -0.0 and +0.0 compare equal: a pivot of either sign keeps both
    z = torch.tensor([0.0, -0.0, -1.0, -2.0], dtype=dtype)
    for k in (1, 2):
        _, probs = _harness(z, 1.0, k, 1, 0)
        assert (probs.float().numpy() != 0).tolist() == [True, True, False, False]


def test_nan_and_single_element():
    logits = S.case_logits(torch.float32, 100, 1.0)
    logits[40] = logits[70] = float("nan")
    assert _harness(logits, 0.8, 20, 1, 5)[0] == 40
    assert _harness(logits, 0.8, None, 1, 5)[0] == 40
    tok, probs = _harness(torch.tensor([-3.0]), 0.8, 20, 1, 5)
    assert tok == 0 and float(probs[0]) == 1.0


# Seeds committed with their statistics (20000 positions, V = 40, 39 degrees of freedom; the 99.9 % quantile is 72.05)
CHI_SEEDS = (11, 12)


def test_generator_quality_on_the_twin():
    """Deterministic: fixed logits over V = 40, positions 0 .. 19999, Pearson's chi-square of the token counts against the float64
    softmax below the 99.9 % quantile of 39 degrees of freedom for two seeds, whose token sequences differ in more than half the
    positions."""
    g = torch.Generator().manual_seed(40)
    logits = torch.randn(40, generator=g)
    p = np.exp(logits.double().numpy())
    p /= p.sum()
    P = 20000
    seqs = []
    for seed in CHI_SEEDS:
        t = S.tokens(logits, 1.0, None, seed, np.arange(P))
        counts = np.bincount(t, minlength=40).astype(np.float64)
        chi2 = float(((counts - P * p) ** 2 / (P * p)).sum())
        print(f"seed {seed}: chi-square {chi2:.2f} (smallest expected count {P * p.min():.1f})")
        assert chi2 < 72.05, (seed, chi2)
        seqs.append(t)
    assert (seqs[0] != seqs[1]).mean() > 0.5


def _tiny_with_caches():
    import cold_compress_amd.cache as cache
    from cold_compress_amd.harness import CONFIGS, ModelArgs, Transformer, setup_caches

    torch.manual_seed(3)
    model = Transformer(ModelArgs(**CONFIGS["tiny"])).to(torch.float32).eval()
    ap = argparse.ArgumentParser()
    cache.add_cache_arguments(ap)
    kw = vars(ap.parse_args([]))
    kw.update(cache_strategy=["recent_global"], prompt_compression_strategy=["recent_global"], max_cache_length=[32], global_tokens=4)
    setup_caches(model, None, "cpu", 64, dict(kw))
    return model


def test_generate_end_to_end_on_the_cpu_twin(monkeypatch, oracle):
    """The tiny model through generate() on CPU tensors (tests/cpu_twin.py): temperature None is today's greedy run bit for bit; a
    seeded run repeats itself; another seed differs; top_k = 1 is the greedy run; teacher forcing returns the forced tokens."""
    from cpu_twin import cpu_twin

    from cold_compress_amd.harness import decode_one_token, generate, greedy, prefill

    model = _tiny_with_caches()
    prompt = torch.randint(0, 128, (20,), generator=torch.Generator().manual_seed(1), dtype=torch.int32)

    def run(**kw):
        for l in model.layers:
            l.attention.kv_cache.reset()
        seq, probs, _ = generate(model, prompt, prefill, decode_one_token, max_new_tokens=24, **kw)
        return seq, probs

    def prefill_parent(m, x, input_pos, next_token=None, **_):  # the greedy steps as they stood before sampling existed
        return greedy(m(x, input_pos, mask=None, is_prefill=True), next_token)

    def decode_parent(m, x, input_pos, next_token=None, attn_top_k=1.0, **_):
        return greedy(m(x, input_pos, is_prefill=False, attn_top_k=attn_top_k), next_token)

    with cpu_twin(monkeypatch, oracle):
        for l in model.layers:
            l.attention.kv_cache.reset()
        want_seq, want_probs, _ = generate(model, prompt, prefill_parent, decode_parent, max_new_tokens=24)
        seq, probs = run()
        assert torch.equal(seq, want_seq) and all(torch.equal(a, b) for a, b in zip(probs, want_probs))
        seq, probs = run(temperature=None, top_k=20, seed=5)
        assert torch.equal(seq, want_seq) and all(torch.equal(a, b) for a, b in zip(probs, want_probs))
        a, pa = run(temperature=0.8, top_k=20, seed=1)
        b, pb = run(temperature=0.8, top_k=20, seed=1)
        assert torch.equal(a, b) and all(torch.equal(x, y) for x, y in zip(pa, pb))
        assert len(a) == 44 and all(int((p != 0).sum()) <= 20 + 4 for p in pa)  # (ties at the pivot aside, top_k entries survive)
        c, _ = run(temperature=0.8, top_k=20, seed=2)
        assert not torch.equal(a, c)
        assert not torch.equal(a, want_seq)
        d, _ = run(temperature=0.8, top_k=1, seed=1)
        assert torch.equal(d, want_seq)
        forced = torch.randint(0, 128, (9,), generator=torch.Generator().manual_seed(2), dtype=torch.int32)
        e, pe = run(temperature=0.8, top_k=20, seed=1, next_tokens=forced)
        assert torch.equal(e[20:], forced) and len(pe) == 9
        assert all(int((p != 0).sum()) <= 24 for p in pe)  # the SAMPLED distribution's probabilities come with the forced tokens


def test_sample_refuses_a_non_positive_temperature():
    from cold_compress_amd.harness import sample

    with pytest.raises(ValueError):
        sample(torch.zeros(1, 1, 8), None, 0.0, None, 0, torch.tensor([0], dtype=torch.int32))


def test_abi_surface():
    """Both symbols are declared in the header and in _abi.py, device-only (their checker is the numpy twin), and exported; argument
    validation happens before any launch."""
    import ctypes as C

    from cold_compress_amd import _abi, _build

    header = open(os.path.join(ROOT, "include", "coldcompress.h")).read()
    assert re.search(r"^size_t\s+cc_sample_topk_workspace_bytes\s*\(void\)", header, re.M)
    m = re.search(r"^int\s+cc_sample_topk\s*\(([^;]*)\);", header, re.M | re.S)
    assert m and len(m.group(1).split(",")) == len(_abi.SIGNATURES["cc_sample_topk"][1]) == 12
    assert {"cc_sample_topk", "cc_sample_topk_workspace_bytes"} <= _abi.DEVICE_ONLY
    fns = _abi.bind(C.CDLL(_build.build()))
    nbytes = fns["cc_sample_topk_workspace_bytes"]()
    assert 0 < nbytes < (1 << 20)
    assert fns["cc_sample_topk"](None, 8, 0, 1.0, 0, 0, None, None, None, None, 0, None) == -1
    buf = (C.c_char * 64)()
    p = C.addressof(buf)
    assert fns["cc_sample_topk"](p, 8, 0, 0.0, 0, 0, p, p, p, p, nbytes, None) == -1  # temperature must be > 0
    assert fns["cc_sample_topk"](p, 8, 0, 1.0, 0, 0, p, p, p, p, 8, None) == -4  # workspace too small
