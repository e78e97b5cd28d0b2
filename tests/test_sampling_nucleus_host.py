"""top-p (nucleus) and min-p sampling on the host side (no GPU): the condition on the case table (tests/sample_nucleus_twin.py), the
harness's CPU path of `sample()` against the twin of cc_sample_nucleus's contract (include/coldcompress.h), the generation loop on the
tiny model over tests/cpu_twin.py, and the ABI rows."""
import argparse
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import sample_nucleus_twin as N
import sample_twin as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ID = lambda d: str(d).split(".")[-1]  # noqa: E731


def _harness(logits, temperature, top_k, seed, pos, **kw):
    from cold_compress_amd.harness import sample

    idx, probs, n_kept = sample(logits.view(1, 1, -1), None, temperature, top_k, seed, torch.tensor([pos], dtype=torch.int32),
                                return_n_kept=True, **kw)
    assert idx.dtype == torch.int32 and tuple(idx.shape) == (1,) and probs.dtype == logits.dtype
    return int(idx), probs, int(n_kept)


def test_the_table_tests_exact_equality():
    """A condition on the inputs, not a measurement: on at least 85 % of the 240 cases the exact nucleus level's margin exceeds the
    band, so that the band admits that level alone."""
    cases = N.table()
    assert len(cases) == 240
    wide = 0
    for dtype, V, temperature, top_k, top_p in cases:
        x = S.scaled(S.case_logits(dtype, V, temperature), temperature)
        wide += N.nucleus(x, S.kept_set(x, top_k), top_p)["margin"] > N.DELTA
    print(f"{wide} of {len(cases)} cases have a margin above 2^-18")
    assert wide >= 0.85 * len(cases)


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_ID)
def test_harness_path_against_the_twin(dtype, audit):
    """The CPU `sample()` over the table: the level read from its number of kept elements inside the band (the exact level wherever the
    margin exceeds the band), probabilities 0 outside the kept set and within the greedy tail's bound inside, the token under the
    acceptance rule with at most 1 % of the cases by the gap rule."""
    n = by_gap = exact = 0
    for dt, V, temperature, top_k, top_p in N.table():
        if dt is not dtype:
            continue
        logits = S.case_logits(dtype, V, temperature)
        seed, pos = 4321 + V, 5 + n
        tok, probs, n_kept = _harness(logits, temperature, top_k, seed, pos, top_p=top_p)
        how, wide = N.check_case(logits, temperature, top_k, top_p, seed, pos, probs, tok, n_kept, dtype)
        n += 1
        by_gap += how == "gap"
        exact += wide
    audit(f"{by_gap} of {n} tokens accepted by the gap rule (limit 1 %); {exact} of {n} nucleus levels held to equality")
    assert n == 80 and by_gap <= 0.01 * n


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_ID)
def test_min_p_keeps_the_exact_set(dtype):
    """min_p in (0.01, 0.1, 0.5, 1.0), alone, with top_k and with top_p: the kept set is the twin's exactly (its size, and the
    non-zero probabilities as far as the dtype can show them)."""
    n = 0
    for V in (7, 1000, 32013):
        logits = S.case_logits(dtype, V, 1.0)
        x = S.scaled(logits, 0.9)
        for top_k in (None, 50):
            for min_p in N.MIN_PS:
                kept = S.kept_set(x, top_k) & N.min_p_set(x, min_p)
                tok, probs, n_kept = _harness(logits, 0.9, top_k, 3, n, min_p=min_p)
                assert n_kept == kept.sum(), (V, top_k, min_p)
                tw = N.twin(logits, 0.9, top_k, 3, n, kept)
                S.check_probs(probs, tw, dtype)
                assert S.accepts(tok, tw) is not None
                if min_p == 1.0:
                    assert np.array_equal(kept, x == x.max())
                n += 1
        # both filters: the intersection of the nucleus (whose mass is taken over the top-k set) and the min-p set
        nuc = N.nucleus(x, S.kept_set(x, 50), 0.9)
        assert nuc["margin"] > N.DELTA
        kept = (x >= nuc["vals"][nuc["j"]]) & N.min_p_set(x, 0.1)
        tok, probs, n_kept = _harness(logits, 0.9, 50, 3, 1, top_p=0.9, min_p=0.1)
        assert n_kept == kept.sum()
        S.check_probs(probs, N.twin(logits, 0.9, 50, 3, 1, kept), dtype)
    z = torch.tensor([0.0, -0.0, -1.0, 0.0], dtype=dtype)  # -0.0 == +0.0: min_p = 1 keeps both signs of the maximum
    _, probs, n_kept = _harness(z, 1.0, None, 1, 0, min_p=1.0)
    assert n_kept == 3 and (probs.float().numpy() != 0).tolist() == [True, True, False, True]


@pytest.mark.parametrize("dtype", S.DTYPES, ids=_ID)
def test_filters_off_is_the_positional_call(dtype):
    from cold_compress_amd.harness import sample

    for V in (7, 1000):
        logits = S.case_logits(dtype, V, 0.7).view(1, 1, -1)
        pos = torch.tensor([9], dtype=torch.int32)
        for top_k in (None, 50):
            want = sample(logits, None, 0.7, top_k, 11, pos)
            for kw in (dict(top_p=None, min_p=None), dict(top_p=1.0, min_p=0.0), dict(top_p=2.0, min_p=-1.0)):
                got = sample(logits, None, 0.7, top_k, 11, pos, **kw)
                assert len(got) == 2 and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_ties_at_the_nucleus_level_and_a_tiny_top_p():
    """Four equal values straddling the 0.9 mass point are all kept; top_p = 1e-6 with a unique maximum keeps that element alone."""
    logits, n_want = N.tie_logits(torch.float32)
    tok, probs, n_kept = _harness(logits, 1.0, None, 9, 3, top_p=0.9)
    assert n_kept == n_want and int((probs != 0).sum()) == n_want
    logits = S.case_logits(torch.float32, 1000, 1.0)
    for pos in range(4):
        tok, probs, n_kept = _harness(logits, 0.8, 50, 3, pos, top_p=1e-6)
        assert n_kept == 1 and tok == int(torch.argmax(logits)) and float(probs[tok]) == 1.0


def test_nan_single_element_and_refusals():
    from cold_compress_amd.harness import sample

    logits = S.case_logits(torch.float32, 100, 1.0)
    logits[40] = logits[70] = float("nan")
    assert _harness(logits, 0.8, 20, 1, 5, top_p=0.9, min_p=0.05)[0] == 40
    assert _harness(logits, 0.8, None, 1, 5, top_p=0.9)[0] == 40
    tok, probs, n_kept = _harness(torch.tensor([-3.0]), 0.8, 20, 1, 5, top_p=0.5, min_p=0.5)
    assert tok == 0 and float(probs[0]) == 1.0 and n_kept == 1
    pos = torch.tensor([0], dtype=torch.int32)
    for kw in (dict(top_p=0.0), dict(top_p=-1.0), dict(top_p=float("nan")), dict(min_p=1.5), dict(min_p=float("nan"))):
        with pytest.raises(ValueError):
            sample(torch.zeros(1, 1, 8), None, 1.0, None, 0, pos, **kw)


def test_abi_surface():
    """Both symbols are in the header and in _abi.py (15 arguments), device-only, exported; refusals come before any launch."""
    from cold_compress_amd import _abi, _build

    header = open(os.path.join(ROOT, "include", "coldcompress.h")).read()
    assert re.search(r"^size_t\s+cc_sample_nucleus_workspace_bytes\s*\(void\)", header, re.M)
    m = re.search(r"^int\s+cc_sample_nucleus\s*\(([^;]*)\);", header, re.M | re.S)
    assert m and len(m.group(1).split(",")) == len(_abi.SIGNATURES["cc_sample_nucleus"][1]) == 15
    assert len(_abi.SIGNATURES["cc_sample_topk"][1]) == 12  # (the old entry point keeps its signature)
    assert {"cc_sample_nucleus", "cc_sample_nucleus_workspace_bytes"} <= _abi.DEVICE_ONLY
    fns = _abi.bind(C.CDLL(_build.build()))
    nbytes = fns["cc_sample_nucleus_workspace_bytes"]()
    assert fns["cc_sample_topk_workspace_bytes"]() < nbytes < (1 << 20)
    f = fns["cc_sample_nucleus"]
    buf = (C.c_char * 64)()
    p = C.addressof(buf)
    assert f(None, 8, 0, 1.0, 0, 0.9, 0.0, 0, p, p, p, None, p, nbytes, None) == -1  # a null pointer
    for top_p in (0.0, -1.0, math.nan):
        assert f(p, 8, 0, 1.0, 0, top_p, 0.0, 0, p, p, p, None, p, nbytes, None) == -1
    for min_p in (1.5, math.nan):
        assert f(p, 8, 0, 1.0, 0, 0.9, min_p, 0, p, p, p, None, p, nbytes, None) == -1
    assert f(p, 8, 0, 0.0, 0, 0.9, 0.0, 0, p, p, p, None, p, nbytes, None) == -1  # temperature must be > 0
    assert f(p, 1 << 24, 0, 1.0, 0, 0.9, 0.0, 0, p, p, p, None, p, nbytes, None) == -1  # V above CC_SAMPLE_NUCLEUS_MAX_V with top-p on
    assert f(p, 8, 0, 1.0, 0, 0.9, 0.0, 0, p, p, p, None, p, 8, None) == -4  # workspace too small
    assert f(p, 8, 0, 1.0, 0, 0.9, 0.0, 0, p, p, p, None, p, fns["cc_sample_topk_workspace_bytes"](), None) == -4


class Tok:  # (the ids the block-eligible tiny model's caches ask for)
    def special_ids(self):
        return [[1], [2, 3]]

    def punctuation_ids(self):
        return [5, 6, 7]


def _tiny(strategy):
    import cold_compress_amd.cache as cache
    from cold_compress_amd.harness import ModelArgs, Transformer, setup_caches

    torch.manual_seed(3)
    cfg = dict(block_size=256, vocab_size=128, n_layer=2, n_head=4, n_local_heads=2, dim=64, intermediate_size=128)
    model = Transformer(ModelArgs(**cfg)).to(torch.float32).eval()
    ap = argparse.ArgumentParser()
    cache.add_cache_arguments(ap)
    kw = vars(ap.parse_args([]))
    kw.update(cache_strategy=[strategy], prompt_compression_strategy=["recent_global"], max_cache_length=[32.0], global_tokens=4, recent_window=8)
    setup_caches(model, Tok(), "cpu", 64, dict(kw))
    return model


def test_generate_end_to_end_on_the_cpu_twin(monkeypatch, oracle):
    """generate() on the tiny model over CPU tensors: top_p = 0.3 at a fixed seed gives another continuation than the same seed
    without it (and a narrower distribution); min_p likewise narrows; forced_block = 4 with sampling settings equals the
    token-by-token loop bit for bit and did run blocks; an invalid top_p raises instead of being ignored."""
    from cpu_twin import cpu_twin

    from cold_compress_amd.harness import decode_one_token, generate, prefill

    model = _tiny("heavy_hitter")
    prompt = torch.randint(0, 128, (20,), generator=torch.Generator().manual_seed(1), dtype=torch.int32)
    blocks = []
    real = model.forward_block

    def counted(idx, input_pos, **kw):
        blocks.append(int(idx.shape[1]))
        return real(idx, input_pos, **kw)

    model.forward_block = counted

    def run(**kw):
        for l in model.layers:
            l.attention.kv_cache.reset()
        seq, probs, _ = generate(model, prompt, prefill, decode_one_token, max_new_tokens=24, **kw)
        return seq, probs

    with cpu_twin(monkeypatch, oracle):
        assert model.block_eligible()
        a, pa = run(temperature=1.0, seed=1)
        b, pb = run(temperature=1.0, seed=1, top_p=0.3)
        assert not torch.equal(a, b)
        assert all(int((q != 0).sum()) < int((p != 0).sum()) for p, q in zip(pa, pb))
        b2, pb2 = run(temperature=1.0, seed=1, top_p=0.3)
        assert torch.equal(b, b2) and all(torch.equal(x, y) for x, y in zip(pb, pb2))
        c, pc = run(temperature=1.0, seed=1, min_p=0.2)
        assert all(int((q != 0).sum()) < int((p != 0).sum()) for p, q in zip(pa, pc))
        assert all(float(q[q != 0].min()) >= 0.2 * float(q.max()) * (1 - 1e-5) for q in pc)
        forced = torch.randint(0, 128, (9,), generator=torch.Generator().manual_seed(2), dtype=torch.int32)
        kw = dict(temperature=0.8, top_k=20, top_p=0.7, min_p=0.02, seed=1, next_tokens=forced)
        assert not blocks
        s1, p1 = run(**kw)
        assert not blocks
        s4, p4 = run(forced_block=4, **kw)
        assert blocks and max(blocks) == 4
        assert torch.equal(s1, s4) and len(p1) == len(p4) and all(torch.equal(x, y) for x, y in zip(p1, p4))
        plain, pp = run(temperature=0.8, top_k=20, seed=1, next_tokens=forced)
        assert any(not torch.equal(x, y) for x, y in zip(p1, pp))  # (the filters reached the forced steps' probabilities)
        with pytest.raises(ValueError):
            run(temperature=0.8, top_p=0.0, seed=1)
