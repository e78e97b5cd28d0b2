"""Per-token log-probabilities on the host side (no GPU): the fp32 twin of cc_logprob_rows's contract against float64 on every input
family (the tolerance is one the contract itself keeps), the harness's CPU path of `token_logprobs`, the ABI rows and the refusals,
`perplexity()` against the reference's arithmetic (eval.py:230-241), and the generation loop with `logprobs=True` on the tiny model
over tests/cpu_twin.py."""
import argparse
import ctypes as C
import math
import os
import re

import pytest
import torch

import logprob_twin as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ID = lambda d: str(d).split(".")[-1]  # noqa: E731
VS = (1, 7, 8, 1023, 1024, 1025, 4099, 32000)


@pytest.mark.parametrize("dtype", L.DTYPES, ids=_ID)
def test_the_twin_keeps_the_tolerance(dtype):
    """The fp32 twin (128 slices, folded in order) against float64 on every family: errors under 2^-18 * (1 + |ref|), classes and
    ranks equal; the all-equal row gives -log V and rank 0 for every target."""
    worst = 0.0
    for V in VS:
        for name in L.FAMILIES:
            fam = L.family(name, dtype, V)
            if fam is None:
                continue
            x, targets = fam
            lsm, lse = L.ref64(x)
            for t in targets:
                lp, ls, rk = L.twin32(x, t)
                worst = max(worst, L.error(lp, lsm[t]), L.error(ls, lse))
                assert rk == L.rank_ref(x, t), (name, V, t)
                if name == "equal":
                    assert rk == 0 and abs(float(lp) + math.log(V)) <= L.TOL * (1 + math.log(V))
    print(f"{_ID(dtype)}: worst twin error {worst:.3e} * (1 + |ref|), bound {L.TOL:.3e}")
    assert worst <= L.TOL


@pytest.mark.parametrize("dtype", L.DTYPES, ids=_ID)
def test_token_logprobs_on_cpu_tensors(dtype):
    """The harness's CPU path against float64: every family's targets in one call of T rows, targets mixed with -1 and a fallback, and
    targets outside the vocabulary (NaN and -1)."""
    from cold_compress_amd.harness import token_logprobs

    for V in (1, 7, 1025, 4099):
        rows, tg = [], []
        for name in L.FAMILIES:
            fam = L.family(name, dtype, V)
            if fam is not None:
                rows += [fam[0]] * len(fam[1])
                tg += list(fam[1])
        logits = torch.stack(rows).unsqueeze(0)
        want = torch.tensor(tg, dtype=torch.int32)
        odd = torch.arange(len(tg)) % 2 == 1
        targets = torch.where(odd, torch.full_like(want, -1), want)
        fallback = torch.where(odd, want, torch.zeros_like(want))
        for args in ((want, None), (targets, fallback), (None, want)):
            lp, rk = token_logprobs(logits, *args)
            assert lp.dtype == torch.float32 and rk.dtype == torch.int32 and lp.shape == rk.shape == (len(tg),)
            for r, t in enumerate(tg):
                lsm, _ = L.ref64(rows[r])
                assert L.error(lp[r], lsm[t]) <= L.TOL, (V, r, t)
                assert int(rk[r]) == L.rank_ref(rows[r], t)
        bad = torch.tensor([V, -1, 2 ** 31 - 1], dtype=torch.int32)
        lp, rk = token_logprobs(logits[:, :3], bad, torch.tensor([0, -7, 0], dtype=torch.int32))
        assert bool(torch.isnan(lp).all()) and rk.tolist() == [-1, -1, -1]
        lp, rk = token_logprobs(logits[:, :1], torch.tensor([-1], dtype=torch.int32))  # no pointer to take the target from
        assert bool(torch.isnan(lp).all()) and rk.tolist() == [-1]


def test_abi_surface_and_refusals():
    """Both symbols are in the header and in _abi.py with matching argument counts, device-only, exported; every refusal comes before
    any launch (this machine has no device: a launch would fail with another code); the workspace is under 1 MB."""
    from cold_compress_amd import _abi, _build

    header = open(os.path.join(ROOT, "include", "coldcompress.h")).read()
    assert re.search(r"^size_t\s+cc_logprob_rows_workspace_bytes\s*\(void\)", header, re.M)
    assert re.search(r"^#define\s+CC_LOGPROB_MAX_ROWS\s+64\b", header, re.M)
    m = re.search(r"^int\s+cc_logprob_rows\s*\(([^;]*)\);", header, re.M | re.S)
    assert m and len(m.group(1).split(",")) == len(_abi.SIGNATURES["cc_logprob_rows"][1]) == 13
    assert _abi.SIGNATURES["cc_logprob_rows_workspace_bytes"][1] == []
    assert {"cc_logprob_rows", "cc_logprob_rows_workspace_bytes"} <= _abi.DEVICE_ONLY
    fns = _abi.bind(C.CDLL(_build.build()))
    nbytes = fns["cc_logprob_rows_workspace_bytes"]()
    assert 0 < nbytes < 1000000
    f = fns["cc_logprob_rows"]
    buf = (C.c_char * 128)()
    p = (C.addressof(buf) + 15) & ~15
    BAD, WS = -1, -4
    ok = dict(logits=p, T=1, V=8, row_stride=8, dtype=0, targets=p, fallback=None, logprob=p, lse=None, rank=None, workspace=p,
              workspace_bytes=nbytes, stream=None)

    def call(**kw):
        return f(*{**ok, **kw}.values())

    for kw in (dict(logits=None), dict(logprob=None), dict(workspace=None), dict(T=0), dict(T=-3), dict(T=65), dict(V=0), dict(V=-1),
               dict(row_stride=7), dict(row_stride=-8), dict(dtype=3), dict(dtype=-1)):
        assert call(**kw) == BAD, kw
    assert call(T=64, row_stride=7) == BAD  # (64 rows are served: the refusal is the stride's)
    for short in (0, 8, nbytes - 1):
        assert call(workspace_bytes=short) == WS, short
    assert call(T=65, workspace_bytes=8) == BAD  # a bad argument is named before the workspace


def test_perplexity_is_the_reference_arithmetic():
    from cold_compress_amd.harness import perplexity

    g = torch.Generator().manual_seed(11)
    probs = torch.rand(1200, generator=g).clamp_min(1e-4)
    logprob = torch.log(probs.double()).float()
    nll = -torch.log(probs.double())  # eval.py:231-236, in float64
    want = {f"ppl@{k}": float(torch.exp(torch.mean(nll[:k]))) for k in range(500, len(nll), 500)}
    want["ppl"] = float(torch.exp(torch.mean(nll)))
    got = perplexity(logprob)
    assert sorted(got) == ["ppl", "ppl@1000", "ppl@500"] == sorted(want)
    for k in want:
        assert abs(got[k] - want[k]) <= 1e-6 * want[k], k
    assert list(perplexity(logprob, every=None)) == ["ppl"] and perplexity(logprob, every=None)["ppl"] == got["ppl"]
    assert sorted(perplexity(logprob, every=400)) == ["ppl", "ppl@400", "ppl@800"]


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


def test_generate_with_logprobs_on_the_cpu_twin(monkeypatch, oracle):
    """generate(next_tokens=forced, logprobs=True) on the tiny model over CPU tensors: TokenScores of the right length whose
    perplexity is the reference's -log(probs[j][next_tokens[j]]) figure of the logprobs=False run within 1e-5; the sequence is the
    same with and without logprobs, greedy and sampled; forced_block = 4 gives bit-identical scores and did run blocks; a free-running
    greedy generation has rank 0 wherever the top logit is unique."""
    from cpu_twin import cpu_twin

    from cold_compress_amd.harness import TokenScores, decode_one_token, generate, perplexity, prefill

    model = _tiny("heavy_hitter")
    prompt = torch.randint(0, 128, (20,), generator=torch.Generator().manual_seed(1), dtype=torch.int32)
    forced = torch.randint(0, 128, (13,), generator=torch.Generator().manual_seed(2), dtype=torch.int32)
    blocks = []
    real = model.forward_block

    def counted(idx, input_pos, **kw):
        blocks.append(int(idx.shape[1]))
        return real(idx, input_pos, **kw)

    model.forward_block = counted

    def run(**kw):
        for l in model.layers:
            l.attention.kv_cache.reset()
        seq, second, stats = generate(model, prompt, prefill, decode_one_token, max_new_tokens=16, **kw)
        return seq, second, stats

    with cpu_twin(monkeypatch, oracle):
        assert model.block_eligible()
        for sampling in (dict(), dict(temperature=0.8, top_k=20, seed=1)):
            seq0, probs, _ = run(next_tokens=forced, **sampling)
            seq1, scores, stats = run(next_tokens=forced, logprobs=True, **sampling)
            assert isinstance(scores, TokenScores) and torch.equal(seq0, seq1)
            assert scores.logprob.shape == scores.rank.shape == (stats["decode_tokens"],) == (len(forced),)
            assert scores.logprob.dtype == torch.float32 and scores.rank.dtype == torch.int32
            if not sampling:  # (the greedy run's rows are the model's own distribution: the reference's perplexity, eval.py:230-241)
                nll = -torch.tensor([torch.log(probs[j][forced[j]]) for j in range(len(forced))])
                want = float(torch.exp(torch.mean(nll)))
                got = perplexity(scores.logprob)["ppl"]
                assert abs(got - want) <= 1e-5 * want, (got, want)
            assert not blocks
            seq4, scores4, _ = run(next_tokens=forced, logprobs=True, forced_block=4, **sampling)
            assert blocks and max(blocks) == 4
            assert torch.equal(seq4, seq1) and torch.equal(scores4.logprob, scores.logprob) and torch.equal(scores4.rank, scores.rank)
            blocks.clear()
            free0, rows, _ = run(**sampling)
            free1, fs, _ = run(logprobs=True, **sampling)
            assert torch.equal(free0, free1) and len(fs.logprob) == len(rows) == 16
            assert bool((fs.logprob <= 0).all()) and bool(torch.isfinite(fs.logprob).all())
            if not sampling:
                # the CPU greedy is the arg-max of an fp32 softmax: the chosen token is the top logit wherever the two largest
                # probabilities of the step differ (equal probabilities: equal or rounding-close logits, not asserted)
                unique = [float(r.topk(2).values.diff().abs()) > 0 for r in rows]
                assert sum(unique) >= 8
                assert all(int(fs.rank[j]) == 0 for j in range(16) if unique[j])
            else:
                assert int(fs.rank.max()) < 20
