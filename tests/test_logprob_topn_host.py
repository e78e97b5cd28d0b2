"""Top-N alternatives on the host side (no GPU): the harness's CPU path of `token_top_logprobs` against the float64 reference
(tests/logprob_topn_twin.py) on every family, the ABI rows and the refusals of cc_logprob_topn, and the generation loop with
`logprobs=True, top_logprobs=5` on the tiny model over tests/cpu_twin.py."""
import ctypes as C
import os
import re

import pytest
import torch

import logprob_topn_twin as TN
import logprob_twin as L
from test_logprob_host import _tiny

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ID = lambda d: str(d).split(".")[-1]  # noqa: E731
VS = (1, 7, 8, 19, 20, 21, 1025)
NS = (1, 5, 20)


@pytest.mark.parametrize("dtype", L.DTYPES, ids=_ID)
def test_token_top_logprobs_on_cpu_tensors(dtype):
    """Every family's row, once per target, in one call of T rows per (V, n): ids exactly the reference's, values inside the tolerance
    by class, (-1, NaN) padding, logprob and rank those of token_logprobs; without targets the alternatives alone."""
    from cold_compress_amd.harness import token_logprobs, token_top_logprobs

    worst = 0.0
    for V in VS:
        rows, tg = [], []
        for name in TN.FAMILIES:
            fam = TN.family(name, dtype, V)
            if fam is not None:
                rows += [fam[0]] * len(fam[1])
                tg += list(fam[1])
        logits = torch.stack(rows).unsqueeze(0)
        want = torch.tensor(tg, dtype=torch.int32)
        odd = torch.arange(len(tg)) % 2 == 1
        targets = torch.where(odd, torch.full_like(want, -1), want)
        fallback = torch.where(odd, want, torch.zeros_like(want))
        lp0, rk0 = token_logprobs(logits, targets, fallback)
        for n in NS:
            lp, rk, ids, vals = token_top_logprobs(logits, n, targets, fallback)
            assert ids.dtype == torch.int32 and vals.dtype == torch.float32 and ids.shape == vals.shape == (len(tg), n)
            assert torch.equal(lp.view(torch.int32), lp0.view(torch.int32)) and torch.equal(rk, rk0) and rk.dtype == torch.int32
            for r in range(len(tg)):
                worst = max(worst, TN.check(rows[r], n, ids[r], vals[r], f"V {V}, n {n}, row {r}"))
                pad = ids[r] < 0
                assert bool(torch.isnan(vals[r][pad]).all()) and bool((ids[r][pad] == -1).all())
                if 0 <= int(rk[r]) < n:  # (position `rank` of the order is the first of the target's tie group: the same value)
                    assert torch.equal(vals[r][int(rk[r])].view(torch.int32), lp[r].view(torch.int32)), (V, n, r)
            lp, rk, ids2, vals2 = token_top_logprobs(logits, n)
            assert bool(torch.isnan(lp).all()) and rk.tolist() == [-1] * len(tg)
            assert torch.equal(ids2, ids) and torch.equal(vals2.view(torch.int32), vals.view(torch.int32))
    print(f"{_ID(dtype)}: worst error {worst:.3e} * (1 + |ref|), bound {L.TOL:.3e}")
    for n in (0, 21, -1):
        with pytest.raises(ValueError):
            token_top_logprobs(logits, n)


def test_abi_surface_and_refusals():
    """Both symbols are in the header and in _abi.py with matching argument counts, device-only, exported; every refusal comes before
    any launch (this machine has no device: a launch would fail with another code); the workspace is under 4 MB."""
    from cold_compress_amd import _abi, _build

    header = open(os.path.join(ROOT, "include", "coldcompress.h")).read()
    assert re.search(r"^size_t\s+cc_logprob_topn_workspace_bytes\s*\(void\)", header, re.M)
    assert re.search(r"^#define\s+CC_LOGPROB_MAX_TOPN\s+20\b", header, re.M)
    m = re.search(r"^int\s+cc_logprob_topn\s*\(([^;]*)\);", header, re.M | re.S)
    assert m and len(m.group(1).split(",")) == len(_abi.SIGNATURES["cc_logprob_topn"][1]) == 16
    assert _abi.SIGNATURES["cc_logprob_topn_workspace_bytes"][1] == []
    assert {"cc_logprob_topn", "cc_logprob_topn_workspace_bytes"} <= _abi.DEVICE_ONLY
    fns = _abi.bind(C.CDLL(_build.build()))
    nbytes = fns["cc_logprob_topn_workspace_bytes"]()
    assert fns["cc_logprob_rows_workspace_bytes"]() <= nbytes < 4 * 1024 * 1024
    f = fns["cc_logprob_topn"]
    buf = (C.c_char * 256)()
    p = (C.addressof(buf) + 15) & ~15
    BAD, WS = -1, -4
    ok = dict(logits=p, T=1, V=8, row_stride=8, dtype=0, targets=p, fallback=None, N=5, logprob=p, lse=None, rank=None, top_ids=p,
              top_logprobs=p, workspace=p, workspace_bytes=nbytes, stream=None)

    def call(**kw):
        return f(*{**ok, **kw}.values())

    for kw in (dict(logits=None), dict(top_ids=None), dict(top_logprobs=None), dict(workspace=None), dict(N=0), dict(N=-1), dict(N=21),
               dict(T=0), dict(T=-3), dict(T=65), dict(V=0), dict(V=-1), dict(row_stride=7), dict(row_stride=-8), dict(dtype=3),
               dict(dtype=-1), dict(workspace=p + 8), dict(logits=p + 1), dict(logits=p + 1, dtype=1)):
        assert call(**kw) == BAD, kw
    # N = 20 and T = 64 are served, with every optional pointer NULL: the next refusal is the workspace's
    for short in (0, 8, fns["cc_logprob_rows_workspace_bytes"](), nbytes - 1):
        assert call(workspace_bytes=short) == WS, short
        assert call(N=20, T=64, logprob=None, targets=None, workspace_bytes=short) == WS, short
    assert call(N=20, T=64, row_stride=7) == BAD  # (the refusal is the stride's)
    for kw in (dict(T=65), dict(N=21), dict(top_ids=None)):  # a bad argument is named before the workspace
        assert call(workspace_bytes=8, **kw) == BAD, kw


def test_generate_with_top_logprobs_on_the_cpu_twin(monkeypatch, oracle):
    """generate(next_tokens=forced, logprobs=True, top_logprobs=5) on the tiny model over CPU tensors: the sequence, logprob and rank
    of the logprobs=True run bit for bit, [decode_tokens, 5] alternatives whose rows do not increase and hold the committed token's
    own score at position `rank`; forced_block = 4 gives the same; both refusals come before anything runs."""
    from cpu_twin import cpu_twin

    from cold_compress_amd.harness import TokenScores, TokenTopScores, decode_one_token, generate, prefill

    model = _tiny("heavy_hitter")
    prompt = torch.randint(0, 128, (20,), generator=torch.Generator().manual_seed(1), dtype=torch.int32)
    forced = torch.randint(0, 128, (13,), generator=torch.Generator().manual_seed(2), dtype=torch.int32)
    calls = []
    real = model.forward

    def counted(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    model.forward = counted

    def run(**kw):
        for l in model.layers:
            l.attention.kv_cache.reset()
        return generate(model, prompt, prefill, decode_one_token, max_new_tokens=16, **kw)

    def bits(t):
        return t.view(torch.int32)

    with cpu_twin(monkeypatch, oracle):
        for sampling in (dict(), dict(temperature=0.8, top_k=20, seed=1)):
            for extra in (dict(next_tokens=forced), dict()):
                seq1, plain, _ = run(logprobs=True, **extra, **sampling)
                assert type(plain) is TokenScores
                for block in (dict(), dict(forced_block=4)):
                    seq5, top, stats = run(logprobs=True, top_logprobs=5, **extra, **block, **sampling)
                    T = stats["decode_tokens"]
                    assert isinstance(top, TokenTopScores) and torch.equal(seq5, seq1)
                    assert torch.equal(bits(top.logprob), bits(plain.logprob)) and torch.equal(top.rank, plain.rank)
                    assert top.top_ids.shape == top.top_logprobs.shape == (T, 5) and len(top.logprob) == T
                    assert top.top_ids.dtype == torch.int32 and top.top_logprobs.dtype == torch.float32
                    assert bool((top.top_ids >= 0).all()) and bool((top.top_logprobs[:, 1:] <= top.top_logprobs[:, :-1]).all())
                    hits = 0
                    for j in range(T):
                        rk = int(top.rank[j])
                        if rk < 5:
                            hits += 1
                            assert torch.equal(bits(top.top_logprobs[j, rk]), bits(top.logprob[j])), j
                    if not sampling and not extra:  # (a free greedy run commits the top probability: the top logit, or one close to it)
                        assert hits >= T // 2
        calls.clear()
        with pytest.raises(ValueError):
            run(top_logprobs=5)
        for n in (0, 21, -2):
            with pytest.raises(ValueError):
                run(logprobs=True, top_logprobs=n)
        assert not calls  # (refused before the prefill ran)
