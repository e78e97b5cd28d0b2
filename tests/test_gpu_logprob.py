"""cc_logprob_rows on the device (include/coldcompress.h) against float64 torch.log_softmax (tests/logprob_twin.py): every input
family over V x T x dtype x row stride, targets taken from `targets` and from `fallback`, determinism (a row alone, as row r of T,
repeated, and under hipGraph replay with the targets rewritten), and the harness's generate(logprobs=True) on the tiny model: eager,
graphed and in forced blocks."""
import argparse
import ctypes as C

import pytest
import torch

import logprob_twin as L
import sample_twin as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
VS = (1, 7, 8, 1023, 1024, 1025, 4099, 32000, 128256)
_ID = lambda d: str(d).split(".")[-1]  # noqa: E731


def _pairs(dtype, V):
    """Every (row, target) of every family at (dtype, V): -> rows [P, V] (CPU), targets [P] (python ints), names."""
    rows, tg, names = [], [], []
    for name in L.FAMILIES:
        fam = L.family(name, dtype, V)
        if fam is None:
            continue
        for t in fam[1]:
            rows.append(fam[0])
            tg.append(t)
            names.append(name)
    return torch.stack(rows), tg, names


def _strided(rows, stride):
    """rows [P, V] on the device as a view of a [P, stride] buffer (the gap holds NaN: reading it would show)."""
    P, V = rows.shape
    buf = torch.full((P * stride + 8,), float("nan"), dtype=rows.dtype, device=DEV)
    view = buf[:P * stride].view(P, stride)[:, :V]
    view.copy_(rows)
    return view


def _check(rows, tg, names, lp, lse, rk, what):
    """device results (CPU tensors) against float64: -> the worst error over (1 + |ref|)."""
    worst = 0.0
    refs = {}
    for r, t in enumerate(tg):
        key = rows[r].data_ptr()
        if key not in refs:
            refs[key] = L.ref64(rows[r])
        lsm, ls = refs[key]
        e = max(L.error(lp[r], lsm[t]), L.error(lse[r], ls) if lse is not None else 0.0)
        assert e <= L.TOL, f"{what}: row {r} ({names[r]}, target {t}): error {e:.3e} * (1 + |ref|)"
        worst = max(worst, e)
        if rk is not None:
            assert int(rk[r]) == L.rank_ref(rows[r], t), f"{what}: row {r} ({names[r]}, target {t}): rank {int(rk[r])}"
    return worst


@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("dtype", L.DTYPES, ids=_ID)
def test_kernel_against_float64(dtype, V):
    """Every family's (row, target) pairs in calls of T = 1, 3 and 4 rows, at row_stride = V and V + 3 (rows of the second are
    misaligned); odd pairs take their target through `fallback` behind a -1; logprob and lse inside the tolerance, ranks exact,
    non-finite results by class.  The worst error is printed."""
    from cold_compress_amd.harness import glue

    rows, tg, names = _pairs(dtype, V)
    fam_rows = {}
    for r in range(len(tg)):  # (one tensor per distinct row, so that _check computes each reference once)
        fam_rows.setdefault(names[r], rows[r])
    rows_l = [fam_rows[n] for n in names]
    P = len(tg)
    want = torch.tensor(tg, dtype=torch.int32, device=DEV)
    odd = torch.arange(P, device=DEV) % 2 == 1
    targets = torch.where(odd, torch.full_like(want, -1), want)
    fallback = torch.where(odd, want, torch.zeros_like(want))
    worst = 0.0
    for stride in (V, V + 3):
        dev_rows = _strided(rows, stride)
        for T in (1, 3, 4):
            out = [glue.logprob_rows(dev_rows[c:c + T], targets[c:c + T], fallback[c:c + T]) for c in range(0, P, T)]
            lp, lse, rk = (torch.cat([o[k] for o in out]).cpu() for k in range(3))
            worst = max(worst, _check(rows_l, tg, names, lp, lse, rk, f"stride {stride}, T {T}"))
    print(f"{_ID(dtype)} V={V}: worst error {worst:.3e} * (1 + |ref|), bound {L.TOL:.3e}")


@pytest.mark.parametrize("dtype", L.DTYPES, ids=_ID)
def test_targets_outside_the_vocabulary_64_rows_and_null_outputs(dtype):
    from cold_compress_amd import _abi
    from cold_compress_amd.harness import glue

    V = 4099
    rows, tg, names = _pairs(dtype, V)
    # out of range through either pointer, and no pointer at all: NaN and -1, lse still written
    x = _strided(rows[:4], V + 3)
    bad = torch.tensor([V, -1, 2 ** 31 - 1, -1], dtype=torch.int32, device=DEV)
    fb = torch.tensor([0, V + 7, 0, -9], dtype=torch.int32, device=DEV)
    lp, lse, rk = glue.logprob_rows(x, bad, fb)
    assert bool(torch.isnan(lp).all()) and rk.tolist() == [-1] * 4
    _, lse_ok, _ = glue.logprob_rows(x, torch.zeros(4, dtype=torch.int32, device=DEV))
    assert torch.equal(lse, lse_ok) and bool(torch.isfinite(lse).all())
    lp, _, rk = glue.logprob_rows(x)
    assert bool(torch.isnan(lp).all()) and rk.tolist() == [-1] * 4
    # T = 64 in one call
    idx = torch.arange(64) % len(tg)
    r64, t64, n64 = rows[idx], [tg[i] for i in idx.tolist()], [names[i] for i in idx.tolist()]
    lp, lse, rk = glue.logprob_rows(r64.to(DEV), torch.tensor(t64, dtype=torch.int32, device=DEV))
    _check(list(r64), t64, n64, lp.cpu(), lse.cpu(), rk.cpu(), "T = 64")
    with pytest.raises(_abi.ColdCompressError):
        glue.logprob_rows(torch.zeros(65, 8, dtype=dtype, device=DEV), torch.zeros(65, dtype=torch.int32, device=DEV))
    # lse and rank NULL: logprob alone, the same bits
    d = r64[:4].to(DEV)
    t = torch.tensor(t64[:4], dtype=torch.int32, device=DEV)
    alone = torch.full((4,), 7.0, dtype=torch.float32, device=DEV)
    ws = torch.empty(int(_abi.lib()["cc_logprob_rows_workspace_bytes"]()), dtype=torch.uint8, device=DEV)
    _abi.call("cc_logprob_rows", C.c_void_p(d.data_ptr()), 4, V, V, glue._DT[dtype], C.c_void_p(t.data_ptr()), None, C.c_void_p(alone.data_ptr()),
              None, None, C.c_void_p(ws.data_ptr()), ws.numel(), glue._stream())
    assert torch.equal(alone.view(torch.int32), lp[:4].view(torch.int32))


def test_a_whole_slice_of_inf():
    """ids 128000..128255 at -inf (a banned block: the last of the 128 slices, ids 128016.., holds nothing else), in the second row
    the first slice as well: logprob, lse and rank as float64 gives them; a banned target scores -inf."""
    from cold_compress_amd.harness import glue

    V, dtype = 128256, torch.bfloat16
    rows = (torch.randn(2, V, generator=torch.Generator().manual_seed(12)) * 3).to(dtype)
    rows[:, 128000:] = -float("inf")
    rows[1, :1008] = -float("inf")
    tg = [5, 127999]
    lp, lse, rk = glue.logprob_rows(rows.to(DEV), torch.tensor(tg, dtype=torch.int32, device=DEV))
    _check(list(rows), tg, ["banned block"] * 2, lp.cpu(), lse.cpu(), rk.cpu(), "whole slice of -inf")
    lp, lse2, _ = glue.logprob_rows(rows.to(DEV), torch.tensor([128100, 3], dtype=torch.int32, device=DEV))
    assert lp.tolist() == [-float("inf")] * 2 and torch.equal(lse2, lse) and bool(torch.isfinite(lse).all())


def _bits(out):
    return [o.cpu().view(torch.int32) for o in out]


@pytest.mark.parametrize("dtype,V", [(torch.bfloat16, 128256), (torch.float32, 4099), (torch.float16, 32000)], ids=["bf16", "f32", "f16"])
def test_determinism(dtype, V):
    """Each row of a T = 4 call (misaligned rows of a strided view) is bit-equal to its own T = 1 call on an aligned copy; two
    repetitions are bit-equal; a captured call replayed three times, `targets` rewritten between the replays, equals the eager answers."""
    from cold_compress_amd.harness import glue

    g = torch.Generator().manual_seed(V)
    rows = (torch.randn(4, V, generator=g) * 3).to(dtype)
    rows[2, V // 3] = float(rows[2].float().max()) + 20
    rows[3, 5::7] = -float("inf")
    x = _strided(rows, V + 3)
    sets = [torch.randint(0, V, (4,), generator=g, dtype=torch.int32).to(DEV) for _ in range(3)]
    sets[1][1] = -1  # (through the fallback)
    fb = torch.full((4,), V - 1, dtype=torch.int32, device=DEV)
    eager = [_bits(glue.logprob_rows(x, s, fb)) for s in sets]
    again = [_bits(glue.logprob_rows(x, s, fb)) for s in sets]
    assert all(torch.equal(a, b) for e, f in zip(eager, again) for a, b in zip(e, f))
    for k, s in enumerate(sets):
        for r in range(4):
            one = _bits(glue.logprob_rows(rows[r].to(DEV), s[r:r + 1], fb[r:r + 1]))
            assert all(torch.equal(o[0], e[r]) for o, e in zip(one, eager[k])), (k, r)
    tg = sets[0].clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = glue.logprob_rows(x, tg, fb)
    for k, s in enumerate(sets):
        tg.copy_(s)
        graph.replay()
        assert all(torch.equal(a, b) for a, b in zip(_bits(out), eager[k])), k


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


def test_generate_with_logprobs_eager_graphed_and_blocks():
    """generate(next_tokens=forced, logprobs=True) for 12 forced tokens on the tiny model: the eager loop, the captured step and
    forced_block = 4 give bit-identical TokenScores; against the logprobs=False run's rows |logprob - log(float(p[target]))| <=
    2 * PROB_ULP wherever p[target] is a normal number, and rank == 0 exactly where the forced token's logit is the row's maximum (the
    step's logits are read through a forward hook on the model).  A sampled free run gives the same
    sequence with and without logprobs, eager and graphed; its scores are finite, <= 0 and of rank < 20."""
    from cold_compress_amd.harness import GraphedDecoder, TokenScores, decode_one_token, generate, prefill

    dtype = torch.bfloat16
    model = _tiny(dtype)
    prompt = torch.randint(0, 128, (20,), generator=torch.Generator().manual_seed(1), dtype=torch.int32).to(DEV)
    forced = torch.randint(0, 128, (12,), generator=torch.Generator().manual_seed(2), dtype=torch.int32).to(DEV)

    def run(dec, **kw):
        for l in model.layers:
            l.attention.kv_cache.reset()
        seq, second, _ = generate(model, prompt, prefill, dec, max_new_tokens=12, **kw)
        torch.cuda.synchronize()
        return seq.cpu(), second

    logits = []
    hook = model.register_forward_hook(lambda m, i, o: logits.append(o[0, -1].detach().float().cpu()))
    seq0, rows = run(decode_one_token, next_tokens=forced)
    hook.remove()
    seq1, eager = run(decode_one_token, next_tokens=forced, logprobs=True)
    assert isinstance(eager, TokenScores) and eager.logprob.shape == eager.rank.shape == (12,) and torch.equal(seq0, seq1)
    seq2, graphed = run(GraphedDecoder(model, logprobs=True), next_tokens=forced, logprobs=True)
    seq3, blocked = run(decode_one_token, next_tokens=forced, logprobs=True, forced_block=4)
    for other, seq in ((graphed, seq2), (blocked, seq3)):
        assert torch.equal(seq, seq1)
        assert torch.equal(other.logprob.view(torch.int32), eager.logprob.view(torch.int32)) and torch.equal(other.rank, eager.rank)
    assert len(rows) == len(logits) == 12
    tiny_normal = torch.finfo(dtype).tiny
    for j in range(12):
        t = int(forced[j])
        p = float(rows[j][t].float())
        if p >= tiny_normal:
            assert abs(float(eager.logprob[j]) - float(torch.log(torch.tensor(p, dtype=torch.float64)))) <= 2 * S.PROB_ULP[dtype], j
        assert (int(eager.rank[j]) == 0) == bool(logits[j][t] == logits[j].max()), j
    kw = dict(temperature=0.8, top_k=20, seed=1)
    free0, _ = run(decode_one_token, **kw)
    free1, fs = run(decode_one_token, logprobs=True, **kw)
    free2, gs = run(GraphedDecoder(model, logprobs=True, **kw), logprobs=True, **kw)
    assert torch.equal(free0, free1) and torch.equal(free0, free2)
    assert torch.equal(fs.logprob.view(torch.int32), gs.logprob.view(torch.int32)) and torch.equal(fs.rank, gs.rank)
    assert bool(torch.isfinite(fs.logprob).all()) and bool((fs.logprob <= 0).all())
    assert int(fs.rank.min()) >= 0 and int(fs.rank.max()) < 20
