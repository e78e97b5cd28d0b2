"""cc_logprob_topn on the device (include/coldcompress.h) against the float64 reference (tests/logprob_topn_twin.py): every input
family over V x T x dtype x row stride x n with the ids exact, the three first results and every listed value bit-equal to
cc_logprob_rows, determinism (a row alone, as row r of T, repeated, under hipGraph replay), 64 rows and NULL outputs, and the harness's
generate(logprobs=True, top_logprobs=5) on the tiny model: eager, graphed and in forced blocks."""
import ctypes as C

import pytest
import torch

import logprob_topn_twin as TN
import logprob_twin as L
from test_gpu_logprob import _strided, _tiny

pytestmark = pytest.mark.gpu
DEV = "cuda"
VS = (1, 7, 8, 19, 20, 21, 1023, 1024, 1025, 4099, 128256, 263173)
NS = (1, 5, 20)
_ID = lambda d: str(d).split(".")[-1]  # noqa: E731


def _bits(t):
    return t.view(torch.int32)


def _same(a, b):
    return all(torch.equal(_bits(x) if x.dtype == torch.float32 else x, _bits(y) if y.dtype == torch.float32 else y) for x, y in zip(a, b))


def _pairs(dtype, V):
    """one (row, target) per family and target at (dtype, V): -> rows [P, V] (CPU), per-pair row tensors (shared per family), targets"""
    per_row, tg, names = [], [], []
    for name in TN.FAMILIES:
        fam = TN.family(name, dtype, V)
        if fam is None:
            continue
        for t in fam[1]:
            per_row.append(fam[0])
            tg.append(t)
            names.append(name)
    return torch.stack(per_row), per_row, tg, names


@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("dtype", L.DTYPES, ids=_ID)
def test_kernel_against_float64(dtype, V):
    """Every family's (row, target) pairs in calls of T = 1, 3 and 4 rows, at row_stride = V and V + 3 (rows of the second are
    misaligned, the gaps hold NaN), n = 1, 5 and 20; odd pairs take their target through `fallback`.  Ids exactly the reference's,
    values inside the tolerance by class, logprob / lse / rank the bits of cc_logprob_rows on the same arguments, and every listed
    value the bits of cc_logprob_rows with that id as the target (at the two largest V for n = 20 alone)."""
    from cold_compress_amd.harness import glue

    rows, per_row, tg, names = _pairs(dtype, V)
    P = len(tg)
    want = torch.tensor(tg, dtype=torch.int32, device=DEV)
    odd = torch.arange(P, device=DEV) % 2 == 1
    targets = torch.where(odd, torch.full_like(want, -1), want)
    fallback = torch.where(odd, want, torch.zeros_like(want))
    refs = {}
    worst = 0.0
    for stride in (V, V + 3):
        dev_rows = _strided(rows, stride)
        for T in (1, 3, 4):
            cuts = range(0, P, T)
            base = [glue.logprob_rows(dev_rows[c:c + T], targets[c:c + T], fallback[c:c + T]) for c in cuts]
            base = [torch.cat([o[k] for o in base]) for k in range(3)]
            for n in NS:
                out = [glue.logprob_topn(dev_rows[c:c + T], n, targets[c:c + T], fallback[c:c + T]) for c in cuts]
                lp, lse, rk, ids, vals = (torch.cat([o[k] for o in out]) for k in range(5))
                what = f"stride {stride}, T {T}, n {n}"
                assert _same((lp, lse, rk), base), what
                if V < 100000 or n == 20:
                    for j in range(n):  # column j's ids as the rows' targets (-1 behind the padding: NaN, as the padding is)
                        col = ids[:, j].contiguous()
                        one = torch.cat([glue.logprob_rows(dev_rows[c:c + T], col[c:c + T])[0] for c in cuts])
                        assert torch.equal(_bits(one), _bits(vals[:, j])), f"{what}: column {j}"
                ids, vals = ids.cpu(), vals.cpu()
                for r in range(P):
                    key = (names[r], n)
                    if key not in refs:  # (one reference per family and n; every further row of the family must repeat its results)
                        worst = max(worst, TN.check(per_row[r], n, ids[r], vals[r], f"{what}, row {r} ({names[r]})"))
                        refs[key] = (ids[r], vals[r])
                    else:
                        assert torch.equal(ids[r], refs[key][0]) and torch.equal(_bits(vals[r]), _bits(refs[key][1])), (what, r, names[r])
    print(f"{_ID(dtype)} V={V}: worst error {worst:.3e} * (1 + |ref|), bound {L.TOL:.3e}")


@pytest.mark.parametrize("dtype,V", [(torch.bfloat16, 128256), (torch.float32, 4099), (torch.float16, 32000)], ids=["bf16", "f32", "f16"])
def test_determinism(dtype, V):
    """Each row of a T = 4 call (misaligned rows of a strided view) is bit-equal to its own T = 1 call on an aligned copy; two
    repetitions are bit-equal; a captured call replayed three times, `targets` rewritten between the replays, equals the eager answers."""
    from cold_compress_amd.harness import glue

    g = torch.Generator().manual_seed(V)
    rows = (torch.randn(4, V, generator=g) * 3).to(dtype)
    rows[1] = TN.family("tie4", dtype, V)[0]
    rows[2, V // 3] = float(rows[2].float().max()) + 20
    rows[3, 5::7] = -float("inf")
    x = _strided(rows, V + 3)
    sets = [torch.randint(0, V, (4,), generator=g, dtype=torch.int32).to(DEV) for _ in range(3)]
    sets[1][1] = -1  # (through the fallback)
    fb = torch.full((4,), V - 1, dtype=torch.int32, device=DEV)
    for n in (5, 20):
        eager = [[o.cpu() for o in glue.logprob_topn(x, n, s, fb)] for s in sets]
        again = [[o.cpu() for o in glue.logprob_topn(x, n, s, fb)] for s in sets]
        assert all(_same(e, a) for e, a in zip(eager, again))
        for k, s in enumerate(sets):
            for r in range(4):
                one = [o.cpu() for o in glue.logprob_topn(rows[r].to(DEV), n, s[r:r + 1], fb[r:r + 1])]
                assert _same([o[0] for o in one], [e[r] for e in eager[k]]), (n, k, r)
        tg = sets[0].clone()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = glue.logprob_topn(x, n, tg, fb)
        for k, s in enumerate(sets):
            tg.copy_(s)
            graph.replay()
            assert _same([o.cpu() for o in out], eager[k]), (n, k)


@pytest.mark.parametrize("dtype", L.DTYPES, ids=_ID)
def test_64_rows_and_null_outputs(dtype):
    """T = 64 in one call with targets inside and outside [0, V) and with no target pointer at all; logprob, lse and rank NULL in turn
    through the raw entry point, with a guard word behind top_ids and behind top_logprobs."""
    from cold_compress_amd import _abi
    from cold_compress_amd.harness import glue

    V, n = 4099, 20
    rows, per_row, tg, names = _pairs(dtype, V)
    idx = torch.arange(64) % len(tg)
    r64 = rows[idx].to(DEV)
    t64 = torch.tensor([tg[i] for i in idx.tolist()], dtype=torch.int32)
    t64[1::4] = torch.tensor([V, -1, 2 ** 31 - 1, -7] * 4, dtype=torch.int32)
    t64 = t64.to(DEV)
    lp, lse, rk, ids, vals = glue.logprob_topn(r64, n, t64)
    assert _same((lp, lse, rk), glue.logprob_rows(r64, t64))
    assert bool(torch.isnan(lp[1::4]).all()) and rk[1::4].tolist() == [-1] * 16
    ids_c, vals_c = ids.cpu(), vals.cpu()
    for r in range(64):
        TN.check(per_row[int(idx[r])], n, ids_c[r], vals_c[r], f"T = 64, row {r}")
    lp0, lse0, rk0, ids0, vals0 = glue.logprob_topn(r64, n)
    assert bool(torch.isnan(lp0).all()) and rk0.tolist() == [-1] * 64 and _same((lse0, ids0, vals0), (lse, ids, vals))
    with pytest.raises(_abi.ColdCompressError):
        glue.logprob_topn(torch.zeros(65, 8, dtype=dtype, device=DEV), 5)
    for bad in (0, 21):
        with pytest.raises(_abi.ColdCompressError):
            glue.logprob_topn(r64, bad)
    ws = torch.empty(int(_abi.lib()["cc_logprob_topn_workspace_bytes"]()), dtype=torch.uint8, device=DEV)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    for drop in (None, 0, 1, 2):
        three = [torch.full((64,), 7, dtype=d, device=DEV) for d in (torch.float32, torch.float32, torch.int32)]
        g_ids = torch.full((64 * n + 1,), 0x5a5a5a5a, dtype=torch.int32, device=DEV)
        g_vals = torch.full((64 * n + 1,), 12345.0, dtype=torch.float32, device=DEV)
        args = [None if k == drop else t for k, t in enumerate(three)]
        _abi.call("cc_logprob_topn", p(r64), 64, V, V, glue._DT[dtype], p(t64), None, n, p(args[0]), p(args[1]), p(args[2]), p(g_ids),
                  p(g_vals), p(ws), ws.numel(), glue._stream())
        for k, (got, ref) in enumerate(zip(three, (lp, lse, rk))):
            if k == drop:
                assert bool((got == 7).all())  # (never written)
            else:
                assert _same((got,), (ref,)), (drop, k)
        assert _same((g_ids[:-1].view(64, n), g_vals[:-1].view(64, n)), (ids, vals)), drop
        assert int(g_ids[-1]) == 0x5a5a5a5a and float(g_vals[-1]) == 12345.0


def test_generate_with_top_logprobs_eager_graphed_and_blocks():
    """generate(next_tokens=forced, logprobs=True, top_logprobs=5) for 12 forced tokens on the tiny model: the eager loop, the
    captured step and forced_block = 4 give bit-identical TokenTopScores and the same sequence; logprob and rank are the logprobs=True
    run's bits; top_ids are the reference order of each step's logits (read through a forward hook).  A sampled free run gives the same
    sequence with and without top_logprobs, eager and graphed, and holds the token's own score at position `rank`.  A decoder called
    with another width captures again."""
    from cold_compress_amd.harness import GraphedDecoder, TokenScores, TokenTopScores, decode_one_token, generate, prefill

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

    def at_rank(s):
        hits = 0
        for j in range(len(s.rank)):
            rk = int(s.rank[j])
            if 0 <= rk < s.top_ids.shape[1]:
                hits += 1
                assert torch.equal(_bits(s.top_logprobs[j, rk]), _bits(s.logprob[j])), j
        return hits

    seq0, plain = run(decode_one_token, next_tokens=forced, logprobs=True)
    assert type(plain) is TokenScores
    logits = []
    hook = model.register_forward_hook(lambda m, i, o: logits.append(o[0, -1].detach().cpu()))
    seq1, eager = run(decode_one_token, next_tokens=forced, logprobs=True, top_logprobs=5)
    hook.remove()
    assert isinstance(eager, TokenTopScores) and torch.equal(seq0, seq1)
    assert eager.top_ids.shape == eager.top_logprobs.shape == (12, 5) and eager.top_ids.dtype == torch.int32
    assert _same(eager[:2], plain)
    assert len(logits) == 12
    for j in range(12):
        TN.check(logits[j], 5, eager.top_ids[j].cpu(), eager.top_logprobs[j].cpu(), f"step {j}")
    at_rank(eager)
    dec = GraphedDecoder(model, logprobs=True, top_logprobs=5)
    seq2, graphed = run(dec, next_tokens=forced, logprobs=True, top_logprobs=5)
    seq3, blocked = run(decode_one_token, next_tokens=forced, logprobs=True, top_logprobs=5, forced_block=4)
    for other, seq in ((graphed, seq2), (blocked, seq3)):
        assert isinstance(other, TokenTopScores) and torch.equal(seq, seq1) and _same(other, eager)
    graph5 = dec.graph
    seq4, wide = run(dec, next_tokens=forced, logprobs=True, top_logprobs=3)  # (another width: captured again)
    assert dec.graph is not graph5 and wide.top_ids.shape == (12, 3) and torch.equal(seq4, seq1)
    assert _same((wide.logprob, wide.rank, wide.top_ids, wide.top_logprobs), (eager.logprob, eager.rank, eager.top_ids[:, :3], eager.top_logprobs[:, :3]))
    kw = dict(temperature=0.8, top_k=20, seed=1)
    free0, _ = run(decode_one_token, logprobs=True, **kw)
    free1, fs = run(decode_one_token, logprobs=True, top_logprobs=5, **kw)
    free2, gs = run(GraphedDecoder(model, logprobs=True, top_logprobs=5, **kw), logprobs=True, top_logprobs=5, **kw)
    assert torch.equal(free0, free1) and torch.equal(free0, free2) and _same(fs, gs)
    at_rank(fs)
    assert bool((fs.top_logprobs[:, 1:] <= fs.top_logprobs[:, :-1]).all())
