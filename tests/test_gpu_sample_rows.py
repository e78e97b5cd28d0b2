"""cc_sample_rows on the device (include/coldcompress.h): every row of a T-row call carries the bits cc_sample_nucleus writes for that
row alone — probabilities, token and kept count — for every V, T, row stride, dtype and filter setting of the table below, with ties
at the top-k pivot, a slice of -inf and a NaN in ONE row among the rows; statelessness across rows (equal rows under different seeds,
equal seeds and positions), and one captured call replayed over positions written to device memory."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
VS = [1, 7, 256, 257, 1031, 4099, 32003]
TS = [1, 2, 3, 4, 8]
# (top_k, top_p, min_p)
FILTERS = {"none": (None, None, None), "k1": (1, None, None), "k5": (5, None, None), "k>=V": ("V+3", None, None),
           "p0.9": (None, 0.9, None), "minp0.05": (None, None, 0.05), "all": (5, 0.9, 0.05)}
TEMPERATURE = 0.8
_ID = lambda d: str(d).split(".")[-1]  # noqa: E731


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _strides(V):
    return [V, V + 1, V + 13, (V + 7) // 8 * 8]


def _pool(dtype, V):
    """eight rows of logits on the CPU: 0 plain, 1 with ONE NaN, 2 with ties at the fifth largest value (the top_k 5 pivot), 3 with
    a whole workgroup's slice of -inf, 4 .. 7 plain with other scales."""
    g = torch.Generator().manual_seed(1000 + V)
    rows = (torch.randn(8, V, generator=g) * torch.tensor([3.0, 2.0, 3.0, 3.0, 0.5, 6.0, 1.0, 4.0])[:, None]).to(dtype)
    rows[1, V // 2] = float("nan")
    if V >= 7:
        fifth = torch.sort(rows[2].float(), descending=True).values[4]
        rows[2, torch.tensor([0, V // 3, V - 1])] = fifth.to(dtype)
    per = ((V + 127) // 128 + 7) // 8 * 8  # one workgroup's slice (cc_sample.hip, sp_slice)
    if V > per:
        rows[3, per:2 * per] = float("-inf")
    return rows


def _settings(name, V):
    k, p, mp = FILTERS[name]
    return (V + 3 if k == "V+3" else k), p, mp


def _single(pool_dev, V, name, with_n):
    """row r of the pool through cc_sample_nucleus under seed 50 + r at position 7 + 3 r -> [(probs, idx, n_kept or None)]"""
    from cold_compress_amd.harness import glue

    k, p, mp = _settings(name, V)
    out = []
    for r in range(pool_dev.shape[0]):
        pos = torch.tensor([7 + 3 * r], dtype=torch.int32, device=DEV)
        res = glue.sample_nucleus(pool_dev[r], TEMPERATURE, k, p, mp, 50 + r, pos, return_n_kept=with_n)
        out.append(res if with_n else (*res, None))
    return out


def _strided(pool_dev, T, stride, offset):
    """rows 0 .. T-1 of the pool at `stride` elements from each other, `offset` elements into a NaN-filled buffer (an element read
    outside a row's own V would change that row's answer) -> a [T, V] view"""
    V = pool_dev.shape[1]
    buf = torch.full((offset + T * stride + 16,), float("nan"), dtype=pool_dev.dtype, device=DEV)
    view = buf[offset:].as_strided((T, V), (stride, 1))
    view.copy_(pool_dev[:T])
    return view


@pytest.mark.parametrize("dtype", DTYPES, ids=_ID)
@pytest.mark.parametrize("V", VS)
def test_every_row_is_the_single_row_call_bit_for_bit(V, dtype):
    from cold_compress_amd.harness import glue

    pool = _pool(dtype, V).to(DEV)
    n = 0
    for name in FILTERS:
        k, p, mp = _settings(name, V)
        for with_n in ((True, False) if name in ("none", "k5") else (True,)):  # (filters off without the count: cc_sample_topk's launches)
            want = _single(pool, V, name, with_n)
            for T in TS:
                seeds = [50 + r for r in range(T)]
                pos = torch.tensor([7 + 3 * r for r in range(T)], dtype=torch.int32, device=DEV)
                for si, stride in enumerate(_strides(V)):
                    x = _strided(pool, T, stride, offset=si % 2)  # (odd offsets: row bases that are not even 4-byte aligned)
                    got = glue.sample_rows(x, TEMPERATURE, k, p, mp, seeds, pos, return_n_kept=with_n)
                    probs, idx = got[0], got[1]
                    assert probs.shape == (T, V) and idx.shape == (T,)
                    for r in range(T):
                        what = (name, with_n, T, stride, r)
                        assert torch.equal(_bits(probs[r]), _bits(want[r][0])), what
                        assert int(idx[r]) == int(want[r][1]), what
                        if with_n:
                            assert int(got[2][r]) == int(want[r][2]), what
                    n += 1
    assert n == 9 * len(TS) * 4
    # the NaN row answers with its NaN's index (V == 1: index 0), whatever else the call holds
    assert int(idx[1]) == V // 2


def test_rows_are_stateless():
    """four equal rows under four seeds give the four single-row answers of those seeds (not all alike); equal seeds and positions
    give equal answers in every row."""
    from cold_compress_amd.harness import glue

    V = 4099
    row = _pool(torch.bfloat16, V)[0].to(DEV)
    x = row.expand(4, V)  # (row stride 0: glue copies it to four contiguous rows)
    seeds = [3, 4, 5, 6]
    pos = torch.tensor([11, 11, 11, 11], dtype=torch.int32, device=DEV)
    probs, idx, n_kept = glue.sample_rows(x, TEMPERATURE, 50, 0.95, None, seeds, pos, return_n_kept=True)
    for r, s in enumerate(seeds):
        p1, i1, n1 = glue.sample_nucleus(row, TEMPERATURE, 50, 0.95, None, s, pos[r:r + 1], return_n_kept=True)
        assert torch.equal(_bits(probs[r]), _bits(p1)) and int(idx[r]) == int(i1) and int(n_kept[r]) == int(n1)
    assert len(set(idx.tolist())) > 1
    probs, idx = glue.sample_rows(x, TEMPERATURE, 50, 0.95, None, [9, 9, 9, 9], pos)
    assert len(set(idx.tolist())) == 1 and all(torch.equal(_bits(probs[0]), _bits(probs[r])) for r in range(1, 4))


def test_a_captured_call_advances_through_device_positions():
    """ONE captured three-row call, replayed after each of three position updates written to device memory, equals three eager calls."""
    from cold_compress_amd.harness import glue

    V, T = 1031, 3
    x = _pool(torch.bfloat16, V)[4:4 + T].to(DEV)
    seeds = [21, 22, 23]
    updates = [[5, 900, 17], [6, 2, 18], [100, 101, 7]]
    args = (TEMPERATURE, 5, 0.9, 0.05, seeds)
    eager = []
    for u in updates:
        p, i, n = glue.sample_rows(x, *args, torch.tensor(u, dtype=torch.int32, device=DEV), return_n_kept=True)
        eager.append((p.clone(), i.clone(), n.clone()))
    assert len({tuple(e[1].tolist()) for e in eager}) > 1
    pos = torch.zeros(T, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        probs, idx, n_kept = glue.sample_rows(x, *args, pos, return_n_kept=True)
    for u, (p, i, n) in zip(updates, eager):
        pos.copy_(torch.tensor(u, dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(probs), _bits(p)) and torch.equal(idx, i) and torch.equal(n_kept, n)
