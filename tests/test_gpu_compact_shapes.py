"""The prompt-compaction and bookkeeping kernels — csrc/cc_compact.hip, the fill / norm / history kernels of csrc/cc_evict.hip,
attn_bandsum and the ring update of csrc/cc_hybrid.hip, prefill_side_kernel of csrc/cc_attn_prefill.hip — against the exact references
of tests/compact_ref.py (held to the oracle's twins on the CPU by tests/test_compact_ref_host.py) and against the twins themselves.

Every comparison is equality of bit patterns, whole buffers at a time: each tensor of a call lives inside a larger device buffer
pre-filled with a sentinel (NaN, -7, 0xAB); margins must survive, inputs must come back unchanged, and since the references start
from the same sentinel-filled outputs every element the contract does not write must still hold its sentinel.  All gather indices
and positions are valid.  The one exception to equality is prefill_side_kernel, whose inputs come out of the attention kernels: it
keeps the fp32 bounds of tests/test_gpu_gqa_ratios.py.

  a. ~40 seeded ragged shapes per entry point in fp32 / bf16 / fp16 (the fp16 instantiations and gather_rows_small_kernel run
     nowhere else), with the edge cases listed in compact_ref's generators;
  b. one case per kernel just past its grid cap, so that the grid-stride loop makes its second pass (the tracked ring update: its
     192-workgroup ticket logic, over 2W + 1 updates that overwrite every ring column twice);
  c. the refusal table."""
import numpy as np
import pytest
import torch

import compact_ref as R

pytestmark = pytest.mark.gpu
F32, BF, HF = R.F32, R.BF, R.HF


def _check(oracle, c, twin=True):
    """One call on the device: return code, the reference's outputs, the oracle twin's outputs.  -> the device's outputs."""
    rc, got = R.run_device(c)
    assert rc == 0, f"{c.id}: device -> {rc}"
    want = R.reference(c)
    for n, w in want.items():
        assert R.same(w, got[n]), f"{c.id}: '{n}' device vs reference: {R.first_diffs(got[n], w)}"
    if twin:
        rc, tw = R.run_oracle(oracle, c)
        assert rc == 0 and set(tw) == set(got), c.id
        for n, w in tw.items():
            assert R.same(w, got[n]), f"{c.id}: '{n}' device vs oracle: {R.first_diffs(got[n], w)}"
    return got


# ------------------------------------------------------------------------------------------------ a. shape fuzz
@pytest.mark.parametrize("op", sorted(R.FUZZ))
def test_shape_fuzz(oracle, op):
    n = 0
    for c in R.FUZZ[op]():
        steps = getattr(c, "steps", 1)  # a ring case is the first of a chain of updates on the device's own state
        for step in range(steps):
            got = _check(oracle, c)
            if step + 1 < steps:
                c = R.ring_next(c, got, c.gen)
        n += 1
    assert n >= 40


# ------------------------------------------------------------------------------------------------ b. the second grid-stride pass
def _gens(seed):
    return np.random.default_rng(seed), torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("op", ["attn_colsum", "attn_bandsum"])
@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
def test_second_pass_attention_sums(oracle, op, dtype):
    H, Lq, Lk = 3, 3, 180001
    assert R.passes(H * Lk, R.CAP_2048) == 2
    _, gen = _gens(41)
    _check(oracle, R.attn_sum_case(op, f"{op}-second-pass-{R.DT_NAME[dtype]}", dtype, H, Lq, Lk, 2, gen))


@pytest.mark.parametrize("op,dtype", [("colsum_to_mean", BF), ("colsum_to_mean", HF), ("snapkv_priority", HF), ("snapkv_priority", F32),
                                      ("gather_vec", BF), ("gather_vec", F32)], ids=lambda v: v if isinstance(v, str) else R.DT_NAME[v])
def test_second_pass_vectors(oracle, op, dtype):
    H, L, K = 3, 180001, 175003
    assert R.passes(H * (K if op == "gather_vec" else L), R.CAP_2048) == 2
    rng, gen = _gens(42)
    cid = f"{op}-second-pass-{R.DT_NAME[dtype]}"
    if op == "colsum_to_mean":
        c = R.colsum_to_mean_case(cid, dtype, H, L, True, rng, gen)
    elif op == "snapkv_priority":
        c = R.snapkv_case(cid, dtype, H, L, 16, 4, gen)
    else:
        c = R.gather_vec_case(cid, dtype, H, L, K, rng, gen)
    _check(oracle, c)


@pytest.mark.parametrize("dtype,H,L,K,D", [(F32, 2, 17500, 17001, 128), (HF, 2, 95000, 90001, 6)], ids=["vector-f32-D128", "scalar-f16-D6"])
def test_second_pass_gather_rows(oracle, dtype, H, L, K, D):
    row_bytes = D * (4 if dtype == F32 else 2)
    items = H * K * (row_bytes // 16 if row_bytes % 16 == 0 else D)  # 16-byte chunks, or elements on the scalar path
    assert R.passes(items, R.CAP_GATHER_ROWS) == 2
    rng, gen = _gens(43)
    _check(oracle, R.gather_rows_case(f"gather_rows-second-pass-{R.DT_NAME[dtype]}-D{D}", dtype, H, L, K, D, H, rng, gen))


@pytest.mark.parametrize("H,S,tracked", [(2, 100003, False), (2, 100003, True), (3, 175003, False)],
                         ids=["plain-200006", "tracked-200006", "plain-525009"])
def test_second_pass_ring_update(oracle, H, S, tracked):
    """2W + 1 successive updates from the state a cache starts with: every ring column is overwritten twice, so the tracked form
    runs its subtract-the-old-entry path on live entries; ring, denom, counter and window sums compared after each.  The tracked
    form's grid is capped at 192 workgroups of 1024 (200,006 slots: two passes, and the last of 192 tickets bumps the counter); the
    plain form's at 2048 x 256, which 200,006 slots do not reach — the third case (525,009 slots, W + 1 updates) does."""
    W, T = 3, S - 5
    assert R.passes(H * S, R.CAP_RING_TRACKED if tracked else R.CAP_2048) == (1 if (not tracked and H == 2) else 2)
    _, gen = _gens(44)
    c = R.ring_case(f"ring_update-second-pass-H{H}-S{S}-{'tracked' if tracked else 'plain'}", BF, H, S, W, T, 5, tracked, gen)
    steps = 2 * W + 1 if H == 2 else W + 1
    for step in range(steps):
        got = _check(oracle, c, twin=step in (0, steps - 1))
        assert int(got["counter"][0]) == 5 + step + 1
        if step + 1 < steps:
            c = R.ring_next(c, got, gen)


def test_second_pass_history_update_and_fill(oracle):
    """cc_hh_update (grid capped at 1024 x 256 slots) and cc_prefill_fill (4096 x 256 32-bit words) past their caps, exactly."""
    rng, gen = _gens(45)
    assert R.passes(3 * 90001, R.CAP_HH_UPDATE) == 2
    _check(oracle, R.hh_update_case("hh_update-second-pass", HF, 3, 90001, 89990, True, rng, gen))
    assert R.passes(2 * 175003 * 3, R.CAP_PREFILL_FILL) == 2  # rows of 6 fp16 values: three words
    _check(oracle, R.prefill_fill_case("prefill_fill-second-pass", HF, 2, 2, 2, 2, 180000, 175003, 6, rng, gen))


def test_second_pass_prefill_side_outputs():
    """prefill_side_kernel folds the per-workgroup partial column / band / observation sums: H x L = 525,000 outputs over a grid capped
    at 2048 x 256.  The VALU prefill at fp32, one query head per kv head, against tests/attn_ref.py at the suite's fp32 bounds (a
    wrapped index moves whole entries, far outside them).  Its 0.8 GB workspace is handed back afterwards."""
    from cold_compress_amd import attention_utils as AU
    from test_gpu_gqa_ratios import BANDS, _prefill_check

    H, L = 2100, 250
    assert BANDS == (3, 17) and R.passes(H * L, R.CAP_2048) == 2
    before, retired = dict(AU._WS), len(AU._RETIRED)
    try:
        _prefill_check(F32, H, 1, L, 16, 46, "prefill side outputs, second pass", forms=("two",))
    finally:
        torch.cuda.synchronize()
        for key in [k for k in AU._WS if k[1] == "prefill" and AU._WS[k] is not before.get(k)]:
            if key in before:
                AU._WS[key] = before[key]
            else:
                del AU._WS[key]
        del AU._RETIRED[retired:]  # (the smaller prefill workspace it superseded is back in place)
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ c. refusals
def test_refusals_leave_every_output_untouched():
    table = R.refusals()
    assert len(table) >= 16
    for what, c in table:
        rc, got = R.run_device(c)
        assert rc == R.BAD_ARG, f"{what}: device -> {rc}"
        for n, g in got.items():
            assert R.same(g, c.t[n]), f"{what}: '{n}' was written"
