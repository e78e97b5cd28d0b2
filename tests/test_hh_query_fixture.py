"""The reference's heavy-hitter decode driven FROM THE QUERY (tests/golden/f2_hh_query_bf16.npz, made by
oracle/gen_golden.py::hh_query_case by importing the reference): update_kv -> repeat_interleave ->
attention_utils.scaled_dot_product_attention(return_attn=True) -> mean over the group -> update_state, i.e.
model.py:389-427 + cache.py:690-765, 160 steps, H = 2, HQ = 8, S = 256, D = 128, bf16 (and f2_hh_query_r7_bf16.npz: 28 steps,
H = 4, HQ = 28, S = 96).

Unlike the f2_hh_* traces (ready-made attention rows) this one ties the FUSED decode step — insert + attention + history
in one pass, single launch and two launches — directly to the reference (VERDICT r2 "next" item 4), and the oracle's
attention + history pipeline as well.

Contract: each side runs on ITS OWN numeric state.  Before every step the side's own eviction choice is read
and compared with the reference's; a different slot must be a near-tie IN THE REFERENCE'S OWN SCORES (the tensor its arg-min
saw, stored in the fixture: gap <= 2 bf16 roundings of a probability average), and the side is then made to follow the
reference so that the caches stay comparable.  y within 1e-3 + 2 bf16 roundings of the reference's y; positions / K / V /
denominators exactly; the float64 history within the drift of `steps` bf16-rounded probabilities per slot."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from helpers import from_np, load_golden, to_np

BF16_ULP = 2.0 ** -8
# H = 2, HQ = 8 (4 query heads per kv head), and Qwen2's geometry: H = 4, HQ = 28 (7 per kv head: several query-head blocks per kv head
# in the decode grid, and the two-launch step — the single launch serves 4 or 8 query heads per kv head)
NAMES = ["f2_hh_query_bf16.npz", "f2_hh_query_r7_bf16.npz"]


def justified(f, t, h, mine, ref):
    sc = f["scores"][t][h].numpy()
    gap = float(sc[mine] - sc[ref])
    return 0 <= gap <= 2 * BF16_ULP * abs(float(sc[ref])) + 1e-12, gap


def score_on_rounding_boundary(q, k_img, h, s, R, scale):
    """Does one of the R query heads of kv head h have its dot product with slot s (exact, from the bf16 operands) within fp32
    accumulation noise of a bf16 rounding midpoint — before or after the scale factor (attention_utils.py:36-40 rounds twice)?
    -> (yes / no, the relative change of a probability when that score moves by one bf16 step, plus two roundings)."""
    kk = torch.from_numpy(k_img[h, s].astype(np.int16)).view(torch.bfloat16).double()
    hit, bound = False, 0.0
    for r in range(R):
        qq = q[h * R + r].double()
        dot, noise = float((qq * kk).sum()), 2e-7 * float((qq * kk).abs().sum())  # (fp32 accumulation of D = 128 products)
        for v in (dot, float(torch.tensor(dot).bfloat16()) * scale):
            if v == 0.0:
                continue
            step = 2.0 ** (math.floor(math.log2(abs(v))) - 7)  # spacing of bf16 at |v|
            frac = (abs(v) / step) % 1.0
            if abs(frac - 0.5) * step <= noise + 1e-12:
                hit = True
                bound = max(bound, math.exp(2.0 ** (math.floor(math.log2(abs(dot * scale) + 1e-30)) - 7 + 1)) - 1.0)
    return hit, bound + 2 * BF16_ULP


def y_close(y_mine, y_ref):
    return float((y_mine - y_ref).abs().max()) <= 1e-3 + 2 * BF16_ULP * float(y_ref.abs().max())


@pytest.mark.parametrize("name", NAMES)
def test_oracle_pipeline_on_reference_query_trace(oracle, audit, name):
    """cc_decode_update_heavy_hitter_cpu + cc_decode_attn_gqa_cpu (history fused) against the reference's own pipeline."""
    o = oracle
    f = load_golden(name)
    H, R, S, D, T, g, w, steps = f["H"], f["R"], f["S"], f["D"], f["T_prefill"], f["g"], f["w"], f["steps"]
    HQ, code, dtype = H * R, 1, torch.bfloat16
    st = dict(k=to_np(f["k_after_prefill"][0]), v=to_np(f["v_after_prefill"][0]), pos=f["pos_after_prefill"][0].numpy().astype(np.int32).copy(),
              mask=f["mask_after_prefill"][0, :, 0].numpy().astype(np.uint8), cts=f["cts_after_prefill"].numpy().astype(np.int32).copy(),
              num=f["num_after_prefill"][0, :, :, 0].numpy().astype(np.float64).copy(), denom=f["denom_after_prefill"][0].numpy().astype(np.int32).copy(),
              ctr=f["counter_after_prefill"].numpy().astype(np.int64).copy())
    n_just = n_flip = 0
    for t in range(steps):
        p = T + t
        pt = np.array([p], np.int32)
        dn = np.maximum(st["denom"], 1).astype(np.float32)
        sc = (st["num"].astype(np.float32) / dn).astype(np.float32)  # ref: cache.py:727-749
        sc[(st["pos"] < g) | (st["pos"] >= p - w)] = 1.0
        sc[st["pos"] == -1] = 0.0
        mine, ref = sc.argmin(axis=1), f["idx"][t].numpy()
        for h in range(H):
            if mine[h] != ref[h]:
                ok, gap = justified(f, t, h, mine[h], ref[h])
                assert ok, f"step {t} head {h}: oracle evicts {mine[h]}, reference {ref[h]} (reference score gap {gap})"
                n_just += 1
                st["num"][h, ref[h]] = -1.0  # follow the reference's (equally good) choice
        view = o.view(st["k"], st["v"], st["pos"], st["mask"], st["cts"], code)
        idx = np.zeros(H, np.int64)
        o.call("cc_decode_update_heavy_hitter", C.byref(view), o.ptr(to_np(f["k_new"][t].reshape(H, D))), o.ptr(to_np(f["v_new"][t].reshape(H, D))),
               o.ptr(pt), o.ptr(st["num"]), o.ptr(st["denom"]), g, w, o.ptr(idx), None)
        assert np.array_equal(idx, ref)
        yo, ao = np.zeros((HQ, D), np.uint16), np.zeros((H, S), np.uint16)
        o.call("cc_decode_attn_gqa", o.ptr(to_np(f["q"][t].reshape(HQ, D))), o.ptr(st["k"]), o.ptr(st["v"]), o.ptr(st["mask"]), HQ, H, S, D, code,
               1.0 / math.sqrt(D), o.ptr(yo), o.ptr(ao), None, o.ptr(st["num"]), o.ptr(st["denom"]), o.ptr(st["ctr"]), None, 0, None)
        assert y_close(from_np(yo, dtype).float(), f["y"][t][0, :, 0].float()), f"step {t}: y"
        a_mine, a_ref = from_np(ao, dtype).float(), f["attn"][t][0, :, 0].float()
        # two roundings = two SPACINGS of bf16 at the reference's value (2^(floor(log2 |a|) - 7): between 2^-8 and 2^-7 of |a|) — the four
        # probabilities of a group are rounded to bf16, their mean is rounded again, and torch's vectorised exp and libm's expf differ in
        # the last bit (r5: a fresh trace had one entry 2.4 x 2^-8 |a| off = 1.3 spacings, which "2 x 2^-8 |a|" read as a violation)
        spacing = torch.exp2(torch.floor(torch.log2(a_ref.abs().clamp_min(1e-38))) - 7)
        for h, s in ((a_mine - a_ref).abs() > 2 * spacing + 1e-30).nonzero().tolist():
            # beyond two roundings: accepted only where the reference's bf16 matmul had a dot product ON a rounding boundary (its
            # blocked fp32 accumulation and the oracle's sequential one land on different sides: the score moves by one bf16 step,
            # the probability by exp(step) — seen on 2 of 83 reference-made traces from other seeds, r5, never on the committed one)
            ok, bound = score_on_rounding_boundary(f["q"][t].reshape(HQ, D), st["k"], h, s, R, 1.0 / math.sqrt(D))
            rel = float((a_mine[h, s] - a_ref[h, s]).abs() / a_ref[h, s].abs())
            assert ok and rel <= bound, f"step {t} head {h} slot {s}: group-mean probability off by {rel / BF16_ULP:.1f} roundings, no score on a rounding boundary"
            n_flip += 1
    audit(f"n_just = {n_just} of {steps * H} evictions (limit 5 %); probabilities behind a score on a bf16 rounding boundary = {n_flip} of {steps * H * S}",
          rule="near-tie eviction", count=n_just, compared=steps * H, limit="5 % of the evictions, each within 2 bf16 roundings of the minimum")
    audit(f"boundary probabilities = {n_flip}", rule="boundary probability", count=n_flip, compared=steps * H * S, limit="1e-4 of the entries, each behind a dot product within 2e-7 of a bf16 midpoint")
    assert n_just <= 0.05 * steps * H, n_just
    assert n_flip <= 1e-4 * steps * H * S + 1, n_flip
    assert np.array_equal(st["pos"], f["final_pos"][0].numpy())
    assert np.array_equal(st["k"], to_np(f["final_k"][0])) and np.array_equal(st["v"], to_np(f["final_v"][0]))
    assert np.array_equal(st["denom"], f["final_denom"][0].numpy())
    assert np.allclose(st["num"], f["final_num"][0, :, :, 0].numpy(), rtol=2 * BF16_ULP, atol=steps * 2.0 ** -16)
    assert int(st["ctr"][0]) == int(f["final_counter"][0])


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("single", [True, False])
def test_fused_step_on_reference_query_trace(single, audit, name):
    """KVCacheHeavyHitter.decode_step — single launch and two launches — replays the reference's query-driven trace.  At 7 query
    heads per kv head the single launch does not serve the shape: single=True must fall back to the two-launch step."""
    import cold_compress_amd.cache as cache

    f = load_golden(name)
    H, R, S, D, T, g, w, steps = f["H"], f["R"], f["S"], f["D"], f["T_prefill"], f["g"], f["w"], f["steps"]
    HQ, dev = H * R, __import__("helpers").TEST_DEVICE
    cls, rk = cache.get_cache_constructor("heavy_hitter")
    kw = dict(max_cache_length=S, global_tokens=g, max_seq_length=4 * S, cache_bits=None, recent_window=w, history_window_size=1,
              attn_thresholding=False)
    with torch.device(dev):
        kv = cls(1, H, D, torch.bfloat16, **{x: kw[x] for x in rk})
    kv.single_launch = single
    assert kv.single_launch_active(HQ) == (single and R in (4, 8)), f"R = {R}: single launch {kv.single_launch_active(HQ)}"
    kv.k_cache.copy_(f["k_after_prefill"]); kv.v_cache.copy_(f["v_after_prefill"]); kv.pos.copy_(f["pos_after_prefill"])
    kv.mask.copy_(f["mask_after_prefill"]); kv.cache_cts.copy_(f["cts_after_prefill"]); kv.attn_history_num.copy_(f["num_after_prefill"])
    kv.attn_history_denom.copy_(f["denom_after_prefill"]); kv.attn_counter.copy_(f["counter_after_prefill"])
    n_just = 0
    for t in range(steps):
        pt = torch.tensor([T + t], dtype=torch.int32, device=dev)
        if not kv._next_valid:
            kv.prepare_decode(pt)
        keys = kv.next_key.cpu().numpy().view(np.uint64)  # the step's own choice: the minimum key of every head's row
        mine = ((keys.min(axis=1) & np.uint64(0xffffffff)) >> np.uint64(1)).astype(np.int64)
        ref = f["idx"][t].numpy()
        for h in range(H):
            if mine[h] != ref[h]:
                ok, gap = justified(f, t, h, mine[h], ref[h])
                assert ok, f"step {t} head {h}: the step evicts {mine[h]}, the reference {ref[h]} (reference score gap {gap})"
                n_just += 1
                row = np.full(keys.shape[1], np.uint64(0xffffffffffffffff))
                row[0] = np.uint64((int(ref[h]) << 1) | int(kv.pos[0, h, ref[h]].item() == -1))
                kv.next_key[h].copy_(torch.from_numpy(row.view(np.int64)))  # follow the reference's (equally good) choice
        y = kv.decode_step(f["q"][t].to(dev), f["k_new"][t].to(dev), f["v_new"][t].to(dev), pt)
        assert y_close(y.cpu().float()[0, :, 0], f["y"][t][0, :, 0].float()), f"step {t}: y"
    assert kv.step_status(HQ) == 0
    audit(f"n_just = {n_just} of {steps * H} evictions (limit 5 %)", rule="near-tie eviction", count=n_just, compared=steps * H, limit="5 % of the evictions, each within 2 bf16 roundings of the minimum")
    assert n_just <= 0.05 * steps * H, n_just
    assert torch.equal(kv.pos.cpu(), f["final_pos"])
    assert torch.equal(kv.k_cache.cpu(), f["final_k"]) and torch.equal(kv.v_cache.cpu(), f["final_v"])
    assert torch.equal(kv.attn_history_denom.cpu(), f["final_denom"])
    assert torch.equal(kv.cache_cts.cpu(), f["final_cts"])
    assert np.allclose(kv.attn_history_num.cpu().numpy(), f["final_num"].numpy(), rtol=2 * BF16_ULP, atol=steps * 2.0 ** -16)
    assert int(kv.attn_counter.item()) == int(f["final_counter"][0])
