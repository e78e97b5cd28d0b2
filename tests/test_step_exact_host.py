"""tests/step_exact.py on the CPU: the oracle's step twins, driven through the real cache classes (tests/cpu_twin.py) in the three-call
form and the decode_step form, return the simulator's answers bit for bit in every buffer; the constructions have the properties the
helper's docstring claims; every one-fault mutant of the simulator is rejected by at least one case (the table below says by which),
while the older comparison — N(0, 1) inputs, a brim-full cache, 1e-3 + two roundings on y — accepts some of them."""
import os

import numpy as np
import pytest
import torch

import step_exact as E
from cpu_twin import cpu_twin

BF, HF, F32 = E.BF, E.HF, E.F32
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cold_compress_amd", "csrc")
HOST_SHAPES = [t for t in E.shape_list() if t[4] <= 4160]


# ------------------------------------------------------------------------------------------------ the plan mirror
@pytest.mark.parametrize("fname", sorted(E.MIRRORED_LINES))
def test_mirrored_plan_lines_are_the_source(fname):
    """plan() copies these lines of the launch plan: when one changes, update the mirror (and INTENDED, and the cases)."""
    src = " ".join(open(os.path.join(CSRC, fname)).read().split())
    for line in E.MIRRORED_LINES[fname]:
        assert " ".join(line.split()) in src, f"{fname} no longer contains: {line}"


def test_every_shape_lands_on_its_intended_path():
    seen = set()
    for (pol, dt, H, HQ, S, D) in E.shape_list():
        pl = E.plan(HQ, H, S, D, dt, pol)
        nw, nt, xl2 = E.intended(dt, D, H, HQ, S)
        assert (pl["nw"], pl["nt"]) == (nw, nt), (pol, H, HQ, S, pl)
        assert (pl["xl2"] and pl["nt"] > 0) == (xl2 and nt > 0)
        seen.add((pl["nw"], pl["nt"], pl["xl2"] and nt > 0, HQ // H))
    assert {r for _, _, _, r in seen} >= {1, 2, 4, 7, 8}
    assert {(w, t) for w, t, _, _ in seen} >= {(4, 1), (8, 1), (4, 2), (4, 5), (4, 9), (4, 0)}
    # the partly filled last split / workgroup of the table: 3, 2, 8 and 10 rows
    for (H, HQ, S), rows in (((2, 2, 67), 3), ((2, 4, 130), 2), ((3, 12, 130), 2), ((1, 8, 200), 8), ((16, 128, 1290), 10)):
        pl = E.plan(HQ, H, S, 128, BF)
        assert S - (pl["n_split"] - 1) * pl["rows_per_split"] == rows


def test_the_valu_table_reaches_every_geometry():
    """Conditions on E.VALU_SHAPES (the shapes served by decode_attn_split_kernel<T, D, RT, 4, 4> and the combine pass with a run-time
    D), not measurements: any shape may change as long as all of these still hold."""
    inst, single, short_tail, two_iter, rt_groups = set(), set(), set(), set(), set()
    many_keys = few_outputs = straddle = further_groups = False
    for (pol, dt, H, HQ, S, D) in E.shape_list():
        es = 4 if dt == F32 else 2
        if es == 2 and D == 128:
            continue  # (the matrix-core kernel)
        pl, geo, R = E.plan(HQ, H, S, D, dt, pol), E.valu_geometry(dt, D), HQ // H
        assert pl["nt"] == 0 and pl["nw"] == 4 and pl["rpi"] == geo["rpi"] and geo["lpr"] * geo["rpw"] == 64, (pol, dt, H, HQ, S, D)
        assert not (pol == "hh" and pl["xl2"] and pl["nt"])
        rps, ns, rpi = pl["rows_per_split"], pl["n_split"], pl["rpi"]
        inst.add((dt, D, pl["rt"]))
        if ns == 1 and S < rpi and S % 2 == 1 and H > 1:  # one partly filled split; head 1's mask row starts at byte S: off a word
            assert (1 * S) % 4 != 0
            single.add((es, D))
        if ns >= 2 and S - (ns - 1) * rps <= 3:
            short_tail.add((es, D))
        if rps == 2 * rpi:
            two_iter.add(es)
        if R // pl["rt"] > 1:
            rt_groups.add(pl["rt"])
        nchunks = (S + E.NEXT_KEY_CHUNK - 1) // E.NEXT_KEY_CHUNK
        many_keys |= nchunks > 64  # the `lane + 64` loop over the partial arg-min keys
        y_total = R * D
        y_per = (y_total + nchunks - 1) // nchunks  # the combine pass: block c of a head takes outputs [c y_per, (c + 1) y_per)
        few_outputs |= y_total < nchunks
        further_groups |= y_total // nchunks > 128
        straddle |= any(c * y_per // D != (min(y_total, (c + 1) * y_per) - 1) // D for c in range(nchunks) if c * y_per < y_total)
    want = {(dt, D, rt) for dt in (BF, HF) for D in (16, 32, 64) for rt in (1, 2, 4)} | {(F32, D, rt) for D in (16, 32, 64, 128) for rt in (1, 2, 4)}
    assert len(want) == 30 and inst == want, want ^ inst
    every = {(2, D) for D in (16, 32, 64)} | {(4, D) for D in (16, 32, 64, 128)}
    assert single == every, every - single
    assert short_tail == every, every - short_tail
    assert two_iter == {2, 4}
    assert rt_groups == {1, 2, 4}
    assert many_keys and few_outputs and straddle and further_groups


def test_amp_of_the_existing_cases_is_unchanged():
    """amp starts at 128 and doubles while the measured gap is below GAP_MIN and amp * D < 16384: 128 at D = 128 (every answer from
    before the VALU table is what it was), 256 for the fp32 / D = 16 case; and no case anywhere falls short of GAP_MIN."""
    for t in E.shape_list():
        pol, dt, H, HQ, S, D = t
        if S > 8300:
            continue  # (D = 128: the loop's second condition already holds amp at 128)
        for c in E.cases_of(t):
            if D == 128:
                assert c.amp == 128, c.id
            if t == ("hh", F32, 2, 4, 77, 16):
                assert c.amp == 256, c.id
            assert c.amp in (128, 256, 512) and c.amp * D <= 16384 and c.gap >= E.GAP_MIN, (c.id, c.amp, c.gap)


def test_caches_without_a_valu_step_say_so_at_head_dim_64():
    """l2, hybrid and the fused quantised cache have their fused decode step in the matrix-core kernel only (head_dim 128): at
    head_dim 64 the first two report that they have none (the callers then take the three-call path) and the third refuses to be
    built — none is handed to the VALU pass, which knows nothing of them."""
    import types

    import cold_compress_amd.cache as cache
    import step_exact_ring as G

    for dt in (BF, HF):
        for D, ok in ((128, True), (64, False)):
            l2 = E.make_cache(types.SimpleNamespace(policy="l2", S=130, g=E.G_TOK, w=E.W_REC, H=2, D=D, dt=dt), "cpu")
            assert l2.supports_fused_step() == ok, (dt, D)
            hyb = G.make_cache(types.SimpleNamespace(family="hyb", S=130, g=G.G_TOK, H=2, D=D, dt=dt), "cpu")
            assert hyb._fused_shape_ok() == ok and not hyb.supports_fused_step(), (dt, D)  # (no fused step before the heads are profiled)
            hyb.cache_strategies = torch.zeros(2, dtype=torch.int64)
            assert hyb.supports_fused_step() == ok, (dt, D)
    cls, rk = cache.get_cache_constructor("heavy_hitter")
    kw = dict(max_cache_length=130, global_tokens=E.G_TOK, max_seq_length=600, cache_bits=8, history_window_size=1, recent_window=E.W_REC,
              attn_thresholding=False)
    kw = {k: kw[k] for k in rk}
    for mode, bits_ in (("fused", 8), ("fp8", 8), ("uint4", 4), ("mxfp4", 4)):
        kw["cache_bits"] = bits_
        cls(1, 2, 128, BF, cache_quant_mode=mode, **kw)
        with pytest.raises(cache.ColdCompressError, match="head_dim 128"):
            cls(1, 2, 64, BF, cache_quant_mode=mode, **kw)


# ------------------------------------------------------------------------------------------------ the constructions
@pytest.mark.parametrize("nbits,T", [(8, 240), (11, 2000), (13, 8000), (15, 32000), (16, 65000)])
def test_gap_by_code_length(nbits, T):
    """The gaps the construction rests on, at every code length the cases use (and 16): >= 181 in both 16-bit dtypes."""
    assert E.P.nbits_for(T + 12) == nbits
    rep = 128 // nbits
    n = 128 - 2 * rep * np.arange(0, nbits + 1)
    for dt in (BF, HF):
        sc = E.P.rounded_scores(n, 128, E.P.default_scale(128), dt)
        assert sc[0] - sc[1:].max() >= 181 and np.isfinite(sc).all(), (dt, sc[0] - sc[1:].max())


def test_constructions():
    zero_run = pairs = 0
    for t in HOST_SHAPES:
        for c in E.cases_of(t):
            assert c.gap >= 150, (c.id, c.gap)  # (measured on the dtype-rounded scores by Case._measure, with its other assertions)
            # integer dot products: ascending and descending fp32 sums equal the float64 one, below 2^24
            q = torch.from_numpy(c.amp * c.codes[c.T - 1]).to(c.dt).double()
            k = c.k_all[0, : min(c.L, 300)].double()
            d64 = k @ q
            asc, desc = torch.zeros(len(k)), torch.zeros(len(k))
            for d in range(c.D):
                asc = asc + (k[:, d] * q[d]).float()
                desc = desc + (k[:, c.D - 1 - d] * q[c.D - 1 - d]).float()
            assert torch.equal(asc.double(), d64) and torch.equal(desc.double(), d64) and float(d64.abs().max()) < 2 ** 24
            assert torch.equal(d64.to(c.dt).double(), d64)
            assert bool((c.v_all.double() != 0).all())
            if c.policy == "hh":  # the planted ties are ties in float32
                avg = (c.num0.astype(np.float32) / np.maximum(c.den0, 1).astype(np.float32))
                if c.hist == "pairs" and c.planted:
                    pairs += 1
                    s = sorted(c.planted)
                    assert len({avg[h, x].tobytes() for h in range(c.H) for x in s}) == 1
                    assert float(avg[:, s].max()) < float(np.delete(avg[:, c.g:c.T - c.w], [x - c.g for x in s], axis=1).min())
                if c.hist == "zeros" and c.T > 140:
                    zero_run += 1
                    assert int((avg[0, c.g:c.T - c.w] == 0).sum()) > 64
            if c.policy == "l2":
                norms = {c.norm_of(e) for e in (0, 1, 2)}
                assert len(norms) == 3
                assert len({tuple(c.e[h, :c.T]) for h in range(c.H)}) == c.H  # the heads differ
    assert zero_run >= 5 and pairs >= 5


# ------------------------------------------------------------------------------------------------ the oracle's twins return the answers
@pytest.mark.parametrize("shape", HOST_SHAPES, ids=E.shape_id)
def test_oracle_twins_return_the_answers(monkeypatch, oracle, shape):
    """Three-call form and decode_step form, every buffer bit for bit after every step; small cases also hold the one-hot answers to
    the float64 evaluation of the contract (attend_dense)."""
    n = 0
    with cpu_twin(monkeypatch, oracle):
        for c in E.cases_of(shape):
            for form in ("three", "two"):
                kv, m = E.run_replay(c, form, "cpu", dense=(c.S <= 200 and form == "three"))
                n += m
    assert n > 0


def test_the_replays_visit_what_they_claim():
    want = {"new", "last_live_of_partial_split", "wave", "workgroup", "different_splits"}
    for t in [x for x in HOST_SHAPES if x[0] == "hh" and x[1] == BF and x[4] <= 1290]:
        notes = set()
        for c in E.cases_of(t):
            sim = E.Sim(c)
            evicted = []
            for i in range(c.steps):
                st = sim.step(i)
                evicted.append(st["idx"][0])
            notes |= sim.notes
            assert "new" in sim.notes, c.id
            if c.fill == "minus3" and c.hist == "pairs":  # the empty slots are taken first (with a run of zeros a live slot at 0 with a
                # lower index goes before them: the contract's tie); the count goes up by three, then evictions start
                assert int(sim.cts[0]) == c.S and evicted[:3] == [c.S - 3, c.S - 2, c.S - 1]
            if c.fill == "brim" and c.hist == "pairs":  # the walk through the planted ties, in index order
                s = sorted(c.planted)
                k = min(len(s), c.w + 1)
                assert evicted[:k] == s[:k], (c.id, evicted, s)
        one_split = E.plan(t[3], t[2], t[4], t[5], t[1])["n_split"] == 1
        miss = want - notes - ({"different_splits"} if t[3] == t[2] or one_split else set())  # (over the shape's three fill levels)
        assert not miss, (t, miss)


# ------------------------------------------------------------------------------------------------ teeth
# one shape of the VALU table per head dim: 16-bit D = 16, 32, 64 and fp32 D = 128
_VALU_MUTANT_SHAPES = (("hh", BF, 2, 8, 515, 16), ("hh", HF, 2, 4, 258, 32), ("hh", BF, 2, 8, 130, 64), ("hh", F32, 2, 4, 67, 128))
_VALU_TAG = {"-D16": "16-bit D = 16", "-D32": "16-bit D = 32", "-D64": "16-bit D = 64", "hh-f32-": "fp32 D = 128"}


def _mutant_cases():
    out = []
    for t in (("hh", BF, 2, 4, 130, 128), ("hh", HF, 3, 12, 130, 128), ("hh", BF, 1, 8, 200, 128), ("hh", BF, 2, 2, 67, 128),
              ("rg", BF, 2, 4, 130, 128), ("hh", BF, 4, 28, 130, 128)) + _VALU_MUTANT_SHAPES:
        out += E.cases_of(t)
    return out


_MUTANT_CASES = _mutant_cases()


def _differs(c, fault):
    """Does the mutant's replay differ from the simulator's anywhere (y or any buffer, at any step)?"""
    a, b = E.Sim(c), E.Sim(c, fault=fault)
    for i in range(c.steps):
        sa, sb = a.step(i), b.step(i)
        if not np.array_equal(E.bits(sa["y"]), E.bits(sb["y"])) or sa["idx"] != sb["idx"]:
            return True
        ba, bb = a.buffers(), b.buffers()
        if any(not np.array_equal(E.bits(ba[k]), E.bits(bb[k])) for k in ba):
            return True
        if not torch.equal(a.K.view(torch.int16), b.K.view(torch.int16)) or not torch.equal(a.V.view(torch.int16), b.V.view(torch.int16)):
            return True
    return False


# which of _MUTANT_CASES reject which mutant (recomputed and asserted: a change of the cases shows up here)
REJECTED_BY = {}


@pytest.mark.parametrize("fault", E.FAULTS)
def test_every_mutant_is_rejected(fault):
    hit = [c.id for c in _MUTANT_CASES if _differs(c, fault)]
    REJECTED_BY[fault] = hit
    print(f"{fault}: rejected by {len(hit)} of {len(_MUTANT_CASES)} cases: {hit}")
    assert hit, f"no case rejects '{fault}'"
    want = {"stale_k": "brim", "stale_v": "brim", "tie_high": "brim", "tie_chunk": "S200-brim", "recent_gt": "brim", "global_off": "brim",
            "denom_live": "sparse", "no_zero": "brim", "stale_hist": "brim", "head_mod": "H2-HQ4", "drop_last": "brim", "no_rescale": "brim",
            "masked_weight": "sparse", "cts_skip": "minus3", "dup_tail": "S515-brim-pairs-D16"}[fault]
    assert any(want in x for x in hit), (fault, want, hit)
    if fault in E._ATTN_FAULTS:  # the faults of the attention: rejected at every head dim of the VALU pass
        for tag, what in _VALU_TAG.items():
            assert any(tag in x for x in hit), f"'{fault}' is not rejected at {what}: {hit}"


# ------------------------------------------------------------------------------------------------ what the older comparison lets through
def _gaussian_step(fault, S=4096, H=1, HQ=4, seed=0, D=128, rps=64):
    """One decode step on N(0, 1) inputs over a brim-full cache (the inputs of test_fused_step_equals_three_calls), evaluated by
    attend_dense with and without the fault.  stale_k / stale_v: the inserted row is read from the cache as it stood."""
    g = torch.Generator().manual_seed(17 + seed)
    K = torch.randn(H, S, D, generator=g).to(BF).double()
    V = torch.randn(H, S, D, generator=g).to(BF).double()
    q = torch.randn(HQ, D, generator=g).to(BF).double()
    k1 = torch.randn(H, D, generator=g).to(BF).double()
    v1 = torch.randn(H, D, generator=g).to(BF).double()
    slot = 77
    Kn, Vn = K.clone(), V.clone()
    Kn[:, slot], Vn[:, slot] = k1, v1
    mask = torch.ones(H, S, dtype=torch.bool)
    ref = E.attend_dense(q, Kn, Vn, mask, E.P.default_scale(D), BF, rps, HQ // H)
    got = E.attend_dense(q, K if fault == "stale_k" else Kn, V if fault == "stale_v" else Vn, mask, E.P.default_scale(D), BF, rps, HQ // H,
                         fault if fault in ("drop_last", "no_rescale", "dup_tail") else None)
    return ref, got


OLD_COMPARISON_ACCEPTS = frozenset({"stale_k"})


def test_old_gaussian_comparison_accepts_these_mutants():
    """1e-3 + two roundings of the output on y, N(0, 1) inputs, brim-full, S = 4096 (the headline shape of test_gpu_fused_step): the new
    token scored from the stale K row moves one probability of ~1 / S and passes at every seed; the stale V row, a dropped split and
    a merge without rescale do not pass.  (The fused forms share their streaming pass, plan and combine order with the three-call
    path they are compared with: a fault they share changes nothing there, whatever the limit.)"""
    accepted = set()
    for fault in ("stale_k", "stale_v", "drop_last", "no_rescale"):
        ok = True
        for seed in range(3):
            (yr, _, _), (yg, _, _) = _gaussian_step(fault, seed=seed)
            ok = ok and float((yg - yr).abs().max()) <= 1e-3 + 2 * E.ULP[BF] * float(yr.abs().max())
        if ok:
            accepted.add(fault)
    assert accepted == OLD_COMPARISON_ACCEPTS, sorted(accepted)


OLD_COMPARISON_ACCEPTS_D64 = frozenset({("stale_k", 0), ("stale_k", 2), ("stale_v", 0), ("dup_tail", 1)})  # (mutant, seed)


def test_old_gaussian_comparison_accepts_these_mutants_at_d64():
    """The same comparison at head_dim 64, S = 4099 in splits of 128 rows (the VALU pass's rpi at 16-bit D = 64; the last split holds
    three rows).  The outputs are smaller here and the errors a few spacings of bf16 either side of the limit, so the verdict is
    recorded per seed: the stale K row passes at two seeds of three, the stale V row and the clamped copy of the ragged split's last
    row counted as live (dup_tail) at one; a dropped split and a merge without rescale pass at none.  Every one of them is rejected
    by an exact case at D = 64 (test_every_mutant_is_rejected)."""
    accepted = set()
    for fault in ("stale_k", "stale_v", "drop_last", "no_rescale", "dup_tail"):
        for seed in range(3):
            (yr, _, _), (yg, _, _) = _gaussian_step(fault, S=4099, seed=seed, D=64, rps=128)
            if float((yg - yr).abs().max()) <= 1e-3 + 2 * E.ULP[BF] * float(yr.abs().max()):
                accepted.add((fault, seed))
    assert accepted == OLD_COMPARISON_ACCEPTS_D64, sorted(accepted)


# ------------------------------------------------------------------------------------------------ B. ramp steps
_RAMP_HOST = [(sh, dt, v) for sh in E.RAMP_SHAPES + E.RAMP_VALU_SHAPES if sh[2] <= 4160 for dt in (BF, HF) for v in E.RAMP_VARIANTS]


def test_ramp_constructions_and_the_reference():
    """The shapes of the ramp do what they are for, and tests/attn_ref.decode_ref agrees with the float64 evaluation of the helper."""
    import attn_ref as A

    for (sh, dt, v) in _RAMP_HOST:
        if sh[2] > 1290:
            continue
        for c in E.ramp_cases(sh, dt, v):
            e = E.ramp_reference(c)
            yr, pr, gr = A.decode_ref(c.q, e["K"][None], e["V"][None], mask=torch.from_numpy(e["mask"].astype(bool))[None, :, None, :],
                                      scale=c.scale, dtype=dt)
            assert float((yr - e["y"]).abs().max()) <= 1e-12 and float((pr - e["p"]).abs().max()) <= 1e-12, c.id
            assert float((gr - torch.from_numpy(e["gm"])).abs().max()) <= 1e-12, c.id
            rps, ns = c.plan["rows_per_split"], c.plan["n_split"]
            live = torch.from_numpy(e["mask"].astype(bool))
            sc = e["scores"].view(c.H, c.R, c.S)
            m = torch.stack([sc[:, :, i * rps:(i + 1) * rps].max(dim=-1).values for i in range(ns)], dim=-1)  # [H, R, splits]
            top = m.max(dim=-1).values
            arg = sc.argmax(dim=-1)
            if v == "up" and c.fill == "brim" and ns > 1:
                run = torch.cummax(m, dim=-1).values  # the running maximum moves at (nearly) every merge of full splits
                full = ns - 1 if c.S % rps else ns
                assert full < 2 or float((run[..., 1:full] > run[..., :full - 1]).double().mean()) >= 0.7, c.id
                assert bool((top > m[..., 0] + (8 if full > 1 else 0)).all()) or full < 2, c.id
            if v == "down" and c.fill == "brim" and ns > 1:
                assert bool((m[..., 0] == top).all()) and bool((m[..., -1] < top - 8).all()), c.id
            if v == "new_max":
                assert bool((arg == torch.from_numpy(e["idx"])[:, None]).all()), c.id
            if v == "last_live":
                s = (c.S - 1) if c.fill == "brim" else (c.T - 1)
                assert bool((arg == s).all()) and (s + 1) % rps != 0 or c.S % rps == 0, c.id
            if v == "steep" and ns > 2 and c.fill == "brim":
                assert int((m < top[..., None] - 110).sum(dim=-1).min()) >= 1, c.id
                assert bool(torch.isfinite(e["y"]).all())
            if c.fill == "sparse" and ns > 2:  # whole splits hold only masked slots
                assert bool((m[..., -1] == float("-inf")).all()), c.id


@pytest.mark.parametrize("shape,dt,variant", _RAMP_HOST, ids=lambda x: E.DT_NAME.get(x, None) or (x if isinstance(x, str) else "-".join(map(str, x))))
def test_oracle_twins_within_the_ramp_bounds(monkeypatch, oracle, shape, dt, variant):
    worst = {}
    with cpu_twin(monkeypatch, oracle):
        for c in E.ramp_cases(shape, dt, variant):
            for form in ("three", "two"):
                _, ry, rn, _, _ = E.run_ramp(c, form, "cpu")
                worst[form] = max(worst.get(form, (0, 0)), (ry, rn))
    print("oracle worst error / bound (y, history increment):", worst)
