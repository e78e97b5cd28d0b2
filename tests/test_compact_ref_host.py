"""CPU checks of tests/compact_ref.py, the references tests/test_gpu_compact_shapes.py holds the compaction and bookkeeping kernels to:
every reference against the oracle's twin, bit for bit, on every fuzz case the GPU file runs; the sensitivity of the comparison
(plausible kernel mistakes applied to a correct output must each be detected by compact_ref.same, the comparison the GPU file uses);
and the refusal table against the oracle's twins."""
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import compact_ref as R
from test_window_sums import exact_round


def _compare(c, want, got, who):
    for n, w in want.items():
        assert n in got, f"{c.id}: {who} returned no '{n}'"
        assert R.same(w, got[n]), f"{c.id}: '{n}' reference vs {who}: {R.first_diffs(w, got[n])}"


def _chain(c):
    """A ring case is the first of c.steps successive updates; every other case stands alone."""
    return getattr(c, "steps", 1)


CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cold_compress_amd", "csrc")


@pytest.mark.parametrize("fname", sorted(R.MIRRORED_LINES))
def test_grid_caps_are_the_launchers(fname):
    """The grid caps the second-pass shapes of the GPU file are sized against are copied from these launcher lines."""
    src = " ".join(open(os.path.join(CSRC, fname)).read().split())
    for line in R.MIRRORED_LINES[fname]:
        assert " ".join(line.split()) in src, f"{fname} no longer contains: {line}"


# ------------------------------------------------------------------------------------------------ reference == oracle twin
@pytest.mark.parametrize("op", sorted(R.FUZZ))
def test_reference_equals_oracle_twin_on_every_fuzz_case(oracle, op):
    n, dts = 0, set()
    for c in R.FUZZ[op]():
        for step in range(_chain(c)):
            rc, got = R.run_oracle(oracle, c)
            assert rc == 0, f"{c.id}: oracle -> {rc}"
            want = R.reference(c)
            assert set(want) <= set(R.OPS[op].outputs)
            _compare(c, want, got, "oracle")
            if step + 1 < _chain(c):
                c = R.ring_next(c, got, c.gen)
        n += 1
        dts.add(c.code)
    assert n >= 40 and dts == {0, 1, 2}, (n, dts)


def test_fuzz_reaches_both_gather_kernels_and_every_listed_edge():
    rows = list(R.cases_gather_rows())
    es = lambda c: 4 if c.code == 0 else 2  # noqa: E731
    assert {c.code for c in rows if (c.D * es(c)) % 16} == {0, 1, 2} and {c.code for c in rows if (c.D * es(c)) % 16 == 0} == {0, 1, 2}
    assert {1} <= {c.K for c in rows} and any(c.K == c.L and c.L > 1 for c in rows) and {c.Hk == 1 for c in rows} == {True, False}
    sk = list(R.cases_snapkv_priority())
    assert any(c.obs_len == 0 for c in sk) and any(c.obs_len == c.L for c in sk) and any(c.obs_len > c.L for c in sk)
    assert any(c.g == 0 for c in sk) and any(c.g >= c.L for c in sk) and any(c.L < 5 for c in sk)
    for gen in (R.cases_hh_update, R.cases_ring_update):
        cs = list(gen())
        assert any(c.T == 0 for c in cs) and any(c.T == c.S and c.S > 1 for c in cs) and any(0 < c.T < c.S for c in cs)
    assert {c.t["counter"] is None for c in R.cases_hh_update()} == {True, False}
    assert {c.tracked for c in R.cases_ring_update()} == {True, False}
    assert {c.t["input_pos"] is None for c in R.cases_colsum_to_mean()} == {True, False}
    assert {c.negate for c in R.cases_row_l2_norm()} == {0, 1} and any(R.passes(c.H * c.N, R.CAP_ROW_NORM) == 2 for c in R.cases_row_l2_norm())
    assert any(c.band >= c.Lq for c in R.cases_attn_bandsum()) and any(c.band < c.Lq for c in R.cases_attn_bandsum())
    al = list(R.cases_analysis_loss())
    assert {(c.S, c.Hp) for c in al} >= {(S, Hp) for S in R.ANALYSIS_S for Hp in R.ANALYSIS_HP}
    ctr = [(int(c.t["ctr"][0]), c.cap) for c in al]
    assert any(v == 0 for v, _ in ctr) and any(v == cap - 1 and v > 0 for v, cap in ctr) and any(v == cap for v, cap in ctr)
    assert any(v < 0 for v, _ in ctr) and any(bool((c.t["pos"] == -1).any()) for c in al) and any(bool((c.t["pos"] != -1).all()) for c in al)


@pytest.mark.parametrize("dtype", R.DTYPES)
def test_round_once_is_the_exact_rounding(dtype):
    """round_once (vectorised, float64 in) against exact rational rounding, on sums of grid values and on ties."""
    rng = np.random.default_rng(3)
    g = R.GRID_BITS[dtype]
    vals = [int(v) for v in rng.integers(0, 1 << (g + 3), 300)] + [int(v) for v in rng.integers(0, 1 << 12, 100)]
    p = R.FMT[dtype][0]
    vals += [(1 << p) + 1, ((1 << p) + 1) << 1 | 1, (1 << (p + 1)) + 2, (1 << (p + 1)) + 6, 3 << p | 1 << (p - 2), 0, 1]  # ties both ways
    x = np.array([v * 2.0 ** -g for v in vals])
    got = R.round_once(x, dtype)
    for v, r in zip(vals, got):
        assert float(r) == exact_round(Fraction(v, 1 << g), dtype), v


# ------------------------------------------------------------------------------------------------ sensitivity
def _further(x, by):
    """the element one grid-stride further: output i holds what belongs at i + by."""
    return torch.roll(x.reshape(-1), -by).view(x.shape)


def _with(c, **t):
    return R.reference(c.replace(t=t))


def _loss_of(c, sums):
    """analysis_loss' loss from per-head sums a wrong kernel would have formed (float64 [Hp])."""
    dt = c.t["attn"].dtype
    r = lambda x: x.to(dt).double()  # noqa: E731
    return (r(1.0 - r(sums)).sum() / c.Hp).to(dt)


def _corruptions(op):
    """(case, [(name, outputs a kernel with that mistake would leave)]) — each list entry maps output names to tensors; outputs it does
    not name are correct."""
    rng, gen = np.random.default_rng(17), torch.Generator().manual_seed(17)
    if op == "gather_rows":
        c = R.gather_rows_case("c", R.BF, 3, 40, 17, 6, 3, rng, gen)
        keep = c.t["keep"]
        return c, [("the element one grid-stride further", dict(dst=_further(R.reference(c)["dst"], 256))),
                   ("head h's keep row used for head h + 1", _with(c, keep=torch.roll(keep, 1, 0))),
                   ("head 0's keep row for every head", _with(c, keep=keep[:1].expand(3, 17).contiguous())),
                   ("source row stride K instead of L", dict(dst=c.t["src"].reshape(-1, 6)[(torch.arange(3).view(3, 1) * 17 + keep).reshape(-1)].view(3, 17, 6)))]
    if op == "gather_vec":
        c = R.gather_vec_case("c", R.HF, 3, 300, 120, rng, gen)
        return c, [("the element one grid-stride further", dict(dst=_further(R.reference(c)["dst"], 256))),
                   ("head h's keep row used for head h + 1", _with(c, keep=torch.roll(c.t["keep"], 1, 0))),
                   ("the index taken as the value", dict(dst=c.t["keep"].to(R.HF)))]
    if op == "prefill_fill":
        c = R.prefill_fill_case("c", R.HF, 3, 3, 3, 3, 17, 9, 4, rng, gen)
        e = R.reference(c)
        k = c.t["k"].clone()
        k.view(-1)[: 3 * 9 * 4] = c.t["k_val"].reshape(-1)
        pos = e["pos"].clone()
        pos[:, :9] = c.t["pos_val"][0].to(torch.int32)
        mask = e["mask"].clone()
        mask[:] = 1
        cts = c.t["cts"].clone()
        cts[0] += 9
        v = e["v"].clone()
        v[:, 9] = v[:, 8]
        pos2 = e["pos"].clone()
        pos2[:, 8] = R.sentinel(torch.int32)
        return c, [("rows land at slot stride T", dict(k=k)), ("head 0's positions for every head", dict(pos=pos)),
                   ("mask set on all S slots", dict(mask=mask)), ("only cache_cts[0] bumped", dict(cts=cts)),
                   ("one slot beyond T written", dict(v=v)), ("the last position left out", dict(pos=pos2))]
    if op == "analysis_loss":
        c = R.analysis_case("c", R.F32, 8, 3000, 3100, 0.3, 2, 5, rng, last_units=1)
        e = R.reference(c)
        sub = e["sub"].double()
        pos0 = c.t["pos"].clone()
        first = torch.gather(c.t["attn"], 1, torch.where(pos0 == -1, torch.zeros_like(pos0), pos0).long())
        s = torch.arange(3000)

        def losses(v, at=2):
            out = c.t["losses"].clone()
            out[at] = v
            return out

        full = c.replace(t=dict(ctr=torch.tensor([5], dtype=torch.int32)))
        lf = R.reference(full)["losses"].clone()
        lf[4] = e["losses"][2]
        return c, [("-1 reads column 0", dict(sub=first)),
                   ("slots from 1024 on left out of the sum", dict(losses=losses(_loss_of(c, sub[:, :1024].sum(1))))),
                   ("only the first wave's partial folded", dict(losses=losses(_loss_of(c, sub[:, (s % 1024) < 64].sum(1))))),
                   ("the loss of head 0 only", dict(losses=losses(_loss_of(c, sub[:1].sum(1).expand(8))))),
                   ("written at the slot after the counter", dict(losses=losses(e["losses"][2], at=3))),
                   ("counter not incremented", dict(ctr=c.t["ctr"].clone())),
                   ("counter at cap: stored in the last slot", dict(losses=lf, _base=full))]
    if op == "hh_update":
        c = R.hh_update_case("c", R.BF, 3, 300, 120, True, rng, gen)
        e = R.reference(c)
        den = c.t["denom"].clone()
        den[:, :120] += 1
        num = c.t["num"].clone()
        num[:, :120] = (num[:, :120].float() + c.t["attn"].float()).double()
        num2 = c.t["num"].clone()
        num2.view(-1)[: 3 * 120] += c.t["attn"].double().reshape(-1)
        return c, [("denom bumped only below T", dict(denom=den)), ("counter untouched", dict(counter=c.t["counter"].clone())),
                   ("accumulated in fp32", dict(num=num)), ("history row stride T instead of S", dict(num=num2)),
                   ("the element one grid-stride further", dict(denom=_further(e["denom"], 256)))]
    if op == "colsum_to_mean":
        c = R.colsum_to_mean_case("c", R.BF, 3, 300, True, rng, gen)
        cs, L = c.t["colsum"], 300
        den = (L - c.t["input_pos"]).float().view(1, L)
        return c, [("L - p off by one", dict(out=(cs.to(R.BF).float() / (den + 1)).to(R.BF))),
                   ("column sum not rounded to the dtype first", dict(out=(cs / den).to(R.BF))),
                   ("input_pos ignored", _with(c, input_pos=None))]
    if op == "snapkv_priority":
        c = R.snapkv_case("c", R.F32, 3, 300, 16, 4, gen)
        obs, L = c.t["obs"], 300
        t = torch.arange(L)
        pad = torch.zeros(3, L + 4)
        pad[:, 2:L + 2] = obs
        forced = (t >= L - 16) | (t < 4)

        def fin(v, f=forced):
            v = v.clone()
            v[:, f] = 1.0
            return dict(out=v)

        cnt = (torch.clamp(t + 2, max=L - 1) - torch.clamp(t - 2, min=0) + 1).float()
        a4 = pad[:, 0:L] + pad[:, 1:L + 1] + pad[:, 2:L + 2] + pad[:, 3:L + 3]
        a5 = a4 + pad[:, 4:L + 4]
        desc = pad[:, 4:L + 4] + pad[:, 3:L + 3] + pad[:, 2:L + 2] + pad[:, 1:L + 1] + pad[:, 0:L]
        free = R.snapkv_case("c", R.F32, 3, 300, 0, 0, gen).replace(t=dict(obs=obs))  # nothing forced: the row's ends show
        return c, [("window clipped one short", fin(a4 / torch.clamp(cnt - 1, min=1))),
                   ("divided by 5 at the row's ends", dict(out=a5 / 5.0, _base=free)),
                   ("summed in descending order", fin(desc / cnt)),
                   ("observation window one short", fin(a5 / cnt, (t > L - 16) | (t < 4))), ("one global token short", fin(a5 / cnt, (t >= L - 16) | (t < 3)))]
    if op in ("attn_colsum", "attn_bandsum"):
        c = R.attn_sum_case(op, "c", R.BF, 3, 20, 300, 3, gen)
        e = R.reference(c)
        a = c.t["attn"]
        out = [("the element one grid-stride further", dict(out=_further(e["out"], 256))),
               ("query and head axes swapped", _with(c, attn=a.reshape(-1)[: 3 * 300 * 20].view(20, 3, 300).transpose(0, 1).contiguous()))]
        if op == "attn_colsum":
            out += [("last query row skipped", dict(out=R.ref_attn_colsum(c.replace(t=dict(attn=a[:, :-1].contiguous())))["out"])),
                    ("summed in descending order", _with(c, attn=a.flip(1).contiguous()))]
        else:
            out += [("band one wider", R.reference(c.replace(band=4))), ("band one short", R.reference(c.replace(band=2))),
                    ("band starts at q = s + 1", _with(c, attn=torch.cat([a[:, 1:], torch.zeros_like(a[:, :1])], 1).contiguous()))]
        return c, out
    if op == "row_l2_norm":
        c = R.row_l2_norm_case("c", R.F32, 3, 300, 24, 1, gen)
        e = R.reference(c)
        x = c.t["x"].float().reshape(-1, 24)
        seq = torch.zeros(900)
        for d in range(24):
            seq = seq + x[:, d] * x[:, d]
        return c, [("plain sequential sum of squares", dict(out=(-torch.sqrt(seq)).view(3, 300))), ("negate ignored", R.reference(c.replace(negate=0))),
                   ("the row one grid-stride further", dict(out=_further(e["out"], 128))),
                   ("elements from 16 on left out", _with(c, x=torch.cat([c.t["x"][..., :16], torch.zeros(3, 300, 8)], -1)))]
    if op == "ring_update":
        c0 = R.ring_case("c", R.BF, 2, 100, 3, 100, 4, True, gen)
        st = R.reference(c0)  # warm the ring: four full updates, so that the fifth (T < S) overwrites live entries everywhere
        for _ in range(3):
            st = R.reference(R.ring_next(c0, dict(st, wacc=c0.t["wacc"]), gen))
        c = R.ring_next(c0.replace(T=60), dict(st, wacc=c0.t["wacc"]), gen)
        e = R.reference(c)
        W, ctr = 3, int(c.t["counter"][0])
        wrong_slot = c.t["num"].clone()
        wrong_slot[:, :, (ctr + 1) % W] = 0
        wrong_slot[:, :60, (ctr + 1) % W] = c.t["attn"]
        keep_old = e["num"].clone()
        keep_old[:, 60:, ctr % W] = c.t["num"][:, 60:, ctr % W]
        den = c.t["denom"].clone()
        den[:, :60] += 1
        stale = torch.from_numpy(R.round_once((e["num"].double().sum(2) + c.t["num"][:, :, ctr % W].double()).reshape(-1).numpy(), R.BF))
        return c, [("slot (counter + 1) % W", dict(num=wrong_slot)), ("entries beyond T keep the old value", dict(num=keep_old)),
                   ("denom bumped only below T", dict(denom=den)), ("counter bumped by every workgroup", dict(counter=e["counter"] + 1)),
                   ("counter not bumped", dict(counter=c.t["counter"].clone())),
                   ("the overwritten entry never leaves the window sum", dict(wsum=stale)),
                   ("window sum of the old ring", dict(wsum=R.window_sums(c.t["num"])))]
    raise KeyError(op)


@pytest.mark.parametrize("op", sorted(R.FUZZ))
def test_every_listed_kernel_mistake_is_detected(op):
    c, wrong = _corruptions(op)
    assert len(wrong) >= 3
    for name, outs in wrong:
        assert outs is not None, f"{op}: '{name}' could not be built"
        outs = dict(outs)
        want = R.reference(outs.pop("_base", c))
        assert outs and set(outs) <= set(want), (op, name)
        assert any(not R.same(want[n], outs[n]) for n in outs), f"{op}: '{name}' is not detected"
        for n in outs:  # ... and it is a change of values, not of shape or type
            assert outs[n].shape == want[n].shape and outs[n].dtype == want[n].dtype, (op, name, n)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusal_table_against_the_oracle_twins(oracle):
    table = R.refusals()
    assert len(table) >= 16
    for what, c in table:
        rc, got = R.run_oracle(oracle, c)
        assert rc == R.BAD_ARG, f"{what}: oracle -> {rc}"
        for n, g in got.items():
            assert R.same(g, c.t[n]), f"{what}: the oracle's twin touched '{n}'"
