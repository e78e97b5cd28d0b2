"""tests/prefill_exact.py on the CPU: the known answers hold for the float64 reference (attn_ref.prefill_ref) and for the oracle's
cc_prefill_attn_bands, the constructions have the properties their docstring claims, and the comparisons reject every mutant of
prefill_exact.FAULTS — while the Gaussian inputs and absolute limits of the older suites accept several of them (recorded below)."""
import numpy as np
import pytest
import torch

import attn_ref as A
import prefill_exact as P

BF, HF, F32 = P.BF, P.HF, P.F32


def _chunks(cases, n):
    return [cases[i::n] for i in range(n)]


_HOST = P.host_selector_cases()


def test_group_mean_quotient_rounds_alike_from_fp32_and_float64():
    for dt in (BF, HF, F32):
        for Rg in range(1, 9):
            for n in range(Rg + 1):
                assert P.gm_value(n, Rg, dt, torch.float64) == P.gm_value(n, Rg, dt, torch.float32), (dt, n, Rg)


def test_selector_cases_have_their_gap_and_exact_sums():
    assert len(_HOST) > 150
    seen = set()
    every = _HOST + [c for c in P.valu_cases() if c.L > 512]
    for dt in (BF, HF):
        every += P.kstat_cases(dt) + [c for L, H in ((2085, 1), (4133, 1), (8231, 1), (2085, 8)) for c in P.mfma_long_cases(dt, L, H)]
    for c in every:
        assert c.gap >= 40, (c.id, c.gap)
        assert P.selector_fig(c) < 1e-12, c.id
        assert float(c.v.double().abs().min()) >= 2.0 ** -6
        # every q . k is amp * n, |n| <= D <= 256: exact in the dtype; ascending and descending fp32 dots equal the float64 one
        q, k = c.q[0, -1].double(), c.k[0].double()
        d64 = (k * q).sum(dim=1)
        asc = torch.zeros(c.L, dtype=F32)
        desc = torch.zeros(c.L, dtype=F32)
        for d in range(c.D):
            asc = asc + (k[:, d] * q[d]).float()
            desc = desc + (k[:, c.D - 1 - d] * q[c.D - 1 - d]).float()
        assert torch.equal(asc.double(), d64) and torch.equal(desc.double(), d64) and torch.equal(A.rnd(d64, c.dt), d64), c.id
        P.expected_selector(c)  # (asserts that the fp32 sums of dtype(n / R) are exact at this L)
        seen.add((c.sel[0][-1] == c.L - 1, c.R, c.D))
    assert {r for _, r, _ in seen} >= {1, 2, 3, 4, 7, 8} and {d for _, _, d in seen} >= {16, 64, 80, 128, 256}


@pytest.mark.parametrize("part", range(4))
def test_reference_and_oracle_return_the_selector_answers(oracle, part):
    """y bit for bit, planes within the case's own figure R L exp(-gap)."""
    bad = []
    for c in _chunks(_HOST, 4)[part]:
        ref = A.prefill_ref(c.q[None], c.k[None], c.v[None], scale=c.scale, dtype=c.dt, obs_len=c.ol, bands=c.bands)
        got = dict(y=ref["y"].to(c.dt), colsum=ref["colsum"].numpy(), obs=ref["obs"].numpy(),
                   bands=np.stack([ref["bands"][b].numpy() for b in c.bands]) if c.bands else None)
        bad += ["prefill_ref " + b for b in P.check_selector(c, got)]
        rc, got = P.run_oracle(oracle, c, "all")
        assert rc == 0, c.id
        bad += ["oracle " + b for b in P.check_selector(c, got)]
    assert not bad, "\n".join(bad[:20])


def _ramps():
    return P.mfma_ramp_cases(BF) + P.mfma_ramp_cases(HF) + P.valu_ramp_cases()


def test_ramp_construction():
    for c in _ramps():
        H, Rg, L, D = c.H, c.R, c.L, c.D
        q, k = c.q.double().view(H, Rg, L, D), c.k.double()
        d64 = torch.einsum("hrid,hsd->hris", q, k)
        asc = torch.zeros_like(d64, dtype=F32)
        desc = torch.zeros_like(d64, dtype=F32)
        for d in range(D):
            asc = asc + torch.einsum("hri,hs->hris", q[..., d], k[..., d]).float()
            desc = desc + torch.einsum("hri,hs->hris", q[..., D - 1 - d], k[..., D - 1 - d]).float()
        assert torch.equal(asc.double(), d64) and torch.equal(desc.double(), d64), c.id
        assert float(d64.abs().max()) < 2 ** 24 and np.log2(c.scale) == round(np.log2(c.scale))
        d = P.dense_ref(c, want_p=True)
        ref, _ = P.ramp_reference(c)
        assert np.abs(d["colsum"] - ref["colsum"]).max() <= 1e-9 and float((d["y"].double() - ref["y"]).abs().max()) <= 1e-9, c.id
        top = d["p"].max(dim=-1).values.reshape(-1, L)
        if c.variant == "up":
            if L >= 400:
                assert float((P.lazy_raises(c) >= 3).double().mean()) > 0.5, c.id
            assert float((top < 0.9).double().mean()) > 0.5, (c.id, float((top < 0.9).double().mean()))
        elif c.variant == "down":
            assert int(P.lazy_raises(c).sum()) == 0
            if L >= 400:
                late = float(d["p"][..., L - 1, L - 64:].max())  # the maximum sits in the first tile, the late tiles underflow
                assert late < 1e-30 and (late == 0.0 or c.dt != HF) and int(d["p"][..., L - 1, :].argmax(dim=-1).max()) < 32, c.id
        else:
            spike = int(c.k[0, :, 0].double().argmax())
            assert spike >= 3 * L // 4 and float(top[:, L - 1].min()) > 0.99


def test_ramp_oracle_within_the_device_bounds(oracle):
    worst = {}
    for c in _ramps():
        rc, got = P.run_oracle(oracle, c, "all")
        assert rc == 0
        bad, ratio = P.check_ramp(c, got)
        assert not bad, "\n".join(bad)
        for n, r in ratio.items():
            worst[n] = max(worst.get(n, 0.0), r)
        # the single pass in float64 (unnormalised rounding, lazy maximum) stays inside the y contract as well
        ref, bound = P.ramp_reference(c)
        assert float((P.flash_ref_y(c) - ref["y"]).abs().max()) <= bound["y"], c.id
    print("oracle worst error / bound:", worst)


_MUTANT_CASES = P.mutant_cases()


def _mutant_rejected(fault):
    for c in _MUTANT_CASES:
        if P.check(c, P.dense_ref(c, fault, nwg=2)):
            return c.id
    return None


def test_unmutated_dense_reference_passes_every_mutant_case():
    for c in _MUTANT_CASES:
        assert not P.check(c, P.dense_ref(c)), c.id


@pytest.mark.parametrize("fault", P.FAULTS)
def test_every_mutant_is_rejected(fault):
    assert _mutant_rejected(fault) is not None, f"no case of mutant_cases() rejects '{fault}'"


# what test_gpu_parity's Gaussian inputs (N(0, 1); bf16, HQ = 4, H = 1, D = 128, L in {130, 300, 400}, obs_len 16, one band of 32) with the
# limits of the older suites (column / band sums 5e-2, window mean 4e-3, absolute) let through at EVERY one of the three lengths: both
# window mutants (they move the mean by 0.5e-3 .. 2e-3), both rescale mutants (no row's maximum ever rises by more than kLazy there) and
# head_mod (the identity at H = 1).  A band one query too wide (4.9e-2) and the live padding pass at L = 400 alone.
OLD_LIMITS_ACCEPT = frozenset({"window_long", "window_short", "no_rescale", "l_only_rescale", "head_mod"})


def test_old_gaussian_inputs_and_limits_accept_these_mutants():
    accepted = set(P.FAULTS)
    for L in (130, 300, 400):
        c = P.gaussian_case(L)
        ref = P.dense_ref(c)
        accepted = {f for f in accepted if P.old_limits_accept(c, P.dense_ref(c, f, nwg=2), ref)}
    assert {"window_long", "window_short"} <= accepted
    assert accepted == OLD_LIMITS_ACCEPT, sorted(accepted)
