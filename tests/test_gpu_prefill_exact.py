"""cc_prefill_attn_bands on the known-answer inputs of tests/prefill_exact.py (held to the float64 reference and the oracle, and shown
to reject every mutant, by tests/test_prefill_exact_host.py): the VALU kernels, the two-pass and the single-pass matrix-core kernels,
and — in one child process — the opt-in K-stationary form (CC_PREFILL_KSTAT=1).

Selector inputs: y bit for bit, every side plane within the case's own R L exp(-gap) (< 1e-12).  Ramp inputs: y within the contract,
every element of every side plane within its derived bound; the worst error / bound per path is reported through `audit`.  The
library is called through raw pointers (prefill_exact.run_device): q, k, v, y and the side outputs are views into NaN-filled buffers
with margins on both sides (K and V: 32 NaN rows behind row L - 1), the workspace is NaN-filled between guard bytes; afterwards the
margins and guards are intact, the inputs unchanged, the return code 0.

Shapes: the smallest that reach each branch — the matrix-core threshold (L = 64) and ragged tiles, a 16-row window before, on and
after a tile edge (L = 79 / 80 / 81), H % 8 == 0 (the XCD remap), the second and third rounds of the persistent loops (L = 2085, 4133,
8231), 0 / 1 / 2 / 4 bands (the NB = 0, 1, -1 instantiations) of widths 1 .. L + 5, obs_len 0 .. L + 3; below the threshold and in
the other geometries the VALU path (f32, D = 16 .. 256, R = 1 .. 8, the second loop of its 32 workgroups above L = 256).
Untested: non-finite inputs; the K-stationary form's segment doubling above 32768 tokens (more than 64 query segments)."""
import json
import os
import subprocess
import sys

import pytest
import torch

import prefill_exact as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, HF, F32 = P.BF, P.HF, P.F32
_DT = pytest.mark.parametrize("dt", (BF, HF), ids=lambda d: P.DT_NAME[d])


def path_of(c, want):
    if P.matrix_core(c):
        return "single-pass" if want == "none" else "two-pass"
    return "VALU"


def _run(c, want, ws=None):
    rc, got = P.run_device(c, want, ws)
    assert rc == 0, f"{c.id} ({want}): device -> {rc}"
    return got


def _exact(cases, wants=("none", "all")):
    bad = []
    for c in cases:
        for want in wants:
            bad += [f"[{want}: {path_of(c, want)}] {b}" for b in P.check_selector(c, _run(c, want))]
    assert not bad, f"{len(bad)} failures\n" + "\n".join(bad[:12])


def _ramps(cases, audit, wants=("none", "all")):
    bad, worst = [], {}
    for c in cases:
        for want in wants:
            b, ratio = P.check_ramp(c, _run(c, want))
            bad += [f"[{want}: {path_of(c, want)}] {x}" for x in b]
            w = worst.setdefault(path_of(c, want), {})
            for n, r in ratio.items():
                w[n] = max(w.get(n, 0.0), r)
    for path, w in sorted(worst.items()):
        audit(f"ramp inputs, {path}: worst error / bound " + ", ".join(f"{n} {r:.3f}" for n, r in sorted(w.items())))
    assert not bad, f"{len(bad)} failures\n" + "\n".join(bad[:12])


# ------------------------------------------------------------------------------------------------ matrix-core path
@_DT
@pytest.mark.parametrize("H", (1, 3))
def test_mfma_short_lengths(dt, H):
    cases = [c for c in P.mfma_short_cases(dt) if c.H == H]
    assert {c.L for c in cases} == set(P.MFMA_SHORT_L)
    _exact(cases)


@_DT
def test_mfma_one_side_output_alone(dt):
    """colsum only and obs only, once at every short length."""
    seen = set()
    for c in P.mfma_short_cases(dt):
        if c.H == 1 and c.L not in seen:
            seen.add(c.L)
            _exact([c], ("colsum", "obs"))


@_DT
def test_mfma_xcd_remap(dt):
    cases = [c for c in P.mfma_short_cases(dt) if c.H % 8 == 0]
    assert {c.H for c in cases} == {8, 16}
    _exact(cases)


@_DT
def test_mfma_band_sets_and_window_lengths(dt):
    cases = P.mfma_band_obs_cases(dt)
    assert {len(c.bands) for c in cases} == {0, 1, 2, 4} and {c.obs_len for c in cases} == {0, 1, 16, 32, 33, 47, 97, 100}
    _exact(cases, ("all",))


@_DT
@pytest.mark.parametrize("L,H", ((2085, 1), (4133, 1), (8231, 1), (2085, 8)))
def test_mfma_further_rounds_of_the_persistent_loops(dt, L, H):
    _exact(P.mfma_long_cases(dt, L, H))


@_DT
def test_mfma_ramp(dt, audit):
    _ramps(P.mfma_ramp_cases(dt), audit)


# ------------------------------------------------------------------------------------------------ VALU path
@pytest.mark.parametrize("dt", (BF, HF, F32), ids=lambda d: P.DT_NAME[d])
def test_valu_selector(dt):
    cases = [c for c in P.valu_cases() if c.dt == dt]
    assert cases and all(path_of(c, "all") == "VALU" for c in cases)
    _exact(cases)


def test_valu_ramp(audit):
    _ramps(P.valu_ramp_cases(), audit)


# ------------------------------------------------------------------------------------------------ one workspace, three calls
def test_workspace_reuse_leaks_no_stale_partial_planes():
    """L = 2085, then L = 97, then L = 2085 with another selector on ONE workspace that is not refilled in between."""
    long_ = P.mfma_long_cases(BF, 2085)
    a, c3 = long_[1], long_[2]
    b = P.selector_case("reuse-L97", BF, 4, 1, 97, 128, "uniform", seed=5, obs_len=33, bands=(1, 33))
    ws = P.new_workspace(P.workspace_bytes(a))
    for c in (a, b, c3):
        bad = P.check_selector(c, _run(c, "all", ws))
        assert not bad, "\n".join(bad[:6])


# ------------------------------------------------------------------------------------------------ the wrapper
@pytest.mark.parametrize("L", (33, 97), ids=("valu", "mfma"))
def test_prefill_attention_wrapper(L):
    """attention_utils.prefill_attention: the obs_len clamp, the band dictionary, the no-side-output form."""
    from cold_compress_amd.attention_utils import prefill_attention

    c = P.selector_case(f"wrap-L{L}", BF, 4, 1, L, 128, "back", 32, seed=9, obs_len=L + 3, bands=(1, 33))
    q, k, v = (t[None].to(DEV) for t in (c.q, c.k, c.v))
    y, none = prefill_attention(q, k, v, return_attn=False, obs_len=c.obs_len, bands=c.bands)
    torch.cuda.synchronize()
    assert none is None
    assert not P.check_selector(c, dict(y=y[0].cpu()))
    y, summ = prefill_attention(q, k, v, return_attn=True, obs_len=c.obs_len, bands=c.bands)
    torch.cuda.synchronize()
    assert summ.obs_len == L and sorted(summ.bands) == [1, 33]
    got = dict(y=y[0].cpu(), colsum=summ.colsum.cpu().numpy(), obs=summ.obs_mean.cpu().numpy(),
               bands=torch.stack([summ.bands[b] for b in c.bands]).cpu().numpy())
    bad = P.check_selector(c, got)
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ the K-stationary form
def _kstat_child():
    """Run in a child process with CC_PREFILL_KSTAT=1 (the launcher reads it once): one JSON line per case."""
    for dt in (BF, HF):
        cases = P.mfma_short_cases(dt) + P.mfma_band_obs_cases(dt) + P.kstat_cases(dt) + P.mfma_long_cases(dt, 2085) + P.mfma_ramp_cases(dt)
        for c in cases:
            rc, got = P.run_device(c, "all")
            if c.family == "sel":
                bad, ratio = P.check_selector(c, got), {}
            else:
                bad, ratio = P.check_ramp(c, got)
            print(json.dumps(dict(id=c.id, rc=rc, bad=bad, ratio=ratio)), flush=True)
    print("kstat child done", flush=True)


def test_k_stationary_form_in_a_child_process(audit):
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, CC_PREFILL_KSTAT="1")
    code = f"import sys; sys.path[:0] = [{here!r}, {os.path.dirname(here)!r}]; import test_gpu_prefill_exact as M; M._kstat_child()"
    r = subprocess.run([sys.executable, *(["-s"] if sys.flags.no_user_site else []), "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "kstat child done" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    rows = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(rows) > 150 and {513, 640, 1153} <= {int(x["id"].split("-L")[1].split("-")[0]) for x in rows}
    bad = [b for x in rows for b in ([f"{x['id']}: device -> {x['rc']}"] if x["rc"] else []) + x["bad"]]
    worst = {}
    for x in rows:
        for n, v in x["ratio"].items():
            worst[n] = max(worst.get(n, 0.0), v)
    audit("ramp inputs, K-stationary: worst error / bound " + ", ".join(f"{n} {v:.3f}" for n, v in sorted(worst.items())))
    assert not bad, f"{len(bad)} failures\n" + "\n".join(bad[:12])
