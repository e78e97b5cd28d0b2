"""The decode step over the fused quantised caches (cache_quant_mode = fused, fp8, uint4, mxfp4) on the device against the known
answers of tests/step_exact.py (Case.quant): every replay as two launches and as one launch, each compared with the SIMULATOR — never
with another form and never with the 16-bit step — bit for bit after every step: y, pos, mask, cache_cts, the history, the K and V
images and the [H, S, 4] parameter words; the device's own decode of its images after the prefill and after the last step.  The
same for the ring policy (cc_decode_step_heavy_hitter_ring_quant) and the hybrid step (cc_decode_step_hybrid_quant_rc) against the
simulators of tests/step_exact_ring.py.  Each
case asserts the launch path it ran on (the plan mirror against cc_decode_step_quant_single_launch, and the XCD-L2 transport where
it is intended).  q, k_new and v_new sit between NaN rows; the status word stays clean.  No assertion has a tolerance."""
import pytest
import torch

import step_exact as E
import step_exact_ring as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
MARGIN = 8  # NaN rows on both sides of q, k_new, v_new
COUNTS = {}  # (family, form) -> elements compared exactly


class Margins:
    """Inputs between NaN rows; check() asserts that the rows are still NaN (nothing may write around an input)."""

    def __init__(self):
        self.bufs = []

    def put(self, name, t):
        rows, D = t.shape
        buf = torch.full((rows + 2 * MARGIN, D), float("nan"), dtype=t.dtype, device=DEV)
        buf[MARGIN:MARGIN + rows] = t.to(DEV)
        self.bufs.append((name, buf, rows))
        return buf[MARGIN:MARGIN + rows]

    def check(self, where):
        for name, buf, rows in self.bufs:
            assert bool(torch.isnan(buf[:MARGIN]).all()) and bool(torch.isnan(buf[MARGIN + rows:]).all()), f"{where}: rows around {name} were written"
        self.bufs = []


@pytest.fixture()
def lib():
    from cold_compress_amd import _abi

    fns = _abi.lib()
    yield fns
    fns["cc_decode_step_set_single_launch"](1)


def _count(family, form, n):
    COUNTS[(family, form)] = COUNTS.get((family, form), 0) + n


def _status_clean(kv, c, where):
    from cold_compress_amd.attention_utils import single_launch_status

    torch.cuda.synchronize()
    if getattr(c, "policy", "hh") == "hh":
        assert kv.step_status(c.HQ) == 0, f"{where}: step_status"
    assert single_launch_status(torch.device(DEV)) == 0, f"{where}: the hand-off's status word is set"


def _path(lib, c, fmt_code):
    """The plan mirror puts the case on its intended path and the device library agrees.
    -> (single launch expected, refused by the device's occupancy query)."""
    from cold_compress_amd.attention_utils import _workspace
    from helpers import DT_CODE

    # (the decode workspace: making it is what probes the device's block placement for the XCD-L2 transport)
    _workspace(lib["cc_decode_attn_workspace_bytes"](c.HQ, c.H, c.S, c.D, DT_CODE[c.dt]), torch.device(DEV))
    nw, nt, xl2 = E.intended(c.dt, c.D, c.H, c.HQ, c.S)
    nt = 1 if nt == 1 else 0  # the step over the images has a single launch with one tile per wave only
    assert (c.plan["nw"], c.plan["nt"]) == (nw, nt), (c.id, c.plan)
    lib["cc_decode_step_set_single_launch"](1)
    dev_one = bool(lib["cc_decode_step_quant_single_launch"](c.HQ, c.H, c.S, c.D, DT_CODE[c.dt], fmt_code))
    if nt == 0:
        assert not dev_one, f"{c.id}: the device library offers a single launch the plan mirror does not know"
        return False, False
    if dev_one and xl2:
        assert lib["cc_decode_step_l2_handoff"]() == 1, f"{c.id}: intended for the XCD-L2 transport, which this device does not offer"
    return True, not dev_one


@pytest.mark.parametrize("shape", E.quant_shape_list(), ids=E.quant_shape_id)
def test_quant_replays_return_the_simulators_answers(lib, shape):
    refused_any = False
    for c in E.quant_cases_of(shape):
        kv = E.make_cache(c, DEV)
        assert kv.fused_quant and kv.k_cache.numel() == 0
        one, refused = _path(lib, c, kv.quant_format)
        refused_any |= one and refused
        forms = [("two", False)] + ([("one", True)] if one and not refused else [])
        for form, is_one in forms:
            where = f"{c.id} [{form}]"
            m = Margins()
            # head-constant policies take the process-wide switch; heavy_hitter the attribute run_replay sets
            lib["cc_decode_step_set_single_launch"](1 if (form == "one" or c.policy == "hh") else 0)
            if c.policy == "hh":
                kv.single_launch = form == "one"
                assert kv.single_launch_active(c.HQ) == is_one, f"{where}: not the intended launch form"
            else:
                from cold_compress_amd.cache import step_is_recoverable

                assert step_is_recoverable(kv, c.HQ) == is_one, f"{where}: not the intended launch form"
            kv, n = E.run_replay(c, form, DEV, put=m.put, sync=torch.cuda.synchronize, kv=kv)
            _count(c.quant, form, n)
            _status_clean(kv, c, where)
            m.check(where)
    lib["cc_decode_step_set_single_launch"](1)
    if refused_any:
        pytest.skip(f"{E.quant_shape_id(shape)}: the two-launch form passed; the device's occupancy query refuses the single launch")


# ------------------------------------------------------------------------------------------------ the ring and the hybrid step
def _ring_forms(lib, c, fmt_code):
    """[(form, runs as one launch)]: the ring step has two launches; the hybrid step one where the plan mirror says so and
    cc_decode_step_hybrid_quant_single_launch agrees (a launch the occupancy query refuses is left out and reported)."""
    from cold_compress_amd.attention_utils import _workspace
    from helpers import DT_CODE

    _workspace(lib["cc_decode_attn_workspace_bytes"](c.HQ, c.H, c.S, c.D, DT_CODE[c.dt]), torch.device(DEV))
    forms = [("two", False)]
    if c.family != "hyb":
        return forms, False
    one = G.intended_single_launch(c)
    lib["cc_decode_step_set_single_launch"](1)
    dev_one = bool(lib["cc_decode_step_hybrid_quant_single_launch"](c.HQ, c.H, c.S, c.D, DT_CODE[c.dt], fmt_code))
    if not one:
        assert not dev_one, f"{c.id}: the device library offers a single launch the plan mirror does not know"
        return forms, False
    if dev_one:
        forms.append(("one", True))
    return forms, not dev_one


@pytest.mark.parametrize("shape", G.quant_shape_list(), ids=G.quant_shape_id)
def test_ring_and_hybrid_quant_replays_return_the_simulators_answers(lib, shape):
    """cc_decode_step_heavy_hitter_ring_quant and cc_decode_step_hybrid_quant_rc: y, every small buffer, the window sums, the written
    ring column, the images and the parameter words after every step; the whole ring and the rebuilt window sums after the last."""
    refused_any = False
    for c in G.quant_cases_of(shape):
        kv = G.make_cache(c, DEV)
        assert kv.fused_quant
        forms, refused = _ring_forms(lib, c, kv.quant_format)
        refused_any |= refused
        for form, is_one in forms:
            where = f"{c.id} [{form}]"
            m = Margins()
            lib["cc_decode_step_set_single_launch"](1 if form == "one" else 0)
            assert bool(kv.single_launch_active(c.HQ)) == is_one, f"{where}: not the intended launch form"
            kv, n, _ = G.run_replay(c, form, DEV, put=m.put, sync=torch.cuda.synchronize, kv=kv)
            _count(f"{c.quant} {c.family}", form, n)
            torch.cuda.synchronize()
            _status_clean(kv, c, where)
            m.check(where)
    lib["cc_decode_step_set_single_launch"](1)
    if refused_any:
        pytest.skip(f"{G.quant_shape_id(shape)}: the two-launch form passed; the device's occupancy query refuses the single launch")


def test_zz_report():
    """Prints what the file compared (run it with -s): elements compared exactly per format and form."""
    for (family, form), n in sorted(COUNTS.items()):
        print(f"format {family} [{form}]: {n} elements compared exactly")
