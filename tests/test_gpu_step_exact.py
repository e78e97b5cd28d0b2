"""The decode steps on the device against the known answers of tests/step_exact.py: every replay (family A) in three forms —
update_kv -> scaled_dot_product_attention -> update_state, decode_step as two launches, decode_step as one launch — each compared
with the SIMULATOR (never with another form), bit for bit in every buffer after every step; every ramp step (family B) within the
bounds derived in the helper.  Each case asserts the launch path it ran on (the plan mirror of the helper against the device
library's own answers).  q, k_new and v_new sit between NaN rows; test_rows_around_y_stay_nan does the same for y through the C ABI.
The workspace is left alone: it holds the epochs and the status word of the single-launch hand-off."""
import math

import numpy as np
import pytest
import torch

import step_exact as E

pytestmark = pytest.mark.gpu
DEV = "cuda"
MARGIN = 8  # NaN rows on both sides of q, k_new, v_new (and y)
COUNTS = {}  # (family, form) -> [elements compared exactly, elements compared under a bound]
WORST = {}   # form -> [worst error / bound of y, of the history increment] (family B)


@pytest.fixture()
def lib():
    from cold_compress_amd import _abi

    fns = _abi.lib()
    yield fns
    fns["cc_decode_step_set_single_launch"](1)


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


def _count(family, form, exact, bounded=0):
    c = COUNTS.setdefault((family, form), [0, 0])
    c[0] += exact
    c[1] += bounded


def _status_clean(kv, c, where):
    from cold_compress_amd.attention_utils import single_launch_status

    torch.cuda.synchronize()
    if c.policy == "hh":
        assert kv.step_status(c.HQ) == 0, f"{where}: step_status"
    assert single_launch_status(torch.device(DEV)) == 0, f"{where}: the hand-off's status word is set"


def _path(lib, c):
    """Asserts that the plan mirror puts the case on its intended path and that the device library agrees.
    -> (single launch expected, refused by the device's occupancy query)."""
    from cold_compress_amd.attention_utils import _workspace
    from helpers import DT_CODE

    # (the decode workspace: making it is what probes the device's block placement for the XCD-L2 transport)
    _workspace(lib["cc_decode_attn_workspace_bytes"](c.HQ, c.H, c.S, c.D, DT_CODE[c.dt]), torch.device(DEV))
    nw, nt, xl2 = E.INTENDED[(c.H, c.HQ, c.S)]
    if c.policy == "l2":
        nt = 1 if nt == 1 else 0
    assert (c.plan["nw"], c.plan["nt"]) == (nw, nt), (c.id, c.plan)
    fn = "cc_decode_step_l2_single_launch" if c.policy == "l2" else "cc_decode_step_single_launch"
    lib["cc_decode_step_set_single_launch"](1)
    dev_one = bool(lib[fn](c.HQ, c.H, c.S, c.D, DT_CODE[c.dt]))
    if nt == 0:
        assert not dev_one, f"{c.id}: the device library offers a single launch the plan mirror does not know"
        return False, False
    if dev_one and xl2:  # the XCD-L2 transport: the placement was verified on this device when the first decode workspace was made
        assert lib["cc_decode_step_l2_handoff"]() == 1, f"{c.id}: intended for the XCD-L2 transport, which this device does not offer"
    return True, not dev_one


def _forms(lib, c):
    """[(form, runs as one launch)] for the case; a single launch the occupancy query refuses is left out and reported."""
    one, refused = _path(lib, c)
    forms = [("three", False), ("two", False)]
    if one and not refused:
        forms.append(("one", True))
    return forms, (one and refused)


def _set_switch(lib, c, form):
    """Head-constant policies and l2 take the process-wide switch; heavy_hitter the attribute run_replay sets."""
    lib["cc_decode_step_set_single_launch"](1 if form == "one" else 0 if c.policy != "hh" else 1)


# ------------------------------------------------------------------------------------------------ A. selector replays
_REUSE = {("hh", 2, 4, 130), ("rg", 2, 4, 130), ("full", 8, 32, 200), ("l2", 8, 32, 200), ("hh", 8, 32, 200)}


@pytest.mark.parametrize("shape", E.shape_list(), ids=E.shape_id)
def test_replays_return_the_simulators_answers(lib, shape):
    refused_any = False
    for c in E.cases_of(shape):
        forms, refused = _forms(lib, c)
        refused_any |= refused
        for form, is_one in forms:
            where = f"{c.id} [{form}]"
            m = Margins()
            _set_switch(lib, c, form)
            kv = E.make_cache(c, DEV)
            if c.policy == "hh":
                kv.single_launch = form == "one"
                assert kv.single_launch_active(c.HQ) == is_one, f"{where}: not the intended launch form"
            kv, n = E.run_replay(c, form, DEV, put=m.put, sync=torch.cuda.synchronize, kv=kv)
            _count("A", form, n)
            _status_clean(kv, c, where)
            m.check(where)
            if form != "three" and c.fill == "brim" and (c.policy, c.H, c.HQ, c.S) in _REUSE and c.dt == E.BF:
                # the same cache object again after reset(): the same answers (a pipeline that kept state across reset() would not)
                kv, n = E.run_replay(c, form, DEV, put=m.put, sync=torch.cuda.synchronize, kv=kv)
                _count("A", form, n)
                _status_clean(kv, c, where + " after reset()")
                m.check(where)
    lib["cc_decode_step_set_single_launch"](1)
    if refused_any:
        pytest.skip(f"{E.shape_id(shape)}: three-call and two-launch forms passed; the device's occupancy query refuses the single launch")


# ------------------------------------------------------------------------------------------------ B. ramp steps
_RAMPS = [(sh, dt, v) for sh in E.RAMP_SHAPES for dt in (E.BF, E.HF) for v in E.RAMP_VARIANTS]


@pytest.mark.parametrize("shape,dt,variant", _RAMPS, ids=lambda x: E.DT_NAME.get(x, None) or (x if isinstance(x, str) else "-".join(map(str, x))))
def test_ramp_steps_within_their_bounds(lib, shape, dt, variant):
    refused_any = False
    for c in E.ramp_cases(shape, dt, variant):
        forms, refused = _forms(lib, c)
        refused_any |= refused
        for form, is_one in forms:
            where = f"{c.id} [{form}]"
            m = Margins()
            lib["cc_decode_step_set_single_launch"](1)
            kv, ry, rn, n_exact, n_bound = E.run_ramp(c, form, DEV, put=m.put, sync=torch.cuda.synchronize)
            assert kv.single_launch_active(c.HQ) == is_one, f"{where}: not the intended launch form"
            _count("B", form, n_exact, n_bound)
            w = WORST.setdefault(form, [0.0, 0.0])
            w[0], w[1] = max(w[0], ry), max(w[1], rn)
            _status_clean(kv, c, where)
            m.check(where)
    if refused_any:
        pytest.skip("three-call and two-launch forms passed; the device's occupancy query refuses the single launch")


# ------------------------------------------------------------------------------------------------ y between NaN rows
@pytest.mark.parametrize("H,HQ,S", [(2, 4, 130), (8, 32, 200), (16, 64, 1280), (8, 32, 4160)])
@pytest.mark.parametrize("one", [False, True])
def test_rows_around_y_stay_nan(lib, H, HQ, S, one):
    """decode_step allocates y itself; here the heavy-hitter step is called through the C ABI with y inside a NaN-filled buffer: the
    answer is the simulator's and the rows on both sides of y stay NaN."""
    from cold_compress_amd import _abi
    from cold_compress_amd.attention_utils import _workspace
    from cold_compress_amd.cache import _DT, _ptr, _stream

    c = E.Case("hh", E.BF, H, HQ, S, 128, "brim", steps=12, hist="zeros", seed=5)
    expect_one, refused = _path(lib, c)
    if one and (not expect_one or refused):
        pytest.skip("the device's occupancy query refuses the single launch")
    sim = E.Sim(c)
    kv = E.make_cache(c, DEV)
    E.seed_cache(kv, c, DEV)
    D = c.D
    nbytes = lib["cc_decode_attn_workspace_bytes"](HQ, H, S, D, _DT[c.dt])
    ws = _workspace(nbytes, torch.device(DEV))
    ybuf = torch.full((HQ + 2 * MARGIN, D), float("nan"), dtype=c.dt, device=DEV)
    y = ybuf[MARGIN:MARGIN + HQ]
    phases = 3 | (_abi.CC_PHASE_ONE_LAUNCH if one else _abi.CC_PHASE_TWO_LAUNCH)
    for i in range(c.steps):
        st = sim.step(i)
        p = torch.tensor([st["p"]], dtype=torch.int32, device=DEV)
        if i == 0:
            kv.prepare_decode(p)
        q, k1, v1 = st["q"].to(DEV), st["k1"].to(DEV), st["v1"].to(DEV)
        _abi.call("cc_decode_step_heavy_hitter_rc", kv._view(), _ptr(q), _ptr(k1), _ptr(v1), _ptr(p), _ptr(kv.attn_history_num),
                  _ptr(kv.attn_history_denom), _ptr(kv.attn_counter), _ptr(kv.next_key), _ptr(kv.step_commit), int(kv.global_tokens),
                  int(kv.recent_window), HQ, 1.0 / math.sqrt(D), _ptr(y), _ptr(ws), ws.numel(), _stream(), phases)
        torch.cuda.synchronize()
        assert np.array_equal(E.bits(y), E.bits(st["y"])), f"{c.id} step {i}: y"
        assert bool(torch.isnan(ybuf[:MARGIN]).all()) and bool(torch.isnan(ybuf[MARGIN + HQ:]).all()), f"{c.id} step {i}: rows around y were written"
        _count("A", "one" if one else "two", HQ * D + E.compare_small(kv, sim, f"{c.id} step {i}"))
    _status_clean(kv, c, c.id)


def test_zz_report():
    """Prints what the file compared (run it with -s): elements per family and form, and family B's worst error / bound."""
    for (family, form), (exact, bounded) in sorted(COUNTS.items()):
        print(f"family {family} [{form}]: {exact} elements compared exactly, {bounded} under a bound")
    for form, (ry, rn) in sorted(WORST.items()):
        print(f"family B [{form}]: worst error / bound: y {ry:.3g}, history increment {rn:.3g}")
