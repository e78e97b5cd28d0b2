"""The ring-history decode steps on the device against the known answers of tests/step_exact_ring.py: every replay of
KVCacheHybrid.decode_step and of KVCacheHeavyHitter with history_window_size > 1, in every form the device offers — update_kv ->
scaled_dot_product_attention(history=fused_history()) -> update_state, decode_step as two launches, decode_step as one launch (hybrid,
where cc_decode_step_hybrid_single_launch says so) — each compared with the SIMULATOR (never with another form), bit for bit in y
and in every buffer after every step, in the whole ring and in a rebuild of the window sums after the last.  q, k_new and v_new sit
between NaN rows; the hand-off's status word is 0 after every replay."""
import time

import pytest
import torch

import step_exact_ring as E
from test_gpu_step_exact import DEV, Margins

pytestmark = pytest.mark.gpu
COUNTS = {}  # (family, form) -> elements compared exactly (nothing is compared under a bound: the two-hot y is one bit pattern)
SECONDS = {}


@pytest.fixture()
def lib():
    from cold_compress_amd import _abi

    fns = _abi.lib()
    yield fns
    fns["cc_decode_step_set_single_launch"](1)


def _status_clean(kv, c, where):
    from cold_compress_amd.attention_utils import single_launch_status

    torch.cuda.synchronize()
    assert kv.step_status(c.HQ) == 0, f"{where}: step_status"
    assert single_launch_status(torch.device(DEV)) == 0, f"{where}: the hand-off's status word is set"


def _forms(lib, c):
    """[(form, runs as one launch)]: asserts that the plan mirror puts the case on its intended path and that the device library
    agrees; a single launch the device's occupancy query refuses is left out and reported.  -> (forms, refused)"""
    from cold_compress_amd.attention_utils import _workspace
    from helpers import DT_CODE

    # (the decode workspace: making it is what probes the device's block placement for the XCD-L2 transport)
    _workspace(lib["cc_decode_attn_workspace_bytes"](c.HQ, c.H, c.S, c.D, DT_CODE[c.dt]), torch.device(DEV))
    forms = [("three", False), ("two", False)]
    one = E.intended_single_launch(c)
    if c.family != "hyb":
        return forms, False
    lib["cc_decode_step_set_single_launch"](1)
    dev_one = bool(lib["cc_decode_step_hybrid_single_launch"](c.HQ, c.H, c.S, c.D, DT_CODE[c.dt]))
    if not one:
        assert not dev_one, f"{c.id}: the device library offers a single launch the plan mirror does not know"
        return forms, False
    if dev_one and E.HYB_SHAPES[(c.H, c.HQ, c.S)][2]:
        assert lib["cc_decode_step_l2_handoff"]() == 1, f"{c.id}: intended for the XCD-L2 transport, which this device does not offer"
    if dev_one:
        forms.append(("one", True))
    return forms, not dev_one


_REUSE = {("hyb", 3, 12, 130), ("ring", 2, 4, 130)}


@pytest.mark.parametrize("shape", E.shape_list(), ids=E.shape_id)
def test_replays_return_the_simulators_answers(lib, shape):
    refused_any = False
    t0 = time.perf_counter()
    for k, c in enumerate(E.cases_of(shape)):
        forms, refused = _forms(lib, c)
        refused_any |= refused
        for form, is_one in forms:
            where = f"{c.id} [{form}]"
            m = Margins()
            lib["cc_decode_step_set_single_launch"](1 if form == "one" else 0)
            kv = E.make_cache(c, DEV)
            assert bool(kv.single_launch_active(c.HQ)) == is_one, f"{where}: not the intended launch form"
            kv, n, _ = E.run_replay(c, form, DEV, put=m.put, sync=torch.cuda.synchronize, kv=kv)
            COUNTS[(c.family, form)] = COUNTS.get((c.family, form), 0) + n
            _status_clean(kv, c, where)
            m.check(where)
            if form != "three" and k == 0 and (c.family, c.H, c.HQ, c.S) in _REUSE and c.dt == E.BF:
                # the same cache object again after reset(): the same answers (a pipeline that kept state across reset() would not)
                kv, n, _ = E.run_replay(c, form, DEV, put=m.put, sync=torch.cuda.synchronize, kv=kv)
                COUNTS[(c.family, form)] += n
                _status_clean(kv, c, where + " after reset()")
                m.check(where)
    lib["cc_decode_step_set_single_launch"](1)
    SECONDS[E.shape_id(shape)] = time.perf_counter() - t0
    if refused_any:
        pytest.skip(f"{E.shape_id(shape)}: three-call and two-launch forms passed; the device's occupancy query refuses the single launch")


def test_zz_report(audit):
    """Prints and audits what the file compared: elements per family and form, all of them exactly."""
    assert COUNTS, "no replay ran"
    for (family, form), exact in sorted(COUNTS.items()):
        audit(f"{family} [{form}]: {exact} elements compared exactly, 0 under a bound")
        print(f"{family} [{form}]: {exact} elements compared exactly, 0 under a bound")
    for k, v in sorted(SECONDS.items(), key=lambda x: -x[1])[:3]:
        print(f"slowest: {k}: {v:.2f} s")
