"""The decode steps on the device against the known answers of tests/step_exact.py: every replay (family A) in three forms —
update_kv -> scaled_dot_product_attention -> update_state, decode_step as two launches, decode_step as one launch — each compared
with the SIMULATOR (never with another form), bit for bit in every buffer after every step; every ramp step (family B) within the
bounds derived in the helper.  Each case asserts the launch path it ran on (the plan mirror of the helper against the device
library's own answers).  q, k_new and v_new sit between NaN rows; test_rows_around_y_stay_nan does the same for y through the C ABI.
The workspace is left alone: it holds the epochs and the status word of the single-launch hand-off."""
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
    nw, nt, xl2 = E.intended(c.dt, c.D, c.H, c.HQ, c.S)
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
_REUSE = {("hh", 2, 4, 130, 128), ("rg", 2, 4, 130, 128), ("full", 8, 32, 200, 128), ("l2", 8, 32, 200, 128), ("hh", 8, 32, 200, 128),
          ("hh", 2, 8, 130, 64), ("full", 2, 4, 515, 16)}


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
            if form != "three" and c.fill == "brim" and (c.policy, c.H, c.HQ, c.S, c.D) in _REUSE and c.dt == E.BF:
                # the same cache object again after reset(): the same answers (a pipeline that kept state across reset() would not)
                kv, n = E.run_replay(c, form, DEV, put=m.put, sync=torch.cuda.synchronize, kv=kv)
                _count("A", form, n)
                _status_clean(kv, c, where + " after reset()")
                m.check(where)
    lib["cc_decode_step_set_single_launch"](1)
    if refused_any:
        pytest.skip(f"{E.shape_id(shape)}: three-call and two-launch forms passed; the device's occupancy query refuses the single launch")


# ------------------------------------------------------------------------------------------------ B. ramp steps
_RAMPS = [(sh, dt, v) for sh in E.RAMP_SHAPES + E.RAMP_VALU_SHAPES for dt in (E.BF, E.HF) for v in E.RAMP_VARIANTS]


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
    _rows_around_y(lib, E.Case("hh", E.BF, H, HQ, S, 128, "brim", steps=12, hist="zeros", seed=5), one)


@pytest.mark.parametrize("dt,H,HQ,S,D", [(E.BF, 2, 8, 130, 64), (E.F32, 1, 8, 35, 128)], ids=lambda x: E.DT_NAME.get(x, None) or str(x))
def test_rows_around_y_stay_nan_valu(lib, dt, H, HQ, S, D):
    """The same behind the VALU streaming pass (two launches): 16-bit head_dim 64, and the fp32 / D = 128 shape whose single combine
    block per head walks 1024 outputs in eight groups (the loop over further output groups)."""
    c = E.Case("hh", dt, H, HQ, S, D, "brim", steps=12, hist="zeros", seed=5)
    assert c.plan["nt"] == 0 and (D != 128 or HQ // H * D // ((S + 127) // 128) > 128)
    _rows_around_y(lib, c, False)


def _rows_around_y(lib, c, one):
    from cold_compress_amd import _abi
    from cold_compress_amd.attention_utils import _workspace
    from cold_compress_amd.cache import _DT, _ptr, _stream

    H, HQ, S = c.H, c.HQ, c.S
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
                  int(kv.recent_window), HQ, c.scale, _ptr(y), _ptr(ws), ws.numel(), _stream(), phases)
        torch.cuda.synchronize()
        assert np.array_equal(E.bits(y), E.bits(st["y"])), f"{c.id} step {i}: y"
        assert bool(torch.isnan(ybuf[:MARGIN]).all()) and bool(torch.isnan(ybuf[MARGIN + HQ:]).all()), f"{c.id} step {i}: rows around y were written"
        _count("A", "one" if one else "two", HQ * D + E.compare_small(kv, sim, f"{c.id} step {i}"))
    _status_clean(kv, c, c.id)


# ------------------------------------------------------------------------------------------------ refused at head_dim 64, not mis-served
def test_steps_without_a_valu_form_are_refused_at_d64(lib):
    """l2, hybrid, the fused quantised cache, the QKV-folded step and the single launch exist in the matrix-core kernel only: at
    head_dim 64 each entry point answers CC_ERR_UNSUPPORTED and leaves K, V, pos, mask, cache_cts, the history, the pipeline's keys
    and y as they were, bit for bit; the availability queries answer 0."""
    import types

    import step_exact_ring as G
    from cold_compress_amd import _abi
    from cold_compress_amd.attention_utils import _workspace
    from cold_compress_amd.cache import _DT, _ptr, _stream

    UNSUPPORTED = -2
    c = E.Case("hh", E.BF, 2, 8, 130, 64, "brim", steps=12, hist="pairs", seed=2)
    H, HQ, S, D, code = c.H, c.HQ, c.S, c.D, _DT[c.dt]
    assert lib["cc_decode_step_single_launch"](HQ, H, S, D, code) == 0 and lib["cc_decode_step_l2_single_launch"](HQ, H, S, D, code) == 0
    assert lib["cc_decode_step_hybrid_single_launch"](HQ, H, S, D, code) == 0
    assert lib["cc_decode_step_qkv_available"](HQ, H, S, D, code, 64) == 0
    sim = E.Sim(c)
    st = sim.step(0)
    ws = _workspace(lib["cc_decode_attn_workspace_bytes"](HQ, H, S, D, code), torch.device(DEV))
    p = torch.tensor([st["p"]], dtype=torch.int32, device=DEV)
    q, k1, v1 = st["q"].to(DEV), st["k1"].to(DEV), st["v1"].to(DEV)
    y = torch.full((HQ, D), float("nan"), dtype=c.dt, device=DEV)

    def snapshot(kv, extra):
        bufs = dict(K=kv.k_cache, V=kv.v_cache, pos=kv.pos, mask=kv.mask, cache_cts=kv.cache_cts, num=kv.attn_history_num,
                    denom=kv.attn_history_denom, counter=kv.attn_counter, next_key=kv.next_key, step_commit=kv.step_commit, y=y, **extra)
        torch.cuda.synchronize()
        return bufs, {k: E.bits(v).copy() for k, v in bufs.items()}

    def unchanged(bufs, before, what):
        torch.cuda.synchronize()
        for k, v in bufs.items():
            assert np.array_equal(E.bits(v), before[k]), f"{what}: refused, but {k} changed"

    # ---- a plain heavy-hitter cache: l2, the quantised step, the QKV-folded step, the forced single launch
    kv = E.make_cache(c, DEV)
    E.seed_cache(kv, c, DEV)
    kv.prepare_decode(p)
    key_norm = torch.ones(H, S, dtype=c.dt, device=DEV)
    qparams = torch.ones(1, H, S, 4, dtype=torch.float32, device=DEV)
    K_IN = 64
    wqkv = torch.ones((HQ + 2 * H) * D, K_IN, dtype=c.dt, device=DEV)
    x, norm_w = torch.ones(K_IN, dtype=c.dt, device=DEV), torch.ones(K_IN, dtype=c.dt, device=DEV)
    bufs, before = snapshot(kv, dict(key_norm=key_norm, qparams=qparams))
    num, den, ctr = _ptr(kv.attn_history_num), _ptr(kv.attn_history_denom), _ptr(kv.attn_counter)
    g, w = int(kv.global_tokens), int(kv.recent_window)
    rc = lib["cc_decode_step_l2"](kv._view(), _ptr(q), _ptr(k1), _ptr(v1), _ptr(p), _ptr(key_norm), _ptr(kv.next_key), g, w, HQ, c.scale,
                                  _ptr(y), _ptr(ws), ws.numel(), _stream())
    assert rc == UNSUPPORTED, ("cc_decode_step_l2", rc)
    unchanged(bufs, before, "cc_decode_step_l2")
    rc = lib["cc_decode_step_quant"](kv._view(), _ptr(qparams), 8, 1, _ptr(q), _ptr(k1), _ptr(v1), _ptr(p), num, den, ctr, None,
                                     _ptr(kv.next_key), g, w, HQ, c.scale, _ptr(y), None, _ptr(ws), ws.numel(), _stream(), 3)
    assert rc == UNSUPPORTED, ("cc_decode_step_quant", rc)
    unchanged(bufs, before, "cc_decode_step_quant")
    rc = lib["cc_decode_step_qkv_rc"](kv._view(), 1, _ptr(wqkv), None, _ptr(x), None, _ptr(norm_w), 1e-5, None, None, K_IN, None, _ptr(p), num,
                                      den, ctr, None, 0, _ptr(kv.next_key), _ptr(kv.step_commit), g, w, HQ, c.scale, _ptr(y), _ptr(ws),
                                      ws.numel(), _stream())
    assert rc == UNSUPPORTED, ("cc_decode_step_qkv_rc", rc)
    unchanged(bufs, before, "cc_decode_step_qkv_rc")
    rc = lib["cc_decode_step_heavy_hitter_rc"](kv._view(), _ptr(q), _ptr(k1), _ptr(v1), _ptr(p), num, den, ctr, _ptr(kv.next_key),
                                               _ptr(kv.step_commit), g, w, HQ, c.scale, _ptr(y), _ptr(ws), ws.numel(), _stream(),
                                               3 | _abi.CC_PHASE_ONE_LAUNCH)
    assert rc == UNSUPPORTED, ("cc_decode_step_heavy_hitter_rc, CC_PHASE_ONE_LAUNCH", rc)
    unchanged(bufs, before, "cc_decode_step_heavy_hitter_rc with CC_PHASE_ONE_LAUNCH")
    # (the cache is intact: the two-launch step that does exist returns the simulator's answer from it)
    _abi.call("cc_decode_step_heavy_hitter_rc", kv._view(), _ptr(q), _ptr(k1), _ptr(v1), _ptr(p), num, den, ctr, _ptr(kv.next_key),
              _ptr(kv.step_commit), g, w, HQ, c.scale, _ptr(y), _ptr(ws), ws.numel(), _stream(), 3 | _abi.CC_PHASE_TWO_LAUNCH)
    torch.cuda.synchronize()
    assert np.array_equal(E.bits(y), E.bits(st["y"]))
    _count("A", "two", HQ * D + E.compare_small(kv, sim, f"{c.id} after the refusals"))

    # ---- a hybrid cache (per-head counts): the hybrid step
    hc = types.SimpleNamespace(family="hyb", S=S, H=H, D=D, dt=c.dt, g=G.G_TOK)
    hv = G.make_cache(hc, DEV)
    assert not hv._fused_shape_ok()
    hv.k_cache.copy_(kv.k_cache)
    hv.v_cache.copy_(kv.v_cache)
    hv.cache_cts.fill_(S - 8)
    hv.mask[0, :, 0, :S - 8] = True
    hv.pos[0, :, :S - 8] = torch.arange(S - 8, dtype=torch.int32, device=DEV)
    strat = torch.zeros(H, dtype=torch.int64, device=DEV)
    tab = torch.from_numpy(G.policy_rows(S)).to(DEV)
    wsum, acc = hv._window_state()
    tok = torch.tensor([G.PLAIN_TOK], dtype=torch.int64, device=DEV)
    y.fill_(float("nan"))
    bufs, before = snapshot(hv, dict(wsum=wsum, acc=acc, special=hv.special_mask, punc=hv.punc_mask, num_punc=hv.num_punc))
    rc = lib["cc_decode_step_hybrid"](hv._view(), _ptr(q), _ptr(k1), _ptr(v1), _ptr(p), _ptr(strat), _ptr(tab), tab.shape[0],
                                      _ptr(hv.attn_history_num), _ptr(hv.attn_history_denom), _ptr(hv.attn_counter), hv.history_window_size,
                                      _ptr(acc), _ptr(wsum), _ptr(hv.special_mask), _ptr(hv.punc_mask), _ptr(tok), _ptr(hv.punc_ids),
                                      hv.punc_ids.numel(), _ptr(hv.num_special), _ptr(hv.num_punc), _ptr(hv.next_key), int(hv.global_tokens),
                                      HQ, c.scale, _ptr(y), None, _ptr(ws), ws.numel(), _stream())
    assert rc == UNSUPPORTED, ("cc_decode_step_hybrid", rc)
    unchanged(bufs, before, "cc_decode_step_hybrid")


def test_zz_report():
    """Prints what the file compared (run it with -s): elements per family and form, and family B's worst error / bound."""
    for (family, form), (exact, bounded) in sorted(COUNTS.items()):
        print(f"family {family} [{form}]: {exact} elements compared exactly, {bounded} under a bound")
    for form, (ry, rn) in sorted(WORST.items()):
        print(f"family B [{form}]: worst error / bound: y {ry:.3g}, history increment {rn:.3g}")
