"""The quantised cases of tests/step_exact.py (Case.quant: the four image formats of the fused KV cache) on the CPU: the uint8
twin against the oracle's converters, the constructions, the shape table against the plan mirror, the one-fault mutants, the uint8
cases through the real cache classes over the oracle's step twin (bit for bit in every buffer, image and parameter word), and for
FP8, uint4 and MXFP4 — which have no CPU statement of the step other than the simulator — the float64 evaluation of the attention
contract on the dequantised values.  Every assertion is equality of bit patterns."""
import hashlib
import os

import numpy as np
import pytest
import torch

import kv_quant_twin as Q
import step_exact as E
import step_exact_ring as G
from cpu_twin import cpu_twin
from helpers import DT_CODE, to_np

BF, HF = E.BF, E.HF
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cold_compress_amd", "csrc")
SMALL = [t for t in E.quant_shape_list() if t[4] <= 200]


# ------------------------------------------------------------------------------------------------ 1. the twin interface
def _edge_rows():
    """The edge rows of tests/test_kv_uint4_host.py::test_edge_rows, and a zero row, a row of -0 and a +-1 code-word row."""
    x = np.zeros((8, 128), np.float32)
    x[0] = 3.25
    x[1] = 1.0
    x[1, 7] = 1.0 + 2.0 ** -7  # (the smallest step above 1 both 16-bit dtypes hold)
    x[2] = np.linspace(-65504, 65504, 128)
    x[3] = np.float32(0.5)
    x[3, 100] = 40.0
    x[5] = -0.0
    x[6] = np.where(np.arange(128) % 3 == 0, -1.0, 1.0)
    x[7] = x[6] * 0.25
    return x


@pytest.mark.parametrize("dt", [BF, HF], ids=["bf16", "f16"])
def test_uint8_twin_is_the_oracles_converter(oracle, dt):
    """kv_uint4_twin's arithmetic with 255 levels against cc_kv_quant_rows_cpu / cc_kv_dequant_rows_cpu: images, the four parameter
    words and the decoded values bit for bit, on random rows over twenty binades with an offset and on the edge rows."""
    g = np.random.default_rng(7)
    x = g.standard_normal((2048, 128)) * np.exp2(g.integers(-10, 10, (2048, 1))) + g.standard_normal((2048, 1)) * 4
    rows = torch.from_numpy(np.concatenate([x.astype(np.float32), _edge_rows()])).to(dt)
    rows = torch.where(torch.isfinite(rows), rows, torch.zeros_like(rows))  # (f16: 65504 stays, nothing beyond it)
    N, D = rows.shape
    kn = to_np(rows)
    vn = to_np(rows.flip(0))
    kq, vq, par = np.zeros((N, D), np.uint8), np.zeros((N, D), np.uint8), np.zeros((N, 4), np.float32)
    oracle.call("cc_kv_quant_rows", oracle.ptr(kn), oracle.ptr(vn), 1, N, D, DT_CODE[dt], 8, oracle.ptr(kq), oracle.ptr(vq), oracle.ptr(par), None)
    ko, vo = np.zeros_like(kn), np.zeros_like(vn)
    oracle.call("cc_kv_dequant_rows", oracle.ptr(kq), oracle.ptr(vq), oracle.ptr(par), 1, N, D, DT_CODE[dt], 8, oracle.ptr(ko), oracle.ptr(vo), None)
    ki, kw, kb = Q.round_trip(rows, dt, "fused")
    vi, vw, vb = Q.round_trip(rows.flip(0), dt, "fused")
    assert np.array_equal(ki, kq) and np.array_equal(vi, vq)
    assert np.array_equal(Q.qparams(kw, vw), par.view(np.uint32))
    assert np.array_equal(kb, ko) and np.array_equal(vb, vo)
    assert float((kb != kn).mean()) > 0.25  # (the round trip is not the identity on such rows: bf16 0.37, f16 more)


def test_the_interface_is_the_three_twins():
    """round_trip(rows, dt, fmt) is the named twin's quantise + decode, and the word pairs have the header's layout."""
    g = torch.Generator().manual_seed(3)
    rows = (torch.randn(64, 128, generator=g) * 3).to(BF)
    xf = rows.float().numpy()
    img, w, b = Q.round_trip(rows, BF, "uint4")
    i2, sc, mn = Q.U4.quant_rows(xf)
    assert np.array_equal(img, i2) and np.array_equal(w[:, 0].view(np.float32), sc) and np.array_equal(w[:, 1].view(np.float32), mn)
    assert np.array_equal(b, Q.U4.round_trip_bits(xf, "bf16")) and img.shape == (64, 64)
    img, w, b = Q.round_trip(rows, BF, "mxfp4")
    i2, sb = Q.MX.quant_rows(xf)
    assert np.array_equal(img, i2) and np.array_equal(w[:, 0], Q.MX.scale_word(sb)) and not w[:, 1].any()
    assert np.array_equal(b, Q.MX.round_trip_bits(xf, "bf16"))
    img, w, b = Q.round_trip(rows, HF, "fp8")
    codes, e = Q.F8.quant_rows(rows.to(HF).float().numpy())
    assert np.array_equal(img, codes) and np.array_equal(w[:, 0].view(np.float32), np.exp2(e).astype(np.float32)) and not w[:, 1].any()
    assert np.array_equal(b, Q.F8.dequant_bits(codes, e, "f16"))
    img, w, b = Q.round_trip(rows, BF, "fused")
    assert img.shape == (64, 128) and int(img.max()) == 255 and int(img.min()) == 0
    assert np.array_equal(Q.swap_nibbles(Q.swap_nibbles(img)), img)


# ------------------------------------------------------------------------------------------------ 2. the constructions
@pytest.mark.parametrize("fmt", Q.FORMATS)
def test_constructions(fmt):
    """Case._quantise asserts, per case: the round trip of every key row is the identity; the round-tripped V rows of a head are
    pairwise distinct; the round trip changes more than half of V's elements; MXFP4 rows carry >= 3 distinct scale bytes; consecutive
    tokens' V parameters differ.  Here, on top: the gap, K's parameters differ between neighbouring slots, the images are not the
    16-bit rows, the dead slots' images, and how much the round trip changes."""
    changed = {}
    for t in E.quant_shape_list():
        if t[5] != fmt:
            continue
        for c in E.quant_cases_of(t):
            assert c.quant == fmt and c.gap >= E.GAP_MIN and c.amp == 128, (c.id, c.gap)
            assert c.e.max() == 2 and (c.e[:, c.T:] <= 1).all()
            kp = c.k_par[:, :c.T]
            assert float((kp[:, 1:] != kp[:, :-1]).any(axis=-1).mean()) > 0.3, c.id  # a stale K scale is a wrong one in 1 of 3 slots
            sim = E.Sim(c)
            assert sim.Kimg.shape == (c.H, c.S, Q.image_width(128, fmt)) and sim.par.shape == (c.H, c.S, 4) and sim.par.dtype == np.uint32
            if c.T < c.S:  # dead slots: the image of a zero row (K; V too but in the sparse fill, where V holds the poison)
                assert not E.bits(sim.K[:, c.T:]).any()
                want = c.poison_img[0] if c.fill == "sparse" else c.zero_img[0]
                assert (sim.Vimg[:, c.T:] == want).all() and (sim.Kimg[:, c.T:] == c.zero_img[0]).all()
                assert bool((sim.V[:, c.T:] == (E.POISON_V if c.fill == "sparse" else 0)).all())
            changed.setdefault(E.DT_NAME[c.dt], []).append(c.changed)
    for name, v in sorted(changed.items()):
        print(f"{fmt} {name}: the round trip changes {min(v):.3f} .. {max(v):.3f} of V's elements")


_DIGESTS = {  # sha256 (first 128 bits) over the inputs and answers of cases as they were before Case took `quant`
    ("hh", BF, 3, 12, 130, 128, "brim", 16, "pairs", 1): "c2c13832fdeaa3ab43f96393b0dc12e4",
    ("hh", HF, 8, 32, 200, 128, "sparse", 16, "zeros", 3): "aaeb4aa79096f24a23f0af72b46699b5",
    ("rg", BF, 1, 8, 200, 128, "minus3", 16, "zeros", 2): "f04b552a25b039f3e95568df8e657fbd",
    ("full", HF, 8, 64, 130, 128, "brim", 16, "zeros", 1): "883b02e0e7454becab5ff554a4cd2f3b",
    ("l2", BF, 2, 4, 130, 128, "sparse", 16, "pairs", 3): "24ac5c6e9d03375ef00a7ea0e063a395",
    ("hh", BF, 16, 64, 1280, 128, "minus3", 12, "zeros", 2): "b787b44441e1ba0c634084031af409e1",
    ("hh", E.F32, 2, 4, 77, 16, "brim", 16, "pairs", 1): "d928e455267a899a4101f460058f1fd9",
}


def test_cases_without_quant_are_bit_identical_to_before():
    """Case(quant=None): inputs (K, V rows, seeded history) and answers (q, k_new, v_new, y, the insert's slots, every buffer, K and V
    after every step) hash to what they hashed to before the quantised cases existed."""
    for (pol, dt, H, HQ, S, D, fill, steps, hist, seed), want in _DIGESTS.items():
        c = E.Case(pol, dt, H, HQ, S, D, fill, steps=steps, hist=hist, seed=seed)
        h = hashlib.sha256()
        sim = E.Sim(c)
        for a in (c.k_all, c.v_all):
            h.update(E.bits(a).tobytes())
        h.update(c.num0.tobytes())
        h.update(c.den0.tobytes())
        for i in range(c.steps):
            st = sim.step(i)
            for k in ("q", "k1", "v1", "y"):
                h.update(E.bits(st[k]).tobytes())
            h.update(np.asarray(st["idx"]).tobytes())
            h.update(st["slots"].tobytes())
            for k, v in sorted(sim.buffers().items()):
                h.update(E.bits(v).tobytes())
            h.update(E.bits(sim.K).tobytes())
            h.update(E.bits(sim.V).tobytes())
        assert h.hexdigest()[:32] == want, c.id
        assert c.quant is None and c.k_deq is c.k_all and c.v_deq is c.v_all


# ------------------------------------------------------------------------------------------------ 3. the shape table
def test_mirrored_quant_plan_lines_are_the_source():
    src = " ".join(open(os.path.join(CSRC, "cc_attn_decode.hip")).read().split())
    for line in E.MIRRORED_QUANT_LINES["cc_attn_decode.hip"]:
        assert " ".join(line.split()) in src, f"cc_attn_decode.hip no longer contains: {line}"


def test_the_quant_table_reaches_every_selector():
    """Conditions on E.QUANT_SHAPES, walked through the plan mirror for every format and both dtypes: the four two-launch selectors
    (rt, nw), the four of the single launch over the memory hand-off, the four over the XCD-L2 transport, a shape of >= 2 splits
    whose last split is partly filled, a shape whose sparse fill leaves whole splits masked, and a shape with no single launch."""
    rows = {}
    for fmt in Q.FORMATS:
        for dt in (BF, HF):
            two, mem, xl2 = set(), set(), set()
            partial = masked = none = False
            policies = {}
            for t in E.quant_shape_list():
                pol, tdt, H, HQ, S, tf = t
                if (tf, tdt) != (fmt, dt):
                    continue
                pl = E.quant_plan(HQ, H, S, dt)
                nw, nt, x = E.intended(dt, 128, H, HQ, S)
                assert pl["nw"] == nw and pl["nt"] == (1 if nt == 1 else 0) and (pl["xl2"] and pl["nt"] == 1) == (x and nt == 1), (t, pl)
                two.add((pl["rt"], pl["nw"]))
                if pl["nt"] == 1:
                    (xl2 if pl["xl2"] else mem).add((pl["rt"], pl["nw"]))
                else:
                    none = True
                ns, rps = pl["n_split"], pl["rows_per_split"]
                partial |= ns >= 2 and S - (ns - 1) * rps < rps
                masked |= ns >= 2 and (ns - 1) * rps >= 70 + 16  # (sparse: 70 live slots and at most 16 inserts: the last split stays masked)
                policies.setdefault(pol, set()).add((pl["rt"], pl["nw"], pl["nt"], pl["xl2"]))
                rows[(H, HQ, S)] = (pl["rt"], pl["nw"], ns, rps, S - (ns - 1) * rps, "none" if pl["nt"] == 0 else "XCD-L2" if pl["xl2"] else "memory hand-off")
            every = {(4, 4), (8, 4), (4, 8), (8, 8)}
            assert two == every and mem == every and xl2 == every, (fmt, dt, two, mem, xl2)
            assert partial and masked and none, (fmt, dt, partial, masked, none)
            for pol in ("rg", "full"):  # the head-constant policies reach a 4- and an 8-wave plan and both transports
                assert {nw for _, nw, _, _ in policies[pol]} == {4, 8} and {x for _, _, nt, x in policies[pol] if nt} == {False, True}
    assert E.quant_plan(32, 8, 4160, BF)["nt"] == 0 and E.plan(32, 8, 4160, 128, BF)["nt"] == 2  # two tiles per wave: no single launch
    assert len(E.quant_shape_list()) == 4 * 2 * (9 + 2 * 4) and max(t[4] for t in E.quant_shape_list()) == 5120
    for (H, HQ, S), r in sorted(rows.items(), key=lambda kv: (kv[0][2], kv[0][1])):
        print(f"({H}, {HQ}, {S}): rt {r[0]}, {r[1]} waves, {r[2]} splits x {r[3]} rows (last {r[4]}), single launch: {r[5]}")


def test_the_quant_replays_visit_what_they_claim():
    """The selection of the row inserted in this very step, the last live slot of a partly filled split, a wave's and a workgroup's
    boundary, heads of one group in different splits; the planted ties are walked in index order (brim, pairs) across a wave, a
    128-slot chunk and a workgroup; every selected key is a full-scale row while scaled rows are live."""
    want = {"new", "last_live_of_partial_split", "wave", "workgroup", "different_splits"}
    for (H, HQ, S) in E.QUANT_SHAPES:
        if S > 1290:
            continue
        notes = set()
        for c in E.quant_cases_of(("hh", BF, H, HQ, S, "uint4")):
            sim = E.Sim(c)
            evicted = []
            for i in range(c.steps):
                st = sim.step(i)
                evicted.append(st["idx"][0])
                assert (c.e[np.arange(c.HQ) // c.R, st["sel"]] == 0).all()
            notes |= sim.notes
            assert "new" in sim.notes, c.id
            scaled_live = [(c.e[h][sim.pos[h][sim.mask[h] == 1]] > 0).mean() for h in range(c.H)]
            assert min(scaled_live) > 0.1, (c.id, scaled_live)
            if c.fill == "brim" and c.hist == "pairs":
                s = sorted(c.planted)
                k = min(len(s), c.w + 1)
                assert evicted[:k] == s[:k], (c.id, evicted, s)
                if S >= 200:
                    assert {63, 64, 127, 128} <= set(s)
        assert not (want - notes), ((H, HQ, S), want - notes)


# ------------------------------------------------------------------------------------------------ 5. teeth
def _mutant_cases(fmt):
    out = []
    for t in (("hh", BF, 3, 12, 130, fmt), ("hh", HF, 1, 8, 200, fmt), ("rg", BF, 3, 12, 130, fmt)):
        out += E.quant_cases_of(t)
    return out


def _differs(c, fault):
    """Does the mutant's replay differ from the simulator's anywhere (y, any buffer, K, V, an image or a parameter word, at any step)?"""
    a, b = E.Sim(c), E.Sim(c, fault=fault)
    for i in range(c.steps):
        sa, sb = a.step(i), b.step(i)
        if not np.array_equal(E.bits(sa["y"]), E.bits(sb["y"])) or sa["idx"] != sb["idx"]:
            return True
        ba, bb = a.buffers(), b.buffers()
        if any(not np.array_equal(E.bits(ba[k]), E.bits(bb[k])) for k in ba):
            return True
        ia, ib = a.images(), b.images()
        if any(not np.array_equal(ia[k], ib[k]) for k in ia):
            return True
        if not np.array_equal(E.bits(a.K), E.bits(b.K)) or not np.array_equal(E.bits(a.V), E.bits(b.V)):
            return True
    return False


def _y_differs(c, fault):
    """The same through y alone (what a caller of the step sees)."""
    a, b = E.Sim(c), E.Sim(c, fault=fault)
    return any(not np.array_equal(E.bits(a.step(i)["y"]), E.bits(b.step(i)["y"])) for i in range(c.steps))


@pytest.mark.parametrize("fmt", Q.FORMATS)
def test_every_quant_mutant_is_rejected(fmt):
    """Each new one-fault mutant is rejected by at least one case of every format it applies to; the attention-side ones (all but
    the stale parameters, which the parameter words show) also through y alone.  Prints the matrix of DESIGN 2.24."""
    cases = _mutant_cases(fmt)
    applies = E.quant_faults_of(fmt)
    assert set(applies) == set(E.QUANT_FAULTS) - ({"nibble_swap"} if fmt not in Q.FOUR_BIT else set()) - ({"block_scale0"} if fmt != "mxfp4" else set())
    for fault in applies:
        hit = [c.id for c in cases if _differs(c, fault)]
        by_y = [c.id for c in cases if c.id in hit and _y_differs(c, fault)]
        fills = lambda ids: ", ".join(f for f in E.FILLS if any(f"-{f}-" in x for x in ids)) or "-"  # noqa: E731
        print(f"{fmt} {fault}: rejected by {len(hit)} of {len(cases)} cases ({fills(hit)}); through y alone by {len(by_y)} ({fills(by_y)})")
        assert hit, f"{fmt}: no case rejects '{fault}'"
        assert by_y, f"{fmt}: no case rejects '{fault}' through y"
        if fault == "poison_live":
            assert any("-sparse-" in x for x in by_y) and not any("-brim-" in x for x in hit)  # (a brim-full cache has no masked slot)
    for fault in E.QUANT_FAULTS:
        if fault not in applies:
            with pytest.raises(AssertionError):
                E.Sim(cases[0], fault=fault)


@pytest.mark.parametrize("fmt", Q.FORMATS)
def test_the_older_mutants_are_still_rejected(fmt):
    """Every attention and decision mutant of step_exact.FAULTS is rejected by at least one quantised case of the format."""
    cases = _mutant_cases(fmt)
    for fault in E.FAULTS:
        if fault == "dup_tail":
            continue  # (the VALU pass's clamped row: the matrix-core kernel, the only one that reads images, has no such copy)
        hit = next((c.id for c in cases if _differs(c, fault)), None)
        print(f"{fmt} {fault}: rejected by {hit}")
        assert hit, f"{fmt}: no quantised case rejects '{fault}'"


# ------------------------------------------------------------------------------------------------ 6. the step itself
_U8_HOST = [t for t in E.quant_shape_list() if t[5] == "fused" and t[4] <= 1280]


@pytest.mark.parametrize("shape", _U8_HOST, ids=E.quant_shape_id)
def test_oracle_twin_returns_the_uint8_answers(monkeypatch, oracle, shape):
    """uint8 images: the real cache classes over the oracle's twins (cc_prefill_fill, cc_kv_quant_rows, cc_decode_step_quant with
    n_bit 8, cc_kv_dequant_rows): y, every small buffer, the images, the parameter words and the decoded cache after every step,
    bit for bit — which also settles what the dead slots hold after the class's own prefill."""
    n = 0
    with cpu_twin(monkeypatch, oracle):
        for c in E.quant_cases_of(shape):
            kv, m = E.run_replay(c, "two", "cpu", dense=(c.S <= 200))
            assert kv.fused_quant and kv.quant_format == 8
            n += m
    assert n > 0


@pytest.mark.parametrize("shape", [t for t in SMALL if t[5] != "fused"], ids=E.quant_shape_id)
def test_dense_attention_returns_the_one_hot_answers(shape):
    """FP8, uint4, MXFP4: the float64 evaluation of the attention contract (step_exact.attend_dense) on the dequantised K and V
    returns the simulator's y and group means bit for bit at every step (asserted inside Sim.step with dense=True), and the
    simulator's K and V are the decode of its images under its parameter words."""
    for c in E.quant_cases_of(shape):
        sim = E.Sim(c, dense=True)
        for i in range(c.steps):
            st = sim.step(i)
            new = [h * c.R for h in range(c.H) if st["slots"][h * c.R] == st["idx"][h if c.Hp > 1 else 0]]
            for j in new:  # a head that selects the row inserted in this step gets its ROUND TRIP, which is not the row
                assert np.array_equal(E.bits(st["y"][j]), E.bits((c.v_deq[j // c.R, st["p"]].double() + 0.0).to(c.dt)))  # (-0 -> +0)
                assert not np.array_equal(E.bits(st["y"][j]), E.bits(st["v1"][j // c.R]))


# ------------------------------------------------------------------------------------------------ 4. the ring and the hybrid step
def test_the_hybrid_quant_table_reaches_every_selector():
    """All ten hybrid selectors per format and dtype: two launches at rt 4 / 8 and 4 / 8 waves; one launch at 8 waves (rt 4, 8), at
    4 waves with one tile per wave (rt 4, 8) and with up to eight (rt 4, 8).  The ring shapes: rt 4 and 8, 4 and 8 waves."""
    for fmt in Q.FORMATS:
        for dt in (BF, HF):
            two, wide, single, multi, ring = set(), set(), set(), set(), set()
            for (fam, tdt, H, HQ, S, W, tf) in G.quant_shape_list():
                if (tf, tdt) != (fmt, dt):
                    continue
                if fam == "ring":
                    pl = E.plan(HQ, H, S, 128, dt)
                    ring.add((pl["rt"], pl["nw"]))
                    continue
                pl = G.quant_hybrid_plan(HQ, H, S, dt)
                assert (pl["nw"], pl["nt"]) == G.QUANT_HYB_SHAPES[(H, HQ, S)], ((H, HQ, S), pl)
                two.add((pl["rt"], pl["nw"]))
                if pl["nw"] == 8 and pl["nt"] == 1:
                    wide.add(pl["rt"])
                if pl["nw"] == 4 and pl["nt"] == 1:
                    single.add(pl["rt"])
                if pl["nw"] == 4 and 1 < pl["nt"] <= 8:
                    multi.add(pl["rt"])
            assert two == {(4, 4), (8, 4), (4, 8), (8, 8)} and wide == single == multi == {4, 8}, (fmt, dt, two, wide, single, multi)
            assert ring >= {(4, 4), (8, 4), (4, 8)}, ring


_RING_SMALL = [t for t in G.quant_shape_list() if t[4] <= 200]


@pytest.mark.parametrize("shape", _RING_SMALL, ids=G.quant_shape_id)
def test_ring_and_hybrid_quant_cases_hold_on_the_cpu(shape):
    """The constructions (asserted in _Case._common: key round trips are the identity, round-tripped V rows pairwise distinct, more
    than half of V changed, consecutive V parameters differ) and, per step, the float64 evaluation of the attention contract on the
    dequantised values (_check_dense); the simulator's K and V are the decode of its images; a step writes one slot per head."""
    for c in G.quant_cases_of(shape):
        sim = G.make_sim(c, dense=True)
        assert sim.n_twohot == 0
        dead = sim.mask == 0
        assert bool((sim.V[torch.from_numpy(dead)] == G.POISON_V).all())
        for i in range(c.steps):
            before = {k: v.copy() for k, v in sim.images().items()}
            st = sim.step(i)
            im = sim.images()
            for k in im:
                changed = {(int(h), int(s)) for h, s in zip(*np.nonzero((im[k] != before[k]).any(axis=-1)))}
                assert changed <= {(h, st["idx"][h]) for h in range(c.H)}, (c.id, i, k)
            for img, w, t in ((im["k_img"], im["qparams"][..., :2], sim.K), (im["v_img"], im["qparams"][..., 2:], sim.V)):
                assert np.array_equal(Q.decode(img, w, c.dt, c.quant), E.bits(t)), (c.id, i)
        assert sim.n_twohot == 0
