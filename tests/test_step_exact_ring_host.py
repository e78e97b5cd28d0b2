"""tests/step_exact_ring.py on the CPU: the oracle's twins of the hybrid step and of the ring-history heavy-hitter step, driven through
the real cache classes (tests/cpu_twin.py) in the three-call form and the decode_step form, return the simulator's answers bit for
bit in every buffer after every step (this is also where the open rule of the header — heads without the heavy_hitter flag get their
ring column, denominator and window sum written like all others — is settled: the twin of cc_hh_ring_update writes every head); the
constructions have the properties the helper's docstring claims; every one-fault mutant of the simulator is rejected by at least
one case (REJECTED_BY records by which), and the one mutant that is equivalent under the contract is shown to be equivalent."""
import os

import numpy as np
import pytest
import torch

import step_exact_ring as E
from cpu_twin import cpu_twin

BF, HF = E.BF, E.HF
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cold_compress_amd", "csrc")
HOST_SHAPES = [t for t in E.shape_list() if t[4] <= 1280]


# ------------------------------------------------------------------------------------------------ the mirrored lines
@pytest.mark.parametrize("fname", sorted(E.RING_LINES))
def test_mirrored_lines_are_the_source(fname):
    """The divisions by l the two-hot argument rests on (plain IEEE divisions: ONE bit pattern for y) and the arg-min's chunk."""
    src = " ".join(open(os.path.join(CSRC, fname)).read().split())
    for line in E.RING_LINES[fname]:
        assert " ".join(line.split()) in src, f"{fname} no longer contains: {line}"
    build = " ".join(open(os.path.join(ROOT, "cold_compress_amd", "_build.py")).read().split())
    assert " ".join(E.BUILD_FLAGS_LINE.split()) in build, "the build flags changed: is the fp32 division still correctly rounded?"
    assert E.NEXT_KEY_CHUNK == 128 and "constexpr int kNextKeyChunk = 128;" in E.MIRRORED_LINES["cc_common.h"]


def test_every_shape_lands_on_its_intended_path():
    seen = set()
    for t in E.shape_list():
        fam, dt, H, HQ, S, W, D = E.unpack(t)
        pl = E.plan(HQ, H, S, D, dt)
        R = HQ // H
        if fam == "hyb":
            nw, nt, xl2 = E.HYB_SHAPES[(H, HQ, S)]
            assert (pl["nw"], pl["nt"] if R in (4, 8) else 0) == (nw, nt), (t, pl)
            assert (pl["xl2"] and nt > 0) == xl2
            seen.add((nw, nt, xl2, R))
        assert pl["n_split"] > 1 or S <= pl["rows_per_split"]
        if D != 128:  # the VALU streaming pass: two launches only, a ragged last split (two rows at D = 64; the only one at D = 32)
            assert fam == "ring" and pl["nt"] == 0 and pl["nw"] == 4 and S % pl["rows_per_split"] == {64: 2, 32: 130}[D], (t, pl)
    assert {r for _, _, _, r in seen} >= {2, 4, 7, 8}
    assert {(w, n, x) for w, n, x, _ in seen} >= {(4, 0, False), (4, 1, False), (4, 1, True), (8, 1, True), (4, 2, True)}
    assert {E.unpack(t)[5] for t in E.shape_list()} >= {8, 33, 400} and (33 * 2) % 16 != 0  # 66-byte ring rows: the unaligned branch
    assert {(E.unpack(t)[1], E.unpack(t)[6]) for t in E.shape_list()} >= {(BF, 64), (HF, 32)}


# ------------------------------------------------------------------------------------------------ the constructions
def _representable(x, dt):
    return float(torch.tensor(x, dtype=torch.float64).to(dt).double()) == x


def test_constructions():
    odd = {("hyb", BF): 0, ("hyb", HF): 0, ("ring", BF): 0}
    ties = 0
    for t in HOST_SHAPES:
        for c in E.cases_of(t):
            assert c.gap >= 150, (c.id, c.gap)
            W = c.W
            assert c.ctr0 % W == W - 5 and c.ctr0 + c.steps > W  # counter % W wraps during the replay
            ws = c.ring0.sum(axis=2, dtype=np.float64)
            live = c.mask0 == 1
            assert ((c.ring0 != 0).sum(axis=2)[live] <= 90).all() and (c.ring0[:, :, c.ctr0 % W] != 0).any()  # sparse rows; the first column overwritten is seeded
            assert set(np.unique(c.den0 if c.family == "hyb" else c.den0[live]).tolist()) >= {1, 2, 3, 4, W - 1, W, W + 7}
            if c.family == "hyb":
                assert (c.den0[live] >= 1).all()
                assert np.array_equal(c.rows, E.policy_rows(c.S))
                for h in range(c.H):  # the poison: every dead slot holds the code word of a live token of the head
                    n = int(c.cts0[h])
                    assert set(c.kpos0[h, n:].tolist()) <= set(c.pos0[h, :n].tolist())
            for h in range(c.H):
                s = c.odd_slot[h]
                if s >= 0:
                    assert not _representable(float(ws[h, s]), c.dt), (c.id, h, ws[h, s])
                    odd[(c.family, c.dt)] = odd.get((c.family, c.dt), 0) + 1
                pl = sorted(c.planted[h])
                if pl:  # the planted scores are one float32 value, below every other unprotected slot, through min(denom, W) only
                    ties += 1
                    sc = E._rnd_np(ws[h], c.dt).astype(np.float32) / np.maximum(np.minimum(c.den0[h], W), 1).astype(np.float32)
                    assert len({sc[x].tobytes() for x in pl}) == 1
                    assert {int(c.den0[h, x]) for x in pl} <= {W, W + 7}
                    raw = ws[h, pl] / c.den0[h, pl]
                    assert len(pl) < 2 or len(set(raw.tolist())) == 2  # (without the min the tie breaks)
    assert min(odd.values()) >= 3, odd  # a window sum the dtype cannot hold, in every family and dtype with the room for one
    assert ties >= 20


def test_the_replays_visit_what_they_claim():
    want = {"hyb": {"append_below_budget", "punc_append", "full_append", "evict_hh", "evict_window", "drop", "drop_full",
                    "dropped_token_selected_in_live_last_slot", "new", "last_live",
                    "last_live_of_partial_split", "wave", "workgroup", "different_splits", "poison_behind_selection", "tie_at_minimum",
                    "counter_wraps", "wrap_drops_entry", "entry_leaves_sum", "twohot_append", "twohot_evict", "dup_dropped_invisible",
                    "dup_drop_full", "twohot_new_in_earlier_split", "twohot_new_in_later_split", "twohot_same_tile", "twohot_other_tile"},
            "ring": {"fills_empty", "evict_hh", "new", "last_live", "last_live_of_partial_split", "wave", "workgroup", "different_splits",
                     "poison_behind_selection", "tie_at_minimum", "counter_wraps", "wrap_drops_entry", "entry_leaves_sum", "twohot_evict",
                     "twohot_new_in_earlier_split", "twohot_new_in_later_split", "twohot_same_tile", "twohot_other_tile"}}
    # where a two-hot pair can lie depends on where the shape's evictions fall: required over the family, not of every shape
    anywhere = {"twohot_new_in_earlier_split", "twohot_new_in_later_split", "twohot_other_tile", "twohot_same_tile"}
    few_heads = {"drop", "drop_full", "dropped_token_selected_in_live_last_slot", "dup_dropped_invisible", "dup_drop_full", "full_append", "punc_append", "evict_window", "evict_hh",
                 "append_below_budget", "twohot_append", "twohot_evict", "workgroup", "tie_at_minimum"}
    family = {"hyb": set(), "ring": set()}
    for t in HOST_SHAPES:
        notes, twohot, rows, kinds = set(), 0, set(), set()
        for c in E.cases_of(t):
            sim = E.make_sim(c)
            for i in range(c.steps):
                sim.step(i)
            notes |= sim.notes
            twohot += sim.n_twohot
            if c.family == "hyb":
                rows |= set(c.strat.tolist())
                kinds |= set(c.kind)
        family[t[0]] |= notes
        assert twohot > 0, t
        miss = want[t[0]] - notes - anywhere
        fam, dt, H, HQ, S, W, D = E.unpack(t)
        if E.plan(HQ, H, S, D, dt)["n_split"] == 1:
            miss -= {"different_splits"}
        if t[2] >= 8:  # (over the shape's three start states; the shapes with one to four heads hold fewer policies at a time)
            assert not miss, (t, miss)
            if t[0] == "hyb":
                assert rows == set(range(len(E.STRATEGIES))) and kinds == set(E.HybCase.KINDS)
        else:
            assert not miss - few_heads, (t, miss)
    for fam in family:
        assert not want[fam] - family[fam], (fam, want[fam] - family[fam])


# ------------------------------------------------------------------------------------------------ the oracle's twins return the answers
@pytest.mark.parametrize("shape", HOST_SHAPES, ids=E.shape_id)
def test_oracle_twins_return_the_answers(monkeypatch, oracle, shape):
    """Three-call form and decode_step form, every buffer bit for bit after every step, the whole ring and a rebuild of the window
    sums after the last; small cases also hold y and the group means to the float64 evaluation of the contract (attend_dense)."""
    n = 0
    with cpu_twin(monkeypatch, oracle):
        for k, c in enumerate(E.cases_of(shape)):
            for form in ("three", "two"):
                kv, m, _ = E.run_replay(c, form, "cpu", dense=(c.S <= 200 and form == "three"))
                n += m
                if form == "two" and k == 0 and c.S <= 130 and c.dt == BF:  # the same cache object again after reset()
                    kv, m, _ = E.run_replay(c, form, "cpu", kv=kv)
                    n += m
    assert n > 0


# ------------------------------------------------------------------------------------------------ teeth
def _mutant_cases():
    out = []
    for t in (("hyb", BF, 2, 4, 130, 400), ("hyb", HF, 3, 12, 130, 400), ("hyb", BF, 8, 32, 200, 400), ("hyb", HF, 8, 64, 130, 400),
              ("hyb", BF, 4, 28, 130, 400), ("ring", BF, 2, 4, 130, 8), ("ring", HF, 4, 28, 130, 33), ("ring", BF, 8, 32, 200, 33),
              ("ring", BF, 2, 4, 130, 8, 64), ("ring", HF, 4, 28, 130, 33, 32)):
        out += E.cases_of(t)
    return out


_MUTANT_CASES = _mutant_cases()


def _differs(c, fault):
    """Does the mutant's replay differ from the simulator's anywhere (y or any buffer the drivers compare, at any step)?"""
    a, b = E.make_sim(c), E.make_sim(c, fault=fault)
    for i in range(c.steps):
        sa, sb = a.step(i), b.step(i)
        if not np.array_equal(E.bits(sa["y"]), E.bits(sb["y"])) or sa["idx"] != sb["idx"]:
            return True
        ba, bb = a.buffers(), b.buffers()
        if any(not np.array_equal(E.bits(ba[k]), E.bits(bb[k])) for k in ba):
            return True
        if a.col[0] != b.col[0] or not np.array_equal(a.col[1], b.col[1]):
            return True
        if not torch.equal(a.K.view(torch.int16), b.K.view(torch.int16)) or not torch.equal(a.V.view(torch.int16), b.V.view(torch.int16)):
            return True
    return not np.array_equal(a.ring, b.ring)


REJECTED_BY = {}
# a case every mutant must be rejected by (the full lists are printed, and recorded in DESIGN 2.22)
WANT = {1: "hyb-", 2: "hyb-", 3: "hyb-", 4: "hyb-", 5: "hyb-", 6: "hyb-", 7: "hyb-", 8: "hyb-", 9: "hyb-", 10: "hyb-", 11: "hyb-", 12: "ring-",
        13: "hyb-", 14: "hyb-", 15: "hyb-", 16: "hyb-", 17: "ring-", 18: "ring-", 19: "ring-", 20: "hyb-"}


@pytest.mark.parametrize("number", sorted(E.FAULTS))
def test_every_mutant_is_rejected(number):
    fault = E.FAULTS[number]
    cases = [c for c in _MUTANT_CASES if not (number in E.HYB_ONLY and c.family != "hyb") and not (number in E.RING_ONLY and c.family != "ring")]
    hit = [c.id for c in cases if _differs(c, fault)]
    REJECTED_BY[number] = hit
    print(f"mutant {number} ({fault}): rejected by {len(hit)} of {len(cases)} cases: {hit}")
    assert hit, f"no case rejects mutant {number} ({fault})"
    assert any(x.startswith(WANT[number]) for x in hit), (number, fault, hit)
    if number in (1, 4, 12, 13, 14, 19, 20):  # faults of the parts both families share: rejected in both
        assert {x.split("-")[0] for x in hit} == {"hyb", "ring"}, (number, hit)


def test_the_equivalent_mutant_is_equivalent():
    """"The decision reads the NEW num_punc": num_punc enters the budget of punctuation-flag heads only, and on the step that bumps
    it (a punctuation token) those heads append whatever the budget says — no case can reject it.  Its stale neighbour (mutant 11)
    is rejected above."""
    assert not any(_differs(c, E.EQUIVALENT_FAULT) for c in _MUTANT_CASES if c.family == "hyb")
