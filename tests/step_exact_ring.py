"""Known-answer replays for the two families of decode steps that keep a W-entry attention-history RING: KVCacheHybrid.decode_step
(cc_decode_step_hybrid[_rc], the HYB instantiations of decode_attn_split_mfma_kernel; W = 400) and KVCacheHeavyHitter with
history_window_size > 1 (cc_decode_step_heavy_hitter_ring, cc_decode_attn_gqa_ring).  A helper, not a test, on the model of
tests/step_exact.py: tests/test_step_exact_ring_host.py holds the oracle's twins to these answers on the CPU and shows the teeth
(FAULTS below); tests/test_gpu_step_exact_ring.py holds the kernels to them.  CPU tensors only.

The SIMULATOR (HybSim, RingSim and their base) is plain numpy / torch-CPU arithmetic written from the contract of
include/coldcompress.h (cc_hybrid_decode_update, cc_decode_step_hybrid, cc_decode_update_heavy_hitter_ring, cc_hh_ring_update).  It
shares no code with the kernels, the oracle or tests/attn_ref.py.  From tests/step_exact.py it takes plan, bits, attend_dense (the
float64 evaluation of the attention contract the small cases are held to), GAP_MIN, ULP and MIRRORED_LINES; from
tests/prefill_exact.py the code words and the rounded-score table.  The drivers at the end are the only users of cold_compress_amd.

INPUTS (the selector construction of step_exact, section A).  Keys are +-1 code words, queries 128 x a code word, D = 128 (64 and 32
in the two ring replays of RING_VALU_SHAPES, which run behind the VALU streaming pass instead of the matrix-core kernel); the gap
between the dtype-rounded score of a matching key and of any other key is measured per case and asserted >= GAP_MIN, so every
non-matching probability is +0.  New here:
  poison     every slot a head does not see (hybrid: at or beyond cache_cts[h]; ring policy: the empty slots) holds the code word of
             a token the head's queries select, with a V row of 2^14 (finite: 0 x V must stay 0).  A pass that ignores the mask or
             masks with another head's count halves a probability and moves y by thousands.
  two-hot    on chosen steps head h's incoming KEY is the code word of a token t still live in h, and one query head selects t:
             the two scores are one bit pattern, both probabilities are exp(0) / 2 = 0.5 (a correctly rounded division of 1 by 2),
             the group mean is a multiple of 1 / (2 R), and y = dtype((V[t] + v_new) / 2): the fp32 sum of two dtype values with
             exponents in [-6, 3] is exact and the division by l = 2 is exact, so that is ONE rounding and y is ONE bit pattern.
             (The tail divides with a correctly rounded IEEE division — RING_LINES pins the two lines — not through v_rcp_f32.)
             A hybrid head that DROPS the token keeps it invisible (p(t) = 1, y = V[t]) unless the head is full: then slot S - 1 is
             live and the token replaces what was there (the reference's behaviour).
  ring seeds entries multiples of 1 / 8 in [0, 3], most of them 0; denominators 1 .. 4, W - 1, W, W + 7 (a live hybrid slot never 0:
             the hybrid score divides by min(denom, W), unclamped below); attn_counter = W - 5, so that counter % W wraps during the
             replay and seeded entries LEAVE the tracked sums; ties of the scores planted at slots 63/64, 127/128, on both sides of
             every kNextKeyChunk boundary and at the first and the last unprotected slot (tie only through min(denom, W): the pair
             holds denominators W and W + 7); one slot per head whose window sum is NOT representable in the dtype (bf16: 33.125,
             fp16: 258.125, both rounding to even) wherever W leaves room for it (bf16: W >= 14, fp16: W >= 89).

WHAT THE SIMULATOR COMPUTES PER STEP — all exact:
  window sum    float64 sum of the slot's W ring entries (at most 400 values of at most 11 significant bits between 2^-10 and 4: no
                rounding), rounded ONCE to the dtype; kept incrementally, and recomputed from the whole ring after every step for
                S <= 300 (asserted equal).
  hybrid        head h, policy row (flags, win, hhs), count cts, position p, in the header's order: punctuation token on a punc head
                -> append at min(cts, S - 1); full -> the same; budget = g + [special] num_special + [punc] num_punc(OLD) +
                [window] win + [heavy_hitter] hhs; cts < budget -> append; else a heavy_hitter / window head evicts its candidate,
                any other head drops (pos, K, V to slot S - 1; mask and count untouched).  Candidate: arg-min over slots < cts of
                f32(wsum) / f32(min(denom, W)) (heavy_hitter) or f32(pos) (window), +inf for slot < g, for a special / punctuation
                slot of a head whose policy carries that flag, and for pos > p - win (STRICT); lowest index wins.  An append sets
                the mask and cts += 1; a punctuation token sets punc_mask[slot] in EVERY head; num_punc += 1 once per step.
  history       hybrid (reset_history_on_evict = False): nothing is cleared on an eviction.  Every step, for EVERY head — the rule
                the header leaves open, settled against the oracle's twin of the three-call path: heads without the heavy_hitter
                flag get their column, denominator and window sum written like all others — ring[h, s, counter % W] = gm[h, s]
                (0 where masked), denom += 1 everywhere, counter += 1.
  ring policy   avg = f32(dtype(sum_W)) / f32(clamp(denom, 1, W)); (pos < g) | (pos >= p - w) -> 1.0; pos == -1 -> 0.0 (last);
                arg-min, lowest index; the evicted slot's ring row, denominator and window sum restart from zero BEFORE the step's
                column is written.
  y, gm         y as above; gm = dtype(f32(sum of the group's dtype probabilities) / f32(R)): the sum is a multiple of 1 / 2, and the
                float64 and the float32 quotient round to the same dtype value for every such sum (asserted per case).
y, group means (the written ring column), pos, mask, cache_cts, K, V, punc_mask, num_punc, denominators, window sums and
attn_counter are compared as bit patterns after every step; the whole ring after the last one.

One mutant of the issue's list is EQUIVALENT under the contract and is asserted to be so instead of rejected: "the decision reads the
NEW num_punc" — num_punc enters the budget of punctuation-flag heads only, and on the one step that bumps it those heads append
unconditionally (first link of the chain).  Its neighbour that is NOT equivalent stands in for it: the decision reads a STALE num_punc
(the previous punctuation step's bump not yet visible: the hazard of a ticket-ordered write racing the next prologue).

Over the fused quantised caches (HybCase / RingCase(quant=...)): V rows as in step_exact section C, attention reads
their round trip through tests/kv_quant_twin.py; the keys stay unscaled code words; the poison is the image of a row of 2^14; no
two-hot step is planted; images and parameter words are compared after every step (decode_step only: two launches, hybrid also one)."""
import numpy as np
import torch

import kv_quant_twin as Q
import prefill_exact as P
from step_exact import BF, DT_NAME, GAP_MIN, HF, MIRRORED_LINES, NEXT_KEY_CHUNK, ULP, _first_diff, attend_dense, bits, plan  # noqa: F401

G_TOK, W_REC, W_HYB = 4, 5, 400
PUNC_TOK, PLAIN_TOK = 6, 11  # every fifth token is punctuation, as in tests/test_gpu_hybrid.py
TOKEN_IDS = {"special": [[1], [2, 3]], "punctuation": [5, 6, 7]}
NSP0, NPU0 = 3, 2  # num_special / num_punc of the start state
POISON_V = 2.0 ** 14
# the reference's two policy lists (cache_configs/hybrid.yaml, fastgen.yaml; recorded in oracle/gen_golden.py), restated
HYBRID_YAML = [{"strategy": "window", "recent_window": 0.1},
               {"strategy": "window_heavy_hitter", "heavy_hitter_frac": 0.25, "recent_window": 0.1},
               {"strategy": "window_heavy_hitter", "heavy_hitter_frac": 0.5, "recent_window": 0.1}, {"strategy": "full"}]
FASTGEN_YAML = [{"strategy": "special"}, {"strategy": "special_punc"}, {"strategy": "special_punc_heavy_hitter", "heavy_hitter_frac": 0.3},
                {"strategy": "special_punc_heavy_hitter_window", "recent_window": 0.3, "heavy_hitter_frac": 0.3}, {"strategy": "full"}]
STRATEGIES = HYBRID_YAML[:3] + FASTGEN_YAML  # one list, so that one launch holds all of them side by side ("full" once)
F_HH, F_WIN, F_PUNC, F_SPECIAL, F_FULL = 1, 2, 4, 8, 16
# lines of csrc this helper rests on beyond step_exact.MIRRORED_LINES: the two divisions by l behind the two-hot argument (plain IEEE
# divisions: the build has no fast-math flag, and HIP's fp32 division is correctly rounded by default), and the chunk of the arg-min
RING_LINES = {
    "cc_attn_decode.hip": ["ElemTraits<T>::store(reinterpret_cast<T*>(a.y), (size_t)(h * R + r) * D + d, O / sm_L[r]);",
                           "const float p = ElemTraits<T>::rnd(__fdiv_rn(exp_nonpos(x - sm_M[r]), sm_L[r]));",
                           "const float av = ElemTraits<T>::rnd(__fdiv_rn(sum, (float)R));"],
    "cc_attn_decode_kernels.h": ["if (gg == 0) ElemTraits<T>::store(reinterpret_cast<T*>(a.y), (size_t)(h * RT + r) * D + (to - r * D), part / sm_L1[r]);",
                                 "pr[kk] = ElemTraits<T>::rnd(__fdiv_rn(exp_nonpos(x - sm_M1[r_me]), sm_L1[r_me]));"],
    "cc_common.h": ["constexpr int kNextKeyChunk = 128;"],
}
BUILD_FLAGS_LINE = 'FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wno-unused-function"]'


def policy_rows(S):
    """[n, 3] int32: flags, window slots = round(recent_window S), heavy-hitter slots = round(heavy_hitter_frac S)."""
    rows = []
    for s in STRATEGIES:
        name = s["strategy"]
        flags = F_FULL if name == "full" else sum(v for k, v in (("heavy_hitter", F_HH), ("window", F_WIN), ("punc", F_PUNC), ("special", F_SPECIAL)) if k in name)
        rows.append([flags, round(s.get("recent_window", 0) * S), round(s.get("heavy_hitter_frac", 0) * S)])
    return np.array(rows, np.int32)


def _rnd_np(x, dt):
    """float64 array -> rounded once (nearest-even) to dt -> float64 array."""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dt).double().numpy()


# ------------------------------------------------------------------------------------------------ the cases
class _Case:
    """What both families share: code words, V rows, the measured gap, the group-mean table."""

    def _common(self, dt, H, HQ, S, steps, L, seed, D=128, quant=None):
        self.dt, self.H, self.HQ, self.S, self.D, self.steps, self.L = dt, H, HQ, S, D, steps, L
        self.quant = quant  # None, or the image format of the fused quantised cache (kv_quant_twin.FORMATS)
        assert quant is None or (quant in Q.FORMATS and D == 128 and (HQ // H) in (4, 8))
        if quant:
            self.id += f"-{quant}"
        self.R = HQ // H
        assert self.R * H == HQ and 8 <= steps <= 24
        self.g, self.amp, self.scale = G_TOK, 128, P.default_scale(D)
        self.plan = plan(HQ, H, S, D, dt)
        self.nb = P.nbits_for(L)
        codes, self.rep = P.code_words(L, D)
        self.codes = codes.astype(np.float32)
        gen = torch.Generator().manual_seed(131 * seed + S + 7 * H)
        v = torch.randn(H, L, D, generator=gen, dtype=torch.float32)
        v = torch.where(v.abs() < 2.0 ** -6, torch.copysign(torch.tensor(2.0 ** -6), v), v)
        if quant:  # step_exact.Case's V rows: block b of token t times 2^(3 ((t + b) % 4) - 4), odd tokens times 16
            tb = (np.arange(L)[:, None] + np.arange(D // 32)[None, :]) % 4
            v = v * torch.from_numpy(2.0 ** (3.0 * tb - 4.0)).to(torch.float32).repeat_interleave(32, dim=1)[None]
            v = v * torch.from_numpy(16.0 ** (np.arange(L) % 2)).to(torch.float32)[None, :, None]
        self.v_all = v.to(dt)
        self.v_deq = self.v_all  # what attention reads: the rows themselves, or their round trip
        a = self.v_all.double().abs()
        # exponents in [-6, 3]: the two-hot sum is exact in fp32.  (quant: the round trips reach down to +-0 and up to 2^11, the sum
        # of two of them need not be a float32 — the quantised replays plant no two-hot step, _SimBase._pick_dup)
        assert quant or (bool((a >= 2.0 ** -6).all()) and bool((a < 16.0).all()))
        if quant:
            self.v_img, self.v_par, vb = Q.round_trip(self.v_all, dt, quant)
            self.v_deq = Q.to_tensor(vb, dt)
            assert bool(torch.isfinite(self.v_deq.double()).all()) and float(self.v_deq.double().abs().max()) < POISON_V
            for h in range(H):
                assert len({r.tobytes() for r in vb[h]}) == L, (self.id, h)
            assert float((vb != bits(self.v_all)).mean()) > 0.5, self.id
            assert bool((self.v_par[:, 1:] != self.v_par[:, :-1]).any(axis=-1).all()), self.id
            rows = torch.from_numpy(self.codes).to(dt)  # the keys: unscaled code words, one parameter pair for all of them
            self.k_img_tok, self.k_par_tok, kb = Q.round_trip(rows, dt, quant)
            assert np.array_equal(kb, bits(rows)), (self.id, "the round trip of a key row is not the identity")
            self.poison_img, self.poison_par, pb = Q.round_trip(torch.full((1, D), POISON_V, dtype=dt), dt, quant)
            assert np.array_equal(pb, bits(torch.full((1, D), POISON_V, dtype=dt)))
        n = D - 2 * self.rep * np.arange(0, self.nb + 1)
        for m in range(-D, D + 1):  # amp * n exact in the dtype
            assert float(torch.tensor(float(self.amp * m), dtype=torch.float64).to(dt)) == float(self.amp * m)
        sc = P.rounded_scores(n, self.amp, self.scale, dt)
        assert np.isfinite(sc).all()
        self.gap = float(sc[0] - sc[1:].max())
        assert self.gap >= GAP_MIN, (self.id, self.gap)
        # the group mean of k / 2 (k = 0 .. 2 R): float64 and float32 quotients round to one dtype value
        k = np.arange(2 * self.R + 1)
        g64 = _rnd_np(k / 2.0 / self.R, dt)
        g32 = _rnd_np((np.float32(0.5) * k.astype(np.float32) / np.float32(self.R)).astype(np.float64), dt)
        assert np.array_equal(g64, g32), self.id
        self.gm_half = g64

    def key_rows(self, toks):
        """[n, D] of dt: the code words of the tokens."""
        return torch.from_numpy(self.codes[np.asarray(toks)]).to(self.dt)

    def _seed_ring(self, rng, live_n, hh_head, W, protect_hi):
        """ring0 [H, S, W] float32, den0 [H, S]; planted[h]: the tied slots.  live_n[h]: the head's live slots are [0, live_n[h]);
        hh_head[h]: the head scores by the ring; protect_hi[h]: slots >= this are protected at the first step (not planted)."""
        H, S, dt = self.H, self.S, self.dt
        c0 = self.ctr0 % W
        ring = np.zeros((H, S, W), np.float32)
        cols = [c0, (c0 + 7) % W, (c0 + W // 2) % W, (c0 - 3) % W]  # overwritten first / after the wrap / never (W = 400) / the base
        self.col_keep = cols[3]
        for n, cidx in enumerate(cols):
            val = rng.integers(1, 25, (H, S)) / 8.0
            if n < 3:
                val = val * (rng.random((H, S)) < 0.5)
            ring[:, :, cidx] = val  # (the base column is written last: every unplanted slot sums to at least 1 / 8 ... 3)
        ring[:, :, cols[3]] = rng.integers(8, 25, (H, S)) / 8.0
        den = rng.choice(np.array([1, 2, 3, 4, W - 1, W, W + 7], np.int32), (H, S)).astype(np.int32)
        self.planted = [set() for _ in range(H)]
        self.odd_slot = [-1] * H
        need = 11 if dt == BF else 86
        for h in range(H):
            n = int(live_n[h])
            lo, hi = self.g, min(n, int(protect_hi[h])) - 1
            if hh_head[h] and hi > lo:
                want = {lo, hi, 63, 64, 127, 128}
                for cb in range(NEXT_KEY_CHUNK, n, NEXT_KEY_CHUNK):
                    want |= {cb - 1, cb}
                self.planted[h] = {s for s in want if lo <= s <= hi and s not in self.reserved[h]}
                for k, s in enumerate(sorted(self.planted[h])):  # one score, 0.125 / W, through min(denom, W) only: W, W + 7, W, ...
                    ring[h, s] = 0.0
                    ring[h, s, cols[3]] = 0.125
                    den[h, s] = W + 7 * (k % 2)
            if self.g > 0 and n >= self.g:  # the last slot the global rule protects scores below everything
                ring[h, self.g - 1] = 0.0
            if W >= need + 3:  # a window sum the dtype cannot hold: need x 3.0 + 0.125
                cand = [s for s in range(self.g + 5, n) if s not in self.planted[h] and s not in self.reserved[h]]
                if cand:
                    s = cand[0]
                    ring[h, s] = 0.0
                    free = [j for j in range(W) if j != cols[3]][:need]
                    ring[h, s, free] = 3.0
                    ring[h, s, cols[3]] = 0.125
                    self.odd_slot[h] = s
        assert np.array_equal(ring * 8, np.rint(ring * 8)) and ring.min() >= 0 and ring.max() <= 3
        return ring, den


class HybCase(_Case):
    """One hybrid replay: H heads cycling through STRATEGIES (offset by the start state n), each with a start count of its own."""

    family, W = "hyb", W_HYB
    KINDS = ("at", "below", "full", "few", "tile", "split")

    def __init__(self, dt, H, HQ, S, n, steps=12, quant=None):
        self.n = n
        self.id = f"hyb-{DT_NAME[dt]}-H{H}-HQ{HQ}-S{S}-st{n}"
        p0 = self.p0 = S + 40  # the first decode position: the prompt was longer than the cache
        self._common(dt, H, HQ, S, steps, p0 + steps, seed=n + 1, quant=quant)
        rng = np.random.default_rng(7919 * n + 31 * S + 3 * H + HQ)
        self.rows = policy_rows(S)
        self.strat = np.array([(h + 3 * n) % len(STRATEGIES) for h in range(H)], np.int64)
        self.ctr0 = W_HYB - 5
        rps = self.plan["rows_per_split"]
        g = self.g
        self.kind, self.cts0, self.budget0 = [], np.zeros(H, np.int32), np.zeros(H, np.int32)
        self.pos0 = np.full((H, S), -1, np.int32)
        self.special0, self.punc0 = np.zeros((H, S), np.uint8), np.zeros((H, S), np.uint8)
        self.reserved = [set() for _ in range(H)]
        protect_hi = np.zeros(H, np.int64)
        for h in range(H):
            flags, win, hhs = (int(x) for x in self.rows[self.strat[h]])
            budget = g + (NSP0 if flags & F_SPECIAL else 0) + (NPU0 if flags & F_PUNC else 0) + (win if flags & F_WIN else 0) + (hhs if flags & F_HH else 0)
            kind = self.KINDS[(h + n) % len(self.KINDS)]
            if not flags & (F_HH | F_WIN | F_FULL):  # the two policies that drop: full, at and below their budgets in turn
                kind = (("full", "at", "below") if flags & F_PUNC == 0 else ("at", "full", "few"))[n % 3]
            if flags == (F_SPECIAL | F_PUNC | F_HH) and n % 2 == 0:  # (see `below`)
                kind = "below"
            edge = [16, 17, 64, 65, 127, 128, 129][(h + 2 * n) % 7]
            # below: one slot under the budget — three under it on a punctuation head, which is then ONE under its budget right after the
            # first punctuation token (step 2) has raised both: the step after it appends only if it sees the bumped num_punc
            below = S - 1 if flags & F_FULL else budget - 3 if flags & F_PUNC else budget - 1
            c = {"at": budget if not flags & F_FULL else S - 3, "below": below, "full": S, "few": 9,
                 "tile": min(edge, S - 1), "split": min(rps + (h + n) % 3 - 1, S - 1)}[kind]
            c = max(6, min(int(c), S))
            self.kind.append(kind)
            self.cts0[h], self.budget0[h] = c, budget
            # positions: the g oldest, a random older subset, and the newest tokens as one block — win + 1 of them where the head has the
            # room, so that position p0 - win (unprotected by the STRICT window rule at the first step) is held
            rb = max(0, min(c - g, (win if flags & F_WIN else 5) + 1))
            older = np.sort(rng.choice(np.arange(g, p0 - rb), c - g - rb, replace=False)) if c - g - rb > 0 else np.zeros(0, np.int64)
            ps = np.concatenate([np.arange(min(g, c)), older, np.arange(p0 - rb, p0)]).astype(np.int32)
            if c >= 2 * g and (h + n) % 2 == 0:  # the first g SLOTS do not hold the first g POSITIONS
                ps[:g], ps[g:2 * g] = ps[g:2 * g].copy(), ps[:g].copy()
            assert len(ps) == c and len(set(ps.tolist())) == c
            self.pos0[h, :c] = ps
            sp = {s for s in (1, c // 2, c - 2) if 0 <= s < c}
            pu = {s for s in (c // 3, c - 3) if 0 <= s < c} - sp
            self.special0[h, sorted(sp)] = 1
            self.punc0[h, sorted(pu)] = 1
            self.reserved[h] = sp | pu
            protect_hi[h] = c - rb if flags & F_WIN else c
        hh = [bool(self.rows[self.strat[h], 0] & F_HH) for h in range(H)]
        self.ring0, self.den0 = self._seed_ring(rng, self.cts0, hh, W_HYB, protect_hi)
        for h in range(H):  # protected special / punctuation slots score below everything (heads without the flag evict them first)
            for s in self.reserved[h]:
                if s >= g:
                    self.ring0[h, s] = 0.0
        # the window head's lowest score sits at position p0 - win where it is held (the STRICT rule leaves it unprotected)
        for h in range(H):
            flags, win, _ = (int(x) for x in self.rows[self.strat[h]])
            if flags & F_WIN and flags & F_HH:
                w = np.nonzero(self.pos0[h] == p0 - win)[0]
                if len(w) and int(w[0]) >= g and int(w[0]) not in self.reserved[h]:
                    self.ring0[h, w[0]] = 0.0
                    self.planted[h].discard(int(w[0]))
        live = np.arange(S)[None, :] < self.cts0[:, None]
        assert (self.den0[live] >= 1).all()
        # what a head's queries look at first (see _SimBase._cands): the poison of its dead slots copies those tokens
        self.kpos0 = self.pos0.astype(np.int64).copy()
        for h in range(H):
            c = int(self.cts0[h])
            src = [s for s in (c - 1, 0, 15, 16, 63, 64, 127, 128, rps - 1, rps) if 0 <= s < c and s not in self.planted[h]]
            for k, s in enumerate(range(c, S)):
                self.kpos0[h, s] = self.pos0[h, src[k % len(src)]]
        self.mask0 = live.astype(np.uint8)


class RingCase(_Case):
    """One replay of KVCacheHeavyHitter with history_window_size W > 1: the fill levels of step_exact.Case."""

    family = "ring"

    def __init__(self, dt, H, HQ, S, W, fill, steps=12, seed=0, D=128, quant=None):
        assert fill in ("brim", "minus3", "sparse")
        self.W, self.fill, self.n = W, fill, seed
        self.id = f"ring-{DT_NAME[dt]}-H{H}-HQ{HQ}-S{S}-W{W}-{fill}" + (f"-D{D}" if D != 128 else "")
        self.T = T = S if fill == "brim" else S - 3 if fill == "minus3" else 70
        self.p0 = T
        self._common(dt, H, HQ, S, steps, T + steps, seed=seed + 1, D=D, quant=quant)
        self.w = W_REC
        rng = np.random.default_rng(7919 * seed + 31 * S + 3 * H + HQ + W)
        self.ctr0 = W - 5
        self.reserved = [set() for _ in range(H)]
        self.ring0, self.den0 = self._seed_ring(rng, [T] * H, [True] * H, W, [T - self.w] * H)
        self.ring0[:, T:], self.den0[:, T:] = 0.0, 0
        # clamp(denom, 1, W): a live slot with denominator 0 and window sum 0 BEHIND (at a higher index than) a slot at 0 / 2
        a, b = self.g + 1, self.g + 3
        for s, d in ((a, 2), (b, 0)):
            self.ring0[:, s], self.den0[:, s] = 0.0, d
            for h in range(H):
                self.planted[h].discard(s)
                if self.odd_slot[h] == s:
                    self.odd_slot[h] = -1
        self.pos0 = np.full((H, S), -1, np.int32)
        self.pos0[:, :T] = np.arange(T, dtype=np.int32)
        self.mask0 = (self.pos0 >= 0).astype(np.uint8)
        self.kpos0 = self.pos0.astype(np.int64).copy()
        rps = self.plan["rows_per_split"]
        for h in range(H):
            src = [s for s in (T - 1, 0, 15, 16, 63, 64, 127, 128, rps - 1, rps) if 0 <= s < T and s not in self.planted[h]]
            for k, s in enumerate(range(T, S)):
                self.kpos0[h, s] = self.pos0[h, src[k % len(src)]]


# ------------------------------------------------------------------------------------------------ the simulator
# the one-fault mutants (tests/test_step_exact_ring_host.py lists which case rejects which); numbered as in DESIGN 2.22
FAULTS = {1: "stale_k", 2: "drop_visible", 3: "drop_unwritten", 4: "mask_ignored", 5: "mask_next_head", 6: "win_ge", 7: "cts_le", 8: "global_pos",
          9: "no_protect", 10: "punc_per_head", 11: "punc_stale", 12: "col_plus1", 13: "keep_old", 14: "wsum_f32", 15: "no_min", 16: "hyb_reset",
          17: "ring_row_kept", 18: "clamp_no_low", 19: "tie_high", 20: "equal_max_zero"}
EQUIVALENT_FAULT = "punc_new"  # the issue's mutant 11 as worded: equivalent under the contract (module docstring)
HYB_ONLY = {2, 3, 5, 6, 7, 8, 9, 10, 11, 15, 16}
RING_ONLY = {17, 18}


class _SimBase:
    """State and the parts both families share: selection, attention by matching code words, the ring update."""

    def __init__(self, c, fault=None, dense=False):
        assert fault is None or fault in FAULTS.values() or fault == EQUIVALENT_FAULT
        self.c, self.fault, self.dense = c, fault, dense
        H, S = c.H, c.S
        self.pos, self.mask, self.kpos = c.pos0.copy(), c.mask0.copy(), c.kpos0.copy()
        live = self.mask == 1
        self.K = c.key_rows(self.kpos.reshape(-1)).view(H, S, c.D).clone()
        self.V = torch.full((H, S, c.D), POISON_V, dtype=c.dt)
        hs, ss = np.nonzero(live)
        self.V[hs, ss] = c.v_deq[hs, self.pos[hs, ss].astype(np.int64)]
        if c.quant:  # K and V above are the DEQUANTISED values; beside them the images and the [H, S, 4] parameter words.  POISON_V
            # "goes through the twin": the dead slots hold the image of a row of 2^14 under its own parameters
            Db = Q.image_width(c.D, c.quant)
            self.Kimg = c.k_img_tok[self.kpos]
            self.Vimg = np.tile(c.poison_img.reshape(1, 1, Db), (H, S, 1))
            vpar = np.tile(c.poison_par.reshape(1, 1, 2), (H, S, 1))
            self.Vimg[hs, ss], vpar[hs, ss] = c.v_img[hs, self.pos[hs, ss].astype(np.int64)], c.v_par[hs, self.pos[hs, ss].astype(np.int64)]
            self.par = Q.qparams(c.k_par_tok[self.kpos], vpar)
        self.ring, self.den, self.ctr = c.ring0.copy(), c.den0.copy(), int(c.ctr0)
        self.wsum = self.ring.sum(axis=2, dtype=np.float64)
        self.planted = [set(x) for x in c.planted]
        self.rng = np.random.default_rng(104729 * c.n + c.S + c.HQ)
        self.notes = set()
        self.col = None  # (index, values [H, S]) of the ring column the latest step wrote
        self.n_twohot = 0

    def wsum_dt(self):
        """The window sums as the device holds them: float32 values exact in the dtype."""
        if self.fault == "wsum_f32":
            return self.wsum.astype(np.float32)
        return _rnd_np(self.wsum, self.c.dt).astype(np.float32)

    def _argmin(self, sc):
        if self.fault == "tie_high":
            return len(sc) - 1 - int(np.argmin(sc[::-1]))
        return int(np.argmin(sc))

    # ---- what the queries select
    def _cands(self, h):
        """Live, unplanted slots on the boundaries, relative to THIS head's live slots: its last live slot (the partly filled last
        split of the head), slots 15/16 (a wave's tile), 63/64, 127/128 (workgroups), the two sides of a split boundary and of the
        head's own last split, the first slot."""
        c = self.c
        rps = c.plan["rows_per_split"]
        ok = self.mask[h] == 1
        for s in self.planted[h]:
            ok[s] = False
        live = np.nonzero(ok)[0]
        assert len(live), (c.id, h)
        ll = int(live[-1])
        last0 = (ll // rps) * rps
        order = [ll, 15, 16, 63, 64, 127, 128, rps - 1, rps, last0 - 1, last0, 0, 2 * rps - 1, 2 * rps]
        return [s for s in order if 0 <= s < c.S and ok[s]], live, ll

    def _pick_dup(self, h, new, i):
        """A token live in head h (one slot holds its code word, not `new`, not planted), placed relative to the slot `new`:
        the same 16-row tile, another tile of the same split, an earlier split, a later split — in turn."""
        c = self.c
        if c.quant:  # (the two-hot y is one bit pattern only while V1 + V2 is exact in fp32: see _Case._common)
            return None
        rps = c.plan["rows_per_split"]
        ok = self.mask[h] == 1
        ok[new] = False
        for s in self.planted[h]:
            ok[s] = False
        vals, cnt = np.unique(self.kpos[h][self.mask[h] == 1], return_counts=True)
        multi = set(vals[cnt > 1].tolist())
        live = [int(s) for s in np.nonzero(ok)[0] if int(self.kpos[h, s]) not in multi and int(self.kpos[h, s]) != int(self.kpos[h, new])]
        if not live:
            return None
        want = (i // 4 + h) % 4
        tests = [lambda s: s // 16 == new // 16, lambda s: s // rps == new // rps and s // 16 != new // 16, lambda s: s // rps < new // rps,
                 lambda s: s // rps > new // rps]
        for k in range(4):
            hit = [s for s in live if tests[(want + k) % 4](s)]
            if hit:
                return hit[(i + h) % len(hit)]
        return live[0]

    def _select(self, i, new, visible, dup_slot):
        """sel[j]: the token (code word) query head j selects.  Every third step head 0 of a group takes the token inserted in this
        very step where the head can see it; on a two-hot step head 1 takes the duplicated token; every third step the last head takes
        the head's last live slot; heads 0 and 1 otherwise walk the boundary slots of _cands; the others take random live slots."""
        c = self.c
        R = c.R
        rps = c.plan["rows_per_split"]
        sel = np.zeros(c.HQ, np.int64)
        slots = np.zeros(c.HQ, np.int64)
        for h in range(c.H):
            cand, live, ll = self._cands(h)
            for r in range(R):
                if i % 3 == 0 and r == 0 and visible[h]:
                    s = new[h]
                    self.notes.add("new")
                elif dup_slot[h] is not None and r == min(1, R - 1):
                    s = dup_slot[h]
                elif i % 3 == 1 and r == R - 1:
                    s = ll
                    self.notes.add("last_live")
                    if (ll + 1) % rps:
                        self.notes.add("last_live_of_partial_split")
                elif r < 2 and cand:
                    s = cand[(2 * (i + h) + r) % len(cand)]
                    if s in (15, 16):
                        self.notes.add("wave")
                    if s in (63, 64, 127, 128):
                        self.notes.add("workgroup")
                else:
                    s = int(live[self.rng.integers(len(live))])
                slots[h * R + r], sel[h * R + r] = s, self.kpos[h, s]
                if ((self.mask[h] == 0) & (self.kpos[h] == self.kpos[h, s])).any():
                    self.notes.add("poison_behind_selection")
            if len({int(x) // rps for x in slots[h * R:(h + 1) * R]}) > 1:
                self.notes.add("different_splits")
        return sel, slots

    # ---- attention
    def _attend(self, sel, mask_used, kpos_used):
        """-> (y [HQ, D] of dt, gm [H, S] float64 exact in dt).  A query matches the visible slots that hold its code word: n of
        them, each with probability dtype(1 / n) (n = 1: one-hot; n = 2: the two-hot step, 0.5 each)."""
        c, f = self.c, self.fault
        R, rps = c.R, c.plan["rows_per_split"]
        y = torch.zeros(c.HQ, c.D, dtype=torch.float64)
        half = np.zeros((c.H, c.S), np.int64)  # probability sums in units of 1 / 2
        other = np.zeros((c.H, c.S), np.float64)  # (mutants only: n > 2)
        Vd = self.V.double()
        for j in range(c.HQ):
            h = j // R
            m = np.nonzero((mask_used[h] == 1) & (kpos_used[h] == sel[j]))[0]
            if f == "equal_max_zero" and len(m) == 2 and m[0] // rps != m[1] // rps:
                m = m[:1]
            n = len(m)
            if f is None:
                assert n in (1, 2), (c.id, j, n)
            if n == 0:
                continue
            if n == 2:
                self.n_twohot += 1
            y[j] = Vd[h, m].sum(dim=0) / n
            if c.quant:  # a round trip may hold -0; 1 x (-0) + 0 x ... is +0
                y[j] += 0.0
            if n <= 2:
                half[h, m] += 2 // n
            else:
                other[h, m] += float(_rnd_np(np.array([1.0 / n]), c.dt)[0])
        if other.any():
            gm = _rnd_np((half / 2.0 + other) / R, c.dt)
        else:
            gm = c.gm_half[half]
        return y.to(c.dt), gm

    def _check_dense(self, q, sel, y, gm, where):
        """Small cases: the float64 evaluation of the attention contract (step_exact.attend_dense) returns the same bits."""
        c = self.c
        yd, _, gmd = attend_dense(q.double(), self.K.double(), self.V.double(), torch.from_numpy(self.mask.astype(bool)), c.scale, c.dt,
                                  c.plan["rows_per_split"], c.R)
        # (a two-hot sum that cancels to +0 exactly: the float64 evaluation adds exp(-gap) ~ 1e-157 of other rows and may return -0)
        yd, zero = yd.to(c.dt), (y == 0).numpy()
        assert np.array_equal(bits(yd)[~zero], bits(y)[~zero]) and bool((yd.double().numpy()[zero] == 0).all()), where
        assert np.array_equal(gmd.numpy(), gm), where

    # ---- history
    def _ring_update(self, gm):
        c, f = self.c, self.fault
        W = c.W
        col = (self.ctr + (1 if f == "col_plus1" else 0)) % W
        old = self.ring[:, :, col].astype(np.float64)
        if int(self.ctr) >= W and old.any():
            self.notes.add("wrap_drops_entry")
        if old.any():
            self.notes.add("entry_leaves_sum")
        self.ring[:, :, col] = gm.astype(np.float32)
        self.wsum += gm - (0.0 if f == "keep_old" else old)
        self.den += 1
        self.ctr += 1
        self.col = (col, gm.astype(np.float32))
        if int(self.ctr) % W == 0:
            self.notes.add("counter_wraps")
        if f is None and c.S <= 300:
            assert np.array_equal(self.wsum, self.ring.sum(axis=2, dtype=np.float64)), c.id

    def _write(self, h, s, k1, tok, p):
        """The insert: the token's rows — over the images their round trip, the image and the parameter words."""
        c = self.c
        self.K[h, s], self.V[h, s] = k1[h], c.v_deq[h, p]
        if c.quant:
            self.Kimg[h, s], self.Vimg[h, s] = c.k_img_tok[tok], c.v_img[h, p]
            self.par[h, s, :2], self.par[h, s, 2:] = c.k_par_tok[tok], c.v_par[h, p]

    def images(self):
        return dict(k_img=self.Kimg, v_img=self.Vimg, qparams=self.par)

    def buffers(self):
        return dict(pos=self.pos, mask=self.mask, cache_cts=self.cts, denom=self.den, counter=np.array([self.ctr], np.int64), wsum=self.wsum_dt())

    def ring_dt(self):
        return torch.from_numpy(self.ring).to(self.c.dt)


class HybSim(_SimBase):
    def __init__(self, c, fault=None, dense=False):
        super().__init__(c, fault, dense)
        self.cts = c.cts0.copy()
        self.special, self.punc = c.special0.copy(), c.punc0.copy()
        self.nsp, self.npu, self.npu_prev = NSP0, NPU0, NPU0

    def _candidate(self, h, p):
        c, f = self.c, self.fault
        flags, win, _ = (int(x) for x in c.rows[c.strat[h]])
        n = min(int(self.cts[h]), c.S)
        pos = self.pos[h, :n]
        if flags & F_HH:
            d = self.den[h, :n] if f == "no_min" else np.minimum(self.den[h, :n], c.W)
            with np.errstate(divide="ignore", invalid="ignore"):
                sc = self.wsum_dt()[h, :n] / d.astype(np.float32)
        else:
            sc = pos.astype(np.float32)
        save = (pos < c.g) if f == "global_pos" else (np.arange(n) < c.g)
        if f != "no_protect":
            if flags & F_SPECIAL:
                save = save | (self.special[h, :n] != 0)
            if flags & F_PUNC:
                save = save | (self.punc[h, :n] != 0)
        if flags & F_WIN:
            save = save | ((pos >= p - win) if f == "win_ge" else (pos > p - win))
        sc = np.where(save, np.float32(np.inf), sc).astype(np.float32)
        if len(sc) > 1 and np.isfinite(sc).sum() > 1:
            u = np.sort(sc[np.isfinite(sc)])
            if u[0] == u[1]:
                self.notes.add("tie_at_minimum")
        return self._argmin(sc)

    def step(self, i):
        """-> dict(p, tok, q [HQ, D], k1, v1 [H, D] of dt, y [HQ, D] of dt, idx [H], kinds [H])."""
        c, f = self.c, self.fault
        H, S = c.H, c.S
        p = c.p0 + i
        is_punc = i % 5 == 2
        npu_seen = self.npu_prev if f == "punc_stale" else self.npu + (1 if (f == "punc_new" and is_punc) else 0)
        idx, kinds = [], []
        for h in range(H):
            flags, win, hhs = (int(x) for x in c.rows[c.strat[h]])
            cts = int(self.cts[h])
            end = min(cts, S - 1)
            if (flags & F_PUNC and is_punc) or flags & F_FULL:
                kind, slot = "append", end
                self.notes.add("punc_append" if not flags & F_FULL else "full_append")
            else:
                budget = c.g + (self.nsp if flags & F_SPECIAL else 0) + (npu_seen if flags & F_PUNC else 0) + (win if flags & F_WIN else 0) + (hhs if flags & F_HH else 0)
                if cts < budget or (f == "cts_le" and cts == budget):
                    kind, slot = "append", end
                    self.notes.add("append_below_budget")
                elif flags & (F_HH | F_WIN):
                    kind, slot = "evict", self._candidate(h, p)
                    self.notes.add("evict_hh" if flags & F_HH else "evict_window")
                else:
                    kind, slot = "drop", S - 1
                    self.notes.add("drop_full" if cts >= S else "drop")
            idx.append(slot)
            kinds.append(kind)
        # two-hot steps: the incoming key of some heads is the code word of a token the head still holds
        toks = np.full(H, p, np.int64)
        dup_slot = [None] * H
        if i % 4 == 1 or i % 4 == 3:
            for h in range(H):
                if (h + i // 2) % 2 == 0:
                    s = self._pick_dup(h, idx[h], i)
                    if s is not None:
                        dup_slot[h], toks[h] = s, self.kpos[h, s]
        k1, v1 = c.key_rows(toks), c.v_all[:, p].clone()
        old_kpos = self.kpos.copy()
        visible = []
        for h in range(H):
            s, kind = idx[h], kinds[h]
            if kind == "evict" and f == "hyb_reset":
                self.wsum[h, s], self.den[h, s] = 0.0, 0
                self.ring[h, s] = 0.0
            if not (kind == "drop" and f == "drop_unwritten"):
                self._write(h, s, k1, toks[h], p)
                self.pos[h, s], self.kpos[h, s] = p, toks[h]
                if is_punc:
                    self.punc[h, s] = 1
            if kind == "append":
                self.mask[h, s] = 1
                self.cts[h] += 1
            self.planted[h].discard(s)
            visible.append(self.mask[h, s] == 1)
            if dup_slot[h] is not None:
                rps = c.plan["rows_per_split"]
                if not visible[h]:
                    self.notes.add("dup_dropped_invisible")
                else:
                    a, b = dup_slot[h], s
                    self.notes.add("dup_drop_full" if kind == "drop" else "twohot_" + kind)
                    self.notes.add("twohot_new_in_later_split" if b // rps > a // rps else "twohot_new_in_earlier_split" if b // rps < a // rps
                                   else "twohot_same_tile" if a // 16 == b // 16 else "twohot_other_tile")
        self.npu_prev = self.npu
        if is_punc:
            self.npu += H if f == "punc_per_head" else 1
        sel, slots = self._select(i, idx, visible, dup_slot)
        if any(kinds[h] == "drop" and visible[h] and slots[h * c.R] == S - 1 for h in range(H)):
            self.notes.add("dropped_token_selected_in_live_last_slot")
        q = torch.from_numpy(c.amp * c.codes[sel]).to(c.dt)
        mask_used, kpos_used = self.mask, self.kpos
        if f == "stale_k":
            kpos_used = self.kpos.copy()
            for h in range(H):
                kpos_used[h, idx[h]] = old_kpos[h, idx[h]]
        if f == "drop_visible":
            mask_used = self.mask.copy()
            for h in range(H):
                if kinds[h] == "drop":
                    mask_used[h, S - 1] = 1
        if f == "mask_ignored":
            mask_used = np.ones_like(self.mask)
        if f == "mask_next_head":
            mask_used = (np.arange(S)[None, :] < np.roll(self.cts, -1)[:, None]).astype(np.uint8)
        y, gm = self._attend(sel, mask_used, kpos_used)
        if f is None and self.dense:
            self._check_dense(q, sel, y, gm, f"{c.id} step {i}")
        self._ring_update(gm)
        return dict(p=p, tok=PUNC_TOK if is_punc else PLAIN_TOK, q=q, k1=k1, v1=v1, y=y, idx=idx, kinds=kinds, sel=sel, slots=slots)

    def buffers(self):
        out = super().buffers()
        out.update(punc_mask=self.punc, special_mask=self.special, num_punc=np.array([self.npu], np.int32), num_special=np.array([self.nsp], np.int32))
        return out


class RingSim(_SimBase):
    def __init__(self, c, fault=None, dense=False):
        super().__init__(c, fault, dense)
        self.cts = np.array([c.T], np.int32)

    def step(self, i):
        c, f = self.c, self.fault
        H, W = c.H, c.W
        p = c.p0 + i
        ws = self.wsum_dt()
        idx = []
        for h in range(H):
            d = np.minimum(self.den[h], W) if f == "clamp_no_low" else np.clip(self.den[h], 1, W)
            with np.errstate(divide="ignore", invalid="ignore"):
                sc = (ws[h] / d.astype(np.float32)).astype(np.float32)
            pos = self.pos[h]
            sc[(pos < c.g) | (pos >= p - c.w)] = np.float32(1.0)
            sc[pos == -1] = np.float32(0.0)
            u = np.sort(sc)
            if len(u) > 1 and u[0] == u[1]:
                self.notes.add("tie_at_minimum")
            idx.append(self._argmin(sc))
        was_empty = [self.pos[h, idx[h]] == -1 for h in range(H)]
        self.notes.add("fills_empty" if was_empty[0] else "evict_hh")
        toks = np.full(H, p, np.int64)
        dup_slot = [None] * H
        if i % 4 == 1 or i % 4 == 3:
            for h in range(H):
                if (h + i // 2) % 2 == 0:
                    s = self._pick_dup(h, idx[h], i)
                    if s is not None:
                        dup_slot[h], toks[h] = s, self.kpos[h, s]
        k1, v1 = c.key_rows(toks), c.v_all[:, p].clone()
        old_kpos = self.kpos.copy()
        rps = c.plan["rows_per_split"]
        for h in range(H):
            s = idx[h]
            self.den[h, s] = 0
            if f != "ring_row_kept":
                self.ring[h, s], self.wsum[h, s] = 0.0, 0.0
            self._write(h, s, k1, toks[h], p)
            self.pos[h, s], self.kpos[h, s], self.mask[h, s] = p, toks[h], 1
            self.planted[h].discard(s)
            if dup_slot[h] is not None:
                a, b = dup_slot[h], s
                self.notes.add("twohot_evict")
                self.notes.add("twohot_new_in_later_split" if b // rps > a // rps else "twohot_new_in_earlier_split" if b // rps < a // rps
                               else "twohot_same_tile" if a // 16 == b // 16 else "twohot_other_tile")
        self.cts[0] += int(was_empty[0])
        sel, slots = self._select(i, idx, [True] * H, dup_slot)
        q = torch.from_numpy(c.amp * c.codes[sel]).to(c.dt)
        mask_used, kpos_used = self.mask, self.kpos
        if f == "stale_k":
            kpos_used = self.kpos.copy()
            for h in range(H):
                kpos_used[h, idx[h]] = old_kpos[h, idx[h]]
        if f == "mask_ignored":
            mask_used = np.ones_like(self.mask)
        y, gm = self._attend(sel, mask_used, kpos_used)
        if f is None and self.dense:
            self._check_dense(q, sel, y, gm, f"{c.id} step {i}")
        self._ring_update(gm)
        return dict(p=p, tok=PLAIN_TOK, q=q, k1=k1, v1=v1, y=y, idx=idx, kinds=["evict"] * H, sel=sel, slots=slots)


def make_sim(c, fault=None, dense=False):
    return (HybSim if c.family == "hyb" else RingSim)(c, fault, dense)


# ------------------------------------------------------------------------------------------------ the case table
# (H, HQ, S) -> (waves, tiles per wave of the single launch (0: two launches only), the XCD-L2 transport possible)
HYB_SHAPES = {(2, 4, 130): (4, 0, False), (4, 28, 130): (4, 0, False), (3, 12, 130): (4, 1, False), (1, 8, 200): (4, 1, False),
              (8, 32, 200): (4, 1, True), (8, 64, 130): (4, 1, True), (16, 64, 1280): (8, 1, True), (8, 32, 4160): (4, 2, True)}
RING_SHAPES = [(2, 4, 130, 8), (4, 28, 130, 33), (8, 32, 200, 33), (16, 64, 1280, 8)]  # (H, HQ, S, W): always two launches
# the ring policy behind the VALU streaming pass (decode_attn_split_kernel; there the ring-specific part is the ring_col word block
# (0, 0, 0) writes, the rest is the combine pass): (dtype, H, HQ, S, W, D)
RING_VALU_SHAPES = [(BF, 2, 4, 130, 8, 64), (HF, 4, 28, 130, 33, 32)]
N_STATES = 3


def shape_list():
    """-> [(family, dt, H, HQ, S, W)]: one entry per parametrised test; each runs its three start states / fill levels."""
    out = []
    for dt in (BF, HF):
        out += [("hyb", dt, H, HQ, S, W_HYB) for (H, HQ, S) in HYB_SHAPES]
        out += [("ring", dt, H, HQ, S, W) for (H, HQ, S, W) in RING_SHAPES]
    return out + [("ring", dt, H, HQ, S, W, D) for (dt, H, HQ, S, W, D) in RING_VALU_SHAPES]


def unpack(t):
    """-> (family, dt, H, HQ, S, W, D): the entries from before the VALU shapes carry no D (128)."""
    return tuple(t) + ((128,) if len(t) == 6 else ())


def shape_id(t):
    fam, dt, H, HQ, S, W, D = unpack(t)
    return f"{fam}-{DT_NAME[dt]}-{H}-{HQ}-{S}-W{W}" + (f"-D{D}" if D != 128 else "")


def cases_of(t, steps=None):
    fam, dt, H, HQ, S, W, D = unpack(t)
    st = steps or (16 if S <= 300 else 12)
    if fam == "hyb":
        return [HybCase(dt, H, HQ, S, n + (3 if dt == HF else 0), steps=st) for n in range(N_STATES)]
    return [RingCase(dt, H, HQ, S, W, fill, steps=st, seed=n + (3 if dt == HF else 0), D=D) for n, fill in enumerate(("brim", "minus3", "sparse"))]


# ---- over the images: cc_decode_step_heavy_hitter_ring_quant (two launches) and cc_decode_step_hybrid_quant_rc
QUANT_RING_SHAPES = [(8, 32, 200, 33), (16, 64, 1280, 8), (1, 8, 200, 8)]
# (H, HQ, S) -> (waves, tiles per wave of the single launch): HYB_SHAPES with 4 or 8 query heads per kv head, and two more
QUANT_HYB_SHAPES = {(3, 12, 130): (4, 1), (1, 8, 200): (4, 1), (8, 32, 200): (4, 1), (8, 64, 130): (4, 1), (16, 64, 1280): (8, 1),
                    (8, 32, 4160): (4, 2), (16, 128, 1290): (8, 1), (8, 64, 4160): (4, 2)}


def quant_hybrid_plan(HQ, H, S, dt):
    """plan() for the hybrid step over the images (one_kernel_img, one_kernel kind 208): one launch with one tile per wave at 4 or 8
    waves, or up to eight tiles per wave at 4 waves; never the XCD-L2 transport (one_kernel_xl2 knows no hybrid image kernel)."""
    pl = plan(HQ, H, S, 128, dt)
    assert pl["rt"] in (4, 8) and HQ // H == pl["rt"]
    if not (pl["nt"] == 1 or (pl["nw"] == 4 and 1 < pl["nt"] <= 8)):
        pl["nt"] = 0
    return pl


def quant_shape_list():
    """-> [(family, dt, H, HQ, S, W, fmt)]"""
    out = []
    for fmt in Q.FORMATS:
        for dt in (BF, HF):
            out += [("hyb", dt, H, HQ, S, W_HYB, fmt) for (H, HQ, S) in QUANT_HYB_SHAPES]
            out += [("ring", dt, H, HQ, S, W, fmt) for (H, HQ, S, W) in QUANT_RING_SHAPES]
    return out


def quant_shape_id(t):
    fam, dt, H, HQ, S, W, fmt = t
    return f"{fmt}-{fam}-{DT_NAME[dt]}-{H}-{HQ}-{S}-W{W}"


def quant_cases_of(t, steps=None, states=None):
    """Hybrid: the three start states; ring: the three fill levels (cases_of's, over the images)."""
    fam, dt, H, HQ, S, W, fmt = t
    st = steps or (16 if S <= 300 else 12)
    off = 3 if dt == HF else 0
    if fam == "hyb":
        return [HybCase(dt, H, HQ, S, n + off, steps=st, quant=fmt) for n in (range(N_STATES) if states is None else states)]
    return [RingCase(dt, H, HQ, S, W, fill, steps=st, seed=n + off, quant=fmt) for n, fill in enumerate(("brim", "minus3", "sparse"))]


def intended_single_launch(c):
    """The hybrid step has a single-launch form where the plan has one and HQ / H is 4 or 8 with at most eight tiles; rings run two."""
    if c.family != "hyb":
        return False
    if c.quant:
        pl = quant_hybrid_plan(c.HQ, c.H, c.S, c.dt)
        assert (pl["nw"], pl["nt"]) == QUANT_HYB_SHAPES[(c.H, c.HQ, c.S)], (c.id, pl)
        return pl["nt"] > 0
    nw, nt, _ = HYB_SHAPES[(c.H, c.HQ, c.S)]
    assert (c.plan["nw"], c.plan["nt"] if c.R in (4, 8) else 0) == (nw, nt), (c.id, c.plan)
    return nt > 0


# ------------------------------------------------------------------------------------------------ drivers (the only users of cold_compress_amd)
def make_cache(c, dev):
    import cold_compress_amd.cache as cache

    quant = getattr(c, "quant", None)
    bits_ = Q.cache_bits(quant) if quant else None
    extra = dict(cache_quant_mode=quant) if quant else {}
    if c.family == "hyb":
        cls, rk = cache.get_cache_constructor("hybrid")
        kw = dict(max_cache_length=c.S, max_seq_length=c.S, cache_bits=bits_, global_tokens=c.g, token_ids=TOKEN_IDS, min_recovery_frac=0.9,
                  hybrid_strategies=STRATEGIES)
    else:
        cls, rk = cache.get_cache_constructor("heavy_hitter")
        kw = dict(max_cache_length=c.S, global_tokens=c.g, max_seq_length=4 * c.S + 64, cache_bits=bits_, history_window_size=c.W,
                  recent_window=c.w, attn_thresholding=False)
    with torch.device(dev):
        return cls(1, c.H, c.D, c.dt, **{k: kw[k] for k in rk}, **extra)


def _put_images(kv, sim, dev, lo=0):
    """Slots [lo, S) of the cache's images and parameter words <- the simulator's."""
    im = sim.images()
    kv.k_cache_q[0, :, lo:] = torch.from_numpy(im["k_img"][:, lo:]).to(dev)
    kv.v_cache_q[0, :, lo:] = torch.from_numpy(im["v_img"][:, lo:]).to(dev)
    kv.kv_qparams.view(torch.int32)[0, :, lo:] = torch.from_numpy(im["qparams"][:, lo:].view(np.int32)).to(dev)


def seed_cache(kv, c, sim, dev):
    """The decode-ready state without the profiling pass (hybrid), the prompt through the class's own prefill path (ring policy); then
    the seeded ring — the tracked window state is rebuilt from it by the class's own path (_window_state) at the first step."""
    H, S = c.H, c.S
    if c.family == "hyb":
        kv.cache_strategies = torch.from_numpy(c.strat).to(dev).contiguous()
        kv.requires_heavy_hitter = True
        assert np.array_equal(kv._policy_table().cpu().numpy(), c.rows), c.id
        kv.cache_cts.copy_(torch.from_numpy(c.cts0))
        kv.pos[0] = torch.from_numpy(c.pos0).to(dev)
        kv.mask[0, :, 0] = torch.from_numpy(c.mask0.astype(bool)).to(dev)
        kv.special_mask[0] = torch.from_numpy(c.special0.astype(bool)).to(dev)
        kv.punc_mask[0] = torch.from_numpy(c.punc0.astype(bool)).to(dev)
        kv.num_special.fill_(NSP0)
        kv.num_punc.fill_(NPU0)
        if c.quant:
            _put_images(kv, sim, dev)
        else:
            kv.k_cache.copy_(sim.K[None])
            kv.v_cache.copy_(sim.V[None])
    elif c.quant:  # the prompt's UNROUNDED rows through the class's own prefill (which quantises them); the poison as images
        T = c.T
        ip = torch.arange(T, device=dev)
        kv.update_kv(ip, sim.K[None, :, :T].contiguous().to(dev), c.v_all[None, :, :T].contiguous().to(dev), True)
        if T < S:
            _put_images(kv, sim, dev, lo=T)
    else:
        T = c.T
        ip = torch.arange(T, device=dev)
        kv.update_kv(ip, sim.K[None, :, :T].contiguous().to(dev), sim.V[None, :, :T].contiguous().to(dev), True)
        if T < S:  # the poison of the empty slots
            kv.k_cache[0, :, T:] = sim.K[:, T:].to(dev)
            kv.v_cache[0, :, T:] = sim.V[:, T:].to(dev)
    kv.attn_history_num.copy_(sim.ring_dt()[None])
    kv.attn_history_denom.copy_(torch.from_numpy(c.den0)[None])
    kv.attn_counter.fill_(int(c.ctr0))
    assert kv.supports_fused_step()


def read_cache(kv, c):
    out = dict(pos=kv.pos[0], mask=kv.mask[0, :, 0], cache_cts=kv.cache_cts, denom=kv.attn_history_denom[0], counter=kv.attn_counter,
               wsum=kv._window_state()[0])
    if c.family == "hyb":
        out.update(punc_mask=kv.punc_mask[0], special_mask=kv.special_mask[0], num_punc=kv.num_punc, num_special=kv.num_special)
    return out


def compare_small(kv, sim, where):
    """Every small buffer, the window sums and the ring column the step wrote, bit for bit.  -> elements compared."""
    got, exp = read_cache(kv, sim.c), sim.buffers()
    n = 0
    for name, e in exp.items():
        a, b = bits(got[name]).reshape(-1), bits(e).reshape(-1)
        assert a.shape == b.shape, (where, name, a.shape, b.shape)
        assert np.array_equal(a, b), f"{where}: {name}: {_first_diff(a, b)}"
        n += a.size
    if sim.col is not None:
        col, val = sim.col
        a = bits(kv.attn_history_num[0, :, :, col].contiguous()).reshape(-1)
        b = bits(torch.from_numpy(val).to(sim.c.dt)).reshape(-1)
        assert np.array_equal(a, b), f"{where}: ring column {col}: {_first_diff(a, b)}"
        n += a.size
    return n


def rebuilt_window_sums(kv, c):
    """cc_hh_ring_window_sums over the ring as it stands, into fresh buffers.  -> wsum [H, S] float32."""
    from cold_compress_amd import _abi
    from cold_compress_amd.cache import _DT, _ptr, _stream

    w = torch.zeros_like(kv.attn_window_sum)
    acc = torch.zeros_like(kv.attn_window_acc)
    _abi.call("cc_hh_ring_window_sums", _ptr(kv.attn_history_num), c.H, c.S, int(c.W), _DT[c.dt], _ptr(w), _ptr(acc), _stream())
    return w


def run_replay(c, form, dev, put=None, sync=None, dense=False, kv=None, steps=None):
    """One replay.  form: "three" (update_kv -> scaled_dot_product_attention(history=fused_history()) -> update_state), "two" / "one"
    (decode_step; the process-wide single-launch switch is the caller's).  kv: a cache object to run on again, after its reset().
    -> (cache object, elements compared exactly, the simulator)."""
    from cold_compress_amd.attention_utils import scaled_dot_product_attention as sdpa

    put = put or (lambda name, t: t.to(dev))
    sync = sync or (lambda: None)
    sim = make_sim(c, dense=dense)
    if kv is None:
        kv = make_cache(c, dev)
    else:
        kv.reset()
    seed_cache(kv, c, sim, dev)
    sync()
    n = compare_small(kv, sim, f"{c.id} [{form}] start state")
    if c.quant:
        from step_exact import compare_images

        assert form in ("two", "one"), "the fused quantised caches decode through decode_step() only"
        n += compare_images(kv, sim, f"{c.id} [{form}] start state", dev, dequant=True)
    mk, mv = (None, None) if c.quant else (sim.K.clone().to(dev), sim.V.clone().to(dev))
    small_kv = c.H * c.S * c.D <= (1 << 19)
    hyb = c.family == "hyb"
    for i in range(steps or c.steps):
        st = sim.step(i)
        where = f"{c.id} [{form}] step {i}"
        p = torch.tensor([st["p"]], dtype=torch.int32, device=dev)
        q = put("q", st["q"]).view(1, c.HQ, 1, c.D)
        k1 = put("k_new", st["k1"]).view(1, c.H, 1, c.D)
        v1 = put("v_new", st["v1"]).view(1, c.H, 1, c.D)
        ids = dict(input_ids=torch.tensor([[st["tok"]]], dtype=torch.int64, device=dev)) if hyb else {}
        if form == "three":
            ka, va, ma = kv.update_kv(p, k1, v1, False, **ids)
            hist = kv.fused_history()
            assert hist is not None and len(hist) == 6
            y, _ = sdpa(q, ka, va, attn_mask=ma, group_mean=True, history=hist)
            kv._state_fused = True
            kv.update_state(p, k1, v1, False, None, **ids)
        else:
            y = kv.decode_step(q, k1, v1, p, **ids)
        sync()
        a, b = bits(y).reshape(-1), bits(st["y"]).reshape(-1)
        assert np.array_equal(a, b), f"{where}: y: {_first_diff(a, b)} (heads select slots {st['slots'].tolist()}, insert at {st['idx']}: {st['kinds']})"
        n += a.size + compare_small(kv, sim, where)
        last = i == (steps or c.steps) - 1
        if c.quant:  # the images and the parameter words after every step; the device's decode of them after the last
            n += compare_images(kv, sim, where, dev, dequant=last)
            continue
        for h in range(c.H):
            if not (st["kinds"][h] == "drop" and sim.fault == "drop_unwritten"):
                mk[h, st["idx"][h]], mv[h, st["idx"][h]] = k1[0, h, 0], v1[0, h, 0]
        for name, got, mir, own in (("K", kv.k_cache[0], mk, sim.K), ("V", kv.v_cache[0], mv, sim.V)):
            assert torch.equal(got.view(torch.int16), mir.view(torch.int16)), f"{where}: {name} cache"
            if small_kv or last:
                assert np.array_equal(bits(got), bits(own)), f"{where}: {name} cache against the simulator's own copy"
            n += got.numel()
    where = f"{c.id} [{form}] after the last step"
    ring = kv.attn_history_num[0]
    assert torch.equal(ring.view(torch.int16), sim.ring_dt().to(dev).view(torch.int16)), f"{where}: the whole ring"
    n += ring.numel()
    tracked = kv._window_state()[0]
    a, b = bits(rebuilt_window_sums(kv, c)).reshape(-1), bits(tracked).reshape(-1)
    assert np.array_equal(a, b), f"{where}: window sums rebuilt from the ring against the tracked ones: {_first_diff(a, b)}"
    n += a.size
    return kv, n, sim
