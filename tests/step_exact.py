"""Known-answer inputs for the fused decode steps (decode_attn_split_mfma_kernel in all its instantiations, its two-launch twin, the
VALU streaming pass decode_attn_split_kernel<T, D, RT> that serves every fp32 cache and every 16-bit head_dim below 128, the
combine kernel; csrc/cc_attn_decode.hip, cc_attn_decode_kernels.h) and for the three-call sequence they replace.  A helper, not a
test: tests/test_step_exact_host.py holds the oracle's twins to these answers on the CPU, through the real cache classes, and shows
that the comparison has teeth (FAULTS below); tests/test_gpu_step_exact.py holds the kernels to them on the device.  CPU tensors only.

The SIMULATOR (class Sim, attend_dense, ramp_reference) is plain Python / numpy / torch-CPU arithmetic on integers, float32 and
float64.  It shares no code with the kernels, the oracle or tests/attn_ref.py; from tests/prefill_exact.py it takes the code words,
the rounded-score table and the dtype spacing only.  The drivers at the end (make_cache, run_replay, run_ramp) are the only part that
touches cold_compress_amd.

A. SELECTOR REPLAYS.  Token t (its position) has the +-1 code word of t over nbits = ceil(log2(T + steps)) bits as its key, each bit
   repeated D // nbits times, the remaining dimensions +1 (prefill_exact.code_words).  Query head j is amp * code(sel[j]); amp starts at
   128 and doubles while the measured gap is below GAP_MIN and amp * D < 16384 (128 at D = 128; 256 or 512 at small head dims, where
   few repeats of a code bit and a large scale leave 128 a gap of 128 only).  Every q . k is amp * n with an
   integer |n| <= D: exact in fp32 in any order, exact in bf16, exact and finite in fp16.  The dtype-rounded score of the selected key
   exceeds every other live key's by `gap`, MEASURED per case and asserted >= 150: exp(x - M) is then 0 in fp32 under any rounding or
   flush mode, every unselected probability is +0, the softmax sum is 1 and the selected probability is 1.  So, per step:
     y[j]   = the V row of the slot that holds sel[j], bit for bit, in all three forms (O carries weight 1 and l is 1 in any fold order);
     gm     = dtype(n / R) where n heads of the group select the slot, +0 elsewhere (R in {1, 2, 4, 8}: exact; R = 7: dtype(n / 7));
     num   += gm (float64, exact: the seeded history holds multiples of 1 / 8), denom += 1 for ALL slots, counter += 1;
     the slot of the next insert by the contract of include/coldcompress.h:
       heavy_hitter  avg = f32(num) / f32(max(denom, 1)); (pos < g) | (pos >= p - w) -> 1.0; pos == -1 -> 0.0 (applied last);
                     arg-min; the evicted slot's num and denom are zeroed
       recent_global g + argmin(pos[g:]);   full  argmin(pos) (the first empty slot while there is one)
       l2            dtype(f32(max over ALL heads and slots of key_norm) - f32(key_norm)); pos >= p - w -> +inf; slot < g -> +inf;
                     pos == -1 -> -inf; arg-min; the inserted key's norm dtype(sqrtf(sum of squares in fp32)) recorded
     ARG-MIN TIE RULE: the LOWEST slot index wins (numpy's argmin; torch.argmin; settled against the oracle's twins by the host test,
     which replays every planted tie through them).
   pos, mask, K, V, cache_cts, num, denom, attn_counter and key_norm are compared as bit patterns after every step.
   What the simulator chooses is described at Sim._select and Case._seed_history.

B. RAMP STEPS (16-bit dtypes; D = 128, and 64 / 32 / 16 behind the VALU pass).  One decode_step from a hand-set state.  Small integer
   entries plus one "position" dimension, scale 2^-3 at every D: every
   rounded score is ONE value on the device and here.  Reference: ramp_reference, a float64 evaluation of the contract.  Bounds:
   y: 1e-3 + 2 ulp_of(dtype) max|y_ref|; history increment per element: mean over the group's heads of step(p_ref) + step(gm_ref)
   (step = the dtype's spacing there, the smallest subnormal at 0).  ONE derived widening: the decode kernels' exponentials
   (fast_exp and exp_nonpos of csrc/cc_attn_decode_kernels.h) end in __builtin_amdgcn_exp2f, v_exp_f32, which returns 0 for a
   result below the smallest normal fp32: a probability p_ref < 2^-126 may be off by its whole value.  Everything else is equality.

C. THE FUSED QUANTISED CACHES (Case(quant=...): cache_quant_mode fused / fp8 / uint4 / mxfp4).  Family A over the images:
   keys are code words of which some rows are scaled by 2^-1 / 2^-2 under every policy (their round trip through the format is the
   identity, asserted; only full-scale rows are selected), values are block-scaled Gaussian rows whose ROUND TRIP through the numpy
   twin of the format (tests/kv_quant_twin.py) is what attention reads: the selected probability is still exactly 1 and y is the
   twin's round trip of one V row.  The simulator keeps, beside the dequantised K and V, the K and V images and the [H, S, 4]
   parameter words; an insert writes the twin's image and words of k_new / v_new, and the same step's attention reads their round
   trip.  Images and words are compared as bit patterns after every step.  The three-call form does not exist over the images."""
import math

import numpy as np
import torch

import kv_quant_twin as Q
import prefill_exact as P

BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32
DT_NAME = {BF: "bf16", HF: "f16", F32: "f32"}
ULP = {F32: 1e-5, BF: 2.0 ** -8, HF: 2.0 ** -11}  # the suite's unit roundoff
G_TOK, W_REC = 4, 5  # global tokens / recent window of every replay (full: 0 global tokens)
GAP_MIN = 150.0
POISON_V = 2.0 ** 14  # quantised sparse fills: every channel of the dead slots' V rows (the previous generation's data, as in 2.22)
POLICY_NAME = {"hh": "heavy_hitter", "rg": "recent_global", "full": "full", "l2": "l2"}


def _rnd(x, dt):
    """float64 tensor -> rounded to dt -> float64."""
    return x.to(dt).to(torch.float64)


def bits(t):
    """Bit patterns of a tensor / array as a numpy integer array (so that -0 != +0 and NaN == NaN)."""
    if isinstance(t, np.ndarray):
        return t.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[t.dtype.itemsize])
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.bool:
        return t.numpy().astype(np.uint8)
    return bits(t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]).numpy())


# ------------------------------------------------------------------------------------------------ the launch plan, mirrored
# plan() copies these lines of csrc: when one changes, update the mirror and the case tables of DESIGN 2.18 and 2.23.
MIRRORED_LINES = {
    "cc_attn_decode.hip": [
        "constexpr int kMaxSplit = 512;", "constexpr int kNW = 4;", "constexpr int kU = 4;",
        "return (64 / lpr) * kU * nw;",
        "p.rt = (R % 4 == 0) ? 4 : (R % 2 == 0) ? 2 : 1;",
        "if (R % 8 == 0 && cc_dt_size(dtype) == 2 && D == 128) p.rt = 8;",
        "if (wide_allowed && cc_dt_size(dtype) == 2 && D == 128 && (p.rt == 4 || p.rt == 8) && R == p.rt) {",
        "const long tiles = (long)H * ((S + 15) / 16);",
        "wide_max = e ? atol(e) : 256;",
        "if (tiles >= 1280 && (long)H * ((S + 127) / 128) <= wide_max) p.nw = 8;",
        "int ns_cap = (512 + H * zb - 1) / (H * zb);", "if (ns_cap < 16) ns_cap = 16;", "if (ns_cap > kMaxSplit) ns_cap = kMaxSplit;",
        "int ns = (S + rpi - 1) / rpi;", "int rps = (S + ns - 1) / ns;", "rps = ((rps + rpi - 1) / rpi) * rpi;", "ns = (S + rps - 1) / rps;",
        "if (cc_dt_size(dtype) != 2 || D != 128 || R != p.rt || p.n_split > 64 || H > kOneMaxHeads || p.rt > 8 || p.rows_per_split % rpi) return 0;",
        "return (nt <= kOneMaxTiles && (p.rt == 4 || p.rt == 8)) ? nt : 0;",
        "constexpr int kOneMaxTiles = 16;",
        "if (kind == -1 && H * p.n_split > 3 * p.nw * 64) return nullptr;",
        "if (allow_xl2 && (H & 7) == 0 && xl2_device_ok()) {",
    ],
    "cc_attn_decode_kernels.h": ["constexpr int kOneMaxHeads = 32;", "return __builtin_amdgcn_exp2f(x * 1.4426950408889634f);",
                                 "const float e = __builtin_amdgcn_exp2f(t);"],
    "cc_common.h": ["constexpr int kNextKeyChunk = 128;"],
}
NEXT_KEY_CHUNK = 128


def plan(HQ, H, S, D, dt, policy="hh"):
    """make_plan_w + one_tiles + the shape part of one_pick.  -> dict(nw, rt, n_split, rows_per_split, rpi, nt (tiles per wave of the
    single launch, 0: the shape has no single-launch form), xl2 (the head count allows the XCD-L2 transport))."""
    es = 4 if dt == F32 else 2
    R = HQ // H
    rt = 4 if R % 4 == 0 else 2 if R % 2 == 0 else 1
    if R % 8 == 0 and es == 2 and D == 128:
        rt = 8
    nw = 4
    if es == 2 and D == 128 and rt in (4, 8) and R == rt:
        if H * ((S + 15) // 16) >= 1280 and H * ((S + 127) // 128) <= 256:
            nw = 8
    rpi = (64 // (D // (16 // es))) * 4 * nw
    zb = R // rt
    ns_cap = min(max((512 + H * zb - 1) // (H * zb), 16), 512)
    ns = max(min((S + rpi - 1) // rpi, ns_cap), 1)
    rps = (S + ns - 1) // ns
    rps = (rps + rpi - 1) // rpi * rpi
    ns = (S + rps - 1) // rps
    nt = 0
    if not (es != 2 or D != 128 or R != rt or ns > 64 or H > 32 or rt > 8 or rps % rpi):
        nt = rps // rpi
        if nt != 1 and not (nt <= 16 and rt in (4, 8)):
            nt = 0
    if policy == "l2" and (nt != 1 or H * ns > 3 * nw * 64):
        nt = 0
    return dict(nw=nw, rt=rt, n_split=ns, rows_per_split=rps, rpi=rpi, nt=nt, xl2=(H % 8 == 0))


# ------------------------------------------------------------------------------------------------ A. the cases
def _gm_table(R, dt):
    return np.array([P.gm_value(n, R, dt) for n in range(R + 1)])


class Case:
    """One replay: the prompt state (k_all / v_all [H, T + steps, D] of dt: the rows of EVERY token, prompt and decode), the seeded
    heavy-hitter history, the l2 key scales, and the measured gap."""

    def __init__(self, policy, dt, H, HQ, S, D, fill, steps=12, hist="zeros", seed=0, quant=None):
        assert policy in POLICY_NAME and fill in ("brim", "minus3", "sparse") and 12 <= steps <= 24
        self.policy, self.dt, self.H, self.HQ, self.S, self.D, self.fill, self.steps, self.hist, self.seed = policy, dt, H, HQ, S, D, fill, steps, hist, seed
        self.quant = quant  # None, or the image format of the fused quantised cache (section C of DESIGN 2.24): kv_quant_twin.FORMATS
        assert quant is None or (quant in Q.FORMATS and policy in ("hh", "rg", "full") and D == 128 and dt in (BF, HF) and (HQ // H) in (4, 8))
        self.R = HQ // H
        assert self.R * H == HQ
        self.T = S if fill == "brim" else S - 3 if fill == "minus3" else (70 if S >= 130 else 20)
        self.id = f"{policy}-{DT_NAME[dt]}-H{H}-HQ{HQ}-S{S}-{fill}-{hist}" + (f"-D{D}" if D != 128 else "") + (f"-{quant}" if quant else "")
        self.g, self.w = (0 if policy == "full" else G_TOK), W_REC
        self.Hp = H if policy in ("hh", "l2") else 1
        self.scale = P.default_scale(D)
        self.plan = quant_plan(HQ, H, S, dt) if quant else plan(HQ, H, S, D, dt, policy)
        L = self.L = self.T + steps
        self.nb = P.nbits_for(L)
        codes, self.rep = P.code_words(L, D)
        self.codes = codes.astype(np.float32)  # [L, D] of +-1
        rng = np.random.default_rng(7919 * seed + 31 * S + 3 * H + HQ)
        # l2: some key rows scaled by 2^-1 or 2^-2, differently in every head (the norm maximum runs over all heads); decode tokens
        # of head h are scaled where (step + h) % 4 == 3.  quant: the same under every policy, so that K's row parameters differ
        # from slot to slot and a stale K scale is visible
        self.e = np.zeros((H, L), np.int64)
        if policy == "l2" or quant:
            for h in range(H):
                u = rng.random(L)
                lo = 0.25 + 0.4 * (h % 3) / 2.0  # share of scaled rows: 25 %, 45 %, 65 %
                self.e[h] = np.where(u < lo / 2, 2, np.where(u < lo, 1, 0))
                self.e[h, self.T:] = [1 if (i + h) % 4 == 3 else 0 for i in range(steps)]
        k = torch.from_numpy(self.codes)[None] * torch.from_numpy(2.0 ** -self.e.astype(np.float32))[:, :, None]
        self.k_all = k.to(dt)
        gen = torch.Generator().manual_seed(131 * seed + S + 7 * H)
        v = torch.randn(H, L, D, generator=gen, dtype=torch.float32)
        v = torch.where(v.abs() < 2.0 ** -6, torch.copysign(torch.tensor(2.0 ** -6), v), v)
        if quant:  # block b (32 channels) of token t times 2^(3 ((t + b) % 4) - 4): 2^-4 .. 2^5, every block of a row another power.
            # (Steps of 3, not 2: the largest of 32 Gaussians lies in (0.75, 6], three binades, so with steps of 2 two neighbouring
            # blocks can meet in one MXFP4 exponent and a row of 20 000 ends up with 2 distinct scale bytes; with 3 there are always 4.)
            tb = (np.arange(L)[:, None] + np.arange(D // 32)[None, :]) % 4
            v = v * torch.from_numpy(2.0 ** (3.0 * tb - 4.0)).to(torch.float32).repeat_interleave(32, dim=1)[None]
            # every row holds all four block factors, so a ROW parameter is that of 8 max|N(0, 1)| for every token: FP8's power of two
            # would be 2^-3 .. 2^-1 everywhere, and on the uint8 / uint4 grid two neighbours now and then share a bf16 minimum and
            # maximum.  Odd tokens times 16: consecutive tokens' V parameters differ in every format (asserted in _quantise)
            v = v * torch.from_numpy(16.0 ** (np.arange(L) % 2)).to(torch.float32)[None, :, None]
        self.v_all = v.to(dt)
        self.k_deq, self.v_deq = self.k_all, self.v_all  # what attention reads: the rows themselves, or their round trip
        if quant:
            self._quantise()
        self.gm_table = _gm_table(self.R, dt)
        # amp: 128, doubled while the measured gap is below GAP_MIN and the largest product still doubles within 16384 (128 at D = 128)
        self.amp = 128
        while self._gap() < GAP_MIN and self.amp * D < 16384:
            self.amp *= 2
        self._measure()
        self._seed_history(rng)

    def _quantise(self):
        """The twin's images, row parameters and round trips of every token's rows, and what the construction rests on."""
        fmt, dt = self.quant, self.dt
        self.k_img, self.k_par, kb = Q.round_trip(self.k_all, dt, fmt)
        self.v_img, self.v_par, vb = Q.round_trip(self.v_all, dt, fmt)
        assert np.array_equal(kb, bits(self.k_all)), (self.id, "the round trip of a key row is not the identity")
        self.v_deq = Q.to_tensor(vb, dt)
        assert bool(torch.isfinite(self.v_deq.double()).all())
        for h in range(self.H):  # the selected V row is known by its bits: the round-tripped rows of a head are pairwise distinct
            assert len({r.tobytes() for r in vb[h]}) == self.L, (self.id, h)
        self.changed = float((vb != bits(self.v_all)).mean())
        assert self.changed > 0.5, (self.id, self.changed)
        if fmt == "mxfp4":  # every row carries at least 3 distinct scale bytes
            sb = Q.MX.scale_bytes(self.v_par[..., 0])
            assert min(len(set(r.tolist())) for r in sb.reshape(-1, sb.shape[-1])) >= 3, self.id
        assert bool((self.v_par[:, 1:] != self.v_par[:, :-1]).any(axis=-1).all()), (self.id, "consecutive tokens share their V parameters")
        assert len({tuple(r) for r in self.k_par[0].tolist()}) >= 3  # (K: one parameter pair per scale 1, 1 / 2, 1 / 4)
        # dead slots hold what the class's own prefill leaves there (KVCache._prefill_update, fused branch: the model-dtype staging
        # pair is zeroed, the prompt's rows land in slots [0, T), then EVERY row of the staging pair goes through cc_kv_quant_rows):
        # the image and parameters of an all-zero row; and the previous generation's V data the driver puts there in the sparse fill
        z = torch.zeros(1, self.D, dtype=dt)
        self.zero_img, self.zero_par, zb = Q.round_trip(z, dt, fmt)
        assert not zb.any()
        self.poison_img, self.poison_par, pb = Q.round_trip(torch.full((1, self.D), POISON_V, dtype=dt), dt, fmt)
        assert np.array_equal(pb, bits(torch.full((1, self.D), POISON_V, dtype=dt)))

    def _gap(self):
        """The dtype-rounded score of the selected key minus the largest one of any other key, at the present amp."""
        n = self.D - 2 * self.rep * np.arange(0, self.nb + 1)  # q . k / amp by Hamming distance
        top = None
        rest = []
        for e in sorted(set(self.e.reshape(-1).tolist())):
            sc = P.rounded_scores(n * 2.0 ** -e, self.amp, self.scale, self.dt)
            assert np.isfinite(sc).all()
            if e == 0:
                top, sc = sc[0], sc[1:]
            rest.append(sc)
        return float(top - np.concatenate(rest).max())

    def _measure(self):
        """The gap on the dtype-rounded scores, and the exactness the construction rests on."""
        D, amp, dt = self.D, self.amp, self.dt
        assert amp * D < (1 << 24) and amp * D <= 16384
        for m in range(-D, D + 1):  # amp * n exact in the dtype
            assert float(torch.tensor(float(amp * m), dtype=torch.float64).to(dt)) == float(amp * m)
        self.gap = self._gap()
        assert self.gap >= GAP_MIN, (self.id, self.gap)
        lo = 2.0 ** -10 if self.quant else 2.0 ** -6  # (quant: the block factors reach down to 2^-4)
        assert bool((self.v_all.double().abs() >= lo).all()) and bool(torch.isfinite(self.v_all.double()).all())
        if self.policy == "l2":  # norm roundings are unique: four fp32 ulps either way round to the same dtype value
            for e in (0, 1, 2):
                x = np.float32(np.sqrt(np.float32(self.D * 4.0 ** -e)))
                lo, hi = x, x
                for _ in range(4):
                    lo, hi = np.nextafter(lo, np.float32(0)), np.nextafter(hi, np.float32(np.inf))
                vals = {float(torch.tensor(float(z), dtype=torch.float64).to(dt)) for z in (lo, x, hi)}
                assert len(vals) == 1, (self.id, e, vals)

    def norm_of(self, e):
        """dtype(sqrtf(fp32 sum of squares)) of a code-word row scaled by 2^-e, as float64."""
        x = np.float32(np.sqrt(np.float32(self.D * 4.0 ** -int(e))))
        return float(torch.tensor(float(x), dtype=torch.float64).to(self.dt))

    def _seed_history(self, rng):
        """heavy_hitter: num multiples of 1 / 8 in [1, 3], denom in 1 .. 4 (non-trivial rationals), then
        hist = "pairs": ONE value (1 / 8 over 4, below everything else for the whole replay) at the slot pairs 63/64 and 127/128, on
                either side of every kNextKeyChunk boundary, and at the first and the last unprotected slot: the evictions walk
                through them in index order, each one a tie across a wave, a chunk or a workgroup;
        hist = "zeros": a run of 70 slots at 0 (more than 64 tied at the minimum, across a wave and a chunk boundary) and a quarter
                of all slots at 0 with assorted denominators (mass ties)."""
        H, S, T = self.H, self.S, self.T
        self.num0 = np.zeros((H, S), np.float64)
        self.den0 = np.zeros((H, S), np.int32)
        self.planted = set()
        if self.policy != "hh":
            return
        self.num0[:, :T] = rng.integers(8, 25, (H, T)) / 8.0
        self.den0[:, :T] = rng.integers(1, 5, (H, T))
        first, last = self.g, T - self.w - 1  # positions g .. T - w - 1 are unprotected at the first step
        if self.hist == "pairs":
            want = {first, last, 63, 64, 127, 128}
            for cb in range(NEXT_KEY_CHUNK, T, NEXT_KEY_CHUNK):
                want |= {cb - 1, cb}
            self.planted = {s for s in want if first <= s <= last}
            for s in self.planted:
                self.num0[:, s], self.den0[:, s] = 0.125, 4
        else:
            lo = min(first + 56, max(first, last - 70))
            self.num0[:, lo:min(lo + 70, last + 1)] = 0.0
            self.den0[:, lo:min(lo + 70, last + 1)] = 2
            z = rng.random((H, T)) < 0.25
            self.num0[:, :T][z] = 0.0
        if self.g > 0:  # the last slot the global rule protects scores below everything: a global count one too small evicts it first
            self.num0[:, self.g - 1], self.den0[:, self.g - 1] = (0.125, 4) if self.hist == "pairs" else (0.0, 2)
        assert np.array_equal(self.num0 * 8, np.rint(self.num0 * 8))


# the one-fault mutants of the simulator (tests/test_step_exact_host.py shows which cases reject each)
FAULTS = ("stale_k", "stale_v", "tie_high", "tie_chunk", "recent_gt", "global_off", "denom_live", "no_zero", "stale_hist", "head_mod",
          "drop_last", "no_rescale", "masked_weight", "cts_skip", "dup_tail")
_ATTN_FAULTS = ("stale_k", "stale_v", "head_mod", "drop_last", "no_rescale", "masked_weight", "dup_tail")
# ... and of the quantised cases (Case.quant; tests/test_step_exact_quant_host.py):
#   stale_kparam / stale_vparam  the insert writes the image but keeps the slot's old K / V parameters
#   no_quant_new                 this step's attention reads the unrounded new token
#   nibble_swap                  the inserted rows' nibbles are swapped (4-bit formats)
#   block_scale0                 every block is decoded with block 0's scale (MXFP4)
#   poison_live                  masked_weight, seen through the poisoned V rows of the dead slots (sparse fill)
QUANT_FAULTS = ("stale_kparam", "stale_vparam", "no_quant_new", "nibble_swap", "block_scale0", "poison_live")


def quant_faults_of(fmt):
    return tuple(f for f in QUANT_FAULTS if (f != "nibble_swap" or fmt in Q.FOUR_BIT) and (f != "block_scale0" or fmt == "mxfp4"))


def attend_dense(q, K, V, mask, scale, dt, rps, R, fault=None):
    """The contract of cc_decode_attn_gqa in float64, evaluated split by split the way a streaming pass and a merge would (which
    changes nothing without a fault): q [HQ, D], K / V [H, S, D] float64 tensors, mask [H, S] bool.
    -> (y [HQ, D], p [HQ, S], gm [H, S]) float64 values exact in dt."""
    HQ, (H, S, D) = q.shape[0], K.shape
    y = torch.zeros(HQ, D, dtype=torch.float64)
    p = torch.zeros(HQ, S, dtype=torch.float64)
    nsp = (S + rps - 1) // rps
    for j in range(HQ):
        h = j % H if fault == "head_mod" else j // R
        s = _rnd(_rnd(K[h] @ q[j], dt) * scale, dt)
        s = torch.where(mask[h], s, torch.full_like(s, float("-inf")))
        parts = []
        for i in range(nsp):
            if fault == "drop_last" and nsp > 1 and i == nsp - 1:
                continue
            lo, hi = i * rps, min(S, (i + 1) * rps)
            x = s[lo:hi]
            m = float(x.max())
            if m == float("-inf"):
                if fault != "masked_weight":
                    continue
                parts.append((lo, hi, None, torch.ones(hi - lo, dtype=torch.float64)))
            else:
                parts.append((lo, hi, m, torch.exp(x - m)))
            if fault == "dup_tail" and hi - lo < rps and m != float("-inf"):
                # the VALU pass loads the rows past the end of a ragged split as copies of its last row (clamped to row_end - 1):
                # here one such copy carries weight — it enters l and O, and no slot's probability
                parts.append((hi - 1, hi, m, torch.exp(x[-1:] - m)))
        M = max(m for _, _, m, _ in parts if m is not None)
        Lsum, O = 0.0, torch.zeros(D, dtype=torch.float64)
        ws = []
        for lo, hi, m, e in parts:
            w = 1.0 if (m is None or fault == "no_rescale") else math.exp(m - M)
            ws.append(w)
            Lsum += w * float(e.sum())
            O += w * (e @ V[h, lo:hi])
        for (lo, hi, m, e), w in list(zip(parts, ws))[::-1]:  # (last to first: dup_tail's copy is overwritten by the row itself)
            p[j, lo:hi] = w * e / Lsum
        y[j] = O / Lsum
    p = _rnd(p, dt)
    gm = _rnd(p.reshape(H, R, S).mean(dim=1), dt)
    return _rnd(y, dt), p, gm


class Sim:
    """The state of one replay and its step function.  dense: evaluate the attention with attend_dense as well (small cases) and
    hold the one-hot answers to it."""

    def __init__(self, c, fault=None, dense=False):
        assert fault is None or fault in FAULTS or (c.quant and fault in quant_faults_of(c.quant))
        self.c, self.fault, self.dense = c, fault, dense or fault in _ATTN_FAULTS or fault in QUANT_FAULTS
        H, S, D, T = c.H, c.S, c.D, c.T
        self.pos = np.full((c.Hp, S), -1, np.int32)
        self.pos[:, :T] = np.arange(T, dtype=np.int32)
        self.mask = np.zeros((H, S), np.uint8)
        self.mask[:, :T] = 1
        self.cts = np.array([T], np.int32)
        self.K = torch.zeros(H, S, D, dtype=c.dt)
        self.V = torch.zeros(H, S, D, dtype=c.dt)
        self.K[:, :T], self.V[:, :T] = c.k_deq[:, :T], c.v_deq[:, :T]
        if c.quant:  # K and V above are the DEQUANTISED values (what attention reads); beside them the images and the parameter words
            Db = Q.image_width(D, c.quant)
            self.Kimg = np.tile(c.zero_img.reshape(1, 1, Db), (H, S, 1))
            self.Vimg = self.Kimg.copy()
            self.par = np.tile(Q.qparams(c.zero_par, c.zero_par).reshape(1, 1, 4), (H, S, 1))
            self.Kimg[:, :T], self.Vimg[:, :T] = c.k_img[:, :T], c.v_img[:, :T]
            self.par[:, :T] = Q.qparams(c.k_par[:, :T], c.v_par[:, :T])
            if c.fill == "sparse":  # the driver overwrites the dead slots' V image and V parameters (poison_cache); K is left alone
                self.Vimg[:, T:], self.par[:, T:, 2:], self.V[:, T:] = c.poison_img[0], c.poison_par[0], POISON_V
        self.scaled = bool(c.e.any())  # some key rows are scaled (l2; every quantised case): only full-scale rows are selected
        self.num, self.den, self.ctr = c.num0.copy(), c.den0.copy(), 0
        self.pre = None  # (num, denom) as they stood before the latest history update (the stale_hist mutant scores on them)
        self.norm = np.zeros((H, S), np.float64)
        if c.policy == "l2":
            tab = np.array([c.norm_of(e) for e in (0, 1, 2)])
            self.norm[:, :T] = tab[c.e[:, :T]]
        self.planted = [set(c.planted) for _ in range(H)]
        self.rng = np.random.default_rng(104729 * c.seed + c.S + c.HQ)
        self.notes = set()  # which of the situations of _select occurred (the host test asserts the coverage)

    # ---- eviction
    def _argmin(self, sc):
        f = self.fault
        if f == "tie_high":
            return len(sc) - 1 - int(np.argmin(sc[::-1]))
        if f == "tie_chunk":  # lowest index inside a 128-slot chunk, then the HIGHEST chunk among the tied ones
            best, bi = None, -1
            for lo in range(0, len(sc), NEXT_KEY_CHUNK):
                i = lo + int(np.argmin(sc[lo:lo + NEXT_KEY_CHUNK]))
                if best is None or sc[i] <= best:
                    best, bi = sc[i], i
            return bi
        return int(np.argmin(sc))

    def _evict(self, p):
        c, f = self.c, self.fault
        g = c.g + (-1 if f == "global_off" and c.g > 0 else 1 if f == "global_off" else 0)
        w = c.w
        if c.policy == "full":
            return [self._argmin(self.pos[0])]
        if c.policy == "rg":
            return [g + self._argmin(self.pos[0, g:])]
        idx = []
        if c.policy == "hh":
            num, den = self.pre if (f == "stale_hist" and self.pre is not None) else (self.num, self.den)
            for h in range(c.H):
                pos = self.pos[h]
                sc = num[h].astype(np.float32) / np.maximum(den[h], 1).astype(np.float32)
                recent = (pos > p - w) if f == "recent_gt" else (pos >= p - w)
                sc[(pos < g) | recent] = np.float32(1.0)
                sc[pos == -1] = np.float32(0.0)
                idx.append(self._argmin(sc))
            return idx
        mx = np.float32(self.norm.max())
        for h in range(c.H):
            pos = self.pos[h]
            d = (mx - self.norm[h].astype(np.float32)).astype(np.float32)
            sc = _rnd(torch.from_numpy(d.astype(np.float64)), c.dt).numpy()
            sc[pos >= p - w] = np.inf
            sc[:g] = np.inf
            sc[pos == -1] = -np.inf
            idx.append(self._argmin(sc))
        return idx

    # ---- what the queries select
    def _select(self, i, idx):
        """sel[j]: a token that is live AFTER this step's insert.  On every third step head 0 of every group selects the token
        inserted in this very step (where the policy lets it be selected); otherwise heads 0 and 1 of a group take the two sides of a
        boundary — slots 15/16 (a wave's tile), 63/64, 127/128 (workgroups of the 4- and the 8-wave plan), the two sides of a split
        boundary, the row before the last split and the LAST LIVE slot of the (partly filled) last split, the cache's first and last
        slot — and the other heads seeded live slots, i.e. other splits.  Cases with scaled key rows (l2, quant): full-scale slots only.  heavy_hitter with planted
        pairs: not the planted slots (their tie must survive until they are evicted)."""
        c = self.c
        S, R, pl = c.S, c.R, c.plan
        rps = pl["rows_per_split"]
        last0 = (pl["n_split"] - 1) * rps
        sel = np.zeros(c.HQ, np.int64)
        slots = np.zeros(c.HQ, np.int64)
        for h in range(c.H):
            row = self.pos[h if c.Hp > 1 else 0]
            ok = self.mask[h] == 1
            if self.scaled:
                ok = ok & (c.e[h][np.maximum(row, 0)] == 0)
            for s in self.planted[h]:
                ok[s] = False
            live_last = np.nonzero(ok[last0:])[0]
            ll = last0 + int(live_last[-1]) if len(live_last) else -1
            pairs = [(15, 16), (63, 64), (127, 128), (rps - 1, rps), (last0 - 1, ll), (0, S - 1), (c.T - 2, c.T - 1), (2 * rps - 1, 2 * rps)]
            if pl["nt"] == 0 and rps > pl["rpi"]:  # the VALU pass with several iterations of its row loop per split: their boundary
                pairs.append((pl["rpi"] - 1, pl["rpi"]))
            cand = [s for pr in pairs for s in pr if 0 <= s < S and ok[s]]
            every = np.nonzero(ok)[0]
            assert len(every), (c.id, i, h)
            new = idx[h if c.Hp > 1 else 0]
            for r in range(R):
                if i % 3 == 0 and r == 0 and ok[new]:
                    s = new
                    self.notes.add("new")
                elif i % 3 == 1 and r == R - 1 and ll >= last0:
                    s = ll
                    if S - last0 < rps or not ok[last0:].all():
                        self.notes.add("last_live_of_partial_split")
                elif (r < 2 or R == 1) and cand:
                    s = cand[((2 * (i + h) + r) if R > 1 else (i - i // 3 + h)) % len(cand)]
                    if s == ll and ll >= last0 and (S - last0 < rps or not ok[last0:].all()):
                        self.notes.add("last_live_of_partial_split")
                    if s in (15, 16):
                        self.notes.add("wave")
                    if s in (63, 64, 127, 128):
                        self.notes.add("workgroup")
                else:
                    s = int(every[self.rng.integers(len(every))])
                slots[h * R + r], sel[h * R + r] = s, row[s]
            if len({int(x) // rps for x in slots[h * R:(h + 1) * R]}) > 1:
                self.notes.add("different_splits")
        assert (sel >= 0).all()
        return sel, slots

    def _insert_images(self, h, s, p):
        """The insert writes the twin's image and words of k_new / v_new; "the inserted token is attended to through its image in
        the step that inserts it" (include/coldcompress.h, fused quantised KV cache): K / V hold the round trip from this step on."""
        c, f = self.c, self.fault
        ki, vi, kp, vp = c.k_img[h, p], c.v_img[h, p], c.k_par[h, p], c.v_par[h, p]
        if f == "nibble_swap":
            ki, vi = Q.swap_nibbles(ki), Q.swap_nibbles(vi)
        if f == "stale_kparam":
            kp = self.par[h, s, :2].copy()
        if f == "stale_vparam":
            vp = self.par[h, s, 2:].copy()
        self.Kimg[h, s], self.Vimg[h, s], self.par[h, s, :2], self.par[h, s, 2:] = ki, vi, kp, vp
        if f in ("nibble_swap", "stale_kparam", "stale_vparam"):
            with np.errstate(all="ignore"):
                self.K[h, s] = Q.to_tensor(Q.decode(ki[None], kp[None], c.dt, c.quant), c.dt)[0]
                self.V[h, s] = Q.to_tensor(Q.decode(vi[None], vp[None], c.dt, c.quant), c.dt)[0]

    def images(self):
        """The images and the [H, S, 4] parameter words as the cache classes hold them."""
        return dict(k_img=self.Kimg, v_img=self.Vimg, qparams=self.par)

    # ---- one step
    def step(self, i):
        """-> dict(p, q [HQ, D], k1, v1 [H, D] of dt, y [HQ, D] of dt (the answer), idx [Hp], sel, slots)."""
        c, f = self.c, self.fault
        H, R = c.H, c.R
        p = c.T + i
        idx = self._evict(p)
        hp = lambda h: h if c.Hp > 1 else 0  # noqa: E731
        was_empty = [self.pos[x, idx[x]] == -1 for x in range(c.Hp)]
        k1, v1 = c.k_all[:, p].clone(), c.v_all[:, p].clone()
        Kold, Vold = self.K, self.V
        if f in ("stale_k", "stale_v"):
            Kold, Vold = self.K.clone(), self.V.clone()
        for h in range(H):
            s = idx[hp(h)]
            if c.policy == "hh" and f != "no_zero":
                self.num[h, s], self.den[h, s] = 0.0, 0
            self.K[h, s], self.V[h, s] = c.k_deq[h, p], c.v_deq[h, p]
            if c.quant:
                self._insert_images(h, s, p)
            self.mask[h, s] = 1
            self.planted[h].discard(s)
            if c.policy == "l2":
                self.norm[h, s] = c.norm_of(c.e[h, p])
        for x in range(c.Hp):
            self.pos[x, idx[x]] = p
        if f != "cts_skip":
            self.cts[0] += int(was_empty[0])
        sel, slots = self._select(i, idx)
        q = torch.from_numpy(c.amp * c.codes[sel]).to(c.dt)
        for j in range(c.HQ):  # no selection of a dead token
            assert self.mask[j // R, slots[j]] == 1 and self.pos[hp(j // R), slots[j]] == sel[j]
            assert c.e[j // R, sel[j]] == 0  # l2: a full-scale key (the gap argument is untouched by the scaled rows)
        # the answers: one-hot probabilities
        y = torch.stack([self.V[j // R, slots[j]] for j in range(c.HQ)])
        if c.quant:  # a round trip may return -0 (MXFP4 keeps the sign of what it rounds to zero): O = 1 x (-0) + 0 x ... is +0
            y = (y.double() + 0.0).to(c.dt)
        cnt = np.zeros((H, c.S), np.int64)
        np.add.at(cnt, (np.arange(c.HQ) // R, slots), 1)
        gm = c.gm_table[cnt]
        if self.dense:
            Kd = (Kold if f == "stale_k" else self.K).double()
            Vd = (Vold if f == "stale_v" else self.V).double()
            if f == "no_quant_new":
                Kd, Vd = Kd.clone(), Vd.clone()
                for h in range(H):
                    Kd[h, idx[hp(h)]], Vd[h, idx[hp(h)]] = k1[h].double(), v1[h].double()
            if f == "block_scale0":
                Vd = Q.to_tensor(Q.decode(self.Vimg, self.par[..., 2:], c.dt, c.quant, block0=True), c.dt).double()
            if c.quant and f is None:  # the simulator's own books agree: K and V are the decoded images
                for img, w, t in ((self.Kimg, self.par[..., :2], self.K), (self.Vimg, self.par[..., 2:], self.V)):
                    assert np.array_equal(Q.decode(img, w, c.dt, c.quant), bits(t)), (c.id, i)
            with np.errstate(all="ignore"):
                yd, _, gmd = attend_dense(q.double(), Kd, Vd, torch.from_numpy(self.mask.astype(bool)), c.scale, c.dt, c.plan["rows_per_split"], R,
                                          "masked_weight" if f == "poison_live" else f)
            if f is None and c.quant:
                # (an element that is +-0 in the selected V row: the float64 evaluation multiplies +0 probabilities by negative
                # values and may return -0, where an accumulator that starts at +0 returns +0: zeros are compared by value)
                ydt, zero = yd.to(c.dt), (y == 0).numpy()
                assert np.array_equal(bits(ydt)[~zero], bits(y)[~zero]) and bool((ydt.double().numpy()[zero] == 0).all()), (c.id, i)
                assert np.array_equal(gmd.numpy(), gm), (c.id, i)
            elif f is None:
                assert np.array_equal(bits(yd.to(c.dt)), bits(y)) and np.array_equal(gmd.numpy(), gm), (c.id, i)
            y, gm = ((yd + 0.0) if c.quant else yd).to(c.dt), gmd.numpy()  # (quant: -0 -> +0, as in the answers above)
        if c.policy == "hh":
            self.pre = (self.num.copy(), self.den.copy())
            self.num += gm
            self.den += (self.mask.astype(np.int32) if f == "denom_live" else 1)
            self.ctr += 1
        return dict(p=p, q=q, k1=k1, v1=v1, y=y, idx=idx, sel=sel, slots=slots, was_empty=was_empty)

    def buffers(self):
        """The small buffers as the cache classes hold them (K and V are self.K / self.V)."""
        c = self.c
        out = dict(pos=self.pos, mask=self.mask, cache_cts=self.cts)
        if c.policy == "hh":
            out.update(num=self.num, denom=self.den, counter=np.array([self.ctr], np.int64))
        if c.policy == "l2":
            out["key_norm"] = torch.from_numpy(self.norm).to(c.dt)
        return out


# ------------------------------------------------------------------------------------------------ the case table (ISSUE / DESIGN 2.18)
ROW_4WAVE = [(2, 2, 67), (2, 4, 130), (3, 12, 130), (1, 8, 200)]
ROW_XL2 = [(8, 32, 200), (8, 64, 130)]
ROW_WIDE = [(16, 64, 1280), (16, 128, 1290)]
ROW_TILES = [(8, 32, 4160), (8, 32, 16448), (8, 64, 32832)]
ROW_L2 = [(2, 4, 130), (8, 32, 200), (16, 64, 1280)]
FILLS = ("brim", "minus3", "sparse")
# the VALU streaming pass (decode_attn_split_kernel<T, D, RT, 4, 4> + decode_attn_combine_kernel): every fp32 cache and every 16-bit
# cache with head_dim 16 / 32 / 64; two launches only.  (policy, dtype, H, HQ, S, D), one row per (dtype, D), RT = 4, 2, 1
VALU_SHAPES = [
    ("hh", BF, 2, 8, 130, 64), ("rg", BF, 3, 6, 67, 64), ("hh", BF, 32, 32, 2100, 64),
    ("hh", HF, 2, 8, 8300, 64), ("full", HF, 2, 12, 130, 64), ("hh", HF, 2, 14, 130, 64),
    ("hh", BF, 4, 48, 67, 32), ("rg", BF, 3, 6, 67, 32), ("hh", BF, 2, 2, 258, 32),
    ("hh", HF, 2, 8, 258, 32), ("hh", HF, 2, 4, 258, 32), ("full", HF, 1, 7, 130, 32),
    ("hh", BF, 2, 8, 515, 16), ("full", BF, 2, 4, 515, 16), ("hh", BF, 1, 1, 2200, 16),
    ("rg", HF, 1, 4, 67, 16), ("hh", HF, 3, 6, 67, 16), ("rg", HF, 2, 2, 77, 16),
    ("hh", F32, 16, 128, 600, 128), ("full", F32, 1, 8, 35, 128), ("rg", F32, 3, 6, 67, 128), ("hh", F32, 2, 2, 27, 128),
    ("hh", F32, 2, 8, 130, 64), ("full", F32, 3, 6, 61, 64), ("hh", F32, 1, 7, 130, 64),
    ("hh", F32, 2, 8, 130, 32), ("rg", F32, 3, 6, 258, 32), ("hh", F32, 2, 2, 67, 32),
    ("hh", F32, 2, 8, 258, 16), ("rg", F32, 3, 6, 67, 16), ("hh", F32, 2, 4, 77, 16), ("hh", F32, 1, 3, 515, 16),
]
# (element size, D, H, HQ, S) -> (waves, tiles per wave in the single launch (0: two launches only), the XCD-L2 transport possible)
INTENDED = {(2, 128) + k: v for k, v in {
    (2, 2, 67): (4, 1, False), (2, 4, 130): (4, 1, False), (3, 12, 130): (4, 1, False), (1, 8, 200): (4, 1, False),
    (8, 32, 200): (4, 1, True), (8, 64, 130): (4, 1, True), (16, 64, 1280): (8, 1, True), (16, 128, 1290): (8, 1, True),
    (8, 32, 4160): (4, 2, True), (8, 32, 16448): (4, 5, True), (8, 64, 32832): (4, 9, True), (4, 28, 130): (4, 0, False)}.items()}
INTENDED.update({(4 if dt == F32 else 2, D, H, HQ, S): (4, 0, False) for (_, dt, H, HQ, S, D) in VALU_SHAPES})


def intended(dt, D, H, HQ, S):
    return INTENDED[(4 if dt == F32 else 2, D, H, HQ, S)]


def valu_geometry(dt, D):
    """What decode_attn_split_kernel<T, D, RT, 4, 4> derives from sizeof(T) and D: VEC elements per 16-byte load, LPR lanes per
    row, RPW rows per wave load, rpi rows per workgroup iteration, NP pieces of the row-group partials, NG row groups to merge."""
    es = 4 if dt == F32 else 2
    vec = 16 // es
    lpr = D // vec
    rpw = 64 // lpr
    return dict(es=es, vec=vec, lpr=lpr, rpw=rpw, rpi=rpw * 16, np=2 if es == 2 else 1, ng=4 * rpw,
                passes={rt: -(-rt * 4 // lpr) for rt in (1, 2, 4)})


def shape_list():
    """-> [(policy, dt, H, HQ, S, D)]: one entry per parametrised test; each runs its three fill levels."""
    out = []
    for dt in (BF, HF):
        for (H, HQ, S) in ROW_4WAVE + ROW_XL2 + ROW_WIDE + ROW_TILES + [(4, 28, 130)]:
            out.append(("hh", dt, H, HQ, S, 128))
        for pol in ("rg", "full"):
            for (H, HQ, S) in ROW_4WAVE + ROW_XL2 + [(8, 32, 4160)]:
                out.append((pol, dt, H, HQ, S, 128))
        for (H, HQ, S) in ROW_L2:
            out.append(("l2", dt, H, HQ, S, 128))
    return out + VALU_SHAPES


def shape_id(t):
    pol, dt, H, HQ, S, D = t
    if D == 128 and dt != F32 or t == ("hh", F32, 2, 4, 77, 16):  # (the ids from before the VALU table)
        return f"{pol}-{DT_NAME[dt]}-{H}-{HQ}-{S}"
    return f"{pol}-{DT_NAME[dt]}-{H}-{HQ}-{S}-D{D}"


# ------------------------------------------------------------------------------------------------ C. the quantised caches
# (H, HQ, S): the plain step of cc_decode_step_quant over the images; every image format, bf16 and f16, forms "two" and "one"
QUANT_SHAPES = [(3, 12, 130), (1, 8, 200), (8, 32, 200), (8, 64, 130), (16, 64, 1280), (16, 128, 1290), (4, 16, 5120), (4, 32, 5120),
                (8, 32, 4160)]
QUANT_ALL_POLICIES = [(3, 12, 130), (8, 32, 200), (16, 64, 1280), (4, 32, 5120)]  # rg and full as well as hh
INTENDED.update({(2, 128, 4, 16, 5120): (8, 1, False), (2, 128, 4, 32, 5120): (8, 1, False)})
MIRRORED_QUANT_LINES = {"cc_attn_decode.hip": [
    "if (nt != 1) return nullptr; // as 8: one tile per wave",
    "if (kind != 0 && kind != 8 && kind != kQbFp8 && kind != kQbU4 && kind != kQbMx4 && kind != -1) return nullptr;",
    "if (kind == 208) { // hybrid over uint8 images: 4 or 8 query heads per kv head; one tile per wave or up to eight",
    "if (hyb) { // as 208: one tile per wave or up to eight",
]}


def quant_plan(HQ, H, S, dt):
    """plan() for the plain step over the images: the single launch exists with one tile per wave only (one_kernel, kind 8;
    one_kernel_img), over the memory hand-off or the XCD-L2 transport (one_kernel_xl2), 4 or 8 query heads per kv head."""
    pl = plan(HQ, H, S, 128, dt)
    assert pl["rt"] in (4, 8) and HQ // H == pl["rt"]
    pl["nt"] = 1 if pl["nt"] == 1 else 0
    return pl


def quant_shape_list():
    """-> [(policy, dt, H, HQ, S, fmt)]: one entry per parametrised test; each runs its three fill levels."""
    out = []
    for fmt in Q.FORMATS:
        for dt in (BF, HF):
            out += [("hh", dt, H, HQ, S, fmt) for (H, HQ, S) in QUANT_SHAPES]
            out += [(pol, dt, H, HQ, S, fmt) for pol in ("rg", "full") for (H, HQ, S) in QUANT_ALL_POLICIES]
    return out


def quant_shape_id(t):
    pol, dt, H, HQ, S, fmt = t
    return f"{fmt}-{pol}-{DT_NAME[dt]}-{H}-{HQ}-{S}"


def quant_cases_of(t, steps=None):
    """The three fill levels of one quantised shape (cases_of's alternation of the planted pairs and the runs of zeros)."""
    pol, dt, H, HQ, S, fmt = t
    out = []
    for n, fill in enumerate(FILLS):
        hist = "pairs" if (n + (dt == HF)) % 2 == 0 else "zeros"
        out.append(Case(pol, dt, H, HQ, S, 128, fill, steps=steps or (16 if S <= 300 else 12), hist=hist, seed=n + 1, quant=fmt))
    return out


def cases_of(t, steps=None):
    """The three fill levels of one shape.  The planted pairs and the runs of zeros alternate over the fill levels and the dtypes."""
    pol, dt, H, HQ, S, D = t
    out = []
    for n, fill in enumerate(FILLS):
        hist = "pairs" if (n + (dt == HF)) % 2 == 0 else "zeros"
        st = steps or (16 if S <= 300 else 12)
        out.append(Case(pol, dt, H, HQ, S, D, fill, steps=st, hist=hist, seed=n + 1))
    return out


# ------------------------------------------------------------------------------------------------ drivers (the only users of cold_compress_amd)
def make_cache(c, dev):
    import cold_compress_amd.cache as cache

    cls, rk = cache.get_cache_constructor(POLICY_NAME[c.policy])
    quant = getattr(c, "quant", None)
    kw = dict(max_cache_length=c.S, global_tokens=c.g, max_seq_length=4 * c.S + 64, cache_bits=Q.cache_bits(quant) if quant else None,
              history_window_size=1, recent_window=c.w, attn_thresholding=False)
    extra = dict(cache_quant_mode=quant) if quant else {}
    with torch.device(dev):
        return cls(1, c.H, c.D, c.dt, **{k: kw[k] for k in rk}, **extra)


def seed_cache(kv, c, dev):
    """The prompt through the class's own prefill path, then the seeded history."""
    T = c.T
    ip = torch.arange(T, device=dev)
    k0, v0 = c.k_all[None, :, :T].contiguous().to(dev), c.v_all[None, :, :T].contiguous().to(dev)
    kv.update_kv(ip, k0, v0, True)
    if c.policy == "l2":
        kv.update_state(ip, k0, v0, True, None)
    if c.policy == "hh":
        kv.attn_history_num[0, :, :, 0] = torch.from_numpy(c.num0).to(dev)
        kv.attn_history_denom[0] = torch.from_numpy(c.den0).to(dev)
    if getattr(c, "quant", None) and c.fill == "sparse":
        poison_cache(kv, c, dev)


def poison_cache(kv, c, dev):
    """Stale images: the dead slots' V image and V parameters become those of a row of POISON_V in every channel (the previous
    generation's data; a masked slot that carried weight would show at once).  K is left alone; the answers do not change."""
    T = c.T
    kv.v_cache_q[0, :, T:] = torch.from_numpy(c.poison_img[0]).to(dev)
    kv.kv_qparams.view(torch.int32)[0, :, T:, 2:] = torch.from_numpy(c.poison_par[0].view(np.int32)).to(dev)


def read_cache(kv, c):
    out = dict(pos=kv.pos[0], mask=kv.mask[0, :, 0], cache_cts=kv.cache_cts)
    if c.policy == "hh":
        out.update(num=kv.attn_history_num[0, :, :, 0], denom=kv.attn_history_denom[0], counter=kv.attn_counter)
    if c.policy == "l2":
        out["key_norm"] = kv.key_norm[0]
    return out


def _first_diff(a, b):
    w = np.argwhere(a != b)
    return f"{len(w)} of {a.size} differ, first at {w[0].tolist()}: got 0x{int(a[tuple(w[0])]):x}, expected 0x{int(b[tuple(w[0])]):x}"


def compare_small(kv, sim, where):
    """Every small buffer against the simulator, bit for bit.  -> elements compared."""
    got, exp = read_cache(kv, sim.c), sim.buffers()
    n = 0
    for name, e in exp.items():
        a, b = bits(got[name]).reshape(-1), bits(e).reshape(-1)
        assert a.shape == b.shape, (where, name, a.shape, b.shape)
        assert np.array_equal(a, b), f"{where}: {name}: {_first_diff(a, b)}"
        n += a.size
    return n


def run_replay(c, form, dev, put=None, sync=None, dense=False, full_kv_every_step=None, kv=None):
    """One replay on a fresh cache object.  form: "three" (update_kv -> scaled_dot_product_attention -> update_state), "two" /
    "one" (decode_step with single_launch False / True; the process-wide switch of the head-constant policies is the caller's).
    put(name, tensor): place an input on the device (the GPU test adds its NaN margins there).  K and V are compared on `dev`
    against a mirror that receives the simulator's inserts, and against the simulator's own tensors where they are small.
    kv: a cache object to run on again, after its reset().
    -> (cache object, elements compared exactly)."""
    from cold_compress_amd.attention_utils import scaled_dot_product_attention as sdpa

    put = put or (lambda name, t: t.to(dev))
    sync = sync or (lambda: None)
    sim = Sim(c, dense=dense)
    if kv is None:
        kv = make_cache(c, dev)
    else:
        kv.reset()
    if c.policy == "hh":
        kv.single_launch = form == "one"
    seed_cache(kv, c, dev)
    sync()
    n = compare_small(kv, sim, f"{c.id} [{form}] after prefill")
    if c.quant:
        assert form in ("two", "one"), "the fused quantised caches decode through decode_step() only"
        return kv, n + _replay_quant(c, form, dev, kv, sim, put, sync)
    mk, mv = sim.K.clone().to(dev), sim.V.clone().to(dev)
    small_kv = c.H * c.S * c.D <= (1 << 19) if full_kv_every_step is None else full_kv_every_step
    itype = torch.int32 if c.dt == F32 else torch.int16
    for i in range(c.steps):
        st = sim.step(i)
        where = f"{c.id} [{form}] step {i}"
        p = torch.tensor([st["p"]], dtype=torch.int32, device=dev)
        q = put("q", st["q"]).view(1, c.HQ, 1, c.D)
        k1 = put("k_new", st["k1"]).view(1, c.H, 1, c.D)
        v1 = put("v_new", st["v1"]).view(1, c.H, 1, c.D)
        if form == "three":
            ka, va, ma = kv.update_kv(p, k1, v1, False)
            if c.policy == "hh":
                y, attn = sdpa(q, ka, va, attn_mask=ma, return_attn=True, group_mean=True)
                kv.update_state(p, k1, v1, False, attn)
            else:
                y, _ = sdpa(q, ka, va, attn_mask=ma)
                kv.update_state(p, k1, v1, False, None)
        else:
            y = kv.decode_step(q, k1, v1, p)
        sync()
        a, b = bits(y).reshape(-1), bits(st["y"]).reshape(-1)
        assert np.array_equal(a, b), f"{where}: y: {_first_diff(a, b)} (heads select slots {st['slots'].tolist()}, insert at {st['idx']})"
        n += a.size + compare_small(kv, sim, where)
        for h in range(c.H):
            s = st["idx"][h if c.Hp > 1 else 0]
            mk[h, s], mv[h, s] = k1[0, h, 0], v1[0, h, 0]
        for name, got, mir, own in (("K", kv.k_cache[0], mk, sim.K), ("V", kv.v_cache[0], mv, sim.V)):
            assert torch.equal(got.view(itype), mir.view(itype)), f"{where}: {name} cache"
            if small_kv or i == c.steps - 1:
                assert np.array_equal(bits(got), bits(own)), f"{where}: {name} cache against the simulator's own copy"
            n += got.numel()
    return kv, n


def compare_images(kv, sim, where, dev, dequant=False):
    """The images and the [H, S, 4] parameter words against the simulator's, bit for bit; dequant: also the device's own decode of
    its images (cc_kv_dequant_rows) against the simulator's dequantised K and V.  -> elements compared."""
    n = 0
    exp = sim.images()
    for name, got, e in (("K image", kv.k_cache_q[0], exp["k_img"]), ("V image", kv.v_cache_q[0], exp["v_img"]),
                         ("qparams words", kv.kv_qparams[0].view(torch.int32), exp["qparams"].view(np.int32))):
        if not torch.equal(got, torch.from_numpy(e).to(dev)):
            a, b = bits(got), bits(e)
            raise AssertionError(f"{where}: {name}: {_first_diff(a, b)}")
        n += got.numel()
    if dequant:
        k, v = kv.dequantized_kv()
        for name, got, own in (("K", k[0], sim.K), ("V", v[0], sim.V)):
            a, b = bits(got), bits(own)
            assert np.array_equal(a, b), f"{where}: dequantised {name}: {_first_diff(a, b)}"
            n += a.size
    return n


def _replay_quant(c, form, dev, kv, sim, put, sync):
    """The steps of a quantised replay (run_replay): y and the small buffers as in 16 bits, and the images and parameter words after
    every step.  -> elements compared exactly."""
    n = compare_images(kv, sim, f"{c.id} [{form}] after prefill", dev, dequant=True)
    for i in range(c.steps):
        st = sim.step(i)
        where = f"{c.id} [{form}] step {i}"
        p = torch.tensor([st["p"]], dtype=torch.int32, device=dev)
        q = put("q", st["q"]).view(1, c.HQ, 1, c.D)
        k1 = put("k_new", st["k1"]).view(1, c.H, 1, c.D)
        v1 = put("v_new", st["v1"]).view(1, c.H, 1, c.D)
        y = kv.decode_step(q, k1, v1, p)
        sync()
        a, b = bits(y).reshape(-1), bits(st["y"]).reshape(-1)
        assert np.array_equal(a, b), f"{where}: y: {_first_diff(a, b)} (heads select slots {st['slots'].tolist()}, insert at {st['idx']})"
        n += a.size + compare_small(kv, sim, where) + compare_images(kv, sim, where, dev, dequant=(i == c.steps - 1))
    return n


# ------------------------------------------------------------------------------------------------ B. ramp steps
RAMP_SCALE = 2.0 ** -3
RAMP_VARIANTS = ("up", "down", "new_max", "last_live", "steep")
RAMP_SHAPES = ROW_4WAVE + ROW_WIDE + ROW_TILES
# (H, HQ, S, D): the VALU pass at 16-bit head dims 64 / 32 / 16 — its only cases with fractional softmax weights (the rescale across
# two iterations of the row loop, the LDS merge of up to 128 row groups with different maxima).  The scale stays RAMP_SCALE, passed
# explicitly (it is the default scale at D = 64 only); keys in {-1, 0, 1} plus the position dimension fit any D >= 2
RAMP_VALU_SHAPES = [(2, 8, 130, 64), (32, 32, 2100, 64), (3, 6, 67, 32), (2, 8, 515, 16)]


class RampCase:
    """One heavy-hitter decode step from a hand-set state.  Keys: entries in {-1, 0, 1} and dimension 0 the "position" value k0;
    queries: entries in {-1, 0, 1} and q[0] = 8; scale 2^-3: score = dtype(dtype(8 k0 + small integer) / 8).
      up        k0 = s A // S (A = min(S // 4, 256)): the running maximum moves at every merge
      down      the same, falling
      new_max   up, and the token inserted in this step carries A + 20
      last_live k0 = 0 but 30 at the last live slot of the partly filled last split (brim: slot S - 1; sparse: slot T - 1)
      steep     k0 = 2 (s 200 // S): whole splits sit more than 110 below the maximum; their weight underflows to 0
    History: num = 0 and denom = 2 in every live slot, so that the float64 accumulator holds this step's group mean EXACTLY (added to
    a history of 2.0, a probability below 2^-53 would be lost in the addition and with it the check of the small ones).  All scores
    tie at 0, the empty slots' included: the insert goes to the lowest unprotected index, slot g, at both fill levels (the tie rule
    family A pins); sparse = T = 70 (20 below S = 130) live slots, every later split masked."""

    policy, hist = "hh", "ramp"

    def __init__(self, dt, H, HQ, S, variant, fill, seed=0, D=128):
        assert variant in RAMP_VARIANTS and fill in ("brim", "sparse") and D >= 2
        self.dt, self.H, self.HQ, self.S, self.D, self.variant, self.fill = dt, H, HQ, S, D, variant, fill
        self.R, self.Hp, self.g, self.w, self.scale = HQ // H, H, G_TOK, W_REC, RAMP_SCALE
        self.T = T = S if fill == "brim" else (70 if S >= 130 else 20)
        self.id = f"ramp-{DT_NAME[dt]}-H{H}-HQ{HQ}-S{S}-{variant}-{fill}" + (f"-D{D}" if D != 128 else "")
        self.plan = plan(HQ, H, S, D, dt)
        rng = np.random.default_rng(4241 * seed + 17 * S + HQ + 5 * RAMP_VARIANTS.index(variant) + (fill == "sparse"))
        k = rng.integers(-1, 2, (H, T + 1, D)).astype(np.float32)
        q = rng.integers(-1, 2, (HQ, D)).astype(np.float32)
        q[:, 0] = 8.0
        sl = np.arange(T + 1)
        A = 400 if variant == "steep" else min(max(S // 4, 16), 256)
        ramp = 2 * (sl * 200 // S) if variant == "steep" else sl * A // S  # (even above 256: exact in bf16)
        self.evict = G_TOK  # the slot the insert goes to (asserted against the contract in ramp_reference)
        if variant == "down":
            ramp = (S - 1 - sl) * A // S
        if variant == "last_live":
            ramp = np.zeros(T + 1, np.int64)
            ramp[(S - 1) if fill == "brim" else (T - 1)] = 30
        k[:, :, 0] = ramp[None, :]
        if variant == "new_max":
            k[:, T, 0] = A + 20
        elif variant in ("up", "steep", "down"):
            k[:, T, 0] = ramp[self.evict]
        else:
            k[:, T, 0] = 0
        assert np.abs(k[:, :, 1:]).max() <= 1 and k[:, :, 0].max() <= 512 and np.abs(q).max() <= 8
        self.k_all = torch.from_numpy(k).to(dt)
        self.q = torch.from_numpy(q).to(dt)
        assert torch.equal(self.k_all.float(), torch.from_numpy(k))  # (exact in the dtype)
        gen = torch.Generator().manual_seed(977 * seed + S + HQ)
        self.v_all = torch.randn(H, T + 1, D, generator=gen).to(dt)
        self.num0 = np.zeros((H, S), np.float64)
        self.den0 = np.zeros((H, S), np.int32)
        self.den0[:, :T] = 2
        self._exp = None


def ramp_reference(c):
    """A float64 evaluation of the contract for the one step.  -> dict(idx [H], pos, mask, cache_cts, denom, counter, K, V (tensors of
    dt), num_before [H, S] (after the eviction's zeroing), y [HQ, D], p [HQ, S], gm [H, S] float64 values exact in dt, bound_y,
    bound_num [H, S])."""
    if c._exp is not None:
        return c._exp
    H, S, D, T, R, dt = c.H, c.S, c.D, c.T, c.R, c.dt
    p = T
    pos = np.full((H, S), -1, np.int32)
    pos[:, :T] = np.arange(T)
    mask = np.zeros((H, S), np.uint8)
    mask[:, :T] = 1
    num, den = c.num0.copy(), c.den0.copy()
    sc = num.astype(np.float32) / np.maximum(den, 1).astype(np.float32)
    sc[(pos < c.g) | (pos >= p - c.w)] = np.float32(1.0)
    sc[pos == -1] = np.float32(0.0)
    idx = sc.argmin(axis=1)
    assert (idx == c.evict).all(), (c.id, idx)
    K = torch.zeros(H, S, D, dtype=dt)
    V = torch.zeros(H, S, D, dtype=dt)
    K[:, :T], V[:, :T] = c.k_all[:, :T], c.v_all[:, :T]
    hs = np.arange(H)
    was_empty = pos[hs, idx] == -1
    num[hs, idx], den[hs, idx] = 0.0, 0
    K[hs, idx], V[hs, idx] = c.k_all[:, T], c.v_all[:, T]
    pos[hs, idx], mask[hs, idx] = p, 1
    cts = np.array([T + int(was_empty[0])], np.int32)
    Kd, Vd, qd = K.double(), V.double(), c.q.double().view(H, R, D)
    dots = torch.einsum("hrd,hsd->hrs", qd, Kd)
    assert float(dots.abs().max()) < 2 ** 24 and torch.equal(dots, dots.round())
    s = _rnd(_rnd(dots, dt) * c.scale, dt)
    assert bool(torch.isfinite(s).all())
    live = torch.from_numpy(mask.astype(bool))[:, None, :]
    s = torch.where(live, s, torch.full_like(s, float("-inf")))
    pr = _rnd(torch.softmax(s, dim=-1), dt)
    y = _rnd(torch.einsum("hrs,hsd->hrd", pr, Vd), dt).reshape(c.HQ, D)
    gm = _rnd(pr.mean(dim=1), dt)
    pn = pr.numpy()
    sp = P.step_of(pn, dt)
    sp = np.where(pn < 2.0 ** -126, np.maximum(sp, pn), sp)  # v_exp_f32 returns 0 below the smallest normal fp32 (module docstring)
    bound = (sp.mean(axis=1) + P.step_of(gm.numpy(), dt)) * mask  # a masked slot is an exact zero
    c._exp = dict(idx=idx, pos=pos, mask=mask, cache_cts=cts, denom=den + 1, counter=np.array([1], np.int64), K=K, V=V, num_before=num,
                  y=y, p=pr.reshape(c.HQ, S), gm=gm.numpy(), scores=s.reshape(c.HQ, S),
                  bound_y=1e-3 + 2 * ULP[dt] * float(y.abs().max()), bound_num=bound)
    return c._exp


def ramp_cases(shape, dt, variant):
    H, HQ, S, D = tuple(shape) + ((128,) if len(shape) == 3 else ())
    return [RampCase(dt, H, HQ, S, variant, fill, seed=n, D=D) for n, fill in enumerate(("brim", "sparse"))]


def check_ramp(c, kv, y, where):
    """-> (worst error / bound of y, of the history increment, elements compared exactly, elements compared under a bound)."""
    e = ramp_reference(c)
    got = read_cache(kv, c)
    n_exact = 0
    for name in ("pos", "mask", "cache_cts", "denom", "counter"):
        a, b = bits(got[name]).reshape(-1), bits(e[name]).reshape(-1)
        assert np.array_equal(a, b), f"{where}: {name}: {_first_diff(a, b)}"
        n_exact += a.size
    for name, t in (("K", kv.k_cache[0]), ("V", kv.v_cache[0])):
        assert np.array_equal(bits(t), bits(e[name])), f"{where}: {name} cache"
        n_exact += t.numel()
    yd = y.detach().cpu().double().reshape(c.HQ, c.D)
    assert bool(torch.isfinite(yd).all()), f"{where}: y is not finite"
    ey = float((yd - e["y"]).abs().max())
    print(f"{where}: y error {ey:.3g} / bound {e['bound_y']:.3g}")
    inc = got["num"].detach().cpu().numpy() - e["num_before"]
    err = np.abs(inc - e["gm"])
    b = e["bound_num"]
    exact = b == 0
    assert np.array_equal(inc[exact], e["gm"][exact]), f"{where}: history of a masked slot moved"
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / b)
    rn = float(np.nanmax(np.where(np.isnan(r), np.inf, r)))
    w = np.unravel_index(int(np.argmax(np.where(np.isnan(r), np.inf, r))), r.shape)
    print(f"{where}: history increment worst error / bound {rn:.3g} at {list(w)} (got {inc[w]!r}, reference {e['gm'][w]!r})")
    assert ey <= e["bound_y"], f"{where}: y differs by {ey:.4g} (limit {e['bound_y']:.4g})"
    assert rn <= 1.0, f"{where}: history increment at {list(w)} = {inc[w]!r}, reference {e['gm'][w]!r}: {rn:.3g} of its bound {b[w]:.3g}"
    return ey / e["bound_y"], rn, n_exact + int(exact.sum()), int((~exact).sum()) + yd.numel()


def run_ramp(c, form, dev, put=None, sync=None):
    """The one step in form "three" / "two" / "one" on a fresh cache object.  -> (cache object,) + check_ramp's tuple."""
    from cold_compress_amd.attention_utils import scaled_dot_product_attention as sdpa

    put = put or (lambda name, t: t.to(dev))
    sync = sync or (lambda: None)
    kv = make_cache(c, dev)
    kv.single_launch = form == "one"
    seed_cache(kv, c, dev)
    T = c.T
    p = torch.tensor([T], dtype=torch.int32, device=dev)
    q = put("q", c.q).view(1, c.HQ, 1, c.D)
    k1 = put("k_new", c.k_all[:, T].contiguous()).view(1, c.H, 1, c.D)
    v1 = put("v_new", c.v_all[:, T].contiguous()).view(1, c.H, 1, c.D)
    if form == "three":
        ka, va, ma = kv.update_kv(p, k1, v1, False)
        y, attn = sdpa(q, ka, va, attn_mask=ma, scale=c.scale, return_attn=True, group_mean=True)
        kv.update_state(p, k1, v1, False, attn)
    else:
        y = kv.decode_step(q, k1, v1, p, scale=c.scale)
    sync()
    return (kv,) + check_ramp(c, kv, y, f"{c.id} [{form}]")
