"""Plain references of the prompt-compaction and bookkeeping kernels (csrc/cc_compact.hip, the fill / norm / history kernels of
csrc/cc_evict.hip, attn_bandsum and the ring update of csrc/cc_hybrid.hip), written from the contract comments of those files and
of include/coldcompress.h.  A helper, not a test: tests/test_compact_ref_host.py holds every reference to the oracle's twin bit for
bit on the CPU, tests/test_gpu_compact_shapes.py holds the kernels to the references on the device.

Every reference is EXACT — the comparison is equality of bit patterns:
  by indexing                gather_rows, gather_vec, prefill_fill, the `sub` output of analysis_loss;
  one IEEE operation each    hh_update (float64 add), colsum_to_mean (round, fp32 divide, round), snapkv_priority (five fp32 adds in
                             ascending order — a clipped term adds +0.0, which changes nothing: the sum starts at +0.0 and can never be
                             -0.0 — one fp32 divide, round);
  by the documented order    attn_colsum / attn_bandsum (sequential fp32 add over the query axis, ascending), row_l2_norm (the 16-lane
                             order of sumsq_canonical_16, correctly rounded square root, round);
  ring update                the window sum is the exact sum of the W entries rounded once: float64 holds it exactly for the inputs
                             ring_values() makes (multiples of 2^-24 / 2^-30 below 2^10), round_once() rounds it nearest-even;
  analysis_loss losses       on the order-independent inputs of analysis_case() only (asserted there): every partial sum, 1 - sum and
                             the mean are exactly representable, so any summation order gives one bit pattern.

16-bit values travel through torch for rounding (as tests/attn_ref.py).  Nothing here calls the oracle or the device library's own
arithmetic; run_oracle / run_device only marshal a case's tensors to an entry point."""
import ctypes as C
import math

import numpy as np
import torch

from helpers import DT_CODE, from_np, to_np

F32, BF, HF = torch.float32, torch.bfloat16, torch.float16
DTYPES = (F32, BF, HF)
DT_NAME = {F32: "f32", BF: "bf16", HF: "f16"}
MARGIN = 64  # guard elements on each side of every device buffer (64 elements of any type keep 16-byte alignment)
BAD_ARG = -1

# work items per grid-stride pass (grid cap x block size), from the launchers
CAP_2048 = 2048 * 256
CAP_GATHER_ROWS = 4096 * 256
CAP_RING_TRACKED = 192 * 1024
CAP_HH_UPDATE = 1024 * 256
CAP_PREFILL_FILL = 4096 * 256  # 32-bit words
CAP_ROW_NORM = 2048 * 16  # rows: one 16-lane group each
# ... whose source lines these are: tests/test_compact_ref_host.py fails when one changes (then update the caps and the GPU file's
# second-pass shapes)
MIRRORED_LINES = {
    "cc_compact.hip": ["static dim3 grid_for(size_t n, int cap = 2048) {", "size_t b = (n + 255) / 256;",
                       "dim3 grid = grid_for((size_t)H * K * (row_bytes / 16), 4096), block(256);",
                       "dim3 grid = grid_for((size_t)H * K * D, 4096), block(256);", "dim3(1), dim3(1024), 0, st, (const float*)attn, pos"],
    "cc_hybrid.hip": ["int nb = (n + 255) / 256; if (nb > 2048) nb = 2048;", "int nb = (H * Lk + 255) / 256; if (nb > 2048) nb = 2048;",
                      "grid = dim3((unsigned)((n + 1023) / 1024 < 192 ? (n + 1023) / 1024 : 192));"],
    "cc_evict.hip": ["dim3 grid((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024), block(256);", "size_t nb = (words + 255) / 256; if (nb > 4096) nb = 4096;",
                     "int nb = (rows + 15) / 16; if (nb > 2048) nb = 2048;"],
    "cc_attn_prefill.hip": ["int nb = (a.H * a.L + kThreads - 1) / kThreads; if (nb > 2048) nb = 2048;", "constexpr int kThreads = 256;"],
}


# ------------------------------------------------------------------------------------------------ comparison
def bits(t):
    t = t.contiguous()
    if t.dtype in (BF, HF):
        return t.view(torch.int16)
    if t.dtype == F32:
        return t.view(torch.int32)
    if t.dtype == torch.float64:
        return t.view(torch.int64)
    return t


def same(a, b):
    """THE comparison of both test files: same shape, same dtype, same bit patterns (NaN sentinels included)."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def first_diffs(a, b, n=6):
    if a.shape != b.shape or a.dtype != b.dtype:
        return f"shape/dtype {tuple(a.shape)} {a.dtype} vs {tuple(b.shape)} {b.dtype}"
    idx = (bits(a) != bits(b)).nonzero()
    return f"{idx.shape[0]} differ, first at {idx[:n].tolist()}: {[a[tuple(i)].item() for i in idx[:n]]} vs {[b[tuple(i)].item() for i in idx[:n]]}"


def sentinel(dtype):
    if dtype.is_floating_point:
        return float("nan")
    return 0xAB if dtype == torch.uint8 else -7


def filled(shape, dtype):
    return torch.full(tuple(shape), sentinel(dtype), dtype=dtype)


def holds_sentinel(t):
    if t.dtype.is_floating_point:
        return bool(torch.isnan(t).all())
    return bool((t == sentinel(t.dtype)).all())


# ------------------------------------------------------------------------------------------------ cases and operations
class Case:
    """One call of an entry point: t = {name: CPU tensor or None} (inputs, and outputs as they stand before the call), the scalar
    arguments as attributes."""

    def __init__(self, op, cid, t, **p):
        self.op, self.id, self.t = op, cid, t
        self.__dict__.update(p)

    def replace(self, t=None, **p):
        c = Case(self.op, self.id, dict(self.t), **{k: v for k, v in self.__dict__.items() if k not in ("op", "id", "t")})
        c.t.update(t or {})
        c.__dict__.update(p)
        return c


class Op:
    """entry point, the tensors it may write, its argument list (p(name) -> pointer of the case's tensor), its reference."""

    def __init__(self, entry, outputs, args, ref):
        self.entry, self.outputs, self.args, self.ref = entry, outputs, args, ref


def _view(c, p):
    from cold_compress_amd import _abi

    def raw(n):
        h = p(n)
        return h.value if isinstance(h, C.c_void_p) else h

    v = _abi.KVView(raw("k"), raw("v"), raw("pos"), raw("mask"), raw("cts"), c.H, c.Hp, c.Hc, c.S, c.D, c.code)
    c._keep = v  # the struct must outlive the call
    return C.byref(v)


# ------------------------------------------------------------------------------------------------ references
def ref_gather_rows(c):
    src, keep = c.t["src"], c.t["keep"]
    H, L, D = src.shape
    K = keep.shape[1]
    idx = keep if keep.shape[0] == H else keep[:1].expand(H, K)
    out = torch.gather(bits(src), 1, idx[:, :, None].expand(H, K, D)).view(src.dtype)
    return dict(dst=out)


def ref_gather_vec(c):
    return dict(dst=torch.gather(bits(c.t["src"]), 1, c.t["keep"]).view(c.t["src"].dtype))


def ref_prefill_fill(c):
    T = c.T
    k, v, pos, mask, cts = (c.t[n].clone() for n in ("k", "v", "pos", "mask", "cts"))
    k[:, :T] = c.t["k_val"]
    v[:, :T] = c.t["v_val"]
    pos[:, :T] = c.t["pos_val"].to(torch.int32)  # [1, T] broadcasts over the Hp position heads
    mask[:, :T] = 1
    cts += T
    return dict(k=k, v=v, pos=pos, mask=mask, cts=cts)


def ref_analysis_loss(c):
    attn, pos = c.t["attn"], c.t["pos"].long()
    dt = attn.dtype
    S_full = attn.shape[1]
    idx = torch.where(pos == -1, torch.full_like(pos, S_full - 1), pos)
    sub = torch.gather(bits(attn[: pos.shape[0]]), 1, idx).view(dt)
    r = lambda x: x.to(dt).double()  # noqa: E731
    head = r(1.0 - r(sub.double().sum(dim=1)))
    loss = (head.sum() / pos.shape[0]).to(dt)
    losses, ctr = c.t["losses"].clone(), c.t["ctr"].clone()
    cv = int(ctr[0])
    if 0 <= cv < c.cap:
        losses[cv] = loss
    ctr[0] = cv + 1
    return dict(sub=sub, losses=losses, ctr=ctr)


def ref_hh_update(c):
    num, denom = c.t["num"].clone(), c.t["denom"].clone()
    num[:, : c.T] += c.t["attn"].double()
    denom += 1
    out = dict(num=num, denom=denom)
    if c.t["counter"] is not None:
        out["counter"] = c.t["counter"] + 1
    return out


def ref_colsum_to_mean(c):
    H, L = c.t["colsum"].shape
    p = c.t["input_pos"] if c.t["input_pos"] is not None else torch.arange(L)
    den = (L - p).to(F32)
    return dict(out=(c.t["colsum"].to(c.dtype).float() / den.view(1, L)).to(c.dtype))


def ref_snapkv_priority(c):
    obs = c.t["obs"].float()
    H, L = obs.shape
    pad = torch.zeros((H, L + 4), dtype=F32)
    pad[:, 2:L + 2] = obs
    acc = torch.zeros((H, L), dtype=F32)
    for u in range(5):  # t-2 .. t+2, ascending
        acc = acc + pad[:, u:u + L]
    t = torch.arange(L)
    cnt = (torch.clamp(t + 2, max=L - 1) - torch.clamp(t - 2, min=0) + 1).to(F32)
    v = acc / cnt.view(1, L)
    v[:, (t >= L - c.obs_len) | (t < c.g)] = 1.0
    return dict(out=v.to(c.t["obs"].dtype))


def ref_attn_colsum(c):
    attn = c.t["attn"]
    H, Lq, Lk = attn.shape
    acc = torch.zeros((H, Lk), dtype=F32)
    for q in range(Lq):
        acc = acc + attn[:, q].float()
    return dict(out=acc)


def ref_attn_bandsum(c):
    attn = c.t["attn"]
    H, Lq, Lk = attn.shape
    acc = torch.zeros((H, Lk), dtype=F32)
    for j in range(min(c.band, Lq)):  # out[h, s] += attn[h, s + j, s]: ascending query index
        d = torch.diagonal(attn, offset=-j, dim1=1, dim2=2).float()  # [H, min(Lq - j, Lk)]
        acc[:, : d.shape[1]] = acc[:, : d.shape[1]] + d
    return dict(out=acc)


def ref_row_l2_norm(c, order="canonical"):
    x = c.t["x"]
    H, N, D = x.shape
    n16 = (D + 15) // 16
    xf = torch.zeros((H * N, n16 * 16), dtype=F32)
    xf[:, :D] = x.reshape(H * N, D).float()
    sq = (xf * xf).view(H * N, n16, 16)
    a = torch.zeros((H * N, 16), dtype=F32)
    for i in range(n16):  # lane j: x[j], x[j + 16], ... in turn (a padded term adds +0.0)
        a = a + sq[:, i]
    j = torch.arange(16)
    for k in (8, 4, 2, 1):
        a = a + a[:, j ^ k]
    n = torch.sqrt(a[:, 0].double()).float()  # correctly rounded: 53 >= 2 * 24 + 2 bits make the double rounding innocuous
    return dict(out=(-n if c.negate else n).to(x.dtype).view(H, N))


GRID_BITS = {F32: 30, BF: 24, HF: 24}  # ring_values(): multiples of 2^-GRID_BITS
FMT = {F32: (24, -149), BF: (8, -133), HF: (11, -24)}  # significand bits, log2 of the smallest quantum


def round_once(x64, dtype):
    """float64 numpy array of EXACT values -> nearest-even values of dtype, as float32 (no overflow cases here)."""
    p, qmin = FMT[dtype]
    _, e = np.frexp(x64)  # x = m * 2^e, m in [0.5, 1)
    q = np.maximum(e - p, qmin).astype(np.int32)
    r = np.rint(np.ldexp(x64, -q))  # exact scaling, then round half to even
    return np.ldexp(r, q).astype(np.float32)


def window_sums(ring):
    """[H, S, W] ring of ring_values() -> [H * S] float32: the exact sum rounded once to the ring's dtype."""
    g = GRID_BITS[ring.dtype]
    units = ring.double().numpy() * 2.0 ** g
    assert np.array_equal(units, np.rint(units)) and np.abs(units).max(initial=0) <= 2.0 ** g and ring.shape[2] <= 1024
    exact = units.sum(axis=2) * 2.0 ** -g  # integers below 2^41: every partial sum is exact in float64
    return torch.from_numpy(round_once(exact.reshape(-1), ring.dtype))


def ref_ring_update(c):
    num, denom, counter = c.t["num"].clone(), c.t["denom"].clone(), c.t["counter"].clone()
    H, S, W = num.shape
    slot = int(counter[0]) % W
    num[:, :, slot] = 0
    num[:, : c.T, slot] = c.t["attn"]
    denom += 1
    counter += 1
    out = dict(num=num, denom=denom, counter=counter)
    if c.t["wsum"] is not None:
        out["wsum"] = window_sums(num)
    return out


OPS = {
    "topk_keep": Op("cc_topk_keep", ("keep",), lambda c, p: (p("prio"), c.code, c.H, c.L, c.K, p("keep"), None, 0, None), None),
    "gather_rows": Op("cc_gather_rows", ("dst",), lambda c, p: (p("src"), p("keep"), c.Hk, c.H, c.L, c.K, c.D, c.code, p("dst"), None),
                      ref_gather_rows),
    "gather_vec": Op("cc_gather_vec", ("dst",), lambda c, p: (p("src"), p("keep"), c.H, c.L, c.K, c.code, p("dst"), None), ref_gather_vec),
    "prefill_fill": Op("cc_prefill_fill", ("k", "v", "pos", "mask", "cts"),
                       lambda c, p: (_view(c, p), p("k_val"), p("v_val"), p("pos_val"), c.PH, c.T, None), ref_prefill_fill),
    "analysis_loss": Op("cc_analysis_loss", ("sub", "losses", "ctr"),
                        lambda c, p: (p("attn"), p("pos"), c.Hp, c.S_full, c.S, c.code, p("sub"), p("losses"), p("ctr"), c.cap, None),
                        ref_analysis_loss),
    "hh_update": Op("cc_hh_update", ("num", "denom", "counter"),
                    lambda c, p: (p("num"), p("denom"), p("counter"), p("attn"), c.H, c.S, c.T, c.code, None), ref_hh_update),
    "colsum_to_mean": Op("cc_colsum_to_mean", ("out",), lambda c, p: (p("colsum"), p("input_pos"), c.H, c.L, c.code, p("out"), None),
                         ref_colsum_to_mean),
    "snapkv_priority": Op("cc_snapkv_priority", ("out",), lambda c, p: (p("obs"), c.H, c.L, c.code, c.obs_len, c.g, p("out"), None),
                          ref_snapkv_priority),
    "attn_colsum": Op("cc_attn_colsum", ("out",), lambda c, p: (p("attn"), c.H, c.Lq, c.Lk, c.code, p("out"), None), ref_attn_colsum),
    "attn_bandsum": Op("cc_attn_bandsum", ("out",), lambda c, p: (p("attn"), c.H, c.Lq, c.Lk, c.code, c.band, p("out"), None),
                       ref_attn_bandsum),
    "row_l2_norm": Op("cc_row_l2_norm", ("out",), lambda c, p: (p("x"), c.H, c.N, c.D, c.code, c.negate, p("out"), None), ref_row_l2_norm),
    "ring_update": Op("cc_hh_ring_update", ("num", "denom", "counter", "wacc", "wsum"),
                      lambda c, p: (p("num"), p("denom"), p("counter"), p("attn"), c.H, c.S, c.T, c.W, c.code, p("wacc"), p("wsum"), None),
                      ref_ring_update),
}


def reference(c):
    return OPS[c.op].ref(c)


# ------------------------------------------------------------------------------------------------ marshalling
def run_oracle(o, c, ops=None):
    """-> (return code, {output name: CPU tensor}) of the oracle's twin on host copies of the case's tensors (ops: another module's
    table of operations, tests/glue_ref.py)."""
    op = (ops or OPS)[c.op]
    arrs = {n: (None if v is None else (to_np(v) if v.numel() else np.zeros(1, np.uint8))) for n, v in c.t.items()}
    rc = o.fns()[op.entry](*op.args(c, lambda n: o.ptr(arrs[n])))
    return rc, {n: (from_np(arrs[n], c.t[n].dtype) if c.t[n].numel() else c.t[n].clone()) for n in op.outputs if c.t.get(n) is not None}


def run_device(c, device="cuda", ops=None):
    """-> (return code, {output name: CPU tensor}) of the device entry point.  Every tensor of the case sits inside a larger buffer
    pre-filled with the sentinel of its type (NaN, -7, 0xAB); after the call the margins on both sides of EVERY buffer must still hold
    it, and every tensor that is not an output must be bit for bit what was uploaded."""
    from cold_compress_amd import _abi

    op = (ops or OPS)[c.op]
    bufs = {}
    for n, v in c.t.items():
        if v is None:
            continue
        b = torch.full((v.numel() + 2 * MARGIN,), sentinel(v.dtype), dtype=v.dtype, device=device)
        b[MARGIN:MARGIN + v.numel()] = v.reshape(-1).to(device)
        bufs[n] = b

    def ptr(n):
        b = bufs.get(n)
        return None if b is None else C.c_void_p(b.data_ptr() + MARGIN * b.element_size())

    rc = _abi.lib()[op.entry](*op.args(c, ptr))
    torch.cuda.synchronize()
    outs = {}
    for n, b in bufs.items():
        h = b.cpu()
        assert holds_sentinel(h[:MARGIN]) and holds_sentinel(h[h.numel() - MARGIN:]), f"{c.id}: margin of '{n}' overwritten"
        body = h[MARGIN:h.numel() - MARGIN].view(c.t[n].shape)
        if n in op.outputs:
            outs[n] = body
        else:
            assert same(body, c.t[n]), f"{c.id}: input '{n}' modified"
    return rc, outs


# ------------------------------------------------------------------------------------------------ generators
SIZES = (1, 15, 17, 255, 257, 1023, 1025, 2049)
HEADS = (1, 2, 3, 8, 9)
D_ROWS = {F32: (1, 3, 4, 6, 8, 16, 24, 128, 256), BF: (1, 3, 4, 6, 8, 12, 16, 24, 128, 256), HF: (1, 3, 4, 6, 8, 12, 16, 24, 128, 256)}
D_FILL = {F32: (1, 3, 4, 6, 16, 128), BF: (2, 4, 6, 16, 24, 128), HF: (2, 4, 6, 16, 24, 128)}  # cc_view_ok: rows of whole 32-bit words
N_FUZZ = 40


def _gens(op, i):
    seed = 7919 * (sorted(OPS).index(op) + 1) + i
    return np.random.default_rng(seed), torch.Generator().manual_seed(seed)


def _pick(rng, seq):
    return seq[int(rng.integers(len(seq)))]


def _keep(rng, H, L, K):
    """[H, K] ascending distinct indices in [0, L): what cc_topk_keep hands on."""
    return torch.from_numpy(np.stack([np.sort(rng.choice(L, K, replace=False)) for _ in range(H)]).astype(np.int64))


def _K(rng, i, L):
    return 1 if i % 7 == 0 else L if i % 7 == 1 else int(rng.integers(1, L + 1))


def gather_rows_case(cid, dt, H, L, K, D, Hk, rng, gen):
    src = torch.randn(H, L, D, generator=gen).to(dt)
    return Case("gather_rows", cid, dict(src=src, keep=_keep(rng, Hk, L, K), dst=filled((H, K, D), dt)), H=H, L=L, K=K, D=D, Hk=Hk,
                code=DT_CODE[dt])


def cases_gather_rows():
    for i in range(N_FUZZ):
        rng, gen = _gens("gather_rows", i)
        dt, H = DTYPES[i % 3], HEADS[i % 5]
        D = D_ROWS[dt][(i // 3) % len(D_ROWS[dt])]
        L = SIZES[(i * 3 + 1) % len(SIZES)] if D <= 24 else _pick(rng, (1, 15, 17, 255, 257))
        K = _K(rng, i, L)
        Hk = 1 if i % 2 else H
        yield gather_rows_case(f"gather_rows[{i}]-{DT_NAME[dt]}-H{H}-L{L}-K{K}-D{D}-Hk{Hk}", dt, H, L, K, D, Hk, rng, gen)


def gather_vec_case(cid, dt, H, L, K, rng, gen):
    return Case("gather_vec", cid, dict(src=torch.randn(H, L, generator=gen).to(dt), keep=_keep(rng, H, L, K), dst=filled((H, K), dt)),
                H=H, L=L, K=K, code=DT_CODE[dt])


def cases_gather_vec():
    for i in range(N_FUZZ):
        rng, gen = _gens("gather_vec", i)
        dt, H, L = DTYPES[i % 3], HEADS[i % 5], SIZES[(i * 3 + 2) % len(SIZES)]
        K = _K(rng, i, L)
        yield gather_vec_case(f"gather_vec[{i}]-{DT_NAME[dt]}-H{H}-L{L}-K{K}", dt, H, L, K, rng, gen)


def prefill_fill_case(cid, dt, H, Hp, Hc, PH, S, T, D, rng, gen, T_alloc=None):
    Ta = T if T_alloc is None else T_alloc
    t = dict(k=filled((H, S, D), dt), v=filled((H, S, D), dt), pos=filled((Hp, S), torch.int32), mask=filled((H, S), torch.uint8),
             cts=torch.from_numpy(rng.integers(0, 50, Hc).astype(np.int32)), k_val=torch.randn(H, Ta, D, generator=gen).to(dt),
             v_val=torch.randn(H, Ta, D, generator=gen).to(dt),
             pos_val=torch.from_numpy(rng.integers(0, 1 << 20, (max(PH, 1), Ta)).astype(np.int64)))
    return Case("prefill_fill", cid, t, H=H, Hp=Hp, Hc=Hc, PH=PH, S=S, T=T, D=D, code=DT_CODE[dt])


def cases_prefill_fill():
    for i in range(N_FUZZ):
        rng, gen = _gens("prefill_fill", i)
        dt, H = DTYPES[i % 3], HEADS[i % 5]
        D = D_FILL[dt][(i // 3) % 6]
        S = SIZES[(i * 3) % len(SIZES)] if D <= 24 else _pick(rng, (1, 15, 17, 255, 257))
        T = 1 if i % 7 == 0 else S if i % 7 == 1 else int(rng.integers(1, S + 1))
        Hp = H if (i // 2) % 2 else 1
        Hc = H if (i // 4) % 2 else 1
        PH = Hp if i % 2 else 1
        yield prefill_fill_case(f"prefill_fill[{i}]-{DT_NAME[dt]}-H{H}-Hp{Hp}-Hc{Hc}-PH{PH}-S{S}-T{T}-D{D}", dt, H, Hp, Hc, PH, S, T, D, rng, gen)


ENTRY_BITS = {BF: 8, HF: 11, F32: 20}  # analysis_case(): attention entries are multiples of 2^-ENTRY_BITS ...
HEAD_BITS = {BF: 8, HF: 11, F32: 16}  # ... and every head's total (so its loss) a multiple of 2^-HEAD_BITS


def analysis_case(cid, dt, Hp, S, S_full, share_unfilled, ctr, cap, rng, last_units=0):
    """Order-independent inputs for the losses.  Entries: non-negative multiples of q = 2^-ENTRY_BITS; head totals <= 1 and
    multiples of Q = 2^-HEAD_BITS, chosen in pairs (m + d, m - d) around a mean loss m that is a multiple of Q: then every partial sum
    inside a head is an integer number of q below 2^24 (exact in fp32), dtype(sum) and dtype(1 - sum) are identities, every partial
    sum over the heads is an integer number of Q below 64 / Q <= 2^22, the division by the power of two Hp is exact and the mean is
    m, representable in the dtype.  All of it asserted below."""
    assert Hp & (Hp - 1) == 0 and 1 <= Hp <= 64 and S_full > S
    eb, hb = ENTRY_BITS[dt], HEAD_BITS[dt]
    per = 1 << (eb - hb)  # entry units per head unit
    m = int(rng.integers(0, (1 << hb) + 1))  # mean loss, in head units
    loss = np.full(Hp, m, np.int64)
    for a in range(0, Hp - 1, 2):
        d = int(rng.integers(0, min(m, (1 << hb) - m) + 1))
        loss[a], loss[a + 1] = m + d, m - d
    total = ((1 << hb) - loss) * per  # units of q each head's kept entries sum to
    n_unf = int(share_unfilled * S)
    attn_u = rng.integers(0, 1 << (eb - 4), (Hp, S_full)).astype(np.int64)  # what the shadow cache does NOT hold: never summed
    pos = np.full((Hp, S), -1, np.int32)
    for h in range(Hp):
        cols = rng.permutation(S_full - 1)[: S - n_unf]
        slots = np.sort(rng.permutation(S)[: S - n_unf])
        pos[h, slots] = cols
        lu = last_units if n_unf * last_units <= total[h] else 0
        attn_u[h, S_full - 1] = lu
        attn_u[h, cols] = rng.multinomial(int(total[h] - n_unf * lu), np.ones(len(cols)) / len(cols))
    attn64 = torch.from_numpy(attn_u.astype(np.float64) * 2.0 ** -eb)
    attn = attn64.to(dt)
    # ---- the guarantees
    assert torch.equal(attn.double(), attn64) and bool((attn64 >= 0).all())
    idx = np.where(pos == -1, S_full - 1, pos)
    row_units = np.take_along_axis(attn_u, idx, axis=1).sum(axis=1)
    assert np.array_equal(row_units, total) and row_units.max() <= 1 << eb and (1 << eb) <= 1 << 24
    s = torch.from_numpy(row_units * 2.0 ** -eb)
    assert torch.equal(s.to(dt).double(), s) and torch.equal((1.0 - s).to(dt).double(), 1.0 - s)
    assert int(loss.sum()) == m * Hp and int(np.cumsum(np.sort(loss)[::-1]).max()) <= 1 << 24
    mean = torch.tensor(m * 2.0 ** -hb, dtype=torch.float64)
    assert mean.to(dt).double() == mean
    t = dict(attn=attn, pos=torch.from_numpy(pos), sub=filled((Hp, S), dt), losses=filled((cap,), dt),
             ctr=torch.tensor([ctr], dtype=torch.int32))
    return Case("analysis_loss", cid, t, Hp=Hp, S=S, S_full=S_full, cap=cap, code=DT_CODE[dt], mean_loss=float(mean))


ANALYSIS_S = (1, 24, 63, 64, 65, 1023, 1024, 1025, 3000)
ANALYSIS_HP = (1, 2, 8, 64)


def cases_analysis_loss():
    combos = [(S, Hp) for S in ANALYSIS_S for Hp in ANALYSIS_HP] + [(3000, 64), (1025, 8), (65, 2), (1, 1)]
    for i, (S, Hp) in enumerate(combos):
        rng, _ = _gens("analysis_loss", i)
        dt = DTYPES[(i + i // 4) % 3]
        cap = (1, 5, 16)[i % 3]
        ctr = (0, cap - 1, cap, cap + 3, -1, -5, 0, cap - 1)[i % 8]
        share = (0.0, 0.3, 0.0, 0.6)[(i // 2) % 4]
        S_full = S + (1, 7, 100)[i % 3]
        yield analysis_case(f"analysis_loss[{i}]-{DT_NAME[dt]}-Hp{Hp}-S{S}-Sf{S_full}-unf{share}-ctr{ctr}-cap{cap}", dt, Hp, S, S_full, share,
                            ctr, cap, rng, last_units=1 if i % 5 == 3 else 0)


def _T(rng, i, S):
    return 0 if i % 6 == 0 else S if i % 6 == 1 else int(rng.integers(0, S + 1))


def hh_update_case(cid, dt, H, S, T, with_counter, rng, gen):
    t = dict(num=torch.rand(H, S, generator=gen, dtype=torch.float64) * 3.0,
             denom=torch.from_numpy(rng.integers(0, 1000, (H, S)).astype(np.int32)),
             counter=torch.tensor([int(rng.integers(0, 1 << 40))], dtype=torch.int64) if with_counter else None,
             attn=torch.rand(H, T, generator=gen).to(dt))
    return Case("hh_update", cid, t, H=H, S=S, T=T, code=DT_CODE[dt])


def cases_hh_update():
    for i in range(N_FUZZ):
        rng, gen = _gens("hh_update", i)
        dt, H, S = DTYPES[i % 3], HEADS[i % 5], SIZES[(i * 3 + 1) % len(SIZES)]
        T = _T(rng, i, S)
        yield hh_update_case(f"hh_update[{i}]-{DT_NAME[dt]}-H{H}-S{S}-T{T}-ctr{i % 2}", dt, H, S, T, bool(i % 2), rng, gen)


def colsum_to_mean_case(cid, dt, H, L, with_pos, rng, gen):
    t = dict(colsum=torch.rand(H, L, generator=gen) * float(min(L, 40)),
             input_pos=torch.from_numpy(rng.integers(0, L, L).astype(np.int64)) if with_pos else None, out=filled((H, L), dt))
    return Case("colsum_to_mean", cid, t, H=H, L=L, dtype=dt, code=DT_CODE[dt])


def cases_colsum_to_mean():
    for i in range(N_FUZZ):
        rng, gen = _gens("colsum_to_mean", i)
        dt, H, L = DTYPES[i % 3], HEADS[i % 5], SIZES[(i * 3 + 2) % len(SIZES)]
        yield colsum_to_mean_case(f"colsum_to_mean[{i}]-{DT_NAME[dt]}-H{H}-L{L}-pos{(i // 3) % 2}", dt, H, L, bool((i // 3) % 2), rng, gen)


def snapkv_case(cid, dt, H, L, obs_len, g, gen):
    return Case("snapkv_priority", cid, dict(obs=torch.rand(H, L, generator=gen).to(dt), out=filled((H, L), dt)), H=H, L=L,
                obs_len=obs_len, g=g, code=DT_CODE[dt])


def cases_snapkv_priority():
    Ls = (1, 2, 3, 4, 5, 6) + SIZES[1:]
    for i in range(N_FUZZ):
        rng, gen = _gens("snapkv_priority", i)
        dt, H, L = DTYPES[i % 3], HEADS[i % 5], Ls[(i * 5 + 1) % len(Ls)]
        obs_len = (0, L, L + 3, 16, int(rng.integers(0, L + 1)))[(i // 3) % 5]
        g = (0, L, L + 2, 4, int(rng.integers(0, L + 1)))[(i // 2) % 5]
        yield snapkv_case(f"snapkv_priority[{i}]-{DT_NAME[dt]}-H{H}-L{L}-obs{obs_len}-g{g}", dt, H, L, obs_len, g, gen)


def attn_sum_case(op, cid, dt, H, Lq, Lk, band, gen):
    t = dict(attn=(torch.rand(H, Lq, Lk, generator=gen) ** 3).to(dt), out=filled((H, Lk), F32))
    return Case(op, cid, t, H=H, Lq=Lq, Lk=Lk, band=band, code=DT_CODE[dt])


def _cases_attn(op):
    Lqs = (1, 3, 15, 17, 65, 257)
    for i in range(N_FUZZ):
        rng, gen = _gens(op, i)
        dt, H = DTYPES[i % 3], HEADS[i % 5]
        Lq = Lqs[(i // 2) % len(Lqs)]
        Lk = SIZES[(i * 3 + 1) % len(SIZES)] if Lq <= 65 else _pick(rng, (1, 15, 17, 255, 257))
        band = (1, 2, 3, 17, Lq, Lq + 5)[i % 6]
        yield attn_sum_case(op, f"{op}[{i}]-{DT_NAME[dt]}-H{H}-Lq{Lq}-Lk{Lk}" + (f"-band{band}" if op == "attn_bandsum" else ""), dt, H, Lq, Lk,
                            band, gen)


def cases_attn_colsum():
    return _cases_attn("attn_colsum")


def cases_attn_bandsum():
    return _cases_attn("attn_bandsum")


def row_l2_norm_case(cid, dt, H, N, D, negate, gen):
    return Case("row_l2_norm", cid, dict(x=torch.randn(H, N, D, generator=gen).to(dt), out=filled((H, N), dt)), H=H, N=N, D=D,
                negate=negate, code=DT_CODE[dt])


def cases_row_l2_norm():
    for i in range(N_FUZZ):
        rng, gen = _gens("row_l2_norm", i)
        dt, H = DTYPES[i % 3], HEADS[i % 5]
        D = D_ROWS[dt][(i // 3) % len(D_ROWS[dt])]
        N = SIZES[(i * 3 + 1) % len(SIZES)] if D <= 24 else _pick(rng, (1, 15, 17, 255, 257))
        if i == N_FUZZ - 1:  # more 16-lane groups than the capped grid holds (2048 x 16 rows)
            H, N, D = 9, 4099, 3
        yield row_l2_norm_case(f"row_l2_norm[{i}]-{DT_NAME[dt]}-H{H}-N{N}-D{D}-neg{i % 2}", dt, H, N, D, i % 2, gen)


def ring_values(shape, dt, gen):
    """Attention-like values in [0, 1] on the grid 2^-GRID_BITS, exact in dt: their window sums are exact in float64."""
    g = GRID_BITS[dt]
    x = torch.round(torch.rand(shape, generator=gen, dtype=torch.float64) ** 4 * 2.0 ** g) * 2.0 ** -g
    x = x.to(dt)
    u = x.double() * 2.0 ** g
    assert torch.equal(u, torch.round(u)) and bool((x.double() <= 1).all()) and bool((x.double() >= 0).all())
    return x


def ring_acc_words(H, S, W, dt):
    """cc_hh_ring_acc_words of include/coldcompress.h: accumulators, two ticket words, the column-major shadow, 2H meeting words."""
    hs, es = H * S, 4 if dt == F32 else 2
    return hs * 4 + 2 + (hs * W * es + 7) // 8 + 2 * H


def ring_case(cid, dt, H, S, W, T, c0, tracked, gen, T_alloc=None):
    """The state a cache starts from (cache.py: ring, denominators and the tracked state all zero), at step counter c0."""
    Ta = T if T_alloc is None else T_alloc
    t = dict(num=torch.zeros((H, S, W), dtype=dt), denom=torch.zeros((H, S), dtype=torch.int32), counter=torch.tensor([c0], dtype=torch.int64),
             attn=ring_values((H, Ta), dt, gen), wacc=torch.zeros(ring_acc_words(H, S, W, dt), dtype=torch.int64) if tracked else None,
             wsum=torch.zeros(H * S, dtype=F32) if tracked else None)
    return Case("ring_update", cid, t, H=H, S=S, W=W, T=T, code=DT_CODE[dt], dtype=dt, tracked=tracked)


def ring_next(c, state, gen):
    """The case of the following update: `state` (the outputs of the previous one) and fresh attention."""
    return c.replace(t=dict(state, attn=ring_values((c.H, c.T), c.dtype, gen)))


def cases_ring_update():
    """Each case is the FIRST of a chain of W + 2 updates (ring_next): every ring column written, two of them overwritten."""
    for i in range(N_FUZZ):
        rng, gen = _gens("ring_update", i)
        dt, H, S = DTYPES[i % 3], HEADS[i % 5], SIZES[(i * 3 + 1) % len(SIZES)]
        W = (2, 3, 5, 8)[(i // 3) % 4]
        T = _T(rng, i, S)
        c0 = int(rng.integers(0, 50))
        tracked = bool((i // 2) % 2)
        c = ring_case(f"ring_update[{i}]-{DT_NAME[dt]}-H{H}-S{S}-W{W}-T{T}-c{c0}-{'tracked' if tracked else 'plain'}", dt, H, S, W, T, c0,
                      tracked, gen)
        c.gen, c.steps = gen, W + 2
        yield c


FUZZ = dict(gather_rows=cases_gather_rows, gather_vec=cases_gather_vec, prefill_fill=cases_prefill_fill, analysis_loss=cases_analysis_loss,
            hh_update=cases_hh_update, colsum_to_mean=cases_colsum_to_mean, snapkv_priority=cases_snapkv_priority,
            attn_colsum=cases_attn_colsum, attn_bandsum=cases_attn_bandsum, row_l2_norm=cases_row_l2_norm, ring_update=cases_ring_update)


# ------------------------------------------------------------------------------------------------ refusals
def refusals():
    """[(what, case)]: calls every entry point must answer with CC_ERR_BAD_ARG, leaving its outputs as they were.  Every buffer is
    large enough for the refused shape, so that even a call that went through could not reach outside its buffers."""
    rng, gen = np.random.default_rng(99), torch.Generator().manual_seed(99)
    out = []
    topk = Case("topk_keep", "topk", dict(prio=torch.randn(3, 20, generator=gen), keep=filled((3, 24), torch.int64)), H=3, L=20, K=5, code=0)
    out += [("cc_topk_keep K > L", topk.replace(K=21)), ("cc_topk_keep K = 0", topk.replace(K=0)), ("cc_topk_keep K < 0", topk.replace(K=-3))]
    gr = gather_rows_case("gather_rows", BF, 3, 20, 5, 8, 3, rng, gen)
    out += [("cc_gather_rows Hk = 2, H = 3", gr.replace(Hk=2)), ("cc_gather_rows Hk = 0", gr.replace(Hk=0)),
            ("cc_gather_rows Hk = 4, H = 3", gr.replace(Hk=4))]
    al = analysis_case("analysis", BF, 64, 24, 31, 0.3, 0, 4, rng)
    big = al.replace(t=dict(attn=torch.cat([al.t["attn"], al.t["attn"][:1]]), pos=torch.cat([al.t["pos"], al.t["pos"][:1]]),
                            sub=filled((65, 24), BF)))
    out += [("cc_analysis_loss Hp = 65", big.replace(Hp=65)), ("cc_analysis_loss cap = 0", al.replace(cap=0)),
            ("cc_analysis_loss cap < 0", al.replace(cap=-1))]
    pf = prefill_fill_case("prefill_fill", HF, 3, 3, 3, 3, 17, 9, 4, rng, gen, T_alloc=18)
    out += [("cc_prefill_fill T > S", pf.replace(T=18)), ("cc_prefill_fill PH = 2, Hp = 3", pf.replace(PH=2)),
            ("cc_prefill_fill PH = 3, Hp = 1", pf.replace(Hp=1))]
    bs = attn_sum_case("attn_bandsum", "attn_bandsum", F32, 2, 5, 9, 3, gen)
    out += [("cc_attn_bandsum band = 0", bs.replace(band=0)), ("cc_attn_bandsum band < 0", bs.replace(band=-2))]
    for tracked in (False, True):
        ru = ring_case("ring_update", BF, 2, 17, 3, 9, 4, tracked, gen, T_alloc=18)
        out.append((f"cc_hh_ring_update T > S ({'tracked' if tracked else 'plain'})", ru.replace(T=18)))
    ru = ring_case("ring_update", BF, 2, 17, 3, 9, 4, True, gen)
    out += [("cc_hh_ring_update wsum_acc without wsum", ru.replace(t=dict(wsum=None))),
            ("cc_hh_ring_update wsum without wsum_acc", ru.replace(t=dict(wacc=None)))]
    return out


def passes(n_items, cap):
    """Grid-stride passes a kernel whose grid is capped at `cap` work items makes over n_items."""
    return math.ceil(n_items / cap)
