"""Attention, decode steps and the harness at query-group ratios R = HQ / H other than 1, 2, 4 and 8 — Qwen2-7B's 7 query heads
per kv head above all (harness/model.py CONFIGS) — against the float64 reference of tests/attn_ref.py.

What these ratios reach that the rest of the suite does not: several query-head blocks per kv head in the decode grid (R / rt
z-blocks, of which only the first writes the step's bookkeeping), the combine pass folding R heads from several z-blocks into the
group mean, the two-launch form of every fused step (the single launch serves 4 or 8 query heads per kv head), partly filled
32-row workgroups in the VALU prefill (32 / R query rows per head), and the refusal of the fused quantised caches.  Tolerances are
the suite's: y <= 1e-3 + 2 ulp * max|y|; probabilities and group means < 1e-3 + 2 ulp; column sums < 5e-2 + 1 ulp * |ref|;
observation-window means < 4e-3 (fp32: 1e-3)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import attn_ref as AR
from helpers import load_golden, to_np

pytestmark = pytest.mark.gpu
DEV = __import__("helpers").TEST_DEVICE

PREFILL_RATIOS = [1, 2, 3, 4, 5, 6, 7, 8, 16, 32]
PREFILL_LENGTHS = [1, 2, 31, 32, 33, 63, 64, 65, 97, 129, 1000]
DECODE_RATIOS = [3, 5, 6, 7, 12, 16]
DECODE_LENGTHS = [13, 513, 4096, 8200, 18432]
BANDS = (3, 17)


def _ulp(dtype):
    return AR.ulp_of(dtype)


def _spacing(x, dtype):
    """The spacing of `dtype` at |x| (one ulp), float64."""
    man = {torch.bfloat16: 7, torch.float16: 10, torch.float32: 23}[dtype]
    return torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(1e-30))) - man)


def _kv_heads(R):
    return 4 if R <= 7 else 2 if R <= 16 else 1


# ------------------------------------------------------------------------------------ a. prefill against attn_ref


def _prefill_check(dtype, H, R, L, D, seed, what, forms=("one", "two")):
    from cold_compress_amd.attention_utils import prefill_attention

    gen = torch.Generator(device=DEV).manual_seed(seed)
    HQ = H * R
    q = torch.randn(1, HQ, L, D, generator=gen, device=DEV).to(dtype)
    k = torch.randn(1, H, L, D, generator=gen, device=DEV).to(dtype)
    v = torch.randn(1, H, L, D, generator=gen, device=DEV).to(dtype)
    ref = AR.prefill_ref(q, k, v, obs_len=16, bands=BANDS, need_side="two" in forms)
    yr = ref["y"]
    ytol = 1e-3 + 2 * _ulp(dtype) * float(yr.abs().max())
    if "one" in forms:  # nobody asks for the probabilities: the one-pass (online-softmax) form where the shape has one
        y, none = prefill_attention(q, k, v, return_attn=False)
        assert none is None
        err = float((y[0].double() - yr).abs().max())
        assert err <= ytol, f"{what} one-pass y: {err} > {ytol}"
    if "two" in forms:
        y, summ = prefill_attention(q, k, v, return_attn=True, bands=BANDS)
        err = float((y[0].double() - yr).abs().max())
        assert err <= ytol, f"{what} two-pass y: {err} > {ytol}"
        fp32 = dtype == torch.float32
        cs = summ.colsum.double()
        lim = (1e-3 if fp32 else 5e-2) + _ulp(dtype) * ref["colsum"].abs()
        assert bool(((cs - ref["colsum"]).abs() <= lim).all()), f"{what} colsum: {float((cs - ref['colsum']).abs().max())}"
        err = float((summ.obs_mean.double() - ref["obs"]).abs().max())
        assert err < (1e-3 if fp32 else 4e-3), f"{what} obs mean: {err}"
        for b in BANDS:
            bs = summ.bands[b].double()
            lim = (1e-3 if fp32 else 5e-2) + _ulp(dtype) * ref["bands"][b].abs()
            assert bool(((bs - ref["bands"][b]).abs() <= lim).all()), f"{what} band {b}: {float((bs - ref['bands'][b]).abs().max())}"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("R", PREFILL_RATIOS)
def test_prefill_at_every_ratio(dtype, D, R):
    """Every ratio the prefill serves, at lengths on both sides of the 32-row tile and of the matrix-core path's L >= 64."""
    H = _kv_heads(R)
    for L in PREFILL_LENGTHS:
        _prefill_check(dtype, H, R, L, D, 1000 * R + L, f"{dtype} H={H} R={R} L={L} D={D}")


@pytest.mark.parametrize("R", PREFILL_RATIOS)
def test_prefill_fp32_at_every_ratio(R):
    H = _kv_heads(R)
    for L in (1, 31, 33, 65, 129):
        _prefill_check(torch.float32, H, R, L, 64, 77 * R + L, f"fp32 H={H} R={R} L={L}")


@pytest.mark.parametrize("dtype,H,R,L,D", [(torch.bfloat16, 4, 7, 4096, 128),  # Qwen2-7B
                                           (torch.bfloat16, 8, 8, 2048, 128),  # the 70B shape
                                           # fp16 on the matrix-core path, one-pass and two-pass
                                           (torch.float16, 2, 4, 64, 128), (torch.float16, 2, 4, 97, 128),
                                           (torch.float16, 2, 4, 1000, 128), (torch.float16, 2, 4, 4133, 128),
                                           (torch.float16, 2, 4, 8192, 128)])
def test_prefill_production_shapes(dtype, H, R, L, D):
    _prefill_check(dtype, H, R, L, D, 31 + L, f"{dtype} H={H} R={R} L={L} D={D}")


# ------------------------------------------------------------------------------------ b. known answers


def _exact_values(gen, shape, device):
    """Values exact in every dtype and bounded away from zero: +-{0.5, 0.75, 1, 1.25, 1.5}."""
    mag = torch.tensor([0.5, 0.75, 1.0, 1.25, 1.5], dtype=torch.float64)
    idx = torch.randint(0, 5, shape, generator=gen)
    sign = torch.randint(0, 2, shape, generator=gen) * 2 - 1
    return (mag[idx] * sign).to(device)


def _dominant(gen, H, R, L, D, n_rows, causal):
    """Keys of +-1 entries; query (head h*R + r, row i) = 16 * key j(h, r, i) with j <= i when causal: a score margin of
    >= 40 over every other key (checked).  -> q [1, HQ, n_rows, D], k [1, H, L, D], j [H, R, n_rows]."""
    k = (torch.randint(0, 2, (H, L, D), generator=gen) * 2 - 1).double()
    rows = torch.arange(n_rows)
    hi = (rows + 1) if causal else torch.full((n_rows,), L)
    j = (torch.rand(H, R, n_rows, generator=gen) * hi.double()).long().clamp_max(hi - 1)
    q = 16.0 * k[torch.arange(H).view(H, 1, 1), j]  # [H, R, n, D]
    sc = torch.einsum("hrnd,hld->hrnl", q, k) / math.sqrt(D)
    if causal:
        sc = sc.masked_fill(torch.arange(L).view(1, L) > rows.view(-1, 1), float("-inf"))
    top = sc.gather(-1, j.unsqueeze(-1)).squeeze(-1)
    second = sc.scatter(-1, j.unsqueeze(-1), float("-inf")).amax(-1)
    assert bool(((top - second) >= 40).all() | torch.isinf(second).all())
    return q.reshape(1, H * R, n_rows, D), k.unsqueeze(0), j


def _ramp_keys(gen, H, L, D, rising):
    """key[0] (exact in the dtype once rounded) rises across every key tile — the one-pass form rescales at each — or falls from
    the first tile; with a query (8, 0, ..., 0) the scores span 0 .. 192 * scale."""
    k = 0.3 * torch.randn(H, L, D, generator=gen, dtype=torch.float64)
    ramp = torch.linspace(0.0, 24.0, L, dtype=torch.float64)
    k[:, :, 0] = ramp if rising else ramp.flip(0)
    return k.unsqueeze(0)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("R", PREFILL_RATIOS)
def test_prefill_known_answers(dtype, R):
    from cold_compress_amd.attention_utils import prefill_attention

    H, D = _kv_heads(R), 128
    HQ = H * R
    gen = torch.Generator().manual_seed(R)
    for L in (65, 300):
        what = f"{dtype} H={H} R={R} L={L}"
        # head mapping: V of kv head h is the constant c_h -> every query head h * R + r returns c_h (to one rounding of P . V)
        c = torch.tensor([0.5 + 0.25 * h for h in range(H)], dtype=torch.float64)
        q = torch.randn(1, HQ, L, D, generator=gen).to(dtype).to(DEV)
        k = torch.randn(1, H, L, D, generator=gen).to(dtype).to(DEV)
        v = c.view(1, H, 1, 1).expand(1, H, L, D).to(dtype).to(DEV)
        want = c.repeat_interleave(R).view(HQ, 1, 1).to(DEV)
        for ra in (False, True):
            y, _ = prefill_attention(q, k, v, return_attn=ra)
            err = (y[0].double() - want).abs()
            assert bool((err <= _spacing(want, dtype)).all()), f"{what} head mapping (return_attn={ra}): {float(err.max())}"
        # identical keys: causal rows are uniform, P = dtype(1 / (q + 1)); column sums and observation means follow
        k1 = torch.randn(1, H, 1, D, generator=gen).to(dtype).expand(1, H, L, D).contiguous().to(DEV)
        vr = torch.randn(1, H, L, D, generator=gen).to(dtype).to(DEV)
        y, summ = prefill_attention(q, k1, vr, return_attn=True)
        p = AR.rnd(1.0 / torch.arange(1, L + 1, dtype=torch.float64), dtype)
        cs = p.flip(0).cumsum(0).flip(0)  # sum over q >= k
        ol = min(16, L)
        ob = torch.zeros(L, dtype=torch.float64)
        for i in range(L - ol, L):
            ob[: i + 1] += p[i]
        ob /= ol
        cs_d = summ.colsum.double().cpu()
        assert bool(((cs_d - cs).abs() <= _spacing(cs, dtype)).all()), f"{what} identical keys: column sums {float((cs_d - cs).abs().max())}"
        assert float((summ.obs_mean.double().cpu() - ob).abs().max()) <= float(_spacing(ob, dtype).max()), f"{what} identical keys: obs"
        yr = AR.prefill_ref(q, k1, vr, need_side=False)["y"]
        assert float((y[0].double() - yr).abs().max()) <= 1e-3 + 2 * _ulp(dtype) * float(yr.abs().max()), f"{what} identical keys: y"
        # one dominant key per query: y is that key's V row, bit for bit
        qd, kd, j = _dominant(gen, H, R, L, D, L, causal=True)
        vd = _exact_values(gen, (1, H, L, D), "cpu")
        want = vd[0][torch.arange(H).view(H, 1, 1), j].reshape(HQ, L, D).to(dtype).to(DEV)
        for ra in (False, True):
            y, _ = prefill_attention(qd.to(dtype).to(DEV), kd.to(dtype).to(DEV), vd.to(dtype).to(DEV), return_attn=ra)
            assert torch.equal(y[0], want), f"{what} dominant key (return_attn={ra}): {int((y[0] != want).sum())} entries differ"
        # running maximum: rising across every key tile, then largest in the first tile
        for rising in (True, False):
            qr = torch.zeros(1, HQ, L, D, dtype=torch.float64)
            qr[..., 0] = 8.0  # q . k = 8 * key[0], exact: no score sits on a rounding boundary of the accumulation order
            _prefill_vs_ref(qr.to(dtype).to(DEV), _ramp_keys(gen, H, L, D, rising).to(dtype).to(DEV),
                            torch.randn(1, H, L, D, generator=gen).to(dtype).to(DEV), f"{what} rising={rising}")


def _prefill_vs_ref(q, k, v, what):
    from cold_compress_amd.attention_utils import prefill_attention

    dtype = q.dtype
    yr = AR.prefill_ref(q, k, v, need_side=False)["y"]
    tol = 1e-3 + 2 * _ulp(dtype) * float(yr.abs().max())
    for ra in (False, True):
        y, _ = prefill_attention(q, k, v, return_attn=ra)
        assert float((y[0].double() - yr).abs().max()) <= tol, f"{what} (return_attn={ra})"


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("R", DECODE_RATIOS)
def test_decode_known_answers(R, dtype, D):
    from cold_compress_amd.attention_utils import scaled_dot_product_attention as sdpa

    H = 4 if R <= 7 else 2
    HQ = H * R
    gen = torch.Generator().manual_seed(50 + R)
    for S in (513, 4096):
        what = f"{dtype} H={H} R={R} S={S} D={D}"
        mask = torch.rand(1, H, 1, S, generator=gen) > 0.4
        mask[..., -1] = True
        md = mask.to(DEV)
        c = torch.tensor([0.5 + 0.25 * h for h in range(H)], dtype=torch.float64)
        q = torch.randn(1, HQ, 1, D, generator=gen).to(dtype).to(DEV)
        k = torch.randn(1, H, S, D, generator=gen).to(dtype).to(DEV)
        v = c.view(1, H, 1, 1).expand(1, H, S, D).to(dtype).to(DEV)
        want = c.repeat_interleave(R).view(HQ, 1).to(DEV)
        y, _ = sdpa(q, k, v, attn_mask=md)
        err = (y[0, :, 0].double() - want).abs()
        assert bool((err <= _spacing(want, dtype)).all()), f"{what} head mapping: {float(err.max())}"
        # identical keys: every live slot gets dtype(1 / n_live) in every query head; the group mean is the same value
        k1 = torch.randn(1, H, 1, D, generator=gen).to(dtype).expand(1, H, S, D).contiguous().to(DEV)
        y, probs = sdpa(q, k1, v, attn_mask=md, return_attn=True)
        _, gm = sdpa(q, k1, v, attn_mask=md, return_attn=True, group_mean=True)
        n = mask[0, :, 0].sum(-1).double()
        pw = (AR.rnd(1.0 / n, dtype).view(H, 1) * mask[0, :, 0].double()).to(DEV)
        pr = probs[0, :, 0].double().view(H, R, S)
        assert bool(((pr - pw.view(H, 1, S)).abs() <= _spacing(pw, dtype).view(H, 1, S)).all()), f"{what} identical keys: probabilities"
        assert bool((pr == pr[:, :1]).all()), f"{what} identical keys: the query heads of a group differ"
        assert bool(((gm[0, :, 0].double() - pw).abs() <= _spacing(pw, dtype)).all()), f"{what} identical keys: group mean"
        # one dominant key per query head: y is that key's V row, bit for bit
        qd, kd, j = _dominant(gen, H, R, S, D, 1, causal=False)
        live = torch.ones(1, H, 1, S, dtype=torch.bool)
        live[..., ::3] = False
        live[0, torch.arange(H).view(H, 1), 0, j[:, :, 0]] = True
        vd = _exact_values(gen, (1, H, S, D), "cpu")
        want = vd[0][torch.arange(H).view(H, 1), j[:, :, 0]].reshape(HQ, D).to(dtype).to(DEV)
        for gmode in (False, True):
            y, _ = sdpa(qd.to(dtype).to(DEV), kd.to(dtype).to(DEV), vd.to(dtype).to(DEV), attn_mask=live.to(DEV), return_attn=gmode,
                        group_mean=gmode)
            assert torch.equal(y[0, :, 0], want), f"{what} dominant key: {int((y[0, :, 0] != want).sum())} entries differ"
        # running maximum across the splits, rising and falling
        for rising in (True, False):
            qr = torch.zeros(1, HQ, 1, D, dtype=torch.float64)
            qr[..., 0] = 8.0  # q . k = 8 * key[0], exact: no score sits on a rounding boundary of the accumulation order
            _decode_vs_ref(qr.to(dtype).to(DEV), _ramp_keys(gen, H, S, D, rising).to(dtype).to(DEV),
                           torch.randn(1, H, S, D, generator=gen).to(dtype).to(DEV), md, f"{what} rising={rising}")


# ------------------------------------------------------------------------------------ c. decode attention against attn_ref


def _decode_vs_ref(q, k, v, mask, what):
    from cold_compress_amd.attention_utils import scaled_dot_product_attention as sdpa

    dtype = q.dtype
    yr, pr, gr = AR.decode_ref(q, k, v, mask)
    y, probs = sdpa(q, k, v, attn_mask=mask, return_attn=True)
    y2, gm = sdpa(q, k, v, attn_mask=mask, return_attn=True, group_mean=True)
    y3, none = sdpa(q, k, v, attn_mask=mask, return_attn=False)
    assert none is None and torch.equal(y, y2) and torch.equal(y, y3), f"{what}: y depends on what else is returned"
    ulp = _ulp(dtype)
    err = float((y[0, :, 0].double() - yr).abs().max())
    assert err <= 1e-3 + 2 * ulp * float(yr.abs().max()), f"{what}: y {err}"
    err = float((probs[0, :, 0].double() - pr).abs().max())
    assert err < 1e-3 + 2 * ulp, f"{what}: probabilities {err}"
    err = float((gm[0, :, 0].double() - gr).abs().max())
    assert err < 1e-3 + 2 * ulp, f"{what}: group mean {err}"
    if mask is not None:
        dead = probs[0, :, 0].view(k.shape[1], -1, k.shape[2])[~mask[0, :, 0].unsqueeze(1).expand(-1, q.shape[1] // k.shape[1], -1)]
        assert dead.numel() == 0 or float(dead.abs().max()) == 0.0, f"{what}: masked slots carry probability"


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("R", DECODE_RATIOS)
def test_decode_attention_at_odd_ratios(R, dtype, D):
    H = 4 if R <= 7 else 2
    HQ = H * R
    for S in DECODE_LENGTHS:
        for p_masked in (0.97, 0.5, 0.0):
            gen = torch.Generator().manual_seed(S + 7 * R + int(100 * p_masked))
            q = torch.randn(1, HQ, 1, D, generator=gen).to(dtype).to(DEV)
            k = torch.randn(1, H, S, D, generator=gen).to(dtype).to(DEV)
            v = torch.randn(1, H, S, D, generator=gen).to(dtype).to(DEV)
            mask = torch.rand(1, H, 1, S, generator=gen) >= p_masked
            mask[..., -1] = True
            _decode_vs_ref(q, k, v, mask.to(DEV), f"{dtype} H={H} R={R} S={S} D={D} p_masked={p_masked}")


# ------------------------------------------------------------------------------------ d. fused decode steps, several z-blocks


def _one_launch(kv, HQ):
    import cold_compress_amd.cache as cache
    from cold_compress_amd import _abi

    if hasattr(kv, "single_launch_active"):
        return kv.single_launch_active(HQ)
    fn = "cc_decode_step_l2_single_launch" if isinstance(kv, cache.KVCacheL2) else "cc_decode_step_single_launch"
    return bool(_abi.lib()[fn](HQ, kv.n_heads, kv.max_cache_length, kv.head_dim, cache._DT[kv.k_cache.dtype]))


def _step_twins(strategy, dtype, H, HQ, S, D, T, steps=8, W=1, seed=0):
    """decode_step against update_kv -> attention -> update_state on twin caches: y and every buffer bit for bit at every step
    (the two-launch form is bit-identical to the three calls), and the step ran in its two-launch form."""
    import cold_compress_amd.cache as cache
    from cold_compress_amd.attention_utils import scaled_dot_product_attention as sdpa
    from cold_compress_amd.attention_utils import single_launch_status

    cls, rk = cache.get_cache_constructor(strategy)
    kw = dict(max_cache_length=S, global_tokens=4, recent_window=10, history_window_size=W, attn_thresholding=False,
              max_seq_length=4 * S + 64, cache_bits=None)

    def mk():
        with torch.device(DEV):
            return cls(1, H, D, dtype, **{x: kw[x] for x in rk})

    a, b = mk(), mk()
    assert b.supports_fused_step()
    assert not _one_launch(b, HQ), f"{HQ} query heads over {H} kv heads must take the two-launch step"
    gen = torch.Generator().manual_seed(seed)
    if strategy == "random":
        draws = [torch.rand(S, generator=gen).to(DEV) for _ in range(steps + 1)]
        ia, ib = iter(draws), iter(draws)
        a._rand = lambda: next(ia)
        b._rand = lambda: next(ib)
    k0 = torch.randn(1, H, T, D, generator=gen).to(dtype).to(DEV)
    v0 = torch.randn(1, H, T, D, generator=gen).to(dtype).to(DEV)
    for kv in (a, b):
        kv.update_kv(torch.arange(T, device=DEV), k0, v0, True)
        if strategy == "l2":
            kv.update_state(torch.arange(T, device=DEV), k0, v0, True, None)
    if strategy == "heavy_hitter" and W == 1:  # a history with structure instead of zeros (the ring keeps its tracked sums: zeros)
        hist = torch.rand(H, T, generator=gen, dtype=torch.float64).to(DEV)
        den = torch.randint(1, 5, (H, T), generator=gen, dtype=torch.int32).to(DEV)
        for kv in (a, b):
            kv.attn_history_num[0, :, :T, 0] = hist
            kv.attn_history_denom[0, :, :T] = den
    for t in range(steps):
        p = torch.tensor([T + t], dtype=torch.int32, device=DEV)
        k1 = torch.randn(1, H, 1, D, generator=gen).to(dtype).to(DEV)
        v1 = torch.randn(1, H, 1, D, generator=gen).to(dtype).to(DEV)
        q = (1.5 * torch.randn(1, HQ, 1, D, generator=gen)).to(dtype).to(DEV)
        ka, va, ma = a.update_kv(p, k1, v1, False)
        ya, at = sdpa(q, ka, va, attn_mask=ma, return_attn=a.return_attn(), group_mean=True)
        a.update_state(p, k1, v1, False, at)
        yb = b.decode_step(q, k1, v1, p)
        torch.cuda.synchronize()
        what = f"{strategy} W={W} {dtype} H={H} HQ={HQ} S={S} T={T} step {t}"
        assert torch.equal(ya, yb), f"{what}: y"
        for (na, ta), (nb, tb) in zip(a.named_buffers(), b.named_buffers()):
            if na not in ("next_key", "step_commit"):  # (pipeline bookkeeping of the fused step, not reference state)
                assert torch.equal(ta, tb), f"{what}: {na}"
    assert single_launch_status(b.pos.device) == 0


STEP_SHAPES = [(4, 28, 600, 590), (4, 28, 4096, 4096), (4, 28, 8200, 8190), (8, 24, 2048, 2040), (2, 12, 1500, 1500)]


@pytest.mark.parametrize("H,HQ,S,T", STEP_SHAPES)
@pytest.mark.parametrize("strategy,W", [("heavy_hitter", 1), ("heavy_hitter", 8), ("l2", 1), ("recent_global", 1), ("full", 1),
                                        ("random", 1)])
def test_fused_step_equals_three_calls_at_odd_ratios(strategy, W, H, HQ, S, T):
    dtype = torch.float16 if (S + HQ) % 3 == 0 else torch.bfloat16
    _step_twins(strategy, dtype, H, HQ, S, 128, T, W=W, seed=S + HQ)


@pytest.mark.parametrize("H,HQ,S", [(4, 28, 600), (4, 28, 4096), (8, 24, 2048), (2, 12, 1500)])
def test_hybrid_step_equals_three_calls_at_odd_ratios(H, HQ, S):
    """tools/fuzz_step.py's hybrid-step case (random fill levels, policies, protection masks, punctuation) at these shapes."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import fuzz_step as F

    for i, dt in enumerate((torch.bfloat16, torch.float16)):
        r = F.one_hybrid_step(F.Forced(900 + S + i, {0: dt, 1: H, 2: HQ // H, 4: S}), 900 + i)
        assert r == "", r


def test_heavy_hitter_own_state_vs_oracle_qwen2_shape(oracle):
    """48 fused steps at Qwen2's shape (4 kv heads, 28 query heads) against the oracle's pipeline, each on its own state."""
    import cold_compress_amd.cache as cache
    from helpers import hh_own_state_steps

    H, HQ, S, D, g, w, T = 4, 28, 4096, 128, 4, 10, 4090
    dtype = torch.bfloat16
    with torch.device(DEV):
        kv = cache.KVCacheHeavyHitter(1, H, D, dtype, max_cache_length=S, max_seq_length=4 * S, cache_bits=None, global_tokens=g,
                                      history_window_size=1, recent_window=w, attn_thresholding=False)
    assert not kv.single_launch_active(HQ)
    gen = torch.Generator().manual_seed(28)
    kv.update_kv(torch.arange(T, device=DEV), torch.randn(1, H, T, D, generator=gen).to(dtype).to(DEV),
                 torch.randn(1, H, T, D, generator=gen).to(dtype).to(DEV), True)
    kv.attn_history_num[0, :, :T, 0] = torch.rand(H, T, generator=gen, dtype=torch.float64).to(DEV)
    kv.attn_history_denom[0, :, :T] = 1
    st = dict(k=to_np(kv.k_cache.cpu()[0]), v=to_np(kv.v_cache.cpu()[0]), pos=kv.pos.cpu()[0].numpy().copy(),
              mask=kv.mask.cpu()[0, :, 0].numpy().astype(np.uint8), cts=kv.cache_cts.cpu().numpy().copy(),
              num=kv.attn_history_num.cpu()[0, :, :, 0].numpy().copy(), denom=kv.attn_history_denom.cpu()[0].numpy().copy(),
              ctr=np.zeros(1, np.int64))
    justified, total = hh_own_state_steps(oracle, kv, st, gen, T + 1, 48, HQ, g, w, dtype)
    assert justified <= 0.05 * total, (justified, total)
    assert kv.step_status(HQ) == 0


# ------------------------------------------------------------------------------------ e. the fuzzer at odd ratios


def test_fused_step_fuzz_at_odd_ratios():
    """tools/fuzz_step.py's step and hybrid-step families with 3, 5, 6, 7 or 12 query heads per kv head, 60 cases."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz_step.py"), "--n", "60", "--seed", "11", "--ratios", "3,5,6,7,12"],
                       cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and " 0 mismatches, single-launch hand-off timeouts: 0" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ------------------------------------------------------------------------------------ f. fused quantised caches refuse, untouched


@pytest.mark.parametrize("mode,bits", [("fused", 8), ("fp8", 8), ("uint4", 4)])
@pytest.mark.parametrize("strategy", ["heavy_hitter", "recent_global", "hybrid"])
def test_fused_quant_step_refuses_unserved_ratio_and_leaves_cache_untouched(strategy, mode, bits):
    """The decode kernels over quantised images serve 4 or 8 query heads per pass: at Qwen2's 28 over 4 the step returns
    CC_ERR_UNSUPPORTED, and every buffer — images, qparams, pos, mask, history, next_key, step_commit — is byte-identical after."""
    import cold_compress_amd.cache as cache
    from cold_compress_amd._abi import ColdCompressError

    H, HQ, S, D, T = 4, 28, 600, 128, 590
    dtype = torch.bfloat16
    cls, rk = cache.get_cache_constructor(strategy)
    hyb = [{"strategy": "window_heavy_hitter", "heavy_hitter_frac": 0.25, "recent_window": 0.1}, {"strategy": "full"}]
    kw = dict(max_cache_length=S, global_tokens=4, recent_window=10, history_window_size=1, attn_thresholding=False, max_seq_length=S,
              cache_bits=bits, cache_quant_mode=mode, token_ids={"special": [[1]], "punctuation": [5]}, min_recovery_frac=0.9,
              hybrid_strategies=hyb)
    lk = {x: kw[x] for x in rk}
    lk["cache_quant_mode"] = mode
    with torch.device(DEV):
        kv = cls(1, H, D, dtype, **lk)
    assert kv.fused_quant
    gen = torch.Generator().manual_seed(3)
    extra = {"input_ids": torch.zeros(T, dtype=torch.int64, device=DEV)} if strategy == "hybrid" else {}
    kv.update_kv(torch.arange(T, device=DEV), torch.randn(1, H, T, D, generator=gen).to(dtype).to(DEV),
                 torch.randn(1, H, T, D, generator=gen).to(dtype).to(DEV), True, **extra)
    if strategy == "hybrid":
        kv.cache_strategies = (torch.arange(H, device=DEV) % len(hyb)).to(torch.int64).contiguous()
        kv.requires_heavy_hitter = True
    p = torch.tensor([T], dtype=torch.int32, device=DEV)
    kv.prepare_decode(p)
    torch.cuda.synchronize()
    before = {n: b.clone() for n, b in kv.named_buffers()}
    q = torch.randn(1, HQ, 1, D, generator=gen).to(dtype).to(DEV)
    k1 = torch.randn(1, H, 1, D, generator=gen).to(dtype).to(DEV)
    step_kw = {"input_ids": torch.tensor([[9]], dtype=torch.int64, device=DEV)} if strategy == "hybrid" else {}
    with pytest.raises(ColdCompressError):
        kv.decode_step(q, k1, k1, p, **step_kw)
    torch.cuda.synchronize()
    for n, b in kv.named_buffers():
        assert torch.equal(b.view(torch.uint8) if b.dtype != torch.bool else b, before[n].view(torch.uint8) if b.dtype != torch.bool
                           else before[n]), f"{strategy} {mode}: {n} changed by a refused step"


# ------------------------------------------------------------------------------------ g. the harness at Qwen2's shape


def _qwen2_runs(fused):
    """Qwen2-7B's geometry (28 query heads over 4 kv heads, head_dim 128, projection bias, norm_eps 1e-6, 152064-token vocabulary)
    with 2 layers: a heavy-hitter prefill that evicts, 16 eager decode tokens, then 16 under GraphedDecoder."""
    import argparse

    import cold_compress_amd.cache as cache
    from cold_compress_amd.harness import GraphedDecoder, ModelArgs, Transformer, decode_one_token, prefill, setup_caches
    from cold_compress_amd.harness.model import CONFIGS

    cfg = dict(CONFIGS["Qwen2-7B-Instruct"], n_layer=2, block_size=1024)
    torch.manual_seed(7)
    with torch.device(DEV):
        model = Transformer(ModelArgs(**cfg))
    model = model.to(torch.bfloat16).eval()
    g = torch.Generator(device=DEV).manual_seed(7)
    with torch.no_grad():
        for n, prm in model.named_parameters():
            prm.fill_(1.0) if "norm" in n else prm.normal_(0.0, 0.03, generator=g)
    assert model.config.norm_eps == 1e-6 and model.layers[0].attention.wqkv.bias is not None
    ap = argparse.ArgumentParser()
    cache.add_cache_arguments(ap)
    kw = vars(ap.parse_args([]))
    kw.update(cache_strategy=["heavy_hitter"], prompt_compression_strategy=["heavy_hitter"], max_cache_length=[128], global_tokens=4,
              recent_window=10, history_window_size=1)
    setup_caches(model, None, DEV, 600, dict(kw))
    for layer in model.layers:
        layer.attention.fuse_decode_step = fused
        layer.attention.fuse_state_update = fused
    assert not model.layers[0].attention.kv_cache.single_launch_active(cfg["n_head"])
    prompt = torch.randint(0, cfg["vocab_size"], (300,), generator=torch.Generator().manual_seed(3), dtype=torch.int32).to(DEV)
    toks, probs = [], []
    with torch.no_grad():
        tok, pr = prefill(model, prompt.view(1, -1), torch.arange(300, device=DEV))
        toks.append(int(tok))
        probs.append(pr.clone())
        pos = torch.tensor([300], dtype=torch.int32, device=DEV)
        cur = tok.view(1, 1).to(torch.int32)
        graphed = GraphedDecoder(model)
        for i in range(32):
            step = decode_one_token if i < 16 else graphed
            nt, pr = step(model, cur, pos)
            toks.append(int(nt))
            probs.append(pr.clone())
            cur = nt.view(1, 1).to(torch.int32)
            pos += 1
    torch.cuda.synchronize()
    state = {f"{li}.{n}": b.clone() for li, layer in enumerate(model.layers) for n, b in layer.attention.kv_cache.named_buffers()
             if n not in ("next_key", "step_commit")}
    assert model.layers[0].attention.kv_cache.step_status(cfg["n_head"]) == 0
    del model, graphed
    return toks, probs, state


def test_harness_qwen2_shape_fused_step_equals_three_calls():
    """The fused decode step (two launches at 7 query heads per kv head) against fuse_decode_step = False: tokens, next-token
    distributions and every cache buffer bit for bit, eager and graphed."""
    fused = _qwen2_runs(True)
    plain = _qwen2_runs(False)
    assert fused[0] == plain[0], "generated tokens"
    for i, (a, b) in enumerate(zip(fused[1], plain[1])):
        assert a.shape[-1] == 152064 and torch.equal(a, b), f"token {i}: distribution"
    for n in plain[2]:
        assert torch.equal(fused[2][n], plain[2][n]), n
