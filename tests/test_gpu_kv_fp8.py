"""The FP8 fused KV cache (cache_bits=8, cache_quant_mode="fp8"; include/coldcompress.h): OCP e4m3fn images with one power-of-two
scale per (head, slot) row, dequantised in the decode kernels by v_cvt_scalef32_pk_{bf16,f16}_fp8.  Pinned four ways:
  * cc_kv_dequant_rows on every code and every row exponent, and cc_kv_quant_rows on edge rows, against the numpy twin of the contract
    (tests/kv_fp8_twin.py, itself checked against torch.float8_e4m3fn by tests/test_kv_fp8_host.py), bit for bit;
  * every served policy's FP8 step against the SAME policy's 16-bit step fed the dequantised values (the pattern of
    tests/test_gpu_quant_fused.py and tests/test_gpu_quant_fused_ring_hybrid.py): every buffer and y bit for bit;
  * the graphed harness loop against the unquantised run, with the uint8 mode's bounds;
  * the property the format exists for: on rows with one outlier channel it reconstructs the other channels better than uint8.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from helpers import DT_CODE

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kv_fp8_twin as tw  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = __import__("helpers").TEST_DEVICE
D = 128
FP8 = 0x100 | 8  # CC_QUANT_FP8_E4M3
HYB5 = [{"strategy": "special"}, {"strategy": "special_punc"}, {"strategy": "special_punc_heavy_hitter", "heavy_hitter_frac": 0.3},
        {"strategy": "special_punc_window", "recent_window": 0.3}, {"strategy": "full"}]
HYB_YAML = [{"strategy": "window", "recent_window": 0.1},
            {"strategy": "window_heavy_hitter", "heavy_hitter_frac": 0.25, "recent_window": 0.1},
            {"strategy": "window_heavy_hitter", "heavy_hitter_frac": 0.5, "recent_window": 0.1}, {"strategy": "full"}]
TOKEN_IDS = {"special": [[1], [2, 3]], "punctuation": [5, 6, 7]}
NAME = {torch.bfloat16: "bf16", torch.float16: "f16"}


def _abi():
    from cold_compress_amd import _abi

    return _abi


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _quant_rows(x, fmt=FP8):
    """[N, Dx] rows -> (images [N, Dx] uint8, qparams K pair [N, 2], round trip [N, Dx]) by cc_kv_quant_rows / cc_kv_dequant_rows."""
    N, Dx = x.shape
    kq, vq = torch.empty((N, Dx), dtype=torch.uint8, device=DEV), torch.empty((N, Dx), dtype=torch.uint8, device=DEV)
    par = torch.empty((N, 4), dtype=torch.float32, device=DEV)
    out, out2 = torch.empty_like(x), torch.empty_like(x)
    _abi().call("cc_kv_quant_rows", _p(x), _p(x), 1, N, Dx, DT_CODE[x.dtype], fmt, _p(kq), _p(vq), _p(par), _st())
    _abi().call("cc_kv_dequant_rows", _p(kq), _p(vq), _p(par), 1, N, Dx, DT_CODE[x.dtype], fmt, _p(out), _p(out2), _st())
    return kq, par[:, 0:2], out


# ---------------------------------------------------------------------------------------------------------- the converters
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_exhaustive_decode_matches_the_twin(dtype):
    """All 256 codes x e in {-120, -40 .. 40, 120}: cc_kv_dequant_rows (the kernels' own conversion) is the twin's value bit for bit."""
    es = np.array([-120] + list(range(-40, 41)) + [120], np.int32)
    codes = np.tile(np.arange(256, dtype=np.uint8), (len(es), 1))
    par = np.zeros((len(es), 4), np.float32)
    par[:, 0] = np.ldexp(np.float32(1), es)
    par[:, 2] = par[:, 0]
    kq = torch.from_numpy(codes).to(DEV)
    vq = torch.from_numpy(codes[:, ::-1].copy()).to(DEV)
    k = torch.empty((len(es), 256), dtype=dtype, device=DEV)
    v = torch.empty_like(k)
    _abi().call("cc_kv_dequant_rows", _p(kq), _p(vq), _p(torch.from_numpy(par).to(DEV)), 1, len(es), 256, DT_CODE[dtype], FP8, _p(k), _p(v),
                _st())
    torch.cuda.synchronize()
    for got, cd in ((_bits(k), codes), (_bits(v), codes[:, ::-1])):
        want = tw.dequant_bits(cd, es, NAME[dtype])
        ok = tw.bits_equal(got, want, NAME[dtype])
        if not ok.all():
            r, c = np.argwhere(~ok)[0]
            raise AssertionError(f"{(~ok).sum()} values differ; first: e {es[r]} code {cd[r, c]:#04x}: {got[r, c]:#06x} vs {want[r, c]:#06x}")


def _edge_rows(dtype):
    g = np.random.default_rng(5)
    rows = [g.standard_normal(D) * 2]
    out = g.standard_normal(D)
    out[17] *= 50  # one outlier channel
    rows.append(out)
    rows.append(np.zeros(D))
    rows.append(np.linspace(-65504, 65504, D))  # near the f16 maximum
    tiny = g.standard_normal(D) * (1e-39 if dtype == torch.bfloat16 else 1e-6)  # bf16 subnormals / f16 subnormals
    rows.append(tiny)
    nan = g.standard_normal(D)
    nan[40] = np.nan
    rows.append(nan)
    rows.append(-np.abs(g.standard_normal(D)) * 448)
    return torch.tensor(np.stack(rows), dtype=torch.float32).to(dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_row_quantisation_matches_the_twin(dtype):
    x = _edge_rows(dtype)
    kq, kpar, rt = _quant_rows(x.to(DEV))
    torch.cuda.synchronize()
    codes, e = tw.quant_rows(x.float().numpy())
    assert np.array_equal(kq.cpu().numpy(), codes), np.argwhere(kq.cpu().numpy() != codes)[:5]
    assert np.array_equal(kpar[:, 0].cpu().numpy(), np.ldexp(np.float32(1), e)) and bool((kpar[:, 1] == 0).all())
    assert codes[5, 40] in (0x7F, 0xFF) and e[2] == 0  # the NaN and the all-zero row
    assert tw.bits_equal(_bits(rt), tw.dequant_bits(codes, e, NAME[dtype]), NAME[dtype]).all()


def test_fp8_reconstructs_outlier_rows_better_than_uint8():
    """Rows with one outlier channel (50x): the other channels' RMS reconstruction error is smaller with FP8 than with uint8."""
    g = torch.Generator().manual_seed(9)
    x = torch.randn(256, D, generator=g)
    x[:, 3] *= 50
    x = x.to(torch.bfloat16).to(DEV)
    rest = torch.ones(D, dtype=torch.bool)
    rest[3] = False
    err = {}
    for fmt in (8, FP8):
        _, _, rt = _quant_rows(x, fmt)
        err[fmt] = float(((rt.float() - x.float())[:, rest] ** 2).mean().sqrt())
    assert err[FP8] < err[8], err


def test_formats_other_than_uint8_and_fp8_are_unsupported():
    lib = _abi().lib()
    x = torch.ones(4, D, dtype=torch.bfloat16, device=DEV)
    q = torch.zeros(4, D, dtype=torch.uint8, device=DEV)
    par = torch.zeros(4, 4, device=DEV)
    for fmt in (4, 2, 0x100 | 4, 0x200 | 8):
        assert lib["cc_kv_quant_rows"](_p(x), _p(x), 1, 4, D, 1, fmt, _p(q), _p(q), _p(par), _st()) == -2
        assert lib["cc_decode_step_quant_single_launch"](32, 8, 4096, D, 1, fmt) == 0
        assert lib["cc_decode_step_hybrid_quant_single_launch"](32, 8, 4096, D, 1, fmt) == 0
    xf = x.float()
    assert lib["cc_kv_quant_rows"](_p(xf), _p(xf), 1, 4, D, 0, FP8, _p(q), _p(q), _p(par), _st()) == -2  # 16-bit model dtypes only
    torch.cuda.synchronize()
    assert bool((q == 0).all())


# ---------------------------------------------------------------------------------------------------------- the steps
def _mk(strategy, H, S, dtype, fp8, W=1, g=4, w=10):
    import cold_compress_amd.cache as cache

    cls, rk = cache.get_cache_constructor(strategy)
    kw = dict(max_cache_length=S, max_seq_length=4 * S, cache_bits=8 if fp8 else None, global_tokens=g, recent_window=w,
              history_window_size=W, attn_thresholding=False)
    lk = {k: kw[k] for k in rk}
    if W != 1:
        lk["history_window_size"] = W
    if fp8:
        lk["cache_quant_mode"] = "fp8"
    with torch.device(DEV):
        return cls(1, H, D, dtype, **lk)


@pytest.mark.parametrize("strategy", ["heavy_hitter", "recent_global", "full", "random"])
@pytest.mark.parametrize("dtype,H,HQ,S,T", [(torch.bfloat16, 8, 32, 4096, 4090), (torch.float16, 2, 16, 300, 290)])
@pytest.mark.parametrize("single", [False, True])
def test_fp8_step_equals_16bit_step_on_dequantised_values(strategy, dtype, H, HQ, S, T, single):
    """`b` = the FP8 cache, `a` = the same policy's 16-bit cache holding b's DEQUANTISED values and fed the twin's round trip of every
    new token: y, the cache contents, pos, mask, cache_cts and the history agree bit for bit, 12 steps, in both launch forms."""
    abi = _abi()
    abi.lib()["cc_decode_step_set_single_launch"](1 if single else 0)
    try:
        a, b = _mk(strategy, H, S, dtype, False), _mk(strategy, H, S, dtype, True)
        for kv in (a, b):
            if hasattr(kv, "single_launch"):
                kv.single_launch = single
        gen = torch.Generator().manual_seed(41)
        k0 = torch.randn(1, H, T, D, generator=gen).to(dtype).to(DEV)
        v0 = (2.0 * torch.randn(1, H, T, D, generator=gen)).to(dtype).to(DEV)
        for kv in (a, b):
            kv.update_kv(torch.arange(T, device=DEV), k0, v0, True)
            if strategy == "heavy_hitter":
                g2 = torch.Generator().manual_seed(42)
                kv.attn_history_num[0, :, :T, 0] = torch.rand(H, T, generator=g2, dtype=torch.float64).to(DEV)
                kv.attn_history_denom[0, :, :T] = torch.randint(1, 5, (H, T), generator=g2, dtype=torch.int32).to(DEV)
        kd, vd = b.dequantized_kv()
        a.k_cache.copy_(kd)
        a.v_cache.copy_(vd)
        if strategy == "random":
            draws = [torch.rand(S, generator=gen).to(DEV) for _ in range(20)]
            for kv in (a, b):
                it = iter(list(draws))
                kv._rand = lambda it=it: next(it)
        for t in range(12):
            p = torch.tensor([T + 5 + t], dtype=torch.int32, device=DEV)
            k1 = torch.randn(1, H, 1, D, generator=gen).to(dtype)
            v1 = (2.0 * torch.randn(1, H, 1, D, generator=gen)).to(dtype)
            q = torch.randn(1, HQ, 1, D, generator=gen).to(dtype).to(DEV)
            # the twin's round trip of the new rows (the contract), not the device's
            kh, vh = [torch.from_numpy(tw.dequant_bits(*tw.quant_rows(r.reshape(H, D).float().numpy()), NAME[dtype]).view(np.int16))
                      .view(dtype).view(1, H, 1, D).to(DEV) for r in (k1, v1)]
            ya = a.decode_step(q, kh, vh, p)
            yb = b.decode_step(q, k1.to(DEV), v1.to(DEV), p)
            torch.cuda.synchronize()
            if not torch.equal(ya, yb):
                d = (ya.float() - yb.float()).abs()[0, :, 0]
                kd, vd = b.dequantized_kv()
                raise AssertionError(f"step {t}: attention output: max |dy| {float(d.max()):.3e}; K rows differing "
                                     f"{(kd != a.k_cache).any(-1).nonzero().tolist()[:6]}; V rows {(vd != a.v_cache).any(-1).nonzero().tolist()[:6]}")
            kd, vd = b.dequantized_kv()
            assert torch.equal(kd, a.k_cache) and torch.equal(vd, a.v_cache), f"step {t}: cache contents"
            for name in ("pos", "mask", "cache_cts", "attn_history_num", "attn_history_denom", "attn_counter"):
                if hasattr(a, name):
                    assert torch.equal(getattr(a, name), getattr(b, name)), f"step {t}: {name}"
        if strategy == "heavy_hitter":
            assert b.step_status(HQ) == 0
        if single and S == 4096:
            if strategy == "heavy_hitter":
                assert b.single_launch_active(HQ)
            assert abi.lib()["cc_decode_step_quant_single_launch"](HQ, H, S, D, DT_CODE[dtype], FP8) == 1
    finally:
        abi.lib()["cc_decode_step_set_single_launch"](1)


def _mk_hyb(strategies, H, S, dtype, fp8):
    import cold_compress_amd.cache as cache

    kw = dict(max_cache_length=S, max_seq_length=S, cache_bits=8 if fp8 else None, global_tokens=4, token_ids=TOKEN_IDS,
              min_recovery_frac=0.9, hybrid_strategies=strategies)
    if fp8:
        kw["cache_quant_mode"] = "fp8"
    with torch.device(DEV):
        return cache.KVCacheHybrid(1, H, D, dtype, **kw)


def _pair(kind, W, strategies, H, S, T, dtype, seed):
    """Twin caches in the same decode-ready state: a (16-bit, holding b's dequantised K / V) and b (FP8)."""
    gen = torch.Generator().manual_seed(seed)
    if kind == "hh":
        a, b = _mk("heavy_hitter", H, S, dtype, False, W=W), _mk("heavy_hitter", H, S, dtype, True, W=W)
    else:
        a, b = _mk_hyb(strategies, H, S, dtype, False), _mk_hyb(strategies, H, S, dtype, True)
    k0 = torch.randn(1, H, T, D, generator=gen).to(dtype).to(DEV)
    v0 = (2.0 * torch.randn(1, H, T, D, generator=gen)).to(dtype).to(DEV)
    ring0 = (torch.rand(H, S, a.attn_history_num.shape[-1], generator=gen) * 1e-2).to(dtype)
    den0 = torch.randint(1, 500, (H, S), generator=gen, dtype=torch.int32)
    fill = torch.tensor([T if h % 2 == 0 else max(4, T // 2) for h in range(H)], dtype=torch.int32)
    sp0 = torch.rand(H, S, generator=gen) < 0.02
    pu0 = torch.rand(H, S, generator=gen) < 0.02
    for kv in (a, b):
        if kind == "hh":
            kv.update_kv(torch.arange(T, device=DEV), k0, v0, True)
        else:
            kv.update_kv(torch.arange(T, device=DEV), k0, v0, True, input_ids=torch.zeros(T, dtype=torch.int64, device=DEV))
            kv.cache_strategies = (torch.arange(H, device=DEV) % len(strategies)).to(torch.int64).contiguous()
            kv.requires_heavy_hitter = any("heavy_hitter" in s["strategy"] for s in strategies)
            kv.cache_cts.copy_(fill.to(DEV))
            live = torch.arange(S, device=DEV).view(1, S) < fill.to(DEV).view(H, 1)
            kv.mask[0, :, 0, :] = live
            kv.pos[0] = torch.where(live, torch.arange(S, device=DEV, dtype=kv.pos.dtype).view(1, S).expand(H, S),
                                    torch.full_like(kv.pos[0], -1))
            if hasattr(kv, "special_mask"):
                kv.special_mask[0] = sp0.to(DEV) & live
                kv.num_special.fill_(int(sp0[0, : int(fill[0])].sum()))
            if hasattr(kv, "punc_mask"):
                kv.punc_mask[0] = pu0.to(DEV) & live
                kv.num_punc.fill_(3)
        kv.attn_history_num.copy_(ring0.to(DEV).unsqueeze(0))
        kv.attn_history_denom.copy_(den0.to(DEV).unsqueeze(0))
    kd, vd = b.dequantized_kv()
    a.k_cache.copy_(kd)
    a.v_cache.copy_(vd)
    return a, b, gen


def _run_lockstep(kind, W, strategies, H, HQ, S, T, steps, dtype, seed, check_rows=True):
    a, b, gen = _pair(kind, W, strategies, H, S, T, dtype, seed)
    for t in range(steps):
        p = torch.tensor([T + 3 + t], dtype=torch.int32, device=DEV)
        k1 = torch.randn(1, H, 1, D, generator=gen).to(dtype).to(DEV)
        v1 = (2.0 * torch.randn(1, H, 1, D, generator=gen)).to(dtype).to(DEV)
        q = torch.randn(1, HQ, 1, D, generator=gen).to(dtype).to(DEV)
        kq_new, kpar_new, kh = _quant_rows(k1.reshape(H, D))
        vq_new, vpar_new, vh = _quant_rows(v1.reshape(H, D))
        kimg0, vimg0, par0 = (b.k_cache_q.clone(), b.v_cache_q.clone(), b.kv_qparams.clone()) if check_rows else (None, None, None)
        if kind == "hh":
            ya = a.decode_step(q, kh.view(1, H, 1, D), vh.view(1, H, 1, D), p)
            yb = b.decode_step(q, k1, v1, p)
        else:
            ids = torch.tensor([[6 if t % 5 == 2 else 11]], dtype=torch.int64, device=DEV)  # every fifth token is punctuation
            ya = a.decode_step(q, kh.view(1, H, 1, D), vh.view(1, H, 1, D), p, input_ids=ids)
            yb = b.decode_step(q, k1, v1, p, input_ids=ids)
        torch.cuda.synchronize()
        assert torch.equal(ya, yb), f"step {t}: attention output, max |dy| {float((ya.float() - yb.float()).abs().max()):.3e}"
        kd, vd = b.dequantized_kv()
        assert torch.equal(kd, a.k_cache) and torch.equal(vd, a.v_cache), f"step {t}: cache contents"
        bb = dict(b.named_buffers())
        for name, ta in a.named_buffers():
            if name not in ("k_cache", "v_cache"):
                assert torch.equal(ta, bb[name]), f"step {t}: {name}"
        if check_rows:  # the step writes the inserted token's rows (cc_kv_quant_rows of them) and nothing else
            slot = (b.pos[0] == int(p)).int().argmax(dim=1)
            hs = torch.arange(H, device=DEV)
            assert torch.equal(b.k_cache_q[0, hs, slot], kq_new) and torch.equal(b.v_cache_q[0, hs, slot], vq_new), f"step {t}: image"
            assert torch.equal(b.kv_qparams[0, hs, slot, 0:2], kpar_new) and torch.equal(b.kv_qparams[0, hs, slot, 2:4], vpar_new)
            keep = torch.ones(H, b.max_cache_length, dtype=torch.bool, device=DEV)
            keep[hs, slot] = False
            for now, before in ((b.k_cache_q, kimg0), (b.v_cache_q, vimg0), (b.kv_qparams, par0)):
                assert torch.equal(now[0][keep], before[0][keep]), f"step {t}: rows other than the inserted one changed"
    return a, b


@pytest.mark.parametrize("W", [8, 400])
def test_ring_lockstep_64_steps(W):
    """The windowed heavy hitter at C3 size (8 kv heads, 32 query heads, S = 4096): 64 steps of the FP8 ring step (two launches)."""
    a, b = _run_lockstep("hh", W, None, 8, 32, 4096, 4090, 64, torch.bfloat16, 51 + W, check_rows=(W == 8))
    assert not b.single_launch_active(32) and b.step_status(32) == 0


def test_hybrid_c4_lockstep_64_steps_one_launch():
    """C4 size (8 kv heads, 32 query heads, S = 18432): 64 steps of the FP8 hybrid step, as one launch."""
    H, HQ, S = 8, 32, 18432
    assert _abi().lib()["cc_decode_step_hybrid_quant_single_launch"](HQ, H, S, D, 1, FP8) == 1
    a, b = _run_lockstep("hyb", 400, HYB_YAML, H, HQ, S, 18300, 64, torch.bfloat16, 61, check_rows=False)
    assert b.single_launch_active(HQ) and a.single_launch_active(HQ)
    assert b.step_status(HQ) == 0


@pytest.mark.parametrize("two", [False, True])
def test_hybrid_small_both_forms(two):
    """A small f16 hybrid cache (appends, evictions, dropped and punctuation tokens) in the single- and the two-launch form."""
    fn = _abi().lib()["cc_decode_step_device_single_launch"]
    if two:
        fn(0)
    try:
        a, b = _run_lockstep("hyb", 400, HYB5, 2, 16, 1000, 20, 14, torch.float16, 71)
        assert b.single_launch_active(16) == a.single_launch_active(16)
        assert b.step_status(16) == 0
    finally:
        if two:
            fn(1)


# ---------------------------------------------------------------------------------------------------------- the harness
def test_fp8_end_to_end_in_the_harness():
    """The tiny-Llama loop of tests/test_gpu_quant_fused.py::test_fused_quant_end_to_end_in_the_harness with cache_quant_mode="fp8":
    prefill through the HIP path, row quantisation of the compacted prompt, hipGraph decode over the FP8 images, teacher-forced against
    the unquantised run, with the same bounds."""
    from cold_compress_amd.harness import GraphedDecoder, ModelArgs, Transformer, decode_one_token, prefill, setup_caches

    dev = torch.device(DEV)
    cfg = dict(block_size=1024, vocab_size=512, n_layer=2, n_head=8, n_local_heads=2, dim=1024, intermediate_size=2048)
    torch.manual_seed(5)
    model = Transformer(ModelArgs(**cfg)).to(torch.bfloat16).eval()
    with torch.no_grad():
        g = torch.Generator().manual_seed(5)
        for n, p in model.named_parameters():
            p.fill_(1.0) if "norm" in n else p.normal_(0.0, 0.05, generator=g)
    model = model.to(dev)
    prompt = torch.randint(0, cfg["vocab_size"], (300,), generator=torch.Generator().manual_seed(3), dtype=torch.int32).to(dev)
    runs = {}
    for name, extra in (("bf16", {}), ("fused", {"cache_bits": 8, "cache_quant_mode": "fused"}),
                        ("fp8", {"cache_bits": 8, "cache_quant_mode": "fp8"})):
        kw = dict(max_cache_length=[128.0], cache_bits=None, cache_length_pattern="tile", cache_strategy=["heavy_hitter"],
                  cache_strategy_pattern="tile", feed_long_prompts=False, prompt_compression_strategy=["heavy_hitter"], global_tokens=4,
                  recent_window=10, history_window_size=1, attn_thresholding=False, min_recovery_frac=0.9)
        kw.update(extra)
        setup_caches(model, None, dev, 400, kw)
        with torch.no_grad():
            tok, probs = prefill(model, prompt.view(1, -1), torch.arange(300, device=dev))
            pos = torch.tensor([300], dtype=torch.int32, device=dev)
            plist, toks = [probs.float().clone()], [int(tok)]
            cur = tok.view(1, 1).to(torch.int32)
            step = GraphedDecoder(model) if name != "bf16" else decode_one_token
            for i in range(16):
                nt, pr = step(model, cur, pos)
                plist.append(pr.float().clone())
                toks.append(int(nt))
                cur = (nt if name == "bf16" else torch.tensor(runs["bf16"][0][len(toks) - 1], device=dev)).view(1, 1).to(torch.int32)
                pos += 1
        torch.cuda.synchronize()
        kv = model.layers[0].attention.kv_cache
        runs[name] = (toks, plist, kv.memory_usage(), kv)
    worst, agree = {}, {}
    for name in ("fused", "fp8"):
        assert torch.equal(runs["bf16"][1][0], runs[name][1][0])  # prefill attends to the prompt's own k / v: identical
        worst[name] = max(float((a - b).abs().max() / a.abs().max()) for a, b in zip(runs["bf16"][1], runs[name][1]))
        agree[name] = sum(int(a == b) for a, b in zip(runs["bf16"][0], runs[name][0]))
    print(f"end to end, worst relative probability drift / tokens agreeing: {worst} / {agree} of {len(runs['bf16'][0])}")
    # The uint8 mode's bounds hold for the tokens.  The probability drift bound is WIDER for FP8 than the uint8 test's 0.2, on
    # purpose and measured: on these well-behaved N(0, s) rows e4m3's 3 mantissa bits (relative step 2^-3, ~3x the RMS error of a
    # 255-step min..max grid) move the probability rows more: 0.48 measured on MI355X against uint8's 0.12, tokens 16 / 17 against
    # 17 / 17 (profiles/kv_fp8_bench_ab.jsonl).  The bit-exact checks of the step are the tests above; this one bounds
    # the format's effect on a model.
    assert worst["fused"] < 0.2 and agree["fused"] >= len(runs["bf16"][0]) - 2, (worst, agree)
    assert worst["fp8"] < 0.6 and agree["fp8"] >= len(runs["bf16"][0]) - 2, (worst, agree)
    assert runs["fp8"][2] < 0.6 * runs["bf16"][2]
    kv = runs["fp8"][3]
    assert kv.fused_quant and kv.quant_format == FP8 and kv.k_cache.numel() == 0 and kv.step_status(cfg["n_head"]) == 0
