"""The fused quantised cache (cache_quant_mode="fused", include/coldcompress.h) for the two history-ring policies: the windowed heavy
hitter (history_window_size W > 1, cc_decode_step_heavy_hitter_ring_quant) and the FastGen hybrid cache (cc_decode_step_hybrid_quant_rc).

The mode is the build's own numerical contract, so its checker is the SAME policy's 16-bit step run on the dequantised values (the
pattern of tests/test_gpu_quant_fused.py): `a` = the 16-bit cache holding b's dequantised K / V and fed with the round trip of every new
row, `b` = the fused cache fed with the rows themselves.  After the dequantisation in registers the arithmetic is the 16-bit step's, so y,
positions, mask, counts, the ring, denominators, counter, window sums, next-eviction keys and commit words agree bit for bit, and the only
rows of the images a step writes are the inserted token's: cc_kv_quant_rows of its K / V rows."""
import ctypes as C

import pytest
import torch

from helpers import DT_CODE

pytestmark = pytest.mark.gpu
DEV = __import__("helpers").TEST_DEVICE
D = 128
HYB5 = [{"strategy": "special"}, {"strategy": "special_punc"}, {"strategy": "special_punc_heavy_hitter", "heavy_hitter_frac": 0.3},
        {"strategy": "special_punc_window", "recent_window": 0.3}, {"strategy": "full"}]
HYB_YAML = [{"strategy": "window", "recent_window": 0.1},
            {"strategy": "window_heavy_hitter", "heavy_hitter_frac": 0.25, "recent_window": 0.1},
            {"strategy": "window_heavy_hitter", "heavy_hitter_frac": 0.5, "recent_window": 0.1}, {"strategy": "full"}]
TOKEN_IDS = {"special": [[1], [2, 3]], "punctuation": [5, 6, 7]}
CC_ERR_UNSUPPORTED = -2


def _abi():
    from cold_compress_amd import _abi

    return _abi


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _quant_rows(x):
    """[H, D] rows -> (uint8 images [H, D], qparams K pair [H, 2]) by cc_kv_quant_rows, and their round trip [H, D]."""
    H = x.shape[0]
    kq, vq = torch.empty((H, D), dtype=torch.uint8, device=DEV), torch.empty((H, D), dtype=torch.uint8, device=DEV)
    par = torch.empty((H, 4), dtype=torch.float32, device=DEV)
    out, out2 = torch.empty_like(x), torch.empty_like(x)
    _abi().call("cc_kv_quant_rows", _p(x), _p(x), H, 1, D, DT_CODE[x.dtype], 8, _p(kq), _p(vq), _p(par), _st())
    _abi().call("cc_kv_dequant_rows", _p(kq), _p(vq), _p(par), H, 1, D, DT_CODE[x.dtype], 8, _p(out), _p(out2), _st())
    return kq, par[:, 0:2], out


@pytest.fixture
def two_launch():
    """two_launch(True): this device's steps take their two-launch forms (cc_decode_step_device_single_launch(0)); restored."""
    fn = _abi().lib()["cc_decode_step_device_single_launch"]
    state = {"set": False}

    def set_(on):
        if on:
            fn(0)
            state["set"] = True

    yield set_
    if state["set"]:
        fn(1)


def _mk_hh(W, H, S, dtype, fused):
    import cold_compress_amd.cache as cache

    kw = dict(max_cache_length=S, max_seq_length=4 * S, cache_bits=8 if fused else None, global_tokens=4, recent_window=10,
              history_window_size=W, attn_thresholding=False)
    if fused:
        kw["cache_quant_mode"] = "fused"
    with torch.device(DEV):
        return cache.KVCacheHeavyHitter(1, H, D, dtype, **kw)


def _mk_hyb(strategies, H, S, dtype, fused):
    import cold_compress_amd.cache as cache

    kw = dict(max_cache_length=S, max_seq_length=S, cache_bits=8 if fused else None, global_tokens=4, token_ids=TOKEN_IDS,
              min_recovery_frac=0.9, hybrid_strategies=strategies)
    if fused:
        kw["cache_quant_mode"] = "fused"
    with torch.device(DEV):
        return cache.KVCacheHybrid(1, H, D, dtype, **kw)


def _pair(kind, W, strategies, H, S, T, dtype, seed):
    """Twin caches in the same decode-ready state: a (16-bit, holding b's dequantised K / V) and b (fused)."""
    gen = torch.Generator().manual_seed(seed)
    if kind == "hh":
        a, b = _mk_hh(W, H, S, dtype, False), _mk_hh(W, H, S, dtype, True)
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
            # a decode-ready state without the profiling pass (as tests/test_gpu_hybrid.py): head h runs policy h % n, full-ish and
            # half-empty heads
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


def _compare(a, b, t, step_y):
    ya, yb = step_y
    assert torch.equal(ya, yb), f"step {t}: attention output, max |dy| {float((ya.float() - yb.float()).abs().max()):.3e}"
    kd, vd = b.dequantized_kv()
    assert torch.equal(kd, a.k_cache) and torch.equal(vd, a.v_cache), f"step {t}: cache contents"
    bb = dict(b.named_buffers())
    for name, ta in a.named_buffers():
        if name in ("k_cache", "v_cache"):
            continue
        assert torch.equal(ta, bb[name]), f"step {t}: {name}"


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
        _compare(a, b, t, (ya, yb))
        if check_rows:
            # the step writes the inserted token's rows and nothing else: its image and parameters are cc_kv_quant_rows of the rows
            slot = (b.pos[0] == int(p)).int().argmax(dim=1)  # [H] (every head stores the position, a dropped token at S - 1)
            assert bool((b.pos[0].gather(1, slot.view(H, 1)) == int(p)).all()), f"step {t}: inserted slots"
            hs = torch.arange(H, device=DEV)
            assert torch.equal(b.k_cache_q[0, hs, slot], kq_new) and torch.equal(b.v_cache_q[0, hs, slot], vq_new), f"step {t}: image"
            assert torch.equal(b.kv_qparams[0, hs, slot, 0:2], kpar_new) and torch.equal(b.kv_qparams[0, hs, slot, 2:4], vpar_new)
            keep = torch.ones(H, b.max_cache_length, dtype=torch.bool, device=DEV)
            keep[hs, slot] = False
            for now, before in ((b.k_cache_q, kimg0), (b.v_cache_q, vimg0), (b.kv_qparams, par0)):
                assert torch.equal(now[0][keep], before[0][keep]), f"step {t}: rows other than the inserted one changed"
    return a, b


@pytest.mark.parametrize("W", [8, 33, 400])
@pytest.mark.parametrize("dtype,H,HQ,S,T", [(torch.bfloat16, 8, 32, 4096, 4090), (torch.float16, 2, 16, 300, 290),
                                            (torch.bfloat16, 3, 12, 1001, 700)])
def test_ring_step_equals_16bit_step_on_dequantised_values(W, dtype, H, HQ, S, T):
    a, b = _run_lockstep("hh", W, None, H, HQ, S, T, 6, dtype, 11 + W)
    assert not b.single_launch_active(HQ) and b.step_status(HQ) == 0


@pytest.mark.parametrize("strategies,H,HQ,S,T,dtype", [(HYB5, 5, 20, 300, 280, torch.bfloat16), (HYB_YAML, 8, 32, 4100, 4000, torch.bfloat16),
                                                       (HYB5, 2, 16, 1000, 20, torch.float16), (HYB_YAML, 8, 64, 4096, 4000, torch.float16)])
@pytest.mark.parametrize("two", [False, True])
def test_hybrid_step_equals_16bit_step_on_dequantised_values(strategies, H, HQ, S, T, dtype, two, two_launch):
    """Both forms: the single launch where cc_decode_step_hybrid_quant_single_launch says so, the two launches (switched on for the
    device); appends, evictions, dropped tokens and punctuation tokens."""
    two_launch(two)
    lib = _abi().lib()
    one = bool(lib["cc_decode_step_hybrid_quant_single_launch"](HQ, H, S, D, DT_CODE[dtype], 8))
    assert one == bool(lib["cc_decode_step_hybrid_single_launch"](HQ, H, S, D, DT_CODE[dtype]))  # the 16-bit step's shapes
    a, b = _run_lockstep("hyb", 400, strategies, H, HQ, S, T, 14, dtype, 3 + H)
    assert b.single_launch_active(HQ) == a.single_launch_active(HQ) == (one and not two)
    assert b.step_status(HQ) == 0


def test_hybrid_c4_lockstep_64_steps():
    """C4 size (8 kv heads, 32 query heads, S = 18432): 64 steps of the fused step against its 16-bit twin fed the dequantised values."""
    H, HQ, S = 8, 32, 18432
    one = bool(_abi().lib()["cc_decode_step_hybrid_quant_single_launch"](HQ, H, S, D, 1, 8))
    a, b = _run_lockstep("hyb", 400, HYB_YAML, H, HQ, S, 18300, 64, torch.bfloat16, 21, check_rows=False)
    assert b.single_launch_active(HQ) == one == a.single_launch_active(HQ)
    assert b.step_status(HQ) == 0


def test_ring_c3_lockstep_64_steps():
    """C3 size (8 kv heads, 32 query heads, S = 4096), W = 400: 64 steps against the 16-bit twin."""
    _run_lockstep("hh", 400, None, 8, 32, 4096, 4096, 64, torch.bfloat16, 22, check_rows=False)


def test_n_bit_other_than_8_is_unsupported():
    lib = _abi().lib()
    H, HQ, S = 2, 8, 256
    b = _mk_hh(8, H, S, torch.bfloat16, True)
    h = _mk_hyb(HYB5, H, S, torch.bfloat16, True)
    h.cache_strategies = torch.zeros(H, dtype=torch.int64, device=DEV)
    q = torch.zeros(HQ, D, dtype=torch.bfloat16, device=DEV)
    k = torch.zeros(H, D, dtype=torch.bfloat16, device=DEV)
    p = torch.tensor([300], dtype=torch.int32, device=DEV)
    y = torch.empty(HQ, D, dtype=torch.bfloat16, device=DEV)
    ws = torch.zeros(int(lib["cc_decode_attn_workspace_bytes"](HQ, H, S, D, 1)), dtype=torch.uint8, device=DEV)
    wsum, acc = b._window_state()
    img0 = b.k_cache_q.clone()
    rc = lib["cc_decode_step_heavy_hitter_ring_quant"](b._view(), _p(b.kv_qparams), 4, _p(q), _p(k), _p(k), _p(p), _p(b.attn_history_num),
                                                        _p(b.attn_history_denom), _p(b.attn_counter), 8, _p(acc), _p(wsum), _p(b.next_key),
                                                        4, 10, HQ, 0.1, _p(y), None, _p(ws), ws.numel(), _st())
    assert rc == CC_ERR_UNSUPPORTED
    tab = h._policy_table()
    wsum, acc = h._window_state()
    rc = lib["cc_decode_step_hybrid_quant_rc"](h._view(), _p(h.kv_qparams), 4, _p(q), _p(k), _p(k), _p(p), _p(h.cache_strategies), _p(tab),
                                               tab.shape[0], _p(h.attn_history_num), _p(h.attn_history_denom), _p(h.attn_counter), 400,
                                               _p(acc), _p(wsum), None, None, None, None, 0, None, None, _p(h.next_key), _p(h.step_commit),
                                               4, HQ, 0.1, _p(y), None, _p(ws), ws.numel(), _st())
    assert rc == CC_ERR_UNSUPPORTED
    assert lib["cc_decode_step_hybrid_quant_single_launch"](32, 8, 4096, D, 1, 4) == 0
    torch.cuda.synchronize()
    assert torch.equal(b.k_cache_q, img0) and int(b.attn_counter) == 0  # nothing launched


class _Tok:
    def special_ids(self):
        return [[1], [2, 3]]

    def punctuation_ids(self):
        return [5, 6, 7, 11, 13]


@pytest.mark.parametrize("strategy", ["hybrid", "heavy_hitter_w8"])
def test_fused_ring_and_hybrid_end_to_end_in_the_harness(strategy):
    """The tiny-Llama loop of tests/test_gpu_quant_fused.py::test_fused_quant_end_to_end_in_the_harness for the hybrid cache (prompt
    compression `full`, profiled at prefill) and the heavy hitter with W = 8, hipGraph decode over the uint8 images, teacher-forced
    against the unquantised run: next-token distributions close, the cache statistics smaller by the K / V bytes saved less 16 B of
    row parameters per (head, slot), and the single-launch hand-off never times out."""
    from cold_compress_amd.harness import GraphedDecoder, ModelArgs, Transformer, prefill, setup_caches

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
    if strategy == "hybrid":
        base = dict(max_cache_length=[1.0], cache_strategy=["hybrid"], prompt_compression_strategy=["full"], history_window_size=1,
                    hybrid_strategies=HYB_YAML)
    else:
        base = dict(max_cache_length=[128.0], cache_strategy=["heavy_hitter"], prompt_compression_strategy=["heavy_hitter"],
                    history_window_size=8)
    runs = {}
    for name, extra in (("bf16", {}), ("fused", {"cache_bits": 8, "cache_quant_mode": "fused"})):
        kw = dict(cache_bits=None, cache_length_pattern="tile", cache_strategy_pattern="tile", feed_long_prompts=False, global_tokens=4,
                  recent_window=10, attn_thresholding=False, min_recovery_frac=0.9)
        kw.update(base)
        kw.update(extra)
        setup_caches(model, _Tok(), dev, 400, kw)
        with torch.no_grad():
            tok, probs = prefill(model, prompt.view(1, -1), torch.arange(300, device=dev))
            pos = torch.tensor([300], dtype=torch.int32, device=dev)
            plist, toks = [probs.float().clone()], [int(tok)]
            cur = tok.view(1, 1).to(torch.int32)
            step = GraphedDecoder(model)
            for i in range(16):
                nt, pr = step(model, cur, pos)
                plist.append(pr.float().clone())
                toks.append(int(nt))
                # teacher-force the unquantised run's tokens: both runs see the same inputs
                cur = (nt if name == "bf16" else torch.tensor(runs["bf16"][0][len(toks) - 1], device=dev)).view(1, 1).to(torch.int32)
                pos += 1
        torch.cuda.synchronize()
        kv = model.layers[0].attention.kv_cache
        runs[name] = (toks, plist, kv.memory_usage(), kv)
    assert torch.equal(runs["bf16"][1][0], runs["fused"][1][0])  # prefill attends to the prompt's own k / v: identical
    worst = max(float((a - b).abs().max() / a.abs().max()) for a, b in zip(runs["bf16"][1], runs["fused"][1]))
    agree = sum(int(a == b) for a, b in zip(runs["bf16"][0], runs["fused"][0]))
    assert worst < 0.2 and agree >= len(runs["bf16"][0]) - 2, (worst, agree)
    kv = runs["fused"][3]
    H, S = kv.n_heads, kv.max_cache_length
    saved = 2 * H * S * D * 2 - 2 * H * S * D - 16 * H * S
    assert (runs["bf16"][2] - runs["fused"][2]) * 1024 ** 3 >= saved - 1
    assert kv.fused_quant and kv.k_cache.numel() == 0 and kv.step_status(cfg["n_head"]) == 0
    if strategy == "hybrid":
        assert kv.supports_fused_step() and kv.cache_strategies is not None
