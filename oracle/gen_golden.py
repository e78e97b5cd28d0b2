#!/usr/bin/env python3
"""Generate golden vectors by IMPORTING THE REFERENCE (AnswerDotAI/cold-compress) on CPU.

Runs only in the build container where /root/reference exists; nothing from the reference is copied —
only inputs and the outputs the reference computed for them are written, as small .npz/.json fixtures
under tests/golden/.  The GPU box never sees the reference.

    PYTHONDONTWRITEBYTECODE=1 python oracle/gen_golden.py [--out tests/golden]
    ... --seed_offset N [--jitter_shapes] --out SOME_OTHER_DIR     (r5) the same families from other seeds (and shapes): fresh vectors
        for differential runs (tools/fuzz_fresh_seeds.sh; CC_GOLDEN_DIR=DIR pytest ...); offset 0 without jitter = the committed files

Fixtures:
  f1_e2e_<strategy>.npz   tiny-Llama end-to-end runs through generation_utils.generate
  f1_generate_branches.npz  generate()'s own branches (feed_long_prompts, prompt == cache length, decode_first_token, teacher forcing,
                          terminator ids), the hybrid cache through generate(), per-layer strategy / length plumbing, keep_it_odd
  f2_hh_<dtype>.npz       KVCacheHeavyHitter replay trace (update_kv / update_state, as model.py:389-427)
  f2_hh_query_bf16.npz    the same policy driven from q through the reference's scaled_dot_product_attention + group mean
  f3_l2_<case>.npz        KVCacheL2 replay traces (bf16 rounding ties, unfilled slots, H == 1)
  f4_random.npz           KVCacheRandom with captured torch.rand vectors
  f4_headconst.npz        KVCacheFull / KVCacheRecentGlobal / KVCacheKeepItOdd decode traces
  f5_compress.npz         prompt_compression.* priorities -> keep_idxs (+ boundary-tie flags)
  f7_attn_<dtype>.npz     attention_utils.scaled_dot_product_attention decode + small prefill
  f7_attn_gqa_<dtype>.npz the same at 7 and 3 query heads per kv head (bf16, fp16)
  f2_hh_query_r7_bf16.npz f2_hh_query at 7 query heads per kv head (H = 4, HQ = 28)
  f8_budgets.json         generation_utils budget arithmetic
  f8_budgets_random.json  the same arithmetic on 1000 random inputs (value, or the exception's type name)
  f8_setup_random.json    setup_caches on 80 random configurations: normalised keyword lists and per-layer cache / compressor classes
  f9_quant_*.npz          --cache_bits: quantize/dequantize known answers, quantised heavy-hitter / recent-global replays
                          (the K/V attention sees at every step + the final int8 / packed images), one end-to-end run
Low-precision tensors are stored as their uint16 bit patterns with a "<name>__dtype" tag.
"""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"

SEED_OFFSET = 0  # --seed_offset: every seed below is shifted by it (0 = the committed fixtures; tools/fuzz_fresh_seeds.sh uses others)


JITTER = False  # --jitter_shapes: the cache replays (f2 / f3 / f4 / f9) also move their lengths, windows and step counts with the offset


def _jitter(S, T_prefill, steps, g, w, seed):
    """Shapes of a replay case shifted by a draw that depends on (offset, seed): cache length, prefill length (a case that starts
    from a full cache stays full), protected globals / recent window (kept below the cache length), step count."""
    if not JITTER:
        return S, T_prefill, steps, g, w
    import random

    r = random.Random(1000003 * SEED_OFFSET + int(seed))
    S2 = max(12, S + r.randint(-4, 12))
    g2 = max(0, g + r.randint(-1, 2))
    w2 = max(1, w + r.randint(-2, 3))
    while g2 + w2 > S2 - 4:
        w2, g2 = max(1, w2 - 1), max(0, g2 - 1)
    T2 = S2 if T_prefill >= S else min(S2, max(1, T_prefill + r.randint(-6, 6)))
    return S2, T2, steps + r.randint(0, 12), g2, w2


def _gen(seed):
    return torch.Generator().manual_seed(int(seed) + SEED_OFFSET)


def _seed(seed):
    return torch.manual_seed(int(seed) + SEED_OFFSET)



def _import_reference():
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF)
    tk = types.ModuleType("tiktoken")
    tk.Encoding = object
    tl = types.ModuleType("tiktoken.load")
    tl.load_tiktoken_bpe = lambda p: {}
    tk.load = tl
    sys.modules["tiktoken"] = tk
    sys.modules["tiktoken.load"] = tl
    import attention_utils as A  # noqa
    import cache as C  # noqa
    import generation_utils as G  # noqa
    import model as M  # noqa
    import prompt_compression as P  # noqa

    return A, C, G, M, P


def pack(d):
    """torch tensors -> numpy; bf16/f16 as uint16 bit patterns + dtype tag."""
    out = {}
    for k, v in d.items():
        if torch.is_tensor(v):
            if v.dtype in (torch.bfloat16, torch.float16):
                out[k] = v.contiguous().view(torch.int16).numpy().view(np.uint16)
                out[k + "__dtype"] = np.array("bf16" if v.dtype == torch.bfloat16 else "f16")
            else:
                out[k] = v.contiguous().numpy()
        else:
            out[k] = np.asarray(v)
    return out


# ------------------------------------------------------------------------------------------------ F1


class FakeTok:
    def special_ids(self):
        return [[1], [2, 3]]

    def punctuation_ids(self):
        return [5, 6, 7]


TINY = dict(block_size=256, vocab_size=128, n_layer=2, n_head=4, n_local_heads=2, dim=64, intermediate_size=128)


def run_e2e(C, G, M, name, cache_args, prompt_len=40, new_tokens=12, seed=0, n_layer=2):
    shift = 0
    if JITTER and name != "recent_global":  # --jitter_shapes: prompt length, number of new tokens and the prompt's token pattern move
        import random  # (the weights move with the seed; BASELINE config C1 — recent_global, 40 -> 12 tokens — keeps its lengths)

        r = random.Random(1000003 * SEED_OFFSET + 31 * prompt_len + new_tokens + n_layer)
        prompt_len = max(17, prompt_len + r.randint(-6, 10))
        new_tokens = new_tokens + r.randint(0, 8)
        shift = r.randint(0, 127)
    _seed(seed)
    cfg = dict(TINY)
    cfg["n_layer"] = n_layer
    model = M.Transformer(M.ModelArgs(**cfg)).to(torch.float32).eval()
    state = {k: v.clone() for k, v in model.state_dict().items()}
    parser = argparse.ArgumentParser()
    C.add_cache_arguments(parser)
    G.add_generation_arguments(parser)
    args = parser.parse_args([])
    kw = vars(args)
    kw.update(cache_args)
    cache_kwargs = G.setup_caches(model, FakeTok(), "cpu", prompt_len + new_tokens, dict(kw))

    evict_log = []  # (layer, idx tensor)
    for li, layer in enumerate(model.layers):
        kv = layer.attention.kv_cache
        orig = kv._eviction_idx

        def wrapped(input_pos, _orig=orig, _li=li):
            r = _orig(input_pos)
            evict_log.append((_li, r.clone().view(-1)))
            return r

        kv._eviction_idx = wrapped
    logits_log = []
    orig_fwd = model.forward

    def fwd(*a, **k):
        out = orig_fwd(*a, **k)
        logits_log.append(out[0, -1].detach().clone().float())
        return out

    model.forward = fwd
    prompt = ((torch.arange(prompt_len) * 7 + shift) % 128).to(torch.int32) if name != "recent_global" else (
        (torch.arange(prompt_len) + shift) % 128).to(torch.int32)
    seq, probs, stats = G.generate(model, prompt, G.prefill, G.decode_one_token, max_new_tokens=new_tokens)
    d = {"prompt": prompt, "seq": seq, "logits": torch.stack(logits_log),
         "n_layer": n_layer, "prompt_len": prompt_len, "new_tokens": new_tokens,
         "max_cache_length": np.array(cache_kwargs["max_cache_length"]),
         "recent_window": np.array(cache_kwargs["recent_window"]),
         "cache_args_json": json.dumps({k: v for k, v in cache_args.items()}),
         "torch_version": torch.__version__}
    for k, v in state.items():
        d["sd." + k] = v
    H = TINY["n_local_heads"]
    for li in range(n_layer):
        rows = [r for (l, r) in evict_log if l == li]
        width = max(r.numel() for r in rows) if rows else 1
        d[f"evict_idx_L{li}"] = torch.stack([r.expand(width) if r.numel() == 1 else r for r in rows]) if rows else torch.zeros(0, 1)
        kv = model.layers[li].attention.kv_cache
        d[f"final_pos_L{li}"] = kv.pos.clone()
        d[f"final_mask_L{li}"] = kv.mask.clone()
        d[f"final_cts_L{li}"] = kv.cache_cts.clone()
        d[f"final_k_L{li}"] = kv.k_cache.clone()
        if hasattr(kv, "attn_history_num"):
            d[f"final_num_L{li}"] = kv.attn_history_num.clone()
            d[f"final_denom_L{li}"] = kv.attn_history_denom.clone()
        if hasattr(kv, "key_norm"):
            d[f"final_keynorm_L{li}"] = kv.key_norm.clone()
        if getattr(kv, "quantize", False):
            d[f"final_v_L{li}"] = kv.v_cache.clone()
            d[f"final_k_scales_L{li}"] = kv.k_scales.clone()
            d[f"final_k_zero_points_L{li}"] = kv.k_zero_points.clone()
            d[f"final_v_scales_L{li}"] = kv.v_scales.clone()
            d[f"final_v_zero_points_L{li}"] = kv.v_zero_points.clone()
    cs = model.get_cache_stats(prompt_len, new_tokens)
    d["compression_ratio_avg"] = cs["compression_ratio_avg"]
    return pack(d)


def generate_cases(C, G, M):
    """generation_utils.generate's own branches (ref: generation_utils.py:399-531), which the F1 runs do not reach: a long prompt
    fed token by token behind the prefill (feed_long_prompts), a prompt exactly as long as the smallest cache (split by one),
    decode_first_token, teacher forcing (next_tokens), early stop on a terminator id.  One tiny model; per case the prompt, the
    generate() keywords, the returned sequence, the token counts of its stats and every layer's final positions."""
    import random

    r = random.Random(1000003 * SEED_OFFSET + 97)
    j = (lambda lo, hi: r.randint(lo, hi)) if JITTER else (lambda lo, hi: 0)
    _seed(7)
    model = M.Transformer(M.ModelArgs(**dict(TINY))).to(torch.float32).eval()
    out = {"sd." + k: v.clone() for k, v in model.state_dict().items()}
    hh = dict(cache_strategy=["heavy_hitter"], prompt_compression_strategy=["heavy_hitter"], max_cache_length=[32], global_tokens=4,
              recent_window=4)
    rg = dict(cache_strategy=["recent_global"], prompt_compression_strategy=["recent_global"], max_cache_length=[16], global_tokens=4)
    cases = [("feed_long", hh, 56 + j(-5, 9), 10 + j(0, 5), dict(feed_long_prompts=True)),
             ("prompt_equals_cache", rg, 16, 9 + j(0, 5), dict()),
             # (heavy_hitter, not l2: l2 evicts keys of EQUAL norm — repeated tokens — in an order that follows vector_norm's unspecified
             #  summation order, and a jittered set showed the kept sets drifting apart behind such a tie; the branch is the point here)
             ("decode_first", hh, 48 + j(-5, 9), 8 + j(0, 5), dict(decode_first_token=True)),
             ("teacher_forced", hh, 44 + j(-5, 9), 0, dict(next_tokens=[(11 * i + 3 + j(0, 50)) % 128 for i in range(9 + j(0, 4))])),
             ("terminator", hh, 40 + j(-5, 9), 14 + j(0, 4), dict(terminator_ids="@step5"))]
    # the FastGen hybrid cache THROUGH generate() (cache_configs/hybrid.yaml, fastgen.yaml): prefill profiling from the harness's own
    # attention, the token ids reaching the cache, per-head policies at decode time (the f6 fixtures drive the class directly)
    for hname, strategies, frac in (("hybrid", HYBRID_YAML, 0.5), ("fastgen", FASTGEN_YAML, 0.6)):
        hy = dict(cache_strategy=["hybrid"], prompt_compression_strategy=["full"], max_cache_length=[1.0], global_tokens=4,
                  hybrid_strategies=strategies, min_recovery_frac=round(frac + (r.uniform(-0.1, 0.1) if JITTER else 0.0), 3))
        cases.append((hname, hy, 52 + j(-5, 9), 20 + j(0, 6), dict()))
    # per-layer plumbing: different strategies, a fractional and an absolute cache length, a fractional recent window on the two layers
    # (ref: generation_utils.py:324-388 setup_caches, model.py:191-233), and the toy keep_it_odd policy end to end
    cases.append(("mixed_layers", dict(cache_strategy=["recent_global", "heavy_hitter"], prompt_compression_strategy=["recent_global", "heavy_hitter"],
                                       max_cache_length=[0.25, 32], global_tokens=3, recent_window=0.2), 50 + j(-5, 9), 14 + j(0, 5), dict()))
    # (debug_* through setup_caches cannot be captured: the reference raises in KVCacheAnalysis.__init__ — 'no attribute cache_bits',
    #  cache.py:181 reached before the attribute exists; the f10 fixtures drive the class directly)
    # the quantised KV cache through generate() at 4 and 2 bits (8 bits: f9_e2e_heavy_hitter_q8.npz)
    for nb in (4, 2):
        cases.append((f"heavy_hitter_q{nb}", dict(cache_strategy=["heavy_hitter"], prompt_compression_strategy=["heavy_hitter"], max_cache_length=[32],
                                                  global_tokens=4, recent_window=4, cache_bits=nb), 50 + j(-5, 9), 12 + j(0, 5), dict()))
    cases.append(("keep_it_odd", dict(cache_strategy=["keep_it_odd"], prompt_compression_strategy=["keep_it_odd"], max_cache_length=[24],
                                      global_tokens=4), 45 + j(-5, 9), 10 + j(0, 5), dict()))
    names = []
    for name, cache_args, prompt_len, new_tokens, gk in cases:
        parser = argparse.ArgumentParser()
        C.add_cache_arguments(parser)
        G.add_generation_arguments(parser)
        kw = vars(parser.parse_args([]))
        kw.update(cache_args)
        total = prompt_len + max(new_tokens, len(gk.get("next_tokens", []))) + 2
        prompt = ((torch.arange(prompt_len) * 5 + 2 + j(0, 100)) % 128).to(torch.int32)
        if name in ("hybrid", "fastgen"):  # special ids [1], [2, 3] and punctuation 5, 6, 7 (FakeTok) where the policies look for them
            prompt = prompt.clamp(min=8)
            prompt[0], prompt[10], prompt[11], prompt[20], prompt[33], prompt[40] = 1, 2, 3, 5, 6, 7

        after_prefill = []

        def run(gkw):
            G.setup_caches(model, FakeTok(), "cpu", total, dict(kw))
            g2 = dict(gkw)
            if "next_tokens" in g2:
                g2["next_tokens"] = torch.tensor(g2["next_tokens"], dtype=torch.int32)
            del after_prefill[:]

            def pf(m, x, input_pos, **k2):  # (positions every layer holds when the prefill returns)
                r_ = G.prefill(m, x, input_pos, **k2)
                after_prefill.append([l.attention.kv_cache.pos.clone() for l in m.layers])
                return r_

            return G.generate(model, prompt, pf, G.decode_one_token, max_new_tokens=new_tokens, **g2)

        if gk.get("terminator_ids") == "@step5":  # a token the greedy run really produces: found by a run without terminators
            seq0, _, _ = run({})
            gk = dict(terminator_ids=[int(seq0[prompt_len + 5])])
        seq, probs, stats = run(gk)
        out[name + ".prompt"] = prompt
        out[name + ".seq"] = seq.clone()
        out[name + ".cache_args_json"] = np.array(json.dumps(cache_args))
        out[name + ".gen_kwargs_json"] = np.array(json.dumps(gk))
        out[name + ".new_tokens"] = np.array(new_tokens)
        out[name + ".total"] = np.array(total)
        out[name + ".prefill_tokens"] = np.array(int(stats["prefill_tokens"]))
        out[name + ".decode_tokens"] = np.array(int(stats["decode_tokens"]))
        out[name + ".n_probs"] = np.array(len(probs))
        cs = model.get_cache_stats(prompt_len, new_tokens)  # (ref: model.py get_cache_stats -> KVCache.compute_statistics, cache.py:255-281)
        out[name + ".cache_stats_json"] = np.array(json.dumps({k: float(v) for k, v in cs.items()}))
        for li, layer in enumerate(model.layers):
            out[f"{name}.final_pos_L{li}"] = layer.attention.kv_cache.pos.clone()
            out[f"{name}.pos_after_prefill_L{li}"] = after_prefill[0][li]
            if hasattr(layer.attention.kv_cache, "cache_strategies"):
                out[f"{name}.cache_strategies_L{li}"] = layer.attention.kv_cache.cache_strategies.clone()
                out[f"{name}.final_cts_L{li}"] = layer.attention.kv_cache.cache_cts.clone()
        names.append(name)
    out["cases"] = np.array(names)
    return pack(out)


# ------------------------------------------------------------------------------------------------ F2/F3/F4


def softmax_rows(shape, dtype, gen, mask=None):
    x = torch.randn(shape, generator=gen) * 2.0
    if mask is not None:
        x = x.masked_fill(~mask, float("-inf"))
    return torch.softmax(x, dim=-1).to(dtype)


def replay_cache(C, strategy, dtype, H, S, D, T_prefill, steps, g, w, seed, extra=None, rand_capture=None, capture_kv=False):
    """Drive a reference cache exactly as model.py:389-427 does and record inputs/outputs."""
    S, T_prefill, steps, g, w = _jitter(S, T_prefill, steps, g, w, seed)
    gen = _gen(seed)
    cls, rk = C.get_cache_constructor(strategy)
    kw = dict(max_cache_length=S, global_tokens=g, max_seq_length=4 * S, cache_bits=None, recent_window=w,
              history_window_size=1, attn_thresholding=False)
    if extra:
        kw.update(extra)
    kv = cls(1, H, D, dtype, **{k: kw[k] for k in rk})
    rec = {"H": H, "S": S, "D": D, "T_prefill": T_prefill, "steps": steps, "g": g, "w": w,
           "strategy": np.array(strategy), "dtype": np.array(str(dtype).split(".")[-1])}
    # ---- prefill (no compression: T <= S)
    T = T_prefill
    k0 = (torch.randn(1, H, T, D, generator=gen)).to(dtype)
    v0 = (torch.randn(1, H, T, D, generator=gen)).to(dtype)
    pos0 = torch.arange(T)
    kv.update_kv(pos0, k0, v0, True)
    attn0 = None
    if kv.return_attn():
        causal = torch.tril(torch.ones(T, T, dtype=torch.bool)).view(1, 1, T, T)
        attn0 = softmax_rows((1, H, T, T), dtype, gen, causal.expand(1, H, T, T))
    kv.update_state(pos0, k0, v0, True, attn0)
    rec.update({"k0": k0, "v0": v0})
    if attn0 is not None:
        rec["attn0"] = attn0
        rec["num_after_prefill"] = kv.attn_history_num.clone()
        rec["denom_after_prefill"] = kv.attn_history_denom.clone()
    if hasattr(kv, "key_norm"):
        rec["keynorm_after_prefill"] = kv.key_norm.clone()
    # ---- decode
    ks, vs, attns, idxs, rands, cts = [], [], [], [], [], []
    for t in range(steps):
        p = torch.tensor([T + t], dtype=torch.int32)
        k1 = torch.randn(1, H, 1, D, generator=gen).to(dtype)
        v1 = torch.randn(1, H, 1, D, generator=gen).to(dtype)
        pos_before = kv.pos.clone()
        if rand_capture is not None:
            r = torch.rand(S, generator=gen)
            rands.append(r)
            rand_capture["next"] = r
        ret = kv.update_kv(p, k1, v1, False, input_ids=torch.tensor([[1]]))
        if capture_kv:  # what attention sees this step (quantised caches: the dequantised tensors, cache.py:333-338)
            rec.setdefault("_k_ret", []).append(ret[0].clone())
            rec.setdefault("_v_ret", []).append(ret[1].clone())
        changed = (kv.pos != pos_before)
        # idx per pos-head = the slot whose pos changed (pos always changes: p is new)
        idx = changed.squeeze(0).int().argmax(dim=-1)
        assert bool(changed.squeeze(0).sum(dim=-1).eq(1).all())
        idxs.append(idx.clone().long())
        cts.append(kv.cache_cts.clone())
        a = None
        if kv.return_attn():
            a = softmax_rows((1, H, 1, S), dtype, gen, kv.mask.clone())
            attns.append(a)
        kv.update_state(p, k1, v1, False, a)
        ks.append(k1)
        vs.append(v1)
    rec.update({"k_new": torch.stack(ks), "v_new": torch.stack(vs), "idx": torch.stack(idxs),
                "cache_cts_steps": torch.stack(cts)})
    if attns:
        rec["attn"] = torch.stack(attns)
        rec["final_num"] = kv.attn_history_num.clone()
        rec["final_denom"] = kv.attn_history_denom.clone()
        rec["final_counter"] = kv.attn_counter.clone()
    if rands:
        rec["rand_u"] = torch.stack(rands)
    if hasattr(kv, "key_norm"):
        rec["final_keynorm"] = kv.key_norm.clone()
    rec.update({"final_pos": kv.pos.clone(), "final_mask": kv.mask.clone(), "final_cts": kv.cache_cts.clone(),
                "final_k": kv.k_cache.clone(), "final_v": kv.v_cache.clone()})
    if capture_kv:
        rec["k_ret"] = torch.stack(rec.pop("_k_ret"))
        rec["v_ret"] = torch.stack(rec.pop("_v_ret"))
    if getattr(kv, "quantize", False):
        rec.update({"k_scales": kv.k_scales.clone(), "v_scales": kv.v_scales.clone(), "k_zero_points": kv.k_zero_points.clone(),
                    "v_zero_points": kv.v_zero_points.clone(), "cache_bits": kv.n_bit})
    return pack(rec)


def hh_query_case(A, C, dtype, seed, H=2, R=4, S=256, D=128, T_prefill=236, steps=160, g=4, w=10):
    """Heavy-hitter decode driven from the QUERY, exactly as Attention.forward does (model.py:389-427): update_kv ->
    repeat_interleave -> attention_utils.scaled_dot_product_attention(return_attn=True) -> mean over the group ->
    update_state.  Unlike the f2_hh_* traces (which carry ready-made attention rows) this one lets the reference's own attention
    produce the probabilities the history accumulates: what a fused decode step (insert + attention + history in one pass) must
    reproduce.  Records q / k / v per step, the evicted slot, the reference's eviction SCORES (the tensor its arg-min saw,
    cache.py:738-751: for the near-tie rule), its attention output and group-mean probabilities."""
    gen = _gen(seed)
    HQ = H * R
    cls, rk = C.get_cache_constructor("heavy_hitter")
    kw = dict(max_cache_length=S, global_tokens=g, max_seq_length=4 * S, cache_bits=None, recent_window=w,
              history_window_size=1, attn_thresholding=False)
    kv = cls(1, H, D, dtype, **{k: kw[k] for k in rk})
    T = T_prefill
    k0 = torch.randn(1, H, T, D, generator=gen).to(dtype)
    v0 = torch.randn(1, H, T, D, generator=gen).to(dtype)
    pos0 = torch.arange(T)
    kv.update_kv(pos0, k0, v0, True)
    causal = torch.tril(torch.ones(T, T, dtype=torch.bool)).view(1, 1, T, T)
    attn0 = softmax_rows((1, H, T, T), dtype, gen, causal.expand(1, H, T, T))
    kv.update_state(pos0, k0, v0, True, attn0)
    rec = {"H": H, "R": R, "S": S, "D": D, "T_prefill": T, "steps": steps, "g": g, "w": w,
           "dtype": np.array(str(dtype).split(".")[-1]),
           "k_after_prefill": kv.k_cache.clone(), "v_after_prefill": kv.v_cache.clone(), "pos_after_prefill": kv.pos.clone(),
           "mask_after_prefill": kv.mask.clone(), "cts_after_prefill": kv.cache_cts.clone(),
           "num_after_prefill": kv.attn_history_num.clone(), "denom_after_prefill": kv.attn_history_denom.clone(),
           "counter_after_prefill": kv.attn_counter.clone()}
    qs, ks, vs, idxs, scores, ys, attns = [], [], [], [], [], [], []
    orig_argmin = torch.Tensor.argmin
    cap = {}

    def spy(self, *a, **k):  # the tensor KVCacheHeavyHitter._eviction_idx takes its arg-min of (cache.py:751)
        if self.dtype == torch.float32 and self.shape == (1, H, S):
            cap["scores"] = self.clone()
        return orig_argmin(self, *a, **k)

    for t in range(steps):
        p = torch.tensor([T + t], dtype=torch.int32)
        # a few kv rows are made "sticky" through a shared direction so that real heavy hitters exist
        q1 = torch.randn(1, HQ, 1, D, generator=gen).to(dtype)
        k1 = torch.randn(1, H, 1, D, generator=gen).to(dtype)
        v1 = torch.randn(1, H, 1, D, generator=gen).to(dtype)
        pos_before = kv.pos.clone()
        torch.Tensor.argmin = spy
        try:
            k, v, kv_mask = kv.update_kv(p, k1, v1, False, input_ids=torch.tensor([[1]]))
        finally:
            torch.Tensor.argmin = orig_argmin
        changed = (kv.pos != pos_before).squeeze(0)
        assert bool(changed.sum(dim=-1).eq(1).all())
        idxs.append(changed.int().argmax(dim=-1).long())
        scores.append(cap.pop("scores")[0])
        kv_mask = kv_mask.repeat_interleave(R, dim=1)  # model.py:395-400
        k_rep = k.repeat_interleave(R, dim=1)
        v_rep = v.repeat_interleave(R, dim=1)
        y, attn = A.scaled_dot_product_attention(q1, k_rep, v_rep, attn_mask=kv_mask, dropout_p=0.0, attn_top_k=1.0,
                                                 return_attn=kv.return_attn())
        attn = attn.view(1, H, R, 1, -1).mean(dim=2)  # model.py:413-418
        kv.update_state(p, k, v, False, attn, input_ids=torch.tensor([[1]]))
        qs.append(q1)
        ks.append(k1)
        vs.append(v1)
        ys.append(y.clone())
        attns.append(attn.clone())
    rec.update({"q": torch.stack(qs), "k_new": torch.stack(ks), "v_new": torch.stack(vs), "idx": torch.stack(idxs),
                "scores": torch.stack(scores), "y": torch.stack(ys), "attn": torch.stack(attns),
                "final_num": kv.attn_history_num.clone(), "final_denom": kv.attn_history_denom.clone(),
                "final_counter": kv.attn_counter.clone(), "final_pos": kv.pos.clone(), "final_mask": kv.mask.clone(),
                "final_cts": kv.cache_cts.clone(), "final_k": kv.k_cache.clone(), "final_v": kv.v_cache.clone(),
                "torch_version": np.array(torch.__version__)})
    return pack(rec)


# ------------------------------------------------------------------------------------------------ F9 (quantised KV)


def quant_cases():
    """quantization_utils.quantize_tensor / dequantize_tensor with axis = 2 on [1, H, S, D] tensors: known answers."""
    import quantization_utils as Q

    gen = _gen(23)
    out = {}
    H, S, D = 3, 40, 16
    for dt, tag in ((torch.float32, "f32"), (torch.bfloat16, "bf16"), (torch.float16, "f16")):
        x = (torch.randn(1, H, S, D, generator=gen) * 1.7).to(dt)
        x[:, :, 5] = 0  # an empty slot (range 0 -> the 1e-6 floor)
        x[:, :, 6] = 0.75  # a constant slot
        x[:, :, 7] *= 1e-4  # tiny range
        x[:, :, 8] *= 300.0  # large range
        out[f"x_{tag}"] = x
        for nb in (8, 4, 2):
            q, sc, zp = Q.quantize_tensor(x, n_bit=nb, axis=2)
            y = Q.dequantize_tensor(q, sc, zp, x.shape, n_bit=nb, axis=2)
            out[f"q_{tag}_{nb}"] = q.contiguous().view(torch.uint8) if q.dtype == torch.int8 else q
            out[f"scales_{tag}_{nb}"] = sc
            out[f"zeros_{tag}_{nb}"] = zp
            out[f"y_{tag}_{nb}"] = y.contiguous()
    return pack(out)


# ------------------------------------------------------------------------------------------------ F5


def compress_cases(P):
    gen = _gen(11)
    out = {}
    cases = []

    def boundary_tie(prio, K):
        # True if the K-th largest value equals the (K+1)-th largest in any row
        s = prio.float().sort(dim=-1, descending=True).values
        return bool((s[..., K - 1] == s[..., K]).any()) if prio.shape[-1] > K else False

    def add(name, comp, input_pos, k, v, **kw):
        _seed(5)  # the random compressor draws randperm per call: same draw for both calls
        prio = comp._token_importances(input_pos, k, v, **kw)
        # NB: the heavy-hitter compressor mutates nothing we re-use; call the full path too
        _seed(5)
        keep, k2, v2, st = comp(input_pos, k, v, **kw)
        out[name + ".priority"] = prio.clone()
        out[name + ".keep"] = keep.clone()
        out[name + ".k_in"] = k
        out[name + ".v_in"] = v
        out[name + ".k_out"] = k2
        out[name + ".v_out"] = v2
        out[name + ".tie"] = np.array(boundary_tie(prio, comp.max_cache_length))
        if st is not None:
            out[name + ".state"] = st
        cases.append(name)

    H, L, D, S = 4, 96, 16, 40
    if JITTER:  # --jitter_shapes: prompt length and kept length move (the protected 4 + 10 tokens stay: the tests read them as constants)
        import random

        r = random.Random(1000003 * SEED_OFFSET + 11)
        L, S = r.randint(70, 150), r.randint(24, 64)
    pos = torch.arange(L)
    for dt, tag in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
        k = torch.randn(1, H, L, D, generator=gen).to(dt)
        v = torch.randn(1, H, L, D, generator=gen).to(dt)
        kw = dict(max_cache_length=S, global_tokens=4, recent_window=10)
        add(f"recent_global_{tag}", P.PromptCompressorRecentGlobal(head_specific=False, **kw), pos, k, v)
        add(f"l2_{tag}", P.PromptCompressorL2(head_specific=True, **kw), pos, k, v)
        causal = torch.tril(torch.ones(L, L, dtype=torch.bool)).view(1, 1, L, L).expand(1, H, L, L)
        attn = softmax_rows((1, H, L, L), dt, gen, causal)
        out[f"heavy_hitter_{tag}.attn"] = attn
        add(f"heavy_hitter_{tag}", P.PromptCompressorHeavyHitter(head_specific=True, **kw), pos, k, v, attn=attn)
        # random: capture the permutation through the priority itself (priority is an input of the check)
        _seed(5)
        add(f"random_{tag}", P.PromptCompressorRandom(head_specific=False, **kw), pos, k, v)
        add(f"keep_it_odd_{tag}", P.PromptCompressorKeepItOdd(head_specific=False, **kw), pos, k, v)
    # a larger bf16 L2 case where boundary ties are near-certain
    H, L, D, S = 2, 2048, 32, 640
    k = torch.randn(1, H, L, D, generator=gen).to(torch.bfloat16)
    v = torch.randn(1, H, L, D, generator=gen).to(torch.bfloat16)
    add("l2_big_bf16", P.PromptCompressorL2(head_specific=True, max_cache_length=S, global_tokens=4, recent_window=10),
        torch.arange(L), k, v)
    out["cases"] = np.array(cases)
    return pack(out)


# ------------------------------------------------------------------------------------------------ F7


def attn_cases(A, dtype):
    gen = _gen(3)
    out = {}
    # decode: HQ=8, H=2 (R=4), S=96, D=32, with mask; driven as model.py:395-418
    HQ, H, S, D = 8, 2, 96, 32
    jr = None
    if JITTER:  # --jitter_shapes: the decode cache lengths and the prefill length move
        import random

        jr = random.Random(1000003 * SEED_OFFSET + 3 + (0 if dtype == torch.float32 else 1))
        S = jr.randint(40, 160)
    R = HQ // H
    q = torch.randn(1, HQ, 1, D, generator=gen).to(dtype)
    k = torch.randn(1, H, S, D, generator=gen).to(dtype)
    v = torch.randn(1, H, S, D, generator=gen).to(dtype)
    mask = torch.rand(1, H, 1, S, generator=gen) > 0.2
    mask[..., 0] = True
    y, p = A.scaled_dot_product_attention(q, k.repeat_interleave(R, 1), v.repeat_interleave(R, 1),
                                          attn_mask=mask.repeat_interleave(R, 1), return_attn=True)
    y2, _ = A.scaled_dot_product_attention(q, k.repeat_interleave(R, 1), v.repeat_interleave(R, 1),
                                           attn_mask=mask.repeat_interleave(R, 1), return_attn=False)
    out.update({"dec.q": q, "dec.k": k, "dec.v": v, "dec.mask": mask, "dec.y": y, "dec.probs": p, "dec.y_fused": y2,
                "dec.attn_gm": p.view(1, H, R, 1, -1).mean(dim=2)})
    # decode, Llama-3-8B head geometry but short cache: HQ=32,H=8,D=128,S=256
    HQ, H, S, D = 32, 8, 256, 128
    if jr is not None:
        S = jr.randint(203, 420)
    R = HQ // H
    q = torch.randn(1, HQ, 1, D, generator=gen).to(dtype)
    k = torch.randn(1, H, S, D, generator=gen).to(dtype)
    v = torch.randn(1, H, S, D, generator=gen).to(dtype)
    mask = torch.ones(1, H, 1, S, dtype=torch.bool)
    mask[..., 200:] = False
    y, p = A.scaled_dot_product_attention(q, k.repeat_interleave(R, 1), v.repeat_interleave(R, 1),
                                          attn_mask=mask.repeat_interleave(R, 1), return_attn=True)
    out.update({"dec8b.q": q, "dec8b.k": k, "dec8b.v": v, "dec8b.mask": mask, "dec8b.y": y, "dec8b.probs": p,
                "dec8b.attn_gm": p.view(1, H, R, 1, -1).mean(dim=2)})
    # prefill: HQ=4,H=2,L=48,D=16, causal
    HQ, H, L, D = 4, 2, 48, 16
    if jr is not None:
        L = jr.randint(17, 90)
    R = HQ // H
    q = torch.randn(1, HQ, L, D, generator=gen).to(dtype)
    k = torch.randn(1, H, L, D, generator=gen).to(dtype)
    v = torch.randn(1, H, L, D, generator=gen).to(dtype)
    causal = torch.tril(torch.ones(L, L, dtype=torch.bool)).view(1, 1, L, L)
    y, p = A.scaled_dot_product_attention(q, k.repeat_interleave(R, 1), v.repeat_interleave(R, 1),
                                          attn_mask=causal, return_attn=True)
    gm = p.view(1, H, R, L, -1).mean(dim=2)
    out.update({"pre.q": q, "pre.k": k, "pre.v": v, "pre.y": y, "pre.attn_gm": gm,
                "pre.colsum": gm.sum(dim=2), "pre.obs_mean": gm[:, :, -16:, :].mean(dim=2)})
    return pack(out)


def attn_gqa_cases(A, dtype):
    """attention_utils.scaled_dot_product_attention at query-group ratios other than 4, driven as model.py:395-418
    (repeat_interleave, masked decode, causal prefill, mean over the group): r7 = Qwen2's 7 query heads per kv head
    (H = 4, D = 128), r3 = 3 per kv head (H = 2, D = 64)."""
    gen = _gen(401 if dtype == torch.bfloat16 else 402)
    out = {}
    for tag, H, R, D, S, L in (("r7", 4, 7, 128, 77, 20), ("r3", 2, 3, 64, 150, 40)):
        HQ = H * R
        q = torch.randn(1, HQ, 1, D, generator=gen).to(dtype)
        k = torch.randn(1, H, S, D, generator=gen).to(dtype)
        v = torch.randn(1, H, S, D, generator=gen).to(dtype)
        mask = torch.rand(1, H, 1, S, generator=gen) > 0.3
        mask[..., -1] = True
        y, p = A.scaled_dot_product_attention(q, k.repeat_interleave(R, 1), v.repeat_interleave(R, 1),
                                              attn_mask=mask.repeat_interleave(R, 1), return_attn=True)
        out.update({f"{tag}.dec.q": q, f"{tag}.dec.k": k, f"{tag}.dec.v": v, f"{tag}.dec.mask": mask, f"{tag}.dec.y": y,
                    f"{tag}.dec.probs": p, f"{tag}.dec.attn_gm": p.view(1, H, R, 1, -1).mean(dim=2)})
        q = torch.randn(1, HQ, L, D, generator=gen).to(dtype)
        k = torch.randn(1, H, L, D, generator=gen).to(dtype)
        v = torch.randn(1, H, L, D, generator=gen).to(dtype)
        causal = torch.tril(torch.ones(L, L, dtype=torch.bool)).view(1, 1, L, L)
        y, p = A.scaled_dot_product_attention(q, k.repeat_interleave(R, 1), v.repeat_interleave(R, 1),
                                              attn_mask=causal, return_attn=True)
        gm = p.view(1, H, R, L, -1).mean(dim=2)
        out.update({f"{tag}.pre.q": q, f"{tag}.pre.k": k, f"{tag}.pre.v": v, f"{tag}.pre.y": y, f"{tag}.pre.attn_gm": gm,
                    f"{tag}.pre.colsum": gm.sum(dim=2), f"{tag}.pre.obs_mean": gm[:, :, -16:, :].mean(dim=2)})
    return pack(out)


def attn_topk_case(A):
    """attention_utils.py:24-26, 45-50: top-k decode attention (L == 1, NO mask — with a mask the reference asserts)."""
    gen = _gen(9)
    H, S, D = 4, 64, 16
    q = torch.randn(1, H, 1, D, generator=gen)
    k = torch.randn(1, H, S, D, generator=gen)
    v = torch.randn(1, H, S, D, generator=gen)
    out = {"q": q, "k": k, "v": v}
    for frac in (0.25, 0.5):
        y, p = A.scaled_dot_product_attention(q, k, v, attn_mask=None, return_attn=True, attn_top_k=frac)
        out[f"y_{int(frac * 100)}"] = y
        out[f"p_{int(frac * 100)}"] = p
    try:
        A.scaled_dot_product_attention(q, k, v, attn_mask=torch.ones(1, H, 1, S, dtype=torch.bool), return_attn=True, attn_top_k=0.5)
        out["mask_asserts"] = np.array(False)
    except AssertionError:
        out["mask_asserts"] = np.array(True)
    return pack(out)


# ------------------------------------------------------------------------------------------------ F8


def budgets_random(G, M):
    """normalize_cache_length, apply_pyramid_pattern, apply_pattern and find_multiple on random inputs: [case, answer] pairs."""
    import contextlib
    import io
    import random

    rng = random.Random(20260928 + SEED_OFFSET)
    cases = []
    for _ in range(400):
        mx = rng.choice([52, 77, 1000, 4096, 8192, 10240, 18432, 34816, rng.randint(16, 40000)])
        v = rng.choice([round(rng.uniform(0.01, 1.0), rng.choice([1, 2, 3])), 1, rng.randint(2, 2 * mx), float(rng.randint(2, mx))])
        cases.append(["normalize", [v, mx]])
    for _ in range(300):
        mx = rng.choice([4096, 10240, 18432, 34816])
        n = rng.choice([2, 4, 8, 16, 32, 80, rng.randint(2, 64)])
        cases.append(["pyramid", [rng.choice([64, 256, 300, 512, 1024, 2560, 3488, rng.randint(32, mx // 2)]), mx, n, rng.random() < 0.7]])
    for _ in range(200):
        pat = [rng.choice([128, 512, 1024, "a", 0.5]) for _ in range(rng.choice([1, 1, 2, 4]))]
        n = rng.choice([4, 8, 16, 32, 6])
        cases.append(["pattern", [pat, n, rng.choice(["tile", "repeat", "pyramid", "funnel"]), rng.choice([4096, 18432])]])
    for _ in range(100):
        cases.append(["find_multiple", [rng.randint(0, 5000), rng.choice([1, 8, 16, 256])]])
    out = []
    for fn, args in cases:
        f = {"normalize": G.normalize_cache_length, "pyramid": lambda a, b, c, d: G.apply_pyramid_pattern(a, b, c, decreasing=d),
             "pattern": lambda p, n, s, m: G.apply_pattern(p, n, s, m), "find_multiple": M.find_multiple}[fn]
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                want = f(*args)
        except Exception as e:
            want = type(e).__name__
        out.append([[fn, args], want])
    return json.loads(json.dumps(out))  # (tuples as lists, as the test reads them back)


def setup_random(C, G, M):
    """setup_caches (generation_utils.py:324-388, model.py:191-233) on random configurations: [[n_layer, max_seq, kwargs], answer]
    pairs; the answer is the normalised keyword lists and per layer the cache class, its length, buffer shape, window, sinks and
    the prompt compressor's class, or the exception's type name."""
    import contextlib
    import io
    import random

    rng = random.Random(777 + SEED_OFFSET)
    pairs = [("recent_global", "recent_global"), ("heavy_hitter", "heavy_hitter"), ("l2", "l2"), ("full", "full"), ("random", "random"),
             ("keep_it_odd", "keep_it_odd"), ("recent_global", "l2"), ("l2", "recent_global")]
    cases = []
    for _ in range(80):
        n_layer = rng.choice([2, 4, 8])
        max_seq = rng.choice([96, 200, 256, 1000])
        k = rng.choice([1, 1, 2])
        strat = [rng.choice(pairs) for _ in range(k)]
        lengths = [rng.choice([0.25, 0.5, 0.1, 1.0, 16, 32, 64, 24, 40]) for _ in range(rng.choice([1, 1, 2]))]
        pat = rng.choice(["tile", "repeat", "tile", "repeat", "pyramid", "funnel"])
        kw = dict(cache_strategy=[a for a, _ in strat], prompt_compression_strategy=[b for _, b in strat], max_cache_length=lengths,
                  cache_length_pattern=pat, cache_strategy_pattern=rng.choice(["tile", "repeat"]), global_tokens=rng.choice([1, 4, 4, 8, 30]),
                  recent_window=rng.choice([10, 4, 0.1, 0.5, 1, 100]))
        if "full" in kw["cache_strategy"]:
            kw["max_cache_length"] = [1.0]
        cases.append([n_layer, max_seq, kw])
    out = []
    for n_layer, max_seq, kw in cases:
        cfg = dict(TINY)
        cfg["n_layer"] = n_layer
        cfg["block_size"] = max(256, max_seq)
        model = M.Transformer(M.ModelArgs(**cfg)).to(torch.float32).eval()
        parser = argparse.ArgumentParser()
        C.add_cache_arguments(parser)
        G.add_generation_arguments(parser)
        ck = vars(parser.parse_args([]))
        ck.update(kw)
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                r = G.setup_caches(model, FakeTok(), "cpu", max_seq, dict(ck))
            layers = [[type(l.attention.kv_cache).__name__, int(l.attention.kv_cache.max_cache_length), list(l.attention.kv_cache.pos.shape),
                       int(getattr(l.attention.kv_cache, "recent_window", -1)), int(getattr(l.attention.kv_cache, "global_tokens", -1)),
                       type(l.attention.prompt_compressor).__name__] for l in model.layers]
            want = {"max_cache_length": list(r["max_cache_length"]), "recent_window": list(r["recent_window"]),
                    "cache_strategy": list(r["cache_strategy"]), "prompt_compression_strategy": list(r["prompt_compression_strategy"]),
                    "layers": layers}
        except Exception as e:
            want = type(e).__name__
        out.append([[n_layer, max_seq, kw], want])
    return json.loads(json.dumps(out))


def budgets(G, M, C=None):
    rows = {"normalize": [], "pattern": [], "pyramid": [], "find_multiple": []}
    if C is not None:  # registry surface: relevant_kwargs per strategy + argparse defaults (cache.py:13-118, 1444-1478)
        rows["relevant_kwargs"] = {s: C.get_cache_constructor(s)[1] for s in
                                   ["full", "random", "recent_global", "heavy_hitter", "l2", "hybrid", "keep_it_odd",
                                    "debug_heavy_hitter"]}
        ap = argparse.ArgumentParser()
        C.add_cache_arguments(ap)
        rows["arg_defaults"] = {k: v for k, v in vars(ap.parse_args([])).items()}
        rw = []
        for rwin, lens in [(10, [2560] * 4), (0.5, [100, 7, 1]), (1, [8, 16]), (4000, [2036, 256])]:
            if rwin <= 1:
                rw.append([rwin, lens, [max(1, int(rwin * l)) for l in lens]])
            else:
                rw.append([rwin, lens, [max(1, min(rwin, l)) for l in lens]])
        rows["recent_window"] = rw
    for frac, mx in [(0.25, 10240), (0.1, 34816), (1.0, 18432), (0.5, 52), (4096, 10240), (16, 52), (0.33, 1000),
                     (20000, 10240), (0.05, 8192), (1, 77)]:
        rows["normalize"].append([frac, mx, G.normalize_cache_length(frac, mx)])
    for pat, n, strat in [([1, 2], 4, "tile"), ([1, 2], 4, "repeat"), (["a"], 3, "tile"), ([5, 6, 7, 8], 8, "repeat"),
                          ([5, 6, 7, 8], 8, "tile")]:
        rows["pattern"].append([pat, n, strat, G.apply_pattern(pat, n, strat)])
    for length, mx, n, dec in [(1024, 18432, 32, True), (1024, 18432, 32, False), (2560, 10240, 32, True),
                               (512, 4096, 16, True), (300, 4096, 8, True), (3488, 34816, 80, True)]:
        rows["pyramid"].append([length, mx, n, dec, G.apply_pyramid_pattern(length, mx, n, decreasing=dec)])
    for n, k in [(5, 8), (8, 8), (2557, 8), (0, 8), (13, 256)]:
        rows["find_multiple"].append([n, k, M.find_multiple(n, k)])
    return rows


# ------------------------------------------------------------------------------------------------ F6


HYBRID_YAML = [  # cache_configs/hybrid.yaml of the reference
    {"strategy": "window", "recent_window": 0.1},
    {"strategy": "window_heavy_hitter", "heavy_hitter_frac": 0.25, "recent_window": 0.1},
    {"strategy": "window_heavy_hitter", "heavy_hitter_frac": 0.5, "recent_window": 0.1},
    {"strategy": "full"},
]
FASTGEN_YAML = [  # cache_configs/fastgen.yaml of the reference
    {"strategy": "special"},
    {"strategy": "special_punc"},
    {"strategy": "special_punc_heavy_hitter", "heavy_hitter_frac": 0.3},
    {"strategy": "special_punc_heavy_hitter_window", "recent_window": 0.3, "heavy_hitter_frac": 0.3},
    {"strategy": "full"},
]


def hybrid_case(C, dtype, strategies, min_recovery, seed, H=4, L=48, S=96, D=16, steps=40, peaky=1.5):
    """KVCacheHybrid driven as model.py:389-427 does: prefill (update_kv, then update_state with the [1,H,L,L]
    attention -> profile_and_update) and `steps` decode steps."""
    if JITTER:  # --jitter_shapes: prompt length (the planted special / punctuation ids need L >= 41), step count, recovery threshold
        import random  # and the second head's peakiness move with (offset, seed)

        r = random.Random(1000003 * SEED_OFFSET + int(seed) + 7)
        if L + steps <= S:  # (a head on the `full` policy must never outgrow the cache: cache.py:277 asserts; the 450-step case, whose
            L = min(S - 8, max(42, L + r.randint(-6, 12)))  # recovery threshold selects no `full` head, keeps its lengths)
            steps = min(steps + r.randint(0, 16), S - 1 - L)
        min_recovery = round(min(0.97, max(0.15, min_recovery + r.uniform(-0.08, 0.08))), 3)
        peaky = peaky * r.uniform(0.7, 1.4)
    gen = _gen(seed)
    token_ids = {"special": [[1], [2, 3]], "punctuation": [5, 6, 7]}
    kv = C.KVCacheHybrid(1, H, D, dtype, max_cache_length=S, max_seq_length=S, cache_bits=None, global_tokens=4,
                         token_ids=token_ids, min_recovery_frac=min_recovery, hybrid_strategies=strategies)
    ids = torch.randint(8, 64, (1, L), generator=gen)
    ids[0, 0] = 1
    ids[0, 10], ids[0, 11] = 2, 3
    ids[0, 20] = 5
    ids[0, 33] = 6
    ids[0, 40] = 7
    k0 = torch.randn(1, H, L, D, generator=gen).to(dtype)
    v0 = torch.randn(1, H, L, D, generator=gen).to(dtype)
    causal = torch.tril(torch.ones(L, L, dtype=torch.bool)).view(1, 1, L, L).expand(1, H, L, L)
    # heads of different "peakiness" so that different policies get selected
    x = torch.randn(1, H, L, L, generator=gen) * torch.tensor([0.3, peaky, 3.0, 6.0][:H]).view(1, H, 1, 1)
    x[:, :, :, :4] += 2.0
    attn0 = torch.softmax(x.masked_fill(~causal, float("-inf")), -1).to(dtype)
    pos0 = torch.arange(L)
    kv.update_kv(pos0, k0, v0, True, input_ids=ids)
    # capture the partition order the reference's (non-stable) argsort produced
    cap = {}
    orig_argsort = torch.Tensor.argsort

    def spy(self, *a, **k):
        r = orig_argsort(self, *a, **k)
        if self.dtype == torch.int32 and self.ndim == 2 and self.shape == (H, L):
            cap["order"] = r.clone()
        return r

    torch.Tensor.argsort = spy
    try:
        kv.update_state(pos0, k0, v0, True, attn0, input_ids=ids)
    finally:
        torch.Tensor.argsort = orig_argsort
    rec = {"H": H, "L": L, "S": S, "D": D, "steps": steps, "min_recovery_frac": min_recovery,
           "strategies_json": json.dumps(strategies), "dtype": np.array(str(dtype).split(".")[-1]),
           "ids": ids, "k0": k0, "v0": v0, "attn0": attn0, "order": cap["order"],
           "cache_strategies": kv.cache_strategies.clone(), "cts_after_prefill": kv.cache_cts.clone(),
           "pos_after_prefill": kv.pos.clone(), "mask_after_prefill": kv.mask.clone(),
           "num_after_prefill": kv.attn_history_num.clone(), "denom_after_prefill": kv.attn_history_denom.clone(),
           "k_after_prefill": kv.k_cache.clone(), "requires_hh": int(kv.requires_heavy_hitter),
           "num_special": kv.num_special.clone().view(-1) if hasattr(kv, "num_special") else torch.zeros(1),
           "num_punc": kv.num_punc.clone().view(-1) if hasattr(kv, "num_punc") else torch.zeros(1)}
    if hasattr(kv, "special_mask"):
        rec["special_mask_after_prefill"] = kv.special_mask.clone()
    if hasattr(kv, "punc_mask"):
        rec["punc_mask_after_prefill"] = kv.punc_mask.clone()
    ks, vs, attns, toks, fills, cts = [], [], [], [], [], []
    orig_fill = kv._fill

    def fill_spy(input_pos, k_val, v_val, fill_idxs, **kw):
        fills.append(fill_idxs.clone())
        return orig_fill(input_pos, k_val, v_val, fill_idxs, **kw)

    kv._fill = fill_spy
    for t in range(steps):
        p = torch.tensor([L + t], dtype=torch.int32)
        tok = torch.randint(8, 64, (1, 1), generator=gen)
        if t in (5, 17, 18):
            tok[0, 0] = 6  # punctuation tokens arriving at decode time
        k1 = torch.randn(1, H, 1, D, generator=gen).to(dtype)
        v1 = torch.randn(1, H, 1, D, generator=gen).to(dtype)
        kv.update_kv(p, k1, v1, False, input_ids=tok)
        a = None
        if kv.return_attn():
            a = softmax_rows((1, H, 1, S), dtype, gen, kv.mask.clone())
            attns.append(a)
        kv.update_state(p, k1, v1, False, a, input_ids=tok)
        ks.append(k1)
        vs.append(v1)
        toks.append(tok.view(-1))
        cts.append(kv.cache_cts.clone())
    rec.update({"k_new": torch.stack(ks), "v_new": torch.stack(vs), "tok": torch.stack(toks),
                "fill": torch.stack(fills), "cts_steps": torch.stack(cts), "final_pos": kv.pos.clone(),
                "final_mask": kv.mask.clone(), "final_cts": kv.cache_cts.clone(), "final_num": kv.attn_history_num.clone(),
                "final_denom": kv.attn_history_denom.clone(), "final_k": kv.k_cache.clone()})
    if attns:
        rec["attn"] = torch.stack(attns)
    if hasattr(kv, "punc_mask"):
        rec["final_punc_mask"] = kv.punc_mask.clone()
        rec["final_num_punc"] = kv.num_punc.clone().view(-1)
    st = kv.compute_statistics(torch.tensor(L + steps))
    rec["stats_json"] = json.dumps({k: float(v) for k, v in st.items()})
    return pack(rec)


# ------------------------------------------------------------------------------------------------ F10


def analysis_case(C, dtype, seed, H=2, D=16, S=24, S_full=96, L=40, steps=24, g=2, w=3):
    """KVCacheAnalysis (`debug_heavy_hitter`, cache.py:1291-1420): a full cache with a shadow compressed cache and the
    attention-loss metric, driven as model.py:389-427 does (the shadow cache is larger than the SnapKV observation window
    plus the sinks, so that real priorities — not a 16-way tie at 1.0 — decide part of the keep set).  At this commit the class cannot be constructed — its
    `full_kwargs` (cache.py:1319-1324) omits `cache_bits`, which KVCache.__init__ reads (cache.py:181) — so the fixture pins
    the INTENDED behaviour: the one missing keyword is injected (cache_bits=None for the full cache) by wrapping
    KVCacheFull.__init__ for the duration of the capture; nothing else of the reference is altered."""
    gen = _gen(seed)
    orig_init = C.KVCacheFull.__init__

    def patched(self, *a, **k):
        k.setdefault("cache_bits", None)
        return orig_init(self, *a, **k)

    C.KVCacheFull.__init__ = patched
    try:
        cls, rk = C.get_cache_constructor("debug_heavy_hitter")
        kw = dict(max_cache_length=S, global_tokens=g, max_seq_length=S_full, cache_bits=None, recent_window=w,
                  history_window_size=1, attn_thresholding=False, prompt_compression_strategy="heavy_hitter")
        kv = cls(1, H, D, dtype, **{k: kw[k] for k in rk})
    finally:
        C.KVCacheFull.__init__ = orig_init
    rec = {"H": H, "D": D, "S": S, "S_full": S_full, "L": L, "steps": steps, "g": g, "w": w,
           "dtype": np.array(str(dtype).split(".")[-1]), "relevant_kwargs_json": json.dumps(rk)}
    k0 = torch.randn(1, H, L, D, generator=gen).to(dtype)
    v0 = torch.randn(1, H, L, D, generator=gen).to(dtype)
    pos0 = torch.arange(L)
    causal = torch.tril(torch.ones(L, L, dtype=torch.bool)).view(1, 1, L, L)
    attn0 = softmax_rows((1, H, L, L), dtype, gen, causal.expand(1, H, L, L))
    kv.update_kv(pos0, k0, v0, True)
    kv.update_state(pos0, k0, v0, True, attn0)
    rec.update({"k0": k0, "v0": v0, "attn0": attn0, "comp_pos_after_prefill": kv.compressed.pos.clone(),
                "comp_num_after_prefill": kv.compressed.attn_history_num.clone(), "full_pos_after_prefill": kv.pos.clone()})
    ks, vs, attns, comp_pos, losses = [], [], [], [], []
    for t in range(steps):
        p = torch.tensor([L + t], dtype=torch.int32)
        k1 = torch.randn(1, H, 1, D, generator=gen).to(dtype)
        v1 = torch.randn(1, H, 1, D, generator=gen).to(dtype)
        kc, vc, m = kv.update_kv(p, k1, v1, False)
        a = softmax_rows((1, H, 1, S_full), dtype, gen, m.clone())  # attention over the FULL cache (group mean already taken)
        kv.update_state(p, k1, v1, False, a)
        ks.append(k1)
        vs.append(v1)
        attns.append(a)
        comp_pos.append(kv.compressed.pos.clone())
        losses.append(kv.attention_losses[t].clone())
    st = kv.compute_statistics(torch.tensor(L + steps))
    rec.update({"k_new": torch.stack(ks), "v_new": torch.stack(vs), "attn": torch.stack(attns), "comp_pos_steps": torch.stack(comp_pos),
                "loss_steps": torch.stack(losses), "final_full_pos": kv.pos.clone(), "final_comp_num": kv.compressed.attn_history_num.clone(),
                "final_comp_denom": kv.compressed.attn_history_denom.clone(), "final_comp_k": kv.compressed.k_cache.clone(),
                "loss_ctr": kv.attention_loss_ctr.clone(), "stats_json": json.dumps({k: float(v) for k, v in st.items()})})
    return pack(rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(__file__), "..", "tests", "golden"))
    ap.add_argument("--only", default=None, help="generate only one fixture family (e.g. f6)")
    ap.add_argument("--seed_offset", type=int, default=0, help="shift every seed (0 = the committed fixtures): fresh reference-made "
                    "vectors for the same cases, written wherever --out says — never into tests/golden")
    ap.add_argument("--jitter_shapes", action="store_true", help="with --seed_offset: the cache replays also move their cache length, "
                    "prefill length, protected windows and step counts (a draw per case)")
    a = ap.parse_args()
    global SEED_OFFSET, JITTER
    SEED_OFFSET = a.seed_offset
    JITTER = bool(a.jitter_shapes)
    os.makedirs(a.out, exist_ok=True)
    A, C, G, M, P = _import_reference()
    torch.set_num_threads(1)

    def save(name, d):
        np.savez_compressed(os.path.join(a.out, name), **d)
        print("wrote", name, sum(v.nbytes for v in d.values()) // 1024, "KiB")

    # F2q: heavy hitter driven from the query through the reference's own attention (what the fused decode step replays)
    if a.only in (None, "f2q"):
        save("f2_hh_query_bf16.npz", hh_query_case(A, C, torch.bfloat16, seed=201))
        if a.only == "f2q":
            return

    # F10: debug_* (KVCacheAnalysis): shadow compressed cache + attention-loss metric, intended behaviour
    if a.only in (None, "f10"):
        save("f10_analysis_hh_f32.npz", analysis_case(C, torch.float32, seed=71))
        save("f10_analysis_hh_bf16.npz", analysis_case(C, torch.bfloat16, seed=72, steps=40))
        if a.only == "f10":
            return

    # F6: hybrid (FastGen) prefill profiling + decode traces
    if a.only in (None, "f6"):
        save("f6_hybrid_f32.npz", hybrid_case(C, torch.float32, HYBRID_YAML, 0.9, seed=61))
        save("f6_hybrid_bf16.npz", hybrid_case(C, torch.bfloat16, HYBRID_YAML, 0.55, seed=62, steps=60))
        save("f6_hybrid_mixed_f32.npz", hybrid_case(C, torch.float32, HYBRID_YAML, 0.45, seed=64, steps=60, peaky=0.8))
        save("f6_fastgen_f32.npz", hybrid_case(C, torch.float32, FASTGEN_YAML, 0.7, seed=63))
        # 450 decode steps: the hybrid cache's fixed 400-entry history ring wraps around (bf16 window sums)
        save("f6_hybrid_long_bf16.npz", hybrid_case(C, torch.bfloat16, HYBRID_YAML, 0.55, seed=65, steps=450))
        if a.only == "f6":
            return

    # F2w: heavy hitter with a finite history window (ScissorHands m) and with binary thresholded history
    if a.only in (None, "f2w"):
        save("f2_hh_w8_f32.npz", replay_cache(C, "heavy_hitter", torch.float32, H=4, S=48, D=16, T_prefill=30, steps=80, g=2,
                                              w=3, seed=23, extra={"history_window_size": 8}))
        save("f2_hh_w8_bf16.npz", replay_cache(C, "heavy_hitter", torch.bfloat16, H=4, S=48, D=16, T_prefill=30, steps=80, g=2,
                                               w=3, seed=24, extra={"history_window_size": 8}))
        # a long trace (400 decode steps, the 33-entry ring wraps 12 times, full cache from the start): pins the "exact sum
        # rounded once" definition of the window sums against torch's own bf16 `.sum(dim=-1)` over many evictions
        save("f2_hh_w33_long_bf16.npz", replay_cache(C, "heavy_hitter", torch.bfloat16, H=3, S=64, D=16, T_prefill=64, steps=400,
                                                     g=3, w=5, seed=102, extra={"history_window_size": 33}))
        # attn_thresholding=True cannot be captured: the reference itself raises at cache.py:721
        # ("Index put requires the source and destination dtypes match, got Bool ... and Int") on torch 2.10.
        if a.only == "f2w":
            return

    if a.only in (None, "f8r"):
        for name, rows in (("f8_budgets_random.json", budgets_random(G, M)), ("f8_setup_random.json", setup_random(C, G, M))):
            with open(os.path.join(a.out, name), "w") as f:
                json.dump(rows, f, separators=(",", ":"))
            print("wrote", name)
        if a.only == "f8r":
            return

    if a.only in (None, "f7k"):
        save("f7_attn_topk_f32.npz", attn_topk_case(A))
        if a.only == "f7k":
            return

    if a.only in (None, "f9"):
        save("f9_quant_known_answers.npz", quant_cases())
        for dt, tag in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
            for nb in (8, 4, 2):
                save(f"f9_quant_hh_{tag}_{nb}.npz", replay_cache(C, "heavy_hitter", dt, H=3, S=24, D=16, T_prefill=17, steps=20, g=2,
                                                                w=3, seed=31 + nb, extra=dict(cache_bits=nb), capture_kv=True))
        # 120 steps from a full cache: every slot is round-tripped 120 times by the reference — the device's exact skipping
        # of slots the round trip no longer changes has to stay invisible at every step
        for nb, seed in ((8, 301), (4, 302)):
            save(f"f9_quant_hh_long_bf16_{nb}.npz", replay_cache(C, "heavy_hitter", torch.bfloat16, H=3, S=40, D=16, T_prefill=40, steps=120,
                                                                 g=2, w=3, seed=seed, extra=dict(cache_bits=nb), capture_kv=True))
        save("f9_quant_recent_global_f32_8.npz", replay_cache(C, "recent_global", torch.float32, H=2, S=16, D=8, T_prefill=16, steps=12,
                                                              g=4, w=3, seed=5, extra=dict(cache_bits=8), capture_kv=True))
        save("f9_e2e_heavy_hitter_q8.npz", run_e2e(C, G, M, "heavy_hitter", dict(
            cache_strategy=["heavy_hitter"], prompt_compression_strategy=["heavy_hitter"], max_cache_length=[32],
            global_tokens=4, recent_window=4, cache_bits=8), prompt_len=56, new_tokens=24))
        if a.only == "f9":
            return

    if a.only == "gqa":
        gqa_fixtures(A, C, save)
        return
    # F1: config C1 (README.md:103 of the reference) + companions on the same tiny model
    save("f1_e2e_recent_global.npz", run_e2e(C, G, M, "recent_global", dict(
        cache_strategy=["recent_global"], prompt_compression_strategy=["recent_global"], max_cache_length=[16],
        global_tokens=4)))
    save("f1_e2e_heavy_hitter.npz", run_e2e(C, G, M, "heavy_hitter", dict(
        cache_strategy=["heavy_hitter"], prompt_compression_strategy=["heavy_hitter"], max_cache_length=[32],
        global_tokens=4, recent_window=4), prompt_len=56, new_tokens=24))
    save("f1_e2e_heavy_hitter_short.npz", run_e2e(C, G, M, "heavy_hitter", dict(
        cache_strategy=["heavy_hitter"], prompt_compression_strategy=["heavy_hitter"], max_cache_length=[32],
        global_tokens=2, recent_window=3), prompt_len=20, new_tokens=30))
    save("f1_e2e_l2.npz", run_e2e(C, G, M, "l2", dict(
        cache_strategy=["l2"], prompt_compression_strategy=["l2"], max_cache_length=[24], global_tokens=4,
        recent_window=5), prompt_len=48, new_tokens=16))
    save("f1_e2e_full.npz", run_e2e(C, G, M, "full", dict(
        cache_strategy=["full"], prompt_compression_strategy=["full"], max_cache_length=[1.0]),
        prompt_len=24, new_tokens=10))
    save("f1_e2e_hh_pyramid.npz", run_e2e(C, G, M, "heavy_hitter", dict(
        cache_strategy=["heavy_hitter"], prompt_compression_strategy=["heavy_hitter"], max_cache_length=[64],
        cache_length_pattern="pyramid", global_tokens=2, recent_window=3), prompt_len=120, new_tokens=16, n_layer=4))

    save("f1_generate_branches.npz", generate_cases(C, G, M))

    # F2: heavy-hitter replay
    for dt, tag in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
        save(f"f2_hh_{tag}.npz", replay_cache(C, "heavy_hitter", dt, H=4, S=48, D=16, T_prefill=30, steps=80, g=2, w=3,
                                              seed=21))
    save("f2_hh_h1_bf16.npz", replay_cache(C, "heavy_hitter", torch.bfloat16, H=2, S=130, D=128, T_prefill=100, steps=70,
                                           g=4, w=10, seed=22))
    # F3: L2
    # long traces at the model's head_dim (300 decode steps from a full cache): rare rounding cases get their chance
    save("f2_hh_long_bf16.npz", replay_cache(C, "heavy_hitter", torch.bfloat16, H=2, S=256, D=128, T_prefill=256, steps=300, g=4,
                                             w=10, seed=201))
    save("f3_l2_long_bf16.npz", replay_cache(C, "l2", torch.bfloat16, H=2, S=300, D=128, T_prefill=300, steps=300, g=4, w=10,
                                             seed=202))
    save("f3_l2_bf16.npz", replay_cache(C, "l2", torch.bfloat16, H=4, S=48, D=16, T_prefill=30, steps=80, g=2, w=3, seed=31))
    save("f3_l2_f32.npz", replay_cache(C, "l2", torch.float32, H=4, S=48, D=16, T_prefill=30, steps=60, g=2, w=3, seed=32))
    save("f3_l2_h1_bf16.npz", replay_cache(C, "l2", torch.bfloat16, H=1, S=200, D=128, T_prefill=150, steps=120, g=4, w=10,
                                           seed=33))
    # F4: random with captured rand vectors
    cap = {}
    orig_rand = torch.rand

    def patched_rand(*args, **kw):
        if "generator" in kw or "next" not in cap:
            return orig_rand(*args, **kw)
        return cap["next"].clone()

    torch.rand = patched_rand
    try:
        save("f4_random.npz", replay_cache(C, "random", torch.bfloat16, H=3, S=40, D=16, T_prefill=25, steps=60, g=2, w=4,
                                           seed=41, rand_capture=cap))
    finally:
        torch.rand = orig_rand
    d = {}
    for strat in ("full", "recent_global", "keep_it_odd"):
        S = 64 if strat == "full" else 24
        r = replay_cache(C, strat, torch.bfloat16, H=3, S=S, D=16, T_prefill=12, steps=40, g=3, w=4, seed=42)
        for k, v in r.items():
            d[f"{strat}.{k}"] = v
    save("f4_headconst.npz", d)
    # F5
    save("f5_compress.npz", compress_cases(P))
    # F7
    save("f7_attn_f32.npz", attn_cases(A, torch.float32))
    save("f7_attn_bf16.npz", attn_cases(A, torch.bfloat16))
    # F8
    with open(os.path.join(a.out, "f8_budgets.json"), "w") as f:
        json.dump(budgets(G, M, C), f)
    print("wrote f8_budgets.json")
    if a.only in (None, "gqa"):
        gqa_fixtures(A, C, save)


def gqa_fixtures(A, C, save):
    """Query-group ratios other than 4 (written last: the families above keep their draws)."""
    save("f7_attn_gqa_bf16.npz", attn_gqa_cases(A, torch.bfloat16))
    save("f7_attn_gqa_f16.npz", attn_gqa_cases(A, torch.float16))
    # Qwen2's 7 query heads per kv head, four kv heads; a shorter cache and trace than f2_hh_query_bf16 keep the file small
    save("f2_hh_query_r7_bf16.npz", hh_query_case(A, C, torch.bfloat16, seed=203, H=4, R=7, S=96, T_prefill=88, steps=28))


if __name__ == "__main__":
    main()
