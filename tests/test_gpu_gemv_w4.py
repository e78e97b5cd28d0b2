"""cc_gemv_fused_w4 (int4 group-wise weight-only decode GEMV) against an fp32 torch composition of the contract
(include/coldcompress.h: p = in . ((q - 8) * s + z) with the weight in fp32, t = bf16(p), + bias -> bf16; SwiGLU rounds each t
before silu; RoPE on the rounded t): every fused form at the Llama-3-8B decode shapes, the LM head, the 70B and C5-rank shapes, at
G = 32 and 128 (64 and 256 at three shapes), plus a seeded fuzz.  Tolerance: 2 ulp of bf16 relative to the largest output.  Also:
h_out bit-identical to cc_gemv_fused's, run-to-run and graph-replay bit identity, refused shapes write
nothing, and int4 harness models decoding through the fused GEMVs (eager and hipGraph) against the module formula per layer."""
import argparse
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ULP = {torch.bfloat16: 2 ** -8}
BF = torch.bfloat16


def _rnd(t):
    return t.to(BF).float()


def _quant(N, K, G, gen, scale=0.02):
    """-> (packed uint8 [N, K / 2], per-row bf16 (scale, zero) [N, K / G, 2], fp32 dequantised weight [N, K])."""
    from cold_compress_amd.harness.quantize import dequantize_int4, group_quantize_int4, pack_int4

    w = (torch.randn(N, K, generator=gen, device=DEV) * scale).to(BF)
    q, s, z = group_quantize_int4(w, G)
    packed = pack_int4(q).contiguous()
    sz = torch.stack([s, z], -1).contiguous()
    return packed, sz, dequantize_int4(packed, sz, G)


def _ref(wd, x, wd3=None, delta=None, nw=None, eps=1e-5, bias=None, freqs=None, rope_rows=0, hd=0):
    xf = x.float()
    h = None
    if nw is not None:
        h = _rnd(xf + delta.float()) if delta is not None else xf
        n = _rnd(h * torch.rsqrt((h * h).mean() + eps))
        xin = _rnd(n * nw.float())
    else:
        xin = xf
    t = _rnd(wd @ xin)
    if bias is not None:
        t = _rnd(t + bias.float())
    if wd3 is not None:
        t3 = _rnd(wd3 @ xin)
        t = _rnd(_rnd(torch.nn.functional.silu(t)) * t3)
    if freqs is not None:
        f = freqs.float().view(-1, 2)
        rr = t[:rope_rows].view(-1, hd // 2, 2)
        c, sn = f[:, 0].view(1, -1), f[:, 1].view(1, -1)
        out = torch.stack([rr[..., 0] * c - rr[..., 1] * sn, rr[..., 1] * c + rr[..., 0] * sn], -1).reshape(-1)
        t = torch.cat([_rnd(out), t[rope_rows:]])
    return t, h


def _inputs(N, K, G, seed, norm=False, delta=False, swiglu=False, rope=None, bias=False):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    q, sz, wd = _quant(N, K, G, gen)
    a = dict(q=q, sz=sz, wd=wd, G=G, x=torch.randn(K, generator=gen, device=DEV).to(BF))
    if swiglu:
        q3, sz3, wd3 = _quant(N, K, G, gen)
        a.update(q3=q3, sz3=sz3, wd3=wd3)
    if norm:
        a["nw"] = (1 + 0.1 * torch.randn(K, generator=gen, device=DEV)).to(BF)
        if delta:
            a["delta"] = torch.randn(K, generator=gen, device=DEV).to(BF)
    if bias:
        a["bias"] = (0.1 * torch.randn(N, generator=gen, device=DEV)).to(BF)
    if rope:
        rows, hd = rope
        ang = torch.rand(hd // 2, generator=gen, device=DEV) * 6.28
        a.update(freqs=torch.stack([ang.cos(), ang.sin()], -1).to(BF), rope_rows=rows, hd=hd)
    return a


def _run(a, h_out=None):
    from cold_compress_amd.harness import glue

    return glue.gemv_fused(a["q"], a["x"], w3=a.get("q3"), delta=a.get("delta"), norm_weight=a.get("nw"), h_out=h_out, bias=a.get("bias"),
                           freqs=a.get("freqs"), rope_rows=a.get("rope_rows", 0), head_dim=a.get("hd", 0), scales=a["sz"],
                           scales3=a.get("sz3"), groupsize=a["G"])


def _check(a, what):
    K = a["q"].shape[1] * 2
    h_out = torch.empty(K, dtype=BF, device=DEV) if a.get("nw") is not None else None
    y = _run(a, h_out)
    torch.cuda.synchronize()
    ref, h = _ref(a["wd"], a["x"], a.get("wd3"), a.get("delta"), a.get("nw"), bias=a.get("bias"), freqs=a.get("freqs"),
                  rope_rows=a.get("rope_rows", 0), hd=a.get("hd", 0))
    assert y.dtype == BF and torch.isfinite(y).all(), what
    err = (y.float() - ref).abs().max().item()
    tol = 2 * ULP[BF] * ref.abs().max().item()
    assert err <= tol, f"{what}: max err {err:.3g} > {tol:.3g}"
    if h is not None:
        assert torch.equal(h_out.float(), h), f"{what}: h_out"
    return y


CASES = [
    ("wqkv_rope_norm", 6144, 4096, dict(norm=True, delta=True, rope=(5120, 128))), ("wo", 4096, 4096, {}),
    ("w13_norm", 14336, 4096, dict(norm=True, delta=True, swiglu=True)), ("w2", 4096, 14336, {}),
    ("lm_head_norm", 128256, 4096, dict(norm=True, delta=True)),
    ("qwen_wqkv_bias", 4608, 3584, dict(norm=True, delta=True, rope=(4096, 128), bias=True)),
    ("small_rope_bias", 96, 256, dict(norm=True, rope=(64, 16), bias=True)), ("ragged", 1031, 1024, dict(norm=True)),
    ("ragged_pair", 77, 256, dict(swiglu=True, norm=True, delta=True)),
    ("70b_wqkv", 10240, 8192, dict(norm=True, delta=True, rope=(9216, 128))), ("70b_wo", 8192, 8192, {}),
    ("70b_w13", 28672, 8192, dict(norm=True, delta=True, swiglu=True)), ("70b_w2", 8192, 28672, {}),
    ("c5_rank_wqkv", 1280, 8192, dict(norm=True, delta=True, rope=(1152, 128))), ("c5_rank_wo", 8192, 1024, {}),
    ("c5_rank_w13", 3584, 8192, dict(norm=True, delta=True, swiglu=True)), ("c5_rank_w2", 8192, 3584, {}),
]


@pytest.mark.parametrize("G", [32, 128])
@pytest.mark.parametrize("name,N,K,opt", CASES, ids=[c[0] for c in CASES])
def test_gemv_w4_matches_contract(name, N, K, opt, G):
    _check(_inputs(N, K, G, seed=sum(map(ord, name)) + G, **opt), f"{name} G={G}")


@pytest.mark.parametrize("G", [64, 256])
@pytest.mark.parametrize("name,N,K,opt", [CASES[0], CASES[2], CASES[3]], ids=[CASES[i][0] for i in (0, 2, 3)])
def test_gemv_w4_other_groupsizes(name, N, K, opt, G):
    _check(_inputs(N, K, G, seed=sum(map(ord, name)) + G, **opt), f"{name} G={G}")


def test_gemv_w4_fuzz():
    """40 seeded cases over shapes, groupsizes and options (K a multiple of G, up to 16384)."""
    rng = np.random.default_rng(2025)
    for i in range(40):
        G = int(rng.choice([32, 64, 128, 256]))
        K = G * int(rng.integers(1, 16384 // G + 1))
        N = int(rng.integers(1, 3000))
        swiglu = bool(rng.integers(0, 3) == 0)
        norm = bool(rng.integers(0, 2))
        opt = dict(norm=norm, delta=norm and bool(rng.integers(0, 2)), swiglu=swiglu)
        if not swiglu:
            opt["bias"] = bool(rng.integers(0, 3) == 0)
            hd = int(rng.choice([2, 8, 64, 128]))
            if rng.integers(0, 3) == 0 and N >= hd:
                opt["rope"] = (hd * int(rng.integers(1, N // hd + 1)), hd)
        _check(_inputs(N, K, G, seed=2000 + i, **opt), f"fuzz {i}: N={N} K={K} G={G} {opt}")


@pytest.mark.parametrize("K,delta", [(4096, True), (8192, False), (1024, True), (28672, True)])
def test_h_out_bit_identical_to_16bit_kernel(K, delta):
    from cold_compress_amd.harness import glue

    a = _inputs(512, K, 32, seed=7, norm=True, delta=delta)
    h4 = torch.empty(K, dtype=BF, device=DEV)
    h16 = torch.empty(K, dtype=BF, device=DEV)
    _run(a, h4)
    glue.gemv_fused(a["wd"].to(BF), a["x"], delta=a.get("delta"), norm_weight=a["nw"], h_out=h16)
    torch.cuda.synchronize()
    assert torch.equal(h4.view(torch.int16), h16.view(torch.int16))


@pytest.mark.parametrize("name,N,K,opt", [CASES[0], CASES[2], CASES[3], CASES[4]], ids=[CASES[i][0] for i in (0, 2, 3, 4)])
def test_gemv_w4_run_to_run_and_graph_replay_bit_identical(name, N, K, opt):
    a = _inputs(N, K, 32, seed=11, **opt)
    y1, y2 = _run(a), _run(a)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _run(a)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        yg = _run(a)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y1.view(torch.int16), y2.view(torch.int16))
    assert torch.equal(y1.view(torch.int16), yg.view(torch.int16))


def test_refused_shapes_write_nothing():
    from cold_compress_amd import _abi

    f = _abi.lib()["cc_gemv_fused_w4"]
    gen = torch.Generator(device=DEV).manual_seed(3)
    q = torch.randint(0, 256, (64, 2048), generator=gen, device=DEV, dtype=torch.uint8)
    sz = torch.ones(64, 128, 2, dtype=BF, device=DEV)
    x = torch.randn(4096, generator=gen, device=DEV).to(BF)
    nw = torch.ones(4096, dtype=BF, device=DEV)
    y = torch.full((64,), 7.0, dtype=BF, device=DEV)
    h = torch.full((4096,), 7.0, dtype=BF, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for (KK, G, dt, q3, s3, what) in [(96, 64, _abi.CC_DT_BF16, None, None, "K % G"), (32768 + 32, 32, _abi.CC_DT_BF16, None, None, "K too large"),
                                      (4096, 48, _abi.CC_DT_BF16, None, None, "bad G"), (4096, 32, _abi.CC_DT_F16, None, None, "fp16"),
                                      (4096, 32, _abi.CC_DT_BF16, q, None, "W3 without qparams3")]:
        rc = f(p(q), p(sz), p(q3), p(s3), p(x), None, p(nw), 1e-5, p(h), None, None, 0, 0, p(y), 64, KK, G, dt, st)
        assert rc in (-1, -2), what
    torch.cuda.synchronize()
    assert (y.float() == 7.0).all() and (h.float() == 7.0).all()


# ---------------------------------------------------------------------------------------------------------------- harness decode
def _int4_model(cfg, seed, G):
    from cold_compress_amd.harness import ModelArgs, Transformer
    from cold_compress_amd.harness.quantize import WeightOnlyInt4QuantHandler

    torch.manual_seed(seed)
    with torch.device(DEV):
        dense = Transformer(ModelArgs(**cfg)).to(torch.bfloat16)
    sd = WeightOnlyInt4QuantHandler(dense, G).create_quantized_state_dict()
    del dense
    with torch.device("meta"):
        model = WeightOnlyInt4QuantHandler(Transformer(ModelArgs(**cfg)), G).convert_for_runtime()
    model.load_state_dict(sd, assign=True)
    return model.to(device=DEV, dtype=torch.bfloat16).eval()


def _setup(model, max_seq):
    import cold_compress_amd.cache as cache
    from cold_compress_amd.harness import setup_caches

    ap = argparse.ArgumentParser()
    cache.add_cache_arguments(ap)
    kw = vars(ap.parse_args([]))
    kw.update(dict(cache_strategy=["full"], prompt_compression_strategy=["full"], max_cache_length=[1.0]))
    setup_caches(model, None, DEV, max_seq, dict(kw))


@pytest.mark.parametrize("shape,G", [("tiny", 32), ("llama3_8b_2layer", 32), ("llama3_8b_2layer", 128)])
def test_int4_model_decode_through_fused_gemvs(shape, G, monkeypatch):
    """Teacher-forced decode of an int4 harness model: the fused int4 GEMVs (eager, and captured in GraphedDecoder) against the same
    model with fuse_gemv = False, i.e. WeightOnlyInt4Linear.forward (the module formula) per layer.  Logits within 4 ulp of bf16
    relative to the largest logit; greedy tokens equal (a position where the reference's top two logits lie within that tolerance
    is a tie in the model dtype and is not counted); graph replay equals eager bit for bit."""
    from cold_compress_amd.harness import GraphedDecoder, glue, prefill
    from cold_compress_amd.harness.model import CONFIGS

    if shape == "tiny":
        cfg, P, T = dict(CONFIGS["tiny"]), 40, 16
    else:
        cfg, P, T = dict(CONFIGS["Meta-Llama-3-8B-Instruct"], n_layer=2, block_size=512), 64, 12
    model = _int4_model(cfg, seed=5, G=G)
    assert model.output.weight.dtype == torch.uint8 and model.layers[0].attention.wqkv.weight.dtype == torch.uint8
    assert glue.gemv_supported(model.output.weight, model.layers[0].feed_forward.w2.weight)
    _setup(model, P + T + 8)
    V = cfg["vocab_size"]
    gen = torch.Generator().manual_seed(17)
    prompt = torch.randint(0, V, (P,), generator=gen, dtype=torch.int32).to(DEV)
    forced = torch.randint(0, V, (T,), generator=gen, dtype=torch.int32).to(DEV)

    from cold_compress_amd import _abi

    calls = []
    real_call = _abi.call

    def counting_call(name, *args):  # which kernels decode reaches
        calls.append(name)
        return real_call(name, *args)

    monkeypatch.setattr(_abi, "call", counting_call)

    def run(mode):
        calls.clear()
        for layer in model.layers:
            layer.fuse_gemv = mode != "reference"
        model.reset_caches()
        logits, probs = [], []
        dec = GraphedDecoder(model) if mode == "graph" else None
        with torch.no_grad():
            prefill(model, prompt.view(1, -1), torch.arange(P, device=DEV))
            pos = torch.tensor([P], dtype=torch.int32, device=DEV)
            for t in range(T):
                cur = forced[t].view(1, 1)
                if dec is not None:
                    _, pr = dec(model, cur, pos)
                    probs.append(pr.clone())
                else:
                    lg = model(cur, pos, is_prefill=False)[0, -1]
                    logits.append(lg.float().clone())
                    probs.append(glue.softmax_argmax(lg)[0].clone())
                pos += 1
        torch.cuda.synchronize()
        return logits, probs

    ref_logits, _ = run("reference")
    assert "cc_gemv_fused_w4" not in calls  # the reference formula: WeightOnlyInt4Linear.forward
    fused_logits, fused_probs = run("eager")
    # every decode token streams wqkv, wo, the w1/w3 pair and w2 of each layer and the LM head through the int4 kernel
    assert calls.count("cc_gemv_fused_w4") == T * (4 * cfg["n_layer"] + 1), calls.count("cc_gemv_fused_w4")
    _, graph_probs = run("graph")
    for t in range(T):
        r, f = ref_logits[t], fused_logits[t]
        tol = 4 * ULP[torch.bfloat16] * r.abs().max().item()
        err = (r - f).abs().max().item()
        assert err <= tol, f"step {t}: logits differ by {err:.3g} > {tol:.3g}"
        top2 = torch.topk(r, 2).values
        if (top2[0] - top2[1]).item() > tol:
            assert int(r.argmax()) == int(f.argmax()), f"step {t}: greedy token"
        assert torch.equal(fused_probs[t].view(torch.int16), graph_probs[t].view(torch.int16)), f"step {t}: graph != eager"
    for layer in model.layers:
        layer.fuse_gemv = True
