"""cc_gemv_fused_w8 (int8 weight-only decode GEMV) against an fp32 torch composition with the contract's rounding points
(include/coldcompress.h: p = dtype(in . q), t = dtype(p * scale), + bias -> dtype; SwiGLU applies each matrix's own scale before
silu; RoPE on the rounded t): every fused form at the Llama-3-8B decode shapes, the LM head, the 70B and C5-rank shapes, in bf16
and f16, plus a seeded fuzz.  Tolerance: tests/test_gpu_gemv.py's, 2 ulp of the output dtype relative to the largest output.
Also: h_out bit-identical to cc_gemv_fused's, run-to-run and graph-replay bit-identity, refused shapes write nothing, and int8
harness models decoding through the fused GEMVs (eager and hipGraph) against the reference formula per layer."""
import argparse
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ULP = {torch.bfloat16: 2 ** -8, torch.float16: 2 ** -11}


def _rnd(t, dt):
    return t.to(dt).float()


def _quant(N, K, gen, scale=0.02):
    from cold_compress_amd.harness.quantize import quantize_per_channel_int8

    w = torch.randn(N, K, generator=gen, device=DEV) * scale
    return quantize_per_channel_int8(w)


def _ref(q, s, x, dt, q3=None, s3=None, delta=None, nw=None, eps=1e-5, bias=None, freqs=None, rope_rows=0, hd=0):
    xf = x.float()
    h = None
    if nw is not None:
        h = _rnd(xf + delta.float(), dt) if delta is not None else xf
        n = _rnd(h * torch.rsqrt((h * h).mean() + eps), dt)
        xin = _rnd(n * nw.float(), dt)
    else:
        xin = xf
    t = _rnd(_rnd(q.float() @ xin, dt) * s.float(), dt)
    if bias is not None:
        t = _rnd(t + bias.float(), dt)
    if q3 is not None:
        t3 = _rnd(_rnd(q3.float() @ xin, dt) * s3.float(), dt)
        t = _rnd(_rnd(torch.nn.functional.silu(t), dt) * t3, dt)
    if freqs is not None:
        f = freqs.float().view(-1, 2)
        rr = t[:rope_rows].view(-1, hd // 2, 2)
        c, sn = f[:, 0].view(1, -1), f[:, 1].view(1, -1)
        out = torch.stack([rr[..., 0] * c - rr[..., 1] * sn, rr[..., 1] * c + rr[..., 0] * sn], -1).reshape(-1)
        t = torch.cat([_rnd(out, dt), t[rope_rows:]])
    return t, h


def _inputs(N, K, dt, seed, norm=False, delta=False, swiglu=False, rope=None, bias=False):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    q, s32 = _quant(N, K, gen)
    a = dict(q=q, s=s32.to(dt), x=torch.randn(K, generator=gen, device=DEV).to(dt))
    if swiglu:
        q3, s3 = _quant(N, K, gen)
        a.update(q3=q3, s3=s3.to(dt))
    if norm:
        a["nw"] = (1 + 0.1 * torch.randn(K, generator=gen, device=DEV)).to(dt)
        if delta:
            a["delta"] = torch.randn(K, generator=gen, device=DEV).to(dt)
    if bias:
        a["bias"] = (0.1 * torch.randn(N, generator=gen, device=DEV)).to(dt)
    if rope:
        rows, hd = rope
        ang = torch.rand(hd // 2, generator=gen, device=DEV) * 6.28
        a.update(freqs=torch.stack([ang.cos(), ang.sin()], -1).to(dt), rope_rows=rows, hd=hd)
    return a


def _run(a, h_out=None):
    from cold_compress_amd.harness import glue

    return glue.gemv_fused(a["q"], a["x"], w3=a.get("q3"), delta=a.get("delta"), norm_weight=a.get("nw"), h_out=h_out, bias=a.get("bias"),
                           freqs=a.get("freqs"), rope_rows=a.get("rope_rows", 0), head_dim=a.get("hd", 0), scales=a["s"], scales3=a.get("s3"))


def _check(a, dt, what):
    K = a["q"].shape[1]
    h_out = torch.empty(K, dtype=dt, device=DEV) if a.get("nw") is not None else None
    y = _run(a, h_out)
    torch.cuda.synchronize()
    ref, h = _ref(a["q"], a["s"], a["x"], dt, a.get("q3"), a.get("s3"), a.get("delta"), a.get("nw"), bias=a.get("bias"), freqs=a.get("freqs"),
                  rope_rows=a.get("rope_rows", 0), hd=a.get("hd", 0))
    assert y.dtype == dt and torch.isfinite(y).all(), what
    err = (y.float() - ref).abs().max().item()
    tol = 2 * ULP[dt] * ref.abs().max().item()
    assert err <= tol, f"{what}: max err {err:.3g} > {tol:.3g}"
    if h is not None:
        assert torch.equal(h_out.float(), h), f"{what}: h_out"
    return y


CASES = [
    ("wqkv_rope_norm", 6144, 4096, dict(norm=True, delta=True, rope=(5120, 128))), ("wo", 4096, 4096, {}),
    ("w13_norm", 14336, 4096, dict(norm=True, delta=True, swiglu=True)), ("w2", 4096, 14336, {}),
    ("lm_head_norm", 128256, 4096, dict(norm=True, delta=True)),
    ("qwen_wqkv_bias", 4608, 3584, dict(norm=True, delta=True, rope=(4096, 128), bias=True)),
    ("tiny_rope_bias", 96, 64, dict(norm=True, rope=(64, 16), bias=True)), ("ragged", 1031, 1008, dict(norm=True)),
    ("ragged_pair", 77, 272, dict(swiglu=True, norm=True, delta=True)),
    ("70b_wqkv", 10240, 8192, dict(norm=True, delta=True, rope=(9216, 128))), ("70b_wo", 8192, 8192, {}),
    ("70b_w13", 28672, 8192, dict(norm=True, delta=True, swiglu=True)), ("70b_w2", 8192, 28672, {}),
    ("c5_rank_wqkv", 1280, 8192, dict(norm=True, delta=True, rope=(1152, 128))), ("c5_rank_wo", 8192, 1024, {}),
    ("c5_rank_w13", 3584, 8192, dict(norm=True, delta=True, swiglu=True)), ("c5_rank_w2", 8192, 3584, {}),
]


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("name,N,K,opt", CASES, ids=[c[0] for c in CASES])
def test_gemv_w8_matches_contract(name, N, K, opt, dt):
    _check(_inputs(N, K, dt, seed=sum(map(ord, name)), **opt), dt, name)


def test_gemv_w8_fuzz():
    """40 seeded cases over shapes and options (K a multiple of 16, up to 12288)."""
    rng = np.random.default_rng(2024)
    for i in range(40):
        dt = [torch.bfloat16, torch.float16][i % 2]
        K = 16 * int(rng.integers(1, 769))
        N = int(rng.integers(1, 3000))
        swiglu = bool(rng.integers(0, 3) == 0)
        norm = bool(rng.integers(0, 2))
        opt = dict(norm=norm, delta=norm and bool(rng.integers(0, 2)), swiglu=swiglu)
        if not swiglu:
            opt["bias"] = bool(rng.integers(0, 3) == 0)
            hd = int(rng.choice([2, 8, 64, 128]))
            if rng.integers(0, 3) == 0 and N >= hd:
                opt["rope"] = (hd * int(rng.integers(1, N // hd + 1)), hd)
        _check(_inputs(N, K, dt, seed=1000 + i, **opt), dt, f"fuzz {i}: N={N} K={K} {dt} {opt}")


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("K,delta", [(4096, True), (8192, False), (1008, True)])
def test_h_out_bit_identical_to_16bit_kernel(dt, K, delta):
    from cold_compress_amd.harness import glue

    a = _inputs(512, K, dt, seed=7, norm=True, delta=delta)
    h8 = torch.empty(K, dtype=dt, device=DEV)
    h16 = torch.empty(K, dtype=dt, device=DEV)
    _run(a, h8)
    W = (a["q"].float() * a["s"].float()[:, None]).to(dt)
    glue.gemv_fused(W, a["x"], delta=a.get("delta"), norm_weight=a["nw"], h_out=h16)
    torch.cuda.synchronize()
    assert torch.equal(h8.view(torch.int16), h16.view(torch.int16))


@pytest.mark.parametrize("name,N,K,opt", [CASES[0], CASES[2], CASES[3], CASES[4]], ids=[CASES[i][0] for i in (0, 2, 3, 4)])
def test_gemv_w8_run_to_run_and_graph_replay_bit_identical(name, N, K, opt):
    dt = torch.bfloat16
    a = _inputs(N, K, dt, seed=11, **opt)
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

    f = _abi.lib()["cc_gemv_fused_w8"]
    gen = torch.Generator(device=DEV).manual_seed(3)
    K = 96
    q = torch.randint(-128, 128, (64, 4096), generator=gen, device=DEV, dtype=torch.int8)
    s = torch.ones(64, dtype=torch.bfloat16, device=DEV)
    x = torch.randn(4096, generator=gen, device=DEV).to(torch.bfloat16)
    nw = torch.ones(4096, dtype=torch.bfloat16, device=DEV)
    y = torch.full((64,), 7.0, dtype=torch.bfloat16, device=DEV)
    h = torch.full((4096,), 7.0, dtype=torch.bfloat16, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for (KK, dt, q3, s3, what) in [(72, _abi.CC_DT_BF16, None, None, "K % 16"), (32768 + 16, _abi.CC_DT_BF16, None, None, "K too large"),
                                   (K, _abi.CC_DT_F32, None, None, "fp32"), (K, _abi.CC_DT_BF16, q, None, "W3 without scales3")]:
        rc = f(p(q), p(s), p(q3), p(s3), p(x), None, p(nw), 1e-5, p(h), None, None, 0, 0, p(y), 64, KK, dt, st)
        assert rc in (-1, -2), what
    torch.cuda.synchronize()
    assert (y.float() == 7.0).all() and (h.float() == 7.0).all()


# ---------------------------------------------------------------------------------------------------------------- harness decode
def _int8_model(cfg, seed):
    from cold_compress_amd.harness import ModelArgs, Transformer
    from cold_compress_amd.harness.quantize import WeightOnlyInt8QuantHandler

    torch.manual_seed(seed)
    with torch.device(DEV):
        dense = Transformer(ModelArgs(**cfg)).to(torch.bfloat16)
    sd = WeightOnlyInt8QuantHandler(dense).create_quantized_state_dict()
    del dense
    with torch.device("meta"):
        model = WeightOnlyInt8QuantHandler(Transformer(ModelArgs(**cfg))).convert_for_runtime()
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


@pytest.mark.parametrize("shape", ["tiny", "llama3_8b_2layer"])
def test_int8_model_decode_through_fused_gemvs(shape):
    """Teacher-forced decode of an int8 harness model: the fused int8 GEMVs (eager, and captured in GraphedDecoder) against the same
    model with fuse_gemv = False, i.e. WeightOnlyInt8Linear.forward (the reference formula) per layer.  Logits within 4 ulp of bf16
    relative to the largest logit; greedy tokens equal (a position where the reference's top two logits lie within that tolerance
    is a tie in the model dtype and is not counted); graph replay equals eager bit for bit."""
    from cold_compress_amd.harness import GraphedDecoder, glue, prefill
    from cold_compress_amd.harness.model import CONFIGS

    if shape == "tiny":
        cfg, P, T = dict(CONFIGS["tiny"]), 40, 16
    else:
        cfg, P, T = dict(CONFIGS["Meta-Llama-3-8B-Instruct"], n_layer=2, block_size=512), 64, 12
    model = _int8_model(cfg, seed=5)
    assert model.output.weight.dtype == torch.int8 and model.layers[0].attention.wqkv.weight.dtype == torch.int8
    assert glue.gemv_supported(model.output.weight, model.layers[0].feed_forward.w2.weight)
    _setup(model, P + T + 8)
    V = cfg["vocab_size"]
    gen = torch.Generator().manual_seed(17)
    prompt = torch.randint(0, V, (P,), generator=gen, dtype=torch.int32).to(DEV)
    forced = torch.randint(0, V, (T,), generator=gen, dtype=torch.int32).to(DEV)

    def run(mode):
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
    fused_logits, fused_probs = run("eager")
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
