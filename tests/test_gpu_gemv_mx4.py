"""cc_gemv_fused_mx4 (MXFP4 weight-only decode GEMV) against an fp32 torch composition of the contract (include/coldcompress.h:
p = in . (e2m1(q) * 2^(byte - 127)) with fp32 accumulation, t = bf16(p), + bias -> bf16; SwiGLU rounds each t before silu; RoPE on
the rounded t): the smallest shapes that reach each path (K = 32: one block, one lane; 2048: one full segment; 2080: segment plus
one chunk; 4096: two waves per row; 6144: four; 14336 and 28672: several segments per wave, the 8B and 70B w2; 32768: the limit;
N in {2, 38, 256}, 38 no multiple of any rows-per-workgroup; the launcher's choice does not depend on N), every form at every
waves-per-row split, plus a seeded fuzz.  Tolerance: 2 ulp of bf16 relative to the largest output.  Also: h_out and the normalised
input bit-identical to cc_gemv_fused's, run-to-run and graph-replay bit identity, an error return writes nothing, and a tiny MXFP4
harness model decoding through the fused GEMVs (eager and hipGraph) against the module formula per layer."""
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


def _quant(N, K, gen, scale=0.02):
    """-> (packed uint8 [N, K / 2], uint8 scale bytes [N, K / 32], fp32 dequantised weight [N, K])."""
    from cold_compress_amd.harness.quantize import dequantize_mxfp4, quantize_mxfp4

    w = (torch.randn(N, K, generator=gen, device=DEV) * scale).to(BF)
    packed, sb = quantize_mxfp4(w)
    return packed, sb, dequantize_mxfp4(packed, sb)


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


def _inputs(N, K, seed, norm=False, delta=False, swiglu=False, rope=None, bias=False):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    q, sb, wd = _quant(N, K, gen)
    a = dict(q=q, sb=sb, wd=wd, x=torch.randn(K, generator=gen, device=DEV).to(BF))
    if swiglu:
        q3, sb3, wd3 = _quant(N, K, gen)
        a.update(q3=q3, sb3=sb3, wd3=wd3)
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
                           freqs=a.get("freqs"), rope_rows=a.get("rope_rows", 0), head_dim=a.get("hd", 0), scales=a["sb"],
                           scales3=a.get("sb3"))


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
    print(f"{what}: max err {err:.3g}, tolerance {tol:.3g}")
    assert err <= tol, f"{what}: max err {err:.3g} > {tol:.3g}"
    if h is not None:
        assert torch.equal(h_out.float(), h), f"{what}: h_out"
    return y


NORM = dict(norm=True, delta=True)
PAIR = dict(norm=True, delta=True, swiglu=True)
CASES = [
    # one wave per row
    ("k32_plain", 2, 32, {}), ("k32_norm", 38, 32, NORM), ("k32_pair", 38, 32, PAIR), ("k32_rope_bias", 38, 32, dict(rope=(36, 4), bias=True)),
    ("k2048_plain", 256, 2048, {}), ("k2048_norm", 38, 2048, NORM), ("k2048_pair", 2, 2048, dict(swiglu=True)),
    ("k2048_rope", 256, 2048, dict(norm=True, rope=(128, 64))), ("k2048_bias", 38, 2048, dict(bias=True)),
    # two waves per row
    ("k2080_plain", 38, 2080, {}), ("k2080_pair", 256, 2080, PAIR), ("k2080_norm_rope_bias", 2, 2080, dict(rope=(2, 2), bias=True, **NORM)),
    ("k4096_plain", 256, 4096, {}), ("k4096_norm", 2, 4096, dict(norm=True)), ("k4096_pair", 38, 4096, PAIR),
    ("k4096_rope", 38, 4096, dict(rope=(32, 16), **NORM)), ("k4096_bias", 256, 4096, dict(bias=True, **NORM)),
    # four waves per row
    ("k6144_plain", 38, 6144, {}), ("k6144_norm", 256, 6144, NORM), ("k6144_pair", 2, 6144, PAIR),
    ("k6144_rope_bias", 256, 6144, dict(rope=(128, 128), bias=True, **NORM)),
    ("k14336_plain", 256, 14336, {}), ("k14336_pair", 38, 14336, PAIR), ("k14336_norm", 2, 14336, NORM),
    ("k28672_plain", 38, 28672, {}), ("k28672_pair", 2, 28672, dict(swiglu=True)),
    ("k28672_norm_rope_bias", 256, 28672, dict(rope=(192, 64), bias=True, **NORM)),
    ("k32768_plain", 2, 32768, {}), ("k32768_norm", 38, 32768, NORM), ("k32768_pair", 256, 32768, PAIR),
]


@pytest.mark.parametrize("name,N,K,opt", CASES, ids=[c[0] for c in CASES])
def test_gemv_mx4_matches_contract(name, N, K, opt):
    _check(_inputs(N, K, seed=sum(map(ord, name)), **opt), name)


def test_gemv_mx4_fuzz():
    """40 seeded cases over (N, K, form): K any multiple of 32 up to 32768."""
    rng = np.random.default_rng(2026)
    for i in range(40):
        K = 32 * int(rng.integers(1, 1025))
        N = int(rng.integers(1, 600))
        swiglu = bool(rng.integers(0, 3) == 0)
        norm = bool(rng.integers(0, 2))
        opt = dict(norm=norm, delta=norm and bool(rng.integers(0, 2)), swiglu=swiglu)
        if not swiglu:
            opt["bias"] = bool(rng.integers(0, 3) == 0)
            hd = int(rng.choice([2, 8, 64, 128]))
            if rng.integers(0, 3) == 0 and N >= hd:
                opt["rope"] = (hd * int(rng.integers(1, N // hd + 1)), hd)
        _check(_inputs(N, K, seed=3000 + i, **opt), f"fuzz {i}: N={N} K={K} {opt}")


@pytest.mark.parametrize("K,delta", [(32, True), (2080, False), (4096, True), (28672, True)])
def test_h_out_bit_identical_to_16bit_kernel(K, delta):
    from cold_compress_amd.harness import glue

    a = _inputs(64, K, seed=7, norm=True, delta=delta)
    h4 = torch.empty(K, dtype=BF, device=DEV)
    h16 = torch.empty(K, dtype=BF, device=DEV)
    _run(a, h4)
    glue.gemv_fused(a["wd"].to(BF), a["x"], delta=a.get("delta"), norm_weight=a["nw"], h_out=h16)
    torch.cuda.synchronize()
    assert torch.equal(h4.view(torch.int16), h16.view(torch.int16))


@pytest.mark.parametrize("K,delta", [(32, False), (2080, True), (4096, True), (6144, True)])
def test_normalised_input_bit_identical_to_16bit_kernel(K, delta):
    """a plain product on a norm form: W = the identity (code 2 = 1.0 on the diagonal, scale byte 127), so y IS the normalised
    input, rounded by nothing; the 16-bit kernel over the bf16 identity gives its own.  Equal bit for bit."""
    from cold_compress_amd.harness import glue
    from cold_compress_amd.harness.quantize import dequantize_mxfp4

    gen = torch.Generator(device=DEV).manual_seed(21 + K)
    codes = torch.zeros(K, K, dtype=torch.uint8, device=DEV)
    codes.fill_diagonal_(2)
    q = (codes[:, 0::2] | (codes[:, 1::2] << 4)).contiguous()
    sb = torch.full((K, K // 32), 127, dtype=torch.uint8, device=DEV)
    eye = dequantize_mxfp4(q, sb).to(BF)
    assert torch.equal(eye, torch.eye(K, dtype=BF, device=DEV))
    x = torch.randn(K, generator=gen, device=DEV).to(BF)
    d = torch.randn(K, generator=gen, device=DEV).to(BF) if delta else None
    nw = (1 + 0.1 * torch.randn(K, generator=gen, device=DEV)).to(BF)
    y4 = glue.gemv_fused(q, x, delta=d, norm_weight=nw, scales=sb)
    y16 = glue.gemv_fused(eye, x, delta=d, norm_weight=nw)
    torch.cuda.synchronize()
    assert y4.float().abs().max() > 0
    assert torch.equal(y4.view(torch.int16), y16.view(torch.int16))


@pytest.mark.parametrize("name,N,K,opt", [CASES[7], CASES[14], CASES[22], CASES[29]], ids=[CASES[i][0] for i in (7, 14, 22, 29)])
def test_gemv_mx4_run_to_run_and_graph_replay_bit_identical(name, N, K, opt):
    a = _inputs(N, K, seed=11, **opt)
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


def test_an_error_return_writes_nothing():
    from cold_compress_amd import _abi

    f = _abi.lib()["cc_gemv_fused_mx4"]
    gen = torch.Generator(device=DEV).manual_seed(3)
    q = torch.randint(0, 256, (64, 2048), generator=gen, device=DEV, dtype=torch.uint8)
    sb = torch.full((64, 128), 127, dtype=torch.uint8, device=DEV)
    x = torch.randn(4096, generator=gen, device=DEV).to(BF)
    nw = torch.ones(4096, dtype=BF, device=DEV)
    y = torch.full((64,), 7.0, dtype=BF, device=DEV)
    h = torch.full((4096,), 7.0, dtype=BF, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for (KK, dt, q3, s3, xx, want, what) in [(48, _abi.CC_DT_BF16, None, None, x, -2, "K = 48"), (32768 + 32, _abi.CC_DT_BF16, None, None, x, -2, "K too large"),
                                            (4096, _abi.CC_DT_F16, None, None, x, -2, "fp16"), (4096, _abi.CC_DT_F32, None, None, x, -2, "fp32"),
                                            (4096, _abi.CC_DT_BF16, q, None, x, -1, "W3 without scales3"),
                                            (4064, _abi.CC_DT_BF16, None, None, x[1:], -1, "misaligned x")]:
        rc = f(p(q), p(sb), p(q3), p(s3), p(xx), None, p(nw), 1e-5, p(h), None, None, 0, 0, p(y), 64, KK, dt, st)
        assert rc == want, what
    torch.cuda.synchronize()
    assert (y.float() == 7.0).all() and (h.float() == 7.0).all()


# ---------------------------------------------------------------------------------------------------------------- harness decode
def _mxfp4_model(cfg, seed):
    from cold_compress_amd.harness import ModelArgs, Transformer
    from cold_compress_amd.harness.quantize import WeightOnlyMxfp4QuantHandler

    torch.manual_seed(seed)
    with torch.device(DEV):
        dense = Transformer(ModelArgs(**cfg)).to(torch.bfloat16)
    sd = WeightOnlyMxfp4QuantHandler(dense).create_quantized_state_dict()
    del dense
    with torch.device("meta"):
        model = WeightOnlyMxfp4QuantHandler(Transformer(ModelArgs(**cfg))).convert_for_runtime()
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


def test_mxfp4_model_decode_through_fused_gemvs(monkeypatch):
    """Teacher-forced decode of a tiny MXFP4 harness model: the fused MXFP4 GEMVs (eager, and captured in GraphedDecoder) against the
    same model with fuse_gemv = False, i.e. WeightOnlyMxfp4Linear.forward (the module formula) per layer.  The int4 harness test's
    tolerances: logits within 4 ulp of bf16 relative to the largest logit; greedy tokens equal (a position where the reference's top
    two logits lie within that tolerance is a tie in the model dtype and is not counted); graph replay equals eager bit for bit.
    cc_gemv_fused_mx4 runs T * (4 * n_layer + 1) times per decode and never during prefill."""
    from cold_compress_amd.harness import GraphedDecoder, glue, prefill
    from cold_compress_amd.harness.model import CONFIGS

    cfg, P, T = dict(CONFIGS["tiny"]), 40, 16
    model = _mxfp4_model(cfg, seed=5)
    assert model.output.weight.dtype == torch.uint8 and model.layers[0].attention.wqkv.block_scales.dtype == torch.uint8
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
            assert "cc_gemv_fused_mx4" not in calls and "cc_gemv_fused_w4" not in calls  # prefill keeps the module formula
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
    assert "cc_gemv_fused_mx4" not in calls  # the reference formula: WeightOnlyMxfp4Linear.forward
    fused_logits, fused_probs = run("eager")
    # every decode token streams wqkv, wo, the w1/w3 pair and w2 of each layer and the LM head through the MXFP4 kernel
    assert calls.count("cc_gemv_fused_mx4") == T * (4 * cfg["n_layer"] + 1), calls.count("cc_gemv_fused_mx4")
    assert "cc_gemv_fused_w4" not in calls and "cc_gemv_fused" not in calls
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
