"""Weight-only int8 models on the host side (no GPU): the quantiser against the reference handler's recorded output
(tests/golden/w8_quant_ref.npz, written by tools/gen_w8_golden.py) and against the contract's formula written out in numpy, the
handler's module conversion and state-dict keys, the quantise CLI and `harness.load_model`, the C ABI row and argument validation
of cc_gemv_fused_w8, and tensor parallelism of an int8 model over gloo at world 2 and 4."""
import ctypes as C
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "w8_quant_ref.npz")


def _golden():
    return np.load(GOLDEN)


def _numpy_quant(w):
    """The contract's formula, independently of torch: per row lo / hi clamped through 0, s32 = max(max(-lo, hi) / 127.5, eps)
    in fp32, q = clamp(round_half_even(w / s32), -128, 127)."""
    w = np.asarray(w, np.float32)
    lo = np.minimum(w.min(1), np.float32(0))
    hi = np.maximum(w.max(1), np.float32(0))
    s = np.maximum(np.maximum(-lo, hi) / np.float32(127.5), np.finfo(np.float32).eps).astype(np.float32)
    q = np.clip(np.rint(w / s[:, None]), -128, 127).astype(np.int8)
    return q, s


@pytest.mark.parametrize("tag,dt", [("f32", torch.float32), ("bf16", torch.bfloat16)])
def test_quantiser_matches_reference_fixture_bit_for_bit(tag, dt):
    from cold_compress_amd.harness.quantize import WeightOnlyInt8QuantHandler, quantize_per_channel_int8

    g = _golden()
    w = torch.from_numpy(g[f"wdt_{tag}"]).to(dt)
    lin = nn.Linear(w.shape[1], w.shape[0], bias=True).to(dt)
    with torch.no_grad():
        lin.weight.copy_(w)
        lin.bias.copy_(torch.from_numpy(g["bias_f32"]).to(dt))
    sd = WeightOnlyInt8QuantHandler(nn.Sequential(lin)).create_quantized_state_dict()
    assert sd["0.weight"].dtype == torch.int8 and sd["0.scales"].dtype == dt
    assert np.array_equal(sd["0.weight"].numpy(), g[f"q_{tag}"])
    assert np.array_equal(sd["0.scales"].float().numpy(), g[f"scales_{tag}"])
    # the fp32 scale the division used, and the codes, against the formula written out in numpy
    q32, s32 = quantize_per_channel_int8(w)
    qn, sn = _numpy_quant(w.float().numpy())
    assert np.array_equal(q32.numpy(), qn) and np.array_equal(s32.numpy(), sn)
    assert np.array_equal(torch.from_numpy(sn).to(dt).float().numpy(), g[f"scales_{tag}"])
    # the edge rows are really there: all-zero (eps scale), .5 ties rounded to even, the negative-only row's minimum at -128
    assert g[f"scales_{tag}"][0] == np.finfo(np.float32).eps and not g[f"q_{tag}"][0].any()
    assert list(g[f"q_{tag}"][2, :8]) == [127, 2, -4, 0, 2, 0, -2, 4]
    assert g[f"q_{tag}"][3].min() == -128 and g[f"q_{tag}"][3].max() <= 0


@pytest.mark.parametrize("tag,dt", [("f32", torch.float32), ("bf16", torch.bfloat16)])
def test_int8_linear_forward_matches_reference_fixture(tag, dt):
    """forward = F.linear(x, W.to(dtype)) * scales + bias on CPU.  Tolerance: the CPU GEMM's summation order may differ between host
    ISAs — 4 fp32 ulps of the largest output in fp32, 1 ulp of the largest output in bf16."""
    from cold_compress_amd.harness.quantize import WeightOnlyInt8Linear

    g = _golden()
    K, N = g["w_f32"].shape[1], g["w_f32"].shape[0]
    m = WeightOnlyInt8Linear(K, N, bias=True, dtype=dt)
    m.load_state_dict({"weight": torch.from_numpy(g[f"q_{tag}"]), "scales": torch.from_numpy(g[f"scales_{tag}"]).to(dt),
                       "bias": torch.from_numpy(g["bias_f32"]).to(dt)})
    with torch.no_grad():
        y = m(torch.from_numpy(g["x_f32"]).to(dt))
    assert y.dtype == dt
    ref = g[f"y_{tag}"]
    tol = (4 * 2.0 ** -23 if dt == torch.float32 else 2.0 ** -8) * np.abs(ref).max()
    assert np.abs(y.float().numpy() - ref).max() <= tol


def _tiny(dtype=torch.float32, seed=0):
    from cold_compress_amd.harness import ModelArgs, Transformer
    from cold_compress_amd.harness.model import CONFIGS

    torch.manual_seed(seed)
    return Transformer(ModelArgs(**CONFIGS["tiny"])).to(dtype).eval()


def test_handler_converts_every_linear_and_keeps_the_embedding():
    from cold_compress_amd.harness.quantize import WeightOnlyInt8Linear, WeightOnlyInt8QuantHandler

    model = _tiny(torch.bfloat16)
    linears = [n for n, m in model.named_modules() if isinstance(m, nn.Linear)]
    assert "output" in linears and len(linears) == 1 + 5 * model.config.n_layer
    sd = WeightOnlyInt8QuantHandler(model).create_quantized_state_dict()
    for n in linears:
        assert sd[f"{n}.weight"].dtype == torch.int8 and sd[f"{n}.scales"].dtype == torch.bfloat16
        assert sd[f"{n}.scales"].shape == (sd[f"{n}.weight"].shape[0],)
    assert sd["tok_embeddings.weight"].dtype == torch.bfloat16
    conv = WeightOnlyInt8QuantHandler(model).convert_for_runtime()
    for n in linears:
        assert isinstance(conv.get_submodule(n), WeightOnlyInt8Linear), n
    assert isinstance(conv.tok_embeddings, nn.Embedding)
    keys = set(conv.state_dict())
    assert keys == set(sd), keys ^ set(sd)
    assert all(k.endswith((".weight", ".scales", ".bias")) for k in keys)
    conv.load_state_dict(sd)
    assert conv.output.weight.dtype == torch.int8


def test_quantize_cli_and_load_model(tmp_path):
    from cold_compress_amd import _abi
    from cold_compress_amd.harness import load_model

    d = tmp_path / "tiny"
    d.mkdir()
    model = _tiny(torch.bfloat16, seed=3)
    torch.save(model.state_dict(), str(d / "model.pth"))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "cold_compress_amd.harness.quantize", "--checkpoint_path", str(d / "model.pth"),
                        "--mode", "int8"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert (d / "model_int8.pth").is_file()
    r4 = subprocess.run([sys.executable, "-m", "cold_compress_amd.harness.quantize", "--checkpoint_path", str(d / "model.pth"),
                         "--mode", "int4"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r4.returncode != 0 and not (d / "model_int4.pth").exists()

    m8 = load_model(d / "model_int8.pth", "cpu", torch.bfloat16, False)
    sd = torch.load(str(d / "model_int8.pth"), weights_only=True)
    for n, mod in m8.named_modules():
        if hasattr(mod, "scales"):
            assert mod.weight.dtype == torch.int8 and mod.scales.dtype == torch.bfloat16
            assert torch.equal(mod.weight, sd[f"{n}.weight"]) and torch.equal(mod.scales, sd[f"{n}.scales"])
    assert m8.output.weight.dtype == torch.int8 and m8.tok_embeddings.weight.dtype == torch.bfloat16
    m16 = load_model(d / "model.pth", "cpu", torch.bfloat16, False)
    assert m16.output.weight.dtype == torch.bfloat16 and torch.equal(m16.output.weight, model.output.weight)
    (d / "model_int4.g32.pth").write_bytes(b"")
    with pytest.raises(_abi.ColdCompressError, match="int4"):
        load_model(d / "model_int4.g32.pth", "cpu", torch.bfloat16, False)


def test_abi_row_and_argument_validation_without_gpu():
    from cold_compress_amd import _abi, _build

    header = open(os.path.join(ROOT, "include", "coldcompress.h")).read()
    m = re.search(r"^int cc_gemv_fused_w8\(([^;]*)\);", header, re.M)
    assert m, "cc_gemv_fused_w8 is not declared"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 18 and args[0].startswith("const int8_t*") and args[2].startswith("const int8_t*")
    res, argtypes = _abi.SIGNATURES["cc_gemv_fused_w8"]
    assert res is C.c_int and len(argtypes) == 18 and argtypes[7] is C.c_float
    assert "cc_gemv_fused_w8" in _abi.DEVICE_ONLY
    fns = _abi.bind(C.CDLL(_build.build()))
    f = fns["cc_gemv_fused_w8"]
    assert fns["cc_abi_version"]() == 1
    p = C.c_void_p(0x1000)  # never dereferenced: validation happens before any launch
    BAD, UNS = -1, -2
    call = lambda **k: f(*[k.get(n, d) for n, d in (  # noqa: E731
        ("W", p), ("s", p), ("W3", None), ("s3", None), ("x", p), ("delta", None), ("nw", None), ("eps", 1e-5), ("h", None),
        ("bias", None), ("freqs", None), ("rr", 0), ("hd", 0), ("y", p), ("N", 64), ("K", 64), ("dt", _abi.CC_DT_BF16),
        ("st", None))])
    assert call(W=None) == BAD and call(s=None) == BAD and call(x=None) == BAD and call(y=None) == BAD
    assert call(N=0) == BAD and call(K=-16) == BAD and call(dt=7) == BAD
    assert call(W3=p) == BAD and call(s3=p) == BAD          # W3 and scales3 go together
    assert call(delta=p) == BAD and call(h=p) == BAD        # the residual needs the norm prologue
    assert call(W3=p, s3=p, bias=p) == BAD
    assert call(freqs=p, rr=96, hd=32) == BAD and call(freqs=p, rr=64, hd=3) == BAD and call(freqs=p, W3=p, s3=p, rr=64, hd=32) == BAD
    assert call(K=72) == UNS                                 # K % 16
    assert call(K=32768 + 16) == UNS                         # K * 2 > 64 KiB
    assert call(dt=_abi.CC_DT_F32) == UNS                    # 16-bit activations only


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


class _FullCacheDouble:
    head_specific = False
    max_cache_length = 1 << 20

    def return_attn(self):
        return False

    def update_kv(self, *a, **k):
        return None

    def update_state(self, *a, **k):
        return None


def _attention_double(q, k, v, attn_mask=None, return_attn=False, is_causal=None, **kw):
    HQ, H = q.shape[1], k.shape[1]
    R = HQ // H
    L = q.shape[2]
    kk, vv = k.repeat_interleave(R, 1), v.repeat_interleave(R, 1)
    w = (q @ kk.transpose(-1, -2)) / (q.shape[-1] ** 0.5)
    w = w.masked_fill(~torch.tril(torch.ones(L, L, dtype=torch.bool)), float("-inf"))
    return torch.softmax(w, -1) @ vv, None


def _worker_w8(rank, world, port, q):
    try:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK=str(rank), LOCAL_WORLD_SIZE=str(world))
        import cold_compress_amd.harness.model as hm
        from cold_compress_amd import tp
        from cold_compress_amd.harness import ModelArgs, Transformer
        from cold_compress_amd.harness.quantize import WeightOnlyInt8QuantHandler

        torch.set_num_threads(1)
        assert tp.maybe_init_dist() == rank and dist.get_backend() == "gloo"
        hm.scaled_dot_product_attention = _attention_double
        import host_glue

        host_glue.install(hm.glue)
        torch.manual_seed(0)
        cfg = dict(block_size=64, vocab_size=64, n_layer=2, n_head=32, n_local_heads=8, dim=256, intermediate_size=384, attention_bias=True)
        dense = Transformer(ModelArgs(**cfg)).eval()
        sd = WeightOnlyInt8QuantHandler(dense).create_quantized_state_dict()
        full = WeightOnlyInt8QuantHandler(Transformer(ModelArgs(**cfg))).convert_for_runtime().eval()
        sharded = WeightOnlyInt8QuantHandler(Transformer(ModelArgs(**cfg))).convert_for_runtime().eval()
        full.load_state_dict(sd)
        sharded.load_state_dict(sd)
        tp.apply_tp(sharded)
        for m in (full, sharded):
            m.freqs_cis = hm.precompute_freqs_cis(64, 8, 10000, torch.float32)
            for layer in m.layers:
                layer.attention.kv_cache = _FullCacheDouble()
        a, ff = sharded.layers[0].attention, sharded.layers[0].feed_forward
        fa, fff = full.layers[0].attention, full.layers[0].feed_forward
        hq, hk = 32 // world, 8 // world
        assert a.wqkv.weight.dtype == torch.int8 and "weight" in dict(a.wqkv.named_buffers())
        assert a.wqkv.weight.shape == ((hq + 2 * hk) * 8, 256) and a.wqkv.scales.shape == ((hq + 2 * hk) * 8,)
        assert torch.equal(a.wqkv.scales[: hq * 8], fa.wqkv.scales[rank * hq * 8:(rank + 1) * hq * 8])
        assert torch.equal(a.wqkv.bias[: hq * 8], fa.wqkv.bias[rank * hq * 8:(rank + 1) * hq * 8])
        assert a.wo.weight.shape == (256, hq * 8) and torch.equal(a.wo.scales, fa.wo.scales)  # rowwise: scales whole
        assert torch.equal(ff.w1.scales, fff.w1.scales[rank * 384 // world:(rank + 1) * 384 // world])
        assert ff.w2.weight.shape == (256, 384 // world) and torch.equal(ff.w2.scales, fff.w2.scales)
        idx = torch.arange(12).view(1, 12) % 64
        pos = torch.arange(12)
        with torch.no_grad():
            y_full = full(idx, pos, is_prefill=True)
            y_tp = sharded(idx, pos, is_prefill=True)
        q.put((rank, (y_full - y_tp).abs().max().item()))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:  # pragma: no cover
        q.put((rank, repr(e)))
        raise


@pytest.mark.parametrize("world", [2, 4])
def test_tp_gloo_int8_matches_single_process(world):
    """ref: tp.py:99-100 — colwise int8 linears split weight rows, scales and bias; rowwise split the weight columns and keep the
    scales whole.  The sharded int8 model's logits equal the unsharded int8 model's within the existing gloo test's 1e-4."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker_w8, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=180) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    for rank, err in res:
        assert isinstance(err, float), f"rank {rank}: {err}"
        assert err < 1e-4, f"rank {rank}: int8 TP output differs from the single-process model by {err}"
