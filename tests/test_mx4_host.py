"""Weight-only MXFP4 models on the host side (no GPU): the quantiser against an exact twin written with `fractions` (random rows and
edge blocks), its by-construction bounds, the refusal of non-finite weights, the handler's module conversion and state-dict round
trip, the quantise CLI and `harness.load_model` (and what it refuses), the C ABI row and argument validation of cc_gemv_fused_mx4,
glue's refusals, tensor parallelism of an MXFP4 model over gloo at world 2, the accuracy record against int4, and the launcher mirror
of tests/gemv_mx4_exact.py against the source."""
import ctypes as C
import math
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp
import torch.nn as nn

import gemv_mx4_exact as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = [Fraction(v) for v in ("0", "1/2", "1", "3/2", "2", "3", "4", "6")]


# ------------------------------------------------------------------------------------------------------------ the exact twin
def _twin_block(vals):
    """(codes, scale byte) of one block of 32 Python floats, in exact rational arithmetic: e = the smallest integer with
    amax <= 6 * 2^e, clamped to [-120, 120] (-120 for an all-zero block); the code the nearest grid point to |w| / 2^e, ties to the
    even mantissa (the even index), past 6: 6; the sign bit is the float's own."""
    fr = [Fraction(v) for v in vals]
    amax = max(abs(f) for f in fr)
    if amax == 0:
        e = -120
    else:
        e = -200
        while amax > 6 * Fraction(2) ** e:
            e += 1
        e = max(-120, min(120, e))
    scale = Fraction(2) ** e
    codes = []
    for v, f in zip(vals, fr):
        y = abs(f) / scale
        best = min(range(8), key=lambda i: (abs(GRID[i] - y), i & 1))
        codes.append(best | (8 if math.copysign(1.0, v) < 0 else 0))
    return codes, e + 127


def _twin(w):
    N, K = w.shape
    codes = np.zeros((N, K), np.uint8)
    sb = np.zeros((N, K // 32), np.uint8)
    wl = w.double().tolist()
    for n in range(N):
        for b in range(K // 32):
            c, s = _twin_block(wl[n][32 * b:32 * b + 32])
            codes[n, 32 * b:32 * b + 32] = c
            sb[n, b] = s
    return codes, sb


def _edge_blocks():
    """[rows of 32 fp32 values], each one an edge of the quantiser."""
    g = torch.Generator().manual_seed(11)
    base = torch.randn(32, generator=g) * 0.02
    rows = [torch.zeros(32), torch.full((32,), 0.0123), torch.full((32,), -3.0)]
    for e in (-7, 0, 5):  # every tie, times the block scale 2^e (a 6 * 2^e element pins the scale)
        t = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, -0.25, -0.75, -1.25, -1.75, -2.5, -3.5, -5.0, 6.0] + [0.0] * 17)
        rows.append(t * 2.0 ** e)
    for e in (-9, 3):  # amax exactly 6 * 2^e, and one bf16 step above (the next exponent)
        r = base.clone() * 2.0 ** e
        r[5] = 6.0 * 2.0 ** e
        rows.append(r)
        r = r.clone()
        r[5] = torch.tensor(6.0 * 2.0 ** e).to(torch.bfloat16).view(torch.int16).add(1).view(torch.bfloat16).float()
        rows.append(r)
    r = base.clone()
    r[0], r[1] = -0.0, 0.0
    rows.append(r)
    r = torch.zeros(32)
    r[3] = -0.0  # an all-zero block with a negative zero
    rows.append(r)
    r = base.clone()
    r[7] *= 50  # one outlier
    rows.append(r)
    # subnormal-sized weights at the clamp's lower end: e clamps to -120
    rows.append(torch.full((32,), 2.0 ** -130))
    r = torch.zeros(32)
    r[0], r[1], r[2], r[3] = 6 * 2.0 ** -120, 2.0 ** -121, -(2.0 ** -122), 2.0 ** -140
    rows.append(r)
    r = torch.zeros(32)
    r[0], r[1] = 2.0 ** -126, 2.0 ** -149
    rows.append(r)
    return torch.stack(rows)


def _unpack(packed):
    from cold_compress_amd.harness.quantize import unpack_int4

    return unpack_int4(packed).numpy().astype(np.uint8)


def test_quantiser_matches_the_exact_twin_on_random_rows():
    from cold_compress_amd.harness.quantize import quantize_mxfp4

    g = torch.Generator().manual_seed(1)
    for w in ((torch.randn(6, 128, generator=g) * 0.02), (torch.randn(4, 64, generator=g) * 0.02).to(torch.bfloat16)):
        packed, sb = quantize_mxfp4(w)
        assert packed.dtype == torch.uint8 and tuple(packed.shape) == (w.shape[0], w.shape[1] // 2)
        assert sb.dtype == torch.uint8 and tuple(sb.shape) == (w.shape[0], w.shape[1] // 32)
        codes, tsb = _twin(w.float())
        assert np.array_equal(_unpack(packed), codes)
        assert np.array_equal(sb.numpy(), tsb)
        # the packing: column 2j in the low nibble of byte j
        assert np.array_equal(packed.numpy(), codes[:, 0::2] | (codes[:, 1::2] << 4))


def test_quantiser_matches_the_exact_twin_on_edge_blocks():
    from cold_compress_amd.harness.quantize import dequantize_mxfp4, quantize_mxfp4

    w = _edge_blocks()
    packed, sb = quantize_mxfp4(w)
    codes, tsb = _twin(w)
    got = _unpack(packed)
    assert np.array_equal(sb.numpy(), tsb), (sb.flatten().tolist(), tsb.flatten().tolist())
    assert np.array_equal(got, codes), np.argwhere(got != codes)[:8]
    # the edges are really there
    assert sb[0, 0] == 7 and (got[0] == 0).all()                          # all zero: e = -120
    assert (got[1] == 7).all() or (got[1] == got[1, 0]).all()             # constant
    assert got[3, :15].tolist() == [0, 2, 2, 4, 4, 6, 6, 8, 10, 10, 12, 12, 14, 14, 7]  # ties to the even mantissa, both signs
    assert sb[7, 0] == sb[6, 0] + 1 and sb[9, 0] == sb[8, 0] + 1          # one bf16 step above 6 * 2^e: the next exponent
    assert got[10, 0] == 8 and got[10, 1] == 0 and got[11, 3] == 8        # -0 keeps its sign
    assert sb[13, 0] == 7 and (got[13] == 0).all()                        # 2^-130 under the clamp: code 0
    assert sb[14, 0] == 7 and got[14, :4].tolist() == [7, 1, 8, 0]         # 6, 0.5 and the tie 0.25 (to 0, negative) at 2^-120
    dq = dequantize_mxfp4(packed, sb)
    assert dq.dtype == torch.float32 and torch.equal(dq, dq.to(torch.bfloat16).float())  # exact in bf16
    assert torch.equal(torch.signbit(dq), torch.signbit(w))


def _bounds(w, packed, sb):
    """the by-construction bounds: nothing finite saturates, and every element is within half the widest code gap (4 -> 6)."""
    from cold_compress_amd.harness.quantize import dequantize_mxfp4

    dq = dequantize_mxfp4(packed, sb).double()
    N, K = w.shape
    two_e = torch.ldexp(torch.ones(N, K // 32, dtype=torch.float64), sb.to(torch.int32) - 127)
    amax = w.double().view(N, K // 32, 32).abs().amax(-1)
    assert (amax <= 6 * two_e).all()
    assert (dq.view(N, K // 32, 32).abs().amax(-1) <= 6 * two_e).all()
    err = (w.double() - dq).abs().view(N, K // 32, 32)
    assert (err <= two_e.unsqueeze(-1)).all()
    return dq


def test_by_construction_bounds():
    from cold_compress_amd.harness.quantize import quantize_mxfp4

    g = torch.Generator().manual_seed(2)
    for w in (torch.randn(64, 256, generator=g) * 0.02, _edge_blocks(), torch.randn(8, 64, generator=g) * 1e20,
              (torch.randn(8, 64, generator=g) * 1e-30)):
        _bounds(w, *quantize_mxfp4(w))


def test_non_finite_weights_are_refused():
    from cold_compress_amd.harness.quantize import WeightOnlyMxfp4QuantHandler, quantize_mxfp4

    for bad in (float("inf"), float("-inf"), float("nan")):
        w = torch.zeros(2, 64)
        w[1, 40] = bad
        with pytest.raises(ValueError, match="non-finite"):
            quantize_mxfp4(w)
        model = nn.Sequential(nn.Linear(64, 8, bias=False), nn.Linear(64, 2, bias=False))
        with torch.no_grad():
            model[1].weight.copy_(w)
        with pytest.raises(ValueError, match=r"^1: .*non-finite"):  # names the linear
            WeightOnlyMxfp4QuantHandler(model).create_quantized_state_dict()


def _tiny(dtype=torch.float32, seed=0):
    from cold_compress_amd.harness import ModelArgs, Transformer
    from cold_compress_amd.harness.model import CONFIGS

    torch.manual_seed(seed)
    return Transformer(ModelArgs(**CONFIGS["tiny"])).to(dtype).eval()


def test_handler_converts_every_linear_and_round_trips_the_state_dict():
    from cold_compress_amd.harness.quantize import (WeightOnlyMxfp4Linear, WeightOnlyMxfp4QuantHandler, check_mxfp4_state_dict,
                                                    dequantize_mxfp4, is_int4_linear, is_mxfp4_linear)

    model = _tiny(torch.bfloat16)
    linears = [n for n, m in model.named_modules() if isinstance(m, nn.Linear)]
    assert "output" in linears and len(linears) == 1 + 5 * model.config.n_layer
    sd = WeightOnlyMxfp4QuantHandler(model).create_quantized_state_dict()
    for n in linears:
        lin = model.get_submodule(n)
        assert sd[f"{n}.weight"].dtype == torch.uint8 and tuple(sd[f"{n}.weight"].shape) == (lin.out_features, lin.in_features // 2)
        assert sd[f"{n}.block_scales"].dtype == torch.uint8
        assert tuple(sd[f"{n}.block_scales"].shape) == (lin.out_features, lin.in_features // 32)
        assert 7 <= int(sd[f"{n}.block_scales"].min()) and int(sd[f"{n}.block_scales"].max()) <= 247
    assert sd["tok_embeddings.weight"].dtype == torch.bfloat16
    conv = WeightOnlyMxfp4QuantHandler(_tiny(torch.bfloat16)).convert_for_runtime()
    for n in linears:
        m = conv.get_submodule(n)
        assert isinstance(m, WeightOnlyMxfp4Linear) and is_mxfp4_linear(m) and not is_int4_linear(m), n
    assert isinstance(conv.tok_embeddings, nn.Embedding)
    assert set(conv.state_dict()) == set(sd)
    assert all(k.endswith((".weight", ".block_scales", ".bias")) for k in sd)
    check_mxfp4_state_dict(conv, sd)
    conv.load_state_dict(sd)
    back = conv.state_dict()
    for k, v in sd.items():
        assert back[k].dtype == v.dtype and torch.equal(back[k], v), k
    # the module formula: F.linear(x, bf16(dequantised W))
    x = torch.randn(3, 64).to(torch.bfloat16)
    with torch.no_grad():
        y = conv.output(x)
    want = torch.nn.functional.linear(x, dequantize_mxfp4(sd["output.weight"], sd["output.block_scales"]).to(torch.bfloat16))
    assert y.dtype == torch.bfloat16 and torch.equal(y, want)
    # `.to(dtype)` keeps the uint8 buffers
    conv = conv.to(torch.bfloat16)
    assert conv.output.weight.dtype == torch.uint8 and conv.output.block_scales.dtype == torch.uint8


def test_module_refuses_in_features_not_a_multiple_of_32():
    from cold_compress_amd.harness.quantize import WeightOnlyMxfp4Linear, WeightOnlyMxfp4QuantHandler, quantize_mxfp4

    with pytest.raises(ValueError, match="multiple of 32"):
        WeightOnlyMxfp4Linear(48, 32)
    with pytest.raises(ValueError, match="multiple of"):
        WeightOnlyMxfp4QuantHandler(nn.Sequential(nn.Linear(48, 8))).create_quantized_state_dict()
    with pytest.raises(ValueError):
        quantize_mxfp4(torch.zeros(4, 48))


def _quantize_cli(d, *extra):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "cold_compress_amd.harness.quantize", "--checkpoint_path", str(d / "model.pth"),
                           "--mode", "mxfp4", *extra], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)


def test_quantize_cli_and_load_model(tmp_path):
    from cold_compress_amd.harness import load_model
    from cold_compress_amd.harness.quantize import WeightOnlyMxfp4Linear, WeightOnlyMxfp4QuantHandler

    d = tmp_path / "tiny"
    d.mkdir()
    model = _tiny(torch.bfloat16, seed=3)
    torch.save(model.state_dict(), str(d / "model.pth"))
    r = _quantize_cli(d)
    assert r.returncode == 0, r.stderr
    assert (d / "model_mxfp4.pth").is_file()
    sd_file = torch.load(str(d / "model_mxfp4.pth"), weights_only=True)
    sd_handler = WeightOnlyMxfp4QuantHandler(_tiny(torch.bfloat16, seed=3)).create_quantized_state_dict()
    assert set(sd_file) == set(sd_handler)
    for k, v in sd_handler.items():
        assert torch.equal(sd_file[k], v), k
    m4 = load_model(d / "model_mxfp4.pth", "cpu", torch.bfloat16, False)
    assert isinstance(m4.output, WeightOnlyMxfp4Linear) and isinstance(m4.layers[0].attention.wqkv, WeightOnlyMxfp4Linear)
    assert m4.tok_embeddings.weight.dtype == torch.bfloat16 and m4.output.block_scales.dtype == torch.uint8
    back = m4.state_dict()
    for k, v in sd_handler.items():
        assert back[k].dtype == v.dtype and torch.equal(back[k], v), k


def test_load_model_refusals(tmp_path):
    from cold_compress_amd import _abi
    from cold_compress_amd.harness import load_model
    from cold_compress_amd.harness.quantize import WeightOnlyMxfp4QuantHandler

    d = tmp_path / "tiny"
    d.mkdir()
    path = d / "model_mxfp4.pth"
    sd = WeightOnlyMxfp4QuantHandler(_tiny(torch.bfloat16, seed=4)).create_quantized_state_dict()
    torch.save(sd, str(path))
    load_model(path, "cpu", torch.bfloat16, False)
    for prec in (torch.float16, torch.float32):
        with pytest.raises(_abi.ColdCompressError, match="bfloat16") as ei:
            load_model(path, "cpu", prec, False)
        assert str(path) in str(ei.value)
    bad = dict(sd)
    bad["output.block_scales"] = sd["output.block_scales"][:, :1].contiguous()  # a wrong shape
    torch.save(bad, str(path))
    with pytest.raises(_abi.ColdCompressError, match="block_scales") as ei:
        load_model(path, "cpu", torch.bfloat16, False)
    assert str(path) in str(ei.value)
    bad = dict(sd)
    bad["layers.0.attention.wo.weight"] = sd["layers.0.attention.wo.weight"].to(torch.int8)  # a wrong dtype
    torch.save(bad, str(path))
    with pytest.raises(_abi.ColdCompressError, match="wo.weight"):
        load_model(path, "cpu", torch.bfloat16, False)
    for byte in (3, 0xff):
        bad = dict(sd)
        bad["layers.1.feed_forward.w2.block_scales"] = sd["layers.1.feed_forward.w2.block_scales"].clone()
        bad["layers.1.feed_forward.w2.block_scales"][5, 2] = byte
        torch.save(bad, str(path))
        with pytest.raises(_abi.ColdCompressError, match=r"w2.block_scales.*\[7, 247\]") as ei:
            load_model(path, "cpu", torch.bfloat16, False)
        assert str(path) in str(ei.value)
    torch.save(sd, str(path))
    raw = path.read_bytes()
    path.write_bytes(raw[: len(raw) // 2])  # a truncated file
    with pytest.raises(_abi.ColdCompressError, match="mxfp4") as ei:
        load_model(path, "cpu", torch.bfloat16, False)
    assert str(path) in str(ei.value)
    path.write_bytes(b"")
    with pytest.raises(_abi.ColdCompressError, match="mxfp4"):
        load_model(path, "cpu", torch.bfloat16, False)


# ------------------------------------------------------------------------------------------------------------ the C ABI
def test_abi_row_and_argument_validation_without_gpu():
    from cold_compress_amd import _abi, _build

    header = open(os.path.join(ROOT, "include", "coldcompress.h")).read()
    m = re.search(r"^int cc_gemv_fused_mx4\(([^;]*)\);", header, re.M)
    assert m, "cc_gemv_fused_mx4 is not declared"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["const uint8_t* W", "const uint8_t* scales", "const uint8_t* W3", "const uint8_t* scales3", "const void* x",
                    "const void* delta", "const void* norm_w", "float eps", "void* h_out", "const void* bias", "const void* freqs",
                    "int32_t rope_rows", "int32_t head_dim", "void* y", "int32_t N", "int32_t K", "int32_t dtype", "cc_stream_t stream"]
    res, argtypes = _abi.SIGNATURES["cc_gemv_fused_mx4"]
    ctype = {"float": C.c_float, "int32_t": C.c_int32}
    want = [C.c_void_p if ("*" in a or a.startswith("cc_stream_t")) else ctype[a.split()[0]] for a in args]
    assert res is C.c_int and argtypes == want
    assert "cc_gemv_fused_mx4" in _abi.DEVICE_ONLY
    assert "cc_gemv_mx4.hip" in _build.SOURCES
    fns = _abi.bind(C.CDLL(_build.build()))
    f = fns["cc_gemv_fused_mx4"]
    p = C.c_void_p(0x1000)  # never dereferenced: validation happens before any launch
    BAD, UNS = -1, -2
    call = lambda **k: f(*[k.get(n, d) for n, d in (  # noqa: E731
        ("W", p), ("s", p), ("W3", None), ("s3", None), ("x", p), ("delta", None), ("nw", None), ("eps", 1e-5), ("h", None),
        ("bias", None), ("freqs", None), ("rr", 0), ("hd", 0), ("y", p), ("N", 64), ("K", 256), ("dt", _abi.CC_DT_BF16), ("st", None))])
    assert call(W=None) == BAD and call(s=None) == BAD and call(x=None) == BAD and call(y=None) == BAD
    assert call(N=0) == BAD and call(K=-32) == BAD and call(dt=7) == BAD
    assert call(W3=p) == BAD and call(s3=p) == BAD          # W3 and scales3 go together
    assert call(delta=p) == BAD and call(h=p) == BAD        # the residual needs the norm prologue
    assert call(W3=p, s3=p, bias=p) == BAD
    assert call(freqs=p, rr=96, hd=32) == BAD and call(freqs=p, W3=p, s3=p, rr=64, hd=32) == BAD
    odd16, odd2 = C.c_void_p(0x1008), C.c_void_p(0x1001)    # misaligned for a 16-byte / a 2-byte access
    assert call(W=odd16) == BAD and call(x=odd16) == BAD and call(W3=odd16, s3=p) == BAD
    assert call(nw=odd16) == BAD and call(nw=p, delta=odd16) == BAD and call(nw=p, h=odd16) == BAD
    assert call(y=odd2) == BAD and call(bias=odd2) == BAD and call(freqs=odd2, rr=64, hd=32) == BAD
    assert call(s=odd2) != BAD                               # scale bytes are read one at a time
    assert call(K=48) == UNS                                 # K % 32
    assert call(K=32800) == UNS                              # K * 2 > 64 KiB
    assert call(dt=_abi.CC_DT_F16) == UNS and call(dt=_abi.CC_DT_F32) == UNS  # bf16 only


def test_glue_refusals():
    from cold_compress_amd import _abi
    from cold_compress_amd.harness import glue

    w = torch.zeros(8, 32, dtype=torch.uint8)
    x = torch.zeros(64, dtype=torch.bfloat16)
    sc = torch.full((8, 2), 127, dtype=torch.uint8)
    with pytest.raises(_abi.ColdCompressError, match="block scales"):
        glue.gemv_fused(w, x)                                               # no scales at all
    with pytest.raises(_abi.ColdCompressError, match="scales3"):
        glue.gemv_fused(w, x, w3=w, scales=sc)                              # the pair without its second scales
    for xx in (x.half(), x.float()):
        with pytest.raises(_abi.ColdCompressError, match="bf16 activations"):
            glue.gemv_fused(w, xx, scales=sc)
    with pytest.raises(_abi.ColdCompressError, match=r"contiguous uint8 \[8, K / 32\]"):
        glue.gemv_fused(w, x, scales=torch.full((2, 8), 127, dtype=torch.uint8))
    with pytest.raises(_abi.ColdCompressError, match="contiguous uint8"):
        glue.gemv_fused(w, x, scales=torch.full((8, 4), 127, dtype=torch.uint8)[:, ::2])
    # the int4 branch is where it was: bf16 pairs without a groupsize
    with pytest.raises(_abi.ColdCompressError, match="groupsize"):
        glue.gemv_fused(w, x, scales=torch.zeros(8, 2, 2, dtype=torch.bfloat16))


def test_model_quant_arguments_tell_mxfp4_from_int4():
    from cold_compress_amd.harness.model import _quant
    from cold_compress_amd.harness.quantize import WeightOnlyInt4Linear, WeightOnlyInt8Linear, WeightOnlyMxfp4Linear

    m = WeightOnlyMxfp4Linear(64, 8)
    assert set(_quant(m)) == {"scales"} and _quant(m)["scales"] is m.block_scales
    assert set(_quant(m, "3")) == {"scales3"}
    m4 = WeightOnlyInt4Linear(64, 8, groupsize=32)
    assert _quant(m4) == {"scales": m4.scales_and_zeros, "groupsize": 32}
    assert set(_quant(WeightOnlyInt8Linear(64, 8))) == {"scales"} and _quant(nn.Linear(64, 8)) == {}


# ------------------------------------------------------------------------------------------------------- tensor parallelism
TP_TOL_ULPS = 8


def _worker_mx4(rank, world, port, q):
    try:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK=str(rank), LOCAL_WORLD_SIZE=str(world))
        import torch.distributed as dist

        import cold_compress_amd.harness.model as hm
        from cold_compress_amd import tp
        from cold_compress_amd.harness import ModelArgs, Transformer
        from cold_compress_amd.harness.quantize import WeightOnlyMxfp4QuantHandler
        from test_w8_host import _attention_double, _FullCacheDouble

        torch.set_num_threads(1)
        assert tp.maybe_init_dist() == rank and dist.get_backend() == "gloo"
        hm.scaled_dot_product_attention = _attention_double
        import host_glue

        host_glue.install(hm.glue)
        torch.manual_seed(0)
        cfg = dict(block_size=64, vocab_size=64, n_layer=2, n_head=32, n_local_heads=8, dim=256, intermediate_size=512, attention_bias=True)
        dense = Transformer(ModelArgs(**cfg)).to(torch.bfloat16).eval()
        sd = WeightOnlyMxfp4QuantHandler(dense).create_quantized_state_dict()
        full = WeightOnlyMxfp4QuantHandler(Transformer(ModelArgs(**cfg))).convert_for_runtime().to(torch.bfloat16).eval()
        sharded = WeightOnlyMxfp4QuantHandler(Transformer(ModelArgs(**cfg))).convert_for_runtime().to(torch.bfloat16).eval()
        full.load_state_dict(sd)
        sharded.load_state_dict(sd)
        tp.apply_tp(sharded)
        for m in (full, sharded):
            m.freqs_cis = hm.precompute_freqs_cis(64, 8, 10000, torch.bfloat16)
            for layer in m.layers:
                layer.attention.kv_cache = _FullCacheDouble()
        a, ff = sharded.layers[0].attention, sharded.layers[0].feed_forward
        fa, fff = full.layers[0].attention, full.layers[0].feed_forward
        hq, hk = 32 // world, 8 // world
        assert a.wqkv.weight.dtype == torch.uint8 and a.wqkv.weight.shape == ((hq + 2 * hk) * 8, 128)
        assert a.wqkv.block_scales.dtype == torch.uint8 and a.wqkv.block_scales.shape == ((hq + 2 * hk) * 8, 256 // 32)
        assert torch.equal(a.wqkv.block_scales[: hq * 8], fa.wqkv.block_scales[rank * hq * 8:(rank + 1) * hq * 8])
        kv0 = 256 + rank * hk * 8
        assert torch.equal(a.wqkv.weight[hq * 8:(hq + hk) * 8], fa.wqkv.weight[kv0:kv0 + hk * 8])
        assert torch.equal(a.wqkv.block_scales[hq * 8:(hq + hk) * 8], fa.wqkv.block_scales[kv0:kv0 + hk * 8])
        assert torch.equal(a.wqkv.bias[: hq * 8], fa.wqkv.bias[rank * hq * 8:(rank + 1) * hq * 8])
        per = 256 // world
        assert a.wo.weight.shape == (256, per // 2) and a.wo.in_features == per
        assert torch.equal(a.wo.weight, fa.wo.weight[:, rank * per // 2:(rank + 1) * per // 2])
        assert torch.equal(a.wo.block_scales, fa.wo.block_scales[:, rank * per // 32:(rank + 1) * per // 32])
        assert torch.equal(ff.w1.block_scales, fff.w1.block_scales[rank * 512 // world:(rank + 1) * 512 // world])
        assert ff.w2.weight.shape == (256, 512 // world // 2) and ff.w2.block_scales.shape == (256, 512 // world // 32)
        assert a.wo.weight.is_contiguous() and a.wo.block_scales.is_contiguous()
        idx = torch.arange(12).view(1, 12) % 64
        pos = torch.arange(12)
        with torch.no_grad():
            y_full = full(idx, pos, is_prefill=True).float()
            y_tp = sharded(idx, pos, is_prefill=True).float()
        q.put((rank, (y_full - y_tp).abs().max().item(), y_full.abs().max().item()))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:  # pragma: no cover
        q.put((rank, repr(e), None))
        raise


def test_tp_gloo_mxfp4_matches_single_process():
    """Column-wise MXFP4 linears split the code rows and the scale rows (wqkv per q / k / v block); row-wise ones split the code
    bytes and the scale columns.  The sharded bf16 model's logits equal the unsharded one's within TP_TOL_ULPS bf16 ulps of the
    largest logit (the int4 TP test's bound: the row-wise partial sums round to bf16 before the all-reduce, two layers deep)."""
    from test_w8_host import _free_port

    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker_mx4, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=180) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    for rank, err, scale in res:
        assert isinstance(err, float), f"rank {rank}: {err}"
        assert err <= TP_TOL_ULPS * 2.0 ** -8 * scale, f"rank {rank}: MXFP4 TP logits differ from the single-process model's by {err}"


def test_tp_refuses_a_rowwise_shard_that_splits_a_block(monkeypatch):
    from cold_compress_amd import _abi, tp
    from cold_compress_amd.harness.quantize import WeightOnlyMxfp4Linear

    lin = WeightOnlyMxfp4Linear(64, 16)
    monkeypatch.setattr(tp, "_world_rank", lambda: (4, 0))  # 64 / 4 = 16 input features per rank, half a block
    with pytest.raises(_abi.ColdCompressError, match="multiple of the block of 32"):
        tp._apply_tp_linear(lin, "rowwise")
    lin = WeightOnlyMxfp4Linear(128, 16)
    lin.weight.zero_()
    lin.block_scales.fill_(127)
    tp._apply_tp_linear(lin, "rowwise")  # 32 per rank: whole blocks
    assert lin.in_features == 32 and lin.weight.shape == (16, 16) and lin.block_scales.shape == (16, 1)


# ------------------------------------------------------------------------------------------------------- accuracy record
def test_accuracy_record_against_int4(capsys):
    """Round-trip RMS error on 4096 rows of N(0, 0.02) (K = 256), three seeds, MXFP4 against int4 G = 32 and G = 128: measured 1.51x
    and 1.18x (a power-of-two scale and 15 unevenly spaced levels against an fitted (scale, zero) pair and 16 even ones; DESIGN
    §2.9 quotes them).  Asserted: the two by-construction bounds, and that a row with one outlier x 50 reconstructs better under
    MXFP4, whose block of 32 confines the outlier, than under int4 G = 128 (measured on 64 rows of 128 columns: RMS 0.0128 against 0.0240)."""
    from cold_compress_amd.harness.quantize import dequantize_int4, group_quantize_int4, pack_int4, quantize_mxfp4

    def rms(a, b):
        return float((a.double() - b.double()).pow(2).mean().sqrt())

    def int4(w, G):
        q, s, z = group_quantize_int4(w, G)
        return dequantize_int4(pack_int4(q), torch.stack([s, z], -1), G)

    rows = []
    for seed in (0, 1, 2):
        g = torch.Generator().manual_seed(seed)
        w = (torch.randn(4096, 256, generator=g) * 0.02).to(torch.bfloat16)
        dq = _bounds(w.float(), *quantize_mxfp4(w))
        rows.append((seed, rms(w, dq), rms(w, int4(w, 32)), rms(w, int4(w, 128))))
    g = torch.Generator().manual_seed(5)
    w = (torch.randn(64, 128, generator=g) * 0.02).to(torch.bfloat16)
    w[:, 7] *= 50
    out_mx, out_i4 = rms(w, _bounds(w.float(), *quantize_mxfp4(w))), rms(w, int4(w, 128))
    with capsys.disabled():
        print("\nround-trip RMS error, N(0, 0.02): seed, MXFP4, int4 G=32, int4 G=128, MXFP4 / G=32, MXFP4 / G=128")
        for seed, m, a, b in rows:
            print(f"  {seed}  {m:.6f}  {a:.6f}  {b:.6f}  {m / a:.3f}  {m / b:.3f}")
        print(f"  one outlier x 50 per 128-column row: MXFP4 {out_mx:.5f}, int4 G=128 {out_i4:.5f}")
    assert out_mx < out_i4


# ------------------------------------------------------------------------------------------------------- the launcher mirror
def _switch_keys():
    src = open(os.path.join(ROOT, "cold_compress_amd", "csrc", "cc_gemv_mx4.hip")).read()
    keys = set()
    for sw, ws, xs, rb, cu in re.findall(r"MX4_CASE\((true|false), (\d+), (\d+), (\d+), (\d+)\)", src):
        keys.add((100000 if sw == "true" else 0) + int(ws) * 10000 + int(xs) * 1000 + int(rb) * 10 + int(cu))
    return src, keys


def test_exact_cases_reach_every_default_instantiation_of_the_launcher_switch():
    src, keys = _switch_keys()
    assert "case (SW ? 100000 : 0) + WS_ * 10000 + XS_ * 1000 + RB_ * 10 + CU_:" in src and len(keys) >= 30
    flat = " ".join(src.split())
    for line in X.MIRRORED_LINES:  # geometry() copies these lines: when one changes, update the mirror, DEFAULT_KEYS and the cases
        assert " ".join(line.split()) in flat, f"cc_gemv_mx4.hip no longer contains: {line}"
    got = {X.geometry(pair, N, K).key for K in range(32, 32768 + 1, 32) for pair in (False, True) for N in (1, 32768)}
    assert got == X.DEFAULT_KEYS
    assert X.DEFAULT_KEYS <= keys, X.DEFAULT_KEYS - keys  # every one of them is a case of the switch
    assert X.case_keys() == X.DEFAULT_KEYS
    # ... each with two rounds of the row loop, and every form at every waves-per-row split
    cases = X.gpu_cases()
    two = {X.geometry("pair" in f, N, K).key for (_, N, K, f, _) in cases if N == (lambda g: g.cap * g.rows + 1)(X.geometry("pair" in f, 1, K))}
    assert two == X.DEFAULT_KEYS
    assert {(X.geometry("pair" in f, N, K).ws, f) for (_, N, K, f, _) in cases} == {(ws, f) for ws in (1, 2, 4)
                                                                                  for f in X.PLAIN_FORMS + X.PAIR_FORMS}
    assert any(N == 38 for (_, N, _, _, _) in cases)


def test_exact_cases_keep_their_guarantees_and_match_the_contract_formula():
    """A sample of the GPU file's cases (every K below 8192 would cost minutes on the CPU: the small and the edge ones): make_case
    asserts every guarantee; here the expected y / h_out are compared bit for bit with the float64 contract formula on
    harness/quantize.py's dequantised weights."""
    from cold_compress_amd.harness.quantize import dequantize_mxfp4

    r = lambda t: t.to(torch.bfloat16).double()  # noqa: E731
    for (cid, N, K, form, seed) in [c for c in X.gpu_cases() if c[1] <= 64 and c[2] <= 8224]:
        c = X.make_case(N, K, form, seed)
        assert (np.abs(c.acc) < 256).all() and (c.abs_sum < 2 ** 24).all(), cid
        assert int(c.scales.min()) >= 128
        xf = c.x.double()
        h = None
        if c.norm:
            h = r(xf + c.delta_t.double()) if c.delta else xf
            xin = r(r(h * torch.rsqrt((h * h).mean())) * c.nw.double())
        else:
            xin = xf
        t = r(dequantize_mxfp4(c.W, c.scales).double() @ xin)
        if c.bias is not None:
            t = r(t + c.bias.double())
        if c.pair:
            t = r(r(torch.nn.functional.silu(t)) * r(dequantize_mxfp4(c.W3, c.scales3).double() @ xin))
        if c.freqs is not None:
            fq = c.freqs.double().view(-1, 2)
            rr = t[:c.rope_rows].view(-1, c.hd // 2, 2)
            cs, sn = fq[:, 0].view(1, -1), fq[:, 1].view(1, -1)
            out = torch.stack([rr[..., 0] * cs - rr[..., 1] * sn, rr[..., 1] * cs + rr[..., 0] * sn], -1).reshape(-1)
            t = torch.cat([r(out), t[c.rope_rows:]])
        assert torch.equal(X.bits(t.to(torch.bfloat16)), X.bits(c.y)), cid
        if c.norm:
            assert torch.equal(X.bits(h.to(torch.bfloat16)), X.bits(c.h)), cid


def test_a_corrupted_weight_changes_the_exact_answer():
    """what the random-data tolerance cannot see: one zeroed code, one swapped nibble pair, the neighbouring block's scale."""
    c = X.make_case(16, 4096, "plain", seed=31)
    base, _ = X.dot_exact(c.codes, c.sbytes, c.xin)
    k = int(np.nonzero((c.xin != 0) & ((c.codes[3] & 7) != 0))[0][-1])
    codes = c.codes.copy()
    codes[3, k] = 0
    assert X.dot_exact(codes, c.sbytes, c.xin)[0][3] != base[3]
    j = next(j for j in range(40, 2000) if c.xin[2 * j] != c.xin[2 * j + 1] and (c.codes[5, 2 * j] & 7) != (c.codes[5, 2 * j + 1] & 7))
    codes = c.codes.copy()
    codes[5, 2 * j], codes[5, 2 * j + 1] = c.codes[5, 2 * j + 1], c.codes[5, 2 * j]
    assert X.dot_exact(codes, c.sbytes, c.xin)[0][5] != base[5]
    b = next(b for b in range(1, 127) if c.sbytes[6, b] != c.sbytes[6, b + 1])
    sb = c.sbytes.copy()
    sb[6, b] = c.sbytes[6, b + 1]
    moved = X.dot_exact(c.codes, sb, c.xin)[0][6] != base[6]
    assert moved or not (X.weights_int(c.codes[6:7, 32 * b:32 * b + 32], c.sbytes[6:7, b:b + 1]) @ c.xin[32 * b:32 * b + 32]).any()
