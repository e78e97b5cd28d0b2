"""Weight-only int4 models on the host side (no GPU): the quantiser against the reference's recorded output
(tests/golden/w4_quant_ref.npz, written by tools/gen_w4_golden.py) bit for bit at G = 32, 64, 128 and 256, the module forward
against the reference's CPU int4 kernel, the handler's module conversion, state-dict keys and layout round trip, the quantise CLI
and `harness.load_model` (and what it refuses), the C ABI row and argument validation of cc_gemv_fused_w4, and tensor
parallelism of an int4 model over gloo at world 2 and 4."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "w4_quant_ref.npz")
GS = (32, 64, 128, 256)


def _golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("G", GS)
def test_quantiser_matches_reference_fixture_bit_for_bit(G):
    from cold_compress_amd.harness.quantize import WeightOnlyInt4QuantHandler, unpack_int4

    g = _golden()
    w = torch.from_numpy(g[f"w_g{G}"]).to(torch.bfloat16)
    N, K = w.shape
    lin = nn.Linear(K, N, bias=False).to(torch.bfloat16)
    with torch.no_grad():
        lin.weight.copy_(w)
    sd = WeightOnlyInt4QuantHandler(nn.Sequential(lin), G).create_quantized_state_dict()
    assert sd["0.weight"].dtype == torch.uint8 and tuple(sd["0.weight"].shape) == (N, K // 2)
    assert sd["0.scales_and_zeros"].dtype == torch.bfloat16 and tuple(sd["0.scales_and_zeros"].shape) == (K // G, N, 2)
    assert np.array_equal(unpack_int4(sd["0.weight"]).numpy(), g[f"q_g{G}"].astype(np.int32))
    assert np.array_equal(sd["0.scales_and_zeros"].float().numpy(), g[f"sz_g{G}"])
    # the packing: column 2j in the low nibble of byte j
    q = g[f"q_g{G}"]
    assert np.array_equal(sd["0.weight"].numpy(), (q[:, 0::2] | (q[:, 1::2] << 4)).astype(np.uint8))
    # the edge groups are really there: all zero (the clamped scale), range 15 (scale 1, zero 0.5: .5 ties), negative only
    sz = g[f"sz_g{G}"]
    assert 0 < sz[0, 0, 0] < 1e-6
    assert sz[0, 3, 0] == 1.0 and sz[0, 3, 1] == 0.5
    assert (sz[:, 4, 1] < 0).all()


@pytest.mark.parametrize("G", GS)
def test_dequantiser_matches_reference_fixture(G):
    from cold_compress_amd.harness.quantize import dequantize_int4, pack_int4

    g = _golden()
    q = torch.from_numpy(g[f"q_g{G}"].astype(np.int32))
    sz = torch.from_numpy(g[f"sz_g{G}"]).to(torch.bfloat16).transpose(0, 1).contiguous()
    w = dequantize_int4(pack_int4(q), sz, G)
    assert w.dtype == torch.float32
    assert np.array_equal(w.numpy(), g[f"wdq_g{G}"])


@pytest.mark.parametrize("G", GS)
def test_int4_linear_forward_matches_reference_cpu_kernel(G):
    """forward = F.linear(x, bf16(dequantised W)) against _weight_int4pack_mm_for_cpu (which does not round the weight): within 1
    bf16 ulp of the largest output."""
    from cold_compress_amd.harness.quantize import WeightOnlyInt4Linear, pack_int4

    g = _golden()
    q = torch.from_numpy(g[f"q_g{G}"].astype(np.int32))
    N, K = q.shape
    m = WeightOnlyInt4Linear(K, N, groupsize=G)
    m.load_state_dict({"weight": pack_int4(q), "scales_and_zeros": torch.from_numpy(g[f"sz_g{G}"]).to(torch.bfloat16)})
    with torch.no_grad():
        y = m(torch.from_numpy(g["x_bf16"]).to(torch.bfloat16))
    assert y.dtype == torch.bfloat16
    ref = g[f"y_g{G}"]
    ulp = 2.0 ** (np.floor(np.log2(np.abs(ref).max())) - 7)  # one bf16 ulp at the largest output
    assert np.abs(y.float().numpy() - ref).max() <= ulp


def _tiny(dtype=torch.float32, seed=0):
    from cold_compress_amd.harness import ModelArgs, Transformer
    from cold_compress_amd.harness.model import CONFIGS

    torch.manual_seed(seed)
    return Transformer(ModelArgs(**CONFIGS["tiny"])).to(dtype).eval()


def test_handler_converts_every_linear_and_round_trips_the_state_dict():
    from cold_compress_amd.harness.quantize import WeightOnlyInt4Linear, WeightOnlyInt4QuantHandler, is_int4_linear

    model = _tiny(torch.bfloat16)
    linears = [n for n, m in model.named_modules() if isinstance(m, nn.Linear)]
    assert "output" in linears and len(linears) == 1 + 5 * model.config.n_layer
    sd = WeightOnlyInt4QuantHandler(model, 32).create_quantized_state_dict()
    for n in linears:
        lin = model.get_submodule(n)
        assert sd[f"{n}.weight"].dtype == torch.uint8 and tuple(sd[f"{n}.weight"].shape) == (lin.out_features, lin.in_features // 2)
        assert tuple(sd[f"{n}.scales_and_zeros"].shape) == (lin.in_features // 32, lin.out_features, 2)
    assert sd["tok_embeddings.weight"].dtype == torch.bfloat16
    conv = WeightOnlyInt4QuantHandler(_tiny(torch.bfloat16), 32).convert_for_runtime()
    for n in linears:
        m = conv.get_submodule(n)
        assert isinstance(m, WeightOnlyInt4Linear) and is_int4_linear(m) and m.groupsize == 32, n
    assert isinstance(conv.tok_embeddings, nn.Embedding)
    assert set(conv.state_dict()) == set(sd)
    assert all(k.endswith((".weight", ".scales_and_zeros", ".bias")) for k in sd)
    conv.load_state_dict(sd)
    # held per row after the load; the state dict is the reference's layout again
    assert tuple(conv.output.scales_and_zeros.shape) == (conv.output.out_features, conv.output.in_features // 32, 2)
    assert torch.equal(conv.output.scales_and_zeros, sd["output.scales_and_zeros"].transpose(0, 1))
    back = conv.state_dict()
    for k, v in sd.items():
        assert back[k].dtype == v.dtype and torch.equal(back[k], v), k
    conv2 = WeightOnlyInt4QuantHandler(_tiny(torch.bfloat16), 32).convert_for_runtime()
    conv2.load_state_dict(back)
    x = torch.randn(1, 64).to(torch.bfloat16)
    with torch.no_grad():
        assert torch.equal(conv.output(x), conv2.output(x))


def test_module_refuses_in_features_not_a_multiple_of_the_groupsize():
    from cold_compress_amd.harness.quantize import WeightOnlyInt4Linear, WeightOnlyInt4QuantHandler

    with pytest.raises(ValueError, match="multiple of the groupsize"):
        WeightOnlyInt4Linear(96, 32, groupsize=64)
    with pytest.raises(ValueError):
        WeightOnlyInt4Linear(96, 32, groupsize=48)
    with pytest.raises(ValueError):
        WeightOnlyInt4QuantHandler(nn.Sequential(nn.Linear(64, 8)), 16)


def _quantize_cli(d, *extra):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "cold_compress_amd.harness.quantize", "--checkpoint_path", str(d / "model.pth"),
                           "--mode", "int4", *extra], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)


def test_quantize_cli_and_load_model(tmp_path):
    from cold_compress_amd.harness import load_model
    from cold_compress_amd.harness.quantize import WeightOnlyInt4Linear, WeightOnlyInt4QuantHandler

    d = tmp_path / "tiny"
    d.mkdir()
    model = _tiny(torch.bfloat16, seed=3)
    torch.save(model.state_dict(), str(d / "model.pth"))
    r = _quantize_cli(d)
    assert r.returncode != 0 and not list(d.glob("model_int4*"))  # --groupsize has no default
    r = _quantize_cli(d, "--groupsize", "32")
    assert r.returncode == 0, r.stderr
    assert (d / "model_int4.g32.pth").is_file()
    sd_file = torch.load(str(d / "model_int4.g32.pth"), weights_only=True)
    sd_handler = WeightOnlyInt4QuantHandler(_tiny(torch.bfloat16, seed=3), 32).create_quantized_state_dict()
    assert set(sd_file) == set(sd_handler)
    for k, v in sd_handler.items():
        assert torch.equal(sd_file[k], v), k
    m4 = load_model(d / "model_int4.g32.pth", "cpu", torch.bfloat16, False)
    assert isinstance(m4.output, WeightOnlyInt4Linear) and m4.output.groupsize == 32
    assert m4.tok_embeddings.weight.dtype == torch.bfloat16
    back = m4.state_dict()
    for k, v in sd_handler.items():
        assert back[k].dtype == v.dtype and torch.equal(back[k], v), k


def test_load_model_refusals(tmp_path):
    from cold_compress_amd import _abi
    from cold_compress_amd.harness import load_model
    from cold_compress_amd.harness.quantize import WeightOnlyInt4QuantHandler

    d = tmp_path / "tiny"
    d.mkdir()
    sd = WeightOnlyInt4QuantHandler(_tiny(torch.bfloat16, seed=4), 32).create_quantized_state_dict()
    torch.save(sd, str(d / "model_int4.g32.pth"))
    with pytest.raises(_abi.ColdCompressError, match="bfloat16"):
        load_model(d / "model_int4.g32.pth", "cpu", torch.float16, False)
    # the reference's tinygemm layout: int32 [N / 8, K / (inner_k_tiles * 16), 32, inner_k_tiles / 2]
    ref = dict(sd)
    n, k = sd["output.weight"].shape[0], sd["output.weight"].shape[1] * 2
    ref["output.weight"] = torch.zeros(n // 8, k // 128 or 1, 32, 4, dtype=torch.int32)
    torch.save(ref, str(d / "model_int4.g32.pth"))
    with pytest.raises(_abi.ColdCompressError, match="re-quantise"):
        load_model(d / "model_int4.g32.pth", "cpu", torch.bfloat16, False)
    # in_features % G != 0 (tiny's dim is 64; the name says G = 128)
    torch.save(sd, str(d / "model_int4.g128.pth"))
    with pytest.raises(_abi.ColdCompressError, match="multiple of the groupsize"):
        load_model(d / "model_int4.g128.pth", "cpu", torch.bfloat16, False)
    # a file whose (scale, zero) pairs are not the named groupsize's
    torch.save(sd, str(d / "model_int4.g64.pth"))
    with pytest.raises(_abi.ColdCompressError, match="scales_and_zeros"):
        load_model(d / "model_int4.g64.pth", "cpu", torch.bfloat16, False)
    # unreadable and empty files, a name without a groupsize
    (d / "model_int4.g32.pth").write_bytes(b"not a checkpoint")
    with pytest.raises(_abi.ColdCompressError, match="int4"):
        load_model(d / "model_int4.g32.pth", "cpu", torch.bfloat16, False)
    (d / "model_int4.g32.pth").write_bytes(b"")
    with pytest.raises(_abi.ColdCompressError, match="int4"):
        load_model(d / "model_int4.g32.pth", "cpu", torch.bfloat16, False)
    with pytest.raises(_abi.ColdCompressError, match="gG"):
        load_model(d / "model_int4.pth", "cpu", torch.bfloat16, False)


def test_abi_row_and_argument_validation_without_gpu():
    from cold_compress_amd import _abi, _build

    header = open(os.path.join(ROOT, "include", "coldcompress.h")).read()
    m = re.search(r"^int cc_gemv_fused_w4\(([^;]*)\);", header, re.M)
    assert m, "cc_gemv_fused_w4 is not declared"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 19 and args[0].startswith("const uint8_t*") and args[2].startswith("const uint8_t*")
    assert args[16] == "int32_t groupsize"
    res, argtypes = _abi.SIGNATURES["cc_gemv_fused_w4"]
    assert res is C.c_int and len(argtypes) == 19 and argtypes[7] is C.c_float
    assert "cc_gemv_fused_w4" in _abi.DEVICE_ONLY
    fns = _abi.bind(C.CDLL(_build.build()))
    f = fns["cc_gemv_fused_w4"]
    p = C.c_void_p(0x1000)  # never dereferenced: validation happens before any launch
    BAD, UNS = -1, -2
    call = lambda **k: f(*[k.get(n, d) for n, d in (  # noqa: E731
        ("W", p), ("s", p), ("W3", None), ("s3", None), ("x", p), ("delta", None), ("nw", None), ("eps", 1e-5), ("h", None),
        ("bias", None), ("freqs", None), ("rr", 0), ("hd", 0), ("y", p), ("N", 64), ("K", 256), ("G", 32), ("dt", _abi.CC_DT_BF16),
        ("st", None))])
    assert call(W=None) == BAD and call(s=None) == BAD and call(x=None) == BAD and call(y=None) == BAD
    assert call(N=0) == BAD and call(K=-32) == BAD and call(dt=7) == BAD
    assert call(W3=p) == BAD and call(s3=p) == BAD          # W3 and qparams3 go together: a pair with a null W3 is refused
    assert call(delta=p) == BAD and call(h=p) == BAD        # the residual needs the norm prologue
    assert call(W3=p, s3=p, bias=p) == BAD
    assert call(freqs=p, rr=96, hd=32) == BAD and call(freqs=p, W3=p, s3=p, rr=64, hd=32) == BAD
    for G in (0, 16, 48, 512, -32):
        assert call(G=G) == BAD, G                           # groupsize in {32, 64, 128, 256}
    assert call(K=96, G=64) == UNS                           # K % G
    assert call(K=32768 + 256, G=256) == UNS                 # K * 2 > 64 KiB
    assert call(dt=_abi.CC_DT_F16) == UNS and call(dt=_abi.CC_DT_F32) == UNS  # bf16 only


def test_glue_refuses_int4_calls_without_their_arguments():
    from cold_compress_amd import _abi
    from cold_compress_amd.harness import glue

    w = torch.zeros(8, 32, dtype=torch.uint8)
    x = torch.zeros(64, dtype=torch.bfloat16)
    with pytest.raises(_abi.ColdCompressError, match="groupsize"):
        glue.gemv_fused(w, x, scales=torch.zeros(8, 2, 2, dtype=torch.bfloat16))
    with pytest.raises(_abi.ColdCompressError, match="bf16"):
        glue.gemv_fused(w, x.half(), scales=torch.zeros(8, 2, 2, dtype=torch.bfloat16), groupsize=32)
    with pytest.raises(_abi.ColdCompressError, match="contiguous bf16"):
        glue.gemv_fused(w, x, scales=torch.zeros(2, 8, 2, dtype=torch.bfloat16), groupsize=32)


# ------------------------------------------------------------------------------------------------------- tensor parallelism
TP_TOL_ULPS = 8


def _worker_w4(rank, world, port, q):
    try:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK=str(rank), LOCAL_WORLD_SIZE=str(world))
        import torch.distributed as dist

        import cold_compress_amd.harness.model as hm
        from cold_compress_amd import tp
        from cold_compress_amd.harness import ModelArgs, Transformer
        from cold_compress_amd.harness.quantize import WeightOnlyInt4QuantHandler
        from test_w8_host import _attention_double, _FullCacheDouble

        torch.set_num_threads(1)
        assert tp.maybe_init_dist() == rank and dist.get_backend() == "gloo"
        hm.scaled_dot_product_attention = _attention_double
        import host_glue

        host_glue.install(hm.glue)
        torch.manual_seed(0)
        G = 32
        # the per-rank K of the row-wise linears (wo: 256 / world, w2: 512 / world) is a multiple of G at world 2 and 4
        cfg = dict(block_size=64, vocab_size=64, n_layer=2, n_head=32, n_local_heads=8, dim=256, intermediate_size=512, attention_bias=True)
        dense = Transformer(ModelArgs(**cfg)).to(torch.bfloat16).eval()
        sd = WeightOnlyInt4QuantHandler(dense, G).create_quantized_state_dict()
        full = WeightOnlyInt4QuantHandler(Transformer(ModelArgs(**cfg)), G).convert_for_runtime().to(torch.bfloat16).eval()
        sharded = WeightOnlyInt4QuantHandler(Transformer(ModelArgs(**cfg)), G).convert_for_runtime().to(torch.bfloat16).eval()
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
        assert a.wqkv.scales_and_zeros.shape == ((hq + 2 * hk) * 8, 256 // G, 2)
        assert torch.equal(a.wqkv.scales_and_zeros[: hq * 8], fa.wqkv.scales_and_zeros[rank * hq * 8:(rank + 1) * hq * 8])
        kv0 = 256 + rank * hk * 8
        assert torch.equal(a.wqkv.weight[hq * 8:(hq + hk) * 8], fa.wqkv.weight[kv0:kv0 + hk * 8])
        assert torch.equal(a.wqkv.bias[: hq * 8], fa.wqkv.bias[rank * hq * 8:(rank + 1) * hq * 8])
        per = 256 // world
        assert a.wo.weight.shape == (256, per // 2) and a.wo.in_features == per
        assert torch.equal(a.wo.weight, fa.wo.weight[:, rank * per // 2:(rank + 1) * per // 2])
        assert torch.equal(a.wo.scales_and_zeros, fa.wo.scales_and_zeros[:, rank * per // G:(rank + 1) * per // G])
        assert torch.equal(ff.w1.scales_and_zeros, fff.w1.scales_and_zeros[rank * 512 // world:(rank + 1) * 512 // world])
        assert ff.w2.weight.shape == (256, 512 // world // 2)
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


@pytest.mark.parametrize("world", [2, 4])
def test_tp_gloo_int4_matches_single_process(world):
    """Column-wise int4 linears split the code rows and the (scale, zero) rows (wqkv per q / k / v block); row-wise ones split the
    code bytes and the groups.  The sharded bf16 model's logits equal the unsharded one's within TP_TOL_ULPS bf16 ulps of the
    largest logit: the partial sums of the row-wise linears round to bf16 before the all-reduce, two layers deep."""
    from test_w8_host import _free_port

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker_w4, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=180) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    for rank, err, scale in res:
        assert isinstance(err, float), f"rank {rank}: {err}"
        assert err <= TP_TOL_ULPS * 2.0 ** -8 * scale, f"rank {rank}: int4 TP logits differ from the single-process model's by {err}"


def test_tp_refuses_a_rowwise_shard_that_splits_a_group(monkeypatch):
    from cold_compress_amd import _abi, tp
    from cold_compress_amd.harness.quantize import WeightOnlyInt4Linear

    lin = WeightOnlyInt4Linear(128, 16, groupsize=64)
    monkeypatch.setattr(tp, "_world_rank", lambda: (4, 0))  # 128 / 4 = 32 input features per rank, half a group
    with pytest.raises(_abi.ColdCompressError, match="multiple of the groupsize"):
        tp._apply_tp_linear(lin, "rowwise")
