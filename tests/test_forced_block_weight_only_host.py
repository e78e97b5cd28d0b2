"""`forced_block` for weight-only int8 and MXFP4 models, without a GPU: the two multi entry points' ABI rows
(cc_gemv_fused_w8_multi / cc_gemv_fused_mx4_multi) and their argument validation, Transformer.block_eligible's truth table with
`block_weight_only`, a teacher-forced generation in blocks of four over tests/cpu_twin.py against the token-by-token run on a fresh
model (Transformer.forward_block's row-by-row CPU twin, entered with T = 4), and glue.gemv_fused_multi's refusals."""
import argparse
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn as nn

from cpu_twin import cpu_twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = dict(block_size=256, vocab_size=128, n_layer=2, n_head=4, n_local_heads=2, dim=64, intermediate_size=128)  # K = 64 and 128
BF, HF, F32 = torch.bfloat16, torch.float16, torch.float32


class Tok:
    def special_ids(self):
        return [[1], [2, 3]]

    def punctuation_ids(self):
        return [5, 6, 7]


@pytest.fixture()
def twin(monkeypatch, oracle):
    with cpu_twin(monkeypatch, oracle) as fns:
        yield fns


# ------------------------------------------------------------------------------------------------ the ABI rows
NAMES = {"cc_gemv_fused_w8_multi": ("cc_gemv_fused_w8", "const int8_t*"), "cc_gemv_fused_mx4_multi": ("cc_gemv_fused_mx4", "const uint8_t*")}


def _decl(header, name):
    m = re.search(r"^int %s\(([^;]*)\);" % name, header, re.M)
    assert m, f"{name} is not declared in include/coldcompress.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", sorted(NAMES))
def test_header_signature_table_and_library_agree(name):
    from cold_compress_amd import _abi, _build

    single, wt = NAMES[name]
    header = open(os.path.join(ROOT, "include", "coldcompress.h")).read()
    args = _decl(header, name)
    # the single-vector entry point's arguments with T in front of dtype, where cc_gemv_fused_multi has it
    want_args = _decl(header, single)
    want_args.insert(len(want_args) - 2, "int32_t T")
    assert args == want_args and args[0] == wt + " W" and args[-3:] == ["int32_t T", "int32_t dtype", "cc_stream_t stream"]
    res, argtypes = _abi.SIGNATURES[name]
    ctype = {"float": C.c_float, "int32_t": C.c_int32}
    assert res is C.c_int and argtypes == [C.c_void_p if ("*" in a or a.startswith("cc_stream_t")) else ctype[a.split()[0]] for a in args]
    assert name in _abi.DEVICE_ONLY
    fns = _abi.bind(C.CDLL(_build.build()))
    assert name in fns


@pytest.mark.parametrize("name", sorted(NAMES))
def test_argument_validation_is_the_single_entry_points_plus_the_token_count(name):
    """Only argument sets that BOTH entry points reject before any launch are passed: the pointers are never dereferenced, on a machine
    with a GPU or without.  Every set must return CC_ERR_BAD_ARG or CC_ERR_UNSUPPORTED (a set that reached a launch would return
    CC_OK or CC_ERR_HIP and fails here), the multi entry point (with T = 2) the same code as the single-vector one; and T outside
    1 .. 4 is CC_ERR_BAD_ARG.  The single-vector entry point is never called with a set it accepts."""
    from cold_compress_amd import _abi, _build

    fns = _abi.bind(C.CDLL(_build.build()))
    multi, single = fns[name], fns[NAMES[name][0]]
    mx4 = name.endswith("mx4_multi")
    p = C.c_void_p(0x1000)
    BAD, UNS = -1, -2
    order = (("W", p), ("s", p), ("W3", None), ("s3", None), ("x", p), ("delta", None), ("nw", None), ("eps", 1e-5), ("h", None),
             ("bias", None), ("freqs", None), ("rr", 0), ("hd", 0), ("y", p), ("N", 64), ("K", 256))

    def head(k):
        return [k.get(n, d) for n, d in order], k.get("dt", _abi.CC_DT_BF16)

    # rejected by both kernels' entry points
    cases = [dict(W=None), dict(s=None), dict(x=None), dict(y=None), dict(N=0), dict(K=-32), dict(dt=7), dict(W3=p), dict(s3=p),
             dict(delta=p), dict(h=p), dict(W3=p, s3=p, bias=p), dict(freqs=p, rr=96, hd=32), dict(freqs=p, W3=p, s3=p, rr=64, hd=32),
             dict(K=40), dict(K=72), dict(K=32800), dict(K=65536), dict(dt=_abi.CC_DT_F32)]
    if mx4:  # whole MX blocks, bf16 only, and the alignment checks only this entry point makes
        odd16, odd2 = C.c_void_p(0x1008), C.c_void_p(0x1001)
        cases += [dict(K=48), dict(dt=_abi.CC_DT_F16), dict(W=odd16), dict(x=odd16), dict(W3=odd16, s3=p), dict(nw=odd16),
                  dict(nw=p, delta=odd16), dict(nw=p, h=odd16), dict(y=odd2), dict(bias=odd2), dict(freqs=odd2, rr=64, hd=32)]
    seen = set()
    for k in cases:
        a, dt = head(k)
        m = multi(*a, 2, dt, None)
        assert m in (BAD, UNS), f"{k}: the multi entry point returned {m}: this set is not rejected before a launch"
        s = single(*a, dt, None)
        assert s == m, (k, m, s)
        seen.add(m)
    assert seen == {BAD, UNS}
    a, dt = head({})  # a set both would accept: only the multi entry point sees it, with a token count it must refuse first
    for T in (0, 5, -1, 1 << 20):
        assert multi(*a, T, dt, None) == BAD, T
    a, dt = head(dict(K=40))  # a bad token count with an unsupported K is still a bad argument
    assert multi(*a, 0, dt, None) == BAD
    for k, want in ((dict(delta=p), BAD), (dict(K=40), UNS), (dict(dt=_abi.CC_DT_F32), UNS)):  # the three the GPU file names
        a, dt = head(k)
        assert multi(*a, 2, dt, None) == want, k


# ------------------------------------------------------------------------------------------------ models
def _dense(dtype, seed=0):
    from cold_compress_amd.harness import ModelArgs, Transformer

    torch.manual_seed(seed)
    return Transformer(ModelArgs(**TINY)).to(dtype).eval()


def _convert(mode, dtype, seed=0):
    """the tiny model quantised by the handler of `mode` (int8 / mxfp4 / int4), as tools/run_configs.py --weights does."""
    from cold_compress_amd.harness import ModelArgs, Transformer
    from cold_compress_amd.harness.quantize import WeightOnlyInt4QuantHandler, WeightOnlyInt8QuantHandler, WeightOnlyMxfp4QuantHandler

    if mode == "int4":
        make = lambda m: WeightOnlyInt4QuantHandler(m, groupsize=32)  # noqa: E731
    else:
        make = {"int8": WeightOnlyInt8QuantHandler, "mxfp4": WeightOnlyMxfp4QuantHandler}[mode]
    sd = make(_dense(dtype, seed)).create_quantized_state_dict()
    model = make(Transformer(ModelArgs(**TINY)).to(dtype)).convert_for_runtime()
    model.load_state_dict(sd, strict=True)
    return model.to(dtype).eval()


def _caches(model, strategy="heavy_hitter", max_seq=64, **cache_kw):
    import cold_compress_amd.cache as cache
    from cold_compress_amd.harness import setup_caches

    ap = argparse.ArgumentParser()
    cache.add_cache_arguments(ap)
    kw = vars(ap.parse_args([]))
    kw.update(dict(cache_strategy=[strategy], prompt_compression_strategy=[strategy], max_cache_length=[32.0], global_tokens=4,
                   recent_window=8), **cache_kw)
    setup_caches(model, Tok(), "cpu", max_seq, dict(kw))
    return model


# ------------------------------------------------------------------------------------------------ block_eligible
@pytest.mark.parametrize("mode", ["int8", "mxfp4"])
def test_block_eligible_truth_table_with_block_weight_only(twin, monkeypatch, mode):
    from cold_compress_amd.harness.quantize import WeightOnlyInt8Linear, is_int8_linear, is_mxfp4_linear

    m = _caches(_convert(mode, BF))
    assert m.block_weight_only is False
    check = is_int8_linear if mode == "int8" else is_mxfp4_linear
    assert all(check(x) for l in m.layers for x in (l.attention.wqkv, l.attention.wo, l.feed_forward.w1, l.feed_forward.w3, l.feed_forward.w2))
    assert check(m.output)
    assert not m.block_eligible(), "the default attribute keeps weight-only models on the per-token route"
    m.block_weight_only = True
    assert m.block_eligible() and m.block_eligible(1.0)
    # every condition of the dense table still holds
    assert not m.block_eligible(0.5), "attn_top_k < 1"
    m.layers[1].attention.fuse_qkv_step = True
    assert not m.block_eligible(), "the single-launch QKV step"
    m.layers[1].attention.fuse_qkv_step = False
    assert m.block_eligible()
    q = _caches(_convert(mode, BF), cache_bits=8)
    q.block_weight_only = True
    assert not q.block_eligible(), "--cache_bits 8 in reference mode"
    import cold_compress_amd.harness.generation as G

    monkeypatch.setattr(G, "_tp_world", lambda: 2)
    assert not m.block_eligible(), "world size 2"
    monkeypatch.setattr(G, "_tp_world", lambda: 1)
    assert m.block_eligible()
    # w1 quantised beside a dense w3
    m.layers[0].feed_forward.w3 = nn.Linear(64, 128, bias=False).to(BF)
    assert not m.block_eligible(), "w1 and w3 of different kinds"
    # ... while a dense linear elsewhere is fine (each linear is one of: dense, int8, MXFP4)
    m = _caches(_convert(mode, BF))
    m.block_weight_only = True
    m.layers[0].attention.wo = nn.Linear(64, 64, bias=False).to(BF)
    assert m.block_eligible(), "a dense wo in a weight-only model"
    # a bare int8 parameter on an nn.Linear carries no scales: not a weight-only module
    m.layers[0].attention.wo.weight = nn.Parameter(torch.zeros(64, 64, dtype=torch.int8), requires_grad=False)
    assert not m.block_eligible(), "bare int8 weights without scales"
    # activations the kernel does not serve
    f = _caches(_convert(mode, F32))
    f.block_weight_only = True
    assert not f.block_eligible(), "fp32 activations"
    if mode == "int8":
        h = _caches(_convert(mode, HF))
        h.block_weight_only = True
        assert h.block_eligible(), "int8 weights serve f16 activations"
        assert isinstance(h.output, WeightOnlyInt8Linear)
    # int4 linears have no multi GEMV, whatever the attribute says
    m4 = _caches(_convert("int4", BF))
    assert not m4.block_eligible()
    m4.block_weight_only = True
    assert not m4.block_eligible(), "an int4 model"
    m = _caches(_convert(mode, BF))
    m.block_weight_only = True
    from cold_compress_amd.harness.quantize import WeightOnlyInt4Linear

    m.layers[1].feed_forward.w2 = WeightOnlyInt4Linear(128, 64, groupsize=32)
    assert not m.block_eligible(), "one int4 linear"
    # the dense answers are what they were, with either value of the attribute
    d = _caches(_dense(F32))
    assert d.block_eligible()
    d.block_weight_only = True
    assert d.block_eligible()
    d.output.weight = nn.Parameter(torch.zeros(128, 32, dtype=torch.uint8), requires_grad=False)
    assert not d.block_eligible(), "a bare uint8 LM head"


# ------------------------------------------------------------------------------------------------ the route, on the CPU twin
NEXT = torch.tensor([9, 21, 6, 33, 47, 5, 60, 72, 7, 85, 99, 110, 14, 27], dtype=torch.int32)  # the prefill's token + 13 forced steps


def _generate(mode, forced_block, counts):
    from cold_compress_amd.harness import decode_one_token, generate, prefill

    model = _caches(_convert(mode, BF, seed=11))
    model.block_weight_only = True
    real = model.forward_block

    def counted(idx, input_pos, **k):
        counts.append(int(idx.shape[1]))
        return real(idx, input_pos, **k)

    model.forward_block = counted
    g = torch.Generator().manual_seed(3)
    prompt = torch.randint(8, 128, (40,), generator=g, dtype=torch.int32)
    seq, probs, _ = generate(model, prompt, prefill, decode_one_token, max_new_tokens=0, next_tokens=NEXT.clone(), forced_block=forced_block)
    state = {f"{li}.{n}": b.clone() for li, layer in enumerate(model.layers) for n, b in layer.attention.kv_cache._buffers.items()
             if b is not None}
    return seq, probs, state


@pytest.mark.parametrize("mode", ["int8", "mxfp4"])
def test_teacher_forced_blocks_of_a_weight_only_model_equal_single_steps(twin, mode):
    c4, c1 = [], []
    seq4, probs4, st4 = _generate(mode, 4, c4)
    seq1, probs1, st1 = _generate(mode, 1, c1)
    assert c4 == [4, 4, 4], f"forward_block was entered with {c4}"  # 13 forced steps: three blocks and a tail of one
    assert not c1
    assert torch.equal(seq4, seq1) and seq4[40:].tolist() == NEXT.tolist()
    assert len(probs4) == len(probs1) == 14 and all(torch.equal(a.float(), b.float()) for a, b in zip(probs4, probs1))
    assert st4.keys() == st1.keys() and st4
    for n in st4:
        assert torch.equal(st4[n].float() if st4[n].is_floating_point() else st4[n], st1[n].float() if st1[n].is_floating_point() else st1[n]), n


# ------------------------------------------------------------------------------------------------ glue refusals
def test_gemv_fused_multi_refusals_come_before_the_library(monkeypatch):
    from cold_compress_amd import _abi
    from cold_compress_amd.harness import glue

    def no_call(*a, **k):
        raise AssertionError("the library was called")

    monkeypatch.setattr(_abi, "call", no_call)
    x = torch.zeros(2, 64, dtype=BF)
    w4 = torch.zeros(8, 32, dtype=torch.uint8)
    pairs = torch.zeros(8, 2, 2, dtype=BF)
    with pytest.raises(_abi.ColdCompressError, match="int4"):
        glue.gemv_fused_multi(w4, x, scales=pairs)                       # int4: (scale, zero) pairs
    with pytest.raises(TypeError):
        glue.gemv_fused_multi(w4, x, scales=pairs, groupsize=32)         # what _quant() hands over for an int4 linear
    with pytest.raises(_abi.ColdCompressError, match="uint8 weights need"):
        glue.gemv_fused_multi(w4, x)                                     # uint8 codes without any scales
    w8 = torch.zeros(8, 64, dtype=torch.int8)
    with pytest.raises(_abi.ColdCompressError, match="per-row scales"):
        glue.gemv_fused_multi(w8, x)
    with pytest.raises(_abi.ColdCompressError, match="scales3"):
        glue.gemv_fused_multi(w8, x, w3=w8, scales=torch.ones(8, dtype=BF))
    with pytest.raises(_abi.ColdCompressError, match="w3 must have the shape"):
        glue.gemv_fused_multi(w8, x, w3=torch.zeros(4, 64, dtype=torch.int8), scales=torch.ones(8, dtype=BF), scales3=torch.ones(8, dtype=BF))
    with pytest.raises(_abi.ColdCompressError, match="one value per row"):
        glue.gemv_fused_multi(w8, x, scales=torch.ones(4, dtype=BF))
    with pytest.raises(_abi.ColdCompressError, match="16-bit activations"):
        glue.gemv_fused_multi(w8, x.float(), scales=torch.ones(8, dtype=BF))
    ok = torch.full((8, 2), 127, dtype=torch.uint8)
    with pytest.raises(_abi.ColdCompressError, match=r"contiguous uint8 \[8, K / 32\]"):
        glue.gemv_fused_multi(w4, x, scales=torch.full((2, 8), 127, dtype=torch.uint8))
    with pytest.raises(_abi.ColdCompressError, match="contiguous uint8"):
        glue.gemv_fused_multi(w4, x, scales=torch.full((8, 4), 127, dtype=torch.uint8)[:, ::2])
    with pytest.raises(_abi.ColdCompressError, match="scales3"):
        glue.gemv_fused_multi(w4, x, w3=w4, scales=ok)
    with pytest.raises(_abi.ColdCompressError, match="w3 must have the shape"):
        glue.gemv_fused_multi(w4, x, w3=torch.zeros(8, 16, dtype=torch.uint8), scales=ok, scales3=ok)
    for xx in (x.half(), x.float()):
        with pytest.raises(_abi.ColdCompressError, match="bf16 activations"):
            glue.gemv_fused_multi(w4, xx, scales=ok)
    with pytest.raises(_abi.ColdCompressError, match="takes? no scales"):
        glue.gemv_fused_multi(torch.zeros(8, 64, dtype=BF), x, scales=ok)
    # well-formed arguments on the CPU: the no-fallback refusal
    for w, kw in ((w8, dict(scales=torch.ones(8, dtype=BF))), (w4, dict(scales=ok)), (torch.zeros(8, 64, dtype=BF), {})):
        with pytest.raises(_abi.ColdCompressError, match="no CPU fallback"):
            glue.gemv_fused_multi(w, x, **kw)
