"""The int4 multi-vector route without a GPU: cc_gemv_fused_w4_multi's ABI row and argument validation, glue.gemv_fused_w4_multi's
refusals (all before the library is called), Transformer.block_eligible's truth table with `block_int4`, a teacher-forced generation
in blocks of four over tests/cpu_twin.py against the token-by-token run on a fresh model (Transformer.forward_block's row-by-row CPU
twin, entered with T = 4), and generate_streams on the twin taking the joint route."""
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
NAME, SINGLE = "cc_gemv_fused_w4_multi", "cc_gemv_fused_w4"


class Tok:
    def special_ids(self):
        return [[1], [2, 3]]

    def punctuation_ids(self):
        return [5, 6, 7]


@pytest.fixture()
def twin(monkeypatch, oracle):
    with cpu_twin(monkeypatch, oracle) as fns:
        yield fns


# ------------------------------------------------------------------------------------------------ the ABI row
def _decl(header, name):
    m = re.search(r"^int %s\(([^;]*)\);" % name, header, re.M)
    assert m, f"{name} is not declared in include/coldcompress.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_signature_table_and_library_agree():
    from cold_compress_amd import _abi, _build

    header = open(os.path.join(ROOT, "include", "coldcompress.h")).read()
    args = _decl(header, NAME)
    want_args = _decl(header, SINGLE)  # the single-vector entry point's arguments with T in front of dtype
    want_args.insert(len(want_args) - 2, "int32_t T")
    assert args == want_args and len(args) == 20
    assert args[0] == "const uint8_t* W" and args[-4:] == ["int32_t groupsize", "int32_t T", "int32_t dtype", "cc_stream_t stream"]
    res, argtypes = _abi.SIGNATURES[NAME]
    ctype = {"float": C.c_float, "int32_t": C.c_int32}
    assert res is C.c_int and argtypes == [C.c_void_p if ("*" in a or a.startswith("cc_stream_t")) else ctype[a.split()[0]] for a in args]
    assert NAME in _abi.DEVICE_ONLY
    assert header.index("int cc_gemv_fused_mx4_multi(") < header.index("int " + NAME + "(") < header.index("size_t cc_softmax_argmax_workspace_bytes")
    fns = _abi.bind(C.CDLL(_build.build()))
    assert NAME in fns


def test_argument_validation_is_the_single_entry_points_plus_the_token_count_and_alignment():
    """Only argument sets that are rejected before any launch are passed: the pointers are never dereferenced, on a machine with a GPU
    or without.  Sets both entry points reject return the same code from both; T outside 1 .. 4 is CC_ERR_BAD_ARG; the alignment
    conditions are the multi entry point's own."""
    from cold_compress_amd import _abi, _build

    fns = _abi.bind(C.CDLL(_build.build()))
    multi, single = fns[NAME], fns[SINGLE]
    p = C.c_void_p(0x1000)
    BAD, UNS = -1, -2
    order = (("W", p), ("s", p), ("W3", None), ("s3", None), ("x", p), ("delta", None), ("nw", None), ("eps", 1e-5), ("h", None),
             ("bias", None), ("freqs", None), ("rr", 0), ("hd", 0), ("y", p), ("N", 64), ("K", 256), ("G", 32))

    def head(k):
        return [k.get(n, d) for n, d in order], k.get("dt", _abi.CC_DT_BF16)

    cases = [dict(W=None), dict(s=None), dict(x=None), dict(y=None), dict(N=0), dict(K=-32), dict(dt=7), dict(W3=p), dict(s3=p),
             dict(delta=p), dict(h=p), dict(W3=p, s3=p, bias=p), dict(freqs=p, rr=96, hd=32), dict(freqs=p, W3=p, s3=p, rr=64, hd=32),
             dict(G=48), dict(G=16), dict(G=0), dict(G=512), dict(K=160, G=64), dict(K=384, G=256), dict(K=32800), dict(K=65536),
             dict(dt=_abi.CC_DT_F32), dict(dt=_abi.CC_DT_F16)]
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
    a, dt = head(dict(K=160, G=64))  # a bad token count with an unsupported K is still a bad argument
    assert multi(*a, 0, dt, None) == BAD
    for k, want in ((dict(delta=p), BAD), (dict(K=160, G=64), UNS), (dict(G=48), BAD), (dict(dt=_abi.CC_DT_F16), UNS)):  # the GPU file's four
        a, dt = head(k)
        assert multi(*a, 2, dt, None) == want, k
    # alignment: 16 bytes for W, W3, x, delta, norm_w and h_out, 4 for the (scale, zero) words — the multi entry point only
    odd16, odd4 = C.c_void_p(0x1008), C.c_void_p(0x1002)
    for k in (dict(W=odd16), dict(x=odd16), dict(W3=odd16, s3=p), dict(nw=odd16), dict(nw=p, delta=odd16), dict(nw=p, h=odd16),
              dict(s=odd4), dict(W3=p, s3=odd4)):
        a, dt = head(k)
        assert multi(*a, 2, dt, None) == BAD, k


# ------------------------------------------------------------------------------------------------ glue refusals
def test_gemv_fused_w4_multi_refusals_come_before_the_library(monkeypatch):
    from cold_compress_amd import _abi
    from cold_compress_amd.harness import glue

    def no_call(*a, **k):
        raise AssertionError("the library was called")

    monkeypatch.setattr(_abi, "call", no_call)
    f = glue.gemv_fused_w4_multi
    x = torch.zeros(2, 64, dtype=BF)
    w = torch.zeros(8, 32, dtype=torch.uint8)
    pairs = torch.zeros(8, 2, 2, dtype=BF)
    E = _abi.ColdCompressError
    with pytest.raises(E, match="uint8"):
        f(torch.zeros(8, 64, dtype=torch.int8), x, pairs, 32)
    with pytest.raises(E, match="uint8"):
        f(torch.zeros(8, 64, dtype=BF), x, pairs, 32)
    with pytest.raises(E, match="pairs and groupsize"):
        f(w, x, None, 32)
    with pytest.raises(E, match="pairs and groupsize"):
        f(w, x, pairs, None)
    with pytest.raises(E, match="scales3"):
        f(w, x, pairs, 32, w3=w)
    with pytest.raises(E, match="scales3"):
        f(w, x, pairs, 32, scales3=pairs)
    with pytest.raises(E, match="scales3"):
        f(w, x, pairs, 32, w3=torch.zeros(8, 32, dtype=torch.int8), scales3=pairs)
    with pytest.raises(E, match="groupsize must be"):
        f(w, x, pairs, 48)
    with pytest.raises(E, match="not a multiple of the groupsize"):
        f(w, x, torch.zeros(8, 0, 2, dtype=BF), 128)
    with pytest.raises(E, match="w3 must have the shape"):
        f(w, x, pairs, 32, w3=torch.zeros(8, 16, dtype=torch.uint8), scales3=pairs)
    with pytest.raises(E, match=r"contiguous bf16 \[8, K / 32, 2\]"):
        f(w, x, torch.zeros(8, 1, 2, dtype=BF), 32)                          # the pairs of G = 64
    with pytest.raises(E, match="contiguous bf16"):
        f(w, x, pairs.float(), 32)
    with pytest.raises(E, match="contiguous bf16"):
        f(w, x, torch.zeros(8, 2, 4, dtype=BF)[:, :, ::2], 32)
    with pytest.raises(E, match="contiguous bf16"):
        f(w, x, pairs, 32, w3=w, scales3=torch.zeros(2, 8, 2, dtype=BF))   # the state dict's [K / G, N, 2]
    for xx in (x.half(), x.float()):
        with pytest.raises(E, match="bf16 activations"):
            f(w, xx, pairs, 32)
    with pytest.raises(E, match=r"x must be \[T, 64\]"):
        f(w, x[0], pairs, 32)
    with pytest.raises(E, match=r"x must be \[T, 64\]"):
        f(w, torch.zeros(2, 32, dtype=BF), pairs, 32)
    with pytest.raises(E, match="1 <= T <= 4"):
        f(w, torch.zeros(5, 64, dtype=BF), pairs, 32)
    with pytest.raises(E, match="1 <= T <= 4"):
        f(w, torch.zeros(0, 64, dtype=BF), pairs, 32)
    nw = torch.ones(64, dtype=BF)
    with pytest.raises(E, match=r"delta must be \[2, 64\]"):
        f(w, x, pairs, 32, delta=torch.zeros(64, dtype=BF), norm_weight=nw)
    with pytest.raises(E, match=r"h_out must be \[2, 64\]"):
        f(w, x, pairs, 32, norm_weight=nw, h_out=torch.zeros(1, 64, dtype=BF))
    with pytest.raises(E, match=r"freqs must be \[2, 2, 2\]"):
        f(w, x, pairs, 32, freqs=torch.zeros(2, 2, dtype=BF), rope_rows=4, head_dim=4)
    with pytest.raises(E, match="h_out must be contiguous"):
        f(w, x, pairs, 32, norm_weight=nw, h_out=torch.zeros(2, 128, dtype=BF)[:, ::2])
    with pytest.raises(E, match="norm_weight must be bf16"):
        f(w, x, pairs, 32, norm_weight=nw.float())
    # well-formed arguments on the CPU: the no-fallback refusal
    with pytest.raises(E, match="no CPU fallback"):
        f(w, x, pairs, 32)
    with pytest.raises(E, match="no CPU fallback"):
        f(w, x, pairs, 32, w3=w, scales3=pairs, delta=x, norm_weight=nw, h_out=torch.zeros(2, 64, dtype=BF))
    # gemv_fused_multi keeps its refusals of int4 weights
    with pytest.raises(E, match="int4"):
        glue.gemv_fused_multi(w, x, scales=pairs)
    with pytest.raises(TypeError):
        glue.gemv_fused_multi(w, x, scales=pairs, groupsize=32)


def test_the_route_helper_sends_int4_linears_to_their_own_glue_function(monkeypatch):
    from cold_compress_amd.harness import glue, model as M
    from cold_compress_amd.harness.quantize import WeightOnlyInt4Linear, WeightOnlyInt8Linear

    seen = []
    monkeypatch.setattr(glue, "gemv_fused_w4_multi", lambda *a, **k: seen.append(("w4", a, k)))
    monkeypatch.setattr(glue, "gemv_fused_multi", lambda *a, **k: seen.append(("multi", a, k)))
    x = torch.zeros(2, 64, dtype=BF)
    l4, l4b = WeightOnlyInt4Linear(64, 8, groupsize=32), WeightOnlyInt4Linear(64, 8, groupsize=32)
    M._gemv_multi(l4, x, w3=l4b, delta=x)
    M._gemv_multi(nn.Linear(64, 8, bias=False).to(BF), x)
    M._gemv_multi(WeightOnlyInt8Linear(64, 8), x)
    (k0, a0, kw0), (k1, a1, kw1), (k2, a2, kw2) = seen
    assert k0 == "w4" and a0[0] is l4.weight and kw0["w3"] is l4b.weight and kw0["scales"] is l4.scales_and_zeros
    assert kw0["scales3"] is l4b.scales_and_zeros and kw0["groupsize"] == 32 and kw0["delta"] is x
    assert k1 == "multi" and "groupsize" not in kw1 and "scales" not in kw1
    assert k2 == "multi" and "scales" in kw2 and "groupsize" not in kw2


# ------------------------------------------------------------------------------------------------ models
def _dense(dtype, seed=0):
    from cold_compress_amd.harness import ModelArgs, Transformer

    torch.manual_seed(seed)
    return Transformer(ModelArgs(**TINY)).to(dtype).eval()


def _convert(mode, dtype, seed=0, groupsize=32):
    from cold_compress_amd.harness import ModelArgs, Transformer
    from cold_compress_amd.harness.quantize import WeightOnlyInt4QuantHandler, WeightOnlyInt8QuantHandler

    make = (lambda m: WeightOnlyInt4QuantHandler(m, groupsize=groupsize)) if mode == "int4" else WeightOnlyInt8QuantHandler
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
def test_block_eligible_truth_table_with_block_int4(twin, monkeypatch):
    from cold_compress_amd.harness.quantize import WeightOnlyInt4Linear, is_int4_linear

    m = _caches(_convert("int4", BF))
    assert m.block_int4 is False and m.block_weight_only is False
    assert all(is_int4_linear(x) for l in m.layers for x in (l.attention.wqkv, l.attention.wo, l.feed_forward.w1, l.feed_forward.w3, l.feed_forward.w2))
    assert is_int4_linear(m.output)
    assert not m.block_eligible(), "off: int4 is ineligible"
    m.block_weight_only = True
    assert not m.block_eligible(), "block_weight_only alone is still not enough"
    m.block_weight_only = False
    m.block_int4 = True
    assert m.block_eligible() and m.block_eligible(1.0), "on: eligible"
    m.block_weight_only = True
    assert m.block_eligible(), "both attributes"
    m.block_weight_only = False
    # every other condition of the table still holds
    assert not m.block_eligible(0.5), "attn_top_k < 1"
    m.layers[1].attention.fuse_qkv_step = True
    assert not m.block_eligible(), "the single-launch QKV step"
    m.layers[1].attention.fuse_qkv_step = False
    assert m.block_eligible()
    q = _caches(_convert("int4", BF), cache_bits=8)
    q.block_int4 = True
    assert not q.block_eligible(), "--cache_bits 8 in reference mode"
    import cold_compress_amd.harness.generation as G

    monkeypatch.setattr(G, "_tp_world", lambda: 2)
    assert not m.block_eligible(), "world size 2"
    monkeypatch.setattr(G, "_tp_world", lambda: 1)
    assert m.block_eligible()
    # fp32 activations
    f = _caches(_convert("int4", BF))
    f.tok_embeddings.to(F32)
    f.block_int4 = True
    assert not f.block_eligible(), "fp32 activations"
    f.tok_embeddings.to(BF)
    assert f.block_eligible()
    # w1 int4 beside a dense w3
    f.layers[0].feed_forward.w3 = nn.Linear(64, 128, bias=False).to(BF)
    assert not f.block_eligible(), "w1 int4 beside a dense w3"
    # w1 / w3 of different groupsize
    g = _caches(_convert("int4", BF))
    g.block_int4 = True
    g.layers[1].feed_forward.w3 = WeightOnlyInt4Linear(64, 128, groupsize=64)
    assert is_int4_linear(g.layers[1].feed_forward.w3) and not g.block_eligible(), "w1 / w3 of different groupsize"
    g.layers[1].feed_forward.w3 = WeightOnlyInt4Linear(64, 128, groupsize=32)
    assert g.block_eligible()
    # ... while another groupsize or a dense linear elsewhere is fine (each linear is served on its own)
    g.layers[0].attention.wo = WeightOnlyInt4Linear(64, 64, groupsize=64)
    g.layers[1].attention.wo = nn.Linear(64, 64, bias=False).to(BF)
    assert g.block_eligible()
    # a bare uint8 LM head carries no (scale, zero) pairs and no groupsize: not an int4 module
    g.output = nn.Linear(64, 128, bias=False)
    g.output.weight = nn.Parameter(torch.zeros(128, 32, dtype=torch.uint8), requires_grad=False)
    assert not is_int4_linear(g.output) and not g.block_eligible(), "a bare uint8 LM head"
    # int8 models: block_int4 does not admit them, and one int4 linear in an int8 model needs both attributes
    m8 = _caches(_convert("int8", BF))
    m8.block_int4 = True
    assert not m8.block_eligible(), "block_int4 alone does not cover int8"
    m8.block_weight_only = True
    assert m8.block_eligible()
    m8.layers[1].feed_forward.w2 = WeightOnlyInt4Linear(128, 64, groupsize=32)
    assert m8.block_eligible(), "an int4 w2 in an int8 model with both attributes"
    m8.block_int4 = False
    assert not m8.block_eligible(), "one int4 linear without block_int4"
    # the dense answers are what they were, with either value of the attribute
    d = _caches(_dense(F32))
    assert d.block_eligible()
    d.block_int4 = True
    assert d.block_eligible()


# ------------------------------------------------------------------------------------------------ the route, on the CPU twin
NEXT = torch.tensor([9, 21, 6, 33, 47, 5, 60, 72, 7, 85, 99, 110, 14, 27], dtype=torch.int32)  # the prefill's token + 13 forced steps


def _generate(forced_block, counts, block_int4=True):
    from cold_compress_amd.harness import decode_one_token, generate, prefill

    model = _caches(_convert("int4", BF, seed=11))
    model.block_int4 = block_int4
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


def test_teacher_forced_blocks_of_an_int4_model_equal_single_steps(twin):
    c4, c1, c0 = [], [], []
    seq4, probs4, st4 = _generate(4, c4)
    seq1, probs1, st1 = _generate(1, c1)
    assert c4 == [4, 4, 4], f"forward_block was entered with {c4}"  # 13 forced steps: three blocks and a tail of one
    assert not c1
    assert torch.equal(seq4, seq1) and seq4[40:].tolist() == NEXT.tolist()
    assert len(probs4) == len(probs1) == 14 and all(torch.equal(a.float(), b.float()) for a, b in zip(probs4, probs1))
    assert st4.keys() == st1.keys() and st4
    for n in st4:
        assert torch.equal(st4[n].float() if st4[n].is_floating_point() else st4[n], st1[n].float() if st1[n].is_floating_point() else st1[n]), n
    seq0, _, _ = _generate(4, c0, block_int4=False)
    assert not c0 and torch.equal(seq0, seq4), "with the attribute off the per-token route serves the same request"


@pytest.mark.parametrize("block_int4", [True, False], ids=["on", "off"])
def test_generate_streams_on_the_twin_reports_the_joint_route(twin, block_int4):
    from cold_compress_amd.harness import DecodeStreams, decode_one_token, generate, generate_streams, prefill

    def build():
        m = _caches(_convert("int4", BF, seed=11))
        m.block_int4 = block_int4
        return m

    g = torch.Generator().manual_seed(3)
    prompt = torch.randint(8, 128, (40,), generator=g, dtype=torch.int32)
    model = build()
    streams = DecodeStreams(model, 3)
    assert model.streams_eligible(streams) == block_int4
    seqs, probs, stats = generate_streams(model, prompt, prefill, 6, n_streams=3, seeds=[11, 5, 7], streams=streams, temperature=0.8, top_k=5)
    assert stats["joint_steps"] is block_int4 and stats["streams"] == 3
    for s, seed in enumerate([11, 5, 7]):
        seq, pr, _ = generate(build(), prompt, prefill, decode_one_token, max_new_tokens=6, seed=seed, temperature=0.8, top_k=5)
        assert torch.equal(seqs[s], seq), s
        assert len(probs[s]) == len(pr) and all(torch.equal(a.float(), b.float()) for a, b in zip(probs[s], pr)), s
