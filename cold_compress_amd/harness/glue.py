"""Caller glue (residual + RMSNorm, QKV split + RoPE + head layout, SwiGLU gate) as three fused HIP launches.

These are NOT part of the cache/attention hot path — they are the model-side code around it
(ref: model.py:317-327, 375-387, 442-443, 452-457, 507-519), which the reference leaves to ~45 eager elementwise
launches per layer or to torch.compile.  On device tensors they call the C ABI (`cc_add_rmsnorm`, `cc_qkv_rope`,
`cc_silu_mul`, `cc_gemv_fused`, `cc_gemv_fused_multi` and its int8 / MXFP4 / int4 forms, `cc_softmax_argmax`, `cc_sample_topk`, `cc_sample_nucleus`, `cc_sample_rows`, `cc_logprob_rows`, `cc_logprob_topn`,
`cc_token_counts_add`, `cc_logits_penalize`, `cc_token_history_write`, `cc_logits_constrain`, `cc_logits_penalize_streams`,
`cc_logits_constrain_streams`); CPU tensors raise — there is no host path in the package (the
CPU model-wiring test brings its own eager twins: tests/host_glue.py).
"""
import ctypes as C
import os
import warnings
import weakref

import torch

from .. import _abi

_DT = {torch.float32: _abi.CC_DT_F32, torch.bfloat16: _abi.CC_DT_BF16, torch.float16: _abi.CC_DT_F16}

def _host(t, what):
    raise _abi.ColdCompressError(f"{what} is on {t.device}: the HIP path needs ROCm device tensors (no CPU fallback).")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def add_rmsnorm(x, weight, eps, delta=None):
    """-> (h, normed) with h = x + delta (or x itself when delta is None)."""
    if not x.is_cuda:
        _host(x, "add_rmsnorm input")
    dim = x.shape[-1]
    xc = x.contiguous()
    T = xc.numel() // dim
    out = torch.empty_like(xc)
    h = xc
    dc = None
    if delta is not None:
        dc = delta.contiguous()
        h = torch.empty_like(xc)
    _abi.call("cc_add_rmsnorm", _p(xc), _p(dc), _p(weight), T, dim, float(eps), _DT[x.dtype], _p(h) if delta is not None else None,
              _p(out), _stream())
    return h, out


def qkv_rope(qkv, freqs_cis, n_head, n_local_heads, head_dim):
    """qkv [1, T, (HQ+2H)*D], freqs_cis [T, D/2, 2] -> q [1,HQ,T,D], k [1,H,T,D], v [1,H,T,D] (rotated, head-major)."""
    bsz, T, _ = qkv.shape
    HQ, H, D = n_head, n_local_heads, head_dim
    if not qkv.is_cuda:
        _host(qkv, "qkv_rope input")
    qc = qkv.contiguous()
    fc = freqs_cis.contiguous()
    q = torch.empty((1, HQ, T, D), dtype=qkv.dtype, device=qkv.device)
    k = torch.empty((1, H, T, D), dtype=qkv.dtype, device=qkv.device)
    v = torch.empty((1, H, T, D), dtype=qkv.dtype, device=qkv.device)
    _abi.call("cc_qkv_rope", _p(qc), _p(fc), T, HQ, H, D, _DT[qkv.dtype], _p(q), _p(k), _p(v), _stream())
    return q, k, v


def silu_mul(a, b):
    if not a.is_cuda:
        _host(a, "silu_mul input")
    ac, bc = a.contiguous(), b.contiguous()
    out = torch.empty_like(ac)
    _abi.call("cc_silu_mul", _p(ac), _p(bc), ac.numel(), _DT[a.dtype], _p(out), _stream())
    return out


def gemv_supported(*weights):
    """Single-token dense layers on the device path: the input vector must fit the kernel's LDS staging buffer.  int8 weights
    (weight-only int8 linears) stream through cc_gemv_fused_w8: 16-bit activations, K a multiple of 16.  uint8 weights (weight-only
    int4 linears, two codes per byte: K = 2 * shape[1]) stream through cc_gemv_fused_w4: K a multiple of 32 (of the groupsize,
    which the call checks) or, MXFP4 linears, through cc_gemv_fused_mx4: the same bound."""
    def ok(w):
        if not (w.is_cuda and w.is_contiguous()):
            return False
        if w.dtype == torch.int8:
            return w.shape[1] * 2 <= 64 * 1024 and w.shape[1] % 16 == 0
        if w.dtype == torch.uint8:
            return 2 * w.shape[1] * 2 <= 64 * 1024 and (2 * w.shape[1]) % 32 == 0
        return w.dtype in _DT and w.shape[1] * w.element_size() <= 64 * 1024 and w.shape[1] % (16 // w.element_size()) == 0
    return all(ok(w) for w in weights)


class W12Packed:
    """The lossless 12-bit packed copy of one dense bf16 weight (cc_w12_pack; format: include/coldcompress.h).  `codes` uint32
    [N, K / 8, 3], `records` uint32 [records, 8], `base` the first exponent of the window, (`rb`, `cu`, `xs`, `cap`) the launch
    geometry it was packed for (the records follow `rb` and `cu`); `n_overflow` records hold more than 7 escapes (their tiles are
    read from the dense tensor), `n_escapes` weights lie outside the window.  `layout`: 0 (sign + mantissa bytes and 4-bit exponent
    indices), W12_PLANAR (low bytes and a dword of high-byte fields; `base` is even) or W12_LONG (planar codes with the records of
    the long-row launch, plain matrices with 4096 < K <= 16384); a copy is tied to it as to (`rb`, `cu`)."""
    __slots__ = ("codes", "records", "base", "rb", "cu", "xs", "cap", "n_records", "n_overflow", "n_escapes", "layout")


W12_PLANAR, W12_LONG = 1, 2  # layout ids (include/coldcompress.h): they travel in bits 8 .. 15 of the rb / swiglu words


W12_MAX_OVERFLOW = 0.01  # a tensor with more overflowing records than this share stays on cc_gemv_fused
_W12_MARGIN = 1 << 30  # free device memory kept beyond a packed copy
# (data_ptr, _version, shape, device, swiglu, layout) -> (W12Packed, or None: refused, unsupported or no room, and not tried again for this
# version of the weight; weak reference to the weight: while it lives its storage does, so the address cannot have been given to
# another tensor)
_w12_cache = {}
_w12_geo = {}  # (N, K, swiglu, layout) -> cc_w12_geometry's answer
_w12_drops = 0  # moves whenever a packed copy is dropped: a captured graph may still hold its address (w12_epoch)
_w12_warned = False


def w12_enabled():
    return os.environ.get("CC_W12", "1") != "0"


def w12_geometry(N, K, swiglu=False, layout=0):
    """(RB, CU, input chunks per lane, most workgroups, faster) of the packed GEMV's launch for this shape, form and code layout, or
    None: unsupported.  `faster`: 1 when that launch class measured faster than the dense kernel (layout 0) resp. than the dense
    kernel and layout 0 (W12_PLANAR), than the dense kernel and the planar launch (W12_LONG), else 0."""
    key = (int(N), int(K), bool(swiglu), int(layout))
    if key not in _w12_geo:
        out = (C.c_int32 * 5)()
        ok = _abi.lib()["cc_w12_geometry"](key[0], key[1], int(key[2]) | key[3] << 8, out) == _abi.CC_OK
        _w12_geo[key] = tuple(out) if ok else None
    return _w12_geo[key]


def w12_nbytes(N, K, rb, cu):
    nstep = -(-(-(-K // 512)) // 4)
    return N * K * 3 // 2 + -(-N // rb) * -(-nstep // cu) * 4 * 32


def w12_pack(weight, swiglu=False, refuse=True, layout=0):
    """Pack a dense bf16 [N, K] device tensor for the launch geometry of its shape (`swiglu`: as one of the W / W3 pair) in `layout` ->
    W12Packed, or None when the shape is unsupported or (`refuse`) more than W12_MAX_OVERFLOW of the records overflow.
    Synchronises (reads the packer's counts back): not for use under stream capture."""
    N, K = weight.shape
    geo = w12_geometry(N, K, swiglu, layout)
    if geo is None or weight.dtype != torch.bfloat16 or not (weight.is_cuda and weight.is_contiguous()) or N * K >= 1 << 31:
        return None
    rb, cu = geo[0], geo[1]
    nstep = -(-(-(-K // 512)) // 4)
    nrec = -(-N // rb) * -(-nstep // cu) * 4
    p = W12Packed()
    p.codes = torch.empty((N, K // 8 * 3), dtype=torch.int32, device=weight.device)
    p.records = torch.empty((nrec, 8), dtype=torch.int32, device=weight.device)
    meta = torch.empty((int(_abi.lib()["cc_w12_meta_words"]()),), dtype=torch.int32, device=weight.device)
    _abi.call("cc_w12_pack", _p(weight), N, K, rb | layout << 8, cu, _p(p.codes), _p(p.records), _p(meta), _stream())
    m = meta[:4].tolist()
    p.base, p.n_records, p.n_overflow, p.n_escapes = m
    p.rb, p.cu, p.xs, p.cap = geo[:4]
    p.layout = layout
    if refuse and p.n_overflow > W12_MAX_OVERFLOW * p.n_records:
        return None
    return p


def _w12_drop(key):
    global _w12_drops
    if _w12_cache.pop(key, None) is not None:
        _w12_drops += 1


def _w12_get(weight, swiglu, force=False, layout=None):
    """The packed copy of `weight`, built at its first eager use; None: take the plain path (a launch class that did not measure
    faster than the dense kernel, unless `force`; under capture before a copy exists; refused by the packer; unsupported shape; no
    room).  `layout` None: the long-row launch (W12_LONG) where its class measured faster than the dense kernel and planar, else
    planar where its launch class measured faster than the dense kernel and layout 0, else layout 0.  Keyed on the storage, its
    version counter and the layout: an in-place change of the weight drops the copy."""
    global _w12_warned
    N, K = weight.shape
    if layout is None:
        layout = 0
        for lay in (W12_LONG, W12_PLANAR):
            g = w12_geometry(N, K, swiglu, lay)
            if g is not None and g[4]:
                layout = lay
                break
    geo = w12_geometry(N, K, swiglu, layout)
    if geo is None or not (force or geo[4]):
        return None
    key = (weight.data_ptr(), weight._version, tuple(weight.shape), weight.device, swiglu, layout)
    hit = _w12_cache.get(key)
    if hit is not None and hit[1]() is not None:
        return hit[0]
    if torch.cuda.is_current_stream_capturing():
        return None  # never pack under capture: this replayed graph keeps the plain kernel
    for k in [k for k in _w12_cache if k[0] == key[0] and k[3] == key[3] and (k == key or k[1] != key[1] or k[2] != key[2])]:
        _w12_drop(k)  # the weight changed in place (or its storage was reused): its old copy goes
    # room: what the driver reports free plus what torch's allocator holds cached but unused
    free = torch.cuda.mem_get_info(weight.device)[0] + torch.cuda.memory_reserved(weight.device) - torch.cuda.memory_allocated(weight.device)
    p = None
    if free >= w12_nbytes(N, K, geo[0], geo[1]) + _W12_MARGIN:
        p = w12_pack(weight, swiglu, layout=layout)
    elif not _w12_warned:
        _w12_warned = True
        warnings.warn("cold_compress_amd: not enough free device memory for the 12-bit packed weight copies; the remaining dense "
                      "layers decode from their bf16 weights (CC_W12=0 switches the copies off)")
    _w12_cache[key] = (p, weakref.ref(weight))  # (None as well: not tried again until the weight changes or the cache is cleared)
    weakref.finalize(weight, _w12_drop, key)
    return p


def w12_epoch():
    """Changes whenever a captured graph may hold the address of a packed copy that is gone or out of date: a copy was dropped
    (w12_cache_clear, a repack, a freed weight), or a weight with a copy changed in place since (its version counter moved; the copy
    is rebuilt by the next EAGER use only).  GraphedDecoder compares it before every replay and captures again when it moved; any
    other holder of a captured graph over gemv_fused(..., w12=...) has to do the same."""
    stale = 0
    for key, (p, ref) in _w12_cache.items():
        if p is not None:
            w = ref()
            if w is not None and w._version != key[1]:
                stale += 1
    return (_w12_drops, stale)


def w12_cache_clear():
    """Drop every packed copy.  Their memory is free for reuse at once: a captured graph that launched cc_gemv_fused_w12 must not
    be replayed afterwards (w12_epoch moves; GraphedDecoder captures again)."""
    for k in list(_w12_cache):
        _w12_drop(k)


def gemv_fused(weight, x, w3=None, delta=None, norm_weight=None, eps=1e-5, h_out=None, bias=None, freqs=None, rope_rows=0,
               head_dim=0, scales=None, scales3=None, groupsize=None, w12=False):
    """One decode-time dense layer with its glue fused (cc_gemv_fused): optional RMSNorm(x + delta) prologue (h_out
    receives x + delta), optional SwiGLU pairing with `w3`, optional RoPE epilogue on the first `rope_rows` rows.
    x: [K] (any shape with K elements); returns [N] in the model dtype.
    int8 `weight` (and `w3`): weight-only int8 with per-row `scales` (`scales3`) in x's dtype (cc_gemv_fused_w8).
    uint8 `weight` (and `w3`): weight-only int4, [N, K / 2] packed codes with `scales` (`scales3`) the bf16 (scale, zero) pairs
    per row, [N, K / groupsize, 2], and bf16 activations (cc_gemv_fused_w4).
    uint8 `weight` with uint8 `scales` and no groupsize: weight-only MXFP4, [N, K / 2] packed e2m1 codes with `scales` (`scales3`)
    the e8m0 block-scale bytes, [N, K / 32], and bf16 activations (cc_gemv_fused_mx4)."""
    N, K = weight.shape
    xc = x.contiguous()
    dc = delta.contiguous() if delta is not None else None
    fc = freqs.contiguous() if freqs is not None else None
    if weight.dtype == torch.uint8 and groupsize is None and (scales is None or scales.dtype == torch.uint8):  # MXFP4 (before int4)
        K = 2 * K
        if scales is None or (w3 is not None and (w3.dtype != torch.uint8 or scales3 is None)):
            raise _abi.ColdCompressError("gemv_fused: uint8 weights need their scales: MXFP4 its uint8 block scales (and w3 uint8 with "
                                         "scales3), int4 its (scale, zero) pairs and groupsize")
        if x.dtype != torch.bfloat16:
            raise _abi.ColdCompressError(f"gemv_fused: MXFP4 weights need bf16 activations, got {x.dtype}")
        for t in (scales, scales3):
            if t is not None and (t.dtype != torch.uint8 or not t.is_contiguous() or tuple(t.shape) != (N, K // 32)):
                raise _abi.ColdCompressError(f"gemv_fused: MXFP4 block scales must be contiguous uint8 [{N}, K / 32] (K = {K}), got "
                                             f"{t.dtype} {tuple(t.shape)}")
        y = torch.empty((N,), dtype=torch.bfloat16, device=weight.device)
        _abi.call("cc_gemv_fused_mx4", _p(weight), _p(scales), _p(w3), _p(scales3), _p(xc), _p(dc), _p(norm_weight), float(eps),
                  _p(h_out), _p(bias), _p(fc), int(rope_rows), int(head_dim), _p(y), N, K, _DT[torch.bfloat16], _stream())
        return y
    if weight.dtype == torch.uint8:
        K = 2 * K
        if scales is None or groupsize is None or (w3 is not None and (w3.dtype != torch.uint8 or scales3 is None)):
            raise _abi.ColdCompressError("gemv_fused: int4 weights need their (scale, zero) pairs and groupsize (and w3 uint8 with "
                                         "scales3)")
        if x.dtype != torch.bfloat16:
            raise _abi.ColdCompressError(f"gemv_fused: int4 weights need bf16 activations, got {x.dtype}")
        for t in (scales, scales3):
            if t is not None and (t.dtype != torch.bfloat16 or not t.is_contiguous() or tuple(t.shape) != (N, K // groupsize, 2)):
                raise _abi.ColdCompressError(f"gemv_fused: int4 (scale, zero) pairs must be contiguous bf16 [{N}, K / {groupsize}, 2] "
                                             f"(K = {K}), got {t.dtype} {tuple(t.shape)}")
        y = torch.empty((N,), dtype=torch.bfloat16, device=weight.device)
        _abi.call("cc_gemv_fused_w4", _p(weight), _p(scales), _p(w3), _p(scales3), _p(xc), _p(dc), _p(norm_weight), float(eps), _p(h_out),
                  _p(bias), _p(fc), int(rope_rows), int(head_dim), _p(y), N, K, int(groupsize), _DT[torch.bfloat16], _stream())
        return y
    if weight.dtype == torch.int8:
        if scales is None or (w3 is not None and (w3.dtype != torch.int8 or scales3 is None)):
            raise _abi.ColdCompressError("gemv_fused: int8 weights need their per-row scales (and w3 int8 with scales3)")
        dt = x.dtype
        if dt not in (torch.bfloat16, torch.float16):
            raise _abi.ColdCompressError(f"gemv_fused: int8 weights need 16-bit activations, got {dt}")
        sc = scales.to(dt).contiguous()
        sc3 = scales3.to(dt).contiguous() if w3 is not None else None
        y = torch.empty((N,), dtype=dt, device=weight.device)
        _abi.call("cc_gemv_fused_w8", _p(weight), _p(sc), _p(w3), _p(sc3), _p(xc), _p(dc), _p(norm_weight), float(eps), _p(h_out),
                  _p(bias), _p(fc), int(rope_rows), int(head_dim), _p(y), N, K, _DT[dt], _stream())
        return y
    y = torch.empty((N,), dtype=weight.dtype, device=weight.device)
    if w12 and weight.dtype == torch.bfloat16 and w12_enabled() and (w3 is None or w3.dtype == torch.bfloat16):
        # the lossless 12-bit packed copies of the weights: the same bits from three quarters of the bytes (cc_gemv_fused_w12).
        # w12=True: where that launch class measured faster than the dense kernel, in the layout that measured fastest there;
        # w12="force" / "force-planar" / "force-long": wherever the kernel serves the shape, in layout 0 / the planar layout / the
        # long-row launch (layout id 2)
        force = w12 in ("force", "force-planar", "force-long")
        lay = {"force": 0, "force-planar": W12_PLANAR, "force-long": W12_LONG}.get(w12)
        pk = _w12_get(weight, w3 is not None, force, lay)
        pk3 = _w12_get(w3, True, force, lay) if (w3 is not None and pk is not None) else None
        if pk is not None and (w3 is None or pk3 is not None):
            _abi.call("cc_gemv_fused_w12", _p(pk.codes), _p(pk.records), pk.base, _p(pk3.codes) if pk3 else None,
                      _p(pk3.records) if pk3 else None, pk3.base if pk3 else 0, pk.rb | pk.layout << 8, pk.cu, _p(weight), _p(w3), _p(xc), _p(dc),
                      _p(norm_weight), float(eps), _p(h_out), _p(bias), _p(fc), int(rope_rows), int(head_dim), _p(y), N, K,
                      _DT[weight.dtype], _stream())
            return y
    _abi.call("cc_gemv_fused", _p(weight), _p(w3), _p(xc), _p(dc), _p(norm_weight),
              float(eps), _p(h_out), _p(bias), _p(fc), int(rope_rows), int(head_dim),
              _p(y), N, K, _DT[weight.dtype], _stream())
    return y


GEMV_MULTI_MAX_T = 4  # CC_GEMV_MULTI_MAX_T (include/coldcompress.h)


def gemv_fused_multi(weight, x, w3=None, delta=None, norm_weight=None, eps=1e-5, h_out=None, bias=None, freqs=None, rope_rows=0,
                     head_dim=0, scales=None, scales3=None):
    """gemv_fused for T input vectors from ONE pass over the weights (cc_gemv_fused_multi), 1 <= T <= 4: x [T, K] (delta, h_out
    likewise), freqs [T, head_dim / 2, 2] -> [T, N].  Row t is bit-identical to gemv_fused on row t.
    int8 `weight` (and `w3`) with per-row `scales` (`scales3`): cc_gemv_fused_w8_multi, bf16 or f16 activations.
    uint8 `weight` (and `w3`) with uint8 `scales` (`scales3`), the e8m0 block bytes [N, K / 32]: cc_gemv_fused_mx4_multi, bf16
    activations.  The int4 GEMV (uint8 codes with bf16 (scale, zero) pairs) has no multi form HERE: an error, not a fallback — its
    multi form is gemv_fused_w4_multi below, which takes the groupsize; callers ask Transformer.block_eligible first."""
    if weight.dtype == torch.int8:
        if scales is None or (w3 is not None and (w3.dtype != torch.int8 or scales3 is None)):
            raise _abi.ColdCompressError("gemv_fused_multi: int8 weights need their per-row scales (and w3 int8 with scales3)")
        if x.dtype not in (torch.bfloat16, torch.float16):
            raise _abi.ColdCompressError(f"gemv_fused_multi: int8 weights need 16-bit activations, got {x.dtype}")
        N, K = weight.shape
        for t in (scales, scales3):
            if t is not None and t.numel() != N:
                raise _abi.ColdCompressError(f"gemv_fused_multi: int8 scales must hold one value per row ({N}), got {tuple(t.shape)}")
    elif weight.dtype == torch.uint8:
        if scales is None or scales.dtype != torch.uint8 or (w3 is not None and (w3.dtype != torch.uint8 or scales3 is None)):
            raise _abi.ColdCompressError("gemv_fused_multi: uint8 weights need MXFP4's uint8 block scales (and w3 uint8 with scales3); the "
                                         "int4 GEMV has no multi form")
        if x.dtype != torch.bfloat16:
            raise _abi.ColdCompressError(f"gemv_fused_multi: MXFP4 weights need bf16 activations, got {x.dtype}")
        N, K = weight.shape[0], 2 * weight.shape[1]
        for t in (scales, scales3):
            if t is not None and (t.dtype != torch.uint8 or not t.is_contiguous() or tuple(t.shape) != (N, K // 32)):
                raise _abi.ColdCompressError(f"gemv_fused_multi: MXFP4 block scales must be contiguous uint8 [{N}, K / 32] (K = {K}), got "
                                             f"{t.dtype} {tuple(t.shape)}")
    elif weight.dtype in _DT:
        if scales is not None or scales3 is not None:
            raise _abi.ColdCompressError("gemv_fused_multi: dense weights take no scales")
        N, K = weight.shape
    else:
        raise _abi.ColdCompressError(f"gemv_fused_multi: dense, int8 or MXFP4 weights, got {weight.dtype}")
    if weight.dtype not in _DT and w3 is not None and tuple(w3.shape) != tuple(weight.shape):
        raise _abi.ColdCompressError(f"gemv_fused_multi: w3 must have the shape of weight {tuple(weight.shape)}, got {tuple(w3.shape)}")
    if not x.is_cuda:
        _host(x, "gemv_fused_multi input")
    if x.dim() != 2 or x.shape[1] != K:
        raise _abi.ColdCompressError(f"gemv_fused_multi: x must be [T, {K}], got {tuple(x.shape)}")
    T = x.shape[0]
    for name, t, shape in (("delta", delta, (T, K)), ("h_out", h_out, (T, K)), ("freqs", freqs, (T, head_dim // 2, 2))):
        if t is not None and tuple(t.shape) != shape:
            raise _abi.ColdCompressError(f"gemv_fused_multi: {name} must be {list(shape)}, got {tuple(t.shape)}")
    if h_out is not None and not h_out.is_contiguous():
        raise _abi.ColdCompressError("gemv_fused_multi: h_out must be contiguous")
    xc = x.contiguous()
    dc = delta.contiguous() if delta is not None else None
    fc = freqs.contiguous() if freqs is not None else None
    if weight.dtype == torch.int8:
        dt = x.dtype
        sc = scales.to(dt).contiguous()
        sc3 = scales3.to(dt).contiguous() if w3 is not None else None
        y = torch.empty((T, N), dtype=dt, device=weight.device)
        _abi.call("cc_gemv_fused_w8_multi", _p(weight), _p(sc), _p(w3), _p(sc3), _p(xc), _p(dc), _p(norm_weight), float(eps), _p(h_out),
                  _p(bias), _p(fc), int(rope_rows), int(head_dim), _p(y), N, K, T, _DT[dt], _stream())
        return y
    if weight.dtype == torch.uint8:
        y = torch.empty((T, N), dtype=torch.bfloat16, device=weight.device)
        _abi.call("cc_gemv_fused_mx4_multi", _p(weight), _p(scales), _p(w3), _p(scales3), _p(xc), _p(dc), _p(norm_weight), float(eps),
                  _p(h_out), _p(bias), _p(fc), int(rope_rows), int(head_dim), _p(y), N, K, T, _DT[torch.bfloat16], _stream())
        return y
    y = torch.empty((T, N), dtype=weight.dtype, device=weight.device)
    _abi.call("cc_gemv_fused_multi", _p(weight), _p(w3), _p(xc), _p(dc), _p(norm_weight), float(eps), _p(h_out), _p(bias), _p(fc),
              int(rope_rows), int(head_dim), _p(y), N, K, T, _DT[weight.dtype], _stream())
    return y


def gemv_fused_w4_multi(weight, x, scales, groupsize, w3=None, scales3=None, delta=None, norm_weight=None, eps=1e-5, h_out=None,
                        bias=None, freqs=None, rope_rows=0, head_dim=0):
    """gemv_fused's int4 form for T input vectors from ONE pass over the weights (cc_gemv_fused_w4_multi), 1 <= T <= 4: uint8
    `weight` (and `w3`) [N, K / 2] packed codes, `scales` (`scales3`) the contiguous bf16 (scale, zero) pairs [N, K / groupsize, 2],
    bf16 x [T, K] (delta, h_out likewise), freqs [T, head_dim / 2, 2] -> bf16 [T, N].  Row t is bit-identical to gemv_fused on row t.
    A function of its own: gemv_fused_multi keeps its signature and its refusal of int4 weights.  Every refusal precedes the
    library call."""
    what = "gemv_fused_w4_multi"
    if not torch.is_tensor(weight) or weight.dtype != torch.uint8 or weight.dim() != 2:
        raise _abi.ColdCompressError(f"{what}: int4 weights are uint8 [N, K / 2] packed codes, got "
                                     f"{getattr(weight, 'dtype', type(weight))} {tuple(getattr(weight, 'shape', ()))}")
    if scales is None or groupsize is None or (w3 is not None and (w3.dtype != torch.uint8 or scales3 is None)) or \
            (w3 is None and scales3 is not None):
        raise _abi.ColdCompressError(f"{what}: int4 weights need their (scale, zero) pairs and groupsize (and w3 uint8 with scales3)")
    if int(groupsize) not in (32, 64, 128, 256):
        raise _abi.ColdCompressError(f"{what}: groupsize must be 32, 64, 128 or 256, got {groupsize}")
    groupsize = int(groupsize)
    N, K = weight.shape[0], 2 * weight.shape[1]
    if K % groupsize:
        raise _abi.ColdCompressError(f"{what}: K = {K} is not a multiple of the groupsize {groupsize}")
    if w3 is not None and tuple(w3.shape) != tuple(weight.shape):
        raise _abi.ColdCompressError(f"{what}: w3 must have the shape of weight {tuple(weight.shape)}, got {tuple(w3.shape)}")
    for t in (scales, scales3):
        if t is not None and (t.dtype != torch.bfloat16 or not t.is_contiguous() or tuple(t.shape) != (N, K // groupsize, 2)):
            raise _abi.ColdCompressError(f"{what}: int4 (scale, zero) pairs must be contiguous bf16 [{N}, K / {groupsize}, 2] "
                                         f"(K = {K}), got {t.dtype} {tuple(t.shape)}")
    if x.dtype != torch.bfloat16:
        raise _abi.ColdCompressError(f"{what}: int4 weights need bf16 activations, got {x.dtype}")
    if x.dim() != 2 or x.shape[1] != K:
        raise _abi.ColdCompressError(f"{what}: x must be [T, {K}], got {tuple(x.shape)}")
    T = x.shape[0]
    if not 1 <= T <= GEMV_MULTI_MAX_T:
        raise _abi.ColdCompressError(f"{what}: 1 <= T <= {GEMV_MULTI_MAX_T}, got T = {T}")
    for name, t, shape in (("delta", delta, (T, K)), ("h_out", h_out, (T, K)), ("freqs", freqs, (T, head_dim // 2, 2))):
        if t is not None and tuple(t.shape) != shape:
            raise _abi.ColdCompressError(f"{what}: {name} must be {list(shape)}, got {tuple(t.shape)}")
    for name, t in (("delta", delta), ("h_out", h_out), ("norm_weight", norm_weight), ("bias", bias), ("freqs", freqs)):
        if t is not None and t.dtype != torch.bfloat16:
            raise _abi.ColdCompressError(f"{what}: {name} must be bf16, got {t.dtype}")
    if h_out is not None and not h_out.is_contiguous():
        raise _abi.ColdCompressError(f"{what}: h_out must be contiguous")
    if not x.is_cuda:
        _host(x, f"{what} input")
    xc = x.contiguous()
    dc = delta.contiguous() if delta is not None else None
    fc = freqs.contiguous() if freqs is not None else None
    y = torch.empty((T, N), dtype=torch.bfloat16, device=weight.device)
    _abi.call("cc_gemv_fused_w4_multi", _p(weight), _p(scales), _p(w3), _p(scales3), _p(xc), _p(dc), _p(norm_weight), float(eps),
              _p(h_out), _p(bias), _p(fc), int(rope_rows), int(head_dim), _p(y), N, K, groupsize, T, _DT[torch.bfloat16], _stream())
    return y


def softmax_argmax(logits):
    """probs = softmax(logits) in the model dtype and the greedy token (first index of the largest rounded probability),
    one launch (cc_softmax_argmax).  logits: [V]."""
    lc = logits.contiguous()
    probs = torch.empty_like(lc)
    idx = torch.empty((1,), dtype=torch.int32, device=lc.device)
    ws = _SM_WS.get(lc.device)
    if ws is None:
        ws = _SM_WS[lc.device] = torch.empty(int(_abi.lib()["cc_softmax_argmax_workspace_bytes"]()), dtype=torch.uint8, device=lc.device)
    _abi.call("cc_softmax_argmax", _p(lc), lc.numel(), _DT[lc.dtype], _p(probs), _p(idx), _p(ws), ws.numel(), _stream())
    return probs, idx


_SM_WS = {}


def sample_topk(logits, temperature, top_k, seed, input_pos):
    """probs = the reference's logits_to_probs(logits, temperature, top_k) in the model dtype and one token drawn from it by the
    stateless Gumbel-max rule of (seed, *input_pos) (cc_sample_topk; include/coldcompress.h has the contract).  logits: [V];
    input_pos: a one-element int32 DEVICE tensor, read by the kernels (a captured step advances through it).  -> (probs, idx)."""
    if not logits.is_cuda:
        _host(logits, "sample_topk logits")
    if not (input_pos.is_cuda and input_pos.dtype == torch.int32 and input_pos.numel() == 1):
        raise _abi.ColdCompressError(f"sample_topk: input_pos must be a one-element int32 device tensor, got {input_pos.dtype} "
                                     f"{tuple(input_pos.shape)} on {input_pos.device}")
    if not float(temperature) > 0:
        raise _abi.ColdCompressError(f"sample_topk: temperature must be > 0, got {temperature}")
    lc = logits.contiguous()
    probs = torch.empty_like(lc)
    idx = torch.empty((1,), dtype=torch.int32, device=lc.device)
    ws = _SP_WS.get(lc.device)
    if ws is None:
        ws = _SP_WS[lc.device] = torch.empty(int(_abi.lib()["cc_sample_topk_workspace_bytes"]()), dtype=torch.uint8, device=lc.device)
    k = 0 if top_k is None else max(0, min(int(top_k), 2 ** 31 - 1))
    _abi.call("cc_sample_topk", _p(lc), lc.numel(), _DT[lc.dtype], float(temperature), k, int(seed) & (2 ** 64 - 1), _p(input_pos),
              _p(probs), _p(idx), _p(ws), ws.numel(), _stream())
    return probs, idx


_SP_WS = {}


def sample_nucleus(logits, temperature, top_k, top_p, min_p, seed, input_pos, return_n_kept=False):
    """sample_topk with the top-p (nucleus) and min-p filters of cc_sample_nucleus (include/coldcompress.h has the contract) between the
    top-k cut and the softmax; `top_p` / `min_p` None: that filter is off (both off: sample_topk's launches and its answer, bit for
    bit).  -> (probs, idx), and with `return_n_kept` a one-element int32 device tensor, the size of the kept set, as a third."""
    if not logits.is_cuda:
        _host(logits, "sample_nucleus logits")
    if not (input_pos.is_cuda and input_pos.dtype == torch.int32 and input_pos.numel() == 1):
        raise _abi.ColdCompressError(f"sample_nucleus: input_pos must be a one-element int32 device tensor, got {input_pos.dtype} "
                                     f"{tuple(input_pos.shape)} on {input_pos.device}")
    if not float(temperature) > 0:
        raise _abi.ColdCompressError(f"sample_nucleus: temperature must be > 0, got {temperature}")
    p = 1.0 if top_p is None else float(top_p)
    mp = 0.0 if min_p is None else float(min_p)
    if not p > 0:
        raise _abi.ColdCompressError(f"sample_nucleus: top_p must be > 0 (>= 1: off), got {top_p}")
    if not mp <= 1:
        raise _abi.ColdCompressError(f"sample_nucleus: min_p must be <= 1 (<= 0: off), got {min_p}")
    lc = logits.contiguous()
    probs = torch.empty_like(lc)
    idx = torch.empty((1,), dtype=torch.int32, device=lc.device)
    n_kept = torch.empty((1,), dtype=torch.int32, device=lc.device) if return_n_kept else None
    ws = _SN_WS.get(lc.device)
    if ws is None:
        ws = _SN_WS[lc.device] = torch.empty(int(_abi.lib()["cc_sample_nucleus_workspace_bytes"]()), dtype=torch.uint8, device=lc.device)
    k = 0 if top_k is None else max(0, min(int(top_k), 2 ** 31 - 1))
    _abi.call("cc_sample_nucleus", _p(lc), lc.numel(), _DT[lc.dtype], float(temperature), k, p, mp, int(seed) & (2 ** 64 - 1),
              _p(input_pos), _p(probs), _p(idx), _p(n_kept), _p(ws), ws.numel(), _stream())
    return (probs, idx, n_kept) if return_n_kept else (probs, idx)


_SN_WS = {}

SAMPLE_MAX_ROWS = 8  # CC_SAMPLE_MAX_ROWS (include/coldcompress.h)


def sample_rows(logits_2d, temperature, top_k, top_p, min_p, seeds, input_pos, return_n_kept=False):
    """sample_nucleus for the T rows of `logits_2d` [T, V] (T <= SAMPLE_MAX_ROWS) in the launches of one row (cc_sample_rows;
    include/coldcompress.h has the contract): row r is drawn under seeds[r] at the position input_pos[r], and its probabilities, token
    and kept count are the bits sample_nucleus gives for that row alone.  A view with a row stride is passed as it is, without a
    copy.  seeds: T Python integers; input_pos: a contiguous int32 DEVICE tensor of T elements, read by the kernels (a captured
    call advances through it).  -> (probs [T, V], idx [T] int32), and with `return_n_kept` an int32 tensor of T counts as a third."""
    if not logits_2d.is_cuda:
        _host(logits_2d, "sample_rows logits")
    x = logits_2d
    if x.dim() != 2 or x.dtype not in _DT or x.shape[0] < 1 or x.shape[1] < 1:
        raise _abi.ColdCompressError(f"sample_rows: logits must be [T, V] in float32 / bfloat16 / float16, got {x.dtype} {tuple(x.shape)}")
    T, V = x.shape
    if T > SAMPLE_MAX_ROWS:
        raise _abi.ColdCompressError(f"sample_rows: at most {SAMPLE_MAX_ROWS} rows per call, got {T}")
    seeds = [int(s) & (2 ** 64 - 1) for s in seeds]
    if len(seeds) != T:
        raise _abi.ColdCompressError(f"sample_rows: {T} rows need {T} seeds, got {len(seeds)}")
    if not (input_pos.is_cuda and input_pos.dtype == torch.int32 and input_pos.numel() == T and input_pos.is_contiguous()):
        raise _abi.ColdCompressError(f"sample_rows: input_pos must be a contiguous int32 device tensor of {T} elements, got "
                                     f"{input_pos.dtype} {tuple(input_pos.shape)} on {input_pos.device}")
    if not float(temperature) > 0:
        raise _abi.ColdCompressError(f"sample_rows: temperature must be > 0, got {temperature}")
    p = 1.0 if top_p is None else float(top_p)
    mp = 0.0 if min_p is None else float(min_p)
    if not p > 0:
        raise _abi.ColdCompressError(f"sample_rows: top_p must be > 0 (>= 1: off), got {top_p}")
    if not mp <= 1:
        raise _abi.ColdCompressError(f"sample_rows: min_p must be <= 1 (<= 0: off), got {min_p}")
    if V > 1 and x.stride(1) != 1 or (T > 1 and x.stride(0) < V):
        x = x.contiguous()
    stride = x.stride(0) if T > 1 else V
    probs = torch.empty((T, V), dtype=x.dtype, device=x.device)
    idx = torch.empty((T,), dtype=torch.int32, device=x.device)
    n_kept = torch.empty((T,), dtype=torch.int32, device=x.device) if return_n_kept else None
    ws = _SR_WS.get(x.device)
    if ws is None:  # (one buffer for every T: 6 MB; a captured call holds its address)
        ws = _SR_WS[x.device] = torch.empty(int(_abi.lib()["cc_sample_rows_workspace_bytes"](SAMPLE_MAX_ROWS)), dtype=torch.uint8,
                                            device=x.device)
    k = 0 if top_k is None else max(0, min(int(top_k), 2 ** 31 - 1))
    _abi.call("cc_sample_rows", _p(x), T, V, int(stride), _DT[x.dtype], float(temperature), k, p, mp, (C.c_uint64 * T)(*seeds), _p(input_pos),
              _p(probs), _p(idx), _p(n_kept), _p(ws), ws.numel(), _stream())
    return (probs, idx, n_kept) if return_n_kept else (probs, idx)


_SR_WS = {}


def logprob_rows(logits_2d, targets=None, fallback=None, want_rank=True):
    """Per-row log-probability of a target token, the row's log-sum-exp and the target's rank, in fp32 from the logits themselves
    (cc_logprob_rows; include/coldcompress.h has the contract).  logits_2d: [T, V] (or one row [V]) on the device, T <= 64; a view
    with a row stride is passed as it is, without a copy.  targets / fallback: int32 DEVICE tensors of T elements or None; row r is
    scored against targets[r] where that is >= 0 and against fallback[r] otherwise — both are read by the kernels, so a captured
    step scores the token of each replay.  -> (logprob [T] fp32, lse [T] fp32, rank [T] int32, or None without `want_rank`)."""
    if not logits_2d.is_cuda:
        _host(logits_2d, "logprob_rows logits")
    x = logits_2d.view(1, -1) if logits_2d.dim() == 1 else logits_2d
    if x.dim() != 2 or x.dtype not in _DT:
        raise _abi.ColdCompressError(f"logprob_rows: logits must be [T, V] in float32 / bfloat16 / float16, got {x.dtype} {tuple(x.shape)}")
    T, V = x.shape
    if V > 1 and x.stride(1) != 1 or (T > 1 and x.stride(0) < V):
        x = x.contiguous()
    stride = x.stride(0) if T > 1 else V
    for name, t in (("targets", targets), ("fallback", fallback)):
        if t is not None and not (t.is_cuda and t.dtype == torch.int32 and t.numel() == T and t.is_contiguous()):
            raise _abi.ColdCompressError(f"logprob_rows: {name} must be a contiguous int32 device tensor of {T} elements, got {t.dtype} "
                                         f"{tuple(t.shape)} on {t.device}")
    logprob = torch.empty((T,), dtype=torch.float32, device=x.device)
    lse = torch.empty((T,), dtype=torch.float32, device=x.device)
    rank = torch.empty((T,), dtype=torch.int32, device=x.device) if want_rank else None
    ws = _LP_WS.get(x.device)
    if ws is None:
        ws = _LP_WS[x.device] = torch.empty(int(_abi.lib()["cc_logprob_rows_workspace_bytes"]()), dtype=torch.uint8, device=x.device)
    _abi.call("cc_logprob_rows", _p(x), T, V, int(stride), _DT[x.dtype], _p(targets), _p(fallback), _p(logprob), _p(lse), _p(rank), _p(ws),
              ws.numel(), _stream())
    return logprob, lse, rank


_LP_WS = {}


def logprob_topn(logits_2d, n, targets=None, fallback=None):
    """logprob_rows' three results and each row's `n` most likely alternatives (cc_logprob_topn; include/coldcompress.h has the
    contract): the ids of the n first elements in the order (larger logit first, equal logits by lower id, NaN never) and their fp32
    log-probabilities, padded with -1 / NaN where the row has fewer.  logits_2d, targets and fallback as logprob_rows takes them (a
    strided view is passed as it is; both None: no target, NaN and -1); 1 <= n <= 20.
    -> (logprob [T] fp32, lse [T] fp32, rank [T] int32, top_ids [T, n] int32, top_logprobs [T, n] fp32)."""
    if not logits_2d.is_cuda:
        _host(logits_2d, "logprob_topn logits")
    x = logits_2d.view(1, -1) if logits_2d.dim() == 1 else logits_2d
    if x.dim() != 2 or x.dtype not in _DT:
        raise _abi.ColdCompressError(f"logprob_topn: logits must be [T, V] in float32 / bfloat16 / float16, got {x.dtype} {tuple(x.shape)}")
    if not 1 <= int(n) <= LOGPROB_MAX_TOPN:
        raise _abi.ColdCompressError(f"logprob_topn: n must be in 1..{LOGPROB_MAX_TOPN}, got {n}")
    n = int(n)
    T, V = x.shape
    if V > 1 and x.stride(1) != 1 or (T > 1 and x.stride(0) < V):
        x = x.contiguous()
    stride = x.stride(0) if T > 1 else V
    for name, t in (("targets", targets), ("fallback", fallback)):
        if t is not None and not (t.is_cuda and t.dtype == torch.int32 and t.numel() == T and t.is_contiguous()):
            raise _abi.ColdCompressError(f"logprob_topn: {name} must be a contiguous int32 device tensor of {T} elements, got {t.dtype} "
                                         f"{tuple(t.shape)} on {t.device}")
    logprob = torch.empty((T,), dtype=torch.float32, device=x.device)
    lse = torch.empty((T,), dtype=torch.float32, device=x.device)
    rank = torch.empty((T,), dtype=torch.int32, device=x.device)
    top_ids = torch.empty((T, n), dtype=torch.int32, device=x.device)
    top_logprobs = torch.empty((T, n), dtype=torch.float32, device=x.device)
    ws = _LPT_WS.get(x.device)
    if ws is None:
        ws = _LPT_WS[x.device] = torch.empty(int(_abi.lib()["cc_logprob_topn_workspace_bytes"]()), dtype=torch.uint8, device=x.device)
    _abi.call("cc_logprob_topn", _p(x), T, V, int(stride), _DT[x.dtype], _p(targets), _p(fallback), n, _p(logprob), _p(lse), _p(rank),
              _p(top_ids), _p(top_logprobs), _p(ws), ws.numel(), _stream())
    return logprob, lse, rank, top_ids, top_logprobs


LOGPROB_MAX_TOPN = 20  # (CC_LOGPROB_MAX_TOPN)
_LPT_WS = {}


def _counts_ok(what, V, prompt_count, gen_count, gen_start):
    for name, t, n in (("prompt_count", prompt_count, V), ("gen_count", gen_count, V), ("gen_start", gen_start, 1)):
        if not (t.is_cuda and t.dtype == torch.int32 and t.numel() == n and t.is_contiguous()):
            raise _abi.ColdCompressError(f"{what}: {name} must be a contiguous int32 device tensor of {n} elements, got {t.dtype} "
                                         f"{tuple(t.shape)} on {t.device}")


def token_counts_add(prompt_count, gen_count, tokens, first_pos, gen_start):
    """Add `tokens` (an int32 DEVICE tensor: the inputs at positions first_pos .. first_pos + n - 1, first_pos a host int) to the
    token-history state of cc_logits_penalize, in place: each to `gen_count` where its position is >= *gen_start and to `prompt_count`
    otherwise (cc_token_counts_add; include/coldcompress.h has the contract).  Tokens outside the vocabulary count nothing."""
    V = prompt_count.numel()
    _counts_ok("token_counts_add", V, prompt_count, gen_count, gen_start)
    if not (tokens.is_cuda and tokens.dtype == torch.int32 and tokens.is_contiguous()):
        raise _abi.ColdCompressError(f"token_counts_add: tokens must be a contiguous int32 device tensor, got {tokens.dtype} "
                                     f"{tuple(tokens.shape)} on {tokens.device}")
    _abi.call("cc_token_counts_add", _p(prompt_count), _p(gen_count), V, _p(tokens), tokens.numel(), int(first_pos), _p(gen_start),
              _stream())


def logits_penalize(logits_2d, prompt_count, gen_count, gen_start, tokens=None, pos=None, repetition_penalty=1.0, frequency_penalty=0.0,
                    presence_penalty=0.0, bias=None, out=None):
    """The repetition / frequency / presence penalties and the logit bias on T <= 4 rows of logits, and the rows' input tokens counted
    into the state, in one launch (cc_logits_penalize; include/coldcompress.h has the contract).  logits_2d: [T, V] (or one row [V])
    on the device; a view with a row stride is passed as it is.  tokens / pos: int32 DEVICE tensors of T elements — the inputs of the
    T steps and their positions, read by the kernel, so a captured step counts the token of each replay — or None: count nothing.
    bias: fp32 [V] on the device or None.  out: None (a new contiguous tensor) or `logits_2d` itself (in place).  -> out."""
    if not logits_2d.is_cuda:
        _host(logits_2d, "logits_penalize logits")
    x = logits_2d.view(1, -1) if logits_2d.dim() == 1 else logits_2d
    if x.dim() != 2 or x.dtype not in _DT:
        raise _abi.ColdCompressError(f"logits_penalize: logits must be [T, V] in float32 / bfloat16 / float16, got {x.dtype} {tuple(x.shape)}")
    T, V = x.shape
    inplace = out is not None
    if inplace and out is not logits_2d:
        raise _abi.ColdCompressError("logits_penalize: out must be None or the logits tensor itself")
    if V > 1 and x.stride(1) != 1 or (T > 1 and x.stride(0) < V):
        if inplace:
            raise _abi.ColdCompressError("logits_penalize: in place needs rows of unit element stride that do not overlap")
        x = x.contiguous()
    stride = x.stride(0) if T > 1 else V
    _counts_ok("logits_penalize", V, prompt_count, gen_count, gen_start)
    if (tokens is None) != (pos is None):
        raise _abi.ColdCompressError("logits_penalize: tokens and pos come together")
    for name, t in (("tokens", tokens), ("pos", pos)):
        if t is not None and not (t.is_cuda and t.dtype == torch.int32 and t.numel() == T and t.is_contiguous()):
            raise _abi.ColdCompressError(f"logits_penalize: {name} must be a contiguous int32 device tensor of {T} elements, got {t.dtype} "
                                         f"{tuple(t.shape)} on {t.device}")
    if bias is not None and not (bias.is_cuda and bias.dtype == torch.float32 and bias.numel() == V and bias.is_contiguous()):
        raise _abi.ColdCompressError(f"logits_penalize: bias must be a contiguous float32 device tensor of {V} elements, got {bias.dtype} "
                                     f"{tuple(bias.shape)} on {bias.device}")
    y = x if inplace else torch.empty((T, stride), dtype=x.dtype, device=x.device)[:, :V]  # (one row stride serves both sides)
    _abi.call("cc_logits_penalize", _p(x), _p(y), T, V, int(stride), _DT[x.dtype], _p(prompt_count), _p(gen_count), _p(tokens), _p(pos),
              _p(gen_start), float(repetition_penalty), float(frequency_penalty), float(presence_penalty), _p(bias), _stream())
    return logits_2d if inplace else y


CONSTRAIN_MAX_BW_TOKENS = 4096  # (CC_CONSTRAIN_MAX_BW_TOKENS)
CONSTRAIN_SLICE = 1024  # (CC_CONSTRAIN_SLICE: candidate starts per workgroup of the ban pass)


def _i32_ok(what, name, t, n=None):
    if not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and (n is None or t.numel() == n)):
        raise _abi.ColdCompressError(f"{what}: {name} must be a contiguous int32 device tensor{'' if n is None else f' of {n} elements'}, "
                                     f"got {t.dtype} {tuple(t.shape)} on {t.device}")


def token_history_write(hist, tokens, first_pos=0):
    """hist[first_pos + i] = tokens[i] for the positions inside the history (int32 DEVICE tensors; first_pos a host int): the prompt
    of cc_logits_constrain's positional history in one launch (cc_token_history_write; include/coldcompress.h has the contract)."""
    _i32_ok("token_history_write", "hist", hist)
    _i32_ok("token_history_write", "tokens", tokens)
    _abi.call("cc_token_history_write", _p(hist), hist.numel(), _p(tokens), tokens.numel(), int(first_pos), _stream())


def logits_constrain(logits_2d, hist, gen_start, tokens, pos, ngram=0, ngram_from_gen=False, min_new_tokens=0, term_ids=None,
                     bw_tokens=None, bw_offsets=None, out=None):
    """n-gram blocking, banned sequences and a minimum length on T <= 4 rows of logits: every banned element becomes -inf, every other
    keeps its bits, and the rows' input tokens are stored into the positional history (cc_logits_constrain; include/coldcompress.h has
    the contract).  logits_2d: [T, V] (or one row [V]) on the device; a view with a row stride is passed as it is.  hist: int32 [cap],
    gen_start: int32 [1], pos: int32, at least one element (row t is at position pos[0] + t), tokens: int32 [T] or None (the prefill's
    row) — all DEVICE tensors the kernel reads, so a captured step advances.  term_ids: int32 device tensor or None; bw_tokens /
    bw_offsets: the banned sequences back to back and their n + 1 offsets, or None.  out: None (a new contiguous tensor) or `logits_2d`
    itself (in place).  -> out."""
    if not logits_2d.is_cuda:
        _host(logits_2d, "logits_constrain logits")
    x = logits_2d.view(1, -1) if logits_2d.dim() == 1 else logits_2d
    if x.dim() != 2 or x.dtype not in _DT:
        raise _abi.ColdCompressError(f"logits_constrain: logits must be [T, V] in float32 / bfloat16 / float16, got {x.dtype} {tuple(x.shape)}")
    T, V = x.shape
    inplace = out is not None
    if inplace and out is not logits_2d:
        raise _abi.ColdCompressError("logits_constrain: out must be None or the logits tensor itself")
    if V > 1 and x.stride(1) != 1 or (T > 1 and x.stride(0) < V):
        if inplace:
            raise _abi.ColdCompressError("logits_constrain: in place needs rows of unit element stride that do not overlap")
        x = x.contiguous()
    stride = x.stride(0) if T > 1 else V
    _i32_ok("logits_constrain", "hist", hist)
    _i32_ok("logits_constrain", "gen_start", gen_start, 1)
    _i32_ok("logits_constrain", "pos", pos)
    if pos.numel() < 1:
        raise _abi.ColdCompressError("logits_constrain: pos must hold the first row's position")
    if tokens is not None:
        _i32_ok("logits_constrain", "tokens", tokens, T)
    if term_ids is not None:
        _i32_ok("logits_constrain", "term_ids", term_ids)
    if (bw_tokens is None) != (bw_offsets is None):
        raise _abi.ColdCompressError("logits_constrain: bw_tokens and bw_offsets come together")
    n_bw = 0
    if bw_tokens is not None:
        _i32_ok("logits_constrain", "bw_tokens", bw_tokens)
        _i32_ok("logits_constrain", "bw_offsets", bw_offsets)
        n_bw = bw_offsets.numel() - 1
        if n_bw < 0 or bw_tokens.numel() > CONSTRAIN_MAX_BW_TOKENS:
            raise _abi.ColdCompressError(f"logits_constrain: bw_offsets needs n + 1 elements and bw_tokens at most {CONSTRAIN_MAX_BW_TOKENS}")
    y = x if inplace else torch.empty((T, stride), dtype=x.dtype, device=x.device)[:, :V]  # (one row stride serves both sides)
    _abi.call("cc_logits_constrain", _p(x), _p(y), T, V, int(stride), _DT[x.dtype], _p(hist), hist.numel(), _p(tokens), _p(pos),
              _p(gen_start), int(ngram), int(bool(ngram_from_gen)), int(min_new_tokens), _p(term_ids),
              0 if term_ids is None else term_ids.numel(), _p(bw_tokens), _p(bw_offsets), n_bw, _stream())
    return logits_2d if inplace else y


def _streams_rows(what, logits_2d, states, tokens, pos, out):
    """The checks the two streams entry points share -> (x, y, T, V, stride, inplace)."""
    if not logits_2d.is_cuda:
        _host(logits_2d, f"{what} logits")
    x = logits_2d
    if x.dim() != 2 or x.dtype not in _DT:
        raise _abi.ColdCompressError(f"{what}: logits must be [T, V] in float32 / bfloat16 / float16, got {x.dtype} {tuple(x.shape)}")
    T, V = x.shape
    if not 1 <= T <= GEMV_MULTI_MAX_T:
        raise _abi.ColdCompressError(f"{what}: 1..{GEMV_MULTI_MAX_T} rows per call, got {T}")
    if len(states) != T:
        raise _abi.ColdCompressError(f"{what}: {T} rows need {T} records, got {len(states)}")
    inplace = out is not None
    if inplace and out is not logits_2d:
        raise _abi.ColdCompressError(f"{what}: out must be None or the logits tensor itself")
    if V > 1 and x.stride(1) != 1 or (T > 1 and x.stride(0) < V):
        if inplace:
            raise _abi.ColdCompressError(f"{what}: in place needs rows of unit element stride that do not overlap")
        x = x.contiguous()
    stride = x.stride(0) if T > 1 else V
    for name, t in (("tokens", tokens), ("pos", pos)):
        if t is not None:
            _i32_ok(what, name, t, T)
    y = x if inplace else torch.empty((T, stride), dtype=x.dtype, device=x.device)[:, :V]  # (one row stride serves both sides)
    return x, y, T, V, int(stride), inplace


def logits_penalize_streams(logits_2d, states, tokens=None, pos=None, out=None):
    """logits_penalize for T <= 4 rows that belong to DIFFERENT sequences, in one launch (cc_logits_penalize_streams;
    include/coldcompress.h has the contract): row t is penalised against states[t] alone and carries the bits logits_penalize gives for
    that row at T = 1 on that state.  states: T records, each None (no penalties for the row: its bits as they are) or
    (prompt_count, gen_count, gen_start, repetition_penalty, frequency_penalty, presence_penalty, bias) as logits_penalize takes them;
    no two records may name one count table.  tokens / pos: int32 DEVICE tensors of T elements — row t's input token and its own
    position — or both None: count nothing.  out: None (a new contiguous tensor) or `logits_2d` itself (in place).  -> out."""
    what = "logits_penalize_streams"
    if (tokens is None) != (pos is None):
        raise _abi.ColdCompressError(f"{what}: tokens and pos come together")
    x, y, T, V, stride, inplace = _streams_rows(what, logits_2d, states, tokens, pos, out)
    recs = (_abi.PenaltyRow * T)()
    tables = set()
    for t, s in enumerate(states):
        if s is None:
            continue
        prompt_count, gen_count, gen_start, r, f, p, bias = s
        _counts_ok(what, V, prompt_count, gen_count, gen_start)
        if bias is not None and not (bias.is_cuda and bias.dtype == torch.float32 and bias.numel() == V and bias.is_contiguous()):
            raise _abi.ColdCompressError(f"{what}: bias must be a contiguous float32 device tensor of {V} elements, got {bias.dtype} "
                                         f"{tuple(bias.shape)} on {bias.device}")
        for c in (prompt_count, gen_count):
            if c.data_ptr() in tables:
                raise _abi.ColdCompressError(f"{what}: record {t} names a count table that another record names: one object is one sequence's state")
        tables.update((prompt_count.data_ptr(), gen_count.data_ptr()))
        recs[t] = _abi.PenaltyRow(prompt_count.data_ptr(), gen_count.data_ptr(), gen_start.data_ptr(), None if bias is None else bias.data_ptr(),
                                  float(r), float(f), float(p))
    _abi.call("cc_logits_penalize_streams", _p(x), _p(y), T, V, stride, _DT[x.dtype], recs, _p(tokens), _p(pos), _stream())
    return logits_2d if inplace else y


def logits_constrain_streams(logits_2d, states, tokens, pos, out=None):
    """logits_constrain for T <= 4 rows that belong to DIFFERENT sequences (cc_logits_constrain_streams; include/coldcompress.h has the
    contract): row t sits at its own position pos[t] over states[t]'s history and carries the bits logits_constrain gives for that row
    at T = 1 on that state; hist[pos[t]] = tokens[t] is stored.  states: T records, each None (no rules for the row) or
    (hist, gen_start, ngram, ngram_from_gen, min_new_tokens, term_ids, bw_tokens, bw_offsets) as logits_constrain takes them; no two
    records may share one hist.  pos: int32 DEVICE tensor of T elements; tokens: likewise, or None (the prefill's row).  out: None (a new
    contiguous tensor) or `logits_2d` itself (in place).  -> out."""
    what = "logits_constrain_streams"
    if pos is None:
        raise _abi.ColdCompressError(f"{what}: pos must hold every row's position")
    x, y, T, V, stride, inplace = _streams_rows(what, logits_2d, states, tokens, pos, out)
    recs = (_abi.ConstraintRow * T)()
    hists = set()
    for t, s in enumerate(states):
        if s is None:
            continue
        hist, gen_start, ngram, ngram_from_gen, min_new_tokens, term_ids, bw_tokens, bw_offsets = s
        _i32_ok(what, "hist", hist)
        _i32_ok(what, "gen_start", gen_start, 1)
        if hist.data_ptr() in hists:
            raise _abi.ColdCompressError(f"{what}: record {t} shares its hist with another record: one object is one sequence's state")
        hists.add(hist.data_ptr())
        if term_ids is not None:
            _i32_ok(what, "term_ids", term_ids)
        if (bw_tokens is None) != (bw_offsets is None):
            raise _abi.ColdCompressError(f"{what}: bw_tokens and bw_offsets come together")
        n_bw = 0
        if bw_tokens is not None:
            _i32_ok(what, "bw_tokens", bw_tokens)
            _i32_ok(what, "bw_offsets", bw_offsets)
            n_bw = bw_offsets.numel() - 1
            if n_bw < 0 or bw_tokens.numel() > CONSTRAIN_MAX_BW_TOKENS:
                raise _abi.ColdCompressError(f"{what}: bw_offsets needs n + 1 elements and bw_tokens at most {CONSTRAIN_MAX_BW_TOKENS}")
        ptr = lambda t_: None if t_ is None else t_.data_ptr()  # noqa: E731
        recs[t] = _abi.ConstraintRow(hist.data_ptr(), hist.numel(), gen_start.data_ptr(), int(ngram), int(bool(ngram_from_gen)),
                                     int(min_new_tokens), ptr(term_ids), 0 if term_ids is None else term_ids.numel(), ptr(bw_tokens),
                                     ptr(bw_offsets), n_bw)
    _abi.call("cc_logits_constrain_streams", _p(x), _p(y), T, V, stride, _DT[x.dtype], recs, _p(tokens), _p(pos), _stream())
    return logits_2d if inplace else y
