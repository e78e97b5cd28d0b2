"""Weight-only int8, int4 and MXFP4 models: the checkpoint formats, quantisers and modules of the reference's weight-only paths (ref:
quantize.py:25-57, 60-163, 333-404, 407-530; generation_utils.py:539-553), so that its `model_int8.pth` checkpoints load here and new
int8 and int4 ones can be written.

int8: every `nn.Linear` (the LM head included; embeddings are not linears and stay as they are) becomes a `WeightOnlyInt8Linear`
with the state-dict keys `<fqn>.weight` (int8 [out, in]), `<fqn>.scales` ([out], the model dtype) and `<fqn>.bias`.  Per row of
`w = weight.float()`: lo = min(min w, 0), hi = max(max w, 0), s32 = max(max(-lo, hi) / 127.5, fp32 eps) in fp32,
q = clamp(round_half_even(w / s32), -128, 127), scales = s32 rounded to the model dtype (include/coldcompress.h,
cc_gemv_fused_w8).  The module's forward is the reference's formula in torch — prefill and CPU use it; single-token decode on
the device streams the int8 weights through cc_gemv_fused_w8 (model.py hands each linear's scales to glue.gemv_fused).

int4 (group-wise, G in {32, 64, 128, 256} columns per group): every `nn.Linear` becomes a `WeightOnlyInt4Linear` with the keys
`<fqn>.weight`, `<fqn>.scales_and_zeros` and `<fqn>.bias`.  The codes and the (scale, zero) pairs are the reference's
`group_quantize_tensor(weight.to(bfloat16), 4, G)` bit for bit: per group of G columns, in bf16 torch arithmetic,
scales = (max - min).clamp(min=1e-6) / 15, zeros = min + scales * 8, q = clamp(round((w - (zeros - scales * 8)) / scales), 0, 15).
The code layout is this project's (the reference's tinygemm tile packing is a CUDA artefact): `weight` is uint8 [out, in / 2], two
codes per byte, column 2j in the low nibble.  `scales_and_zeros` is bf16 [in / G, out, 2] (scale, zero) in the state dict, the
reference's layout; the module holds it per row, [out, in / G, 2], the layout the decode GEMV streams (cc_gemv_fused_w4), and
converts on load and save.  forward = F.linear(x, bf16((q - 8) * s + z in fp32)) (+ bias), one linear dequantised at a time.

MXFP4 (OCP microscaling FP4, this project's own extension: the reference has no such mode): every `nn.Linear` becomes a
`WeightOnlyMxfp4Linear` with the keys `<fqn>.weight` (uint8 [out, in / 2], two e2m1 codes per byte, column 2j in the low nibble),
`<fqn>.block_scales` (uint8 [out, in / 32], one e8m0 byte per row and block of 32 consecutive columns, value 2^(byte - 127)) and
`<fqn>.bias`.  Per block of `w = weight.float()`: e = the smallest integer with amax <= 6 * 2^e (from frexp, no division), clamped to
[-120, 120], -120 for an all-zero block; codes = round-to-nearest of w * 2^-e on sign x {0, 0.5, 1, 1.5, 2, 3, 4, 6}, ties to the even
mantissa, -0 keeping its sign; byte = e + 127, in [7, 247] (include/coldcompress.h, cc_gemv_fused_mx4).  A non-finite weight is
refused.  forward = F.linear(x, bf16(code * 2^e)) (+ bias), the dequantised weight being exact in bf16; single-token decode on the
device streams the codes through cc_gemv_fused_mx4.  bf16 models only, in_features a multiple of 32.

    python -m cold_compress_amd.harness.quantize --checkpoint_path DIR/model.pth --mode int8               # -> DIR/model_int8.pth
    python -m cold_compress_amd.harness.quantize --checkpoint_path DIR/model.pth --mode int4 --groupsize G  # -> DIR/model_int4.gG.pth
    python -m cold_compress_amd.harness.quantize --checkpoint_path DIR/model.pth --mode mxfp4              # -> DIR/model_mxfp4.pth
"""
import argparse
import time
from pathlib import Path

import torch
import torch.nn as nn
import torch.nn.functional as F


def quantize_per_channel_int8(w: torch.Tensor):
    """-> (int8 codes [N, K], fp32 scales [N]) of the symmetric per-output-row grid [-128, 127] (scale = range / 255)."""
    w = w.float()
    lo, hi = torch.aminmax(w, dim=1)
    lo = torch.minimum(lo, torch.zeros_like(lo))
    hi = torch.maximum(hi, torch.zeros_like(hi))
    s32 = torch.clamp(torch.maximum(-lo, hi) / 127.5, min=torch.finfo(torch.float32).eps)
    q = torch.clamp(torch.round(w / s32.unsqueeze(-1)), -128, 127).to(torch.int8)
    return q, s32


class WeightOnlyInt8Linear(nn.Module):
    __constants__ = ["in_features", "out_features"]

    def __init__(self, in_features: int, out_features: int, bias: bool = False, device=None, dtype=None) -> None:
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.register_buffer("weight", torch.empty((out_features, in_features), dtype=torch.int8, device=device))
        self.register_buffer("scales", torch.ones(out_features, dtype=dtype or torch.bfloat16, device=device))
        if bias:
            self.register_buffer("bias", torch.zeros(out_features, dtype=dtype or torch.bfloat16, device=device))
        else:
            self.register_parameter("bias", None)

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        """The reference's three rounding points: F.linear in the input dtype, * scales, += bias."""
        output = F.linear(input, self.weight.to(dtype=input.dtype)) * self.scales
        if self.bias is not None:
            output += self.bias
        return output

    def extra_repr(self) -> str:
        return f"in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}"


def replace_linear_weight_only_int8_per_channel(module: nn.Module) -> None:
    for name, child in module.named_children():
        if isinstance(child, nn.Linear):
            setattr(module, name, WeightOnlyInt8Linear(child.in_features, child.out_features, bias=child.bias is not None,
                                                       device=child.weight.device, dtype=child.weight.dtype))
        else:
            replace_linear_weight_only_int8_per_channel(child)


class WeightOnlyInt8QuantHandler:
    def __init__(self, mod: nn.Module):
        self.mod = mod

    @torch.no_grad()
    def create_quantized_state_dict(self):
        sd = self.mod.state_dict()
        for fqn, mod in self.mod.named_modules():
            if isinstance(mod, nn.Linear):
                q, s32 = quantize_per_channel_int8(mod.weight)
                sd[f"{fqn}.weight"] = q
                sd[f"{fqn}.scales"] = s32.to(mod.weight.dtype)
                if mod.bias is not None:
                    sd[f"{fqn}.bias"] = mod.bias
        return sd

    def convert_for_runtime(self) -> nn.Module:
        replace_linear_weight_only_int8_per_channel(self.mod)
        return self.mod


def is_int8_linear(m) -> bool:
    return isinstance(m, WeightOnlyInt8Linear)


INT4_GROUPSIZES = (32, 64, 128, 256)


def group_quantize_int4(w: torch.Tensor, groupsize: int):
    """-> (int32 codes [N, K] in [0, 15], bf16 scales [N, K / G], bf16 zeros [N, K / G]) of `w` (bf16 [N, K]): the reference's
    get_group_qparams + group_quantize_tensor_from_qparams at n_bit = 4, op for op, so every step rounds to w's dtype."""
    assert w.dim() == 2 and w.shape[1] % groupsize == 0 and groupsize > 1
    g = w.reshape(-1, groupsize)
    assert not torch.isnan(g).any()
    hi = g.amax(dim=1, keepdim=True)
    lo = g.amin(dim=1, keepdim=True)
    scales = (hi - lo).clamp(min=1e-6) / 15
    zeros = lo + scales * 8
    scales, zeros = scales.to(torch.bfloat16), zeros.to(torch.bfloat16)
    base = zeros - scales * 8
    q = g.sub(base).div(scales).round().clamp_(0, 15).to(torch.int32).reshape_as(w)
    return q, scales.reshape(w.shape[0], -1), zeros.reshape(w.shape[0], -1)


def pack_int4(q: torch.Tensor) -> torch.Tensor:
    """int codes [N, K] in [0, 15] -> uint8 [N, K / 2], column 2j in the low nibble of byte j."""
    q = q.to(torch.uint8)
    return q[:, 0::2] | (q[:, 1::2] << 4)


def unpack_int4(packed: torch.Tensor) -> torch.Tensor:
    """uint8 [N, K / 2] -> int32 codes [N, K]."""
    return torch.stack([packed & 15, packed >> 4], dim=-1).reshape(packed.shape[0], -1).to(torch.int32)


def dequantize_int4(packed: torch.Tensor, qparams: torch.Tensor, groupsize: int) -> torch.Tensor:
    """fp32 [N, K] = (q - 8) * scale + zero per group (the reference's group_dequantize_tensor); qparams [N, K / G, 2] per row."""
    q = unpack_int4(packed)
    N, K = q.shape
    sz = qparams.float()
    w = (q.view(N, K // groupsize, groupsize) - 8) * sz[..., 0:1] + sz[..., 1:2]
    return w.view(N, K)


_DEQUANT_BLOCK = 1 << 24  # weights dequantised per block in WeightOnlyInt4Linear.forward


class WeightOnlyInt4Linear(nn.Module):
    __constants__ = ["in_features", "out_features", "groupsize"]

    def __init__(self, in_features: int, out_features: int, bias: bool = False, device=None, dtype=None, groupsize: int = 128) -> None:
        super().__init__()
        if groupsize not in INT4_GROUPSIZES:
            raise ValueError(f"int4 groupsize must be one of {INT4_GROUPSIZES}, got {groupsize}")
        if in_features % groupsize:
            raise ValueError(f"int4 weight-only needs in_features ({in_features}) to be a multiple of the groupsize ({groupsize})")
        self.in_features, self.out_features, self.groupsize = in_features, out_features, groupsize
        self.register_buffer("weight", torch.empty((out_features, in_features // 2), dtype=torch.uint8, device=device))
        # per row [out, in / G, 2] (scale, zero); the state dict holds the reference's [in / G, out, 2]
        self.register_buffer("scales_and_zeros", torch.empty((out_features, in_features // groupsize, 2), dtype=torch.bfloat16,
                                                             device=device))
        if bias:
            self.register_buffer("bias", torch.zeros(out_features, dtype=torch.bfloat16, device=device))
        else:
            self.register_parameter("bias", None)

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        super()._save_to_state_dict(destination, prefix, keep_vars)
        destination[prefix + "scales_and_zeros"] = self.scales_and_zeros.transpose(0, 1).contiguous()

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        k = prefix + "scales_and_zeros"
        if k in state_dict and state_dict[k].dim() == 3:
            state_dict[k] = state_dict[k].transpose(0, 1).contiguous()
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        """F.linear(x, bf16(group dequantised W)) (+= bias): bf16 activations, the weight dequantised in fp32 and rounded once.
        The rows are dequantised in blocks into one bf16 weight, so the int32 / fp32 temporaries stay small (the 8B LM head's
        would be several GB)."""
        w = torch.empty((self.out_features, self.in_features), dtype=torch.bfloat16, device=self.weight.device)
        rows = max(1, _DEQUANT_BLOCK // self.in_features)
        for r0 in range(0, self.out_features, rows):
            w[r0:r0 + rows] = dequantize_int4(self.weight[r0:r0 + rows], self.scales_and_zeros[r0:r0 + rows], self.groupsize)
        output = F.linear(input.to(torch.bfloat16), w)
        if self.bias is not None:
            output += self.bias
        return output

    def extra_repr(self) -> str:
        return (f"in_features={self.in_features}, out_features={self.out_features}, groupsize={self.groupsize}, "
                f"bias={self.bias is not None}")


def replace_linear_int4(module: nn.Module, groupsize: int) -> None:
    for name, child in module.named_children():
        if isinstance(child, nn.Linear):
            setattr(module, name, WeightOnlyInt4Linear(child.in_features, child.out_features, bias=child.bias is not None,
                                                       device=child.weight.device, groupsize=groupsize))
        else:
            replace_linear_int4(child, groupsize)


class WeightOnlyInt4QuantHandler:
    def __init__(self, mod: nn.Module, groupsize: int = 128):
        if groupsize not in INT4_GROUPSIZES:
            raise ValueError(f"int4 groupsize must be one of {INT4_GROUPSIZES}, got {groupsize}")
        self.mod = mod
        self.groupsize = groupsize

    @torch.no_grad()
    def create_quantized_state_dict(self):
        sd = self.mod.state_dict()
        for fqn, mod in self.mod.named_modules():
            if isinstance(mod, nn.Linear):
                if mod.in_features % self.groupsize:
                    raise ValueError(f"{fqn}: in_features {mod.in_features} is not a multiple of the int4 groupsize {self.groupsize}")
                q, scales, zeros = group_quantize_int4(mod.weight.to(torch.bfloat16), self.groupsize)
                sd[f"{fqn}.weight"] = pack_int4(q)
                sd[f"{fqn}.scales_and_zeros"] = torch.stack([scales, zeros], dim=-1).transpose(0, 1).contiguous()
                if mod.bias is not None:
                    sd[f"{fqn}.bias"] = mod.bias
        return sd

    def convert_for_runtime(self) -> nn.Module:
        replace_linear_int4(self.mod, self.groupsize)
        return self.mod


def is_int4_linear(m) -> bool:
    """The module with its (scale, zero) pairs and groupsize, not a bare uint8 weight."""
    return isinstance(m, WeightOnlyInt4Linear) and getattr(m, "scales_and_zeros", None) is not None and hasattr(m, "groupsize")


def check_int4_state_dict(model: nn.Module, sd) -> None:
    """Raise ValueError unless `sd` holds, for every int4 linear of the converted `model`, this project's uint8 [N, K / 2] codes, the
    bf16 [K / G, N, 2] (scale, zero) pairs and a [N] bias where the linear has one.  A reference (tinygemm) weight gets its own
    message."""
    for fqn, m in model.named_modules():
        if not isinstance(m, WeightOnlyInt4Linear):
            continue
        N, K, G = m.out_features, m.in_features, m.groupsize
        w, sz = sd.get(f"{fqn}.weight"), sd.get(f"{fqn}.scales_and_zeros")
        if w is None or sz is None:
            raise ValueError(f"{fqn}: missing weight or scales_and_zeros")
        if w.dtype == torch.int32 and w.dim() == 4:
            raise ValueError(f"{fqn}.weight is the reference's tinygemm-packed int32 {tuple(w.shape)} layout, which this project does "
                             "not read: re-quantise from the 16-bit model.pth with `python -m cold_compress_amd.harness.quantize "
                             f"--checkpoint_path DIR/model.pth --mode int4 --groupsize {G}`")
        if w.dtype != torch.uint8 or tuple(w.shape) != (N, K // 2):
            raise ValueError(f"{fqn}.weight: expected uint8 [{N}, {K // 2}] packed codes, got {w.dtype} {tuple(w.shape)}")
        if sz.dtype != torch.bfloat16 or tuple(sz.shape) != (K // G, N, 2):
            raise ValueError(f"{fqn}.scales_and_zeros: expected bf16 [{K // G}, {N}, 2] (groupsize {G}), got {sz.dtype} "
                             f"{tuple(sz.shape)}")
        b = sd.get(f"{fqn}.bias")
        if (b is None) != (m.bias is None) or (b is not None and tuple(b.shape) != (N,)):
            raise ValueError(f"{fqn}.bias: expected {'none' if m.bias is None else [N]}, got {None if b is None else tuple(b.shape)}")


MXFP4_BLOCK = 32
MXFP4_SCALE_BYTES = (7, 247)  # e + 127 for e in [-120, 120]: code x scale is exact in bf16
_E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def quantize_mxfp4(w: torch.Tensor, name: str = "weight"):
    """-> (uint8 codes [N, K / 2], two e2m1 codes per byte, column 2j in the low nibble; uint8 e8m0 scale bytes [N, K / 32]) of
    `w.float()` ([N, K], K a multiple of 32).  Per block: e = the smallest integer with amax <= 6 * 2^e, clamped to [-120, 120]
    (-120 for an all-zero block), the code the nearest of sign x {0, 0.5, 1, 1.5, 2, 3, 4, 6} to w * 2^-e, ties to the even
    mantissa.  Raises ValueError naming `name` for a non-finite weight."""
    if w.dim() != 2 or w.shape[1] % MXFP4_BLOCK:
        raise ValueError(f"{name}: MXFP4 needs a [N, K] weight with K a multiple of {MXFP4_BLOCK}, got {tuple(w.shape)}")
    w = w.float()
    if not torch.isfinite(w).all():
        raise ValueError(f"{name}: MXFP4 weight-only quantisation refuses a non-finite weight (inf or NaN)")
    N, K = w.shape
    b = w.reshape(N, K // MXFP4_BLOCK, MXFP4_BLOCK)
    amax = b.abs().amax(dim=-1)
    m, k = torch.frexp(amax)  # amax = m * 2^k, m in [0.5, 1); 6 = 0.75 * 2^3
    e = torch.where(m <= 0.75, k - 3, k - 2)
    e = torch.where(amax > 0, e, torch.full_like(e, -120)).clamp_(-120, 120)
    y = torch.ldexp(b, -e.unsqueeze(-1)).abs()  # a power-of-two product: exact
    code = ((y > 0.25).to(torch.uint8) + (y >= 0.75) + (y > 1.25) + (y >= 1.75) + (y > 2.5) + (y >= 3.5) + (y > 5.0)).to(torch.uint8)
    code |= torch.signbit(b).to(torch.uint8) << 3
    return pack_int4(code.reshape(N, K)).contiguous(), (e + 127).to(torch.uint8).contiguous()


def dequantize_mxfp4(packed: torch.Tensor, block_scales: torch.Tensor) -> torch.Tensor:
    """fp32 [N, K] = e2m1(code) * 2^(byte - 127); every value is exact in bf16 for scale bytes in [7, 247]."""
    q = unpack_int4(packed)
    N, K = q.shape
    mag = torch.tensor(_E2M1, dtype=torch.float32, device=packed.device)[(q & 7).long()]
    val = torch.where((q & 8) != 0, -mag, mag).view(N, K // MXFP4_BLOCK, MXFP4_BLOCK)
    return torch.ldexp(val, (block_scales.to(torch.int32) - 127).unsqueeze(-1)).view(N, K)


class WeightOnlyMxfp4Linear(nn.Module):
    __constants__ = ["in_features", "out_features"]

    def __init__(self, in_features: int, out_features: int, bias: bool = False, device=None, dtype=None) -> None:
        super().__init__()
        if in_features % MXFP4_BLOCK:
            raise ValueError(f"MXFP4 weight-only needs in_features ({in_features}) to be a multiple of {MXFP4_BLOCK}")
        self.in_features, self.out_features = in_features, out_features
        self.register_buffer("weight", torch.empty((out_features, in_features // 2), dtype=torch.uint8, device=device))
        self.register_buffer("block_scales", torch.empty((out_features, in_features // MXFP4_BLOCK), dtype=torch.uint8, device=device))
        if bias:
            self.register_buffer("bias", torch.zeros(out_features, dtype=torch.bfloat16, device=device))
        else:
            self.register_parameter("bias", None)

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        """F.linear(x, bf16(dequantised W)) (+= bias): bf16 activations; the rows are dequantised in blocks, as the int4 module's."""
        w = torch.empty((self.out_features, self.in_features), dtype=torch.bfloat16, device=self.weight.device)
        rows = max(1, _DEQUANT_BLOCK // self.in_features)
        for r0 in range(0, self.out_features, rows):
            w[r0:r0 + rows] = dequantize_mxfp4(self.weight[r0:r0 + rows], self.block_scales[r0:r0 + rows])
        output = F.linear(input.to(torch.bfloat16), w)
        if self.bias is not None:
            output += self.bias
        return output

    def extra_repr(self) -> str:
        return f"in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}"


def replace_linear_mxfp4(module: nn.Module) -> None:
    for name, child in module.named_children():
        if isinstance(child, nn.Linear):
            setattr(module, name, WeightOnlyMxfp4Linear(child.in_features, child.out_features, bias=child.bias is not None,
                                                        device=child.weight.device))
        else:
            replace_linear_mxfp4(child)


class WeightOnlyMxfp4QuantHandler:
    def __init__(self, mod: nn.Module):
        self.mod = mod

    @torch.no_grad()
    def create_quantized_state_dict(self):
        sd = self.mod.state_dict()
        for fqn, mod in self.mod.named_modules():
            if isinstance(mod, nn.Linear):
                if mod.in_features % MXFP4_BLOCK:
                    raise ValueError(f"{fqn}: in_features {mod.in_features} is not a multiple of the MXFP4 block of {MXFP4_BLOCK}")
                sd[f"{fqn}.weight"], sd[f"{fqn}.block_scales"] = quantize_mxfp4(mod.weight, fqn)
                if mod.bias is not None:
                    sd[f"{fqn}.bias"] = mod.bias
        return sd

    def convert_for_runtime(self) -> nn.Module:
        replace_linear_mxfp4(self.mod)
        return self.mod


def is_mxfp4_linear(m) -> bool:
    return isinstance(m, WeightOnlyMxfp4Linear)


def check_mxfp4_state_dict(model: nn.Module, sd) -> None:
    """Raise ValueError unless `sd` holds, for every MXFP4 linear of the converted `model`, uint8 [N, K / 2] codes, uint8 [N, K / 32]
    scale bytes, all of them in [7, 247], and a [N] bias where the linear has one."""
    lo, hi = MXFP4_SCALE_BYTES
    for fqn, m in model.named_modules():
        if not isinstance(m, WeightOnlyMxfp4Linear):
            continue
        N, K = m.out_features, m.in_features
        w, sc = sd.get(f"{fqn}.weight"), sd.get(f"{fqn}.block_scales")
        if w is None or sc is None:
            raise ValueError(f"{fqn}: missing weight or block_scales")
        if w.dtype != torch.uint8 or tuple(w.shape) != (N, K // 2):
            raise ValueError(f"{fqn}.weight: expected uint8 [{N}, {K // 2}] packed e2m1 codes, got {w.dtype} {tuple(w.shape)}")
        if sc.dtype != torch.uint8 or tuple(sc.shape) != (N, K // MXFP4_BLOCK):
            raise ValueError(f"{fqn}.block_scales: expected uint8 [{N}, {K // MXFP4_BLOCK}] e8m0 bytes, got {sc.dtype} {tuple(sc.shape)}")
        if sc.numel() and (int(sc.min()) < lo or int(sc.max()) > hi):
            raise ValueError(f"{fqn}.block_scales: scale bytes must lie in [{lo}, {hi}] (2^-120 .. 2^120), got "
                             f"[{int(sc.min())}, {int(sc.max())}]")
        b = sd.get(f"{fqn}.bias")
        if (b is None) != (m.bias is None) or (b is not None and tuple(b.shape) != (N,)):
            raise ValueError(f"{fqn}.bias: expected {'none' if m.bias is None else [N]}, got {None if b is None else tuple(b.shape)}")


def quantize(checkpoint_path: Path, mode: str = "int8", groupsize: int = None) -> Path:
    """Write the weight-only checkpoint next to `checkpoint_path` (model.pth -> model_int8.pth, model_int4.gG.pth or model_mxfp4.pth); the model
    shape is the `CONFIGS` entry named by the checkpoint's directory (ref: quantize.py's quantize())."""
    from .model import Transformer

    if mode not in ("int8", "int4", "mxfp4"):
        raise ValueError(f"quantisation mode {mode!r} is not supported (int8, int4 and mxfp4 weight-only only)")
    if mode == "int4" and groupsize not in INT4_GROUPSIZES:
        raise ValueError(f"int4 needs --groupsize, one of {INT4_GROUPSIZES} (got {groupsize})")
    checkpoint_path = Path(checkpoint_path)
    assert checkpoint_path.is_file(), checkpoint_path
    t0 = time.time()
    with torch.device("meta"):
        model = Transformer.from_name(checkpoint_path.parent.name)
    checkpoint = torch.load(str(checkpoint_path), mmap=True, weights_only=True)
    model.load_state_dict(checkpoint, assign=True)
    if mode == "int8":
        sd = WeightOnlyInt8QuantHandler(model).create_quantized_state_dict()
        out = checkpoint_path.parent / checkpoint_path.name.replace(".pth", "_int8.pth")
    elif mode == "mxfp4":
        sd = WeightOnlyMxfp4QuantHandler(model).create_quantized_state_dict()
        out = checkpoint_path.parent / checkpoint_path.name.replace(".pth", "_mxfp4.pth")
    else:
        sd = WeightOnlyInt4QuantHandler(model, groupsize).create_quantized_state_dict()
        out = checkpoint_path.parent / checkpoint_path.name.replace(".pth", f"_int4.g{groupsize}.pth")
    torch.save(sd, str(out))
    print(f"wrote {out} in {time.time() - t0:.1f} s")
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description="Quantise a checkpoint to weight-only int8, int4 or MXFP4.")
    ap.add_argument("--checkpoint_path", type=Path, required=True, help="DIR/model.pth, DIR named after a CONFIGS key")
    ap.add_argument("--mode", type=str, default="int8", choices=["int8", "int4", "mxfp4"],
                    help="int8, int4 or mxfp4 weight-only (GPTQ is not supported)")
    ap.add_argument("--groupsize", type=int, default=None, choices=list(INT4_GROUPSIZES),
                    help="int4: columns per (scale, zero) group; required, it names the output file (model_int4.gG.pth)")
    args = ap.parse_args(argv)
    if args.mode == "int4" and args.groupsize is None:
        ap.error("--mode int4 needs --groupsize (32, 64, 128 or 256)")
    quantize(args.checkpoint_path, args.mode, args.groupsize)


if __name__ == "__main__":
    main()
