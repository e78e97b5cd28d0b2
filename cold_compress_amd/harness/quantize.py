"""Weight-only int8 models: the checkpoint format, quantiser and module of the reference's int8 path (ref: quantize.py:25-57,
333-404; generation_utils.py:539-544), so that its `model_int8.pth` checkpoints load here and new ones can be written.

Every `nn.Linear` (the LM head included; embeddings are not linears and stay as they are) becomes a `WeightOnlyInt8Linear`
with the state-dict keys `<fqn>.weight` (int8 [out, in]), `<fqn>.scales` ([out], the model dtype) and `<fqn>.bias`.  Per row of
`w = weight.float()`: lo = min(min w, 0), hi = max(max w, 0), s32 = max(max(-lo, hi) / 127.5, fp32 eps) in fp32,
q = clamp(round_half_even(w / s32), -128, 127), scales = s32 rounded to the model dtype (include/coldcompress.h,
cc_gemv_fused_w8).  The module's forward is the reference's formula in torch — prefill and CPU use it; single-token decode on
the device streams the int8 weights through cc_gemv_fused_w8 (model.py hands each linear's scales to glue.gemv_fused).

    python -m cold_compress_amd.harness.quantize --checkpoint_path DIR/model.pth --mode int8   # -> DIR/model_int8.pth
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


def quantize(checkpoint_path: Path, mode: str = "int8") -> Path:
    """Write the weight-only int8 checkpoint next to `checkpoint_path` (model.pth -> model_int8.pth); the model shape is the
    `CONFIGS` entry named by the checkpoint's directory (ref: quantize.py's quantize())."""
    from .model import Transformer

    if mode != "int8":
        raise ValueError(f"quantisation mode {mode!r} is not supported (int8 weight-only only)")
    checkpoint_path = Path(checkpoint_path)
    assert checkpoint_path.is_file(), checkpoint_path
    t0 = time.time()
    with torch.device("meta"):
        model = Transformer.from_name(checkpoint_path.parent.name)
    checkpoint = torch.load(str(checkpoint_path), mmap=True, weights_only=True)
    model.load_state_dict(checkpoint, assign=True)
    sd = WeightOnlyInt8QuantHandler(model).create_quantized_state_dict()
    out = checkpoint_path.parent / checkpoint_path.name.replace(".pth", "_int8.pth")
    torch.save(sd, str(out))
    print(f"wrote {out} in {time.time() - t0:.1f} s")
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description="Quantise a checkpoint to weight-only int8.")
    ap.add_argument("--checkpoint_path", type=Path, required=True, help="DIR/model.pth, DIR named after a CONFIGS key")
    ap.add_argument("--mode", type=str, default="int8", choices=["int8"], help="int8 weight-only (int4 / GPTQ are not supported)")
    args = ap.parse_args(argv)
    quantize(args.checkpoint_path, args.mode)


if __name__ == "__main__":
    main()
