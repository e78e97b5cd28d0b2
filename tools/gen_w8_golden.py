#!/usr/bin/env python3
"""Write tests/golden/w8_quant_ref.npz: the weight-only int8 quantiser and forward of the reference implementation on a few weight
matrices with edge rows (all zero, one outlier, exact .5 ties, a negative-only row), for tests/test_w8_host.py.  Needs the
reference checkout importable (its quantize.py); the tests only read the file.

    python tools/gen_w8_golden.py --reference PATH/TO/cold-compress [--out tests/golden/w8_quant_ref.npz]

The reference's quantize.py imports its tokenizer module at the top, which is not needed here: a stub stands in for it.
"""
import argparse
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def weights():
    g = torch.Generator().manual_seed(1234)
    K = 64
    w = torch.randn(10, K, generator=g) * 0.05
    w[0] = 0.0                                                   # all zero: scale = fp32 eps
    w[1, 7] = 3.0                                                # one outlier
    w[2] = torch.tensor([127.5, 2.5, -3.5, 0.5, 1.5, -0.5, -2.5, 4.5] * 8)  # scale exactly 1.0: .5 ties (and 127.5 -> clamp)
    w[3] = -(torch.rand(K, generator=g) + 0.01)                  # negative only: the minimum lands on -128
    w[4] = torch.rand(K, generator=g) + 0.01                     # positive only
    w[5, :] = 1e-30                                              # tiny: scale clamps to eps
    return w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="directory holding the reference's quantize.py")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "w8_quant_ref.npz"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.reference))
    if "tokenizer" not in sys.modules:
        stub = types.ModuleType("tokenizer")
        stub.get_tokenizer = None
        sys.modules["tokenizer"] = stub
    import quantize as refq  # noqa: E402

    out = {}
    w = weights()
    g = torch.Generator().manual_seed(99)
    x = torch.randn(3, w.shape[1], generator=g)
    bias = torch.randn(w.shape[0], generator=g) * 0.1
    out["w_f32"] = w.numpy()
    out["x_f32"] = x.numpy()
    out["bias_f32"] = bias.numpy()
    for tag, dt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
        lin = nn.Linear(w.shape[1], w.shape[0], bias=True)
        with torch.no_grad():
            lin.weight.copy_(w)
            lin.bias.copy_(bias)
        mod = nn.Sequential(lin).to(dt)
        sd = refq.WeightOnlyInt8QuantHandler(mod).create_quantized_state_dict()
        q, s = sd["0.weight"], sd["0.scales"]
        assert q.dtype == torch.int8 and s.dtype == dt
        out[f"q_{tag}"] = q.numpy()
        out[f"scales_{tag}"] = s.float().numpy()  # (bf16 -> fp32 is exact)
        rt = refq.WeightOnlyInt8QuantHandler(nn.Sequential(nn.Linear(w.shape[1], w.shape[0], bias=True))).convert_for_runtime().to(dt)
        rt.load_state_dict(sd)
        with torch.no_grad():
            y = rt(x.to(dt))
        assert y.dtype == dt
        out[f"y_{tag}"] = y.float().numpy()
        out[f"wdt_{tag}"] = mod[0].weight.detach().float().numpy()  # the weight the handler saw (bf16: rounded)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    np.savez_compressed(a.out, **out)
    print(f"wrote {a.out}: " + ", ".join(f"{k}{list(v.shape)}" for k, v in out.items()))


if __name__ == "__main__":
    main()
