#!/usr/bin/env python3
"""Write tests/golden/w4_quant_ref.npz: the reference implementation's int4 group-wise quantiser (`group_quantize_tensor`), its
dequantiser (`group_dequantize_tensor`) and a forward through torch's CPU int4 kernels (`_convert_weight_to_int4pack_for_cpu` +
`_weight_int4pack_mm_for_cpu`, the reference's int4 op on the CPU backend; its CUDA tinygemm packing cannot run on the CPU) at
G = 32, 64, 128 and 256, on bf16 weight matrices with edge groups, for tests/test_w4_host.py.  Needs the reference checkout
importable (its quantize.py); the tests only read the file.

    python tools/gen_w4_golden.py --reference PATH/TO/cold-compress [--out tests/golden/w4_quant_ref.npz]

The reference's quantize.py imports its tokenizer module at the top, which is not needed here: a stub stands in for it.
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 512
N = 16


def weights(G):
    """bf16 [N, K]: random rows, plus rows whose first groups are edge cases (every row has K / G >= 2 groups)."""
    g = torch.Generator().manual_seed(4321 + G)
    w = torch.randn(N, K, generator=g) * 0.05
    w[0] = 0.0                                                            # all zero: the scale clamps to 1e-6 / 15
    w[1] = 0.37                                                           # constant groups
    w[2, 5] = 4.0                                                         # one outlier
    w[3, :G] = torch.arange(G, dtype=torch.float32) % 16 - 7.5           # range 15 -> scale 1: exact .5 ties
    w[4] = -(torch.rand(K, generator=g) + 0.01)                           # negative only
    w[5, :G] = 0.0                                                        # mixed groups in one row: zero, constant, random
    w[5, G:2 * G] = -0.25
    w[6, :G] = torch.linspace(-1.0, 1.0, G)                               # evenly spaced
    return w.to(torch.bfloat16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="directory holding the reference's quantize.py")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "w4_quant_ref.npz"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.reference))
    if "tokenizer" not in sys.modules:
        stub = types.ModuleType("tokenizer")
        stub.get_tokenizer = None
        sys.modules["tokenizer"] = stub
    import quantize as refq  # noqa: E402

    out = {}
    gx = torch.Generator().manual_seed(77)
    x = torch.randn(3, K, generator=gx).to(torch.bfloat16)
    out["x_bf16"] = x.float().numpy()
    for G in (32, 64, 128, 256):
        w = weights(G)
        q, sz = refq.group_quantize_tensor(w, n_bit=4, groupsize=G)   # the handler's call, on weight.to(bfloat16)
        assert q.dtype == torch.int32 and sz.dtype == torch.bfloat16 and tuple(sz.shape) == (K // G, N, 2)
        wdq = refq.group_dequantize_tensor(q, sz.float(), n_bit=4, groupsize=G)
        packed = torch.ops.aten._convert_weight_to_int4pack_for_cpu(q, 8)
        y = torch.ops.aten._weight_int4pack_mm_for_cpu(x, packed, G, sz)
        assert y.dtype == torch.bfloat16
        out[f"w_g{G}"] = w.float().numpy()                 # (bf16 -> fp32 is exact)
        out[f"q_g{G}"] = q.to(torch.uint8).numpy()
        out[f"sz_g{G}"] = sz.float().numpy()
        out[f"wdq_g{G}"] = wdq.float().numpy()
        out[f"y_g{G}"] = y.float().numpy()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    np.savez_compressed(a.out, **out)
    print(f"wrote {a.out}: " + ", ".join(f"{k}{list(v.shape)}" for k, v in out.items()))


if __name__ == "__main__":
    main()
