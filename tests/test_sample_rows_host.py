"""cc_sample_rows on a machine without a device: the header, _abi.py and the library agree on the two symbols, the library
cross-compiles and exports them, every refusal of the contract (include/coldcompress.h) comes back before any launch (a launch here
would fail with another code), and glue.sample_rows refuses host tensors and bad shapes."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD, WORKSPACE = 0, -1, -4


def test_abi_surface():
    from cold_compress_amd import _abi, _build
    from cold_compress_amd.harness import glue

    header = open(os.path.join(ROOT, "include", "coldcompress.h")).read()
    m = re.search(r"^int\s+cc_sample_rows\s*\(([^;]*)\);", header, re.M | re.S)
    assert m and len(m.group(1).split(",")) == len(_abi.SIGNATURES["cc_sample_rows"][1]) == 17
    m = re.search(r"^size_t\s+cc_sample_rows_workspace_bytes\s*\(([^;]*)\);", header, re.M | re.S)
    assert m and len(m.group(1).split(",")) == len(_abi.SIGNATURES["cc_sample_rows_workspace_bytes"][1]) == 1
    assert {"cc_sample_rows", "cc_sample_rows_workspace_bytes"} <= _abi.DEVICE_ONLY
    m = re.search(r"^#define\s+CC_SAMPLE_MAX_ROWS\s+(\d+)", header, re.M)
    assert m and int(m.group(1)) == glue.SAMPLE_MAX_ROWS == 8
    assert "cc_sample.hip" in _build.SOURCES


def test_library_builds_and_refuses_before_any_launch():
    from cold_compress_amd import _abi, _build

    fns = _abi.bind(C.CDLL(_build.build()))
    size = fns["cc_sample_rows_workspace_bytes"]
    one = fns["cc_sample_nucleus_workspace_bytes"]()
    assert [size(t) for t in (0, -1, 9)] == [0, 0, 0] and [size(t) for t in (1, 2, 8)] == [one, 2 * one, 8 * one]
    buf = (C.c_char * 512)()
    p = (C.addressof(buf) + 15) & ~15
    seeds = (C.c_uint64 * 8)(*range(8))
    f = fns["cc_sample_rows"]
    big = 8 * one
    ok = dict(logits=p, T=2, V=8, row_stride=8, dtype=_abi.CC_DT_BF16, temperature=0.8, top_k=5, top_p=0.9, min_p=0.05,
              seeds=C.cast(seeds, C.c_void_p), input_pos=p + 64, probs=p + 128, idx_out=p + 256, n_kept_out=p + 320, workspace=p + 384,
              workspace_bytes=big, stream=None)

    def call(**kw):
        return f(*{**ok, **kw}.values())

    inf, nan = float("inf"), float("nan")
    for kw in (dict(T=0), dict(T=-1), dict(T=9), dict(T=64),  # rows
               dict(row_stride=7), dict(row_stride=0), dict(row_stride=-8),  # row stride
               dict(logits=None), dict(seeds=None), dict(input_pos=None), dict(probs=None), dict(idx_out=None), dict(workspace=None),
               dict(V=0), dict(V=-3), dict(dtype=3), dict(dtype=-1),  # cc_sample_nucleus's own
               dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=nan),
               dict(top_p=0.0), dict(top_p=-0.5), dict(top_p=nan), dict(min_p=1.5), dict(min_p=inf), dict(min_p=nan),
               dict(V=1 << 24, row_stride=1 << 24),  # top_p on with V beyond CC_SAMPLE_NUCLEUS_MAX_V
               dict(workspace=p + 385)):  # alignment
        assert call(**kw) == BAD, kw
    for kw in (dict(workspace_bytes=2 * one - 1), dict(workspace_bytes=0), dict(T=8, workspace_bytes=8 * one - 1),
               dict(T=1, workspace_bytes=one - 1, n_kept_out=None, top_p=1.0, min_p=0.0)):
        assert call(**kw) == WORKSPACE, kw
    assert call(T=9, workspace_bytes=0) == BAD  # a bad argument is named before the workspace


def test_glue_refuses_host_tensors_and_bad_shapes():
    from cold_compress_amd import _abi
    from cold_compress_amd.harness import glue

    pos = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(_abi.ColdCompressError, match="no CPU fallback"):
        glue.sample_rows(torch.zeros(2, 16), 0.8, 5, 0.9, None, [0, 1], pos)

    class Dev:  # a tensor that says it is on the device: the shape checks come before anything touches memory
        def __init__(self, t):
            self.t = t

        is_cuda = True

        def __getattr__(self, n):
            return getattr(self.t, n)

    x = Dev(torch.zeros(2, 16))
    for logits, seeds, ipos, kw in ((Dev(torch.zeros(16)), [0], Dev(pos[:1]), {}),  # one dimension
                                    (Dev(torch.zeros(9, 16)), list(range(9)), Dev(torch.zeros(9, dtype=torch.int32)), {}),  # too many rows
                                    (Dev(torch.zeros(2, 16, dtype=torch.float64)), [0, 1], Dev(pos), {}),
                                    (Dev(torch.zeros(0, 16)), [], Dev(pos[:0]), {}),
                                    (x, [0], Dev(pos), {}),  # seeds
                                    (x, [0, 1], Dev(pos[:1]), {}), (x, [0, 1], Dev(pos.long()), {}), (x, [0, 1], pos, {}),  # positions
                                    (x, [0, 1], Dev(pos), dict(temperature=0.0)), (x, [0, 1], Dev(pos), dict(top_p=0.0)),
                                    (x, [0, 1], Dev(pos), dict(min_p=1.5))):
        args = dict(temperature=0.8, top_k=5, top_p=0.9, min_p=None)
        args.update(kw)
        with pytest.raises(_abi.ColdCompressError):
            glue.sample_rows(logits, args["temperature"], args["top_k"], args["top_p"], args["min_p"], seeds, ipos)
