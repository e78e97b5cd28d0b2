"""cc_gemv_fused_w12 keeps a registry of packed copies by ADDRESS (which layout a `codes` buffer was packed in) that never forgets.
A buffer handed in at the address of an earlier copy of another layout must not change the verdict on a SHAPE the id does not serve:
that is CC_ERR_UNSUPPORTED before anything is launched, whatever the registry remembers about the address (a fresh torch tensor may
sit where a freed copy sat: tests/test_gpu_gemv_w12_long.py's refusal test then saw CC_ERR_BAD_ARG, depending on what ran before it).
Here the address is reused on purpose — the very buffer that was packed under the planar id is handed in under the long-row id.
A shape that the id serves keeps its CC_ERR_BAD_ARG for a copy of the other layout."""
import pytest
import torch

import test_gpu_gemv_w12 as T12
import test_gpu_gemv_w12_planar as TP

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
PLANAR, LONG = 1, 2
UNSUPPORTED, BAD_ARG = -2, -1  # CC_ERR_UNSUPPORTED, CC_ERR_BAD_ARG (include/coldcompress.h)
_p, _stream = T12._p, T12._stream


def _launch(pk, W, x, N, K, layout, pair=False):
    from cold_compress_amd import _abi

    y = torch.full((N,), 7.0, dtype=BF, device=DEV)
    rc = _abi.lib()["cc_gemv_fused_w12"](_p(pk.codes), _p(pk.records), pk.base, _p(pk.codes) if pair else None, _p(pk.records) if pair else None,
                                         pk.base, pk.rb | layout << 8, pk.cu, _p(W), _p(W) if pair else None, _p(x), None, None, 1e-5, None,
                                         None, None, 0, 0, _p(y), N, K, _abi.CC_DT_BF16, _stream())
    torch.cuda.synchronize()
    return rc, y


@pytest.mark.parametrize("N,K,pair", [(10, 4096, False), (9, 4104, True)], ids=["short_rows", "pair"])
def test_an_unserved_shape_is_unsupported_at_the_address_of_a_planar_copy(N, K, pair):
    gen = torch.Generator(device=DEV).manual_seed(6)
    W = T12._normal(N, K, gen)
    x = torch.randn(K, generator=gen, device=DEV).to(BF)
    pk = TP._pack(W, pair, layout=PLANAR)  # registers pk.codes as a planar copy
    assert pk is not None and pk.layout == PLANAR and pk.base % 2 == 0
    rc, y = _launch(pk, W, x, N, K, LONG, pair)
    assert rc == UNSUPPORTED and bool((y == 7.0).all()), rc


def test_a_served_shape_still_refuses_a_copy_of_the_other_layout():
    N, K = 9, 4104
    gen = torch.Generator(device=DEV).manual_seed(7)
    W = T12._normal(N, K, gen)
    x = torch.randn(K, generator=gen, device=DEV).to(BF)
    pk = TP._pack(W, False, layout=PLANAR)
    rc, y = _launch(pk, W, x, N, K, LONG)
    assert rc == BAD_ARG and bool((y == 7.0).all()), rc
