"""CPU tests of the fused quantised cache (cache_quant_mode="fused") for the two history-ring policies: the windowed heavy hitter
(history_window_size > 1) and the FastGen hybrid cache.  Construction registers the uint8 images and the per-row parameters (and
no model-dtype K / V), the refusals that are not part of the mode stay loud, and the new C-ABI entry points are declared, exported
and device-only (their checker is the same policy's 16-bit step on the dequantised values: tests/test_gpu_quant_fused_ring_hybrid.py)."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cc_decode_step_heavy_hitter_ring_quant", "cc_decode_step_hybrid_quant_rc", "cc_decode_step_hybrid_quant_single_launch")
HYBRID = [{"strategy": "special"}, {"strategy": "special_punc"}, {"strategy": "special_punc_heavy_hitter", "heavy_hitter_frac": 0.3},
          {"strategy": "special_punc_window", "recent_window": 0.3}, {"strategy": "full"}]


def _hybrid(H=2, S=64, dtype=torch.bfloat16, **extra):
    from cold_compress_amd.cache import KVCacheHybrid

    kw = dict(max_cache_length=S, max_seq_length=4 * S, cache_bits=8, global_tokens=4, min_recovery_frac=0.9, hybrid_strategies=HYBRID,
              token_ids={"special": [[1], [2, 3]], "punctuation": [5, 6, 7]}, cache_quant_mode="fused")
    kw.update(extra)
    return KVCacheHybrid(1, H, 128, dtype, **kw)


def _hh(W, H=2, S=64, dtype=torch.bfloat16, **extra):
    from cold_compress_amd.cache import KVCacheHeavyHitter

    kw = dict(max_cache_length=S, max_seq_length=4 * S, cache_bits=8, global_tokens=4, recent_window=10, history_window_size=W,
              attn_thresholding=False, cache_quant_mode="fused")
    kw.update(extra)
    return KVCacheHeavyHitter(1, H, 128, dtype, **kw)


def _check_images(kv, H, S):
    assert kv.fused_quant and not kv.quantize
    assert kv.k_cache.numel() == 0 and kv.v_cache.numel() == 0
    for name in ("k_cache_q", "v_cache_q"):
        t = getattr(kv, name)
        assert t.dtype == torch.uint8 and tuple(t.shape) == (1, H, S, 128), name
        assert name in dict(kv.named_buffers())
    assert kv.kv_qparams.dtype == torch.float32 and tuple(kv.kv_qparams.shape) == (1, H, S, 4)
    assert "kv_qparams" in dict(kv.named_buffers())
    # the reference mode's round-trip buffers are not there: the images are the cache
    assert not hasattr(kv, "k_scales") and not hasattr(kv, "_quant_stable")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_hybrid_fused_construction_registers_images(dtype):
    kv = _hybrid(2, 128, dtype)
    _check_images(kv, 2, 128)
    assert kv._fused_quant_policy() == 6
    # the ring, denominators, counter and window sums stay the 16-bit cache's
    assert kv.attn_history_num.dtype == dtype and tuple(kv.attn_history_num.shape) == (1, 2, 128, 400)
    assert kv.attn_history_denom.dtype == torch.int32 and kv.attn_counter.dtype == torch.int64
    assert not kv.supports_fused_step()  # not profiled yet


@pytest.mark.parametrize("W", [8, 33, 400])
def test_windowed_heavy_hitter_fused_construction_registers_images(W):
    kv = _hh(W, 2, 96)
    _check_images(kv, 2, 96)
    assert kv._fused_quant_policy() == 5
    assert tuple(kv.attn_history_num.shape) == (1, 2, 96, W) and kv.attn_history_num.dtype == torch.bfloat16
    assert kv.supports_fused_step() and not kv.recoverable()
    assert not kv.single_launch_active(8)  # the ring step has two launches
    assert _hh(1)._fused_quant_policy() == 1  # W == 1: cc_decode_step_quant, unchanged


def test_fused_memory_is_images_plus_row_parameters():
    H, S, W = 2, 64, 8
    a = _hh(W, H, S, cache_bits=None, cache_quant_mode="reference")
    b = _hh(W, H, S)
    kv16 = 2 * H * S * 128 * 2
    saved = kv16 - 2 * H * S * 128 - H * S * 16  # half the K/V bytes, less 16 B of qparams per (head, slot)
    assert abs((a.memory_usage() - b.memory_usage()) * 1024 ** 3 - saved) < 1
    stats = b.compute_statistics(torch.tensor(10))
    assert "working_cache_gb" not in stats and stats["cache_memory_gb"] == b.memory_usage()


def test_refusals_that_stay():
    from cold_compress_amd._abi import ColdCompressError
    from cold_compress_amd.cache import KVCacheHybrid, KVCacheL2, KVCacheRecentGlobal

    with pytest.raises(ColdCompressError):  # l2 is not served by the fused mode
        KVCacheL2(1, 2, 128, torch.bfloat16, max_cache_length=64, max_seq_length=128, cache_bits=8, global_tokens=4, recent_window=10,
                  cache_quant_mode="fused")
    with pytest.raises(ColdCompressError):  # 4-bit images are not in this mode
        KVCacheRecentGlobal(1, 2, 128, torch.bfloat16, max_cache_length=64, max_seq_length=128, cache_bits=4, global_tokens=4,
                            cache_quant_mode="fused")
    with pytest.raises(ColdCompressError):
        _hybrid(cache_bits=4)
    with pytest.raises(ColdCompressError):
        _hh(8, cache_bits=4)
    with pytest.raises(ColdCompressError):  # the fused mode needs a 16-bit model
        _hybrid(dtype=torch.float32)
    with pytest.raises(NotImplementedError):  # the reference's quantised hybrid cache: unchanged
        _hybrid(cache_quant_mode="reference")

    class ResetOnEvict(KVCacheHybrid):
        reset_history_on_evict = True

    with pytest.raises(ColdCompressError, match="fused"):  # no fused step for it: refused at construction, never a three-call path
        ResetOnEvict(1, 2, 128, torch.bfloat16, max_cache_length=64, max_seq_length=256, cache_bits=8, global_tokens=4,
                     min_recovery_frac=0.9, hybrid_strategies=HYBRID, token_ids={"special": [[1]], "punctuation": [5]},
                     cache_quant_mode="fused")
    with pytest.raises(ColdCompressError, match="fused"):
        _hybrid(hybrid_strategies=HYBRID * 5)  # 25 policies: more than the step's table holds


def test_three_call_decode_path_refused():
    from cold_compress_amd._abi import ColdCompressError

    kv = _hybrid()
    kv.cache_strategies = torch.zeros(2, dtype=torch.int64)
    z = torch.zeros(1, 2, 1, 128, dtype=torch.bfloat16)
    with pytest.raises(ColdCompressError, match="decode_step"):
        kv._decoding_update(torch.tensor([70]), z, z, input_ids=torch.tensor([[9]]))
    with pytest.raises(ColdCompressError, match="decode_step"):
        _hh(8)._decoding_update(torch.tensor([70]), z, z)


def test_new_entry_points_declared_exported_and_device_only():
    import ctypes as C

    from cold_compress_amd import _abi

    with open(os.path.join(ROOT, "include", "coldcompress.h")) as fh:
        header = fh.read()
    for name in NEW:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _abi.SIGNATURES and name in _abi.DEVICE_ONLY, name
    so = C.CDLL(_abi.LIB_PATH)
    for name in NEW:
        getattr(so, name)  # exported
    from oracle import oracle_lib

    ocdll = C.CDLL(oracle_lib.SO) if os.path.exists(oracle_lib.SO) else None
    if ocdll is not None:
        for name in NEW:
            assert not hasattr(ocdll, name + "_cpu"), name  # no CPU twin: the checker is the 16-bit step
