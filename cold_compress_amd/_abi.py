"""ctypes binding of the C ABI declared in include/coldcompress.h (+ the hooks of include/coldcompress_debug.h).

The product path has NO CPU fallback: `lib()` raises if `libcoldcompress_hip.so` has not been built
(`python -c "import __graft_entry__ as g; g.build()"`), and every wrapper raises `ColdCompressError` on a
non-zero return code.  The same signature table binds the CPU oracle (`oracle/oracle_lib.py`, `_cpu`
suffix) for tests — the oracle is never imported from here.
"""
import ctypes as C
import os

import torch  # noqa: F401  (must load ITS bundled HIP runtime before our library resolves libamdhip64)

CC_OK = 0
CC_DT_F32, CC_DT_BF16, CC_DT_F16 = 0, 1, 2
CC_QUANT_FP8_E4M3 = 0x100 | 8  # image format of cache_quant_mode='fp8' (the n_bit argument of the fused-cache entry points)
CC_QUANT_UINT4 = 0x200 | 4  # image format of cache_quant_mode='uint4': two 4-bit codes per byte
CC_QUANT_MXFP4 = 0x300 | 4  # image format of cache_quant_mode='mxfp4': two e2m1 codes per byte, one e8m0 scale per 32 values
CC_PRIO_F32, CC_PRIO_BF16, CC_PRIO_F16, CC_PRIO_I64 = 0, 1, 2, 3

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libcoldcompress_hip.so")


class ColdCompressError(RuntimeError):
    pass


class KVView(C.Structure):
    """struct cc_kv_view (include/coldcompress.h)."""

    _fields_ = [
        ("k_cache", C.c_void_p),
        ("v_cache", C.c_void_p),
        ("pos", C.c_void_p),
        ("mask", C.c_void_p),
        ("cache_cts", C.c_void_p),
        ("H", C.c_int32),
        ("Hp", C.c_int32),
        ("Hc", C.c_int32),
        ("S", C.c_int32),
        ("D", C.c_int32),
        ("dtype", C.c_int32),
    ]


class PenaltyRow(C.Structure):
    """struct cc_penalty_row_t (include/coldcompress.h): one row's state and settings for cc_logits_penalize_streams."""

    _fields_ = [
        ("prompt_count", C.c_void_p),
        ("gen_count", C.c_void_p),
        ("gen_start", C.c_void_p),
        ("bias", C.c_void_p),
        ("r", C.c_float),
        ("f", C.c_float),
        ("p", C.c_float),
    ]


class ConstraintRow(C.Structure):
    """struct cc_constraint_row_t (include/coldcompress.h): one row's state and settings for cc_logits_constrain_streams."""

    _fields_ = [
        ("hist", C.c_void_p),
        ("cap", C.c_int32),
        ("gen_start", C.c_void_p),
        ("ngram", C.c_int32),
        ("ngram_from_gen", C.c_int32),
        ("min_new_tokens", C.c_int32),
        ("term_ids", C.c_void_p),
        ("n_term", C.c_int32),
        ("bw_tokens", C.c_void_p),
        ("bw_offsets", C.c_void_p),
        ("n_bw", C.c_int32),
    ]


_vp, _i32, _f32, _sz = C.c_void_p, C.c_int32, C.c_float, C.c_size_t
_view = C.POINTER(KVView)

# name -> (restype, argtypes); one row per declaration in include/coldcompress.h
SIGNATURES = {
    "cc_abi_version": (C.c_int, []),
    "cc_error_string": (C.c_char_p, [C.c_int]),
    "cc_device_info": (C.c_int, [_vp, _vp, _vp, C.c_char_p, C.c_int]),
    "cc_decode_update_full": (C.c_int, [_view, _vp, _vp, _vp, _vp, _vp]),
    "cc_decode_update_recent_global": (C.c_int, [_view, _vp, _vp, _vp, _i32, _vp, _vp]),
    "cc_decode_update_scores": (C.c_int, [_view, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp]),
    "cc_decode_update_random": (C.c_int, [_view, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp]),
    "cc_decode_update_l2_workspace_bytes": (_sz, [_i32, _i32]),
    "cc_decode_update_l2": (C.c_int, [_view, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _sz, _vp]),
    "cc_decode_update_heavy_hitter": (C.c_int, [_view, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp]),
    "cc_hh_update": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    "cc_decode_attn_workspace_bytes": (_sz, [_i32, _i32, _i32, _i32, _i32]),
    "cc_decode_attn_gqa": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _f32, _vp, _vp, _vp,
                                     _vp, _vp, _vp, _vp, _sz, _vp]),
    "cc_decode_attn_gqa_ring": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _f32, _vp, _vp, _vp, _vp, _vp, _i32,
                                          _vp, _vp, _vp, _sz, _vp]),
    "cc_softmax_argmax_workspace_bytes": (_sz, []),
    "cc_softmax_argmax": (C.c_int, [_vp, _i32, _i32, _vp, _vp, _vp, _sz, _vp]),
    "cc_sample_topk_workspace_bytes": (_sz, []),
    "cc_sample_topk": (C.c_int, [_vp, _i32, _i32, _f32, _i32, C.c_uint64, _vp, _vp, _vp, _vp, _sz, _vp]),
    "cc_sample_nucleus_workspace_bytes": (_sz, []),
    "cc_sample_nucleus": (C.c_int, [_vp, _i32, _i32, _f32, _i32, _f32, _f32, C.c_uint64, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "cc_sample_rows_workspace_bytes": (_sz, [_i32]),
    "cc_sample_rows": (C.c_int, [_vp, _i32, _i32, C.c_int64, _i32, _f32, _i32, _f32, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "cc_logprob_rows_workspace_bytes": (_sz, []),
    "cc_logprob_rows": (C.c_int, [_vp, _i32, _i32, C.c_int64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "cc_logprob_topn_workspace_bytes": (_sz, []),
    "cc_logprob_topn": (C.c_int, [_vp, _i32, _i32, C.c_int64, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "cc_token_counts_add": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _i32, _vp, _vp]),
    "cc_logits_penalize": (C.c_int, [_vp, _vp, _i32, _i32, C.c_int64, _i32, _vp, _vp, _vp, _vp, _vp, _f32, _f32, _f32, _vp, _vp]),
    "cc_token_history_write": (C.c_int, [_vp, _i32, _vp, _i32, _i32, _vp]),
    "cc_logits_constrain": (C.c_int, [_vp, _vp, _i32, _i32, C.c_int64, _i32, _vp, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _i32, _vp, _vp,
                                      _i32, _vp]),
    "cc_logits_penalize_streams": (C.c_int, [_vp, _vp, _i32, _i32, C.c_int64, _i32, C.POINTER(PenaltyRow), _vp, _vp, _vp]),
    "cc_logits_constrain_streams": (C.c_int, [_vp, _vp, _i32, _i32, C.c_int64, _i32, C.POINTER(ConstraintRow), _vp, _vp, _vp]),
    "cc_gemv_fused":(C.c_int, [_vp, _vp, _vp, _vp, _vp, _f32, _vp, _vp, _vp, _i32, _i32, _vp, _i32, _i32, _i32, _vp]),
    "cc_gemv_fused_multi": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _f32, _vp, _vp, _vp, _i32, _i32, _vp, _i32, _i32, _i32, _i32, _vp]),
    "cc_w12_geometry": (C.c_int, [_i32, _i32, _i32, _vp]),
    "cc_w12_meta_words": (_sz, []),
    "cc_w12_pack": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "cc_gemv_fused_w12": (C.c_int, [_vp, _vp, _i32, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _f32, _vp, _vp, _vp, _i32, _i32,
                                    _vp, _i32, _i32, _i32, _vp]),
    "cc_gemv_fused_w8": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _f32, _vp, _vp, _vp, _i32, _i32, _vp, _i32, _i32, _i32, _vp]),
    "cc_gemv_fused_w4": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _f32, _vp, _vp, _vp, _i32, _i32, _vp, _i32, _i32, _i32, _i32, _vp]),
    "cc_gemv_fused_mx4": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _f32, _vp, _vp, _vp, _i32, _i32, _vp, _i32, _i32, _i32, _vp]),
    "cc_gemv_fused_w8_multi": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _f32, _vp, _vp, _vp, _i32, _i32, _vp, _i32, _i32, _i32, _i32, _vp]),
    "cc_gemv_fused_mx4_multi": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _f32, _vp, _vp, _vp, _i32, _i32, _vp, _i32, _i32, _i32, _i32, _vp]),
    "cc_gemv_fused_w4_multi": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _f32, _vp, _vp, _vp, _i32, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _vp]),
    "cc_kv_requant": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp]),
    "cc_kv_requant_pair": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp]),
    "cc_kv_requant_batch": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "cc_kv_dequant": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp]),
    "cc_kv_quant_rows": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "cc_kv_dequant_rows": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "cc_decode_step_quant": (C.c_int, [_view, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _f32,
                                       _vp, _vp, _vp, _sz, _vp, _i32]),
    "cc_decode_step_quant_rc": (C.c_int, [_view, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_uint64, _vp, _vp, _i32, _i32, _i32,
                                          _f32, _vp, _vp, _sz, _vp, _i32]),
    "cc_decode_step_quant_single_launch": (_i32, [_i32, _i32, _i32, _i32, _i32, _i32]),
    "cc_decode_step_heavy_hitter_ring_quant": (C.c_int, [_view, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _i32, _i32,
                                                         _i32, _f32, _vp, _vp, _vp, _sz, _vp]),
    "cc_decode_step_hybrid_quant_rc": (C.c_int, [_view, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _vp,
                                                 _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _f32, _vp, _vp, _vp, _sz, _vp]),
    "cc_decode_step_hybrid_quant_single_launch": (_i32, [_i32, _i32, _i32, _i32, _i32, _i32]),
    "cc_decode_step_hybrid_single_launch": (_i32, [_i32, _i32, _i32, _i32, _i32]),
    "cc_decode_step_l2_single_launch": (_i32, [_i32, _i32, _i32, _i32, _i32]),
    "cc_decode_step_single_launch_enabled": (_i32, []),
    "cc_decode_step_device_single_launch": (_i32, [_i32]),
    "cc_hh_next_key_slots": (_i32, [_i32]),
    "cc_decode_step_single_launch": (_i32, [_i32, _i32, _i32, _i32, _i32]),
    "cc_decode_step_status_offset": (_i32, []),
    "cc_decode_step_wait_bound_us": (_i32, []),
    "cc_decode_step_trace": (None, [_vp]),
    "cc_decode_step_set_single_launch": (None, [_i32]),
    "cc_decode_step_set_wide": (None, [_i32]),
    "cc_decode_step_probe_xcd": (_i32, []),
    "cc_decode_step_set_l2_handoff": (None, [_i32]),
    "cc_decode_step_l2_handoff": (_i32, []),
    "cc_decode_step_demote_l2_handoff": (_i32, [_i32]),
    "cc_decode_step_heavy_hitter_rc": (C.c_int, [_view, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _f32, _vp, _vp, _sz,
                                                 _vp, _i32]),
    "cc_decode_step_qkv_available": (_i32, [_i32, _i32, _i32, _i32, _i32, _i32]),
    "cc_decode_step_qkv_rc": (C.c_int, [_view, _i32, _vp, _vp, _vp, _vp, _vp, _f32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp,
                                        C.c_uint64, _vp, _vp, _i32, _i32, _i32, _f32, _vp, _vp, _sz, _vp]),
    "cc_debug_occupy": (C.c_int, [_i32, _i32, _i32, _vp, _vp]),
    "cc_debug_qkv_trace": (None, [_vp]),
    "cc_decode_step_stream_floor": (C.c_int, [_view, _i32, _vp, _vp]),
    "cc_decode_step_stream_floor_geom": (C.c_int, [_view, _i32, _i32, _vp, _vp]),
    "cc_rg_next_key_init": (C.c_int, [_view, _vp, _i32, _vp, _vp]),
    "cc_decode_step_recent_global": (C.c_int, [_view, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _f32, _vp, _vp, _sz, _vp]),
    "cc_hh_ring_next_key_init": (C.c_int, [_view, _vp, _vp, _i32, _vp, _i32, _i32, _vp, _vp]),
    "cc_decode_step_heavy_hitter_ring": (C.c_int, [_view, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _i32, _i32, _i32,
                                                   _f32, _vp, _vp, _vp, _sz, _vp]),
    "cc_hybrid_next_key_init": (C.c_int, [_view, _vp, _vp, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _vp]),
    "cc_decode_step_hybrid": (C.c_int, [_view, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp,
                                        _i32, _vp, _vp, _vp, _i32, _i32, _f32, _vp, _vp, _vp, _sz, _vp]),
    "cc_decode_step_hybrid_rc": (C.c_int, [_view, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp,
                                           _i32, _vp, _vp, _vp, _vp, _i32, _i32, _f32, _vp, _vp, _vp, _sz, _vp]),
    "cc_l2_next_key_init": (C.c_int, [_view, _vp, _vp, _i32, _i32, _vp, _vp]),
    "cc_decode_step_l2": (C.c_int, [_view, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _f32, _vp, _vp, _sz, _vp]),
    "cc_decode_step_l2_rc": (C.c_int, [_view, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _f32, _vp, _vp, _sz, _vp]),
    "cc_decode_step_commit_stride": (_i32, []),
    "cc_random_next_key_init": (C.c_int, [_view, _vp, _vp, _i32, _i32, _vp, _vp]),
    "cc_decode_step_random": (C.c_int, [_view, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _f32, _vp, _vp, _sz, _vp]),
    "cc_random_next_key_init_rng": (C.c_int, [_view, _vp, C.c_uint64, _i32, _i32, _vp, _vp]),
    "cc_decode_step_head_constant_rc": (C.c_int, [_view, _i32, _vp, _vp, _vp, _vp, _vp, C.c_uint64, _vp, _vp, _i32, _i32, _i32, _f32,
                                                  _vp, _vp, _sz, _vp]),
    "cc_decode_step_random_rng": (C.c_int, [_view, _vp, _vp, _vp, _vp, C.c_uint64, _vp, _i32, _i32, _i32, _f32, _vp, _vp, _sz, _vp]),
    "cc_hh_next_key_init": (C.c_int, [_view, _vp, _vp, _vp, _i32, _i32, _vp, _vp]),
    "cc_decode_step_heavy_hitter": (C.c_int, [_view, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _f32, _vp, _vp,
                                              _vp, _sz, _vp]),
    "cc_decode_step_heavy_hitter_phases": (C.c_int, [_view, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _f32, _vp,
                                                     _vp, _vp, _sz, _vp, _i32]),
    "cc_decode_attn_gqa_phases": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _f32, _vp, _vp, _vp,
                                            _vp, _vp, _vp, _vp, _sz, _vp, _i32]),
    "cc_prefill_fill": (C.c_int, [_view, _vp, _vp, _vp, _i32, _i32, _vp]),
    "cc_row_l2_norm": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "cc_topk_keep_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "cc_topk_keep": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _sz, _vp]),
    "cc_gather_rows": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "cc_gather_vec": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp]),
    "cc_analysis_loss": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _vp]),
    "cc_snapkv_priority": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "cc_prefill_attn_workspace_bytes": (_sz, [_i32, _i32, _i32, _i32, _i32]),
    "cc_prefill_attn": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _f32, _vp, _vp, _vp, _i32, _vp,
                                  _sz, _vp]),
    "cc_prefill_attn_bands": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _f32, _vp, _vp, _vp, _i32, _vp, _i32,
                                        _vp, _vp, _sz, _vp]),
    "cc_attn_colsum": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _vp]),
    "cc_colsum_to_mean": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, _vp]),
    "cc_hybrid_decode_update": (C.c_int, [_view, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32,
                                          _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp]),
    "cc_decode_update_heavy_hitter_ring": (C.c_int, [_view, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "cc_hh_ring_update": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "cc_hh_ring_acc_words": (_sz, [_i32, _i32, _i32, _i32]),
    "cc_hh_ring_window_sums": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "cc_attn_bandsum": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "cc_add_rmsnorm": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _f32, _i32, _vp, _vp, _vp]),
    "cc_qkv_rope": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "cc_silu_mul": (C.c_int, [_vp, _vp, C.c_int64, _i32, _vp, _vp]),
    "cc_allreduce_handle_bytes": (_sz, []),
    "cc_allreduce_create": (C.c_int, [_i32, _i32, _sz, C.POINTER(_vp)]),
    "cc_allreduce_export": (C.c_int, [_vp, _vp]),
    "cc_allreduce_connect": (C.c_int, [_vp, _vp]),
    "cc_allreduce_sum": (C.c_int, [_vp, _vp, C.c_int64, _i32, _vp]),
    "cc_allreduce_status": (_i32, [_vp]),
    "cc_allreduce_destroy": (C.c_int, [_vp]),
}

# entry points that only the device library has (no `_cpu` twin)
DEVICE_ONLY = {"cc_error_string", "cc_device_info", "cc_decode_step_single_launch", "cc_decode_step_status_offset", "cc_decode_step_wait_bound_us",
               "cc_decode_step_trace", "cc_decode_step_set_single_launch", "cc_decode_step_set_wide", "cc_decode_step_probe_xcd", "cc_decode_step_commit_stride", "cc_decode_step_l2_rc", "cc_decode_step_quant_rc", "cc_decode_step_set_l2_handoff", "cc_decode_step_l2_handoff", "cc_decode_step_demote_l2_handoff", "cc_decode_step_stream_floor", "cc_decode_step_stream_floor_geom", "cc_debug_occupy", "cc_decode_step_quant_single_launch",
               "cc_decode_step_hybrid_single_launch", "cc_decode_step_l2_single_launch", "cc_decode_step_single_launch_enabled", "cc_decode_step_device_single_launch",
               "cc_decode_step_qkv_available", "cc_debug_qkv_trace",
               "cc_kv_requant_batch",  # (its oracle is the per-cache twin of cc_kv_requant_pair)
               "cc_gemv_fused_multi",  # cc_gemv_fused for up to 4 input vectors: its checker is cc_gemv_fused itself, row by row, bit for bit
               # the 12-bit packed copy of dense bf16 weights: its checker is cc_gemv_fused itself, bit for bit, and a numpy decoder of the format
               "cc_w12_geometry", "cc_w12_meta_words", "cc_w12_pack", "cc_gemv_fused_w12",
               "cc_gemv_fused_w8",  # int8 weight-only GEMV: its checker is the fp32 torch composition of the reference's formula
               "cc_gemv_fused_w4",  # int4 group-wise weight-only GEMV: likewise
               "cc_gemv_fused_mx4",  # MXFP4 weight-only GEMV: likewise (and bit-exact known-answer cases)
               # the two for up to 4 input vectors: their checkers are cc_gemv_fused_w8 / cc_gemv_fused_mx4 themselves, row by row, bit for bit
               "cc_gemv_fused_w8_multi", "cc_gemv_fused_mx4_multi",
               "cc_gemv_fused_w4_multi",  # the int4 one: its checker is cc_gemv_fused_w4 itself, row by row, bit for bit
               "cc_sample_topk_workspace_bytes", "cc_sample_topk",  # sampling tail: its checker is the numpy twin of the contract (tests/sample_twin.py)
               "cc_sample_nucleus_workspace_bytes", "cc_sample_nucleus",  # top-p / min-p on the same tail: likewise (tests/sample_nucleus_twin.py)
               "cc_sample_rows_workspace_bytes", "cc_sample_rows",  # the same tail for up to 8 rows: its checker is cc_sample_nucleus itself, row by row, bit for bit
               "cc_logprob_rows_workspace_bytes", "cc_logprob_rows",  # per-token log-probabilities: float64 torch.log_softmax and the fp32 twin of the contract (tests/logprob_twin.py)
               "cc_logprob_topn_workspace_bytes", "cc_logprob_topn",  # the N best alternatives of a row: the float64 order and values (tests/logprob_topn_twin.py)
               "cc_token_counts_add", "cc_logits_penalize",  # token-history penalties: the fp32 torch twin of the contract (tests/penalty_twin.py)
               "cc_token_history_write", "cc_logits_constrain",  # n-gram blocking, banned sequences, minimum length: the plain-Python twin (tests/constraint_twin.py)
               # the two for rows of different sequences: their checkers are cc_logits_penalize / cc_logits_constrain themselves at T = 1, bit for bit
               "cc_logits_penalize_streams", "cc_logits_constrain_streams",
               # the fused quantised cache's ring and hybrid steps: their checker is the same policy's 16-bit step on the dequantised values
               "cc_decode_step_heavy_hitter_ring_quant", "cc_decode_step_hybrid_quant_rc", "cc_decode_step_hybrid_quant_single_launch",
               # inter-GPU transport: no CPU twin (the oracle of the all-reduce is torch.distributed's)
               "cc_allreduce_handle_bytes", "cc_allreduce_create", "cc_allreduce_export", "cc_allreduce_connect", "cc_allreduce_sum",
               "cc_allreduce_status", "cc_allreduce_destroy"}
CC_PHASE_TWO_LAUNCH, CC_PHASE_ONE_LAUNCH = 0x10000, 0x20000


def bind(cdll, suffix=""):
    """Attach restype/argtypes for every ABI symbol; raises AttributeError if one is missing."""
    fns = {}
    for name, (res, args) in SIGNATURES.items():
        if suffix and name in DEVICE_ONLY:
            continue
        fn = getattr(cdll, name + suffix)
        fn.restype = res
        fn.argtypes = args
        fns[name] = fn
    return fns


_LIB = None
_FNS = None


def built():
    """True when the HIP extension exists (host-side constructors size their pipeline buffers through it)."""
    return os.path.exists(LIB_PATH)


def lib():
    """The device library's bound functions; raises loudly when it has not been built."""
    global _LIB, _FNS
    if _FNS is None:
        if not os.path.exists(LIB_PATH):
            raise ColdCompressError(
                f"{LIB_PATH} not found: build the HIP extension first "
                "(python -c 'import __graft_entry__ as g; g.build()'). There is no CPU fallback.")
        _LIB = C.CDLL(LIB_PATH)
        _FNS = bind(_LIB)
        v = _FNS["cc_abi_version"]()
        if v != 1:
            raise ColdCompressError(f"ABI version mismatch: library {v}, python 1")
        # (no device probe here — ADVICE r4: loading the library must not allocate or launch on whatever device happens to be current,
        #  possibly before a TP rank has selected its own; the probe runs when a decode workspace is created: attention_utils._workspace)
    return _FNS


def probe_device():
    """Observe the current device's block -> XCD dispatch order once (cc_decode_step_probe_xcd: synchronous, outside capture): where
    it is verified, caches with a multiple of 8 kv heads run their single-tile step with the L2-resident hand-off
    (include/coldcompress.h).  No GPU: nothing happens.  Called when a decode workspace is created on a device (attention_utils._workspace)."""
    if _FNS is None:
        return 0
    try:
        import torch

        if not torch.cuda.is_available() or torch.cuda.is_current_stream_capturing():
            return 0
    except Exception:  # pragma: no cover
        return 0
    return int(_FNS["cc_decode_step_probe_xcd"]())


def check(code, what):
    if code != CC_OK:
        msg = lib()["cc_error_string"](code)
        raise ColdCompressError(f"{what} failed: {code} ({msg.decode() if msg else '?'})")


def call(name, *args):
    check(lib()[name](*args), name)
