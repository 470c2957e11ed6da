"""ctypes binding of the C-ABI library (include/bayeformers_amd.h -> lib/libbayeformers_amd.so).

The product path has no fallback: if the library is missing or a call fails, an exception is raised.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BF_LIB_PATH") or os.path.join(_HERE, "lib", "libbayeformers_amd.so")  # BF_LIB_PATH: load another build of the library

BF_DT_F32, BF_DT_BF16, BF_DT_F16 = 0, 1, 2
BF_PRIOR_MIXTURE, BF_PRIOR_GAUSSIAN, BF_PRIOR_NONE = 0, 1, 2


class bf_prior_t(ctypes.Structure):
    _fields_ = [
        ("kind", ctypes.c_int32),
        ("pi", ctypes.c_float),
        ("sigma1", ctypes.c_float),
        ("sigma2", ctypes.c_float),
        ("d_mu", ctypes.c_void_p),
        ("d_rho", ctypes.c_void_p),
        ("d_pi", ctypes.c_void_p),      # mixture: the device scalars pi / sigma1 / sigma2 were read from (re-checked by
        ("d_sigma1", ctypes.c_void_p),  # the kernels, bf_stale_counter)
        ("d_sigma2", ctypes.c_void_p),
    ]


class bf_tensor_t(ctypes.Structure):
    _fields_ = [
        ("d_mu", ctypes.c_void_p),
        ("d_rho", ctypes.c_void_p),
        ("n", ctypes.c_uint64),
        ("prior", bf_prior_t),
        ("stream_id", ctypes.c_uint32),
        ("out_dtype", ctypes.c_int32),
        ("d_sample_out", ctypes.c_void_p),
    ]


# every symbol include/bayeformers_amd.h declares: name -> (restype, argtypes)
_vp, _i, _u32, _u64, _i64, _sz = (ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int64,
                                  ctypes.c_size_t)
_tp = ctypes.POINTER(bf_tensor_t)
SYMBOLS = {
    "bf_version": (_i, []),
    "bf_last_error": (ctypes.c_char_p, []),
    "bf_stale_counter": (_i, [ctypes.POINTER(ctypes.POINTER(ctypes.c_uint32))]),
    "bf_set_sample_counter": (_i, [_vp]),
    "bf_get_sample_counter": (_vp, []),
    "bf_device_info": (_i, [ctypes.c_char_p, _sz, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "bf_philox_normal_host": (_i, [_vp, _u64, _u64, _u32, _u32, _u64]),
    "bf_philox_normal": (_i, [_vp, _u64, _i, _u64, _u32, _u32, _vp]),
    "bf_sample_logprob_workspace_bytes": (_sz, [_tp, _i, _i]),
    "bf_sample_logprob": (_i, [_tp, _i, _i, _u64, _u32, _vp, _vp, _sz, _vp]),
    "bf_sample_table_bytes": (_sz, [_tp, _i, ctypes.POINTER(ctypes.c_uint32)]),
    "bf_sample_table_build": (_i, [_tp, _i, _vp, _sz, _vp, _vp]),
    "bf_sample_logprob_table": (_i, [_vp, _i, _u32, _u32, _i, _u64, _u32, _vp, _i, _vp]),
    "bf_reduce_logprob": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    "bf_gemm_nt": (_i, [_vp, _i, _i64, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "bf_gemm_nt_act": (_i, [_vp, _i, _i64, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "bf_gemm_nt_act_pre": (_i, [_vp, _i, _i64, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "bf_gemm_nt_layers": (_i, [_vp, _i, _i64, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "bf_gemm_nt_skinny": (_i, [_vp, _i, _i64, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "bf_gemm_nt_skinny_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "bf_gemm_nt_skinny_max_rows": (_i, []),
    "bf_gemm_nt_rows": (_i, [_vp, _i, _i64, _i64, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "bf_gemm_nt_rows_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "bf_gemm_nn_layers": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "bf_gemm_nn": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "bf_gemm_tn": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "bf_gemm_prepare": (_i, [_i, _i, _i, _i, _vp]),
    "bf_gemm_schedule": (_sz, [_i, _i, _i, _i, _i, _vp, _sz, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "bf_gemm_schedule_policy": (_sz, [_i, _i, _i, _i, _i, _i, _vp, _sz, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "bf_gemm_schedule_fetch_rows": (ctypes.c_int64, [_vp, _i, _i]),
    "bf_linear_fwd_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i, _i]),
    "bf_linear_fwd": (_i, [_vp, _i, _i64, _tp, _tp, _vp, _i, _i, _i, _i, _i, _i, _u64, _u32, _vp, _vp, _sz, _vp]),
    "bf_linear_bwd_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i, _i]),
    "bf_linear_bwd": (_i, [_vp, _i64, _vp, _i, _tp, _tp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _u64, _u32, _i, _vp,
                           _vp, _vp, _vp, _vp, _sz, _vp]),
    "bf_linear_bwd_splits": (_i, [_i, _i, _i, _i, _i]),
    "bf_gemm_nn_actgrad_supported": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i]),
    "bf_gemm_nn_actgrad": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "bf_param_grad_table_bytes": (_sz, [_vp, _i, ctypes.POINTER(ctypes.c_uint32)]),
    "bf_param_grad_table_build": (_i, [_vp, _i, _vp, _sz]),
    "bf_param_grad_table": (_i, [_vp, _i, _u32, _i, _u64, _u32, _vp]),
    "bf_kl_grad": (_i, [_tp, _i, _u64, _u32, _vp, _vp, _vp, _vp]),
    "bf_embedding_fwd": (_i, [_vp, _vp, _vp, _vp, _i, _i64, _i64, _i64, _i, _u64, _u32, _u32, _vp]),
    "bf_embedding_bwd": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _i64, _i64, _i64, _i, _u64, _u32, _u32, _vp]),
    "bf_attention_fwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i64, ctypes.c_float, _vp]),
    "bf_attention_fwd_rows": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i64, _i, ctypes.c_float, _vp]),
    "bf_attention_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i64,
                              ctypes.c_float, _vp]),
    "bf_add_layernorm_bwd_workspace_bytes": (_sz, [_i64, _i]),
    "bf_add_layernorm_bwd": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _sz, _i, _i64, _i, ctypes.c_float, _vp]),
    "bf_embed_layernorm": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _i64, _i, _i, _i64, _i64, _i64, _i64, ctypes.c_float, _vp]),
    "bf_add_layernorm": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _i, _i64, _i, ctypes.c_float, _vp]),
    "bf_add_layernorm_rows": (_i, [_vp, _vp, _i64, _vp, _vp, _i, _vp, _i, _i64, _i, ctypes.c_float, _vp]),
    "bf_dropout_keep_host": (_i, [_vp, _u64, _u64, ctypes.c_float, _u64, _u32, _u32]),
    "bf_attention_fwd_dropout": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i64, ctypes.c_float,
                                      ctypes.c_float, _u64, _u32, _u32, _u64, _vp, _vp, _vp]),
    "bf_attention_bwd_dropout": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i64,
                                      ctypes.c_float, ctypes.c_float, _vp, _vp]),
    "bf_add_layernorm_dropout": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _i, _i64, _i, ctypes.c_float, ctypes.c_float, _u64, _u32,
                                      _u32, _u64, _vp, _vp]),
    "bf_add_layernorm_dropout_bwd": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _i, _i64, _i, ctypes.c_float,
                                          ctypes.c_float, _u64, _u32, _u32, _u64, _vp, _vp]),
    "bf_add_layernorm_bwd_sum": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _i, _i64, _i, ctypes.c_float,
                                      ctypes.c_float, _u64, _u32, _u32, _u64, _vp, _vp]),
    "bf_attention_bwd_colsum": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i64,
                                     ctypes.c_float, ctypes.c_float, _vp, _i, _vp, _vp, _vp]),
    "bf_attention_fwd_gqa": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, ctypes.c_float, _vp]),
    "bf_attention_bwd_gqa": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, ctypes.c_float, _vp]),
    "bf_attention_decode_gqa": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, ctypes.c_float, _vp]),
    "bf_attention_decode_workspace_bytes": (_i64, [_vp]),
    "bf_attention_decode_gqa_len": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, ctypes.c_float, _vp]),
    # the sliding-window siblings: the same arguments plus int32 window before scaling
    "bf_attention_fwd_gqa_window": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, ctypes.c_float, _vp]),
    "bf_attention_bwd_gqa_window": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i,
                                         ctypes.c_float, _vp]),
    "bf_attention_decode_gqa_window": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, ctypes.c_float, _vp]),
    "bf_attention_decode_gqa_len_window": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, ctypes.c_float, _vp]),
    # the decoder layer's own ops (bf_decoder_blocks.hip)
    "bf_add_rmsnorm": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _i, _i64, _i, ctypes.c_float, _vp]),
    "bf_rope_qk": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp]),
    "bf_swiglu": (_i, [_vp, _i64, _vp, _i64, _vp, _i64, _i, _i64, _i, _vp]),
    # ... and their backward
    "bf_add_rmsnorm_bwd_workspace_bytes": (_sz, [_i64, _i]),
    "bf_add_rmsnorm_bwd": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _sz, _i, _i64, _i, ctypes.c_float, _vp]),
    "bf_rope_qk_bwd": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp]),
    "bf_swiglu_bwd": (_i, [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i, _i64, _i, _vp]),
    "bf_generate_step": (_i, [_vp, _vp, _vp, _vp, _i64, _i64, _i, _vp, _i64, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _i64,
                              _i64, _i, _vp, _vp]),
    "bf_generate_step_stat_probs": (_i, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i, _vp, _i64, _vp, _i64, _i64, _vp, _vp, _vp,
                                         _vp, _vp, _i64, _i64, _i, _vp, _vp]),
    "bf_probs_truncate": (_i, [_vp, _vp, _i64, _i64, _i64, ctypes.c_float, ctypes.c_float, _vp]),
    "bf_logits_process": (_i, [_vp, _i, _i64, _i64, _i64, _vp, _vp, _i64, _i64, _i64, _vp, _i64, ctypes.c_float, _i64,
                               _i64, _i64, ctypes.c_float, _vp]),
    "bf_profile_enable": (_i, [_i]),
    "bf_profile_reset": (_i, []),
    "bf_probe_stream_read": (_i, [_vp, _sz, _vp, _vp]),
    "bf_fused_small_max_rows": (_i, []),
    "bf_set_fused_small_max_rows": (_i, [_i]),
    "bf_fused_small_rows_for": (_i, [_i, _i]),
    "bf_profile_read": (_i, [_i, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_double),
                             ctypes.POINTER(ctypes.c_double)]),
    "bf_profile_read_launches": (_sz, [_i, _vp, _vp, _sz]),
    "bf_mc_predictive_bytes": (_sz, [_i64, _i64, _i, _i, ctypes.POINTER(ctypes.c_size_t)]),
    "bf_mc_predictive_workspace_bytes": (_sz, [_i]),
    "bf_mc_predictive_partial": (_i, [_vp, _i, _i64, _i64, _i, _i64, _i64, _vp, _i64, _i, _i, _vp, _vp, _sz, _vp]),
    "bf_mc_predictive_finish": (_i, [_vp, _i64, _i64, _i, _vp, _i64, _vp, _vp, _sz, _vp]),
}


class bf_predictive_out_t(ctypes.Structure):
    _fields_ = [(name, ctypes.c_void_p) for name in (
        "d_probs", "d_predictive_entropy", "d_expected_entropy", "d_mutual_information", "d_prediction",
        "d_log_likelihood", "d_correct_per_sample", "d_scalars", "d_counts")]


class bf_attn_gqa_t(ctypes.Structure):
    _fields_ = [("B", ctypes.c_int32), ("T", ctypes.c_int32), ("H", ctypes.c_int32), ("Hkv", ctypes.c_int32),
                ("head_dim", ctypes.c_int32), ("causal", ctypes.c_int32), ("q_stride", ctypes.c_int64 * 3),
                ("k_stride", ctypes.c_int64 * 3), ("v_stride", ctypes.c_int64 * 3)]


class bf_attn_decode_t(ctypes.Structure):
    _fields_ = [("N", ctypes.c_int32), ("Tq", ctypes.c_int32), ("Tk", ctypes.c_int32), ("H", ctypes.c_int32),
                ("Hkv", ctypes.c_int32), ("head_dim", ctypes.c_int32), ("q_stride", ctypes.c_int64 * 3),
                ("k_stride", ctypes.c_int64 * 3), ("v_stride", ctypes.c_int64 * 3)]


class bf_rope_t(ctypes.Structure):
    _fields_ = [("B", ctypes.c_int32), ("T", ctypes.c_int32), ("H", ctypes.c_int32), ("Hkv", ctypes.c_int32),
                ("head_dim", ctypes.c_int32), ("cos_batch", ctypes.c_int32), ("q_stride", ctypes.c_int64 * 3),
                ("k_stride", ctypes.c_int64 * 3), ("q_out_stride", ctypes.c_int64 * 3), ("k_out_stride", ctypes.c_int64 * 3)]


class bf_pgrad_t(ctypes.Structure):
    _fields_ = [("d_dw", ctypes.c_void_p), ("d_rho", ctypes.c_void_p), ("d_dmu", ctypes.c_void_p), ("d_drho", ctypes.c_void_p),
                ("n", ctypes.c_uint64), ("stream_id", ctypes.c_uint32), ("splits", ctypes.c_int32)]


# what include/bayeformers_amd_softcap.h declares (the soft-cap attention entries, Gemma 2): the arguments of the window
# entries with int32 window (0 = none) and float softcap before scaling; the decode entry takes a nullable kv_len
SOFTCAP_SYMBOLS = {
    "bf_attention_fwd_gqa_softcap": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, ctypes.c_float, ctypes.c_float,
                                          _vp]),
    "bf_attention_bwd_gqa_softcap": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i,
                                          ctypes.c_float, ctypes.c_float, _vp]),
    "bf_attention_decode_gqa_softcap": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, ctypes.c_float,
                                             ctypes.c_float, _vp]),
}

# what include/bayeformers_amd_family_blocks.h declares (the decoder-block entries of the Gemma and Qwen3 families):
# bf_add_rmsnorm with a second gamma, a weight offset and a second eps; bf_rope_qk with (gamma_q, gamma_k, param_dtype,
# weight_offset, eps) behind cs_dtype; bf_swiglu's arguments
FAMILY_BLOCK_SYMBOLS = {
    "bf_norm_add_rmsnorm": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _i, _i64, _i, ctypes.c_float, ctypes.c_float, _vp]),
    "bf_qknorm_rope": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _i, ctypes.c_float, _vp, _vp, _i, _vp, _vp]),
    "bf_geglu": (_i, [_vp, _i64, _vp, _i64, _vp, _i64, _i, _i64, _i, _vp]),
}

# what include/bayeformers_amd_family_blocks_bwd.h declares, their backward entries: the forwards' arguments with the gradients, the parameter gradients
# (fp32) and a workspace
FAMILY_BLOCK_BWD_SYMBOLS = {
    "bf_norm_add_rmsnorm_bwd_workspace_bytes": (_sz, [_i64, _i, _i]),
    "bf_norm_add_rmsnorm_bwd": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _i, _i64, _i,
                                     ctypes.c_float, ctypes.c_float, _vp]),
    "bf_qknorm_rope_bwd_workspace_bytes": (_sz, [_vp, _i]),
    "bf_qknorm_rope_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _i, ctypes.c_float, _vp, _vp, _vp, _vp, _vp,
                                _sz, _i, _vp, _vp]),
    "bf_geglu_bwd": (_i, [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i, _i64, _i, _vp]),
}

# what include/bayeformers_amd_packed.h declares (banded causal attention for packed sequences): the plain entries'
# arguments with the int32 bounds d_lo (and d_hi in the backward) in place of the key mask and its flag
PACKED_SYMBOLS = {
    "bf_attention_fwd_gqa_band": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, ctypes.c_float, _vp]),
    "bf_attention_bwd_gqa_band": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, ctypes.c_float,
                                       _vp]),
}

# what include/bayeformers_amd_fp8.h declares (the centred FP8 rows of Model.pinned_samples(keep_weights="fp8")): quantise,
# dequantise, and bf_gemm_nt_skinny's arguments with (q, scale, center) in place of (w, w_dtype)
FP8_SYMBOLS = {
    "bf_fp8_rows_quantize": (_i, [_vp, _i, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "bf_fp8_rows_dequantize": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "bf_gemm_nt_skinny_fp8": (_i, [_vp, _i, _i64, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "bf_gemm_nt_skinny_fp8_workspace_bytes": (_sz, [_i, _i, _i, _i]),
}

# what include/bayeformers_amd_kv8.h declares (the FP8 KV cache of sample_generate(kv_cache="fp8")): append (K and V with
# their strides, the four cache buffers, the device fill pointer), dequantise, and bf_attention_decode_gqa_softcap's
# arguments with (kq, vq, k_scale, v_scale) in place of (k, v)
KV8_SYMBOLS = {
    "bf_kv8_append": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "bf_kv8_dequantize": (_i, [_vp, _vp, _vp, _i, _i64, _i, _vp]),
    "bf_attention_decode_gqa_kv8": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, ctypes.c_float,
                                         ctypes.c_float, _vp]),
}

# what include/bayeformers_amd_ring.h declares (the ring-buffer KV cache of sample_generate(sliding_cache="ring")): the
# 16-bit append (K and V with their strides, the two cache buffers, the device fill pointer, N, Hkv, T, D, ring_slots),
# bf_kv8_append's arguments with ring_slots in place of the capacity, and the decode entries: bf_attention_decode_gqa_softcap's
# and bf_attention_decode_gqa_kv8's arguments with ring_slots in front of the window
RING_SYMBOLS = {
    "bf_kv_ring_append": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "bf_kv8_ring_append": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "bf_attention_decode_gqa_ring": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _i, ctypes.c_float,
                                          ctypes.c_float, _vp]),
    "bf_attention_decode_gqa_ring_kv8": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _i,
                                              ctypes.c_float, ctypes.c_float, _vp]),
}

# what include/bayeformers_amd_chunk.h declares (the cached-chunk attention of sample_generate(prefill_chunk=...)):
# (q, k, v, mask, mask_off, kv_len, out, dtype, shape, window, key_origin, softcap, scaling, stream), and the same on an FP8 cache with
# (kq, vq, k_scale, v_scale) in place of (k, v)
CHUNK_SYMBOLS = {
    "bf_attention_chunk_gqa": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _i, ctypes.c_float, ctypes.c_float,
                                    _vp]),
    "bf_attention_chunk_gqa_kv8": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _i, _i, ctypes.c_float,
                                        ctypes.c_float, _vp]),
}

# what include/bayeformers_amd_encoder_any.h declares (the encoder attention at any sequence length): each entry takes the
# arguments of its sibling above (bf_attention_fwd, _fwd_dropout, _fwd_rows, bf_attention_bwd, _bwd_dropout)
ENCODER_ANY_SYMBOLS = {
    "bf_attention_fwd_any": SYMBOLS["bf_attention_fwd"],
    "bf_attention_fwd_any_dropout": SYMBOLS["bf_attention_fwd_dropout"],
    "bf_attention_fwd_any_rows": SYMBOLS["bf_attention_fwd_rows"],
    "bf_attention_bwd_any": SYMBOLS["bf_attention_bwd"],
    "bf_attention_bwd_any_dropout": SYMBOLS["bf_attention_bwd_dropout"],
}

# what include/bayeformers_amd_lora.h declares (the rank-r terms of bnn.LoRALinear): forward (x, A_s, B, y, h, scale, dtype, S, M,
# N, K, r, workspace, bytes, stream), backward (x, dy, A_s, B, h, dx, dA, dB, scale, dtype, ...), and the reduction of dA to
# (dmu, drho) with bf_param_grad_table's arithmetic
LORA_SYMBOLS = {
    "bf_lora_fwd_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i]),
    "bf_lora_fwd": (_i, [_vp, _vp, _vp, _vp, _vp, ctypes.c_float, _i, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "bf_lora_bwd_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i]),
    "bf_lora_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_float, _i, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "bf_lora_reduce_da": (_i, [_vp, _vp, _u64, _i, _u64, _u32, _u32, _vp, _vp, _vp]),
}

# what include/bayeformers_amd_spec.h declares (the epilogue of one speculative iteration of sample_generate): (argmax, draft,
# probs, the three entropies, B, gamma, V, S, state, max_new_tokens, sequences, seq_stride, T0, stats, finished, lengths,
# verify ids / positions, draft ids / positions, rewind, speculation, eos, pad, stream)
SPEC_SYMBOLS = {
    "bf_spec_accept": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i, _vp, _i64, _vp, _i64, _i64, _vp, _vp, _vp,
                            _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp]),
}

# what include/bayeformers_amd_lrt.h declares (bnn.Linear with local = True: the passes around the two products of the local
# reparameterisation estimator, and the closed-form Gaussian KL terms)
LRT_SYMBOLS = {
    "bf_lrt_operands": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "bf_lrt_square": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "bf_lrt_combine": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _u64, _u32, _u32, _vp]),
    "bf_lrt_zeta": (_i, [_vp, _i, _i, _i, _u64, _u32, _u32, _vp]),
    "bf_lrt_grad_prepare_workspace_bytes": (_sz, [_i, _i]),
    "bf_lrt_grad_prepare": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _u64, _u32, _u32, _vp, _sz, _vp]),
    "bf_lrt_dx": (_i, [_vp, _i64, _vp, _vp, _i, _i, _i, _vp]),
    "bf_lrt_drho": (_i, [_vp, _vp, _vp, _u64, _vp]),
    "bf_sample_logprob_like": (_i, [_tp, _i, _i, _u64, _u32, _vp, _vp, _sz, _i, _vp]),
    "bf_kl_gaussian_workspace_bytes": (_sz, []),
    "bf_kl_gaussian": (_i, [_vp, _vp, _vp, _vp, _u64, _vp, _vp, _sz, _vp]),
}

# what include/bayeformers_amd_moe.h declares (bnn.Experts: the route of the slots to their (sample, expert) groups, the two
# grouped products over the tile table and the weighted sum over a row's k slots)
MOE_SYMBOLS = {
    "bf_moe_max_tiles": (_sz, [_i, _i, _i, _i]),
    "bf_moe_route_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "bf_moe_route": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp, _sz, _vp]),
    "bf_moe_gate_up_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i, _i]),
    "bf_moe_gate_up": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "bf_moe_down_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i, _i]),
    "bf_moe_down": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    "bf_moe_combine_workspace_bytes": (_sz, [_i, _i, _i]),
    "bf_moe_combine": (_i, [_vp, _vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
}
BF_MOE_TILE_ROWS, BF_MOE_MAX_TOPK, BF_MOE_MAX_GROUPS = 16, 16, 4096  # include/bayeformers_amd_moe.h

BF_LRT_STREAM = 0x20000000  # csrc/bf_philox.h

BF_PROF_SAMPLE, BF_PROF_GEMM, BF_PROF_FUSED_SMALL, BF_PROF_FUSED_WS = 0, 1, 2, 3
BF_ACT_NONE, BF_ACT_GELU = 0, 1

ABI_VERSION = 6  # bf_version() of the library these bindings describe (include/bayeformers_amd.h: BF_VERSION_*)

_lib = None


class BayeFormersAMDError(RuntimeError):
    pass


def lib():
    """Load (once) and return the C-ABI library; raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise BayeFormersAMDError(
                f"{LIB_PATH} is missing: build it with `python -m bayeformers_amd.build` "
                "(there is no CPU or PyTorch fallback for the Monte-Carlo forward path)")
        l = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in list(SYMBOLS.items()) + list(SOFTCAP_SYMBOLS.items()):
            fn = getattr(l, name)  # AttributeError here = header/library drift
            fn.restype = res
            fn.argtypes = args
        for name, (res, args) in list(FAMILY_BLOCK_SYMBOLS.items()) + list(FAMILY_BLOCK_BWD_SYMBOLS.items()):
            fn = getattr(l, name, None)
            if fn is None:  # a library from before these entries reports the version these bindings expect
                raise BayeFormersAMDError(
                    f"{LIB_PATH} lacks {name} (the Gemma / Qwen3 decoder-block entries): rebuild it with "
                    "`python -m bayeformers_amd.build`")
            fn.restype = res
            fn.argtypes = args
        for name, (res, args) in PACKED_SYMBOLS.items():
            fn = getattr(l, name, None)
            if fn is None:  # likewise: a library from before these entries reports the same version
                raise BayeFormersAMDError(
                    f"{LIB_PATH} lacks {name} (the packed-sequence attention entries): rebuild it with "
                    "`python -m bayeformers_amd.build`")
            fn.restype = res
            fn.argtypes = args
        for name, (res, args) in FP8_SYMBOLS.items():
            fn = getattr(l, name, None)
            if fn is None:  # likewise
                raise BayeFormersAMDError(
                    f"{LIB_PATH} lacks {name} (the FP8 kept-weight entries): rebuild it with "
                    "`python -m bayeformers_amd.build`")
            fn.restype = res
            fn.argtypes = args
        for name, (res, args) in KV8_SYMBOLS.items():
            fn = getattr(l, name, None)
            if fn is None:  # likewise
                raise BayeFormersAMDError(
                    f"{LIB_PATH} lacks {name} (the FP8 KV-cache entries): rebuild it with "
                    "`python -m bayeformers_amd.build`")
            fn.restype = res
            fn.argtypes = args
        for name, (res, args) in CHUNK_SYMBOLS.items():
            fn = getattr(l, name, None)
            if fn is None:  # likewise
                raise BayeFormersAMDError(
                    f"{LIB_PATH} lacks {name} (the cached-chunk attention entries): rebuild it with "
                    "`python -m bayeformers_amd.build`")
            fn.restype = res
            fn.argtypes = args
        for name, (res, args) in ENCODER_ANY_SYMBOLS.items():
            fn = getattr(l, name, None)
            if fn is None:  # likewise
                raise BayeFormersAMDError(
                    f"{LIB_PATH} lacks {name} (the any-length encoder attention entries): rebuild it with "
                    "`python -m bayeformers_amd.build`")
            fn.restype = res
            fn.argtypes = args
        for name, (res, args) in RING_SYMBOLS.items():
            fn = getattr(l, name, None)
            if fn is None:  # likewise
                raise BayeFormersAMDError(
                    f"{LIB_PATH} lacks {name} (the ring-buffer KV-cache entries): rebuild it with "
                    "`python -m bayeformers_amd.build`")
            fn.restype = res
            fn.argtypes = args
        for name, (res, args) in LORA_SYMBOLS.items():
            fn = getattr(l, name, None)
            if fn is None:  # likewise
                raise BayeFormersAMDError(
                    f"{LIB_PATH} lacks {name} (the Bayesian LoRA entries): rebuild it with "
                    "`python -m bayeformers_amd.build`")
            fn.restype = res
            fn.argtypes = args
        for name, (res, args) in SPEC_SYMBOLS.items():
            fn = getattr(l, name, None)
            if fn is None:  # likewise
                raise BayeFormersAMDError(
                    f"{LIB_PATH} lacks {name} (the speculative-decoding entry): rebuild it with "
                    "`python -m bayeformers_amd.build`")
            fn.restype = res
            fn.argtypes = args
        for name, (res, args) in LRT_SYMBOLS.items():
            fn = getattr(l, name, None)
            if fn is None:  # likewise
                raise BayeFormersAMDError(
                    f"{LIB_PATH} lacks {name} (the local reparameterisation entries): rebuild it with "
                    "`python -m bayeformers_amd.build`")
            fn.restype = res
            fn.argtypes = args
        for name, (res, args) in MOE_SYMBOLS.items():
            fn = getattr(l, name, None)
            if fn is None:  # likewise
                raise BayeFormersAMDError(
                    f"{LIB_PATH} lacks {name} (the mixture-of-experts entries): rebuild it with "
                    "`python -m bayeformers_amd.build`")
            fn.restype = res
            fn.argtypes = args
        if l.bf_version() != ABI_VERSION:  # a stale .so called through newer signatures corrupts the stack: refuse it
            raise BayeFormersAMDError(
                f"{LIB_PATH} is version {l.bf_version()}, these bindings expect {ABI_VERSION}: rebuild it with "
                "`python -m bayeformers_amd.build`")
        _lib = l
    return _lib


_stale = None


def stale_counter() -> int:
    """Current value of the library's stale-prior counter (bf_stale_counter): a host-memory word the kernels bump when a
    prior's baked constants fail their device-side re-check.  Reading it does not synchronise."""
    global _stale
    if _stale is None:
        p = ctypes.POINTER(ctypes.c_uint32)()
        if lib().bf_stale_counter(ctypes.byref(p)) != 0:
            return 0  # no HIP device in this process (host-only tests): nothing can have bumped it
        _stale = p
    return int(_stale[0])


def check(rc, what):
    if rc != 0:
        msg = lib().bf_last_error()
        raise BayeFormersAMDError(f"{what} failed: {msg.decode() if msg else 'unknown error'}")
