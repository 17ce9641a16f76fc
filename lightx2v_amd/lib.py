"""ctypes binding of the C-ABI (include/x2v.h) + thin torch-tensor wrappers.

PyTorch is plumbing here: it owns device memory (caching allocator) and the stream; every wrapper passes
raw `data_ptr()`s, element strides and `torch.cuda.current_stream().cuda_stream` to libx2v_hip.so.
The library is REQUIRED: importing this module without the built .so, or calling an op on a non-gfx950
device, raises — there is no eager/PyTorch fallback on the product path.
"""
import ctypes
import os

import math

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("X2V_LIB_PATH") or os.path.join(_HERE, "libx2v_hip.so")  # X2V_LIB_PATH: an alternative build of the same sources (tools/build_variant.sh, A/B runs)

EPI_NONE, EPI_GELU_TANH, EPI_RESIDUAL, EPI_SILU = 0, 1, 2, 3
ACT_GELU_ERF = 4  # x2v.h X2V_ACT_GELU_ERF (activation() only: exact GELU of the i2v CLIP-feature MLP)
ROUND_FP32, ROUND_REF = 0, 1

_c_void_p, _i64, _i32, _f32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float

# name -> argtypes (restype int unless listed in _RESTYPES); mirrors include/x2v.h one to one
PROTOTYPES = {
    "x2v_init": [_i32],
    "x2v_last_error": [],
    "x2v_version": [],
    "x2v_device_info": [_i32, ctypes.POINTER(_i32), ctypes.POINTER(_i32), ctypes.c_char_p, _i32],
    "x2v_switches": [ctypes.c_char_p, _i32],
    "x2v_quant_fp8_rowwise_blocked": [_c_void_p, _i64, _i32, _i64, _c_void_p, _i64, _c_void_p, _i64, _i32, _c_void_p],
    "x2v_rmsnorm_bf16": [_c_void_p, _i64, _c_void_p, _c_void_p, _i64, _i64, _i32, _f32, _i32, _c_void_p],
    "x2v_layernorm_bf16": [_c_void_p, _i64, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _i64, _i64, _i32, _f32, _c_void_p],
    "x2v_layernorm_bf16_variant": [_c_void_p, _i64, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _i64, _i64, _i32, _f32, _i32, _c_void_p],
    "x2v_rmsnorm_rope_scaled_bf16_variant": [_c_void_p, _i64, _c_void_p, _i64, _c_void_p, _c_void_p, _c_void_p, _i64, _i32, _i64, _i32, _i32, _i32, _f32, _i32, _f32, _i32, _c_void_p],
    "x2v_rmsnorm_rope_bf16": [_c_void_p, _i64, _c_void_p, _i64, _c_void_p, _c_void_p, _c_void_p, _i64, _i32, _i64, _i32, _i32, _i32, _f32, _i32, _c_void_p],
    "x2v_rmsnorm_rope_scaled_bf16": [_c_void_p, _i64, _c_void_p, _i64, _c_void_p, _c_void_p, _c_void_p, _i64, _i32, _i64, _i32, _i32, _i32, _f32, _i32, _f32, _c_void_p],
    "x2v_gemm_bf16_vt": [_c_void_p, _i64, _c_void_p, _i64, _c_void_p, _c_void_p, _i64, _i64, _i32, _i32, _c_void_p],
    "x2v_headnorm_rope_blocked_bf16": [_c_void_p, _c_void_p, _i64, _i32, _i64, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _i64, _i32, _i64, _f32, _i32, _f32, _c_void_p],
    "x2v_headnorm_rope_bf16": [_c_void_p, _i64, _c_void_p, _i64, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _i64, _i32, _i64, _f32, _i32, _f32, _c_void_p],
    "x2v_gate_residual_bf16": [_c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _i32, _c_void_p],
    "x2v_activation_bf16": [_c_void_p, _c_void_p, _i64, _i32, _c_void_p],
    "x2v_gemm_bf16": [_c_void_p, _i64, _c_void_p, _i64, _c_void_p, _c_void_p, _i64, _i64, _i32, _i32, _i32, _c_void_p, _i64, _c_void_p, _c_void_p],
    "x2v_gemm_bf16_resid_period": [_c_void_p, _i64, _c_void_p, _i64, _c_void_p, _c_void_p, _i64, _i64, _i32, _i32, _c_void_p, _i64, _i64, _c_void_p, _i32, _c_void_p],
    "x2v_gemm_fp8_resid_period": [_c_void_p, _i64, _c_void_p, _c_void_p, _i64, _c_void_p, _c_void_p, _c_void_p, _i64, _i64, _i32, _i32, _c_void_p, _i64, _i64, _c_void_p, _i32, _c_void_p],
    "x2v_gemm_bf16_variant": [_c_void_p, _i64, _c_void_p, _i64, _c_void_p, _c_void_p, _i64, _i64, _i32, _i32, _i32, _c_void_p, _i64, _c_void_p, _i32, _c_void_p],
    "x2v_gemm_bf16_blocked": [_c_void_p, _i64, _i32, _i64, _c_void_p, _i64, _c_void_p, _c_void_p, _i64, _i32, _i64, _i64, _i32, _i32, _i32, _c_void_p, _i64, _c_void_p, _c_void_p],
    "x2v_gemm_fp8_blocked": [_c_void_p, _i64, _i32, _i64, _c_void_p, _c_void_p, _i64, _c_void_p, _c_void_p, _c_void_p, _i64, _i32, _i64, _i64, _i32, _i32, _i32, _c_void_p, _i64,
                             _c_void_p, _c_void_p],
    "x2v_rmsnorm_rope_blocked_bf16": [_c_void_p, _i64, _c_void_p, _i64, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _i64, _i32, _i64, _i64, _i32, _i64, _i32, _i32, _i32, _f32,
                                      _i32, _f32, _c_void_p],
    "x2v_gemm_kernel_choice": [_i64, _i32, _i32, _i64, _i64, _i32],
    "x2v_attn_fwd_bf16": [_c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _i64, _i64, _i32, _i32, _f32, _c_void_p],
    "x2v_transpose_heads_bf16": [_c_void_p, _i64, _c_void_p, _i64, _i64, _i32, _c_void_p],
    "x2v_transpose_heads_append_bf16": [_c_void_p, _i64, _c_void_p, _i64, _i64, _i64, _i32, _c_void_p],
    "x2v_attn_fwd_bf16_vt_batched": [_c_void_p, _i64, _i64, _c_void_p, _i64, _i64, _c_void_p, _i64, _i64, _c_void_p, _i64, _i64, _i64, _i64, _i32, _i32, _i32, _f32, _i32, _c_void_p],
    "x2v_attn_vt_launch_plan": [_i64, _i64, _i32, _i32, _i32],
    "x2v_mfma_probe_bf16": [_i32, ctypes.POINTER(_f32), _c_void_p],
    "x2v_attn_fwd_bf16_vt": [_c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _i64, _i64, _i32, _i32, _f32, _i32, _c_void_p],
    "x2v_attn_fwd_bf16_vt_carry": [_c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _i64, _i64, _i32, _i32, _f32, _i32,
                                   _c_void_p],
    "x2v_attn_bsr_fwd_bf16_vt": [_c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _i64, _i64, _i32, _i32, _f32, _i32, _c_void_p, _i64, _i64, _i32, _c_void_p],
    "x2v_attn_fwd_bf16_variant": [_c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _i64, _i64, _i32, _i32, _f32, _i32, _c_void_p],
    "x2v_attn_mx_sizes": [_i64, _i64, _i32, ctypes.POINTER(_i64)],
    "x2v_attn_mx_kmean_f32": [_c_void_p, _i64, _c_void_p, _i64, _i32, _c_void_p],
    "x2v_attn_mx_quant_qk": [_c_void_p, _i64, _c_void_p, _i32, _f32, _c_void_p, _c_void_p, _i64, _i64, _i32, _c_void_p],
    "x2v_attn_mx_quant_vt": [_c_void_p, _i64, _c_void_p, _c_void_p, _i64, _i32, _c_void_p],
    "x2v_attn_mx_fwd": [_c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _i64, _i64, _i64, _i32, _c_void_p],
    "x2v_quant_fp8_rowwise": [_c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _i32, _c_void_p],
    "x2v_layernorm_quant_fp8": [_c_void_p, _i64, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _i64, _c_void_p, _i64, _i32, _f32, _c_void_p],
    "x2v_quant_mxfp8_bf16": [_c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _i32, _c_void_p],
    "x2v_gemm_mxfp8_variant": [_c_void_p, _i64, _c_void_p, _c_void_p, _i64, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _i64, _i64, _i32, _i32, _i32, _c_void_p],
    "x2v_gemm_mxfp8_epi": [_c_void_p, _i64, _c_void_p, _c_void_p, _i64, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _i64, _i64, _i32, _i32, _i32, _c_void_p, _i64, _c_void_p, _c_void_p],
    "x2v_gemm_mxfp8": [_c_void_p, _i64, _c_void_p, _c_void_p, _i64, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _i64, _i64, _i32, _i32, _c_void_p],
    "x2v_quant_mxfp6_bf16": [_c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _i32, _c_void_p],
    "x2v_gemm_mxfp6_mxfp8_variant": [_c_void_p, _i64, _c_void_p, _c_void_p, _i64, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _i64, _i64, _i32, _i32, _i32, _c_void_p],
    "x2v_gemm_mxfp6_mxfp8_epi": [_c_void_p, _i64, _c_void_p, _c_void_p, _i64, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _i64, _i64, _i32, _i32, _i32, _c_void_p, _i64, _c_void_p, _c_void_p],
    "x2v_gemm_mxfp6_mxfp8": [_c_void_p, _i64, _c_void_p, _c_void_p, _i64, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _i64, _i64, _i32, _i32, _c_void_p],
    "x2v_quant_mxfp4_bf16": [_c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _i32, _c_void_p],
    "x2v_gemm_mxfp4_variant": [_c_void_p, _i64, _c_void_p, _c_void_p, _i64, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _i64, _i64, _i32, _i32, _i32, _c_void_p],
    "x2v_gemm_mxfp4_epi": [_c_void_p, _i64, _c_void_p, _c_void_p, _i64, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _i64, _i64, _i32, _i32, _i32, _c_void_p, _i64, _c_void_p, _c_void_p],
    "x2v_gemm_mxfp4": [_c_void_p, _i64, _c_void_p, _c_void_p, _i64, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _i64, _i64, _i32, _i32, _c_void_p],
    "x2v_gemm_fp8": [_c_void_p, _i64, _c_void_p, _c_void_p, _i64, _c_void_p, _c_void_p, _c_void_p, _i64, _i64, _i32, _i32, _i32, _c_void_p, _i64, _c_void_p, _c_void_p],
    "x2v_gemm_fp8_variant": [_c_void_p, _i64, _c_void_p, _c_void_p, _i64, _c_void_p, _c_void_p, _c_void_p, _i64, _i64, _i32, _i32, _i32, _c_void_p, _i64, _c_void_p, _i32, _c_void_p],
    "x2v_quant_int8_rowwise": [_c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _i32, _c_void_p],
    "x2v_quant_int8_rowwise_blocked": [_c_void_p, _i64, _i32, _i64, _c_void_p, _i64, _c_void_p, _i64, _i32, _c_void_p],
    "x2v_layernorm_quant_int8": [_c_void_p, _i64, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _i64, _c_void_p, _i64, _i32, _f32, _c_void_p],
    "x2v_gemm_int8": [_c_void_p, _i64, _c_void_p, _c_void_p, _i64, _c_void_p, _c_void_p, _c_void_p, _i64, _i64, _i32, _i32, _i32, _c_void_p, _i64, _c_void_p, _c_void_p],
    "x2v_gemm_int8_variant": [_c_void_p, _i64, _c_void_p, _c_void_p, _i64, _c_void_p, _c_void_p, _c_void_p, _i64, _i64, _i32, _i32, _i32, _c_void_p, _i64, _c_void_p, _i32, _c_void_p],
    "x2v_gemm_int8_resid_period": [_c_void_p, _i64, _c_void_p, _c_void_p, _i64, _c_void_p, _c_void_p, _c_void_p, _i64, _i64, _i32, _i32, _c_void_p, _i64, _i64, _c_void_p, _i32, _c_void_p],
    "x2v_gemm_int8_blocked": [_c_void_p, _i64, _i32, _i64, _c_void_p, _c_void_p, _i64, _c_void_p, _c_void_p, _c_void_p, _i64, _i32, _i64, _i64, _i32, _i32, _i32, _c_void_p, _i64,
                              _c_void_p, _c_void_p],
    "x2v_gemm_int8_kernel_choice": [_i64, _i32, _i32, _i64, _i64],
    "x2v_gemm_mx_kernel_choice": [_i32, _i64, _i32, _i32, _i64, _i64],
    "x2v_unipc_step_f32": [_c_void_p, _c_void_p, _c_void_p, _i32, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, ctypes.POINTER(_f32), _i32, _i32, _i64,
                           _c_void_p],
    "x2v_distill_step_f32": [_c_void_p, _c_void_p, _f32, _c_void_p, _i32, _c_void_p, _f32, _f32, _f32, _c_void_p, _c_void_p, _i64, _c_void_p],
    "x2v_sinusoid_embed_bf16": [_c_void_p, _c_void_p, _i32, _i32, _c_void_p],
    "x2v_sinusoid_embed_f64_bf16": [_c_void_p, _c_void_p, _i32, _i32, _c_void_p],
    "x2v_causal_conv3d_f32": [_c_void_p, _c_void_p, _i32, _c_void_p, _c_void_p, _c_void_p, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _c_void_p],
    "x2v_vae_conv_f32": [_c_void_p, _i64, _i64, _i64, _c_void_p, _i64, _c_void_p, _c_void_p, _c_void_p, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _c_void_p],
    "x2v_vae_prep_f32": [_c_void_p, _c_void_p, _i32, _i32, _i32, _i32, _c_void_p, _c_void_p, _c_void_p, _i32, _i32, _i64, _i64, _c_void_p],
    "x2v_softmax_rows_f32": [_c_void_p, _i64, _i64, _i32, _f32, _c_void_p],
    "x2v_vae_conv_f16": [_c_void_p, _i64, _i64, _i64, _c_void_p, _i64, _c_void_p, _c_void_p, _c_void_p, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _c_void_p],
    "x2v_vae_conv_f16_cached": [_c_void_p, _c_void_p, _i64, _i64, _i64, _c_void_p, _i64, _c_void_p, _c_void_p, _c_void_p, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _c_void_p],
    "x2v_vae_conv_f16_cached_ok": [_i32, _i32, _i32, _i32, _i32, _i32],
    "x2v_vae_prep_f16": [_c_void_p, _c_void_p, _i32, _i32, _i32, _i32, _c_void_p, _c_void_p, _c_void_p, _i32, _i32, _i64, _i64, _i64, _c_void_p],
    "x2v_vae_prep_split_f16": [_c_void_p, _c_void_p, _i32, _i32, _i32, _i32, _c_void_p, _c_void_p, _c_void_p, _i32, _i32, _i64, _i64, _i64, _c_void_p],
    "x2v_vae_prep_ex_f16": [_c_void_p, _c_void_p, _i32, _i32, _i32, _i32, _c_void_p, _c_void_p, _i32, _i32, _i32, _i32, _i64, _i64, _c_void_p],
    "x2v_vae_prep_ex_f32": [_c_void_p, _c_void_p, _i32, _i32, _i32, _i32, _c_void_p, _c_void_p, _i32, _i32, _i32, _i32, _i64, _i64, _c_void_p],
    "x2v_vae_conv_s2_f16": [_c_void_p, _i64, _i64, _i64, _c_void_p, _i64, _c_void_p, _c_void_p, _i32, _i32, _i32, _i32, _i32, _i32, _c_void_p],
    "x2v_vae_video_prep": [_c_void_p, _i64, _i64, _i64, _i32, _i32, _i32, _c_void_p, _i64, _i64, _i64, _i32, _c_void_p],
    "x2v_vae_tile_compose_f32": [_c_void_p, _c_void_p, _c_void_p, _c_void_p, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _c_void_p, _i64, _i64, _i64, _i32, _c_void_p],
    "x2v_gemm_f16": [_c_void_p, _i64, _c_void_p, _i64, _c_void_p, _c_void_p, _i64, _i64, _i32, _i32, _i32, _c_void_p, _i64, _c_void_p],
    "x2v_gemm_f16_tile_choice": [_i64, _i32],
    "x2v_attn_f16_d80": [_c_void_p, _i64, _c_void_p, _i64, _i32, _i32, _i32, _f32, _c_void_p],
    "x2v_layernorm_f16": [_c_void_p, _i64, _c_void_p, _c_void_p, _c_void_p, _i64, _i64, _i32, _f32, _c_void_p],
    "x2v_clip_embed_f16": [_c_void_p, _i64, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _i64, _i32, _i32, _i32, _f32, _c_void_p],
    "x2v_clip_preprocess_f16": [_c_void_p, _i64, _i64, _i32, _i32, _c_void_p, _i64, _i32, _i32, _f32, _f32, _f32, _f32, _f32, _f32, _c_void_p],
    "x2v_gemm_rows_bf16": [_c_void_p, _i64, _c_void_p, _i64, _c_void_p, _i64, _i64, _i32, _i32, _i32, _c_void_p, _i64, _c_void_p],
    "x2v_gemm_rows_bf16_tile_choice": [_i64, _i32, _i32],
    "x2v_attn_bf16_d64_relbias": [_c_void_p, _i64, _c_void_p, _c_void_p, _i64, ctypes.POINTER(_i32), _i32, _i32, _f32, _c_void_p],
    "x2v_attn_f16_causal": [_c_void_p, _i64, _c_void_p, _i64, ctypes.POINTER(_i32), _i32, _i32, _i32, _i32, _c_void_p, _c_void_p, _f32, _c_void_p],
    "x2v_rmsnorm_f16": [_c_void_p, _i64, _c_void_p, _c_void_p, _i64, _i64, _i32, _f32, _c_void_p],
    "x2v_vae_replicate_border_f32": [_c_void_p, _i32, _i32, _i32, _i32, _i32, _i32, _c_void_p],
    "x2v_groupnorm_affine_f32": [_c_void_p, _i64, _i32, _i32, _c_void_p, _c_void_p, _f32, _c_void_p, _c_void_p, _c_void_p, _c_void_p],
    "x2v_softmax_rows_causal_f32": [_c_void_p, _i64, _i64, _i32, _f32, _i32, _i32, _c_void_p],
    "x2v_blend_axis_f32": [_c_void_p, _c_void_p, _i64, _i32, _i32, _i64, _i64, _i64, _i32, _c_void_p],
    "x2v_conv2d_bf16": [_c_void_p, _c_void_p, _i64, _i64, _i64, _c_void_p, _c_void_p, _c_void_p, _c_void_p, _i64, _i64, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32,
                        _c_void_p],
    "x2v_taehv_clamp_bf16": [_c_void_p, _i32, _i64, _i64, _c_void_p, _i32, _i32, _i32, _i32, _c_void_p],
}
_RESTYPES = {"x2v_last_error": ctypes.c_char_p, "x2v_version": ctypes.c_char_p}


class X2VError(RuntimeError):
    pass


def load_library(path=LIB_PATH):
    if not os.path.exists(path):
        raise X2VError(f"{path} is missing: build it with `python -m lightx2v_amd.build` (hipcc, gfx950). There is no fallback path.")
    lib = ctypes.CDLL(path)
    for name, argtypes in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError if the header and the library disagree
        fn.argtypes = argtypes
        fn.restype = _RESTYPES.get(name, ctypes.c_int)
    return lib


_lib = load_library()
_inited = set()


def version():
    return _lib.x2v_version().decode()


def switches():
    """The library's process-wide A/B switches (effective values, latched from the environment at first use) as a dict — x2v_switches."""
    buf = ctypes.create_string_buffer(256)
    _check(_lib.x2v_switches(buf, 256), "x2v_switches")
    return {k: int(v) for k, v in (kv.split("=") for kv in buf.value.decode().split())}


def _check(rc, what):
    if rc != 0:
        raise X2VError(f"{what} failed ({rc}): {_lib.x2v_last_error().decode()}")


def init(device_index=None):
    """Verify the device is gfx950 (raises otherwise)."""
    if not torch.cuda.is_available():
        raise X2VError("no HIP device visible: the x2v HIP path has no CPU fallback")
    idx = torch.cuda.current_device() if device_index is None else device_index
    if idx not in _inited:
        _check(_lib.x2v_init(idx), "x2v_init")
        _inited.add(idx)
    return idx


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _row2d(t, name):
    if t.dim() != 2 or t.stride(1) != 1:
        raise X2VError(f"{name}: expected a 2-D tensor with unit inner stride, got shape {tuple(t.shape)} strides {t.stride()}")
    if not t.is_cuda:
        raise X2VError(f"{name}: tensor is on {t.device}; the x2v HIP path has no CPU fallback")
    return t


def _bf16(t, name):
    if t.dtype != torch.bfloat16:
        raise X2VError(f"{name}: expected bfloat16, got {t.dtype}")
    return t


def _vt_operand(vt, who, num_heads, rows):  # vt as an attention operand: the V^T of transpose_heads / gemm_vt over `rows` key rows
    if vt.dtype != torch.bfloat16 or not vt.is_cuda or not vt.is_contiguous() or tuple(vt.shape) != (num_heads, (rows + 63) // 64, 128, 64):
        raise X2VError(f"{who}: vt must be the contiguous bf16 [H, ceil(rows/64), 128, 64] tensor of transpose_heads over {rows} rows, got {tuple(vt.shape)}")
    return vt


def _attn_out(out, who, rows, width, device):  # an attention call's bf16 result [rows, width]: `out` checked (its token stride may be longer), or a new tensor
    out2 = torch.empty((rows, width), dtype=torch.bfloat16, device=device) if out is None else _row2d(_bf16(out, "out"), "out")
    if out2.shape[0] != rows or out2.shape[1] < width:
        raise X2VError(f"{who}: out is {tuple(out2.shape)}, expected {rows} rows of at least {width} elements")
    return out2


def _vec(t, name, n=None, dtype=torch.bfloat16):
    """A per-channel operand (bias / norm weight / gate / scale row): None passes through; otherwise a contiguous device vector of
    `dtype` with `n` elements (any leading unit dims) — the C side only sees a pointer, so a wrong dtype would be silent."""
    if t is None:
        return None
    if t.dtype != dtype:
        raise X2VError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_cuda:
        raise X2VError(f"{name}: tensor is on {t.device}; the x2v HIP path has no CPU fallback")
    if n is not None and t.numel() != n:
        raise X2VError(f"{name}: expected {n} elements, got shape {tuple(t.shape)}")
    return t if t.is_contiguous() else t.contiguous()


# ----------------------------------------------------------------------------------------------------
def rmsnorm(x, weight, eps=1e-6, out=None, round_mode=ROUND_FP32):
    shape = x.shape
    x2 = _row2d(_bf16(x.reshape(-1, shape[-1]) if x.dim() != 2 else x, "x"), "x")
    out2 = torch.empty((x2.shape[0], x2.shape[1]), dtype=torch.bfloat16, device=x.device) if out is None else _row2d(out.reshape(-1, shape[-1]) if out.dim() != 2 else out, "out")
    init()
    if x2.shape[0] == 0:  # empty shard: torch hands out a null data_ptr, nothing to launch
        return out2.view(shape) if out is None else out
    _check(_lib.x2v_rmsnorm_bf16(_p(x2), x2.stride(0), _p(_vec(weight, "rmsnorm weight", x2.shape[1])), _p(out2), out2.stride(0), x2.shape[0], x2.shape[1], eps, round_mode, _stream()), "rmsnorm")
    return out2.view(shape) if out is None else out


def layernorm(x, weight=None, bias=None, scale=None, shift=None, eps=1e-6, out=None, variant=0):
    """LN(x)[*w+b] then optional adaLN `* (1 + scale) + shift` (scale/shift: [D] or [1,D] bf16).  variant: x2v_layernorm_bf16_variant."""
    x2 = _row2d(_bf16(x, "x"), "x")
    out2 = torch.empty_like(x2) if out is None else _row2d(out, "out")
    D = x2.shape[1]
    if (scale is None) != (shift is None):
        raise X2VError("layernorm: scale and shift must be given together")
    weight, bias = _vec(weight, "layernorm weight", D), _vec(bias, "layernorm bias", D)
    scale, shift = _vec(scale, "layernorm scale", D), _vec(shift, "layernorm shift", D)
    init()
    if x2.shape[0] == 0:
        return out2
    _check(
        _lib.x2v_layernorm_bf16_variant(_p(x2), x2.stride(0), _p(weight), _p(bias), _p(scale), _p(shift), _p(out2), out2.stride(0), x2.shape[0], x2.shape[1], eps, variant,
                                        _stream()),
        "layernorm",
    )
    return out2


ATTN_Q_PRESCALED = 0x100
ATTN_STAGGER = 0x200  # x2v.h X2V_ATTN_VT_STAGGER: query block b starts its key walk (b mod 8) tiles in (an opt-in; wan.SELF_ATTN_STAGGER decides for the Wan drivers)
ATTN_ONE_WALK = 0x400  # x2v.h X2V_ATTN_VT_ONE_WALK: never the persistent short-walk form (A/B runs, the bit-equality test of the two forms)
ATTN_FAST = 12  # "ping-pong" kernel on a pre-transposed V (x2v_transpose_heads_bf16 + x2v_attn_fwd_bf16_vt); used with
#                 ATTN_Q_PRESCALED by the fused block drivers.  attention() does the transposition itself for this variant.
ATTN_PRESCALE = 1.4426950408889634 / math.sqrt(128.0)  # softmax scale * log2(e) for head_dim 128


def rmsnorm_rope_(q, k, wq, wk, rope_cs, grid, num_heads, s0=0, eps=1e-6, round_mode=ROUND_FP32, q_out_scale=1.0, variant=0):
    """In place: q,k [S, H*128] ← RoPE3D(RMSNorm(q|k)); q additionally * q_out_scale inside its final rounding."""
    q2, k2 = _row2d(_bf16(q, "q"), "q"), _row2d(_bf16(k, "k"), "k")
    if rope_cs.dtype != torch.float32 or tuple(rope_cs.shape) != (1024, 64, 2) or not rope_cs.is_contiguous():
        raise X2VError("rope_cs must be a contiguous float32 [1024,64,2] (cos,sin) table")
    gf, gh, gw = grid
    wq, wk = _vec(wq, "norm_q weight", q2.shape[1]), _vec(wk, "norm_k weight", k2.shape[1])
    init()
    if q2.shape[0] == 0:
        return q, k
    _check(
        _lib.x2v_rmsnorm_rope_scaled_bf16_variant(_p(q2), q2.stride(0), _p(k2), k2.stride(0), _p(wq), _p(wk), _p(rope_cs), q2.shape[0], num_heads, s0, gf, gh, gw, eps,
                                                  round_mode, q_out_scale, variant, _stream()),
        "rmsnorm_rope",
    )
    return q, k


def rmsnorm_rope_blocked(q, k, wq, wk, rope_cs, grid, num_heads, q_out, k_out, s0=0, eps=1e-6, round_mode=ROUND_FP32, q_out_scale=1.0):
    """x2v_rmsnorm_rope_blocked_bf16: RoPE3D(RMSNorm(q|k)) written out of place into N-blocked buffers q_out / k_out [B, S, H*128/B]
    (the Ulysses seq->head send buffers)."""
    q2, k2 = _row2d(_bf16(q, "q"), "q"), _row2d(_bf16(k, "k"), "k")
    if rope_cs.dtype != torch.float32 or tuple(rope_cs.shape) != (1024, 64, 2) or not rope_cs.is_contiguous():
        raise X2VError("rope_cs must be a contiguous float32 [1024,64,2] (cos,sin) table")
    cb, cbs, ldo = _blocks3d(_bf16(q_out, "q_out"), "q_out")
    if tuple(k_out.shape) != tuple(q_out.shape) or k_out.stride() != q_out.stride() or k_out.dtype != torch.bfloat16 or not k_out.is_cuda:
        raise X2VError("rmsnorm_rope_blocked: q_out and k_out must have the same shape, strides and dtype")
    if q_out.shape[0] * cb != num_heads * 128 or q_out.shape[1] != q2.shape[0]:
        raise X2VError(f"rmsnorm_rope_blocked: outputs {tuple(q_out.shape)} do not hold [{q2.shape[0]}, {num_heads * 128}]")
    gf, gh, gw = grid
    wq, wk = _vec(wq, "norm_q weight", q2.shape[1]), _vec(wk, "norm_k weight", k2.shape[1])
    init()
    if q2.shape[0] == 0:
        return q_out, k_out
    _check(
        _lib.x2v_rmsnorm_rope_blocked_bf16(_p(q2), q2.stride(0), _p(k2), k2.stride(0), _p(wq), _p(wk), _p(rope_cs), _p(q_out), _p(k_out), ldo, cb, cbs, q2.shape[0], num_heads, s0, gf,
                                           gh, gw, eps, round_mode, q_out_scale, _stream()),
        "rmsnorm_rope_blocked",
    )
    return q_out, k_out


def gate_residual_(x, y, gate=None):
    x2, y2 = _row2d(_bf16(x, "x"), "x"), _row2d(_bf16(y, "y"), "y")
    gate = _vec(gate, "gate", x2.shape[1])
    init()
    if x2.shape[0] == 0:
        return x
    _check(_lib.x2v_gate_residual_bf16(_p(x2), x2.stride(0), _p(y2), y2.stride(0), _p(gate), x2.shape[0], x2.shape[1], _stream()), "gate_residual")
    return x


def activation(x, act):
    xc = _bf16(x, "x").contiguous()
    out = torch.empty_like(xc)
    init()
    _check(_lib.x2v_activation_bf16(_p(xc), _p(out), xc.numel(), act, _stream()), "activation")
    return out


def _blocks3d(t, name):
    """A block-strided operand [B, M, c] (unit inner stride): returns (block columns, block stride, row stride)."""
    if t.dim() != 3 or t.stride(2) != 1 or not t.is_cuda:
        raise X2VError(f"{name}: a blocked operand is a 3-D device tensor [blocks, rows, cols] with unit inner stride, got {tuple(t.shape)} / {t.stride()}")
    return t.shape[2], t.stride(0), t.stride(1)


def gemm_blocked(x, weight_nk, bias=None, epilogue=EPI_NONE, out=None):
    """x2v_gemm_bf16_blocked.  `x`: [M, K] or K-blocked [B, M, K/B]; `out`: None / [M, N] or N-blocked [B', M, N/B'] (preallocated) — the
    Ulysses exchange buffers read / written in place.  Returns `out`."""
    w2 = _row2d(_bf16(weight_nk, "weight"), "weight")
    N, K = w2.shape
    if x.dim() == 3:
        kb, kbs, ldx = _blocks3d(_bf16(x, "x"), "x")
        M = x.shape[1]
        if kb * x.shape[0] != K:
            raise X2VError(f"gemm_blocked: x blocks {tuple(x.shape)} do not make K={K}")
    else:
        x2 = _row2d(_bf16(x, "x"), "x")
        kb, kbs, ldx, M = 0, 0, x2.stride(0), x2.shape[0]
        if x2.shape[1] != K:
            raise X2VError(f"gemm_blocked: x [M,{x2.shape[1]}] vs weight [{N},{K}]")
    if out is None:
        out = torch.empty((M, N), dtype=torch.bfloat16, device=x.device)
    if out.dim() == 3:
        nb, nbs, ldy = _blocks3d(_bf16(out, "out"), "out")
        if nb * out.shape[0] != N or out.shape[1] != M:
            raise X2VError(f"gemm_blocked: out blocks {tuple(out.shape)} do not make [{M}, {N}]")
    else:
        o2 = _row2d(_bf16(out, "out"), "out")
        nb, nbs, ldy = 0, 0, o2.stride(0)
        if tuple(o2.shape) != (M, N):
            raise X2VError(f"gemm_blocked: out is {tuple(o2.shape)}, expected {(M, N)}")
    if epilogue == EPI_RESIDUAL:
        raise X2VError("gemm_blocked: use gemm(..., resid=) for the residual epilogue (x may be 3-D there)")
    bias = _vec(bias, "gemm bias", N)
    init()
    if M == 0:
        return out
    _check(_lib.x2v_gemm_bf16_blocked(_p(x), ldx, kb, kbs, _p(w2), w2.stride(0), _p(bias), _p(out), ldy, nb, nbs, M, N, K, epilogue, None, 0, None, _stream()), "gemm_bf16_blocked")
    return out


def _resid_period_out(who, resid, resid_period, out, M, N, x):
    """(out [M, N], resid [period, N]) of a residual epilogue with a row period: the output is a tensor of its own (never resid itself)."""
    r2 = _row2d(_bf16(resid, "resid"), "resid")
    if resid_period <= 0 or tuple(r2.shape) != (resid_period, N) or resid_period > M:
        raise X2VError(f"{who}: resid is {tuple(r2.shape)}, expected {(resid_period, N)} with 0 < resid_period <= M={M}")
    out2 = torch.empty((M, N), dtype=torch.bfloat16, device=x.device) if out is None else _row2d(out, "out")
    if _bf16(out2, "out").shape != (M, N):
        raise X2VError(f"{who}: out is {tuple(out2.shape)}, expected {(M, N)}")
    return out2, r2


def gemm(x, weight_nk, bias=None, epilogue=EPI_NONE, resid=None, gate=None, out=None, variant=0, resid_period=0):
    """y = epi(x @ weight_nk.T + bias); weight_nk is the checkpoint's [N,K] tensor.  variant: see x2v_gemm_bf16_variant.
    A 3-D `x` ([B, M, K/B], K-blocked) or 3-D `out` ([B, M, N/B], N-blocked) goes through x2v_gemm_bf16_blocked.
    resid_period > 0 (residual epilogue): `resid` is [resid_period, N] and output row r combines with its row r % resid_period
    (x2v_gemm_bf16_resid_period); the output is a new tensor unless `out` is given."""
    if resid_period:
        if epilogue != EPI_RESIDUAL or resid is None or x.dim() != 2 or (out is not None and out.dim() != 2):
            raise X2VError("gemm: resid_period needs the residual epilogue on row-major operands")
        x2, w2 = _row2d(_bf16(x, "x"), "x"), _row2d(_bf16(weight_nk, "weight"), "weight")
        (M, K), N = x2.shape, w2.shape[0]
        if w2.shape[1] != K:
            raise X2VError(f"gemm: x [M,{K}] vs weight [{N},{w2.shape[1]}]")
        out2, r2 = _resid_period_out("gemm", resid, resid_period, out, M, N, x)
        init()
        _check(_lib.x2v_gemm_bf16_resid_period(_p(x2), x2.stride(0), _p(w2), w2.stride(0), _p(_vec(bias, "gemm bias", N)), _p(out2), out2.stride(0), M, N, K, _p(r2), r2.stride(0),
                                               resid_period, _p(_vec(gate, "gemm gate", N)), variant, _stream()), "gemm_bf16_resid_period")
        return out2
    if x.dim() == 3 or (out is not None and out.dim() == 3):
        if epilogue != EPI_RESIDUAL:
            return gemm_blocked(x, weight_nk, bias, epilogue, out)
        # residual epilogue on a K-blocked x (the Ulysses output projection): y = resid, row-major
        w2 = _row2d(_bf16(weight_nk, "weight"), "weight")
        N, K = w2.shape
        kb, kbs, ldx = _blocks3d(_bf16(x, "x"), "x")
        M = x.shape[1]
        if kb * x.shape[0] != K or resid is None:
            raise X2VError(f"gemm: K-blocked x {tuple(x.shape)} vs weight [{N},{K}] (residual epilogue needs resid)")
        out2 = _row2d(_bf16(resid if out is None else out, "out"), "out")
        r2 = _row2d(_bf16(resid, "resid"), "resid")
        if tuple(out2.shape) != (M, N):
            raise X2VError(f"gemm: out is {tuple(out2.shape)}, expected {(M, N)}")
        init()
        if M == 0:
            return out2
        _check(_lib.x2v_gemm_bf16_blocked(_p(x), ldx, kb, kbs, _p(w2), w2.stride(0), _p(_vec(bias, "gemm bias", N)), _p(out2), out2.stride(0), 0, 0, M, N, K, epilogue, _p(r2),
                                          r2.stride(0), _p(_vec(gate, "gemm gate", N)), _stream()), "gemm_bf16_blocked")
        return out2
    x2, w2 = _row2d(_bf16(x, "x"), "x"), _row2d(_bf16(weight_nk, "weight"), "weight")
    M, K = x2.shape
    N = w2.shape[0]
    if w2.shape[1] != K:
        raise X2VError(f"gemm: x [M,{K}] vs weight [{N},{w2.shape[1]}]")
    if epilogue == EPI_RESIDUAL:
        if resid is None:
            raise X2VError("gemm: residual epilogue needs resid")
        out2 = _row2d(resid if out is None else out, "out")
        r2 = _row2d(_bf16(resid, "resid"), "resid")
        gate = _vec(gate, "gemm gate", N)
    else:
        out2 = torch.empty((M, N), dtype=torch.bfloat16, device=x.device) if out is None else _row2d(out, "out")
        r2 = None
    bias = _vec(bias, "gemm bias", N)
    if _bf16(out2, "out").shape != (M, N):
        raise X2VError(f"gemm: out is {tuple(out2.shape)}, expected {(M, N)}")
    init()
    if M == 0:
        return out2
    _check(
        _lib.x2v_gemm_bf16_variant(_p(x2), x2.stride(0), _p(w2), w2.stride(0), _p(bias), _p(out2), out2.stride(0), M, N, K, epilogue, _p(r2), 0 if r2 is None else r2.stride(0), _p(gate), variant, _stream()),
        "gemm_bf16",
    )
    return out2


def attention_batched(q, k, vt, num_heads, batch, rows_per_seq, seq_len, out=None, prescaled=False, scale=0.0, all_rows_query=True, one_launch=None, timed=None, stagger=False):
    """`batch` independent self-attentions over stacked rows (x2v_attn_fwd_bf16_vt_batched): q, k, out are [batch * rows_per_seq, H*128]
    row-major (any token stride), sequence b in rows [b * rows_per_seq, b * rows_per_seq + seq_len); vt = V^T [H, batch * rows_per_seq / 64,
    128, 64] over the stacked rows (gemm_vt / transpose_heads of the stacked v; rows_per_seq % 64 == 0).  Keys are the first seq_len rows of
    a sequence's slot; with all_rows_query (default) every row of the slot is a query, so every row of `out` is written (the padding rows
    of a stacked activation buffer stay finite), else only the first seq_len.
    one_launch: True = all sequences in one launch (grid z), False = one launch per sequence, None = by size — measured on MI355X: one
    launch wins when a sequence alone already fills the chip many times over (Wan-14B 720p, 11 840 workgroups each: -0.85 %), and loses
    when it does not (Wan-1.3B 480p, 960 workgroups each: +2 %, the two sequences' K/V share the L2s).  Same results either way.
    timed: optional callable(fn) that runs fn() — called once per kernel launch (bench.py's per-launch HIP-event timer).
    stagger: X2V_ATTN_VT_STAGGER (see x2v.h): same for every launch form here, since a row's query block index does not depend on it."""
    q2, k2 = _row2d(_bf16(q, "q"), "q"), _row2d(_bf16(k, "k"), "k")
    rows = batch * rows_per_seq
    if rows_per_seq % 64 or not 0 < seq_len <= rows_per_seq or q2.shape[0] != rows or k2.shape[0] != rows or min(q2.shape[1], k2.shape[1]) < num_heads * 128:
        raise X2VError(f"attention_batched: q {tuple(q2.shape)} k {tuple(k2.shape)} do not hold {batch} sequences of {rows_per_seq} (multiple of 64) rows x {num_heads} heads")
    _vt_operand(vt, "attention_batched", num_heads, rows)  # over the stacked rows
    out2 = _attn_out(out, "attention_batched", rows, num_heads * 128, q.device)
    init()
    sq = rows_per_seq if all_rows_query else seq_len
    if one_launch is None:
        one_launch = ((sq + 255) // 256) * num_heads >= 4096
    qb, kb, ob, vb = rows_per_seq * q2.stride(0), rows_per_seq * k2.stride(0), rows_per_seq * out2.stride(0), rows_per_seq * 128
    for b0, nb in ([(0, batch)] if one_launch else [(b, 1) for b in range(batch)]):
        def launch(b0=b0, nb=nb):
            _check(_lib.x2v_attn_fwd_bf16_vt_batched(q2.data_ptr() + 2 * b0 * qb, q2.stride(0), qb, k2.data_ptr() + 2 * b0 * kb, k2.stride(0), kb, vt.data_ptr() + 2 * b0 * vb, rows,
                                                     vb, out2.data_ptr() + 2 * b0 * ob, out2.stride(0), ob, sq, seq_len, num_heads, nb, 128, scale, int(bool(prescaled)) | (2 if stagger else 0), _stream()),
                   "attn_fwd_vt_batched")

        timed(launch) if timed is not None else launch()
    return out2


def gemm_vt(x, weight_nk, bias, num_heads):
    """V^T [H, ceil(M/64), 128, 64] of v = x @ weight_nk.T + bias (what transpose_heads(gemm(...)) returns, same bits): one kernel when the
    shape takes the single-stream 256x256 GEMM (x2v_gemm_bf16_vt), the two-kernel sequence otherwise."""
    x2, w2 = _row2d(_bf16(x, "x"), "x"), _row2d(_bf16(weight_nk, "weight"), "weight")
    M, K = x2.shape
    N = w2.shape[0]
    if w2.shape[1] != K or N != num_heads * 128:
        raise X2VError(f"gemm_vt: x [M,{K}] vs weight [{N},{w2.shape[1]}] for {num_heads} heads of 128")
    init()
    if M == 0 or (_lib.x2v_gemm_kernel_choice(M, N, K, x2.stride(0), w2.stride(0), 0) & 0xff) != 3:
        return transpose_heads(gemm(x2, w2, bias), num_heads)
    ldvt = (M + 63) // 64 * 64
    vt = torch.empty((num_heads, ldvt // 64, 128, 64), dtype=torch.bfloat16, device=x.device)
    _check(_lib.x2v_gemm_bf16_vt(_p(x2), x2.stride(0), _p(w2), w2.stride(0), _p(_vec(bias, "gemm bias", N)), _p(vt), ldvt, M, N, K, _stream()), "gemm_bf16_vt")
    return vt


def gemm_kernel_choice(M, N, K, ldx=None, ldw=None, fp8=False, with_form=False):
    """Tile family variant 0 launches for this shape (x2v_gemm_kernel_choice): 1 = 128x128 kernel, 2 = the 256x256 fp8 kernels, 3 = the 256x256
    single-stream kernel (bf16).  with_form: (family, continuous) — continuous = the continuous-pipeline form (gemm256c / gemm256c8) runs for a
    row-major y, else one tile per workgroup / ping-pong (same bits)."""
    rc = _lib.x2v_gemm_kernel_choice(M, N, K, K if ldx is None else ldx, K if ldw is None else ldw, int(fp8))
    if rc < 0:
        raise X2VError(f"gemm_kernel_choice: bad shape M={M} N={N} K={K}")
    return (rc & 0xff, bool(rc & 0x100)) if with_form else rc & 0xff


def attn_vt_launch_plan(Sq, Sk, num_heads, batch=1, stagger=False, one_walk=False, with_short=False):
    """(xcd_remap, staggered_walk) that x2v_attn_fwd_bf16_vt(_batched) takes for this shape (x2v_attn_vt_launch_plan; host-only);
    with_short: (xcd_remap, staggered_walk, persistent_short_walk)."""
    rc = _lib.x2v_attn_vt_launch_plan(Sq, Sk, num_heads, batch, (2 if stagger else 0) | (4 if one_walk else 0))
    if rc < 0:
        raise X2VError(f"attn_vt_launch_plan: bad shape Sq={Sq} Sk={Sk} H={num_heads} B={batch}")
    return (bool(rc & 1), bool(rc & 0x100), bool(rc & 0x200)) if with_short else (bool(rc & 1), bool(rc & 0x100))


def mfma_probe(milliseconds=1500):
    """TFLOP/s this board sustains on bare 16x16x32 bf16 MFMAs right now (x2v_mfma_probe_bf16): the box calibration bench.py prints."""
    init()
    out = _f32(0.0)
    _check(_lib.x2v_mfma_probe_bf16(int(milliseconds), ctypes.byref(out), _stream()), "mfma_probe")
    return float(out.value)


def transpose_heads(v, num_heads):
    """v [Sk, H*128] (any token stride) → V^T [H, ceil(Sk/64), 128, 64] (per head and 64-key tile a contiguous [dv][key] block)
    with the key padding zero-filled: the operand of the pre-transposed-V attention kernel."""
    v2 = _row2d(_bf16(v, "v"), "v")
    Sk = v2.shape[0]
    ldvt = (Sk + 63) // 64 * 64
    vt = torch.empty((num_heads, ldvt // 64, 128, 64), dtype=torch.bfloat16, device=v.device)
    init()
    _check(_lib.x2v_transpose_heads_bf16(_p(v2), v2.stride(0), _p(vt), ldvt, Sk, num_heads, _stream()), "transpose_heads")
    return vt


def attention(q, k, v, num_heads, head_dim=128, scale=0.0, out=None, variant=0, vt=None):
    """q [Sq, H*d] (or [Sq,H,d]), k/v [Sk, H*d]; any token stride (fused-QKV views are fine).
    variant ATTN_FAST runs on V^T: pass `vt` (transpose_heads(v, H)) or let this call transpose v."""

    def as2d(t, name):
        if t.dim() == 3:
            if t.stride(2) != 1 or t.stride(1) != t.shape[2]:
                raise X2VError(f"attention: {name} heads must be packed (stride {t.stride()})")
            t = t.as_strided((t.shape[0], t.shape[1] * t.shape[2]), (t.stride(0), 1))
        return _row2d(_bf16(t, name), name)

    if v is None:  # V^T only (gemm_vt): the pre-transposed-V kernel never reads row-major v
        if vt is None or (variant & 0xFF) != ATTN_FAST:
            raise X2VError("attention: v may be omitted only together with vt= and variant ATTN_FAST")
        v = k
    q2, k2, v2 = as2d(q, "q"), as2d(k, "k"), as2d(v, "v")
    Sq, Sk = q2.shape[0], k2.shape[0]
    out2 = _attn_out(out, "attention", Sq, num_heads * head_dim, q.device)
    if v2.shape[0] != Sk or min(q2.shape[1], k2.shape[1], v2.shape[1]) < num_heads * head_dim:
        raise X2VError(f"attention: q {tuple(q2.shape)} k {tuple(k2.shape)} v {tuple(v2.shape)} do not describe {num_heads} heads of {head_dim}")
    if Sk == 0:
        raise X2VError("attention: no keys (softmax over an empty set)")
    init()
    if Sq == 0:
        return out2
    if (variant & 0xFF) == ATTN_FAST:
        vt = transpose_heads(v2, num_heads) if vt is None else _vt_operand(vt, "attention", num_heads, Sk)
        _check(
            _lib.x2v_attn_fwd_bf16_vt(_p(q2), q2.stride(0), _p(k2), k2.stride(0), _p(vt), vt.shape[1] * 64, _p(out2), out2.stride(0), Sq, Sk, num_heads, head_dim, scale,
                                      (1 if (variant & ATTN_Q_PRESCALED) else 0) | (2 if (variant & ATTN_STAGGER) else 0) | (4 if (variant & ATTN_ONE_WALK) else 0), _stream()),
            "attn_fwd_vt",
        )
        return out2
    _check(
        _lib.x2v_attn_fwd_bf16_variant(_p(q2), q2.stride(0), _p(k2), k2.stride(0), _p(v2), v2.stride(0), _p(out2), out2.stride(0), Sq, Sk, num_heads, head_dim, scale, variant, _stream()),
        "attn_fwd",
    )
    return out2


def _vt_cache(vt, who, num_heads=None):  # a V^T cache [H, tiles, 128, 64]: more tiles than the keys in use, appended to in place
    if vt.dim() != 4 or vt.dtype != torch.bfloat16 or not vt.is_cuda or not vt.is_contiguous() or tuple(vt.shape[2:]) != (128, 64) or (num_heads is not None and vt.shape[0] != num_heads):
        raise X2VError(f"{who}: the V^T cache must be a contiguous bf16 [H, tiles, 128, 64] tensor on the GPU, got {vt.dtype} {tuple(vt.shape)} on {vt.device}")
    return vt


def transpose_heads_append(v, vt, key0):
    """x2v_transpose_heads_append_bf16: v [S, H*128] (any token stride) into the key columns [key0, key0 + S) of the V^T cache vt [H, tiles, 128, 64],
    a bit copy that changes no other byte of vt (key0 and S need not be multiples of the 64-key tile, nor even).  Appends to one cache and the
    attention over it are ordered on one stream.  Returns vt."""
    v2 = _row2d(_bf16(v, "v"), "v")
    vt = _vt_cache(vt, "transpose_heads_append")
    H, S = vt.shape[0], v2.shape[0]
    if v2.shape[1] < H * 128:
        raise X2VError(f"transpose_heads_append: v {tuple(v2.shape)} does not hold {H} heads of 128")
    init()
    if S == 0:  # torch hands out a null data_ptr for an empty tensor; the C entry would call it a null pointer
        if key0 < 0 or key0 > vt.shape[1] * 64:
            raise X2VError(f"transpose_heads_append: key0={key0} outside the cache's {vt.shape[1] * 64} keys")
        return vt
    _check(_lib.x2v_transpose_heads_append_bf16(_p(v2), v2.stride(0), _p(vt), vt.shape[1] * 64, key0, S, H, _stream()), "transpose_heads_append")
    return vt


def attention_cached(q, k_cache, vt_cache, kv_end, num_heads, out=None, prescaled=False, scale=0.0):
    """Attention of q [Sq, H*128] over the first kv_end keys of a KV cache: k_cache [capacity, H*128] row-major, vt_cache [H, tiles, 128, 64] as
    transpose_heads_append fills it (tiles * 64 >= kv_end) — x2v_attn_fwd_bf16_vt on k_cache[:kv_end] with ldvt = tiles * 64, one-walk or
    short-walk form by the shape as for lib.attention; flags: X2V_ATTN_VT_PRESCALED when `prescaled`, nothing else.
    The kernel gives a key >= kv_end of the last tile probability 0 and still multiplies it with the V^T entry there, so the cache's bytes at keys
    >= kv_end must be FINITE (0 * inf = nan): causvid.KVCache zero-fills its tensors once and nothing but transpose_heads_append writes them."""
    q2, k2 = _row2d(_bf16(q, "q"), "q"), _row2d(_bf16(k_cache, "k_cache"), "k_cache")
    vt = _vt_cache(vt_cache, "attention_cached", num_heads)
    Sq, W = q2.shape[0], num_heads * 128
    if min(q2.shape[1], k2.shape[1]) < W:
        raise X2VError(f"attention_cached: q {tuple(q2.shape)} k_cache {tuple(k2.shape)} do not describe {num_heads} heads of 128")
    if kv_end < 1 or kv_end > k2.shape[0] or kv_end > vt.shape[1] * 64:
        raise X2VError(f"attention_cached: kv_end={kv_end} outside the cache (k_cache holds {k2.shape[0]} keys, vt_cache {vt.shape[1] * 64})")
    out2 = _attn_out(out, "attention_cached", Sq, W, q.device)
    init()
    if Sq == 0:
        return out2
    _check(
        _lib.x2v_attn_fwd_bf16_vt(_p(q2), q2.stride(0), _p(k2), k2.stride(0), _p(vt), vt.shape[1] * 64, _p(out2), out2.stride(0), Sq, kv_end, num_heads, 128, scale,
                                  1 if prescaled else 0, _stream()),
        "attention_cached",
    )
    return out2


ATTN_CARRY_IN = 8  # x2v.h X2V_ATTN_CARRY_IN: the launch continues from the state in acc / lse
ATTN_CARRY_OUT = 16  # x2v.h X2V_ATTN_CARRY_OUT: the launch leaves its state in acc / lse and does not write o


class AttnCarryState:
    """The running softmax state of a chain of attention_carry launches over key chunks: `acc` fp32 [Sq, >= H*128] (the output so far; any
    16-byte-aligned row stride) and `lse` fp32 [H, >= Sq] (its base-2 log-sum-exp), plus how many launches have left their result in it.
    `AttnCarryState.alloc` makes one for a shape; a chain owns it until its last launch has written the bf16 output."""

    def __init__(self, acc, lse, steps=0):
        if acc.dtype != torch.float32 or lse.dtype != torch.float32 or acc.dim() != 2 or lse.dim() != 2 or acc.stride(1) != 1 or lse.stride(1) != 1:
            raise X2VError(f"AttnCarryState: acc / lse are 2-D float32 tensors with unit inner stride, got {acc.dtype} {tuple(acc.shape)} / {lse.dtype} {tuple(lse.shape)}")
        if not (acc.is_cuda and lse.is_cuda):
            raise X2VError("AttnCarryState: tensors are not on a HIP device; the x2v HIP path has no CPU fallback")
        self.acc, self.lse, self.steps = acc, lse, steps

    @classmethod
    def alloc(cls, rows, num_heads, device):
        return cls(torch.empty((rows, num_heads * 128), dtype=torch.float32, device=device), torch.empty((num_heads, rows), dtype=torch.float32, device=device))

    def reset(self):
        self.steps = 0
        return self


def attention_carry(q, k, vt, num_heads, state=None, last=False, prescaled=False, out=None, scale=0.0):
    """One launch of a chain over key chunks (x2v_attn_fwd_bf16_vt_carry): q [Sq, H*128], this chunk's k [Sk, H*128] (any token stride) and its
    V^T (transpose_heads over the chunk's Sk rows).  `state`: None or a fresh AttnCarryState (steps == 0) starts a chain, one that earlier launches
    wrote (steps > 0) continues it.  Not `last`: the launch leaves the state behind (allocated here when None) and returns it; `last`: it writes the
    chain's bf16 result (one rounding of the fp32 state) into `out` / a new tensor and returns that — the state is then spent (steps back to 0).
    A chain of one launch (no state, last) is the dense one-walk launch: same bits as attention(..., ATTN_FAST | ATTN_ONE_WALK)."""
    q2, k2 = _row2d(_bf16(q, "q"), "q"), _row2d(_bf16(k, "k"), "k")
    Sq, Sk = q2.shape[0], k2.shape[0]
    if min(q2.shape[1], k2.shape[1]) < num_heads * 128:
        raise X2VError(f"attention_carry: q {tuple(q2.shape)} k {tuple(k2.shape)} do not describe {num_heads} heads of 128")
    if Sk == 0:
        raise X2VError("attention_carry: no keys (softmax over an empty set)")
    _vt_operand(vt, "attention_carry", num_heads, Sk)
    flags = int(bool(prescaled))
    if state is not None and state.steps > 0:
        flags |= ATTN_CARRY_IN
    if not last:
        flags |= ATTN_CARRY_OUT
        if state is None:
            state = AttnCarryState.alloc(Sq, num_heads, q.device)
    if state is not None and (state.acc.shape[0] != Sq or state.acc.shape[1] < num_heads * 128 or state.lse.shape[0] != num_heads or state.lse.shape[1] < Sq):
        raise X2VError(f"attention_carry: the state (acc {tuple(state.acc.shape)}, lse {tuple(state.lse.shape)}) was not made for {Sq} rows x {num_heads} heads")
    out2 = _attn_out(out, "attention_carry", Sq, num_heads * 128, q.device) if last else None
    init()
    if Sq > 0:
        carry = flags & (ATTN_CARRY_IN | ATTN_CARRY_OUT)
        acc, lse = (state.acc, state.lse) if carry else (None, None)
        _check(
            _lib.x2v_attn_fwd_bf16_vt_carry(_p(q2), q2.stride(0), _p(k2), k2.stride(0), _p(vt), vt.shape[1] * 64, _p(out2), 0 if out2 is None else out2.stride(0), _p(acc),
                                            0 if acc is None else acc.stride(0), _p(lse), 0 if lse is None else lse.stride(0), Sq, Sk, num_heads, 128, scale, flags, _stream()),
            "attn_fwd_vt_carry",
        )
    if last:
        if state is not None:
            state.steps = 0
        return out2
    state.steps += 1
    return state


def attention_lse(q, k, v, num_heads, vt=None, prescaled=False, scale=0.0):
    """Attention with its log-sum-exp, as flash-attention callers expect it: (out bf16 [Sq, H*128], lse fp32 [H, Sq]) with
    lse[h, r] = ln sum_j exp(scale * q_r . k_j) in natural-log units.  One CARRY_OUT launch (x2v.h): the kernel works in base 2 on scores
    that carry scale * log2(e), so its value L2 = log2 sum_j 2^(scale * log2(e) * q_r . k_j) and lse = L2 * ln 2; `out` is the fp32 state rounded
    to bf16 once (round to nearest even, what the kernel's own bf16 store does).  v may be None when `vt` is given."""
    if vt is None:
        vt = transpose_heads(v, num_heads)
    state = attention_carry(q, k, vt, num_heads, prescaled=prescaled, scale=scale)
    return state.acc.to(torch.bfloat16), state.lse * math.log(2.0)


class AttnBlockPlan:
    """What x2v_attn_bsr_fwd_bf16_vt walks for one sequence length: `table` (host, uint32) = ceil(S / 256) records {256-row query block, first entry,
    entries}, the longest walk first, then the entries (64-key tile << 2) | bit 0: the block's rows 0-127 attend the tile | bit 1: its rows 128-255
    do.  Tiles of a record ascend, so the tile that may hold fewer than 64 keys (the last of the sequence) ends its record, and tiles at or beyond
    ceil(S / 64) never appear.  `device_table(device)` uploads it once per device."""

    def __init__(self, table, seq_len, n_wgs, kept_blocks, union_tiles):
        self.table, self.seq_len, self.n_wgs, self.kept_blocks, self.union_tiles = table, seq_len, n_wgs, kept_blocks, union_tiles
        self._dev = {}

    def device_table(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = torch.from_numpy(self.table.view("int32")).to(device)
        return self._dev[key]

    def records(self):
        """[(query block, [(tile, member bits), ..]), ..] in launch order (host-side reading of the table: tests, tools)."""
        t = self.table
        return [(int(t[3 * w]), [(int(e) >> 2, int(e) & 3) for e in t[int(t[3 * w + 1]) : int(t[3 * w + 1]) + int(t[3 * w + 2])]]) for w in range(self.n_wgs)]


def attn_block_plan(mask_or_csr, Sq, Sk):
    """The launch plan of attention_block_sparse for a static block mask: `mask_or_csr` is the bool [ceil(Sq/128), ceil(Sk/128)] block mask (tensor or
    array), or CSR (indptr, indices) over 128-row x 128-key blocks — what the reference hands to its block-sparse wrapper (radial_attn.py:34-46,
    R = C = 128).  Host-only (no GPU).  Raises X2VError for Sq != Sk, dimensions that are not ceil(S/128) on both sides, a block row with no
    entry (softmax over nothing), and CSR indices out of range, unsorted or duplicated."""
    import numpy as np

    Sq, Sk = int(Sq), int(Sk)
    if Sq != Sk or Sq <= 0:
        raise X2VError(f"attn_block_plan: self-attention only (Sq={Sq}, Sk={Sk})")
    nb, ntile = (Sq + 127) // 128, (Sq + 63) // 64
    if isinstance(mask_or_csr, (tuple, list)) and len(mask_or_csr) == 2:
        indptr, indices = (np.asarray(a.cpu() if isinstance(a, torch.Tensor) else a).astype(np.int64).reshape(-1) for a in mask_or_csr)
        if indptr.shape[0] != nb + 1:
            raise X2VError(f"attn_block_plan: indptr has {indptr.shape[0]} entries, {nb} block rows need {nb + 1}")
        if indptr[0] != 0 or indptr[-1] != indices.shape[0] or np.any(np.diff(indptr) < 0):
            raise X2VError("attn_block_plan: indptr must start at 0, not decrease, and end at len(indices)")
        if indices.size and (indices.min() < 0 or indices.max() >= nb):
            raise X2VError(f"attn_block_plan: block index out of range [0, {nb})")
        rows = np.repeat(np.arange(nb), np.diff(indptr))
        same_row = rows[1:] == rows[:-1]
        if np.any(same_row & (np.diff(indices) <= 0)):
            raise X2VError("attn_block_plan: the block indices of a row must ascend strictly (unsorted or duplicated entry)")
        mask = np.zeros((nb, nb), dtype=bool)
        mask[rows, indices] = True
    else:
        mask = np.asarray(mask_or_csr.cpu() if isinstance(mask_or_csr, torch.Tensor) else mask_or_csr)
        if mask.dtype != np.bool_ or mask.shape != (nb, nb):
            raise X2VError(f"attn_block_plan: the mask must be bool [{nb}, {nb}] for {Sq} rows, got {mask.dtype} {tuple(mask.shape)}")
    empty = np.flatnonzero(~mask.any(axis=1))
    if empty.size:
        raise X2VError(f"attn_block_plan: block row {int(empty[0])} attends no block (softmax over nothing)")
    n_wgs = (nb + 1) // 2
    pair = np.zeros((2 * n_wgs, nb), dtype=np.uint32)
    pair[:nb] = mask
    bits = pair[0::2] | (pair[1::2] << 1)  # [n_wgs, nb]: member bits per key block
    tile_bits = np.repeat(bits, 2, axis=1)[:, :ntile]  # key block b = tiles 2b, 2b + 1
    counts = (tile_bits != 0).sum(axis=1)
    order = np.argsort(-counts, kind="stable")  # heaviest walk first: the grid's tail is made of the short ones
    wg, tile = np.nonzero(tile_bits[order])  # row-major: a record's tiles ascend
    entries = (tile.astype(np.uint32) << 2) | tile_bits[order][wg, tile]
    starts = 3 * n_wgs + np.concatenate(([0], np.cumsum(counts[order])[:-1]))
    table = np.empty(3 * n_wgs + entries.shape[0], dtype=np.uint32)
    table[0 : 3 * n_wgs : 3] = order
    table[1 : 3 * n_wgs : 3] = starts
    table[2 : 3 * n_wgs : 3] = counts[order]
    table[3 * n_wgs :] = entries
    return AttnBlockPlan(table, Sq, n_wgs, int(mask.sum()), int(counts.sum()))


def attention_block_sparse(q, k, vt, num_heads, plan, prescaled=False, out=None, scale=0.0):
    """Self-attention restricted to the 128 x 128 blocks of `plan` (attn_block_plan) — x2v_attn_bsr_fwd_bf16_vt.  q, k [S, H*128] (any token stride),
    vt = transpose_heads(v, H) / gemm_vt's V^T [H, ceil(S/64), 128, 64]; prescaled: q already carries scale * log2(e).  Returns out [S, H*128]."""
    if not isinstance(plan, AttnBlockPlan):
        raise X2VError("attention_block_sparse: plan must come from attn_block_plan")
    q2, k2 = _row2d(_bf16(q, "q"), "q"), _row2d(_bf16(k, "k"), "k")
    S = q2.shape[0]
    out2 = _attn_out(out, "attention_block_sparse", S, num_heads * 128, q.device)
    if k2.shape[0] != S or min(q2.shape[1], k2.shape[1]) < num_heads * 128:
        raise X2VError(f"attention_block_sparse: q {tuple(q2.shape)} k {tuple(k2.shape)} do not describe one sequence of {num_heads} heads of 128")
    _vt_operand(vt, "attention_block_sparse", num_heads, S)
    init()
    tab = plan.device_table(q2.device)
    _check(
        _lib.x2v_attn_bsr_fwd_bf16_vt(_p(q2), q2.stride(0), _p(k2), k2.stride(0), _p(vt), vt.shape[1] * 64, _p(out2), out2.stride(0), S, k2.shape[0], num_heads, 128, scale,
                                      1 if prescaled else 0, _p(tab), tab.numel(), plan.seq_len, plan.n_wgs, _stream()),
        "attn_bsr_fwd",
    )
    return out2


def attention_mx_sizes(Sq, Sk, num_heads):
    """Bytes of (q codes, q scales, k codes, k scales, V^T codes, V^T scales, kmean buffer) for one sequence — x2v_attn_mx_sizes (host-only)."""
    sizes = (_i64 * 7)()
    rc = _lib.x2v_attn_mx_sizes(Sq, Sk, num_heads, sizes)
    if rc != 0:
        raise X2VError(f"attention_mx_sizes failed ({rc}): {_lib.x2v_last_error().decode()}")
    return tuple(int(s) for s in sizes)


class AttnMxOperands:
    """The quantised operands of attention_mx for one sequence (layouts: include/x2v.h): q_codes [H, Sq, 128], q_scales [H, Sq, 4], k_codes
    [H, Sk_pad, 128], k_scales [H, Sk_pad, 4], vt_codes [H, NT, 128 dv, 128 keys], vt_scales [H, NT, 128 dv, 4], all uint8; kmean fp32 [H*128]
    (None without smoothing), a view of kmean_buf, which also keeps the chunk sums of the two-pass reduction."""

    def __init__(self, Sq, Sk, H, q_codes, q_scales, k_codes, k_scales, vt_codes, vt_scales, kmean, kmean_buf):
        self.Sq, self.Sk, self.H = Sq, Sk, H
        self.q_codes, self.q_scales, self.k_codes, self.k_scales, self.vt_codes, self.vt_scales = q_codes, q_scales, k_codes, k_scales, vt_codes, vt_scales
        self.kmean, self.kmean_buf = kmean, kmean_buf


def attention_mx_prepare(q, k, v, num_heads, prescaled=False, smooth_k=True, scale=0.0):
    """The three preparation steps of attention_mx: the fp32 column mean of k (x2v_attn_mx_kmean_f32, when smooth_k), MXFP8 q and k - kmean along the
    head dimension (x2v_attn_mx_quant_qk; q is multiplied by scale * log2(e) in fp32 unless `prescaled` says it carries it already) and MXFP8 V^T
    along the keys (x2v_attn_mx_quant_vt).  q [Sq, H*128], k, v [Sk, H*128] bf16, any token stride that is a multiple of 8.  Returns AttnMxOperands."""
    q2, k2, v2 = _row2d(_bf16(q, "q"), "q"), _row2d(_bf16(k, "k"), "k"), _row2d(_bf16(v, "v"), "v")
    H, Sq, Sk = int(num_heads), q2.shape[0], k2.shape[0]
    if H <= 0 or v2.shape[0] != Sk or min(q2.shape[1], k2.shape[1], v2.shape[1]) < H * 128:
        raise X2VError(f"attention_mx: q {tuple(q2.shape)} k {tuple(k2.shape)} v {tuple(v2.shape)} do not describe one sequence of {H} heads of 128")
    if Sk == 0:
        raise X2VError("attention_mx: no keys (softmax over an empty set)")
    attention_mx_sizes(Sq, Sk, H)  # the shape limits, before anything is allocated
    init()
    dev, u8 = q2.device, torch.uint8
    nt = (Sk + 127) // 128
    ops = AttnMxOperands(Sq, Sk, H, torch.empty((H, Sq, 128), dtype=u8, device=dev), torch.empty((H, Sq, 4), dtype=u8, device=dev),
                         torch.empty((H, nt * 128, 128), dtype=u8, device=dev), torch.empty((H, nt * 128, 4), dtype=u8, device=dev),
                         torch.empty((H, nt, 128, 128), dtype=u8, device=dev), torch.empty((H, nt, 128, 4), dtype=u8, device=dev), None, None)
    st = _stream()
    if smooth_k:
        ops.kmean_buf = torch.empty((1 + (Sk + 255) // 256, H * 128), dtype=torch.float32, device=dev)
        ops.kmean = ops.kmean_buf[0]
        _check(_lib.x2v_attn_mx_kmean_f32(_p(k2), k2.stride(0), _p(ops.kmean_buf), Sk, H, st), "attn_mx_kmean")
    if Sq > 0:
        qs = 1.0 if prescaled else (scale * 1.4426950408889634 if scale > 0 else ATTN_PRESCALE)  # handed over as the nearest fp32
        _check(_lib.x2v_attn_mx_quant_qk(_p(q2), q2.stride(0), None, 0, qs, _p(ops.q_codes), _p(ops.q_scales), Sq, Sq, H, st), "attn_mx_quant_qk (q)")
    _check(_lib.x2v_attn_mx_quant_qk(_p(k2), k2.stride(0), _p(ops.kmean), 1 if smooth_k else 0, 1.0, _p(ops.k_codes), _p(ops.k_scales), Sk, nt * 128, H, st),
           "attn_mx_quant_qk (k)")
    _check(_lib.x2v_attn_mx_quant_vt(_p(v2), v2.stride(0), _p(ops.vt_codes), _p(ops.vt_scales), Sk, H, st), "attn_mx_quant_vt")
    return ops


def attention_mx(q, k, v, num_heads, prescaled=False, smooth_k=True, scale=0.0, out=None, prepared=None):
    """Block-scaled fp8 self-attention of one sequence at head dim 128 (x2v_attn_mx_fwd; the contract is in include/x2v.h): q [Sq, H*128], k, v
    [Sk, H*128] bf16 -> out [Sq, H*128] bf16.  prepared: the AttnMxOperands of attention_mx_prepare for the same tensors (q, k, v are then not read)."""
    H = int(num_heads)
    ops = attention_mx_prepare(q, k, v, H, prescaled, smooth_k, scale) if prepared is None else prepared
    if not isinstance(ops, AttnMxOperands) or ops.H != H:
        raise X2VError("attention_mx: prepared must come from attention_mx_prepare with the same number of heads")
    Sq = ops.Sq
    out2 = _attn_out(out, "attention_mx", Sq, H * 128, ops.k_codes.device)
    init()
    if Sq == 0:
        return out2
    _check(_lib.x2v_attn_mx_fwd(_p(ops.q_codes), _p(ops.q_scales), _p(ops.k_codes), _p(ops.k_scales), _p(ops.vt_codes), _p(ops.vt_scales), _p(out2), out2.stride(0), Sq,
                                ops.Sk, H, _stream()), "attn_mx_fwd")
    return out2


# The two w8a8 code types: torch dtype of the codes, what the error messages call it, the tag in the wrappers' names, and the C entries.  The fp8 and
# int8 wrappers below are the same argument checks over these.
class _W8A8:
    def __init__(self, dtype, dtype_name, tag, quant_blocked, layernorm_quant, gemm_variant, gemm_resid_period, gemm_blocked):
        self.dtype, self.dtype_name, self.tag = dtype, dtype_name, tag
        self.quant_blocked, self.layernorm_quant = quant_blocked, layernorm_quant
        self.gemm_variant, self.gemm_resid_period, self.gemm_blocked = gemm_variant, gemm_resid_period, gemm_blocked


_FP8 = _W8A8(torch.float8_e4m3fn, "float8_e4m3fn (OCP; gfx950)", "fp8", _lib.x2v_quant_fp8_rowwise_blocked, _lib.x2v_layernorm_quant_fp8, _lib.x2v_gemm_fp8_variant,
             _lib.x2v_gemm_fp8_resid_period, _lib.x2v_gemm_fp8_blocked)
_INT8 = _W8A8(torch.int8, "int8", "int8", _lib.x2v_quant_int8_rowwise_blocked, _lib.x2v_layernorm_quant_int8, _lib.x2v_gemm_int8_variant,
              _lib.x2v_gemm_int8_resid_period, _lib.x2v_gemm_int8_blocked)


def _quant8_rowwise(x, kind):
    dtype, tag = kind.dtype, kind.tag
    if x.dim() == 3:
        kb, kbs, ldx = _blocks3d(_bf16(x, "x"), "x")
        M, K = x.shape[1], kb * x.shape[0]
        x2 = x
    else:
        x2 = _row2d(_bf16(x, "x"), "x")
        (M, K), kb, kbs, ldx = x2.shape, 0, 0, x2.stride(0)
    xq = torch.empty((M, K), dtype=dtype, device=x.device)
    s = torch.empty((M, 1), dtype=torch.float32, device=x.device)
    init()
    if M == 0:
        return xq, s
    _check(kind.quant_blocked(_p(x2), ldx, kb, kbs, _p(xq), xq.stride(0), _p(s), M, K, _stream()), f"quant_{tag}_rowwise")
    return xq, s


def quant_fp8_rowwise(x):
    """(e4m3 codes [M, K] row-major, fp32 scales [M, 1]) of a bf16 x [M, K] — or of a K-blocked x [B, M, K/B] (the Ulysses head->seq receive
    buffer; x2v_quant_fp8_rowwise_blocked: the codes come out row-major, the de-blocking rides in the quantisation pass)."""
    return _quant8_rowwise(x, _FP8)


def quant_int8_rowwise(x):
    """quant_fp8_rowwise for the int8 operator: (int8 codes [M, K] row-major, fp32 scales [M, 1] = amax / 127) — x2v_quant_int8_rowwise_blocked."""
    return _quant8_rowwise(x, _INT8)


def _layernorm_quant8(x, weight, bias, scale, shift, eps, kind):
    dtype, tag = kind.dtype, kind.tag
    x2 = _row2d(_bf16(x, "x"), "x")
    M, D = x2.shape
    if D <= 512:
        return _quant8_rowwise(layernorm(x2, weight, bias, scale, shift, eps), kind)
    if (scale is None) != (shift is None):
        raise X2VError(f"layernorm_quant_{tag}: scale and shift must be given together")
    weight, bias = _vec(weight, "layernorm weight", D), _vec(bias, "layernorm bias", D)
    scale, shift = _vec(scale, "layernorm scale", D), _vec(shift, "layernorm shift", D)
    xq = torch.empty((M, D), dtype=dtype, device=x.device)
    s = torch.empty((M, 1), dtype=torch.float32, device=x.device)
    init()
    if M == 0:
        return xq, s
    _check(kind.layernorm_quant(_p(x2), x2.stride(0), _p(weight), _p(bias), _p(scale), _p(shift), _p(xq), xq.stride(0), _p(s), M, D, eps, _stream()),
           f"layernorm_quant_{tag}")
    return xq, s


def layernorm_quant_fp8(x, weight=None, bias=None, scale=None, shift=None, eps=1e-6):
    """(e4m3 codes [M, D], fp32 scales [M, 1]) of LN(x)[*w+b][*(1+scale)+shift] — x2v_layernorm_quant_fp8, bit-identical to
    quant_fp8_rowwise(layernorm(...)).  Rows of <= 512 elements go through the two kernels."""
    return _layernorm_quant8(x, weight, bias, scale, shift, eps, _FP8)


def layernorm_quant_int8(x, weight=None, bias=None, scale=None, shift=None, eps=1e-6):
    """layernorm_quant_fp8 for the int8 operator — x2v_layernorm_quant_int8, bit-identical to quant_int8_rowwise(layernorm(...))."""
    return _layernorm_quant8(x, weight, bias, scale, shift, eps, _INT8)


def _quant_mx(bits, x):
    """quant_mxfp8 / quant_mxfp6 / quant_mxfp4: a row of K elements of `bits` bits is K * bits / 8 bytes (e4m3 bytes as torch's dtype, the packed codes as uint8)."""
    tag = f"quant_mxfp{bits}"
    x2 = _row2d(_bf16(x, "x"), "x")
    M, K = x2.shape
    q = torch.empty((M, K // 8 * bits), dtype=torch.float8_e4m3fn if bits == 8 else torch.uint8, device=x.device)
    sc = torch.empty((max(K // 128, 1), M, 4), dtype=torch.uint8, device=x.device)
    init()
    if M == 0:
        return q, sc
    _check(getattr(_lib, f"x2v_{tag}_bf16")(_p(x2), x2.stride(0), _p(q), q.stride(0), _p(sc), M, K, _stream()), tag)
    return q, sc


def quant_mxfp8(x):
    """bf16 [M, K] → (e4m3 [M, K], e8m0 scale bytes [K/128, M, 4]) — see include/x2v.h::x2v_quant_mxfp8_bf16.
    `mx_scales_rowmajor` turns the scale tensor into the logical [M, K/32] table."""
    return _quant_mx(8, x)


def quant_mxfp6(x):
    """bf16 [M, K] → (uint8 [M, 3K/4]: e3m2 codes, the dense little-endian 6-bit string, code j of a row at bits 6j .. 6j+5 of its bytes;
    e8m0 scale bytes [K/128, M, 4]) — see include/x2v.h::x2v_quant_mxfp6_bf16."""
    return _quant_mx(6, x)


def quant_mxfp4(x):
    """bf16 [M, K] → (uint8 [M, K/2]: e2m1 codes, two per byte, the dense little-endian nibble string, code j of a row at bits 4j .. 4j+3 of its
    bytes; e8m0 scale bytes [K/128, M, 4]) — see include/x2v.h::x2v_quant_mxfp4_bf16."""
    return _quant_mx(4, x)


def mx_scales_rowmajor(sc):
    """[K/128, rows, 4] (kernel layout) → logical [rows, K/32]."""
    return sc.permute(1, 0, 2).reshape(sc.shape[1], -1)


def mx_scales_tiled(sc_rm):
    """logical [rows, K/32] → [K/128, rows, 4] (kernel layout)."""
    rows, kb = sc_rm.shape
    return sc_rm.reshape(rows, kb // 4, 4).permute(1, 0, 2).contiguous()


_MX_PACKED = {6: "uint8 matrix of packed e3m2 codes [rows, 3K/4]", 4: "uint8 matrix of packed e2m1 codes [rows, K/2]"}


def _gemm_mx(tag, bits_a, bits_b, a, sa, b, sb, alpha, bias, out, variant, epilogue, resid, gate):
    """gemm_mxfp8, gemm_mxfp6_mxfp8 and gemm_mxfp4: one set of checks, the entries x2v_gemm_<tag>_variant / _epi.  bits_a, bits_b: the element width
    of each operand — 8: e4m3 bytes [rows, K]; 6: the packed uint8 [rows, 3K/4]; 4: the packed uint8 [rows, K/2] (K % 256 == 0)."""
    M = a.shape[0]
    K = a.shape[1] * 8 // bits_a
    N = b.shape[0]
    kmult = 256 if 4 in (bits_a, bits_b) else 128
    for t, name, bits in ((a, "a", bits_a), (b, "b", bits_b)):
        if t.dtype not in ((torch.float8_e4m3fn, torch.uint8) if bits == 8 else (torch.uint8,)) or not t.is_cuda or t.stride(1) != 1:
            raise X2VError(f"gemm_{tag}: {name} must be a CUDA " + (_MX_PACKED[bits] if bits != 8 else "e4m3 (or raw uint8) matrix") + " with unit inner stride")
    for t, name, rows in ((sa, "scales_a", M), (sb, "scales_b", N)):
        if t.element_size() != 1 or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != (K // 128, rows, 4):
            raise X2VError(f"gemm_{tag}: {name} must be the contiguous CUDA byte tensor [K/128, {rows}, 4] of quant_mxfp8, got {tuple(t.shape)}")
    if a.shape[1] * 8 % bits_a or b.shape[1] != K * bits_b // 8 or K % kmult:
        raise X2VError(f"gemm_{tag}: shapes a{tuple(a.shape)} b{tuple(b.shape)} do not agree (K % {kmult} == 0, a row holds {bits_a}K/8 bytes of a and {bits_b}K/8 of b)")
    if alpha is not None and (alpha.dtype != torch.float32 or not alpha.is_cuda):
        raise X2VError(f"gemm_{tag}: alpha must be a float32 CUDA tensor")
    if bias is not None:
        bias = _bf16(bias, "bias").reshape(-1)
        if bias.numel() != N:
            raise X2VError(f"gemm_{tag}: bias must have N elements")
    if epilogue != EPI_NONE:
        if epilogue == EPI_RESIDUAL:
            out2 = _row2d(resid if out is None else out, "out")
            r2 = _row2d(_bf16(resid, "resid"), "resid")
            gate = _vec(gate, f"gemm_{tag} gate", N)
        else:
            out2 = torch.empty((M, N), dtype=torch.bfloat16, device=a.device) if out is None else _row2d(out, "out")
            r2 = None
        init()
        _check(
            getattr(_lib, f"x2v_gemm_{tag}_epi")(_p(a), a.stride(0), _p(sa), _p(b), b.stride(0), _p(sb), _p(bias), _p(alpha), _p(out2), out2.stride(0), M, N, K, epilogue, _p(r2),
                                                0 if r2 is None else r2.stride(0), _p(gate), _stream()),
            f"gemm_{tag}_epi",
        )
        return out2
    out2 = torch.empty((M, N), dtype=torch.bfloat16, device=a.device) if out is None else _row2d(out, "out")
    init()
    _check(
        getattr(_lib, f"x2v_gemm_{tag}_variant")(_p(a), a.stride(0), _p(sa), _p(b), b.stride(0), _p(sb), _p(bias), _p(alpha), _p(out2), out2.stride(0), M, N, K, variant, _stream()),
        f"gemm_{tag}",
    )
    return out2


def gemm_mxfp8(a, sa, b, sb, alpha=None, bias=None, out=None, variant=0, epilogue=EPI_NONE, resid=None, gate=None):
    """alpha * deq(a)[M,K] @ deq(b)[N,K]^T + bias → bf16 [M,N]; scales uint8/e8m0 [K/128, rows, 4] as produced by quant_mxfp8;
    alpha: fp32 device tensor or None."""
    return _gemm_mx("mxfp8", 8, 8, a, sa, b, sb, alpha, bias, out, variant, epilogue, resid, gate)


def gemm_mxfp6_mxfp8(a, sa, b, sb, alpha=None, bias=None, out=None, variant=0, epilogue=EPI_NONE, resid=None, gate=None):
    """gemm_mxfp8 with b = the packed e3m2 codes uint8 [N, 3K/4] and scales of quant_mxfp6; a and sa from quant_mxfp8.  variant as gemm_mxfp8 — see
    include/x2v.h::x2v_gemm_mxfp6_mxfp8."""
    return _gemm_mx("mxfp6_mxfp8", 8, 6, a, sa, b, sb, alpha, bias, out, variant, epilogue, resid, gate)


def gemm_mxfp4(a, sa, b, sb, alpha=None, bias=None, out=None, variant=0, epilogue=EPI_NONE, resid=None, gate=None):
    """gemm_mxfp8 with both operands the packed e2m1 codes uint8 [rows, K/2] and scales of quant_mxfp4 (K % 256 == 0).  variant as gemm_mxfp8 — see
    include/x2v.h::x2v_gemm_mxfp4."""
    return _gemm_mx("mxfp4", 4, 4, a, sa, b, sb, alpha, bias, out, variant, epilogue, resid, gate)


def gemm_mx_kernel_choice(bits_a, bits_b, M, N, K, lda=None, ldb=None):
    """The body variant 0 of gemm_mxfp8 (bits 8, 8), gemm_mxfp6_mxfp8 (8, 6) or gemm_mxfp4 (4, 4) launches for this shape without a fused epilogue:
    1 = the 128x128 kernel, 2 = the 256x256 ping-pong kernel (x2v_gemm_mx_kernel_choice; host arithmetic).  lda, ldb in bytes, default: dense rows."""
    fmt = {(8, 8): 1, (8, 6): 2, (4, 4): 3}.get((bits_a, bits_b), 0)
    rc = _lib.x2v_gemm_mx_kernel_choice(fmt, M, N, K, K * bits_a // 8 if lda is None else lda, K * bits_b // 8 if ldb is None else ldb)
    if rc < 0:
        raise X2VError(f"gemm_mx_kernel_choice: bad format or shape ({bits_a}, {bits_b}) M={M} N={N} K={K}")
    return rc


def _gemm8(kind, xq, sx, wq_nk, sw, bias, epilogue, resid, gate, out, variant, resid_period):
    dtype, dtype_name, tag = kind.dtype, kind.dtype_name, kind.tag
    M, K = xq.shape
    N = wq_nk.shape[0]
    if xq.dtype != dtype or wq_nk.dtype != dtype:
        raise X2VError(f"gemm_{tag}: operands must be {dtype_name}")
    if resid_period:
        if epilogue != EPI_RESIDUAL or resid is None:
            raise X2VError(f"gemm_{tag}: resid_period needs the residual epilogue")
        out2, r2 = _resid_period_out(f"gemm_{tag}", resid, resid_period, out, M, N, xq)
        gate = _vec(gate, f"gemm_{tag} gate", N)
    elif epilogue == EPI_RESIDUAL:
        out2 = _row2d(resid if out is None else out, "out")
        r2 = _row2d(_bf16(resid, "resid"), "resid")
        gate = _vec(gate, f"gemm_{tag} gate", N)
    else:
        out2 = torch.empty((M, N), dtype=torch.bfloat16, device=xq.device) if out is None else _row2d(out, "out")
        r2 = None
    if wq_nk.shape[1] != K or not xq.is_cuda or not wq_nk.is_cuda or xq.stride(1) != 1 or wq_nk.stride(1) != 1:
        raise X2VError(f"gemm_{tag}: xq {tuple(xq.shape)} / wq {tuple(wq_nk.shape)} must be device matrices with unit inner stride and equal K")
    sw, sx = _vec(sw, f"gemm_{tag} weight scales", N, torch.float32), _vec(sx, f"gemm_{tag} activation scales", M, torch.float32)
    bias = _vec(bias, f"gemm_{tag} bias", N)
    init()
    if M == 0:
        return out2
    if resid_period:
        _check(kind.gemm_resid_period(_p(xq), xq.stride(0), _p(sx), _p(wq_nk), wq_nk.stride(0), _p(sw), _p(bias), _p(out2), out2.stride(0), M, N, K, _p(r2), r2.stride(0),
                                              resid_period, _p(gate), variant, _stream()), f"gemm_{tag}_resid_period")
        return out2
    _check(
        kind.gemm_variant(_p(xq), xq.stride(0), _p(sx), _p(wq_nk), wq_nk.stride(0), _p(sw), _p(bias), _p(out2), out2.stride(0), M, N, K, epilogue, _p(r2), 0 if r2 is None else r2.stride(0), _p(gate), variant, _stream()),
        f"gemm_{tag}",
    )
    return out2


def gemm_fp8(xq, sx, wq_nk, sw, bias=None, epilogue=EPI_NONE, resid=None, gate=None, out=None, variant=0, resid_period=0):
    """resid_period: as gemm() (x2v_gemm_fp8_resid_period)."""
    return _gemm8(_FP8, xq, sx, wq_nk, sw, bias, epilogue, resid, gate, out, variant, resid_period)


def gemm_int8(xq, sx, wq_nk, sw, bias=None, epilogue=EPI_NONE, resid=None, gate=None, out=None, variant=0, resid_period=0):
    """epi(float(xq . wq^T) * sx * sw + bias) -> bf16 on int8 codes with an exact int32 accumulator (x2v_gemm_int8_variant / _resid_period);
    arguments as gemm_fp8.  variant: 1 = the 128x128 kernel (every legal shape), 5 = the continuous 256x256 kernel (X2VError where the shape does not
    allow it), 0 = chosen by shape (gemm_int8_kernel_choice tells which); 2, 3, 4 are refused: there is no int8 ping-pong kernel."""
    return _gemm8(_INT8, xq, sx, wq_nk, sw, bias, epilogue, resid, gate, out, variant, resid_period)


def gemm_int8_kernel_choice(M, N, K, ldx=None, ldw=None, with_form=False):
    """gemm_kernel_choice for gemm_int8's variant 0 (x2v_gemm_int8_kernel_choice)."""
    rc = _lib.x2v_gemm_int8_kernel_choice(M, N, K, K if ldx is None else ldx, K if ldw is None else ldw)
    if rc < 0:
        raise X2VError(f"gemm_int8_kernel_choice: bad shape M={M} N={N} K={K}")
    return (rc & 0xff, bool(rc & 0x100)) if with_form else rc & 0xff


def _gemm8_blocked(kind, xq, sx, wq_nk, sw, bias, epilogue, out, resid, gate):
    dtype, tag = kind.dtype, kind.tag
    if wq_nk.dtype != dtype or xq.dtype != dtype or wq_nk.dim() != 2 or wq_nk.stride(1) != 1 or not wq_nk.is_cuda or not xq.is_cuda:
        raise X2VError(f"gemm_{tag}_blocked: operands must be {str(dtype).removeprefix('torch.')} device tensors (weight [N, K] with unit inner stride)")
    N, K = wq_nk.shape
    if xq.dim() == 3:
        kb, kbs, ldx = _blocks3d(xq, "xq")
        M = xq.shape[1]
        if kb * xq.shape[0] != K:
            raise X2VError(f"gemm_{tag}_blocked: xq blocks {tuple(xq.shape)} do not make K={K}")
    else:
        if xq.dim() != 2 or xq.stride(1) != 1 or xq.shape[1] != K:
            raise X2VError(f"gemm_{tag}_blocked: xq {tuple(xq.shape)} vs weight [{N},{K}]")
        kb, kbs, ldx, M = 0, 0, xq.stride(0), xq.shape[0]
    r2 = None
    if epilogue == EPI_RESIDUAL:
        if resid is None:
            raise X2VError(f"gemm_{tag}_blocked: residual epilogue needs resid")
        r2 = _row2d(_bf16(resid, "resid"), "resid")
        out = resid if out is None else out
        gate = _vec(gate, f"gemm_{tag}_blocked gate", N)
    if out is None:
        out = torch.empty((M, N), dtype=torch.bfloat16, device=xq.device)
    if out.dim() == 3:
        nb, nbs, ldy = _blocks3d(_bf16(out, "out"), "out")
        if nb * out.shape[0] != N or out.shape[1] != M:
            raise X2VError(f"gemm_{tag}_blocked: out blocks {tuple(out.shape)} do not make [{M}, {N}]")
    else:
        o2 = _row2d(_bf16(out, "out"), "out")
        nb, nbs, ldy = 0, 0, o2.stride(0)
        if tuple(o2.shape) != (M, N):
            raise X2VError(f"gemm_{tag}_blocked: out is {tuple(o2.shape)}, expected {(M, N)}")
    sw, sx = _vec(sw, f"gemm_{tag}_blocked weight scales", N, torch.float32), _vec(sx, f"gemm_{tag}_blocked activation scales", M, torch.float32)
    bias = _vec(bias, f"gemm_{tag}_blocked bias", N)
    init()
    if M == 0:
        return out
    _check(
        kind.gemm_blocked(_p(xq), ldx, kb, kbs, _p(sx), _p(wq_nk), wq_nk.stride(0), _p(sw), _p(bias), _p(out), ldy, nb, nbs, M, N, K, epilogue, _p(r2),
                                  0 if r2 is None else r2.stride(0), _p(gate) if epilogue == EPI_RESIDUAL else None, _stream()),
        f"gemm_{tag}_blocked",
    )
    return out


def gemm_fp8_blocked(xq, sx, wq_nk, sw, bias=None, epilogue=EPI_NONE, out=None, resid=None, gate=None):
    """x2v_gemm_fp8_blocked: the w8a8 GEMM on block-strided operands (see gemm_blocked).  `xq`: e4m3 codes [M, K] or K-blocked [B, M, K/B]
    (the codes of the ROW's quantisation, `sx` [M] stays per row); `out`: None / [M, N] or N-blocked [B', M, N/B'] (preallocated); the residual
    epilogue needs a row-major `resid` (= the output).  Returns the output tensor."""
    return _gemm8_blocked(_FP8, xq, sx, wq_nk, sw, bias, epilogue, out, resid, gate)


def gemm_int8_blocked(xq, sx, wq_nk, sw, bias=None, epilogue=EPI_NONE, out=None, resid=None, gate=None):
    """gemm_fp8_blocked on int8 codes (x2v_gemm_int8_blocked)."""
    return _gemm8_blocked(_INT8, xq, sx, wq_nk, sw, bias, epilogue, out, resid, gate)


def sinusoid_embed(t, dim):
    """Timestep sinusoid [n, dim] bf16.  Integer timesteps (the UniPC scheduler's) go to x2v_sinusoid_embed_bf16; floating-point ones (the step-distill
    scheduler's sigma * 1000, fractional) keep their fraction, as in the reference: x2v_sinusoid_embed_f64_bf16."""
    if t.is_floating_point():
        t = t.reshape(-1).to(torch.float64)
        out = torch.empty((t.numel(), dim), dtype=torch.bfloat16, device=t.device)
        init()
        _check(_lib.x2v_sinusoid_embed_f64_bf16(_p(t), _p(out), t.numel(), dim, _stream()), "sinusoid_embed")
        return out
    t = t.reshape(-1).to(torch.int64)
    out = torch.empty((t.numel(), dim), dtype=torch.bfloat16, device=t.device)
    init()
    _check(_lib.x2v_sinusoid_embed_bf16(_p(t), _p(out), t.numel(), dim, _stream()), "sinusoid_embed")
    return out


def causal_conv3d(x, weight, bias=None, cache=None):
    """x [T,H,W,Cin] fp32 channels-last, weight [Cout,kt,kh,kw,Cin], cache [nc,H,W,Cin] or None."""
    if x.dtype != torch.float32 or not x.is_contiguous() or not weight.is_contiguous():
        raise X2VError("causal_conv3d: x and weight must be contiguous float32")
    T, H, W, Cin = x.shape
    Cout, kt, kh, kw, _ = weight.shape
    nc = 0 if cache is None else cache.shape[0]
    out = torch.empty((T, H, W, Cout), dtype=torch.float32, device=x.device)
    init()
    _check(_lib.x2v_causal_conv3d_f32(_p(x), _p(cache), nc, _p(weight), _p(bias), _p(out), T, H, W, Cin, Cout, kt, kh, kw, _stream()), "causal_conv3d")
    return out


VCONV_CLAMP, VCONV_TSPLIT = 1, 2
VCONV_PER_TAP, VCONV_HALO64, VCONV_ZERO_TAIL32 = 4, 8, 16  # x2v_vae_conv_f16 only: kernel choice for A/B runs; the last 32 channels of Cin are zero padding


def _f32c(t, name):
    if t is not None and (t.dtype != torch.float32 or not t.is_cuda):
        raise X2VError(f"{name}: expected a float32 device tensor")
    return t


def _f32dense(t, name, dim=None, numel=None):
    """None passes through; otherwise a contiguous float32 device tensor (of rank `dim` / `numel` elements when given)."""
    if t is None:
        return None
    if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
        raise X2VError(f"{name}: expected a contiguous float32 device tensor, got {t.dtype} {tuple(t.shape)} strides {t.stride()} on {t.device}")
    if dim is not None and t.dim() != dim:
        raise X2VError(f"{name}: expected rank {dim}, got shape {tuple(t.shape)}")
    if numel is not None and t.numel() != numel:
        raise X2VError(f"{name}: expected {numel} elements, got shape {tuple(t.shape)}")
    return t


def _dev_view(t, name, dtypes):
    if t.dtype not in dtypes or not t.is_cuda:
        raise X2VError(f"{name}: expected a device tensor of {' / '.join(str(d) for d in dtypes)}, got {t.dtype} on {t.device}")
    return t


def vae_conv(xp, strides, weight, out, T, H, W, bias=None, resid=None, flags=0, w_row_stride=None, cin=None):
    """Implicit-GEMM convolution over a zero-bordered buffer (x2v_vae_conv_f32).  `xp`: tensor VIEW whose first element is
    what tap (0,0,0) of output pixel (0,0,0) reads; strides = (frame, row, pixel) in floats; weight [Cout,kt,kh,kw,Cin]
    (or [Cout, K] with kt=kh=kw=1); out [T,H,W,Cout] (preallocated, contiguous)."""
    _f32c(xp, "vae_conv x"), _f32c(weight, "vae_conv weight"), _f32c(out, "vae_conv out")
    if weight.dim() == 5:
        Cout, kt, kh, kw, Cin = weight.shape
    else:
        Cout, kt, kh, kw = weight.shape[0], 1, 1, 1
        Cin = weight.shape[1] if cin is None else cin
    wrs = weight.stride(0) if w_row_stride is None else w_row_stride
    fs, rs, ps = strides
    init()
    _check(_lib.x2v_vae_conv_f32(_p(xp), fs, rs, ps, _p(weight), wrs, _p(bias), _p(resid), _p(out), T, H, W, Cin, Cout, kt, kh, kw, flags, _stream()), "vae_conv")
    return out


_VCONV16_KERNELS = {"": 0, "halo64": VCONV_HALO64, "pertap": VCONV_PER_TAP}
if os.environ.get("X2V_VAE_CONV16", "") not in _VCONV16_KERNELS:
    raise X2VError(f"X2V_VAE_CONV16={os.environ['X2V_VAE_CONV16']!r}: accepted values are 'halo64' and 'pertap' (or unset / empty: the default dispatch)")
_VCONV16_FORCE = _VCONV16_KERNELS[os.environ.get("X2V_VAE_CONV16", "")]  # A/B runs: force one of the older 3x3 kernels


def vae_conv16_cached_ok(W, weight, flags=0):
    """Whether vae_conv16(..., cache=...) is available for this weight [Cout,kt,kh,kw,Cin] and image width (x2v_vae_conv_f16_cached_ok)."""
    Cout, kt, kh, kw, Cin = weight.shape
    init()
    return kt > 1 and _lib.x2v_vae_conv_f16_cached_ok(W, Cin, Cout, kh, kw, flags | _VCONV16_FORCE) == 1


def vae_conv16(xp, strides, weight, out, T, H, W, bias=None, resid=None, flags=0, cache=None):
    """x2v_vae_conv_f16: fp16 operand buffer `xp` (strides in halves) and fp16 weight [Cout,kt,kh,kw,Cin], fp32 bias / resid / out.
    cache: the kt - 1 leading input frames in a tensor of their own ([kt-1, H+2, W+2, Cin], xp's layout; x2v_vae_conv_f16_cached) — xp's own leading frames are not read."""
    if xp.dtype != torch.float16 or weight.dtype != torch.float16 or not xp.is_cuda or not weight.is_contiguous():
        raise X2VError("vae_conv16: operand buffer and weight must be CUDA float16 (weight contiguous)")
    _f32c(out, "vae_conv16 out")
    Cout, kt, kh, kw, Cin = weight.shape
    fs, rs, ps = strides
    init()
    flags |= _VCONV16_FORCE
    if cache is not None:
        if cache.dtype != torch.float16 or not cache.is_cuda or not cache.is_contiguous() or cache.shape[0] != kt - 1 or cache[0].numel() != fs:
            raise X2VError("vae_conv16: cache must be a contiguous CUDA float16 tensor of kt - 1 frames in xp's layout")
        _check(_lib.x2v_vae_conv_f16_cached(_p(xp), _p(cache), fs, rs, ps, _p(weight), weight.stride(0), _p(bias), _p(resid), _p(out), T, H, W, Cin, Cout, kt, kh, kw, flags, _stream()), "vae_conv16 (cached)")
        return out
    _check(_lib.x2v_vae_conv_f16(_p(xp), fs, rs, ps, _p(weight), weight.stride(0), _p(bias), _p(resid), _p(out), T, H, W, Cin, Cout, kt, kh, kw, flags, _stream()), "vae_conv16")
    return out


def vae_prep(x, y_view, y_strides, gamma=None, a=None, b=None, silu=False, upsample=False, split=False):
    """x [T,H,W,C] contiguous fp32 -> y_view (first element = destination of pixel (0,0,0)); y_strides = (frame, row) in floats.
    split (fp16 y_view only): write the hi/lo split [hi | hi * 2^-12 | lo] (3*C channels per pixel, x2v_vae_prep_split_f16; weights [hi | lo * 2^12 | hi])."""
    T, H, W, C = _f32dense(x, "vae_prep x", 4).shape
    for nm, t in (("gamma", gamma), ("a", a), ("b", b)):
        _f32dense(t, f"vae_prep {nm}", numel=C)
    _dev_view(y_view, "vae_prep y", (torch.float32, torch.float16))
    init()
    if y_view.dtype == torch.float16:  # operand buffer of the 16-bit convolution: channel axis possibly padded (pixel stride from the view)
        fn = _lib.x2v_vae_prep_split_f16 if split else _lib.x2v_vae_prep_f16
        _check(fn(_p(x), _p(y_view), T, H, W, C, _p(gamma), _p(a), _p(b), int(silu), int(upsample), y_strides[0], y_strides[1], y_view.stride(2), _stream()), "vae_prep_f16")
        return
    if split:
        raise X2VError("vae_prep: split needs an fp16 destination")
    _check(_lib.x2v_vae_prep_f32(_p(x), _p(y_view), T, H, W, C, _p(gamma), _p(a), _p(b), int(silu), int(upsample), y_strides[0], y_strides[1], _stream()), "vae_prep")


def softmax_rows_(s, scale):
    _f32c(s, "softmax_rows")
    M, N = s.shape
    init()
    _check(_lib.x2v_softmax_rows_f32(_p(s), s.stride(0), M, N, float(scale), _stream()), "softmax_rows")
    return s


def headnorm_rope_(q, k, wq, wk, cos, sin, num_heads, l_rope, eps=1e-6, round_mode=ROUND_FP32, q_out_scale=1.0):
    """In place on q, k [L, H*128] views (unit inner stride, any token stride): per-head RMSNorm + real RoPE on the
    first l_rope tokens (x2v_headnorm_rope_bf16)."""
    _row2d(_bf16(q, "headnorm_rope q"), "headnorm_rope q"), _row2d(_bf16(k, "headnorm_rope k"), "headnorm_rope k")
    L = q.shape[0]
    if q.shape != k.shape or q.shape[1] != num_heads * 128:
        raise X2VError(f"headnorm_rope: q {tuple(q.shape)} and k {tuple(k.shape)} must both be [L, {num_heads}*128]")
    if not 0 <= l_rope <= L:
        raise X2VError(f"headnorm_rope: l_rope={l_rope} outside [0, {L}]")
    wq, wk = _vec(wq, "headnorm_rope wq", 128), _vec(wk, "headnorm_rope wk", 128)
    cos, sin = _vec(cos, "headnorm_rope cos"), _vec(sin, "headnorm_rope sin")
    if l_rope and (cos is None or sin is None or cos.numel() < l_rope * 128 or sin.numel() < l_rope * 128):
        raise X2VError(f"headnorm_rope: cos/sin must be bf16 tables of at least [{l_rope}, 128]")
    init()
    _check(_lib.x2v_headnorm_rope_bf16(_p(q), q.stride(0), _p(k), k.stride(0), _p(wq), _p(wk), _p(cos), _p(sin), L, num_heads, l_rope, eps, round_mode, q_out_scale, _stream()),
           "headnorm_rope")


def headnorm_rope_blocked_(q, k, wq, wk, cos, sin, num_heads, l_rope, eps=1e-6, round_mode=ROUND_FP32, q_out_scale=1.0):
    """headnorm_rope_ in place on head-blocked q, k [N, L, (H/N)*128] (contiguous: the send buffers of the Ulysses exchange)."""
    for t, nm in ((q, "q"), (k, "k")):
        if t.dim() != 3 or t.dtype != torch.bfloat16 or not t.is_cuda or not t.is_contiguous():
            raise X2VError(f"headnorm_rope_blocked {nm}: expected a contiguous bf16 device tensor [N, L, (H/N)*128], got {t.dtype} {tuple(t.shape)}")
    nb, L, bc = q.shape
    if q.shape != k.shape or bc % 128 or nb * bc != num_heads * 128:
        raise X2VError(f"headnorm_rope_blocked: q {tuple(q.shape)} / k {tuple(k.shape)} do not hold {num_heads} heads of 128 in equal blocks")
    if not 0 <= l_rope <= L:
        raise X2VError(f"headnorm_rope_blocked: l_rope={l_rope} outside [0, {L}]")
    wq, wk = _vec(wq, "headnorm_rope wq", 128), _vec(wk, "headnorm_rope wk", 128)
    cos, sin = _vec(cos, "headnorm_rope cos"), _vec(sin, "headnorm_rope sin")
    if l_rope and (cos is None or sin is None or cos.numel() < l_rope * 128 or sin.numel() < l_rope * 128):
        raise X2VError(f"headnorm_rope_blocked: cos/sin must be bf16 tables of at least [{l_rope}, 128]")
    init()
    _check(_lib.x2v_headnorm_rope_blocked_bf16(_p(q), _p(k), bc, bc // 128, L * bc, _p(wq), _p(wk), _p(cos), _p(sin), L, num_heads, l_rope, eps, round_mode, q_out_scale, _stream()),
           "headnorm_rope_blocked")


def vae_prep_ex(x, y_view, y_strides, mul=None, add=None, silu=False, clamp01=False, up_hw=False, up_t=False):
    """fp32 x [T,H,W,C] → y_view (fp32, or fp16 for the 16-bit convolution's operand buffer; strides in elements of y)."""
    T, H, W, C = _f32dense(x, "vae_prep_ex x", 4).shape
    _f32dense(mul, "vae_prep_ex mul", numel=C), _f32dense(add, "vae_prep_ex add", numel=C)
    _dev_view(y_view, "vae_prep_ex y", (torch.float32, torch.float16))
    init()
    if y_view.dtype == torch.float16:
        _check(_lib.x2v_vae_prep_ex_f16(_p(x), _p(y_view), T, H, W, C, _p(mul), _p(add), int(silu), int(clamp01), int(up_hw), int(up_t), y_strides[0], y_strides[1], _stream()),
               "vae_prep_ex_f16")
        return
    _check(_lib.x2v_vae_prep_ex_f32(_p(x), _p(y_view), T, H, W, C, _p(mul), _p(add), int(silu), int(clamp01), int(up_hw), int(up_t), y_strides[0], y_strides[1], _stream()),
           "vae_prep_ex")


def vae_conv_s2(x, weight, out, bias=None):
    """x2v_vae_conv_s2_f16: 3x3 stride-2 convolution with the bottom / right zero pad of Resample downsample2d / 3d.  x: fp16 view [T, Hin, Win, >= Cin]
    (pixel stride from the view, the pixel axis may be padded); weight: contiguous fp16 [Cout, 3, 3, Cin] (or [Cout, 1, 3, 3, Cin]); out: fp32 [T, Hin // 2, Win // 2, Cout]."""
    if x.dtype != torch.float16 or weight.dtype != torch.float16 or not x.is_cuda or not weight.is_cuda or not weight.is_contiguous():
        raise X2VError("vae_conv_s2: operand and weight must be CUDA float16 (weight contiguous)")
    if x.dim() != 4 or x.stride(3) != 1:
        raise X2VError("vae_conv_s2: x must be a [T, H, W, C] view with unit channel stride")
    _f32dense(out, "vae_conv_s2 out", 4), _f32dense(bias, "vae_conv_s2 bias")
    cout, cin = weight.shape[0], weight.shape[-1]
    T, H, W, _ = x.shape
    if tuple(out.shape) != (T, H // 2, W // 2, cout) or weight.numel() != cout * 9 * cin:
        raise X2VError(f"vae_conv_s2: out {tuple(out.shape)} / weight {tuple(weight.shape)} do not match x {tuple(x.shape)}")
    init()
    _check(_lib.x2v_vae_conv_s2_f16(_p(x), x.stride(0), x.stride(1), x.stride(2), _p(weight), weight.stride(0), _p(bias), _p(out), T, H, W, cin, cout, 0, _stream()),
           "vae_conv_s2")
    return out


VIDEO_PREP_MODES = {torch.float32: 0, torch.float16: 1, "split": 2}


def vae_video_prep(video, y_view, split=False):
    """x2v_vae_video_prep: video [3, T, H, W] fp32 (a view with unit W stride: read in place) -> y_view [T, H, W, >= 3 (9 split)] channels-last fp32 /
    fp16 / hi-lo split fp16 (strides from the view)."""
    _f32c(video, "vae_video_prep video")
    if video.dim() != 4 or video.shape[0] != 3 or video.stride(3) != 1:
        raise X2VError(f"vae_video_prep: expected a [3, T, H, W] video with unit W stride, got {tuple(video.shape)} strides {video.stride()}")
    _dev_view(y_view, "vae_video_prep y", (torch.float32, torch.float16))
    if split and y_view.dtype != torch.float16:
        raise X2VError("vae_video_prep: split needs an fp16 destination")
    if y_view.dim() != 4 or tuple(y_view.shape[:3]) != tuple(video.shape[1:]) or y_view.stride(3) != 1:
        raise X2VError(f"vae_video_prep: destination {tuple(y_view.shape)} does not match video {tuple(video.shape)}")
    _, T, H, W = video.shape
    init()
    mode = 2 if split else VIDEO_PREP_MODES[y_view.dtype]
    _check(_lib.x2v_vae_video_prep(_p(video), video.stride(0), video.stride(1), video.stride(2), T, H, W, _p(y_view), y_view.stride(0), y_view.stride(1),
                                   y_view.stride(2), mode, _stream()), "vae_video_prep")


def vae_tile_compose(center, up, left, up_left, ev, eh, out_region, clamp=False):
    """x2v_vae_tile_compose_f32: one output tile of the Wan VAE's tiled decode / encode from its raw tiles.  center [T, ch, cw, C], up [T, uh, cw, C],
    left [T, ch, lw, C], up_left [T, uh, lw, C]: contiguous fp32 channels-last (None where the tile has no such neighbour; ev / eh = 0 then);
    out_region: the [C, T, rh, rw] view (unit x stride) of the channel-first output that this tile owns, rh <= ch, rw <= cw."""
    T, ch, cw, C = _f32dense(center, "vae_tile_compose center", 4).shape
    uh = lw = 0
    if ev:
        if up is None or tuple(_f32dense(up, "vae_tile_compose up", 4).shape[::2]) != (T, cw) or up.shape[3] != C:
            raise X2VError(f"vae_tile_compose: a vertical extent needs an upper tile [T, uh, {cw}, {C}]")
        uh = up.shape[1]
    if eh:
        if left is None or tuple(_f32dense(left, "vae_tile_compose left", 4).shape[:2]) != (T, ch) or left.shape[3] != C:
            raise X2VError(f"vae_tile_compose: a horizontal extent needs a left tile [{T}, {ch}, lw, {C}]")
        lw = left.shape[2]
    if ev and eh and (up_left is None or tuple(_f32dense(up_left, "vae_tile_compose up_left", 4).shape) != (T, uh, lw, C)):
        raise X2VError(f"vae_tile_compose: both extents need an up-left tile [{T}, {uh}, {lw}, {C}]")
    _dev_view(out_region, "vae_tile_compose out", (torch.float32,))
    if out_region.dim() != 4 or out_region.shape[0] != C or out_region.shape[1] != T or out_region.stride(3) != 1:
        raise X2VError(f"vae_tile_compose: the output region must be a [{C}, {T}, rh, rw] view with unit x stride, got {tuple(out_region.shape)} strides {out_region.stride()}")
    rh, rw = out_region.shape[2:]
    if not (0 < rh <= ch and 0 < rw <= cw and 0 <= ev <= min(ch, uh if ev else ch) and 0 <= eh <= min(cw, lw if eh else cw)):
        raise X2VError(f"vae_tile_compose: region {rh}x{rw} / extents {ev}, {eh} do not fit the tiles (centre {ch}x{cw}, up {uh} rows, left {lw} columns)")
    init()
    _check(_lib.x2v_vae_tile_compose_f32(_p(center), _p(up) if ev else None, _p(left) if eh else None, _p(up_left) if ev and eh else None, T, C, ch, cw, uh, lw, ev, eh,
                                         rh, rw, _p(out_region), out_region.stride(0), out_region.stride(1), out_region.stride(2), int(bool(clamp)), _stream()),
           "vae_tile_compose")


def vae_replicate_border_(buf, lead, pad):
    frames, hp, wp, c = buf.shape
    if buf.dtype == torch.float16:  # the kernel moves whole pixels: a pixel of C halves is C/2 floats
        c //= 2
    init()
    _check(_lib.x2v_vae_replicate_border_f32(_p(buf), frames, lead, hp, wp, c, pad, _stream()), "vae_replicate_border")


C2D_RELU, C2D_UPSAMPLE_READ, C2D_TWO_SOURCE, C2D_HEAD = 1, 2, 4, 8  # x2v.h X2V_C2D_*


def conv2d_bf16(x, weight, out, H, W, bias=None, resid=None, mem=None, flags=0, tsplit=1, frame_trim=0, out_strides=None):
    """x2v_conv2d_bf16.  x: bf16 device VIEW [T, Hin, Win, Cin] with unit channel stride (Hin, Win = H, W, or their halves rounded up with C2D_UPSAMPLE_READ);
    weight [Cout, k, k, Cin] (or [.., 2 Cin] with C2D_TWO_SOURCE) contiguous; mem: the frame in front of x[0] for the two-source form ([Hin, Win, Cin] in x's row and
    pixel strides) or None (zero); out: bf16 device view whose first element is output frame 0, pixel (0, 0), channel 0, addressed by out_strides = (frame, row, pixel,
    channel) in elements (default: a channels-last [T_out, H, W, Cout / tsplit] tensor's own); resid: bf16 view in out's strides."""
    for t, name in ((x, "x"), (weight, "weight"), (out, "out"), (bias, "bias"), (resid, "resid"), (mem, "mem")):
        if t is not None and (t.dtype != torch.bfloat16 or not t.is_cuda):
            raise X2VError(f"conv2d_bf16 {name}: expected a bfloat16 device tensor, got {t.dtype} on {t.device}; the x2v HIP path has no CPU fallback")
    if x.dim() != 4 or x.stride(3) != 1 or weight.dim() != 4 or not weight.is_contiguous() or weight.shape[1] != weight.shape[2]:
        raise X2VError(f"conv2d_bf16: x must be [T, H, W, C] with unit channel stride and weight a contiguous [Cout, k, k, C], got {tuple(x.shape)} {x.stride()} / {tuple(weight.shape)}")
    T, Hin, Win, Cin = x.shape
    Cout, k = weight.shape[0], weight.shape[1]
    up = 1 if flags & C2D_UPSAMPLE_READ else 0
    if weight.shape[3] != (2 if flags & C2D_TWO_SOURCE else 1) * Cin or (Hin, Win) != ((H + up) >> up, (W + up) >> up):
        raise X2VError(f"conv2d_bf16: x {tuple(x.shape)} / weight {tuple(weight.shape)} / output {H} x {W} / flags {flags} disagree")
    if mem is not None and (tuple(mem.shape) != (Hin, Win, Cin) or mem.stride() != x.stride()[1:]):
        raise X2VError(f"conv2d_bf16: mem must be one frame in x's layout, got {tuple(mem.shape)} strides {mem.stride()}")
    if bias is not None and (bias.numel() != Cout or not bias.is_contiguous()):
        raise X2VError(f"conv2d_bf16: bias of {bias.numel()} elements for {Cout} output channels")
    if out_strides is None:
        if out.dim() != 4 or tuple(out.shape[1:]) != (H, W, Cout // tsplit) or out.shape[0] != (T - frame_trim) * tsplit:
            raise X2VError(f"conv2d_bf16: out {tuple(out.shape)} is not [{(T - frame_trim) * tsplit}, {H}, {W}, {Cout // tsplit}]")
        out_strides = out.stride()
    if resid is not None and out_strides == tuple(out.stride()) and (resid.shape != out.shape or resid.stride() != out.stride()):
        raise X2VError("conv2d_bf16: resid must have out's shape and strides")
    ys = [int(s) for s in out_strides]
    init()
    _check(_lib.x2v_conv2d_bf16(_p(x), _p(mem), x.stride(0), x.stride(1), x.stride(2), _p(weight), _p(bias), _p(resid), _p(out), ys[0], ys[1], ys[2], ys[3], T, H, W, Cin, Cout,
                                k, flags, tsplit, frame_trim, _stream()), "conv2d_bf16")
    return out


def taehv_clamp(z, out):
    """x2v_taehv_clamp_bf16: z [C, T, h, w] fp32 or bf16 device tensor with contiguous rows -> out [T, h, w, C] contiguous bf16 = tanh(z / 3) * 3 in the reference's roundings."""
    if z.dtype not in (torch.float32, torch.bfloat16) or not z.is_cuda or z.dim() != 4 or z.stride(3) != 1 or (z.shape[2] > 1 and z.stride(2) != z.shape[3]):
        raise X2VError(f"taehv_clamp: expected a [C, T, h, w] float32 / bfloat16 device tensor with contiguous frames, got {z.dtype} {tuple(z.shape)} {z.stride()} on {z.device}")
    C, T, h, w = z.shape
    if out.dtype != torch.bfloat16 or not out.is_cuda or not out.is_contiguous() or tuple(out.shape) != (T, h, w, C):
        raise X2VError(f"taehv_clamp: out must be a contiguous bfloat16 device tensor [{T}, {h}, {w}, {C}], got {out.dtype} {tuple(out.shape)}")
    init()
    _check(_lib.x2v_taehv_clamp_bf16(_p(z), int(z.dtype == torch.float32), z.stride(0), z.stride(1), _p(out), T, h, w, C, _stream()), "taehv_clamp")
    return out


def groupnorm_affine(x, groups, gamma, beta, eps=1e-6):
    """x [..., C] contiguous fp32 → (mul[C], add[C]) such that GroupNorm(x)[..., c] = x[..., c]*mul[c] + add[c]."""
    c = _f32dense(x, "groupnorm_affine x").shape[-1]
    if groups <= 0 or c % groups:
        raise X2VError(f"groupnorm_affine: {c} channels do not split into {groups} groups")
    _f32dense(gamma, "groupnorm_affine gamma", numel=c), _f32dense(beta, "groupnorm_affine beta", numel=c)
    npix = x.numel() // c
    ws = torch.empty(2 * groups, dtype=torch.float64, device=x.device)
    mul, add = torch.empty(c, dtype=torch.float32, device=x.device), torch.empty(c, dtype=torch.float32, device=x.device)
    init()
    _check(_lib.x2v_groupnorm_affine_f32(_p(x), npix, c, groups, _p(gamma), _p(beta), eps, _p(ws), _p(mul), _p(add), _stream()), "groupnorm_affine")
    return mul, add


def softmax_rows_causal_(s, scale, hw, n_keys=None):
    _dev_view(s, "softmax_rows_causal", (torch.float32,))
    if s.dim() != 2 or s.stride(1) != 1:
        raise X2VError(f"softmax_rows_causal: expected a 2-D fp32 tensor with unit inner stride, got {tuple(s.shape)} strides {s.stride()}")
    M, N = s.shape
    if hw <= 0 or not 0 <= (N if n_keys is None else n_keys) <= N:
        raise X2VError(f"softmax_rows_causal: hw={hw}, n_keys={n_keys} for {N} columns")
    init()
    _check(_lib.x2v_softmax_rows_causal_f32(_p(s), s.stride(0), M, N, float(scale), hw, N if n_keys is None else n_keys, _stream()), "softmax_rows_causal")
    return s


def blend_axis_(a, b, axis, extent):
    """b[.., idx, ..] = a[.., na-extent+idx, ..]*(1-idx/extent) + b*(idx/extent) along `axis` of two contiguous fp32 tensors
    that agree in every other dimension."""
    _f32dense(a, "blend_axis a"), _f32dense(b, "blend_axis b")
    if a.dim() != b.dim():
        raise X2VError(f"blend_axis: ranks differ: {tuple(a.shape)} vs {tuple(b.shape)}")
    axis = axis % a.dim()
    if any(x_ != y_ for i_, (x_, y_) in enumerate(zip(a.shape, b.shape)) if i_ != axis):
        raise X2VError(f"blend_axis: {tuple(a.shape)} and {tuple(b.shape)} must agree outside axis {axis}")
    outer = 1
    for d in a.shape[:axis]:
        outer *= d
    inner = 1
    for d in a.shape[axis + 1 :]:
        inner *= d
    na, nb = a.shape[axis], b.shape[axis]
    init()
    _check(_lib.x2v_blend_axis_f32(_p(a), _p(b), outer, na, nb, inner, na * inner, nb * inner, min(extent, na, nb), _stream()), "blend_axis")
    return b


def _f32flat(t, name, n):
    if t is None:
        return None
    if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or t.numel() != n:
        raise X2VError(f"{name}: expected a contiguous float32 device tensor of {n} elements, got {t.dtype} {tuple(t.shape)} on {t.device}")
    return t


def _latents(t, name, n):
    if t.dtype not in (torch.float32, torch.bfloat16) or not t.is_cuda or not t.is_contiguous() or t.numel() != n:
        raise X2VError(f"{name}: expected a contiguous float32 / bfloat16 device tensor of {n} elements")
    return t


def unipc_step(cond, uncond, latents, last_sample, m0, m1, coef, order_c, order_p, want_noise_pred=False):
    """x2v_unipc_step_f32: (noise_pred | None, x0, corrected sample, next latents) — CFG combine + WanScheduler.step_post in one launch.
    `coef`: the 12 fp32 coefficients of include/x2v.h as Python floats."""
    n = cond.numel()
    _f32flat(cond, "cond", n), _f32flat(uncond, "uncond", n), _latents(latents, "latents", n)
    _f32flat(last_sample, "last_sample", n), _f32flat(m0, "m0", n), _f32flat(m1, "m1", n)
    if len(coef) != 12:
        raise X2VError("unipc_step: coef must hold 12 values")
    new = lambda: torch.empty(cond.shape, dtype=torch.float32, device=cond.device)  # noqa: E731
    noise_pred = new() if want_noise_pred else None
    x0, sample, lat = new(), new(), new()
    init()
    carr = (_f32 * 12)(*[float(c) for c in coef])
    _check(
        _lib.x2v_unipc_step_f32(_p(cond), _p(uncond), _p(latents), int(latents.dtype == torch.bfloat16), _p(last_sample), _p(m0), _p(m1), _p(noise_pred), _p(x0), _p(sample),
                                _p(lat), carr, order_c, order_p, n, _stream()),
        "unipc_step",
    )
    return noise_pred, x0, sample, lat


def distill_step(cond, uncond, guide, latents, noise, sigma, one_minus_next, sigma_next, want_noise_pred=False):
    """x2v_distill_step_f32: (noise_pred | None, next latents in the dtype of `latents`)."""
    n = cond.numel()
    _f32flat(cond, "cond", n), _f32flat(uncond, "uncond", n), _latents(latents, "latents", n), _f32flat(noise, "noise", n)
    noise_pred = torch.empty(cond.shape, dtype=torch.float32, device=cond.device) if want_noise_pred else None
    out = torch.empty(cond.shape, dtype=latents.dtype, device=cond.device)
    init()
    _check(
        _lib.x2v_distill_step_f32(_p(cond), _p(uncond), float(guide), _p(latents), int(latents.dtype == torch.bfloat16), _p(noise), float(sigma), float(one_minus_next),
                                  float(sigma_next), _p(noise_pred), _p(out), n, _stream()),
        "distill_step",
    )
    return noise_pred, out


# ---- CLIP image tower (fp16; csrc/clip.hip) ---------------------------------------------------------------------------------------------------------
EPI16_NONE, EPI16_GELU_ERF, EPI16_RESIDUAL, EPI16_QUICK_GELU, EPI16_SWIGLU = 0, 1, 2, 3, 4


def _f16rows(t, name):
    if t.dtype != torch.float16:
        raise X2VError(f"{name}: expected float16, got {t.dtype}")
    return _row2d(t, name)


def gemm_f16(x, weight_nk, bias=None, epilogue=EPI16_NONE, resid=None, out=None):
    """x2v_gemm_f16: y[M, N] = epi(x[M, K] . W[N, K]^T + bias) in fp16 (fp32 accumulation); K % 32 == 0, N % 4 == 0.  With EPI16_SWIGLU W is [2N, K]
    (rows of gate_proj and up_proj interleaved) and there is no bias."""
    x, w = _f16rows(x, "gemm_f16 x"), _f16rows(weight_nk, "gemm_f16 weight")
    M, K = x.shape
    if epilogue == EPI16_SWIGLU and w.shape[0] % 2:
        raise X2VError(f"gemm_f16: the SwiGLU epilogue needs an even number of weight rows, got {w.shape[0]}")
    N = w.shape[0] // 2 if epilogue == EPI16_SWIGLU else w.shape[0]
    if w.shape[1] != K:
        raise X2VError(f"gemm_f16: x {tuple(x.shape)} and weight {tuple(w.shape)} disagree on K")
    bias = _vec(bias, "gemm_f16 bias", N, dtype=torch.float16)
    out = torch.empty((M, N), dtype=torch.float16, device=x.device) if out is None else _f16rows(out, "gemm_f16 out")
    if out.shape != (M, N) or (resid is not None and _f16rows(resid, "gemm_f16 resid").shape != (M, N)):
        raise X2VError(f"gemm_f16: out / resid must be [{M}, {N}]")
    init()
    _check(_lib.x2v_gemm_f16(_p(x), x.stride(0), _p(w), w.stride(0), _p(bias), _p(out), out.stride(0), M, N, K, epilogue, _p(resid), 0 if resid is None else resid.stride(0),
                             _stream()), "gemm_f16")
    return out


def gemm_f16_tile_choice(M, N):
    """x2v_gemm_f16_tile_choice: (rows, columns) of the workgroup tile x2v_gemm_f16 launches for (M, N) — host arithmetic."""
    t = _lib.x2v_gemm_f16_tile_choice(M, N)
    _check(min(t, 0), "gemm_f16_tile_choice")
    return ((128, 64), (64, 64), (64, 32), (64, 16))[t]


def attention_f16_d80(qkv, batch, num_heads, out=None, scale=0.0):
    """x2v_attn_f16_d80 on the to_qkv output qkv [batch * S, 3 * num_heads * 80] (read in place) -> [batch * S, num_heads * 80] fp16."""
    qkv = _f16rows(qkv, "attention_f16_d80 qkv")
    D = num_heads * 80
    if qkv.shape[1] != 3 * D or batch < 1 or qkv.shape[0] % batch:
        raise X2VError(f"attention_f16_d80: qkv {tuple(qkv.shape)} is not [batch * S, 3 * {num_heads} * 80] for batch {batch}")
    out = torch.empty((qkv.shape[0], D), dtype=torch.float16, device=qkv.device) if out is None else _f16rows(out, "attention_f16_d80 out")
    if out.shape != (qkv.shape[0], D):
        raise X2VError(f"attention_f16_d80: out must be [{qkv.shape[0]}, {D}]")
    init()
    _check(_lib.x2v_attn_f16_d80(_p(qkv), qkv.stride(0), _p(out), out.stride(0), batch, qkv.shape[0] // batch, num_heads, scale, _stream()), "attention_f16_d80")
    return out


def layernorm_f16(x, weight, bias, eps=1e-5, out=None):
    """x2v_layernorm_f16: fp16 rows, fp32 weight / bias and statistics, one rounding."""
    x = _f16rows(x, "layernorm_f16 x")
    D = x.shape[1]
    weight, bias = _vec(weight, "layernorm_f16 weight", D, dtype=torch.float32), _vec(bias, "layernorm_f16 bias", D, dtype=torch.float32)
    if weight is None or bias is None:
        raise X2VError("layernorm_f16: weight and bias are required")
    out = torch.empty_like(x) if out is None else _f16rows(out, "layernorm_f16 out")
    if out.shape != x.shape:
        raise X2VError(f"layernorm_f16: out must be {tuple(x.shape)}, got {tuple(out.shape)}")
    init()
    _check(_lib.x2v_layernorm_f16(_p(x), x.stride(0), _p(weight), _p(bias), _p(out), out.stride(0), x.shape[0], D, eps, _stream()), "layernorm_f16")
    return out


def clip_embed(patches, cls, pos, weight, bias, batch, eps=1e-5, out=None):
    """x2v_clip_embed_f16: patches [batch * (T - 1), D] fp16, cls [D], pos [T, D] fp16, pre_norm weight / bias fp32 -> [batch * T, D] fp16."""
    patches = _f16rows(patches, "clip_embed patches")
    D = patches.shape[1]
    if batch < 1 or patches.shape[0] == 0 or patches.shape[0] % batch:
        raise X2VError(f"clip_embed: patches {tuple(patches.shape)} is not [batch * (T - 1), D] for batch {batch}")
    T = patches.shape[0] // batch + 1
    cls, pos = _vec(cls, "clip_embed cls", D, dtype=torch.float16), _vec(pos, "clip_embed pos", T * D, dtype=torch.float16)
    weight, bias = _vec(weight, "clip_embed weight", D, dtype=torch.float32), _vec(bias, "clip_embed bias", D, dtype=torch.float32)
    out = torch.empty((batch * T, D), dtype=torch.float16, device=patches.device) if out is None else _f16rows(out, "clip_embed out")
    if out.shape != (batch * T, D):
        raise X2VError(f"clip_embed: out must be [{batch * T}, {D}], got {tuple(out.shape)}")
    init()
    _check(_lib.x2v_clip_embed_f16(_p(patches), patches.stride(0), _p(cls), _p(pos), _p(weight), _p(bias), _p(out), out.stride(0), batch, T, D, eps, _stream()), "clip_embed")
    return out


def clip_preprocess(img, out, image_size, patch, mean, std):
    """x2v_clip_preprocess_f16: img [3, H, W] fp32 in [-1, 1] (unit W stride, read in place) -> out [(image_size / patch)^2, >= 3 patch^2] fp16 rows.
    The kernel writes whole rows of the row stride (columns beyond 3 patch^2 are zeroed), so `out` must own its rows: no column-sliced view."""
    _f32c(img, "clip_preprocess img")
    if img.dim() != 3 or img.shape[0] != 3 or img.stride(2) != 1:
        raise X2VError(f"clip_preprocess: expected a [3, H, W] image with unit W stride, got {tuple(img.shape)} strides {img.stride()}")
    out = _f16rows(out, "clip_preprocess out")
    if out.shape[0] != (image_size // patch) ** 2:
        raise X2VError(f"clip_preprocess: out has {out.shape[0]} rows, expected {(image_size // patch) ** 2}")
    if out.shape[1] != out.stride(0):
        raise X2VError(f"clip_preprocess: out is a column slice ({out.shape[1]} of a row stride of {out.stride(0)}); the kernel zero-fills every row up to its stride")
    init()
    _check(_lib.x2v_clip_preprocess_f16(_p(img), img.stride(0), img.stride(1), img.shape[1], img.shape[2], _p(out), out.stride(0), image_size, patch, *[float(m) for m in mean],
                                        *[float(s) for s in std], _stream()), "clip_preprocess")
    return out


# ---- umT5 text encoder (bf16; csrc/t5.hip) ------------------------------------------------------------------------------------------------------------
EPIR_NONE, EPIR_RESIDUAL, EPIR_GEGLU = 0, 2, 3
ATTN_D64_MAX_BATCH, ATTN_D64_MAX_LEN = 8, 512


def _bf16rows(t, name):
    return _row2d(_bf16(t, name), name)


def gemm_rows_bf16(x, weight_nk, epilogue=EPIR_NONE, resid=None, out=None):
    """x2v_gemm_rows_bf16: y[M, N] = epi(x[M, K] . W^T) in bf16 (fp32 accumulation), M <= 4096; K % 32 == 0, N % 4 == 0.  W is [N, K], or [2N, K] with
    EPIR_GEGLU (rows of fc1 and gate.0 interleaved)."""
    x, w = _bf16rows(x, "gemm_rows_bf16 x"), _bf16rows(weight_nk, "gemm_rows_bf16 weight")
    M, K = x.shape
    if w.shape[1] != K:
        raise X2VError(f"gemm_rows_bf16: x {tuple(x.shape)} and weight {tuple(w.shape)} disagree on K")
    if epilogue == EPIR_GEGLU and w.shape[0] % 2:
        raise X2VError(f"gemm_rows_bf16: the GEGLU epilogue needs an even number of weight rows, got {w.shape[0]}")
    N = w.shape[0] // 2 if epilogue == EPIR_GEGLU else w.shape[0]
    if (resid is not None) != (epilogue == EPIR_RESIDUAL):
        raise X2VError("gemm_rows_bf16: resid goes with EPIR_RESIDUAL, and only with it")
    out = torch.empty((M, N), dtype=torch.bfloat16, device=x.device) if out is None else _bf16rows(out, "gemm_rows_bf16 out")
    if out.shape != (M, N) or (resid is not None and _bf16rows(resid, "gemm_rows_bf16 resid").shape != (M, N)):
        raise X2VError(f"gemm_rows_bf16: out / resid must be [{M}, {N}]")
    init()
    _check(_lib.x2v_gemm_rows_bf16(_p(x), x.stride(0), _p(w), w.stride(0), _p(out), out.stride(0), M, N, K, epilogue, _p(resid), 0 if resid is None else resid.stride(0), _stream()),
           "gemm_rows_bf16")
    return out


def gemm_rows_bf16_tile_choice(M, N, epilogue=EPIR_NONE):
    """x2v_gemm_rows_bf16_tile_choice: (rows of x, rows of W) of the workgroup tile x2v_gemm_rows_bf16 launches — host arithmetic."""
    t = _lib.x2v_gemm_rows_bf16_tile_choice(M, N, epilogue)
    _check(min(t, 0), "gemm_rows_bf16_tile_choice")
    return ((128, 64), (64, 64), (64, 32), (64, 16))[t]


def _cu_seqlens(cu_seqlens, rows, who):
    cu = [int(c) for c in cu_seqlens]
    if not 2 <= len(cu) <= ATTN_D64_MAX_BATCH + 1:
        raise X2VError(f"{who}: {len(cu) - 1} sequences; the kernel takes 1..{ATTN_D64_MAX_BATCH} (batch <= {ATTN_D64_MAX_BATCH})")
    lens = [b - a for a, b in zip(cu, cu[1:])]
    if cu[0] < 0 or min(lens) < 1:
        raise X2VError(f"{who}: cu_seqlens {cu} must start at >= 0 and increase")
    if max(lens) > ATTN_D64_MAX_LEN:
        raise X2VError(f"{who}: a sequence of {max(lens)} tokens; the kernel holds at most {ATTN_D64_MAX_LEN} keys (length <= {ATTN_D64_MAX_LEN})")
    if cu[-1] > rows:
        raise X2VError(f"{who}: cu_seqlens ends at row {cu[-1]} but qkv has {rows} rows")
    return (_i32 * len(cu))(*cu), len(cu) - 1


def attention_bf16_d64_relbias(qkv, bias, cu_seqlens, num_heads, out=None, scale=1.0):
    """x2v_attn_bf16_d64_relbias on the fused q | k | v GEMM output qkv [rows, 3 * num_heads * 64] (read in place; a row stride beyond its columns is fine, a
    column slice that starts inside a row is not) -> [rows, num_heads * 64] bf16.  cu_seqlens: host ints, sequence b = rows cu[b] .. cu[b + 1] - 1;
    bias [num_heads, 1023] fp32 on the device.  Rows outside every sequence are not written."""
    who = "attention_bf16_d64_relbias"
    qkv = _bf16rows(qkv, who + " qkv")
    D = num_heads * 64
    if qkv.shape[1] != 3 * D:
        raise X2VError(f"{who}: qkv {tuple(qkv.shape)} is not [rows, 3 * {num_heads} * 64] (q | k | v side by side; pass the whole rows, not a column slice)")
    bias = _vec(bias, who + " bias", num_heads * 1023, dtype=torch.float32)
    if bias is None:
        raise X2VError(f"{who}: bias is required")
    cu, batch = _cu_seqlens(cu_seqlens, qkv.shape[0], who)
    out = torch.empty((qkv.shape[0], D), dtype=torch.bfloat16, device=qkv.device) if out is None else _bf16rows(out, who + " out")
    if out.shape != (qkv.shape[0], D):
        raise X2VError(f"{who}: out must be [{qkv.shape[0]}, {D}]")
    init()
    _check(_lib.x2v_attn_bf16_d64_relbias(_p(qkv), qkv.stride(0), _p(bias), _p(out), out.stride(0), cu, batch, num_heads, float(scale), _stream()), who)
    return out


# ---- HunyuanVideo's text towers (fp16; csrc/txt_enc.hip) ------------------------------------------------------------------------------------------------
ATTN_CAUSAL_MAX_BATCH, ATTN_CAUSAL_MAX_LEN = 8, 512


def attention_f16_causal(qkv, cu_seqlens, num_heads, num_kv_heads, head_dim, rope=None, out=None, scale=0.0):
    """x2v_attn_f16_causal on the fused q | k | v GEMM output qkv [rows, (num_heads + 2 num_kv_heads) * head_dim] fp16 (read in place; a row stride beyond
    its columns is fine) -> [rows, num_heads * head_dim] fp16.  cu_seqlens: host ints, sequence b = rows cu[b] .. cu[b + 1] - 1.  rope: None or the
    (cos, sin) fp32 device tables [>= 512, head_dim / 2] (head_dim 128).  Rows outside every sequence are not written."""
    who = "attention_f16_causal"
    qkv = _f16rows(qkv, who + " qkv")
    D = num_heads * head_dim
    if qkv.shape[1] != (num_heads + 2 * num_kv_heads) * head_dim:
        raise X2VError(f"{who}: qkv {tuple(qkv.shape)} is not [rows, ({num_heads} + 2 * {num_kv_heads}) * {head_dim}] (q | k | v side by side; pass the whole rows)")
    cos = sin = None
    if rope is not None:
        cos, sin = (_vec(t, who + " rope table", None, dtype=torch.float32) for t in rope)
        if cos.numel() != sin.numel() or cos.numel() < ATTN_CAUSAL_MAX_LEN * (head_dim // 2):
            raise X2VError(f"{who}: the rope tables must both hold at least [{ATTN_CAUSAL_MAX_LEN}, {head_dim // 2}] fp32 values")
    cu, batch = _cu_seqlens(cu_seqlens, qkv.shape[0], who)
    out = torch.empty((qkv.shape[0], D), dtype=torch.float16, device=qkv.device) if out is None else _f16rows(out, who + " out")
    if out.shape != (qkv.shape[0], D):
        raise X2VError(f"{who}: out must be [{qkv.shape[0]}, {D}]")
    init()
    _check(_lib.x2v_attn_f16_causal(_p(qkv), qkv.stride(0), _p(out), out.stride(0), cu, batch, num_heads, num_kv_heads, head_dim, _p(cos), _p(sin), float(scale), _stream()), who)
    return out


def rmsnorm_f16(x, weight, eps=1e-5, out=None):
    """x2v_rmsnorm_f16: fp16 rows and weight, fp32 statistics, one rounding."""
    x = _f16rows(x, "rmsnorm_f16 x")
    D = x.shape[1]
    weight = _vec(weight, "rmsnorm_f16 weight", D, dtype=torch.float16)
    if weight is None:
        raise X2VError("rmsnorm_f16: weight is required")
    out = torch.empty_like(x) if out is None else _f16rows(out, "rmsnorm_f16 out")
    if out.shape != x.shape:
        raise X2VError(f"rmsnorm_f16: out must be {tuple(x.shape)}, got {tuple(out.shape)}")
    init()
    _check(_lib.x2v_rmsnorm_f16(_p(x), x.stride(0), _p(weight), _p(out), out.stride(0), x.shape[0], D, eps, _stream()), "rmsnorm_f16")
    return out
