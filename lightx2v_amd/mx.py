"""MXFP8 quantise + GEMM with the call signatures of the reference's `lightx2v_kernel.gemm` module
(lightx2v_kernel/python/lightx2v_kernel/gemm.py:73-83 `scaled_fp8_quant`, :93-97 `cutlass_scaled_mxfp8_mm`), on gfx950's block-scaled
MFMA.  One difference a caller can see: the scale tensor is the `[K/128, rows, 4]` e8m0 table of this GEMM (K-tile major), not the
reference's `[ceil128(rows), ceil4(K/32)]` sm120-swizzled int32 view — either way it is the consumer's format and callers pass it
straight back to the GEMM (`lib.mx_scales_rowmajor` gives the logical [rows, K/32] table).  K must be a multiple of 128.

    a_q, a_s = scaled_fp8_quant(activation)          # bf16 [m, k] -> e4m3 bytes [m, k], e8m0 [k/128, m, 4]
    w_q, w_s = scaled_fp8_quant(weight)              # [n, k]
    y = cutlass_scaled_mxfp8_mm(a_q, w_q, a_s, w_s, alpha=alpha, bias=bias)   # bf16 [m, n]

The package's 4-bit pair, `scaled_fp4_quant(input, input_global_scale)` / `cutlass_scaled_fp4_mm`, is NOT mirrored under its names: it is NVFP4 (e2m1
elements with one e4m3 scale per 16 elements plus a global fp32 scale), and gfx950's block-scaled matrix instruction applies one e8m0 scale per
32 elements and nothing else.  The w4a4 slot is filled by MXFP4 x MXFP4 under names of its own, `scaled_mxfp4_quant` / `scaled_mxfp4_mm` below:
the same e2m1 elements and rounding table, the scale format the hardware has.
"""
import torch

from . import lib

_E8M0 = getattr(torch, "float8_e8m0fnu", None)


def _e8m0(scales):
    """The scale bytes as torch's e8m0 dtype, where this torch has it."""
    return scales.view(_E8M0) if _E8M0 is not None else scales


def _bytes(scales):
    return scales.view(torch.uint8) if scales.dtype != torch.uint8 else scales


def _mm(gemm, mat_a, mat_b, scales_a, scales_b, alpha, bias):
    return gemm(mat_a, _bytes(scales_a), mat_b, _bytes(scales_b), alpha=alpha, bias=None if bias is None else bias.reshape(-1))


def scaled_fp8_quant(input: torch.Tensor):
    q, sc = lib.quant_mxfp8(input)
    return q.view(torch.uint8), _e8m0(sc)


def cutlass_scaled_mxfp8_mm(mat_a, mat_b, scales_a, scales_b, alpha, bias=None):
    return _mm(lib.gemm_mxfp8, mat_a, mat_b, scales_a, scales_b, alpha, bias)


scaled_mxfp8_mm = cutlass_scaled_mxfp8_mm  # the name without the CUDA library in it


# ---- MXFP6 weights x MXFP8 activations (gemm.py:58-68 `scaled_fp6_quant`, :84-88 `cutlass_scaled_mxfp6_mxfp8_mm`): A = e4m3 activations of
#      scaled_fp8_quant, B = e3m2 weights packed 4 codes to 3 bytes (uint8 [n, 3k/4], the reference's layout), both with the e8m0 table above.
#
#     w_q, w_s = scaled_fp6_quant(weight)              # bf16 [n, k] -> uint8 [n, 3k/4], e8m0 [k/128, n, 4]
#     a_q, a_s = scaled_fp8_quant(activation)
#     y = cutlass_scaled_mxfp6_mxfp8_mm(a_q, w_q, a_s, w_s, alpha=alpha, bias=bias)
def scaled_fp6_quant(input: torch.Tensor):
    q, sc = lib.quant_mxfp6(input)
    return q, _e8m0(sc)


def cutlass_scaled_mxfp6_mxfp8_mm(mat_a, mat_b, scales_a, scales_b, alpha, bias=None):
    return _mm(lib.gemm_mxfp6_mxfp8, mat_a, mat_b, scales_a, scales_b, alpha, bias)


scaled_mxfp6_mxfp8_mm = cutlass_scaled_mxfp6_mxfp8_mm


# ---- MXFP4 x MXFP4: the w4a4 slot.  The reference's `scaled_fp4_quant(input, input_global_scale)` / `cutlass_scaled_fp4_mm` (gemm.py) are NVFP4:
#      e2m1 elements with one e4m3 scale per 16 elements plus a global fp32 scale.  gfx950's matrix instruction applies one e8m0 scale per 32
#      elements and nothing else, so those two names are NOT aliased here: a tensor quantised for one format is garbage to the other.  What runs is
#      MXFP4 (OCP: e2m1 elements, two codes per byte, code j of a row at bits 4j .. 4j+3, the e8m0 table above), activations and weights alike.
#      K must be a multiple of 256.
#
#     w_q, w_s = scaled_mxfp4_quant(weight)            # bf16 [n, k] -> uint8 [n, k/2], e8m0 [k/128, n, 4]
#     a_q, a_s = scaled_mxfp4_quant(activation)
#     y = scaled_mxfp4_mm(a_q, w_q, a_s, w_s, alpha=alpha, bias=bias)
def scaled_mxfp4_quant(input: torch.Tensor):
    q, sc = lib.quant_mxfp4(input)
    return q, _e8m0(sc)


def scaled_mxfp4_mm(mat_a, mat_b, scales_a, scales_b, alpha, bias=None):
    return _mm(lib.gemm_mxfp4, mat_a, mat_b, scales_a, scales_b, alpha, bias)
