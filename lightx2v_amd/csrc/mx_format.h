// The MX linear-layer formats (OCP microscaling: one e8m0 scale per 32 consecutive K elements), one row each.  mx.hip's quantiser, its argument
// checks and its body rule, and the MX dispatch of gemm.hip and gemm256.hip read this table; a further format is a further row (and a further
// value of the two GEMM kernels' MXM mode), not a further copy of that code.
#pragma once

namespace x2v {

struct MxFormat {
  const char* gemm_name;   // the names that open the entries' messages
  const char* quant_name;
  int mxm;                 // the MXM template value of gemm_kernel / gemm256_kernel, and `format` of x2v_gemm_mx_kernel_choice
  int bits_a, bits_b;      // element bits of the GEMM's a (activations) and b (weights); a row of K elements is K * bits / 8 bytes
  int k_tile;              // k-values per 128-byte stage row of a (one K-tile of the GEMM kernels): what K must be a multiple of
  int min_ktiles_256;      // K-tiles from which the 256x256 body is worth its pipeline
  // the quantiser x2v_quant_<format>_bf16 writes elements of bits_b bits (largest magnitude 448, 28, 6: in the kernels' text, mx.hip)
  int q_elems;             // consecutive elements per lane (8 or 16)
  int q_align;             // alignment of q and ldq in bytes: a lane's codes leave as one 8-byte store or as dwords
  int q_max_blocks;        // grid cap (workgroups of 256 lanes; the kernel strides over the rest)
  constexpr int q_bytes() const { return q_elems * bits_b / 8; }  // output bytes per lane
};

// MXFP4 wants 6 K-tiles where the others want 8: at 20280 x 1536 -> 8960 (6 K-tiles of 256, the K of every 1.3B block linear but one) the 256x256
// body measured 2803 TFLOP/s against the 128x128 body's 2376 (profiles/mxfp4_bench.json; MXFP8 at its 12 K-tiles of that shape: 1964 against 1682).
constexpr MxFormat kMxFormats[] = {
    {"gemm_mxfp8", "quant_mxfp8", 1, 8, 8, 128, 8, 8, 8, 256 * 32},   // e4m3 x e4m3
    {"gemm_mxfp6_mxfp8", "quant_mxfp6", 2, 8, 6, 128, 8, 16, 4, 256 * 16},  // e4m3 activations x e3m2 weights (4 codes in 3 bytes)
    {"gemm_mxfp4", "quant_mxfp4", 3, 4, 4, 256, 6, 16, 8, 256 * 16},  // e2m1 x e2m1 (two codes per byte)
};
constexpr int kMxFormatCount = sizeof(kMxFormats) / sizeof(kMxFormats[0]);
constexpr const MxFormat& mx_format(int mxm) { return kMxFormats[mxm - 1]; }
static_assert(mx_format(1).mxm == 1 && mx_format(2).mxm == 2 && mx_format(3).mxm == 3 && kMxFormatCount == 3, "row i holds MXM = i + 1");

// Alignment of a GEMM operand's rows (pointer and leading dimension, bytes): the kernels stage 16-byte pieces, 12-byte ones of a 6-bit row
constexpr int mx_row_align(int bits) { return bits == 6 ? 4 : 16; }

}  // namespace x2v
