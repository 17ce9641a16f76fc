// MXFP8 (OCP microscaling: e4m3 elements, one e8m0 power-of-two scale per 32 consecutive K elements) quantisation and GEMM on
// gfx950's native block-scaled matrix instruction — the counterpart of the reference's lightx2v_kernel package
//   scaled_fp8_quant            lightx2v_kernel/python/lightx2v_kernel/gemm.py:73-83, csrc/gemm/mxfp8_quant_kernels_sm120.cu:139-196
//   cutlass_scaled_mxfp8_mm     gemm.py:93-97, csrc/gemm/mxfp8_scaled_mm_kernels_sm120.cu:60-66,150-160  (D = alpha * A.B^T + bias[n], bf16)
//
// Scale layout: sc[K/128][rows][4] bytes — K-tile major, then operand row, then the 4 k blocks of that 128-wide K-tile.  Like the
// reference's [m/128][k/128][32][4][4] swizzle (the operand format of the sm120 tensor core) it is the consumer's format:
// v_mfma_scale_f32_32x32x64_f8f6f4 takes, per lane, the scale byte of that lane's operand row and 32-wide k block from a VGPR, so a
// GEMM wave needs one dword per row and K-tile, and with this layout the 32 rows of a fragment are 128 contiguous bytes (one cache
// line per load instead of 32 with a row-major [rows][K/32] table: 1.6-1.85 -> 2.4-2.7 PFLOP/s on the 14B shapes, profiles/r01_mxfp8_*).
//
// quant: HBM-bound — reads M*K bf16, writes M*K bytes + M*K/32 scale bytes (algorithmic bytes 3.03 per element).
// GEMM:  MFMA-bound — 2*M*N*K FLOP per launch against the 5 PFLOP/s fp8 peak.  Two bodies, both the MX mode of a kernel of the GEMM family: gemm.hip's
//        128x128-tile / two-barrier kernel (small shapes) and gemm256.hip's 256x256 ping-pong kernel (shapes that fill the chip, and every call
//        with a fused epilogue); gemm_mxfp8_impl chooses.  This file keeps the quantiser, the entries and their argument checks.
//
// MXFP6 weights x MXFP8 activations (e3m2 weights packed 4 codes to 3 bytes, the same e8m0 scale per 32 K elements) — the package's second MX path
//   scaled_fp6_quant                gemm.py:58-68, csrc/gemm/mxfp6_quant_kernels_sm120.cu:168-225
//   cutlass_scaled_mxfp6_mxfp8_mm   gemm.py:84-88, csrc/gemm/mxfp6_mxfp8_scaled_mm_kernels_sm120.cu:39-46
// is quant_mxfp6_kernel below and one more value (2) of the same two kernels' MX mode; gemm_mxfp6_impl chooses with the same rule.
// quant: HBM-bound — 2 + 0.75 + 1/32 bytes per element.  GEMM: MFMA-bound at the fp8 rate (one operand is e4m3).
//
// MXFP4 x MXFP4 (OCP e2m1 elements, two codes per byte, the same e8m0 scale per 32 K elements, weights and activations alike) fills the slot of the
// package's NVFP4 pair (scaled_fp4_quant / cutlass_scaled_fp4_mm: e4m3 scales per 16 elements plus a global scale, which the gfx950 instruction does
// not have) with the 4-bit format the hardware has: quant_mxfp4_kernel below and value 3 of the two kernels' MX mode; gemm_mxfp4_impl chooses with
// MXFP8's rule on the number of 128-byte K-tiles (K / 256).
// quant: HBM-bound — 2 + 0.5 + 1/32 bytes per element.  GEMM: MFMA-bound at twice the fp8 rate (both operands 4-bit).
#include "x2v_common.h"

namespace x2v {

// ------------------------------------------------------------------------------------------------ quantisation
// One lane = 8 consecutive elements (16 B in, 8 B out), 4 lanes = one 32-element scale block.
//   vecMax = max |x|;  SF = vecMax / 448;  scale byte = e8m0(SF) rounded towards +inf (smallest power of two >= SF), saturating;
//   q = e4m3fn_rne(x * 2^-(byte-127))   — |x| * 2^-e <= 448 by construction, so the conversion never saturates.
// An all-zero block gives byte 0 (2^-127) and zero elements (the reference's 0 * rcp(flushed denormal) = NaN there is not reproduced).
// e8m0_ceil lives in x2v_common.h (attn_mx.hip's quantisers use the same rule).

__global__ __launch_bounds__(256) void quant_mxfp8_kernel(const unsigned short* __restrict__ x, int64_t ldx, unsigned char* __restrict__ q, int64_t ldq,
                                                          unsigned* __restrict__ sc, int64_t M, int K) {
  const int kc = K >> 3;  // 16-byte chunks per row
  const int64_t total = M * kc;
  for (int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x; id < total + 3; id += (int64_t)gridDim.x * 256) {
    // the 16 lanes of one K-tile of one row (16 consecutive ids) are always all in range or all out of range (kc % 16 == 0)
    const bool ok = id < total;
    const int64_t row = ok ? id / kc : 0;
    const int c = ok ? (int)(id - row * kc) : 0;
    float v[8];
    float amax = 0.f;
    if (ok) {
      unpack8(*reinterpret_cast<const uint4*>(x + row * ldx + c * 8), v);
#pragma unroll
      for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(v[j]));
    }
    amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
    amax = fmaxf(amax, __shfl_xor(amax, 2, 64));
    if (!ok) continue;
    unsigned w[2];
    const unsigned byte = mxfp8_block<8>(v, amax, w);
    *reinterpret_cast<uint2*>(q + row * ldq + c * 8) = make_uint2(w[0], w[1]);
    // the 4 scale bytes of a row's K-tile sit in lanes c, c+4, c+8, c+12 (16 lanes = 128 elements)
    const unsigned dw = e8m0_gather4(byte, 4);
    if ((c & 15) == 0) sc[(int64_t)(c >> 4) * M + row] = dw;
  }
}

// MXFP6 (e3m2: 1 sign, 3 exponent bits of bias 3, 2 mantissa bits; subnormals m * 2^-4, largest number 28, no NaN / Inf) — the weight side of the
// reference's mxfp6 x mxfp8 product (csrc/gemm/mxfp6_quant_kernels_sm120.cu:168-225).  The scale rule is MXFP8's with 28 in place of 448.
// One lane = 16 consecutive elements (32 B in, 12 B = 16 codes of 6 bits out, the reference's dense little-endian string: code j of a row at bits
// 6 j .. 6 j + 5 of the row's bytes), 2 lanes = one scale block, 8 lanes = one K-tile of a row.
// |x| * 2^(127 - byte) <= 28 by construction; the clamp to 0x1f only keeps a NaN / Inf element (outside the contract) inside its 6 bits.
__device__ __forceinline__ unsigned e3m2_rne(float v) {
  const unsigned bits = __float_as_uint(v), sign = (bits >> 26) & 0x20u, mag = bits & 0x7fffffffu;
  unsigned code;
  if (mag >= 0x3e800000u) {  // >= 2^-2, the least normal: round the fp32 significand to 2 bits, ties to even; a carry moves into the exponent field
    code = ((mag + 0xfffffu + ((mag >> 21) & 1u)) >> 21) - (124u << 2);
    code = code > 0x1fu ? 0x1fu : code;
  } else {
    code = (unsigned)__builtin_rintf(__uint_as_float(mag) * 16.0f);  // steps of 2^-4; 4 is the least normal's code
  }
  return sign | code;
}

__global__ __launch_bounds__(256) void quant_mxfp6_kernel(const unsigned short* __restrict__ x, int64_t ldx, unsigned char* __restrict__ q, int64_t ldq,
                                                          unsigned* __restrict__ sc, int64_t M, int K) {
  const int kc = K >> 4;  // 32-byte chunks per row
  const int64_t total = M * kc;
  // the 8 lanes of one K-tile of one row (8 consecutive ids) are always all in range or all out of range (kc % 8 == 0)
  for (int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x; id < total; id += (int64_t)gridDim.x * 256) {
    const int64_t row = id / kc;
    const int c = (int)(id - row * kc);
    float v[16];
    unpack8(*reinterpret_cast<const uint4*>(x + row * ldx + c * 16), v);
    unpack8(*reinterpret_cast<const uint4*>(x + row * ldx + c * 16 + 8), v + 8);
    float amax = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) amax = fmaxf(amax, fabsf(v[j]));
    amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
    const unsigned byte = e8m0_ceil(amax / 28.0f);
    const float inv = e8m0_inv(byte);
    unsigned t[4];  // 4 codes = 24 bits
#pragma unroll
    for (int g = 0; g < 4; ++g)
      t[g] = e3m2_rne(v[4 * g] * inv) | (e3m2_rne(v[4 * g + 1] * inv) << 6) | (e3m2_rne(v[4 * g + 2] * inv) << 12) | (e3m2_rne(v[4 * g + 3] * inv) << 18);
    unsigned* dst = reinterpret_cast<unsigned*>(q + row * ldq + c * 12);
    dst[0] = t[0] | (t[1] << 24);
    dst[1] = (t[1] >> 8) | (t[2] << 16);
    dst[2] = (t[2] >> 16) | (t[3] << 8);
    // the 4 scale bytes of a row's K-tile sit in lanes c, c+2, c+4, c+6 (8 lanes = 128 elements)
    const unsigned dw = e8m0_gather4(byte, 2);
    if ((c & 7) == 0) sc[(int64_t)(c >> 3) * M + row] = dw;
  }
}

// MXFP4 (e2m1: 1 sign, 2 exponent bits of bias 1, 1 mantissa bit; magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6; no NaN / Inf).  The scale rule is MXFP8's
// with 6 in place of 448.  One lane = 16 consecutive elements (32 B in, 8 B = 16 codes of 4 bits out, the dense little-endian nibble string: code j
// of a row at bits 4 j .. 4 j + 3 of the row's bytes), 2 lanes = one scale block, 8 lanes = one 128-wide K-tile of the scale table.
// |x| * 2^(127 - byte) <= 6 by construction; the clamp to 7 only keeps a NaN / Inf element (outside the contract) inside its 4 bits.
__device__ __forceinline__ unsigned e2m1_rne(float v) {
  const unsigned bits = __float_as_uint(v), sign = (bits >> 28) & 0x8u, mag = bits & 0x7fffffffu;
  unsigned code;
  if (mag >= 0x3f800000u) {  // >= 1, the least normal: round the fp32 significand to 1 bit, ties to even; a carry moves into the exponent field
    code = ((mag + 0x1fffffu + ((mag >> 22) & 1u)) >> 22) - (126u << 1);
    code = code > 7u ? 7u : code;
  } else {
    code = (unsigned)__builtin_rintf(__uint_as_float(mag) * 2.0f);  // steps of 0.5; 2 is the least normal's code
  }
  return sign | code;
}

__global__ __launch_bounds__(256) void quant_mxfp4_kernel(const unsigned short* __restrict__ x, int64_t ldx, unsigned char* __restrict__ q, int64_t ldq,
                                                          unsigned* __restrict__ sc, int64_t M, int K) {
  const int kc = K >> 4;  // 32-byte chunks per row
  const int64_t total = M * kc;
  // the 8 lanes of one K-tile of one row (8 consecutive ids) are always all in range or all out of range (kc % 8 == 0)
  for (int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x; id < total; id += (int64_t)gridDim.x * 256) {
    const int64_t row = id / kc;
    const int c = (int)(id - row * kc);
    float v[16];
    unpack8(*reinterpret_cast<const uint4*>(x + row * ldx + c * 16), v);
    unpack8(*reinterpret_cast<const uint4*>(x + row * ldx + c * 16 + 8), v + 8);
    float amax = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) amax = fmaxf(amax, fabsf(v[j]));
    amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
    const unsigned byte = e8m0_ceil(amax / 6.0f);
    const float inv = e8m0_inv(byte);
    unsigned w[2] = {0u, 0u};
#pragma unroll
    for (int j = 0; j < 16; ++j) w[j >> 3] |= e2m1_rne(v[j] * inv) << (4 * (j & 7));
    *reinterpret_cast<uint2*>(q + row * ldq + c * 8) = make_uint2(w[0], w[1]);
    // the 4 scale bytes of a row's K-tile sit in lanes c, c+2, c+4, c+6 (8 lanes = 128 elements)
    const unsigned dw = e8m0_gather4(byte, 2);
    if ((c & 7) == 0) sc[(int64_t)(c >> 3) * M + row] = dw;
  }
}

// ------------------------------------------------------------------------------------------------ GEMM
// gemm.hip: the MX mode of the 128x128-tile kernel (small shapes, no fused epilogue)
int gemm128_mx_dispatch(const void* a, int64_t lda, const void* sa, const void* b, int64_t ldb, const void* sb, const void* bias, const float* alpha, void* y,
                        int64_t ldy, int64_t M, int N, int nk, hipStream_t st);
// gemm256.hip: the 256x256-tile ping-pong kernel with hardware block scales (large shapes)
int gemm256_mx_dispatch(int epilogue, const void* a, int64_t lda, const void* sa, const void* b, int64_t ldb, const void* sb, const void* bias, const float* alpha,
                        void* y, int64_t ldy, int64_t M, int N, int nk, const void* resid, int64_t ldr, const void* gate, hipStream_t st);

// the MXFP6-weight modes of the same two kernels
int gemm128_mx6_dispatch(const void* a, int64_t lda, const void* sa, const void* b, int64_t ldb, const void* sb, const void* bias, const float* alpha, void* y,
                         int64_t ldy, int64_t M, int N, int nk, hipStream_t st);
int gemm256_mx6_dispatch(int epilogue, const void* a, int64_t lda, const void* sa, const void* b, int64_t ldb, const void* sb, const void* bias, const float* alpha,
                         void* y, int64_t ldy, int64_t M, int N, int nk, const void* resid, int64_t ldr, const void* gate, hipStream_t st);

// the MXFP4 x MXFP4 modes of the same two kernels; nk counts K-tiles of 256 (128 bytes per operand row)
int gemm128_mx4_dispatch(const void* a, int64_t lda, const void* sa, const void* b, int64_t ldb, const void* sb, const void* bias, const float* alpha, void* y,
                         int64_t ldy, int64_t M, int N, int nk, hipStream_t st);
int gemm256_mx4_dispatch(int epilogue, const void* a, int64_t lda, const void* sa, const void* b, int64_t ldb, const void* sb, const void* bias, const float* alpha,
                         void* y, int64_t ldy, int64_t M, int N, int nk, const void* resid, int64_t ldr, const void* gate, hipStream_t st);

}  // namespace x2v

using namespace x2v;

extern "C" __attribute__((visibility("default"))) int x2v_quant_mxfp8_bf16(const void* x, int64_t ldx, void* q, int64_t ldq, void* scales, int64_t M, int K,
                                                                          void* stream) {
  X2V_REQUIRE(x && q && scales, X2V_E_ARG, "quant_mxfp8: null pointer");
  X2V_REQUIRE(K > 0 && K % 128 == 0, X2V_E_SHAPE, "quant_mxfp8: K=%d must be a multiple of 128 (4 scale blocks = one K-tile of the GEMM)", K);
  X2V_REQUIRE(ldx % 8 == 0 && ldq % 8 == 0 && ldx >= K && ldq >= K && aligned16(x) && ((uintptr_t)q % 8) == 0 && ((uintptr_t)scales % 4) == 0, X2V_E_ALIGN,
              "quant_mxfp8: rows must be 16-byte (input) / 8-byte (output) aligned, the scale table 4-byte aligned");
  if (M <= 0) return X2V_OK;
  const int64_t total = M * (K / 8);
  const unsigned blocks = (unsigned)std::min<int64_t>((total + 255) / 256, 256 * 32);
  hipLaunchKernelGGL(quant_mxfp8_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const unsigned short*)x, ldx, (unsigned char*)q, ldq,
                     (unsigned*)scales, M, K);
  X2V_LAUNCH_CHECK("quant_mxfp8 launch");
  return X2V_OK;
}

static int gemm_mxfp8_impl(const void* a, int64_t lda, const void* sa, const void* b, int64_t ldb, const void* sb, const void* bias, const float* alpha, void* y,
                           int64_t ldy, int64_t M, int N, int K, int variant, void* stream, int epilogue = X2V_EPI_NONE, const void* resid = nullptr,
                           int64_t ldr = 0, const void* gate = nullptr) {
  X2V_REQUIRE(a && sa && b && sb && y, X2V_E_ARG, "gemm_mxfp8: null pointer");
  X2V_REQUIRE(M > 0 && N > 0 && K > 0 && K % 128 == 0 && N % 8 == 0, X2V_E_SHAPE, "gemm_mxfp8: M=%lld N=%d K=%d (K %% 128 == 0, N %% 8 == 0)", (long long)M, N, K);
  X2V_REQUIRE(lda % 16 == 0 && ldb % 16 == 0 && lda >= K && ldb >= K && ldy % 8 == 0 && ldy >= N && aligned16(a) && aligned16(b) && aligned16(y) &&
                  ((uintptr_t)sa % 4) == 0 && ((uintptr_t)sb % 4) == 0,
              X2V_E_ALIGN, "gemm_mxfp8: operand rows 16-byte aligned, scale tables 4-byte aligned");
  X2V_REQUIRE((int64_t)(K / 128) * std::max<int64_t>(M, N) * 4 < (1ll << 32), X2V_E_SHAPE, "gemm_mxfp8: scale table of 4 GiB or more");
  // The kernel choice of the other GEMMs, asked of the same function (gemm.hip::choose_kernel behind x2v_gemm_kernel_choice; low byte 2 = the 256x256
  // ping-pong kernel: at least 192 tiles of 256x256, at least 8 K tiles, leading dimensions below 2^24 and tile spans below 2^32 bytes), else 128x128
  // tiles.  The operands here are unblocked and ld >= K is required above, so 255 * ld + K <= 256 * ld < 2^32 whenever ld < 2^24: the span condition
  // adds nothing to the leading-dimension one for MXFP8.
  // The fused epilogues (activation / gated residual) live in the 256x256 kernel only: any shape with one goes there.
  const bool big = variant == 2 || epilogue != X2V_EPI_NONE || (variant == 0 && (x2v_gemm_kernel_choice(M, N, K, lda, ldb, 1) & 0xff) == 2);
  if (epilogue == X2V_EPI_RESIDUAL)
    X2V_REQUIRE(resid != nullptr && ldr % 8 == 0 && ldr >= N && aligned16(resid) && (gate == nullptr || aligned16(gate)), X2V_E_ALIGN,
                "gemm_mxfp8: residual epilogue needs a 16-byte aligned residual (and gate)");
  if (big) return gemm256_mx_dispatch(epilogue, a, lda, sa, b, ldb, sb, bias, alpha, y, ldy, M, N, K / 128, resid, ldr, gate, (hipStream_t)stream);
  return gemm128_mx_dispatch(a, lda, sa, b, ldb, sb, bias, alpha, y, ldy, M, N, K / 128, (hipStream_t)stream);
}

extern "C" __attribute__((visibility("default"))) int x2v_gemm_mxfp8(const void* a, int64_t lda, const void* sa, const void* b, int64_t ldb, const void* sb,
                                                                    const void* bias, const float* alpha, void* y, int64_t ldy, int64_t M, int N, int K,
                                                                    void* stream) {
  return gemm_mxfp8_impl(a, lda, sa, b, ldb, sb, bias, alpha, y, ldy, M, N, K, 0, stream);
}

// variant: 0 = automatic, 1 = 128x128-tile kernel, 2 = 256x256-tile ping-pong kernel (tests and A/B measurements)
extern "C" __attribute__((visibility("default"))) int x2v_gemm_mxfp8_variant(const void* a, int64_t lda, const void* sa, const void* b, int64_t ldb, const void* sb,
                                                                            const void* bias, const float* alpha, void* y, int64_t ldy, int64_t M, int N, int K,
                                                                            int variant, void* stream) {
  X2V_REQUIRE(variant >= 0 && variant <= 2, X2V_E_ARG, "gemm_mxfp8: unknown variant %d", variant);
  return gemm_mxfp8_impl(a, lda, sa, b, ldb, sb, bias, alpha, y, ldy, M, N, K, variant, stream);
}

// With the fused epilogues of x2v_gemm_bf16 / x2v_gemm_fp8 (X2V_EPI_*): what the block drivers call for an MXFP8 linear layer.
extern "C" __attribute__((visibility("default"))) int x2v_gemm_mxfp8_epi(const void* a, int64_t lda, const void* sa, const void* b, int64_t ldb, const void* sb,
                                                                        const void* bias, const float* alpha, void* y, int64_t ldy, int64_t M, int N, int K,
                                                                        int epilogue, const void* resid, int64_t ldr, const void* gate, void* stream) {
  return gemm_mxfp8_impl(a, lda, sa, b, ldb, sb, bias, alpha, y, ldy, M, N, K, 0, stream, epilogue, resid, ldr, gate);
}

// ------------------------------------------------------------------------------------------------ MXFP6 weights x MXFP8 activations
extern "C" __attribute__((visibility("default"))) int x2v_quant_mxfp6_bf16(const void* x, int64_t ldx, void* q, int64_t ldq, void* scales, int64_t M, int K,
                                                                          void* stream) {
  X2V_REQUIRE(x && q && scales, X2V_E_ARG, "quant_mxfp6: null pointer");
  X2V_REQUIRE(K > 0 && K % 128 == 0, X2V_E_SHAPE, "quant_mxfp6: K=%d must be a multiple of 128 (4 scale blocks = one K-tile of the GEMM)", K);
  X2V_REQUIRE(ldx % 8 == 0 && ldq % 4 == 0 && ldx >= K && ldq >= K / 4 * 3 && aligned16(x) && ((uintptr_t)q % 4) == 0 && ((uintptr_t)scales % 4) == 0, X2V_E_ALIGN,
              "quant_mxfp6: rows must be 16-byte (input) / 4-byte (output, ldq >= 3K/4 bytes) aligned, the scale table 4-byte aligned");
  if (M <= 0) return X2V_OK;
  const int64_t total = M * (K / 16);
  const unsigned blocks = (unsigned)std::min<int64_t>((total + 255) / 256, 256 * 16);
  hipLaunchKernelGGL(quant_mxfp6_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const unsigned short*)x, ldx, (unsigned char*)q, ldq,
                     (unsigned*)scales, M, K);
  X2V_LAUNCH_CHECK("quant_mxfp6 launch");
  return X2V_OK;
}

// Two bodies, the MXM = 2 mode of gemm.hip's 128x128 kernel and of gemm256.hip's ping-pong kernel, chosen as for MXFP8 (gemm_mxfp8_impl): the
// 256x256 body where gemm.hip::choose_kernel gives an fp8 product of this shape to it, and for every call with a fused epilogue.
static int gemm_mxfp6_impl(const void* a, int64_t lda, const void* sa, const void* b, int64_t ldb, const void* sb, const void* bias, const float* alpha, void* y,
                           int64_t ldy, int64_t M, int N, int K, int variant, void* stream, int epilogue = X2V_EPI_NONE, const void* resid = nullptr,
                           int64_t ldr = 0, const void* gate = nullptr) {
  X2V_REQUIRE(a && sa && b && sb && y, X2V_E_ARG, "gemm_mxfp6_mxfp8: null pointer");
  X2V_REQUIRE(variant >= 0 && variant <= 2, X2V_E_ARG, "gemm_mxfp6_mxfp8: unknown variant %d", variant);
  X2V_REQUIRE(M > 0 && N > 0 && K > 0 && K % 128 == 0 && N % 8 == 0, X2V_E_SHAPE, "gemm_mxfp6_mxfp8: M=%lld N=%d K=%d (K %% 128 == 0, N %% 8 == 0)", (long long)M, N, K);
  X2V_REQUIRE(lda % 16 == 0 && lda >= K && aligned16(a) && ldb % 4 == 0 && ldb >= K / 4 * 3 && ((uintptr_t)b % 4) == 0 && ldy % 8 == 0 && ldy >= N && aligned16(y) &&
                  ((uintptr_t)sa % 4) == 0 && ((uintptr_t)sb % 4) == 0 && (bias == nullptr || ((uintptr_t)bias % 8) == 0),
              X2V_E_ALIGN, "gemm_mxfp6_mxfp8: rows of a and y 16-byte aligned, rows of b (3K/4 bytes) and the scale tables 4-byte aligned, bias 8-byte aligned");
  X2V_REQUIRE((int64_t)(K / 128) * std::max<int64_t>(M, N) * 4 < (1ll << 32), X2V_E_SHAPE, "gemm_mxfp6_mxfp8: scale table of 4 GiB or more");
  X2V_REQUIRE((M + 127) / 128 * (int64_t)((N + 127) / 128) < (1ll << 31), X2V_E_SHAPE, "gemm_mxfp6_mxfp8: too many tiles");
  if (epilogue == X2V_EPI_RESIDUAL) {
    X2V_REQUIRE(resid != nullptr, X2V_E_ARG, "gemm_mxfp6_mxfp8: residual epilogue needs resid");
    X2V_REQUIRE(ldr % 8 == 0 && ldr >= N && aligned16(resid) && (gate == nullptr || aligned16(gate)), X2V_E_ALIGN,
                "gemm_mxfp6_mxfp8: residual epilogue needs a 16-byte aligned residual (and gate)");
  }
  // lda >= K > ldb's 3K/4: the choice asked for (lda, lda) covers the span condition of both operands
  const bool big = variant == 2 || epilogue != X2V_EPI_NONE || (variant == 0 && ldb < (1 << 24) && (x2v_gemm_kernel_choice(M, N, K, lda, lda, 1) & 0xff) == 2);
  if (big) {
    X2V_REQUIRE(lda < (1 << 24) && ldb < (1 << 24), X2V_E_SHAPE, "gemm_mxfp6_mxfp8: leading dimension too large for the 256x256 kernel (32-bit tile addressing)");
    return gemm256_mx6_dispatch(epilogue, a, lda, sa, b, ldb, sb, bias, alpha, y, ldy, M, N, K / 128, resid, ldr, gate, (hipStream_t)stream);
  }
  return gemm128_mx6_dispatch(a, lda, sa, b, ldb, sb, bias, alpha, y, ldy, M, N, K / 128, (hipStream_t)stream);
}

extern "C" __attribute__((visibility("default"))) int x2v_gemm_mxfp6_mxfp8(const void* a, int64_t lda, const void* sa, const void* b, int64_t ldb, const void* sb,
                                                                          const void* bias, const float* alpha, void* y, int64_t ldy, int64_t M, int N, int K,
                                                                          void* stream) {
  return gemm_mxfp6_impl(a, lda, sa, b, ldb, sb, bias, alpha, y, ldy, M, N, K, 0, stream);
}

// variant: 0 = automatic, 1 = 128x128-tile kernel, 2 = 256x256-tile ping-pong kernel (tests and A/B measurements)
extern "C" __attribute__((visibility("default"))) int x2v_gemm_mxfp6_mxfp8_variant(const void* a, int64_t lda, const void* sa, const void* b, int64_t ldb, const void* sb,
                                                                                  const void* bias, const float* alpha, void* y, int64_t ldy, int64_t M, int N,
                                                                                  int K, int variant, void* stream) {
  return gemm_mxfp6_impl(a, lda, sa, b, ldb, sb, bias, alpha, y, ldy, M, N, K, variant, stream);
}

extern "C" __attribute__((visibility("default"))) int x2v_gemm_mxfp6_mxfp8_epi(const void* a, int64_t lda, const void* sa, const void* b, int64_t ldb, const void* sb,
                                                                              const void* bias, const float* alpha, void* y, int64_t ldy, int64_t M, int N, int K,
                                                                              int epilogue, const void* resid, int64_t ldr, const void* gate, void* stream) {
  return gemm_mxfp6_impl(a, lda, sa, b, ldb, sb, bias, alpha, y, ldy, M, N, K, 0, stream, epilogue, resid, ldr, gate);
}

// ------------------------------------------------------------------------------------------------ MXFP4 x MXFP4
extern "C" __attribute__((visibility("default"))) int x2v_quant_mxfp4_bf16(const void* x, int64_t ldx, void* q, int64_t ldq, void* scales, int64_t M, int K,
                                                                          void* stream) {
  X2V_REQUIRE(x && q && scales, X2V_E_ARG, "quant_mxfp4: null pointer");
  X2V_REQUIRE(K > 0 && K % 128 == 0, X2V_E_SHAPE, "quant_mxfp4: K=%d must be a multiple of 128 (4 scale blocks = one dword of the scale table)", K);
  X2V_REQUIRE(ldx % 8 == 0 && ldq % 8 == 0 && ldx >= K && ldq >= K / 2 && aligned16(x) && ((uintptr_t)q % 8) == 0 && ((uintptr_t)scales % 4) == 0, X2V_E_ALIGN,
              "quant_mxfp4: rows must be 16-byte (input) / 8-byte (output, ldq >= K/2 bytes) aligned, the scale table 4-byte aligned");
  if (M <= 0) return X2V_OK;
  const int64_t total = M * (K / 16);
  const unsigned blocks = (unsigned)std::min<int64_t>((total + 255) / 256, 256 * 16);
  hipLaunchKernelGGL(quant_mxfp4_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const unsigned short*)x, ldx, (unsigned char*)q, ldq,
                     (unsigned*)scales, M, K);
  X2V_LAUNCH_CHECK("quant_mxfp4 launch");
  return X2V_OK;
}

// Two bodies, the MXM = 3 mode of gemm.hip's 128x128 kernel and of gemm256.hip's ping-pong kernel.  A 128-byte operand row per stage holds 256 k, so
// the rule of gemm_mxfp8_impl (gemm.hip::choose_kernel: at least 192 tiles of 256x256, leading dimensions below 2^24 bytes) is asked for the byte
// image, K / 2 bytes per row = K / 256 K-tiles — with 6 K-tiles where MXFP8 wants 8: at 20280 x 1536 -> 8960 (6 K-tiles, the K of every 1.3B block
// linear but one) the 256x256 body measured 2803 TFLOP/s against the 128x128 body's 2376 (profiles/mxfp4_bench.json; MXFP8 at its 12 K-tiles of
// the same shape: 1964 against 1682).  Every call with a fused epilogue goes to the 256x256 body.
static int gemm_mxfp4_impl(const void* a, int64_t lda, const void* sa, const void* b, int64_t ldb, const void* sb, const void* bias, const float* alpha, void* y,
                           int64_t ldy, int64_t M, int N, int K, int variant, void* stream, int epilogue = X2V_EPI_NONE, const void* resid = nullptr,
                           int64_t ldr = 0, const void* gate = nullptr) {
  X2V_REQUIRE(a && sa && b && sb && y, X2V_E_ARG, "gemm_mxfp4: null pointer");
  X2V_REQUIRE(variant >= 0 && variant <= 2, X2V_E_ARG, "gemm_mxfp4: unknown variant %d", variant);
  X2V_REQUIRE(M > 0 && N > 0 && K > 0 && K % 256 == 0 && N % 8 == 0, X2V_E_SHAPE, "gemm_mxfp4: M=%lld N=%d K=%d (K %% 256 == 0, N %% 8 == 0)", (long long)M, N, K);
  X2V_REQUIRE(lda % 16 == 0 && ldb % 16 == 0 && lda >= K / 2 && ldb >= K / 2 && ldy % 8 == 0 && ldy >= N && aligned16(a) && aligned16(b) && aligned16(y) &&
                  ((uintptr_t)sa % 4) == 0 && ((uintptr_t)sb % 4) == 0 && (bias == nullptr || ((uintptr_t)bias % 8) == 0),
              X2V_E_ALIGN, "gemm_mxfp4: rows of a, b (K/2 bytes, lda / ldb in bytes) and y 16-byte aligned, scale tables 4-byte aligned, bias 8-byte aligned");
  X2V_REQUIRE((int64_t)(K / 128) * std::max<int64_t>(M, N) * 4 < (1ll << 32), X2V_E_SHAPE, "gemm_mxfp4: scale table of 4 GiB or more");
  X2V_REQUIRE((M + 127) / 128 * (int64_t)((N + 127) / 128) < (1ll << 31), X2V_E_SHAPE, "gemm_mxfp4: too many tiles");
  if (epilogue == X2V_EPI_RESIDUAL) {
    X2V_REQUIRE(resid != nullptr, X2V_E_ARG, "gemm_mxfp4: residual epilogue needs resid");
    X2V_REQUIRE(ldr % 8 == 0 && ldr >= N && aligned16(resid) && (gate == nullptr || aligned16(gate)), X2V_E_ALIGN,
                "gemm_mxfp4: residual epilogue needs a 16-byte aligned residual (and gate)");
  }
  // ld >= K / 2 is required above, so 255 * ld + K / 2 <= 256 * ld < 2^32 whenever ld < 2^24: the span condition adds nothing (as for MXFP8)
  const bool big = variant == 2 || epilogue != X2V_EPI_NONE ||
                   (variant == 0 && lda < (1 << 24) && ldb < (1 << 24) && ((M + 255) / 256) * (int64_t)((N + 255) / 256) >= 192 && K / 256 >= 6);
  if (big) {
    X2V_REQUIRE(lda < (1 << 24) && ldb < (1 << 24), X2V_E_SHAPE, "gemm_mxfp4: leading dimension too large for the 256x256 kernel (32-bit tile addressing)");
    return gemm256_mx4_dispatch(epilogue, a, lda, sa, b, ldb, sb, bias, alpha, y, ldy, M, N, K / 256, resid, ldr, gate, (hipStream_t)stream);
  }
  return gemm128_mx4_dispatch(a, lda, sa, b, ldb, sb, bias, alpha, y, ldy, M, N, K / 256, (hipStream_t)stream);
}

extern "C" __attribute__((visibility("default"))) int x2v_gemm_mxfp4(const void* a, int64_t lda, const void* sa, const void* b, int64_t ldb, const void* sb,
                                                                    const void* bias, const float* alpha, void* y, int64_t ldy, int64_t M, int N, int K,
                                                                    void* stream) {
  return gemm_mxfp4_impl(a, lda, sa, b, ldb, sb, bias, alpha, y, ldy, M, N, K, 0, stream);
}

// variant: 0 = automatic, 1 = 128x128-tile kernel, 2 = 256x256-tile ping-pong kernel (tests and A/B measurements)
extern "C" __attribute__((visibility("default"))) int x2v_gemm_mxfp4_variant(const void* a, int64_t lda, const void* sa, const void* b, int64_t ldb, const void* sb,
                                                                            const void* bias, const float* alpha, void* y, int64_t ldy, int64_t M, int N, int K,
                                                                            int variant, void* stream) {
  return gemm_mxfp4_impl(a, lda, sa, b, ldb, sb, bias, alpha, y, ldy, M, N, K, variant, stream);
}

extern "C" __attribute__((visibility("default"))) int x2v_gemm_mxfp4_epi(const void* a, int64_t lda, const void* sa, const void* b, int64_t ldb, const void* sb,
                                                                        const void* bias, const float* alpha, void* y, int64_t ldy, int64_t M, int N, int K,
                                                                        int epilogue, const void* resid, int64_t ldr, const void* gate, void* stream) {
  return gemm_mxfp4_impl(a, lda, sa, b, ldb, sb, bias, alpha, y, ldy, M, N, K, 0, stream, epilogue, resid, ldr, gate);
}
