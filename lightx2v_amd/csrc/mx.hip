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
//        with a fused epilogue); mx_body is the rule.  This file keeps ONE quantiser kernel, ONE quantiser entry body, ONE GEMM entry body with the
//        argument checks and ONE body rule for the three formats below; what differs between them is a row of kMxFormats (mx_format.h).
//
// MXFP6 weights x MXFP8 activations (e3m2 weights packed 4 codes to 3 bytes, the same e8m0 scale per 32 K elements) — the package's second MX path
//   scaled_fp6_quant                gemm.py:58-68, csrc/gemm/mxfp6_quant_kernels_sm120.cu:168-225
//   cutlass_scaled_mxfp6_mxfp8_mm   gemm.py:84-88, csrc/gemm/mxfp6_mxfp8_scaled_mm_kernels_sm120.cu:39-46
// is quant_mx_kernel<2> below and one more value (2) of the same two kernels' MX mode.
// quant: HBM-bound — 2 + 0.75 + 1/32 bytes per element.  GEMM: MFMA-bound at the fp8 rate (one operand is e4m3).
//
// MXFP4 x MXFP4 (OCP e2m1 elements, two codes per byte, the same e8m0 scale per 32 K elements, weights and activations alike) fills the slot of the
// package's NVFP4 pair (scaled_fp4_quant / cutlass_scaled_fp4_mm: e4m3 scales per 16 elements plus a global scale, which the gfx950 instruction does
// not have) with the 4-bit format the hardware has: quant_mx_kernel<3> below and value 3 of the two kernels' MX mode; the body rule counts its
// 128-byte K-tiles (K / 256).
// quant: HBM-bound — 2 + 0.5 + 1/32 bytes per element.  GEMM: MFMA-bound at twice the fp8 rate (both operands 4-bit).
#include "gemm256_pipe.h"  // MxFormat (mx_format.h), the two MX dispatch entries

namespace x2v {

// ------------------------------------------------------------------------------------------------ quantisation
// One kernel template, quant_mx_kernel<MXM>, with the format's constants from kMxFormats (QMAX = largest magnitude of the element format).  Per
// 32-element block
//   vecMax = max |x|;  SF = vecMax / QMAX;  scale byte = e8m0(SF) rounded towards +inf (smallest power of two >= SF), saturating;
//   code = rne(x * 2^-(byte-127))   — |x| * 2^-e <= QMAX by construction, so the conversion never saturates.
// An all-zero block gives byte 0 (2^-127) and zero elements (the reference's 0 * rcp(flushed denormal) = NaN there is not reproduced).
// e8m0_ceil and mxfp8_block live in x2v_common.h (attn_mx.hip's quantisers use the same rule).  The element encoders of the two narrow formats:

// MXFP6 (e3m2: 1 sign, 3 exponent bits of bias 3, 2 mantissa bits; subnormals m * 2^-4, largest number 28, no NaN / Inf) — the weight side of the
// reference's mxfp6 x mxfp8 product (csrc/gemm/mxfp6_quant_kernels_sm120.cu:168-225).
// The clamp to 0x1f only keeps a NaN / Inf element (outside the contract) inside its 6 bits.
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

// MXFP4 (e2m1: 1 sign, 2 exponent bits of bias 1, 1 mantissa bit; magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6; no NaN / Inf).
// The clamp to 7 only keeps a NaN / Inf element (outside the contract) inside its 4 bits.
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

// The skeleton, as MXFP8 instantiates it (QMAX = 448 inside mxfp8_block): one lane = E consecutive elements (2 E bytes in, E out), 32 / E lanes =
// one scale block, 128 / E lanes = one 128-element K-tile of a row (one dword of the scale table).
template <int MXM>
__global__ __launch_bounds__(256) void quant_mx_kernel(const unsigned short* __restrict__ x, int64_t ldx, unsigned char* __restrict__ q, int64_t ldq,
                                                       unsigned* __restrict__ sc, int64_t M, int K) {
  constexpr int BITS = mx_format(MXM).bits_b, E = mx_format(MXM).q_elems, OUT = mx_format(MXM).q_bytes();
  constexpr int LOG_E = E == 8 ? 3 : 4, LOG_TILE = 7 - LOG_E;  // log2 of E and of the lanes per K-tile
  static_assert(BITS == 8 && (E == 8 || E == 16), "the skeleton with the e4m3 block step; the 6- and 4-bit formats are the specialisations below");
  const int kc = K >> LOG_E;  // lanes per row
  const int64_t total = M * kc;
  // K % 128 == 0 makes total a multiple of the 128 / E lanes of one K-tile of one row, and the grid stride is a multiple of 256: those lanes
  // (consecutive ids) are always all in range or all out of range, so the shuffles below never meet a lane that left the loop
  for (int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x; id < total; id += (int64_t)gridDim.x * 256) {
    const int64_t row = id / kc;
    const int c = (int)(id - row * kc);
    float v[E];
#pragma unroll
    for (int j = 0; j < E; j += 8) unpack8(*reinterpret_cast<const uint4*>(x + row * ldx + c * E + j), v + j);
    float amax = 0.f;
#pragma unroll
    for (int j = 0; j < E; ++j) amax = fmaxf(amax, fabsf(v[j]));
#pragma unroll
    for (int o = 1; o < 32 / E; o <<= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
    unsigned w[OUT / 4];
    const unsigned byte = mxfp8_block<E>(v, amax, w);  // scale byte and the hardware's e4m3 conversion
    *reinterpret_cast<uint2*>(q + row * ldq + c * OUT) = make_uint2(w[0], w[1]);
    // the 4 scale bytes of a row's K-tile sit in lanes c, c + 32 / E, .. of its 128 / E lanes
    const unsigned dw = e8m0_gather4(byte, 32 / E);
    if ((c & ((1 << LOG_TILE) - 1)) == 0) sc[(int64_t)(c >> LOG_TILE) * M + row] = dw;
  }
}

// The e3m2 and e2m1 quantisers through the skeleton above (E = 16, their encoder and packer in the place of mxfp8_block) wrote the same bytes but
// came out 0.1 us and 0.2 us slower at 20 280 x 1536 (18.9 and 17.7 us; parent spread 0.05 us) with the packing's ORs scheduled in another order
// (profiles/mx_unify.txt, profiles/mx_unify_isa.txt), so they keep their own text, whose instruction streams are the earlier kernels':
// one lane = 16 consecutive elements (32 B in), 2 lanes = one scale block, 8 lanes = one K-tile of a row (kc % 8 == 0: those 8 consecutive ids
// are always all in range or all out of range).
// MXFP6: 12 B = 16 codes of 6 bits out, the reference's dense little-endian string: code j of a row at bits 6 j .. 6 j + 5 of the row's bytes.
template <>
__global__ __launch_bounds__(256) void quant_mx_kernel<2>(const unsigned short* __restrict__ x, int64_t ldx, unsigned char* __restrict__ q, int64_t ldq,
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

// MXFP4: 8 B = 16 codes of 4 bits out, the dense little-endian nibble string: code j of a row at bits 4 j .. 4 j + 3 of the row's bytes.
template <>
__global__ __launch_bounds__(256) void quant_mx_kernel<3>(const unsigned short* __restrict__ x, int64_t ldx, unsigned char* __restrict__ q, int64_t ldq,
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

}  // namespace x2v

using namespace x2v;

// x2v_quant_<format>_bf16: accepts and rejects per format what the table says (ldq and q's alignment, the row's bytes)
template <int MXM>
static int quant_mx_entry(const void* x, int64_t ldx, void* q, int64_t ldq, void* scales, int64_t M, int K, void* stream) {
  constexpr MxFormat f = mx_format(MXM);
  X2V_REQUIRE(x && q && scales, X2V_E_ARG, "%s: null pointer", f.quant_name);
  X2V_REQUIRE(K > 0 && K % 128 == 0, X2V_E_SHAPE, "%s: K=%d must be a multiple of 128 (4 scale blocks = one dword of the scale table)", f.quant_name, K);
  X2V_REQUIRE(ldx % 8 == 0 && ldq % f.q_align == 0 && ldx >= K && ldq >= K / 8 * f.bits_b && aligned16(x) && ((uintptr_t)q % f.q_align) == 0 &&
                  ((uintptr_t)scales % 4) == 0,
              X2V_E_ALIGN, "%s: rows must be 16-byte (input) / %d-byte (output, ldq >= %d K / 8 bytes) aligned, the scale table 4-byte aligned", f.quant_name,
              f.q_align, f.bits_b);
  if (M <= 0) return X2V_OK;
  const int64_t total = M * (K / f.q_elems);
  const unsigned blocks = (unsigned)std::min<int64_t>((total + 255) / 256, f.q_max_blocks);
  hipLaunchKernelGGL(quant_mx_kernel<MXM>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const unsigned short*)x, ldx, (unsigned char*)q, ldq,
                     (unsigned*)scales, M, K);
  X2V_LAUNCH_CHECK(f.quant_name);
  return X2V_OK;
}

// ------------------------------------------------------------------------------------------------ GEMM
// The body variant 0 takes without a fused epilogue, 2 = the 256x256 ping-pong kernel, 1 = 128x128 tiles: gemm.hip::choose_kernel's rule for an fp8
// product (at least 192 tiles of 256x256, leading dimensions below 2^24 bytes, tile spans below 2^32 bytes) on the byte image of the operands —
// a 128-byte stage row holds f.k_tile k-values — from f.min_ktiles_256 K-tiles on.  The operands are unblocked and ld >= the row's bytes is
// required by every caller, so 255 * ld + the row's bytes <= 256 * ld < 2^32 whenever ld < 2^24: the span condition adds nothing to the
// leading-dimension one.  For MXFP8 and MXFP6 this is x2v_gemm_kernel_choice(M, N, K, lda, ., 1) == 2 (tests/test_mx_ref_host.py sweeps the edges).
static int mx_body(const MxFormat& f, int64_t M, int N, int K, int64_t lda, int64_t ldb) {
  const int64_t tiles256 = ((M + 255) / 256) * (int64_t)((N + 255) / 256);
  return tiles256 >= 192 && lda < (1 << 24) && ldb < (1 << 24) && K / f.k_tile >= f.min_ktiles_256 ? 2 : 1;
}

// variant: 0 = automatic, 1 = 128x128-tile kernel, 2 = 256x256-tile ping-pong kernel (tests and A/B measurements).  The fused epilogues
// (activation / gated residual) live in the 256x256 kernel only: any shape with one goes there.
static int gemm_mx_impl(const MxFormat& f, const void* a, int64_t lda, const void* sa, const void* b, int64_t ldb, const void* sb, const void* bias,
                        const float* alpha, void* y, int64_t ldy, int64_t M, int N, int K, int variant, void* stream, int epilogue = X2V_EPI_NONE,
                        const void* resid = nullptr, int64_t ldr = 0, const void* gate = nullptr) {
  const char* who = f.gemm_name;
  const int align_a = mx_row_align(f.bits_a), align_b = mx_row_align(f.bits_b);
  X2V_REQUIRE(a && sa && b && sb && y, X2V_E_ARG, "%s: null pointer", who);
  X2V_REQUIRE(variant >= 0 && variant <= 2, X2V_E_ARG, "%s: unknown variant %d", who, variant);
  X2V_REQUIRE(M > 0 && N > 0 && K > 0 && K % f.k_tile == 0 && N % 8 == 0, X2V_E_SHAPE, "%s: M=%lld N=%d K=%d (K %% %d == 0, N %% 8 == 0)", who, (long long)M, N, K,
              f.k_tile);
  X2V_REQUIRE(lda % align_a == 0 && lda >= K / 8 * f.bits_a && ((uintptr_t)a % align_a) == 0 && ldb % align_b == 0 && ldb >= K / 8 * f.bits_b &&
                  ((uintptr_t)b % align_b) == 0 && ldy % 8 == 0 && ldy >= N && aligned16(y) && ((uintptr_t)sa % 4) == 0 && ((uintptr_t)sb % 4) == 0 &&
                  (bias == nullptr || ((uintptr_t)bias % 8) == 0),
              X2V_E_ALIGN, "%s: rows of a (%d K / 8 bytes, lda in bytes) %d-byte, of b (%d K / 8 bytes, ldb in bytes) %d-byte and of y 16-byte aligned, scale tables 4-byte, bias 8-byte aligned",
              who, f.bits_a, align_a, f.bits_b, align_b);
  X2V_REQUIRE((int64_t)(K / 128) * std::max<int64_t>(M, N) * 4 < (1ll << 32), X2V_E_SHAPE, "%s: scale table of 4 GiB or more", who);
  X2V_REQUIRE((M + 127) / 128 * (int64_t)((N + 127) / 128) < (1ll << 31), X2V_E_SHAPE, "%s: too many tiles", who);
  if (epilogue == X2V_EPI_RESIDUAL) {
    X2V_REQUIRE(resid != nullptr, X2V_E_ARG, "%s: residual epilogue needs resid", who);
    X2V_REQUIRE(ldr % 8 == 0 && ldr >= N && aligned16(resid) && (gate == nullptr || aligned16(gate)), X2V_E_ALIGN,
                "%s: residual epilogue needs a 16-byte aligned residual (and gate)", who);
  }
  const int nk = K / f.k_tile;
  if (variant == 2 || epilogue != X2V_EPI_NONE || (variant == 0 && mx_body(f, M, N, K, lda, ldb) == 2)) {
    X2V_REQUIRE(lda < (1 << 24) && ldb < (1 << 24), X2V_E_SHAPE, "%s: leading dimension too large for the 256x256 kernel (32-bit tile addressing)", who);
    return gemm256_mx_dispatch(f, epilogue, a, lda, sa, b, ldb, sb, bias, alpha, y, ldy, M, N, nk, resid, ldr, gate, (hipStream_t)stream);
  }
  return gemm128_mx_dispatch(f, a, lda, sa, b, ldb, sb, bias, alpha, y, ldy, M, N, nk, (hipStream_t)stream);
}

// Which body variant 0 of x2v_gemm_<format>_variant launches (mx_body), format = MxFormat::mxm.  Host arithmetic only.
extern "C" __attribute__((visibility("default"))) int x2v_gemm_mx_kernel_choice(int format, int64_t M, int N, int K, int64_t lda, int64_t ldb) {
  if (format < 1 || format > kMxFormatCount) return X2V_E_ARG;
  const MxFormat& f = mx_format(format);
  if (M <= 0 || N <= 0 || K <= 0 || K % f.k_tile != 0 || N % 8 != 0 || lda < K / 8 * f.bits_a || ldb < K / 8 * f.bits_b) return X2V_E_SHAPE;
  return mx_body(f, M, N, K, lda, ldb);
}

// The four C entries of a format: x2v_quant_<Q>_bf16, x2v_gemm_<G> (what the shim calls), x2v_gemm_<G>_variant (a forced body) and x2v_gemm_<G>_epi
// (the fused epilogues of x2v_gemm_bf16 / x2v_gemm_fp8, X2V_EPI_*: what the block drivers call for an MX linear layer).
#define X2V_MX_ENTRIES(Q, G, MXM)                                                                                                                              \
  extern "C" __attribute__((visibility("default"))) int x2v_quant_##Q##_bf16(const void* x, int64_t ldx, void* q, int64_t ldq, void* scales, int64_t M, int K, \
                                                                             void* stream) {                                                                   \
    return quant_mx_entry<MXM>(x, ldx, q, ldq, scales, M, K, stream);                                                                                          \
  }                                                                                                                                                            \
  extern "C" __attribute__((visibility("default"))) int x2v_gemm_##G(const void* a, int64_t lda, const void* sa, const void* b, int64_t ldb, const void* sb,   \
                                                                     const void* bias, const float* alpha, void* y, int64_t ldy, int64_t M, int N, int K,      \
                                                                     void* stream) {                                                                           \
    return gemm_mx_impl(mx_format(MXM), a, lda, sa, b, ldb, sb, bias, alpha, y, ldy, M, N, K, 0, stream);                                                      \
  }                                                                                                                                                            \
  extern "C" __attribute__((visibility("default"))) int x2v_gemm_##G##_variant(const void* a, int64_t lda, const void* sa, const void* b, int64_t ldb,         \
                                                                               const void* sb, const void* bias, const float* alpha, void* y, int64_t ldy,     \
                                                                               int64_t M, int N, int K, int variant, void* stream) {                           \
    return gemm_mx_impl(mx_format(MXM), a, lda, sa, b, ldb, sb, bias, alpha, y, ldy, M, N, K, variant, stream);                                                \
  }                                                                                                                                                            \
  extern "C" __attribute__((visibility("default"))) int x2v_gemm_##G##_epi(const void* a, int64_t lda, const void* sa, const void* b, int64_t ldb,             \
                                                                           const void* sb, const void* bias, const float* alpha, void* y, int64_t ldy,         \
                                                                           int64_t M, int N, int K, int epilogue, const void* resid, int64_t ldr,              \
                                                                           const void* gate, void* stream) {                                                   \
    return gemm_mx_impl(mx_format(MXM), a, lda, sa, b, ldb, sb, bias, alpha, y, ldy, M, N, K, 0, stream, epilogue, resid, ldr, gate);                          \
  }
X2V_MX_ENTRIES(mxfp8, mxfp8, 1)
X2V_MX_ENTRIES(mxfp6, mxfp6_mxfp8, 2)
X2V_MX_ENTRIES(mxfp4, mxfp4, 3)
