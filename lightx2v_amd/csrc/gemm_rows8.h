// The weight-streaming small-M GEMM on 8-bit operands (x2v_gemm_rows_w8a8, instantiated from t5_quant.hip): the Linears of the quantised umT5 text encoder,
// QuantLinearInt8 / QuantLinearFp8 of the reference's q_linear.py behind their activation quantiser.
//
// gemm_rows8_kernel — y[M,N] = epi(float(xq[M,K] . wq[N,K]^T) * sx[m] * sw[n]) for M of a few hundred rows.  gemm_rows.h's launch shape with a plan of
//   its own, because an 8-bit element changes what a k-step is, how many bytes a lane keeps in flight and what the epilogue has to fetch:
//   * No LDS.  W is streamed once, x (a few hundred KB of codes) is served from L2.  D = W . x^T, so a lane ends up with 4 consecutive output columns
//     of one row (8-byte stores, one 16-byte read of sw).  Workgroup = 4 waves stacked along M, wave tile (16 MT) x (16 NT).
//   * int8: v_mfma_i32_16x16x64_i8.  A lane's fragment of either operand is 16 contiguous bytes of one row (bytes 16 g4 .. 16 g4 + 15 of the 64-byte
//     k-step: both operands put the same k into the same slot, which is all a dot product asks of the layout), a ring of 4 k-steps: 4 x (MT + NT)
//     16-byte loads per lane in flight, the byte count of the 16-bit kernel over twice the K.  The i32 accumulator is exact; v_cvt_f32_i32 runs once,
//     in the epilogue.
//   * e4m3: the codes are streamed as bytes and decoded in registers: a fragment is 32 contiguous bytes (two 16-byte loads) of a 128-byte k-step, a ring
//     of 2 k-steps: again 4 x (MT + NT) 16-byte loads per lane in flight.  Each fragment is turned into 4 x 8 fp16 values once per k-step by 16
//     v_cvt_scalef32_pk_f16_fp8 (scale 1: every e4m3 number is an fp16 number) and multiplied by 4 v_mfma_f32_16x16x32_f16: exact products, fp32 sums in k
//     order.  The e4m3 matrix instructions (v_mfma_scale_f32_16x16x128_f8f6f4 with unit scales, v_mfma_f32_16x16x32_fp8_fp8) were built first and are
//     not used: the unit truncates addends when it aligns them, an error of about 2^-16 of an instruction's addends rather than of its result, which
//     is not the fp32 accumulation of the contract (both forms gave the same bits).
//   * The epilogue's operands — sx[m] per row fragment, sw[n .. n + 3] as one 16-byte load per column group — are requested right behind the ring's
//     first fill, so they arrive under the K loop and are no exposed round trip at the end of a latency-bound launch.
//   * Tiles: the accumulators are the 16-bit kernel's size and the fragments the 16-bit kernel's bytes, so the register budget admits the same set
//     {128x64, 64x64, 64x32, 64x16} and the same rule (the largest that still yields >= 192 workgroups; gemm_rows_tile_choice).
//   Every output value is reduced in k order by one lane whatever the tile and whatever M: batching rows is bit-identical.  Rows beyond M or N read
//   the last valid row and never store; there is no barrier.
// Epilogues (ROWS_EPI_NONE / _RESIDUAL / _GEGLU of gemm_rows.h), on v = (float(acc) * sx[m]) * sw[n] — the statement order and rounding points of
//   x2v_gemm_int8 / x2v_gemm_fp8: bf16(v); bf16(resid + bf16(v)); bf16(bf16(v_fc1) * gelu_tanh(bf16(v_gate))) with W and sw holding fc1 and gate.0
//   interleaved row by row.
#pragma once
#include <stdio.h>

#include "gemm_rows.h"
#include "x2v_common.h"

namespace x2v {

template <int KIND>
struct Rows8;
template <>
struct Rows8<X2V_W8A8_INT8> {
  typedef i32x4_t frag;
  typedef i32x4_t op;  // what the matrix instruction reads: the fragment itself
  typedef i32x4_t acc4;
  static constexpr int KSTEP = 64, RING = 4;
  static __device__ __forceinline__ frag load(const unsigned char* p) { return *reinterpret_cast<const i32x4_t*>(p); }
  static __device__ __forceinline__ op prep(frag f) { return f; }
  static __device__ __forceinline__ acc4 mfma(const op& a, const op& b, acc4 c) { return __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c, 0, 0, 0); }
};
template <>
struct Rows8<X2V_W8A8_E4M3> {
  typedef i32x8_t frag;
  struct op {
    half8_t h[4];  // the fragment's 32 codes as fp16, 8 per matrix instruction
  };
  typedef f32x4_t acc4;
  static constexpr int KSTEP = 128, RING = 2;
  static __device__ __forceinline__ frag load(const unsigned char* p) {
    const i32x4_t lo = *reinterpret_cast<const i32x4_t*>(p), hi = *reinterpret_cast<const i32x4_t*>(p + 16);
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
  }
  // Exact: e4m3 (4 significant bits, 2^-9 .. 448) lies inside fp16.  Both operands put code c of the fragment into the same slot.
  static __device__ __forceinline__ op prep(frag f) {
    typedef _Float16 half2_t __attribute__((ext_vector_type(2)));
    op o;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const half2_t a = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((unsigned)f[2 * q], 1.0f, false), b = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((unsigned)f[2 * q], 1.0f, true);
      const half2_t c = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((unsigned)f[2 * q + 1], 1.0f, false), d = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((unsigned)f[2 * q + 1], 1.0f, true);
      o.h[q] = half8_t{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
    }
    return o;
  }
  static __device__ __forceinline__ acc4 mfma(const op& a, const op& b, acc4 c) {
#pragma unroll
    for (int q = 0; q < 4; ++q) c = __builtin_amdgcn_mfma_f32_16x16x32_f16(a.h[q], b.h[q], c, 0, 0, 0);
    return c;
  }
};

template <int KIND, int MT, int NT>
__global__ __launch_bounds__(256) void gemm_rows8_kernel(const unsigned char* __restrict__ xq, int64_t ldx, const float* __restrict__ sx, const unsigned char* __restrict__ wq,
                                                         int64_t ldw, const float* __restrict__ sw, __bf16* y, int64_t ldy, int M, int N, int K, int epi, const __bf16* resid,
                                                         int64_t ldr) {  // y may alias resid: neither is __restrict__
  typedef Rows8<KIND> E;
  typedef typename E::frag frag;
  typedef typename E::acc4 acc4;
  constexpr int KS = E::KSTEP, RING = E::RING;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int c16 = lane & 15, g4 = lane >> 4;
  const int n0 = blockIdx.x * 16 * NT, m0 = blockIdx.y * 64 * MT + wid * 16 * MT;
  if (m0 >= M) return;  // no barrier in this kernel: a wave without rows leaves
  // rows beyond M / N read the last valid row (never stored)
  const unsigned char* xr[MT];
  const unsigned char* wr[NT];
#pragma unroll
  for (int i = 0; i < MT; ++i) xr[i] = xq + (int64_t)min(m0 + 16 * i + c16, M - 1) * ldx + g4 * (KS / 4);
#pragma unroll
  for (int j = 0; j < NT; ++j) wr[j] = wq + (int64_t)min(n0 + 16 * j + c16, N - 1) * ldw + g4 * (KS / 4);

  acc4 acc[NT][MT];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int i = 0; i < MT; ++i) acc[j][i] = acc4{0, 0, 0, 0};

  const int ksteps = K / KS, last = ksteps - 1;
  frag xf[RING][MT], wf[RING][NT];
#pragma unroll
  for (int s = 0; s < RING; ++s) {
    const int ko = min(s, last) * KS;
#pragma unroll
    for (int i = 0; i < MT; ++i) xf[s][i] = E::load(xr[i] + ko);
#pragma unroll
    for (int j = 0; j < NT; ++j) wf[s][j] = E::load(wr[j] + ko);
  }
  // the epilogue's scales, behind the ring's first fill: in flight under the K loop (a column group of 4 is wholly inside or outside N)
  float sxv[MT];
  float4 swv[NT];
#pragma unroll
  for (int i = 0; i < MT; ++i) sxv[i] = sx[min(m0 + 16 * i + c16, M - 1)];
#pragma unroll
  for (int j = 0; j < NT; ++j) swv[j] = *reinterpret_cast<const float4*>(sw + min(n0 + 16 * j + 4 * g4, N - 4));

  for (int ks = 0; ks < ksteps; ks += RING) {
#pragma unroll
    for (int s = 0; s < RING; ++s) {
      if (ks + s < ksteps) {
        typename E::op xo[MT], wo[NT];
#pragma unroll
        for (int i = 0; i < MT; ++i) xo[i] = E::prep(xf[s][i]);
#pragma unroll
        for (int j = 0; j < NT; ++j) wo[j] = E::prep(wf[s][j]);
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
          for (int i = 0; i < MT; ++i) acc[j][i] = E::mfma(wo[j], xo[i], acc[j][i]);
      }
      const int ko = min(ks + s + RING, last) * KS;  // past the end: the last k-step again (read, not used)
#pragma unroll
      for (int i = 0; i < MT; ++i) xf[s][i] = E::load(xr[i] + ko);
#pragma unroll
      for (int j = 0; j < NT; ++j) wf[s][j] = E::load(wr[j] + ko);
    }
  }

  // acc[j][i][e] = row m0 + 16 i + c16, column n0 + 16 j + 4 g4 + e
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int m = m0 + 16 * i + c16;
    if (m >= M) continue;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int n = n0 + 16 * j + 4 * g4;
      if (n >= N) continue;
      const float sws[4] = {swv[j].x, swv[j].y, swv[j].z, swv[j].w};
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = ((float)acc[j][i][e] * sxv[i]) * sws[e];  // int8: v_cvt_f32_i32 of the exact sum
      if (epi == ROWS_EPI_GEGLU) {  // fc1(h) * gelu(gate.0(h)): two bf16 Linear outputs, the GELU of one evaluated in fp32
        bf16x2_t o2;
#pragma unroll
        for (int e = 0; e < 2; ++e) o2[e] = (__bf16)((float)(__bf16)v[2 * e] * gelu_tanh_f((float)(__bf16)v[2 * e + 1]));
        *reinterpret_cast<bf16x2_t*>(y + (int64_t)m * ldy + n / 2) = o2;
        continue;
      }
      if (epi == ROWS_EPI_RESIDUAL) {  // torch: x + linear(...) on two bf16 tensors
        const bf16x4_t rv = *reinterpret_cast<const bf16x4_t*>(resid + (int64_t)m * ldr + n);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (float)rv[e] + (float)(__bf16)v[e];
      }
      bf16x4_t o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = (__bf16)v[e];
      *reinterpret_cast<bf16x4_t*>(y + (int64_t)m * ldy + n) = o;
    }
  }
}

// Checks and launch (the entry has mapped its epilogue to ROWS_EPI_*).  N counts W's rows: with the gated epilogue y has N / 2 columns.
template <int KIND>
static int gemm_rows8_launch(const void* xq, int64_t ldx, const float* sx, const void* wq, int64_t ldw, const float* sw, void* y, int64_t ldy, int64_t M, int N, int K, int epilogue,
                             const void* resid, int64_t ldr, void* stream) {
  const char* who = "gemm_rows_w8a8";
  constexpr int KS = Rows8<KIND>::KSTEP;
  X2V_REQUIRE(xq && sx && wq && sw && y, X2V_E_ARG, "%s: null pointer", who);
  X2V_REQUIRE(epilogue != ROWS_EPI_RESIDUAL || resid != nullptr, X2V_E_ARG, "%s: the residual epilogue needs resid", who);
  X2V_REQUIRE(M >= 0 && N > 0 && K > 0, X2V_E_SHAPE, "%s: bad shape M=%lld N=%d K=%d", who, (long long)M, N, K);
  X2V_REQUIRE(K % KS == 0, X2V_E_SHAPE, "%s: K=%d must be a multiple of %d (the %s k-step; pad the operands with zero columns)", who, K, KS, KIND == X2V_W8A8_INT8 ? "int8" : "e4m3");
  X2V_REQUIRE(KIND != X2V_W8A8_INT8 || K <= 65536, X2V_E_SHAPE, "%s: K=%d is beyond 65536 (the int32 accumulator)", who, K);
  X2V_REQUIRE(N % 4 == 0, X2V_E_SHAPE, "%s: N=%d must be a multiple of 4", who, N);
  const int ny = rows_epi_gated(epilogue) ? N / 2 : N;
  X2V_REQUIRE(ldx >= K && ldw >= K && ldy >= ny && ldx % 16 == 0 && ldw % 16 == 0 && ldy % 4 == 0 && (resid == nullptr || (ldr >= N && ldr % 4 == 0)), X2V_E_ALIGN,
              "%s: leading dimensions must cover the rows (ldx, ldw multiples of 16 bytes, ldy, ldr of 4 elements)", who);
  X2V_REQUIRE(aligned16(xq) && aligned16(wq) && aligned16(sw) && aligned16(y) && aligned16(resid) && ((uintptr_t)sx & 3) == 0, X2V_E_ALIGN,
              "%s: pointers must be 16-byte aligned (sx: 4-byte)", who);
  if (M == 0) return X2V_OK;
  const int t = gemm_rows_tile_choice(M, N);
  const int mt = kGemmRowsTiles[t][0], nt = kGemmRowsTiles[t][1];
  const dim3 grid((unsigned)((N + 16 * nt - 1) / (16 * nt)), (unsigned)((M + 64 * mt - 1) / (64 * mt)));
  hipStream_t st = (hipStream_t)stream;
  const unsigned char *xp = (const unsigned char*)xq, *wp = (const unsigned char*)wq;
  const __bf16* rp = (const __bf16*)resid;
  __bf16* yp = (__bf16*)y;
  if (t == 0)
    hipLaunchKernelGGL((gemm_rows8_kernel<KIND, 2, 4>), grid, dim3(256), 0, st, xp, ldx, sx, wp, ldw, sw, yp, ldy, (int)M, N, K, epilogue, rp, ldr);
  else if (t == 1)
    hipLaunchKernelGGL((gemm_rows8_kernel<KIND, 1, 4>), grid, dim3(256), 0, st, xp, ldx, sx, wp, ldw, sw, yp, ldy, (int)M, N, K, epilogue, rp, ldr);
  else if (t == 2)
    hipLaunchKernelGGL((gemm_rows8_kernel<KIND, 1, 2>), grid, dim3(256), 0, st, xp, ldx, sx, wp, ldw, sw, yp, ldy, (int)M, N, K, epilogue, rp, ldr);
  else
    hipLaunchKernelGGL((gemm_rows8_kernel<KIND, 1, 1>), grid, dim3(256), 0, st, xp, ldx, sx, wp, ldw, sw, yp, ldy, (int)M, N, K, epilogue, rp, ldr);
  return check_hip(hipGetLastError(), "gemm_rows_w8a8 launch");
}

}  // namespace x2v
