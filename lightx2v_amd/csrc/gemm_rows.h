// The weight-streaming small-M GEMM, one kernel for both 16-bit element types: x2v_gemm_f16 (clip.hip, the CLIP tower) and x2v_gemm_rows_bf16 (t5.hip, the
// umT5 text encoder) instantiate it.
//
// gemm_rows_kernel — y[M,N] = epi(x[M,K] . W[N,K]^T + b) on v_mfma_f32_16x16x32_{f16,bf16} for M of a few hundred rows.  No LDS: the launch is bound by
//   streaming W once, x (a few MB) is served from L2.  D = W . x^T, so a lane ends up with 4 consecutive output columns of one row (8-byte stores, bias /
//   residual reads of the same shape).  Workgroup = 4 waves stacked along M, wave tile (16 MT) x (16 NT); a lane's fragment of either operand is 16
//   contiguous bytes of one row.  A 4-deep register ring of k-steps keeps 4 x (MT + NT) 16-byte loads per lane in flight.  The launcher takes the largest tile
//   of {128x64, 64x64, 64x32, 64x16} that still yields >= 192 workgroups.  Every output value is reduced in k order by one lane whatever the tile and whatever
//   M: batching rows is bit-identical.
// Epilogues (ROWS_EPI_*; each entry admits its own subset): plain, exact GELU (fp16), quick-GELU (fp16), residual, and the two gated ones, GEGLU (bf16) and
//   SwiGLU (fp16): W holds the rows of two Linears interleaved (row 2n of one, row 2n + 1 of the other), so a lane's 4 columns are two pairs and it stores
//   2 output columns of y[M, N / 2].  GEGLU: (value, gate) = fc1 * gelu_tanh(gate.0); SwiGLU: (gate, up) = silu(gate_proj) * up_proj.
#pragma once
#include <math.h>
#include <stdio.h>

#include <type_traits>

#include "x2v_common.h"

namespace x2v {

typedef _Float16 half8_t __attribute__((ext_vector_type(8)));
typedef _Float16 half4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float gelu_erf_f(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }

constexpr int GF_RING = 4;
constexpr int ROWS_EPI_NONE = 0, ROWS_EPI_GELU_ERF = 1, ROWS_EPI_RESIDUAL = 2, ROWS_EPI_GEGLU = 3;  // NONE / GELU_ERF / RESIDUAL are X2V_EPI16_*'s values
constexpr int ROWS_EPI_QUICK_GELU = 4, ROWS_EPI_SWIGLU = 5;                                           // fp16 only (X2V_EPI16_QUICK_GELU / _SWIGLU, mapped by the entry)
constexpr bool rows_epi_gated(int epi) { return epi == ROWS_EPI_GEGLU || epi == ROWS_EPI_SWIGLU; }

__device__ __forceinline__ float sigmoid_f(float x) { return 1.0f / (1.0f + expf(-x)); }

template <typename T>
struct RowsElem;
template <>
struct RowsElem<_Float16> {
  typedef half8_t v8;
  typedef half4_t v4;
  typedef _Float16 v2 __attribute__((ext_vector_type(2)));
  static const char* unit() { return "halves"; }
  static __device__ __forceinline__ f32x4_t mfma(v8 a, v8 b, f32x4_t c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
};
template <>
struct RowsElem<__bf16> {
  typedef bf16x8_t v8;
  typedef bf16x4_t v4;
  typedef bf16x2_t v2;
  static const char* unit() { return "elements"; }
  static __device__ __forceinline__ f32x4_t mfma(v8 a, v8 b, f32x4_t c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};

template <typename T, int MT, int NT>
__global__ __launch_bounds__(256) void gemm_rows_kernel(const T* __restrict__ x, int64_t ldx, const T* __restrict__ w, int64_t ldw, const T* __restrict__ bias, T* y,
                                                        int64_t ldy, int M, int N, int K, int epi, const T* resid, int64_t ldr) {  // y may alias resid: neither is __restrict__
  typedef typename RowsElem<T>::v8 v8;
  typedef typename RowsElem<T>::v4 v4;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int c16 = lane & 15, g4 = lane >> 4;
  const int n0 = blockIdx.x * 16 * NT, m0 = blockIdx.y * 64 * MT + wid * 16 * MT;
  if (m0 >= M) return;  // no barrier in this kernel: a wave without rows leaves
  // rows beyond M / N read the last valid row (never stored)
  const T* xr[MT];
  const T* wr[NT];
#pragma unroll
  for (int i = 0; i < MT; ++i) xr[i] = x + (int64_t)min(m0 + 16 * i + c16, M - 1) * ldx + g4 * 8;
#pragma unroll
  for (int j = 0; j < NT; ++j) wr[j] = w + (int64_t)min(n0 + 16 * j + c16, N - 1) * ldw + g4 * 8;

  f32x4_t acc[NT][MT];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int i = 0; i < MT; ++i) acc[j][i] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  const int ksteps = K / 32, last = ksteps - 1;
  v8 xf[GF_RING][MT], wf[GF_RING][NT];
#pragma unroll
  for (int s = 0; s < GF_RING; ++s) {
    const int ko = min(s, last) * 32;
#pragma unroll
    for (int i = 0; i < MT; ++i) xf[s][i] = *reinterpret_cast<const v8*>(xr[i] + ko);
#pragma unroll
    for (int j = 0; j < NT; ++j) wf[s][j] = *reinterpret_cast<const v8*>(wr[j] + ko);
  }
  for (int ks = 0; ks < ksteps; ks += GF_RING) {
#pragma unroll
    for (int s = 0; s < GF_RING; ++s) {
      if (ks + s < ksteps) {
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
          for (int i = 0; i < MT; ++i) acc[j][i] = RowsElem<T>::mfma(wf[s][j], xf[s][i], acc[j][i]);
      }
      const int ko = min(ks + s + GF_RING, last) * 32;  // past the end: the last k-step again (read, not used)
#pragma unroll
      for (int i = 0; i < MT; ++i) xf[s][i] = *reinterpret_cast<const v8*>(xr[i] + ko);
#pragma unroll
      for (int j = 0; j < NT; ++j) wf[s][j] = *reinterpret_cast<const v8*>(wr[j] + ko);
    }
  }

  // acc[j][i][e] = row m0 + 16 i + c16, column n0 + 16 j + 4 g4 + e (N % 4 == 0: a group of 4 columns is wholly inside or outside)
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int m = m0 + 16 * i + c16;
    if (m >= M) continue;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int n = n0 + 16 * j + 4 * g4;
      if (n >= N) continue;
      float v[4] = {acc[j][i][0], acc[j][i][1], acc[j][i][2], acc[j][i][3]};
      // the gated epilogues: torch multiplies two 16-bit Linear outputs, the activation of one of them evaluated in fp32.  GEGLU (bf16): fc1(h) *
      // gelu(gate(h)); SwiGLU (fp16): silu(gate_proj(h)) * up_proj(h)
      if (epi == (std::is_same<T, __bf16>::value ? ROWS_EPI_GEGLU : ROWS_EPI_SWIGLU)) {
        typename RowsElem<T>::v2 o2;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const float a = (float)(T)v[2 * e], g = (float)(T)v[2 * e + 1];
          if constexpr (std::is_same<T, __bf16>::value) o2[e] = (T)(a * gelu_tanh_f(g));
          else o2[e] = (T)(a * sigmoid_f(a) * g);
        }
        *reinterpret_cast<typename RowsElem<T>::v2*>(y + (int64_t)m * ldy + n / 2) = o2;
        continue;
      }
      if (bias != nullptr) {
        const v4 bv = *reinterpret_cast<const v4*>(bias + n);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] += (float)bv[e];
      }
      if (std::is_same<T, _Float16>::value && epi == ROWS_EPI_GELU_ERF) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = gelu_erf_f(v[e]);
      } else if (std::is_same<T, _Float16>::value && epi == ROWS_EPI_QUICK_GELU) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] * sigmoid_f(1.702f * v[e]);
      } else if (epi == ROWS_EPI_RESIDUAL) {  // torch: x + linear(...) on two 16-bit tensors
        const v4 rv = *reinterpret_cast<const v4*>(resid + (int64_t)m * ldr + n);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (float)rv[e] + (float)(T)v[e];
      }
      v4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = (T)v[e];
      *reinterpret_cast<v4*>(y + (int64_t)m * ldy + n) = o;
    }
  }
}

// tile code: 0 = 128 x 64, 1 = 64 x 64, 2 = 64 x 32, 3 = 64 x 16
static const int kGemmRowsTiles[4][2] = {{2, 4}, {1, 4}, {1, 2}, {1, 1}};

static inline int gemm_rows_tile_choice(int64_t M, int N) {
  if (M <= 0 || N <= 0) return X2V_E_SHAPE;
  for (int t = 0; t < 3; ++t) {
    const int64_t bm = 64 * kGemmRowsTiles[t][0], bn = 16 * kGemmRowsTiles[t][1];
    if (((M + bm - 1) / bm) * ((N + bn - 1) / bn) >= 192) return t;
  }
  return 3;
}

// Checks and launch shared by the two entries (`who` starts every error text; the entry has checked its own epilogue set).  N counts W's rows: with
// a gated epilogue y has N / 2 columns.
template <typename T>
static int gemm_rows_launch(const char* who, const void* x, int64_t ldx, const void* w, int64_t ldw, const void* bias, void* y, int64_t ldy, int64_t M, int N, int K, int epilogue,
                            const void* resid, int64_t ldr, void* stream) {
  X2V_REQUIRE(x && w && y, X2V_E_ARG, "%s: null pointer", who);
  X2V_REQUIRE(epilogue != ROWS_EPI_RESIDUAL || resid != nullptr, X2V_E_ARG, "%s: the residual epilogue needs resid", who);
  X2V_REQUIRE(M >= 0 && M < (1ll << 31) && N > 0 && K > 0, X2V_E_SHAPE, "%s: bad shape M=%lld N=%d K=%d", who, (long long)M, N, K);
  X2V_REQUIRE(K % 32 == 0, X2V_E_SHAPE, "%s: K=%d must be a multiple of 32 (pad the operands with zero columns)", who, K);
  X2V_REQUIRE(N % 4 == 0, X2V_E_SHAPE, "%s: N=%d must be a multiple of 4", who, N);
  const int ny = rows_epi_gated(epilogue) ? N / 2 : N;
  X2V_REQUIRE(ldx >= K && ldw >= K && ldy >= ny && ldx % 8 == 0 && ldw % 8 == 0 && ldy % 4 == 0 && (resid == nullptr || (ldr >= N && ldr % 4 == 0)), X2V_E_ALIGN,
              "%s: leading dimensions must cover the rows (ldx, ldw multiples of 8, ldy, ldr of 4 %s)", who, RowsElem<T>::unit());
  X2V_REQUIRE(aligned16(x) && aligned16(w) && aligned16(y) && aligned16(bias) && aligned16(resid), X2V_E_ALIGN, "%s: pointers must be 16-byte aligned", who);
  if (M == 0) return X2V_OK;
  const int t = gemm_rows_tile_choice(M, N);
  const int mt = kGemmRowsTiles[t][0], nt = kGemmRowsTiles[t][1];
  const dim3 grid((unsigned)((N + 16 * nt - 1) / (16 * nt)), (unsigned)((M + 64 * mt - 1) / (64 * mt)));
  X2V_REQUIRE(grid.y < 65536, X2V_E_SHAPE, "%s: M=%lld is beyond this kernel's grid (a skinny-M GEMM)", who, (long long)M);
  hipStream_t st = (hipStream_t)stream;
  const T *xp = (const T*)x, *wp = (const T*)w, *bp = (const T*)bias, *rp = (const T*)resid;
  T* yp = (T*)y;
  if (t == 0)
    hipLaunchKernelGGL((gemm_rows_kernel<T, 2, 4>), grid, dim3(256), 0, st, xp, ldx, wp, ldw, bp, yp, ldy, (int)M, N, K, epilogue, rp, ldr);
  else if (t == 1)
    hipLaunchKernelGGL((gemm_rows_kernel<T, 1, 4>), grid, dim3(256), 0, st, xp, ldx, wp, ldw, bp, yp, ldy, (int)M, N, K, epilogue, rp, ldr);
  else if (t == 2)
    hipLaunchKernelGGL((gemm_rows_kernel<T, 1, 2>), grid, dim3(256), 0, st, xp, ldx, wp, ldw, bp, yp, ldy, (int)M, N, K, epilogue, rp, ldr);
  else
    hipLaunchKernelGGL((gemm_rows_kernel<T, 1, 1>), grid, dim3(256), 0, st, xp, ldx, wp, ldw, bp, yp, ldy, (int)M, N, K, epilogue, rp, ldr);
  char what[64];
  snprintf(what, sizeof(what), "%s launch", who);
  return check_hip(hipGetLastError(), what);
}

}  // namespace x2v
