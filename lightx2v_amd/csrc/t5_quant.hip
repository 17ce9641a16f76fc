// The kernels the quantised umT5 text encoder adds to t5.hip's (t5_quantized with t5_quant_scheme int8 | fp8: every Linear of T5Attention and T5FeedForward
// is a QuantLinearInt8 / QuantLinearFp8, models/input_encoders/hf/q_linear.py:20-39, 69-87, built by t5/model.py:84-96, 145-155).
//
// gemm_rows8_kernel (gemm_rows8.h) — the weight-streaming small-M GEMM on int8 or e4m3 codes with per-row and per-channel scales: x2v_gemm_rows_w8a8.
// rmsnorm_quant_kernel — T5LayerNorm (:68-72) fused with the per-token quantiser of its bf16 output: rmsnorm_kernel's steps (rowwise.h) on rmsnorm_kernel's
//   lane layout, then quant8_rowwise_kernel's scale and pack (quant8.h) on the values rounded where the norm's store rounds them.  q, k and v read the one
//   quantised h, which is what three QuantLinears make of the same input.
// A source of its own because it is built without the packed fp32 instructions (build.py): the 16-bit kernels of t5.hip keep their instruction streams.
#include <math.h>
#include <stdio.h>

#include "gemm_rows8.h"
#include "rowwise.h"
#include "x2v_common.h"

namespace x2v {

// x2v_rmsnorm_bf16 (X2V_ROUND_FP32) + x2v_quant_{int8,fp8}_rowwise in one pass: the row stays in registers between its one read and the store of its codes.
// NW waves share a row exactly as in rmsnorm_kernel (NW = 1: one wave per row, 4 rows per block, for D <= 512), so the sum of squares is reduced in that
// kernel's order; the maximum the quantiser takes has no order.
template <int CH, int NW, bool I8>
__global__ __launch_bounds__(256) void rmsnorm_quant_kernel(const unsigned short* __restrict__ x, int64_t ldx, const unsigned short* __restrict__ w, unsigned char* __restrict__ xq,
                                                            int64_t ldq, float* __restrict__ sx, int64_t M, int D, float eps) {
  __shared__ float red[4];
  constexpr int ROWS = 4 / NW;
  const int t = threadIdx.x % (NW * 64);
  const int64_t row = (int64_t)blockIdx.x * ROWS + threadIdx.x / (NW * 64);
  const bool live = row < M;  // NW == 4: always (one block per row); NW == 1: whole waves, and no barrier below
  RowRegs<CH, NW> r;
  if (live) r.load(x + row * ldx, D, t);
  float ss = 0.f;
  if (live) ss = rms_sumsq<X2V_ROUND_FP32>(r.v);
  ss = row_sum<NW>(ss, red);
  if (!live) return;
  const float rs = rms_rstd<X2V_ROUND_FP32>(ss, (float)D, eps);
  float amax = 0.f;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    if (!r.ok[c]) continue;
    const int e = (c * NW * 64 + t) * 8;
    float wv[8], o[8];
    unpack8(*reinterpret_cast<const uint4*>(w + e), wv);
    rms_norm8<X2V_ROUND_FP32>(r.v[c], rs, wv, o);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      r.v[c][j] = rbf(o[j]);  // the bf16 tensor the reference quantises
      amax = fmaxf(amax, fabsf(r.v[c][j]));
    }
  }
  amax = block_max<NW>(amax, red);
  const float s = I8 ? int8_scale(amax) : e4m3_scale(amax);
  if (t == 0) sx[row] = s;
  const float inv = int8_inv_scale(amax);
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    if (!r.ok[c]) continue;
    const int e = (c * NW * 64 + t) * 8;
    uint2 o;
    if constexpr (I8) o = int8_codes8(r.v[c], inv);
    else o = e4m3_codes8(r.v[c], s);
    *reinterpret_cast<uint2*>(xq + row * ldq + e) = o;
  }
}

}  // namespace x2v

using namespace x2v;

extern "C" __attribute__((visibility("default"))) int x2v_gemm_rows_w8a8_tile_choice(int64_t M, int N, int epilogue) { return x2v_gemm_rows_bf16_tile_choice(M, N, epilogue); }

extern "C" __attribute__((visibility("default"))) int x2v_gemm_rows_w8a8(const void* xq, int64_t ldx, const float* sx, const void* wq, int64_t ldw, const float* sw, void* y,
                                                                         int64_t ldy, int64_t M, int N, int K, int kind, int epilogue, const void* resid, int64_t ldr,
                                                                         void* stream) {
  const int epi = epilogue == X2V_EPIR_NONE ? ROWS_EPI_NONE : epilogue == X2V_EPIR_RESIDUAL ? ROWS_EPI_RESIDUAL : epilogue == X2V_EPIR_GEGLU ? ROWS_EPI_GEGLU : -1;
  X2V_REQUIRE(kind == X2V_W8A8_INT8 || kind == X2V_W8A8_E4M3, X2V_E_ARG, "gemm_rows_w8a8: unknown code type %d", kind);
  X2V_REQUIRE(epi >= 0, X2V_E_ARG, "gemm_rows_w8a8: unknown epilogue %d", epilogue);
  X2V_REQUIRE(M <= 4096, X2V_E_SHAPE, "gemm_rows_w8a8: M=%lld is beyond the 4096 rows this weight-streaming form is meant for (x2v_gemm_int8 / x2v_gemm_fp8 take large M)",
              (long long)M);
  X2V_REQUIRE(N > 0 && N < (1 << 30), X2V_E_SHAPE, "gemm_rows_w8a8: bad shape M=%lld N=%d K=%d", (long long)M, N, K);
  X2V_REQUIRE(epi != ROWS_EPI_GEGLU || N % 2 == 0, X2V_E_SHAPE, "gemm_rows_w8a8: N=%d must be even with the GEGLU epilogue", N);
  X2V_REQUIRE(epi == ROWS_EPI_RESIDUAL || resid == nullptr, X2V_E_ARG, "gemm_rows_w8a8: resid is read by the residual epilogue only");
  const int rows = epi == ROWS_EPI_GEGLU ? 2 * N : N;
  if (kind == X2V_W8A8_INT8) return gemm_rows8_launch<X2V_W8A8_INT8>(xq, ldx, sx, wq, ldw, sw, y, ldy, M, rows, K, epi, resid, ldr, stream);
  return gemm_rows8_launch<X2V_W8A8_E4M3>(xq, ldx, sx, wq, ldw, sw, y, ldy, M, rows, K, epi, resid, ldr, stream);
}

template <bool I8>
static int rmsnorm_quant(const char* who, const void* x, int64_t ldx, const void* w, void* xq, int64_t ldq, float* sx, int64_t M, int D, float eps, void* stream) {
  X2V_REQUIRE(x && w && xq && sx, X2V_E_ARG, "%s: null pointer", who);
  X2V_REQUIRE(D > 0 && D % 8 == 0 && D <= 16384, X2V_E_SHAPE, "%s: D=%d must be a multiple of 8 and <= 16384", who, D);
  X2V_REQUIRE(ldx % 8 == 0 && ldx >= D && ldq % 8 == 0 && ldq >= D && aligned16(x) && aligned16(w) && ((uintptr_t)xq % 8) == 0 && ((uintptr_t)sx & 3) == 0, X2V_E_ALIGN,
              "%s: row alignment (x rows 16-byte, code rows 8-byte, both covering D)", who);
  if (M <= 0) return X2V_OK;
  X2V_REQUIRE(M < (1ll << 31), X2V_E_SHAPE, "%s: too many rows", who);
  auto xs = (const unsigned short*)x, ws = (const unsigned short*)w;
  hipStream_t st = (hipStream_t)stream;
  int rc = X2V_OK;
  if (D <= 512) {  // one wave per row, 4 rows per block: x2v_rmsnorm_bf16's split, so that the sum of squares is reduced in its order
    hipLaunchKernelGGL((rmsnorm_quant_kernel<1, 1, I8>), dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, xs, ldx, ws, (unsigned char*)xq, ldq, sx, M, D, eps);
  } else {
    rc = dispatch_ch(chunks_for(D, 4), D, [&](auto chc) {
      hipLaunchKernelGGL((rmsnorm_quant_kernel<decltype(chc)::value, 4, I8>), dim3((unsigned)M), dim3(256), 0, st, xs, ldx, ws, (unsigned char*)xq, ldq, sx, M, D, eps);
    });
  }
  if (rc != X2V_OK) return rc;
  char what[64];
  snprintf(what, sizeof(what), "%s launch", who);
  return check_hip(hipGetLastError(), what);
}

extern "C" __attribute__((visibility("default"))) int x2v_rmsnorm_quant_int8(const void* x, int64_t ldx, const void* w, void* xq, int64_t ldq, float* sx, int64_t M, int D, float eps,
                                                                             void* stream) {
  return rmsnorm_quant<true>("rmsnorm_quant_int8", x, ldx, w, xq, ldq, sx, M, D, eps, stream);
}

extern "C" __attribute__((visibility("default"))) int x2v_rmsnorm_quant_fp8(const void* x, int64_t ldx, const void* w, void* xq, int64_t ldq, float* sx, int64_t M, int D, float eps,
                                                                            void* stream) {
  return rmsnorm_quant<false>("rmsnorm_quant_fp8", x, ldx, w, xq, ldq, sx, M, D, eps, stream);
}
