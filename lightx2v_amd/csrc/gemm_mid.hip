// x2v_gemm_mid_f16: the fp16 instantiation of the LDS-tiled, K-split mid-M GEMM (gemm_mid.h) — the four Linears of a Llama text-tower layer at 128 or more
// packed rows (lightx2v_amd/llama.py, mid_gemm), with the rounding points of x2v_gemm_f16.  A bf16 entry is one more instantiation of gemm_mid_launch.
#include "gemm_mid.h"

using namespace x2v;

extern "C" __attribute__((visibility("default"))) int x2v_gemm_mid_f16(const void* x, int64_t ldx, const void* w, int64_t ldw, const void* bias, void* y, int64_t ldy, int64_t M,
                                                                       int N, int K, int epilogue, const void* resid, int64_t ldr, int splits, void* workspace,
                                                                       int64_t workspace_bytes, void* stream) {
  X2V_REQUIRE(x && w && y, X2V_E_ARG, "gemm_mid_f16: null pointer");
  X2V_REQUIRE(epilogue == X2V_EPI16_NONE || epilogue == X2V_EPI16_RESIDUAL || epilogue == X2V_EPI16_SWIGLU, X2V_E_ARG,
              "gemm_mid_f16: epilogue %d is not built (NONE, RESIDUAL and SWIGLU are)", epilogue);
  if (epilogue == X2V_EPI16_SWIGLU) {  // W holds 2N rows (gate_proj and up_proj interleaved), y has N columns
    X2V_REQUIRE(bias == nullptr, X2V_E_ARG, "gemm_mid_f16: the SwiGLU epilogue takes no bias");
    X2V_REQUIRE(N > 0 && N < (1 << 30), X2V_E_SHAPE, "gemm_mid_f16: bad N=%d", N);
    return gemm_mid_launch<_Float16>("gemm_mid_f16", x, ldx, w, ldw, nullptr, y, ldy, M, 2 * N, K, ROWS_EPI_SWIGLU, resid, ldr, splits, workspace, workspace_bytes, stream);
  }
  return gemm_mid_launch<_Float16>("gemm_mid_f16", x, ldx, w, ldw, bias, y, ldy, M, N, K, epilogue, resid, ldr, splits, workspace, workspace_bytes, stream);
}

extern "C" __attribute__((visibility("default"))) int64_t x2v_gemm_mid_workspace_bytes(int64_t M, int N, int K, int splits) {
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  return gemm_mid_ws_bytes(M, N, splits == 0 ? gemm_mid_splits(M, N, K, gemm_mid_cu_count()) : splits);
}

extern "C" __attribute__((visibility("default"))) int x2v_gemm_mid_choice(int64_t M, int N, int K, int cu_count) {
  if (M <= 0 || M > 4096 || N <= 0 || K <= 0 || cu_count <= 0) return X2V_E_SHAPE;
  return 1 | gemm_mid_splits(M, N, K, cu_count) << 8;
}
