// The umT5-XXL text encoder's kernels (bf16, as the reference runs it: T5EncoderModel(dtype=torch.bfloat16), runners/wan/wan_runner.py:38-50).
// reference: models/input_encoders/hf/t5/model.py — T5Encoder.forward :314-347, T5SelfAttention :190-205, T5Attention :99-136, T5FeedForward :158-170,
// T5RelativeEmbedding :255-281.  The norm is x2v_rmsnorm_bf16 (norm.hip).
//
// gemm_rows_kernel<__bf16> (gemm_rows.h, shared with the fp16 CLIP tower) — y[M,N] = epi(x[M,K] . W[N,K]^T), the weight-streaming small-M GEMM, with the
//   residual and the GEGLU epilogue (fc1 and gate.0 interleaved row by row in one weight matrix).
// attn_d64_relbias_kernel — non-causal attention, head dim 64, with T5's additive relative-position bias, over packed sequences of 1..512 tokens; q | k | v
//   read in place from the fused QKV GEMM's output rows.  Workgroup = (64 query rows, one head of one sequence).  The sequence bounds arrive by value
//   (a kernel argument: no device copy, no sync).  The head's K [KR][64] and V^T [64][KR] live in LDS next to the head's bias row [1023] in fp32; KR is
//   the sequence's OWN length rounded up to 64 / 128 / 256 / 512 keys (the body is instantiated per size and chosen per workgroup), so a 77-token prompt
//   packed with a 300-token one walks 128 keys.  At 512 keys: 4 KB + 72 KB + 65 KB = 141 KB of the CU's 160.  Built from enc_attn.h's steps (the staging,
//   lane and fragment convention is described there): score * scale + bias, the row maximum, exp and the sum are fp32 in registers, keys >= length masked
//   to -inf (probability exactly 0).
#include <math.h>

#include "enc_attn.h"
#include "gemm_rows.h"
#include "x2v_common.h"

namespace x2v {

constexpr int TA_D = 64;
constexpr int TA_NBIAS = 2 * ENC_MAXLEN - 1;  // deltas -511 .. 511
constexpr int TA_BIAS_BYTES = 4096;           // the bias row's slot at the start of LDS
constexpr int TA_KP = TA_D + 8;               // K row pitch in elements
constexpr int TA_VPAD = 8;                    // V^T row pitch = KR + 8

constexpr int ta_lds_bytes(int kr) { return TA_BIAS_BYTES + (kr * TA_KP + TA_D * (kr + TA_VPAD)) * 2; }
static inline int ta_key_rows(int len) { return len <= 64 ? 64 : len <= 128 ? 128 : len <= 256 ? 256 : 512; }

// NT key tiles of 16 (KR = 16 NT keys in LDS); `base` = the sequence's first row at this head's q columns, `qb` the query block of 64.
template <int NT>
__device__ __forceinline__ void attn_d64_body(char* smem, const __bf16* __restrict__ base, int64_t ld, int64_t D, const float* __restrict__ bias_h, __bf16* __restrict__ out_rows,
                                              int64_t ldo, int len, int qb, float scale) {
  constexpr int KR = 16 * NT, VP = KR + TA_VPAD;
  float* Bs = reinterpret_cast<float*>(smem);
  __bf16* Ks = reinterpret_cast<__bf16*>(smem + TA_BIAS_BYTES);
  __bf16* Vt = Ks + KR * TA_KP;
  const EncLanes L = enc_lanes();

  for (int i = L.tid; i < TA_NBIAS; i += 256) Bs[i] = bias_h[i];
  stage_k<__bf16, TA_D, KR, TA_KP>(Ks, base + D, ld, 0, len, L.tid);
  stage_vt<__bf16, TA_D, KR, VP>(Vt, base + 2 * D, ld, 0, len, L.tid);

  const int q = enc_query(L, qb);
  bf16x8_t qf[2];
  load_q<__bf16, 2>(base + (int64_t)enc_read_row(q, len) * ld, L.g4, qf);
  __syncthreads();
  if (qb * 64 + L.wid * 16 >= len) return;  // no barrier below: a wave without queries leaves

  // scores: sc[t][e] = scale * q . k[16 t + 4 g4 + e] + bias[key - q + 511]   (q <= 511, key <= 511: the index stays inside the row)
  f32x4_t sc[NT];
  float mx = -INFINITY;
  const float* bq = Bs + (ENC_MAXLEN - 1) - q + 4 * L.g4;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    f32x4_t a = score_tile<__bf16, TA_D / 32, TA_KP>(Ks, t, L, qf);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      a[e] = a[e] * scale + bq[16 * t + e];
      if (16 * t + 4 * L.g4 + e >= len) a[e] = -INFINITY;
      mx = fmaxf(mx, a[e]);
    }
    sc[t] = a;
  }
  mx = quad_max(mx);  // finite: key 0 is never masked
  float sum = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float p = __builtin_amdgcn_exp2f((sc[t][e] - mx) * 1.4426950408889634f);
      sc[t][e] = p;
      sum += p;
    }
  sum = quad_sum(sum);

  f32x4_t o[TA_D / 16];
#pragma unroll
  for (int c = 0; c < TA_D / 16; ++c) o[c] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kk = 0; kk < NT / 2; ++kk) pv_step<__bf16, TA_D / 16, VP>(Vt, kk, sc[2 * kk], sc[2 * kk + 1], L, o);
  if (q >= len) return;
  store_out<__bf16, TA_D / 16>(out_rows + (int64_t)q * ldo, o, 1.0f / sum, L.g4);
}

__global__ __launch_bounds__(256) void attn_d64_relbias_kernel(const __bf16* __restrict__ qkv, int64_t ld, const float* __restrict__ bias, __bf16* __restrict__ out, int64_t ldo,
                                                               PackedSeqs seqs, int H, float scale) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int b = blockIdx.y / H, h = blockIdx.y % H, qb = blockIdx.x;
  const int row0 = seqs.cu[b], len = seqs.cu[b + 1] - row0;
  if (qb * 64 >= len) return;  // the whole workgroup: the grid is sized for the longest sequence
  const int64_t D = (int64_t)H * TA_D;
  const __bf16* base = qkv + (int64_t)row0 * ld + h * TA_D;
  const float* bias_h = bias + (int64_t)h * TA_NBIAS;
  __bf16* out_rows = out + (int64_t)row0 * ldo + h * TA_D;
  if (len <= 64)
    attn_d64_body<4>(smem, base, ld, D, bias_h, out_rows, ldo, len, qb, scale);
  else if (len <= 128)
    attn_d64_body<8>(smem, base, ld, D, bias_h, out_rows, ldo, len, qb, scale);
  else if (len <= 256)
    attn_d64_body<16>(smem, base, ld, D, bias_h, out_rows, ldo, len, qb, scale);
  else
    attn_d64_body<32>(smem, base, ld, D, bias_h, out_rows, ldo, len, qb, scale);
}

}  // namespace x2v

using namespace x2v;

static int rows_bf16_epilogue(int epilogue) {
  return epilogue == X2V_EPIR_NONE ? ROWS_EPI_NONE : epilogue == X2V_EPIR_RESIDUAL ? ROWS_EPI_RESIDUAL : epilogue == X2V_EPIR_GEGLU ? ROWS_EPI_GEGLU : -1;
}

extern "C" __attribute__((visibility("default"))) int x2v_gemm_rows_bf16_tile_choice(int64_t M, int N, int epilogue) {
  if (N <= 0 || N >= (1 << 30) || rows_bf16_epilogue(epilogue) < 0) return X2V_E_SHAPE;
  return gemm_rows_tile_choice(M, epilogue == X2V_EPIR_GEGLU ? 2 * N : N);
}

extern "C" __attribute__((visibility("default"))) int x2v_gemm_rows_bf16(const void* x, int64_t ldx, const void* w, int64_t ldw, void* y, int64_t ldy, int64_t M, int N, int K,
                                                                         int epilogue, const void* resid, int64_t ldr, void* stream) {
  const int epi = rows_bf16_epilogue(epilogue);
  X2V_REQUIRE(epi >= 0, X2V_E_ARG, "gemm_rows_bf16: unknown epilogue %d", epilogue);
  X2V_REQUIRE(M <= 4096, X2V_E_SHAPE, "gemm_rows_bf16: M=%lld is beyond the 4096 rows this weight-streaming form is meant for (x2v_gemm_bf16 takes large M)", (long long)M);
  X2V_REQUIRE(N > 0 && N < (1 << 30), X2V_E_SHAPE, "gemm_rows_bf16: bad shape M=%lld N=%d K=%d", (long long)M, N, K);
  X2V_REQUIRE(epi != ROWS_EPI_GEGLU || N % 2 == 0, X2V_E_SHAPE, "gemm_rows_bf16: N=%d must be even with the GEGLU epilogue", N);
  X2V_REQUIRE(epi == ROWS_EPI_RESIDUAL || resid == nullptr, X2V_E_ARG, "gemm_rows_bf16: resid is read by the residual epilogue only");
  return gemm_rows_launch<__bf16>("gemm_rows_bf16", x, ldx, w, ldw, nullptr, y, ldy, M, epi == ROWS_EPI_GEGLU ? 2 * N : N, K, epi, resid, ldr, stream);
}

extern "C" __attribute__((visibility("default"))) int x2v_attn_bf16_d64_relbias(const void* qkv, int64_t ld, const float* bias, void* out, int64_t ldo, const int* cu_seqlens,
                                                                                int batch, int num_heads, float scale, void* stream) {
  X2V_REQUIRE(qkv && bias && out && cu_seqlens, X2V_E_ARG, "attn_bf16_d64_relbias: null pointer");
  PackedSeqs seqs;
  int longest;
  int rc = packed_seqs_check("attn_bf16_d64_relbias", cu_seqlens, batch, ENC_MAXLEN, "keys this kernel holds in LDS", &seqs, &longest);
  if (rc != X2V_OK) return rc;
  X2V_REQUIRE(num_heads > 0 && (int64_t)batch * num_heads < 65536, X2V_E_SHAPE, "attn_bf16_d64_relbias: bad head count %d", num_heads);
  X2V_REQUIRE(scale == scale && fabsf(scale) <= 3.0e38f, X2V_E_ARG, "attn_bf16_d64_relbias: scale must be finite (T5 passes 1)");
  X2V_REQUIRE(ld >= 3ll * num_heads * TA_D && ldo >= (int64_t)num_heads * TA_D && ld % 8 == 0 && ldo % 4 == 0, X2V_E_ALIGN,
              "attn_bf16_d64_relbias: ld must cover [q | k | v] of %d heads x 64 (a multiple of 8 elements), ldo the output row (of 4)", num_heads);
  X2V_REQUIRE(aligned16(qkv) && aligned16(out) && ((uintptr_t)bias & 3) == 0, X2V_E_ALIGN, "attn_bf16_d64_relbias: qkv / out must be 16-byte aligned, bias 4-byte");
  const int lds = ta_lds_bytes(ta_key_rows(longest));
  rc = ensure_dynamic_lds((const void*)attn_d64_relbias_kernel, ta_lds_bytes(ENC_MAXLEN), "attn_bf16_d64_relbias attr");
  if (rc != X2V_OK) return rc;
  hipLaunchKernelGGL(attn_d64_relbias_kernel, dim3((unsigned)((longest + 63) / 64), (unsigned)(batch * num_heads)), dim3(256), lds, (hipStream_t)stream, (const __bf16*)qkv, ld,
                     bias, (__bf16*)out, ldo, seqs, num_heads, scale);
  X2V_LAUNCH_CHECK("attn_bf16_d64_relbias launch");
  return X2V_OK;
}
