// The CLIP ViT-H/14 image tower's kernels (fp16, as the reference runs it: CLIPModel(dtype=torch.float16), runners/wan/wan_runner.py:71-72).
// reference: models/input_encoders/hf/xlm_roberta/model.py — CLIPModel.visual :436-450, VisionTransformer.forward :274-295, AttentionBlock :157-164,
// SelfAttention :75-91, LayerNorm :47-49.
//
// gemm_rows_kernel<_Float16> (gemm_rows.h, shared with the bf16 text encoder) — y[M,N] = epi(x[M,K] . W[N,K]^T + b), the weight-streaming small-M GEMM.
// attn_f16_d80_kernel — non-causal attention, head dim 80, <= 272 keys, q/k/v read in place from the QKV GEMM's output rows.  Workgroup = (64 query rows, one
//   head of one image); the head's K [272][80] and V^T [80][288] live in LDS (93 KiB).  Built from enc_attn.h's steps (the staging, lane and fragment
//   convention is described there): three k-steps over d, 32 + 32 + 16, the last half zero in both operands; a query's 272 scores sit in 17 accumulator
//   tiles, the softmax is done in registers (fp32), keys >= S masked to -inf; an 18th all-zero tile fills the second half of the 9th PV k-step.
// ln_f16_kernel — LayerNorm of an fp16 row in registers: fp32 two-pass statistics, fp32 affine, one rounding.  EMBED: the row is built first as
//   fp16(cls | patch token + pos_embedding) (VisionTransformer.forward :278-287).
// clip_preprocess_kernel — bicubic resample (A = -0.75, align_corners=False, border-clamped taps: F.interpolate(mode="bicubic")), (x * 0.5 + 0.5 - mean) / std,
//   written as the patch-major fp16 operand of the patch-embedding GEMM (column c * P * P + py * P + px: the flattened Conv2d weight), pad columns zeroed.
#include <math.h>

#include <algorithm>

#include "enc_attn.h"
#include "gemm_rows.h"
#include "x2v_common.h"

namespace x2v {

// ---- attention -----------------------------------------------------------------------------------------------------------------------------------------
constexpr int AT_D = 80;
constexpr int AT_TILES = 17;               // key tiles of 16: S <= 272
constexpr int AT_KROWS = AT_TILES * 16;    // 272
constexpr int AT_KP = 88;                  // K row pitch in halves (176 B: 16-byte aligned rows, 8 pad halves never read)
constexpr int AT_VKEYS = 288;              // 9 k-steps of 32 keys
constexpr int AT_VP = 296;                 // V^T row pitch in halves
constexpr int AT_LDS = (AT_KROWS * AT_KP + AT_D * AT_VP) * 2;  // 95232 B

__global__ __launch_bounds__(256) void attn_f16_d80_kernel(const _Float16* __restrict__ qkv, int64_t ld, _Float16* __restrict__ out, int64_t ldo, int S, int H,
                                                           float scale_log2e) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  _Float16* Ks = reinterpret_cast<_Float16*>(smem);
  _Float16* Vt = Ks + AT_KROWS * AT_KP;
  const EncLanes L = enc_lanes();
  const int b = blockIdx.y / H, h = blockIdx.y % H;
  const int64_t D = (int64_t)H * AT_D;
  const _Float16* base = qkv + (int64_t)b * S * ld + h * AT_D;

  stage_k<_Float16, AT_D, AT_KROWS, AT_KP>(Ks, base + D, ld, 0, S, L.tid);
  stage_vt<_Float16, AT_D, AT_VKEYS, AT_VP>(Vt, base + 2 * D, ld, 0, S, L.tid);

  const int q = enc_query(L, blockIdx.x);
  const _Float16* qp = base + (int64_t)enc_read_row(q, S) * ld;
  half8_t qf[3];
  load_q<_Float16, 2>(qp, L.g4, qf);
  qf[2] = half8_t{};
  if (L.g4 < 2) qf[2] = *reinterpret_cast<const half8_t*>(qp + 64 + 8 * L.g4);
  __syncthreads();

  // scores: sc[t][e] = q . k[16 t + 4 g4 + e]   (three k-steps over d: 32 + 32 + 16)
  f32x4_t sc[AT_TILES + 1];
  float mx = -INFINITY;
#pragma unroll
  for (int t = 0; t < AT_TILES; ++t) {
    f32x4_t a = score_tile<_Float16, 2, AT_KP, true>(Ks, t, L, qf);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (16 * t + 4 * L.g4 + e >= S) a[e] = -INFINITY;
      mx = fmaxf(mx, a[e]);
    }
    sc[t] = a;
  }
  sc[AT_TILES] = f32x4_t{0.f, 0.f, 0.f, 0.f};  // the second half of the last k-step: no keys
  mx = quad_max(mx);                          // finite: key 0 is never masked
  float sum = 0.f;
#pragma unroll
  for (int t = 0; t < AT_TILES; ++t)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float p = __builtin_amdgcn_exp2f((sc[t][e] - mx) * scale_log2e);
      sc[t][e] = p;
      sum += p;
    }
  sum = quad_sum(sum);

  f32x4_t o[AT_D / 16];
#pragma unroll
  for (int c = 0; c < AT_D / 16; ++c) o[c] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kk = 0; kk < AT_VKEYS / 32; ++kk) pv_step<_Float16, AT_D / 16, AT_VP>(Vt, kk, sc[2 * kk], sc[2 * kk + 1], L, o);
  if (q >= S) return;
  store_out<_Float16, AT_D / 16>(out + ((int64_t)b * S + q) * ldo + h * AT_D, o, 1.0f / sum, L.g4);
}

// ---- LayerNorm (and the token assembly in front of pre_norm) ------------------------------------------------------------------------------------------
template <bool EMBED>
__global__ __launch_bounds__(256) void ln_f16_kernel(const _Float16* __restrict__ x, int64_t ldx, const _Float16* __restrict__ cls, const _Float16* __restrict__ pos,
                                                     int tokens, const float* __restrict__ w, const float* __restrict__ bb, _Float16* __restrict__ y, int64_t ldy, int D,
                                                     float eps) {
  __shared__ float red[4];
  const int64_t row = blockIdx.x;
  const int c0 = threadIdx.x * 8;
  const bool live = c0 < D;
  float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (live) {
    half8_t hv;
    if constexpr (EMBED) {
      const int t = (int)(row % tokens);
      const int64_t img = row / tokens;
      hv = t == 0 ? *reinterpret_cast<const half8_t*>(cls + c0) : *reinterpret_cast<const half8_t*>(x + (img * (tokens - 1) + t - 1) * ldx + c0);
      const half8_t pv = *reinterpret_cast<const half8_t*>(pos + (int64_t)t * D + c0);
#pragma unroll
      for (int e = 0; e < 8; ++e) hv[e] = (_Float16)((float)hv[e] + (float)pv[e]);  // the fp16 add x + e (model.py:285)
    } else {
      hv = *reinterpret_cast<const half8_t*>(x + row * ldx + c0);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (float)hv[e];
  }
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) s += v[e];
  const float mean = block_sum<4>(s, red) / (float)D;
  float s2 = 0.f;
  if (live) {
#pragma unroll
    for (int e = 0; e < 8; ++e) s2 += (v[e] - mean) * (v[e] - mean);
  }
  const float rstd = 1.0f / sqrtf(block_sum<4>(s2, red) / (float)D + eps);
  if (!live) return;
  half8_t o;
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = (_Float16)((v[e] - mean) * rstd * w[c0 + e] + bb[c0 + e]);
  *reinterpret_cast<half8_t*>(y + row * ldy + c0) = o;
}

// ---- image front end -------------------------------------------------------------------------------------------------------------------------------------
struct ClipNorm {
  float mean[3], std[3];
};

__device__ __forceinline__ void cubic_coeffs(float t, float* c) {
  const float A = -0.75f;  // aten/src/ATen/native/UpSample.h: cubic_convolution1 / 2
  const float x0 = t + 1.0f, x3 = 2.0f - t, x2 = 1.0f - t;
  c[0] = ((A * x0 - 5.0f * A) * x0 + 8.0f * A) * x0 - 4.0f * A;
  c[1] = ((A + 2.0f) * t - (A + 3.0f)) * t * t + 1.0f;
  c[2] = ((A + 2.0f) * x2 - (A + 3.0f)) * x2 * x2 + 1.0f;
  c[3] = ((A * x3 - 5.0f * A) * x3 + 8.0f * A) * x3 - 4.0f * A;
}

__global__ __launch_bounds__(256) void clip_preprocess_kernel(const float* __restrict__ img, int64_t cs, int64_t rs, int H, int W, _Float16* __restrict__ out, int64_t ldo,
                                                              int size, int P, ClipNorm nm) {
  const int G = size / P, kk = 3 * P * P;
  const int64_t total = (int64_t)G * G * ldo;
  const float sh = (float)H / (float)size, sw = (float)W / (float)size;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int col = (int)(i % ldo), patch = (int)(i / ldo);
    if (col >= kk) {
      out[i] = (_Float16)0.f;
      continue;
    }
    const int c = col / (P * P), r = col % (P * P);
    const int oy = (patch / G) * P + r / P, ox = (patch % G) * P + r % P;
    const float ry = sh * ((float)oy + 0.5f) - 0.5f, rx = sw * ((float)ox + 0.5f) - 0.5f;
    const float fy = floorf(ry), fx = floorf(rx);
    float cy[4], cx[4];
    cubic_coeffs(ry - fy, cy);
    cubic_coeffs(rx - fx, cx);
    const int iy = (int)fy, ix = (int)fx;
    const float* src = img + c * cs;
    float acc = 0.f;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const float* rowp = src + (int64_t)min(max(iy - 1 + a, 0), H - 1) * rs;
      float ra = 0.f;
#pragma unroll
      for (int bq = 0; bq < 4; ++bq) ra += rowp[min(max(ix - 1 + bq, 0), W - 1)] * cx[bq];
      acc += ra * cy[a];
    }
    out[i] = (_Float16)((acc * 0.5f + 0.5f - nm.mean[c]) / nm.std[c]);
  }
}

}  // namespace x2v

using namespace x2v;

extern "C" __attribute__((visibility("default"))) int x2v_gemm_f16_tile_choice(int64_t M, int N) { return gemm_rows_tile_choice(M, N); }

extern "C" __attribute__((visibility("default"))) int x2v_gemm_f16(const void* x, int64_t ldx, const void* w, int64_t ldw, const void* bias, void* y, int64_t ldy, int64_t M,
                                                                   int N, int K, int epilogue, const void* resid, int64_t ldr, void* stream) {
  X2V_REQUIRE(x && w && y, X2V_E_ARG, "gemm_f16: null pointer");
  X2V_REQUIRE(epilogue >= X2V_EPI16_NONE && epilogue <= X2V_EPI16_SWIGLU, X2V_E_ARG, "gemm_f16: unknown epilogue %d", epilogue);
  X2V_REQUIRE(epilogue != X2V_EPI16_QUICK_GELU || bias != nullptr, X2V_E_ARG, "gemm_f16: the quick-GELU epilogue needs a bias (CLIPMLP.fc1 has one)");
  if (epilogue == X2V_EPI16_SWIGLU) {  // W holds 2N rows (gate_proj and up_proj interleaved), y has N columns
    X2V_REQUIRE(bias == nullptr, X2V_E_ARG, "gemm_f16: the SwiGLU epilogue takes no bias");
    X2V_REQUIRE(N > 0 && N % 2 == 0 && N < (1 << 30), X2V_E_SHAPE, "gemm_f16: N=%d must be even with the SwiGLU epilogue", N);
    return gemm_rows_launch<_Float16>("gemm_f16", x, ldx, w, ldw, nullptr, y, ldy, M, 2 * N, K, ROWS_EPI_SWIGLU, resid, ldr, stream);
  }
  return gemm_rows_launch<_Float16>("gemm_f16", x, ldx, w, ldw, bias, y, ldy, M, N, K, epilogue == X2V_EPI16_QUICK_GELU ? ROWS_EPI_QUICK_GELU : epilogue, resid, ldr, stream);
}

extern "C" __attribute__((visibility("default"))) int x2v_attn_f16_d80(const void* qkv, int64_t ld, void* out, int64_t ldo, int batch, int S, int num_heads, float scale,
                                                                       void* stream) {
  X2V_REQUIRE(qkv && out, X2V_E_ARG, "attn_f16_d80: null pointer");
  X2V_REQUIRE(batch > 0 && num_heads > 0 && S >= 1, X2V_E_SHAPE, "attn_f16_d80: bad shape");
  X2V_REQUIRE(S <= AT_KROWS, X2V_E_SHAPE, "attn_f16_d80: S=%d keys exceed the %d this kernel holds in LDS", S, AT_KROWS);
  X2V_REQUIRE((int64_t)batch * num_heads < 65536, X2V_E_SHAPE, "attn_f16_d80: batch * heads must be below 65536");
  X2V_REQUIRE(ld >= 3ll * num_heads * AT_D && ldo >= (int64_t)num_heads * AT_D && ld % 8 == 0 && ldo % 4 == 0, X2V_E_ALIGN,
              "attn_f16_d80: ld must cover [q | k | v] of %d heads x 80 (a multiple of 8 halves), ldo the output row (of 4)", num_heads);
  X2V_REQUIRE(aligned16(qkv) && aligned16(out), X2V_E_ALIGN, "attn_f16_d80: pointers must be 16-byte aligned");
  int rc = ensure_dynamic_lds((const void*)attn_f16_d80_kernel, AT_LDS, "attn_f16_d80 attr");
  if (rc != X2V_OK) return rc;
  if (scale == 0.f) scale = 1.0f / sqrtf((float)AT_D);
  hipLaunchKernelGGL(attn_f16_d80_kernel, dim3((unsigned)((S + 63) / 64), (unsigned)(batch * num_heads)), dim3(256), AT_LDS, (hipStream_t)stream, (const _Float16*)qkv, ld,
                     (_Float16*)out, ldo, S, num_heads, scale * 1.4426950408889634f);
  X2V_LAUNCH_CHECK("attn_f16_d80 launch");
  return X2V_OK;
}

extern "C" __attribute__((visibility("default"))) int x2v_layernorm_f16(const void* x, int64_t ldx, const float* w, const float* b, void* y, int64_t ldy, int64_t M, int D,
                                                                        float eps, void* stream) {
  X2V_REQUIRE(x && w && b && y, X2V_E_ARG, "layernorm_f16: null pointer");
  X2V_REQUIRE(M >= 0 && M < (1ll << 31) && D > 0 && D % 8 == 0 && D <= 2048, X2V_E_SHAPE, "layernorm_f16: D=%d must be a multiple of 8, at most 2048", D);
  X2V_REQUIRE(ldx >= D && ldy >= D && ldx % 8 == 0 && ldy % 8 == 0, X2V_E_ALIGN, "layernorm_f16: leading dimensions must be multiples of 8 halves covering D");
  X2V_REQUIRE(aligned16(x) && aligned16(y) && aligned16(w) && aligned16(b), X2V_E_ALIGN, "layernorm_f16: pointers must be 16-byte aligned");
  if (M == 0) return X2V_OK;
  hipLaunchKernelGGL(ln_f16_kernel<false>, dim3((unsigned)M), dim3(256), 0, (hipStream_t)stream, (const _Float16*)x, ldx, (const _Float16*)nullptr, (const _Float16*)nullptr, 1, w,
                     b, (_Float16*)y, ldy, D, eps);
  X2V_LAUNCH_CHECK("layernorm_f16 launch");
  return X2V_OK;
}

extern "C" __attribute__((visibility("default"))) int x2v_clip_embed_f16(const void* patches, int64_t ldp, const void* cls, const void* pos, const float* w, const float* b,
                                                                         void* y, int64_t ldy, int batch, int tokens, int D, float eps, void* stream) {
  X2V_REQUIRE(patches && cls && pos && w && b && y, X2V_E_ARG, "clip_embed_f16: null pointer");
  X2V_REQUIRE(batch > 0 && tokens >= 2 && (int64_t)batch * tokens < (1ll << 31) && D > 0 && D % 8 == 0 && D <= 2048, X2V_E_SHAPE,
              "clip_embed_f16: bad shape (tokens >= 2 with the class token, D=%d a multiple of 8, at most 2048)", D);
  X2V_REQUIRE(ldp >= D && ldy >= D && ldp % 8 == 0 && ldy % 8 == 0, X2V_E_ALIGN, "clip_embed_f16: leading dimensions must be multiples of 8 halves covering D");
  X2V_REQUIRE(aligned16(patches) && aligned16(cls) && aligned16(pos) && aligned16(y) && aligned16(w) && aligned16(b), X2V_E_ALIGN,
              "clip_embed_f16: pointers must be 16-byte aligned");
  hipLaunchKernelGGL(ln_f16_kernel<true>, dim3((unsigned)(batch * tokens)), dim3(256), 0, (hipStream_t)stream, (const _Float16*)patches, ldp, (const _Float16*)cls,
                     (const _Float16*)pos, tokens, w, b, (_Float16*)y, ldy, D, eps);
  X2V_LAUNCH_CHECK("clip_embed_f16 launch");
  return X2V_OK;
}

extern "C" __attribute__((visibility("default"))) int x2v_clip_preprocess_f16(const float* img, int64_t c_stride, int64_t row_stride, int H, int W, void* out, int64_t ld_out,
                                                                              int image_size, int patch, float mean0, float mean1, float mean2, float std0, float std1,
                                                                              float std2, void* stream) {
  X2V_REQUIRE(img && out, X2V_E_ARG, "clip_preprocess_f16: null pointer");
  X2V_REQUIRE(H > 0 && W > 0 && patch > 0 && image_size >= patch && image_size % patch == 0 && image_size <= 4096, X2V_E_SHAPE,
              "clip_preprocess_f16: bad shape (image_size=%d must be a multiple of patch=%d)", image_size, patch);
  X2V_REQUIRE(row_stride >= W && c_stride >= (int64_t)(H - 1) * row_stride + W, X2V_E_SHAPE, "clip_preprocess_f16: image strides must cover the extents");
  X2V_REQUIRE(ld_out >= 3ll * patch * patch && ld_out < (1ll << 24), X2V_E_SHAPE, "clip_preprocess_f16: ld_out=%lld must cover 3 * patch^2 columns", (long long)ld_out);
  X2V_REQUIRE(std0 != 0.f && std1 != 0.f && std2 != 0.f, X2V_E_ARG, "clip_preprocess_f16: zero std");
  X2V_REQUIRE(aligned16(out), X2V_E_ALIGN, "clip_preprocess_f16: out must be 16-byte aligned");
  const int G = image_size / patch;
  const int64_t total = (int64_t)G * G * ld_out;
  ClipNorm nm{{mean0, mean1, mean2}, {std0, std1, std2}};
  hipLaunchKernelGGL(clip_preprocess_kernel, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 1 << 20)), dim3(256), 0, (hipStream_t)stream, img, c_stride, row_stride, H, W,
                     (_Float16*)out, ld_out, image_size, patch, nm);
  X2V_LAUNCH_CHECK("clip_preprocess_f16 launch");
  return X2V_OK;
}
