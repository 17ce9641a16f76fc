// The kernels of HunyuanVideo's two text towers (fp16, as the reference runs them: runners/hunyuan/hunyuan_runner.py:30-37,58-67).
// reference: models/input_encoders/hf/llama/model.py (TextEncoderHFLlamaModel: transformers' LlamaModel, hidden_states[-3]) and
// models/input_encoders/hf/clip/model.py (TextEncoderHFClipModel: transformers' CLIPTextModel, pooler_output).  The Linears are gemm_rows_kernel<_Float16>
// (x2v_gemm_f16, clip.hip) with the quick-GELU and SwiGLU epilogues, the LayerNorm is x2v_layernorm_f16.
//
// attn_f16_causal_kernel<D> — causal attention, head dim 64 or 128, grouped-query (query head h reads key/value head h / (H / Hkv)), over packed sequences
//   of 1..512 tokens; q | k | v read in place from the fused QKV GEMM's output rows.  Workgroup = (64 query rows, one query head of one sequence); the
//   sequence bounds arrive by value.  It walks the 64-key tiles 0 .. its own diagonal tile: K [64][D] and V^T [D][64] of one tile live in LDS (35 KiB at
//   D = 128).  Built from enc_attn.h's steps (the staging, lane and fragment convention is described there).  With rope tables given (D = 128), q (in
//   registers) and k (while it is staged, in a loop of its own over half rows) are rotated in fp32, rotate-half at position = index within the sequence,
//   and rounded once to fp16.  The running maximum, exp and sum of a query's row are fp32 in registers (online softmax), the diagonal tile masks
//   key > query to -inf (probability exactly 0).
// rmsnorm_f16_kernel — RMSNorm of an fp16 row with an fp16 weight: rowwise.h's statistic and normalise steps (X2V_ROUND_FP32), one rounding.
#include <math.h>

#include "enc_attn.h"
#include "rowwise.h"
#include "x2v_common.h"

namespace x2v {

constexpr int CA_TILE = 64;           // keys per tile = query rows per workgroup
constexpr int CA_VP = CA_TILE + 8;    // V^T row pitch in halves (144 B: 8-byte aligned fragments)

template <int D>
__global__ __launch_bounds__(256) void attn_f16_causal_kernel(const _Float16* __restrict__ qkv, int64_t ld, _Float16* __restrict__ out, int64_t ldo, PackedSeqs seqs, int H,
                                                              int Hkv, const float* __restrict__ rope_cos, const float* __restrict__ rope_sin, float scale_log2e) {
  constexpr int KP = D + 8;     // K row pitch in halves
  constexpr int KS = D / 32;    // k-steps of S^T = K . Q^T
  constexpr int HD = D / 2;     // the rotation's partner distance = the tables' row length
  __shared__ __attribute__((aligned(16))) _Float16 Ks[CA_TILE * KP];
  __shared__ __attribute__((aligned(16))) _Float16 Vt[D * CA_VP];
  const EncLanes L = enc_lanes();
  const int tid = L.tid, g4 = L.g4;
  const int b = blockIdx.y / H, h = blockIdx.y % H, qb = blockIdx.x;
  const int row0 = seqs.cu[b], len = seqs.cu[b + 1] - row0;
  if (qb * CA_TILE >= len) return;  // the whole workgroup: the grid is sized for the longest sequence
  const int hkv = h / (H / Hkv);
  const _Float16* qbase = qkv + (int64_t)row0 * ld + h * D;
  const _Float16* kbase = qkv + (int64_t)row0 * ld + (int64_t)H * D + hkv * D;
  const _Float16* vbase = kbase + (int64_t)Hkv * D;
  const bool rope = rope_cos != nullptr;

  const int q = enc_query(L, qb);
  const int qr = enc_read_row(q, len);
  const bool active = qb * CA_TILE + L.wid * 16 < len;  // a wave without queries only helps staging
  half8_t qf[KS];
  load_q<_Float16, KS>(qbase + (int64_t)qr * ld, g4, qf);
  if constexpr (D == 128) {
    if (rope) {  // out[i] = t[i] cos[i] - t[i + 64] sin[i] (i < 64), out[i + 64] = t[i + 64] cos[i] + t[i] sin[i]
#pragma unroll
      for (int ks = 0; ks < KS / 2; ++ks) {
        const float* cr = rope_cos + (int64_t)qr * HD + 32 * ks + 8 * g4;
        const float* sr = rope_sin + (int64_t)qr * HD + 32 * ks + 8 * g4;
        const half8_t lo = qf[ks], hi = qf[ks + KS / 2];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float a = (float)lo[e], bb = (float)hi[e], co = cr[e], si = sr[e];
          qf[ks][e] = (_Float16)(a * co - bb * si);
          qf[ks + KS / 2][e] = (_Float16)(bb * co + a * si);
        }
      }
    }
  }

  f32x4_t o[D / 16];
#pragma unroll
  for (int c = 0; c < D / 16; ++c) o[c] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float mx = -INFINITY, sum = 0.f;  // the running maximum of the query's row, and this lane's share of its sum

  for (int kt = 0; kt <= qb; ++kt) {
    const int k0 = kt * CA_TILE;
    __syncthreads();  // the previous tile has been read
    if (D == 128 && rope) {
      for (int i = tid; i < CA_TILE * (HD / 8); i += 256) {
        const int key = i / (HD / 8), ch = i % (HD / 8);
        half8_t lo = {}, hi = {};
        if (k0 + key < len) {
          const _Float16* kr = kbase + (int64_t)(k0 + key) * ld + ch * 8;
          const float* cr = rope_cos + (int64_t)(k0 + key) * HD + ch * 8;
          const float* sr = rope_sin + (int64_t)(k0 + key) * HD + ch * 8;
          const half8_t tl = *reinterpret_cast<const half8_t*>(kr), th = *reinterpret_cast<const half8_t*>(kr + HD);
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float a = (float)tl[e], bb = (float)th[e], co = cr[e], si = sr[e];
            lo[e] = (_Float16)(a * co - bb * si);
            hi[e] = (_Float16)(bb * co + a * si);
          }
        }
        *reinterpret_cast<half8_t*>(Ks + key * KP + ch * 8) = lo;
        *reinterpret_cast<half8_t*>(Ks + key * KP + HD + ch * 8) = hi;
      }
    } else {
      stage_k<_Float16, D, CA_TILE, KP>(Ks, kbase, ld, k0, len, tid);
    }
    stage_vt<_Float16, D, CA_TILE, CA_VP>(Vt, vbase, ld, k0, len, tid);
    __syncthreads();
    if (!active) continue;

    // scores: sc[t][e] = q . k[k0 + 16 t + 4 g4 + e]
    f32x4_t sc[4];
    float tmx = -INFINITY;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      f32x4_t a = score_tile<_Float16, KS, KP>(Ks, t, L, qf);
      if (kt == qb) {  // the diagonal tile: keys behind the query (and with them every key beyond the sequence) are masked
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (k0 + 16 * t + 4 * g4 + e > q) a[e] = -INFINITY;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) tmx = fmaxf(tmx, a[e]);
      sc[t] = a;
    }
    tmx = quad_max(tmx);  // finite: the tile's first key is never behind a query of this block
    const float mnew = fmaxf(mx, tmx);
    const float alpha = __builtin_amdgcn_exp2f((mx - mnew) * scale_log2e);  // 0 at the first tile (mx = -inf)
    mx = mnew;
    sum *= alpha;
#pragma unroll
    for (int c = 0; c < D / 16; ++c)
#pragma unroll
      for (int e = 0; e < 4; ++e) o[c][e] *= alpha;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float p = __builtin_amdgcn_exp2f((sc[t][e] - mnew) * scale_log2e);
        sc[t][e] = p;
        sum += p;
      }
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) pv_step<_Float16, D / 16, CA_VP>(Vt, kk, sc[2 * kk], sc[2 * kk + 1], L, o);
  }
  if (q >= len) return;
  sum = quad_sum(sum);
  store_out<_Float16, D / 16>(out + (int64_t)(row0 + q) * ldo + h * D, o, 1.0f / sum, g4);
}

// ---- RMSNorm ---------------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void unpack8h(const half8_t& h, float* f) {
#pragma unroll
  for (int e = 0; e < 8; ++e) f[e] = (float)h[e];
}

// CH 16-byte chunks per lane of a row shared by NW waves, chunk-interleaved as RowRegs lays them out; 4 / NW rows per block.
template <int CH, int NW>
__global__ __launch_bounds__(256) void rmsnorm_f16_kernel(const _Float16* __restrict__ x, int64_t ldx, const _Float16* __restrict__ w, _Float16* __restrict__ y, int64_t ldy,
                                                          int64_t M, int D, float eps) {
  __shared__ float red[4];
  constexpr int ROWS = 4 / NW;
  const int t = threadIdx.x % (NW * 64);
  const int64_t row = (int64_t)blockIdx.x * ROWS + threadIdx.x / (NW * 64);
  const bool live = row < M;
  float v[CH][8];
  bool ok[CH];
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int e = (c * NW * 64 + t) * 8;
    ok[c] = live && e < D;
    half8_t hv = {};
    if (ok[c]) hv = *reinterpret_cast<const half8_t*>(x + row * ldx + e);
    unpack8h(hv, v[c]);
  }
  const float ss = row_sum<NW>(rms_sumsq<X2V_ROUND_FP32, CH>(v), red);
  if (!live) return;
  const float rs = rms_rstd<X2V_ROUND_FP32>(ss, (float)D, eps);
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    if (!ok[c]) continue;
    const int e = (c * NW * 64 + t) * 8;
    float wv[8], o[8];
    unpack8h(*reinterpret_cast<const half8_t*>(w + e), wv);
    rms_norm8<X2V_ROUND_FP32>(v[c], rs, wv, o);
    half8_t r;
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = (_Float16)o[j];
    *reinterpret_cast<half8_t*>(y + row * ldy + e) = r;
  }
}

}  // namespace x2v

using namespace x2v;

extern "C" __attribute__((visibility("default"))) int x2v_attn_f16_causal(const void* qkv, int64_t ld, void* out, int64_t ldo, const int* cu_seqlens, int batch, int num_heads,
                                                                          int num_kv_heads, int head_dim, const float* rope_cos, const float* rope_sin, float scale,
                                                                          void* stream) {
  X2V_REQUIRE(qkv && out && cu_seqlens, X2V_E_ARG, "attn_f16_causal: null pointer");
  X2V_REQUIRE(head_dim == 64 || head_dim == 128, X2V_E_SHAPE, "attn_f16_causal: head_dim=%d must be 64 or 128", head_dim);
  X2V_REQUIRE((rope_cos == nullptr) == (rope_sin == nullptr), X2V_E_ARG, "attn_f16_causal: rope_cos and rope_sin must be given together");
  X2V_REQUIRE(rope_cos == nullptr || head_dim == 128, X2V_E_ARG, "attn_f16_causal: the rotary tables go with head_dim 128 only (got %d)", head_dim);
  PackedSeqs seqs;
  int longest;
  int rc = packed_seqs_check("attn_f16_causal", cu_seqlens, batch, ENC_MAXLEN, "this kernel (and its rotary tables) takes", &seqs, &longest);
  if (rc != X2V_OK) return rc;
  X2V_REQUIRE(num_heads > 0 && num_kv_heads > 0 && num_heads % num_kv_heads == 0 && (int64_t)batch * num_heads < 65536, X2V_E_SHAPE,
              "attn_f16_causal: bad head counts %d / %d (query heads must be a multiple of key/value heads)", num_heads, num_kv_heads);
  X2V_REQUIRE(scale == scale && scale >= 0.f && scale <= 3.0e38f, X2V_E_ARG, "attn_f16_causal: scale must be finite and >= 0 (0 = head_dim^-1/2)");
  const int64_t cols = ((int64_t)num_heads + 2 * num_kv_heads) * head_dim;
  X2V_REQUIRE(ld >= cols && ldo >= (int64_t)num_heads * head_dim && ld % 8 == 0 && ldo % 4 == 0, X2V_E_ALIGN,
              "attn_f16_causal: ld must cover [q | k | v] of %d + 2 x %d heads x %d (a multiple of 8 halves), ldo the output row (of 4)", num_heads, num_kv_heads, head_dim);
  X2V_REQUIRE(aligned16(qkv) && aligned16(out) && aligned16(rope_cos) && aligned16(rope_sin), X2V_E_ALIGN, "attn_f16_causal: pointers must be 16-byte aligned");
  if (scale == 0.f) scale = 1.0f / sqrtf((float)head_dim);
  const dim3 grid((unsigned)((longest + CA_TILE - 1) / CA_TILE), (unsigned)(batch * num_heads));
  const float sl2 = scale * 1.4426950408889634f;
  if (head_dim == 128)
    hipLaunchKernelGGL(attn_f16_causal_kernel<128>, grid, dim3(256), 0, (hipStream_t)stream, (const _Float16*)qkv, ld, (_Float16*)out, ldo, seqs, num_heads, num_kv_heads,
                       rope_cos, rope_sin, sl2);
  else
    hipLaunchKernelGGL(attn_f16_causal_kernel<64>, grid, dim3(256), 0, (hipStream_t)stream, (const _Float16*)qkv, ld, (_Float16*)out, ldo, seqs, num_heads, num_kv_heads,
                       rope_cos, rope_sin, sl2);
  X2V_LAUNCH_CHECK("attn_f16_causal launch");
  return X2V_OK;
}

extern "C" __attribute__((visibility("default"))) int x2v_rmsnorm_f16(const void* x, int64_t ldx, const void* w, void* y, int64_t ldy, int64_t M, int D, float eps,
                                                                      void* stream) {
  X2V_REQUIRE(x && w && y, X2V_E_ARG, "rmsnorm_f16: null pointer");
  X2V_REQUIRE(M >= 0 && M < (1ll << 31) && D > 0 && D % 8 == 0 && D <= 8192, X2V_E_SHAPE, "rmsnorm_f16: D=%d must be a multiple of 8, at most 8192", D);
  X2V_REQUIRE(ldx >= D && ldy >= D && ldx % 8 == 0 && ldy % 8 == 0, X2V_E_ALIGN, "rmsnorm_f16: leading dimensions must be multiples of 8 halves covering D");
  X2V_REQUIRE(aligned16(x) && aligned16(y) && aligned16(w), X2V_E_ALIGN, "rmsnorm_f16: pointers must be 16-byte aligned");
  if (M == 0) return X2V_OK;
  hipStream_t st = (hipStream_t)stream;
  auto xp = (const _Float16*)x, wp = (const _Float16*)w;
  auto yp = (_Float16*)y;
  if (D <= 512) {  // one wave per row, 4 rows per block
    hipLaunchKernelGGL((rmsnorm_f16_kernel<1, 1>), dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, xp, ldx, wp, yp, ldy, M, D, eps);
  } else {
    int rc = dispatch_ch(chunks_for(D, 4), D, [&](auto chc) {
      hipLaunchKernelGGL((rmsnorm_f16_kernel<decltype(chc)::value, 4>), dim3((unsigned)M), dim3(256), 0, st, xp, ldx, wp, yp, ldy, M, D, eps);
    });
    if (rc != X2V_OK) return rc;
  }
  X2V_LAUNCH_CHECK("rmsnorm_f16 launch");
  return X2V_OK;
}
