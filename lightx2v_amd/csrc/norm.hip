// Row-wise HBM-bound kernels of the DiT block: RMSNorm, LayerNorm(+adaLN modulate), fused
// RMSNorm+3-axis RoPE on q/k, gate-residual, activations, timestep sinusoid.
//
// Roofline: each is one read + one write of an [M,D] bf16 tensor (2*M*D*2 bytes) against ~6.3 TB/s
// achievable HBM.  Structure: a row lives entirely in registers between its single 16-byte-vector read
// and its single write (two-pass statistics cost no extra HBM traffic); NW waves cooperate on one row
// (NW=4 for the model dim, NW=1 for short rows so a 256-thread block carries 4 rows).
#include "rowwise.h"

namespace x2v {

template <int CH, int NW, int ROUND>
__global__ __launch_bounds__(256) void rmsnorm_kernel(const unsigned short* __restrict__ x, int64_t ldx, const unsigned short* __restrict__ w,
                                                      unsigned short* __restrict__ y, int64_t ldy, int64_t M, int D, float eps) {
  __shared__ float red[4];
  constexpr int ROWS = 4 / NW;
  const int t = threadIdx.x % (NW * 64);
  const int64_t row = (int64_t)blockIdx.x * ROWS + threadIdx.x / (NW * 64);
  const bool live = row < M;
  RowRegs<CH, NW> r;
  if (live) r.load(x + row * ldx, D, t);
  float ss = 0.f;
  if (live) ss = rms_sumsq<ROUND>(r.v);
  ss = row_sum<NW>(ss, red);
  if (!live) return;
  const float rs = rms_rstd<ROUND>(ss, (float)D, eps);
  unsigned short* yr = y + row * ldy;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    if (!r.ok[c]) continue;
    const int e = (c * NW * 64 + t) * 8;
    float wv[8], o[8];
    unpack8(*reinterpret_cast<const uint4*>(w + e), wv);
    rms_norm8<ROUND>(r.v[c], rs, wv, o);
    *reinterpret_cast<uint4*>(yr + e) = pack8(o);
  }
}

// ln_chunk of the per-row kernels: every operand is read from global memory where ln_chunk uses it.
__device__ __forceinline__ void ln_chunk_at(const float* v, float mean, float rstd, const unsigned short* w, const unsigned short* b, const unsigned short* scale,
                                            const unsigned short* shift, int e, float* o) {
  auto at = [e](const unsigned short* p) { return [p, e] { return *reinterpret_cast<const uint4*>(p + e); }; };
  ln_chunk(v, mean, rstd, w != nullptr, at(w), b != nullptr, at(b), scale != nullptr, at(scale), at(shift), o);
}

// LayerNorm (+ optional affine, + optional adaLN modulate), reference rounding chain.
template <int CH, int NW>
__global__ __launch_bounds__(256) void layernorm_kernel(const unsigned short* __restrict__ x, int64_t ldx, const unsigned short* __restrict__ w,
                                                        const unsigned short* __restrict__ b, const unsigned short* __restrict__ scale,
                                                        const unsigned short* __restrict__ shift, unsigned short* __restrict__ y, int64_t ldy,
                                                        int64_t M, int D, float eps) {
  __shared__ float red[4];
  constexpr int ROWS = 4 / NW;
  const int t = threadIdx.x % (NW * 64);
  const int64_t row = (int64_t)blockIdx.x * ROWS + threadIdx.x / (NW * 64);
  const bool live = row < M;
  RowRegs<CH, NW> r;
  if (live) r.load(x + row * ldx, D, t);
  const float mean = ln_mean<CH, NW>(r.v, D, red);
  const float rstd = ln_rstd<CH, NW>(r.v, r.ok, mean, D, eps, red);
  if (!live) return;
  unsigned short* yr = y + row * ldy;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    if (!r.ok[c]) continue;
    const int e = (c * NW * 64 + t) * 8;
    float o[8];
    ln_chunk_at(r.v[c], mean, rstd, w, b, scale, shift, e, o);
    *reinterpret_cast<uint4*>(yr + e) = pack8(o);
  }
}

// LayerNorm (+affine, +adaLN modulate) fused with the per-token dynamic e4m3 quantisation of its output (w8a8 path): what the reference
// runs as LNWeight.apply + mul_/add_ + scaled_fp8_quant in front of the q / k / v (or ffn_0) projections (mm_weight.py:236-245) — the
// bf16 activation never goes to HBM, and the one quantised copy serves every projection that consumes it.  The normalised values come
// from layernorm_kernel's own ln_mean / ln_rstd / ln_chunk and are rounded to bf16 where that kernel's pack8 rounds them, then quantised by
// quant8.hip's own scale and pack (quant8.h): codes and scales are bit-identical to x2v_layernorm_bf16 followed by x2v_quant_fp8_rowwise.  One block per row.
// I8: the same in front of the per-token int8 quantiser (x2v_layernorm_quant_int8 == x2v_layernorm_bf16 + x2v_quant_int8_rowwise).
template <int CH, bool I8>
__global__ __launch_bounds__(256) void layernorm_quant_kernel(const unsigned short* __restrict__ x, int64_t ldx, const unsigned short* __restrict__ w,
                                                            const unsigned short* __restrict__ b, const unsigned short* __restrict__ scale,
                                                            const unsigned short* __restrict__ shift, unsigned char* __restrict__ xq, int64_t ldq,
                                                            float* __restrict__ sx, int D, float eps) {
  __shared__ float red[4];
  const int t = threadIdx.x;
  const int64_t row = blockIdx.x;
  RowRegs<CH, 4> r;
  r.load(x + row * ldx, D, t);
  const float mean = ln_mean<CH, 4>(r.v, D, red);
  const float rstd = ln_rstd<CH, 4>(r.v, r.ok, mean, D, eps, red);
  float amax = 0.f;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    if (!r.ok[c]) continue;
    const int e = (c * 256 + t) * 8;
    float o[8];
    ln_chunk_at(r.v[c], mean, rstd, w, b, scale, shift, e, o);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      r.v[c][j] = rbf(o[j]);  // the bf16 tensor the reference quantises
      amax = fmaxf(amax, fabsf(r.v[c][j]));
    }
  }
  amax = block_max<4>(amax, red);
  if constexpr (I8) {
    if (t == 0) sx[row] = int8_scale(amax);
    const float inv = int8_inv_scale(amax);
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      if (!r.ok[c]) continue;
      const int e = (c * 256 + t) * 8;
      *reinterpret_cast<uint2*>(xq + row * ldq + e) = int8_codes8(r.v[c], inv);
    }
  } else {
    const float qs = e4m3_scale(amax);
    if (t == 0) sx[row] = qs;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      if (!r.ok[c]) continue;
      const int e = (c * 256 + t) * 8;
      *reinterpret_cast<uint2*>(xq + row * ldq + e) = e4m3_codes8(r.v[c], qs);
    }
  }
}

// Where the q|k norm+RoPE kernels write a row: in place (qo == nullptr), or out of place into N-blocked buffers — column e of token
// `row` at (e / cbw) * cbs + row * ldo + e % cbw: the [N_ranks][S/N][(H/N) d] send buffer of the Ulysses seq->head exchange
// (x2v_rmsnorm_rope_blocked_bf16), so no transposing copy stands between this kernel and the all-to-all.
struct RopeOut {
  unsigned short* qo = nullptr;
  unsigned short* ko = nullptr;
  int64_t ldo = 0, cbs = 0;
  int cbw = 0;
  __device__ __forceinline__ unsigned short* dst(int which, int64_t row, int e, unsigned short* inplace_row) const {
    if (qo == nullptr) return inplace_row + e;
    return (which == 0 ? qo : ko) + (int64_t)(e / cbw) * cbs + row * ldo + e % cbw;
  }
};

// Fused q/k RMSNorm over the full model dim + 3-axis RoPE.  blockIdx.y selects q (0) or k (1).
// One block per token row; D = H*128 so every 16-byte chunk holds 4 (re,im) pairs of one head.
template <int CH, int ROUND>
__global__ __launch_bounds__(256) void rmsnorm_rope_kernel(unsigned short* __restrict__ q, int64_t ldq, unsigned short* __restrict__ k, int64_t ldk,
                                                           const unsigned short* __restrict__ wq, const unsigned short* __restrict__ wk,
                                                           const float2* __restrict__ cs, int64_t S, int D, int64_t s0, int gf, int gh, int gw,
                                                           float eps, float q_out_scale, RopeOut ro) {
  __shared__ float red[4];
  const int t = threadIdx.x;
  const int64_t row = blockIdx.x;
  const float oscale = blockIdx.y == 0 ? q_out_scale : 1.f;  // folded into q's single final rounding (attention prescale)
  unsigned short* base = (blockIdx.y == 0 ? q + row * ldq : k + row * ldk);
  const unsigned short* w = blockIdx.y == 0 ? wq : wk;
  RowRegs<CH, 4> r;
  r.load(base, D, t);
  float rs = 1.f;
  if (w != nullptr) rs = rms_rstd<ROUND>(block_sum<4>(rms_sumsq<ROUND>(r.v), red), (float)D, eps);
  bool rot;
  int pf, ph, pw;
  rope3d_pos(s0 + row, gf, gh, gw, rot, pf, ph, pw);  // s0 + row: this token's global index
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    if (!r.ok[c]) continue;
    const int e = (c * 256 + t) * 8;
    float o[8];
    rms_rope_chunk<ROUND>(
        r.v[c], w != nullptr, rs, [&] { return *reinterpret_cast<const uint4*>(w + e); }, [&](int p) { return rope3d_factor(cs, rot, pf, ph, pw, rope_pair0(e) + p); }, oscale, o);
    *reinterpret_cast<uint4*>(ro.dst(blockIdx.y, row, e, base)) = pack8(o);
  }
}

// ------------------------------------------------------------------------------------------------
// Streaming forms of the two kernels above for long inputs (M >> #CUs; the DiT's [S, D] activations).
// One block per row pays the whole load -> reduce -> reduce -> store chain once per 20 KB and re-fetches / re-unpacks the
// per-channel operands for every row; with ~11 VALU operations per element (three bf16 rounding points) these kernels sit at
// 62-70 % of the achievable bandwidth, issue-bound as much as latency-bound.  Here a block is persistent (grid = what fits the
// chip at once), walks rows blockIdx.x, +gridDim.x, ..., issues the NEXT row's 16-byte loads before the current row's
// reductions, and keeps the per-channel operands (affine / modulation rows with 1 + scale already rounded, norm weights) in
// registers and the token's rotation factors in LDS, fetched once per block / per token instead of once per row.  (A deeper
// prefetch — two rows ahead — measured slower: more registers, fewer resident blocks, and the hoisted operand math gone.)  The arithmetic
// is that of the kernels above, the same helpers of rowwise.h on the same values in the same order: the two forms give bit-identical
// outputs, which tools/x2v_check and tests/test_gpu_edge.py assert.
template <int CH, bool AFF, bool MOD>
__global__ __launch_bounds__(256) void layernorm_stream_kernel(const unsigned short* __restrict__ x, int64_t ldx, const unsigned short* __restrict__ w,
                                                               const unsigned short* __restrict__ b, const unsigned short* __restrict__ scale,
                                                               const unsigned short* __restrict__ shift, unsigned short* __restrict__ y, int64_t ldy,
                                                               int64_t M, int D, float eps) {
  __shared__ float red[4];
  const int t = threadIdx.x;
  // per-channel operands, resident for every row of this block (absent w -> 1.0, absent b -> 0: unused placeholders); the optimiser
  // hoists their unpacking and the rounding of 1 + scale out of the row loop, which is where most of the gain over the per-row form
  // comes from: at 6 TB/s these kernels are as much VALU-issue bound (~11 operations per element) as they are latency bound
  uint4 wv[AFF ? CH : 1], bv[AFF ? CH : 1], scv[MOD ? CH : 1], shv[MOD ? CH : 1];
  bool ok[CH];
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int e = (c * 256 + t) * 8;
    ok[c] = e < D;
    if constexpr (AFF) {
      wv[c] = (ok[c] && w != nullptr) ? *reinterpret_cast<const uint4*>(w + e) : make_uint4(0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u);
      bv[c] = (ok[c] && b != nullptr) ? *reinterpret_cast<const uint4*>(b + e) : make_uint4(0u, 0u, 0u, 0u);
    }
    if constexpr (MOD) {
      scv[c] = ok[c] ? *reinterpret_cast<const uint4*>(scale + e) : make_uint4(0u, 0u, 0u, 0u);
      shv[c] = ok[c] ? *reinterpret_cast<const uint4*>(shift + e) : make_uint4(0u, 0u, 0u, 0u);
    }
  }
  const int64_t stride = gridDim.x;
  int64_t row = blockIdx.x;
  uint4 cur[CH], nxt[CH];
  if (row < M) load_row_raw<CH>(cur, x + row * ldx, D, t);
  for (; row < M; row += stride) {
    if (row + stride < M) load_row_raw<CH>(nxt, x + (row + stride) * ldx, D, t);  // in flight across this row's reductions
    float v[CH][8];
#pragma unroll
    for (int c = 0; c < CH; ++c) unpack8(cur[c], v[c]);
    const float mean = ln_mean<CH, 4>(v, D, red);
    const float rstd = ln_rstd<CH, 4>(v, ok, mean, D, eps, red);
    unsigned short* yr = y + row * ldy;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      if (!ok[c]) continue;
      const int e = (c * 256 + t) * 8;
      float o[8];
      ln_chunk(v[c], mean, rstd, AFF && w != nullptr, [&] { return wv[AFF ? c : 0]; }, AFF && b != nullptr, [&] { return bv[AFF ? c : 0]; }, MOD, [&] { return scv[MOD ? c : 0]; },
               [&] { return shv[MOD ? c : 0]; }, o);
      *reinterpret_cast<uint4*>(yr + e) = pack8(o);
    }
#pragma unroll
    for (int c = 0; c < CH; ++c) cur[c] = nxt[c];
  }
}

// q and k rows of one token are handled back to back by the same block, so the token's 64 rotation factors are gathered once
// (64 lanes, into LDS) instead of 4 scalar 8-byte gathers per 16-byte chunk for q and again for k.
template <int CH, int ROUND>
__global__ __launch_bounds__(256) void rmsnorm_rope_stream_kernel(unsigned short* __restrict__ q, int64_t ldq, unsigned short* __restrict__ k, int64_t ldk,
                                                                  const unsigned short* __restrict__ wq, const unsigned short* __restrict__ wk,
                                                                  const float2* __restrict__ cs, int64_t S, int D, int64_t s0, int gf, int gh, int gw,
                                                                  float eps, float q_out_scale, RopeOut ro) {
  __shared__ float red[4];
  __shared__ __attribute__((aligned(16))) float2 tab[2][64];  // by row parity: staging row n+1 never races readers of row n
  const int t = threadIdx.x;
  const bool has_w = wq != nullptr;
  uint4 wqv[CH], wkv[CH];
  bool ok[CH];
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int e = (c * 256 + t) * 8;
    ok[c] = e < D;
    wqv[c] = (ok[c] && has_w) ? *reinterpret_cast<const uint4*>(wq + e) : make_uint4(0u, 0u, 0u, 0u);
    wkv[c] = (ok[c] && has_w) ? *reinterpret_cast<const uint4*>(wk + e) : make_uint4(0u, 0u, 0u, 0u);
  }
  const int64_t stride = gridDim.x;
  int64_t row = blockIdx.x;
  uint4 cur[CH], nxt[CH];
  if (row < S) load_row_raw<CH>(cur, q + row * ldq, D, t);
  int par = 0;
  for (; row < S; row += stride, par ^= 1) {
    if (t < 64) {  // this token's rotation factors
      bool rot;
      int pf, ph, pw;
      rope3d_pos(s0 + row, gf, gh, gw, rot, pf, ph, pw);
      tab[par][t] = rope3d_factor(cs, rot, pf, ph, pw, t);
    }
#pragma unroll
    for (int which = 0; which < 2; ++which) {
      unsigned short* base = which == 0 ? q + row * ldq : k + row * ldk;
      // the next item (this token's k row, then the next token's q row) is in flight across this item's reduction
      if (which == 0) load_row_raw<CH>(nxt, k + row * ldk, D, t);
      else if (row + stride < S) load_row_raw<CH>(nxt, q + (row + stride) * ldq, D, t);
      const float oscale = which == 0 ? q_out_scale : 1.f;
      float v[CH][8];
#pragma unroll
      for (int c = 0; c < CH; ++c) unpack8(cur[c], v[c]);
      float rs = 1.f;
      if (has_w) rs = rms_rstd<ROUND>(block_sum<4>(rms_sumsq<ROUND>(v), red), (float)D, eps);  // block_sum's barriers also publish tab[par]
      else if (which == 0) __syncthreads();                                                     // publish tab[par]
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        if (!ok[c]) continue;
        const int e = (c * 256 + t) * 8;
        float o[8];
        rms_rope_chunk<ROUND>(v[c], has_w, rs, [&] { return which == 0 ? wqv[c] : wkv[c]; }, [&](int p) { return tab[par][rope_pair0(e) + p]; }, oscale, o);
        *reinterpret_cast<uint4*>(ro.dst(which, row, e, base)) = pack8(o);
      }
#pragma unroll
      for (int c = 0; c < CH; ++c) cur[c] = nxt[c];
    }
  }
}

__global__ __launch_bounds__(256) void gate_residual_kernel(unsigned short* __restrict__ x, int64_t ldx, const unsigned short* __restrict__ y,
                                                            int64_t ldy, const unsigned short* __restrict__ gate, int64_t M, int D) {
  const int cpr = D / 8;
  const int64_t total = M * (int64_t)cpr;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = i / cpr;
    const int e = (int)(i % cpr) * 8;
    float xv[8], yv[8], o[8];
    unpack8(*reinterpret_cast<const uint4*>(x + row * ldx + e), xv);
    unpack8(*reinterpret_cast<const uint4*>(y + row * ldy + e), yv);
    if (gate != nullptr) {
      float gv[8];
      unpack8(*reinterpret_cast<const uint4*>(gate + e), gv);
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = xv[j] + rbf(yv[j] * gv[j]);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = xv[j] + yv[j];
    }
    *reinterpret_cast<uint4*>(x + row * ldx + e) = pack8(o);
  }
}

template <int ACT>
__device__ __forceinline__ float act_f(float x) {
  if constexpr (ACT == X2V_EPI_GELU_TANH) return gelu_tanh_f(x);
  else if constexpr (ACT == X2V_ACT_GELU_ERF) {
    // torch gelu(approximate="none") on a bf16 tensor: fp32 math.  Below -3 the sum 1 + erf cancels (at x < -5.9 to exactly 0, where the
    // function is still ~ -1e-9): there 1 + erf(z) is taken as erfc(-z), which keeps its relative accuracy down the whole tail
    if (x < -3.0f) return 0.5f * x * erfcf(-x * 0.7071067811865476f);
    return 0.5f * x * (1.0f + erff(x * 0.7071067811865476f));
  } else return silu_f(x);
}

template <int ACT>
__global__ __launch_bounds__(256) void activation_kernel(const unsigned short* __restrict__ x, unsigned short* __restrict__ y, int64_t n) {
  const int64_t nv = n / 8;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (int64_t)gridDim.x * blockDim.x) {
    float v[8];
    unpack8(reinterpret_cast<const uint4*>(x)[i], v);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = act_f<ACT>(v[j]);
    reinterpret_cast<uint4*>(y)[i] = pack8(v);
  }
  // tail (n % 8) handled by the first block
  if (blockIdx.x == 0) {
    for (int64_t i = nv * 8 + threadIdx.x; i < n; i += blockDim.x) {
      float f = bf2f(x[i]);
      y[i] = f2bf(act_f<ACT>(f));
    }
  }
}

__global__ void sinusoid_kernel(const int64_t* __restrict__ t, unsigned short* __restrict__ y, int n, int dim) {
  const int half = dim / 2;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n * half; i += gridDim.x * blockDim.x) {
    const int r = i / half, j = i % half;
    // float64 as the reference (utils.py:165-171): pos * 10000^(-j/half)
    const double f = pow(10000.0, -((double)j / (double)half));
    const double a = (double)t[r] * f;
    y[(int64_t)r * dim + j] = f2bf((float)cos(a));
    y[(int64_t)r * dim + half + j] = f2bf((float)sin(a));
  }
}

// The same for fractional timesteps (float64 positions): the step-distill scheduler's timesteps are sigma * 1000 in fp32 (999.87 for step 999 at
// shift 8), and the reference embeds them as they are (utils.py:163 `position.type(torch.float64)`).
__global__ void sinusoid_f64_kernel(const double* __restrict__ t, unsigned short* __restrict__ y, int n, int dim) {
  const int half = dim / 2;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n * half; i += gridDim.x * blockDim.x) {
    const int r = i / half, j = i % half;
    const double f = pow(10000.0, -((double)j / (double)half));
    const double a = t[r] * f;
    y[(int64_t)r * dim + j] = f2bf((float)cos(a));
    y[(int64_t)r * dim + half + j] = f2bf((float)sin(a));
  }
}

// ------------------------------------------------------------------------------------------------
// HunyuanVideo q/k path: per-head RMSNorm over d = 128 followed (for the first `l_rope` tokens = the image
// tokens) by the real-valued RoPE  x*cos + rotate_half(x)*sin  with bf16 cos/sin tables [l_rope, 128] —
// replaces RMSWeightSgl.apply on [L,H,128] (rms_norm_weight.py:102-113) + utils_bf16.apply_rotary_emb
// (hunyuan/infer/utils_bf16.py:5-31), in place on the q and k column blocks of the fused QKV GEMM output.
// 16 lanes x 16 bytes per (token, head) row, 16 rows per 256-thread block; blockIdx.y selects q / k.
// Rounding: X2V_ROUND_REF reproduces the reference's bf16 chain (pow, mean, +eps, rsqrt, *rstd, *w; then the
// three roundings of the rotary form); X2V_ROUND_FP32 keeps fp32 through the norm (sgl_kernel.rmsnorm) and
// rounds once before the (always bf16-chained) rotary step.
template <int ROUND>
__global__ __launch_bounds__(256) void headnorm_rope_kernel(unsigned short* __restrict__ q, int64_t ldq, unsigned short* __restrict__ k, int64_t ldk,
                                                            const unsigned short* __restrict__ wq, const unsigned short* __restrict__ wk,
                                                            const unsigned short* __restrict__ cosb, const unsigned short* __restrict__ sinb, int64_t L,
                                                            int H, int64_t l_rope, float eps, float q_out_scale, int hpb, int64_t cbs) {
  const int sub = threadIdx.x & 15;
  const int64_t row = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  if (row >= L * H) return;  // whole 16-lane groups leave together; the shuffles below stay inside a group
  const int64_t tok = row / H;
  const int head = (int)(row - tok * H);
  // head-blocked operand (hpb < H): heads [j hpb, (j+1) hpb) of every token form the matrix [L][hpb*128] (token stride ld) that starts
  // j * cbs elements into the buffer — the [N_ranks][S/N][(H/N) d] send buffer of the Ulysses exchange
  const int hb = head / hpb;
  unsigned short* base = (blockIdx.y == 0 ? q + tok * ldq : k + tok * ldk) + hb * cbs;
  const unsigned short* w = blockIdx.y == 0 ? wq : wk;
  unsigned short* p = base + (head - hb * hpb) * 128 + sub * 8;
  const float oscale = (blockIdx.y == 0 && ROUND != X2V_ROUND_REF) ? q_out_scale : 1.f;
  float v[8], wv[8];
  unpack8(*reinterpret_cast<const uint4*>(p), v);
  if (w != nullptr) {
    unpack8(*reinterpret_cast<const uint4*>(w + sub * 8), wv);
    float ss = rms_sumsq<ROUND>(v, 0.f);
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
    const float rs = rms_rstd<ROUND>(ss, 128.f, eps);
    // q_out_scale (attention prescale, FP32 mode only): folded into the value's last rounding — for un-rotated (text)
    // rows that is the norm's rounding, for rotated rows the rotary sum's
    const bool scale_here = ROUND != X2V_ROUND_REF && tok >= l_rope;
    rms_norm8<ROUND>(v, rs, wv, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = scale_here ? v[j] * oscale : rbf(v[j]);
  } else if (ROUND != X2V_ROUND_REF && tok >= l_rope) {
    // no norm, no rotation: the store below is the row's one rounding, so the scale goes in front of it (oscale is 1 for k)
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] *= oscale;
  }
  if (tok < l_rope) {
    float c[8], sn[8];
    unpack8(*reinterpret_cast<const uint4*>(cosb + tok * 128 + sub * 8), c);
    unpack8(*reinterpret_cast<const uint4*>(sinb + tok * 128 + sub * 8), sn);
#pragma unroll
    for (int j = 0; j < 8; j += 2) {
      const float re = v[j], im = v[j + 1];
      v[j] = (rbf(re * c[j]) + rbf(-im * sn[j])) * oscale;
      v[j + 1] = (rbf(im * c[j + 1]) + rbf(re * sn[j + 1])) * oscale;
    }
  }
  *reinterpret_cast<uint4*>(p) = pack8(v);
}

}  // namespace x2v

using namespace x2v;

extern "C" __attribute__((visibility("default"))) int x2v_rmsnorm_bf16(const void* x, int64_t ldx, const void* w, void* y, int64_t ldy, int64_t M, int D, float eps, int round_mode,
                                void* stream) {
  X2V_REQUIRE(x && w && y, X2V_E_ARG, "rmsnorm: null pointer");
  X2V_REQUIRE(D > 0 && D % 8 == 0 && D <= 16384, X2V_E_SHAPE, "rmsnorm: D=%d must be a multiple of 8 and <= 16384", D);
  X2V_REQUIRE(ldx % 8 == 0 && ldy % 8 == 0 && aligned16(x) && aligned16(y) && aligned16(w), X2V_E_ALIGN, "rmsnorm: rows must be 16-byte aligned");
  X2V_REQUIRE(round_mode == X2V_ROUND_FP32 || round_mode == X2V_ROUND_REF, X2V_E_ARG, "rmsnorm: bad round_mode %d", round_mode);
  if (M <= 0) return X2V_OK;
  auto xs = (const unsigned short*)x, ws = (const unsigned short*)w;
  auto ys = (unsigned short*)y;
  hipStream_t st = (hipStream_t)stream;
  int rc = X2V_OK;
  dispatch_value<X2V_ROUND_REF, X2V_ROUND_FP32>(round_mode, [&](auto rm) {
    constexpr int ROUND = decltype(rm)::value;
    if (D <= 512) {  // one wave per row, 4 rows per block
      hipLaunchKernelGGL((rmsnorm_kernel<1, 1, ROUND>), dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, xs, ldx, ws, ys, ldy, M, D, eps);
    } else {
      rc = dispatch_ch(chunks_for(D, 4), D, [&](auto chc) {
        hipLaunchKernelGGL((rmsnorm_kernel<decltype(chc)::value, 4, ROUND>), dim3((unsigned)M), dim3(256), 0, st, xs, ldx, ws, ys, ldy, M, D, eps);
      });
    }
  });
  if (rc != X2V_OK) return rc;
  X2V_LAUNCH_CHECK("rmsnorm launch");
  return X2V_OK;
}

extern "C" __attribute__((visibility("default"))) int x2v_layernorm_bf16_variant(const void* x, int64_t ldx, const void* w, const void* b, const void* scale, const void* shift,
                                                                                 void* y, int64_t ldy, int64_t M, int D, float eps, int variant, void* stream) {
  X2V_REQUIRE(x && y, X2V_E_ARG, "layernorm: null pointer");
  X2V_REQUIRE(variant >= 0 && variant <= 2, X2V_E_ARG, "layernorm: unknown variant %d", variant);
  X2V_REQUIRE((scale == nullptr) == (shift == nullptr), X2V_E_ARG, "layernorm: scale and shift must be given together");
  X2V_REQUIRE(D > 0 && D % 8 == 0 && D <= 16384, X2V_E_SHAPE, "layernorm: D=%d must be a multiple of 8 and <= 16384", D);
  X2V_REQUIRE(ldx % 8 == 0 && ldy % 8 == 0 && aligned16(x) && aligned16(y) && aligned16(w) && aligned16(b) && aligned16(scale) && aligned16(shift),
              X2V_E_ALIGN, "layernorm: rows must be 16-byte aligned");
  if (M <= 0) return X2V_OK;
  auto xs = (const unsigned short*)x;
  auto ws = (const unsigned short*)w, bs = (const unsigned short*)b, scs = (const unsigned short*)scale, shs = (const unsigned short*)shift;
  auto ys = (unsigned short*)y;
  hipStream_t st = (hipStream_t)stream;
  if (D <= 512) {
    X2V_REQUIRE(variant != 2, X2V_E_SHAPE, "layernorm: the streaming kernel covers 512 < D <= 8192 (D=%d)", D);
    const unsigned grid = (unsigned)((M + 3) / 4);
    hipLaunchKernelGGL((layernorm_kernel<1, 1>), dim3(grid), dim3(256), 0, st, xs, ldx, ws, bs, scs, shs, ys, ldy, M, D, eps);
  } else {
    const int ch = chunks_for(D, 4);
    const unsigned grid = (unsigned)M;
    const bool aff = ws != nullptr || bs != nullptr, mod = scs != nullptr;
    bool streamed = false;
    int rc = dispatch_ch(ch, D, [&](auto chc) {
      constexpr int CH = decltype(chc)::value;
      if constexpr (CH <= 4) {
        // persistent form for long inputs (bit-identical results; see layernorm_stream_kernel)
        auto go = [&](auto affc, auto modc) {
          streamed = launch_persistent<layernorm_stream_kernel<CH, decltype(affc)::value, decltype(modc)::value>>(variant, M, st, xs, ldx, ws, bs, scs, shs, ys, ldy, M, D, eps);
        };
        if (aff && mod) go(std::true_type{}, std::true_type{});
        else if (aff) go(std::true_type{}, std::false_type{});
        else if (mod) go(std::false_type{}, std::true_type{});
        else go(std::false_type{}, std::false_type{});
      }
      if (!streamed) hipLaunchKernelGGL((layernorm_kernel<CH, 4>), dim3(grid), dim3(256), 0, st, xs, ldx, ws, bs, scs, shs, ys, ldy, M, D, eps);
    });
    if (rc != X2V_OK) return rc;
    X2V_REQUIRE(variant != 2 || streamed, X2V_E_SHAPE, "layernorm: the streaming kernel covers 512 < D <= 8192 (D=%d)", D);
  }
  X2V_LAUNCH_CHECK("layernorm launch");
  return X2V_OK;
}

template <bool I8>
static int layernorm_quant(const char* who, const void* x, int64_t ldx, const void* w, const void* b, const void* scale, const void* shift, void* xq, int64_t ldq, float* sx, int64_t M,
                           int D, float eps, void* stream) {
  X2V_REQUIRE(x && xq && sx, X2V_E_ARG, "%s: null pointer", who);
  X2V_REQUIRE((scale == nullptr) == (shift == nullptr), X2V_E_ARG, "%s: scale and shift must be given together", who);
  X2V_REQUIRE(D > 512 && D % 8 == 0 && D <= 16384, X2V_E_SHAPE, "%s: D=%d must be a multiple of 8 in (512, 16384] (smaller rows: call the two kernels)", who, D);
  X2V_REQUIRE(ldx % 8 == 0 && ldq % 8 == 0 && aligned16(x) && ((uintptr_t)xq % 8) == 0 && aligned16(w) && aligned16(b) && aligned16(scale) && aligned16(shift), X2V_E_ALIGN,
              "%s: row alignment", who);
  if (M <= 0) return X2V_OK;
  const int ch = chunks_for(D, 4);
  int rc = dispatch_ch(ch, D, [&](auto chc) {
    constexpr int CH = decltype(chc)::value;
    hipLaunchKernelGGL((layernorm_quant_kernel<CH, I8>), dim3((unsigned)M), dim3(256), 0, (hipStream_t)stream, (const unsigned short*)x, ldx, (const unsigned short*)w,
                       (const unsigned short*)b, (const unsigned short*)scale, (const unsigned short*)shift, (unsigned char*)xq, ldq, sx, D, eps);
  });
  if (rc != X2V_OK) return rc;
  X2V_LAUNCH_CHECK(I8 ? "layernorm_quant_int8 launch" : "layernorm_quant_fp8 launch");
  return X2V_OK;
}

extern "C" __attribute__((visibility("default"))) int x2v_layernorm_quant_fp8(const void* x, int64_t ldx, const void* w, const void* b, const void* scale, const void* shift,
                                                                              void* xq, int64_t ldq, float* sx, int64_t M, int D, float eps, void* stream) {
  return layernorm_quant<false>("layernorm_quant_fp8", x, ldx, w, b, scale, shift, xq, ldq, sx, M, D, eps, stream);
}

extern "C" __attribute__((visibility("default"))) int x2v_layernorm_quant_int8(const void* x, int64_t ldx, const void* w, const void* b, const void* scale, const void* shift,
                                                                               void* xq, int64_t ldq, float* sx, int64_t M, int D, float eps, void* stream) {
  return layernorm_quant<true>("layernorm_quant_int8", x, ldx, w, b, scale, shift, xq, ldq, sx, M, D, eps, stream);
}

extern "C" __attribute__((visibility("default"))) int x2v_layernorm_bf16(const void* x, int64_t ldx, const void* w, const void* b, const void* scale, const void* shift, void* y,
                                  int64_t ldy, int64_t M, int D, float eps, void* stream) {
  return x2v_layernorm_bf16_variant(x, ldx, w, b, scale, shift, y, ldy, M, D, eps, 0, stream);
}

extern "C" __attribute__((visibility("default"))) int x2v_rmsnorm_rope_bf16(void* q, int64_t ldq, void* k, int64_t ldk, const void* wq, const void* wk, const void* rope_cs, int64_t S,
                                     int H, int64_t s0, int gf, int gh, int gw, float eps, int round_mode, void* stream) {
  return x2v_rmsnorm_rope_scaled_bf16(q, ldq, k, ldk, wq, wk, rope_cs, S, H, s0, gf, gh, gw, eps, round_mode, 1.0f, stream);
}

static int rmsnorm_rope_impl(void* q, int64_t ldq, void* k, int64_t ldk, const void* wq, const void* wk, const void* rope_cs, int64_t S, int H, int64_t s0, int gf, int gh,
                             int gw, float eps, int round_mode, float q_out_scale, int variant, RopeOut ro, void* stream) {
  X2V_REQUIRE(q && k && rope_cs, X2V_E_ARG, "rmsnorm_rope: null pointer");
  X2V_REQUIRE(variant >= 0 && variant <= 2, X2V_E_ARG, "rmsnorm_rope: unknown variant %d", variant);
  X2V_REQUIRE(q_out_scale > 0.f, X2V_E_ARG, "rmsnorm_rope: q_out_scale must be positive");
  X2V_REQUIRE((wq == nullptr) == (wk == nullptr), X2V_E_ARG, "rmsnorm_rope: wq and wk must be given together");
  const int D = H * 128;
  X2V_REQUIRE(H > 0 && D <= 16384, X2V_E_SHAPE, "rmsnorm_rope: H=%d out of range", H);
  X2V_REQUIRE(gf > 0 && gh > 0 && gw > 0 && gf <= 1024 && gh <= 1024 && gw <= 1024, X2V_E_SHAPE, "rmsnorm_rope: grid (%d,%d,%d) out of range", gf, gh, gw);
  X2V_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0 && aligned16(q) && aligned16(k) && aligned16(wq) && aligned16(wk), X2V_E_ALIGN,
              "rmsnorm_rope: rows must be 16-byte aligned");
  X2V_REQUIRE(round_mode == X2V_ROUND_FP32 || round_mode == X2V_ROUND_REF, X2V_E_ARG, "rmsnorm_rope: bad round_mode %d", round_mode);
  if (S <= 0) return X2V_OK;
  const int ch = chunks_for(D, 4);
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((unsigned)S, 2);
  auto qs = (unsigned short*)q, ks = (unsigned short*)k;
  auto wqs = (const unsigned short*)wq, wks = (const unsigned short*)wk;
  auto cs = (const float2*)rope_cs;
  bool streamed = false;
  int rc = dispatch_ch(ch, D, [&](auto chc) {
    constexpr int CH = decltype(chc)::value;
    dispatch_value<X2V_ROUND_REF, X2V_ROUND_FP32>(round_mode, [&](auto rm) {
      constexpr int ROUND = decltype(rm)::value;
      // persistent form for long inputs (bit-identical results; see rmsnorm_rope_stream_kernel)
      if constexpr (CH <= 4) streamed = launch_persistent<rmsnorm_rope_stream_kernel<CH, ROUND>>(variant, S, st, qs, ldq, ks, ldk, wqs, wks, cs, S, D, s0, gf, gh, gw, eps, q_out_scale, ro);
      if (!streamed) hipLaunchKernelGGL((rmsnorm_rope_kernel<CH, ROUND>), grid, dim3(256), 0, st, qs, ldq, ks, ldk, wqs, wks, cs, S, D, s0, gf, gh, gw, eps, q_out_scale, ro);
    });
  });
  if (rc != X2V_OK) return rc;
  X2V_REQUIRE(variant != 2 || streamed, X2V_E_SHAPE, "rmsnorm_rope: the streaming kernel covers D <= 8192 (D=%d)", D);
  X2V_LAUNCH_CHECK("rmsnorm_rope launch");
  return X2V_OK;
}

extern "C" __attribute__((visibility("default"))) int x2v_rmsnorm_rope_scaled_bf16_variant(void* q, int64_t ldq, void* k, int64_t ldk, const void* wq, const void* wk,
                                                                                           const void* rope_cs, int64_t S, int H, int64_t s0, int gf, int gh, int gw, float eps,
                                                                                           int round_mode, float q_out_scale, int variant, void* stream) {
  return rmsnorm_rope_impl(q, ldq, k, ldk, wq, wk, rope_cs, S, H, s0, gf, gh, gw, eps, round_mode, q_out_scale, variant, RopeOut(), stream);
}

extern "C" __attribute__((visibility("default"))) int x2v_rmsnorm_rope_blocked_bf16(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* wq, const void* wk,
                                                                                    const void* rope_cs, void* q_out, void* k_out, int64_t ldo, int block_cols,
                                                                                    int64_t block_stride, int64_t S, int H, int64_t s0, int gf, int gh, int gw, float eps,
                                                                                    int round_mode, float q_out_scale, void* stream) {
  X2V_REQUIRE(q_out && k_out, X2V_E_ARG, "rmsnorm_rope_blocked: null output");
  X2V_REQUIRE(block_cols > 0 && block_cols % 8 == 0 && (H * 128) % block_cols == 0 && ldo % 8 == 0 && ldo >= block_cols && block_stride % 8 == 0 && aligned16(q_out) &&
                  aligned16(k_out),
              X2V_E_SHAPE, "rmsnorm_rope_blocked: block_cols=%d must divide H*128 and be a multiple of 8; ldo / block_stride multiples of 8", block_cols);
  RopeOut ro;
  ro.qo = (unsigned short*)q_out;
  ro.ko = (unsigned short*)k_out;
  ro.ldo = ldo;
  ro.cbw = block_cols;
  ro.cbs = block_stride;
  return rmsnorm_rope_impl((void*)q, ldq, (void*)k, ldk, wq, wk, rope_cs, S, H, s0, gf, gh, gw, eps, round_mode, q_out_scale, 0, ro, stream);
}

extern "C" __attribute__((visibility("default"))) int x2v_rmsnorm_rope_scaled_bf16(void* q, int64_t ldq, void* k, int64_t ldk, const void* wq, const void* wk, const void* rope_cs,
                                                                                   int64_t S, int H, int64_t s0, int gf, int gh, int gw, float eps, int round_mode,
                                                                                   float q_out_scale, void* stream) {
  return x2v_rmsnorm_rope_scaled_bf16_variant(q, ldq, k, ldk, wq, wk, rope_cs, S, H, s0, gf, gh, gw, eps, round_mode, q_out_scale, 0, stream);
}

extern "C" __attribute__((visibility("default"))) int x2v_gate_residual_bf16(void* x, int64_t ldx, const void* y, int64_t ldy, const void* gate, int64_t M, int D, void* stream) {
  X2V_REQUIRE(x && y, X2V_E_ARG, "gate_residual: null pointer");
  X2V_REQUIRE(D > 0 && D % 8 == 0, X2V_E_SHAPE, "gate_residual: D=%d must be a multiple of 8", D);
  X2V_REQUIRE(ldx % 8 == 0 && ldy % 8 == 0 && aligned16(x) && aligned16(y) && aligned16(gate), X2V_E_ALIGN, "gate_residual: rows must be 16-byte aligned");
  if (M <= 0) return X2V_OK;
  const int64_t total = M * (int64_t)(D / 8);
  const unsigned grid = (unsigned)((total + 255) / 256 < 2048 * 4 ? (total + 255) / 256 : 2048 * 4);
  hipLaunchKernelGGL(gate_residual_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (unsigned short*)x, ldx, (const unsigned short*)y, ldy,
                     (const unsigned short*)gate, M, D);
  X2V_LAUNCH_CHECK("gate_residual launch");
  return X2V_OK;
}

extern "C" __attribute__((visibility("default"))) int x2v_activation_bf16(const void* x, void* y, int64_t n, int act, void* stream) {
  X2V_REQUIRE(x && y, X2V_E_ARG, "activation: null pointer");
  X2V_REQUIRE(act == X2V_EPI_GELU_TANH || act == X2V_EPI_SILU || act == X2V_ACT_GELU_ERF, X2V_E_ARG, "activation: unknown act %d", act);
  X2V_REQUIRE(aligned16(x) && aligned16(y), X2V_E_ALIGN, "activation: pointers must be 16-byte aligned");
  if (n <= 0) return X2V_OK;
  const int64_t nv = n / 8;
  const unsigned grid = (unsigned)((nv + 255) / 256 < 8192 ? ((nv + 255) / 256 > 0 ? (nv + 255) / 256 : 1) : 8192);
  dispatch_value<X2V_EPI_GELU_TANH, X2V_ACT_GELU_ERF, X2V_EPI_SILU>(act, [&](auto a) {
    hipLaunchKernelGGL((activation_kernel<decltype(a)::value>), dim3(grid), dim3(256), 0, (hipStream_t)stream, (const unsigned short*)x, (unsigned short*)y, n);
  });
  X2V_LAUNCH_CHECK("activation launch");
  return X2V_OK;
}

extern "C" __attribute__((visibility("default"))) int x2v_sinusoid_embed_bf16(const int64_t* t, void* y, int n, int dim, void* stream) {
  X2V_REQUIRE(t && y, X2V_E_ARG, "sinusoid: null pointer");
  X2V_REQUIRE(n > 0 && dim > 0 && dim % 2 == 0, X2V_E_SHAPE, "sinusoid: n=%d dim=%d", n, dim);
  const int total = n * (dim / 2);
  hipLaunchKernelGGL(sinusoid_kernel, dim3((total + 127) / 128), dim3(128), 0, (hipStream_t)stream, t, (unsigned short*)y, n, dim);
  X2V_LAUNCH_CHECK("sinusoid launch");
  return X2V_OK;
}

extern "C" __attribute__((visibility("default"))) int x2v_sinusoid_embed_f64_bf16(const double* t, void* y, int n, int dim, void* stream) {
  X2V_REQUIRE(t && y, X2V_E_ARG, "sinusoid_f64: null pointer");
  X2V_REQUIRE(n > 0 && dim > 0 && dim % 2 == 0, X2V_E_SHAPE, "sinusoid_f64: n=%d dim=%d", n, dim);
  const int total = n * (dim / 2);
  hipLaunchKernelGGL(sinusoid_f64_kernel, dim3((total + 127) / 128), dim3(128), 0, (hipStream_t)stream, t, (unsigned short*)y, n, dim);
  X2V_LAUNCH_CHECK("sinusoid_f64 launch");
  return X2V_OK;
}

static int headnorm_rope_impl(void* q, int64_t ldq, void* k, int64_t ldk, const void* wq, const void* wk, const void* cos_tab, const void* sin_tab, int64_t L, int H,
                              int64_t l_rope, float eps, int round_mode, float q_out_scale, int hpb, int64_t cbs, void* stream) {
  X2V_REQUIRE(q_out_scale > 0.f, X2V_E_ARG, "headnorm_rope: q_out_scale must be positive");
  X2V_REQUIRE(q && k, X2V_E_ARG, "headnorm_rope: null pointer");
  X2V_REQUIRE(L > 0 && H > 0 && l_rope >= 0 && l_rope <= L, X2V_E_SHAPE, "headnorm_rope: bad shape L=%lld H=%d l_rope=%lld", (long long)L, H, (long long)l_rope);
  X2V_REQUIRE(l_rope == 0 || (cos_tab && sin_tab), X2V_E_ARG, "headnorm_rope: rope tables missing");
  X2V_REQUIRE(hpb > 0 && H % hpb == 0 && cbs >= 0 && cbs % 8 == 0, X2V_E_SHAPE, "headnorm_rope: bad head blocking (H=%d, heads per block %d, block stride %lld)", H, hpb,
              (long long)cbs);
  X2V_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0 && ldq >= (int64_t)hpb * 128 && ldk >= (int64_t)hpb * 128 && aligned16(q) && aligned16(k) && aligned16(wq) && aligned16(wk) &&
                  aligned16(cos_tab) && aligned16(sin_tab),
              X2V_E_ALIGN, "headnorm_rope: rows must be 16-byte aligned");
  const int64_t rows = L * H;
  X2V_REQUIRE((rows + 15) / 16 < (1ll << 31), X2V_E_SHAPE, "headnorm_rope: too many rows");
  dim3 grid((unsigned)((rows + 15) / 16), 2);
  dispatch_value<X2V_ROUND_REF, X2V_ROUND_FP32>(round_mode, [&](auto rm) {
    hipLaunchKernelGGL((headnorm_rope_kernel<decltype(rm)::value>), grid, dim3(256), 0, (hipStream_t)stream, (unsigned short*)q, ldq, (unsigned short*)k, ldk,
                       (const unsigned short*)wq, (const unsigned short*)wk, (const unsigned short*)cos_tab, (const unsigned short*)sin_tab, L, H, l_rope, eps, q_out_scale, hpb,
                       cbs);
  });
  X2V_LAUNCH_CHECK("headnorm_rope launch");
  return X2V_OK;
}

extern "C" __attribute__((visibility("default"))) int x2v_headnorm_rope_bf16(void* q, int64_t ldq, void* k, int64_t ldk, const void* wq, const void* wk, const void* cos_tab,
                                                                             const void* sin_tab, int64_t L, int H, int64_t l_rope, float eps, int round_mode,
                                                                             float q_out_scale, void* stream) {
  return headnorm_rope_impl(q, ldq, k, ldk, wq, wk, cos_tab, sin_tab, L, H, l_rope, eps, round_mode, q_out_scale, H, 0, stream);
}

extern "C" __attribute__((visibility("default"))) int x2v_headnorm_rope_blocked_bf16(void* q, void* k, int64_t ld, int heads_per_block, int64_t block_stride, const void* wq,
                                                                                     const void* wk, const void* cos_tab, const void* sin_tab, int64_t L, int H, int64_t l_rope,
                                                                                     float eps, int round_mode, float q_out_scale, void* stream) {
  return headnorm_rope_impl(q, ld, k, ld, wq, wk, cos_tab, sin_tab, L, H, l_rope, eps, round_mode, q_out_scale, heads_per_block, block_stride, stream);
}
