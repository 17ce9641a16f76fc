// The row-wise kernels' shared pieces (norm.hip, quant8.hip): the register row, each statistic / normalise / rotate step written once (the
// quantisers' arithmetic: quant8.h), and the host helpers that turn runtime choices into template arguments.  The per-row and the streaming kernels, and the fused and
// the two-call quantising forms, must agree bit for bit: they do because they run the same helper, not because two texts were kept in step.
// The device helpers take plain arrays (float v[CH][8], bool ok[CH]), so kernels that hold a RowRegs and kernels that hold raw uint4 rows
// call the same ones.
#pragma once
#include <algorithm>
#include <type_traits>

#include "quant8.h"
#include "x2v_common.h"

namespace x2v {

// ------------------------------------------------------------------------------------------------
// Row holder: CH 16-byte chunks per lane, lanes of the row's NW waves interleaved chunk-wise so every
// wave-instruction reads NW... 64 consecutive chunks (1 KiB) — fully coalesced.
template <int CH, int NW>
struct RowRegs {
  float v[CH][8];
  bool ok[CH];
  __device__ __forceinline__ void load(const unsigned short* row, int D, int t) {
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int e = (c * NW * 64 + t) * 8;
      ok[c] = e < D;
      if (ok[c]) {
        uint4 u = *reinterpret_cast<const uint4*>(row + e);
        unpack8(u, v[c]);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[c][j] = 0.f;
      }
    }
  }
};

// The same row still packed (NW = 4), for the streaming kernels: they keep the next row in flight as raw loads.
template <int CH>
__device__ __forceinline__ void load_row_raw(uint4 (&dst)[CH], const unsigned short* row, int D, int t) {
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int e = (c * 256 + t) * 8;
    if (e < D) dst[c] = *reinterpret_cast<const uint4*>(row + e);
    else dst[c] = make_uint4(0u, 0u, 0u, 0u);
  }
}

// Sum over the NW waves that share a row (`red`: 4 floats of LDS; every lane of the block must arrive when NW == 4).
template <int NW>
__device__ __forceinline__ float row_sum(float v, float* red) {
  return (NW == 1) ? wave_sum(v) : block_sum<4>(v, red);
}

// ---- LayerNorm ---------------------------------------------------------------------------------------
// Two-pass statistics of a row of D elements: mean, then the centred variance over the live chunks (dead chunks hold zeros: they add
// nothing to the first sum and are skipped in the second), rstd = 1 / sqrt(var + eps).
template <int CH, int NW>
__device__ __forceinline__ float ln_mean(const float (&v)[CH][8], int D, float* red) {
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < CH; ++c)
#pragma unroll
    for (int j = 0; j < 8; ++j) s += v[c][j];
  s = row_sum<NW>(s, red);
  return s / (float)D;
}
template <int CH, int NW>
__device__ __forceinline__ float ln_rstd(const float (&v)[CH][8], const bool (&ok)[CH], float mean, int D, float eps, float* red) {
  float q = 0.f;
#pragma unroll
  for (int c = 0; c < CH; ++c)
    if (ok[c]) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float d = v[c][j] - mean;
        q += d * d;
      }
    }
  q = row_sum<NW>(q, red);
  return 1.0f / sqrtf(q / (float)D + eps);
}

// One chunk of the output, one rounding (the caller's pack8 or rbf) short of bf16: (v - mean) * rstd, then the operands that are present —
// * w, + b, and the adaLN modulation norm_out.mul_(1 + scale).add_(shift) with its three bf16 roundings.  Each operand comes as a callable
// that returns its packed chunk, called where the operand is used and only if it is present: a per-row kernel's reads global memory there,
// the streaming kernel's returns the chunk it keeps in registers across rows, which leaves its unpacking and rbf(1 + scale) loop-invariant,
// for the optimiser to hoist.
template <typename W, typename B, typename SC, typename SH>
__device__ __forceinline__ void ln_chunk(const float* v, float mean, float rstd, bool has_w, W w, bool has_b, B b, bool has_mod, SC scale, SH shift, float* o) {
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = (v[j] - mean) * rstd;
  if (has_w) {
    float wf[8];
    unpack8(w(), wf);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] *= wf[j];
  }
  if (has_b) {
    float bf[8];
    unpack8(b(), bf);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] += bf[j];
  }
  if (has_mod) {
    float sc[8], sh[8];
    unpack8(scale(), sc);
    unpack8(shift(), sh);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float ln = rbf(o[j]);
      float m = rbf(ln * rbf(1.0f + sc[j]));
      o[j] = m + sh[j];
    }
  }
}

// ---- RMSNorm, both rounding models ---------------------------------------------------------------------
// Sum of squares of one chunk added to ss, in element order.  X2V_ROUND_REF: torch's x.pow(2) is a bf16 tensor, so each square is rounded.
template <int ROUND>
__device__ __forceinline__ float rms_sumsq(const float (&v)[8], float ss) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float p = v[j] * v[j];
    ss += (ROUND == X2V_ROUND_REF) ? rbf(p) : p;
  }
  return ss;
}
template <int ROUND, int CH>
__device__ __forceinline__ float rms_sumsq(const float (&v)[CH][8]) {
  float ss = 0.f;
#pragma unroll
  for (int c = 0; c < CH; ++c) ss = rms_sumsq<ROUND>(v[c], ss);
  return ss;
}
// rstd of a row of n elements from its (reduced) sum of squares
template <int ROUND>
__device__ __forceinline__ float rms_rstd(float ss, float n, float eps) {
  if (ROUND == X2V_ROUND_REF) {
    float mean = rbf(ss / n);       // .mean(-1): fp32 accumulate, bf16 result
    float tt = rbf(mean + eps);     // + eps   → bf16
    return rbf(1.0f / sqrtf(tt));   // rsqrt   → bf16
  }
  return 1.0f / sqrtf(ss / n + eps);
}
// One normalised chunk, its last rounding (the caller's pack8 or rbf) short of bf16.  X2V_ROUND_REF: (x * rstd) → bf16, then * weight → bf16.
template <int ROUND>
__device__ __forceinline__ void rms_norm8(const float* v, float rs, const float* w, float* o) {
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = (ROUND == X2V_ROUND_REF) ? rbf(v[j] * rs) * w[j] : v[j] * rs * w[j];
}

// ---- 3-axis RoPE -----------------------------------------------------------------------------------------
// One complex rotation (a + i b) * (co + i si), then the optional output scale — written with explicit fused multiply-adds so every
// kernel that rotates (per-row and streaming forms) rounds identically whatever the optimiser would contract on its own.
__device__ __forceinline__ void rope_pair(float a, float bb, float co, float si, float oscale, float& o0, float& o1) {
  o0 = __builtin_fmaf(a, co, -(bb * si)) * oscale;
  o1 = __builtin_fmaf(a, si, bb * co) * oscale;
}
// Position of token g (global index) on the (gf, gh, gw) grid; a token beyond the grid is not rotated.
__device__ __forceinline__ void rope3d_pos(int64_t g, int gf, int gh, int gw, bool& rot, int& pf, int& ph, int& pw) {
  rot = g < (int64_t)gf * gh * gw;
  pw = (int)(g % gw), ph = (int)((g / gw) % gh), pf = (int)(g / ((int64_t)gw * gh));
}
// (cos, sin) of complex index ci (0..63 within a head) at that position, from the [1024][64] table: indices 0..21 turn with the frame,
// 22..42 with the row, 43..63 with the column; the identity beyond the grid.
__device__ __forceinline__ float2 rope3d_factor(const float2* __restrict__ cs, bool rot, int pf, int ph, int pw, int ci) {
  if (!rot) return make_float2(1.f, 0.f);
  const int pos = ci < 22 ? pf : (ci < 43 ? ph : pw);
  return cs[pos * 64 + ci];
}
// A 16-byte chunk of a q / k row = 4 (re, im) pairs of one head, complex indices rope_pair0(e) .. + 3: RMS-normalised (has_w; the norm's
// bf16 output feeds RoPE in the reference) or as loaded, then rotated.  w() returns the weight's packed chunk and f(p) pair p's (cos, sin),
// each called where it is used (see ln_chunk).
__device__ __forceinline__ int rope_pair0(int e) { return (e & 127) >> 1; }
template <int ROUND, typename W, typename F>
__device__ __forceinline__ void rms_rope_chunk(const float* v, bool has_w, float rs, W w, F f, float oscale, float* o) {
  float xn[8];
  if (has_w) {
    float wf[8];
    unpack8(w(), wf);
    rms_norm8<ROUND>(v, rs, wf, xn);
#pragma unroll
    for (int j = 0; j < 8; ++j) xn[j] = rbf(xn[j]);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) xn[j] = v[j];
  }
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const float2 cs = f(p);
    rope_pair(xn[2 * p], xn[2 * p + 1], cs.x, cs.y, oscale, o[2 * p], o[2 * p + 1]);
  }
}

}  // namespace x2v

// ---- host: runtime choices to template arguments ------------------------------------------------------------
// 16-byte chunks per lane of a D-element row shared by nw waves
static inline int chunks_for(int D, int nw) { return (D / 8 + nw * 64 - 1) / (nw * 64); }

// Dispatch a runtime chunk count to a compile-time CH (generic lambda receives std::integral_constant).
template <typename F>
static int dispatch_ch(int ch, int D, F&& f) {
  switch (ch) {
    case 1: f(std::integral_constant<int, 1>{}); return X2V_OK;
    case 2: f(std::integral_constant<int, 2>{}); return X2V_OK;
    case 3: f(std::integral_constant<int, 3>{}); return X2V_OK;
    case 4: f(std::integral_constant<int, 4>{}); return X2V_OK;
    case 5: case 6: case 7: case 8: f(std::integral_constant<int, 8>{}); return X2V_OK;
    default: ::x2v::set_error("row too long: D=%d (max 16384)", D); return X2V_E_SHAPE;
  }
}

// Likewise a runtime enumerator (a round_mode, an activation): f receives the first of VALUES... that equals v, the last one if none does.
template <int FIRST, int... REST, typename F>
static void dispatch_value(int v, F&& f) {
  if constexpr (sizeof...(REST) == 0) f(std::integral_constant<int, FIRST>{});
  else if (v == FIRST) f(std::integral_constant<int, FIRST>{});
  else dispatch_value<REST...>(v, f);
}

// Blocks of a 256-thread kernel that are resident on the whole chip at once (occupancy x CUs), queried once per kernel: the grid of
// the persistent "stream" kernels.  0 = query failed (callers fall back to the one-block-per-row form).
template <auto KERNEL>
static int resident_blocks() {
  static int cached = 0;
  if (cached == 0) {
    int dev = 0, nb = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void*)KERNEL, 256, 0) != hipSuccess || nb <= 0)
      return 0;
    cached = nb * prop.multiProcessorCount;
  }
  return cached;
}

// Launches the persistent kernel KERNEL over `rows` rows on min(rows, resident) blocks if the variant allows it: 1 never, 2 always,
// 0 from two rows per resident block on.  false: nothing was launched (also when the occupancy query failed).
template <auto KERNEL, typename... Args>
static bool launch_persistent(int variant, int64_t rows, hipStream_t st, Args... args) {
  const int resident = resident_blocks<KERNEL>();
  if (variant == 1 || resident <= 0 || (variant == 0 && rows < 2 * (int64_t)resident)) return false;
  hipLaunchKernelGGL(KERNEL, dim3((unsigned)std::min<int64_t>(rows, resident)), dim3(256), 0, st, args...);
  return true;
}
