// Shared device helpers for the gfx950 kernels (wave64, MFMA fragment types, bf16 conversion).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "x2v.h"

namespace x2v {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4_t __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef short s16x4_t __attribute__((ext_vector_type(4)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));
typedef int i32x4_t __attribute__((ext_vector_type(4)));
typedef int i32x8_t __attribute__((ext_vector_type(8)));
typedef int i32x16_t __attribute__((ext_vector_type(16)));

constexpr int kWave = 64;  // CDNA wavefront width

// ---- error plumbing (host) -------------------------------------------------------------------------
void set_error(const char* fmt, ...);
// Process-wide A/B switches read ONCE from the environment (latched at first use; x2v_switches reports the effective values so that a bench line
// or a test can record which kernels a process really ran):
int gemm_continuous_switch();      // X2V_GEMM_CONTINUOUS      default 1: bf16 256x256 GEMMs take the continuous pipeline (gemm256c.hip) where the shape allows
int gemm_fp8_continuous_switch();  // X2V_GEMM_FP8_CONTINUOUS  default 2: w8a8 likewise (gemm256c8.hip), block-strided operands included; 1 = row-major only, 0 = ping-pong kernel
int attn_map_switch();             // X2V_ATTN_MAP             default -1: the launcher's rule; 0 / 1 force the plain / XCD-aware work mapping
int attn_rot_switch();             // X2V_ATTN_ROT             default -1: the caller's flag; 0 / 1 force the key walk from tile 0 / staggered
int check_hip(hipError_t e, const char* what);
bool aligned16(const void* p);
// Raise a kernel's dynamic-LDS cap to `bytes` on the current device (once per kernel and device; thread-safe).
int ensure_dynamic_lds(const void* kernel, int bytes, const char* what);

#define X2V_REQUIRE(cond, code, ...) \
  do {                               \
    if (!(cond)) {                   \
      ::x2v::set_error(__VA_ARGS__); \
      return (code);                 \
    }                                \
  } while (0)

#define X2V_LAUNCH_CHECK(what) \
  do {                                                              \
    int _rc = ::x2v::check_hip(hipGetLastError(), what);            \
    if (_rc != X2V_OK) return _rc;                                  \
  } while (0)

// Block addressing of the GEMM kernels (x2v_gemm_bf16_blocked): x may be stored as K-blocks — K-tile kt (128 bytes of a row) at
// (kt / a_kpb) * a_cbs + (kt % a_kpb) * 128 bytes from the row's start — and y as N-blocks — column n at (n / y_cbw) * y_cbs + n % y_cbw
// elements from the row's start.  These are the [N_ranks][S/N][(H/N)d] buffers of the Ulysses exchanges read / written in place.
// a_kpb <= 0 / y_cbw <= 0: plain row-major.
// r_period > 0 (residual epilogue, x2v_gemm_*_resid_period): output row r combines with row r mod r_period of resid — a residual of r_period rows
// fanned out over M rows without being copied.  It sits in the padding the struct had, so the kernels' argument layout is what it was.
struct GemmBlocking {
  int a_kpb = 0;        // K-tiles (128 B) per x block
  unsigned a_cbs = 0;   // bytes between x blocks
  int y_cbw = 0;        // columns per y block (a multiple of 8)
  int r_period = 0;     // rows of resid (0: M, row r reads row r)
  int64_t y_cbs = 0;    // elements between y blocks
};
// Template value of the residual epilogue WITH a row period (never crosses the ABI): a kernel instantiation of its own, so that the kernels of
// X2V_EPI_RESIDUAL keep their instruction streams (tools/isa_diff.py, profiles/gemm_resid_period_isa.txt).
constexpr int EPI_RESIDUAL_PERIODIC = 0x100 | X2V_EPI_RESIDUAL;
constexpr bool epi_is_residual(int epi) { return epi == X2V_EPI_RESIDUAL || epi == EPI_RESIDUAL_PERIODIC; }

// Batch strides and launch form of the pre-transposed-V attention kernel (attn.hip; tools/probes/attn_pc.hip takes the same struct)
struct AttnBatch {
  int64_t q, k, vt, o;  // elements from one sequence of the batch to the next (0: single sequence)
  int xcd_remap;        // bit 0: XCD-aware head-major work mapping (see the kernel), bit 8: staggered key walk; 0: the grid as dispatched, walk from tile 0
};

// ---- bf16 <-> fp32 (device) -------------------------------------------------------------------------
__device__ __forceinline__ float bf2f(unsigned short u) { return __uint_as_float(((unsigned)u) << 16); }
__device__ __forceinline__ float bf_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf_hi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }

// round-to-nearest-even via the hardware v_cvt_pk_bf16_f32 (what `(__bf16)x` lowers to on gfx950)
__device__ __forceinline__ unsigned short f2bf(float x) {
  __bf16 b = (__bf16)x;
  return __builtin_bit_cast(unsigned short, b);
}
__device__ __forceinline__ unsigned pack_bf2(float lo, float hi) {
  bf16x2_t p;
  p[0] = (__bf16)lo;
  p[1] = (__bf16)hi;
  return __builtin_bit_cast(unsigned, p);
}
// round an fp32 value to bf16 precision and back (one reference rounding point)
__device__ __forceinline__ float rbf(float x) { return bf2f(f2bf(x)); }

__device__ __forceinline__ void unpack8(const uint4& v, float* f) {
  f[0] = bf_lo(v.x); f[1] = bf_hi(v.x);
  f[2] = bf_lo(v.y); f[3] = bf_hi(v.y);
  f[4] = bf_lo(v.z); f[5] = bf_hi(v.z);
  f[6] = bf_lo(v.w); f[7] = bf_hi(v.w);
}
__device__ __forceinline__ uint4 pack8(const float* f) {
  uint4 v;
  v.x = pack_bf2(f[0], f[1]);
  v.y = pack_bf2(f[2], f[3]);
  v.z = pack_bf2(f[4], f[5]);
  v.w = pack_bf2(f[6], f[7]);
  return v;
}

// ---- MX block scale (mx.hip's quantisers, attn_mx.hip's) ------------------------------------------------
// e8m0 byte of the smallest power of two >= sf (sf >= 0, fp32 with denormals), saturating at 254: the scale rule of x2v_quant_mxfp8_bf16.
__device__ __forceinline__ unsigned e8m0_ceil(float sf) {
  const unsigned bits = __float_as_uint(sf);
  const unsigned ex = bits >> 23, man = bits & 0x7fffffu;
  unsigned byte;
  if (ex == 0) byte = man > 0x400000u ? 1u : 0u;  // denormal SF: 2^-127 covers (0, 2^-127], 2^-126 the rest
  else byte = ex + (man != 0u ? 1u : 0u);
  return byte > 254u ? 254u : byte;
}
// 2^(127 - byte) as an fp32 (2^-127, a denormal, for byte 254): what a block's values are multiplied by in front of the code conversion
__device__ __forceinline__ float e8m0_inv(unsigned byte) {
  const unsigned e = 254u - byte;
  return __uint_as_float(e >= 1u ? (e << 23) : 0x00400000u);
}
// The MXFP8 block step on N values of a block whose max |x| is amax: returns the block's scale byte e8m0_ceil(amax / 448) and writes the values times
// 2^(127 - byte) as e4m3 codes (RNE; never saturating, since |x| * 2^(127 - byte) <= 448), value j in byte j of the N / 4 dwords w.
template <int N>
__device__ __forceinline__ unsigned mxfp8_block(const float* v, float amax, unsigned* w) {
  const unsigned byte = e8m0_ceil(amax / 448.0f);
  const float inv = e8m0_inv(byte);
#pragma unroll
  for (int j = 0; j < N / 4; ++j) {
    unsigned d = 0;
    d = __builtin_amdgcn_cvt_pk_fp8_f32(v[4 * j] * inv, v[4 * j + 1] * inv, d, false);
    d = __builtin_amdgcn_cvt_pk_fp8_f32(v[4 * j + 2] * inv, v[4 * j + 3] * inv, d, true);
    w[j] = d;
  }
  return byte;
}
// The scale bytes of lanes c, c + s, c + 2 s, c + 3 s (the 4 scale blocks of a row's 128-element K-tile) as one dword in lane c
__device__ __forceinline__ unsigned e8m0_gather4(unsigned byte, int s) {
  return byte | (unsigned)__shfl_down((int)byte, s, 64) << 8 | (unsigned)__shfl_down((int)byte, 2 * s, 64) << 16 | (unsigned)__shfl_down((int)byte, 3 * s, 64) << 24;
}

// ---- activations (fp32 math on a bf16-rounded input, as torch does for bf16 tensors) ------------------
__device__ __forceinline__ float gelu_tanh_f(float x) {
  // torch: 0.5*x*(1+tanh(sqrt(2/pi)*(x+0.044715 x^3)))
  // 0.5*(1+tanh(u)) == 1/(1+exp(-2u)): one v_exp_f32 + one v_rcp_f32 instead of tanhf's long polynomial path
  // (fp32 relative error ~3e-7, far below the bf16 rounding that follows; limits: x -> -inf gives -0, +inf gives x)
  const float kBeta = 0.7978845608028654f, kKappa = 0.044715f;
  const float inner = kBeta * (x + kKappa * x * x * x);
  return x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-2.8853900817779268f * inner));
}
__device__ __forceinline__ float silu_f(float x) { return x / (1.0f + __expf(-x)); }

// The bias and activation step of every GEMM epilogue (tests/gemm_ref.py::finish): four consecutive output columns get their bf16 bias (two packed
// pairs), and an activation takes the sum rounded to bf16.  The dequantisation in front and the pack and store behind differ per kernel and stay there.
// The rule is written as a macro and wrapped by the function: gemm256s.hip expands the macro in place, because through the function call the GELU and
// SiLU instantiations of its one-tile kernel came out with 165 / 84 instructions in another order (profiles/gemm128_mx_merge_isa.txt); every other
// GEMM body calls the function and keeps its instruction stream.
#define X2V_EPI_BIAS_ACT4(EPI, vv, bias01, bias23)                                \
  do {                                                                            \
    (vv)[0] += bf_lo(bias01);                                                     \
    (vv)[1] += bf_hi(bias01);                                                     \
    (vv)[2] += bf_lo(bias23);                                                     \
    (vv)[3] += bf_hi(bias23);                                                     \
    if ((EPI) == X2V_EPI_GELU_TANH) {                                             \
      _Pragma("unroll") for (int e = 0; e < 4; ++e) (vv)[e] = gelu_tanh_f(rbf((vv)[e])); \
    } else if ((EPI) == X2V_EPI_SILU) {                                           \
      _Pragma("unroll") for (int e = 0; e < 4; ++e) (vv)[e] = silu_f(rbf((vv)[e]));      \
    }                                                                             \
  } while (0)
template <int EPI>
__device__ __forceinline__ void epi_bias_act4(float* vv, unsigned bias01, unsigned bias23) {
  X2V_EPI_BIAS_ACT4(EPI, vv, bias01, bias23);
}

// ---- wave / block reductions -------------------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
// Block-wide sum for blockDim.x = NW*64; `red` is NW floats of LDS. Every thread gets the total.
template <int NW>
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  if (NW == 1) return v;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  __syncthreads();  // protect `red` from the previous use
  if (lane == 0) red[wid] = v;
  __syncthreads();
  float t = 0.f;
#pragma unroll
  for (int i = 0; i < NW; ++i) t += red[i];
  return t;
}
template <int NW>
__device__ __forceinline__ float block_max(float v, float* red) {
  v = wave_max(v);
  if (NW == 1) return v;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wid] = v;
  __syncthreads();
  float t = red[0];
#pragma unroll
  for (int i = 1; i < NW; ++i) t = fmaxf(t, red[i]);
  return t;
}

// XCD-aware remap of a 1-D block id: the dispatcher places block b on XCD b % 8 (observed, speed only);
// give every XCD a contiguous chunk of the logical tile space so neighbouring tiles share one L2.
// Bijective for any grid size (cdna_hip_programming.md §5 "XCD swizzle must be bijective").
__device__ __forceinline__ unsigned xcd_remap(unsigned bid, unsigned nblk) {
  const unsigned nx = 8;
  const unsigned q = nblk / nx, r = nblk % nx;
  const unsigned xcd = bid % nx, idx = bid / nx;
  const unsigned base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + idx;
}

}  // namespace x2v
