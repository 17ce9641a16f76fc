// The arithmetic of the two per-token dynamic quantisers, shared by quant8.hip and norm.hip's fused LayerNorm form so that the two give the same bits.
// int8, symmetric: restated from vLLM's dynamic `scaled_int8_quant(x, scale=None, azp=None, symmetric=True)` (reference call site
// mm_weight.py:247-249); every operation is one correctly rounded fp32 operation:
//   scale = amax / 127,  inv = 127 / amax,  q = clamp(rint(x * inv), -128, 127)  (round half to even)
// An all-zero row has inv = 0 (not 127 / 0): codes 0, scale 0, and no NaN reaches the codes.
// e4m3fn: reference mm_weight.py:236-245 -> vLLM's dynamic per-token `scaled_fp8_quant`:
//   scale = max(amax / 448, 1 / (448 * 512)),  q = e4m3(clamp(x / scale, -448, 448)): a division per element, and a floor under the scale
//   (an all-zero row: codes 0, scale = the floor).
#pragma once
#include "x2v_common.h"

namespace x2v {

__device__ __forceinline__ float int8_scale(float amax) { return amax / 127.0f; }
__device__ __forceinline__ float int8_inv_scale(float amax) { return amax > 0.f ? 127.0f / amax : 0.f; }
__device__ __forceinline__ unsigned int8_code(float x, float inv) {
  const float r = fminf(fmaxf(__builtin_rintf(x * inv), -128.f), 127.f);  // fmaxf drops a NaN: it becomes -128, never an undefined conversion
  return (unsigned)(int)r & 0xffu;
}
// 8 consecutive codes, element 0 in the lowest byte
__device__ __forceinline__ uint2 int8_codes8(const float* x, float inv) {
  uint2 o;
  o.x = int8_code(x[0], inv) | (int8_code(x[1], inv) << 8) | (int8_code(x[2], inv) << 16) | (int8_code(x[3], inv) << 24);
  o.y = int8_code(x[4], inv) | (int8_code(x[5], inv) << 8) | (int8_code(x[6], inv) << 16) | (int8_code(x[7], inv) << 24);
  return o;
}

__device__ __forceinline__ float e4m3_scale(float amax) { return fmaxf(amax / 448.0f, 1.0f / (448.0f * 512.0f)); }
// 8 consecutive codes, element 0 in the lowest byte
__device__ __forceinline__ uint2 e4m3_codes8(const float* x, float s) {
  float q[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) q[j] = fminf(fmaxf(x[j] / s, -448.f), 448.f);
  unsigned lo = 0, hi = 0;
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(q[0], q[1], lo, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(q[2], q[3], lo, true);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(q[4], q[5], hi, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(q[6], q[7], hi, true);
  return make_uint2(lo, hi);
}

}  // namespace x2v
