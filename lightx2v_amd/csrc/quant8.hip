// Per-token dynamic quantisation of activations for the two w8a8 paths: e4m3fn (BASELINE config #4) and symmetric int8 (the reference's published
// int8 presets).  One kernel, quant8_rowwise_kernel<CH, I8>: the loads, the amax reduction and the store are shared, the scale and the 8-value pack
// are each format's own (quant8.h, which norm.hip's fused LayerNorm form shares).
// HBM-bound: reads M*K bf16, writes M*K bytes + M floats.  One workgroup per row, row held in registers.
#include "rowwise.h"

namespace x2v {

template <int CH, bool I8>
__global__ __launch_bounds__(256) void quant8_rowwise_kernel(const unsigned short* __restrict__ x, int64_t ldx, unsigned char* __restrict__ xq, int64_t ldq,
                                                             float* __restrict__ scale, int K, int kblock, int64_t kblock_stride) {
  __shared__ float red[4];
  const int t = threadIdx.x;
  const int64_t row = blockIdx.x;
  const unsigned short* xr = x + row * ldx;
  float v[CH][8];
  bool ok[CH];
  float amax = 0.f;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int e = (c * 256 + t) * 8;
    ok[c] = e < K;
    if (ok[c]) {
      // K-blocked x (kblock > 0; the Ulysses head->seq receive buffer [N, S/N, (H/N) d]): element e of the row sits in block e / kblock
      const int64_t off = kblock > 0 ? (int64_t)(e / kblock) * kblock_stride + e % kblock : e;
      unpack8(*reinterpret_cast<const uint4*>(xr + off), v[c]);
#pragma unroll
      for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(v[c][j]));
    }
  }
  amax = block_max<4>(amax, red);
  // Each format uses its own of s and inv; inv behind the scale's store is the order the instruction scheduler was handed before the two
  // kernels became one (profiles/w8a8_one_kernel_isa.txt)
  const float s = I8 ? 0.f : e4m3_scale(amax);
  if (t == 0) scale[row] = I8 ? int8_scale(amax) : s;
  const float inv = I8 ? int8_inv_scale(amax) : 0.f;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    if (!ok[c]) continue;
    const int e = (c * 256 + t) * 8;
    uint2 o;
    if constexpr (I8) o = int8_codes8(v[c], inv);
    else o = e4m3_codes8(v[c], s);
    *reinterpret_cast<uint2*>(xq + row * ldq + e) = o;
  }
}

}  // namespace x2v

using namespace x2v;

// `who`: "quant_fp8" or "quant_int8", the prefix of every message
template <bool I8>
static int quant8_rowwise(const char* who, const void* x, int64_t ldx, int kblock, int64_t kblock_stride, void* xq, int64_t ldq, float* scale, int64_t M, int K, void* stream) {
  X2V_REQUIRE(x && xq && scale, X2V_E_ARG, "%s: null pointer", who);
  X2V_REQUIRE(K > 0 && K % 8 == 0 && K <= 16384, X2V_E_SHAPE, "%s: K=%d must be a multiple of 8 and <= 16384", who, K);
  X2V_REQUIRE(ldx % 8 == 0 && ldq % 8 == 0 && aligned16(x) && ((uintptr_t)xq % 8) == 0, X2V_E_ALIGN, "%s: row alignment", who);
  X2V_REQUIRE(kblock == 0 || (kblock > 0 && kblock % 8 == 0 && K % kblock == 0 && kblock_stride % 8 == 0 && ldx >= kblock), X2V_E_SHAPE,
              "%s: x K-block of %d elements must be a multiple of 8 dividing K=%d, block stride a multiple of 8", who, kblock, K);
  if (M <= 0) return X2V_OK;
  int rc = dispatch_ch(chunks_for(K, 4), K, [&](auto chc) {
    hipLaunchKernelGGL((quant8_rowwise_kernel<decltype(chc)::value, I8>), dim3((unsigned)M), dim3(256), 0, (hipStream_t)stream, (const unsigned short*)x, ldx, (unsigned char*)xq, ldq,
                       scale, K, kblock, kblock_stride);
  });
  if (rc != X2V_OK) return rc;
  X2V_LAUNCH_CHECK(I8 ? "quant_int8 launch" : "quant_fp8 launch");
  return X2V_OK;
}

extern "C" __attribute__((visibility("default"))) int x2v_quant_fp8_rowwise_blocked(const void* x, int64_t ldx, int x_kblock, int64_t x_kblock_stride, void* xq, int64_t ldq,
                                                                                   float* scale, int64_t M, int K, void* stream) {
  return quant8_rowwise<false>("quant_fp8", x, ldx, x_kblock, x_kblock_stride, xq, ldq, scale, M, K, stream);
}

extern "C" __attribute__((visibility("default"))) int x2v_quant_fp8_rowwise(const void* x, int64_t ldx, void* xq, int64_t ldq, float* scale, int64_t M, int K, void* stream) {
  return quant8_rowwise<false>("quant_fp8", x, ldx, 0, 0, xq, ldq, scale, M, K, stream);
}

extern "C" __attribute__((visibility("default"))) int x2v_quant_int8_rowwise_blocked(const void* x, int64_t ldx, int x_kblock, int64_t x_kblock_stride, void* xq, int64_t ldq,
                                                                                    float* scale, int64_t M, int K, void* stream) {
  return quant8_rowwise<true>("quant_int8", x, ldx, x_kblock, x_kblock_stride, xq, ldq, scale, M, K, stream);
}

extern "C" __attribute__((visibility("default"))) int x2v_quant_int8_rowwise(const void* x, int64_t ldx, void* xq, int64_t ldq, float* scale, int64_t M, int K, void* stream) {
  return quant8_rowwise<true>("quant_int8", x, ldx, 0, 0, xq, ldq, scale, M, K, stream);
}
