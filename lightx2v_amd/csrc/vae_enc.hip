// The Wan VAE encoder's own kernels: the stride-2 downsampling convolution and the producer that turns the caller's [3, T, H, W] video into the first
// convolution's operand buffer.  Everything else of the encoder (3x3x3 causal convolutions, RMS_norm + SiLU producers, the attention block, the (3,1,1)
// time convolution one output frame per launch) runs on the decoder's kernels (vae.hip, vae16g.hip).
// reference: models/video_encoders/hf/wan/vae.py — Resample downsample2d / downsample3d :96-100,141-158 (nn.ZeroPad2d((0, 1, 0, 1)) + nn.Conv2d(dim, dim, 3,
// stride=(2, 2))), Encoder3d.conv1 :286 (CausalConv3d(3, 96, 3, padding=1)), WanVAE_.encode :684-711.
//
// vae_conv_s2_kernel — y[t,oy,ox,co] = bias[co] + sum_{dh,dw,c} x[t, 2 oy + dh, 2 ox + dw, c] w[co, dh, dw, c], input rows >= Hin / columns >= Win read as zero
// (the bottom / right ZeroPad2d: the kernel bounds its reads, so the operand buffer needs no border).  Implicit GEMM on v_mfma_f32_16x16x32_f16, D = W . X as in
// vae16g.hip (a lane ends up with 4 consecutive couts of one pixel: 16-byte channels-last stores):
//   * workgroup = 4 waves, output tile 16 x 16 pixels of one frame x 96 couts; wave = 4 output rows x 16 pixels x 96 couts = 4 x 6 accumulator tiles (96 VGPRs);
//   * per 32-channel slab the (2 * 16 + 1) x (2 * 16 + 1) input tile is staged once in LDS (70 KiB: two workgroups per CU, one's staging under the other's MFMAs)
//     and serves the nine taps; its columns are stored de-interleaved by parity (even columns 0..32, then odd 1..31, 17 slots each), so the 16 pixels of a
//     fragment read — input columns 2 ox + dw — are 16 CONSECUTIVE 64-byte slots, as in a stride-1 convolution; chunk index XOR 2 ((slot >> 2) & 1) (vae16g.hip);
//   * weight fragments straight from global memory (the whole weight tensor is <= 8 MiB and read by every workgroup: L2-resident);
//   * per tap 24 MFMAs against 4 LDS and 6 global fragment reads.
// The reduction order of an output value is (slab, dh, dw, channel), independent of T, of the tile position and of the launch: frame batching is bit-identical.
// In the hi/lo split mode the operands are [hi | hi * 2^-12 | lo] (activations, x2v_vae_prep_split_f16) against [hi | lo * 2^12 | hi] (weights): fp32-grade.
#include <algorithm>

#include "x2v_common.h"

namespace x2v {

typedef _Float16 s2_half8_t __attribute__((ext_vector_type(8)));

constexpr int S2_TH = 16, S2_TW = 16;                  // output tile
constexpr int S2_HR = 2 * S2_TH + 1, S2_HC = 2 * S2_TW + 1;  // input tile 33 x 33
constexpr int S2_SLOTS = 2 * (S2_TW + 1);              // 34 slots per input row: 17 even columns, 17 (16 used) odd
constexpr int S2_LDS = S2_HR * S2_SLOTS * 64;          // 71808 B
constexpr int S2_NCB = 6;                              // cout blocks of 16 per workgroup

__device__ __forceinline__ int s2_slot_addr(int s, int chunk) { return s * 64 + ((chunk ^ (((s >> 2) & 1) << 1)) << 4); }

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void vae_conv_s2_kernel(const _Float16* __restrict__ xp, int64_t fs, int64_t rs, int64_t ps, const _Float16* __restrict__ w, int64_t wrs,
                                                          const float* __restrict__ bias, float* __restrict__ y, int Hin, int Win, int Ho, int Wo, int Cin, int Cout,
                                                          int tiles_x, int tiles_y, int ncol) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int c16 = lane & 15, g4 = lane >> 4;
  unsigned b = blockIdx.x;
  const int cbk = (int)(b % (unsigned)ncol);  // cout blocks of one pixel tile are neighbours: they share the staged input in L2
  b /= (unsigned)ncol;
  const int tx = (int)(b % (unsigned)tiles_x);
  b /= (unsigned)tiles_x;
  const int ty = (int)(b % (unsigned)tiles_y);
  const int t = (int)(b / (unsigned)tiles_y);
  const int oy0 = ty * S2_TH, ox0 = tx * S2_TW, co0 = cbk * 16 * S2_NCB;
  const int iy0 = 2 * oy0, ix0 = 2 * ox0;
  const _Float16* xf = xp + (int64_t)t * fs;

  // weight rows of this lane (row c16 of each cout block); rows at or beyond Cout read as zero
  const _Float16* wrow[S2_NCB];
  bool wlive[S2_NCB];
#pragma unroll
  for (int cb = 0; cb < S2_NCB; ++cb) {
    const int co = co0 + cb * 16 + c16;
    wlive[cb] = co < Cout;
    wrow[cb] = w + (int64_t)(wlive[cb] ? co : 0) * wrs + g4 * 8;
  }

  f32x4_t acc[S2_NCB][4];
#pragma unroll
  for (int cb = 0; cb < S2_NCB; ++cb)
#pragma unroll
    for (int pb = 0; pb < 4; ++pb) acc[cb][pb] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  const int nslabs = Cin / 32;
  for (int kc = 0; kc < nslabs; ++kc) {
    __syncthreads();  // the previous slab's fragment reads are done
    for (int i = tid; i < S2_HR * S2_HC * 4; i += 256) {
      const int q = i & 3, p = i >> 2;
      const int r = p / S2_HC, c = p - r * S2_HC;
      const int iy = iy0 + r, ix = ix0 + c;
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (iy < Hin && ix < Win) v = *reinterpret_cast<const uint4*>(xf + (int64_t)iy * rs + (int64_t)ix * ps + kc * 32 + q * 8);
      *reinterpret_cast<uint4*>(smem + s2_slot_addr(r * S2_SLOTS + (c & 1) * (S2_TW + 1) + (c >> 1), q)) = v;
    }
    __syncthreads();
#pragma unroll 1
    for (int dh = 0; dh < 3; ++dh)  // a tap row per iteration: unrolled over all nine taps the weight loads are hoisted into 400 registers
#pragma unroll
    for (int dw = 0; dw < 3; ++dw) {
      const int tap = dh * 3 + dw;
      s2_half8_t wf[S2_NCB], xfr[4];
#pragma unroll
      for (int cb = 0; cb < S2_NCB; ++cb) {
        wf[cb] = wlive[cb] ? *reinterpret_cast<const s2_half8_t*>(wrow[cb] + tap * Cin + kc * 32) : s2_half8_t{};
      }
#pragma unroll
      for (int pb = 0; pb < 4; ++pb) {
        const int s = (2 * (4 * wid + pb) + dh) * S2_SLOTS + (dw & 1) * (S2_TW + 1) + (dw >> 1) + c16;
        xfr[pb] = *reinterpret_cast<const s2_half8_t*>(smem + s2_slot_addr(s, g4));
      }
#pragma unroll
      for (int cb = 0; cb < S2_NCB; ++cb)
#pragma unroll
        for (int pb = 0; pb < 4; ++pb) acc[cb][pb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[cb], xfr[pb], acc[cb][pb], 0, 0, 0);
    }
  }

  // epilogue: acc[cb][pb][e] = output pixel (oy0 + 4 wid + pb, ox0 + c16), cout co0 + 16 cb + 4 g4 + e.  Every lane is bounded by the last row, the last
  // column and the cout tail (Cout % 4 == 0: a 4-cout group is wholly inside or wholly outside)
  const int ox = ox0 + c16;
#pragma unroll
  for (int pb = 0; pb < 4; ++pb) {
    const int oy = oy0 + 4 * wid + pb;
    if (oy >= Ho || ox >= Wo) continue;
    float* yp = y + (((int64_t)t * Ho + oy) * Wo + ox) * Cout;
#pragma unroll
    for (int cb = 0; cb < S2_NCB; ++cb) {
      const int co = co0 + cb * 16 + 4 * g4;
      if (co >= Cout) continue;
      const float4 bv = bias != nullptr ? *reinterpret_cast<const float4*>(bias + co) : make_float4(0.f, 0.f, 0.f, 0.f);
      *reinterpret_cast<float4*>(yp + co) = make_float4(acc[cb][pb][0] + bv.x, acc[cb][pb][1] + bv.y, acc[cb][pb][2] + bv.z, acc[cb][pb][3] + bv.w);
    }
  }
}

// One thread per pixel: reads the 3 channels of video[c, t, h, w] (w contiguous: coalesced across the wave) and writes them channels-last as fp32 (MODE 0),
// fp16 (1) or the hi/lo split [hi(3) | hi * 2^-12 (3) | lo(3)] (2) — the same conversion as x2v_vae_prep_split_f16 (vae.hip).  Pad channels are not written.
template <int MODE>
__global__ __launch_bounds__(256) void vae_video_prep_kernel(const float* __restrict__ v, int64_t cs, int64_t ts, int64_t vrs, int T, int H, int W, void* __restrict__ y,
                                                             int64_t yfs, int64_t yrs, int64_t yps) {
  const int64_t npix = (int64_t)T * H * W;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (int64_t)gridDim.x * blockDim.x) {
    const int xw = (int)(i % W);
    const int64_t r = i / W;
    const int xh = (int)(r % H), t = (int)(r / H);
    const int64_t src = (int64_t)t * ts + (int64_t)xh * vrs + xw, dst = (int64_t)t * yfs + (int64_t)xh * yrs + (int64_t)xw * yps;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float x = v[src + c * cs];
      if constexpr (MODE == 0) {
        reinterpret_cast<float*>(y)[dst + c] = x;
      } else if constexpr (MODE == 1) {
        reinterpret_cast<_Float16*>(y)[dst + c] = (_Float16)x;
      } else {
        const float o = fminf(fmaxf(x, -131008.f), 131008.f);
        const _Float16 hi = (_Float16)fminf(fmaxf(o, -65504.f), 65504.f);
        _Float16* yh = reinterpret_cast<_Float16*>(y) + dst;
        yh[c] = hi;
        yh[3 + c] = (_Float16)((float)hi * 0.000244140625f);
        yh[6 + c] = (_Float16)(o - (float)hi);
      }
    }
  }
}

}  // namespace x2v

using namespace x2v;

extern "C" __attribute__((visibility("default"))) int x2v_vae_conv_s2_f16(const void* xp, int64_t x_frame_stride, int64_t x_row_stride, int64_t x_px_stride, const void* w,
                                                                          int64_t w_row_stride, const float* bias, float* y, int T, int Hin, int Win, int Cin, int Cout, int flags,
                                                                          void* stream) {
  X2V_REQUIRE(xp && w && y, X2V_E_ARG, "vae_conv_s2_f16: null pointer");
  X2V_REQUIRE(flags == 0, X2V_E_ARG, "vae_conv_s2_f16: flags must be 0");
  X2V_REQUIRE(T > 0 && Hin >= 2 && Win >= 2 && Cin > 0 && Cout > 0, X2V_E_SHAPE, "vae_conv_s2_f16: bad shape (T >= 1, Hin, Win >= 2)");
  X2V_REQUIRE(Cin % 32 == 0, X2V_E_SHAPE, "vae_conv_s2_f16: Cin=%d must be a multiple of 32 (one 64-byte slab per K step)", Cin);
  X2V_REQUIRE(Cout % 4 == 0, X2V_E_SHAPE, "vae_conv_s2_f16: Cout=%d must be a multiple of 4", Cout);
  X2V_REQUIRE(x_px_stride % 8 == 0 && x_row_stride % 8 == 0 && x_frame_stride % 8 == 0 && w_row_stride % 8 == 0 && x_px_stride >= Cin &&
                  x_row_stride >= (int64_t)Win * x_px_stride && x_frame_stride >= (int64_t)Hin * x_row_stride && w_row_stride >= 9ll * Cin,
              X2V_E_ALIGN, "vae_conv_s2_f16: strides must be multiples of 8 halves and cover the extents");
  X2V_REQUIRE(aligned16(xp) && aligned16(w) && aligned16(y) && aligned16(bias), X2V_E_ALIGN, "vae_conv_s2_f16: pointers must be 16-byte aligned");
  const int Ho = Hin / 2, Wo = Win / 2;
  const int tiles_x = (Wo + S2_TW - 1) / S2_TW, tiles_y = (Ho + S2_TH - 1) / S2_TH, ncol = (Cout + 16 * S2_NCB - 1) / (16 * S2_NCB);
  const int64_t blocks = (int64_t)T * tiles_y * tiles_x * ncol;
  X2V_REQUIRE(blocks < (1ll << 31), X2V_E_SHAPE, "vae_conv_s2_f16: too many tiles");
  int rc = ensure_dynamic_lds((const void*)vae_conv_s2_kernel, S2_LDS, "vae conv s2 attr");
  if (rc != X2V_OK) return rc;
  hipLaunchKernelGGL(vae_conv_s2_kernel, dim3((unsigned)blocks), dim3(256), S2_LDS, (hipStream_t)stream, (const _Float16*)xp, x_frame_stride, x_row_stride, x_px_stride,
                     (const _Float16*)w, w_row_stride, bias, y, Hin, Win, Ho, Wo, Cin, Cout, tiles_x, tiles_y, ncol);
  X2V_LAUNCH_CHECK("vae_conv_s2_f16 launch");
  return X2V_OK;
}

extern "C" __attribute__((visibility("default"))) int x2v_vae_video_prep(const float* video, int64_t c_stride, int64_t t_stride, int64_t row_stride, int T, int H, int W,
                                                                         void* y, int64_t y_frame_stride, int64_t y_row_stride, int64_t y_px_stride, int mode, void* stream) {
  X2V_REQUIRE(video && y, X2V_E_ARG, "vae_video_prep: null pointer");
  X2V_REQUIRE(mode >= 0 && mode <= 2, X2V_E_ARG, "vae_video_prep: mode = 0 fp32 | 1 fp16 | 2 hi/lo split fp16");
  X2V_REQUIRE(T > 0 && H > 0 && W > 0, X2V_E_SHAPE, "vae_video_prep: bad shape");
  X2V_REQUIRE(y_px_stride >= (mode == 2 ? 9 : 3) && y_row_stride >= (int64_t)W * y_px_stride && y_frame_stride >= (int64_t)H * y_row_stride && row_stride >= W &&
                  t_stride >= (int64_t)H * row_stride && c_stride > 0,
              X2V_E_SHAPE, "vae_video_prep: strides must cover the extents (pixel stride >= the channels written)");
  const int64_t npix = (int64_t)T * H * W;
  const unsigned grid = (unsigned)std::min<int64_t>((npix + 255) / 256, 65536 * 4);
  hipStream_t st = (hipStream_t)stream;
  if (mode == 0)
    hipLaunchKernelGGL(vae_video_prep_kernel<0>, dim3(grid), dim3(256), 0, st, video, c_stride, t_stride, row_stride, T, H, W, y, y_frame_stride, y_row_stride, y_px_stride);
  else if (mode == 1)
    hipLaunchKernelGGL(vae_video_prep_kernel<1>, dim3(grid), dim3(256), 0, st, video, c_stride, t_stride, row_stride, T, H, W, y, y_frame_stride, y_row_stride, y_px_stride);
  else
    hipLaunchKernelGGL(vae_video_prep_kernel<2>, dim3(grid), dim3(256), 0, st, video, c_stride, t_stride, row_stride, T, H, W, y, y_frame_stride, y_row_stride, y_px_stride);
  X2V_LAUNCH_CHECK("vae_video_prep launch");
  return X2V_OK;
}
