// TAEHV (the Wan runner's `tiny_vae` decoder): channels-last bf16 implicit-GEMM conv2d family + the Clamp pixel kernel.
// reference: models/video_encoders/hf/tae.py — conv :15-16, Clamp :19-21, MemBlock :24-32, TGrow :46-55, the decoder :193-217;
//            models/video_encoders/hf/wan/vae_tiny.py:21-27 (the x 2 - 1 behind the decoder).
//
// One kernel body, templated on the kernel size KS (3: zero "same" padding, 1: TGrow) and on NCB = 16-cout blocks per workgroup (4, or 1 for Cout <= 16: the 3-channel head).
// Activations [T][H][W][C] bf16, weights [Cout][KS][KS][Ctot] bf16 (Ctot = Cin, or 2 Cin in the two-source form), fp32 accumulation on v_mfma_f32_16x16x32_bf16, bf16 out.
//   * workgroup = 4 waves = a 16 x 16 pixel tile of one output frame x 16 NCB couts; wave w owns image rows 4w .. 4w + 3 = 4 pixel blocks of 16 x NCB cout blocks:
//     D = W . X (A = 16 weight rows, B = 16 pixels), so a lane ends with 4 consecutive couts of one pixel (8-byte channels-last stores).
//   * K loop over 32-channel chunks.  Per chunk the (16 + KS - 1)^2 halo ([rows][64 B]) and the KS^2 x 16 NCB weight rows ([rows][64 B]) are staged in LDS once and serve
//     every tap: 16 NCB MFMAs per tap and wave against 18 + 9 NCB fragment reads per chunk (KS = 3).  The next chunk's global loads are issued into registers in front of
//     the chunk's MFMAs.  LDS chunk index XOR 2 ((row >> 2) & 1): ds_read_b128 conflict-free for every tap shift (the rule vae16g.hip found).
//   * the halo loader computes every source address itself, which is where the fusions sit:
//       zero padding        halo pixels outside the OUTPUT image read as zero (no bordered buffers);
//       upsample-read       nn.Upsample(2) commutes with TGrow's 1x1 convolution bit for bit, so TGrow runs at the low resolution and the 3x3 behind it reads its operand
//                           at (h >> 1, w >> 1): the upsampled tensor is never written (a quarter of the bytes of writing it once from the 1x1's epilogue and reading it back);
//       two sources         MemBlock's conv(cat([x_t, x_{t-1}], 1)): chunks 0 .. Cin/32 - 1 come from frame t, the next Cin/32 from frame t - 1 of the same buffer; frame -1 is
//                           `mem` (the carried frame of a chunked decode) or zero.  No concatenated tensor exists;
//       channel tails       8-channel pieces at or beyond Cin read as zero in both operands (Cin = 16: the first convolution), weight rows at or beyond Cout read as zero.
//   * epilogues in the reference's rounding order, every step one round-to-nearest-even to bf16: v = RN(acc + bias); resid: v = RN(v + resid); head: v = RN(2 v - 1);
//     ReLU last.  Time-split (TGrow): cout block j of input frame t -> output frame tsplit t + j.  y strides are explicit, so the head stores channel-first and drops the
//     first `trim` frames by addressing (those frames are not computed).
// Reduction order of an output value: (source, chunk, in-MFMA channel order, dh, dw) — independent of the tile, the frame count and the frame index, so a chunked decode is
// bit-identical to the whole clip.
//
// Bound: the 256- and 128-channel stages are MFMA-bound; the 64-channel stages and the head lean on HBM (DESIGN §4.4.1 has the per-layer table).
// Values are written with vector stores / plain C++ only.
#include "x2v_common.h"

namespace x2v {

constexpr int TQ_T = 16;  // tile edge (pixels)
constexpr int TQF_RELU = 1, TQF_UPS = 2, TQF_TWO = 4, TQF_HEAD = 8;

struct TConvArgs {
  const __bf16 *x, *mem, *w, *bias, *resid;
  __bf16* y;
  int64_t xfs, xrs, xps, yfs, yrs, yps, ycs;
  int T, H, W, Cin, Cout, flags, tsplit, trim, kchunks, tiles_x, tiles_y, ncol, vec;
};

__device__ __forceinline__ int tq_swz(int row, int c) { return row * 64 + ((c ^ (((row >> 2) & 1) << 1)) << 4); }

template <int KS, int NCB>
__global__ __launch_bounds__(256) void taehv_conv_kernel(const TConvArgs a) {
#if defined(__HIP_DEVICE_COMPILE__)
  constexpr int PAD = KS / 2, HC = TQ_T + KS - 1, HROWS = HC * HC, WROWS = KS * KS * NCB * 16;
  constexpr int HP = (HROWS * 4 + 255) / 256, WP = (WROWS * 4 + 255) / 256, XR = 4 + KS - 1;
  __shared__ __attribute__((aligned(16))) char s_h[HROWS * 64];
  __shared__ __attribute__((aligned(16))) char s_w[WROWS * 64];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, c16 = lane & 15, g4 = lane >> 4;
  unsigned b = blockIdx.x;
  const int co0 = (int)(b % (unsigned)a.ncol) * (NCB * 16);
  b /= (unsigned)a.ncol;
  const int x0 = (int)(b % (unsigned)a.tiles_x) * TQ_T;
  b /= (unsigned)a.tiles_x;
  const int y0 = (int)(b % (unsigned)a.tiles_y) * TQ_T;
  const int fo = (int)(b / (unsigned)a.tiles_y);  // output frame (before the time-split)
  const int frame = fo + a.trim;                  // input frame
  const int ups = (a.flags & TQF_UPS) ? 1 : 0, nsrc = (a.flags & TQF_TWO) ? 2 : 1;
  const int Ctot = nsrc * a.Cin, pc = tid & 3;  // pc: this thread's 8-channel piece of a 32-channel chunk (256 % 4 == 0: the same for all its pieces)
  const int64_t wrs = (int64_t)KS * KS * Ctot;

  // ---- tile-invariant piece addresses
  int64_t h_off[HP];
  int h_lds[HP];
#pragma unroll
  for (int i = 0; i < HP; ++i) {
    const int p = tid + i * 256, r = p >> 2;
    const int hy = r / HC, hx = r - hy * HC, oy = y0 + hy - PAD, ox = x0 + hx - PAD;
    const bool in = p < HROWS * 4 && oy >= 0 && oy < a.H && ox >= 0 && ox < a.W;
    h_off[i] = in ? (int64_t)(oy >> ups) * a.xrs + (int64_t)(ox >> ups) * a.xps + pc * 8 : -1;
    h_lds[i] = p < HROWS * 4 ? tq_swz(r, pc) : -1;
  }
  int64_t w_off[WP];
  int w_lds[WP];
#pragma unroll
  for (int i = 0; i < WP; ++i) {
    const int p = tid + i * 256, row = p >> 2;
    const int tap = row / (NCB * 16), co = co0 + row - tap * (NCB * 16);
    w_off[i] = (p < WROWS * 4 && co < a.Cout) ? (int64_t)co * wrs + (int64_t)tap * Ctot + pc * 8 : -1;
    w_lds[i] = p < WROWS * 4 ? tq_swz(row, pc) : -1;
  }
  const __bf16* src[2];
  src[0] = a.x + (int64_t)frame * a.xfs;
  src[1] = frame > 0 ? a.x + (int64_t)(frame - 1) * a.xfs : a.mem;  // may be null: zero memory

  uint4 hreg[HP], wreg[WP];
  auto fetch = [&](int q) {
    const int s = q >= a.kchunks ? 1 : 0, kc = q - s * a.kchunks;
    const bool chan_ok = kc * 32 + pc * 8 < a.Cin;
    const __bf16* xs = src[s];
#pragma unroll
    for (int i = 0; i < HP; ++i)
      hreg[i] = (h_off[i] >= 0 && chan_ok && xs != nullptr) ? *reinterpret_cast<const uint4*>(xs + h_off[i] + kc * 32) : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
    for (int i = 0; i < WP; ++i)
      wreg[i] = (w_off[i] >= 0 && chan_ok) ? *reinterpret_cast<const uint4*>(a.w + w_off[i] + s * a.Cin + kc * 32) : make_uint4(0u, 0u, 0u, 0u);
  };

  f32x4_t acc[NCB][4];
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
    for (int pb = 0; pb < 4; ++pb) acc[cb][pb] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  const int nq = nsrc * a.kchunks;
  fetch(0);
  for (int q = 0; q < nq; ++q) {
    __syncthreads();  // the previous chunk's fragment reads are done
#pragma unroll
    for (int i = 0; i < HP; ++i)
      if (h_lds[i] >= 0) *reinterpret_cast<uint4*>(s_h + h_lds[i]) = hreg[i];
#pragma unroll
    for (int i = 0; i < WP; ++i)
      if (w_lds[i] >= 0) *reinterpret_cast<uint4*>(s_w + w_lds[i]) = wreg[i];
    __syncthreads();
    if (q + 1 < nq) fetch(q + 1);
    bf16x8_t xf[XR][KS];
#pragma unroll
    for (int rr = 0; rr < XR; ++rr)
#pragma unroll
      for (int dw = 0; dw < KS; ++dw) xf[rr][dw] = *reinterpret_cast<const bf16x8_t*>(s_h + tq_swz((4 * wid + rr) * HC + dw + c16, g4));
#pragma unroll
    for (int dh = 0; dh < KS; ++dh)
#pragma unroll
      for (int dw = 0; dw < KS; ++dw)
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) {
          const bf16x8_t wf = *reinterpret_cast<const bf16x8_t*>(s_w + tq_swz(((dh * KS + dw) * NCB + cb) * 16 + c16, g4));
#pragma unroll
          for (int pb = 0; pb < 4; ++pb) acc[cb][pb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, xf[pb + dh][dw], acc[cb][pb], 0, 0, 0);
        }
  }

  // ---- epilogue: acc[cb][pb][e] = pixel (y0 + 4 wid + pb, x0 + c16), cout co0 + 16 cb + 4 g4 + e
  const int Cb = a.Cout / a.tsplit;  // couts of one time-split block
  const int px = x0 + c16;
#pragma unroll
  for (int pb = 0; pb < 4; ++pb) {
    const int py = y0 + 4 * wid + pb;
    if (py >= a.H || px >= a.W) continue;
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
      const int co = co0 + cb * 16 + 4 * g4;
      if (co >= a.Cout) continue;
      const int j = co / Cb, cc = co - j * Cb;
      const int64_t o = (int64_t)(fo * a.tsplit + j) * a.yfs + (int64_t)py * a.yrs + (int64_t)px * a.yps + (int64_t)cc * a.ycs;
      float v[4];
      float r[4] = {0.f, 0.f, 0.f, 0.f};
      if (a.resid != nullptr) {
        if (a.vec) {
          const uint2 rv = *reinterpret_cast<const uint2*>(a.resid + o);
          r[0] = bf_lo(rv.x), r[1] = bf_hi(rv.x), r[2] = bf_lo(rv.y), r[3] = bf_hi(rv.y);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (co + e < a.Cout) r[e] = (float)a.resid[o + (int64_t)e * a.ycs];
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float t = acc[cb][pb][e];
        if (a.bias != nullptr && co + e < a.Cout) t += (float)a.bias[co + e];
        t = rbf(t);
        if (a.resid != nullptr) t = rbf(t + r[e]);
        if (a.flags & TQF_HEAD) t = rbf(t * 2.0f - 1.0f);
        if (a.flags & TQF_RELU) t = fmaxf(t, 0.f);
        v[e] = t;
      }
      if (a.vec) {
        *reinterpret_cast<uint2*>(a.y + o) = make_uint2(pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]));
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (co + e < a.Cout) a.y[o + (int64_t)e * a.ycs] = (__bf16)v[e];
      }
    }
  }
#endif
}

// Clamp (tae.py:19-21) on the caller's channel-first latent, written as the first convolution's channels-last operand:
// y[t][h][w][c] = RN(RN(tanh(RN(RN(z) / 3))) * 3), z[c * c_stride + t * t_stride + h * W + w] fp32 (rounded to bf16 first, the reference's .to(bf16)) or bf16.
template <typename TI>
__global__ __launch_bounds__(256) void taehv_clamp_kernel(const TI* __restrict__ z, int64_t c_stride, int64_t t_stride, __bf16* __restrict__ y, int T, int HW, int C) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;  // pixel index over [T][HW]
  if (i >= (int64_t)T * HW) return;
  const int t = (int)(i / HW);
  const int64_t zo = (int64_t)t * t_stride + (i - (int64_t)t * HW);
  for (int c0 = 0; c0 < C; c0 += 8) {
    float f[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float v = rbf((float)z[zo + (int64_t)(c0 + e) * c_stride]);
      f[e] = rbf(rbf(tanhf(rbf(v / 3.0f))) * 3.0f);
    }
    *reinterpret_cast<uint4*>(y + i * C + c0) = pack8(f);
  }
}

template <int KS, int NCB>
static int launch_tconv(const TConvArgs& a, hipStream_t st) {
  const int64_t blocks = (int64_t)(a.T - a.trim) * a.tiles_y * a.tiles_x * a.ncol;
  X2V_REQUIRE(blocks < (1ll << 31), X2V_E_SHAPE, "x2v_conv2d_bf16: too many tiles");
  hipLaunchKernelGGL((taehv_conv_kernel<KS, NCB>), dim3((unsigned)blocks), dim3(256), 0, st, a);
  X2V_LAUNCH_CHECK("x2v_conv2d_bf16 launch");
  return X2V_OK;
}

}  // namespace x2v

using namespace x2v;

extern "C" __attribute__((visibility("default"))) int x2v_conv2d_bf16(const void* x, const void* mem, int64_t x_frame_stride, int64_t x_row_stride, int64_t x_px_stride, const void* w,
                                                                      const void* bias, const void* resid, void* y, int64_t y_frame_stride, int64_t y_row_stride,
                                                                      int64_t y_px_stride, int64_t y_ch_stride, int T, int H, int W, int Cin, int Cout, int ksize, int flags,
                                                                      int tsplit, int frame_trim, void* stream) {
  X2V_REQUIRE(x != nullptr && w != nullptr && y != nullptr, X2V_E_ARG, "x2v_conv2d_bf16: null operand (x %p, w %p, y %p)", x, w, y);
  X2V_REQUIRE(ksize == 1 || ksize == 3, X2V_E_SHAPE, "x2v_conv2d_bf16: kernel size %d (1 and 3 are built)", ksize);
  X2V_REQUIRE((flags & ~(X2V_C2D_RELU | X2V_C2D_UPSAMPLE_READ | X2V_C2D_TWO_SOURCE | X2V_C2D_HEAD)) == 0, X2V_E_ARG, "x2v_conv2d_bf16: unknown flag bits in %d", flags);
  X2V_REQUIRE(mem == nullptr || (flags & X2V_C2D_TWO_SOURCE), X2V_E_ARG, "x2v_conv2d_bf16: mem goes with X2V_C2D_TWO_SOURCE");
  X2V_REQUIRE(T >= 0 && H >= 1 && W >= 1 && Cin >= 8 && Cout >= 1, X2V_E_SHAPE, "x2v_conv2d_bf16: T=%d H=%d W=%d Cin=%d Cout=%d", T, H, W, Cin, Cout);
  X2V_REQUIRE(Cin % 8 == 0, X2V_E_SHAPE, "x2v_conv2d_bf16: Cin=%d is not a multiple of 8", Cin);
  X2V_REQUIRE(!(flags & X2V_C2D_TWO_SOURCE) || Cin % 32 == 0, X2V_E_SHAPE, "x2v_conv2d_bf16: the two-source form needs Cin %% 32 == 0 (Cin=%d)", Cin);
  X2V_REQUIRE(tsplit >= 1 && Cout % tsplit == 0, X2V_E_SHAPE, "x2v_conv2d_bf16: tsplit=%d does not divide Cout=%d", tsplit, Cout);
  X2V_REQUIRE(tsplit == 1 || (Cout / tsplit) % 4 == 0, X2V_E_SHAPE, "x2v_conv2d_bf16: time-split blocks of %d couts (a multiple of 4 is needed)", Cout / tsplit);
  X2V_REQUIRE(tsplit == 1 || resid == nullptr, X2V_E_ARG, "x2v_conv2d_bf16: no residual with the time-split");
  X2V_REQUIRE(frame_trim >= 0 && frame_trim <= T, X2V_E_SHAPE, "x2v_conv2d_bf16: frame_trim=%d outside 0..T=%d", frame_trim, T);
  X2V_REQUIRE(x_frame_stride % 8 == 0 && x_row_stride % 8 == 0 && x_px_stride % 8 == 0 && x_px_stride >= Cin, X2V_E_ALIGN,
              "x2v_conv2d_bf16: x strides (%lld, %lld, %lld) must be multiples of 8 elements, pixel stride >= Cin", (long long)x_frame_stride, (long long)x_row_stride,
              (long long)x_px_stride);
  X2V_REQUIRE(aligned16(x) && aligned16(w) && aligned16(mem), X2V_E_ALIGN, "x2v_conv2d_bf16: x, mem and w must be 16-byte aligned");
  X2V_REQUIRE(y_ch_stride >= 1, X2V_E_SHAPE, "x2v_conv2d_bf16: y_ch_stride=%lld", (long long)y_ch_stride);
  if (T - frame_trim == 0) return X2V_OK;
  TConvArgs a;
  a.x = (const __bf16*)x, a.mem = (const __bf16*)mem, a.w = (const __bf16*)w, a.bias = (const __bf16*)bias, a.resid = (const __bf16*)resid, a.y = (__bf16*)y;
  a.xfs = x_frame_stride, a.xrs = x_row_stride, a.xps = x_px_stride, a.yfs = y_frame_stride, a.yrs = y_row_stride, a.yps = y_px_stride, a.ycs = y_ch_stride;
  a.T = T, a.H = H, a.W = W, a.Cin = Cin, a.Cout = Cout, a.tsplit = tsplit, a.trim = frame_trim;
  a.flags = ((flags & X2V_C2D_RELU) ? TQF_RELU : 0) | ((flags & X2V_C2D_UPSAMPLE_READ) ? TQF_UPS : 0) | ((flags & X2V_C2D_TWO_SOURCE) ? TQF_TWO : 0) |
            ((flags & X2V_C2D_HEAD) ? TQF_HEAD : 0);
  a.kchunks = (Cin + 31) / 32;
  a.tiles_x = (W + TQ_T - 1) / TQ_T, a.tiles_y = (H + TQ_T - 1) / TQ_T;
  const int ncb = Cout > 16 ? 4 : 1;
  a.ncol = (Cout + ncb * 16 - 1) / (ncb * 16);
  // 8-byte stores of a lane's 4 couts: channels-last, whole groups of 4, every address a multiple of 4 elements
  a.vec = y_ch_stride == 1 && (Cout / tsplit) % 4 == 0 && y_frame_stride % 4 == 0 && y_row_stride % 4 == 0 && y_px_stride % 4 == 0 && (reinterpret_cast<uintptr_t>(y) & 7u) == 0 &&
          (resid == nullptr || (reinterpret_cast<uintptr_t>(resid) & 7u) == 0);
  hipStream_t st = (hipStream_t)stream;
  if (ksize == 3) return ncb == 4 ? launch_tconv<3, 4>(a, st) : launch_tconv<3, 1>(a, st);
  return ncb == 4 ? launch_tconv<1, 4>(a, st) : launch_tconv<1, 1>(a, st);
}

extern "C" __attribute__((visibility("default"))) int x2v_taehv_clamp_bf16(const void* z, int z_is_f32, int64_t c_stride, int64_t t_stride, void* y, int T, int H, int W, int C,
                                                                           void* stream) {
  X2V_REQUIRE(z != nullptr && y != nullptr, X2V_E_ARG, "x2v_taehv_clamp_bf16: null operand (z %p, y %p)", z, y);
  X2V_REQUIRE(z_is_f32 == 0 || z_is_f32 == 1, X2V_E_ARG, "x2v_taehv_clamp_bf16: z_is_f32=%d", z_is_f32);
  X2V_REQUIRE(T >= 0 && H >= 1 && W >= 1 && C >= 8 && C % 8 == 0, X2V_E_SHAPE, "x2v_taehv_clamp_bf16: T=%d H=%d W=%d C=%d (C a multiple of 8)", T, H, W, C);
  X2V_REQUIRE((int64_t)H * W < (1ll << 31), X2V_E_SHAPE, "x2v_taehv_clamp_bf16: frame of %lld pixels", (long long)H * W);
  X2V_REQUIRE(aligned16(y), X2V_E_ALIGN, "x2v_taehv_clamp_bf16: y must be 16-byte aligned");
  const int64_t n = (int64_t)T * H * W;
  if (n == 0) return X2V_OK;
  const int64_t blocks = (n + 255) / 256;
  X2V_REQUIRE(blocks < (1ll << 31), X2V_E_SHAPE, "x2v_taehv_clamp_bf16: too many pixels");
  hipStream_t st = (hipStream_t)stream;
  if (z_is_f32) hipLaunchKernelGGL(taehv_clamp_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, st, (const float*)z, c_stride, t_stride, (__bf16*)y, T, H * W, C);
  else hipLaunchKernelGGL(taehv_clamp_kernel<__bf16>, dim3((unsigned)blocks), dim3(256), 0, st, (const __bf16*)z, c_stride, t_stride, (__bf16*)y, T, H * W, C);
  X2V_LAUNCH_CHECK("x2v_taehv_clamp_bf16 launch");
  return X2V_OK;
}
