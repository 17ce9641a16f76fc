// Per-frame cross-attention, head dim 128 (x2v.h, x2v_attn_frames_fwd_bf16): every query row attends the Kf = 32 .. 128 keys of its own frame and
// nothing else — the audio adapter's PerceiverAttentionCA, where each latent frame's h w tokens attend that frame's 128 audio tokens.
//
// A kernel designed around bytes: per launch the q rows come in and the o rows go out once (HBM), while a frame-head's K and V are 2 Kf 128 2 B
// <= 64 KiB, re-read by every query tile of the frame.  So:
//   work item   (frame, head, chunk of the frame's rows in this launch): a workgroup never straddles a frame.  A chunk is `tpc` consecutive 64-row
//               tiles; the launcher picks the chunks per frame so that the grid is about 8 rounds of the chip's 512 resident workgroups
//               (2 per CU by LDS), and never fewer tiles per chunk than that needs.
//   LDS         staged ONCE per work item: K as [Kf][128 + 8], V transposed as [128][Kf + 8] (the kernel transposes row-major V itself: there is
//               no V^T pre-pass in the ABI).  Kf = 128: 34 816 + 34 816 = 69 632 bytes, dynamic.  One barrier per work item, none in the tile loop.
//   queries     stream through registers: a wave owns 16 rows of the tile, a lane reads its row's four 16-byte k-step fragments straight from
//               global memory (4 lanes cover 64 contiguous bytes of a row per k-step; no LDS ring — q is read once and by one lane only).
//   scores      S^T = K . Q^T with v_mfma_f32_16x16x32_bf16 (enc_attn.h's convention): all Kf scores of a row sit in the 4 lanes of its
//               column before anything is exponentiated, Kf / 16 accumulators of 4.
//   PV          O^T = V^T . P^T, P as the B operand without lane movement.  The V^T row that A-row i of output tile c reads is
//               d = 32 (c / 2) + 8 (i / 4) + i % 4 + 4 (c % 2): tiles 2 j and 2 j + 1 then leave output columns 32 j + 8 g4 .. + 7 of a query
//               in ONE lane, and the row goes out as 16-byte segments (4 lanes: 64 contiguous bytes).
// Arithmetic: x2v.h, steps 1-6.  A row past the chunk's end reads the frame's last row of the launch and is never stored.
#include "enc_attn.h"

namespace x2v {

constexpr int AF_D = 128;        // head dim
constexpr int AF_KP = AF_D + 8;  // K row pitch in LDS (elements)
constexpr int AF_ROWS = 64;      // query rows per tile: 4 waves x 16
constexpr int AF_TARGET_WGS = 4096;  // workgroups a launch aims at: 8 rounds of 256 CUs x 2 resident (derived from the LDS budget, not measured)

constexpr int af_lds_bytes(int kf) { return (kf * AF_KP + AF_D * (kf + 8)) * 2; }

template <int NK, bool PRE>
__global__ __launch_bounds__(256) void attn_frames_kernel(const __bf16* __restrict__ q, int64_t ldq, const __bf16* __restrict__ k, int64_t ldk, const __bf16* __restrict__ v,
                                                          int64_t ldv, __bf16* __restrict__ o, int64_t ldo, int64_t Sq, int64_t row0, int64_t rpf, int nchunk, int tpc,
                                                          float scale_log2e) {
  constexpr int KF = 16 * NK, VP = KF + 8;
  extern __shared__ __attribute__((aligned(16))) unsigned char af_lds[];
  __bf16* Ks = reinterpret_cast<__bf16*>(af_lds);
  __bf16* Vt = Ks + KF * AF_KP;
  const EncLanes L = enc_lanes();
  const int head = blockIdx.y;
  const int64_t t = row0 / rpf + blockIdx.x / nchunk;  // the frame
  const int chunk = blockIdx.x % nchunk;
  // the frame's rows in this launch, as local rows [lo, hi)
  const int64_t lo = max(t * rpf, row0) - row0, hi = min((t + 1) * rpf, row0 + Sq) - row0;
  const int64_t tile0 = (int64_t)chunk * tpc, tile1 = min((hi - lo + AF_ROWS - 1) / AF_ROWS, tile0 + tpc);
  if (tile0 >= tile1) return;  // a partial frame has fewer chunks (the whole workgroup leaves, in front of the barrier)

  stage_k<__bf16, AF_D, KF, AF_KP>(Ks, k + t * KF * ldk + (int64_t)head * AF_D, ldk, 0, KF, L.tid);
  stage_vt<__bf16, AF_D, KF, VP>(Vt, v + t * KF * ldv + (int64_t)head * AF_D, ldv, 0, KF, L.tid);
  __syncthreads();

  const int drow = 8 * (L.c16 >> 2) + (L.c16 & 3);  // this lane's A-row of an output tile, as a V^T row inside the tile pair
  for (int64_t tile = tile0; tile < tile1; ++tile) {
    const int64_t wave_r = lo + tile * AF_ROWS + L.wid * 16;
    if (wave_r >= hi) break;  // a wave without rows (no barrier in this loop)
    const int64_t r = wave_r + L.c16;
    bf16x8_t qf[4];
    load_q<__bf16, 4>(q + min(r, hi - 1) * ldq + (int64_t)head * AF_D, L.g4, qf);
    if constexpr (!PRE) {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
#pragma unroll
        for (int e = 0; e < 8; ++e) qf[ks][e] = (__bf16)((float)qf[ks][e] * scale_log2e);
    }
    f32x4_t s[NK];
    float m = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < NK; ++kt) {
      s[kt] = score_tile<__bf16, 4, AF_KP>(Ks, kt, L, qf);
#pragma unroll
      for (int e = 0; e < 4; ++e) m = fmaxf(m, s[kt][e]);
    }
    m = quad_max(m);
    float l = 0.f;
#pragma unroll
    for (int kt = 0; kt < NK; ++kt)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        s[kt][e] = __builtin_amdgcn_exp2f(s[kt][e] - m);
        l += s[kt][e];
      }
    l = quad_sum(l);

    f32x4_t acc[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[c] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < NK / 2; ++kk) {
      bf16x8_t pb;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        pb[e] = (__bf16)s[2 * kk][e];
        pb[4 + e] = (__bf16)s[2 * kk + 1][e];
      }
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const __bf16* vr = Vt + (32 * (c >> 1) + 4 * (c & 1) + drow) * VP + 32 * kk + 4 * L.g4;
        const bf16x4_t v_lo = *reinterpret_cast<const bf16x4_t*>(vr), v_hi = *reinterpret_cast<const bf16x4_t*>(vr + 16);
        const bf16x8_t vf = {v_lo[0], v_lo[1], v_lo[2], v_lo[3], v_hi[0], v_hi[1], v_hi[2], v_hi[3]};
        acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pb, acc[c], 0, 0, 0);
      }
    }
    if (r < hi) {
      const float inv = 1.0f / l;
      __bf16* op = o + r * ldo + (int64_t)head * AF_D + 8 * L.g4;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        bf16x8_t w;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          w[e] = (__bf16)(acc[2 * j][e] * inv);
          w[4 + e] = (__bf16)(acc[2 * j + 1][e] * inv);
        }
        *reinterpret_cast<bf16x8_t*>(op + 32 * j) = w;
      }
    }
  }
}

template <int NK>
static int launch_attn_frames(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* o, int64_t ldo, int64_t Sq, int64_t row0,
                              int64_t rpf, int H, float scale, bool prescaled, hipStream_t st) {
  const int64_t frames = (row0 + Sq - 1) / rpf - row0 / rpf + 1;
  const int64_t max_tiles = (std::min(rpf, Sq) + AF_ROWS - 1) / AF_ROWS;  // of one frame's rows in this launch
  X2V_REQUIRE(max_tiles < (1ll << 31), X2V_E_SHAPE, "attn_frames: %lld query tiles in one frame", (long long)max_tiles);
  const int64_t want = (AF_TARGET_WGS + frames * H - 1) / (frames * H);
  const int tpc = (int)((max_tiles + std::min(want, max_tiles) - 1) / std::min(want, max_tiles));
  const int nchunk = (int)((max_tiles + tpc - 1) / tpc);
  X2V_REQUIRE(frames * nchunk < (1ll << 31), X2V_E_SHAPE, "attn_frames: %lld frames x %d chunks in one launch", (long long)frames, nchunk);
  const dim3 grid((unsigned)(frames * nchunk), (unsigned)H);
  const float sl2 = scale * 1.4426950408889634f;
  const int lds = af_lds_bytes(16 * NK);
#define AF_LAUNCH(PRE)                                                                                                                                        \
  do {                                                                                                                                                        \
    int rc = ensure_dynamic_lds((const void*)attn_frames_kernel<NK, PRE>, lds, "attn_frames attr");                                                           \
    if (rc != X2V_OK) return rc;                                                                                                                              \
    hipLaunchKernelGGL((attn_frames_kernel<NK, PRE>), grid, dim3(256), lds, st, (const __bf16*)q, ldq, (const __bf16*)k, ldk, (const __bf16*)v, ldv, (__bf16*)o, ldo, Sq, \
                       row0, rpf, nchunk, tpc, sl2);                                                                                                          \
  } while (0)
  if (prescaled) AF_LAUNCH(true);
  else AF_LAUNCH(false);
#undef AF_LAUNCH
  X2V_LAUNCH_CHECK("attn_frames launch");
  return X2V_OK;
}

}  // namespace x2v
using namespace x2v;

extern "C" __attribute__((visibility("default"))) int x2v_attn_frames_fwd_bf16(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* o,
                                                                               int64_t ldo, int64_t Sq, int64_t row0, int64_t rows_per_frame, int n_frames, int keys_per_frame,
                                                                               int H, int head_dim, float scale, int flags, void* stream) {
  const int Kf = keys_per_frame;
  X2V_REQUIRE(head_dim == AF_D, X2V_E_SHAPE, "attn_frames: head_dim=%d (only 128 is built)", head_dim);
  X2V_REQUIRE(Kf % 32 == 0 && Kf >= 32 && Kf <= 128, X2V_E_SHAPE, "attn_frames: keys_per_frame=%d must be 32, 64, 96 or 128", Kf);
  X2V_REQUIRE(rows_per_frame >= 1 && row0 >= 0 && Sq >= 0 && row0 < (1ll << 62) && Sq < (1ll << 62) && n_frames >= 1 && H >= 1 && H <= 65535, X2V_E_SHAPE,
              "attn_frames: bad shape Sq=%lld row0=%lld rows_per_frame=%lld n_frames=%d H=%d", (long long)Sq, (long long)row0, (long long)rows_per_frame, n_frames, H);
  if (Sq == 0) return X2V_OK;  // no query rows: nothing to write (empty shard)
  X2V_REQUIRE((row0 + Sq - 1) / rows_per_frame < n_frames, X2V_E_SHAPE, "attn_frames: rows [%lld, %lld) of %lld per frame reach beyond the %d frames of k / v", (long long)row0,
              (long long)(row0 + Sq), (long long)rows_per_frame, n_frames);
  X2V_REQUIRE(q && k && v && o, X2V_E_ARG, "attn_frames: null pointer");
  X2V_REQUIRE(ldq % 8 == 0 && ldk % 8 == 0 && ldv % 8 == 0 && ldo % 8 == 0 && aligned16(q) && aligned16(k) && aligned16(v) && aligned16(o), X2V_E_ALIGN,
              "attn_frames: rows must be 16-byte aligned (q, k, v, o, and every ld a multiple of 8)");
  X2V_REQUIRE(ldq >= (int64_t)H * AF_D && ldk >= (int64_t)H * AF_D && ldv >= (int64_t)H * AF_D && ldo >= (int64_t)H * AF_D, X2V_E_SHAPE,
              "attn_frames: token stride smaller than H*128");
  X2V_REQUIRE((flags & ~X2V_ATTN_VT_PRESCALED) == 0, X2V_E_ARG, "attn_frames: flags = X2V_ATTN_VT_PRESCALED");
  if (scale <= 0.f) scale = 0.08838834764831845f;
  const bool pre = (flags & X2V_ATTN_VT_PRESCALED) != 0;
  hipStream_t st = (hipStream_t)stream;
  switch (Kf) {
    case 32: return launch_attn_frames<2>(q, ldq, k, ldk, v, ldv, o, ldo, Sq, row0, rows_per_frame, H, scale, pre, st);
    case 64: return launch_attn_frames<4>(q, ldq, k, ldk, v, ldv, o, ldo, Sq, row0, rows_per_frame, H, scale, pre, st);
    case 96: return launch_attn_frames<6>(q, ldq, k, ldk, v, ldv, o, ldo, Sq, row0, rows_per_frame, H, scale, pre, st);
    default: return launch_attn_frames<8>(q, ldq, k, ldk, v, ldv, o, ldo, Sq, row0, rows_per_frame, H, scale, pre, st);
  }
}
