// fp8 block-128 linear layer (the reference's DeepGEMM numeric format, mm_weight.py:203-256 and :418-494): e4m3 weights with one fp32 scale per
// 128 x 128 block, e4m3 activations with one fp32 scale per token and 128 K elements.
//
//   x2v_quant_fp8_group128   x bf16 [M, K] -> codes e4m3 [M, K] + scales fp32, k-group-major (sx[g * lds + m])
//   x2v_gemm_fp8_block128    y[m, n] = epi( sum_g (sx[g, m] * sw[n / 128, g]) * P_g[m, n] + bias[n] ) -> bf16,  P_g = sum_{k in group g} xq[m, k] wq[n, k]
//
// Why a kernel of its own: the scale of a product changes every 128 k, so it can neither wait for the epilogue (gemm256.hip's per-channel form) nor ride
// in the instruction (the MX forms: powers of two).  One v_mfma_scale_f32_16x16x128_f8f6f4 with unit scales and a ZERO C operand is exactly one scale
// group of a 16 x 16 output fragment: the partial product P_g needs no zeroing and no running accumulator, lives for one instruction's latency, and is
// folded into the main accumulator by 4 v_fma_f32 with s = sx * sw.  The folds of one instruction issue under the following ones.
//
// GEMM structure (bound: MFMA; 2 M N K FLOP per launch, plus M N K / 32 fp32 FMAs = a quarter of a VALU slot per matrix cycle):
//   * a 256-thread workgroup owns a 128 (m) x 256 (n) output tile; wave (wr, wc) of the 2 x 2 grid owns 64 rows x 128 columns = 4 x 8 fragments of
//     16 x 16, 128 accumulator registers.  Its 128 columns are one block row of sw (tiles start at multiples of 256), so sw[n / 128, g] is ONE scalar
//     per wave and K group: a scalar load, issued one group ahead.  One wave per SIMD: main accumulators, 4 partials in flight, 4 x and 1-2 W
//     fragments stay far inside the 512 registers a single wave has.
//   * the W fragment is the instruction's first operand, so a lane of the 16 x 16 result holds ONE row m (lane & 15) and 4 consecutive columns:
//     s = sx[g, m] * sw is one register per m-fragment and group (4 multiplies per wave-lane and group), and the epilogue packs 4 columns per lane.
//   * a K group (128 bytes of every operand row) is one stage: x 128 rows (16 KiB) | W 256 rows (32 KiB), staged by LDS-DMA (buffer_load .. lds,
//     16 bytes per lane) in the image of the other fp8 kernels: 16-byte chunk c of row r at chunk c ^ ((r >> 1) & 7), the exclusive-or applied on the
//     per-lane SOURCE offset (the DMA destination is lane-linear) and on the ds_read_b128 address.  The 128 sx values of the group ride along as one
//     4-byte-per-lane DMA piece into a table beside the ring.  A ring of 3 stages, 13 DMA pieces per wave and group, ONE barrier per group:
//         wait (own pieces of group t landed: vmcnt leaves group t+1's 13 in flight) | barrier | issue group t+2 into the stage group t-1 left | compute t
//     RAW: every wave waits for its own pieces of group t in front of the barrier.  WAR: the stage of group t+2 is that of group t-1, whose last
//     ds_read every wave has completed (lgkmcnt(0)) in front of the same barrier.
//   * a lane's two 16-byte chunks of a fragment row are chunks g and 4 + g (g = lane >> 4): with unit scales any k order shared by both operands
//     gives the same sum of exact products.
//   * M / N tails: the descriptors start at the tile's first row and cover only its valid rows, so rows past M (or N) read as zero; the sx piece
//     sends lanes past the last valid row out of range; a wave whose 128 columns lie past the last block row of sw reads the last one (nothing of
//     it is stored).  Stores are masked.
//   * epilogue through LDS ([128][528 B]) so that global stores are 16 bytes per lane; bias / activation by the shared epi_bias_act4.
#include "gemm256_pipe.h"

namespace x2v {

constexpr int B_M = 128, B_N = 256;
constexpr int B_X_BYTES = B_M * 128, B_W_BYTES = B_N * 128;
constexpr int B_STAGE_BYTES = B_X_BYTES + B_W_BYTES;  // 49152
constexpr int B_STAGES = 3;
constexpr int B_SX_OFF = B_STAGES * B_STAGE_BYTES;    // the sx tables: one 1 KiB slot per stage (4 waves x 64 lanes x 4 B; rows 0..127 are used)
constexpr int B_SX_BYTES = 1024;
constexpr int B_LDS_BYTES = B_SX_OFF + B_STAGES * B_SX_BYTES;  // 150528
constexpr int B_EPI_LD = 528;                         // bytes per epilogue row (256 bf16 + 16 pad)
constexpr int B_PIECES = 4 + 8 + 1;                   // DMA pieces per wave and K group: x, W, sx
static_assert(B_M * B_EPI_LD <= B_SX_OFF && B_LDS_BYTES <= 160 * 1024, "LDS plan");

typedef __attribute__((address_space(3))) void* b_lds_ptr_t;

template <int EPI>
__global__ __launch_bounds__(256) void gemm_b128_kernel(const char* __restrict__ A, int64_t lda, const char* __restrict__ W, int64_t ldw,
                                                        const float* __restrict__ sx, int64_t ldsx, const float* __restrict__ sw, int64_t ldsw, int nbw,
                                                        const unsigned short* __restrict__ bias, unsigned short* __restrict__ Y, int64_t ldy, int64_t M, int N,
                                                        int nk, const unsigned short* __restrict__ resid, int64_t ldr,
                                                        const unsigned short* __restrict__ gate, int ntm, int ntn) {
#if defined(__HIP_DEVICE_COMPILE__)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wid >> 1, wc = wid & 1;
  const int r16 = lane & 15, g16 = lane >> 4;

  // ---- tile coordinates: XCD chunking + groups of 8 m-tiles x all n-tiles (neighbouring workgroups share W in L2)
  const unsigned nblk = (unsigned)ntm * (unsigned)ntn;
  const unsigned v = xcd_remap(blockIdx.x, nblk);
  const unsigned GM = 8u, per_group = GM * (unsigned)ntn;
  const unsigned group = v / per_group, in_g = v % per_group;
  const unsigned first_m = group * GM;
  const unsigned gsz = min((unsigned)ntm - first_m, GM);
  const int tm = (int)(first_m + in_g % gsz), tn = (int)(in_g / gsz);
  const int64_t m0 = (int64_t)tm * B_M;
  const int n0 = tn * B_N;

  // ---- buffer descriptors over this tile's valid rows (wave-uniform)
  const int rows_a = (int)min((int64_t)B_M, M - m0), rows_w = min(B_N, N - n0);
  const unsigned row_bytes = (unsigned)nk * 128u;
  const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc((void*)(A + m0 * lda), 0, (unsigned)((rows_a - 1) * lda) + row_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)(W + (int64_t)n0 * ldw), 0, (unsigned)((rows_w - 1) * ldw) + row_bytes, 0x00020000);
  // sx[g * ldsx + m0 + row], row < rows_a: the range ends behind the last group's valid rows
  const __amdgpu_buffer_rsrc_t rs =
      __builtin_amdgcn_make_buffer_rsrc((void*)(sx + m0), 0, (unsigned)(((int64_t)(nk - 1) * ldsx + rows_a) * 4), 0x00020000);

  // ---- per-lane DMA source offsets: a piece = 8 rows x 8 chunks; wave `wid` stages x rows [wid*32, +32) and W rows [wid*64, +64)
  unsigned a_voff[4], w_voff[8];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = (wid * 4 + i) * 8 + (lane >> 3);
    a_voff[i] = (unsigned)(r * lda) + (unsigned)((((lane & 7) ^ ((r >> 1) & 7))) << 4);
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int r = (wid * 8 + i) * 8 + (lane >> 3);
    w_voff[i] = (unsigned)(r * ldw) + (unsigned)((((lane & 7) ^ ((r >> 1) & 7))) << 4);
  }
  const int s_row = wid * 64 + lane;
  const unsigned s_voff = s_row < rows_a ? (unsigned)(s_row * 4) : 0x80000000u;  // past the tile's rows: out of any range, nothing is read
  const unsigned s_step = (unsigned)(ldsx * 4);                                   // bytes from one group's scales to the next

#define B_ISSUE(T_, SLOT_)                                                                                                                \
  {                                                                                                                                       \
    char* const st_ = smem + (SLOT_) * B_STAGE_BYTES;                                                                                     \
    _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_)                                                                                      \
      __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (b_lds_ptr_t)(st_ + (wid * 4 + i_) * 1024), 16, a_voff[i_], (unsigned)(T_) * 128u, 0, 0); \
    _Pragma("unroll") for (int i_ = 0; i_ < 8; ++i_)                                                                                      \
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (b_lds_ptr_t)(st_ + B_X_BYTES + (wid * 8 + i_) * 1024), 16, w_voff[i_], (unsigned)(T_) * 128u, 0, 0); \
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (b_lds_ptr_t)(smem + B_SX_OFF + (SLOT_) * B_SX_BYTES + wid * 256), 4, s_voff, (unsigned)(T_) * s_step, 0, 0); \
  }

  // ---- fragment read offsets inside a stage: row (fragment base + r16), chunks g16 and 4 + g16 through the swizzle
  const int swz = (r16 >> 1) & 7;
  const int c0 = (g16 ^ swz) << 4, c1 = ((4 | g16) ^ swz) << 4;
  const int rd_x = (wr * 64 + r16) * 128;              // + mi * 2048
  const int rd_w = B_X_BYTES + (wc * 128 + r16) * 128; // + nj * 2048
  const int rd_s = B_SX_OFF + (wr * 64 + r16) * 4;     // + slot * B_SX_BYTES + mi * 64

  // the wave's block row of sw (clamped for a wave that lies wholly past N)
  const int swrow = min(n0 / 128 + wc, nbw - 1);
  const float* __restrict__ swp = sw + (int64_t)swrow * ldsw;

  f32x4_t acc[4][8];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  const f32x4_t zero = {0.f, 0.f, 0.f, 0.f};
  constexpr int kOne = 0x7f7f7f7f;  // e8m0 2^0 block scales

  B_ISSUE(0, 0)
  if (nk > 1) B_ISSUE(1, 1)
  float sw_next = swp[0];
  int slot = 0, slot2 = 2;  // stage of group t and of group t + 2
  for (int t = 0; t < nk; ++t) {
    // group t has landed (this wave's pieces), every wave is done with group t - 1
    if (t + 1 < nk) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(B_PIECES) : "memory");
    else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    if (t + 2 < nk) B_ISSUE(t + 2, slot2)
    const float swg = sw_next;
    if (t + 1 < nk) sw_next = swp[t + 1];

    const char* const st = smem + slot * B_STAGE_BYTES;
    i32x8_t xf[4];
    float s[4];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
      const i32x4_t lo = *reinterpret_cast<const i32x4_t*>(st + rd_x + mi * 2048 + c0);
      const i32x4_t hi = *reinterpret_cast<const i32x4_t*>(st + rd_x + mi * 2048 + c1);
      xf[mi] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
      s[mi] = *reinterpret_cast<const float*>(smem + rd_s + slot * B_SX_BYTES + mi * 64) * swg;
    }
#pragma unroll
    for (int nj = 0; nj < 8; ++nj) {
      const i32x4_t lo = *reinterpret_cast<const i32x4_t*>(st + rd_w + nj * 2048 + c0);
      const i32x4_t hi = *reinterpret_cast<const i32x4_t*>(st + rd_w + nj * 2048 + c1);
      const i32x8_t wf = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
      f32x4_t p[4];
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) p[mi] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wf, xf[mi], zero, 0, 0, 0, kOne, 0, kOne);
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[mi][nj][e] = __builtin_fmaf(s[mi], p[mi][e], acc[mi][nj][e]);
    }
    slot = slot == B_STAGES - 1 ? 0 : slot + 1;
    slot2 = slot2 == B_STAGES - 1 ? 0 : slot2 + 1;
  }
#undef B_ISSUE
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();  // every wave is past its last fragment read: the ring becomes the epilogue image
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);

  // ---- epilogue phase 1: acc + bias (+ activation) -> bf16 -> LDS [128][B_EPI_LD]
  //      acc[mi][nj][e] = tile row wr*64 + mi*16 + r16, tile column wc*128 + nj*16 + 4*g16 + e
  uint2 bv[8];
#pragma unroll
  for (int nj = 0; nj < 8; ++nj) {
    int gn = n0 + wc * 128 + nj * 16 + 4 * g16;
    gn = gn + 3 < N ? gn : N - 4;  // N >= 8
    bv[nj] = make_uint2(0u, 0u);
    if (bias != nullptr) bv[nj] = *reinterpret_cast<const uint2*>(bias + gn);
  }
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int nj = 0; nj < 8; ++nj) {
      const int ml = wr * 64 + mi * 16 + r16, nl = wc * 128 + nj * 16 + 4 * g16;
      float vv[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) vv[e] = acc[mi][nj][e];
      epi_bias_act4<EPI>(vv, bv[nj].x, bv[nj].y);
      uint2 pk;
      pk.x = pack_bf2(vv[0], vv[1]);
      pk.y = pack_bf2(vv[2], vv[3]);
      *reinterpret_cast<uint2*>(smem + ml * B_EPI_LD + nl * 2) = pk;
    }
  __syncthreads();
  // ---- epilogue phase 2: 16-byte stores, 32 lanes per 512-byte output row; the residual step on the bf16 values
#pragma unroll 4
  for (int it = 0; it < 16; ++it) {
    const int id = it * 256 + tid;
    const int row = id >> 5, cc = id & 31;
    const int64_t gmr = m0 + row;
    const int gn = n0 + cc * 8;
    if (gmr < M && gn < N) {
      uint4 o = *reinterpret_cast<const uint4*>(smem + row * B_EPI_LD + cc * 16);
      if (EPI == X2V_EPI_RESIDUAL) {
        float yv[8], xv[8], ov[8];
        unpack8(o, yv);
        unpack8(*reinterpret_cast<const uint4*>(resid + gmr * ldr + gn), xv);
        if (gate != nullptr) {
          float gv[8];
          unpack8(*reinterpret_cast<const uint4*>(gate + gn), gv);
#pragma unroll
          for (int e = 0; e < 8; ++e) ov[e] = xv[e] + rbf(yv[e] * gv[e]);
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) ov[e] = xv[e] + yv[e];
        }
        o = pack8(ov);
      }
      *reinterpret_cast<uint4*>(Y + gmr * ldy + gn) = o;
    }
  }
#endif
}

// ---- activation quantiser: 16 lanes per 128-element group (8 bf16 = 16 bytes each), amax across them by shuffles, one 8-byte code store per
//      lane; a workgroup takes 16 groups per pass and walks whole rows.  HBM-bound: reads 2 M K bytes, writes M K + 4 M K / 128.
//      Arithmetic = the reference's torch expression, every step one correctly rounded fp32 operation (include/x2v.h).
__global__ __launch_bounds__(256) void quant_fp8_group128_kernel(const unsigned short* __restrict__ x, int64_t ldx, unsigned char* __restrict__ xq, int64_t ldq,
                                                                 float* __restrict__ sx, int64_t ldsx, int64_t M, int K) {
  const int sub = threadIdx.x & 15, grp = threadIdx.x >> 4;
  const int ng = K >> 7;
  for (int64_t row = blockIdx.x; row < M; row += gridDim.x)
    for (int g = grp; g < ng; g += 16) {
      const int e = g * 128 + sub * 8;
      float v[8];
      unpack8(*reinterpret_cast<const uint4*>(x + row * ldx + e), v);
      float amax = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(v[j]));
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
      const float a = fmaxf(amax, 1e-4f);
      const float r = (1.0f / a) * 448.0f;  // torch's `448.0 / tensor` is reciprocal() * 448.0: two roundings, kept
      unsigned lo = 0, hi = 0;
      lo = __builtin_amdgcn_cvt_pk_fp8_f32(v[0] * r, v[1] * r, lo, false);
      lo = __builtin_amdgcn_cvt_pk_fp8_f32(v[2] * r, v[3] * r, lo, true);
      hi = __builtin_amdgcn_cvt_pk_fp8_f32(v[4] * r, v[5] * r, hi, false);
      hi = __builtin_amdgcn_cvt_pk_fp8_f32(v[6] * r, v[7] * r, hi, true);
      *reinterpret_cast<uint2*>(xq + row * ldq + e) = make_uint2(lo, hi);
      if (sub == 0) sx[(int64_t)g * ldsx + row] = a / 448.0f;
    }
}

}  // namespace x2v

using namespace x2v;

extern "C" __attribute__((visibility("default"))) int x2v_quant_fp8_group128(const void* x, int64_t ldx, void* xq, int64_t ldq, float* sx, int64_t lds, int64_t M, int K,
                                                                            void* stream) {
  X2V_REQUIRE(x && xq && sx, X2V_E_ARG, "quant_fp8_group128: null pointer");
  X2V_REQUIRE(K > 0 && K % 128 == 0, X2V_E_SHAPE, "quant_fp8_group128: K=%d must be a positive multiple of 128", K);
  X2V_REQUIRE(M >= 0 && lds >= M && ldx >= K && ldq >= K, X2V_E_SHAPE, "quant_fp8_group128: M=%lld with ldx=%lld, ldq=%lld (>= K) and lds=%lld (>= M)", (long long)M,
              (long long)ldx, (long long)ldq, (long long)lds);
  X2V_REQUIRE(ldx % 8 == 0 && ldq % 8 == 0 && aligned16(x) && ((uintptr_t)xq % 8) == 0 && ((uintptr_t)sx % 4) == 0, X2V_E_ALIGN, "quant_fp8_group128: row alignment");
  if (M == 0) return X2V_OK;
  const unsigned grid = (unsigned)(M < 65536 ? M : 65536);
  hipLaunchKernelGGL(quant_fp8_group128_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const unsigned short*)x, ldx, (unsigned char*)xq, ldq, sx, lds, M, K);
  X2V_LAUNCH_CHECK("quant_fp8_group128 launch");
  return X2V_OK;
}

extern "C" __attribute__((visibility("default"))) int x2v_gemm_fp8_block128(const void* xq, int64_t ldx, const float* sx, int64_t lds, const void* wq, int64_t ldw, const float* sw,
                                                                           int64_t ldsw, const void* bias, void* y, int64_t ldy, int64_t M, int N, int K, int epilogue,
                                                                           const void* resid, int64_t ldr, const void* gate, void* stream) {
  const char* who = "gemm_fp8_block128";
  X2V_REQUIRE(xq && sx && wq && sw && y, X2V_E_ARG, "%s: null pointer", who);
  X2V_REQUIRE(K > 0 && K % 128 == 0, X2V_E_SHAPE, "%s: K=%d must be a positive multiple of 128", who, K);
  X2V_REQUIRE(M >= 0 && N > 0 && N % 8 == 0, X2V_E_SHAPE, "%s: bad shape M=%lld N=%d (N a multiple of 8)", who, (long long)M, N);
  const int nk = K / 128;
  X2V_REQUIRE(lds >= M && ldsw >= nk, X2V_E_SHAPE, "%s: lds=%lld must be >= M=%lld and the weight-scale row stride %lld >= K / 128 = %d", who, (long long)lds, (long long)M,
              (long long)ldsw, nk);
  X2V_REQUIRE(ldx >= K && ldw >= K && ldx < (1 << 24) && ldw < (1 << 24) && (int64_t)nk * lds * 4 < (1ll << 31), X2V_E_SHAPE,
              "%s: leading dimensions must be >= K and < 16 MiB, the activation-scale table below 2 GiB", who);
  X2V_REQUIRE(ldx % 16 == 0 && ldw % 16 == 0 && aligned16(xq) && aligned16(wq) && ((uintptr_t)sx % 4) == 0 && ((uintptr_t)sw % 4) == 0, X2V_E_ALIGN,
              "%s: operand rows must be 16-byte aligned", who);
  X2V_REQUIRE(ldy % 8 == 0 && ldy >= N && aligned16(y), X2V_E_ALIGN, "%s: output rows must be 16-byte aligned", who);
  X2V_REQUIRE(bias == nullptr || ((uintptr_t)bias % 8) == 0, X2V_E_ALIGN, "%s: bias must be 8-byte aligned", who);
  X2V_REQUIRE(epilogue == X2V_EPI_NONE || epilogue == X2V_EPI_GELU_TANH || epilogue == X2V_EPI_RESIDUAL || epilogue == X2V_EPI_SILU, X2V_E_ARG, "%s: unknown epilogue %d", who,
              epilogue);
  if (epilogue == X2V_EPI_RESIDUAL) {
    X2V_REQUIRE(resid != nullptr, X2V_E_ARG, "%s: residual epilogue needs resid", who);
    X2V_REQUIRE(ldr % 8 == 0 && ldr >= N && aligned16(resid) && aligned16(gate), X2V_E_ALIGN, "%s: resid/gate alignment", who);
  }
  const int64_t ntm = (M + B_M - 1) / B_M;
  const int ntn = (N + B_N - 1) / B_N;
  X2V_REQUIRE(ntm * ntn < (1ll << 31), X2V_E_SHAPE, "%s: too many tiles", who);
  if (M == 0) return X2V_OK;
  return with_epilogue(who, epilogue, resid, ldr, gate, [&](auto epi, const void* r, int64_t lr, const void* g) {
    constexpr int EPI = decltype(epi)::value;
    int rc = ensure_dynamic_lds((const void*)gemm_b128_kernel<EPI>, B_LDS_BYTES, "gemm_fp8_block128 attr");
    if (rc != X2V_OK) return rc;
    hipLaunchKernelGGL((gemm_b128_kernel<EPI>), dim3((unsigned)(ntm * ntn)), dim3(256), B_LDS_BYTES, (hipStream_t)stream, (const char*)xq, ldx, (const char*)wq, ldw, sx, lds, sw,
                       ldsw, (N + 127) / 128, (const unsigned short*)bias, (unsigned short*)y, ldy, M, N, nk, (const unsigned short*)r, lr, (const unsigned short*)g, (int)ntm,
                       ntn);
    X2V_LAUNCH_CHECK("gemm_fp8_block128 launch");
    return (int)X2V_OK;
  });
}
