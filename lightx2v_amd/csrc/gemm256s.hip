// y[M,N] = epi(x[M,K] . W[N,K]^T + bias), bf16 — the large-shape GEMM as ONE wave per SIMD running a single software-pipelined stream.
// Same contract, operand layouts, epilogues and rounding points as gemm.hip / gemm256.hip.
//
// Bound: MFMA (bf16 dense peak ~2.5 PFLOP/s; at this board's 1400 W limit a bare 16x16x32 MFMA loop with GEMM-like LDS traffic sustains
// ~1.8 PFLOP/s, tools/probes/mfma_power_probe.hip).  Algorithmic work 2*M*N*K FLOP per launch.
//
// Why a third structure.  gemm256.hip keeps two waves per SIMD and hands the matrix pipe from one to the other through a barrier every
// 16 MFMAs; the pipe idles over every hand-off (85 % MFMA-busy) and each wave's 128x64 tile reads 0.75 KiB of LDS per MFMA-equivalent.
// Here a 256-thread workgroup owns the same 256x256 output tile with four waves of 128x128 (2 x 2), one per SIMD:
//   * 64 accumulator tiles of 16x16 per wave = the whole accumulator half of the register file (a[0:255]), addressed by literal
//     register number from the asm MFMA statements of this file only — hipcc never sees them (audit rule below);
//   * no hand-off: the wave's own stream is {MFMA | at most one ds_read_b128 or one LDS-DMA issue} per slot, 128 slots per 64-wide K tile,
//     pinned with sched_barrier; fragments for k-step s+1 are read while k-step s multiplies (0.5 KiB of LDS per MFMA-equivalent);
//   * two LDS stages of {W tile | x tile} (2 x 64 KiB, [256 rows][128 B] images with the chunk ^= (row>>1)&7 swizzle on the DMA source
//     offset and on the fragment address); which slot of a K tile carries which read, DMA piece, wait and barrier: the slot plan in
//     gemm256_pipe.h, which this file shares with the continuous kernels gemm256c.hip / gemm256c8.hip;
//   * M / N tails, K-blocked x and N-blocked y (GemmBlocking), the LDS-staged epilogue: as gemm256.hip.
// AUDIT after every edit (the accumulator half is invisible to the compiler): `hipcc -S` must show .vgpr_spill_count 0,
// .private_segment_fixed_size 0 and no v_accvgpr_* / a[..] operand outside ;;#ASMSTART / ;;#ASMEND.
#include "gemm256_pipe.h"

namespace x2v {
using namespace pipe;

constexpr int S_EPI_LD = 528;                // bytes per epilogue row (256 bf16 + 16 pad)
constexpr int S_LDS_BYTES = 256 * S_EPI_LD;  // 135168 >= the two stages (LDS_BYTES)
static_assert(S_LDS_BYTES >= LDS_BYTES, "the epilogue's staging area covers the two stages");

template <int R>
__device__ __forceinline__ void s_acc_zero() {
  asm volatile("v_accvgpr_write_b32 a[%c0], 0" ::"i"(R) : X2V_AGPRS);
}

// VT (epilogue NONE only): y is written TRANSPOSED per head and 64-token block — V^T [N/128][ldy/64][128][64], the operand layout of the
// ping-pong attention kernel (x2v_transpose_heads_bf16's output), tokens in [M, ldy) zero-filled.  The MFMA operands swap roles, so a lane
// owns four consecutive TOKENS of one output channel and the staging / store code stays 8- and 16-byte wide; every (m, n) sums the same
// products in the same order as in the row-major form (bit-identical values).
template <int EPI, bool VT = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void gemm256s_kernel(
    const char* __restrict__ A, int64_t lda_bytes, const char* __restrict__ W, int64_t ldw_bytes, const unsigned short* __restrict__ bias,
    unsigned short* __restrict__ Y, int64_t ldy, int64_t M, int N, int nk, const unsigned short* __restrict__ resid, int64_t ldr,
    const unsigned short* __restrict__ gate, int ntm, int ntn, int gm_tiles, GemmBlocking gb) {
#if defined(__HIP_DEVICE_COMPILE__)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  claim_accumulators();
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wid >> 1, wc = wid & 1;
  const int r16 = lane & 15, g16 = lane >> 4;

  // ---- this workgroup's tile: XCD chunking + grouped ordering
  const unsigned nblk = (unsigned)ntm * (unsigned)ntn;
  const unsigned v = xcd_remap(blockIdx.x, nblk);
  X2V_PIPE_COORDS()
  int tm, tn;
  coords(v, tm, tn);
  const int64_t m0 = (int64_t)tm * TILE;
  const int n0 = tn * TILE;

  // ---- buffer descriptors over this tile's valid rows: rows past M / N read as zero through the bounds check.  Written out here, and the K-block
  //      wrap computed in place below: through gemm256_pipe.h's `operands` lambda / with the wrap hoisted into a named value as in the continuous
  //      kernels, this kernel allocates one SGPR less and ~700 instructions of its stream move (tools/isa_diff.py).
  const unsigned row_bytes = (unsigned)nk * 128u;
  const int rows_a = (int)min((int64_t)TILE, M - m0), rows_w = min(TILE, N - n0);
  const int a_kpb = gb.a_kpb > 0 && gb.a_kpb < nk ? gb.a_kpb : nk;  // K tiles per K block of x (GemmBlocking)
  const unsigned a_span = a_kpb < nk ? (unsigned)((nk - 1) / a_kpb) * gb.a_cbs + (unsigned)a_kpb * 128u : row_bytes;
  const __amdgpu_buffer_rsrc_t ra =
      __builtin_amdgcn_make_buffer_rsrc((void*)(A + m0 * lda_bytes), 0, (unsigned)((rows_a - 1) * lda_bytes) + a_span, 0x00020000);
  const __amdgpu_buffer_rsrc_t rw =
      __builtin_amdgcn_make_buffer_rsrc((void*)(W + (int64_t)n0 * ldw_bytes), 0, (unsigned)((rows_w - 1) * ldw_bytes) + row_bytes, 0x00020000);
  // byte offsets of x's K tiles t+1 and t+2 within a row (K-blocked x: GemmBlocking) and the index of tile t+2 within its K block
  unsigned ak1 = 0, ak2 = 0;
  int akc2 = 0;
#define S_AK_NEXT(OFF_, CNT_) X2V_PIPE_NEXT_KA(OFF_, CNT_, X2V_PIPE_A_WRAP())
  S_AK_NEXT(ak2, akc2)
  ak1 = ak2;
  S_AK_NEXT(ak2, akc2)

  X2V_PIPE_DMA_OFFSETS()
  X2V_PIPE_BF16_FRAGMENTS()
#define S_DMA(P_, STAGE_, KW_, KA_) X2V_PIPE_DMA_AT(P_, STAGE_, ra, rw, KW_, KA_)
#define S_SB() __builtin_amdgcn_sched_barrier(0)

  static_for<0, 256>([&](auto rc) { s_acc_zero<decltype(rc)::value>(); });

  // ---- prologue: tile 0 and the first EARLY pieces of tile 1 in flight, tile 0 landed, k-step 0 of tile 0 in registers
  static_for<0, 16>([&](auto pc) { S_DMA(decltype(pc)::value, 0, 0u, 0u) });
  if (nk > 1) {
    static_for<0, EARLY>([&](auto pc) { S_DMA(decltype(pc)::value, 1, 128u, ak1) });
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(EARLY) : "memory");
  } else {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __builtin_amdgcn_s_barrier();
  S_SB();
  static_for<0, 16>([&](auto rc) { X2V_PIPE_BF16_READ(decltype(rc)::value, 0, 0) });
  S_SB();

  // One K tile.  ST = its stage; CHK = 0: steady state (tiles t+1 and t+2 exist), 1: tail (run-time tests).
  auto tile = [&](auto stc, auto chkc, int t) {
    constexpr int ST = decltype(stc)::value;
    constexpr bool CHK = decltype(chkc)::value != 0;
    const bool has1 = CHK ? (t + 1 < nk) : true, has2 = CHK ? (t + 2 < nk) : true;
    const unsigned kw1 = (unsigned)(t + 1) * 128u, kw2 = (unsigned)(t + 2) * 128u;
    static_for<0, 128>([&](auto nc) {
      constexpr int n = decltype(nc)::value, ks = n >> 6, xb = (n >> 3) & 7, wb = n & 7;
      if constexpr (VT) mfma_bf16<xb * 8 + wb>(fx[ks][xb], fw[ks][wb]);
      else mfma_bf16<xb * 8 + wb>(fw[ks][wb], fx[ks][xb]);
      if constexpr (n < 32 && (n & 1) == 0) X2V_PIPE_BF16_READ(n >> 1, ST, 1)  // k-step 1 of this tile
      // the last 16 - EARLY pieces of tile t+1 (its stage was freed by the previous tile's first barrier)
      if constexpr (late_slot(n)) {
        if (has1) S_DMA(EARLY + (n - LATE0) / STEP, ST ^ 1, kw1, ak1)
      }
      if constexpr (n == FREE) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // every fragment of this tile is in registers: the stage may be overwritten
        __builtin_amdgcn_s_barrier();
      }
      // the first EARLY pieces of tile t+2 into this tile's stage
      if constexpr (dma_slot(n)) {
        if (has2) S_DMA((n - FREE - 1) / STEP, ST, kw2, ak2)
      }
      if constexpr (n == READY) {
        if (has1) {
          // tile t+1 has landed; the pieces of tile t+2 issued so far in this tile may stay in flight
          if (has2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NEWER) : "memory");
          else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          __builtin_amdgcn_s_barrier();
        }
      }
      if constexpr (n > READY + 1 && (n & 1) == 0) {
        if (has1) X2V_PIPE_BF16_READ((n - READY - 2) >> 1, ST ^ 1, 0)  // k-step 0 of the next tile
      }
      S_SB();
    });
    ak1 = ak2;
    if (has2) S_AK_NEXT(ak2, akc2)
  };
  using c0 = std::integral_constant<int, 0>;
  using c1 = std::integral_constant<int, 1>;
  int t = 0;
  const int nmain = nk > 2 ? ((nk - 2) & ~1) : 0;  // tiles [0, nmain): t + 2 < nk throughout
  for (; t < nmain; t += 2) {
    tile(c0{}, c0{}, t);
    tile(c1{}, c0{}, t + 1);
  }
  for (; t < nk; t += 2) {
    tile(c0{}, c1{}, t);
    if (t + 1 < nk) tile(c1{}, c1{}, t + 1);
  }
#undef S_DMA
#undef S_AK_NEXT
  asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 7" ::: "memory");  // the last MFMAs' results before the accumulator reads below
  __builtin_amdgcn_s_barrier();                                 // every wave is past its last fragment read: LDS becomes the staging area
  S_SB();

  if constexpr (VT) {
    static_assert(EPI == X2V_EPI_NONE, "V^T output: plain epilogue only");
    // ---- phase 1: tile (xb, wb), register e: channel wc*128 + wb*16 + r16, token wr*128 + xb*16 + 4*g16 + e  ->  LDS [256 channels][S_EPI_LD]
    float bvt[8];
#pragma unroll
    for (int wb = 0; wb < 8; ++wb) {
      const int gn = n0 + wc * 128 + wb * 16 + r16;
      bvt[wb] = (bias != nullptr && gn < N) ? bf2f(bias[gn]) : 0.f;
    }
    static_for<0, 64>([&](auto ic) {
      constexpr int I = decltype(ic)::value, xb = I >> 3, wb = I & 7;
      const int nl = wc * 128 + wb * 16 + r16, ml = wr * 128 + xb * 16 + 4 * g16;
      uint2 pk;
      pk.x = pack_bf2(acc_read<4 * I + 0>() + bvt[wb], acc_read<4 * I + 1>() + bvt[wb]);
      pk.y = pack_bf2(acc_read<4 * I + 2>() + bvt[wb], acc_read<4 * I + 3>() + bvt[wb]);
      *reinterpret_cast<uint2*>(smem + nl * S_EPI_LD + ml * 2) = pk;
    });
    __syncthreads();
    // ---- phase 2: a channel's 256 tokens = four 128-byte runs of V^T; 16-byte stores, tokens past M zeroed, blocks past ldy skipped
#pragma unroll 4
    for (int it = 0; it < 32; ++it) {
      const int id = it * 256 + tid;
      const int ch = id >> 5, cc = id & 31;  // channel within the tile, 8-token chunk
      const int gn = n0 + ch;
      const int64_t tok = m0 + cc * 8;
      if (gn < N && tok < ldy) {
        uint4 o = *reinterpret_cast<const uint4*>(smem + ch * S_EPI_LD + cc * 16);
        if (tok + 8 > M) {
          unsigned short h[8];
          *reinterpret_cast<uint4*>(h) = o;
#pragma unroll
          for (int e = 0; e < 8; ++e)
            if (tok + e >= M) h[e] = 0;
          o = *reinterpret_cast<const uint4*>(h);
        }
        const int64_t blocks = ldy >> 6;  // 64-token blocks per head
        unsigned short* dst = Y + (((int64_t)(gn >> 7) * blocks + (tok >> 6)) * 128 + (gn & 127)) * 64 + (tok & 63);
        *reinterpret_cast<uint4*>(dst) = o;
      }
    }
  } else {
  // ---- epilogue addressing: the output tile (and the residual tile) through buffer descriptors whose base is the tile's first element; a thread's
    //      chunk (row tid>>5 + 8 it, columns 8 (tid&31)..) is a per-thread 32-bit offset + a per-iteration SCALAR offset 8 it rows — no 64-bit
    //      address registers per iteration (they cost the residual variant 9 spilled VGPRs once its loads were hoisted).  Rows / columns past M / N
    //      are predicated off below; the descriptor range only has to cover the tile.
    const int erow = tid >> 5, ecc = tid & 31;
    const int egn = n0 + ecc * 8;
    const int64_t eycol = gb.y_cbw > 0 ? (int64_t)(egn / gb.y_cbw) * gb.y_cbs + egn % gb.y_cbw : egn;  // N-blocked y (GemmBlocking)
    const bool ecol_ok = egn < N;
    const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc((void*)(Y + m0 * ldy), 0, 0xffffffffu, 0x00020000);
    const unsigned y_voff = (unsigned)((erow * ldy + eycol) * 2), y_step = (unsigned)(8 * ldy * 2);
  // ---- epilogue phase 0 (residual epilogue): this thread's 32 residual chunks (the rows / columns it will store in phase 2) are requested NOW,
    //      into the registers the fragments no longer need, so that ONE memory latency runs under the accumulator -> LDS pass instead of eight
    //      dependent round trips inside the store loop (the residual variant ran 8 % below the plain one per FLOP: ~10 us of a 117 us tile).
    u32x4_t rres[32];
    if constexpr (EPI == EPI_RESIDUAL_PERIODIC) {
      // row period: the residual addressed from ITS first row, each chunk (one row per lane) at its own row mod the period
      const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc((void*)resid, 0, 0xffffffffu, 0x00020000);
      const unsigned row0 = resid_tile_row(m0, gb.r_period);
  #pragma unroll
      for (int it = 0; it < 32; ++it) {
        rres[it] = u32x4_t{0u, 0u, 0u, 0u};
        if (ecol_ok && m0 + erow + 8 * it < M)
          rres[it] = __builtin_amdgcn_raw_buffer_load_b128(rr, (resid_row(row0, erow + 8 * it, gb.r_period) * (unsigned)ldr + (unsigned)egn) * 2u, 0u, 0);
      }
    } else if constexpr (EPI == X2V_EPI_RESIDUAL) {
      const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc((void*)(resid + m0 * ldr), 0, 0xffffffffu, 0x00020000);
      const unsigned r_voff = (unsigned)((erow * ldr + egn) * 2), r_step = (unsigned)(8 * ldr * 2);
  #pragma unroll
      for (int it = 0; it < 32; ++it) {
        rres[it] = u32x4_t{0u, 0u, 0u, 0u};
        if (ecol_ok && m0 + erow + 8 * it < M) rres[it] = __builtin_amdgcn_raw_buffer_load_b128(rr, r_voff, (unsigned)it * r_step, 0);
      }
    }
  // ---- epilogue phase 1: acc (+bias, activation) -> bf16 -> LDS [256][S_EPI_LD]
    //      tile (xb, wb), register e: tile row wr*128 + xb*16 + r16, tile col wc*128 + wb*16 + 4*g16 + e
    uint2 bv[8];
  #pragma unroll
    for (int wb = 0; wb < 8; ++wb) {
      int gn = n0 + wc * 128 + wb * 16 + 4 * g16;
      gn = gn + 3 < N ? gn : (N >= 4 ? N - 4 : 0);
      bv[wb] = make_uint2(0u, 0u);
      if (bias != nullptr) bv[wb] = *reinterpret_cast<const uint2*>(bias + gn);
    }
    static_for<0, 64>([&](auto ic) {
      constexpr int I = decltype(ic)::value, xb = I >> 3, wb = I & 7;
      const int ml = wr * 128 + xb * 16 + r16, nl = wc * 128 + wb * 16 + 4 * g16;
      float vv[4] = {acc_read<4 * I + 0>(), acc_read<4 * I + 1>(), acc_read<4 * I + 2>(), acc_read<4 * I + 3>()};
      X2V_EPI_BIAS_ACT4(EPI, vv, bv[wb].x, bv[wb].y);  // epi_bias_act4's body in place (x2v_common.h says why)
      uint2 pk;
      pk.x = pack_bf2(vv[0], vv[1]);
      pk.y = pack_bf2(vv[2], vv[3]);
      *reinterpret_cast<uint2*>(smem + ml * S_EPI_LD + nl * 2) = pk;
    });
    __syncthreads();
    // ---- epilogue phase 2: 16-byte stores, 32 lanes per 512-byte output row
    if constexpr (epi_is_residual(EPI)) {
      float gv[8];  // per-column gate chunk: the same 8 columns in every iteration of this thread
      {
        uint4 g4 = make_uint4(0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u);
        if (gate != nullptr && ecol_ok) g4 = *reinterpret_cast<const uint4*>(gate + egn);
        unpack8(g4, gv);
      }
  #pragma unroll
      for (int it = 0; it < 32; ++it) {
        if (ecol_ok && m0 + erow + 8 * it < M) {
          float yv[8], xv[8], ov[8];
          unpack8(*reinterpret_cast<const uint4*>(smem + (erow + 8 * it) * S_EPI_LD + ecc * 16), yv);
          unpack8(__builtin_bit_cast(uint4, rres[it]), xv);
          if (gate != nullptr) {
  #pragma unroll
            for (int e = 0; e < 8; ++e) ov[e] = xv[e] + rbf(yv[e] * gv[e]);
          } else {
  #pragma unroll
            for (int e = 0; e < 8; ++e) ov[e] = xv[e] + yv[e];
          }
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, pack8(ov)), ry, y_voff, (unsigned)it * y_step, 0);
        }
      }
    } else {
  #pragma unroll 4
      for (int it = 0; it < 32; ++it) {
        if (ecol_ok && m0 + erow + 8 * it < M)
          __builtin_amdgcn_raw_buffer_store_b128(*reinterpret_cast<const u32x4_t*>(smem + (erow + 8 * it) * S_EPI_LD + ecc * 16), ry, y_voff, (unsigned)it * y_step, 0);
      }
    }
}
#undef S_SB
#endif
}

template <int EPI, bool VT = false>
static int launch_gemm256s(const void* x, int64_t ldx_bytes, const void* w, int64_t ldw_bytes, const void* bias, void* y, int64_t ldy, int64_t M, int N, int nk,
                           const void* resid, int64_t ldr, const void* gate, int gm_tiles, hipStream_t st, GemmBlocking gb) {
  if (gm_tiles <= 0) gm_tiles = 4;
  const int ntm = (int)((M + TILE - 1) / TILE), ntn = (N + TILE - 1) / TILE;
  int rc = ensure_dynamic_lds((const void*)gemm256s_kernel<EPI, VT>, S_LDS_BYTES, "gemm256s attr");
  if (rc != X2V_OK) return rc;
  hipLaunchKernelGGL((gemm256s_kernel<EPI, VT>), dim3((unsigned)ntm * (unsigned)ntn), dim3(256), S_LDS_BYTES, st, (const char*)x, ldx_bytes, (const char*)w, ldw_bytes,
                     (const unsigned short*)bias, (unsigned short*)y, ldy, M, N, nk, (const unsigned short*)resid, ldr, (const unsigned short*)gate, ntm, ntn, gm_tiles, gb);
  X2V_LAUNCH_CHECK("gemm256s launch");
  return X2V_OK;
}

// Called by gemm.hip's dispatcher (arguments already validated there; ld*_bytes < 16 MiB checked by the caller).
int gemm256s_dispatch(int epilogue, const void* x, int64_t ldxb, const void* w, int64_t ldwb, const void* bias, void* y, int64_t ldy, int64_t M, int N, int nk,
                      const void* resid, int64_t ldr, const void* gate, int gm_tiles, hipStream_t st, GemmBlocking gb) {
  return with_epilogue("gemm", epilogue, resid, ldr, gate, gb, [&](auto epi, const void* r, int64_t lr, const void* g) {
    return launch_gemm256s<decltype(epi)::value>(x, ldxb, w, ldwb, bias, y, ldy, M, N, nk, r, lr, g, gm_tiles, st, gb);
  });
}

// V^T-producing form (x2v_gemm_bf16_vt): y = V^T [N/128][ldvt/64][128][64]; `ldvt` travels in the ldy argument
int gemm256s_vt_dispatch(const void* x, int64_t ldxb, const void* w, int64_t ldwb, const void* bias, void* vt, int64_t ldvt, int64_t M, int N, int nk, hipStream_t st) {
  return launch_gemm256s<X2V_EPI_NONE, true>(x, ldxb, w, ldwb, bias, vt, ldvt, M, N, nk, nullptr, 0, nullptr, 0, st, GemmBlocking());
}

}  // namespace x2v
