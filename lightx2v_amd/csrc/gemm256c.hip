// y[M,N] = epi(x[M,K] . W[N,K]^T + bias), bf16 — gemm256s.hip's single-stream 256x256 kernel as a CONTINUOUS pipeline over output tiles.
// Same contract, operand layouts, epilogues, rounding points, MFMA and k order as gemm.hip / gemm256.hip / gemm256s.hip: bit-equal results
// (asserted in tests/test_gpu_bench_shapes.py::test_gemm_continuous_pipeline_equals_one_tile_per_workgroup against the one-tile-per-workgroup kernel).
//
// Bound: MFMA (bf16 dense peak ~2.5 PFLOP/s; at this board's 1400 W limit a bare 16x16x32 MFMA loop with GEMM-like LDS traffic sustains
// ~1.8 PFLOP/s, tools/probes/mfma_power_probe.hip).  Algorithmic work 2*M*N*K FLOP per launch.
//
// What this file changes.  A one-workgroup-per-CU kernel has nothing on its matrix pipe during its own prologue
// (first operand tiles in flight: a full memory latency) and epilogue (accumulators -> LDS -> barrier -> 16-byte stores): ~5 us of a 117 us
// output tile at K = 5120, ~20 % of a tile at K = 1536.  Here
//   * a workgroup is PERSISTENT: it walks the output tiles of its XCD's chunk of the grouped tile order (the same assignment an in-order
//     dispatch of gemm256s gives), grid = CUs;
//   * the K loop is ONE software pipeline over (output tile, K tile) pairs: the "tile t+1 / t+2" LDS-DMA cursors of gemm256s's slot plan simply
//     run on into the next output tile with that tile's buffer descriptors, so after the first output tile there is no prologue — when an output
//     tile's last K tile retires, K tile 0 of the next one has landed in LDS and K tile 1 is in flight;
//   * the epilogue needs no workgroup barrier and no tile-wide LDS staging — LDS is busy holding the next output tile's operands: each wave
//     transposes its own 128 x 128 part through a private 4 KiB strip, 16 rows at a time, and stores whole 128-byte lines (see "epilogue" below);
//   * the per-column epilogue operands (bias, gate) and the first residual chunks are requested inside the LAST K tile's slot stream (one buffer
//     load in an otherwise empty slot), the following residual chunks one x block ahead of their use;
//   * the first k-step of an output tile issues its 64 MFMAs with C = 0 (inline constant) instead of 256 v_accvgpr_write.
// Measured (profiles/r04_gemm_continuous_ab.txt): +5..12 % at K = 1536 (a 25 us tile), -0.3..+1.8 % at K = 5120 / 13824, where the board's power cap and
// not the per-tile overhead sets the rate.  The first form of the epilogue — 8-byte stores straight from the accumulator layout, four partial writes per
// 128-byte line — was 5 % (K = 5120) to 13 % (K = 1536) slower than not storing at all; hence the transposition strip.
// Slot plan, LDS images and swizzle, tile schedule, LDS-DMA pieces, the K-tile slot stream and the output-tile loop: gemm256_pipe.h, shared with
// gemm256s.hip and gemm256c8.hip; this file holds the bf16 MFMA placement and the epilogue.  Needs an even number of K tiles >= 4 (every output
// tile then starts in LDS stage 0) and N a multiple of 256; other shapes, the V^T output mode and y blocks that are not multiples of a wave's 128
// columns stay on gemm256s (gemm.hip: continuous_ok).
// Cache policies (profiles/r04_call6_i2v_and_gemm_policy_sweep.txt): non-temporal output stores gain 1.9 % at 5120->13824 + GELU only, nothing elsewhere;
// a non-temporal x-operand LDS-DMA loses 2..6 % (every x tile is re-read by the n-tiles of its group).  Both stay at the default policy.
// AUDIT after every edit (the accumulator half is invisible to the compiler): `hipcc -S` must show .vgpr_spill_count 0,
// .private_segment_fixed_size 0 and no v_accvgpr_* / a[..] operand outside ;;#ASMSTART / ;;#ASMEND.
#include "gemm256_pipe.h"

namespace x2v {
using namespace pipe;

constexpr int C_STRIP_BYTES = 16 * 256;  // per wave: the epilogue's transposition strip, one x block (16 rows x 128 bf16) at a time
constexpr int C_LDS_TOTAL = LDS_BYTES + 4 * C_STRIP_BYTES;
static_assert(xload_slots() >= 13, "bias (8) + gate (1) + the residual chunks of one x block (4) need a slot each");

template <int EPI>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void gemm256c_kernel(
    const char* __restrict__ A, int64_t lda_bytes, const char* __restrict__ W, int64_t ldw_bytes, const unsigned short* __restrict__ bias, unsigned short* Y,
    int64_t ldy, int64_t M, int N, int nk, const unsigned short* resid, int64_t ldr, const unsigned short* __restrict__ gate, int ntm, int ntn, int gm_tiles,
    GemmBlocking gb) {
#if defined(__HIP_DEVICE_COMPILE__)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  claim_accumulators();
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wid >> 1, wc = wid & 1;
  const int r16 = lane & 15, g16 = lane >> 4;
  X2V_PIPE_PERSISTENT_CHUNK()
  X2V_PIPE_COORDS()
  X2V_PIPE_OPERANDS()
  X2V_PIPE_DMA_OFFSETS()
  X2V_PIPE_BF16_FRAGMENTS()

  // ---- epilogue of the CURRENT output tile.  LDS holds the next output tile's operands, so the accumulators cannot be staged tile-wide as in
  //      gemm256s; going straight from the accumulator layout to memory (8 bytes per lane, four partial writes per 128-byte line) was measured
  //      5 % (K = 5120) to 13 % (K = 1536) slower than not storing at all (profiles/r04_gemm_continuous_*).  So each WAVE transposes its own
  //      128 x 128 part through a private 4 KiB strip of the LDS the two stages leave free — 16 rows (one x block) at a time, no workgroup
  //      barrier: phase A writes the 8 accumulator tiles of an x block (+ bias, activation, bf16) as 8-byte pieces into a [16 rows][256 B] image
  //      (16-byte chunk index XOR row: conflict-free both ways), phase B reads it back row-major, 16 bytes per lane, and issues 4 stores of
  //      4 rows x 256 contiguous bytes (whole 128-byte lines), combining with the residual chunk of the same shape first.  LDS executes a wave's
  //      instructions in order, so phase A of the next x block may overwrite the strip right behind phase B's reads.
  //      Addressing: N is a multiple of 256 and y blocks (GemmBlocking) are whole multiples of a wave's 128 columns (dispatcher), so a wave's 128
  //      columns are contiguous in memory and start at a wave-uniform offset; a phase-B access of x block xb, instruction i is
  //      vector offset = lane part (row wr*128 + (lane>>4), columns 8 (lane&15).. of the wave) or the "row does not exist" mark 0x80000000 (outside
  //      every descriptor's range: the bounds check drops the access)  +  scalar offset = wave's column base + (16 xb + 4 i) rows.
  //      The per-column operands (bias in phase-A layout, gate in phase-B layout) and the residual chunks of x block 0 are requested inside the
  //      LAST K tile's slot stream; the residual chunks of x block xb + 1 while x block xb is processed.
  u32x2_t e_bias[8];
  u32x4_t e_gate4, e_res[2][4];
  __amdgpu_buffer_rsrc_t r_y, r_res, r_bias, r_gate;
  char* const strip = smem + LDS_BYTES + wid * C_STRIP_BYTES;
  const int l4 = lane >> 4, c16 = lane & 15;
  const unsigned lane_off = (unsigned)((wr * 128 + l4) * ldy * 2) + (unsigned)(16 * c16);  // phase B: bytes from the tile's first row / the wave's first column
  unsigned s_col = 0u;    // the wave's first column in the output / residual row, bytes (wave-uniform)
  unsigned s_bias = 0u;   // the wave's first column in bias / gate, bytes
  int rows_left = 0;      // valid rows of the current tile below row wr*128 + (lane>>4): phase-B row 16 xb + 4 i of the lane exists iff it is < rows_left
  const unsigned y_row = (unsigned)(ldy * 2);  // one row of y (and of the residual: ldr == ldy, y row-major — dispatcher), bytes
  constexpr bool RES = epi_is_residual(EPI);
  constexpr bool RP = EPI == EPI_RESIDUAL_PERIODIC;  // output row r combines with residual row r mod gb.r_period
  // RP: the residual is addressed from ITS first row; a chunk's row travels in the scalar offset, the lane keeps its row within the chunk
  const unsigned lane_off_r = (unsigned)(l4 * ldy * 2) + (unsigned)(16 * c16);
  unsigned s_rrow = 0u;  // RP: residual row of the wave's first row of the current tile (wave-uniform)
  constexpr int NXLOAD = RES ? 8 + 1 + 4 : 8;  // bias (8) [+ gate (1) + the residual chunks of x block 0 (4)]

  // Set up the epilogue addressing of output tile (tm, tn).  Runs when the tile becomes current (scalar instructions + one vector subtract).
  auto epilogue_setup = [&](int tm, int tn) {
    const int64_t m0 = (int64_t)tm * TILE;
    const int gn0 = tn * TILE + wc * 128;  // first column of this wave (wave-uniform)
    r_y = __builtin_amdgcn_make_buffer_rsrc((void*)(Y + m0 * ldy), 0, 0x80000000u, 0x00020000);
    r_bias = __builtin_amdgcn_make_buffer_rsrc((void*)bias, 0, bias != nullptr ? (unsigned)N * 2u : 0u, 0x00020000);
    unsigned col = (unsigned)gn0;
    if (gb.y_cbw > 0) {  // N-blocked y: column n at (n / y_cbw) * y_cbs + n % y_cbw elements from the row's start
      const unsigned qb = (unsigned)gn0 / (unsigned)gb.y_cbw;
      col = qb * (unsigned)gb.y_cbs + ((unsigned)gn0 - qb * (unsigned)gb.y_cbw);
    }
    s_col = col * 2u;
    s_bias = (unsigned)gn0 * 2u;
    rows_left = (int)min((int64_t)TILE, M - m0) - wr * 128 - l4;
    if constexpr (RP) {
      r_res = __builtin_amdgcn_make_buffer_rsrc((void*)resid, 0, 0x80000000u, 0x00020000);
      s_rrow = resid_tile_row(m0 + wr * 128, gb.r_period);
      r_gate = __builtin_amdgcn_make_buffer_rsrc((void*)gate, 0, gate != nullptr ? (unsigned)N * 2u : 0u, 0x00020000);
    } else if constexpr (RES) {
      r_res = __builtin_amdgcn_make_buffer_rsrc((void*)(resid + m0 * ldy), 0, 0x80000000u, 0x00020000);
      r_gate = __builtin_amdgcn_make_buffer_rsrc((void*)gate, 0, gate != nullptr ? (unsigned)N * 2u : 0u, 0x00020000);
    }
  };
  auto row_voff = [&](int row16) { return row16 < rows_left ? lane_off : 0x80000000u; };  // phase-B vector offset of local row `row16` (= 16 xb + 4 i)
  auto res_load = [&](auto xbc, auto ic) {  // residual chunk i of x block xb: the 16 bytes phase B's store i of that block will overwrite
    constexpr int xb = decltype(xbc)::value, i = decltype(ic)::value;
    if constexpr (RP)  // the chunk's 4 rows lie on one side of the period (gemm256_pipe.h: resid_chunk_row)
      e_res[xb & 1][i] = __builtin_bit_cast(u32x4_t, __builtin_amdgcn_raw_buffer_load_b128(r_res, 16 * xb + 4 * i < rows_left ? lane_off_r : 0x80000000u,
                                                                                           s_col + resid_chunk_row(s_rrow, 16 * xb + 4 * i, gb.r_period) * y_row, 0));
    else
    e_res[xb & 1][i] = __builtin_bit_cast(u32x4_t, __builtin_amdgcn_raw_buffer_load_b128(r_res, row_voff(16 * xb + 4 * i), s_col + (unsigned)(16 * xb + 4 * i) * y_row, 0));
  };
  // epilogue-operand load J_ of the current output tile (LAST K tile)
  auto xload = [&](auto jc) {
    constexpr int J = decltype(jc)::value;
    if constexpr (J < 8) {
      e_bias[J] = __builtin_bit_cast(u32x2_t, __builtin_amdgcn_raw_buffer_load_b64(r_bias, (unsigned)(8 * g16), s_bias + (unsigned)(J * 32), 0));
    } else if constexpr (RES && J == 8) {
      e_gate4 = __builtin_bit_cast(u32x4_t, __builtin_amdgcn_raw_buffer_load_b128(r_gate, (unsigned)(16 * c16), s_bias, 0));
    } else if constexpr (RES && J < 8 + 1 + 4) {
      res_load(std::integral_constant<int, 0>{}, std::integral_constant<int, J - 9>{});
    }
  };

  // Phase A of accumulator tile I: value e of the lane = row wr*128 + xb*16 + r16, column wc*128 + wb*16 + 4*g16 + e of the output tile: bias,
  // activation, bf16, 8 bytes into the strip's image of x block xb.
  auto epi_phase_a = [&](auto ic) {
    constexpr int I = decltype(ic)::value, wb = I & 7;
    float vv[4] = {acc_read<4 * I + 0>(), acc_read<4 * I + 1>(), acc_read<4 * I + 2>(), acc_read<4 * I + 3>()};
    epi_bias_act4<EPI>(vv, e_bias[wb].x, e_bias[wb].y);
    // [row r16][256 B], 16-byte chunk (2 wb + (g16 >> 1)) ^ r16, half g16 & 1
    const int wa = r16 * 256 + (((((g16 >> 1) ^ r16) << 4)) ^ (wb * 32)) + (g16 & 1) * 8;
    *reinterpret_cast<u32x2_t*>(strip + wa) = u32x2_t{pack_bf2(vv[0], vv[1]), pack_bf2(vv[2], vv[3])};
  };
  // Phase B, instruction i of x block xb: local rows 16 xb + 4 i + (lane >> 4), this lane's 8 columns 8 (lane & 15)..: strip -> (residual) -> memory
  auto epi_phase_b = [&](auto xbc, auto ic) {
    constexpr int xb = decltype(xbc)::value, i = decltype(ic)::value;
    const int ra = (4 * i + l4) * 256 + ((c16 ^ (4 * i + l4)) << 4);
    u32x4_t yv4 = *reinterpret_cast<const u32x4_t*>(strip + ra);
    if constexpr (RES) {
      float yv[8], xv[8], gv[8], ov[8];
      unpack8(__builtin_bit_cast(uint4, yv4), yv);
      unpack8(__builtin_bit_cast(uint4, e_res[xb & 1][i]), xv);
      unpack8(__builtin_bit_cast(uint4, e_gate4), gv);
#pragma unroll
      for (int e = 0; e < 8; ++e) ov[e] = xv[e] + rbf(yv[e] * gv[e]);
      yv4 = __builtin_bit_cast(u32x4_t, pack8(ov));
    }
    __builtin_amdgcn_raw_buffer_store_b128(yv4, r_y, row_voff(16 * xb + 4 * i), s_col + (unsigned)(16 * xb + 4 * i) * y_row, 0);
  };
  auto epilogue = [&]() {
    asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 7" ::: "memory");  // the last MFMAs' results before the accumulator reads below
    if constexpr (RES) {
      if (gate == nullptr) e_gate4 = u32x4_t{0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u};  // x + y: gate 1.0 gives the same bits (y is already bf16)
    }
    // (The walk software-pipelined by one x block — gemm256c8.hip's form: A(xb + 1) under the strip reads of block xb — was measured in round 5 and is
    //  a wash in bf16: 5120->13824 plain +1..2 %, GELU -1 %, 13824->5120 +0.8 %, K = 1536 inside the noise; profiles/r05_call1_*.  Not kept.)
    static_for<0, 8>([&](auto xbc) {
      constexpr int xb = decltype(xbc)::value;
      if constexpr (RES && xb < 7) {  // the next x block's residual chunks fly under this block's arithmetic
        static_for<0, 4>([&](auto ic) { res_load(std::integral_constant<int, xb + 1>{}, ic); });
      }
      static_for<0, 8>([&](auto wbc) { epi_phase_a(std::integral_constant<int, xb * 8 + decltype(wbc)::value>{}); });
      __builtin_amdgcn_sched_barrier(0);  // one x block at a time: left alone, the scheduler hoists the unpacking of every operand and spills
      static_for<0, 4>([&](auto ic) { epi_phase_b(xbc, ic); });
      __builtin_amdgcn_sched_barrier(0);
    });
  };

  // what slot n of a K tile multiplies: every slot holds an MFMA
#define C_MFMA(N_, FIRST_)                                                                      \
  {                                                                                             \
    constexpr int ks = (N_) >> 6, xb = ((N_) >> 3) & 7, wb = (N_) & 7;                          \
    if constexpr ((FIRST_) && ks == 0) mfma_bf16_first<xb * 8 + wb>(fw[ks][wb], fx[ks][xb]);    \
    else mfma_bf16<xb * 8 + wb>(fw[ks][wb], fx[ks][xb]);                                        \
  }
  X2V_PIPE_CONTINUOUS(C_MFMA, X2V_PIPE_BF16_READ)
#undef C_MFMA
#endif
}

template <int EPI>
static int launch_gemm256c(const void* x, int64_t ldx_bytes, const void* w, int64_t ldw_bytes, const void* bias, void* y, int64_t ldy, int64_t M, int N, int nk,
                           const void* resid, int64_t ldr, const void* gate, int gm_tiles, hipStream_t st, GemmBlocking gb) {
  if (gm_tiles <= 0) gm_tiles = 4;
  const int ntm = (int)((M + TILE - 1) / TILE), ntn = (N + TILE - 1) / TILE;
  int rc = ensure_dynamic_lds((const void*)gemm256c_kernel<EPI>, C_LDS_TOTAL, "gemm256c attr");
  if (rc != X2V_OK) return rc;
  hipLaunchKernelGGL((gemm256c_kernel<EPI>), dim3(persistent_grid((unsigned)ntm * (unsigned)ntn)), dim3(256), C_LDS_TOTAL, st, (const char*)x, ldx_bytes, (const char*)w, ldw_bytes, (const unsigned short*)bias,
                     (unsigned short*)y, ldy, M, N, nk, (const unsigned short*)resid, ldr, (const unsigned short*)gate, ntm, ntn, gm_tiles, gb);
  X2V_LAUNCH_CHECK("gemm256c launch");
  return X2V_OK;
}

// Called by gemm.hip's dispatcher, which also decides which shapes take this kernel (continuous_ok there).
int gemm256c_dispatch(int epilogue, const void* x, int64_t ldxb, const void* w, int64_t ldwb, const void* bias, void* y, int64_t ldy, int64_t M, int N, int nk,
                      const void* resid, int64_t ldr, const void* gate, int gm_tiles, hipStream_t st, GemmBlocking gb) {
  return with_epilogue("gemm", epilogue, resid, ldr, gate, gb, [&](auto epi, const void* r, int64_t lr, const void* g) {
    return launch_gemm256c<decltype(epi)::value>(x, ldxb, w, ldwb, bias, y, ldy, M, N, nk, r, lr, g, gm_tiles, st, gb);
  });
}

}  // namespace x2v
