// y[M,N] = epi((xq[M,K] . Wq[N,K]^T) * sx[m] * sw[n] + bias), e4m3 or int8 operands with per-token / per-channel fp32 scales (w8a8) — gemm256c.hip's
// CONTINUOUS single-stream pipeline for the two w8a8 operators: ONE kernel, gemm256c8_kernel<EPI, I8> (the name follows gemm_kernel<FP8, EPI, I8>).
// The text below describes the e4m3 form (I8 = false); "What int8 changes" lists the three places where I8 = true differs.  Same contract, operand layouts, epilogues, rounding points, MFMA (v_mfma_scale_f32_32x32x64_f8f6f4 with
// unit block scales) and k order as the fp8 instantiation of gemm256.hip: bit-equal results (tools/gemm_fp8_continuous_check.py,
// tests/test_gpu_bench_shapes.py::test_gemm_fp8_continuous_pipeline_equals_ping_pong).
// Replaces the cutlass_scaled_mm / fp8_scaled_mm call of common/ops/mm/mm_weight.py:287-319 at the large shapes, behind x2v_gemm_fp8[_variant|_blocked].
//
// Bound: MFMA (fp8 dense peak ~5 PFLOP/s; at the board's 1400 W limit a bare 32x32x64 loop with this LDS fragment traffic sustains ~3.9 PFLOP/s,
// profiles/r02_mfma_power_probe.log PROBE_SET=2).  Algorithmic work 2*M*N*K FLOP per launch.
//
// Why: gemm256.hip's two-groups-of-four-waves ping-pong reaches 2.6-2.85 PFLOP/s in the w8a8 step, 68-73 % of what the
// chip sustains for this instruction mix; its prologue and epilogue (dequantise -> LDS -> barrier -> stores) are un-overlapped and weigh twice what
// they weigh in bf16 because an fp8 K tile (128 k) takes the time of a bf16 one (64 k).  The bf16 answer (gemm256s -> gemm256c) carries over because
// the BYTES are the same: a K tile is one 128-byte line per operand row either way, so the LDS images, the LDS-DMA pieces, the cursors that run on into
// the next output tile, the slot plan and the pipeline itself are shared with gemm256c.hip (gemm256_pipe.h); what this file holds is
//   * the matrix instruction: a wave's 128 x 128 part = 4 x 4 accumulator tiles of 32 x 32 (16 AGPRs each); a K tile = 2 k-steps of 16 MFMAs of 16
//     passes (2048 matrix cycles, as in bf16), so the 128 "slots" of gemm256c's plan become 4 instruction positions behind each of the 32 MFMAs;
//   * fragments: 32 bytes per lane (row fl = lane & 31 of a 32-row block, 16-byte chunks 4 s + fh and 4 s + 2 + fh of k-step s: the instruction's own
//     k order, as gemm256.hip) = two ds_read_b128 into the halves of an 8-register operand; 16 reads per k-step, the same count as bf16;
//   * the epilogue dequantises in the accumulator layout (value * sx[row] * sw[col] + bias, then the activation, then bf16 — gemm256.hip's order) and
//     transposes through the wave's private 4 KiB strip in half-blocks of 32 rows x 64 columns: 8-byte pieces in, 16-byte row-major pieces out (8 rows
//     x 128 contiguous bytes = whole lines per store instruction).  The walk is column-half-major so that only one half's per-column operands (8 x float4
//     scales + 8 x 4 bf16 bias) have to be requested while the fragment registers are still in use: the first half's ride in the LAST K tile's slots, the second half's
//     are requested when the epilogue starts and arrive under the first half's work.
// Shapes: as gemm256c (even number of K tiles >= 4, N a multiple of 256, y blocks multiples of 128 columns, residual with y's row stride); the rest
// stays on gemm256.hip.  First contact on MI355X (profiles/r04_call16_*): 84 / 84 equality cases bit-equal, +2..5 % plain, +1.5..2.5 % GELU, +4..10 %
// residual at the w8a8 step's shapes (2.55-2.87 PFLOP/s).  The dispatcher's default for row-major operands; block-strided operands (Ulysses buffers) keep
// the ping-pong kernel until that path has met a GPU (X2V_GEMM_FP8_CONTINUOUS=2; =0: never).  Variant 5 of x2v_gemm_fp8_variant forces this kernel.
//
// What int8 changes (I8 = true: the reference's W-int8-channel-sym-A-int8-channel-sym-dynamic-* classes, mm_weight.py:322-354).  An int8 K tile is the
// same 128-byte line per operand row as an e4m3 one, so the fragment reads, the epilogue's addressing, operand loads, statements and walk, the constants
// below and the launch are the e4m3 form's own text.  What differs:
//   * the matrix instruction: v_mfma_i32_32x32x32_i8, 16 operand bytes per lane.  Each e4m3 MFMA (32 operand bytes per lane = the two ds_read_b128
//     halves e = 0, 1 of a fragment) becomes TWO int8 MFMAs, one per half, in the slots 4 m and 4 m + 2 of the plan: 64 MFMAs per K tile, one in
//     every even slot, 32 fragment reads as before.  Both operands take the same half, i.e. the same (lane half, byte) -> k map, which is all the
//     instruction requires; the order in which the k values are summed is free because the int32 sum is exact (K <= 65536: |acc| < 2^31).
//     Every fragment is consumed in the slot window in which the e4m3 form consumes it, so the plan's read-before-use and stage-free points hold as
//     they are.  The two MFMAs of a pair accumulate into the same tile back to back: an accumulate chain (D taken whole as C) needs no wait states.
//   * the epilogue reads the accumulators as int32 and converts (v_cvt_f32_i32, round to nearest even) in front of the dequantisation (acc_value).
//     The wait behind the last MFMA: the instruction is TAKEN to be 8-pass (the cycles of the bf16 32x32x16 form, half the block-scaled e4m3 one's;
//     not measured in isolation here), whose result needs 12 states before another reader.  The 24 that the 16-pass e4m3 instruction needs are
//     kept, so the reads are safe under either pass count (once per 256 x 256 output tile).  The slot plan's arithmetic (64 MFMAs in a K tile's
//     time) rests on the same assumption; measured, int8 takes 1.08-1.11x the e4m3 form's time at the w8a8 step's shapes.
//   Bit-equal with the 128x128 int8 kernel (gemm.hip, I8): same exact sum, same conversion, same epilogue statements (tests/test_gpu_int8.py).
//   Variant 5 of x2v_gemm_int8_variant forces this kernel; its shapes are the e4m3 form's (a residual row period: a multiple of 8 and >= 256).
// AUDIT after every edit (the accumulator half is invisible to the compiler): `hipcc -S` must show .vgpr_spill_count 0,
// .private_segment_fixed_size 0 and no v_accvgpr_* / a[..] operand outside ;;#ASMSTART / ;;#ASMEND (tools/isa_diff.py reports it).  Both formats'
// instruction streams are those of the two per-format files this one replaced (profiles/w8a8_one_kernel_isa.txt).
#include "gemm256_pipe.h"

namespace x2v {
namespace {
using namespace pipe;

constexpr int C8_STRIP_BYTES = 32 * 128;  // per wave: the epilogue's transposition strip, one half-block (32 rows x 64 bf16) at a time
constexpr int C8_LDS_TOTAL = LDS_BYTES + 4 * C8_STRIP_BYTES;
// sx (4) + sw of a column half (8) + bias of a column half (8) [+ gate of a column half (1) + the residual chunks of the first half-block (4)]
constexpr int C8_NX_PLAIN = 4 + 8 + 8, C8_NX_RES = C8_NX_PLAIN + 1 + 4;
static_assert(xload_slots() >= C8_NX_RES, "the LAST K tile has a position for every epilogue-operand load");
static_assert(NEWER + C8_NX_RES <= 63, "vmcnt immediate");

// accumulator tile I (= x block * 4 + W block, 32 x 32) is a[16 I : 16 I + 15].  The UNSCALED encoding v_mfma_f32_32x32x64_f8f6f4 (8 bytes; both
// operands e4m3 by its default cbsz / blgp): per-channel w8a8 has no block scales, and the scaled encoding with unit e8m0 scales (16 bytes + a
// scale register read per MFMA; what gemm256.hip's builtin emits) gives the same bits — 84 / 84 equality cases — and is 0.5-1.0 % slower at every
// shape and epilogue measured (profiles/r05_call1_*: 13824->5120 plain 2905 -> 2933 TFLOP/s).
template <int I>
__device__ __forceinline__ void c8_mfma(const i32x8_t& wf, const i32x8_t& xf) {
  asm volatile("v_mfma_f32_32x32x64_f8f6f4 a[%c2:%c3], %0, %1, a[%c2:%c3]" ::"v"(wf), "v"(xf), "i"(16 * I), "i"(16 * I + 15) : X2V_AGPRS);
}
template <int I>
__device__ __forceinline__ void c8_mfma_first(const i32x8_t& wf, const i32x8_t& xf) {  // first k-step of an output tile: C = 0
  asm volatile("v_mfma_f32_32x32x64_f8f6f4 a[%c2:%c3], %0, %1, 0" ::"v"(wf), "v"(xf), "i"(16 * I), "i"(16 * I + 15) : X2V_AGPRS);
}

// int8: the same tile as 32 x 32 int32; one MFMA per fragment half
template <int I>
__device__ __forceinline__ void ci8_mfma(const i32x4_t& wf, const i32x4_t& xf) {
  asm volatile("v_mfma_i32_32x32x32_i8 a[%c2:%c3], %0, %1, a[%c2:%c3]" ::"v"(wf), "v"(xf), "i"(16 * I), "i"(16 * I + 15) : X2V_AGPRS);
}
template <int I>
__device__ __forceinline__ void ci8_mfma_first(const i32x4_t& wf, const i32x4_t& xf) {  // first MFMA of an output tile into tile I: C = 0
  asm volatile("v_mfma_i32_32x32x32_i8 a[%c2:%c3], %0, %1, 0" ::"v"(wf), "v"(xf), "i"(16 * I), "i"(16 * I + 15) : X2V_AGPRS);
}
// accumulator register R as the float the epilogue dequantises: the e4m3 sum itself, the int32 sum converted
template <bool I8, int R>
__device__ __forceinline__ float acc_value() {
  if constexpr (I8) {
    int x;
    asm volatile("v_accvgpr_read_b32 %0, a[%c1]" : "=v"(x) : "i"(R) : X2V_AGPRS);
    return (float)x;
  } else {
    return acc_read<R>();
  }
}

template <int EPI, bool I8>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void gemm256c8_kernel(
    const char* __restrict__ A, int64_t lda_bytes, const char* __restrict__ W, int64_t ldw_bytes, const unsigned short* __restrict__ bias, unsigned short* Y,
    int64_t ldy, int64_t M, int N, int nk, const unsigned short* resid, int64_t ldr, const unsigned short* __restrict__ gate, const float* __restrict__ sx,
    const float* __restrict__ sw, int ntm, int ntn, int gm_tiles, GemmBlocking gb) {
#if defined(__HIP_DEVICE_COMPILE__)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  claim_accumulators();
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wid >> 1, wc = wid & 1;
  const int fl = lane & 31, fh = lane >> 5;
  X2V_PIPE_PERSISTENT_CHUNK()
  X2V_PIPE_COORDS()
  X2V_PIPE_OPERANDS()
  X2V_PIPE_DMA_OFFSETS()

  // ---- fragment addresses (32x32x64: row fl of a 32-row block; half e of k-step s = 16-byte chunk 4 s + 2 e + fh; int8: the 32 k values of its k-step
  //      2 s + e, 16 of them in lane half fh), block offsets travel as immediates
  int rd_x[2][2], rd_w[2][2];
  {
    const int swz = (fl >> 1) & 7;
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int o = fl * 128 + ((((s << 2) | (e << 1) | fh) ^ swz) << 4);
        rd_x[s][e] = o + OP_BYTES + wr * 16384;
        rd_w[s][e] = o + wc * 16384;
      }
  }
  // fragment halves: fx[ks][xb][e], fw[ks][wb][e]; an e4m3 MFMA operand is the 8-register pair (e = 0, 1), an int8 one a single half
  i32x4_t fx[2][4][2], fw[2][4][2];
  // read R_ in 0..15 of k-step KS_ of the tile in stage STAGE_: fragment R_ / 2 (order x0, W0..W3, x1..x3: the first MFMA of a k-step needs x0, W0), half R_ % 2
#define C8_READ(R_, STAGE_, KS_)                                                                                                                \
  {                                                                                                                                            \
    constexpr int f_ = (R_) >> 1, e_ = (R_) & 1;                                                                                               \
    if constexpr (f_ == 0) fx[KS_][0][e_] = *reinterpret_cast<const i32x4_t*>(smem + (STAGE_) * STAGE_BYTES + rd_x[KS_][e_]);                   \
    else if constexpr (f_ <= 4) fw[KS_][f_ - 1][e_] = *reinterpret_cast<const i32x4_t*>(smem + (STAGE_) * STAGE_BYTES + (f_ - 1) * 4096 + rd_w[KS_][e_]); \
    else fx[KS_][f_ - 4][e_] = *reinterpret_cast<const i32x4_t*>(smem + (STAGE_) * STAGE_BYTES + (f_ - 4) * 4096 + rd_x[KS_][e_]);              \
  }
  // what position n of a K tile multiplies: e4m3 MFMA m = n / 4 sits at n % 4 == 0 (one bf16 MFMA slot = a quarter of an fp8 one); int8 has an MFMA in
  // every even slot: slots 4 m and 4 m + 2 hold the halves e = 0, 1 of MFMA m
#define C8_MFMA(N_, FIRST_)                                                                                   \
  if constexpr (((N_) & (I8 ? 1 : 3)) == 0) {                                                                 \
    constexpr int m = (N_) >> 2, e = ((N_) >> 1) & 1, ks = m >> 4, xb = (m >> 2) & 3, wb = m & 3;             \
    if constexpr (I8) {                                                                                       \
      if constexpr ((FIRST_) && ks == 0 && e == 0) ci8_mfma_first<xb * 4 + wb>(fw[ks][wb][e], fx[ks][xb][e]); \
      else ci8_mfma<xb * 4 + wb>(fw[ks][wb][e], fx[ks][xb][e]);                                               \
    } else {                                                                                                  \
      const i32x8_t wf = __builtin_shufflevector(fw[ks][wb][0], fw[ks][wb][1], 0, 1, 2, 3, 4, 5, 6, 7);       \
      const i32x8_t xf = __builtin_shufflevector(fx[ks][xb][0], fx[ks][xb][1], 0, 1, 2, 3, 4, 5, 6, 7);       \
      if constexpr ((FIRST_) && ks == 0) c8_mfma_first<xb * 4 + wb>(wf, xf);                                  \
      else c8_mfma<xb * 4 + wb>(wf, xf);                                                                      \
    }                                                                                                         \
  }

  // ---- epilogue of the CURRENT output tile (see the header).  Half-block (ch, xb) = rows [32 xb, 32 xb + 32) x columns [64 ch, 64 ch + 64) of the
  //      wave's 128 x 128 part, walked ch-major.
  //      Phase A (accumulator layout: lane = row fl, columns 8 g + 4 fh + e of W block wb): dequantise, bias, activation, bf16; the 4 values of a
  //      (wb, g) = 8 bytes = unit u = ((wb & 1) * 4 + g) * 2 + fh of the strip row, stored at unit u ^ (fl >> 1): 32 lanes of one fh hit 64 banks once.
  //      Phase B (row-major: lane = row 8 i + (lane >> 3), 16-byte chunk c8 = lane & 7 of the 128-byte half-row): the two units of chunk c8 sit in
  //      chunk c8 ^ (row >> 2), swapped when (row >> 1) & 1; one ds_read_b128, a conditional swap, (residual), one 16-byte store — the store
  //      instruction covers 8 rows x 128 contiguous bytes.  LDS executes a wave's instructions in order, so phase A of the next half-block may
  //      overwrite the strip right behind phase B's reads.
  //      Addressing as gemm256c.hip: vector offset = lane part or the "row does not exist" mark 0x80000000, scalar offset = column base + rows.
  u32x2_t e_bias[2][8];  // [column half][j]
  f32x4_t e_sw[2][8];
  float e_sx[4];
  u32x4_t e_gate4[2], e_res[2][4];
  __amdgpu_buffer_rsrc_t r_y, r_res, r_bias, r_gate, r_sw, r_sx;
  char* const strip = smem + LDS_BYTES + wid * C8_STRIP_BYTES;
  const int l8 = lane >> 3, c8 = lane & 7;
  const unsigned lane_off = (unsigned)((wr * 128 + l8) * ldy * 2) + (unsigned)(16 * c8);  // phase B: bytes from the tile's first row / the half-block's first column
  const int wa0 = fl * 128 + ((fh ^ ((fl >> 1) & 15)) << 3);                                // phase A: unit fh ^ (fl >> 1) of row fl
  const int rb0 = l8 * 128 + ((c8 ^ (l8 >> 2)) << 4);                                       // phase B: chunk c8 ^ (row >> 2) of row l8 (+ 8 i rows: ^ (i << 5), + 1024 i)
  const bool swap_b = ((l8 >> 1) & 1) != 0;
  unsigned s_col = 0u;   // the wave's first column in the output / residual row, bytes (wave-uniform)
  unsigned s_bias = 0u;  // the wave's first column in bias / gate (bf16), bytes; scales (fp32): twice that
  int rows_left = 0;     // valid rows of the current tile below row wr*128 + (lane>>3): phase-B row 32 xb + 8 i of the lane exists iff it is < rows_left
  const unsigned y_row = (unsigned)(ldy * 2);  // one row of y (and of the residual: ldr == ldy, y row-major — dispatcher), bytes
  constexpr bool RES = epi_is_residual(EPI);
  constexpr bool RP = EPI == EPI_RESIDUAL_PERIODIC;  // output row r combines with residual row r mod gb.r_period (as gemm256c.hip; chunks of 8 rows here)
  const unsigned lane_off_r = (unsigned)(l8 * ldy * 2) + (unsigned)(16 * c8);
  unsigned s_rrow = 0u;  // RP: residual row of the wave's first row of the current tile (wave-uniform)
  constexpr int NXLOAD = RES ? C8_NX_RES : C8_NX_PLAIN;

  auto epilogue_setup = [&](int tm, int tn) {
    const int64_t m0 = (int64_t)tm * TILE;
    const int gn0 = tn * TILE + wc * 128;  // first column of this wave (wave-uniform)
    r_y = __builtin_amdgcn_make_buffer_rsrc((void*)(Y + m0 * ldy), 0, 0x80000000u, 0x00020000);
    r_bias = __builtin_amdgcn_make_buffer_rsrc((void*)bias, 0, bias != nullptr ? (unsigned)N * 2u : 0u, 0x00020000);
    r_sw = __builtin_amdgcn_make_buffer_rsrc((void*)sw, 0, (unsigned)N * 4u, 0x00020000);
    // rows past M read scale 0: their results are never stored
    r_sx = __builtin_amdgcn_make_buffer_rsrc((void*)(sx + m0 + wr * 128), 0, (unsigned)(max((int64_t)0, min((int64_t)128, M - m0 - wr * 128)) * 4), 0x00020000);
    unsigned col = (unsigned)gn0;
    if (gb.y_cbw > 0) {  // N-blocked y: column n at (n / y_cbw) * y_cbs + n % y_cbw elements from the row's start
      const unsigned qb = (unsigned)gn0 / (unsigned)gb.y_cbw;
      col = qb * (unsigned)gb.y_cbs + ((unsigned)gn0 - qb * (unsigned)gb.y_cbw);
    }
    s_col = col * 2u;
    s_bias = (unsigned)gn0 * 2u;
    rows_left = (int)min((int64_t)TILE, M - m0) - wr * 128 - l8;
    if constexpr (RP) {
      r_res = __builtin_amdgcn_make_buffer_rsrc((void*)resid, 0, 0x80000000u, 0x00020000);
      s_rrow = resid_tile_row(m0 + wr * 128, gb.r_period);
      r_gate = __builtin_amdgcn_make_buffer_rsrc((void*)gate, 0, gate != nullptr ? (unsigned)N * 2u : 0u, 0x00020000);
    } else if constexpr (RES) {
      r_res = __builtin_amdgcn_make_buffer_rsrc((void*)(resid + m0 * ldy), 0, 0x80000000u, 0x00020000);
      r_gate = __builtin_amdgcn_make_buffer_rsrc((void*)gate, 0, gate != nullptr ? (unsigned)N * 2u : 0u, 0x00020000);
    }
  };
  auto row_voff = [&](int row8) { return row8 < rows_left ? lane_off : 0x80000000u; };  // phase-B vector offset of local row `row8` (= 32 xb + 8 i)
  // half-block hb = 4 ch + xb in walk order; residual chunk i of it: the 16 bytes phase B's store i of that half-block will overwrite
  auto res_load = [&](auto hbc, auto ic) {
    constexpr int hb = decltype(hbc)::value, ch = hb >> 2, xb = hb & 3, i = decltype(ic)::value;
    if constexpr (RP)  // the chunk's 8 rows lie on one side of the period (gemm256_pipe.h: resid_chunk_row)
      e_res[hb & 1][i] = __builtin_bit_cast(u32x4_t, __builtin_amdgcn_raw_buffer_load_b128(r_res, 32 * xb + 8 * i < rows_left ? lane_off_r : 0x80000000u,
                                                                                           s_col + (unsigned)(ch * 128) + resid_chunk_row(s_rrow, 32 * xb + 8 * i, gb.r_period) * y_row, 0));
    else
    e_res[hb & 1][i] = __builtin_bit_cast(u32x4_t, __builtin_amdgcn_raw_buffer_load_b128(r_res, row_voff(32 * xb + 8 * i), s_col + (unsigned)(ch * 128) + (unsigned)(32 * xb + 8 * i) * y_row, 0));
  };
  // per-column operands of column half ch: scales and bias in phase-A layout (tile wb = 2 ch + (j >> 2), g = j & 3: columns 32 wb + 8 g + 4 fh ..+3)
  auto sw_load = [&](auto chc, auto jc) {
    constexpr int ch = decltype(chc)::value, j = decltype(jc)::value;
    e_sw[ch][j] = __builtin_bit_cast(f32x4_t, __builtin_amdgcn_raw_buffer_load_b128(r_sw, (unsigned)(16 * fh), 2u * s_bias + (unsigned)((ch * 64 + j * 8) * 4), 0));
  };
  auto bias_load = [&](auto chc, auto jc) {
    constexpr int ch = decltype(chc)::value, j = decltype(jc)::value;
    e_bias[ch][j] = __builtin_bit_cast(u32x2_t, __builtin_amdgcn_raw_buffer_load_b64(r_bias, (unsigned)(8 * fh), s_bias + (unsigned)((ch * 64 + j * 8) * 2), 0));
  };
  auto gate_load = [&](auto chc) {
    constexpr int ch = decltype(chc)::value;
    e_gate4[ch] = __builtin_bit_cast(u32x4_t, __builtin_amdgcn_raw_buffer_load_b128(r_gate, (unsigned)(16 * c8), s_bias + (unsigned)(ch * 128), 0));
  };
  // epilogue-operand load J of the current output tile (LAST K tile): sx, then column half 0's scales and bias, [gate half 0, residual of half-block 0]
  auto xload = [&](auto jc) {
    constexpr int J = decltype(jc)::value;
    if constexpr (J < 4) {
      e_sx[J] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r_sx, (unsigned)(4 * fl), (unsigned)(J * 128), 0));
    } else if constexpr (J < 12) {
      sw_load(k0{}, std::integral_constant<int, J - 4>{});
    } else if constexpr (J < 20) {
      bias_load(k0{}, std::integral_constant<int, J - 12>{});
    } else if constexpr (RES && J == 20) {
      gate_load(k0{});
    } else if constexpr (RES && J < C8_NX_RES) {
      res_load(k0{}, std::integral_constant<int, J - 21>{});
    }
  };

  // Phase A of accumulator tile I = 4 xb + wb: value 4 g + e of the lane = row 32 xb + fl, column 32 wb + 8 g + 4 fh + e of the wave's part
  auto epi_phase_a = [&](auto ic) {
    constexpr int I = decltype(ic)::value, xb = I >> 2, wb = I & 3, ch = wb >> 1;
    static_for<0, 4>([&](auto gc) {
      constexpr int g = decltype(gc)::value, j = (wb & 1) * 4 + g;
      float vv[4] = {acc_value<I8, 16 * I + 4 * g + 0>(), acc_value<I8, 16 * I + 4 * g + 1>(), acc_value<I8, 16 * I + 4 * g + 2>(), acc_value<I8, 16 * I + 4 * g + 3>()};
      // gemm256.hip's statements, in its order
      vv[0] = vv[0] * e_sx[xb] * e_sw[ch][j].x;
      vv[1] = vv[1] * e_sx[xb] * e_sw[ch][j].y;
      vv[2] = vv[2] * e_sx[xb] * e_sw[ch][j].z;
      vv[3] = vv[3] * e_sx[xb] * e_sw[ch][j].w;
      epi_bias_act4<EPI>(vv, e_bias[ch][j].x, e_bias[ch][j].y);
      *reinterpret_cast<u32x2_t*>(strip + (wa0 ^ (j << 4))) = u32x2_t{pack_bf2(vv[0], vv[1]), pack_bf2(vv[2], vv[3])};
    });
  };
  // Phase B, instruction i of half-block hb: local rows 32 xb + 8 i + (lane >> 3), the lane's 8 columns 64 ch + 8 (lane & 7)..: strip -> (residual) -> memory.
  // The four strip reads of a half-block are issued back to back (one LDS latency per half-block, not four), then combined and stored.
  u32x4_t e_raw[4];
  auto epi_read_b = [&](auto ic) {
    constexpr int i = decltype(ic)::value;
    e_raw[i] = *reinterpret_cast<const u32x4_t*>(strip + ((rb0 ^ (i << 5)) + i * 1024));
  };
  auto epi_phase_b = [&](auto hbc, auto ic) {
    constexpr int hb = decltype(hbc)::value, ch = hb >> 2, xb = hb & 3, i = decltype(ic)::value;
    const u32x4_t raw = e_raw[i];
    u32x4_t yv4 = swap_b ? u32x4_t{raw.z, raw.w, raw.x, raw.y} : raw;
    if constexpr (RES) {
      float yv[8], xv[8], gv[8], ov[8];
      unpack8(__builtin_bit_cast(uint4, yv4), yv);
      unpack8(__builtin_bit_cast(uint4, e_res[hb & 1][i]), xv);
      unpack8(__builtin_bit_cast(uint4, e_gate4[ch]), gv);
#pragma unroll
      for (int e = 0; e < 8; ++e) ov[e] = xv[e] + rbf(yv[e] * gv[e]);
      yv4 = __builtin_bit_cast(u32x4_t, pack8(ov));
    }
    __builtin_amdgcn_raw_buffer_store_b128(yv4, r_y, row_voff(32 * xb + 8 * i), s_col + (unsigned)(ch * 128) + (unsigned)(32 * xb + 8 * i) * y_row, 0);
  };
  // Walk order (software-pipelined by one half-block so that no LDS round trip is waited for): A(0) R(0) | A(1) B(0) R(1) | .. | A(7) B(6) R(7) | B(7),
  // A = phase A (accumulators -> strip), R = the four strip reads, B = combine + store.  R(hb - 1) is in flight while A(hb) overwrites the strip: LDS
  // executes a wave's instructions in order, so the reads return the old contents.
  auto epilogue = [&]() {
    // column half 1's operands fly under half 0's four half-blocks (the fragment registers are free here)
    static_for<0, 8>([&](auto jc) { sw_load(k1{}, jc); });
    static_for<0, 8>([&](auto jc) { bias_load(k1{}, jc); });
    if constexpr (RES) {
      if (gate != nullptr) {
        gate_load(k1{});
      } else {  // x + y: gate 1.0 gives the same bits (y is already bf16)
        e_gate4[0] = u32x4_t{0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u};
        e_gate4[1] = e_gate4[0];
      }
    }
    asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 7" ::: "memory");  // the last MFMAs' results before the accumulator reads below
    __builtin_amdgcn_sched_barrier(0);
    static_for<0, 9>([&](auto hbc) {
      constexpr int hb = decltype(hbc)::value;
      if constexpr (hb < 8) {
        constexpr int ch = hb >> 2, xb = hb & 3;
        static_for<0, 2>([&](auto wc2) { epi_phase_a(std::integral_constant<int, xb * 4 + ch * 2 + decltype(wc2)::value>{}); });
        __builtin_amdgcn_sched_barrier(0);  // one half-block at a time: left alone, the scheduler hoists the unpacking of every operand and spills
      }
      if constexpr (hb > 0) {
        static_for<0, 4>([&](auto ic) { epi_phase_b(std::integral_constant<int, hb - 1>{}, ic); });
        __builtin_amdgcn_sched_barrier(0);
      }
      if constexpr (hb < 8) {
        if constexpr (RES && hb < 7) {  // the next half-block's residual chunks (their buffer was last read by B(hb - 1) above)
          static_for<0, 4>([&](auto ic) { res_load(std::integral_constant<int, hb + 1>{}, ic); });
        }
        static_for<0, 4>([&](auto ic) { epi_read_b(ic); });
        __builtin_amdgcn_sched_barrier(0);
      }
    });
  };

  X2V_PIPE_CONTINUOUS(C8_MFMA, C8_READ)
#undef C8_MFMA
#undef C8_READ
#endif
}

template <int EPI, bool I8>
int launch_gemm256c8(const void* x, int64_t ldx_bytes, const void* w, int64_t ldw_bytes, const void* bias, void* y, int64_t ldy, int64_t M, int N, int nk,
                     const void* resid, int64_t ldr, const void* gate, const float* sx, const float* sw, int gm_tiles, hipStream_t st, GemmBlocking gb) {
  if (gm_tiles <= 0) gm_tiles = 4;
  const int ntm = (int)((M + TILE - 1) / TILE), ntn = (N + TILE - 1) / TILE;
  int rc = ensure_dynamic_lds((const void*)gemm256c8_kernel<EPI, I8>, C8_LDS_TOTAL, I8 ? "gemm256ci8 attr" : "gemm256c8 attr");
  if (rc != X2V_OK) return rc;
  hipLaunchKernelGGL((gemm256c8_kernel<EPI, I8>), dim3(persistent_grid((unsigned)ntm * (unsigned)ntn)), dim3(256), C8_LDS_TOTAL, st, (const char*)x, ldx_bytes, (const char*)w, ldw_bytes, (const unsigned short*)bias,
                     (unsigned short*)y, ldy, M, N, nk, (const unsigned short*)resid, ldr, (const unsigned short*)gate, sx, sw, ntm, ntn, gm_tiles, gb);
  X2V_LAUNCH_CHECK(I8 ? "gemm256ci8 launch" : "gemm256c8 launch");
  return X2V_OK;
}

}  // namespace

// Called by gemm.hip's dispatchers (dispatch_epi<true>, dispatch_int8), which also decide which shapes take this kernel (continuous_ok there).
int gemm256c8_dispatch(int epilogue, const void* x, int64_t ldxb, const void* w, int64_t ldwb, const void* bias, void* y, int64_t ldy, int64_t M, int N, int nk,
                       const void* resid, int64_t ldr, const void* gate, const float* sx, const float* sw, int gm_tiles, hipStream_t st, GemmBlocking gb) {
  return with_epilogue("gemm_fp8", epilogue, resid, ldr, gate, gb, [&](auto epi, const void* r, int64_t lr, const void* g) {
    return launch_gemm256c8<decltype(epi)::value, false>(x, ldxb, w, ldwb, bias, y, ldy, M, N, nk, r, lr, g, sx, sw, gm_tiles, st, gb);
  });
}
int gemm256ci8_dispatch(int epilogue, const void* x, int64_t ldxb, const void* w, int64_t ldwb, const void* bias, void* y, int64_t ldy, int64_t M, int N, int nk,
                        const void* resid, int64_t ldr, const void* gate, const float* sx, const float* sw, int gm_tiles, hipStream_t st, GemmBlocking gb) {
  return with_epilogue("gemm_int8", epilogue, resid, ldr, gate, gb, [&](auto epi, const void* r, int64_t lr, const void* g) {
    return launch_gemm256c8<decltype(epi)::value, true>(x, ldxb, w, ldwb, bias, y, ldy, M, N, nk, r, lr, g, sx, sw, gm_tiles, st, gb);
  });
}

}  // namespace x2v
