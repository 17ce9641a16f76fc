// What the GEMM sources share: host side the dispatch entries, the epilogue switch and the persistent grid rule (gemm.hip, gemm256.hip and the
// three files below); device side the single-stream pipeline of gemm256s.hip (one output tile per workgroup), gemm256c.hip (continuous, bf16) and gemm256c8.hip (continuous, e4m3 and int8):
// accumulator-register access, the slot plan of a K tile, the LDS images, the tile schedule, the LDS-DMA pieces, the bf16 fragments, and the K-tile
// slot stream + output-tile loop of the two continuous kernels.  A change to the plan is made HERE, once; the kernels keep what really differs
// (matrix instruction, fragments, epilogue).
// The kernels' instruction streams are those of the per-file copies this header replaced (tools/isa_diff.py, profiles/gemm256_refactor_isa.txt).
#pragma once
#include <type_traits>

#include "mx_format.h"
#include "x2v_common.h"

namespace x2v {

// ---- dispatch entries (arguments validated by gemm.hip's / mx.hip's callers; ld*_bytes < 16 MiB and the 32-bit tile spans checked there) ----------
// gemm256.hip: the 256x256-tile ping-pong kernel for large shapes
template <bool FP8>
int gemm256_dispatch(int epilogue, const void* x, int64_t ldxb, const void* w, int64_t ldwb, const void* bias, void* y, int64_t ldy, int64_t M, int N, int nk,
                     const void* resid, int64_t ldr, const void* gate, const float* sx, const float* sw, int gm_tiles, hipStream_t st, GemmBlocking gb);
// gemm256s.hip: the same tile as one software-pipelined wave per SIMD (bf16), and its V^T-producing form
int gemm256s_dispatch(int epilogue, const void* x, int64_t ldxb, const void* w, int64_t ldwb, const void* bias, void* y, int64_t ldy, int64_t M, int N, int nk,
                      const void* resid, int64_t ldr, const void* gate, int gm_tiles, hipStream_t st, GemmBlocking gb);
int gemm256s_vt_dispatch(const void* x, int64_t ldxb, const void* w, int64_t ldwb, const void* bias, void* vt, int64_t ldvt, int64_t M, int N, int nk, hipStream_t st);
// gemm256c.hip: the single-stream kernel as a continuous pipeline over output tiles (persistent workgroups, register-direct epilogue)
int gemm256c_dispatch(int epilogue, const void* x, int64_t ldxb, const void* w, int64_t ldwb, const void* bias, void* y, int64_t ldy, int64_t M, int N, int nk,
                      const void* resid, int64_t ldr, const void* gate, int gm_tiles, hipStream_t st, GemmBlocking gb);
// gemm256c8.hip: the same continuous pipeline for the w8a8 operator (e4m3 operands, per-token / per-channel scales)
int gemm256c8_dispatch(int epilogue, const void* x, int64_t ldxb, const void* w, int64_t ldwb, const void* bias, void* y, int64_t ldy, int64_t M, int N, int nk,
                       const void* resid, int64_t ldr, const void* gate, const float* sx, const float* sw, int gm_tiles, hipStream_t st, GemmBlocking gb);
// gemm256c8.hip, I8 form: the same kernel for the w8a8 int8 operator (v_mfma_i32_32x32x32_i8, int32 accumulators)
int gemm256ci8_dispatch(int epilogue, const void* x, int64_t ldxb, const void* w, int64_t ldwb, const void* bias, void* y, int64_t ldy, int64_t M, int N, int nk,
                        const void* resid, int64_t ldr, const void* gate, const float* sx, const float* sw, int gm_tiles, hipStream_t st, GemmBlocking gb);
// The MX modes (mx.hip; f.mxm picks the kernels' MXM): a, b = rows of f.bits_a / f.bits_b-bit codes, lda / ldb in bytes, sa / sb = e8m0 block-scale
// tables [K/128][rows][4], alpha = device pointer or null, nk = K / f.k_tile.  gemm.hip: the 128x128-tile kernel (small shapes, no fused epilogue);
// gemm256.hip: the ping-pong kernel (shapes that fill the chip, and every fused epilogue)
int gemm128_mx_dispatch(const MxFormat& f, const void* a, int64_t lda, const void* sa, const void* b, int64_t ldb, const void* sb, const void* bias,
                        const float* alpha, void* y, int64_t ldy, int64_t M, int N, int nk, hipStream_t st);
int gemm256_mx_dispatch(const MxFormat& f, int epilogue, const void* a, int64_t lda, const void* sa, const void* b, int64_t ldb, const void* sb, const void* bias,
                        const float* alpha, void* y, int64_t ldy, int64_t M, int N, int nk, const void* resid, int64_t ldr, const void* gate, hipStream_t st);

// ---- host: run-time epilogue -> template argument.  f(integral_constant<int, EPI>, resid, ldr, gate); the non-residual epilogues get no residual.
template <class F>
int with_epilogue(const char* who, int epilogue, const void* resid, int64_t ldr, const void* gate, F&& f) {
  switch (epilogue) {
    case X2V_EPI_NONE: return f(std::integral_constant<int, X2V_EPI_NONE>{}, nullptr, 0, nullptr);
    case X2V_EPI_GELU_TANH: return f(std::integral_constant<int, X2V_EPI_GELU_TANH>{}, nullptr, 0, nullptr);
    case X2V_EPI_SILU: return f(std::integral_constant<int, X2V_EPI_SILU>{}, nullptr, 0, nullptr);
    case X2V_EPI_RESIDUAL: return f(std::integral_constant<int, X2V_EPI_RESIDUAL>{}, resid, ldr, gate);
    default: set_error("%s: unknown epilogue %d", who, epilogue); return X2V_E_ARG;
  }
}
// the same for the kernels that take a residual row period (GemmBlocking::r_period > 0: the EPI_RESIDUAL_PERIODIC instantiation)
template <class F>
int with_epilogue(const char* who, int epilogue, const void* resid, int64_t ldr, const void* gate, const GemmBlocking& gb, F&& f) {
  if (epilogue == X2V_EPI_RESIDUAL && gb.r_period > 0) return f(std::integral_constant<int, EPI_RESIDUAL_PERIODIC>{}, resid, ldr, gate);
  return with_epilogue(who, epilogue, resid, ldr, gate, f);
}

// ---- residual row period, device side (EPI_RESIDUAL_PERIODIC; the caller guarantees M < 2^31 and that resid's period rows do not overlap y).
//      The residual is addressed from ITS first row (not from the tile's, as the plain epilogue does): the residual row of a tile's first row
//      once per tile, then per access either the row of any local row (the kernels that load one row per lane) ..
__device__ __forceinline__ unsigned resid_tile_row(int64_t m0, int period) { return (unsigned)m0 % (unsigned)period; }
__device__ __forceinline__ unsigned resid_row(unsigned tile_row, int local, int period) { return (tile_row + (unsigned)local) % (unsigned)period; }
//      .. or, in the continuous kernels, the first row of a chunk of CH rows that one load instruction covers (wave-uniform: a scalar add, compare
//      and select).  Tiles, wave parts and chunks start at multiples of CH and the period is a multiple of CH (dispatcher: resid_period_continuous_ok),
//      so a chunk never straddles the period; the period is >= 256, so `base` (< period) + a local row (< 128) wraps at most once.
__device__ __forceinline__ unsigned resid_chunk_row(unsigned base, int local, int period) {
  const unsigned r = base + (unsigned)local;
  return r >= (unsigned)period ? r - (unsigned)period : r;
}

// ---- host: grid of a persistent kernel = one workgroup per CU, CUs rounded down to whole XCD octets (the kernels' chunking counts on it), or one
//      workgroup per output tile when there are fewer tiles than that
inline unsigned persistent_grid(unsigned nblk) {
  static const int cus = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 8) n = 256;
    return n & ~7;
  }();
  return nblk > (unsigned)cus ? (unsigned)cus : nblk;
}

namespace pipe {

constexpr int TILE = 256;                    // output tile: TILE x TILE, four waves of 128 x 128 (2 x 2), one per SIMD
constexpr int OP_BYTES = 256 * 128;          // one operand tile of one stage: [256 rows][128 B], 16-byte chunk c of row r at chunk c ^ ((r >> 1) & 7)
constexpr int STAGE_BYTES = 2 * OP_BYTES;    // W tile | x tile
constexpr int LDS_BYTES = 2 * STAGE_BYTES;   // 131072: the two stages

// ---- slot plan.  A K tile (one 128-byte line per operand row: 64 bf16 / 128 e4m3 k values) is 128 instruction positions ("slots") per wave = 2048
//      matrix cycles: 128 MFMAs of 16x16x32 bf16, or 32 of 32x32x64 e4m3 with three empty positions behind each.  Per K tile t (stage t & 1):
//   LATE0 + STEP i      the last 16 - EARLY LDS-DMA pieces of tile t+1                0, 2, .., 30   fragment reads of k-step 1
//   FREE                lgkmcnt(0) + barrier "this tile's stage is free"
//   FREE + 1 + STEP i   the first EARLY pieces of tile t+2 into this tile's stage
//   READY               vmcnt + barrier "tile t+1 has landed"                         READY + 2, + 4, ..   fragment reads of k-step 0 of t+1
//   (continuous kernels, LAST K tile of an output tile) one epilogue-operand buffer load in each slot of [X0, READY) that holds no piece
// The 64 pieces a workgroup moves per tile keep the CU's texture path busy for half of the tile's 2048 cycles: issued in a burst (all four waves
// right behind the first barrier) they queue up and stall the issuing waves; spread over the tile they cost ~nothing.
// (Round 6, profiles/r06_gemm_vs_hipblaslt_pmc_and_knockouts.txt: pieces every 5 / 6 slots, READY at 106 with a read per slot, k-step-1 reads a slot
//  apart, FREE at 44 and a W-major k-step order are all nil or slower at the step's shapes; builds without the vmcnt / lgkmcnt waits — invalid
//  results — gain 0.1-0.6 %: the plan is at its optimum.)
constexpr int STEP = 7, FREE = 36, READY = 94, LATE0 = 3;
constexpr int EARLY = (127 - FREE - 1) / STEP + 1 < 16 ? (127 - FREE - 1) / STEP + 1 : 16;              // pieces of tile t+2 that fit behind FREE
constexpr int NEWER = (READY - FREE - 1) / STEP + 1 < EARLY ? (READY - FREE - 1) / STEP + 1 : EARLY;  // of them issued before READY
static_assert(LATE0 + (16 - EARLY - 1) * STEP < FREE && READY + 2 + 30 <= 127, "slot plan");
// fragments of k-step 1 are last read at slot 30 and the stage is declared free at FREE: every ds_read of the tile is issued before the barrier
static_assert(30 < FREE, "slot plan: fragment reads before the stage is freed");
constexpr int X0 = FREE + 2;  // first slot that may carry an epilogue-operand load
constexpr bool late_slot(int n) { return n >= LATE0 && (n - LATE0) % STEP == 0 && (n - LATE0) / STEP < 16 - EARLY; }  // a piece of tile t+1
constexpr bool dma_slot(int n) { return n > FREE && (n - FREE - 1) % STEP == 0 && (n - FREE - 1) / STEP < EARLY; }     // a piece of tile t+2
constexpr int xload_index(int n) {  // which epilogue-operand load sits in slot n (-1: none)
  if (n < X0 || n >= READY || dma_slot(n)) return -1;
  int idx = 0;
  for (int s = X0; s < n; ++s)
    if (!dma_slot(s)) ++idx;
  return idx;
}
constexpr int xload_slots() {
  int c = 0;
  for (int s = X0; s < READY; ++s)
    if (!dma_slot(s)) ++c;
  return c;
}

typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));

// ---- accumulators: the whole accumulator half of the register file (a[0:255]), addressed by literal register number from asm statements only.
// Every asm statement that touches it names ALL of it as clobbered: hipcc must never park a value of its own in an AGPR across one of them.
// (Round 3: with only a0 / a255 named once at kernel entry, the register allocator put part of the hoisted residual chunks into a1..a8 —
// `v_accvgpr_write` outside the asm blocks — and two accumulator tiles per wave were overwritten: the kernels' AUDIT rule exists for exactly this.)
#define X2V_AGPRS "a0", "a1", "a2", "a3", "a4", "a5", "a6", "a7", "a8", "a9", "a10", "a11", "a12", "a13", "a14", "a15", "a16", "a17", "a18", "a19", "a20", "a21", "a22", "a23", "a24", "a25", "a26", "a27", "a28", "a29", "a30", "a31", "a32", "a33", "a34", "a35", "a36", "a37", "a38", "a39", "a40", "a41", "a42", "a43", "a44", "a45", "a46", "a47", "a48", "a49", "a50", "a51", "a52", "a53", "a54", "a55", "a56", "a57", "a58", "a59", "a60", "a61", "a62", "a63", "a64", "a65", "a66", "a67", "a68", "a69", "a70", "a71", "a72", "a73", "a74", "a75", "a76", "a77", "a78", "a79", "a80", "a81", "a82", "a83", "a84", "a85", "a86", "a87", "a88", "a89", "a90", "a91", "a92", "a93", "a94", "a95", "a96", "a97", "a98", "a99", "a100", "a101", "a102", "a103", "a104", "a105", "a106", "a107", "a108", "a109", "a110", "a111", "a112", "a113", "a114", "a115", "a116", "a117", "a118", "a119", "a120", "a121", "a122", "a123", "a124", "a125", "a126", "a127", "a128", "a129", "a130", "a131", "a132", "a133", "a134", "a135", "a136", "a137", "a138", "a139", "a140", "a141", "a142", "a143", "a144", "a145", "a146", "a147", "a148", "a149", "a150", "a151", "a152", "a153", "a154", "a155", "a156", "a157", "a158", "a159", "a160", "a161", "a162", "a163", "a164", "a165", "a166", "a167", "a168", "a169", "a170", "a171", "a172", "a173", "a174", "a175", "a176", "a177", "a178", "a179", "a180", "a181", "a182", "a183", "a184", "a185", "a186", "a187", "a188", "a189", "a190", "a191", "a192", "a193", "a194", "a195", "a196", "a197", "a198", "a199", "a200", "a201", "a202", "a203", "a204", "a205", "a206", "a207", "a208", "a209", "a210", "a211", "a212", "a213", "a214", "a215", "a216", "a217", "a218", "a219", "a220", "a221", "a222", "a223", "a224", "a225", "a226", "a227", "a228", "a229", "a230", "a231", "a232", "a233", "a234", "a235", "a236", "a237", "a238", "a239", "a240", "a241", "a242", "a243", "a244", "a245", "a246", "a247", "a248", "a249", "a250", "a251", "a252", "a253", "a254", "a255"

template <int B, int E, class F>
__device__ __forceinline__ void static_for(F&& f) {  // f(integral_constant<int, i>) for i = B .. E-1, fully unrolled with constant indices
  if constexpr (B < E) {
    f(std::integral_constant<int, B>{});
    static_for<B + 1, E>(f);
  }
}
using k0 = std::integral_constant<int, 0>;
using k1 = std::integral_constant<int, 1>;

__device__ __forceinline__ void claim_accumulators() { asm volatile("" ::: X2V_AGPRS); }  // at kernel entry: the accumulator half belongs to the asm statements
template <int R>
__device__ __forceinline__ float acc_read() {
  float x;
  asm volatile("v_accvgpr_read_b32 %0, a[%c1]" : "=v"(x) : "i"(R) : X2V_AGPRS);
  return x;
}
// bf16: accumulator tile I (16 x 16; I = x block * 8 + W block) is a[4 I : 4 I + 3]
template <int I>
__device__ __forceinline__ void mfma_bf16(const bf16x8_t& wf, const bf16x8_t& xf) {
  asm volatile("v_mfma_f32_16x16x32_bf16 a[%c2:%c3], %0, %1, a[%c2:%c3]" ::"v"(wf), "v"(xf), "i"(4 * I), "i"(4 * I + 3) : X2V_AGPRS);
}
template <int I>
__device__ __forceinline__ void mfma_bf16_first(const bf16x8_t& wf, const bf16x8_t& xf) {  // first k-step of an output tile: C = 0
  asm volatile("v_mfma_f32_16x16x32_bf16 a[%c2:%c3], %0, %1, 0" ::"v"(wf), "v"(xf), "i"(4 * I), "i"(4 * I + 3) : X2V_AGPRS);
}

// ---- The pieces below live INSIDE a kernel body and are macros, each defined once here, and not functions: these kernels sit at the SGPR limit
//      with a slot stream pinned by sched_barrier and an accumulator half the compiler cannot see, and the function form of the same statements
//      (structs for the schedule, the DMA offsets and the fragments, a template for the K tile) came out with a different register allocation —
//      gemm256c 436 -> 440 VGPRs, other scalar spill lanes — and ~1400 moved instructions per kernel; even a lambda in place of
//      X2V_PIPE_STEP_CURSORS renamed the scalar registers of ~140.  As macros the kernels are instruction-identical to the measured ones.
//      They use the kernel's own names: A, lda_bytes, W, ldw_bytes, M, N, nk, ntm, ntn, gm_tiles, gb, smem, lane, wid, wr, wc.

// LDS-DMA cursor: which K tile of which output tile a piece belongs to.  Descriptors are wave-uniform (SGPRs).
struct Cursor {
  __amdgpu_buffer_rsrc_t ra, rw;
  unsigned kw;  // byte offset of the K tile within a W row
  unsigned ka;  // byte offset of the K tile within an x row (K-blocked x: GemmBlocking)
  int kc;       // index of the K tile within its K block of x
  int k;        // index of the K tile within the output tile
};

// ---- tile schedule of a PERSISTENT workgroup: its output tiles are positions v, v + vstep, .. < vend of the grouped tile order; XCD x (= blockIdx % 8,
//      the dispatcher's placement) owns the contiguous chunk x of that order — the same assignment an in-order dispatch of one workgroup per tile
//      gives — and its workgroups take the chunk's positions round-robin.
#define X2V_PIPE_PERSISTENT_CHUNK()                                                                                                                    \
  const unsigned nblk = (unsigned)ntm * (unsigned)ntn;                                                                                               \
  unsigned v, vstep, vend;                                                                                                                           \
  if (gridDim.x == nblk) {                                                                                                                           \
    v = xcd_remap(blockIdx.x, nblk);                                                                                                                 \
    vstep = 1u;                                                                                                                                      \
    vend = v + 1u;                                                                                                                                   \
  } else {                                                                                                                                           \
    const unsigned x = blockIdx.x & 7u, j = blockIdx.x >> 3, per = gridDim.x >> 3;                                                                   \
    const unsigned q = nblk >> 3, r = nblk & 7u;                                                                                                     \
    const unsigned base = x < r ? x * (q + 1u) : r * (q + 1u) + (x - r) * q;                                                                         \
    v = base + j;                                                                                                                                    \
    vstep = per;                                                                                                                                     \
    vend = base + q + (x < r ? 1u : 0u);                                                                                                             \
  }
// ---- tiles (X2V_PIPE_COORDS) and their operands' K tiles (X2V_PIPE_OPERANDS), one workgroup per tile as well as persistent:
//   coords(p, tm, tn)                 tile coordinates of position p: grouped ordering, gm_tiles m-tiles x all n-tiles per group (as gemm256.hip)
//   operands(tm, tn, live, ra, rw)    buffer descriptors over a tile's valid rows: rows past M / N read as zero through the bounds check; `live`
//                                     false: an empty range (every piece reads as zero) — what the cursors point at behind the last output tile
//   X2V_PIPE_NEXT_KA(ka, kc, wrap)    K-blocked x: byte offset `ka` within a row and index `kc` within its K block, to the next K tile
//   advance(cursor, nra, nrw)         to the next K tile of the pipeline; behind an output tile's last K tile: K tile 0 of the tile (nra, nrw) describe
#define X2V_PIPE_A_WRAP() (gb.a_cbs - (unsigned)(a_kpb - 1) * 128u) /* from the last K tile of an x block to the first of the next */
#define X2V_PIPE_NEXT_KA(OFF_, CNT_, WRAP_) { if (++(CNT_) == a_kpb) { (CNT_) = 0; (OFF_) += (WRAP_); } else (OFF_) += 128u; }
#define X2V_PIPE_COORDS()                                                                                                                            \
  const unsigned GM = (unsigned)gm_tiles;                                                                                                            \
  const unsigned per_group = GM * (unsigned)ntn;                                                                                                     \
  auto coords = [&](unsigned p, int& tm, int& tn) {                                                                                                  \
    const unsigned group = p / per_group, in_g = p % per_group;                                                                                      \
    const unsigned first_m = group * GM;                                                                                                             \
    const unsigned gsz = min((unsigned)ntm - first_m, GM);                                                                                           \
    tm = (int)(first_m + in_g % gsz);                                                                                                                \
    tn = (int)(in_g / gsz);                                                                                                                          \
  };
#define X2V_PIPE_OPERANDS()                                                                                                                          \
  const unsigned row_bytes = (unsigned)nk * 128u;                                                                                                    \
  const int a_kpb = gb.a_kpb > 0 && gb.a_kpb < nk ? gb.a_kpb : nk; /* K tiles per K block of x (GemmBlocking) */                                     \
  const unsigned a_span = a_kpb < nk ? (unsigned)((nk - 1) / a_kpb) * gb.a_cbs + (unsigned)a_kpb * 128u : row_bytes;                                 \
  const unsigned a_wrap = X2V_PIPE_A_WRAP();                                                                                                         \
  auto operands = [&](int tm, int tn, bool live, __amdgpu_buffer_rsrc_t& ra, __amdgpu_buffer_rsrc_t& rw) {                                           \
    const int64_t m0 = (int64_t)tm * TILE;                                                                                                           \
    const int n0 = tn * TILE;                                                                                                                        \
    const int rows_a = (int)min((int64_t)TILE, M - m0), rows_w = min(TILE, N - n0);                                                                  \
    ra = __builtin_amdgcn_make_buffer_rsrc((void*)(A + m0 * lda_bytes), 0, live ? (unsigned)((rows_a - 1) * lda_bytes) + a_span : 0u, 0x00020000);   \
    rw = __builtin_amdgcn_make_buffer_rsrc((void*)(W + (int64_t)n0 * ldw_bytes), 0, live ? (unsigned)((rows_w - 1) * ldw_bytes) + row_bytes : 0u,    \
                                           0x00020000);                                                                                              \
  };                                                                                                                                                 \
  auto advance = [&](Cursor& c, const __amdgpu_buffer_rsrc_t& nra, const __amdgpu_buffer_rsrc_t& nrw) {                                              \
    if (++c.k == nk) {                                                                                                                               \
      c.k = 0;                                                                                                                                       \
      c.kw = 0u;                                                                                                                                     \
      c.ka = 0u;                                                                                                                                     \
      c.kc = 0;                                                                                                                                      \
      c.ra = nra;                                                                                                                                    \
      c.rw = nrw;                                                                                                                                    \
    } else {                                                                                                                                         \
      c.kw += 128u;                                                                                                                                  \
      X2V_PIPE_NEXT_KA(c.ka, c.kc, a_wrap)                                                                                                           \
    }                                                                                                                                                \
  };

// ---- LDS-DMA: wave `wid` stages rows [64 wid, 64 wid + 64) of both operand tiles as 8 pieces of 8 rows (1 KiB, lane-linear in LDS).
//      Piece i = 2 j + par: row 64 wid + 16 j + 8 par + (lane>>3); its swizzle (row>>1)&7 = ((lane>>4) + 4 par) & 7 does not depend on j,
//      so two per-lane offsets per operand serve all pieces and 16 j rows travel in the scalar offset with the K offset.
#define X2V_PIPE_DMA_OFFSETS()                                                    \
  unsigned a_voff[2], w_voff[2];                                                  \
  _Pragma("unroll") for (int par = 0; par < 2; ++par) {                           \
    const int r = wid * 64 + par * 8 + (lane >> 3);                               \
    const int c = (lane & 7) ^ (((lane >> 4) + 4 * par) & 7);                     \
    a_voff[par] = (unsigned)(r * lda_bytes) + (unsigned)(c << 4);                 \
    w_voff[par] = (unsigned)(r * ldw_bytes) + (unsigned)(c << 4);                 \
  }                                                                               \
  const unsigned a_j = (unsigned)(16 * lda_bytes), w_j = (unsigned)(16 * ldw_bytes);
// piece P_ in 0..15 (0..7 = W pieces, 8..15 = x pieces) of the K tile at byte offsets KW_ / KA_ of the rows (RW_, RA_) describe, into stage STAGE_
#define X2V_PIPE_DMA_AT(P_, STAGE_, RA_, RW_, KW_, KA_)                                                                                             \
  {                                                                                                                                                 \
    constexpr int i_ = (P_) & 7;                                                                                                                    \
    if constexpr ((P_) < 8)                                                                                                                         \
      __builtin_amdgcn_raw_ptr_buffer_load_lds(RW_, (lds_ptr_t)(smem + (STAGE_) * STAGE_BYTES + wid * 8192 + i_ * 1024), 16, w_voff[i_ & 1],        \
                                               (KW_) + (unsigned)(i_ >> 1) * w_j, 0, 0);                                                            \
    else                                                                                                                                            \
      __builtin_amdgcn_raw_ptr_buffer_load_lds(RA_, (lds_ptr_t)(smem + (STAGE_) * STAGE_BYTES + OP_BYTES + wid * 8192 + i_ * 1024), 16,             \
                                               a_voff[i_ & 1], (KA_) + (unsigned)(i_ >> 1) * a_j, 0, 0);                                            \
  }
#define X2V_PIPE_DMA(P_, STAGE_, CUR_) X2V_PIPE_DMA_AT(P_, STAGE_, (CUR_).ra, (CUR_).rw, (CUR_).kw, (CUR_).ka)  // of the K tile a cursor points at

// ---- bf16 fragments (16x16x32: row r16 of a 16-row block, 16-byte chunk ks*4 + g16), block offsets travel as immediates; uses the kernel's r16, g16
#define X2V_PIPE_BF16_FRAGMENTS()                                        \
  int rd_x[2], rd_w[2];                                                  \
  {                                                                      \
    const int swz = (r16 >> 1) & 7;                                      \
    _Pragma("unroll") for (int ks = 0; ks < 2; ++ks) {                   \
      const int o = r16 * 128 + ((((ks << 2) | g16) ^ swz) << 4);        \
      rd_x[ks] = o + OP_BYTES + wr * 16384;                              \
      rd_w[ks] = o + wc * 16384;                                         \
    }                                                                    \
  }                                                                      \
  bf16x8_t fx[2][8], fw[2][8];
// read R_ in 0..15 of k-step KS_ of the tile in stage STAGE_; order x0, W0..W7, x1..x7 (the first MFMA of a k-step needs x0 and W0)
#define X2V_PIPE_BF16_READ(R_, STAGE_, KS_)                                                                                                               \
  {                                                                                                                                                       \
    if constexpr ((R_) == 0) fx[KS_][0] = *reinterpret_cast<const bf16x8_t*>(smem + (STAGE_) * STAGE_BYTES + rd_x[KS_]);                                  \
    else if constexpr ((R_) <= 8) fw[KS_][(R_) - 1] = *reinterpret_cast<const bf16x8_t*>(smem + (STAGE_) * STAGE_BYTES + ((R_) - 1) * 2048 + rd_w[KS_]); \
    else fx[KS_][(R_) - 8] = *reinterpret_cast<const bf16x8_t*>(smem + (STAGE_) * STAGE_BYTES + ((R_) - 8) * 2048 + rd_x[KS_]);                           \
  }

// ---- the continuous kernels' K-tile slot stream and output-tile loop: ONE software pipeline over (output tile, K tile) pairs.  The "tile t+1 / t+2"
//      cursors simply run on into the next output tile with that tile's descriptors, so after the first output tile there is no prologue — when an
//      output tile's last K tile retires, K tile 0 of the next one has landed in LDS and K tile 1 is in flight.  Needs an even number of K tiles >= 4
//      (every output tile then starts in LDS stage 0).  Parameterised by what differs between bf16 and e4m3:
//        MFMA_(n, FIRST)        what slot n multiplies (bf16: an MFMA in every slot; e4m3: in every fourth; int8: in every second); FIRST: C = 0
//        READ_(R, STAGE, KS)    fragment read R in 0..15 of k-step KS
//      and by the kernel's own NXLOAD, xload(integral_constant<j>) (epilogue-operand load j, riding in the LAST K tile's slots),
//      epilogue_setup(tm, tn) (an output tile becomes current) and epilogue() (behind its last K tile).
//      tile(ST, FIRST, LAST, c1, c2) is one K tile.  ST = its LDS stage; FIRST: K tile 0 of an output tile (k-step 0 starts the accumulators from 0);
//      LAST: the output tile's last K tile (the k-step-0 fragments of the next output tile are read behind the epilogue instead of here — the
//      epilogue needs the registers).  c1 / c2: cursors of the pipeline's next / next-but-one K tile.
//      vmcnt: the counted waits (LDS-DMA landed) have only LOADS younger than the pieces they wait for; older stores of the previous output tile's
//      epilogue only make them stricter.  Waits for register-returning loads (bias, gate, residual, scales) are the compiler's.
#define X2V_PIPE_STEP_CURSORS() { cu1 = cu2; advance(cu2, nra, nrw); }  // the cursors one K tile on
#define X2V_PIPE_CONTINUOUS(MFMA_, READ_)                                                                                                            \
  auto tile = [&](auto stc, auto firstc, auto lastc, const Cursor& c1, const Cursor& c2) {                                                           \
    constexpr int ST = decltype(stc)::value;                                                                                                         \
    constexpr bool FIRST = decltype(firstc)::value != 0, LAST = decltype(lastc)::value != 0;                                                         \
    static_for<0, 128>([&](auto nc) {                                                                                                                \
      constexpr int n = decltype(nc)::value;                                                                                                         \
      MFMA_(n, FIRST)                                                                                                                                \
      if constexpr (n < 32 && (n & 1) == 0) READ_(n >> 1, ST, 1) /* k-step 1 of this tile */                                                         \
      /* the last 16 - EARLY pieces of tile t+1 (its stage was freed by the previous tile's first barrier) */                                        \
      if constexpr (late_slot(n)) X2V_PIPE_DMA(EARLY + (n - LATE0) / STEP, ST ^ 1, c1)                                                               \
      if constexpr (n == FREE) {                                                                                                                     \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); /* every fragment of this tile is in registers: the stage may be overwritten */           \
        __builtin_amdgcn_s_barrier();                                                                                                                \
      }                                                                                                                                              \
      /* the first EARLY pieces of tile t+2 into this tile's stage */                                                                                \
      if constexpr (dma_slot(n)) X2V_PIPE_DMA((n - FREE - 1) / STEP, ST, c2)                                                                         \
      if constexpr (LAST && xload_index(n) >= 0 && xload_index(n) < NXLOAD) xload(std::integral_constant<int, xload_index(n)>{});                    \
      if constexpr (n == READY) {                                                                                                                    \
        /* tile t+1 has landed; younger loads may stay in flight: the pieces of tile t+2 issued so far in this tile (+ the epilogue operands) */     \
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NEWER + (LAST ? NXLOAD : 0)) : "memory");                                                           \
        __builtin_amdgcn_s_barrier();                                                                                                                \
      }                                                                                                                                              \
      if constexpr (!LAST && n > READY + 1 && (n & 1) == 0) READ_((n - READY - 2) >> 1, ST ^ 1, 0) /* k-step 0 of the next tile */                   \
      __builtin_amdgcn_sched_barrier(0);                                                                                                             \
    });                                                                                                                                              \
  };                                                                                                                                                 \
  /* pipeline start: K tile 0 of the first output tile and the first EARLY pieces of its K tile 1 in flight, tile 0 landed */                        \
  int tm, tn;                                                                                                                                        \
  coords(v, tm, tn);                                                                                                                                 \
  Cursor cu1, cu2;                                                                                                                                   \
  {                                                                                                                                                  \
    __amdgpu_buffer_rsrc_t ra, rw;                                                                                                                   \
    operands(tm, tn, true, ra, rw);                                                                                                                  \
    cu1 = Cursor{ra, rw, 0u, 0u, 0, 0};                                                                                                              \
    static_for<0, 16>([&](auto pc) { X2V_PIPE_DMA(decltype(pc)::value, 0, cu1) });                                                                   \
    advance(cu1, ra, rw); /* K tile 1 (nk >= 4: no wrap here) */                                                                                     \
    static_for<0, EARLY>([&](auto pc) { X2V_PIPE_DMA(decltype(pc)::value, 1, cu1) });                                                                \
    cu2 = cu1;                                                                                                                                       \
    advance(cu2, ra, rw); /* K tile 2 */                                                                                                             \
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(EARLY) : "memory");                                                                                     \
  }                                                                                                                                                  \
  __builtin_amdgcn_s_barrier();                                                                                                                      \
  __builtin_amdgcn_sched_barrier(0);                                                                                                                 \
  for (;;) {                                                                                                                                         \
    /* current output tile (tm, tn); the one behind it, whose K tiles the cursors run into near the end of this one */                               \
    const bool has_next = v + vstep < vend;                                                                                                          \
    int ntm_ = tm, ntn_ = tn;                                                                                                                        \
    if (has_next) coords(v + vstep, ntm_, ntn_);                                                                                                     \
    __amdgpu_buffer_rsrc_t nra, nrw;                                                                                                                 \
    operands(ntm_, ntn_, has_next, nra, nrw);                                                                                                        \
    epilogue_setup(tm, tn);                                                                                                                          \
    static_for<0, 16>([&](auto rc) { READ_(decltype(rc)::value, 0, 0) }); /* k-step 0 of K tile 0 (stage 0: nk is even) */                           \
    __builtin_amdgcn_sched_barrier(0);                                                                                                               \
    tile(k0{}, k1{}, k0{}, cu1, cu2); /* K tile 0 */                                                                                                 \
    X2V_PIPE_STEP_CURSORS()                                                                                                                          \
    tile(k1{}, k0{}, k0{}, cu1, cu2); /* K tile 1 */                                                                                                 \
    X2V_PIPE_STEP_CURSORS()                                                                                                                          \
    for (int t = 2; t < nk - 2; t += 2) {                                                                                                            \
      tile(k0{}, k0{}, k0{}, cu1, cu2);                                                                                                              \
      X2V_PIPE_STEP_CURSORS()                                                                                                                        \
      tile(k1{}, k0{}, k0{}, cu1, cu2);                                                                                                              \
      X2V_PIPE_STEP_CURSORS()                                                                                                                        \
    }                                                                                                                                                \
    tile(k0{}, k0{}, k0{}, cu1, cu2); /* K tile nk - 2: cu2 already points at K tile 0 of the next output tile */                                    \
    X2V_PIPE_STEP_CURSORS()                                                                                                                          \
    tile(k1{}, k0{}, k1{}, cu1, cu2); /* K tile nk - 1 (LAST) */                                                                                     \
    X2V_PIPE_STEP_CURSORS()                                                                                                                          \
    epilogue();                                                                                                                                      \
    if (!has_next) break;                                                                                                                            \
    v += vstep;                                                                                                                                      \
    tm = ntm_;                                                                                                                                       \
    tn = ntn_;                                                                                                                                       \
  }                                                                                                                                                  \
  /* the pieces issued for the (non-existent) K tiles behind the last output tile read an empty range; let them retire before the LDS goes away */   \
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

}  // namespace pipe
}  // namespace x2v
