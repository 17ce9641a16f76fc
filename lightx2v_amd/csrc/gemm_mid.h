// The LDS-tiled mid-M GEMM with split K, written over RowsElem<T> (gemm_rows.h); x2v_gemm_mid_f16 (gemm_mid.hip) instantiates it for fp16.
//
// gemm_mid_kernel — y[M,N] = epi(x[M,K] . W[N,K]^T + b) for 128 <= M <= 512 or so: too many rows for gemm_rows_kernel (no LDS, every wave re-reads its x
//   fragments from L2) and too few for the 256x256 pipeline (two row tiles at M = 351, 31 % of them padding, 32-48 workgroups for 256 CUs).
//   Workgroup = 128 rows of x by 128 rows of W, four waves as 2 x 2, a wave owns 64 x 64 = 4 x 4 accumulator tiles of 16 x 16 (64 VGPRs).  ONE tile
//   form: at the Llama tower's widths the K split, not a narrower tile, is what fills the machine.
//   Matrix instruction: v_mfma_f32_16x16x32_f16.  At a 64 x 64 wave tile it and 32x32x16 read the same LDS bytes per flop (both operands as one
//   ds_read_b128 per lane and 16 rows x 32 k / 32 rows x 16 k) and hold the same 64 accumulator registers; 16x16x32 is taken because with D = W . x^T a
//   lane ends up with 4 consecutive output columns of one row — 8-byte stores, bias / residual reads of the same shape, a SwiGLU (gate, up) pair inside
//   one lane, exactly gemm_rows_kernel's epilogue — and because 16-row blocks that lie wholly beyond M or N (M = 351: 2 of the last tile's 8) then drop
//   out of the workspace traffic and the epilogue wave-uniformly.  (Skipping their MFMAs too was tried in the first build: a branch per accumulator tile
//   broke the K loop into 32 pieces with a wait in each; the loop multiplies all 16 tiles.)
//   K tile = 64 elements = one 128-byte line per operand row.  LDS image of an operand tile (gemm256_pipe.h's): [128 rows][128 B], the 16-byte chunk c of
//   row r stored at chunk c ^ ((r >> 1) & 7).  A fragment read is one ds_read_b128 of row 16 b + (lane & 15), chunk 4 ks + (lane >> 4): the 16 lanes
//   served together differ in the row, rows r and r + 1 sit in the two 128-byte halves of the 256 bytes the banks span, and (r >> 1) & 7 permutes the
//   chunk over the 8 row pairs — 16 distinct 16-byte slots, no bank conflict.  Stage = W tile | x tile = 32 KiB; TWO stages = 64 KiB, so that two
//   workgroups share a CU (8 waves, 2 per SIMD: one's barriers and epilogue hide under the other's MFMAs).  A third stage would cost that second
//   workgroup; it is not taken.
//   Loads go from global memory to LDS directly (buffer_load ... lds, 16 bytes per lane, a wave-piece = 8 rows = 1 KiB lane-linear, the swizzle applied on
//   the global side), 4 + 4 pieces per wave and K tile.  Per K tile t: issue tile t + 1 into the other stage, s_waitcnt vmcnt(8) (tile t has landed,
//   t + 1 stays in flight under this tile's 32 MFMAs per wave), barrier, fragments + MFMAs of the two k-steps, barrier (the stage is free).
//   Tails: a lane whose row lies beyond M / N reads the tile's last valid row (never stored); K % 32 == 0, and in a last K tile of 32 elements the lanes
//   of chunks 4..7 read chunks 0..3 again and the second k-step is skipped.  The buffer descriptors span exactly the tile's valid rows.
//   Split K: workgroup (tm, s, tn) reduces the contiguous range s of whole K tiles (the first ranges take the extra tile).  With splits > 1 every
//   workgroup stores its fp32 tile to workspace slot (tile, s) (lane-linear 16-byte stores), __threadfence(), and one lane draws a ticket with atomicAdd
//   on the tile's counter.  The workgroup that draws splits - 1 sums the slots 0 .. splits - 1 IN THAT ORDER (its own from memory too: the bits do not
//   depend on who arrived last), applies the epilogue, stores y and sets the counter back to 0.  Nobody waits for anybody.
//   Grid: 1-D, workgroup ids round-robin over the 8 XCDs; xcd_remap gives XCD c the contiguous chunk c of the order (tn, s, tm) with tm fastest, so the
//   row tiles and K splits that read one W panel sit in one L2, next to each other in time.
//   Resources (hipcc -Rpass-analysis=kernel-resource-usage): 64 KiB LDS, see DESIGN §4.9 for the registers.
#pragma once
#include <algorithm>

#include "gemm_rows.h"

namespace x2v {

constexpr int MID_TILE = 128;                  // rows of x and rows of W per workgroup
constexpr int MID_KT = 64;                     // K elements per K tile (16-bit elements: 128 bytes per row)
constexpr int MID_OP_BYTES = MID_TILE * 128;   // one operand tile of one stage
constexpr int MID_STAGE_BYTES = 2 * MID_OP_BYTES;
constexpr int MID_LDS = 2 * MID_STAGE_BYTES;   // 65536
constexpr int MID_MAX_SPLITS = 16;
constexpr int MID_PART_FLOATS = MID_TILE * MID_TILE;  // one workspace slot

typedef __attribute__((address_space(3))) void* mid_lds_ptr_t;

template <typename T>
__global__ __launch_bounds__(256, 2) void gemm_mid_kernel(const T* __restrict__ x, int64_t ldx, const T* __restrict__ w, int64_t ldw, const T* __restrict__ bias, T* y, int64_t ldy,
                                                          int M, int N, int K, int epi, const T* resid, int64_t ldr, int splits, float* part,
                                                          unsigned* counters) {  // y may alias resid: neither is __restrict__
  static_assert(sizeof(T) == 2, "the LDS image is written for 16-bit elements");
  typedef typename RowsElem<T>::v8 v8;
  typedef typename RowsElem<T>::v4 v4;
  __shared__ __attribute__((aligned(16))) char smem[MID_LDS];
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c16 = lane & 15, g4 = lane >> 4;
  const int wm = wid >> 1, wn = wid & 1;
  const unsigned ntm = (unsigned)(M + MID_TILE - 1) / MID_TILE;
  const unsigned v = xcd_remap(blockIdx.x, gridDim.x);
  const unsigned tm = v % ntm, s = (v / ntm) % (unsigned)splits, tn = v / (ntm * (unsigned)splits);
  const int m0 = (int)tm * MID_TILE, n0 = (int)tn * MID_TILE;
  const int rows_x = min(MID_TILE, M - m0), rows_w = min(MID_TILE, N - n0);
  // this workgroup's K tiles [kt0, kt0 + nkt)
  const int kt_all = (K + MID_KT - 1) / MID_KT;
  const int kq = kt_all / splits, kr = kt_all % splits;
  const int kt0 = (int)s * kq + min((int)s, kr), nkt = kq + ((int)s < kr ? 1 : 0);

  const unsigned ldx_bytes = (unsigned)ldx * 2u, ldw_bytes = (unsigned)ldw * 2u;
  const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)(x + (int64_t)m0 * ldx), 0, (unsigned)(rows_x - 1) * ldx_bytes + (unsigned)K * 2u, 0x00020000);
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)(w + (int64_t)n0 * ldw), 0, (unsigned)(rows_w - 1) * ldw_bytes + (unsigned)K * 2u, 0x00020000);
  // wave `wid` stages rows [32 wid, 32 wid + 32) of both tiles as 4 pieces of 8 rows: piece q, lane -> row 32 wid + 8 q + (lane >> 3), LDS chunk
  // lane & 7 = global chunk (lane & 7) ^ swizzle(row), swizzle(row) = (4 (q & 1) + (lane >> 4)) & 7
  unsigned xo[4], wo[4], tail[2];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = wid * 32 + q * 8 + (lane >> 3);
    const unsigned gc = (unsigned)((lane & 7) ^ ((4 * (q & 1) + (lane >> 4)) & 7));
    xo[q] = (unsigned)min(r, rows_x - 1) * ldx_bytes + gc * 16u;
    wo[q] = (unsigned)min(r, rows_w - 1) * ldw_bytes + gc * 16u;
    if (q < 2) tail[q] = gc >= 4u ? 64u : 0u;  // a K tile of 32 elements: chunks 4..7 read 0..3 again (in bounds, never multiplied)
  }
  auto issue = [&](int kt, int st) {
    const unsigned ko = (unsigned)kt * 128u;
    const bool half = kt * MID_KT + MID_KT > K;
    char* base = smem + st * MID_STAGE_BYTES + wid * 4096;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const unsigned adj = half ? tail[q & 1] : 0u;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (mid_lds_ptr_t)(base + q * 1024), 16, wo[q] - adj, ko, 0, 0);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (mid_lds_ptr_t)(base + MID_OP_BYTES + q * 1024), 16, xo[q] - adj, ko, 0, 0);
    }
  };

  // 16-row blocks of this wave's 64 x 64 that hold a valid row of x / of W
  const int mlive = min(4, max(0, (rows_x - 64 * wm + 15) / 16)), nlive = min(4, max(0, (rows_w - 64 * wn + 15) / 16));
  f32x4_t acc[4][4];  // [W block j][x block i]
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[j][i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  // fragment of 16-row block b, k-step ks: b * 2048 + rd[ks]
  int rd[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) rd[ks] = c16 * 128 + ((((ks << 2) | g4) ^ ((c16 >> 1) & 7)) << 4);

  issue(kt0, 0);
  for (int t = 0; t < nkt; ++t) {
    const int st = t & 1;
    if (t + 1 < nkt) {
      issue(kt0 + t + 1, st ^ 1);
      asm volatile("s_waitcnt vmcnt(8)" ::: "memory");  // this wave's pieces of tile t have landed; the 8 of tile t + 1 stay in flight
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();  // every wave's pieces of tile t have landed
    asm volatile("" ::: "memory");
    const char* ws_ = smem + st * MID_STAGE_BYTES + wn * 8192;
    const char* xs_ = smem + st * MID_STAGE_BYTES + MID_OP_BYTES + wm * 8192;
    const int ksteps = (kt0 + t) * MID_KT + MID_KT > K ? 1 : 2;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      if (ks < ksteps) {
        v8 xf[4], wf[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          wf[b] = *reinterpret_cast<const v8*>(ws_ + b * 2048 + rd[ks]);
          xf[b] = *reinterpret_cast<const v8*>(xs_ + b * 2048 + rd[ks]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[j][i] = RowsElem<T>::mfma(wf[j], xf[i], acc[j][i]);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // every fragment of this tile is in registers
    __builtin_amdgcn_s_barrier();                        // stage st may be overwritten (by the issue of the next iteration)
    asm volatile("" ::: "memory");
  }

  if (splits > 1) {
    // slot (tile, s): value e of accumulator tile (j, i) of thread tid at ((j * 4 + i) * 256 + tid) * 4 + e — a wave stores 1 KiB per instruction
    const unsigned tile = tn * ntm + tm;
    float* slot0 = part + (size_t)tile * (unsigned)splits * MID_PART_FLOATS + tid * 4;
    float* mine = slot0 + (size_t)s * MID_PART_FLOATS;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (i < mlive && j < nlive) *reinterpret_cast<f32x4_t*>(mine + (j * 4 + i) * 1024) = acc[j][i];
    __threadfence();
    __syncthreads();
    unsigned* ticket = reinterpret_cast<unsigned*>(smem);  // the stages are free behind the K loop's last barrier
    if (tid == 0) *ticket = atomicAdd(counters + tile, 1u);
    __syncthreads();
    if (*ticket != (unsigned)splits - 1u) return;
    __threadfence();
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[j][i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    for (int p = 0; p < splits; ++p) {
      const float* from = slot0 + (size_t)p * MID_PART_FLOATS;
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (i < mlive && j < nlive) acc[j][i] += *reinterpret_cast<const f32x4_t*>(from + (j * 4 + i) * 1024);
    }
    if (tid == 0) counters[tile] = 0u;  // the next launch on this stream finds the workspace as the allocator left it
  }

  // acc[j][i][e] = row m0 + 64 wm + 16 i + c16, column n0 + 64 wn + 16 j + 4 g4 + e (N % 8 == 0: a group of 4 columns is wholly inside or outside).
  // The rounding points are gemm_rows_kernel's.
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + 64 * wm + 16 * i + c16;
    if (i >= mlive || m >= M) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = n0 + 64 * wn + 16 * j + 4 * g4;
      if (j >= nlive || n >= N) continue;
      float o[4] = {acc[j][i][0], acc[j][i][1], acc[j][i][2], acc[j][i][3]};
      if (epi == ROWS_EPI_SWIGLU) {  // (gate, up) pairs: silu(gate_proj(h)) * up_proj(h), fp32 on the two 16-bit Linear outputs
        typename RowsElem<T>::v2 o2;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const float a = (float)(T)o[2 * e], g = (float)(T)o[2 * e + 1];
          o2[e] = (T)(a * sigmoid_f(a) * g);
        }
        *reinterpret_cast<typename RowsElem<T>::v2*>(y + (int64_t)m * ldy + n / 2) = o2;
        continue;
      }
      if (bias != nullptr) {
        const v4 bv = *reinterpret_cast<const v4*>(bias + n);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] += (float)bv[e];
      }
      if (epi == ROWS_EPI_RESIDUAL) {
        const v4 rv = *reinterpret_cast<const v4*>(resid + (int64_t)m * ldr + n);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (float)rv[e] + (float)(T)o[e];
      }
      v4 ov;
#pragma unroll
      for (int e = 0; e < 4; ++e) ov[e] = (T)o[e];
      *reinterpret_cast<v4*>(y + (int64_t)m * ldy + n) = ov;
    }
  }
}

// ---- host: the split rule, the workspace layout and the launch ----------------------------------------------------------------------------------------
static inline int64_t gemm_mid_tiles(int64_t M, int N) { return ((M + MID_TILE - 1) / MID_TILE) * ((N + MID_TILE - 1) / MID_TILE); }
// K splits for `cus` compute units: none where the output tiles fill them; else enough ranges to, of at least two K tiles each, 16 at the most
static inline int gemm_mid_splits(int64_t M, int N, int K, int cus) {
  const int64_t tiles = gemm_mid_tiles(M, N);
  if (tiles >= cus) return 1;
  const int kt = (K + MID_KT - 1) / MID_KT;
  const int64_t want = (cus + tiles - 1) / tiles;
  const int cap = std::min(MID_MAX_SPLITS, std::max(1, kt / 2));
  return (int)std::min<int64_t>(want, cap);
}
// workspace: MID_MAX_SPLIT_TILES 32-bit counters, one per output tile, then the slots [tile][split][128 x 128] fp32.  The counters' place and size do NOT
// depend on the shape: launches of different shapes share one workspace, and a slot of one must never land on a counter of the next.
constexpr int MID_MAX_SPLIT_TILES = 1024;
constexpr int64_t MID_COUNTER_BYTES = MID_MAX_SPLIT_TILES * 4;
static inline int64_t gemm_mid_ws_bytes(int64_t M, int N, int splits) {
  return splits <= 1 ? 0 : MID_COUNTER_BYTES + gemm_mid_tiles(M, N) * splits * MID_PART_FLOATS * 4;
}
inline int gemm_mid_cu_count() {  // of the current device; 256 where none answers (host arithmetic on a machine without one)
  int dev = 0, n = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 8) n = 256;
  return n;
}

// N counts W's rows: with the gated epilogue y has N / 2 columns.  The entry has checked its own epilogue set.
template <typename T>
static int gemm_mid_launch(const char* who, const void* x, int64_t ldx, const void* w, int64_t ldw, const void* bias, void* y, int64_t ldy, int64_t M, int N, int K, int epilogue,
                           const void* resid, int64_t ldr, int splits, void* workspace, int64_t workspace_bytes, void* stream) {
  X2V_REQUIRE(x && w && y, X2V_E_ARG, "%s: null pointer", who);
  X2V_REQUIRE(epilogue != ROWS_EPI_RESIDUAL || resid != nullptr, X2V_E_ARG, "%s: the residual epilogue needs resid", who);
  X2V_REQUIRE(M >= 0 && M <= 4096 && N > 0 && K > 0, X2V_E_SHAPE, "%s: bad shape M=%lld N=%d K=%d (M <= 4096: the mid-M form)", who, (long long)M, N, K);
  X2V_REQUIRE(K % 32 == 0, X2V_E_SHAPE, "%s: K=%d must be a multiple of 32 (pad the operands with zero columns)", who, K);
  X2V_REQUIRE(N % 8 == 0, X2V_E_SHAPE, "%s: N=%d (rows of W) must be a multiple of 8", who, N);
  const int ny = rows_epi_gated(epilogue) ? N / 2 : N;
  X2V_REQUIRE(ldx >= K && ldw >= K && ldy >= ny && ldx % 8 == 0 && ldw % 8 == 0 && ldy % 4 == 0 && (resid == nullptr || (ldr >= N && ldr % 4 == 0)), X2V_E_ALIGN,
              "%s: leading dimensions must cover the rows (ldx, ldw multiples of 8, ldy, ldr of 4 %s)", who, RowsElem<T>::unit());
  X2V_REQUIRE(ldx < (1 << 22) && ldw < (1 << 22), X2V_E_SHAPE, "%s: ldx, ldw must be below 2^22 (a tile's 128 rows are addressed with 32 bits)", who);
  X2V_REQUIRE(aligned16(x) && aligned16(w) && aligned16(y) && aligned16(bias) && aligned16(resid), X2V_E_ALIGN, "%s: pointers must be 16-byte aligned", who);
  const int kt = (K + MID_KT - 1) / MID_KT;
  X2V_REQUIRE(splits >= 0 && splits <= kt, X2V_E_ARG, "%s: splits=%d, but K=%d has %d K tiles of %d", who, splits, K, kt, MID_KT);
  if (M == 0) return X2V_OK;
  if (splits == 0) splits = gemm_mid_splits(M, N, K, gemm_mid_cu_count());
  X2V_REQUIRE(splits == 1 || gemm_mid_tiles(M, N) <= MID_MAX_SPLIT_TILES, X2V_E_ARG, "%s: %lld output tiles fill any device; K is split for at most %d", who,
              (long long)gemm_mid_tiles(M, N), MID_MAX_SPLIT_TILES);
  const int64_t need = gemm_mid_ws_bytes(M, N, splits);
  X2V_REQUIRE(splits == 1 || (workspace != nullptr && workspace_bytes >= need), X2V_E_ARG, "%s: %d K splits need a zero-initialised workspace of %lld bytes, got %lld", who, splits,
              (long long)need, (long long)(workspace ? workspace_bytes : 0));
  X2V_REQUIRE(splits == 1 || aligned16(workspace), X2V_E_ALIGN, "%s: the workspace must be 16-byte aligned", who);
  unsigned* counters = splits > 1 ? (unsigned*)workspace : nullptr;
  float* part = splits > 1 ? (float*)((char*)workspace + MID_COUNTER_BYTES) : nullptr;
  const dim3 grid((unsigned)(gemm_mid_tiles(M, N) * splits));
  hipLaunchKernelGGL(gemm_mid_kernel<T>, grid, dim3(256), 0, (hipStream_t)stream, (const T*)x, ldx, (const T*)w, ldw, (const T*)bias, (T*)y, ldy, (int)M, N, K, epilogue,
                     (const T*)resid, ldr, splits, part, counters);
  char what[64];
  snprintf(what, sizeof(what), "%s launch", who);
  return check_hip(hipGetLastError(), what);
}

}  // namespace x2v
