// Fused fp16 attention of ONE head as wide as the channel count, under the frame-causal prefix mask: the mid block of the HunyuanVideo VAE decoder
// (x2v.h: x2v_vae_attn_prep_f16, x2v_vae_attn_f16; arithmetic contract there).  No score matrix: online softmax over 64-key tiles.
//
// At head dimension 512 the LDS read rate limits a flash kernel before the matrix pipe does: a wave that owns 16 query rows and walks a whole key tile makes
// the workgroup read every K and V^T byte four times.  The split below reads 448 LDS bytes per v_mfma_f32_16x16x32_f16 (3.5 clocks of a 128 B/clk LDS
// against the 4 clocks a CU's four SIMDs need per instruction) where that plain split reads 1152.
//   workgroup   64 query rows, 4 waves, one per SIMD (the full register file: Q fragments 128 + O accumulators 128 registers per lane at C = 512).
//   Q K^T       2 x 2: wave (wr, wc) = (wid >> 1, wid & 1) multiplies rows 32 wr .. + 31 with keys 32 wc .. + 31 of the tile, S^T = K . Q^T.  Its Q
//               fragments (2 row groups x C / 32 k-steps x 16 bytes) are loaded once and stay in registers for the whole key walk; a K fragment read
//               from LDS feeds two instructions.  Accumulator element e of lane (g4, c16): query 32 wr + 16 qg + c16, key 32 wc + 16 kg + 4 g4 + e.
//   softmax     a row's 64 scores of a tile sit in two waves (4 lanes each): the two halves' maxima meet through LDS (mx), the running maximum is kept
//               by both waves, the row sum per wave over its own keys (added at the end).  p goes to LDS as fp16 [64 rows][64 keys], the rescale
//               factor of each row (al) next to it.
//   P V         by output columns: wave w owns all 64 rows x columns [C / 4 w, C / 4 (w + 1)), O^T = V^T . P^T — it reads only its quarter of the
//               V^T tile, and the P tile; a V^T fragment feeds four instructions.  Element e of lane (g4, c16): query 16 qg + c16, column
//               C / 4 w + 16 c + 4 g4 + e, so a row leaves as 16-byte fp32 stores.
//   LDS         one K tile [64 keys][C] and one V^T tile [C][64 keys], each single-buffered: K is free from the end of Q K^T on, so tile t + 1 is
//               fetched under softmax and P V of tile t; V^T is free from the end of P V on, so tile t + 1 is fetched under Q K^T of tile t + 1.  Both
//               come by LDS-DMA (buffer_load ... lds, 16 bytes per lane, 1 KiB lane-linear per instruction), un-padded, with the 16-byte chunk
//               swizzled on the global side: K chunk c of row r at c ^ (r & 15), V^T and P chunk c of row r at c ^ ((r >> 1) & 7) — the 16 lanes of a
//               fragment read differ in the row and land on 16 distinct 16-byte slots.  C = 512: 64 + 64 + 8 KiB + 768 B = 140 032 bytes.
//   key walk    a workgroup walks tiles 0 .. up to the last key its last row sees.  A tile that ends at or below the prefix limit of the block's FIRST row
//               is visible to every row: no mask code.  The others (a frame boundary inside, or the end of the sequence) take a select per score:
//               -inf for the maximum, 0 for p.  hw need not be a multiple of anything; a block may span frames.  Key 0 is visible to every row, so
//               the running maximum is finite from tile 0 on.
//   launch      block b is query block nqb - 1 - b: the longest walks start first.
//   Rows beyond n (the last block) read row n - 1 and are never stored.
#include "gemm_rows.h"
#include "x2v_common.h"

namespace x2v {

constexpr int VA_ROWS = 64;  // query rows per workgroup
constexpr int VA_KEYS = 64;  // keys per tile
// The reference maximum of a row (what the exponent subtracts) follows the row's running maximum only when that has grown by more than VA_LAZY: in
// between p = 2^(s - m) is at most 2^8, exact range for fp16 and fp32, relative rounding unchanged, and the accumulator rescale (128 registers per lane
// at C = 512) is skipped by every tile in which no row of the block moves.
constexpr float VA_LAZY = 8.0f;
constexpr int va_tile_bytes(int C) { return VA_KEYS * C * 2; }
constexpr int va_lds_bytes(int C) { return 2 * va_tile_bytes(C) + VA_ROWS * VA_KEYS * 2 + 3 * VA_ROWS * 4; }

typedef __attribute__((address_space(3))) void* va_lds_ptr_t;

// ---- preparation: fp32 [n, 3C] q|k|v -> fp16 q [n][C], k [64 nt][C] (zero rows from n on), V^T tiles [nt][C][64] (zero keys from n on) ---------------
__global__ __launch_bounds__(256) void vae_attn_prep_kernel(const float* __restrict__ qkv, int64_t ld, _Float16* __restrict__ q16, _Float16* __restrict__ k16,
                                                            _Float16* __restrict__ vt16, int n, int C) {
  const int t = blockIdx.x, tid = threadIdx.x;
  const int cpr = C / 8;  // 16-byte chunks of a q / k row
  for (int i = tid; i < VA_KEYS * cpr; i += 256) {
    const int row = t * VA_KEYS + i / cpr, ch = i % cpr;
    half8_t qh = {}, kh = {};
    if (row < n) {
      const float* src = qkv + (int64_t)row * ld + ch * 8;
      const f32x4_t q0 = *reinterpret_cast<const f32x4_t*>(src), q1 = *reinterpret_cast<const f32x4_t*>(src + 4);
      const f32x4_t k0 = *reinterpret_cast<const f32x4_t*>(src + C), k1 = *reinterpret_cast<const f32x4_t*>(src + C + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        qh[e] = (_Float16)q0[e];
        qh[4 + e] = (_Float16)q1[e];
        kh[e] = (_Float16)k0[e];
        kh[4 + e] = (_Float16)k1[e];
      }
      *reinterpret_cast<half8_t*>(q16 + (int64_t)row * C + ch * 8) = qh;
    }
    *reinterpret_cast<half8_t*>(k16 + (int64_t)row * C + ch * 8) = kh;
  }
  // V^T: one 16-byte chunk = 8 keys of one column; consecutive lanes take consecutive columns (each of the 8 reads is one coalesced row segment)
  for (int i = tid; i < C * 8; i += 256) {
    const int d = i % C, kc = i / C;
    half8_t vh = {};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int row = t * VA_KEYS + kc * 8 + j;
      if (row < n) vh[j] = (_Float16)qkv[(int64_t)row * ld + 2 * C + d];
    }
    *reinterpret_cast<half8_t*>(vt16 + ((int64_t)t * C + d) * VA_KEYS + kc * 8) = vh;
  }
}

// ---- the fused forward -------------------------------------------------------------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(256) void vae_attn_kernel(const _Float16* __restrict__ q16, const _Float16* __restrict__ k16, const _Float16* __restrict__ vt16,
                                                       float* __restrict__ out, int64_t ldo, int n, int hw, float scale_log2e) {
  constexpr int KS = C / 32;        // k-steps of Q K^T
  constexpr int DW = C / 4;         // output columns of a wave
  constexpr int DC = DW / 16;       // its column groups
  constexpr int NI = C / 32;        // DMA instructions per wave and operand tile (C / 8 KiB over 4 waves)
  constexpr int CPR = C / 8;        // 16-byte chunks of a K row
  constexpr int RPI = 64 / CPR > 0 ? 64 / CPR : 1;  // K rows per DMA instruction
  constexpr int TB = va_tile_bytes(C);
  static_assert(C % 128 == 0 && CPR <= 64, "a K row is at most one DMA instruction");
  extern __shared__ __attribute__((aligned(16))) char va_smem[];
  char* const Ks = va_smem;
  char* const Vs = va_smem + TB;
  char* const Ps = va_smem + 2 * TB;
  float* const mx = reinterpret_cast<float*>(va_smem + 2 * TB + VA_ROWS * VA_KEYS * 2);  // [2][64]: tile maxima of the two key halves; row sums at the end
  float* const al = mx + 2 * VA_ROWS;                                                    // [64]: this tile's rescale factor per row

  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c16 = lane & 15, g4 = lane >> 4;
  const int wr = wid >> 1, wc = wid & 1;
  const int nqb = (n + VA_ROWS - 1) / VA_ROWS;
  const int r0 = (nqb - 1 - (int)blockIdx.x) * VA_ROWS;
  const int nkt = (n + VA_KEYS - 1) / VA_KEYS;

  // prefix limits: of the block's first row (tiles below it take no mask), of its last row (the walk's end), of this lane's two rows
  const int lim_first = min(n, (r0 / hw + 1) * hw);
  const int lim_last = min(n, (min(r0 + VA_ROWS - 1, n - 1) / hw + 1) * hw);
  const int nt = (lim_last + VA_KEYS - 1) / VA_KEYS;
  int lim[2];
  half8_t qf[2][KS];
#pragma unroll
  for (int qg = 0; qg < 2; ++qg) {
    const int row = min(r0 + 32 * wr + 16 * qg + c16, n - 1);
    lim[qg] = min(n, (row / hw + 1) * hw);
    const _Float16* qp = q16 + (int64_t)row * C + 8 * g4;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[qg][ks] = *reinterpret_cast<const half8_t*>(qp + 32 * ks);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the Q fragments are in registers: from here on vmcnt counts tile DMA only

  const __amdgpu_buffer_rsrc_t rk = __builtin_amdgcn_make_buffer_rsrc((void*)k16, 0, (unsigned)nkt * (unsigned)TB, 0x00020000);
  const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc((void*)vt16, 0, (unsigned)nkt * (unsigned)TB, 0x00020000);
  // The per-lane source offsets are recomputed at every issue (one or two VALU operations each) from a lane id the compiler cannot see through: hoisted
  // out of the walk they would be 2 NI registers that the Q fragments and the accumulators do not leave.
  auto issue_k = [&](int t) {
    int ln = lane;
    asm volatile("" : "+v"(ln));
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int I = wid * NI + j;
      const int r = RPI * I + ln / CPR, pc = ln % CPR;
      const unsigned vo = (unsigned)r * (unsigned)(C * 2) + (unsigned)(pc ^ (r & 15)) * 16u;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rk, (va_lds_ptr_t)(Ks + I * 1024), 16, vo, (unsigned)t * (unsigned)TB, 0, 0);
    }
  };
  auto issue_v = [&](int t) {
    int ln = lane;
    asm volatile("" : "+v"(ln));
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int I = wid * NI + j;
      const int r = 8 * I + (ln >> 3), pc = ln & 7;
      const unsigned vo = (unsigned)r * 128u + (unsigned)(pc ^ ((r >> 1) & 7)) * 16u;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rv, (va_lds_ptr_t)(Vs + I * 1024), 16, vo, (unsigned)t * (unsigned)TB, 0, 0);
    }
  };

  f32x4_t o[DC][4];  // [column group][row group]
#pragma unroll
  for (int c = 0; c < DC; ++c)
#pragma unroll
    for (int i = 0; i < 4; ++i) o[c][i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float m[2] = {-INFINITY, -INFINITY}, l[2] = {0.f, 0.f};

  // LDS byte offsets of this lane's fragments
  int k_off[2], p_rd[4], v_rd;
#pragma unroll
  for (int kg = 0; kg < 2; ++kg) k_off[kg] = (32 * wc + 16 * kg + c16) * (C * 2);
#pragma unroll
  for (int i = 0; i < 4; ++i) p_rd[i] = (16 * i + c16) * 128;
  v_rd = (DW * wid + c16) * 128;
  const int sw8 = (c16 >> 1) & 7;  // the V^T / P swizzle of a row 16 b + c16

  issue_k(0);
  issue_v(0);
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NI) : "memory");  // K tile 0 has landed (this wave's pieces), V^T tile 0 may still fly
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");

  for (int t = 0; t < nt; ++t) {
    const bool more = t + 1 < nt;
    // ---- S^T = K . Q^T ------------------------------------------------------------------------------------------------------------------------------
    f32x4_t s[2][2];  // [row group][key group]
#pragma unroll
    for (int qg = 0; qg < 2; ++qg)
#pragma unroll
      for (int kg = 0; kg < 2; ++kg) s[qg][kg] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    // one wave per SIMD: nobody else hides the LDS latency, so the K fragments run two k-steps ahead of the instructions that take them
    half8_t kf[3][2];
#define VA_KFRAG(KS_) \
  _Pragma("unroll") for (int kg = 0; kg < 2; ++kg) kf[(KS_) % 3][kg] = *reinterpret_cast<const half8_t*>(Ks + k_off[kg] + (((((KS_) << 2) | g4) ^ c16) << 4))
    VA_KFRAG(0);
    VA_KFRAG(1);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      if (ks + 2 < KS) VA_KFRAG(ks + 2);
#pragma unroll
      for (int kg = 0; kg < 2; ++kg)
#pragma unroll
        for (int qg = 0; qg < 2; ++qg) s[qg][kg] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[ks % 3][kg], qf[qg][ks], s[qg][kg], 0, 0, 0);
    }
#undef VA_KFRAG
    const bool masked = (t + 1) * VA_KEYS > lim_first;  // workgroup-uniform
    const int key0 = t * VA_KEYS + 32 * wc + 4 * g4;
    float mloc[2];
#pragma unroll
    for (int qg = 0; qg < 2; ++qg) {
      mloc[qg] = -INFINITY;
#pragma unroll
      for (int kg = 0; kg < 2; ++kg)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float v = s[qg][kg][e] * scale_log2e;
          if (masked) v = key0 + 16 * kg + e < lim[qg] ? v : -INFINITY;
          s[qg][kg][e] = v;
          mloc[qg] = fmaxf(mloc[qg], v);
        }
      mloc[qg] = fmaxf(mloc[qg], __shfl_xor(mloc[qg], 16, 64));
      mloc[qg] = fmaxf(mloc[qg], __shfl_xor(mloc[qg], 32, 64));
      if (g4 == 0) mx[wc * VA_ROWS + 32 * wr + 16 * qg + c16] = mloc[qg];
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // A: the K tile is read (it may be overwritten), the tile maxima are in LDS
    asm volatile("" ::: "memory");
    if (more) issue_k(t + 1);

    // ---- online softmax, base 2 ------------------------------------------------------------------------------------------------------------------------
#pragma unroll
    for (int qg = 0; qg < 2; ++qg) {
      const int row = 32 * wr + 16 * qg + c16;
      const float mrow = fmaxf(mloc[qg], mx[(wc ^ 1) * VA_ROWS + row]);
      const bool move = mrow > m[qg] + VA_LAZY;  // tile 0: m = -inf, always
      const float mnew = move ? mrow : m[qg];
      const float alpha = move ? __builtin_amdgcn_exp2f(m[qg] - mnew) : 1.0f;  // tile 0: exp2(-inf) = 0
      m[qg] = mnew;
      float sum = 0.f;
#pragma unroll
      for (int kg = 0; kg < 2; ++kg) {
        half4_t ph;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float p = __builtin_amdgcn_exp2f(s[qg][kg][e] - mnew);
          if (masked) p = key0 + 16 * kg + e < lim[qg] ? p : 0.f;
          sum += p;  // the fp32 p, before it is rounded
          ph[e] = (_Float16)p;
        }
        const int ch = 4 * wc + 2 * kg + (g4 >> 1);
        *reinterpret_cast<half4_t*>(Ps + row * 128 + ((ch ^ sw8) << 4) + (g4 & 1) * 8) = ph;
      }
      sum += __shfl_xor(sum, 16, 64);
      sum += __shfl_xor(sum, 32, 64);
      l[qg] = l[qg] * alpha + sum;
      if (wc == 0 && g4 == 0) al[row] = alpha;
    }
    if (more) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NI) : "memory");  // V^T tile t has landed; K tile t + 1 stays in flight
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // B: P, the rescale factors and the V^T tile are in LDS
    asm volatile("" ::: "memory");

    // ---- O^T = alpha O^T + V^T . P^T --------------------------------------------------------------------------------------------------------------------
    float a[4];
    bool same = true;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      a[i] = al[16 * i + c16];
      same = same && a[i] == 1.0f;
    }
    if (!__all(same)) {  // wave-uniform, and rare behind the first tiles (VA_LAZY)
      // The accumulators live in the accumulation registers, which no vector instruction multiplies: each takes the round trip read, multiply, write
      // here, spelled out so that the register allocator does not move them (or the Q fragments) between the two files anywhere else in the walk.
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < DC; ++c)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float x = o[c][i][e], tmp;
            asm volatile("v_accvgpr_read_b32 %1, %0\n\tv_mul_f32 %1, %1, %2\n\tv_accvgpr_write_b32 %0, %1" : "+a"(x), "=&v"(tmp) : "v"(a[i]));
            o[c][i][e] = x;
          }
    }
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int chs = (((kk << 2) | g4) ^ sw8) << 4;
      half8_t pf[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) pf[i] = *reinterpret_cast<const half8_t*>(Ps + p_rd[i] + chs);
      half8_t vf[2];  // one column group ahead
      vf[0] = *reinterpret_cast<const half8_t*>(Vs + v_rd + chs);
#pragma unroll
      for (int c = 0; c < DC; ++c) {
        if (c + 1 < DC) vf[(c + 1) & 1] = *reinterpret_cast<const half8_t*>(Vs + v_rd + (c + 1) * 2048 + chs);
#pragma unroll
        for (int i = 0; i < 4; ++i) o[c][i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf[c & 1], pf[i], o[c][i], 0, 0, 0);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // K tile t + 1 has landed
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // C: V^T, P, al and mx are read; every wave's pieces of K tile t + 1 are in LDS
    asm volatile("" ::: "memory");
    if (more) issue_v(t + 1);
  }

  // ---- row sums of the two key halves meet; o / l goes out ------------------------------------------------------------------------------------------------
  if (g4 == 0) {
#pragma unroll
    for (int qg = 0; qg < 2; ++qg) mx[wc * VA_ROWS + 32 * wr + 16 * qg + c16] = l[qg];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = 16 * i + c16;
    if (r0 + row >= n) continue;
    const float inv = 1.0f / (mx[row] + mx[VA_ROWS + row]);
    float* op = out + (int64_t)(r0 + row) * ldo + DW * wid + 4 * g4;
#pragma unroll
    for (int c = 0; c < DC; ++c) {
      f32x4_t w;
#pragma unroll
      for (int e = 0; e < 4; ++e) w[e] = o[c][i][e] * inv;
      *reinterpret_cast<f32x4_t*>(op + 16 * c) = w;
    }
  }
}

template <int C>
static int launch_vae_attn(const void* q16, const void* k16, const void* vt16, float* out, int64_t ldo, int n, int hw, float scale, hipStream_t st) {
  const int lds = va_lds_bytes(C);
  int rc = ensure_dynamic_lds((const void*)vae_attn_kernel<C>, lds, "vae_attn_f16 attr");
  if (rc != X2V_OK) return rc;
  hipLaunchKernelGGL(vae_attn_kernel<C>, dim3((unsigned)((n + VA_ROWS - 1) / VA_ROWS)), dim3(256), lds, st, (const _Float16*)q16, (const _Float16*)k16, (const _Float16*)vt16, out,
                     ldo, n, hw, scale * 1.4426950408889634f);
  X2V_LAUNCH_CHECK("vae_attn_f16 launch");
  return X2V_OK;
}

// what both entries ask of the token count and the width: n tokens of C halves stay below 2^30 bytes (the tile DMA addresses an operand with 32 bits)
static int vae_attn_shape(const char* who, int64_t n, int C) {
  X2V_REQUIRE(C == 512 || C == 128, X2V_E_SHAPE, "%s: C=%d (the head widths built are 512 and 128)", who, C);
  X2V_REQUIRE(n >= 1 && n <= (1ll << 20), X2V_E_SHAPE, "%s: n=%lld tokens must be 1 .. 2^20", who, (long long)n);
  return X2V_OK;
}

}  // namespace x2v
using namespace x2v;

extern "C" __attribute__((visibility("default"))) int x2v_vae_attn_prep_f16(const float* qkv, int64_t ld, void* q16, void* k16, void* vt16, int64_t n, int C, void* stream) {
  int rc = vae_attn_shape("vae_attn_prep_f16", n, C);
  if (rc != X2V_OK) return rc;
  X2V_REQUIRE(ld >= 3ll * C, X2V_E_SHAPE, "vae_attn_prep_f16: row stride %lld is smaller than 3 C = %d", (long long)ld, 3 * C);
  X2V_REQUIRE(qkv && q16 && k16 && vt16, X2V_E_ARG, "vae_attn_prep_f16: null pointer");
  X2V_REQUIRE(ld % 4 == 0 && aligned16(qkv) && aligned16(q16) && aligned16(k16) && aligned16(vt16), X2V_E_ALIGN,
              "vae_attn_prep_f16: pointers must be 16-byte aligned and the row stride a multiple of 4 floats");
  hipLaunchKernelGGL(vae_attn_prep_kernel, dim3((unsigned)((n + VA_KEYS - 1) / VA_KEYS)), dim3(256), 0, (hipStream_t)stream, qkv, ld, (_Float16*)q16, (_Float16*)k16,
                     (_Float16*)vt16, (int)n, C);
  X2V_LAUNCH_CHECK("vae_attn_prep_f16 launch");
  return X2V_OK;
}

extern "C" __attribute__((visibility("default"))) int x2v_vae_attn_f16(const void* q16, const void* k16, const void* vt16, float* out, int64_t ldo, int frames, int hw, int C,
                                                                       float scale, void* stream) {
  X2V_REQUIRE(frames >= 1 && hw >= 1, X2V_E_SHAPE, "vae_attn_f16: frames=%d, hw=%d must be positive", frames, hw);
  const int64_t n = (int64_t)frames * hw;
  int rc = vae_attn_shape("vae_attn_f16", n, C);
  if (rc != X2V_OK) return rc;
  X2V_REQUIRE(ldo >= C, X2V_E_SHAPE, "vae_attn_f16: output row stride %lld is smaller than C = %d", (long long)ldo, C);
  X2V_REQUIRE(q16 && k16 && vt16 && out, X2V_E_ARG, "vae_attn_f16: null pointer");
  X2V_REQUIRE(ldo % 4 == 0 && aligned16(q16) && aligned16(k16) && aligned16(vt16) && aligned16(out), X2V_E_ALIGN,
              "vae_attn_f16: pointers must be 16-byte aligned and the output row stride a multiple of 4 floats");
  X2V_REQUIRE(scale > 0.f, X2V_E_ARG, "vae_attn_f16: scale must be positive");
  if (C == 512) return launch_vae_attn<512>(q16, k16, vt16, out, ldo, (int)n, hw, scale, (hipStream_t)stream);
  return launch_vae_attn<128>(q16, k16, vt16, out, ldo, (int)n, hw, scale, (hipStream_t)stream);
}
