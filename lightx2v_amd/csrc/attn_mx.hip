// Block-scaled fp8 self-attention, head dim 128 (attention type "hip_mxfp8"; the contract is in include/x2v.h, its float64 restatement in
// tests/attn_mx_ref.py): Q^ and K^ are MXFP8 along the head dimension, V^T^ is MXFP8 along the keys, and both products run on
// v_mfma_scale_f32_16x16x128_f8f6f4 — one instruction spans the whole head dimension (QK^T) or a whole 128-key tile (PV), applies the operands'
// e8m0 block scales itself and does twice the bf16 work per clock.
//
// Bound: MFMA.  Algorithmic work per launch = 4 * Sq * Sk * H * 128 FLOP; the preparation passes are HBM-bound (k is read twice, q and v once).
//
// Preparation (three small kernels): the fp32 column mean of k in a fixed summation order, the q / k quantiser (codes [H][S_pad][128], one scale
// dword per token and head) and the V quantiser (codes [H][NT][128 dv][128 keys], one scale dword per dv row and tile).
//
// The forward keeps v9's work split (attn.hip): one workgroup = 8 waves x 32 query rows of one head, a wave's rows are two groups of 16, "swapped"
// products S^T = K^ . Q^^T and O^T += V^T^ . P^ so that a lane owns one query column per group and P never leaves registers; K^ / V^T^ tiles of
// 128 keys (16 KiB each, the bytes of v9's 64-key bf16 tiles) and their 512 + 512 scale bytes arrive by LDS-DMA, double buffered, one barrier per
// tile.  What it does not take over is the ping-pong of wave pairs: every wave runs QK^T, softmax and PV of a tile in turn, and the two waves of a
// SIMD overlap only as the scheduler lets them.
//   * operand map of the 16x16x128 e4m3 form (probed on the hardware with one-hot operands, as gemm.hip's map of the 32x32x64 form was): lane
//     (c = lane & 15, g = lane >> 4) holds row / column c; of its 32 code bytes the first 16 are k = 16 g .. 16 g + 15 and the last 16 are
//     k = 64 + 16 g .. 64 + 16 g + 15; scale block b (k = 32 b .. 32 b + 31) takes byte `opsel` of the scale VGPR of lane (c, b).  So a lane reads
//     the 16-byte chunks g and 4 + g of its 128-byte operand row and shifts the row's scale dword down by g bytes.
//   * S^T sub-tile tt (8 per tile) holds, in row i, key kappa(tt, i) = 64 (tt >> 2) + 16 (i >> 2) + 4 (tt & 3) + (i & 3) of the tile: the output lane
//     (c, g) owns rows 4 g + r, i.e. over tt = 0..7 exactly the keys {16 g .. 16 g + 15} u {64 + 16 g .. 64 + 16 g + 15} in k-slot order — the 32
//     packed e4m3 P^ of a lane ARE the B operand of the PV instruction against V^T^ rows in natural key order.
//   * LDS images: K^ [128 keys][128 B] and V^T^ [128 dv][128 B], the 16-byte chunk index XORed with hK(key) = ((key >> 4) & 3) | (((key >> 1) & 1) << 2)
//     resp. hV(dv) = (dv >> 1) & 7 (the 16 rows a 16-lane group reads hit 16 distinct 16-byte slots); the swizzle sits on the DMA source address.
//   * softmax: scores leave the MFMA relative to the running max (C = -m); the running max is exact (no lazy threshold, x2v.h), P <= 1,
//     P^ = e4m3(P * 2^8) with operand scale byte 119; l accumulates the fp32 P.
#include "x2v_common.h"

namespace x2v {

constexpr int MX_KV = 128;                          // keys per tile
constexpr int MX_TILE_BYTES = MX_KV * 128;          // 16 KiB: one K^ or V^T^ tile
constexpr int MX_SC_BYTES = 512;                    // scale dwords of a tile (128 rows)
constexpr int MX_BUF_BYTES = 2 * MX_TILE_BYTES + 2 * MX_SC_BYTES;
constexpr int MX_LDS_BYTES = 2 * MX_BUF_BYTES;      // 67,584 B
constexpr int MX_MEAN_CHUNK = 256;                  // tokens per chunk of the column-mean reduction (part of the contract)
constexpr int MX_P_SHIFT = 8;                       // P^ = e4m3(P * 2^8)

typedef __attribute__((address_space(3))) void* mx_lds_ptr_t;

// ------------------------------------------------------------------------------------------------ column mean of k
// pass 1: block (chunk, head), 64 lanes x 2 columns: part[chunk][col] = fp32 sum over the chunk's tokens in token order
__global__ __launch_bounds__(64) void mx_kmean_part_kernel(const unsigned short* __restrict__ k, int64_t ldk, float* __restrict__ part, int64_t Sk, int cols) {
  const int64_t t0 = (int64_t)blockIdx.x * MX_MEAN_CHUNK;
  const int64_t t1 = t0 + MX_MEAN_CHUNK < Sk ? t0 + MX_MEAN_CHUNK : Sk;
  const int col = blockIdx.y * 128 + threadIdx.x * 2;
  const unsigned short* p = k + t0 * ldk + col;
  unsigned w = *reinterpret_cast<const unsigned*>(p);
  float s0 = bf_lo(w), s1 = bf_hi(w);
  for (int64_t t = t0 + 1; t < t1; ++t) {
    p += ldk;
    w = *reinterpret_cast<const unsigned*>(p);
    s0 = __fadd_rn(s0, bf_lo(w));
    s1 = __fadd_rn(s1, bf_hi(w));
  }
  *reinterpret_cast<float2*>(part + (int64_t)blockIdx.x * cols + col) = make_float2(s0, s1);
}
// pass 2: one lane per column: the chunk sums in chunk order, divided by Sk
__global__ __launch_bounds__(128) void mx_kmean_final_kernel(const float* __restrict__ part, float* __restrict__ mean, int nchunk, int cols, float fsk) {
  const int col = blockIdx.x * 128 + threadIdx.x;
  float s = part[col];
  for (int c = 1; c < nchunk; ++c) s = __fadd_rn(s, part[(int64_t)c * cols + col]);
  mean[col] = __fdiv_rn(s, fsk);
}

// ------------------------------------------------------------------------------------------------ q / k quantiser
// mx.hip's quantiser with (x - mean) * scale in front and head-major output.  One lane = 8 consecutive channels, 4 lanes = one scale block,
// 16 lanes = one token of one head (one scale dword).  Rows S .. S_pad - 1 are written as zeros.
__global__ __launch_bounds__(256) void mx_quant_qk_kernel(const unsigned short* __restrict__ x, int64_t ldx, const float* __restrict__ mean, float scale,
                                                          unsigned char* __restrict__ q, unsigned* __restrict__ sc, int64_t S, int64_t S_pad, int H) {
  const int kc = H * 16;
  const int64_t total = S_pad * kc;  // a multiple of 16: the 16 lanes of a token and head are in range together
  for (int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x; id < total; id += (int64_t)gridDim.x * 256) {
    const int64_t row = id / kc;
    const int c = (int)(id - row * kc);
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = 0.f;
    if (row < S) {
      unpack8(*reinterpret_cast<const uint4*>(x + row * ldx + c * 8), v);
      float m[8];
      if (mean != nullptr) {
        const float4 m0 = *reinterpret_cast<const float4*>(mean + c * 8), m1 = *reinterpret_cast<const float4*>(mean + c * 8 + 4);
        m[0] = m0.x; m[1] = m0.y; m[2] = m0.z; m[3] = m0.w;
        m[4] = m1.x; m[5] = m1.y; m[6] = m1.z; m[7] = m1.w;
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) m[j] = 0.f;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = __fmul_rn(__fsub_rn(v[j], m[j]), scale);
    }
    float amax = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(v[j]));
    amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
    amax = fmaxf(amax, __shfl_xor(amax, 2, 64));
    unsigned w[2];
    const unsigned byte = mxfp8_block<8>(v, amax, w);
    const int head = c >> 4, c16 = c & 15;
    const int64_t orow = (int64_t)head * S_pad + row;
    *reinterpret_cast<uint2*>(q + orow * 128 + c16 * 8) = make_uint2(w[0], w[1]);
    const unsigned dw = e8m0_gather4(byte, 4);
    if (c16 == 0) sc[orow] = dw;
  }
}

// ------------------------------------------------------------------------------------------------ V quantiser
// block (tile, head): the tile's 128 keys x 128 dv go through LDS (keys >= Sk as zeros); a lane then owns (dv row, 32-key block) twice.
__global__ __launch_bounds__(256) void mx_quant_vt_kernel(const unsigned short* __restrict__ v, int64_t ldv, unsigned char* __restrict__ q, unsigned char* __restrict__ sc,
                                                          int64_t Sk) {
  __shared__ __attribute__((aligned(16))) unsigned short tile[MX_KV * 128];
  const int tid = threadIdx.x, head = blockIdx.y;
  const int64_t k0 = (int64_t)blockIdx.x * MX_KV;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int ch = tid + 256 * i, key = ch >> 4, c = ch & 15;
    uint4 w = make_uint4(0u, 0u, 0u, 0u);
    if (k0 + key < Sk) w = *reinterpret_cast<const uint4*>(v + (k0 + key) * ldv + head * 128 + c * 8);
    *reinterpret_cast<uint4*>(tile + key * 128 + c * 8) = w;
  }
  __syncthreads();
  const int64_t trow = ((int64_t)head * gridDim.x + blockIdx.x) * 128;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int dv = tid & 127, blk = (tid >> 7) + 2 * i;
    float f[32];
    float amax = 0.f;
#pragma unroll
    for (int j = 0; j < 32; ++j) {
      f[j] = bf2f(tile[(32 * blk + j) * 128 + dv]);
      amax = fmaxf(amax, fabsf(f[j]));
    }
    unsigned w[8];
    const unsigned byte = mxfp8_block<32>(f, amax, w);
    unsigned char* dst = q + (trow + dv) * 128 + blk * 32;
    *reinterpret_cast<uint4*>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
    *reinterpret_cast<uint4*>(dst + 16) = make_uint4(w[4], w[5], w[6], w[7]);
    sc[(trow + dv) * 4 + blk] = (unsigned char)byte;
  }
}

// ------------------------------------------------------------------------------------------------ forward
__global__ __launch_bounds__(512, 2) void attn_mx_fwd_kernel(const unsigned char* __restrict__ Qc, const unsigned* __restrict__ Qs, const unsigned char* __restrict__ Kc,
                                                             const unsigned* __restrict__ Ks, const unsigned char* __restrict__ Vc, const unsigned* __restrict__ Vs,
                                                             unsigned short* __restrict__ O, int64_t ldo, int64_t Sq, int64_t Sk, int64_t Sk_pad) {
#if defined(__HIP_DEVICE_COMPILE__)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int K_OFF = 0, V_OFF = MX_TILE_BYTES, KS_OFF = 2 * MX_TILE_BYTES, VS_OFF = 2 * MX_TILE_BYTES + MX_SC_BYTES;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c16 = lane & 15, g4 = lane >> 4;
  const int head = blockIdx.y;
  const int64_t q0 = (int64_t)blockIdx.x * 256 + wid * 32;
  const int nt = (int)((Sk + MX_KV - 1) / MX_KV);

  // Q^ fragments (B operand) and scale bytes: chunks g and 4 + g of the lane's query row, the row's scale dword shifted down by g bytes
  i32x8_t qf[2];
  int qsc[2];
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    int64_t qr = q0 + 16 * g + c16;
    qr = qr < Sq ? qr : Sq - 1;
    const int64_t row = (int64_t)head * Sq + qr;
    const i32x4_t a0 = *reinterpret_cast<const i32x4_t*>(Qc + row * 128 + g4 * 16);
    const i32x4_t a1 = *reinterpret_cast<const i32x4_t*>(Qc + row * 128 + 64 + g4 * 16);
    qf[g] = __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7);
    qsc[g] = (int)(Qs[row] >> (8 * g4));
  }

  // LDS-DMA: a tile's K^ and V^T^ images are 16 pieces of 1 KiB (8 rows) each; wave w issues pieces 2 w and 2 w + 1 of both, waves 0-3 one
  // 256-byte piece of the scale dwords each.  Lane i of a piece: row 8 pc + (i >> 3), LDS chunk i & 7 <- source chunk (i & 7) ^ h(row).
  const __amdgpu_buffer_rsrc_t rk = __builtin_amdgcn_make_buffer_rsrc((void*)(Kc + (int64_t)head * Sk_pad * 128), 0, (unsigned)(Sk_pad * 128), 0x00020000);
  const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc((void*)(Vc + (int64_t)head * nt * MX_TILE_BYTES), 0, (unsigned)nt * MX_TILE_BYTES, 0x00020000);
  const __amdgpu_buffer_rsrc_t rks = __builtin_amdgcn_make_buffer_rsrc((void*)(Ks + (int64_t)head * Sk_pad), 0, (unsigned)(Sk_pad * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t rvs = __builtin_amdgcn_make_buffer_rsrc((void*)(Vs + (int64_t)head * nt * 128), 0, (unsigned)nt * MX_SC_BYTES, 0x00020000);
  const int prow = lane >> 3;  // row within a piece
  const unsigned k_voff = (unsigned)(prow * 128 + (((lane & 7) ^ ((wid & 3) | (((prow >> 1) & 1) << 2))) << 4));  // hK: (row >> 4) & 3 = (pc >> 1) & 3 = wid & 3
  unsigned v_voff[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) v_voff[j] = (unsigned)(prow * 128 + (((lane & 7) ^ (4 * j + (prow >> 1))) << 4));  // hV: (row >> 1) & 7 = 4 (pc & 1) + (prow >> 1)
  const unsigned s_voff = (unsigned)(lane * 4);
#define MX_DMA(T_, BUF_)                                                                                                                          \
  {                                                                                                                                                \
    char* const b_ = smem + (BUF_) * MX_BUF_BYTES;                                                                                                 \
    _Pragma("unroll") for (int j = 0; j < 2; ++j) {                                                                                               \
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rk, (mx_lds_ptr_t)(b_ + K_OFF + (2 * wid + j) * 1024), 16, k_voff,                                 \
                                               (unsigned)(T_) * MX_TILE_BYTES + (unsigned)(2 * wid + j) * 1024u, 0, 0);                            \
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rv, (mx_lds_ptr_t)(b_ + V_OFF + (2 * wid + j) * 1024), 16, v_voff[j],                              \
                                               (unsigned)(T_) * MX_TILE_BYTES + (unsigned)(2 * wid + j) * 1024u, 0, 0);                            \
    }                                                                                                                                              \
    if (wid < 2)                                                                                                                                   \
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rks, (mx_lds_ptr_t)(b_ + KS_OFF + wid * 256), 4, s_voff, (unsigned)(T_) * MX_SC_BYTES + wid * 256u, 0, 0); \
    else if (wid < 4)                                                                                                                              \
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rvs, (mx_lds_ptr_t)(b_ + VS_OFF + (wid - 2) * 256), 4, s_voff,                                     \
                                               (unsigned)(T_) * MX_SC_BYTES + (wid - 2) * 256u, 0, 0);                                             \
  }

  // fragment offsets.  K^: row kappa(tt, c) = 16 (c >> 2) + (c & 3) [+ 64 (tt >> 2) + 4 (tt & 3) as an immediate], chunks g, 4 + g XOR hK = (c >> 2) | (((c >> 1) & 1) << 2).
  // V^T^: row 16 T + c, chunks g, 4 + g XOR hV = (c >> 1) & 7.
  const int krow = 16 * (c16 >> 2) + (c16 & 3);
  const int hk = (c16 >> 2) | (((c16 >> 1) & 1) << 2), hv = (c16 >> 1) & 7;
  const int kb0 = krow * 128 + ((g4 ^ hk) << 4), kb1 = krow * 128 + (((4 + g4) ^ hk) << 4);
  const int vb0 = c16 * 128 + ((g4 ^ hv) << 4), vb1 = c16 * 128 + (((4 + g4) ^ hv) << 4);
  const int sh = 8 * g4;

  f32x4_t oacc[8][2], sc[8][2], negm[2];
#pragma unroll
  for (int g = 0; g < 2; ++g)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      negm[g][e] = 0.f;
#pragma unroll
      for (int T = 0; T < 8; ++T) oacc[T][g][e] = 0.f;
    }
  float m_run[2] = {0.f, 0.f}, lsum[2] = {0.f, 0.f};
  bool force = true;  // first tile: adopt its row max in either direction
  int pscale = 127 - MX_P_SHIFT;
  asm volatile("" : "+v"(pscale));  // the operand's scale byte lives in a VGPR like the others

  MX_DMA(0, 0)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  for (int t = 0; t < nt; ++t) {
    if (t + 1 < nt) MX_DMA(t + 1, (t + 1) & 1)
    const char* const buf = smem + (t & 1) * MX_BUF_BYTES;
    // ---- S^T - m = K^ . Q^^T - m: 8 sub-tiles x 2 query groups
#pragma unroll
    for (int tt = 0; tt < 8; ++tt) {
      const int ro = (64 * (tt >> 2) + 4 * (tt & 3)) * 128;
      const i32x4_t a0 = *reinterpret_cast<const i32x4_t*>(buf + K_OFF + ro + kb0);
      const i32x4_t a1 = *reinterpret_cast<const i32x4_t*>(buf + K_OFF + ro + kb1);
      const i32x8_t kf = __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7);
      const int ksc = (int)(*reinterpret_cast<const unsigned*>(buf + KS_OFF + (ro >> 5) + krow * 4) >> sh);
#pragma unroll
      for (int g = 0; g < 2; ++g) sc[tt][g] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(kf, qf[g], negm[g], 0, 0, 0, ksc, 0, qsc[g]);
    }
    // ---- softmax.  Register r of sc[tt][g] is key 64 (tt >> 2) + 16 g4 + 4 (tt & 3) + r of the tile.
    if (t == nt - 1 && (int64_t)nt * MX_KV > Sk) {
      const int left = (int)(Sk - (int64_t)t * MX_KV);
#pragma unroll
      for (int tt = 0; tt < 8; ++tt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (64 * (tt >> 2) + 16 * g4 + 4 * (tt & 3) + r >= left) {
            sc[tt][0][r] = -1e30f;
            sc[tt][1][r] = -1e30f;
          }
    }
    float d[2];
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      float mx = sc[0][g][0];
#pragma unroll
      for (int tt = 0; tt < 8; ++tt)
#pragma unroll
        for (int r = 0; r < 4; ++r) mx = fmaxf(mx, sc[tt][g][r]);
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      d[g] = force ? mx : fmaxf(mx, 0.f);
    }
    if (force || __any(fmaxf(d[0], d[1]) > 0.f)) {  // some row's max grew (or first tile): everything at the old reference moves to the new one
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        m_run[g] += d[g];
        if (!force) {
          const float al = __builtin_amdgcn_exp2f(-d[g]);
          lsum[g] *= al;
#pragma unroll
          for (int T = 0; T < 8; ++T)
#pragma unroll
            for (int e = 0; e < 4; ++e) oacc[T][g][e] *= al;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) negm[g][e] = -m_run[g];
#pragma unroll
        for (int tt = 0; tt < 8; ++tt)
#pragma unroll
          for (int e = 0; e < 4; ++e) sc[tt][g][e] -= d[g];
      }
      force = false;
    }
    i32x8_t pw[2];  // [query group]: 32 e4m3 codes of P * 2^8 in k-slot order = the B operand of the PV instruction
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
      for (int tt = 0; tt < 8; ++tt) {
        const float p0 = __builtin_amdgcn_exp2f(sc[tt][g][0]), p1 = __builtin_amdgcn_exp2f(sc[tt][g][1]);
        const float p2 = __builtin_amdgcn_exp2f(sc[tt][g][2]), p3 = __builtin_amdgcn_exp2f(sc[tt][g][3]);
        lsum[g] += (p0 + p1) + (p2 + p3);
        constexpr float kShift = (float)(1 << MX_P_SHIFT);
        int w = 0;
        w = __builtin_amdgcn_cvt_pk_fp8_f32(p0 * kShift, p1 * kShift, w, false);
        w = __builtin_amdgcn_cvt_pk_fp8_f32(p2 * kShift, p3 * kShift, w, true);
        pw[g][tt] = w;
      }
    // ---- O^T += V^T^ . P^: 8 dv tiles x 2 query groups
#pragma unroll
    for (int T = 0; T < 8; ++T) {
      const i32x4_t a0 = *reinterpret_cast<const i32x4_t*>(buf + V_OFF + T * 2048 + vb0);
      const i32x4_t a1 = *reinterpret_cast<const i32x4_t*>(buf + V_OFF + T * 2048 + vb1);
      const i32x8_t vf = __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7);
      const int vsc = (int)(*reinterpret_cast<const unsigned*>(buf + VS_OFF + (16 * T + c16) * 4) >> sh);
#pragma unroll
      for (int g = 0; g < 2; ++g) oacc[T][g] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(vf, pw[g], oacc[T][g], 0, 0, 0, vsc, 0, pscale);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
#undef MX_DMA

#pragma unroll
  for (int g = 0; g < 2; ++g) {
    float l_run = lsum[g];
    l_run += __shfl_xor(l_run, 16, 64);
    l_run += __shfl_xor(l_run, 32, 64);
    const float inv = 1.0f / l_run;
    const int64_t qrow = q0 + 16 * g + c16;
    if (qrow < Sq) {
      unsigned short* op = O + qrow * ldo + (int64_t)head * 128 + 4 * g4;
#pragma unroll
      for (int T = 0; T < 8; ++T) {
        uint2 pk;
        pk.x = pack_bf2(oacc[T][g][0] * inv, oacc[T][g][1] * inv);
        pk.y = pack_bf2(oacc[T][g][2] * inv, oacc[T][g][3] * inv);
        *reinterpret_cast<uint2*>(op + 16 * T) = pk;
      }
    }
  }
#endif
}

static bool mx_shape_ok(int64_t Sq, int64_t Sk, int H) { return Sq >= 0 && Sk >= 0 && Sq < (1ll << 24) && Sk < (1ll << 24) && H > 0 && H <= 1024; }

}  // namespace x2v

using namespace x2v;

extern "C" __attribute__((visibility("default"))) int x2v_attn_mx_sizes(int64_t Sq, int64_t Sk, int H, int64_t* sizes) {
  X2V_REQUIRE(sizes != nullptr, X2V_E_ARG, "attn_mx_sizes: null pointer");
  X2V_REQUIRE(mx_shape_ok(Sq, Sk, H), X2V_E_SHAPE, "attn_mx_sizes: Sq=%lld Sk=%lld H=%d (0 <= S < 2^24, 1 <= H <= 1024)", (long long)Sq, (long long)Sk, H);
  const int64_t nt = (Sk + MX_KV - 1) / MX_KV, skp = nt * MX_KV, nch = (Sk + MX_MEAN_CHUNK - 1) / MX_MEAN_CHUNK;
  sizes[0] = (int64_t)H * Sq * 128;
  sizes[1] = (int64_t)H * Sq * 4;
  sizes[2] = (int64_t)H * skp * 128;
  sizes[3] = (int64_t)H * skp * 4;
  sizes[4] = (int64_t)H * nt * MX_TILE_BYTES;
  sizes[5] = (int64_t)H * nt * MX_SC_BYTES;
  sizes[6] = (1 + nch) * (int64_t)H * 128 * 4;
  return X2V_OK;
}

extern "C" __attribute__((visibility("default"))) int x2v_attn_mx_kmean_f32(const void* k, int64_t ldk, float* kmean, int64_t Sk, int H, void* stream) {
  X2V_REQUIRE(k && kmean, X2V_E_ARG, "attn_mx_kmean: null pointer");
  X2V_REQUIRE(mx_shape_ok(0, Sk, H) && Sk > 0, X2V_E_SHAPE, "attn_mx_kmean: Sk=%lld H=%d (0 < Sk < 2^24, 1 <= H <= 1024)", (long long)Sk, H);
  X2V_REQUIRE(ldk % 2 == 0 && ldk >= (int64_t)H * 128 && ((uintptr_t)k % 4) == 0 && ((uintptr_t)kmean % 16) == 0, X2V_E_ALIGN,
              "attn_mx_kmean: rows of k 4-byte aligned (ldk even, >= H*128), kmean 16-byte aligned");
  const int cols = H * 128, nch = (int)((Sk + MX_MEAN_CHUNK - 1) / MX_MEAN_CHUNK);
  float* part = kmean + cols;
  hipLaunchKernelGGL(mx_kmean_part_kernel, dim3((unsigned)nch, (unsigned)H), dim3(64), 0, (hipStream_t)stream, (const unsigned short*)k, ldk, part, Sk, cols);
  X2V_LAUNCH_CHECK("attn_mx_kmean part launch");
  hipLaunchKernelGGL(mx_kmean_final_kernel, dim3((unsigned)H), dim3(128), 0, (hipStream_t)stream, (const float*)part, kmean, nch, cols, (float)Sk);
  X2V_LAUNCH_CHECK("attn_mx_kmean final launch");
  return X2V_OK;
}

extern "C" __attribute__((visibility("default"))) int x2v_attn_mx_quant_qk(const void* x, int64_t ldx, const float* mean, int smooth, float scale, void* codes,
                                                                          void* scales, int64_t S, int64_t S_pad, int H, void* stream) {
  X2V_REQUIRE(x && codes && scales, X2V_E_ARG, "attn_mx_quant_qk: null pointer");
  X2V_REQUIRE(smooth == 0 || mean != nullptr, X2V_E_ARG, "attn_mx_quant_qk: smoothing needs the column mean");
  X2V_REQUIRE(mx_shape_ok(S, S_pad, H) && S_pad >= S, X2V_E_SHAPE, "attn_mx_quant_qk: S=%lld S_pad=%lld H=%d (0 <= S <= S_pad < 2^24, 1 <= H <= 1024)", (long long)S,
              (long long)S_pad, H);
  X2V_REQUIRE(ldx % 8 == 0 && ldx >= (int64_t)H * 128 && aligned16(x) && aligned16(codes) && ((uintptr_t)scales % 4) == 0 && (mean == nullptr || aligned16(mean)),
              X2V_E_ALIGN, "attn_mx_quant_qk: rows of x 16-byte aligned (ldx %% 8 == 0, >= H*128), codes and mean 16-byte, scales 4-byte aligned");
  if (S_pad == 0) return X2V_OK;
  const int64_t total = S_pad * H * 16;
  const unsigned blocks = (unsigned)std::min<int64_t>((total + 255) / 256, 256 * 32);
  hipLaunchKernelGGL(mx_quant_qk_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const unsigned short*)x, ldx, smooth ? mean : nullptr, scale,
                     (unsigned char*)codes, (unsigned*)scales, S, S_pad, H);
  X2V_LAUNCH_CHECK("attn_mx_quant_qk launch");
  return X2V_OK;
}

extern "C" __attribute__((visibility("default"))) int x2v_attn_mx_quant_vt(const void* v, int64_t ldv, void* codes, void* scales, int64_t Sk, int H, void* stream) {
  X2V_REQUIRE(v && codes && scales, X2V_E_ARG, "attn_mx_quant_vt: null pointer");
  X2V_REQUIRE(mx_shape_ok(0, Sk, H) && Sk > 0, X2V_E_SHAPE, "attn_mx_quant_vt: Sk=%lld H=%d (0 < Sk < 2^24, 1 <= H <= 1024)", (long long)Sk, H);
  X2V_REQUIRE(ldv % 8 == 0 && ldv >= (int64_t)H * 128 && aligned16(v) && aligned16(codes) && ((uintptr_t)scales % 4) == 0, X2V_E_ALIGN,
              "attn_mx_quant_vt: rows of v 16-byte aligned (ldv %% 8 == 0, >= H*128), codes 16-byte, scales 4-byte aligned");
  const unsigned nt = (unsigned)((Sk + MX_KV - 1) / MX_KV);
  hipLaunchKernelGGL(mx_quant_vt_kernel, dim3(nt, (unsigned)H), dim3(256), 0, (hipStream_t)stream, (const unsigned short*)v, ldv, (unsigned char*)codes,
                     (unsigned char*)scales, Sk);
  X2V_LAUNCH_CHECK("attn_mx_quant_vt launch");
  return X2V_OK;
}

extern "C" __attribute__((visibility("default"))) int x2v_attn_mx_fwd(const void* q_codes, const void* q_scales, const void* k_codes, const void* k_scales,
                                                                     const void* vt_codes, const void* vt_scales, void* o, int64_t ldo, int64_t Sq, int64_t Sk, int H,
                                                                     void* stream) {
  X2V_REQUIRE(q_codes && q_scales && k_codes && k_scales && vt_codes && vt_scales && o, X2V_E_ARG, "attn_mx_fwd: null pointer");
  X2V_REQUIRE(mx_shape_ok(Sq, Sk, H), X2V_E_SHAPE, "attn_mx_fwd: Sq=%lld Sk=%lld H=%d (0 <= S < 2^24, 1 <= H <= 1024)", (long long)Sq, (long long)Sk, H);
  X2V_REQUIRE(Sk > 0, X2V_E_SHAPE, "attn_mx_fwd: no keys (softmax over an empty set)");
  X2V_REQUIRE(aligned16(q_codes) && aligned16(k_codes) && aligned16(vt_codes) && ((uintptr_t)q_scales % 4) == 0 && ((uintptr_t)k_scales % 4) == 0 &&
                  ((uintptr_t)vt_scales % 4) == 0 && ldo % 4 == 0 && ldo >= (int64_t)H * 128 && ((uintptr_t)o % 8) == 0,
              X2V_E_ALIGN, "attn_mx_fwd: code buffers 16-byte, scale tables 4-byte aligned; rows of o 8-byte aligned (ldo %% 4 == 0, >= H*128)");
  if (Sq == 0) return X2V_OK;
  int rc = ensure_dynamic_lds((const void*)attn_mx_fwd_kernel, MX_LDS_BYTES, "attn mx attr");
  if (rc != X2V_OK) return rc;
  const int64_t skp = (Sk + MX_KV - 1) / MX_KV * MX_KV;
  hipLaunchKernelGGL(attn_mx_fwd_kernel, dim3((unsigned)((Sq + 255) / 256), (unsigned)H), dim3(512), MX_LDS_BYTES, (hipStream_t)stream, (const unsigned char*)q_codes,
                     (const unsigned*)q_scales, (const unsigned char*)k_codes, (const unsigned*)k_scales, (const unsigned char*)vt_codes, (const unsigned*)vt_scales,
                     (unsigned short*)o, ldo, Sq, Sk, skp);
  X2V_LAUNCH_CHECK("attn_mx_fwd launch");
  return X2V_OK;
}
