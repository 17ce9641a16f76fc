// Append to a V^T cache: rows of a row-major v written into the key columns [key0, key0 + S) of an existing V^T [H][ldvt/64][128][64] — the KV cache
// of the autoregressive Wan (CausVid) driver, whose blocks start at token offsets that are no multiple of the 64-key tile (4680 % 64 = 8, 10 800 % 64 =
// 48, odd for some i2v grids).  x2v_transpose_heads_bf16 (attn.hip) writes a whole sequence from key 0 and zero-fills its tail; this kernel writes
// only its own key columns and leaves every other byte of the cache as it was.
//
// ORDERING.  Appends to one cache, and the attention launches that read it, are ordered on ONE stream: an append's first and last tile hold keys that
// an earlier append wrote (and that a later one will write), a tile is touched by as many appends as blocks meet in it, and attention reads what
// the appends left.  Nothing in here synchronises two appends to the same tile; stream order does.
#include "x2v_common.h"

namespace x2v {

constexpr int KA_D = 128;   // head dim
constexpr int KA_KV = 64;   // keys per V^T tile

// One workgroup per (touched 64-key tile, head), through LDS, as transpose_heads_kernel.  Tile t = key0 / 64 + blockIdx.x holds the keys
// [lo, hi) of the range (tile-local): interior tiles have lo = 0, hi = 64 and run that kernel's 16-byte store path; the first and last tile store only
// the 16-byte words (8 keys of one dv) that lie inside [lo, hi).  A word that STRADDLES lo or hi (only when key0 or key0 + S is no multiple of 8,
// EDGE = true) is written by the one thread that owns it with 2-byte stores of its in-range keys: nothing is read back, no two threads touch the
// same word.  EDGE = false (key0 % 8 == 0 and (key0 + S) % 8 == 0: every 480p / 720p t2v offset) carries no straddle code at all.
// v rows outside [0, S) are never read: a tile row outside [lo, hi) stays zero in LDS and is never stored.
template <bool EDGE>
__global__ __launch_bounds__(256) void transpose_heads_append_kernel(const unsigned short* __restrict__ V, int64_t ldv, unsigned short* __restrict__ VT, int64_t ldvt,
                                                                     int64_t key0, int64_t S) {
  __shared__ unsigned short tile[KA_KV][KA_D + 2];
  const int head = blockIdx.y;
  const int64_t t = key0 / KA_KV + blockIdx.x;
  const int64_t k0 = t * KA_KV;
  const int lo = key0 > k0 ? (int)(key0 - k0) : 0;
  const int hi = key0 + S < k0 + KA_KV ? (int)(key0 + S - k0) : KA_KV;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int id = i * 256 + threadIdx.x;
    const int row = id >> 4, c = id & 15;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (row >= lo && row < hi) v = *reinterpret_cast<const uint4*>(V + (k0 + row - key0) * ldv + (int64_t)head * KA_D + c * 8);
    unsigned short* d = &tile[row][c * 8];
    d[0] = (unsigned short)(v.x & 0xffff); d[1] = (unsigned short)(v.x >> 16);
    d[2] = (unsigned short)(v.y & 0xffff); d[3] = (unsigned short)(v.y >> 16);
    d[4] = (unsigned short)(v.z & 0xffff); d[5] = (unsigned short)(v.z >> 16);
    d[6] = (unsigned short)(v.w & 0xffff); d[7] = (unsigned short)(v.w >> 16);
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int id = i * 256 + threadIdx.x;
    const int dv = id >> 3, kc = id & 7;
    unsigned short* dst = VT + (((int64_t)head * (ldvt >> 6) + t) * KA_D + dv) * KA_KV + kc * 8;
    if (kc * 8 >= lo && kc * 8 + 8 <= hi) {
      unsigned w[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) w[e] = (unsigned)tile[kc * 8 + 2 * e][dv] | ((unsigned)tile[kc * 8 + 2 * e + 1][dv] << 16);
      *reinterpret_cast<uint4*>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
    } else if (EDGE && kc * 8 < hi && kc * 8 + 8 > lo) {
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (kc * 8 + e >= lo && kc * 8 + e < hi) dst[e] = tile[kc * 8 + e][dv];
    }
  }
}

}  // namespace x2v
using namespace x2v;

extern "C" __attribute__((visibility("default"))) int x2v_transpose_heads_append_bf16(const void* v, int64_t ldv, void* vt, int64_t ldvt, int64_t key0, int64_t S, int H,
                                                                                      void* stream) {
  X2V_REQUIRE(v && vt, X2V_E_ARG, "transpose_heads_append: null pointer");
  X2V_REQUIRE(ldvt >= 0 && ldvt % 64 == 0 && key0 >= 0 && S >= 0 && key0 <= ldvt && S <= ldvt - key0 && H >= 1 && H <= 65535, X2V_E_SHAPE,
              "transpose_heads_append: bad shape key0=%lld S=%lld ldvt=%lld H=%d (ldvt must be a multiple of 64 and >= key0 + S)", (long long)key0, (long long)S,
              (long long)ldvt, H);
  X2V_REQUIRE(aligned16(v) && aligned16(vt) && ldv % 8 == 0, X2V_E_ALIGN, "transpose_heads_append: 16-byte alignment (v, vt, and ldv a multiple of 8)");
  X2V_REQUIRE(ldv >= (int64_t)H * KA_D, X2V_E_SHAPE, "transpose_heads_append: token stride ldv=%lld smaller than H*128", (long long)ldv);
  if (S == 0) return X2V_OK;
  const int64_t tiles = (key0 + S - 1) / KA_KV - key0 / KA_KV + 1;
  X2V_REQUIRE(tiles < (1ll << 31), X2V_E_SHAPE, "transpose_heads_append: %lld key tiles in one launch", (long long)tiles);
  const dim3 grid((unsigned)tiles, (unsigned)H);
  if (key0 % 8 == 0 && (key0 + S) % 8 == 0)
    hipLaunchKernelGGL(transpose_heads_append_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, (const unsigned short*)v, ldv, (unsigned short*)vt, ldvt, key0, S);
  else
    hipLaunchKernelGGL(transpose_heads_append_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, (const unsigned short*)v, ldv, (unsigned short*)vt, ldvt, key0, S);
  X2V_LAUNCH_CHECK("transpose_heads_append launch");
  return X2V_OK;
}
