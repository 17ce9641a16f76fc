// The steps the encoder towers' attention kernels share: attn_f16_d80_kernel (clip.hip), attn_d64_relbias_kernel (t5.hip) and attn_f16_causal_kernel<D>
// (txt_enc.hip) are built from them; the element type comes from RowsElem<T> (gemm_rows.h).  What differs stays in those files: T5's bias row and its
// per-length bodies, the causal kernel's rotary paths, diagonal mask and online softmax, the d80 kernel's 17 + 1 tiles.
//
// The convention, for a workgroup of 4 waves on 64 query rows and v_mfma_f32_16x16x32 (lane = 16 g4 + c16):
//   LDS — K as [key][D + 8] (16-byte aligned rows, the 8 pad elements never read), V transposed as [d][keys + pad]; both zero-filled from the sequence's
//     last key on, so rows of another sequence are never read.
//   queries — lane column c16 of wave `wid` is query qb 64 + wid 16 + c16; its fragment of k-step ks is elements 32 ks + 8 g4 .. + 7 of the row.  A query
//     past the end reads the sequence's last row and is never stored.
//   scores — S^T = K . Q^T: the A operand of key tile t is row 16 t + c16 of K, same elements.  Accumulator element e of lane (g4, c16) is
//     q[c16] . k[16 t + 4 g4 + e]: a query's scores sit in the 4 lanes that share its column, which quad_max / quad_sum reduce over.
//   PV — O^T = V^T . P^T takes the probabilities as the B operand without lane movement: k-step kk packs the lane's key tiles 2 kk (elements 0..3) and
//     2 kk + 1 (4..7), so element j of lane group g4 is key 32 kk + 4 g4 + j (j < 4) or 32 kk + 16 + 4 g4 + j - 4.  The V^T fragment reads the same keys
//     of row 16 c + c16: two 8-byte reads 16 keys apart.  Element e of o[c] in lane (g4, c16) is output column 16 c + 4 g4 + e of query c16.
//   Everything between the two products is fp32; the output is o * (1 / sum), rounded once.
#pragma once
#include <algorithm>

#include "gemm_rows.h"
#include "x2v_common.h"

namespace x2v {

// ---- device steps ----------------------------------------------------------------------------------------------------------------------------------------
struct EncLanes {
  int tid, wid, c16, g4;
};
__device__ __forceinline__ EncLanes enc_lanes() {
  const int tid = threadIdx.x, lane = tid & 63;
  return {tid, tid >> 6, lane & 15, lane >> 4};
}
__device__ __forceinline__ int enc_query(const EncLanes& L, int qb) { return qb * 64 + L.wid * 16 + L.c16; }
__device__ __forceinline__ int enc_read_row(int q, int len) { return min(q, len - 1); }

// KS full k-steps of this lane's query row
template <typename T, int KS>
__device__ __forceinline__ void load_q(const T* __restrict__ qrow, int g4, typename RowsElem<T>::v8* qf) {
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) qf[ks] = *reinterpret_cast<const typename RowsElem<T>::v8*>(qrow + 32 * ks + 8 * g4);
}

// NROWS K rows of width D from key k0 on (`src` = key 0 at this head's k columns) → Ks [NROWS][KP], 16-byte chunks, zero from key `len` on
template <typename T, int D, int NROWS, int KP>
__device__ __forceinline__ void stage_k(T* Ks, const T* __restrict__ src, int64_t ld, int k0, int len, int tid) {
  typedef typename RowsElem<T>::v8 v8;
  for (int i = tid; i < NROWS * (D / 8); i += 256) {
    const int key = i / (D / 8), ch = i % (D / 8);
    v8 v = {};
    if (k0 + key < len) v = *reinterpret_cast<const v8*>(src + (int64_t)(k0 + key) * ld + ch * 8);
    *reinterpret_cast<v8*>(Ks + key * KP + ch * 8) = v;
  }
}

// NKEYS V rows from key k0 on → Vt [D][VP] transposed, zero from key `len` on
template <typename T, int D, int NKEYS, int VP>
__device__ __forceinline__ void stage_vt(T* Vt, const T* __restrict__ src, int64_t ld, int k0, int len, int tid) {
  typedef typename RowsElem<T>::v8 v8;
  for (int i = tid; i < NKEYS * (D / 8); i += 256) {
    const int ch = i / NKEYS, key = i % NKEYS;  // consecutive lanes: consecutive keys of one V^T row group
    v8 v = {};
    if (k0 + key < len) v = *reinterpret_cast<const v8*>(src + (int64_t)(k0 + key) * ld + ch * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) Vt[(ch * 8 + e) * VP + key] = v[e];
  }
}

// scores of key tile t: KS full k-steps, and with HALF a last one of 16 elements (lane groups 2 and 3 hold zeros in both operands; qf[KS] is theirs)
template <typename T, int KS, int KP, bool HALF = false>
__device__ __forceinline__ f32x4_t score_tile(const T* Ks, int t, const EncLanes& L, const typename RowsElem<T>::v8* qf) {
  typedef typename RowsElem<T>::v8 v8;
  const T* kr = Ks + (16 * t + L.c16) * KP + L.g4 * 8;
  f32x4_t a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) a = RowsElem<T>::mfma(*reinterpret_cast<const v8*>(kr + 32 * ks), qf[ks], a);
  if constexpr (HALF) {
    v8 k2 = {};
    if (L.g4 < 2) k2 = *reinterpret_cast<const v8*>(kr + 32 * KS);
    a = RowsElem<T>::mfma(k2, qf[KS], a);
  }
  return a;
}

// over the 4 lanes that share a query's column
__device__ __forceinline__ float quad_max(float v) {
  v = fmaxf(v, __shfl_xor(v, 16, 64));
  return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float quad_sum(float v) {
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}

// k-step kk of O^T += V^T . P^T over DC tiles of 16 output columns: p_lo / p_hi are the lane's probabilities of key tiles 2 kk / 2 kk + 1
template <typename T, int DC, int VP>
__device__ __forceinline__ void pv_step(const T* Vt, int kk, const f32x4_t& p_lo, const f32x4_t& p_hi, const EncLanes& L, f32x4_t* o) {
  typedef typename RowsElem<T>::v8 v8;
  typedef typename RowsElem<T>::v4 v4;
  v8 pb;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    pb[e] = (T)p_lo[e];
    pb[4 + e] = (T)p_hi[e];
  }
#pragma unroll
  for (int c = 0; c < DC; ++c) {
    const T* vr = Vt + (16 * c + L.c16) * VP + 32 * kk + 4 * L.g4;
    const v4 lo = *reinterpret_cast<const v4*>(vr), hi = *reinterpret_cast<const v4*>(vr + 16);
    const v8 vf = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    o[c] = RowsElem<T>::mfma(vf, pb, o[c]);
  }
}

// `op` = the query's output row at this head's columns
template <typename T, int DC>
__device__ __forceinline__ void store_out(T* op, const f32x4_t* o, float inv, int g4) {
  typedef typename RowsElem<T>::v4 v4;
#pragma unroll
  for (int c = 0; c < DC; ++c) {
    v4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = (T)(o[c][e] * inv);
    *reinterpret_cast<v4*>(op + 16 * c + 4 * g4) = r;
  }
}

// ---- packed sequences (host) -----------------------------------------------------------------------------------------------------------------------------
constexpr int ENC_MAXBATCH = 8;  // sequences of one packed launch
constexpr int ENC_MAXLEN = 512;  // tokens of one sequence

// The sequence bounds as a kernel argument: no device copy, no sync.
struct PackedSeqs {
  int cu[ENC_MAXBATCH + 1];
};

// batch 1..ENC_MAXBATCH sequences of 1..max_len tokens each, cu_seqlens (not null) increasing from >= 0: → seqs, the longest length.  `limit` ends the
// message of a sequence beyond max_len ("... more than the <max_len> <limit>").
static inline int packed_seqs_check(const char* who, const int* cu_seqlens, int batch, int max_len, const char* limit, PackedSeqs* seqs, int* longest) {
  X2V_REQUIRE(batch >= 1 && batch <= ENC_MAXBATCH, X2V_E_SHAPE, "%s: batch=%d must be 1..%d packed sequences", who, batch, ENC_MAXBATCH);
  X2V_REQUIRE(cu_seqlens[0] >= 0, X2V_E_SHAPE, "%s: cu_seqlens[0]=%d is negative", who, cu_seqlens[0]);
  *seqs = PackedSeqs{};
  *longest = 0;
  for (int b = 0; b <= batch; ++b) seqs->cu[b] = cu_seqlens[b];
  for (int b = 0; b < batch; ++b) {
    const int64_t len = (int64_t)seqs->cu[b + 1] - seqs->cu[b];
    X2V_REQUIRE(len >= 1, X2V_E_SHAPE, "%s: cu_seqlens must increase (sequence %d has %lld tokens)", who, b, (long long)len);
    X2V_REQUIRE(len <= max_len, X2V_E_SHAPE, "%s: sequence %d has %lld tokens, more than the %d %s", who, b, (long long)len, max_len, limit);
    *longest = std::max(*longest, (int)len);
  }
  return X2V_OK;
}

}  // namespace x2v
