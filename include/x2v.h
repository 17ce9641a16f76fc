/*
 * x2v.h — C-ABI of libx2v_hip.so: hand-written gfx950 (MI355X / CDNA4) kernels for the LightX2V DiT
 * denoise-step hot path.  This is the drop-in boundary: plain pointers, sizes and a
 * hipStream_t; no torch types.  Each entry point names the reference call site it replaces
 * (paths relative to /root/reference/lightx2v/).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless stated; bf16 tensors are passed as `const void*`/`void*`
 *     (raw bfloat16 bits, little-endian); fp8 tensors are OCP e4m3fn bytes (gfx950 format, not fnuz)
 *   - `ld*` / strides are in ELEMENTS; rows must be 16-byte aligned (ld % 8 == 0 for bf16)
 *   - `stream` is a hipStream_t passed as void* (the Python shim passes
 *     torch.cuda.current_stream().cuda_stream); every call is asynchronous, re-entrant, never
 *     synchronises the device and keeps no mutable global state besides the thread-local error string
 *   - return value: X2V_OK (0) or a negative X2V_E_* code; x2v_last_error() then describes it.
 *     No exceptions or exit() cross the ABI (reference convention: Python exceptions / TORCH_CHECK →
 *     RuntimeError, lightx2v_kernel/csrc/gemm/mxfp8_scaled_mm_kernels_sm120.cu:13-25; the shim raises
 *     RuntimeError from the code)
 */
#ifndef X2V_H
#define X2V_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define X2V_OK 0
#define X2V_E_SHAPE (-1)  /* unsupported shape / size constraint violated */
#define X2V_E_ALIGN (-2)  /* pointer or leading dimension not 16-byte aligned */
#define X2V_E_ARCH (-3)   /* device is not gfx950 */
#define X2V_E_HIP (-4)    /* a HIP runtime call failed */
#define X2V_E_ARG (-5)    /* null pointer / bad enum */

/* GEMM epilogues (x2v_gemm_bf16 / x2v_gemm_fp8) */
#define X2V_EPI_NONE 0      /* y = bf16(acc + bias) */
#define X2V_EPI_GELU_TANH 1 /* y = bf16(gelu_tanh(bf16(acc + bias)))          (transformer_infer.py:488-492) */
#define X2V_EPI_RESIDUAL 2  /* y = bf16(resid + bf16(bf16(acc + bias) * gate)) (transformer_infer.py:402,468,503);
                               gate may be NULL (plain add); y may alias resid */
#define X2V_EPI_SILU 3      /* y = bf16(silu(bf16(acc + bias)))                (pre_infer.py:74-76) */

/* rounding model of the norm kernels */
#define X2V_ROUND_FP32 0 /* fp32 statistics, one final rounding (what sgl_kernel.rmsnorm does on the reference's GPU path) */
#define X2V_ROUND_REF 1  /* reproduce the reference's bf16 torch chain rounding for rounding (rms_norm_weight.py:111-113) */

/* Library / device. x2v_init checks that `device` is gfx950 and caches its properties. */
int x2v_init(int device);
const char* x2v_last_error(void);
const char* x2v_version(void);
int x2v_device_info(int device, int* cu_count, int* lds_bytes_per_cu, char* arch_name, int arch_name_len);

/* The process-wide A/B switches this library reads ONCE from the environment, as "NAME=value NAME=value ..." (effective values, defaults
 * included): X2V_GEMM_CONTINUOUS, X2V_GEMM_FP8_CONTINUOUS (kernel forms, same bits), X2V_ATTN_MAP, X2V_ATTN_ROT (launch forms of
 * x2v_attn_fwd_bf16_vt; ROT changes the key-walk order, i.e. low bits).  The reference has no counterpart (its kernel choice is the config
 * string, utils/registry_factory.py:47-56); bench.py prints the string into its JSON line so that a stray variable on a rank is visible. */
int x2v_switches(char* buf, int buf_len);

/* y[M,D] = x * rsqrt(mean(x^2) + eps) * w     — replaces RMSWeight/RMSWeightSgl.apply
 * (common/ops/norm/rms_norm_weight.py:53-118; sgl_kernel.rmsnorm :102-108).  D % 8 == 0, D <= 16384.
 * y may alias x. */
int x2v_rmsnorm_bf16(const void* x, int64_t ldx, const void* w, void* y, int64_t ldy, int64_t M, int D, float eps, int round_mode,
                     void* stream);

/* y[M,D] = LN(x; w,b,eps) [* (1 + scale) + shift]   — replaces LNWeight.apply (layer_norm_weight.py:78-111)
 * fused with the adaLN modulate `norm_out.mul_(1 + scale).add_(shift)` (transformer_infer.py:329-334,
 * 481-484; post_infer.py:24-28).  w,b (affine, norm3) and scale,shift (modulate, [D] bf16) are each
 * optional (NULL).  Rounding follows the reference chain: bf16 after LN, after the multiply, after the add. */
int x2v_layernorm_bf16(const void* x, int64_t ldx, const void* w, const void* b, const void* scale, const void* shift, void* y, int64_t ldy,
                       int64_t M, int D, float eps, void* stream);

/* Same, selecting the kernel form (tuning / validation hook): 0 = by shape (what x2v_layernorm_bf16 does: the persistent
 * "streaming" kernel — next row prefetched under the current row's reductions, per-channel operands resident in registers —
 * when 512 < D <= 8192 and M is at least twice the resident grid, else one block per row), 1 = one block per row,
 * 2 = streaming (X2V_E_SHAPE outside 512 < D <= 8192).  The forms are bit-identical. */
int x2v_layernorm_bf16_variant(const void* x, int64_t ldx, const void* w, const void* b, const void* scale, const void* shift, void* y, int64_t ldy,
                               int64_t M, int D, float eps, int variant, void* stream);

/* In-place q,k <- RoPE3D(RMSNorm_D(q|k)) for Wan self-attention — replaces rms_norm_weight.py apply on
 * q and k (transformer_infer.py:341-342) + compute_freqs/apply_rotary_emb (wan/infer/utils.py:7-20,
 * 107-115).  q,k: [S, H*128] bf16 with token stride ldq/ldk; wq,wk: [H*128] bf16 (NULL = skip the norm);
 * rope_cs: float2 (cos,sin) table [1024][64] = the reference's `freqs` [1024,64] (pre_infer.py:12-19),
 * columns [0,22) t-axis, [22,43) h-axis, [43,64) w-axis; token s has grid position
 * ((s0+s) / (gh*gw), ((s0+s) / gw) % gh, (s0+s) % gw); tokens with s0+s >= gf*gh*gw are rotated by 1
 * (compute_freqs_dist's ones padding, utils.py:78-83).  s0 = first global token of this rank's shard. */
int x2v_rmsnorm_rope_bf16(void* q, int64_t ldq, void* k, int64_t ldk, const void* wq, const void* wk, const void* rope_cs, int64_t S, int H,
                          int64_t s0, int gf, int gh, int gw, float eps, int round_mode, void* stream);

/* Same, with q additionally multiplied by q_out_scale inside its single final rounding (k untouched).  Used by the fused
 * block driver to hand the attention kernel a q that already carries softmax_scale * log2(e)
 * (X2V_ATTN_Q_PRESCALED): numerically one rounding of the scaled value instead of one rounding of the unscaled one. */
int x2v_rmsnorm_rope_scaled_bf16(void* q, int64_t ldq, void* k, int64_t ldk, const void* wq, const void* wk, const void* rope_cs, int64_t S, int H,
                                 int64_t s0, int gf, int gh, int gw, float eps, int round_mode, float q_out_scale, void* stream);

/* Same, selecting the kernel form (tuning / validation hook; bit-identical results): 0 = by shape, 1 = one block per (token, q|k)
 * row, 2 = persistent streaming kernel (a token's q and k rows back to back, its 64 rotation factors gathered once into LDS, the
 * next row prefetched under the reduction; D <= 8192). */
int x2v_rmsnorm_rope_scaled_bf16_variant(void* q, int64_t ldq, void* k, int64_t ldk, const void* wq, const void* wk, const void* rope_cs, int64_t S,
                                         int H, int64_t s0, int gf, int gh, int gw, float eps, int round_mode, float q_out_scale, int variant,
                                         void* stream);

/* x2v_rmsnorm_rope_scaled_bf16 out of place into N-blocked outputs: q/k [S, H*128] are read, column e of token s is written to
 * q_out / k_out[(e / block_cols) * block_stride + s * ldo + e % block_cols] — the seq->head send buffer [N_ranks][S/N][(H/N) d] of the
 * Ulysses exchange (block_cols = (H/N)*128), replacing the reference's view + transpose + contiguous copy (all2all.py:29-33). */
int x2v_rmsnorm_rope_blocked_bf16(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* wq, const void* wk, const void* rope_cs, void* q_out, void* k_out,
                                  int64_t ldo, int block_cols, int64_t block_stride, int64_t S, int H, int64_t s0, int gf, int gh, int gw, float eps, int round_mode,
                                  float q_out_scale, void* stream);

/* In-place per-head RMSNorm (d = 128) of q and k [L, H*128] (token strides ldq/ldk, e.g. the column blocks of a fused
 * QKV GEMM output), followed for tokens < l_rope by the real-valued RoPE x*cos + rotate_half(x)*sin with bf16 tables
 * cos/sin [l_rope, 128] — replaces RMSWeightSgl.apply on [L,H,128] (rms_norm_weight.py:102-113; hunyuan
 * transformer_infer.py:271-272,289-290,338-339) + hunyuan/infer/utils_bf16.apply_rotary_emb (:5-31).
 * wq/wk [128] bf16 (NULL = no norm); tokens >= l_rope (the text tokens) are only normalised.  q_out_scale (1 = none;
 * ignored with X2V_ROUND_REF) multiplies q inside its final rounding, see x2v_rmsnorm_rope_scaled_bf16. */
int x2v_headnorm_rope_bf16(void* q, int64_t ldq, void* k, int64_t ldk, const void* wq, const void* wk, const void* cos_tab, const void* sin_tab, int64_t L,
                           int H, int64_t l_rope, float eps, int round_mode, float q_out_scale, void* stream);

/* x2v_headnorm_rope_bf16 in place on HEAD-BLOCKED q and k: heads [j*heads_per_block, (j+1)*heads_per_block) of all L tokens form the matrix
 * [L][heads_per_block*128] (token stride ld) that starts j*block_stride elements into the buffer — the [N_ranks][S/N][(H/N) d] send buffer of
 * the Ulysses exchange, written in that layout by x2v_gemm_bf16_blocked (replaces the reference's view + transpose + contiguous copy of
 * q/k/v in front of all_to_all, attentions/distributed/ulysses/attn.py:36-46 / comm/all2all.py:29-33). */
int x2v_headnorm_rope_blocked_bf16(void* q, void* k, int64_t ld, int heads_per_block, int64_t block_stride, const void* wq, const void* wk, const void* cos_tab,
                                   const void* sin_tab, int64_t L, int H, int64_t l_rope, float eps, int round_mode, float q_out_scale, void* stream);

/* x[M,D] = bf16(x + bf16(y * gate)) (gate [D] bf16, NULL = plain add) — replaces `x.add_(y * gate)`
 * (transformer_infer.py:402,468,503) for callers that do not fuse it into the GEMM epilogue. */
int x2v_gate_residual_bf16(void* x, int64_t ldx, const void* y, int64_t ldy, const void* gate, int64_t M, int D, void* stream);

/* y = act(x) elementwise on [n] bf16: act 1 = gelu-tanh (transformer_infer.py:492), 3 = silu (pre_infer.py:74,76), X2V_ACT_GELU_ERF = the exact
 * GELU of the i2v CLIP-feature MLP (pre_infer.py:106: gelu(approximate="none")). */
#define X2V_ACT_GELU_ERF 4
int x2v_activation_bf16(const void* x, void* y, int64_t n, int act, void* stream);

/* y[M,N] = epi(x[M,K] . W[N,K]^T + bias[N])   — replaces MMWeight.apply = torch.addmm(bias, x, W.t())
 * (common/ops/mm/mm_weight.py:70-96); W is the checkpoint's [N,K] row-major tensor (the reference's
 * `.t()` view, :76).  bf16 in, fp32 MFMA accumulate, bf16 out.  K % 64 == 0, N % 8 == 0, any M >= 1.
 * resid/gate only for X2V_EPI_RESIDUAL (resid [M,N] ld = ldr; gate [N] or NULL). */
int x2v_gemm_bf16(const void* x, int64_t ldx, const void* w, int64_t ldw, const void* bias, void* y, int64_t ldy, int64_t M, int N, int K,
                  int epilogue, const void* resid, int64_t ldr, const void* gate, void* stream);

/* Same, selecting the kernel (tuning / validation hook).  variant & 0xff: 0 = by shape (what x2v_gemm_bf16 does:
 * the 256x256-tile ping-pong kernel of gemm256.hip when the grid fills the chip, else the 128x128 kernel of
 * gemm.hip), 1 = 128x128 kernel, 2 = 256x256 ping-pong kernel (two waves per SIMD; fp8's and mxfp8's large-shape kernel), 3 = 256x256
 * single-stream kernel (one software-pipelined wave per SIMD; bf16 only, its large-shape kernel) in the form the dispatcher prefers, 4 = its
 * one-output-tile-per-workgroup form (gemm256s.hip), 5 = its continuous-pipeline form (gemm256c.hip: persistent workgroups, the K loop runs on
 * into the next output tile, epilogue straight from the accumulators; needs K a multiple of 128 and >= 256, N a multiple of 256, y blocks
 * that are multiples of 128 columns and resid with y's row stride, else X2V_E_SHAPE; same bits as form 4); (variant >> 8) & 0xff = m-tiles per
 * scheduling group of the 256x256 kernels (0 = default). */
int x2v_gemm_bf16_variant(const void* x, int64_t ldx, const void* w, int64_t ldw, const void* bias, void* y, int64_t ldy, int64_t M, int N, int K,
                          int epilogue, const void* resid, int64_t ldr, const void* gate, int variant, void* stream);

/* x2v_gemm_bf16_variant with X2V_EPI_RESIDUAL and a ROW PERIOD of the residual: resid holds resid_period rows (ld = ldr) and output row r is
 * y[r] = bf16(resid[r mod resid_period] + bf16(bf16(acc + bias) * gate)) — the bytes the plain entry writes when given resid repeated M / resid_period
 * times, without the copy.  It is the fan-out of a CFG step whose two forwards share everything up to block 0's cross-attention (same latents, same
 * timestep: transformer_infer.py runs that front twice): one residual stream of S rows, a stacked cross-attention output of 2 S rows.
 * resid_period = 0: the plain entry.  y must not overlap resid (X2V_E_ARG); M and resid_period below 2^31.  Every kernel takes every period, except
 * that the continuous forms (variant 5) need a multiple of 8 that is >= 256 with the residual inside 2^31 bytes — variant 0 / 3 then take the
 * one-tile-per-workgroup form, variant 5 answers X2V_E_SHAPE.  Error texts start with the entry's name, as everywhere. */
int x2v_gemm_bf16_resid_period(const void* x, int64_t ldx, const void* w, int64_t ldw, const void* bias, void* y, int64_t ldy, int64_t M, int N, int K,
                               const void* resid, int64_t ldr, int64_t resid_period, const void* gate, int variant, void* stream);

/* x2v_gemm_bf16 on block-strided operands — what lets the Ulysses exchange buffers (attentions/distributed/comm/all2all.py:6-89) be GEMM
 * operands in place instead of being transposed by copies (all2all.py:29-33, :70-75,87):
 *   x K-blocked (x_kblock > 0): element k of row m at x[(k / x_kblock) * x_kblock_stride + m * ldx + k % x_kblock] — the received
 *     head->seq buffer [N_ranks][S/N][(H/N) d] read as the [S/N, H d] input of the output projection (x_kblock = (H/N) d, a multiple
 *     of 64 elements dividing K; ldx >= x_kblock);
 *   y N-blocked (y_nblock > 0): column n of row m at y[(n / y_nblock) * y_nblock_stride + m * ldy + n % y_nblock] — the q/k/v projection
 *     writing straight into the seq->head send buffer [N_ranks][S/N][(H/N) d] (y_nblock a multiple of 8 dividing N; ldy >= y_nblock;
 *     not with X2V_EPI_RESIDUAL).
 * 0 disables either blocking (plain row-major).  The kernel is chosen by shape as in x2v_gemm_bf16. */
int x2v_gemm_bf16_blocked(const void* x, int64_t ldx, int x_kblock, int64_t x_kblock_stride, const void* w, int64_t ldw, const void* bias, void* y, int64_t ldy,
                          int y_nblock, int64_t y_nblock_stride, int64_t M, int N, int K, int epilogue, const void* resid, int64_t ldr, const void* gate, void* stream);

/* v = x . W^T + bias written as V^T [N/128][ldvt/64][128][64] with tokens in [M, ldvt) zero-filled — x2v_gemm_bf16 followed by
 * x2v_transpose_heads_bf16 in one kernel (same bits): the self-attention v projection (transformer_infer.py:345-347) handing its result to
 * x2v_attn_fwd_bf16_vt without the transposing pass.  Only for shapes that x2v_gemm_kernel_choice maps to kernel 3 (else X2V_E_SHAPE). */
int x2v_gemm_bf16_vt(const void* x, int64_t ldx, const void* w, int64_t ldw, const void* bias, void* vt, int64_t ldvt, int64_t M, int N, int K, void* stream);

/* Which kernel variant 0 of x2v_gemm_bf16_variant (fp8 = 0) / x2v_gemm_fp8_variant (fp8 = 1) launches for this shape.  Low byte = tile family:
 * 1 = the 128x128 kernel, 2 = the 256x256 fp8 kernels, 3 = the 256x256 single-stream kernel (bf16).  Bit 8 (0x100) = the CONTINUOUS-pipeline
 * form of that family (gemm256c.hip / gemm256c8.hip) for a row-major y and a residual of y's stride; clear = one output tile per workgroup
 * (gemm256s.hip) / the ping-pong kernel (gemm256.hip) — same bits either way, asserted by the equality tests.  Negative = X2V_E_SHAPE.
 * Host-only; lets a parity test and the bench line record WHICH kernel was compared with the oracle / timed (the X2V_GEMM_*CONTINUOUS
 * switches are folded in). */
int x2v_gemm_kernel_choice(int64_t M, int N, int K, int64_t ldx, int64_t ldw, int fp8);

/* Dense non-causal attention, head_dim 128: o[Sq, H*128] = softmax(q k^T * scale) v per head —
 * replaces FlashAttn2Weight/FlashAttn3Weight/TorchSDPAWeight.apply (common/ops/attn/attn_weight.py:71-126,
 * 209-239) for one sequence (cu_seqlens = [0, S]).  q/k/v: token stride in elements (ldq/ldk/ldv), head h
 * at column offset h*128; fp32 softmax, bf16 P, fp32 accumulate.  scale <= 0 selects 1/sqrt(128).
 * Sq == 0 (an empty query shard) is a no-op returning X2V_OK; Sk == 0 is X2V_E_SHAPE (softmax over nothing). */
int x2v_attn_fwd_bf16(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* o, int64_t ldo, int64_t Sq,
                      int64_t Sk, int H, int head_dim, float scale, void* stream);

/* Same, selecting the lazy-rescale threshold of the online softmax (validation hook for the rare, data-dependent rescale branch: the three
 * must agree to rounding): 0 = default (= 6), 4 = rescale O on every tile, 5 = when a row max grew by more than 4 (base-2 units), 6 = by
 * more than 8.  X2V_ATTN_Q_PRESCALED is a flag of the Python layer's `variant` word (lib.attention); at the C-ABI the pre-scaled-q form is
 * X2V_ATTN_VT_PRESCALED in x2v_attn_fwd_bf16_vt's `flags`. */
#define X2V_ATTN_Q_PRESCALED 0x100
#define X2V_ATTN_LOG2E_SCALE(head_dim_rsqrt) ((head_dim_rsqrt) * 1.4426950408889634f)
int x2v_attn_fwd_bf16_variant(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* o, int64_t ldo, int64_t Sq,
                              int64_t Sk, int H, int head_dim, float scale, int variant, void* stream);

/* V [Sk, H*128] (token stride ldv) -> V^T [H][ldvt/64][128][64] (per head and 64-key tile a contiguous [dv][key] block) with
 * keys >= Sk zero-filled (ldvt % 64 == 0, ldvt >= Sk): the operand layout of x2v_attn_fwd_bf16_vt. */
int x2v_transpose_heads_bf16(const void* v, int64_t ldv, void* vt, int64_t ldvt, int64_t Sk, int H, void* stream);

/* Append to a V^T cache — the KV cache of the autoregressive Wan (models/networks/wan/infer/causvid/transformer_infer.py:85-120, where the cache is
 * row-major and flash-attention reads it in place): v [S, H*128] bf16 (token stride ldv) into the key columns [key0, key0 + S) of
 * vt [H][ldvt/64][128][64] bf16.  After the call key key0 + s of head h, component dv — element vt[((h * (ldvt/64) + (key0+s)/64) * 128 + dv) * 64 +
 * (key0+s) % 64] — holds v[s][h*128 + dv] for 0 <= s < S, a bit copy, and NO other byte of vt has changed: not the keys < key0 (the key0 % 64 of them
 * that share the first tile included), not the keys >= key0 + S (the rest of the last tile included), no other tile.  No row of v outside [0, S) is
 * read.  key0 and S are arbitrary (odd too); ranges whose ends are multiples of 8 keys take a kernel without the edge handling.
 * Appends to one cache, and the attention launches over it, must be ordered on one stream.
 * ldvt % 64 == 0, key0 >= 0, S >= 0, key0 + S <= ldvt, 1 <= H <= 65535 (else X2V_E_SHAPE); v, vt 16-byte aligned and ldv % 8 == 0 (X2V_E_ALIGN);
 * ldv >= H*128; S == 0 is X2V_OK without a launch. */
int x2v_transpose_heads_append_bf16(const void* v, int64_t ldv, void* vt, int64_t ldvt, int64_t key0, int64_t S, int H, void* stream);

/* x2v_attn_fwd_bf16 on a pre-transposed V (x2v_transpose_heads_bf16) — the "ping-pong" kernel the fused block drivers launch for
 * self-attention (transformer_infer.py:369-379): V^T is staged by LDS-DMA and read as plain 16-byte fragments, the softmax scale * log2(e)
 * lives in q.  flags: X2V_ATTN_VT_PRESCALED — q already carries scale*log2(e) (x2v_rmsnorm_rope_scaled_bf16 / x2v_headnorm_rope_bf16 folded it
 * into q's one rounding; without it the kernel multiplies and re-rounds q itself); X2V_ATTN_VT_STAGGER — query block b starts its walk over the
 * key tiles (b mod 8) tiles in (the online softmax does not care where the walk starts; the L2 does: +1.3 % at Wan-14B 720p in 2-step runs, but
 * -0.9 % at sustained load, profiles/r04_call12_*: the fused drivers stopped setting it in round 4).  The result of a
 * query row then depends on which 256-row block of the launch it sits in (another fp32 summation order, same tolerance): callers that compare
 * bits across differently partitioned launches (the Ulysses driver) leave it off.  X2V_ATTN_VT_ONE_WALK — never the persistent short-walk form
 * (below): one workgroup per 256-row query block, as for long walks (A/B runs and the bit-equality test of the two forms).
 * Short walks — cross-attention over the text context, transformer_infer.py:424-455: 4..32 whole 64-key tiles and >= 512 query blocks x heads —
 * run as a persistent launch: a workgroup walks a contiguous range of the (sequence, head, query block) list as one tile stream, the next
 * block's q rows prefetched through LDS, the previous block's output stored under the next block's first tile.  Same bits as the one-walk form. */
#define X2V_ATTN_VT_PRESCALED 1
#define X2V_ATTN_VT_STAGGER 2
#define X2V_ATTN_VT_ONE_WALK 4
int x2v_attn_fwd_bf16_vt(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* vt, int64_t ldvt, void* o, int64_t ldo, int64_t Sq, int64_t Sk,
                         int H, int head_dim, float scale, int flags, void* stream);

/* Carry form of x2v_attn_fwd_bf16_vt: a launch that can start from, and leave behind, the running softmax state of its query rows, so that attention
 * over all keys is a chain of launches over key chunks with one rounding to bf16 at the end — the kernel layer of ring attention
 * (attentions/distributed/ring/attn.py:25-63 `_update_out_and_lse`, 99-193: bf16 block outputs merged by four fp32 elementwise passes per step; here
 * the merge is the epilogue of the attention kernel) and the library's attention-with-LSE.  q / k / V^T / o: operands, layouts and checks as
 * x2v_attn_fwd_bf16_vt (Sq != Sk allowed, head_dim 128).  State: acc fp32 [Sq, H*128], row stride ldacc elements (ldacc % 4 == 0, acc 16-byte
 * aligned), head h at column h*128; lse fp32 [H][ldlse], ldlse >= Sq, row r of head h at lse[h*ldlse + r].
 * flags: X2V_ATTN_VT_PRESCALED, plus
 *   X2V_ATTN_CARRY_IN   the launch continues from the state in acc / lse (which a CARRY_OUT launch over other keys of the same q left there);
 *   X2V_ATTN_CARRY_OUT  the launch leaves its state in acc / lse and does not write o (o may be null).
 * Without CARRY_OUT it writes bf16 o and does not write acc / lse.  With neither bit it is x2v_attn_fwd_bf16_vt with X2V_ATTN_VT_ONE_WALK (same
 * kernel, same bits; acc / lse are not looked at).  CARRY_OUT alone is attention with LSE: o = bf16(acc), lse = base-2 log-sum-exp.
 * Always one workgroup per 256-row query block (never the persistent short-walk form), the key walk starts at tile 0, and the XCD-aware work mapping
 * follows x2v_attn_vt_launch_plan(Sq, Sk, H, 1, X2V_ATTN_VT_ONE_WALK) (it only renumbers workgroups).
 *
 * Arithmetic.  The walk over the launch's keys is the dense kernel's, unchanged; scores s are in base 2 (q carries scale*log2(e)).  At its end a
 * query row has the kernel's running reference m, the fp32 row sum l of 2^(s - m) (the four partial sums of the row's lanes added as
 * ((p0 + p1) + (p2 + p3)) pairwise across lanes, as in the dense kernel) and the unnormalised fp32 accumulator a[0..127].  Then, all in fp32,
 * exp2 / log2 the hardware's v_exp_f32 / v_log_f32 (1 ulp), every line one rounding:
 *   1.  Lb = m + log2(l)
 *   without CARRY_IN:  2.  L' = Lb      3.  w = 1 / l      4.  A'[d] = a[d] * w          (the dense kernel's own normalisation)
 *   with CARRY_IN, (A, L) read from acc / lse:
 *   2.  M  = max(L, Lb)
 *   3.  L' = M + log2(exp2(L - M) + exp2(Lb - M))
 *   4.  wA = exp2(L - L'),  wa = exp2(m - L')
 *   5.  A'[d] = fma(A[d], wA, a[d] * wa)           (a[d] * wa rounded first; the unnormalised accumulator is weighted directly, no division by l)
 *   6.  CARRY_OUT: acc <- A' (fp32), lse <- L'; else o <- bf16(A') (round to nearest even).
 * lse is in base-2 units of the scaled scores: the natural-log value of softmax(scale * q k^T) is lse * ln 2.  tests/attn_carry_ref.py restates
 * steps 1-6 in float64. */
#define X2V_ATTN_CARRY_IN 8
#define X2V_ATTN_CARRY_OUT 16
int x2v_attn_fwd_bf16_vt_carry(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* vt, int64_t ldvt, void* o, int64_t ldo, void* acc,
                               int64_t ldacc, void* lse, int64_t ldlse, int64_t Sq, int64_t Sk, int H, int head_dim, float scale, int flags, void* stream);

/* Which launch form x2v_attn_fwd_bf16_vt / _batched takes for a shape (host-only, no GPU needed): bit 0 = the XCD-aware head-major work mapping
 * (on while the K / V^T streams of the <= 8 heads in flight fit the Infinity Cache and the launch has >= 512 workgroups — e.g. the Ulysses
 * rank's 5 heads x 75 600 keys; off for 40 heads at 720p), bit 8 = the staggered key walk (X2V_ATTN_VT_STAGGER and Sk >= 16 tiles), bit 9 = the
 * persistent short-walk form (then bits 0 and 8 are clear).  `flags` as x2v_attn_fwd_bf16_vt's.  Lets a parity
 * test assert that the kernel branch it compared with the oracle is the one a model's shapes take — the launches replace
 * attentions/distributed/ulysses/attn.py:68-80 (per rank) and transformer_infer.py:369-379 (single GPU).  Negative = X2V_E_SHAPE. */
int x2v_attn_vt_launch_plan(int64_t Sq, int64_t Sk, int H, int B, int flags);

/* x2v_attn_fwd_bf16_vt over B independent sequences in ONE launch: sequence b uses q / k / V^T / o at b * {q,k,vt,o}_bstride elements from the
 * base pointers (same Sq, Sk, H, strides).  The fused Wan driver runs the conditional and unconditional forwards of a CFG step
 * (models/networks/wan/model.py:197-226) as one pass over both token sets; this is their self-attention — 2 x 11 840 workgroups fill the 256 CUs'
 * last round better than two launches do.  V^T is one array [H][ldvt/64][128][64] over the stacked tokens of all sequences (each sequence padded to
 * a multiple of 64 rows), so vt_bstride = rows_per_sequence * 128. */
int x2v_attn_fwd_bf16_vt_batched(const void* q, int64_t ldq, int64_t q_bstride, const void* k, int64_t ldk, int64_t k_bstride, const void* vt, int64_t ldvt,
                                 int64_t vt_bstride, void* o, int64_t ldo, int64_t o_bstride, int64_t Sq, int64_t Sk, int H, int B, int head_dim, float scale,
                                 int flags, void* stream);

/* Block-sparse self-attention: x2v_attn_fwd_bf16_vt restricted to a static mask of 128 x 128 (query rows x keys) blocks — replaces
 * RadialAttnWeight.apply (common/ops/attn/attn_weight.py:129-162 -> attentions/common/radial_attn.py:34-46, the block-sparse wrapper with
 * R = C = 128 it plans and runs) for one sequence.  Operands, layouts and flags (X2V_ATTN_VT_PRESCALED only) as x2v_attn_fwd_bf16_vt, Sq == Sk.
 * `plan` is a device table of plan_words 32-bit words built on the host from the mask (lightx2v_amd.lib.attn_block_plan, which also checks it):
 * plan_wgs = ceil(Sq / 256) records {256-row query block, first entry, entries}, the longest walk first, then the entries
 * (64-key tile << 2) | (bit 0: rows 0-127 of the query block attend the tile) | (bit 1: rows 128-255 do); the tile that may hold fewer than 64
 * keys is the last entry of its record and tiles at or beyond ceil(Sk / 64) never appear.  plan_seq is the sequence length the plan was built
 * for (a mismatch is X2V_E_SHAPE, no launch).  Keys >= Sk are excluded as in the dense kernel: the reference instead zero-pads q / k / v to a
 * multiple of 128 and attends the padded keys with score 0 (radial_attn.py:21-31); DESIGN.md §5 has the measured difference. */
int x2v_attn_bsr_fwd_bf16_vt(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* vt, int64_t ldvt, void* o, int64_t ldo, int64_t Sq, int64_t Sk,
                             int H, int head_dim, float scale, int flags, const void* plan, int64_t plan_words, int64_t plan_seq, int plan_wgs, void* stream);

/* ---- Block-scaled fp8 self-attention (attention type "hip_mxfp8", attn_mx.hip): the slot the reference fills with sage_attn2 (8-bit QK^T, fp8 PV),
 * with this project's own numerics; one sequence, head dim 128.  Three preparation steps and the forward; tests/attn_mx_ref.py restates all of
 * it in float64 / NumPy.
 *
 * Arithmetic.  Inputs bf16 q [Sq, H*128], k, v [Sk, H*128] (any token stride).
 *   kmean   x2v_attn_mx_kmean_f32: kmean[col] = fl32(T / (float)Sk), T = the fp32 sum over the 256-token chunks, in chunk order, of the fp32 sum of
 *           k[token, col] over the chunk's tokens in token order (chunk c = tokens 256 c .. 256 c + 255; chunk sums start from the first token,
 *           T from the first chunk's sum).  The order is part of the contract: the result does not depend on the launch.
 *   Q^, K^  x2v_attn_mx_quant_qk: x' = fl32(fl32(x - mean[col]) * scale) (mean taken as 0 unless `smooth`; q is quantised with smooth = 0 and
 *           scale = softmax scale * log2(e), or 1.0f when q already carries it; k with scale = 1.0f and, for smoothing, kmean: softmax does not
 *           change when a per-query constant q.kmean is taken off a row of scores).  MXFP8 along the head dimension with the rule of
 *           x2v_quant_mxfp8_bf16: per token, head and 32-channel block one e8m0 byte = the smallest power of two >= amax / 448 (fp32 quotient,
 *           an all-zero block -> byte 0), codes = e4m3fn_rne(x' * 2^(127 - byte)).
 *           codes: bytes [H][S_pad][128]; scales: bytes [H][S_pad][4] (one dword per token and head, byte b = channels 32 b .. 32 b + 31).
 *           Rows S .. S_pad - 1 are written as code 0 / scale byte 0.  q: S_pad = Sq; k: S_pad = ceil(Sk / 128) * 128.
 *   V^T^    x2v_attn_mx_quant_vt: per head and dv row one e8m0 byte per 32 consecutive keys, blocks starting at key 0, same scale rule over the
 *           block's keys < Sk (x' = v); keys >= Sk up to the end of the last 128-key tile are code 0 and do not enter the block's amax (a block
 *           with no key < Sk has byte 0).  No scale byte written is 0xFF (the rule saturates at 254).
 *           codes: bytes [H][NT][128 dv][128 keys], NT = ceil(Sk / 128), keys of a tile in their natural order; scales: bytes [H][NT][128 dv][4]
 *           (byte b = keys 32 b .. 32 b + 31 of the tile).
 *   scores  s = Q^ . K^^T in fp32 from v_mfma_scale_f32_16x16x128_f8f6f4 (one instruction spans the head dimension and applies both operands'
 *           scale bytes), accumulated onto C = -m, m the row's running max before the tile; keys >= Sk are excluded (score -1e30, P = 0).
 *   P       Running max: exact, no lazy threshold (threshold 2^0).  After a tile's scores s - m_old are known, d = max(0, row max of them);
 *           m_new = fl32(m_old + d) (the first tile adopts its row max, whatever its sign), the tile's scores become fl32(s' - d) and l and o are
 *           multiplied by exp2(-d) wherever some row of the wave has d > 0.  P = exp2(s - m_new) <= 1 always (v_exp_f32).  l accumulates the fp32
 *           P.  For P.V, P^ = e4m3fn_rne(P * 2^8) with operand scale byte 127 - 8 = 119: the largest P the rule allows, 1.0, is code value 256
 *           (of 448), the smallest positive code is 2^-9, i.e. P = 2^-17, and P < 2^-18 (ties included) is flushed to 0: 17 binades of tail.
 *           A lazy threshold of 2^T would cost T of them; T = 0 was chosen, and the rescale multiplications it adds run only in tiles where a
 *           row maximum grows.
 *   o       (sum over keys of P^ . V^^)/l in fp32 (MFMA accumulation, 128 keys per instruction), one rounding to bf16.
 * Sq != Sk is allowed; Sq == 0 is a no-op; Sk == 0 is X2V_E_SHAPE. */

/* Host-only: sizes[0..6] = bytes of {q codes, q scales, k codes, k scales, V^T codes, V^T scales, kmean buffer} for (Sq, Sk, H).  The kmean
 * buffer is H*128 floats (the mean) followed by the chunk sums the two-pass reduction keeps (ceil(Sk / 256) * H*128 floats). */
int x2v_attn_mx_sizes(int64_t Sq, int64_t Sk, int H, int64_t* sizes);
/* kmean (see above): k bf16 [Sk, H*128], token stride ldk (even, 4-byte aligned rows); kmean: the buffer of sizes[6] bytes. */
int x2v_attn_mx_kmean_f32(const void* k, int64_t ldk, float* kmean, int64_t Sk, int H, void* stream);
/* Q^ / K^ (see above): x bf16 [S, H*128] (ldx % 8 == 0, 16-byte aligned); mean fp32 [H*128] (used, and required, when smooth != 0). */
int x2v_attn_mx_quant_qk(const void* x, int64_t ldx, const float* mean, int smooth, float scale, void* codes, void* scales, int64_t S, int64_t S_pad, int H,
                         void* stream);
/* V^T^ (see above): v bf16 [Sk, H*128] (ldv % 8 == 0, 16-byte aligned). */
int x2v_attn_mx_quant_vt(const void* v, int64_t ldv, void* codes, void* scales, int64_t Sk, int H, void* stream);
/* The forward on the prepared operands (buffers of x2v_attn_mx_sizes for the same Sq, Sk, H, 16-byte aligned); o bf16 [Sq, H*128], ldo % 4 == 0,
 * 8-byte aligned rows. */
int x2v_attn_mx_fwd(const void* q_codes, const void* q_scales, const void* k_codes, const void* k_scales, const void* vt_codes, const void* vt_scales, void* o,
                    int64_t ldo, int64_t Sq, int64_t Sk, int H, void* stream);

/* Per-token dynamic fp8 quantisation: s[m] = amax(|x[m,:]|)/448, xq = e4m3fn(x / s) — replaces
 * vllm ops.scaled_fp8_quant(use_per_token_if_dynamic=True) / sgl_kernel.sgl_per_token_quant_fp8
 * (mm_weight.py:236-245).  xq [M,K] bytes (ld = ldq), scale fp32 [M]. */
int x2v_quant_fp8_rowwise(const void* x, int64_t ldx, void* xq, int64_t ldq, float* scale, int64_t M, int K, void* stream);

/* x2v_quant_fp8_rowwise reading a K-BLOCKED x (element k of row m at x[(k / x_kblock) * x_kblock_stride + m * ldx + k % x_kblock]: the Ulysses
 * head->seq receive buffer [N_ranks][S/N][(H/N) d], attentions/distributed/ulysses/attn.py:82-91 after its transposing copy) and writing ROW-MAJOR
 * codes — the quantisation pass reads every element once anyway, so under w8a8 the de-blocking costs nothing and the output projection
 * (mm_weight.py:236-245 + :287-319) runs the plain row-major x2v_gemm_fp8.  x_kblock = 0: plain row-major x (= x2v_quant_fp8_rowwise). */
int x2v_quant_fp8_rowwise_blocked(const void* x, int64_t ldx, int x_kblock, int64_t x_kblock_stride, void* xq, int64_t ldq, float* scale, int64_t M, int K,
                                  void* stream);

/* x2v_layernorm_bf16 fused with x2v_quant_fp8_rowwise on its output: xq [M,D] e4m3 codes (ld = ldq) and sx [M] fp32 scales of the
 * normalised (+affine, +modulated) row, bit-identical to the two calls in sequence — the w8a8 path's LayerNorm -> scaled_fp8_quant in front
 * of the q/k/v and ffn_0 projections (transformer_infer.py:329-342,481-492 with mm_weight.py:236-245), without the bf16 round trip through
 * HBM and quantised once for every projection that reads it.  512 < D <= 16384. */
int x2v_layernorm_quant_fp8(const void* x, int64_t ldx, const void* w, const void* b, const void* scale, const void* shift, void* xq, int64_t ldq, float* sx,
                            int64_t M, int D, float eps, void* stream);

/* y[M,N] = epi((xq[M,K] . wq[N,K]^T) * sx[m] * sw[n] + bias[n]) → bf16 — replaces
 * torch.ops._C.cutlass_scaled_mm / sgl_kernel.fp8_scaled_mm (mm_weight.py:310-318,551-558,581-588).
 * e4m3fn operands, fp32 MFMA accumulate.  K % 128 == 0, N % 8 == 0. */
int x2v_gemm_fp8(const void* xq, int64_t ldx, const float* sx, const void* wq, int64_t ldw, const float* sw, const void* bias, void* y,
                 int64_t ldy, int64_t M, int N, int K, int epilogue, const void* resid, int64_t ldr, const void* gate, void* stream);

/* Same with the kernel selector of x2v_gemm_bf16_variant: 0 = by shape, 1 = 128x128 kernel, 2 = 256x256 ping-pong kernel (gemm256.hip, the large-shape
 * default), 5 = the continuous single-stream pipeline (gemm256c8.hip: gemm256c's structure on v_mfma_scale_f32_32x32x64_f8f6f4; needs K a multiple
 * of 256 and >= 512, N a multiple of 256, y blocks that are multiples of 128 columns and resid with y's row stride, else X2V_E_SHAPE; meant to give
 * variant 2's bits: 84 / 84 cases equal on MI355X, tools/gemm_fp8_continuous_check.py).  Variant 0 takes the continuous form where the shape
 * allows and the operands are row-major (X2V_GEMM_FP8_CONTINUOUS=0: never, =2: also for x2v_gemm_fp8_blocked's operands).  3 / 4 are bf16 only
 * (X2V_E_ARG). */
int x2v_gemm_fp8_variant(const void* xq, int64_t ldx, const float* sx, const void* wq, int64_t ldw, const float* sw, const void* bias, void* y,
                         int64_t ldy, int64_t M, int N, int K, int epilogue, const void* resid, int64_t ldr, const void* gate, int variant,
                         void* stream);

/* x2v_gemm_fp8_variant with X2V_EPI_RESIDUAL and a row period of the residual (see x2v_gemm_bf16_resid_period). */
int x2v_gemm_fp8_resid_period(const void* xq, int64_t ldx, const float* sx, const void* wq, int64_t ldw, const float* sw, const void* bias, void* y,
                              int64_t ldy, int64_t M, int N, int K, const void* resid, int64_t ldr, int64_t resid_period, const void* gate, int variant,
                              void* stream);

/* x2v_gemm_fp8 on block-strided operands (see x2v_gemm_bf16_blocked; x_kblock in e4m3 elements = bytes, a multiple of 128; sx stays [M]). */
int x2v_gemm_fp8_blocked(const void* xq, int64_t ldx, int x_kblock, int64_t x_kblock_stride, const float* sx, const void* wq, int64_t ldw, const float* sw,
                         const void* bias, void* y, int64_t ldy, int y_nblock, int64_t y_nblock_stride, int64_t M, int N, int K, int epilogue, const void* resid,
                         int64_t ldr, const void* gate, void* stream);

/* ---- w8a8 int8: the reference's W-int8-channel-sym-A-int8-channel-sym-dynamic-* operators (mm_weight.py:322-354 Vllm, :592-... Sgl-ActVllm;
 * weight load :185-201, activation quantiser :247-249).  Numeric contract, every fp32 operation IEEE and correctly rounded:
 *   activation  amax = max|x[m,:]|, scale[m] = amax / 127.0f, inv = 127.0f / amax, q = clamp(rint(float(x) * inv), -128, 127), round half to
 *               even (restated from vLLM's dynamic scaled_int8_quant(x, scale=None, azp=None, symmetric=True)); an all-zero row gives codes 0
 *               and scale 0, and no NaN reaches the codes
 *   weight      per output channel, IntegerQuantizer(8, True, "per_channel"): scale = max(amax, 1e-5) / 127, q = clamp(round(w / scale), -128, 127)
 *               (done at load by the operator class, or by tools/convert_ckpt.py --linear_dtype torch.int8)
 *   product     acc_i32 = xq[M,K] . wq[N,K]^T exactly (v_mfma_i32_32x32x32_i8), float(acc) by v_cvt_f32_i32 (round to nearest even), then
 *               y = epi(float(acc) * sx[m] * sw[n] + bias[n]) -> bf16 in the statement order and with the rounding points of x2v_gemm_fp8
 * Codes are two's-complement int8 bytes. */

/* Per-token dynamic int8 quantisation (see the contract above).  Arguments and limits of x2v_quant_fp8_rowwise: K % 8 == 0, K <= 16384. */
int x2v_quant_int8_rowwise(const void* x, int64_t ldx, void* xq, int64_t ldq, float* scale, int64_t M, int K, void* stream);

/* The same reading a K-blocked x and writing row-major codes (see x2v_quant_fp8_rowwise_blocked). */
int x2v_quant_int8_rowwise_blocked(const void* x, int64_t ldx, int x_kblock, int64_t x_kblock_stride, void* xq, int64_t ldq, float* scale, int64_t M, int K,
                                   void* stream);

/* x2v_layernorm_bf16 fused with x2v_quant_int8_rowwise on its output, bit-identical to the two calls in sequence.  512 < D <= 16384. */
int x2v_layernorm_quant_int8(const void* x, int64_t ldx, const void* w, const void* b, const void* scale, const void* shift, void* xq, int64_t ldq, float* sx,
                             int64_t M, int D, float eps, void* stream);

/* y[M,N] = epi(float(xq[M,K] . wq[N,K]^T) * sx[m] * sw[n] + bias[n]) -> bf16 — replaces torch.ops._C.cutlass_scaled_mm on int8 operands
 * (mm_weight.py:346-353) / sgl_kernel.int8_scaled_mm (:616-...).  Arguments of x2v_gemm_fp8.  K % 128 == 0, N % 8 == 0, K <= 65536 (|acc| < 2^31). */
int x2v_gemm_int8(const void* xq, int64_t ldx, const float* sx, const void* wq, int64_t ldw, const float* sw, const void* bias, void* y,
                  int64_t ldy, int64_t M, int N, int K, int epilogue, const void* resid, int64_t ldr, const void* gate, void* stream);

/* Same, selecting the kernel.  variant & 0xff: 0 = by shape, 1 = the 128x128 kernel (gemm.hip's structure on v_mfma_i32_32x32x32_i8; every legal
 * shape), 5 = the continuous 256x256 kernel (gemm256c8.hip's int8 form: the fp8 kernel's pipeline and shape conditions — K a multiple of 256 and >= 512, N a multiple
 * of 256, y blocks that are multiples of 128 columns, resid with y's row stride, a residual row period that is a multiple of 8 and >= 256 — else
 * X2V_E_SHAPE; bit-equal with variant 1).  Variant 0 takes it where x2v_gemm_fp8's rule takes a 256x256 kernel and these conditions hold.  There is
 * no int8 ping-pong kernel: 2, 3 and 4 return X2V_E_ARG.  Bits 8..15 = m-tiles per scheduling group of the 256x256 kernel (0 = default). */
int x2v_gemm_int8_variant(const void* xq, int64_t ldx, const float* sx, const void* wq, int64_t ldw, const float* sw, const void* bias, void* y,
                          int64_t ldy, int64_t M, int N, int K, int epilogue, const void* resid, int64_t ldr, const void* gate, int variant,
                          void* stream);

/* x2v_gemm_int8_variant with X2V_EPI_RESIDUAL and a row period of the residual (see x2v_gemm_bf16_resid_period). */
int x2v_gemm_int8_resid_period(const void* xq, int64_t ldx, const float* sx, const void* wq, int64_t ldw, const float* sw, const void* bias, void* y,
                               int64_t ldy, int64_t M, int N, int K, const void* resid, int64_t ldr, int64_t resid_period, const void* gate, int variant,
                               void* stream);

/* x2v_gemm_int8 on block-strided operands (see x2v_gemm_fp8_blocked; x_kblock in codes = bytes, a multiple of 128; sx stays [M]). */
int x2v_gemm_int8_blocked(const void* xq, int64_t ldx, int x_kblock, int64_t x_kblock_stride, const float* sx, const void* wq, int64_t ldw, const float* sw,
                          const void* bias, void* y, int64_t ldy, int y_nblock, int64_t y_nblock_stride, int64_t M, int N, int K, int epilogue, const void* resid,
                          int64_t ldr, const void* gate, void* stream);

/* Which kernel variant 0 of x2v_gemm_int8_variant launches for this shape, with x2v_gemm_kernel_choice's convention: low byte = tile family
 * (1 = the 128x128 kernel, 2 = the 256x256 kernel), bit 8 = its continuous form (the only 256x256 int8 kernel: 2 comes with bit 8), for a
 * row-major y.  Negative = X2V_E_SHAPE.  Host-only. */
int x2v_gemm_int8_kernel_choice(int64_t M, int N, int K, int64_t ldx, int64_t ldw);

/* Which body variant 0 of the MX GEMMs launches for this shape without a fused epilogue: 1 = the 128x128 kernel, 2 = the 256x256 ping-pong kernel.
 * format: 1 = x2v_gemm_mxfp8, 2 = x2v_gemm_mxfp6_mxfp8, 3 = x2v_gemm_mxfp4 (anything else: X2V_E_ARG); lda, ldb in bytes, as there.  The rule: at
 * least 192 tiles of 256x256, both leading dimensions below 2^24 bytes, and at least 8 (formats 1, 2: K / 128) or 6 (format 3: K / 256) K-tiles of
 * 128 bytes per row of a.  Negative = X2V_E_SHAPE (K not a multiple of the format's K-tile, N % 8, a leading dimension below the row's bytes).
 * Host-only. */
int x2v_gemm_mx_kernel_choice(int format, int64_t M, int N, int K, int64_t lda, int64_t ldb);

/* MXFP8 (OCP microscaling) activation / weight quantisation — replaces lightx2v_kernel.gemm.scaled_fp8_quant
 * (lightx2v_kernel/python/lightx2v_kernel/gemm.py:73-83, csrc/gemm/mxfp8_quant_kernels_sm120.cu:139-196): per 32 consecutive K
 * elements one e8m0 scale = the smallest power of two >= max|x|/448, elements = e4m3fn_rne(x / scale).
 * x bf16 [M,K]; q bytes [M,K] (ld = ldq); scales: bytes [K/128][M][4] — K-tile major, row, the 4 k blocks of that K-tile: the
 * layout x2v_gemm_mxfp8 consumes (as the reference's 128x4 swizzle is the sm120 tensor core's; logical element (m, kb) sits at
 * ((kb/4)*M + m)*4 + kb%4).  K % 128 == 0.
 * NaN and Inf elements are outside the contract of their own 32-wide block and leave every other block's codes and scale byte as they
 * are with 0 in the element's place (tests/test_gpu_mx_fp64.py); measured, not promised: a NaN is skipped by the block maximum (the
 * scale byte and the other 31 codes are those with 0 in its place) and becomes a NaN code (0x7f / 0xff), an Inf gives scale byte 254,
 * code 0x7f and +/-0 for the other 31 (profiles/mx_fp64_parity.txt). */
int x2v_quant_mxfp8_bf16(const void* x, int64_t ldx, void* q, int64_t ldq, void* scales, int64_t M, int K, void* stream);

/* y[M,N] = alpha * (deq(a)[M,K] . deq(b)[N,K]^T) + bias[n] → bf16, deq = e4m3 element * 2^(scale byte - 127) of its row and
 * 32-wide k block — replaces lightx2v_kernel.gemm.cutlass_scaled_mxfp8_mm (gemm.py:93-97,
 * csrc/gemm/mxfp8_scaled_mm_kernels_sm120.cu:60-66,150-160).  sa [K/128][M][4], sb [K/128][N][4] as written by
 * x2v_quant_mxfp8_bf16; alpha: device pointer to one fp32 (NULL = 1), bias bf16 [N] or NULL.
 * Runs on v_mfma_scale_f32_32x32x64_f8f6f4 with the block scales applied by the matrix instruction.
 * K % 128 == 0, N % 8 == 0; a, b, y: rows 16-byte aligned (lda % 16, ldb % 16, both >= K, ldy % 8); scale tables 4-byte, bias 8-byte aligned.
 * Anything else: X2V_E_SHAPE / X2V_E_ALIGN / X2V_E_ARG before any HIP call.
 * Two bodies, chosen by x2v_gemm_mx_kernel_choice's rule: the MX mode of the 128x128-tile kernel and of the 256x256-tile ping-pong kernel (shapes that
 * fill the chip and every fused epilogue; it addresses a tile with 32-bit offsets: lda, ldb < 2^24 bytes, else X2V_E_SHAPE). */
int x2v_gemm_mxfp8(const void* a, int64_t lda, const void* sa, const void* b, int64_t ldb, const void* sb, const void* bias, const float* alpha, void* y,
                   int64_t ldy, int64_t M, int N, int K, void* stream);

/* x2v_gemm_mxfp8 with the fused epilogues of x2v_gemm_bf16 / x2v_gemm_fp8 (X2V_EPI_*; y = epi(alpha * a.b^T + bias); X2V_EPI_RESIDUAL without
 * resid: X2V_E_ARG): what the fused block drivers call for a linear layer held in MXFP8 (operator class MMWeightMxfp8Hip).  Every fused epilogue
 * runs the 256x256 body: lda, ldb < 2^24 bytes, else X2V_E_SHAPE. */
int x2v_gemm_mxfp8_epi(const void* a, int64_t lda, const void* sa, const void* b, int64_t ldb, const void* sb, const void* bias, const float* alpha, void* y,
                       int64_t ldy, int64_t M, int N, int K, int epilogue, const void* resid, int64_t ldr, const void* gate, void* stream);

/* Same with a kernel selector: 0 = automatic (as x2v_gemm_mxfp8), 1 = 128x128-tile kernel, 2 = 256x256-tile ping-pong kernel (lda, ldb < 2^24
 * bytes, else X2V_E_SHAPE); anything else: X2V_E_ARG. */
int x2v_gemm_mxfp8_variant(const void* a, int64_t lda, const void* sa, const void* b, int64_t ldb, const void* sb, const void* bias, const float* alpha,
                           void* y, int64_t ldy, int64_t M, int N, int K, int variant, void* stream);

/* MXFP6 weight quantisation — replaces lightx2v_kernel.gemm.scaled_fp6_quant (lightx2v_kernel/python/lightx2v_kernel/gemm.py:58-68,
 * csrc/gemm/mxfp6_quant_kernels_sm120.cu:168-225).  x2v_quant_mxfp8_bf16's contract with 28 in place of 448 and e3m2 in place of e4m3fn:
 * per 32 consecutive K elements the scale byte = biased exponent of the smallest power of two >= max|x| / 28 (the quotient in fp32 with
 * denormals, saturating at 254; an all-zero block -> byte 0 and zero codes), code = e3m2(x * 2^(127 - byte)), one rounding to nearest-even,
 * saturating at +/-28, sign of zero kept.  e3m2: 1 sign, 3 exponent bits (bias 3), 2 mantissa bits, code = s<<5 | e<<2 | m; subnormals
 * m * 2^-4, largest number 28, no NaN / Inf.
 * x bf16 [M,K] (ldx % 8 == 0, 16-byte aligned); q bytes [M, 3K/4] (ldq in bytes, ldq % 4 == 0, 4-byte aligned): the reference's dense
 * little-endian packing (mxfp6_quant_kernels_sm120.cu:74-99, 4 codes -> 3 bytes) — code j of a row sits at bits 6j .. 6j+5 of the row's
 * bytes; scales: the [K/128][M][4] table of x2v_quant_mxfp8_bf16.  K % 128 == 0.
 * NaN and Inf elements are outside the contract of their own 32-wide block and leave every other block as with 0 in their place
 * (tests/test_gpu_mx6.py); measured, not promised: a NaN is skipped by the block maximum (the scale byte and the other 31 codes are those
 * with 0 in its place) and saturates to +/-28 (e3m2 has no NaN code), an Inf gives scale byte 254, code 0x1f and +/-0 for the other 31
 * (profiles/mx6_fp64_parity.txt). */
int x2v_quant_mxfp6_bf16(const void* x, int64_t ldx, void* q, int64_t ldq, void* scales, int64_t M, int K, void* stream);

/* y[M,N] = alpha * (deq(a)[M,K] . deq(b)[N,K]^T) + bias[n] → bf16 with a = MXFP8 (e4m3) activations of x2v_quant_mxfp8_bf16 and
 * b = MXFP6 (e3m2) weights of x2v_quant_mxfp6_bf16, packed [N, 3K/4], ldb in BYTES — replaces
 * lightx2v_kernel.gemm.cutlass_scaled_mxfp6_mxfp8_mm (gemm.py:84-88, csrc/gemm/mxfp6_mxfp8_scaled_mm_kernels_sm120.cu:39-46).  sa, sb, alpha,
 * bias and the rounding points as x2v_gemm_mxfp8.  Runs on v_mfma_scale_f32_32x32x64_f8f6f4 with the weight operand in format 3 (e3m2) next
 * to the e4m3 one, the e8m0 block scales applied by the instruction.
 * K % 128 == 0, N % 8 == 0; a, y: rows 16-byte aligned (lda % 16, ldy % 8); b: 4-byte aligned with ldb % 4 == 0 and ldb >= 3K/4 (the
 * weight tile is staged in 12-byte pieces); scale tables 4-byte, bias 8-byte aligned.
 * Two bodies, chosen as for x2v_gemm_mxfp8: the fp6 mode of the 128x128-tile kernel and of the 256x256-tile ping-pong kernel (shapes that fill
 * the chip and every fused epilogue; it addresses a tile with 32-bit offsets: lda, ldb < 2^24 bytes, else X2V_E_SHAPE). */
int x2v_gemm_mxfp6_mxfp8(const void* a, int64_t lda, const void* sa, const void* b, int64_t ldb, const void* sb, const void* bias, const float* alpha,
                         void* y, int64_t ldy, int64_t M, int N, int K, void* stream);

/* x2v_gemm_mxfp6_mxfp8 with the fused epilogues of x2v_gemm_mxfp8_epi (X2V_EPI_*; X2V_EPI_RESIDUAL without resid: X2V_E_ARG): what the fused
 * block drivers call for a linear layer held in MXFP6 (operator class MMWeightMxfp6Hip). */
int x2v_gemm_mxfp6_mxfp8_epi(const void* a, int64_t lda, const void* sa, const void* b, int64_t ldb, const void* sb, const void* bias, const float* alpha,
                             void* y, int64_t ldy, int64_t M, int N, int K, int epilogue, const void* resid, int64_t ldr, const void* gate, void* stream);

/* Same with x2v_gemm_mxfp8_variant's kernel selector: 0 = automatic, 1 = 128x128-tile kernel, 2 = 256x256-tile ping-pong kernel; anything else:
 * X2V_E_ARG. */
int x2v_gemm_mxfp6_mxfp8_variant(const void* a, int64_t lda, const void* sa, const void* b, int64_t ldb, const void* sb, const void* bias,
                                 const float* alpha, void* y, int64_t ldy, int64_t M, int N, int K, int variant, void* stream);

/* MXFP4 quantisation (OCP microscaling, 4-bit elements), activations and weights alike — the w4a4 slot of the reference's kernel package, whose
 * own pair (scaled_fp4_quant / cutlass_scaled_fp4_mm) is NVFP4: an e4m3 scale per 16 elements plus a global scale, which gfx950's matrix
 * instruction does not apply.  This is x2v_quant_mxfp6_bf16's contract with 6 in place of 28 and e2m1 in place of e3m2:
 * e2m1: 1 sign bit, 2 exponent bits (bias 1), 1 mantissa bit, code = s<<3 | e<<1 | m; e = 0: value m * 0.5, otherwise (2 + m) * 2^(e-2);
 * magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6; no NaN / Inf.
 * Per 32 consecutive K elements the scale byte = biased exponent of the smallest power of two >= max|x| / 6 (the quotient in fp32 with
 * denormals, saturating at 254; an all-zero block -> byte 0 and zero codes); code = e2m1(x * 2^(127 - byte)), one rounding to nearest-even on
 * the e2m1 grid from the exact product (ties at 0.25, 1.25, 2.5 and 5 go down, at 0.75, 1.75 and 3.5 up), the sign of zero kept; +/-6 is
 * reached by saturation only for NaN / Inf elements.
 * x bf16 [M,K] (ldx % 8 == 0, 16-byte aligned); q bytes [M, K/2] (ldq in bytes, ldq % 8 == 0, ldq >= K/2, 8-byte aligned): two codes per byte,
 * the dense little-endian nibble string — code j of a row sits at bits 4j .. 4j+3 of the row's bytes (the even code in the low nibble), the
 * order in which the matrix instruction reads a lane's 16 bytes (tests/test_gpu_mx4.py walks it); scales: the [K/128][M][4] table of
 * x2v_quant_mxfp8_bf16.  K % 128 == 0.
 * NaN and Inf elements are outside the contract of their own 32-wide block and leave every other block as with 0 in their place
 * (tests/test_gpu_mx4.py); measured, not promised: a NaN is skipped by the block maximum (the scale byte and the other 31 codes are those
 * with 0 in its place) and saturates to +/-6 (e2m1 has no NaN code), an Inf gives scale byte 254, code 0x7 and +/-0 for the other 31
 * (profiles/mx4_fp64_parity.txt). */
int x2v_quant_mxfp4_bf16(const void* x, int64_t ldx, void* q, int64_t ldq, void* scales, int64_t M, int K, void* stream);

/* y[M,N] = epi(alpha * (deq(a)[M,K] . deq(b)[N,K]^T) + bias[n]) → bf16 with a and b MXFP4 as written by x2v_quant_mxfp4_bf16: packed e2m1 codes
 * [rows, K/2], lda and ldb in BYTES; deq = e2m1 value * 2^(scale byte - 127) of its row and 32-wide k block.  sa [K/128][M][4], sb [K/128][N][4];
 * alpha: device pointer to one fp32 (NULL = 1), bias bf16 [N] or NULL; bias, alpha and the rounding points as x2v_gemm_mxfp8.
 * Runs on v_mfma_scale_f32_32x32x64_f8f6f4 with both operands in format 4 (e2m1), the e8m0 block scales applied by the instruction: the form
 * that takes the cycles of the bf16 instruction at four times the K.
 * K % 256 == 0 (a 128-byte operand row per K-tile holds 256 k), N % 8 == 0; a, b, y: rows 16-byte aligned (lda % 16, ldb % 16, both >= K/2,
 * ldy % 8); scale tables 4-byte, bias 8-byte aligned.  Anything else: X2V_E_SHAPE / X2V_E_ALIGN / X2V_E_ARG before any HIP call.
 * Two bodies, chosen by x2v_gemm_mxfp8's rule on the number of 128-byte K-tiles (K / 256; from 6 K-tiles on, where MXFP8 wants 8): the fp4 mode
 * of the 128x128-tile kernel and of the 256x256-tile ping-pong kernel (shapes that fill the chip and every fused epilogue; it addresses a tile with 32-bit offsets: lda, ldb < 2^24
 * bytes, else X2V_E_SHAPE). */
int x2v_gemm_mxfp4(const void* a, int64_t lda, const void* sa, const void* b, int64_t ldb, const void* sb, const void* bias, const float* alpha, void* y,
                   int64_t ldy, int64_t M, int N, int K, void* stream);

/* x2v_gemm_mxfp4 with the fused epilogues of x2v_gemm_mxfp8_epi (X2V_EPI_*; X2V_EPI_RESIDUAL without resid: X2V_E_ARG): what the fused block
 * drivers call for a linear layer held in MXFP4 (operator class MMWeightMxfp4Hip). */
int x2v_gemm_mxfp4_epi(const void* a, int64_t lda, const void* sa, const void* b, int64_t ldb, const void* sb, const void* bias, const float* alpha, void* y,
                       int64_t ldy, int64_t M, int N, int K, int epilogue, const void* resid, int64_t ldr, const void* gate, void* stream);

/* Same with x2v_gemm_mxfp8_variant's kernel selector: 0 = automatic, 1 = 128x128-tile kernel, 2 = 256x256-tile ping-pong kernel; anything else:
 * X2V_E_ARG. */
int x2v_gemm_mxfp4_variant(const void* a, int64_t lda, const void* sa, const void* b, int64_t ldb, const void* sb, const void* bias, const float* alpha,
                           void* y, int64_t ldy, int64_t M, int N, int K, int variant, void* stream);

/* Timestep sinusoid: y[n, dim] bf16 = [cos(t*f_j) | sin(t*f_j)], f_j = 10000^(-j/(dim/2)) computed in
 * float64 then rounded — replaces sinusoidal_embedding_1d (wan/infer/utils.py:161-172).  t: int64 [n]. */
int x2v_sinusoid_embed_bf16(const int64_t* t, void* y, int n, int dim, void* stream);

/* The same for fractional timesteps, t: float64 [n] — the step-distill scheduler's timesteps are sigma * 1000 in fp32 (999.87 for step 999 at
 * shift 8) and sinusoidal_embedding_1d takes them as they are (`position.type(torch.float64)`, utils.py:163).  For integral t the bits of
 * x2v_sinusoid_embed_bf16. */
int x2v_sinusoid_embed_f64_bf16(const double* t, void* y, int n, int dim, void* stream);

/* One denoise step's sampler update on the fp32 latent tensor as a single elementwise kernel — replaces the CFG combine
 * `noise_pred = uncond + guide * (cond - uncond)` (models/networks/wan/model.py:218) followed by WanScheduler.step_post
 * (models/schedulers/wan/scheduler.py:322-360: x0 = sample - sigma_i * noise_pred; UniPC-bh2 corrector :224-320 when order_c > 0;
 * predictor :130-222), solver order <= 2.  Every product / sum / quotient is rounded separately, in the reference's order (the result is
 * bit-identical to the reference's op sequence on CPU tensors).
 *   cond, uncond (NULL = no CFG): fp32 [n];  latents: the sample (bf16 if latents_bf16 — the reference's DTYPE=BF16 step_pre — else fp32);
 *   last_sample, m0, m1: the previous step's corrected sample and the x0 predictions of steps i-1, i-2 (fp32 [n]; NULL where unused);
 *   outputs (fp32 [n], must not alias the inputs): noise_pred (NULL = not wanted), x0_out (this step's x0 prediction), sample_out (the
 *   corrected sample = next step's last_sample), latents_out (the predictor's output = next latents);
 *   coef: HOST array of 12 floats {guide, sigma_i, c_a = sigma_t/sigma_s0, c_b = alpha_t*h_phi_1, c_c = alpha_t*B_h, c_rk = r_1,
 *   c_rho0 = rhos_c[0], c_rhol = rhos_c[-1], p_a, p_b, p_c, p_rk} (corrector c_*, predictor p_*), each computed as the reference
 *   computes it; order_c in {0 (no corrector), 1, 2}, order_p in {1, 2}. */
int x2v_unipc_step_f32(const float* cond, const float* uncond, const void* latents, int latents_bf16, const float* last_sample, const float* m0,
                       const float* m1, float* noise_pred, float* x0_out, float* sample_out, float* latents_out, const float* coef, int order_c, int order_p,
                       int64_t n, void* stream);

/* The 4-step-distilled scheduler's update (schedulers/wan/step_distill/scheduler.py:40-56) with the optional CFG combine in front:
 * x0 = latents - sigma * noise_pred;  noise != NULL (not the last step): x0 = one_minus_next * x0 + sigma_next * noise;
 * latents_out = x0 in the dtype of `latents` (bf16 if latents_bf16).  latents_out may alias latents. */
int x2v_distill_step_f32(const float* cond, const float* uncond, float guide, const void* latents, int latents_bf16, const float* noise, float sigma,
                         float one_minus_next, float sigma_next, float* noise_pred, void* latents_out, int64_t n, void* stream);

/* Causal Conv3d on channels-last fp32 activations — replaces CausalConv3d.forward
 * (models/video_encoders/hf/wan/vae.py:19-44; with kt = 1 also the decoder's Conv2d, vae.py:70-118).
 * Time axis input = [zeros(kt-1-cache_frames) | cache (cache_frames frames) | x (T frames)], output T frames;
 * zero 'same' padding spatially (kh/2, kw/2).  fp32 in/out, fp32-input MFMA (exact fp32 fma chain).
 * x:  [T, Hh, Ww, Cin]   cache: [cache_frames, Hh, Ww, Cin] or NULL when cache_frames == 0
 * w:  [Cout, kt, kh, kw, Cin]   bias: [Cout] or NULL   y: [T, Hh, Ww, Cout].  Cin % 4 == 0. */
int x2v_causal_conv3d_f32(const float* x, const float* cache, int cache_frames, const float* w, const float* bias, float* y, int T, int Hh, int Ww,
                          int Cin, int Cout, int kt, int kh, int kw, void* stream);

/* ---- Wan VAE decoder (models/video_encoders/hf/wan/vae.py), fp32, channels-last --------------------------------
 * Convolution inputs live in zero-bordered buffers [lead + T][H + 2*ph][W + 2*pw][C] whose `lead` = kt-1 leading
 * frames are the reference's per-conv feature cache (CACHE_T = 2, vae.py:16); see lightx2v_amd/csrc/vae.hip. */

#define X2V_VCONV_CLAMP 1  /* clamp the result to [-1, 1] (WanVAE.decode: .clamp_(-1, 1), vae.py:951-955) */
#define X2V_VCONV_TSPLIT 2 /* Cout = 2C: channel block j of frame t goes to frame 2t + j (Resample upsample3d, vae.py:136-138) */

/* y[t,h,w,co] = bias[co] + resid[t,h,w,co] + sum_{dt,dh,dw,c} xp[(t+dt)*fs + (h+dh)*rs + (w+dw)*ps + c] * w[co*wrs + ((dt*kh+dh)*kw+dw)*Cin + c]
 * — replaces CausalConv3d.forward (vae.py:19-44), the decoder's nn.Conv2d (vae.py:87-95) and, with kt=kh=kw=1, its
 * 1x1 convolutions and the attention block's GEMMs (vae.py:226-262).  `xp` points at the element tap (0,0,0) of output
 * pixel (0,0,0) reads (strides in floats; borders must be zero).  fp32 in/out on the fp32-input MFMA.
 * Cin % 16 == 0; strides % 4 == 0; bias/resid optional; resid has y's layout; y is [T,H,W,Cout] (or [2T,H,W,Cout/2]
 * with X2V_VCONV_TSPLIT). */
int x2v_vae_conv_f32(const float* xp, int64_t x_frame_stride, int64_t x_row_stride, int64_t x_px_stride, const float* w, int64_t w_row_stride,
                     const float* bias, const float* resid, float* y, int T, int Hh, int Ww, int Cin, int Cout, int kt, int kh, int kw, int flags,
                     void* stream);

/* Pixel-wise producer of conv input buffers — replaces RMS_norm (vae.py:47-59) + nn.SiLU (ResidualBlock, head),
 * Upsample nearest-exact x2 (vae.py:62-67) and the latent un-normalisation z / scale[1] + scale[0] (vae.py:716-719):
 *   v = x[t,h,w,:];  gamma != NULL: v = v / max(||v||_2, 1e-12) * sqrt(C) * gamma;  else v = v / a + b (a, b optional);
 *   silu: v *= sigmoid(v);  written to y + t*y_frame_stride + h*y_row_stride + w*C (2x2 replicated when upsample). */
int x2v_vae_prep_f32(const float* x, float* y, int T, int Hh, int Ww, int C, const float* gamma, const float* a, const float* b, int silu, int upsample,
                     int64_t y_frame_stride, int64_t y_row_stride, void* stream);

/* In-place s[M,N] = softmax(scale * s) rows, fp32 — the softmax of F.scaled_dot_product_attention in the VAE
 * AttentionBlock (vae.py:249-253).  N % 4 == 0; scale > 0 (the row maximum is taken before scaling; anything else, NaN included, is X2V_E_ARG). */
int x2v_softmax_rows_f32(float* s, int64_t ld, int64_t M, int N, float scale, void* stream);

/* ---- Wan VAE encoder (models/video_encoders/hf/wan/vae.py Encoder3d :265-374, WanVAE_.encode :684-711) ------------------------
 * The encoder's other convolutions run on the decoder's entries above; see lightx2v_amd/csrc/vae_enc.hip. */

/* 3x3 stride-2 convolution of Resample downsample2d / downsample3d (vae.py:96-100: nn.ZeroPad2d((0, 1, 0, 1)) + nn.Conv2d(dim, dim, 3, stride=(2, 2))):
 *   y[t,h,w,co] = bias[co] + sum_{dh,dw,c} xp[t*fs + (2h+dh)*rs + (2w+dw)*ps + c] * w[co*wrs + (dh*3+dw)*Cin + c],  h < Hin/2, w < Win/2,
 * where input rows >= Hin and columns >= Win read as zero (the bottom / right pad; xp needs no border).  fp16 operands (strides in halves), fp32
 * accumulate on v_mfma_f32_16x16x32_f16, fp32 bias / output y [T][Hin/2][Win/2][Cout].  With the hi/lo split operands of x2v_vae_prep_split_f16
 * (activations [hi | hi * 2^-12 | lo], weights [hi | lo * 2^12 | hi], Cin = 3 * C rounded up to 32) the result is fp32-grade.
 * Cin % 32 == 0, Cout % 4 == 0, Hin, Win >= 2, strides % 8 == 0, flags = 0. */
int x2v_vae_conv_s2_f16(const void* xp, int64_t x_frame_stride, int64_t x_row_stride, int64_t x_px_stride, const void* w, int64_t w_row_stride, const float* bias,
                        float* y, int T, int Hin, int Win, int Cin, int Cout, int flags, void* stream);

/* Producer of Encoder3d.conv1's operand buffer (vae.py:286) from the caller's video, read in place: video[c*c_stride + t*t_stride + h*row_stride + w]
 * (c < 3, w contiguous) -> y + t*y_frame_stride + h*y_row_stride + w*y_px_stride, channels-last: mode 0 = 3 fp32, 1 = 3 fp16, 2 = the hi/lo split
 * [hi(3) | hi * 2^-12 (3) | lo(3)] of x2v_vae_prep_split_f16 (9 halves).  Channels behind those are not written (pad channels stay zero). */
int x2v_vae_video_prep(const float* video, int64_t c_stride, int64_t t_stride, int64_t row_stride, int T, int H, int W, void* y, int64_t y_frame_stride,
                       int64_t y_row_stride, int64_t y_px_stride, int mode, void* stream);

/* One output tile of WanVAE_.tiled_decode / tiled_encode (vae.py:568-682: blend_v with the tile above, blend_h with the tile to the left, crop to the
 * stride, cat) from the RAW tiles in one pass.  Tiles are fp32 channels-last: center [T][ch][cw][C], up [T][uh][cw][C], left [T][ch][lw][C], up_left
 * [T][uh][lw][C]; ev / eh = the vertical / horizontal blend extents min(len_a, len_b, blend) (0 = no neighbour on that axis: its pointer may be NULL;
 * up_left is read only where both are set).  For y < rh, x < rw the value
 *   u = up[uh-ev+y][x] (x < eh: up_left[uh-ev+y][lw-eh+x]*(1-x/eh) + u*(x/eh));  v = u*(1-y/ev) + center[y][x]*(y/ev) for y < ev, else center[y][x];
 *   l = left[y][lw-eh+x] (y < ev: up_left[..]*(1-y/ev) + l*(y/ev));              out = l*(1-x/eh) + v*(x/eh) for x < eh, else v
 * goes to out[c*out_c_stride + t*out_t_stride + y*out_row_stride + x] (out = the region's first element in a channel-first video), clamped to [-1, 1]
 * when clamp = 1.  Weights are formed in double and rounded once to fp32, every product and sum is rounded on its own: the bits of the reference's
 * in-place row-major blending whenever blend <= stride on both axes (a neighbour's rows read here then lie outside its own blend zone). */
int x2v_vae_tile_compose_f32(const float* center, const float* up, const float* left, const float* up_left, int T, int C, int ch, int cw, int uh, int lw,
                             int ev, int eh, int rh, int rw, float* out, int64_t out_c_stride, int64_t out_t_stride, int64_t out_row_stride, int clamp,
                             void* stream);

/* ---- HunyuanVideo VAE decode (video_encoders/hf/autoencoder_kl_causal_3d/), fp32, channels-last ------------------- */

/* Pixel-wise producer: v = x*mul[c] + add[c] (mul/add optional; GroupNorm applied as a per-channel affine), optional SiLU
 * and clamp to [0,1]; nearest x2 upsampling in H,W (up_hw) and/or in T where frame 0 is not duplicated (up_t) — replaces
 * GroupNorm+SiLU in ResnetBlockCausal3D (unet_causal_3d_blocks.py:377-410), UpsampleCausal3D.forward (:168-187) and the
 * final (x/2+0.5).clamp(0,1) of VideoEncoderKLCausal3DModel.decode (model.py:41).  Output addressing as x2v_vae_prep_f32. */
int x2v_vae_prep_ex_f32(const float* x, float* y, int T, int Hh, int Ww, int C, const float* mul, const float* add, int silu, int clamp01, int up_hw, int up_t,
                        int64_t y_frame_stride, int64_t y_row_stride, void* stream);

/* 16-bit-operand form of x2v_vae_conv_f32 for the HunyuanVideo VAE, which the reference runs in fp16 (hunyuan_runner.py:40): xp and w
 * are fp16 (strides in halves, Cin % 64 == 0), accumulation fp32 on v_mfma_f32_32x32x16_f16, bias / residual / output fp32 — the residual
 * stream and the normalisation statistics keep fp32, only the convolution operands are rounded.  Same flags and layouts as the fp32 entry, plus
 * 4 = the per-tap kernel and 8 = the 64-pixel halo kernel (kernel choice for A/B runs and tests: by default 3x3 kernels on images at least 16 pixels wide
 * with Cin % 32 == 0 and Cout % 96 == 0, Cout % 128 == 0 or Cout <= 16, without the time-split, take the 128-pixel kernel on v_mfma_f32_16x16x32_f16, whose
 * reduction order differs in rounding; other 3x3 kernels at least 16 pixels wide, without the time-split, the 64-pixel halo kernel — in the released models the
 * Wan encoder's 32-cout head alone; everything else the per-tap kernel) and 16 = the last 32 channels of Cin are zero padding in both operands (the 128-pixel
 * kernel, which steps in 32 channels, skips them; a no-op for the results). */
int x2v_vae_conv_f16(const void* xp, int64_t x_frame_stride, int64_t x_row_stride, int64_t x_px_stride, const void* w, int64_t w_row_stride, const float* bias,
                     const float* resid, float* y, int T, int H, int W, int Cin, int Cout, int kt, int kh, int kw, int flags, void* stream);

/* x2v_vae_conv_f16 with the causal convolution's feature cache (the reference's feat_cache entry, vae.py:16,199-214: the last kt - 1 input frames of the
 * previous chunk) in a buffer of its own: input frames 0 .. kt-2 are read from `cache` ([kt-1][H+2][W+2][Cin], xp's strides), the rest from xp, whose own
 * leading kt - 1 frames are not read — a frame buffer shared by several convolutions then needs no copy of the cache in front of it.  Only where
 * x2v_vae_conv_f16_cached_ok(...) == 1 (the shapes that take the 128-pixel kernel, see x2v_vae_conv_f16, without the time-split and kernel-choice flags); bit-identical to x2v_vae_conv_f16 on a buffer
 * that carries the same frames. */
int x2v_vae_conv_f16_cached(const void* xp, const void* cache, int64_t x_frame_stride, int64_t x_row_stride, int64_t x_px_stride, const void* w, int64_t w_row_stride,
                            const float* bias, const float* resid, float* y, int T, int H, int W, int Cin, int Cout, int kt, int kh, int kw, int flags, void* stream);
int x2v_vae_conv_f16_cached_ok(int W, int Cin, int Cout, int kh, int kw, int flags);

/* x2v_vae_prep_f32 writing fp16 with an explicit pixel stride y_px_stride >= C (the Wan decoder's 96-channel stage pads its operand
 * buffers to 128 channels for x2v_vae_conv_f16's 64-channel K steps; pad channels are never written and stay zero). */
int x2v_vae_prep_f16(const float* x, void* y, int T, int H, int W, int C, const float* gamma, const float* a, const float* b, int silu, int upsample,
                     int64_t y_frame_stride, int64_t y_row_stride, int64_t y_px_stride, void* stream);

/* x2v_vae_prep_f16 writing the hi/lo fp16 split of its result (x = hi + lo, hi = fp16(x), lo = fp16(x - hi): ~22 mantissa bits) as channels
 * [hi | hi * 2^-12 | lo] (3*C halves per pixel, y_px_stride >= 3*C; hi saturates at the fp16 range instead of overflowing).  With weights laid out
 * [hi | lo * 2^12 | hi] along Cin (the power-of-two pair keeps the weights' lo halves normal fp16 numbers), x2v_vae_conv_f16 accumulates
 * xh.wh + xh.wl + xl.wh in fp32: the Wan VAE's fp32 convolutions (vae.py:794) at fp32-grade accuracy on the 16-bit matrix instruction. */
int x2v_vae_prep_split_f16(const float* x, void* y, int T, int Hh, int Ww, int C, const float* gamma, const float* a, const float* b, int silu, int upsample,
                           int64_t y_frame_stride, int64_t y_row_stride, int64_t y_px_stride, void* stream);

/* x2v_vae_prep_ex_f32 writing fp16: fills the operand buffer of x2v_vae_conv_f16 (y strides in halves, C % 8 == 0). */
int x2v_vae_prep_ex_f16(const float* x, void* y, int T, int H, int W, int C, const float* mul, const float* add, int silu, int clamp01, int up_hw, int up_t,
                        int64_t y_frame_stride, int64_t y_row_stride, void* stream);

/* Fill the borders of a conv input buffer [frames][Hp][Wp][C] by replication: spatial borders (width `pad`) from the
 * nearest interior pixel, the `lead` leading frames from frame `lead` — F.pad(mode="replicate") of CausalConv3d
 * (unet_causal_3d_blocks.py:84-91). */
int x2v_vae_replicate_border_f32(float* buf, int frames, int lead, int Hp, int Wp, int C, int pad, void* stream);

/* GroupNorm over x [npix, C] (G groups of consecutive channels, statistics over all pixels) reduced to a per-channel
 * affine: mul[c] = rstd_g*gamma[c], add[c] = beta[c] - mean_g*mul[c] (apply with x2v_vae_prep_ex_f32) — replaces
 * torch.nn.GroupNorm (unet_causal_3d_blocks.py:318,341; vae.py conv_norm_out; the attention block's group_norm).
 * workspace: 2*G doubles (device).  fp64 accumulation. */
int x2v_groupnorm_affine_f32(const float* x, int64_t npix, int C, int G, const float* gamma, const float* beta, float eps, double* workspace, float* mul,
                             float* add, void* stream);

/* In-place s[M,N] = softmax(scale*s) over the frame-causal prefix: row i sees keys j < min(n_keys, (i/hw + 1)*hw), the
 * rest (incl. padding columns n_keys..N) becomes 0 (prepare_causal_attention_mask, unet_causal_3d_blocks.py:48-63, in
 * UNetMidBlockCausal3D.forward :629-634).  scale > 0 (the row maximum is taken before scaling; anything else, NaN included, is X2V_E_ARG). */
int x2v_softmax_rows_causal_f32(float* s, int64_t ld, int64_t M, int N, float scale, int hw, int n_keys, void* stream);

/* Linear cross-fade of overlapping tiles along one axis, tensors viewed as [outer][axis][inner]:
 * b[idx] = a[na-extent+idx]*(1-idx/extent) + b[idx]*(idx/extent), idx < extent — blend_v / blend_h / blend_t
 * (autoencoder_kl_causal_3d.py:347-364). */
int x2v_blend_axis_f32(const float* a, float* b, int64_t outer, int na, int nb, int64_t inner, int64_t a_outer_stride, int64_t b_outer_stride, int extent,
                       void* stream);

/* ---- Wan tiny VAE / TAEHV decoder (models/video_encoders/hf/tae.py, wan/vae_tiny.py), bf16, channels-last; see lightx2v_amd/csrc/taehv.hip ---- */

#define X2V_C2D_RELU 1          /* ReLU behind everything else (nn.ReLU after a conv, MemBlock.act) */
#define X2V_C2D_UPSAMPLE_READ 2 /* the operand is read at (h >> 1, w >> 1): nn.Upsample(scale_factor=2) in front of the convolution, never materialised; x is [T][(H+1)/2][(W+1)/2][Cin] */
#define X2V_C2D_TWO_SOURCE 4    /* MemBlock's conv(cat([x_t, x_{t-1}], 1)): weights [Cout][k][k][2 Cin], channels Cin .. 2 Cin - 1 read frame t - 1 of x; frame -1 is `mem` or, mem NULL, zero */
#define X2V_C2D_HEAD 8          /* v = RN(2 v - 1) behind the bias (WanVAE_tiny.decode's .mul_(2).sub_(1)) */

/* 2-D convolution, k = ksize in {1, 3} with zero "same" padding, bf16 operands, fp32 accumulation on v_mfma_f32_16x16x32_bf16, bf16 out; RN = one rounding to
 * nearest even to bf16, as the reference's bf16 modules round:
 *   acc[t,h,w,co] = sum_{s, dh, dw, c} X_s[t][(h + dh - k/2) >> u][(w + dw - k/2) >> u][c] * w[((co * k + dh) * k + dw) * Ctot + s * Cin + c]
 *   X_0[t] = x + t * x_frame_stride, X_1[t] = X_0[t - 1] (X_1[0] = mem, or zero), X[..][r][q][c] = X + r * x_row_stride + q * x_px_stride + c; taps whose (h + dh - k/2,
 *   w + dw - k/2) lies outside [0, H) x [0, W) read zero; u = 1 with X2V_C2D_UPSAMPLE_READ else 0; s < 2, Ctot = 2 Cin with X2V_C2D_TWO_SOURCE else s < 1, Ctot = Cin;
 *   v = RN(acc + bias[co]) (bias optional);  resid: v = RN(v + resid[same offset as y]);  X2V_C2D_HEAD: v = RN(2 v - 1);  X2V_C2D_RELU: v = max(v, 0);
 *   y[((t - frame_trim) * tsplit + co / Cb) * y_frame_stride + h * y_row_stride + w * y_px_stride + (co % Cb) * y_ch_stride] = v,  Cb = Cout / tsplit
 * for t = frame_trim .. T - 1 (frames below frame_trim are neither computed nor stored).  tsplit > 1 is TGrow (tae.py:46-55): cout block j of frame t goes to
 * frame tsplit * t + j.  A channel-first y (y_ch_stride != 1) is the output head's [3][T][H][W] store.
 * Cin % 8 == 0 (% 32 with X2V_C2D_TWO_SOURCE), any Cout; x strides in elements, multiples of 8; x, mem, w 16-byte aligned; resid shares y's strides; no residual with tsplit > 1. */
int x2v_conv2d_bf16(const void* x, const void* mem, int64_t x_frame_stride, int64_t x_row_stride, int64_t x_px_stride, const void* w, const void* bias, const void* resid,
                    void* y, int64_t y_frame_stride, int64_t y_row_stride, int64_t y_px_stride, int64_t y_ch_stride, int T, int H, int W, int Cin, int Cout, int ksize,
                    int flags, int tsplit, int frame_trim, void* stream);

/* Clamp (tae.py:19-21) from the caller's channel-first latent to the first convolution's channels-last operand:
 *   y[((t * H + h) * W + w) * C + c] = RN(RN(tanh(RN(RN(z[c * c_stride + t * t_stride + h * W + w]) / 3))) * 3)
 * z fp32 (z_is_f32 = 1; its RN is the reference's .to(bfloat16)) or bf16 (0); y bf16, 16-byte aligned; C % 8 == 0. */
int x2v_taehv_clamp_bf16(const void* z, int z_is_f32, int64_t c_stride, int64_t t_stride, void* y, int T, int H, int W, int C, void* stream);

/* ---- CLIP ViT-H/14 image tower (fp16): the producer of i2v's clip_encoder_out (runners/wan/wan_runner.py:191-198; the reference runs the tower in fp16,
 * :71-72).  fp16 tensors are raw IEEE half bits; LayerNorm parameters are fp32. ---- */

/* epilogues of x2v_gemm_f16 */
#define X2V_EPI16_NONE 0     /* y = fp16(acc + bias) */
#define X2V_EPI16_GELU_ERF 1 /* y = fp16(gelu_erf(acc + bias))                       (nn.GELU() of AttentionBlock.mlp, xlm_roberta/model.py:150-153) */
#define X2V_EPI16_RESIDUAL 2 /* y = fp16(resid + fp16(acc + bias)); y may alias resid (x + self.attn(...) / x + self.mlp(...), model.py:162-163) */
#define X2V_EPI16_QUICK_GELU 3 /* y = fp16(v * sigmoid(1.702 v)), v = acc + bias in fp32; bias must be given (transformers' QuickGELUActivation after CLIPMLP.fc1) */
#define X2V_EPI16_SWIGLU 4     /* W is [2N, K], row 2n = gate_proj row n, row 2n + 1 = up_proj row n: y[M, N] = fp16(silu(fp16(acc_gate)) * fp16(acc_up)), the SiLU
                                * and the product in fp32 on the two fp16 Linear outputs (transformers' LlamaMLP); bias must be NULL, N even */

/* y[M,N] = epi(x[M,K] . W[N,K]^T + bias) in fp16 with fp32 accumulation, for M of a few hundred rows (257 tokens per image) — replaces the nn.Linear calls
 * of SelfAttention.to_qkv / proj (model.py:82,89), AttentionBlock.mlp (:150-153) and, on the patch-major operand of x2v_clip_preprocess_f16 with
 * bias = NULL, VisionTransformer.patch_embedding (:253,278).  K % 32 == 0 (pad both operands with zero columns), N % 4 == 0; bias may be NULL.
 * Each output value is reduced in k order whatever M: rows of a batch equal the rows computed alone, bit for bit.  Every M from 0 (nothing launched) to
 * 4 194 240 (the grid's limit at the smallest tile) is admitted; the form streams W once per 64 or 128 rows and is meant for M up to a few thousand.
 * With X2V_EPI16_SWIGLU N counts y's columns, W has 2N rows and the tile is the one x2v_gemm_f16_tile_choice gives for (M, 2N). */
int x2v_gemm_f16(const void* x, int64_t ldx, const void* w, int64_t ldw, const void* bias, void* y, int64_t ldy, int64_t M, int N, int K, int epilogue,
                 const void* resid, int64_t ldr, void* stream);

/* The tile x2v_gemm_f16 launches for (M, N): 0 = 128 x 64, 1 = 64 x 64, 2 = 64 x 32, 3 = 64 x 16 (host arithmetic; no reference counterpart). */
int x2v_gemm_f16_tile_choice(int64_t M, int N);

/* out[b*S + i, h*80 : h*80 + 80] = softmax(scale * q_i . k_j) v_j over the S keys of image b, non-causal, head dim 80 — replaces
 * attention(q, k, v, attention_type="torch_sdpa") of SelfAttention.forward (model.py:82-86).  qkv is the to_qkv output [batch*S, >= 3*H*80] read in
 * place: q | k | v at columns 0, H*80, 2*H*80 of a row.  1 <= S <= 272; scale = 0 means 80^-1/2.  fp32 softmax statistics. */
int x2v_attn_f16_d80(const void* qkv, int64_t ld, void* out, int64_t ldo, int batch, int S, int num_heads, float scale, void* stream);

/* y[M,D] = fp16(LN(x; w, b, eps)) with fp32 statistics and fp32 w, b — replaces LayerNorm.forward (model.py:47-49: super().forward(x.float()).type_as(x)).
 * D % 8 == 0, D <= 2048. */
int x2v_layernorm_f16(const void* x, int64_t ldx, const float* w, const float* b, void* y, int64_t ldy, int64_t M, int D, float eps, void* stream);

/* y[b*tokens + t] = LN(fp16(tok + pos[t])), tok = cls for t = 0 and patches[b*(tokens-1) + t - 1] otherwise — replaces the concatenation with
 * cls_embedding, the pos_embedding add and pre_norm of VisionTransformer.forward (model.py:278-287).  pos is [tokens, D] fp16 contiguous. */
int x2v_clip_embed_f16(const void* patches, int64_t ldp, const void* cls, const void* pos, const float* w, const float* b, void* y, int64_t ldy, int batch,
                       int tokens, int D, float eps, void* stream);

/* One image [3, H, W] fp32 in [-1, 1] (read in place: channel / row strides in elements, unit column stride) -> the patch-major fp16 operand
 * out[(image_size/patch)^2, ld_out] of the patch-embedding GEMM, column c*patch^2 + py*patch + px, columns 3*patch^2 .. ld_out zeroed — replaces
 * F.interpolate(size=(224, 224), mode="bicubic", align_corners=False), mul_(0.5).add_(0.5) and Normalize(mean, std) of CLIPModel.visual (model.py:440-442,
 * constants :379-380) and the unfold that Conv2d(kernel = stride = patch) implies. */
int x2v_clip_preprocess_f16(const float* img, int64_t c_stride, int64_t row_stride, int H, int W, void* out, int64_t ld_out, int image_size, int patch,
                            float mean0, float mean1, float mean2, float std0, float std1, float std2, void* stream);

/* ---- umT5-XXL text encoder (bf16): the producer of text_encoder_output["context"] / ["context_null"] (runners/wan/wan_runner.py:178-191; the model is
 * models/input_encoders/hf/t5/model.py, T5Encoder.forward :314-347).  Its T5LayerNorm (:68-72) is x2v_rmsnorm_bf16 with X2V_ROUND_FP32. ---- */

/* epilogues of x2v_gemm_rows_bf16 */
#define X2V_EPIR_NONE 0     /* y = bf16(acc) */
#define X2V_EPIR_RESIDUAL 2 /* y = bf16(resid + bf16(acc)); y may alias resid          (x + self.attn(...) / x + self.ffn(...), t5/model.py:202-203) */
#define X2V_EPIR_GEGLU 3    /* W is [2N, K], row 2n = fc1 row n, row 2n + 1 = gate.0 row n: y = bf16(bf16(acc_fc1) * gelu_tanh(bf16(acc_gate))), the GELU
                             * in fp32 by the module's formula (:58)                     (self.fc1(x) * self.gate(x), :165) */

/* y[M,N] = epi(x[M,K] . W[N,K]^T) in bf16 with fp32 accumulation for 1 <= M <= 4096, the weight-streaming small-M form (the kernel of x2v_gemm_f16
 * instantiated for bf16) — replaces the bias-free nn.Linear calls of T5Attention q / k / v / o (t5/model.py:110-112,134; q, k, v as one [3 dim_attn, dim]
 * weight) and T5FeedForward gate.0 / fc1 / fc2 (:165,168).  K % 32 == 0, N % 4 == 0 (N % 2 == 0 and W of 2N rows with X2V_EPIR_GEGLU); resid is read by
 * X2V_EPIR_RESIDUAL only (else NULL).  Each output value is reduced in k order whatever M: rows of a packed batch equal the rows computed alone, bit for bit. */
int x2v_gemm_rows_bf16(const void* x, int64_t ldx, const void* w, int64_t ldw, void* y, int64_t ldy, int64_t M, int N, int K, int epilogue, const void* resid,
                       int64_t ldr, void* stream);

/* The tile x2v_gemm_rows_bf16 launches for (M, N, epilogue): 0 = 128 x 64, 1 = 64 x 64, 2 = 64 x 32, 3 = 64 x 16 rows of x by rows of W (host arithmetic;
 * no reference counterpart). */
int x2v_gemm_rows_bf16_tile_choice(int64_t M, int N, int epilogue);

/* out[r0_b + i, h*64 : h*64 + 64] = softmax_j(scale * q_i . k_j + bias[h][j - i + 511]) v_j over the keys of sequence b only, non-causal, head dim 64 —
 * replaces the einsum / attn_bias / softmax / einsum of T5Attention.forward (t5/model.py:115-129) with the block's T5RelativeEmbedding (:255-263) and the
 * padding mask (:121) folded in: `batch` <= 8 sequences of 1..512 tokens are packed row after row, sequence b being rows cu_seqlens[b] .. cu_seqlens[b+1] - 1
 * (r0_b = cu_seqlens[b]), and keys outside a query's own sequence never contribute.  cu_seqlens is a HOST array of batch + 1 increasing ints, passed on to
 * the kernel by value (no copy, no sync).  qkv is the fused q | k | v GEMM output read in place: columns 0, H*64, 2*H*64 of a row of stride ld.  bias is a
 * device table [H][1023] fp32, entry [h][d + 511] for key position - query position = d.  scale multiplies q . k as given (T5 passes 1: "T5 does not use
 * scaling", :123).  fp32 scores, bias and softmax statistics with the row maximum subtracted; P rounded to bf16 for the PV product, fp32 accumulation, one
 * rounding of the output. */
int x2v_attn_bf16_d64_relbias(const void* qkv, int64_t ld, const float* bias, void* out, int64_t ldo, const int* cu_seqlens, int batch, int num_heads,
                              float scale, void* stream);

/* ---- HunyuanVideo's text towers (fp16): the producers of text_encoder_output["text_encoder_1_text_states"] / ["text_encoder_2_text_states"]
 * (runners/hunyuan/hunyuan_runner.py:58-67) — transformers' LlamaModel behind input_encoders/hf/llama/model.py and CLIPTextModel behind
 * input_encoders/hf/clip/model.py.  Their Linears are x2v_gemm_f16 (X2V_EPI16_SWIGLU / X2V_EPI16_QUICK_GELU), CLIP's LayerNorm is x2v_layernorm_f16. ---- */

/* out[r0_b + i, h*d : h*d + d] = softmax_{j <= i}(scale * q_i . k_j) v_j over the keys 0..i of sequence b only: causal, grouped-query attention in fp16,
 * d = head_dim in {64, 128} — replaces apply_rotary_pos_emb, repeat_kv and the causal softmax attention of transformers' LlamaAttention.forward, and (with
 * the tables NULL, num_kv_heads = num_heads) CLIPAttention.forward under CLIPTextTransformer's causal mask.  `batch` <= 8 sequences of 1..512 tokens are
 * packed row after row, sequence b being rows cu_seqlens[b] .. cu_seqlens[b+1] - 1 (r0_b = cu_seqlens[b]); cu_seqlens is a HOST array of batch + 1
 * increasing ints, passed on to the kernel by value.  qkv is the fused projection output read in place: a row of stride ld holds q at column 0
 * (num_heads * d), k at num_heads * d (num_kv_heads * d) and v at (num_heads + num_kv_heads) * d; query head h reads key/value head
 * h / (num_heads / num_kv_heads); rows outside every sequence are neither read nor written.  rope_cos / rope_sin: device fp32 tables [>= 512][d / 2],
 * entry [p][i] = cos / sin(p * theta^(-2i/d)), or both NULL; given (head_dim 128 only, else X2V_E_ARG), q and k are rotated in fp32 at p = index within
 * the sequence, t * cos + cat(-t[d/2:], t[:d/2]) * sin with the table row repeated over both halves, and rounded once to fp16 as the matrix operands.
 * scale = 0 means d^-1/2.  fp32 scores, maximum, exp and sum (online over 64-key tiles); P rounded to fp16 for the PV product, fp32 accumulation, one
 * rounding of the output. */
int x2v_attn_f16_causal(const void* qkv, int64_t ld, void* out, int64_t ldo, const int* cu_seqlens, int batch, int num_heads, int num_kv_heads, int head_dim,
                        const float* rope_cos, const float* rope_sin, float scale, void* stream);

/* y[M,D] = fp16(w * x * rsqrt(mean(x^2) + eps)) with fp32 statistics and one rounding; x, w, y fp16 — replaces transformers' LlamaRMSNorm.forward, which
 * rounds x * rsqrt(...) to fp16 before the weight multiply and the product again.  D % 8 == 0, D <= 8192. */
int x2v_rmsnorm_f16(const void* x, int64_t ldx, const void* w, void* y, int64_t ldy, int64_t M, int D, float eps, void* stream);

/* Box calibration (measurement plumbing; no reference counterpart): runs bare v_mfma_f32_16x16x32_bf16 loops (operands in registers,
 * 8 waves per CU, every CU) for `milliseconds` on `stream` and returns in *tflops what the board sustained over the second half of that time.
 * bench.py calls it before and after its timed region so that a roofline fraction measured on one box can be compared with another's
 * (boxes of one pool differ by several percent under the 1400 W board limit).  Synchronises the stream. */
int x2v_mfma_probe_bf16(int milliseconds, float* tflops, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* X2V_H */
