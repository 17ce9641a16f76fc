"""float64 references, seeded inputs, fp32 restatements, case lists and the acceptance rules for the kernels that sit between the VAE convolutions
(lightx2v_amd/csrc/vae.hip: vae_prep_kernel, vae_prep_ex_kernel, vae_replicate_border_kernel, groupnorm_stats / finalize, softmax_rows_kernel,
softmax_rows_causal_kernel, blend_axis_kernel; vae_enc.hip: vae_video_prep_kernel).  Plain PyTorch; nothing here imports the library or the oracle.
Shared by tests/test_vae_pixel_ref_host.py (the yardstick and the rejection of subtly wrong kernels, without a GPU) and
tests/test_gpu_vae_pixel_fp64.py (the kernels against it), which take their cases from the lists at the end of this file.

Every function restates a contract of include/x2v.h, not a kernel, and takes `dtype`: float64 is the reference; float32 is the same formula with
every step rounded to fp32 — the stand-in for a correct fp32 kernel, with the fast exponential written as exp2(fp32(v * log2 e)).  The fp16 forms
return the float64 / fp32 value rounded once to fp16; the split form returns vae_conv_ref.split_x of it.

Two input families, as in the convolution suite; no share of elements is left out of either rule.

  I  exact: integers, power-of-two a / mul, integer b / add, dyadic blend weights, GroupNorm groups of m +- 2^k with eps = 0, constant and one-hot
     softmax rows.  No step rounds, so any correct kernel gives the reference's bits: check_exact asks for equality on every element.
  R  random, |x| <= 2^10 (fp32 sums of squares stay in range).  check_bound asks, on every element, |got - ref| <= tol and, over the case,
     relL2(got, ref) <= 1.5 Y with Y the relL2 of the fp32 restatement on the same inputs (1.5 = vae_conv_ref.MARGIN; Y never comes from a kernel).
     Where the contract leaves a choice open Y is the largest over the restatements that differ in it, as vae_conv_ref takes the largest over its
     orders: behind SiLU exp2 correctly rounded or an ulp off (fp32_restatements); for the softmaxes that, scale s - mx in two roundings or one,
     and the row sum by pairs or in the kernels' documented lane order (softmax_restatements).

Per-element bounds, unit U = 2^-23 = twice the round-to-nearest unit roundoff u, every rounding of the x2v.h formula counted as one U or less:
  affine      v = x / a + b or x * mul + add: one rounding on the quotient / product, one on the sum                  2 U (|x / a| + |b|)
  RMS norm    ss = sum of C squares in fp32: relative error <= C u in any order, halved by the square root = C/4 U; then sqrtf, the quotient
              sqrt(C) / ||v|| (its numerator rounded too), and the two products with inv and gamma: 5 roundings <= 2.5 U; 8 leaves room for the
              squares' own roundings and a fused or unfused order                                                      (C/4 + 8) U |ref|
  SiLU        v / (1 + exp(-v)): the argument v log2 e is rounded (relative u, i.e. |v| u absolute in the exponent, and as much again for the
              rounded constant) = |v| U on exp; the hardware exp2 is good to 1 ulp = 1 U; 1 + e and the quotient 1 U together; 4 + 1.5 |v| doubles
              the constant part and takes 1.5 |v| for the exponent's share.  An error t of the pre-activation adds 1.01 |silu'(v)| t (first
              order; the second-order term is below 1e-12 t)                                                           (4 + 1.5 |v|) U |ref|
  clamp01     1-Lipschitz: the bound passes through
  softmax     with A = max |scale s| of the row and N its reduced length: scale s - mx is rounded twice at magnitude <= 2 A (2 A U on the exponent),
              the exponent's conversion to base 2 another 2 A U, exp2 1 U; the same again, averaged, on the sum, plus the sum's own accumulation:
              256 lanes x 4 partial sums of N / 1024 terms, then a tree = N / 256 U at the most; 1 / sum and the product 1 U.  18 + 4 A + N / 256
              keeps a factor two on the constant part                                                                   (18 + 4 A + N/256) U ref
  GroupNorm   sums in fp64 (cancellation of mean^2 at mean / sigma = 64 is 4096 x 2^-53: invisible); rstd rounded to fp32 and multiplied by gamma:
              2 roundings on mul = 1 U, doubled twice for eps entering as an fp32 number                                mul: 4 U |ref|
              add = beta - fp32(mean) mul: mean's rounding, mul's own error, the product and the difference            add: 4 U (|beta| + |mean mul|)
  blend       idx / extent, 1 - w, two products and a sum                                                              4 U (|a| + |b|)
  fp16 out    + half an fp16 ulp of the reference (taken at |ref| + tol; 2^-25 below the fp16 normal range)
  split       hi + lo against ref: lo = fp16(x - hi) keeps 11 bits of a remainder below 2^-11 |x|                      + 2^-22 |ref| + 2^-25
  all         + 2^-126 absolute for results below the fp32 normal range (a kernel may flush them)
test_vae_pixel_ref_host.py shows every family-R case's fp32 restatement within HALF of its bound (the fp16 and split rounding terms, which a correct
rounding reaches, stay whole there; the softmaxes' other restatements are inside the whole bound): the bounds are satisfiable by a correct kernel.
Measured there: the restatement's worst |d| / bound is 0.08-0.16 of the softmax form at A = 3 and 0.22-0.36 at A = 40 (N = 4 .. 4100), 0.39 of the
SiLU form on [-80, 80], 0.15 of the RMS form.

Recorded yardsticks Y (largest relL2 of the fp32 restatement per operation over the family-R cases below):
  vae_prep f32 9.1e-8   f16 2.4e-4   split (hi + lo) 1.2e-7      vae_prep_ex f32 6.8e-8   f16 2.8e-4
  groupnorm mul 5.7e-8  add 1.1e-7   softmax_rows 6.0e-7   softmax_rows_causal 9.6e-8   blend_axis 4.4e-8

On an MI355X the kernels' largest |d| / bound is 0.48 where only fp32 terms count (1.0 where an fp16 rounding term is reached, as it must be) and the
largest relL2 / (1.5 Y) is 0.95 (vae_prep f32, C = 4, norm + SiLU: 168 values), 0.89 for the split, 0.82 for GroupNorm, below 0.7 for the softmaxes.

What the cases reach, per entry point:
  vae_prep f32      LPP 32 (C 4: one live lane per group; 16; 124 / 128: the last lane ragged / full), LPP 64 (132: the arm switch; 384; 1020 / 1024:
                    the fourth chunk step ragged / full); norm, norm + SiLU, + upsample; affine none / a / b / a + b, plain and upsampled
  vae_prep f16      LPP 8 (96), 16 (192), 32 (384; 4, 128), 64 (256, 1024); pixel stride C and the next multiple of 64 (pad channels keep the sentinel);
                    C = 4 at stride 4 is refused (strides are multiples of 8 halves) and asserted as a refusal
  vae_prep split    the same arms at 3 C and the next multiple of 64; mid and lo planes of all four upsampled pixels; the saturating values
  vae_prep_ex       LPP 32 (4, 8, 128), LPP 64 (136: one pass of its channel loop; 640: three, the last ragged; 1032 > 1024: a fifth pass, which vae_prep's
                    four fixed steps do not have); mul / add / both / none x
                    SiLU x clamp01 x up_hw x up_t, T = 1 (no frame duplicated), 2, 3
  grid-stride       npix = 8 * 262144 + 11: the second sweep has 8 live groups in block 0 and 3 in block 1 (C = 4 / 8, all four producers)
  replicate_border  lead 0..2 x pad 0..2, one interior pixel and ordinary sizes, C 4 and 64, fp16 pixels of 8 and 64 halves
  groupnorm_affine  a thread's group changes between iterations (96, 8; 128, 32: one chunk per group) or never (64, 1; 4, 1); G = 64 fills the LDS
                    array; npix 1, 7, 1000; 21851 pixels of 96 channels = 524424 chunks > 2048 x 256: the block cap and a second sweep; the offset
                    case; a second call on fresh inputs
  softmax_rows      1 pass (4, 64, 1020, 1024), 2 (1028), 5 passes (4100) of the 1024-float stride; M 1 and 5; ld = N and N + 12
  softmax_causal    valid <= 256 (1 pass), 300 / 600 (2 and 3 passes), 1000 (4 passes, Wan's form: only padding columns cut); padded rows; ld > N
  blend_axis        axes 0, 1, 2 (inner = everything behind the axis, outer in front), extent 0 (nothing launched), 1, 4, 8, 3, 5, 12 and clamped
  video_prep        modes 0, 1, 2 on a crop of a larger video (all three strides exceed the extents); pixel strides 3 / 16 and 9 / 64
Left out on purpose: the grid caps of replicate_border, blend_axis and video_prep (65536 * 4 blocks of 256 threads: 2^26 float4 chunks / elements /
pixels) need a GiB per tensor."""
import math
from collections import namedtuple

import torch

from tests.vae_conv_ref import F16, F32, F64, MARGIN, UNIT, Reject, _gen, rel_l2, split_x

LOG2E = 1.4426950408889634
TINY = 2.0 ** -126
SENTINEL = -1984.0  # exact in fp16 and fp32; no output of these cases equals it
LOUD = 3.0e4  # what masked and padding score columns hold
GEOMS = ((1, 1, 1), (2, 3, 5), (3, 2, 7))  # 1, 30 and 42 pixels: no multiple of 4, 8 or 32 (the pixel groups per block); W odd
SPLIT_SPECIALS = (65504.0, 65519.0, 65520.0, 1e5, 131008.0, 2e5, math.inf, 2.0 ** -14, 2.0 ** -24, 2.0 ** -25)  # each with both signs (2^-n: +)


def f32_scalar(v):
    """A Python number as the fp32 value a kernel receives."""
    return float(torch.tensor(v, dtype=F32))


# ------------------------------------------------------------------------------------------------------------------- formulas
_EXP_ULP = 0  # fp32_restatements: the fp32 exponential one ulp high (1) or low (-1)


def exp_(v):
    """exp(v): float64, or the fast fp32 form exp2(fp32(v * log2 e))."""
    if v.dtype == F64:
        return torch.exp(v)
    e = torch.exp2(v * LOG2E)
    return e if not _EXP_ULP else torch.nextafter(e, torch.full_like(e, math.inf) if _EXP_ULP > 0 else torch.zeros_like(e))


def fp32_restatements(fn, silu_):
    """[fn()] — an fp32 restatement — and, behind SiLU, the same with exp2 one ulp high and one ulp low on every element: the hardware's exp2 is
    specified to 1 ulp (the bound's derivation counts it), so a correct kernel may be any of them.  Y is the largest relL2 among them."""
    global _EXP_ULP
    out = [fn()]
    for d in (1, -1) if silu_ else ():
        _EXP_ULP = d
        try:
            out.append(fn())
        finally:
            _EXP_ULP = 0
    return out


def silu(v):
    return v / (1 + exp_(-v))


def dsilu(v):
    s = torch.sigmoid(v)
    return s * (1 + v * (1 - s))


def up_hw(v):
    """nearest x2 in H and W of [T, H, W, C]."""
    return v.repeat_interleave(2, 1).repeat_interleave(2, 2)


def up_t(v, mut=None):
    """nearest x2 in T where frame 0 is not duplicated: [T, ...] -> [2 T - 1, ...]."""
    if mut == "up_t_dup0":  # frame 0 duplicated, the last frame once
        return v.repeat_interleave(2, 0)[: 2 * v.shape[0] - 1]
    return torch.cat([v[:1], v[1:].repeat_interleave(2, 0)])


def lpp_of(C, f16):
    """Lanes per pixel of vae_prep_kernel (vae.hip x2v_vae_prep_f32 / vae_prep_f16_impl)."""
    if f16 and C // 4 in (24, 48, 96):
        return C // 12
    return 32 if C <= 128 else 64


def vae_prep(x, gamma=None, a=None, b=None, silu_=False, upsample=False, dtype=F64, mut=None, lpp=64):
    """x2v_vae_prep_f32: x [T, H, W, C] -> [T, H, W, C] (upsample: [T, 2 H, 2 W, C]) in `dtype`."""
    v = x.to(dtype).clone()
    C = v.shape[-1]
    if mut == "drop_k3":  # the fourth chunk step dropped: channels from 12 LPP up are neither read nor written
        v[..., 12 * lpp :] = 0
    if gamma is not None:
        ss = (v * v).sum(-1, keepdim=True)
        inv = torch.tensor(float(C), dtype=dtype).sqrt() / ss.sqrt().clamp_min(1e-12)
        v = v * inv * gamma.to(dtype)
    else:
        if a is not None:
            v = v / a.to(dtype)
        if b is not None:
            v = v + b.to(dtype)
    if silu_:
        v = silu(v)
    if mut == "drop_k3":
        v[..., 12 * lpp :] = 0
    if upsample:
        v = up_hw(v)
        if mut == "up3":  # three of the four pixels written
            v[:, 1::2, 1::2] = 0
    return v


def vae_prep_f16(*args, **kw):
    """x2v_vae_prep_f16: the value of vae_prep rounded once to fp16 (pad channels are the caller's)."""
    return vae_prep(*args, **kw).to(F16)


def split_planes(v, mut=None):
    if mut == "split_nosat":  # hi = fp16(x) overflows, lo = fp16(x - hi)
        hi = v.to(F16)
        return torch.cat([hi, (hi.to(F64) * 2.0 ** -12).to(F16), (v.to(F64) - hi.to(F64)).to(F16)], dim=-1)
    return split_x(v)


def vae_prep_split_f16(*args, mut=None, **kw):
    """x2v_vae_prep_split_f16: [hi | hi 2^-12 | lo] of the value of vae_prep."""
    return split_planes(vae_prep(*args, mut=mut, **kw), mut)


def vae_prep_ex(x, mul=None, add=None, silu_=False, clamp01=False, up_hw_=False, up_t_=False, dtype=F64, mut=None):
    """x2v_vae_prep_ex_f32: v = x * mul + add, SiLU, clamp to [0, 1], nearest x2 in H, W and / or T (frame 0 not duplicated)."""
    v = x.to(dtype).clone()
    if mul is not None:
        v = v * mul.to(dtype)
    if add is not None:
        v = v + add.to(dtype)
    if silu_:
        v = silu(v)
    if clamp01:
        v = v.clamp(0.0, 1.0)
    if up_hw_:
        v = up_hw(v)
    if up_t_:
        v = up_t(v, mut)
    return v


def vae_prep_ex_f16(*args, **kw):
    return vae_prep_ex(*args, **kw).to(F16)


def replicate_border(buf, lead, pad, mut=None):
    """x2v_vae_replicate_border_f32 on [frames, Hp, Wp, C] of any dtype: pure data movement."""
    Fr, Hp, Wp, _ = buf.shape
    f, h, w = torch.arange(Fr), torch.arange(Hp), torch.arange(Wp)
    fi, hi, wi = f.clamp_min(lead), h.clamp(pad, Hp - 1 - pad), w.clamp(pad, Wp - 1 - pad)
    if mut == "lead_from_0":
        fi = torch.where(f < lead, torch.zeros_like(f), f)
    if mut == "border_far":  # the far edge of the interior instead of the nearest interior pixel
        hi = torch.where(h < pad, torch.full_like(h, Hp - 1 - pad), torch.where(h > Hp - 1 - pad, torch.full_like(h, pad), h))
        wi = torch.where(w < pad, torch.full_like(w, Wp - 1 - pad), torch.where(w > Wp - 1 - pad, torch.full_like(w, pad), w))
    return buf[fi][:, hi][:, :, wi].clone()


def groupnorm_stats(x, G, mut=None):
    """(mean, var) per group of x [npix, C] in float64 (the contract: fp64 accumulation), var = max(E x^2 - mean^2, 0)."""
    npix, C = x.shape
    cpg = C // G
    xs = x.roll(-4, 1) if mut == "grp_shift" else x  # every chunk counted to the group of the chunk behind it
    count = (-(-npix // 8) * 8 if mut == "count_pad" else npix) * cpg
    if mut == "acc_fp32":
        xg = xs.to(F32).view(npix, G, cpg)
        s, q = xg.sum((0, 2)), (xg * xg).sum((0, 2))
        mean = s / count
        return mean.to(F64), (q / count - mean * mean).clamp_min(0).to(F64)
    xg = xs.to(F64).view(npix, G, cpg)
    mean = xg.sum((0, 2)) / count
    return mean, ((xg * xg).sum((0, 2)) / count - mean * mean).clamp_min(0)


def groupnorm_affine(x, G, gamma, beta, eps, dtype=F64, mut=None):
    """x2v_groupnorm_affine_f32: (mul, add) [C] with GroupNorm(x)[:, c] = x[:, c] mul[c] + add[c].  eps is the fp32 number the entry receives."""
    cpg = x.shape[1] // G
    mean, var = groupnorm_stats(x, G, mut)
    rstd = 1.0 / (var + f32_scalar(eps)).sqrt()
    mean, rstd = mean.repeat_interleave(cpg), rstd.repeat_interleave(cpg)
    mul = rstd.to(dtype) * gamma.to(dtype)
    return mul, beta.to(dtype) - mean.to(dtype) * mul


def groupnorm_tol(x, G, gamma, beta, eps):
    mean, _ = groupnorm_stats(x, G)
    mul, _ = groupnorm_affine(x, G, gamma, beta, eps)
    return 4 * UNIT * mul.abs() + TINY, 4 * UNIT * (beta.to(F64).abs() + (mean.repeat_interleave(x.shape[1] // G) * mul).abs()) + TINY


def causal_valid(M, N, hw, n_keys, mut=None):
    """Keys row i sees: min(n_keys, (i / hw + 1) hw)."""
    fr = torch.arange(M) // hw
    v = (fr + (2 if mut == "valid_frame" else 1)) * hw + (1 if mut == "valid_key" else 0)
    return v.clamp_max(n_keys)


def softmax_rows(s, scale, valid=None, dtype=F64, mut=None):
    """x2v_softmax_rows_f32 (valid = None) / x2v_softmax_rows_causal_f32 (valid [M] from causal_valid): softmax(scale s) over the first valid[i]
    columns of row i, 0 behind them.  scale is the fp32 number the entry receives."""
    M, N = s.shape
    valid = torch.full((M,), N) if valid is None else valid
    live = torch.arange(N)[None, :] < valid[:, None]
    v, sc = s.to(dtype), f32_scalar(scale)
    if dtype == F64:
        z = (v * sc).masked_fill(~live, -math.inf)
        e = torch.exp(z - z.max(1, keepdim=True).values)
        return e / e.sum(1, keepdim=True)
    seen = torch.ones_like(live) if mut == "max_all" else live
    mx = v.masked_fill(~seen, -3.0e38).max(1, keepdim=True).values * sc
    e = exp_(v * sc - mx).masked_fill(~live, 0.0)
    out = e * (1.0 / e.sum(1, keepdim=True))
    return torch.where(live, out, v) if mut == "masked_unnormalised" else out


def _sum_orders(e, vec):
    """Row sums of fp32 e [M, N] in two orders: torch's pairwise sum, and the documented order of the kernels — 256 lanes, lane t chaining the `vec`
    consecutive floats at vec t + 256 vec k (vec = 4: (x + y) + (z + w) first), then the xor butterfly over each wave of 64 and a chain over the four
    waves (x2v_common.h block_sum)."""
    M, N = e.shape
    ep = torch.cat([e, torch.zeros(M, -N % (256 * vec))], 1).view(M, -1, 256, vec)
    part = torch.zeros(M, 256)
    for k in range(ep.shape[1]):
        part = part + ((ep[:, k, :, 0] + ep[:, k, :, 1]) + (ep[:, k, :, 2] + ep[:, k, :, 3]) if vec == 4 else ep[:, k, :, 0])
    w, lane = part.view(M, 4, 64), torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):  # wave_sum: v += shfl_xor(v, o)
        w = w + w[..., lane ^ o]
    tot = torch.zeros(M)
    for i in range(4):  # block_sum: lane 0 of each wave, chained
        tot = tot + w[:, i, 0]
    return e.sum(1, keepdim=True), tot[:, None]


def softmax_restatements(s, scale, valid=None, vec=4):
    """The fp32 restatements of softmax_rows that differ only in what x2v.h leaves open: scale s - mx rounded twice or fused into one rounding; the
    exponential correctly rounded, or one ulp high, or one ulp low on every entry (the hardware's exp2 is specified to 1 ulp, which the bound's
    derivation counts as well); the row sum by pairs or in the kernels' documented lane order (_sum_orders).  The first is
    softmax_rows(dtype=float32) itself.  Y is the largest relL2 among them, as vae_conv_ref takes the largest over its chain and slab orders: the
    relL2 of a near one-hot row is one or two roundings of 1 / sum (an entry near 2^-24 beside a 1 tips the sum by an ulp, the quotient by two),
    and which way they fall depends on these choices and on nothing else."""
    M, N = s.shape
    valid = torch.full((M,), N) if valid is None else valid
    live = torch.arange(N)[None, :] < valid[:, None]
    v, sc = s.to(F32), torch.tensor(f32_scalar(scale), dtype=F32)
    mx = v.masked_fill(~live, -3.0e38).max(1, keepdim=True).values * sc
    out = []
    for z in (v * sc - mx, (v.to(F64) * sc.to(F64) - mx.to(F64)).to(F32)):
        e0 = exp_(z)
        for e in (e0, torch.nextafter(e0, torch.full_like(e0, 4.0)), torch.nextafter(e0, torch.zeros_like(e0))):
            e = e.masked_fill(~live, 0.0)
            out += [e * (1.0 / sm) for sm in _sum_orders(e, vec)]
    return out


def softmax_tol(s, scale, valid=None):
    M, N = s.shape
    valid = torch.full((M,), N) if valid is None else valid
    live = torch.arange(N)[None, :] < valid[:, None]
    A = (s.to(F64) * f32_scalar(scale)).abs().masked_fill(~live, 0.0).max(1, keepdim=True).values
    return (18 + 4 * A + valid[:, None].to(F64) / 256) * UNIT * softmax_rows(s, scale, valid) + TINY * live


def blend_axis(a, b, axis, extent, dtype=F64, mut=None):
    """x2v_blend_axis_f32 behind the wrapper's clamp: b[idx] = a[na - e + idx] (1 - idx / e) + b[idx] (idx / e), idx < e = min(extent, na, nb)."""
    na, nb = a.shape[axis], b.shape[axis]
    e = min(extent, na, nb)
    out, av = b.to(dtype).clone(), a.to(dtype)
    for idx in range(e):
        w = torch.tensor(float(idx), dtype=dtype) / torch.tensor(float(max(e - 1, 1) if mut == "w_extent_m1" else e), dtype=dtype)
        src = na - e + idx - (1 if mut == "src_m1" else 0)
        out.select(axis, idx).copy_(av.select(axis, src) * (1 - w) + out.select(axis, idx) * w)
    return out


def blend_tol(a, b, axis, extent):
    na, nb = a.shape[axis], b.shape[axis]
    e = min(extent, na, nb)
    tol = torch.zeros(b.shape, dtype=F64)
    if e:
        tol.narrow(axis, 0, e).copy_(4 * UNIT * (a.to(F64).narrow(axis, na - e, e).abs() + b.to(F64).narrow(axis, 0, e).abs()) + TINY)
    return tol


def video_prep(video, mode):
    """x2v_vae_video_prep: video [3, T, H, W] fp32 -> channels-last [T, H, W, 3] fp32 (mode 0), fp16 (1) or the split's 9 halves (2)."""
    v = video.permute(1, 2, 3, 0).contiguous()
    return v if mode == 0 else v.to(F16) if mode == 1 else split_x(v)


# ------------------------------------------------------------------------------------------------------------------- bounds of the producers
def half_ulp16(r):
    """Half an fp16 ulp at magnitude r (float64, >= 0): 2^-25 below the normal range."""
    return torch.exp2(torch.floor(torch.log2(r.clamp_min(2.0 ** -14))) - 11)


def _through_silu(v, t):
    """The bound behind SiLU of a pre-activation v (float64) known to t."""
    return (4 + 1.5 * v.abs()) * UNIT * silu(v).abs() + 1.01 * dsilu(v).abs() * t


def prep_tol(x, gamma=None, a=None, b=None, silu_=False, upsample=False):
    """Per-element fp32 bound of vae_prep on these inputs (float64)."""
    v, xd = vae_prep(x, gamma, a, b), x.to(F64)
    if gamma is not None:
        t = (x.shape[-1] / 4 + 8) * UNIT * v.abs()
    elif a is not None or b is not None:
        t = 2 * UNIT * ((xd / a.to(F64) if a is not None else xd).abs() + (b.to(F64).abs() if b is not None else 0.0))
    else:
        t = torch.zeros_like(v)
    if silu_:
        t = _through_silu(v, t)
    t = t + TINY
    return up_hw(t) if upsample else t


def ex_tol(x, mul=None, add=None, silu_=False, clamp01=False, up_hw_=False, up_t_=False):
    v, xd = vae_prep_ex(x, mul, add), x.to(F64)
    if mul is not None or add is not None:
        t = 2 * UNIT * ((xd * mul.to(F64) if mul is not None else xd).abs() + (add.to(F64).abs() if add is not None else 0.0))
    else:
        t = torch.zeros_like(v)
    if silu_:
        t = _through_silu(v, t)
    t = t + TINY
    t = up_hw(t) if up_hw_ else t
    return up_t(t) if up_t_ else t


def f16_tol(ref, tol):
    return tol + half_ulp16(ref.abs() + tol)


# ------------------------------------------------------------------------------------------------------------------- acceptance
def check_exact(got, want, tag):
    """Family I: got equals want on every element (same dtype and shape; NaN equals NaN)."""
    if got.shape != want.shape or got.dtype != want.dtype:
        raise Reject("shape", f"{tag}: {tuple(got.shape)} {got.dtype} vs {tuple(want.shape)} {want.dtype}")
    want = want.to(got.device)
    ne = ~((got == want) | (torch.isnan(got) & torch.isnan(want)))
    bad = int(ne.sum())
    if bad:
        i = tuple(int(v) for v in ne.nonzero()[0])
        raise Reject("exact", f"{tag}: {bad} of {got.numel()} elements differ from the float64 result; first at {i}: got {float(got[i])!r} want {float(want[i])!r}")
    return 0


def check_bits(got, want, tag):
    """Data movement: the same bit patterns."""
    it = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[got.element_size()]
    if got.shape != want.shape or got.dtype != want.dtype:
        raise Reject("shape", f"{tag}: {tuple(got.shape)} {got.dtype} vs {tuple(want.shape)} {want.dtype}")
    ne = got.contiguous().view(it) != want.to(got.device).contiguous().view(it)
    if bool(ne.any()):
        raise Reject("exact", f"{tag}: {int(ne.sum())} of {got.numel()} bit patterns differ; first at {tuple(int(v) for v in ne.nonzero()[0])}")
    return 0


def check_bound(got, ref, tol, y32, tag):
    """Family R: finite, |got - ref| <= tol on every element, relL2(got, ref) <= 1.5 Y with Y = relL2(y32, ref), y32 the fp32 restatement's result.
    Returns (largest |d| / tol, relL2 / Y)."""
    g = got.to(ref.device).to(F64)
    if g.shape != ref.shape:
        raise Reject("shape", f"{tag}: {tuple(g.shape)} vs {tuple(ref.shape)}")
    if not bool(torch.isfinite(g).all()):
        raise Reject("finite", f"{tag}: non-finite output")
    err = (g - ref).abs()
    ratio = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if worst > 1.0:
        i = tuple(int(v) for v in (ratio == ratio.max()).nonzero()[0])
        raise Reject("bound", f"{tag}: {int((ratio > 1).sum())} of {g.numel()} elements outside the bound; worst |d| / bound {worst:.3f} at {i}: got {float(g[i]):.9g} "
                              f"ref {float(ref[i]):.9g} bound {float(tol[i]):.3g}")
    Y, r = max(rel_l2(y, ref) for y in (y32 if isinstance(y32, (list, tuple)) else [y32])), rel_l2(g, ref)
    if r > MARGIN * Y:
        raise Reject("yardstick", f"{tag}: relL2 {r:.3e} > {MARGIN} x Y = {MARGIN * Y:.3e}")
    return worst, (r / Y if Y > 0 else 0.0)


def check_split(got, ref, tol, y32, tag):
    """The split's planes [hi | mid | lo] (fp16 [..., 3 C]) against the float64 value ref [..., C] known to tol in fp32: mid == fp16(hi 2^-12)
    exactly, hi within the fp16 bound, hi + lo within tol + 2^-22 |ref| + 2^-25 and the yardstick of the restatement's hi + lo."""
    C, ys = ref.shape[-1], (y32 if isinstance(y32, (list, tuple)) else [y32])
    hi, mid, lo = (got[..., k * C : (k + 1) * C] for k in range(3))
    check_exact(mid, (hi.to(F64) * 2.0 ** -12).to(F16), tag + " mid plane")
    check_bound(hi, ref, f16_tol(ref, tol), [y[..., :C] for y in ys], tag + " hi plane")
    return check_bound(hi.to(F64) + lo.to(F64), ref, tol + 2.0 ** -22 * ref.abs() + 2.0 ** -25, [y[..., :C].to(F64) + y[..., 2 * C :].to(F64) for y in ys], tag + " hi + lo")


# ------------------------------------------------------------------------------------------------------------------- layout
def framed(T, H, W, ps, lead, dtype, device="cpu"):
    """A sentinel-filled [lead + T, H + 2, W + 2, ps] buffer and its interior view [T, H, W, ps]: a 1-pixel border, `lead` frames in front."""
    buf = torch.full((lead + T, H + 2, W + 2, ps), SENTINEL, dtype=dtype, device=device)
    return buf, buf[lead:, 1 : H + 1, 1 : W + 1]


def frame_intact(buf, lead, written):
    """Everything but channels [0, written) of the interior still holds the sentinel."""
    chk = buf.clone()
    chk[lead:, 1:-1, 1:-1, :written] = SENTINEL
    return bool((chk == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------------- inputs
_Mode = namedtuple("Mode", "gamma a b silu up")
_Ex = namedtuple("Ex", "mul add silu clamp up_hw up_t")


def mode_name(m):
    return "+".join(k for k, on in zip(m._fields, m) if on) or "copy"


def prep_inputs(family, C, geom, mode, seed=0):
    """(x, gamma, a, b) for vae_prep.  I: integers in [-8, 8], a a power of two, b an integer.  R: the norm path N(0, 1) * 2^k per pixel, k in -6..9
    clipped to 2^10, gamma N(0, 1) * 2 (pre-activations to about +-25), pixel 0 all zero; the affine path a in [0.5, 2], b N(0, 1) and x such that
    x / a + b is uniform in [-79, 79] (SiLU's range: below -88.7 the formula's exp overflows and the result is -0)."""
    g = _gen("IR".index(family), C, *geom, *[int(v) for v in mode], seed, 11)
    T, H, W = geom
    if family == "I":
        x = torch.randint(-8, 9, (T, H, W, C), generator=g).to(F32)
        a = torch.exp2(torch.randint(-2, 3, (C,), generator=g).to(F32))
        b = torch.randint(-16, 17, (C,), generator=g).to(F32)
        gamma = None
        assert not mode.gamma and not mode.silu
    elif mode.gamma:
        x = (torch.randn(T, H, W, C, generator=g) * torch.exp2(torch.randint(-6, 10, (T, H, W, 1), generator=g).to(F32))).clamp(-1024.0, 1024.0)
        x[0, 0, 0] = 0.0
        gamma, a, b = torch.randn(C, generator=g) * 2, None, None
    else:
        a = torch.rand(C, generator=g) * 1.5 + 0.5
        b = torch.randn(C, generator=g)
        x = (torch.rand(T, H, W, C, generator=g) * 158 - 79 - (b if mode.b else 0.0)) * (a if mode.a else 1.0)  # x / a + b in [-79, 79] before rounding
        gamma = None
    return x, gamma, (a if mode.a else None), (b if mode.b else None)


def with_specials(x):
    """x with the split's saturating and subnormal values in its first elements (flat order)."""
    vals = [s * v for v in SPLIT_SPECIALS[:7] for s in (1.0, -1.0)] + list(SPLIT_SPECIALS[7:])
    x = x.clone()
    flat = x.view(-1)
    n = min(len(vals), flat.numel())
    flat[:n] = torch.tensor(vals[:n], dtype=F32)
    return x


def ex_inputs(family, C, geom, ex, seed=0):
    """(x, mul, add) for vae_prep_ex.  I: integers in [-8, 8], mul in 2^-3..2^0, add in -1..1: values on both sides of and inside [0, 1].
    R: mul in [0.5, 1.5) with a random sign, add N(0, 1), x such that x mul + add is N(0, 1) * 20 clipped to +-79 (SiLU's range;
    / 40 for the clamp alone)."""
    g = _gen("IR".index(family), C, *geom, *[int(v) for v in ex], seed, 12)
    T, H, W = geom
    if family == "I":
        assert not ex.silu
        x = torch.randint(-8, 9, (T, H, W, C), generator=g).to(F32)
        mul = torch.exp2(torch.randint(-3, 1, (C,), generator=g).to(F32))
        add = torch.randint(-1, 2, (C,), generator=g).to(F32)
    else:
        mul = (torch.rand(C, generator=g) + 0.5) * (torch.randint(0, 2, (C,), generator=g) * 2 - 1).to(F32)
        add = torch.randn(C, generator=g)
        x = (torch.randn(T, H, W, C, generator=g) * 20).clamp(-79.0, 79.0) / (40 if ex.clamp and not ex.silu else 1)
        x = (x - (add if ex.add else 0.0)) / (mul if ex.mul else 1.0)
    return x, (mul if ex.mul else None), (add if ex.add else None)


def groupnorm_inputs(family, C, G, npix, seed=0, offset=False):
    """(x [npix, C], gamma, beta, eps).  I: group g holds m_g + 2^k_g and m_g - 2^k_g in equal numbers (C / G is a multiple of 4, so every pixel holds
    as many of one as of the other), eps = 0, gamma and beta multiples of 1/8: the fp64 sums are exact in any order, rstd = 2^-k_g, mul and add exact.
    R: N(mu_g, sigma_g^2), sigma_g in [0.5, 4]; offset: mu_g = 64 sigma_g."""
    g = _gen("IR".index(family), C, G, npix, seed, int(offset), 13)
    cpg = C // G
    if family == "I":
        m, k = torch.randint(-5, 6, (G,), generator=g).to(F32), torch.randint(-2, 4, (G,), generator=g).to(F32)
        sign = torch.tensor([1.0, -1.0]).repeat(cpg // 2)
        perm = torch.stack([torch.randperm(cpg, generator=g) for _ in range(min(npix, 16))])[torch.arange(npix) % min(npix, 16)]  # [npix, cpg]
        x = m[None, :, None] + sign[perm][:, None, :] * torch.exp2(k)[None, :, None]
        x = x.reshape(npix, C)
        return x, torch.randint(-16, 17, (C,), generator=g).to(F32) / 8, torch.randint(-16, 17, (C,), generator=g).to(F32) / 8, 0.0
    sigma = torch.rand(G, generator=g) * 3.5 + 0.5
    mu = 64 * sigma if offset else torch.randn(G, generator=g) * 2
    x = (mu[None, :, None] + sigma[None, :, None] * torch.randn(npix, G, cpg, generator=g)).reshape(npix, C)
    return x, 1 + 0.5 * torch.randn(C, generator=g), torch.randn(C, generator=g), 1e-6


def softmax_inputs(M, N, scale, A, seed=0):
    """s [M, N] N(0, 1) rescaled so that max |scale s| = A."""
    u = torch.randn(M, N, generator=_gen(M, N, int(scale * 1e6), A, seed, 14))
    return u / u.abs().max() * (A / f32_scalar(scale))


def causal_inputs(hw, frames, N, n_keys, scale, A, seed=0):
    """s [N, N] as softmax_inputs; the padding columns n_keys .. N hold LOUD (a row maximum taken over them underflows every live entry)."""
    s = softmax_inputs(N, N, scale, A, seed + 7 * hw + frames)
    s[:, n_keys:] = LOUD
    return s


# ------------------------------------------------------------------------------------------------------------------- cases
Mode = lambda gamma=False, a=False, b=False, silu=False, up=False: _Mode(gamma, a, b, silu, up)  # noqa: E731
Ex = lambda mul=False, add=False, silu=False, clamp=False, up_hw=False, up_t=False: _Ex(mul, add, silu, clamp, up_hw, up_t)  # noqa: E731

PREP_F32_C = (4, 16, 124, 128, 132, 384, 1020, 1024)
PREP_MODES_I = [Mode(a=a, b=b, up=up) for up in (False, True) for a, b in ((False, False), (True, False), (False, True), (True, True))]
PREP_MODES_R = [Mode(gamma=True), Mode(gamma=True, silu=True), Mode(gamma=True, silu=True, up=True)] + \
               [Mode(a=a, b=b, up=up) for up in (False, True) for a, b in ((True, False), (False, True), (True, True))] + [Mode(a=True, b=True, silu=True)]
PREP_F16_C = (4, 96, 192, 384, 128, 256, 1024)
PREP16_MODES_I = [Mode(), Mode(a=True), Mode(b=True, up=True), Mode(a=True, b=True, up=True)]
PREP16_MODES_R = [Mode(gamma=True), Mode(gamma=True, silu=True, up=True), Mode(a=True, b=True, silu=True), Mode(a=True, b=True, up=True)]


def next64(n):
    return (n // 64 + 1) * 64


EX_F32_C = (4, 8, 128, 136, 640, 1032)
EX_F16_C = (8, 128, 136, 640, 1032)
EX_I = [Ex(), Ex(mul=True, up_hw=True), Ex(add=True, up_t=True), Ex(mul=True, add=True, up_hw=True, up_t=True), Ex(mul=True, add=True, clamp=True),
        Ex(mul=True, clamp=True, up_hw=True, up_t=True), Ex(add=True, clamp=True, up_t=True), Ex(clamp=True, up_hw=True)]
EX_R = [Ex(mul=True, add=True), Ex(mul=True, add=True, silu=True), Ex(mul=True, add=True, silu=True, up_hw=True, up_t=True), Ex(add=True, silu=True, clamp=True, up_t=True),
        Ex(silu=True, up_t=True), Ex(mul=True, silu=True, clamp=True, up_hw=True), Ex(mul=True, add=True, clamp=True, up_hw=True)]

GRID_NPIX = 8 * 262144 + 11

BORDER_CASES = [(lead, pad, 2 * pad + dh, 2 * pad + dw, C) for lead in (0, 1, 2) for pad in (0, 1, 2) for dh, dw in ((1, 1), (3, 4)) for C in (4, 64)]  # (lead, pad, Hp, Wp, C)
BORDER_F16_HALVES = (8, 64)

GN_SHAPES = ((4, 1), (64, 1), (128, 32), (512, 32), (96, 8), (256, 64))
GN_NPIX = (1, 7, 1000)
GN_CAP = (96, 8, 21851)

SOFTMAX_N = (4, 64, 1020, 1024, 1028, 4100)
SOFTMAX_M = (1, 5)
SOFTMAX_SCALES = (0.25, 1 / math.sqrt(384))
SOFTMAX_A = (3, 40)
CAUSAL_CASES = ((1, 5, 16, 5, 16), (6, 3, 32, 18, 32), (300, 2, 608, 600, 608), (16, 1, 16, 16, 16), (1008, 1, 1008, 1000, 1008), (5, 3, 15, 15, 15),
                (6, 3, 32, 18, 44))  # (hw, frames, N, n_keys, ld)

BLEND_BASE, BLEND_NA, BLEND_NB = (2, 3, 5, 4), 13, 14
BLEND_EXTENTS_I = (0, 1, 4, 8)
BLEND_EXTENTS_R = (3, 5, 12, 20)  # 20 > min(na, nb): the wrapper clamps to 13


def blend_inputs(family, axis, extent, seed=0):
    """a, b [T, H, W, C] with na = 13, nb = 14 along `axis`.  I: integers in [-8, 8] (with extent a power of two every product and sum is exact)."""
    g = _gen("IR".index(family), axis, extent, seed, 15)
    sa, sb = list(BLEND_BASE), list(BLEND_BASE)
    sa[axis], sb[axis] = BLEND_NA, BLEND_NB
    if family == "I":
        return torch.randint(-8, 9, sa, generator=g).to(F32), torch.randint(-8, 9, sb, generator=g).to(F32)
    return torch.randn(sa, generator=g), torch.randn(sb, generator=g)


VIDEO_GEOM = (2, 3, 13)
VIDEO_STRIDES = {0: (3, 16), 1: (3, 16), 2: (9, 64)}


def video_crop(big):
    T, H, W = VIDEO_GEOM
    return big[:, 1:, 1 : 1 + H, 2 : 2 + W]


def video_inputs(seed=0):
    """(big, video_crop(big)): a [3, 2, 3, 13] crop (unit W stride) of a larger N(0, 1) * 3 video, the split's special values in its first elements."""
    T, H, W = VIDEO_GEOM
    big = torch.randn(3, T + 1, H + 2, W + 3, generator=_gen(T, H, W, seed, 16)) * 3
    vals = [s * v for v in SPLIT_SPECIALS[:7] for s in (1.0, -1.0)] + list(SPLIT_SPECIALS[7:])
    crop = video_crop(big)
    for i, v in enumerate(vals):
        crop[i % 3, (i // 3) // (H * W) % T, (i // 3) // W % H, (i // 3) % W] = v
    return big, crop


# ------------------------------------------------------------------------------------------------------------------- acceptance per entry point
def prep_eval(kind, x, gamma, a, b, mode, dtype, mut=None, lpp=64):
    fn = {"f32": vae_prep, "f16": vae_prep_f16, "split": vae_prep_split_f16}[kind]
    return fn(x, gamma, a, b, mode.silu, mode.up, dtype=dtype, mut=mut, lpp=lpp)


def accept_prep(kind, family, C, geom, mode, got=None, x=None, share=1.0):
    """The acceptance of one vae_prep case on `got` (default: the fp32 restatement).  share: the fp32 term of the bound scaled (0.5: the restatement's
    own test; the fp16 rounding terms stay whole, a correct rounding reaches them).  Returns (worst, relL2 of the restatement)."""
    tag = f"vae_prep {kind} {family} C={C} {geom} {mode_name(mode)}"
    xs, gamma, a, b = prep_inputs(family, C, geom, mode)
    x = xs if x is None else x
    ys = fp32_restatements(lambda: prep_eval(kind, x, gamma, a, b, mode, F32), mode.silu)
    got = ys[0] if got is None else got
    if family == "I":
        return check_exact(got, prep_eval(kind, x, gamma, a, b, mode, F64).to(got.dtype), tag), 0.0
    ref, tol = vae_prep(x, gamma, a, b, mode.silu, mode.up), prep_tol(x, gamma, a, b, mode.silu, mode.up)
    if kind == "split":
        for y in ys[1:]:
            check_split(y, ref, tol, ys, tag + " (exp2 an ulp off)")
        return check_split(got, ref, share * tol, ys, tag)[0], max(rel_l2(y[..., :C].to(F64) + y[..., 2 * C :].to(F64), ref) for y in ys)
    wrap = (lambda t: f16_tol(ref, t)) if kind == "f16" else (lambda t: t)
    for y in ys[1:]:
        check_bound(y, ref, wrap(tol), ys, tag + " (exp2 an ulp off)")
    return check_bound(got, ref, wrap(share * tol), ys, tag)[0], max(rel_l2(y, ref) for y in ys)


def accept_ex(kind, family, C, geom, ex, got=None, share=1.0):
    tag = f"vae_prep_ex {kind} {family} C={C} {geom} {mode_name(ex)}"
    x, mul, add = ex_inputs(family, C, geom, ex)
    fn = vae_prep_ex if kind == "f32" else vae_prep_ex_f16
    ys = fp32_restatements(lambda: fn(x, mul, add, *ex[2:], dtype=F32), ex.silu)
    got = ys[0] if got is None else got
    if family == "I":
        return check_exact(got, fn(x, mul, add, *ex[2:]).to(got.dtype), tag), 0.0
    ref, tol = vae_prep_ex(x, mul, add, *ex[2:]), ex_tol(x, mul, add, *ex[2:])
    wrap = (lambda t: f16_tol(ref, t)) if kind == "f16" else (lambda t: t)
    for y in ys[1:]:
        check_bound(y, ref, wrap(tol), ys, tag + " (exp2 an ulp off)")
    return check_bound(got, ref, wrap(share * tol), ys, tag)[0], max(rel_l2(y, ref) for y in ys)


def accept_groupnorm(family, C, G, npix, offset=False, got=None, seed=0):
    tag = f"groupnorm {family} C={C} G={G} npix={npix}" + (" offset" if offset else "")
    x, gamma, beta, eps = groupnorm_inputs(family, C, G, npix, seed, offset)
    y32 = groupnorm_affine(x, G, gamma, beta, eps, dtype=F32)
    got = y32 if got is None else got
    ref = groupnorm_affine(x, G, gamma, beta, eps)
    if family == "I":
        return [check_exact(g_, r.to(F32), f"{tag} {nm}") for g_, r, nm in zip(got, ref, ("mul", "add"))], (0.0, 0.0)
    tol = groupnorm_tol(x, G, gamma, beta, eps)
    return [check_bound(g_, r, t, y, f"{tag} {nm}")[0] for g_, r, t, y, nm in zip(got, ref, tol, y32, ("mul", "add"))], tuple(rel_l2(y, r) for y, r in zip(y32, ref))


def accept_softmax(s, scale, valid, tag, got=None, every=False):
    """every: all fp32 restatements against the bound (the host module); returns (worst |d| / bound of got, or of restatement 0; Y)."""
    y32 = softmax_restatements(s, scale, valid, vec=4 if valid is None else 1)
    assert torch.equal(y32[0], softmax_rows(s, scale, valid, dtype=F32))
    ref, tol = softmax_rows(s, scale, valid), softmax_tol(s, scale, valid)
    for y in y32[1:] if every else ():
        check_bound(y, ref, tol, y32, tag)
    return check_bound(y32[0] if got is None else got, ref, tol, y32, tag)[0], max(rel_l2(y, ref) for y in y32)


def accept_blend(family, axis, extent, got=None):
    a, b = blend_inputs(family, axis, extent)
    y32 = blend_axis(a, b, axis, extent, dtype=F32)
    got = y32 if got is None else got
    tag = f"blend_axis {family} axis={axis} extent={extent}"
    if family == "I":
        return check_exact(got, blend_axis(a, b, axis, extent).to(F32), tag), 0.0
    ref = blend_axis(a, b, axis, extent)
    return check_bound(got, ref, blend_tol(a, b, axis, extent), y32, tag)[0], rel_l2(y32, ref)


def border_buffers(lead, pad, Hp, Wp, C, seed=0, bits=32):
    """(before, want) as int32 / int16: random bit patterns everywhere (the border and the lead frames hold garbage), and the contract's result."""
    buf = torch.randint(-2 ** (bits - 1), 2 ** (bits - 1) - 1, (lead + 2, Hp, Wp, C), generator=_gen(lead, pad, Hp, Wp, C, seed, bits, 17), dtype=torch.int64)
    buf = buf.to(torch.int32 if bits == 32 else torch.int16)
    return buf, replicate_border(buf, lead, pad)
