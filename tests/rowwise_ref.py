"""float64 references of the row-wise DiT operators of lightx2v_amd/csrc/norm.hip, written from the formulas in include/x2v.h.  Plain PyTorch on
the CPU; nothing here imports the library, the oracle or lightx2v_amd/wan.py.  Shared by tests/test_rowwise_ref_host.py (the references checked
without a GPU) and tests/test_gpu_rowwise_fp64.py (the kernels checked against them), together with the seeded input sets both use.

Two kinds of reference, by the kernel's documented rounding model:
  * EXACT (forms with one final rounding: RMSNorm X2V_ROUND_FP32, LayerNorm without modulate, RoPE without norm, the activations, the
    sinusoid): the formula in float64, NOT rounded to bf16.
  * CHAIN (forms whose contract is a sequence of bf16 roundings: RMSNorm X2V_ROUND_REF, LayerNorm + modulate, norm + RoPE, headnorm + RoPE,
    gate-residual): float64 arithmetic with an explicit round-to-nearest-even to bf16 (`rne_bf16`) at every point x2v.h / norm.hip name.

Every function takes `dtype` (float64 by default).  With dtype=torch.float32 the SAME formula runs in fp32 torch — the host module uses that as
a stand-in for any correct fp32 kernel when it checks that the acceptance caps hold for the references alone.

In the X2V_ROUND_REF chains `mean`, `mean + eps` and `rstd` are roundings that scale a whole row.  A `Ref` carries, per row, the relative
distance of each of the three to the nearest bf16 rounding boundary (`gaps` [3, rows]); `alt=i` rebuilds the reference with the OTHER
neighbour of intermediate i on the rows whose gap i is below FLAG_GAP — fp32 and fp64 may legitimately round such a row differently."""
import math

import torch

F64 = torch.float64
BF16 = torch.bfloat16
ULP = 2.0 ** -7  # the project's one-ulp (tests/util.py::assert_bf16_close: the widest relative bf16 spacing)
FLAG_GAP = 2.0 ** -20  # a row-scaling intermediate closer than this (relative) to a bf16 rounding boundary flags its row
FLIP_CAP = 2e-3  # tests/test_gpu_ops.py's bad_frac for these kernels
FLAGGED_ROWS_CAP = 1e-2
ROUND_FP32, ROUND_REF = 0, 1  # x2v.h X2V_ROUND_*
ACT_GELU_TANH, ACT_SILU, ACT_GELU_ERF = 1, 3, 4  # x2v.h X2V_EPI_GELU_TANH, X2V_EPI_SILU, X2V_ACT_GELU_ERF


def rne_bf16(x):
    """Round to the nearest bf16 value, ties to even, staying in x's dtype.  float64: on the bit pattern (52 - 7 = 45 dropped mantissa bits), so
    there is no double rounding through fp32; magnitudes below 2^-126 (bf16 subnormals, spacing 2^-133) by scaling.  float32: torch's own cast."""
    if x.dtype != F64:
        return x.to(BF16).to(x.dtype)
    x = x.contiguous()
    bits = x.view(torch.int64)
    r = (((bits + ((1 << 44) - 1) + ((bits >> 45) & 1)) >> 45) << 45).view(F64)
    return torch.where(x.abs() < 2.0 ** -126, torch.round(x * 2.0 ** 133) * 2.0 ** -133, r)


def boundary_gap(v):
    """For positive pre-rounding values v: (relative distance of v to the nearest bf16 rounding boundary, the bf16 neighbour on the far side of
    that boundary).  v == 0 (an all-zero row) has gap 1: every precision computes it exactly."""
    v = v.to(F64)
    r = rne_bf16(v)
    _, e = torch.frexp(r)  # r = m * 2^e, m in [0.5, 1)
    up = torch.ldexp(torch.ones_like(r), e - 8)  # spacing above r
    down = torch.where(r == torch.ldexp(torch.ones_like(r), e - 1), up / 2, up)  # below a power of two the spacing halves
    d_hi, d_lo = (r + up / 2) - v, v - (r - down / 2)
    gap = torch.minimum(d_hi, d_lo) / v
    other = torch.where(d_hi < d_lo, r + up, r - down)
    zero = v == 0
    return torch.where(zero, torch.ones_like(gap), gap), torch.where(zero, r, other)


class Ref:
    """y: the reference values (unrounded for an exact reference, bf16-valued for a chain); atol: the absolute term of the hard bound (0 or a
    tensor broadcastable to y, derived from the operands of a cancelling sum); gaps: None or [3, rows] (see the module docstring), rows being
    y.reshape(rows, -1)."""

    def __init__(self, y, atol=0.0, gaps=None):
        self.y, self.atol, self.gaps = y, atol, gaps


def _chain_rstd(v, eps, alt):
    """rstd of the X2V_ROUND_REF chain from v = sum(bf16(x^2)) / n: mean = bf16(v), t = bf16(mean + eps), rstd = bf16(1 / sqrt(t))."""
    gaps, cur = [], v
    for i, step in enumerate((lambda a: a, lambda a: a + eps, lambda a: 1.0 / torch.sqrt(a))):
        pre = step(cur)
        gap, other = boundary_gap(pre)
        cur = rne_bf16(pre)
        if alt == i:
            cur = torch.where(gap < FLAG_GAP, other.to(cur.dtype), cur)
        gaps.append(gap)
    return cur, torch.stack([g.reshape(-1) for g in gaps])


def _f32eps(eps):
    return float(torch.tensor(eps, dtype=torch.float32))  # the C ABI takes eps as a float


def _rms_norm(x, w, eps, mode, alt, dtype):
    """x [..., n] -> (x * rsqrt(mean(x^2) + eps) * w rounded per `mode` to what feeds a following op, unrounded in FP32 mode, gaps)."""
    x, eps = x.to(dtype), _f32eps(eps)
    n = x.shape[-1]
    if mode == ROUND_REF:  # torch chain: x.pow(2) is a bf16 tensor, .mean() accumulates wide and rounds, + eps rounds, rsqrt rounds, x * rstd rounds, * w rounds
        rs, gaps = _chain_rstd(rne_bf16(x * x).sum(-1, keepdim=True) / n, eps, alt)
        return rne_bf16(rne_bf16(x * rs) * w.to(dtype)), gaps
    rs = 1.0 / torch.sqrt((x * x).sum(-1, keepdim=True) / n + eps)
    return x * rs * w.to(dtype), None


def rmsnorm(x, w, eps=1e-6, mode=ROUND_FP32, alt=-1, dtype=F64):
    """x2v_rmsnorm_bf16: y = x * rsqrt(mean(x^2) + eps) * w.  ROUND_FP32: exact reference (one final rounding); ROUND_REF: chain."""
    y, gaps = _rms_norm(x, w, eps, mode, alt, dtype)
    return Ref(y, 0.0, gaps)


def layernorm(x, w=None, b=None, scale=None, shift=None, eps=1e-6, dtype=F64):
    """x2v_layernorm_bf16: LN(x; w, b, eps) [* (1 + scale) + shift].  Without modulate an exact reference; with it the chain
    bf16 after LN, after 1 + scale, after the multiply, after the add.  atol: LN's output is a difference of larger terms — one ulp of the
    row's largest |x - mean| * rstd * |w| term; the modulate add — one ulp of |m| + |shift| (plus LN's term carried through 1 + scale)."""
    x, eps = x.to(dtype), _f32eps(eps)
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    rstd = 1.0 / torch.sqrt((d * d).mean(-1, keepdim=True) + eps)
    y = d * rstd
    term = y.abs()
    if w is not None:
        y, term = y * w.to(dtype), term * w.to(dtype).abs()
    if b is not None:
        y = y + b.to(dtype)
    atol = ULP * term.amax(-1, keepdim=True)
    if scale is None:
        return Ref(y, atol)
    s1 = rne_bf16(1.0 + scale.to(dtype).reshape(-1))
    m = rne_bf16(rne_bf16(y) * s1)
    sh = shift.to(dtype).reshape(-1)
    return Ref(rne_bf16(m + sh), ULP * (m.abs() + sh.abs()) + atol * s1.abs())


def quant_fp8_scale(y):
    """Per-token scale of x2v_quant_fp8_rowwise / x2v_layernorm_quant_fp8 on a bf16-valued y: max(amax|y| / 448, 1 / (448 * 512))."""
    return torch.clamp(y.abs().amax(-1, keepdim=True) / 448.0, min=1.0 / (448.0 * 512.0))


def rope_factors(cs, S, s0, grid, dtype=F64):
    """(cos, sin) [S, 64] of tokens s0 .. s0+S-1 from the table cs [1024, 64, 2]: complex column ci takes its angle from table row
    t-position for ci in [0,22), h-position for [22,43), w-position for [43,64); token g = s0 + s sits at (g / (gh*gw), (g / gw) % gh, g % gw);
    g >= gf*gh*gw is rotated by 1."""
    gf, gh, gw = grid
    g = s0 + torch.arange(S, dtype=torch.int64)
    inside = g < gf * gh * gw
    gc = torch.where(inside, g, torch.zeros_like(g))
    pos = torch.empty(S, 64, dtype=torch.int64)
    pos[:, :22] = (gc // (gh * gw)).unsqueeze(1)
    pos[:, 22:43] = ((gc // gw) % gh).unsqueeze(1)
    pos[:, 43:] = (gc % gw).unsqueeze(1)
    f = cs.to(dtype)[pos, torch.arange(64).unsqueeze(0)]  # [S, 64, 2]
    co = torch.where(inside.unsqueeze(1), f[..., 0], torch.ones((), dtype=dtype))
    si = torch.where(inside.unsqueeze(1), f[..., 1], torch.zeros((), dtype=dtype))
    return co, si


def rmsnorm_rope(x, w, cs, s0, grid, eps=1e-6, mode=ROUND_FP32, out_scale=1.0, alt=-1, dtype=F64):
    """One operand (q or k) of x2v_rmsnorm_rope_scaled_bf16: x [S, H*128], w [H*128] or None, out_scale = q_out_scale for q and 1 for k.
    Without w an exact reference (one rounding after rotation and scale).  With w a chain: the norm over the whole row rounded to bf16 (one
    rounding of x*rs*w in ROUND_FP32, the torch chain in ROUND_REF) feeds the rotation (a + ib)(cos + i sin), times out_scale, rounded once.
    atol: a rotated component is a sum of two products — one ulp of (|a| + |b|) * out_scale of the normalised pair."""
    S, D = x.shape
    gaps = None
    if w is None:
        xn = x.to(dtype)
    else:
        xn, gaps = _rms_norm(x, w, eps, mode, alt, dtype)
        xn = rne_bf16(xn)
    co, si = rope_factors(cs, S, s0, grid, dtype)
    p = xn.reshape(S, D // 128, 64, 2)
    a, b = p[..., 0], p[..., 1]
    co, si = co.unsqueeze(1), si.unsqueeze(1)
    y = torch.stack([a * co - b * si, a * si + b * co], dim=-1).reshape(S, D) * out_scale
    atol = (ULP * out_scale * (a.abs() + b.abs())).unsqueeze(-1).expand(S, D // 128, 64, 2).reshape(S, D)
    return Ref(y if w is None else rne_bf16(y), atol, gaps)


def headnorm_rope(x, w, cos, sin, H, l_rope, eps=1e-6, mode=ROUND_FP32, out_scale=1.0, alt=-1, dtype=F64):
    """One operand of x2v_headnorm_rope_bf16: x [L, H*128], w [128] or None (no norm), bf16 cos/sin [>= l_rope, 128]; out_scale = q_out_scale
    for q (ignored with ROUND_REF) and 1 for k.  Per-(token, head) RMSNorm over 128, then for tokens < l_rope the real-valued rotation
    x*cos + rotate_half(x)*sin with rotate_half(x)[2i] = -x[2i+1], [2i+1] = x[2i] on bf16 tensors: both products and the sum round.
    ROUND_REF: torch chain in the norm.  ROUND_FP32: fp32 norm; an un-rotated row has ONE rounding, of x*rs*w*out_scale; a rotated row
    rounds x*rs*w, the two products, and (sum * out_scale).  gaps rows are (token, head).  atol (rotated rows): one ulp of
    (|re| + |im|) * out_scale of the normalised pair."""
    L = x.shape[0]
    if mode == ROUND_REF:
        out_scale = 1.0
    xh = x.to(dtype).reshape(L, H, 128)
    gaps = None
    if w is None:
        xn = xh
    else:
        xn, gaps = _rms_norm(xh, w, eps, mode, alt, dtype)
    y = rne_bf16(xn * out_scale)  # tokens >= l_rope: only normalised (the scale inside that one rounding)
    atol = torch.zeros_like(y)
    if l_rope > 0:
        v = rne_bf16(xn[:l_rope]).reshape(l_rope, H, 64, 2)
        re, im = v[..., 0], v[..., 1]
        c = cos.to(dtype)[:l_rope].reshape(l_rope, 1, 64, 2)
        s = sin.to(dtype)[:l_rope].reshape(l_rope, 1, 64, 2)
        o0 = rne_bf16(re * c[..., 0]) + rne_bf16(-im * s[..., 0])
        o1 = rne_bf16(im * c[..., 1]) + rne_bf16(re * s[..., 1])
        y[:l_rope] = rne_bf16(torch.stack([o0, o1], dim=-1) * out_scale).reshape(l_rope, H, 128)
        atol[:l_rope] = (ULP * out_scale * (re.abs() + im.abs())).unsqueeze(-1).expand(l_rope, H, 64, 2).reshape(l_rope, H, 128)
    return Ref(y.reshape(L, H * 128), atol.reshape(L, H * 128), gaps)


def gate_residual(x, y, gate=None, dtype=F64):
    """x2v_gate_residual_bf16: bf16(x + bf16(y * gate)), gate None = plain add.  Products and sums of bf16 values are exact in float64."""
    x, y = x.to(dtype), y.to(dtype)
    return Ref(rne_bf16(x + (y if gate is None else rne_bf16(y * gate.to(dtype).reshape(-1)))))


def activation(x, act, dtype=F64):
    """x2v_activation_bf16, exact references.  gelu-tanh 0.5 x (1 + tanh(u)), u = sqrt(2/pi)(x + 0.044715 x^3), is evaluated as x / (1 + e^-2u)
    and the exact GELU 0.5 x (1 + erf(x / sqrt 2)) as 0.5 x erfc(-x / sqrt 2): the same functions without the cancellation of 1 + tanh /
    1 + erf in the negative tail, so the reference is accurate to its last bits there.  atol 1e-6 (tests/test_gpu_ops.py:76-77)."""
    x = x.to(dtype)
    if act == ACT_GELU_TANH:
        y = x * torch.sigmoid(2.0 * math.sqrt(2.0 / math.pi) * (x + 0.044715 * x * x * x))
    elif act == ACT_GELU_ERF:
        y = 0.5 * x * torch.special.erfc(-x / math.sqrt(2.0))
    elif act == ACT_SILU:
        y = x * torch.sigmoid(x)
    else:
        raise ValueError(act)
    return Ref(y, 1e-6)


def sinusoid(t, dim, dtype=F64):
    """x2v_sinusoid_embed_bf16: [cos(t f_j) | sin(t f_j)], f_j = 10000^(-j / (dim/2)), j < dim/2.  atol 1e-6 (tests/test_gpu_ops.py:77)."""
    half = dim // 2
    f = torch.pow(torch.tensor(10000.0, dtype=dtype), -torch.arange(half, dtype=dtype) / half)
    a = t.to(dtype).reshape(-1, 1) * f
    return Ref(torch.cat([torch.cos(a), torch.sin(a)], dim=1), 1e-6)


# ------------------------------------------------------------------------------------------------------------------- acceptance
def bf16_bits(t):
    return t.to(BF16).contiguous().view(torch.int16)


def resolve_flagged(got, make):
    """make(alt) -> Ref.  Returns (y, atol, rows, flagged rows): the base reference, with every row flagged at intermediate i (gap < FLAG_GAP)
    replaced by the alt=i reference where that one matches `got` in more elements — a flagged row is accepted against either neighbour."""
    ref = make(-1)
    y, atol = ref.y, ref.atol
    if ref.gaps is None:
        return y, atol, 0, 0
    rows = ref.gaps.shape[1]
    g = got.to(F64).reshape(rows, -1)
    y2 = y.reshape(rows, -1).clone()
    a2 = atol.reshape(rows, -1).clone() if torch.is_tensor(atol) and atol.numel() == y.numel() else None
    flagged = ref.gaps < FLAG_GAP
    for i in range(3):
        if flagged[i].any():
            alt = make(i)
            ya = alt.y.reshape(rows, -1)
            better = flagged[i] & ((ya != g).sum(1) < (y2 != g).sum(1))
            y2[better] = ya[better]
            if a2 is not None:
                a2[better] = alt.atol.reshape(rows, -1)[better]
    return y2.reshape(y.shape), (a2.reshape(y.shape) if a2 is not None else atol), rows, int(flagged.any(0).sum())


class Case:
    """Accumulates one operator case: the hard bound is asserted per call, the flip share and the flagged-row share over the whole case."""

    def __init__(self, name):
        self.name, self.n, self.flips, self.rows, self.flagged, self.max_ulps = name, 0, 0, 0, 0, 0.0

    def check(self, got, make, what=""):
        """got: a bf16 (or bf16-valued) CPU tensor; make: a Ref, or alt -> Ref for a chain with flagged rows.
        Hard bound, every element, no exempt fraction: |got - ref| <= 2^-7 |ref| + atol.  2^-7 is the project's one-ulp (tests/util.py); atol is
        zero except where the output is a difference of larger terms and then comes from the operands (see each reference's docstring):
        LayerNorm one ulp of the row's largest |x - mean| rstd |w| term; a rotated pair one ulp of |a| + |b| of the normalised pair;
        the modulate add one ulp of |m| + |shift|; activations and sinusoid 1e-6."""
        y, atol, rows, nflag = resolve_flagged(got, make if callable(make) else (lambda alt: make))
        g = got.to(F64)
        assert g.shape == y.shape, f"{self.name} {what}: shape {tuple(g.shape)} vs {tuple(y.shape)}"
        assert torch.isfinite(g).all(), f"{self.name} {what}: non-finite output"
        err = (g - y).abs()
        bound = ULP * y.abs() + atol
        over = err > bound
        if over.any():
            i = int((err - bound).reshape(-1).argmax())
            raise AssertionError(f"{self.name} {what}: {int(over.sum())} of {y.numel()} elements outside 2^-7|ref| + atol; worst at flat index {i}: "
                                 f"got {g.reshape(-1)[i].item():.9g} ref {y.reshape(-1)[i].item():.9g} bound {bound.reshape(-1)[i].item() if torch.is_tensor(bound) else bound:.3g}")
        flips = int((bf16_bits(g) != bf16_bits(rne_bf16(y))).sum())
        denom = torch.maximum(ULP * y.abs(), torch.as_tensor(atol, dtype=F64).expand_as(y) if torch.is_tensor(atol) else torch.full_like(y, atol))
        ulps = torch.where(denom > 0, err / denom.clamp_min(1e-300), torch.zeros_like(err))
        self.n += y.numel()
        self.flips += flips
        self.rows += rows
        self.flagged += nflag
        self.max_ulps = max(self.max_ulps, float(ulps.max()) if ulps.numel() else 0.0)
        return flips

    @property
    def flip_share(self):
        return self.flips / max(self.n, 1)

    @property
    def flagged_share(self):
        return self.flagged / max(self.rows, 1)

    def finish(self, cap=FLIP_CAP, record=True):
        if record:
            from tests.util import record as rec

            rec("rowwise_fp64 " + self.name, flip_share=self.flip_share, max_err_ulps=self.max_ulps, elements=self.n, flagged_rows=self.flagged)
        assert self.flip_share <= cap, f"{self.name}: {self.flips} of {self.n} elements ({self.flip_share:.2e}) differ from bf16(ref), cap {cap:.0e}"
        assert self.flagged_share <= FLAGGED_ROWS_CAP, f"{self.name}: {self.flagged} of {self.rows} rows near a rounding boundary"


# ------------------------------------------------------------------------------------------------------------------- seeded input sets
NORM_D = (8, 128, 504, 512, 520, 1536, 2048, 2056, 4096, 5120, 6144, 8192, 8200, 13824, 16384)
RMS_M = (1, 3, 5, 9)  # straddle the four-rows-per-block edge of the short-row kernel
RMS_SETS = ("n01", "small", "large", "zero_row")
LN_SETS = ("n01", "offset40", "const_row", "one_hot_row")
LN_COMBOS = ("none", "w", "b", "wb", "mod", "all")
ROPE_H = (1, 2, 12, 16, 24, 40, 64, 72, 128)
ROPE_GRIDS = (((2, 3, 5), 0, 33), ((3, 4, 6), 7, 24), ((1, 1, 1000), 990, 40), ((1024, 1, 1), 1020, 8))  # (grid, s0, S)
HEAD_SHAPES = ((1, 37), (3, 11), (24, 5))  # (H, L): L*H is no multiple of 16 and fills at least two 16-row blocks
# q_out_scale of the scaled cases.  The references multiply by the real number 0.1275; the float the C ABI carries is 1.9e-8 below it, which
# is part of what an fp32 evaluation may differ by.  (0.1275 = 51/400 puts x * 0.1275 exactly on a bf16 tie for ~1 % of bf16 x: against the
# float's own value every correct fp32 product-then-round would land on the other side of those ties.)
Q_SCALE = 0.1275
SIN_T = (0, 1, 3, 727, 999, 1000)
SIN_DIMS = (2, 64, 256, 5120)
ACT_LENGTHS = (1, 7, 8, 9, 2055)


def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 17) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def randn_bf16(gen, *shape, std=1.0, mean=0.0):
    return (torch.randn(*shape, generator=gen) * std + mean).to(BF16)


RMS_RESEED = {8: 1}  # D = 8 has 72 chain rows in all: the first draw put one of them (1.4 % > 1 %) next to a rounding boundary


def rms_inputs(D, M, kind):
    g = _gen(1, D, M, RMS_SETS.index(kind), RMS_RESEED.get(D, 0))
    w = randn_bf16(g, D, std=0.1, mean=1.0)
    x = randn_bf16(g, M, D, std={"small": 1e-3, "large": 2e3}.get(kind, 1.0))  # small: eps takes part; large: a large sum of squares
    if kind == "zero_row":
        x[M // 2] = 0
    return x, w


def ln_rows(D):
    return (5, 9) if D <= 512 else (5,)


def ln_inputs(D, M, kind):
    """x and the per-channel operands (w, b, scale, shift)."""
    g = _gen(2, D, M, LN_SETS.index(kind))
    ops = (randn_bf16(g, D, std=0.1, mean=1.0), randn_bf16(g, D, std=0.1), randn_bf16(g, D, std=0.3), randn_bf16(g, D, std=0.3))
    if kind == "offset40":
        # mean 40, std 0.5: a one-pass variance E[x^2] - mean^2 loses everything here.  The right half mirrors the left about 40, so the row
        # mean is 40 in every precision: bf16 spaces these values 0.25 apart, a row holds about ten distinct x - mean, and the 2^-24 relative
        # error of an fp32 mean (2e-6 absolute against |x - mean| ~ 0.5) then flips whole groups of equal elements at once — the host module
        # measured up to 4.6e-3 of a case for a plain N(40, 0.5) draw in correct fp32, above the cap for no fault of a kernel
        x = randn_bf16(g, M, D, std=0.5, mean=40.0)
        x[:, D // 2 :] = (80.0 - x[:, : D // 2].float()).to(BF16)
    else:
        x = randn_bf16(g, M, D)
    if kind == "const_row":
        x[M // 2] = 3.0  # variance 0
    if kind == "one_hot_row":
        x[M // 2] = 0
        x[M // 2, D // 3] = 5.0
    return x, ops


def ln_operands(ops, combo):
    w, b, sc, sh = ops
    return {"none": {}, "w": dict(w=w), "b": dict(b=b), "wb": dict(w=w, b=b), "mod": dict(scale=sc, shift=sh), "all": dict(w=w, b=b, scale=sc, shift=sh)}[combo]


def rope_table(seed=5):
    """A [1024, 64, 2] fp32 (cos, sin) table of RANDOM angles: a wrong column or axis index cannot land on a similar value."""
    ang = torch.rand(1024, 64, generator=_gen(3, seed)) * (2 * math.pi)
    return torch.stack([ang.cos(), ang.sin()], dim=-1).float().contiguous()


def rope_inputs(H, gi):
    """q != k, wq != wk."""
    g = _gen(4, H, gi)
    S, D = ROPE_GRIDS[gi][2], H * 128
    return randn_bf16(g, S, D, std=1.5), randn_bf16(g, S, D, std=0.7), randn_bf16(g, D, std=0.1, mean=1.0), randn_bf16(g, D, std=0.2, mean=0.8)


def head_inputs(H, L):
    g = _gen(5, H, L)
    D = H * 128
    ang = torch.rand(L, 128, generator=g) * (2 * math.pi)
    return (randn_bf16(g, L, D, std=1.5), randn_bf16(g, L, D, std=0.7), randn_bf16(g, 128, std=0.1, mean=1.0), randn_bf16(g, 128, std=0.2, mean=0.8),
            ang.cos().to(BF16), ang.sin().to(BF16))


def residual_inputs(M, D, seed=0):
    g = _gen(6, M, D, seed)
    return randn_bf16(g, M, D), randn_bf16(g, M, D), randn_bf16(g, D, std=0.5)


def all_finite_bf16():
    """Every finite bf16 bit pattern (65 280 values: +-0, subnormals, normals)."""
    bits = torch.arange(65536, dtype=torch.int32)
    bits = bits[(bits & 0x7F80) != 0x7F80]
    return bits.to(torch.int16).view(BF16)


# ------------------------------------------------------------------------------------------------------------------- case iterators
# One definition of "every input set" for the host module (fp32 twin against the reference) and the GPU module (kernel against the reference).
def rms_items(D):
    for M in RMS_M:
        for kind in RMS_SETS:
            x, w = rms_inputs(D, M, kind)
            for mode in (ROUND_FP32, ROUND_REF):
                yield f"M={M} {kind} mode={mode}", x, w, mode, kind


def ln_items(D):
    for M in ln_rows(D):
        for kind in LN_SETS:
            x, ops = ln_inputs(D, M, kind)
            for combo in LN_COMBOS:
                yield f"M={M} {kind} {combo}", x, ln_operands(ops, combo), kind, combo


def rope_items(H):
    for gi in range(len(ROPE_GRIDS)):
        q, k, wq, wk = rope_inputs(H, gi)
        for mode in (ROUND_FP32, ROUND_REF):
            for with_w in (True, False):
                yield f"grid#{gi} mode={mode} norm={with_w}", gi, q, k, (wq if with_w else None), (wk if with_w else None), mode


def head_items(H, L):
    q, k, wq, wk, cos, sin = head_inputs(H, L)
    for l_rope in (0, 1, L - 1, L):
        for mode in (ROUND_FP32, ROUND_REF):
            for with_w in (True, False):
                for scale in (1.0, Q_SCALE):
                    yield f"l_rope={l_rope} mode={mode} norm={with_w} scale={scale}", q, k, (wq if with_w else None), (wk if with_w else None), cos, sin, l_rope, mode, scale
