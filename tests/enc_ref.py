"""float64 references, seeded inputs, fp32 emulations, acceptance rules and the case lists for the kernels of the four encoder towers (CLIP ViT-H, umT5,
Llama, CLIP-L): gemm_rows_kernel (gemm_rows.h: x2v_gemm_f16, x2v_gemm_rows_bf16), the three attention kernels built from enc_attn.h (x2v_attn_f16_d80,
x2v_attn_bf16_d64_relbias, x2v_attn_f16_causal) and the norms of clip.hip / txt_enc.hip (x2v_rmsnorm_f16, x2v_layernorm_f16, x2v_clip_embed_f16).  Plain
PyTorch on the CPU; nothing here imports the library or the oracle.  Shared by tests/test_enc_ref_host.py (the yardstick checked without a GPU) and
tests/test_gpu_enc_fp64.py (the kernels checked against it): both walk the case lists at the end of this file, so they cannot drift.

The references restate the contracts of include/x2v.h and the header comments of the five source files, not a kernel.  T = the element type, fp16
(u = 2^-10, p = h = 2^-11) or bf16 (u = 2^-7, p = h = 2^-8): u the widest relative spacing, p = h the largest relative error of one rounding.

ATTENTION (head-major here: q [H, n, d], k / v [Hkv, n, d] of ONE sequence; a packed launch is a list of sequences)
  s_ij = scale * q_i . k_j (+ bias[h][j - i + 511], T5), keys j <= i only (causal), P = exp(s - max), o = sum_j P_j v_j / sum_j P_j.  Rounding points: the
  rotary entry rotates q and k from the fp16 inputs and the fp32 tables and rounds them to fp16 ONCE; everything after that is float64.  scale is the
  fp32 number the launchers compute (80^-1/2, 1, d^-1/2).  ref64 returns (o, A, F), A = sum_j w_j |v_jd|.
  Acceptance (AttnCase.check), no share of elements left out:
    * every element |got - o| <= u |o| + 1.05 * p * A + F.  o' - o = sum_j w_j delta_j v_j with |delta_j| <= p (P's rounding to T for the PV product)
      plus the one rounding of O; 1.05 and (u, p) are the constants of the three encoder attention tests.  F is the fp16 subnormal term, derived the way
      tests/test_gpu_attn_mx.py derives its own: a probability below 2^-14 (fp16's smallest normal) is rounded on a grid of spacing 2^-24, so it moves
      by at most 2^-25 absolutely (one below 2^-25 is flushed to 0, the same bound); one that was normal relative to an earlier running maximum of the
      online softmax moved by at most 2^-11 * P, which ends below 2^-25 once P ends below 2^-14.  F_d = 2^-25 / l * sum_{j: P_j < 2^-14} |v_jd|, l = sum P.
      F = 0 for bf16 (its exponent range is fp32's).  The rotary entry adds R (rope_slack): the fp16 rounding of a rotated q or k element whose exact
      value lies within the fp32 evaluation's error of a rounding boundary may fall to either side in a correct kernel; R bounds what those
      elements (and only those) can move the output by.  It is zero for rows that meet no such element.
    * aggregate relL2(got - o) <= 1.5 * Y, Y the larger relative L2 error of this module's two fp32 emulations of a correct kernel on the same inputs:
      one pass with the global row maximum (the d80 and d64 kernels), and 64-key tiles with a rescale on every tile (the causal kernel).  In both P is
      rounded to T for the PV product only, the row sum takes it unrounded, O is rounded once.  1.5 is the project's triangle factor.
    * families H, U and S (below) bit for bit.
  Input families (AttnInputs), q and k drawn at amplitude (1 / scale)^(1/2) d^-1/4 each, so that T5 (scale 1) sees the score spread of the others:
    R  randn, one key four times as long placed first (key 0), middle, last (key n - 1: the last key of the last 16-key tile) or nowhere;
    N  flat: q / 16 (and bias / 16), every score within a fraction of a unit, every key weighs about 1 / n;
    H  one key j(i) leads every other by >= 40 base-2 units (asserted): the output is that key's V row bit for bit (every other P is far below 2^-25
       relative to V's own grid);
    U  k = 0, zero bias, v = 1: the output is 1 bit for bit;
    B  (T5) q = 0: the scores are the bias alone;
    S  sharp: q = 0, zero bias, V one-hot (key j lights column j mod d): row i is histogram / len, every P is 1, the PV sum and l are small integers:
       T(count / len) bit for bit.  (A kernel forms count * fl(1 / len): two fp32 roundings, 2^-23 relative; a quotient of integers count <= 512 over
       len <= 512 is either a T number or further than 1 / (count * 2^20) from every rounding boundary of T, so the T result is the same.)  A leaked zero
       key (len + 1 in the denominator) or a dropped key shows in every non-zero element.
    The T5 bias table is N(0, 1), distinct per head and per delta, not symmetric.

GEMM  t = x . W^T + bias; NONE T(t) | GELU_ERF T(gelu(t)) | QUICK_GELU T(t sigmoid(1.702 t)) | RESIDUAL T(resid + T(t)) | GEGLU (bf16)
  T(T(a) gelu_tanh(T(g))) | SWIGLU (fp16) T(silu(T(a)) T(g)), (a, g) = columns 2n, 2n + 1 of t (rows 2n, 2n + 1 of W), no bias.  gemm_ref's two families:
    I  small integers, every operand sum of one sign per output column (x = |x| s_k, W = |W| s_k sigma_n), so |t| ~ 8 K passes 256 (bf16, which has no
       bias) from K = 32 on; the fp16 bias range is doubled until acc + bias passes 2048 often enough.  Everything is exact in fp32 (|t| < 2^24 asserted):
       NONE and RESIDUAL equal the float64 chain BIT FOR BIT; >= 5 % of t inexact before its rounding is asserted.
    R  randn x, W / sqrt(K): a bound on EVERY element against the unrounded float64 result.  S = |x| . |W|^T + |bias|, E = (K + 1) 2^-23 S,
       e0 = h |t| + (1 + h) E (gemm_ref's) + SUB, SUB = 2^-25 for fp16 and 0 for bf16: a result below 2^-14 is rounded on fp16's subnormal grid of
       spacing 2^-24; every final rounding below adds SUB likewise:
         NONE      e0
         act       tol = L e0 + 2^-16 |f|, then tol += h (|f| + tol)            (L from gemm_ref.lipschitz, asserted by the host test)
         RESIDUAL  tol = e0 + h (|resid + t| + e0)
         gated     y = T(T(a) f(T(g))) (GEGLU; SWIGLU with the roles exchanged: y = T(f(T(a)) T(g))).  T(a) = a + da, |da| <= e0(a); T(g) = g + dg,
                   |dg| <= e0(g); f(T(g)) evaluated in fp32 = G + dG, G = f(g), |dG| <= L e0(g) + 2^-16 (|G| + L e0(g)).  The product
                   (a + da)(G + dG) - a G = a dG + G da + da dG: ep = |a| dG + |G| da + da dG; the fp32 product adds 2^-23 (|a G| + ep); the final
                   rounding h (|a G| + ep'): tol = ep' + h (|a G| + ep'), ep' = ep + 2^-23 (|a G| + ep).
  None of these constants is fitted to a kernel's output.

NORMS  float64 with one rounding (clip_embed: the documented fp16 add tok + pos first, a chain).  rowwise_ref's rule for its one-rounding row kernels:
  every element |got - y| <= u |y| + atol, atol = 0 (RMSNorm) or u * the row's largest |x - mean| rstd |w| term (LayerNorm: a difference of larger
  terms), and at most 2e-3 of a case's elements differ from T(y).  fp16 adds SUB = 2^-25 to atol: an output below 2^-14 sits on the subnormal grid of
  spacing 2^-24.

Worst d / tol of the CORRECT emulations over the case lists below, as tests/test_enc_ref_host.py::test_emulations_pass_every_listed_case prints them
(-s).  Two emulations failed the rules as first written, and each time the derivation lacked a term, now in it: the rotary term R (a rotated element
beside a rounding boundary; c128r R-first n = 128 stood at 1.284 without it) and the fp16 subnormal term of a GEMM result (SWIGLU 145x6148x32 at 1.812:
an output of 2^-23).  No constant was changed.
  attention d80 0.455 | t5 0.517 | c64 0.623 | c128 0.672 | c128r 0.645        GEMM f16 0.982 | bf16 0.994 (NONE: the rounding itself is up to h / (1 + h))
  rmsnorm 0.722 | layernorm 0.235 | clip_embed 0.256"""
import math

import torch

from tests import attn_ref, gemm_ref

F64, F32, F16, BF16 = torch.float64, torch.float32, torch.float16, torch.bfloat16
P_SLACK, TRIANGLE = 1.05, attn_ref.TRIANGLE
UNIT, ACT_EVAL, MIN_INEXACT = gemm_ref.UNIT, gemm_ref.ACT_EVAL, gemm_ref.MIN_INEXACT
SUB16 = 2.0 ** -25  # half the spacing of fp16's subnormal grid
FLIP_CAP = 2e-3  # rowwise_ref.FLIP_CAP


class Fmt:
    def __init__(self, name, dtype, keep, emin):
        self.name, self.dtype, self.keep, self.emin = name, dtype, keep, emin
        self.u, self.h = 2.0 ** -keep, 2.0 ** -(keep + 1)
        self.p = self.h


FMT = {"f16": Fmt("f16", F16, 10, -14), "bf16": Fmt("bf16", BF16, 7, -126)}


def rnd(t, fmt, mode="rne"):
    """float64 -> the nearest number of the format, as float64: ONE rounding (torch's float64 -> 16-bit casts go through fp32).  Below 2^emin the grid is
    the subnormal one.  mode 'rne' = ties to even (the contract); 'half_up' = the wrong rounding of a host mutation.  The powers of two are put together
    from their bits, so every step is exact."""
    fmt = FMT[fmt] if isinstance(fmt, str) else fmt
    t = t.contiguous()
    e = ((t.view(torch.int64) >> 52) & 0x7FF).clamp_min(1023 + fmt.emin) - fmt.keep
    q, qinv = (e << 52).view(F64), ((2046 - e) << 52).view(F64)
    r = t * qinv
    r = torch.round(r) if mode == "rne" else torch.floor(r + 0.5)
    return r * q


def to_fmt(t64, fmt):
    """rnd, as a tensor of the element type (exact: the value is representable)."""
    fmt = FMT[fmt] if isinstance(fmt, str) else fmt
    return rnd(t64, fmt).to(F32).to(fmt.dtype)


def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 37) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def rel_l2(got, o):
    n = o.norm()
    return float((got.to(F64) - o).norm() / n) if n > 0 else float((got.to(F64) - o).norm())


class Reject(AssertionError):
    def __init__(self, criterion, msg):
        super().__init__(msg)
        self.criterion = criterion


def _ratio(err, tol):
    return torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))


# =================================================================================================================== attention
def _f32(v):
    return float(torch.tensor(v, dtype=F32))


def _rsqrt32(d):
    return float(1.0 / torch.sqrt(torch.tensor(float(d), dtype=F32)))  # the launchers' 1.0f / sqrtf((float)d)


class Kind:
    def __init__(self, name, fmt, d, causal=False, bias=False, rope=False, scale=None, max_len=512, zero_image=None):
        self.name, self.fmt, self.d, self.causal, self.bias, self.rope, self.max_len = name, FMT[fmt], d, causal, bias, rope, max_len
        self.scale = _rsqrt32(d) if scale is None else scale
        self.zero_image = zero_image  # len -> whether the kernel's LDS image holds a zero-filled key `len`


KINDS = {
    "d80": Kind("d80", "f16", 80, max_len=272, zero_image=lambda n: n < 272),  # 17 tiles of 16 keys, always
    "t5": Kind("t5", "bf16", 64, bias=True, scale=1.0, zero_image=lambda n: n not in (64, 128, 256, 512)),  # the body of 64 / 128 / 256 / 512 keys
    "c64": Kind("c64", "f16", 64, causal=True, zero_image=lambda n: n % 64 != 0),  # to the end of the diagonal tile
    "c128": Kind("c128", "f16", 128, causal=True, zero_image=lambda n: n % 64 != 0),
    "c128r": Kind("c128r", "f16", 128, causal=True, rope=True, zero_image=lambda n: n % 64 != 0),
}
NBIAS = 1023
TILE = 64  # keys per tile of the causal kernel's online softmax
SPIKES = ("none", "first", "middle", "last")
H_GAIN, H_MARGIN = 16.0, 40.0  # family H: q = 16 k_j; the lead in base-2 units that Inputs.assert_margins asserts
ROPE_THETA, ROPE_ROWS = 500000.0, 1024  # the kernel reads rows < 512; the packed-row-index mutation reads further

_ROPE = {}


def rope_tables(d=128, theta=ROPE_THETA, rows=ROPE_ROWS):
    """fp32 [rows][d / 2], entry [p][i] = cos / sin(p * theta^(-2 i / d)) (x2v.h), from float64."""
    if (d, theta, rows) not in _ROPE:
        ang = torch.arange(rows, dtype=F64)[:, None] * theta ** (-torch.arange(0, d, 2, dtype=F64) / d)[None, :]
        _ROPE[(d, theta, rows)] = (torch.cos(ang).to(F32), torch.sin(ang).to(F32))
    return _ROPE[(d, theta, rows)]


def rotate(t, pos, dtype, flags=False):
    """t [h, n, d] fp16 rotated at positions pos in `dtype` (t cos + cat(-t[d/2:], t[:d/2]) sin, the table row repeated over both halves), rounded once.
    flags (float64 only): also return, per element, the fp16 spacing where the unrounded value lies within 2^-22 (|t cos| + |t' sin|) of a rounding
    boundary (two fp32 products and their sum, fused or not, stay inside that), else 0: how far an fp32 evaluation may legitimately land from this one."""
    d = t.shape[-1]
    cos, sin = (torch.cat([tab[pos], tab[pos]], -1).to(dtype) for tab in rope_tables(d))
    x = t.to(dtype)
    x2 = torch.cat([-x[..., d // 2 :], x[..., : d // 2]], -1)
    y = x * cos + x2 * sin
    if dtype != F64:
        return y.to(F16)
    r = rnd(y, "f16")
    if not flags:
        return to_fmt(y, "f16")
    space = (((y.contiguous().view(torch.int64) >> 52) & 0x7FF).clamp_min(1023 - 14) - 10 << 52).view(F64)  # the grid's spacing in y's binade
    near = space / 2 - (y - r).abs() <= 2.0 ** -22 * ((x * cos).abs() + (x2 * sin).abs())
    return to_fmt(y, "f16"), torch.where(near, space, torch.zeros_like(space))


def h_map(n, causal):
    """Family H's leading key of row i.  Non-causal: attn_ref's map (keys n - 1, 0, 63, 64 in its image).  Causal: (37 i + 11) mod (i + 1), with the
    diagonal key itself at the tile edges 63, 64, 127, 128 and the last row."""
    if not causal:
        return attn_ref.h_map(n, n)
    i = torch.arange(n, dtype=torch.int64)
    j = (37 * i + 11) % (i + 1)
    for e in (63, 64, 127, 128, n - 1):
        if e < n:
            j[e] = e
    return j


class AttnInputs:
    """One seeded sequence: q [H, n, d], k, v [Hkv, n, d] of the kind's element type on the CPU, bias [H, 1023] fp32 or None.  pos0 = its first row in
    the packed launch, nb = the (k, v) a kernel would read from the neighbouring sequence's rows (set by pack())."""

    def __init__(self, kind, family, n, H, Hkv=None, spike="none", seed=0):
        K = KINDS[kind]
        Hkv = H if Hkv is None else Hkv
        fams = ("R", "N", "H", "U", "B", "S")
        assert family in fams and spike in SPIKES and (spike == "none" or family == "R") and (family != "B" or K.bias) and 1 <= n <= K.max_len and H % Hkv == 0
        self.kind, self.family, self.n, self.H, self.Hkv, self.spike, self.seed, self.pos0, self.nb = kind, family, n, H, Hkv, spike, seed, 0, None
        g = _gen(list(KINDS).index(kind), fams.index(family), n, H, Hkv, SPIKES.index(spike), seed)
        T, d = K.fmt.dtype, K.d
        amp = (1.0 / (K.scale * math.sqrt(d))) ** 0.5  # 1 for the scaled kernels, d^-1/4 for T5
        rn = lambda *shape: torch.randn(*shape, generator=g)
        self.kv_of = [h // (H // Hkv) for h in range(H)]
        bias = rn(H, NBIAS) if K.bias else None
        self.j = None
        if family == "R":
            q, k, v = rn(H, n, d) * amp, rn(Hkv, n, d) * amp, rn(Hkv, n, d)
            if spike != "none":
                j = {"first": 0, "middle": n // 2, "last": n - 1}[spike]
                k[:, j] = k[:, j] * 4
        elif family == "N":
            q, k, v = rn(H, n, d) * amp / 16, rn(Hkv, n, d) * amp, rn(Hkv, n, d)
            bias = None if bias is None else bias / 16
        elif family == "H":
            k = ((torch.randint(0, 2, (Hkv, n, d), generator=g) * 2 - 1) * amp).to(T).to(F32)
            self.j = h_map(n, K.causal)
            q = H_GAIN * k[self.kv_of][:, self.j]
            v = rn(Hkv, n, d)
            v = torch.where(v.abs() < 2.0 ** -6, torch.where(v < 0, -(2.0 ** -6), 2.0 ** -6), v)
        elif family == "U":
            q, k, v = rn(H, n, d) * amp, torch.zeros(Hkv, n, d), torch.ones(Hkv, n, d)
            bias = None if bias is None else torch.zeros_like(bias)
        elif family == "B":
            q, k, v = torch.zeros(H, n, d), rn(Hkv, n, d) * amp, rn(Hkv, n, d)
        else:
            q, k, v = torch.zeros(H, n, d), rn(Hkv, n, d) * amp, torch.zeros(Hkv, n, d)
            v[:, torch.arange(n), torch.arange(n) % d] = 1.0
            bias = None if bias is None else torch.zeros_like(bias)
        self.q, self.k, self.v, self.bias = q.to(T), k.to(T), v.to(T), bias

    @property
    def name(self):
        return f"{self.kind} {self.family}{'' if self.spike == 'none' else '-' + self.spike} n={self.n} H={self.H}/{self.Hkv}" + (f" @{self.pos0}" if self.pos0 else "")

    @property
    def key(self):
        return (self.kind, self.family, self.n, self.H, self.Hkv, self.spike, self.seed, self.pos0)

    def exact(self):
        """What the output must equal bit for bit (H, U, S), or None."""
        K = KINDS[self.kind]
        if self.family == "H":
            return self.v[self.kv_of][:, self.j]
        if self.family == "U":
            return torch.ones(self.H, self.n, K.d, dtype=K.fmt.dtype)
        if self.family == "S":
            hot = torch.zeros(self.n, K.d, dtype=F64)
            hot[torch.arange(self.n), torch.arange(self.n) % K.d] = 1.0
            if K.causal:
                want = hot.cumsum(0) / torch.arange(1, self.n + 1, dtype=F64)[:, None]
            else:
                want = (hot.sum(0) / self.n).expand(self.n, K.d)
            return to_fmt(want, K.fmt).expand(self.H, self.n, K.d)
        return None

    def assert_margins(self):
        """Family H: the matched key leads every other visible key by >= H_MARGIN base-2 units, in float64 on the scores of the entry."""
        if self.family != "H":
            return None
        s, _ = operands(self, F64)
        rows = torch.arange(self.n)
        lead = s[:, rows, self.j].clone()
        assert (s.argmax(-1) == self.j).all(), f"{self.name}: a row is not led by its matched key"
        s[:, rows, self.j] = -math.inf
        margin = float(((lead - s.amax(-1)) * math.log2(math.e)).min()) if self.n > 1 else math.inf
        assert margin >= H_MARGIN, f"{self.name}: the matched key leads by only {margin:.1f} base-2 units"
        return margin


def pack(kind, family, lens, H, Hkv=None, spike="none", seed=0):
    """The sequences of one packed launch, each with its own seed (and the first one's bias table), its first packed row (pos0) and the neighbour's keys (nb): the k / v rows a kernel
    that started one sequence too early would read, (cu[b - 1] + i) for sequence b >= 1."""
    seqs = [AttnInputs(kind, family, n, H, Hkv, spike, seed=1000 * (seed + 1) + b) for b, n in enumerate(lens)]
    allk, allv = torch.cat([s.k for s in seqs], 1), torch.cat([s.v for s in seqs], 1)
    r0 = 0
    for b, s in enumerate(seqs):
        s.pos0, s.bias = r0, seqs[0].bias  # one bias table per launch
        if b >= 1:
            idx = (r0 - lens[b - 1] + torch.arange(s.n)) % allk.shape[1]
            s.nb = (allk[:, idx], allv[:, idx])
        r0 += s.n
    return seqs


ATTN_MUTATIONS = ("drop_last_key", "leak_zero_key", "swap_v_rows", "skip_o_rescale", "mask_late", "mask_early", "bias_delta", "bias_head", "gqa_mod",
                  "rope_packed_pos", "neighbour_keys", "d80_low64")


def mutation_applies(mut, inp):
    K, n = KINDS[inp.kind], inp.n
    return {"drop_last_key": n >= 2, "leak_zero_key": K.zero_image(n), "swap_v_rows": n >= 2, "skip_o_rescale": K.causal and n > TILE, "mask_late": K.causal and n >= 2,
            "mask_early": K.causal and n >= 2, "bias_delta": K.bias, "bias_head": K.bias and inp.H >= 2,
            "gqa_mod": K.causal and any(h % inp.Hkv != h // (inp.H // inp.Hkv) for h in range(inp.H)), "rope_packed_pos": K.rope and inp.pos0 > 0,
            "neighbour_keys": inp.nb is not None, "d80_low64": inp.kind == "d80"}[mut]


def operands(inp, dtype, mut=None):
    """(s [H, n, nk] the scores in natural units with -inf on the masked keys, v [H, nk, d]) in `dtype`; nk = n, or n + 1 with the leaked key.
    mut: one of ATTN_MUTATIONS (a subtly WRONG kernel) or None."""
    K, n, H = KINDS[inp.kind], inp.n, inp.H
    q, (k, v) = inp.q, (inp.nb if mut == "neighbour_keys" else (inp.k, inp.v))
    if K.rope:
        pos = torch.arange(n)
        q, k = rotate(q, pos + (inp.pos0 if mut == "rope_packed_pos" else 0), dtype), rotate(k, pos + (inp.pos0 if mut == "rope_packed_pos" else 0), dtype)
    kv_of = [h % inp.Hkv for h in range(H)] if mut == "gqa_mod" else inp.kv_of
    qd, kd, vd = q.to(dtype), k.to(dtype)[kv_of], v.to(dtype)[kv_of]
    if mut == "d80_low64":
        qd, kd = qd[..., :64], kd[..., :64]
    if mut == "swap_v_rows":
        a, b = 0, min(TILE - 1, n - 1)
        vd = vd.clone()
        vd[:, [a, b]] = vd[:, [b, a]]
    leak = mut == "leak_zero_key"
    if leak:  # its K row and its V^T column are the zero fill of the LDS image
        kd, vd = torch.cat([kd, torch.zeros_like(kd[:, :1])], 1), torch.cat([vd, torch.zeros_like(vd[:, :1])], 1)
    nk = n + int(leak)
    s = (qd @ kd.transpose(-1, -2)) * torch.tensor(K.scale, dtype=dtype)
    i, j = torch.arange(n)[:, None], torch.arange(nk)[None, :]
    if K.bias:
        b = inp.bias.to(dtype)
        if mut == "bias_head":
            b = b.roll(-1, 0)
        s = s + b[:, (j - i + 511 + int(mut == "bias_delta")).clamp(0, NBIAS - 1)]
    if K.causal:
        ok = (j <= i + 1) & (j < n) if mut == "mask_late" else ((j < i) | (j == 0)) if mut == "mask_early" else (j <= i) & (j < n)
        if leak:  # the diagonal tile's mask is what hides it: the rows of the last 64-row block see it
            ok = ok | ((j == n) & (i >= (n - 1) // TILE * TILE))
        s = s.masked_fill(~ok, -math.inf)
    if mut == "drop_last_key":
        s = s.clone()
        s[..., n - 1] = -math.inf  # causal: only row n - 1 ever saw it
    return s, vd


def rope_slack(inp, w, A, v):
    """The rotary entries' term R of the element bound: the fp16 rounding of a rotated q or k element whose exact value lies next to a rounding
    boundary may fall to either side in a correct fp32 kernel (rotate's flags): dq, dk = one spacing on those elements, else 0.  The scores then move
    by at most DS_ij = scale (dq_i . |k_j| + |q_i| . dk_j + dq_i . dk_j), the weights to w'_j = w_j e^(ds_j) / Z, Z = sum_k w_k e^(ds_k).  With
    |e^x - 1| <= |x| e^|x| and Z >= e^-max DS: |w'_j - w_j| <= w_j e^(2 max DS) (DS_ij + sum_k w_k DS_ik), hence
    R_d = e^(2 max_j DS_ij) (sum_j w_j DS_ij |v_jd| + (sum_k w_k DS_ik) A_d).  Zero for rows that meet no flagged element."""
    K = KINDS[inp.kind]
    pos = torch.arange(inp.n)
    (q, dq), (k, dk) = rotate(inp.q, pos, F64, True), rotate(inp.k, pos, F64, True)
    q, k, dk = q.to(F64).abs(), k.to(F64).abs()[inp.kv_of], dk[inp.kv_of]
    DS = K.scale * (dq @ k.transpose(-1, -2) + q @ dk.transpose(-1, -2) + dq @ dk.transpose(-1, -2))
    DS = torch.where(w > 0, DS, torch.zeros_like(DS))  # masked keys
    return torch.exp(2 * DS.amax(-1, keepdim=True)) * ((w * DS) @ v.abs() + (w * DS).sum(-1, keepdim=True) * A)


def ref64(inp):
    """float64 attention of the entry.  Returns (o, A, F), each [H, n, d]; F holds the fp16 subnormal term and, for the rotary entry, rope_slack's R."""
    s, v = operands(inp, F64)
    P = torch.exp(s - s.amax(-1, keepdim=True))
    l = P.sum(-1, keepdim=True)
    w = P / l
    o, A = w @ v, w @ v.abs()
    if KINDS[inp.kind].fmt.name == "f16":
        F = SUB16 / l * (((P > 0) & (P < 2.0 ** -14)).to(F64) @ v.abs())
    else:
        F = torch.zeros_like(o)
    if KINDS[inp.kind].rope:
        F = F + rope_slack(inp, w, A, v)
    return o, A, F


EMULATIONS = ("global", "tiled")


def emulate_attn(inp, how="global", mut=None):
    """A correct kernel in fp32 torch: 'global' (one pass, the global row maximum) or 'tiled' (64-key tiles, a rescale on every tile).  P is rounded
    to T for the PV product only, the row sum takes it unrounded, O is divided in fp32 and rounded once.  mut: a subtly WRONG kernel."""
    T = KINDS[inp.kind].fmt.dtype
    s, v = operands(inp, F32, mut)
    if how == "global":
        p = torch.exp(s - s.amax(-1, keepdim=True))
        return ((p.to(T).to(F32) @ v) / p.sum(-1, keepdim=True)).to(T)
    H, n, nk = s.shape
    m, l, o = torch.full((H, n, 1), -math.inf), torch.zeros(H, n, 1), torch.zeros(H, n, v.shape[-1])
    for t0 in range(0, nk, TILE):
        st = s[..., t0 : t0 + TILE]
        m_new = torch.maximum(m, st.amax(-1, keepdim=True))  # finite from the first tile on: key 0 is never masked
        al = torch.exp(m - m_new)
        p = torch.exp(st - m_new)
        l = l * al + p.sum(-1, keepdim=True)
        o = (o if mut == "skip_o_rescale" else o * al) + p.to(T).to(F32) @ v[:, t0 : t0 + TILE]
        m = m_new
    return (o / l).to(T)


class AttnExpect:
    def __init__(self, inp, keep=False):
        self.inp = inp
        self.o, self.A, self.F = ref64(inp)
        outs = {how: emulate_attn(inp, how) for how in EMULATIONS}
        self.y = {how: rel_l2(e, self.o) for how, e in outs.items()}
        self.Y = max(self.y.values())
        self.emulated = outs if keep else None

    def tol(self):
        f = KINDS[self.inp.kind].fmt
        return f.u * self.o.abs() + P_SLACK * f.p * self.A + self.F


_EXPECT = {}


def attn_expect(inp):
    """AttnExpect computed once per case and shared by the tests of a run."""
    if inp.key not in _EXPECT:
        _EXPECT[inp.key] = AttnExpect(inp)
    return _EXPECT[inp.key]


class AttnCase:
    """Accumulates the figures of one kernel over its inputs; every check asserts all criteria."""

    def __init__(self, name):
        self.name, self.rows = name, []

    def check(self, got, exp, what=""):
        """got: T [H, n, d] on the CPU.  Returns (relL2, Y, worst d / tol)."""
        tag = f"{self.name} {exp.inp.name} {what}".strip()
        g = got.to(F64)
        if g.shape != exp.o.shape:
            raise Reject("shape", f"{tag}: shape {tuple(g.shape)} vs {tuple(exp.o.shape)}")
        if not torch.isfinite(g).all():
            raise Reject("finite", f"{tag}: non-finite output")
        err, tol = (g - exp.o).abs(), exp.tol()
        ratio = _ratio(err, tol)
        worst, rel = float(ratio.max()), rel_l2(g, exp.o)
        self.rows.append((exp.inp.family, rel, exp.Y, worst))
        if worst > 1.0:
            i = int(ratio.reshape(-1).argmax())
            over = ratio > 1.0
            raise Reject("element", f"{tag}: {int(over.sum())} of {err.numel()} elements ({float(over.double().mean()):.2%}) outside u|o| + 1.05 p A + F; worst d/tol {worst:.3f} at "
                                    f"flat index {i}: got {g.reshape(-1)[i].item():.9g} ref {exp.o.reshape(-1)[i].item():.9g} tol {tol.reshape(-1)[i].item():.3g}")
        if rel > TRIANGLE * exp.Y:
            raise Reject("aggregate", f"{tag}: relL2 {rel:.4e} > 1.5 * Y, Y = {exp.Y:.4e} ({', '.join(f'{k} {y:.4e}' for k, y in exp.y.items())})")
        ex = exp.inp.exact()
        if ex is not None and not torch.equal(got, ex):
            raise Reject("exact", f"{tag}: {int((got != ex).sum())} elements differ from the exact answer of family {exp.inp.family}")
        return rel, exp.Y, worst

    def table(self):
        """One line per family: number of checks, worst d / tol, the largest relL2 with its Y."""
        out = []
        for fam in sorted({r[0] for r in self.rows}):
            rows = [r for r in self.rows if r[0] == fam]
            _, rel, Y, _ = max(rows, key=lambda r: (r[1] / r[2] if r[2] > 0 else 0.0, r[1]))
            out.append(f"{self.name:<28} family {fam:<2} n={len(rows):<4} worst d/tol {max(r[3] for r in rows):5.3f}  relL2 {rel:.4e}  Y {Y:.4e}")
        return out


# ------------------------------------------------------------------------------------------------------------------- the attention case list
D80_S = (1, 15, 16, 17, 63, 64, 65, 256, 257, 271, 272)
D80_BATCH = (257, 257)
T5_LENS = (1, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512)
T5_PACKS = ((37, 64, 1, 130), (300, 77))  # the second: two different key-row classes (512 and 128) in one launch
CAUSAL_LENS = (1, 63, 64, 65, 127, 128, 129, 511, 512)
CAUSAL_PACKS = ((1, 64, 65), (33,) * 8)
CAUSAL_HEADS = ((4, 1), (4, 2), (2, 2))
CAUSAL_KINDS = ("c64", "c128", "c128r")


def attn_families(kind):
    fams = [("R", s) for s in SPIKES] + [("N", "none"), ("H", "none"), ("U", "none"), ("S", "none")]
    return fams + ([("B", "none")] if KINDS[kind].bias else [])


def attn_launches():
    """Every launch of the GPU module: (kind, lens, H, Hkv).  Each runs every family of attn_families(kind)."""
    out = [("d80", (S,), 2, 2) for S in D80_S] + [("d80", D80_BATCH, 3, 3)]
    out += [("t5", (n,), 3, 3) for n in T5_LENS] + [("t5", T5_PACKS[0], 4, 4), ("t5", T5_PACKS[1], 2, 2)]
    for kind in CAUSAL_KINDS:
        out += [(kind, lens, H, Hkv) for lens in [(n,) for n in CAUSAL_LENS] + list(CAUSAL_PACKS) for H, Hkv in CAUSAL_HEADS]
    return out


def attn_sequences(kind, lens, H, Hkv, family, spike):
    """The sequences of one launch and family: one AttnInputs, or pack()'s list."""
    return [AttnInputs(kind, family, lens[0], H, Hkv, spike)] if len(lens) == 1 else pack(kind, family, lens, H, Hkv, spike)


# =================================================================================================================== GEMM
EPI_NONE, EPI_GELU_ERF, EPI_QUICK_GELU, EPI_RESIDUAL, EPI_GEGLU, EPI_SWIGLU = "none", "gelu_erf", "quick_gelu", "resid", "geglu", "swiglu"
ENTRY_EPIS = {"f16": (EPI_NONE, EPI_GELU_ERF, EPI_QUICK_GELU, EPI_RESIDUAL, EPI_SWIGLU), "bf16": (EPI_NONE, EPI_RESIDUAL, EPI_GEGLU)}
GATED = (EPI_GEGLU, EPI_SWIGLU)
L_GELU_ERF, L_QUICK_GELU, L_SILU, L_GELU_TANH = 1.13, 1.10, gemm_ref.L_SILU, gemm_ref.L_GELU


def gelu_erf64(t):
    return 0.5 * t * (1.0 + torch.erf(t * math.sqrt(0.5)))


def quick_gelu64(t):
    return t / (1.0 + torch.exp(-1.702 * t))


ACT64 = {EPI_GELU_ERF: (gelu_erf64, L_GELU_ERF), EPI_QUICK_GELU: (quick_gelu64, L_QUICK_GELU), EPI_GEGLU: (gemm_ref.gelu64, L_GELU_TANH), EPI_SWIGLU: (gemm_ref.silu64, L_SILU)}
TILES = ((128, 64), (64, 64), (64, 32), (64, 16))


def tile_choice(M, Nw):
    """gemm_rows.h: the largest tile of {128x64, 64x64, 64x32, 64x16} (rows of x by rows of W) that still yields >= 192 workgroups, else the smallest."""
    for bm, bn in TILES[:3]:
        if -(-M // bm) * -(-Nw // bn) >= 192:
            return (bm, bn)
    return TILES[3]


class GemmInputs:
    """One seeded case: x [M, K], w [Nw, K], resid [M, Nw] of the entry's element type, bias [Nw] (the fp16 entry; the bf16 entry has none).  The gated
    epilogues read the same w as [2 N, K], N = Nw / 2, without the bias."""

    def __init__(self, family, fmt, M, Nw, K, seed=0):
        assert family in ("I", "R") and fmt in FMT and K % 32 == 0 and Nw % 4 == 0
        self.family, self.fmt, self.M, self.Nw, self.K, self.seed = family, FMT[fmt], M, Nw, K, seed
        T = self.fmt.dtype
        g = _gen("IR".index(family), list(FMT).index(fmt), M, Nw, K, seed)
        ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).to(F32)
        rn = lambda *shape: torch.randn(*shape, generator=g)
        self.bias = self.bias_range = None
        if family == "I":
            sk, sn = ri(0, 1, K) * 2 - 1, ri(0, 1, Nw) * 2 - 1
            x, w, resid = ri(0, 8, M, K) * sk, ri(0, 4, Nw, K) * sk * sn[:, None], ri(-200, 200, M, Nw)
        else:
            x, w, resid = rn(M, K), rn(Nw, K) / math.sqrt(K), rn(M, Nw)
        self.x, self.w, self.resid = x.to(T), w.to(T), resid.to(T)
        x64, w64 = self.x.to(F64), self.w.to(F64)
        self.acc = x64 @ w64.T
        self.absacc = x64.abs() @ w64.abs().T if family == "R" else None
        if fmt == "f16":
            if family == "R":
                self.bias = rn(Nw).to(T)
            else:  # gemm_ref's widening: double the range until the roundings of acc + bias are exercised, with a factor of two in hand
                b = 64
                while True:
                    self.bias = ri(-b, b, Nw).to(T)
                    t = self.t()
                    if float((rnd(t, self.fmt) != t).double().mean()) >= 2 * MIN_INEXACT or b >= 16384:
                        break
                    b *= 2
                self.bias_range = b

    @property
    def name(self):
        return f"{self.family} {self.fmt.name} {self.M}x{self.Nw}x{self.K}"

    def t(self, use_bias=True):
        return self.acc + self.bias.to(F64)[None, :] if (use_bias and self.bias is not None) else self.acc

    def S(self, use_bias=True):
        return self.absacc + self.bias.to(F64).abs()[None, :] if (use_bias and self.bias is not None) else self.absacc

    def assert_exercises_roundings(self):
        """Family I's premises: |t| < 2^24, t an fp32 number, >= 5 % of t inexact before its rounding.  Returns the fraction."""
        assert self.family == "I"
        t = self.t()
        assert float(t.abs().max()) < 2.0 ** 24 and float(self.acc.abs().max()) < 2.0 ** 24 and torch.equal(t.to(F32).to(F64), t), f"{self.name}: t is not exact in fp32"
        frac = float((rnd(t, self.fmt) != t).double().mean())
        assert frac >= MIN_INEXACT, f"{self.name}: only {frac:.1%} of t is inexact before its rounding (bias range {self.bias_range})"
        return frac


class GemmExpect:
    """Reference side of one (inputs, epilogue): f, tol (family R) or exact (family I: NONE and RESIDUAL)."""

    def __init__(self, inp, epi):
        assert epi in ENTRY_EPIS[inp.fmt.name]
        self.inp, self.epi = inp, epi
        fmt, h = inp.fmt, inp.fmt.h
        self.f = self.tol = self.exact = None
        if inp.family == "I":
            assert epi in (EPI_NONE, EPI_RESIDUAL)
            y = rnd(inp.t(), fmt)
            if epi == EPI_RESIDUAL:
                y = rnd(inp.resid.to(F64) + y, fmt)
            self.exact = y.to(F32).to(fmt.dtype)
            return
        gated = epi in GATED
        t, S = inp.t(not gated), inp.S(not gated)
        sub = SUB16 if fmt.name == "f16" else 0.0  # a result below 2^-14 is rounded on fp16's subnormal grid: at most 2^-25 absolutely
        e0 = h * t.abs() + sub + (1 + h) * (inp.K + 1) * UNIT * S
        if epi == EPI_NONE:
            self.f, self.tol = t, e0
        elif epi == EPI_RESIDUAL:
            self.f = inp.resid.to(F64) + t
            self.tol = e0 + h * (self.f.abs() + e0) + sub
        elif not gated:
            f, L = ACT64[epi]
            self.f = f(t)
            tol = L * e0 + ACT_EVAL * self.f.abs()
            self.tol = tol + h * (self.f.abs() + tol) + sub
        else:
            f, L = ACT64[epi]
            if epi == EPI_GEGLU:  # T(T(a) f(T(g))): a = fc1 (row 2n), g = gate.0 (row 2n + 1)
                lin, ein, act, eact = t[:, 0::2], e0[:, 0::2], t[:, 1::2], e0[:, 1::2]
            else:  # T(f(T(a)) T(g)): a = gate_proj (row 2n) under the SiLU, g = up_proj (row 2n + 1)
                lin, ein, act, eact = t[:, 1::2], e0[:, 1::2], t[:, 0::2], e0[:, 0::2]
            G = f(act)
            dG = L * eact + ACT_EVAL * (G.abs() + L * eact)
            self.f = lin * G
            ep = lin.abs() * dG + G.abs() * ein + ein * dG
            ep = ep + UNIT * (self.f.abs() + ep)
            self.tol = ep + h * (self.f.abs() + ep) + sub

    @property
    def what(self):
        return self.epi


_GEMM_INPUTS = {}


def gemm_inputs(family, fmt, M, Nw, K):
    key = (family, fmt, M, Nw, K)
    if key not in _GEMM_INPUTS:
        _GEMM_INPUTS[key] = GemmInputs(family, fmt, M, Nw, K)
    return _GEMM_INPUTS[key]


class GemmCase(gemm_ref.Case):
    """gemm_ref's two rules (check_exact bit for bit, check_bound on every element) for either 16-bit element type."""

    def __init__(self, name):
        super().__init__(name, record=False)

    def check_exact(self, got, exp, body=""):
        tag = f"{self.name} {exp.inp.name} {body} {exp.what}"
        if got.shape != exp.exact.shape or got.dtype != exp.exact.dtype:
            raise Reject("shape", f"{tag}: {tuple(got.shape)} {got.dtype} vs {tuple(exp.exact.shape)} {exp.exact.dtype}")
        ne = got.view(torch.int16) != exp.exact.view(torch.int16)
        bad = int(ne.sum())
        self._row(exp, body, "exact", float(bad), got.numel())
        if bad:
            m, n = divmod(int(ne.reshape(-1).double().argmax()), got.shape[1])
            rows, cols = ne.any(1).nonzero().flatten(), ne.any(0).nonzero().flatten()
            raise Reject("exact", f"{tag}: {bad} of {got.numel()} elements differ from the float64 chain; first at ({m}, {n}): got {float(got[m, n])} want {float(exp.exact[m, n])}; "
                                  f"rows {int(rows[0])}..{int(rows[-1])} ({rows.numel()}), columns {int(cols[0])}..{int(cols[-1])} ({cols.numel()})")
        return 0.0

    def check_bound(self, got, exp, body=""):
        try:
            return super().check_bound(got, exp, body)
        except gemm_ref.Reject as e:
            raise Reject(e.criterion, str(e)) from None

    def summary(self):
        """One line per epilogue and rule: number of checks, worst d / tol or unequal elements."""
        out = []
        for what in sorted({r[2] for r in self.rows}):
            for rule in ("exact", "bound"):
                rows = [r for r in self.rows if r[2] == what and r[3] == rule]
                if rows:
                    fig = f"worst d/tol {max(r[4] for r in rows):5.3f}" if rule == "bound" else f"unequal {int(sum(r[4] for r in rows))}"
                    out.append(f"{self.name:<28} {what:<11} {'family R' if rule == 'bound' else 'family I'} n={len(rows):<4} {fig}  elements {sum(r[5] for r in rows)}")
        return out


GEMM_MUTATIONS = {"drop_last_kstep": ("I", EPI_NONE), "last_kstep_twice": ("I", EPI_NONE), "resid_one_rounding": ("I", EPI_RESIDUAL), "half_up": ("I", EPI_NONE),
                  "swap_value_gate": ("R", "gated")}  # mutation -> the family and epilogue whose check must reject it


def _r32(v, fmt, mode="rne"):
    return rnd(v.to(F64), fmt, mode).to(F32)


def emulate_gemm(inp, epi, mut=None, chunk=32):
    """A correct kernel in fp32 torch: the product accumulated over 32-wide k-steps in fp32, the bias add in fp32, then the contract's roundings around
    fp32 activations.  mut: one of GEMM_MUTATIONS — a subtly WRONG kernel.  Returns T [M, N]."""
    fmt = inp.fmt
    x, w = inp.x.to(F32), inp.w.to(F32)
    steps = list(range(0, inp.K, chunk))
    if mut == "drop_last_kstep":
        steps = steps[:-1]
    elif mut == "last_kstep_twice":
        steps = steps + steps[-1:]
    acc = torch.zeros(inp.M, inp.Nw, dtype=F32)
    for k0 in steps:
        acc = acc + x[:, k0 : k0 + chunk] @ w[:, k0 : k0 + chunk].T
    mode = "half_up" if mut == "half_up" else "rne"
    r = lambda v: _r32(v, fmt, mode)
    if epi in GATED:
        a, g = r(acc[:, 0::2]), r(acc[:, 1::2])
        if mut == "swap_value_gate":
            a, g = g, a
        if epi == EPI_GEGLU:
            u = 0.7978845608028654 * (g + 0.044715 * g * g * g)
            y = a * (g / (1.0 + torch.exp(-2.0 * u)))
        else:
            y = a / (1.0 + torch.exp(-a)) * g
        return r(y).to(fmt.dtype)
    t = acc + inp.bias.to(F32) if inp.bias is not None else acc
    if epi == EPI_GELU_ERF:
        y = 0.5 * t * (1.0 + torch.erf(t * 0.70710678118654752440))
    elif epi == EPI_QUICK_GELU:
        y = t / (1.0 + torch.exp(-1.702 * t))
    elif epi == EPI_RESIDUAL:
        y = inp.resid.to(F32) + (t if mut == "resid_one_rounding" else r(t))
    else:
        y = t
    return r(y).to(fmt.dtype)


# ------------------------------------------------------------------------------------------------------------------- the GEMM case list
GEMM_K = (32, 64, 96, 128, 160, 224, 256)  # K / 32 = 1, 2, 3, 4, 5, 7, 8: below, at and past the ring of 4
GEMM_K3 = (32, 160, 256)
GEMM_M = (1, 15, 16, 17, 63, 64, 65, 129, 145)
GEMM_TILE_SHAPES = (((128, 64), 145, 6148), ((64, 64), 65, 6148), ((64, 32), 65, 3076), ((64, 16), 65, 132))  # (tile, M, rows of W); an N tail of 4 columns each
GEMM_TAIL20 = (((128, 64), 145, 6164), ((64, 32), 65, 3092), ((64, 16), 17, 148))  # the last column block holds 20 (64-wide, 32-wide) and 4 of a second 16 (148 = 9 * 16 + 4)
GEMM_BATCHED = (145, 6148, 160, ((0, 65), (65, 145)))  # M, rows of W, K, the row ranges computed alone: 128x64 against 64x64


def gemm_shapes():
    """(M, rows of W, K, tile) of every GEMM call family of the GPU module."""
    out = [(M, Nw, K, tile) for tile, M, Nw in GEMM_TILE_SHAPES for K in (GEMM_K if tile == (64, 16) else GEMM_K3)]
    out += [(M, 132, 160, (64, 16)) for M in GEMM_M if M != 65]
    out += [(M, Nw, 160, tile) for tile, M, Nw in GEMM_TAIL20]
    for M, Nw, K, tile in out:
        assert tile_choice(M, Nw) == tile, (M, Nw, tile_choice(M, Nw), tile)
    return out


def gemm_strides(K, Nw, Ny):
    """(ldx, ldw, ldy, ldr): four different values, all larger than the extent, ldx / ldw multiples of 8, ldy / ldr of 4."""
    ldx, ldw, ldy, ldr = K + 8, K + 16, (Ny + 4 + 3) // 4 * 4, Nw + 12
    while ldy in (ldx, ldw, ldr):
        ldy += 4
    while ldr in (ldx, ldw, ldy):
        ldr += 4
    assert len({ldx, ldw, ldy, ldr}) == 4
    return ldx, ldw, ldy, ldr


# =================================================================================================================== norms
RMS_D = (8, 504, 512, 520, 2048, 2056, 4096, 4104, 6144, 6152, 8192)  # the one-wave path to 512, then chunks_for(D, 4) = 1 | 2 | 3 | 4 at 2048 | 4096 | 6144
RMS_M = (1, 3, 4, 5)  # four rows per block on the one-wave path
RMS_SETS = ("n01", "small", "large")
LN_D = (8, 160, 2040, 2048)
LN_SETS = ("n01", "offset")
LN_M = 5
EMBED_SHAPES = ((1, 2), (3, 2), (1, 257), (3, 257))  # (batch, tokens)
NORM_EPS = 1e-5


def _f32eps(eps):
    return float(torch.tensor(eps, dtype=F32))


def norm_inputs(kind, D, M, which):
    g = _gen(["rms", "ln", "embed"].index(kind), D, M, (RMS_SETS + LN_SETS).index(which))
    x = torch.randn(M, D, generator=g) * {"n01": 1.0, "small": 2.0 ** -6, "large": 100.0, "offset": 1.0}[which] + (8.0 if which == "offset" else 0.0)
    w = 1.0 + 0.25 * torch.randn(D, generator=g)
    b = 0.25 * torch.randn(D, generator=g)
    return x.to(F16), (w.to(F16) if kind == "rms" else w), b


def rmsnorm64(x, w, eps=NORM_EPS, dtype=F64):
    """x2v_rmsnorm_f16: w * x * rsqrt(mean(x^2) + eps), unrounded.  Returns (y, atol)."""
    x = x.to(dtype)
    y = x * (1.0 / torch.sqrt((x * x).mean(-1, keepdim=True) + _f32eps(eps))) * w.to(dtype)
    return y, torch.full_like(y[:, :1], SUB16)


def layernorm64(x, w, b, eps=NORM_EPS, dtype=F64):
    """x2v_layernorm_f16: LN(x; w, b, eps), unrounded.  Returns (y, atol): one ulp of the row's largest |x - mean| rstd |w| term, plus SUB16."""
    x = x.to(dtype)
    d = x - x.mean(-1, keepdim=True)
    y = d * (1.0 / torch.sqrt((d * d).mean(-1, keepdim=True) + _f32eps(eps))) * w.to(dtype)
    return y + b.to(dtype), FMT["f16"].u * y.abs().amax(-1, keepdim=True) + SUB16


def clip_embed64(patches, cls, pos, w, b, batch, eps=NORM_EPS, dtype=F64):
    """x2v_clip_embed_f16: row b * tokens + t = LN(fp16(tok + pos[t])), tok = cls (t = 0) or patches[b * (tokens - 1) + t - 1]."""
    tokens = patches.shape[0] // batch + 1
    rows = torch.cat([torch.cat([cls[None], patches[i * (tokens - 1) : (i + 1) * (tokens - 1)]], 0) for i in range(batch)], 0)
    s = rows.to(dtype) + pos.repeat(batch, 1).to(dtype)
    s = rnd(s, "f16") if dtype == F64 else s.to(F16).to(dtype)
    return layernorm64(s, w, b, eps, dtype)


class NormCase:
    """rowwise_ref.Case's rule at fp16: the hard bound per call, the flip share over the whole case."""

    def __init__(self, name):
        self.name, self.n, self.flips, self.checks, self.worst = name, 0, 0, 0, 0.0

    def check(self, got, ref, what=""):
        y, atol = ref
        g = got.to(F64)
        if g.shape != y.shape:
            raise Reject("shape", f"{self.name} {what}: shape {tuple(g.shape)} vs {tuple(y.shape)}")
        if not torch.isfinite(g).all():
            raise Reject("finite", f"{self.name} {what}: non-finite output")
        err, bound = (g - y).abs(), FMT["f16"].u * y.abs() + atol
        ratio = _ratio(err, bound)
        self.worst = max(self.worst, float(ratio.max()))
        if float(ratio.max()) > 1.0:
            i = int(ratio.reshape(-1).argmax())
            raise Reject("element", f"{self.name} {what}: {int((ratio > 1).sum())} of {y.numel()} elements outside 2^-10|ref| + atol; worst at flat index {i}: "
                                    f"got {g.reshape(-1)[i].item():.9g} ref {y.reshape(-1)[i].item():.9g}")
        self.flips += int((got.view(torch.int16) != to_fmt(y, "f16").view(torch.int16)).sum())
        self.n += y.numel()
        self.checks += 1

    @property
    def flip_share(self):
        return self.flips / max(self.n, 1)

    def finish(self):
        if self.flip_share > FLIP_CAP:
            raise Reject("flips", f"{self.name}: {self.flips} of {self.n} elements ({self.flip_share:.2e}) differ from fp16(ref), cap {FLIP_CAP:.0e}")

    def summary(self):
        return [f"{self.name:<28} n={self.checks:<4} worst d/tol {self.worst:5.3f}  flip share {self.flip_share:.2e}  elements {self.n}"]
