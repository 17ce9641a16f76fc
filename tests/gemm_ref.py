"""float64 references, seeded inputs, fp32 emulations and the acceptance rules for the GEMM family of lightx2v_amd/csrc (gemm.hip, gemm256.hip,
gemm256s.hip, gemm256c.hip, gemm256c8.hip).  Plain PyTorch; nothing here imports the library or the oracle.  Shared by tests/test_gemm_ref_host.py
(the yardstick checked without a GPU) and tests/test_gpu_gemm_fp64.py (the kernels checked against it).

The references restate the contracts of include/x2v.h, not a kernel:
  bf16   t = x . W^T + bias                                   w8a8   t = (xq . wq^T) * sx[m] * sw[n] + bias     (codes and scales taken as given)
  NONE bf16(t) | GELU_TANH bf16(gelu(bf16(t))) | SILU bf16(silu(bf16(t))) | RESIDUAL bf16(resid + bf16(bf16(t) * gate)), without a gate bf16(resid + bf16(t))

Two input families, two acceptance rules (Case.check_exact / Case.check_bound), no share of elements left out of either:

  I  small integers (x in [-8, 8], W in [-4, 4], bias in [-64, 64] and wider at short K, gate a multiple of 0.5, resid in [-200, 200], sx and sw powers
     of two, codes integers).  Every product and partial sum is exact in fp32 (|t| < 2^24 and t an fp32 number are asserted), every later step is one
     correctly rounded operation on exact inputs: NONE and RESIDUAL must equal the float64 chain rounded to bf16 BIT FOR BIT at any K.  This is what
     sees a missing or extra rounding point, round-half-up in place of ties-to-even, and a K tile dropped, doubled or read from the wrong stage.
     Inputs.assert_exercises_roundings() asserts that at least 5 % of acc + bias and of bf16(acc + bias) * gate are inexact before their rounding.

  R  seeded N(0, 1) x, W ~ N(0, 1) / sqrt(K), bf16-rounded (w8a8: codes of such values, positive scales): a bound on EVERY element against the
     unrounded float64 result.  With S = |x| . |W|^T (* sx * sw) + |bias|, E = (K + 1) 2^-23 S (w8a8: K + 3, for the two scale multiplications and
     the bias add), h = 2^-8 and e0 = h |t| + (1 + h) E:
        NONE        |got - t| <= e0
        GELU, SILU  tol = L e0 + 2^-16 |f|, then tol += h (|f| + tol); L the Lipschitz constant of f (L_GELU, L_SILU below, asserted by the host test)
        RESIDUAL    p = t gate, e1 = |gate| e0, e1 += h (|p| + e1) (only with a gate), tol = e1 + h (|resid + p| + e1)
     E is the a-priori bound of an fp32 accumulation of exact products in any order, with the unit 2^-23 = twice the round-to-nearest unit roundoff,
     so that a matrix unit that truncates when it aligns addends is covered too; 2^-16 |f| covers the fp32 evaluation of the activation.  None of
     these constants is fitted to a kernel's output."""
import math

import torch

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
E4M3, I8 = torch.float8_e4m3fn, torch.int8
EPI_NONE, EPI_GELU, EPI_RESIDUAL, EPI_SILU = 0, 1, 2, 3  # x2v.h X2V_EPI_*
EPI_NAMES = {EPI_NONE: "none", EPI_GELU: "gelu", EPI_RESIDUAL: "resid", EPI_SILU: "silu"}
H = 2.0 ** -8  # largest relative error of one rounding to bf16
UNIT = 2.0 ** -23
ACT_EVAL = 2.0 ** -16
L_GELU, L_SILU = 1.13, 1.10
DTYPES = ("bf16", "e4m3", "int8")
KTILE = {"bf16": 64, "e4m3": 128, "int8": 128}  # K elements per K tile of the kernels
MIN_INEXACT = 0.05


# ------------------------------------------------------------------------------------------------------------------- float64 pieces
def round_bf16(t, mode="rne"):
    """float64 -> the nearest number with 8 significant bits, as float64 (one rounding: never through fp32).  mode 'rne' = ties to even (the
    contract), 'half_up' and 'trunc' = the wrong roundings of the host module's mutations.  Normal range only.  The two powers of two are put
    together from their bits, so every step is exact on any device (torch.ldexp goes through pow, which need not be)."""
    e = ((t.view(torch.int64) >> 52) & 0x7FF).clamp_min(8)  # biased exponent of t = 1.m * 2^(e - 1023)
    q, qinv = ((e - 7) << 52).view(F64), ((2046 - (e - 7)) << 52).view(F64)  # 2^(e - 1023 - 7) and its reciprocal
    r = t * qinv  # exact: |r| in [128, 256)
    r = {"rne": torch.round, "half_up": lambda v: torch.floor(v + 0.5), "trunc": torch.trunc}[mode](r)
    return r * q


def gelu64(t):
    return 0.5 * t * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (t + 0.044715 * t ** 3)))


def silu64(t):
    return t / (1.0 + torch.exp(-t))


ACT64 = {EPI_GELU: (gelu64, L_GELU), EPI_SILU: (silu64, L_SILU)}


def lipschitz(f, lo=-12.0, hi=12.0, n=2_400_001):
    """max |f'| on [lo, hi] in float64 by central differences on a grid of 1e-5 (f' is flat beyond |t| = 12 for both activations)."""
    t = torch.linspace(lo, hi, n, dtype=F64)
    d = (f(t[2:]) - f(t[:-2])) / (t[2:] - t[:-2])
    return float(d.abs().max())


def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 31) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _pow2(g, n, lo, hi):
    return torch.ldexp(torch.ones(n, dtype=F32), torch.randint(lo, hi + 1, (n,), generator=g, dtype=torch.int32))


# ------------------------------------------------------------------------------------------------------------------- inputs
class Inputs:
    """One seeded case on `device`: x [M, K], w [N, K] (bf16, or e4m3 / int8 codes with sx [M], sw [N] fp32), bias, gate [N] bf16, resid [R, N] bf16
    (R = resid_rows or M).  The float64 product and |product| are computed once, on `device` (rocBLAS's float64 matmul is independent of the kernels
    under test; the small cases stay on the CPU)."""

    def __init__(self, family, dtype, M, N, K, seed=0, resid_rows=None, device="cpu"):
        assert family in ("I", "R") and dtype in DTYPES
        self.family, self.dtype, self.M, self.N, self.K, self.seed, self.device = family, dtype, M, N, K, seed, device
        R = resid_rows or M
        g = _gen("IR".index(family), DTYPES.index(dtype), M, N, K, seed, R)
        ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).to(F32)
        rn = lambda *shape: torch.randn(*shape, generator=g)
        code = {"bf16": BF16, "e4m3": E4M3, "int8": I8}[dtype]
        self.sx = self.sw = None
        if family == "I":
            x, w = ri(-8, 8, M, K).to(code), ri(-4, 4, N, K).to(code)
            gate = (0.5 * ((torch.arange(N) % 7) - 3)[torch.randperm(N, generator=g)]).to(BF16)  # every multiple of 0.5 in [-1.5, 1.5] equally often, at any N
            resid = ri(-200, 200, R, N).to(BF16)
            if dtype != "bf16":
                self.sx, self.sw = _pow2(g, M, -1, 1), _pow2(g, N, -2, 0)
        else:
            if dtype == "bf16":
                x, w = rn(M, K).to(BF16), (rn(N, K) / math.sqrt(K)).to(BF16)
            elif dtype == "e4m3":
                x, w = rn(M, K).to(E4M3), rn(N, K).to(E4M3)
                self.sx, self.sw = 0.5 + torch.rand(M, generator=g), (0.5 + torch.rand(N, generator=g)) / math.sqrt(K)
            else:
                x, w = (40 * rn(M, K)).round().clamp(-127, 127).to(I8), (40 * rn(N, K)).round().clamp(-127, 127).to(I8)
                self.sx, self.sw = (0.5 + torch.rand(M, generator=g)) / 40, (0.5 + torch.rand(N, generator=g)) / (40 * math.sqrt(K))
            gate, resid = rn(N).to(BF16), rn(R, N).to(BF16)
        mv = lambda t: None if t is None else t.to(device)
        self.x, self.w, self.gate, self.resid, self.sx, self.sw = mv(x), mv(w), mv(gate), mv(resid), mv(self.sx), mv(self.sw)
        x64, w64 = self.x.to(F32).to(F64), self.w.to(F32).to(F64)
        self.acc = x64 @ w64.T
        self.absacc = x64.abs() @ w64.abs().T if family == "R" else None
        if self.sx is not None:
            s = self.sx.to(F64)[:, None] * self.sw.to(F64)[None, :]
            self.acc = self.acc * s
            self.absacc = None if self.absacc is None else self.absacc * s
        if family == "R":
            self.bias, self.bias_range = rn(N).to(BF16).to(device), None
        else:  # widen the bias range from [-64, 64] by doubling until the roundings of acc + bias are exercised (short K: |acc| < 256 is exact in
            # bf16), with a factor of two over MIN_INEXACT in hand; assert_exercises_roundings() then asserts the condition itself
            b = 64
            while True:
                self.bias = ri(-b, b, N).to(BF16).to(device)
                t = self.t(True)
                if float((round_bf16(t) != t).double().mean()) >= 2 * MIN_INEXACT or b >= 16384:
                    break
                b *= 2
            self.bias_range = b

    @property
    def name(self):
        return f"{self.family} {self.dtype} {self.M}x{self.N}x{self.K}"

    def t(self, use_bias=True):
        return self.acc + self.bias.to(F64)[None, :] if use_bias else self.acc

    def S(self, use_bias=True):
        return self.absacc + self.bias.to(F64).abs()[None, :] if use_bias else self.absacc

    def resid_rows(self, period=0):
        """resid [M, N] in float64: row r is resid[r mod period]."""
        r = self.resid.to(F64)
        if period:
            r = r[torch.arange(self.M, device=r.device) % period]
        assert r.shape[0] == self.M
        return r

    def assert_exercises_roundings(self):
        """Family I's premises: |t| < 2^24 and t (and the scaled product under it) an fp32 number, >= 5 % of acc + bias and of bf16(acc + bias) * gate
        inexact before their rounding.  Returns the two fractions."""
        assert self.family == "I"
        t = self.t(True)
        assert float(t.abs().max()) < 2.0 ** 24 and float(self.acc.abs().max()) < 2.0 ** 24, f"{self.name}: |t| reaches 2^24"
        assert torch.equal(t.to(F32).to(F64), t) and torch.equal(self.acc.to(F32).to(F64), self.acc), f"{self.name}: t is not an fp32 number"
        y = round_bf16(t)
        p = y * self.gate.to(F64)[None, :]
        ft, fp = float((y != t).double().mean()), float((round_bf16(p) != p).double().mean())
        assert ft >= MIN_INEXACT and fp >= MIN_INEXACT, f"{self.name}: only {ft:.1%} of acc + bias and {fp:.1%} of the gated products are inexact (bias range {self.bias_range})"
        return ft, fp


class Expect:
    """Reference side of one (inputs, epilogue, bias?, gate?, resid period): f = the unrounded float64 result (family R, with tol) and
    exact = the float64 chain rounded to bf16 at the contract's rounding points (family I; NONE and RESIDUAL)."""

    def __init__(self, inp, epi, use_bias=True, use_gate=True, period=0):
        self.inp, self.epi, self.use_bias, self.use_gate, self.period = inp, epi, use_bias, use_gate, period
        t = inp.t(use_bias)
        gate = inp.gate.to(F64)[None, :] if use_gate else None
        self.f = self.tol = self.exact = None
        if inp.family == "I":
            y = round_bf16(t)
            if epi == EPI_RESIDUAL:
                y = round_bf16(inp.resid_rows(period) + (y if gate is None else round_bf16(y * gate)))
            elif epi != EPI_NONE:
                y = round_bf16(ACT64[epi][0](y))  # not an exact chain (the activation is irrational): never compared bit for bit
            self.exact = y.to(F32).to(BF16)
            return
        e0 = H * t.abs() + (1 + H) * (inp.K + (1 if inp.dtype == "bf16" else 3)) * UNIT * inp.S(use_bias)
        if epi == EPI_NONE:
            self.f, self.tol = t, e0
        elif epi == EPI_RESIDUAL:
            p = t if gate is None else t * gate
            e1 = e0 if gate is None else gate.abs() * e0
            if gate is not None:
                e1 = e1 + H * (p.abs() + e1)
            self.f = inp.resid_rows(period) + p
            self.tol = e1 + H * (self.f.abs() + e1)
        else:
            f, L = ACT64[epi]
            self.f = f(t)
            tol = L * e0 + ACT_EVAL * self.f.abs()
            self.tol = tol + H * (self.f.abs() + tol)

    @property
    def what(self):
        e = EPI_NAMES[self.epi]
        if self.epi == EPI_RESIDUAL:
            e += ("+gate" if self.use_gate else "") + (f" period={self.period}" if self.period else "")
        return e + ("" if self.use_bias else " no-bias")


# ------------------------------------------------------------------------------------------------------------------- acceptance
class Reject(AssertionError):
    def __init__(self, criterion, msg):
        super().__init__(msg)
        self.criterion = criterion


class Case:
    """The checks of one test: (shape, body, epilogue, rule, largest d/tol or number of unequal elements, elements compared)."""

    def __init__(self, name, record=True, prefix="gemm_fp64"):
        self.name, self.record, self.rows, self.prefix = name, record, [], prefix

    def _row(self, exp, body, rule, worst, n):
        self.rows.append((exp.inp.name, body, exp.what, rule, worst, n))
        if self.record:
            from tests.util import record as rec

            rec(f"{self.prefix} {self.name} {exp.inp.name} {body} {exp.what}", rule=rule, worst=worst, elements=n)

    def check(self, got, exp, body=""):
        return self.check_exact(got, exp, body) if exp.inp.family == "I" else self.check_bound(got, exp, body)

    def check_exact(self, got, exp, body=""):
        """Family I: got (bf16 [M, N]) equals the float64 chain bit for bit."""
        assert exp.epi in (EPI_NONE, EPI_RESIDUAL) and exp.exact is not None
        tag = f"{self.name} {exp.inp.name} {body} {exp.what}"
        if got.shape != exp.exact.shape or got.dtype != BF16:
            raise Reject("shape", f"{tag}: {tuple(got.shape)} {got.dtype} vs {tuple(exp.exact.shape)}")
        ne = got.view(torch.int16) != exp.exact.to(got.device).view(torch.int16)
        bad = int(ne.sum())
        self._row(exp, body, "exact", float(bad), got.numel())
        if bad:
            i = int(ne.reshape(-1).double().argmax())
            m, n = divmod(i, got.shape[1])
            rows, cols = ne.any(1).nonzero().flatten(), ne.any(0).nonzero().flatten()
            raise Reject("exact", f"{tag}: {bad} of {got.numel()} elements differ from the float64 chain; first at ({m}, {n}): got {float(got[m, n])} want {float(exp.exact[m, n])}; "
                                  f"rows {int(rows[0])}..{int(rows[-1])} ({rows.numel()}), columns {int(cols[0])}..{int(cols[-1])} ({cols.numel()})")
        return 0.0

    def check_bound(self, got, exp, body=""):
        """Family R: |got - f| <= tol on every element."""
        tag = f"{self.name} {exp.inp.name} {body} {exp.what}"
        g = got.to(exp.f.device).to(F32).to(F64)
        if g.shape != exp.f.shape:
            raise Reject("shape", f"{tag}: {tuple(g.shape)} vs {tuple(exp.f.shape)}")
        if not bool(torch.isfinite(g).all()):
            raise Reject("finite", f"{tag}: non-finite output")
        err = (g - exp.f).abs()
        ratio = torch.where(exp.tol > 0, err / exp.tol.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
        worst = float(ratio.max())
        self._row(exp, body, "bound", worst, g.numel())
        if worst > 1.0:
            i = int(ratio.reshape(-1).argmax())
            m, n = divmod(i, g.shape[1])
            over = ratio > 1.0
            raise Reject("bound", f"{tag}: {int(over.sum())} of {g.numel()} elements ({float(over.double().mean()):.2%}) outside the bound; worst d/tol {worst:.3f} at ({m}, {n}): "
                                  f"got {float(g[m, n]):.9g} ref {float(exp.f[m, n]):.9g} tol {float(exp.tol[m, n]):.3g}")
        return worst

    @property
    def worst_ratio(self):
        return max((r[4] for r in self.rows if r[3] == "bound"), default=0.0)

    def table(self):
        return [f"{self.name:<24} {shape:<24} {body:<34} {what:<18} {rule:<5} " + (f"d/tol {worst:5.3f}" if rule == "bound" else f"unequal {int(worst)}") + f"  n={n}"
                for shape, body, what, rule, worst, n in self.rows]

    def header(self):
        nb, ne = sum(r[3] == "bound" for r in self.rows), sum(r[3] == "exact" for r in self.rows)
        return f"# {self.name}: {len(self.rows)} checks ({ne} bit for bit, {nb} bounded)" + (f", largest d/tol = {self.worst_ratio:.3f}" if nb else "")


# ------------------------------------------------------------------------------------------------------------------- emulations
R_MUTATIONS = {"drop_k": EPI_NONE, "swap_w_cols": EPI_NONE, "bias_shift": EPI_NONE, "acc_bf16": EPI_NONE, "truncate": EPI_NONE, "gate_shift": EPI_RESIDUAL,
               "resid_row": EPI_RESIDUAL}  # mutation -> the epilogue whose family-R check must reject it
I_MUTATIONS = {"no_mid_rounding": EPI_RESIDUAL, "half_up": EPI_NONE, "k_tile_twice": EPI_NONE, "quadrant_low": EPI_NONE}


def _r32(v, mode="rne"):
    """fp32 -> bf16 in one rounding, kept as fp32."""
    return round_bf16(v.to(F64), mode).to(F32)


def emulate(inp, epi, use_bias=True, use_gate=True, period=0, chunk=0, mut=None):
    """A correct kernel in fp32 torch on the CPU: fp32 matmul (whole, or accumulated over `chunk`-wide k slices), w8a8's two scale multiplications
    and the bias add in fp32, then the contract's roundings; the activations in the kernels' fp32 form (x / (1 + exp(-2u)), x / (1 + exp(-x))).
    mut: one of R_MUTATIONS / I_MUTATIONS — a subtly WRONG kernel, for the host module's rejection tests.  Returns bf16 [M, N]."""
    x, w = inp.x.to(F32), inp.w.to(F32)
    bias, gate, resid = inp.bias.to(F32), inp.gate.to(F32), inp.resid_rows(period).to(F32)
    if mut == "drop_k":
        x = x.clone()
        x[:, inp.K // 2 + 1] = 0
    elif mut == "swap_w_cols":
        w = w.clone()
        w[:, [3, 70]] = w[:, [70, 3]]
    elif mut == "k_tile_twice":  # tile 1 read in place of tile 0 too
        x, w = x.clone(), w.clone()
        x[:, :64], w[:, :64] = x[:, 64:128], w[:, 64:128]
    elif mut == "bias_shift":
        bias = bias.roll(1)
    elif mut == "gate_shift":
        gate = gate.roll(1)
    elif mut == "resid_row":
        resid = resid.roll(1, 0)
    if chunk:
        acc = torch.zeros(inp.M, inp.N, dtype=F32)
        for k0 in range(0, inp.K, chunk):
            acc = acc + x[:, k0 : k0 + chunk] @ w[:, k0 : k0 + chunk].T
    else:
        acc = x @ w.T
    if inp.sx is not None:
        acc = acc * inp.sx[:, None] * inp.sw[None, :]
    if mut == "acc_bf16":
        acc = _r32(acc)
    return finish(acc + bias if use_bias else acc, epi, gate if use_gate else None, resid, mut)


def finish(t32, epi, gate=None, resid=None, mut=None):
    """The epilogue of a correct kernel from t32 = the fp32 value in front of the first rounding (emulate's, and tests/mx_ref.py's for the MXFP8
    bodies): the contract's roundings around the kernels' fp32 activations.  gate, resid: fp32, or None.  mut as in emulate.  Returns bf16."""
    rnd = "half_up" if mut == "half_up" else "trunc" if mut == "truncate" else "rne"
    use_gate = gate is not None
    y = _r32(t32, rnd)
    if epi == EPI_GELU:
        u = 0.7978845608028654 * (y + 0.044715 * y * y * y)
        y = _r32(y / (1.0 + torch.exp(-2.0 * u)), rnd)
    elif epi == EPI_SILU:
        y = _r32(y / (1.0 + torch.exp(-y)), rnd)
    elif epi == EPI_RESIDUAL:
        if use_gate:
            y = y * gate if mut == "no_mid_rounding" else _r32(y * gate, rnd)
        y = _r32(resid + y, rnd)
    if mut == "quadrant_low":  # the upper left 128x128 quadrant of the first 256x256 tile lands 128 rows too low
        good = y.clone()
        y[128:256, :128] = good[:128, :128]
        y[:128, :128] = 0
    return y.to(BF16)


# ------------------------------------------------------------------------------------------------------------------- the GPU module's lists
VARIANTS = {"bf16": (1, 2, 4, 5), "e4m3": (1, 2, 5), "int8": (1, 5)}
BODY = {("bf16", 1): "gemm 128x128 bf16", ("bf16", 2): "gemm256 ping-pong bf16", ("bf16", 4): "gemm256s one-tile", ("bf16", 5): "gemm256c continuous",
        ("e4m3", 1): "gemm 128x128 e4m3", ("e4m3", 2): "gemm256 ping-pong e4m3", ("e4m3", 5): "gemm256c8 e4m3", ("int8", 1): "gemm 128x128 int8",
        ("int8", 5): "gemm256c8 int8"}
EPILOGUES = ((EPI_NONE, True, False), (EPI_NONE, False, False), (EPI_GELU, True, False), (EPI_SILU, True, False), (EPI_RESIDUAL, True, True),
             (EPI_RESIDUAL, True, False))  # (epilogue, bias?, gate?)
K_TILES = (1, 2, 3, 4, 5, 8, 9)  # prologue and tail of the K loop (variants 1, 2, 4) at M = 300, N = 264
K_TILES_MN = (300, 264)
K_TILES_CONT = (4, 6, 8)  # variant 5 at N = 256; 3 and 5 tiles and N = 264 are refused
M_TAILS = (1, 127, 129, 255, 257)  # every body at N = 256, K = 256 (bf16) / 512 (w8a8)
N_TAILS = (8, 136, 248, 264, 520)  # variants 1, 2, 4 at M = 129
SCHED_MN = (2100, 768)  # 9 x 3 tiles of 256: 27, no multiple of 8
SCHED_GROUPS = (0, 1, 7)
SCHED_128_MN = (1100, 264)  # 9 x 3 tiles of 128 for the 128x128 kernel's own grouping of 8
DEEP = (257, 256, 13824)
BLOCKED_M = 96 * 256 - 219  # x 2 n-tiles = 192 tiles: the fewest the dispatcher gives a 256x256 kernel through the blocked entries (no variant there)
VT_SHAPE = (BLOCKED_M, 512, 512)  # 96 x 2 output tiles, four heads, 8 K tiles: the fewest tiles that x2v_gemm_bf16_vt accepts; M % 64 = 37


def mid_k(dtype):
    return 256 if dtype == "bf16" else 512


def accepts(dtype, variant, N, K):
    """Whether body `variant` takes the shape (x2v.h: the continuous forms need an even number of K tiles >= 4 and N % 256 == 0)."""
    nk = K // KTILE[dtype]
    return variant != 5 or (nk >= 4 and nk % 2 == 0 and N % 256 == 0)


def persistent_ms(cus, ntn):
    """M with cus + 1 and 2 cus + 3 output tiles of 256 x 256 at ntn n-tiles (rounded up to whole rows of tiles), the last m-tile ragged."""
    return [256 * (-(-tiles // ntn)) - 219 for tiles in (cus + 1, 2 * cus + 3)]
