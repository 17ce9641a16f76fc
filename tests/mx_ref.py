"""float64 references, seeded inputs, fp32 emulations and the GPU module's lists for the MXFP8 path: quant_mx_kernel<1>
(lightx2v_amd/csrc/mx.hip) and the MX instantiations of gemm_kernel (gemm.hip, 128x128) and gemm256_kernel (gemm256.hip).  Plain PyTorch on float64; nothing here imports the library or
oracle/.  bf16 rounding, Expect, Case, the epilogue chains and both acceptance rules are tests/gemm_ref.py's.  Shared by tests/test_mx_ref_host.py
(the yardstick checked without a GPU) and tests/test_gpu_mx_fp64.py (the kernels checked against it).

The references restate include/x2v.h:
  quantiser   per 32 consecutive K elements: scale byte = biased exponent of the smallest power of two >= max|x| / 448, the quotient taken in fp32
              WITH denormals, saturating at 254, an all-zero block -> byte 0; element = e4m3fn(x * 2^(127 - byte)), one rounding to nearest-even
              from the exact float64 product, sign of zero kept; scale table [K/128][rows][4]
  GEMM        t = alpha * (deq(a) . deq(b)^T) + bias, deq = e4m3 element * 2^(scale byte - 127) of its row and 32-wide k block, then gemm_ref's
              chain: NONE bf16(t) | GELU_TANH, SILU act(bf16(t)) | RESIDUAL bf16(resid + bf16(bf16(t) * gate)), without a gate bf16(resid + bf16(t))

Family I (bit for bit).  Codes are the integers x in [-8, 8], W in [-4, 4]; the scale byte of (row, block) is base[row] + d[row, block] with d drawn
independently per row and block from 0..spread(K), so every byte of every K-tile dword matters, and base[row] = 127 + g[row], g in [-20, 20] with
both ends present, so a dword taken from another row shows.  In units of the smallest term of an output element, 2^(g_a[m] + g_b[n]), every term is
an integer and sum |terms| < 2^24 (asserted): any accumulation order is exact in fp32, and so is any alignment of addends inside the matrix
instruction that keeps 24 bits.  alpha is 0.5 or 0.75 (alpha * acc an fp32 number, asserted).
  A bias is per column, the scale of a's rows per row: t = alpha acc + bias is an fp32 number for every row only when the rows of a share their
base (2^40 between two rows' units leaves no common 24-bit grid), and an inexact fp32 sum in front of the bf16 rounding would make a correct
kernel differ from the one-rounding chain at ties.  So every shape has two inputs: `flat_a=False` (g_a per row, no bias: the checks without bias)
and `flat_a=True` (one g_a for all rows, g_b still per row of W, bias[n] an integer times 2^(g_a + g_b[n]) widened by gemm_ref's rule until
>= 5 % of t is inexact before its rounding: the checks with bias).  resid[m, n] is an integer in [-200, 200] times 2^(g_a[m] + g_b[n] + c), c from
the median |acc|, so that resid + p is an fp32 number too (asserted) and the last rounding is exercised.

Family R (bound on every element).  x ~ N(0, 1) and W ~ N(0, 1) / sqrt(K) in bf16, x multiplied and W divided by the per-block ramp
logspace(-3, 3, K / 32), both quantised by quant() below; Expect's bound with the w8a8 term (K + 3) 2^-23 S, S = |deq a| . |deq b|^T |alpha| + |bias|."""
import copy
import math

import torch

from tests import gemm_ref as G
from tests.gemm_ref import BF16, EPI_GELU, EPI_NONE, EPI_RESIDUAL, EPI_SILU, F32, F64, MIN_INEXACT, round_bf16

I64, U8 = torch.int64, torch.uint8
BLOCK, KTILE = 32, 128


# ------------------------------------------------------------------------------------------------------------------- float64 pieces
def pow2(n):
    """2^n as float64 from its bits (n an int64 tensor in [-1022, 1023]): exact on any device."""
    return ((n.to(I64) + 1023) << 52).view(F64)


def floor_log2(a):
    """floor(log2 a) of positive normal float64 numbers (every finite bf16 number but 0 is one); -1023 at 0."""
    return ((a.view(I64) >> 52) & 0x7FF) - 1023


def round_fp32(q):
    """Non-negative float64 -> the nearest fp32 number, ties to even, denormals kept (steps of 2^-149 below 2^-126), as float64."""
    e = floor_log2(q).clamp(-126, 127)
    return torch.round(q * pow2(23 - e)) * pow2(e - 23)


def e8m0_byte(amax, mode="ceil"):
    """Block maxima (float64, finite, >= 0) -> scale bytes (int64).  mode 'floor' = the wrong rounding of the host module's mutation."""
    sf = round_fp32(amax / 448.0)  # amax has 8 significant bits: the float64 quotient rounds to fp32 as the exact one does (m / 7 is periodic)
    e = floor_log2(sf)
    up = (sf != pow2(e.clamp_min(-1022))) & (sf > 0) if mode == "ceil" else torch.zeros_like(sf, dtype=torch.bool)
    return torch.where(sf > 0, (e + up.to(I64) + 127).clamp(0, 254), torch.zeros_like(e))


def e4m3_codes(v, rnd="rne", neg_zero=True):
    """float64 -> e4m3fn code bytes (uint8): 4 significant bits, least exponent -6 (steps of 2^-9 below 2^-6), one rounding, saturating at 448
    (0x7E).  rnd 'trunc' and neg_zero=False ('-0 -> +0') are the host module's mutations."""
    a = v.abs()
    e = floor_log2(a).clamp(-6, 8)
    r = a * pow2(3 - e)  # exact; [8, 16) in the normal range, [0, 8) below 2^-6
    r = (torch.round(r) if rnd == "rne" else torch.trunc(r)).to(I64)
    code = (((e + 7) << 3) + r - 8).clamp(0, 0x7E)  # r = 16 carries into the exponent field by itself
    sign = torch.signbit(v) if neg_zero else torch.signbit(v) & (code != 0)
    return (code + (sign.to(I64) << 7)).to(U8)


def e4m3_values(code):
    """e4m3fn code bytes -> float64."""
    c = code.to(I64)
    e, m = (c >> 3) & 15, c & 7
    mag = torch.where(e == 0, m.to(F64) * 2.0 ** -9, (8 + m).to(F64) * pow2(e - 10))
    return torch.where((c >> 7) == 1, -mag, mag)


def quant(x, e8m0="ceil", rnd="rne", neg_zero=True, rows_per_step=1024):
    """x bf16 [M, K] (finite) -> (e4m3 code bytes uint8 [M, K], scale bytes uint8 [M, K / 32]), row-major."""
    M, K = x.shape
    assert K % BLOCK == 0 and x.dtype == BF16
    q, sc = torch.empty(M, K, dtype=U8, device=x.device), torch.empty(M, K // BLOCK, dtype=U8, device=x.device)
    for r0 in range(0, M, rows_per_step):
        xb = x[r0 : r0 + rows_per_step].to(F32).to(F64).reshape(-1, K // BLOCK, BLOCK)
        byte = e8m0_byte(xb.abs().amax(-1), e8m0)
        q[r0 : r0 + rows_per_step] = e4m3_codes(xb * pow2(127 - byte).unsqueeze(-1), rnd, neg_zero).reshape(-1, K)
        sc[r0 : r0 + rows_per_step] = byte.to(U8)
    return q, sc


def tiled(sc):
    """Scale bytes [rows, K / 32] -> the kernels' table [K / 128][rows][4]."""
    rows, kb = sc.shape
    return sc.reshape(rows, kb // 4, 4).permute(1, 0, 2).contiguous()


def rowmajor(table):
    """[K / 128][rows][4] -> [rows, K / 32]."""
    return table.permute(1, 0, 2).reshape(table.shape[1], -1)


def dequant(code, sc):
    """Code bytes [rows, K] and scale bytes [rows, K / 32] -> float64 [rows, K] (exact)."""
    rows, K = code.shape
    return (e4m3_values(code).reshape(rows, K // BLOCK, BLOCK) * pow2(sc.to(I64) - 127).unsqueeze(-1)).reshape(rows, K)


def is_fp32(t):
    return bool(torch.equal(t.to(F32).to(F64), t))


# ------------------------------------------------------------------------------------------------------------------- inputs
def spread(K):
    """Largest d of family I at this K: sum |terms| / smallest term stays below 2^24 (measured 0.69 of it at K = 128 with 7, 0.58 at K = 1152 with
    6, 0.13 at K = 13824 with 3, at 257 x 264; Inputs lowers it by one where a shape with more elements reaches 0.9 of 2^24, and
    Inputs.assert_premises() asserts the bound for every input)."""
    return 7 if K <= 128 else 6 if K <= 1152 else 3


class Inputs:
    """One seeded MXFP8 case with gemm_ref.Inputs' interface towards Expect (acc, absacc, bias, gate, resid, t, S, resid_rows, name): a, b code bytes
    [M, K], [N, K]; sa, sb scale bytes [M, K / 32], [N, K / 32] (row-major: tiled() gives the kernels' table); alpha; bias, gate [N] and resid [M, N]
    bf16.  acc = deq(a) . deq(b)^T in float64 on `device`.  scaled(use_alpha) is the view that Expect takes."""

    dtype = "mxfp8"  # Expect: the w8a8 term K + 3
    sx = sw = None

    def __init__(self, family, M, N, K, seed=0, flat_a=False, device="cpu"):
        assert family in ("I", "R") and K % KTILE == 0 and not (flat_a and family == "R")
        self.family, self.M, self.N, self.K, self.seed, self.flat_a, self.device = family, M, N, K, seed, flat_a, device
        g = G._gen(77, "IR".index(family), M, N, K, seed, int(flat_a))
        ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g)
        rn = lambda *shape: torch.randn(*shape, generator=g)
        KB = K // BLOCK
        self.alpha = (0.5, 0.75)[int(ri(0, 1, 1))]
        self.alpha_used, self.bias_range, self.units = None, None, None
        if family == "I":
            self.spread = spread(K)
            a, b = e4m3_codes(ri(-8, 8, M, K).to(F64)), e4m3_codes(ri(-4, 4, N, K).to(F64))
            ga, gb = ri(-20, 20, M), ri(-20, 20, N)
            for gr in (ga, gb):  # both ends of the range on some row
                ends = torch.randperm(gr.numel(), generator=g)[:2]
                gr[ends] = torch.tensor([-20, 20])[: ends.numel()]
            if flat_a:
                ga = ga[:1].expand(M).clone()
            rel = lambda code, d: e4m3_values(code).abs().reshape(code.shape[0], KB, BLOCK).mul(pow2(d).unsqueeze(-1)).reshape(code.shape[0], K).to(device)
            while True:  # sum |terms| in units of the element's smallest term (the codes times 2^d: small integers, exact in float64); its largest
                # value grows with M N, so a shape with many elements may need one step less than spread(K)
                da, db = ri(0, self.spread, M, KB), ri(0, self.spread, N, KB)
                self.sum_terms = float((rel(a, da) @ rel(b, db).T).max())
                if self.sum_terms < 0.9 * 2.0 ** 24:
                    break
                self.spread -= 1
            sa, sb = (127 + ga[:, None] + da).to(U8), (127 + gb[:, None] + db).to(U8)
            self.ga, self.gb = ga, gb
            unit_exp = ga[:, None] + gb[None, :]  # log2 of the smallest term of element (m, n)
            gate = (0.5 * ((torch.arange(N) % 7) - 3)[torch.randperm(N, generator=g)]).to(BF16)
            rint, bint = ri(-200, 200, M, N), [ri(-b, b, N) for b in (64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384)]
        else:
            ramp = torch.logspace(-3, 3, KB).repeat_interleave(BLOCK)
            x = (rn(M, K).to(BF16).to(F32) * ramp).to(BF16)
            w = ((rn(N, K) / math.sqrt(K)).to(BF16).to(F32) / ramp).to(BF16)
            (a, sa), (b, sb) = quant(x), quant(w)
            gate, resid, bias = rn(N).to(BF16), rn(M, N).to(BF16), rn(N).to(BF16)
        self.a, self.b, self.sa, self.sb = a.to(device), b.to(device), sa.to(device), sb.to(device)
        a64, b64 = dequant(self.a, self.sa), dequant(self.b, self.sb)
        self.acc = self.acc0 = a64 @ b64.T
        self.absacc = self.absacc0 = None
        if family == "R":
            self.absacc = self.absacc0 = a64.abs() @ b64.abs().T
            self.gate, self.resid, self.bias = gate.to(device), resid.to(device), bias.to(device)
        else:
            self.units = pow2(unit_exp).to(device)
            c = max(int(round(math.log2(float((self.acc0.abs() / self.units).median()) + 1.0))) - 7, 0)
            self.resid_shift = c
            self.resid = (rint.to(F64).to(device) * self.units * 2.0 ** c).to(F32).to(BF16)
            self.gate = gate.to(device)
            self.bias = None
            if flat_a:  # gemm_ref.Inputs' rule: double the range until the rounding of t is exercised, a factor of two over MIN_INEXACT in hand
                col = pow2(ga[0] + gb).to(device)
                for b_, bi in zip((64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384), bint):
                    self.bias = (bi.to(F32).to(BF16).to(F64).to(device) * col).to(F32).to(BF16)
                    self.bias_range = b_
                    if min(self._inexact(self.scaled(u).t(True)) for u in (False, True)) >= 2 * MIN_INEXACT:
                        break

    @staticmethod
    def _inexact(t):
        return float((round_bf16(t) != t).double().mean())

    @property
    def name(self):
        al = "" if self.alpha_used is None else f" alpha={self.alpha_used:g}"
        return f"{self.family} mxfp8 {self.M}x{self.N}x{self.K}" + (" flat-a" if self.flat_a else "") + al

    def scaled(self, use_alpha):
        """The view with acc = alpha * (deq a . deq b^T) (use_alpha) or the plain product: what Expect, Case and emulate() take."""
        v = copy.copy(self)
        v.alpha_used = self.alpha if use_alpha else None
        v.acc = self.acc0 * self.alpha if use_alpha else self.acc0
        v.absacc = self.absacc0 * self.alpha if use_alpha and self.absacc0 is not None else self.absacc0
        return v

    def t(self, use_bias=True):
        assert not use_bias or self.bias is not None, f"{self.name}: family I has a bias only with flat_a (see the module's docstring)"
        return self.acc + self.bias.to(F64)[None, :] if use_bias else self.acc

    def S(self, use_bias=True):
        return self.absacc + self.bias.to(F64).abs()[None, :] if use_bias else self.absacc

    def resid_rows(self, period=0):
        assert not period
        return self.resid.to(F64)

    def assert_premises(self):
        """Family I's premises, for the plain product and for alpha times it: sum |terms| < 2^24 smallest terms; alpha acc, t and resid + p (with and
        without the gate) fp32 numbers; everything in bf16's normal range; >= 5 % of t and of bf16(t) * gate inexact before their rounding.  Returns
        (sum |terms| / 2^24, least share of t inexact, least share of gated products inexact, least share of resid + p inexact)."""
        assert self.family == "I" and self.alpha_used is None
        assert self.sum_terms < 2.0 ** 24, f"{self.name}: sum |terms| = {self.sum_terms / 2 ** 24:.2f} of 2^24 smallest terms"
        assert int(self.ga.max()) - int(self.ga.min()) == (0 if self.flat_a or self.M == 1 else 40) and int(self.gb.max()) - int(self.gb.min()) == 40
        fts, fps, frs = [], [], []
        for use_alpha in (False, True):
            v = self.scaled(use_alpha)
            assert is_fp32(v.acc), f"{v.name}: alpha * acc is not an fp32 number"
            t = v.t(self.flat_a)
            assert is_fp32(t), f"{v.name}: t is not an fp32 number"
            nz = t[t != 0].abs()
            assert float(nz.min()) >= 2.0 ** -120 and float(nz.max()) < 2.0 ** 120, f"{v.name}: t leaves bf16's normal range"
            y = round_bf16(t)
            p = y * self.gate.to(F64)[None, :]
            r = self.resid.to(F64)
            for s in (r + y, r + round_bf16(p)):
                assert is_fp32(s), f"{v.name}: resid + p is not an fp32 number (resid shift {self.resid_shift})"
                frs.append(self._inexact(s))
            fts.append(self._inexact(t))
            fps.append(self._inexact(p))
        ft, fp, fr = min(fts), min(fps), min(frs)
        assert ft >= MIN_INEXACT and fp >= MIN_INEXACT and fr >= MIN_INEXACT, (f"{self.name}: only {ft:.1%} of t, {fp:.1%} of the gated products and {fr:.1%} of resid + p "
                                                                               f"are inexact (bias range {self.bias_range})")
        return self.sum_terms / 2.0 ** 24, ft, fp, fr


# ------------------------------------------------------------------------------------------------------------------- emulations
GEMM_MUTATIONS = {"scale_bytes_swapped": EPI_NONE, "scale_dword_late": EPI_NONE, "drop_last_tile": EPI_NONE, "k_tile_twice": EPI_NONE, "alpha_after_bias": EPI_NONE,
                  "bias_after_rounding": EPI_NONE, "half_up": EPI_NONE, "truncate": EPI_NONE, "no_mid_rounding": EPI_RESIDUAL,
                  "rowmajor_table_read_as_tiled": EPI_NONE}  # mutation -> the epilogue whose check must reject it
QUANT_MUTATIONS = {"e8m0_floor": dict(e8m0="floor"), "e4m3_trunc": dict(rnd="trunc"), "neg_zero_to_zero": dict(neg_zero=False)}


def trunc_fp32(v):
    """float64 -> fp32 by dropping the low 29 bits of the significand (a matrix unit that truncates when it aligns addends)."""
    return (v.view(I64) & ~((1 << 29) - 1)).view(F64).to(F32)


def emulate(v, epi, use_bias=True, use_gate=True, truncating=False, mut=None):
    """A correct kernel in fp32 torch on the CPU, from the view v = Inputs.scaled(...): per 32-wide k block an fp32 dot product times the two block
    scales, the blocks accumulated in K order in fp32 (truncating=True: every addition truncated to fp32 instead of rounded), alpha and bias in
    fp32, then gemm_ref.finish.  mut: one of GEMM_MUTATIONS — a subtly WRONG kernel.  Returns bf16 [M, N]."""
    A, B = e4m3_values(v.a.cpu()).to(F32), e4m3_values(v.b.cpu()).to(F32)
    sa, sb = v.sa.cpu().to(I64), v.sb.cpu().to(I64)
    KB, NT = v.K // BLOCK, v.K // KTILE
    if mut == "scale_bytes_swapped":  # blocks 0 and 1 of every K-tile dword of a
        sa = sa.reshape(v.M, NT, 4)[:, :, [1, 0, 2, 3]].reshape(v.M, KB)
    elif mut == "scale_dword_late":  # K-tile t + 1 of a runs with the dword of K-tile t
        sa = torch.cat([sa[:, :4], sa[:, :-4]], 1)
    elif mut == "rowmajor_table_read_as_tiled":  # a's table written [rows][K / 32], read as [K / 128][rows][4]
        sa = rowmajor(sa.contiguous().reshape(NT, v.M, 4))
    blocks = list(range(KB))
    if mut == "drop_last_tile":
        blocks = blocks[:-4]
    elif mut == "k_tile_twice":
        blocks = blocks + blocks[-4:]
    acc = torch.zeros(v.M, v.N, dtype=F32)
    for kb in blocks:
        k = slice(kb * BLOCK, (kb + 1) * BLOCK)
        term = (A[:, k] @ B[:, k].T) * (pow2(sa[:, kb] - 127).to(F32)[:, None] * pow2(sb[:, kb] - 127).to(F32)[None, :])
        acc = trunc_fp32(acc.to(F64) + term.to(F64)) if truncating else acc + term
    alpha = 1.0 if v.alpha_used is None else v.alpha_used
    bias = v.bias.cpu().to(F32)[None, :] if use_bias else torch.zeros(1, v.N)
    if mut == "alpha_after_bias":
        t32 = (acc + bias) * alpha
    elif mut == "bias_after_rounding":
        t32 = G._r32(acc * alpha) + bias
    else:
        t32 = acc * alpha + bias
    return G.finish(t32, epi, v.gate.cpu().to(F32) if use_gate else None, v.resid.cpu().to(F32), mut)


# ------------------------------------------------------------------------------------------------------------------- quantiser inputs
def bf16_bits(bits):
    """int32 bit patterns 0 .. 0xFFFF -> bf16."""
    return bits.to(torch.int16).view(BF16)


def _pin(v):
    t = torch.tensor([v], dtype=F64).to(F32).to(BF16)
    assert float(t) == v, f"{v} is no bf16 number"
    return int(t.view(torch.int16)) & 0x7FFF


PINS = {f"{m}*2^{k}": _pin(m * 2.0 ** k) for k in (0, -60, 60) for m in (446, 448, 450)}  # at, one bf16 step below and one above 448 * 2^k
PINS.update({"1.75*2^-119 - 1 step": _pin(1.75 * 2.0 ** -119) - 1, "1.75*2^-119": _pin(1.75 * 2.0 ** -119), "1.75*2^-119 + 1 step": _pin(1.75 * 2.0 ** -119) + 1,
             "2^-126": _pin(2.0 ** -126), "least subnormal": 1, "largest finite": 0x7F7F})  # max / 448 = 2^-127: the ex == 0 branch of e8m0_ceil


def sweep(pin_bits):
    """bf16 [rows, 128]: slot 0 of every 32-wide block holds the pin (the block maximum), the other 31 slots run through every finite bf16 bit pattern
    with |v| <= the pin, both signs and both zeros; what is left of the last row is +0."""
    mags = torch.arange(0, pin_bits + 1, dtype=torch.int32)
    pats = torch.cat([mags, mags | 0x8000])
    nblk = -(-pats.numel() // 31)
    rows = -(-nblk // 4)
    body = torch.zeros(rows * 4 * 31, dtype=torch.int32)
    body[: pats.numel()] = pats
    bits = torch.cat([torch.full((rows * 4, 1), pin_bits, dtype=torch.int32), body.reshape(rows * 4, 31)], 1).reshape(rows, 128)
    return bf16_bits(bits), pats.numel()


def quant_input(M, K, seed=0):
    """bf16 [M, K] for the layout cases: N(0, 1) times a per-row factor from 1e-4 to 1e4, an all-zero block next to non-zero ones, one block of
    -0, one at 448 exactly."""
    g = G._gen(78, M, K, seed)
    x = (torch.randn(M, K, generator=g) * torch.logspace(-4, 4, M).unsqueeze(1)).to(BF16)
    x[M // 2, 32:64] = 0
    x[M - 1, K - 32 :] = -0.0
    x[0, :32] = 448.0
    return x


# ------------------------------------------------------------------------------------------------------------------- the GPU module's lists
BODY = {1: "gemm_mxfp8 128x128", 2: "gemm256 MX ping-pong"}
K_TILES = (1, 2, 3, 4, 5, 9)  # 128x128: ring parity and the tail without prefetch; 256x256: 1 tile = total < LEAD, 2 = exactly one ring
K_TILES_MN = (257, 264)  # ragged in both directions for either tile size
M_TAILS = (1, 127, 128, 129, 255, 256, 257)  # at N = 136, K = 256
N_TAILS = (8, 120, 128, 136, 248, 256, 264)  # at M = 129, K = 256
TAIL_K = 256
SCHED = ((1100, 264, 128), (1061, 264, 256))  # 9 x 3 tiles of 128 at one K tile (groups of 8: a last group of 1); 5 x 2 tiles of 256 (groups of 4)
DEEP = ((136, 136, 13824), (264, 264, 13824))
EPI_SHAPES = ((257, 264, 384), (255, 248, 256), (1, 8, 128))
EPILOGUES = ((EPI_NONE, False), (EPI_GELU, False), (EPI_SILU, False), (EPI_RESIDUAL, True), (EPI_RESIDUAL, False))  # (epilogue, gate?)
AUTO = ((3073, 4096, 1024), (3073, 4096, 896))  # 13 x 16 = 208 tiles of 256: 8 K tiles -> the 256x256 body, 7 -> the 128x128 body
QUANT_LAYOUT = tuple((M, K) for K in (128, 256, 1152) for M in (1, 3, 5, 257))
QUANT_GRID = ((2050, 8192), (5131, 8192))  # M K / 8 = 2_099_200 and 5_254_144 chunks: past the 8192 x 256 threads of the capped grid


def family_i_shapes():
    """Every (M, N, K) at which the GPU module runs family I."""
    s = [(K_TILES_MN[0], K_TILES_MN[1], nk * KTILE) for nk in K_TILES] + [(M, 136, TAIL_K) for M in M_TAILS] + [(129, N, TAIL_K) for N in N_TAILS]
    return list(dict.fromkeys(s + list(SCHED) + list(DEEP) + list(EPI_SHAPES) + list(AUTO)))


def auto_body(M, N, K):
    """The body variant 0 takes without an epilogue (mx.hip mx_body; operand row strides far below 2^24)."""
    return 2 if -(-M // 256) * -(-N // 256) >= 192 and K // 128 >= 8 else 1
