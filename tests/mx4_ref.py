"""float64 references, seeded inputs and fp32 emulations for the MXFP4 x MXFP4 path: quant_mx_kernel<3> (lightx2v_amd/csrc/mx.hip) and the MXM = 3
instantiations of gemm_kernel (gemm.hip, 128x128) and gemm256_kernel (gemm256.hip, 256x256 ping-pong) — OCP e2m1 elements on both sides.  Plain PyTorch
on float64; nothing here imports the library or oracle/.  The scale rule, the table layout, family I / R, Expect, Case, the epilogue chains and both
acceptance rules are tests/mx_ref.py's and tests/gemm_ref.py's; this module adds the 4-bit element, its packing and the inputs whose a and b are e2m1.
Shared by tests/test_mx4_ref_host.py (the yardstick checked without a GPU) and tests/test_gpu_mx4.py (the kernels checked against it).

The references restate include/x2v.h:
  e2m1        code = s << 3 | e << 1 | m: 1 sign, 2 exponent bits (bias 1), 1 mantissa bit; e = 0: m * 0.5, else (2 + m) * 2^(e - 2); magnitudes
              0, 0.5, 1, 1.5, 2, 3, 4, 6; no NaN / Inf
  packing     the dense little-endian nibble string: code j of a row at bits 4 j .. 4 j + 3 of the row's bytes (2 codes = 1 byte, the even one low)
  quantiser   mx_ref's with 6 in place of 448: scale byte = biased exponent of the smallest power of two >= max|x| / 6 (fp32 quotient with
              denormals, saturating at 254, all-zero block -> 0); code = e2m1(x * 2^(127 - byte)), one rounding to nearest-even (ties at 0.25, 1.25,
              2.5 and 5 go down, at 0.75, 1.75 and 3.5 up), saturating at +/-6, sign of zero kept
  GEMM        mx_ref's chain with deq = e2m1 value * 2^(scale byte - 127) on both sides; K % 256 == 0

Family I: mx_ref's, with the codes of a mapped onto the e2m1 integers {0, +-1, +-2, +-3, +-4, +-6} (5 -> 4; 7, 8 -> 6) in front of everything the
parent derives from them — the spread loop, acc, the units, resid and the bias rule run on the mapped codes — and W's integers in [-4, 4], which are
e2m1 numbers already.  Family R quantises the parent's ramped x and W with quant4."""
import copy

import torch

from tests import gemm_ref as G
from tests import mx6_ref as R6
from tests import mx_ref as X
from tests.gemm_ref import BF16, F32, F64
from tests.mx_ref import BLOCK, I64, U8, floor_log2, pow2

DIVISOR = 6.0  # the largest e2m1 number
KTILE4 = 256  # k per 128-byte operand row: one K-tile of the kernels in this mode (two dwords of the scale table)


# ------------------------------------------------------------------------------------------------------------------- float64 pieces
def e8m0_byte(amax, mode="ceil", divisor=DIVISOR):
    """Block maxima (float64, finite, >= 0) -> scale bytes (int64): mx6_ref.e8m0_byte with the divisor 6 (= 3 * 2: the float64 quotient of an 8-bit
    significand by 3 is periodic, so it rounds to fp32 as the exact one does — tests/test_mx4_ref_host.py asserts it for every finite bf16 number).
    Divisors 28 and 448 and mode 'floor' are the host module's mutations."""
    return R6.e8m0_byte(amax, mode, divisor)


def e2m1_codes(v, rnd="rne", neg_zero=True):
    """float64 -> e2m1 codes (uint8, 0..15): 2 significant bits, least exponent 0 (steps of 0.5 below 1), one rounding, saturating at 6 (0x7).
    rnd 'trunc' and neg_zero=False ('-0 -> +0') are the host module's mutations."""
    a = v.abs()
    e = floor_log2(a).clamp(0, 2)
    r = a * pow2(1 - e)  # exact; [2, 4) in the normal range, [0, 2) below 1
    r = (torch.round(r) if rnd == "rne" else torch.trunc(r)).to(I64)
    code = (((e + 1) << 1) + r - 2).clamp(0, 7)  # r = 4 carries into the exponent field by itself
    sign = torch.signbit(v) if neg_zero else torch.signbit(v) & (code != 0)
    return (code + (sign.to(I64) << 3)).to(U8)


def e2m1_values(code):
    """e2m1 codes -> float64."""
    c = code.to(I64)
    e, m = (c >> 1) & 3, c & 1
    mag = torch.where(e == 0, m.to(F64) * 0.5, (2 + m).to(F64) * pow2(e - 2))
    return torch.where(((c >> 3) & 1) == 1, -mag, mag)


def pack4(codes, order="low_first"):
    """Codes uint8 [rows, K] (0..15) -> bytes uint8 [rows, K / 2]: code j of a row at bits 4 j .. 4 j + 3.  order 'high_first' (the even code in the
    high nibble) is the host module's mutation."""
    rows, K = codes.shape
    assert K % 2 == 0 and int(codes.max()) < 16
    c = codes.to(I64).reshape(rows, K // 2, 2)
    lo, hi = (c[..., 0], c[..., 1]) if order == "low_first" else (c[..., 1], c[..., 0])
    return (lo | (hi << 4)).to(U8)


def unpack4(packed):
    """Bytes uint8 [rows, K / 2] -> codes uint8 [rows, K]."""
    b = packed.to(I64)
    return torch.stack([b & 15, b >> 4], -1).to(U8).reshape(packed.shape[0], -1)


def quant4(x, e8m0="ceil", rnd="rne", neg_zero=True, divisor=DIVISOR, rows_per_step=1024):
    """x bf16 [M, K] (finite) -> (e2m1 codes uint8 [M, K], UNPACKED, scale bytes uint8 [M, K / 32]), row-major; pack4 gives the kernel's bytes."""
    M, K = x.shape
    assert K % BLOCK == 0 and x.dtype == BF16
    q, sc = torch.empty(M, K, dtype=U8, device=x.device), torch.empty(M, K // BLOCK, dtype=U8, device=x.device)
    for r0 in range(0, M, rows_per_step):
        xb = x[r0 : r0 + rows_per_step].to(F32).to(F64).reshape(-1, K // BLOCK, BLOCK)
        byte = e8m0_byte(xb.abs().amax(-1), e8m0, divisor)
        q[r0 : r0 + rows_per_step] = e2m1_codes(xb * pow2(127 - byte).unsqueeze(-1), rnd, neg_zero).reshape(-1, K)
        sc[r0 : r0 + rows_per_step] = byte.to(U8)
    return q, sc


def dequant4(code, sc):
    """e2m1 codes [rows, K] (unpacked) and scale bytes [rows, K / 32] -> float64 [rows, K] (exact)."""
    rows, K = code.shape
    return (e2m1_values(code).reshape(rows, K // BLOCK, BLOCK) * pow2(sc.to(I64) - 127).unsqueeze(-1)).reshape(rows, K)


# ------------------------------------------------------------------------------------------------------------------- inputs
def _onto_e2m1(v):
    """Integers in [-8, 8] -> the e2m1 integers of no larger magnitude: 5 -> 4; 7, 8 -> 6."""
    a = v.abs()
    return torch.sign(v) * torch.where(a == 5, torch.full_like(a, 4), torch.where(a >= 7, torch.full_like(a, 6), a))


class Inputs(X.Inputs):
    """mx_ref.Inputs whose a and b are e2m1: `a`, `b` the unpacked codes [rows, K] (0..15), `a_packed`, `b_packed` the kernels' bytes [rows, K / 2].
    Family I: the parent's constructor runs with a's integers mapped onto {0, +-1, +-2, +-3, +-4, +-6} where it turns them into codes, so the scale
    bytes, ga / gb, the spread loop (sum |terms| < 0.9 * 2^24), alpha, the flat_a bias rule, resid and assert_premises are the parent's own, on these
    values.  Family R: quant4 of the parent's ramped x and W, drawn again from the parent's seed; acc and absacc recomputed."""

    dtype = "mxfp8"  # Expect: the w8a8 term K + 3 (fp32 accumulation of exact products, as MXFP8)

    def __init__(self, family, M, N, K, seed=0, flat_a=False, device="cpu"):
        assert K % KTILE4 == 0
        if family == "I":
            calls, codes = [], X.e4m3_codes

            def mapped(v, *args, **kw):  # the parent's two conversions of family I: a first, then b
                calls.append(1)
                return codes(_onto_e2m1(v) if len(calls) == 1 else v, *args, **kw)

            X.e4m3_codes = mapped
            try:
                super().__init__(family, M, N, K, seed, flat_a, device)
            finally:
                X.e4m3_codes = codes
            assert len(calls) == 2
            va, vb = X.e4m3_values(self.a), X.e4m3_values(self.b)
            assert set(va.abs().unique().tolist()) <= {0.0, 1.0, 2.0, 3.0, 4.0, 6.0} and float(vb.abs().max()) <= 4 and bool((vb == vb.round()).all())
            self.a, self.b = e2m1_codes(va), e2m1_codes(vb)
            assert torch.equal(e2m1_values(self.a), va) and torch.equal(e2m1_values(self.b), vb)
        else:
            super().__init__(family, M, N, K, seed, flat_a, device)
            g = G._gen(77, 1, M, N, K, seed, int(flat_a))  # the parent's draws, in its order: alpha, x, w
            torch.randint(0, 2, (1,), generator=g)
            ramp = torch.logspace(-3, 3, K // BLOCK).repeat_interleave(BLOCK)
            x = (torch.randn(M, K, generator=g).to(BF16).to(F32) * ramp).to(BF16)
            w = ((torch.randn(N, K, generator=g) / K ** 0.5).to(BF16).to(F32) / ramp).to(BF16)
            (a, sa), (b, sb) = quant4(x), quant4(w)
            self.a, self.sa, self.b, self.sb = a.to(device), sa.to(device), b.to(device), sb.to(device)
            a64, b64 = dequant4(self.a, self.sa), dequant4(self.b, self.sb)
            self.acc = self.acc0 = a64 @ b64.T
            self.absacc = self.absacc0 = a64.abs() @ b64.abs().T
        self.a_packed, self.b_packed = pack4(self.a), pack4(self.b)

    @property
    def name(self):
        return super().name.replace(" mxfp8 ", " mxfp4 ")


def given(x, w, bias, alpha=1.0, device="cpu"):
    """A family-R Inputs from given bf16 x [M, K], w [N, K] and bias [N]: both quantised with quant4, acc and absacc from the dequantised codes in
    float64 on `device` — the float64 chain of quantise-then-multiply."""
    inp = object.__new__(Inputs)
    (M, K), N = x.shape, w.shape[0]
    inp.family, inp.M, inp.N, inp.K, inp.seed, inp.flat_a, inp.device = "R", M, N, K, 0, False, device
    inp.alpha, inp.alpha_used, inp.bias_range, inp.units = alpha, None, None, None
    (a, sa), (b, sb) = quant4(x.to(device)), quant4(w.to(device))
    inp.a, inp.sa, inp.b, inp.sb = a, sa, b, sb
    a64, b64 = dequant4(a, sa), dequant4(b, sb)
    inp.acc = inp.acc0 = a64 @ b64.T
    inp.absacc = inp.absacc0 = a64.abs() @ b64.abs().T
    inp.bias = bias.to(device)
    inp.gate, inp.resid = torch.ones(N, dtype=BF16, device=device), torch.zeros(M, N, dtype=BF16, device=device)
    inp.a_packed, inp.b_packed = pack4(a), pack4(b)
    return inp


# ------------------------------------------------------------------------------------------------------------------- emulations
GEMM4_MUTATIONS = ("nibbles_swapped", "fragment_halves_swapped", "second_scale_dword_reused")  # each rejected under EPI_NONE, next to mx_ref.GEMM_MUTATIONS
QUANT4_MUTATIONS = {"divisor_28": dict(divisor=28.0), "divisor_448": dict(divisor=448.0), "e8m0_floor": dict(e8m0="floor"), "e2m1_trunc": dict(rnd="trunc"),
                    "neg_zero_to_zero": dict(neg_zero=False)}


def emulate(v, epi, use_bias=True, use_gate=True, truncating=False, mut=None):
    """mx_ref.emulate — a correct kernel in fp32 torch, block-ordered accumulation — on e2m1 operands: every e2m1 number is an e4m3 number, so the
    view's a and b go in as the e4m3 codes of the same values.  mut: one of mx_ref.GEMM_MUTATIONS, or of GEMM4_MUTATIONS:
      nibbles_swapped            the weight bytes read with the two codes of every byte exchanged: k and k ^ 1 of the weight trade places
      fragment_halves_swapped    the two 32-code pieces of a 64-wide step exchanged on the weight side: k and k ^ 32 trade places, scales stay
      second_scale_dword_reused  k blocks 4..7 of every 256-wide K-tile of a scaled with the bytes of its blocks 0..3 (the tile's first table dword)"""
    w = copy.copy(v)
    va, vb = e2m1_values(v.a.cpu()), e2m1_values(v.b.cpu())
    if mut == "nibbles_swapped":
        vb = vb[:, torch.arange(v.K) ^ 1]
    elif mut == "fragment_halves_swapped":
        vb = vb[:, torch.arange(v.K) ^ 32]
    elif mut == "second_scale_dword_reused":
        kb = torch.arange(v.K // BLOCK)
        w.sa = v.sa.cpu()[:, kb - 4 * ((kb >> 2) & 1)]
    w.a, w.b = X.e4m3_codes(va), X.e4m3_codes(vb)
    assert torch.equal(X.e4m3_values(w.a), va) and torch.equal(X.e4m3_values(w.b), vb)
    return X.emulate(w, epi, use_bias, use_gate, truncating, None if mut in GEMM4_MUTATIONS else mut)


# ------------------------------------------------------------------------------------------------------------------- quantiser inputs
PINS = {f"{m}*2^{k}": X._pin(m * 2.0 ** k) for k in (0, -60, 60) for m in (5.96875, 6, 6.03125)}  # at, one bf16 step below and one above 6 * 2^k
PINS.update({"1.5*2^-125 - 1 step": X._pin(1.5 * 2.0 ** -125) - 1, "1.5*2^-125": X._pin(1.5 * 2.0 ** -125), "1.5*2^-125 + 1 step": X._pin(1.5 * 2.0 ** -125) + 1,
             "2^-126": X._pin(2.0 ** -126), "least subnormal": 1, "largest finite": 0x7F7F})  # max / 6 = 2^-127: the ex == 0 branch of e8m0_ceil


def quant_input(M, K, seed=0):
    """mx_ref.quant_input with the block at the format's largest number (6) in place of 448."""
    x = X.quant_input(M, K, seed)
    x[0, :32] = 6.0
    return x


# ------------------------------------------------------------------------------------------------------------------- the GPU module's lists
BODY = {1: "gemm_mxfp4 128x128", 2: "gemm256 MX4 ping-pong"}
K_TILES = X.K_TILES  # 1, 2, 3, 4, 5 and 9 tiles, here of 256
M_TAILS, N_TAILS, TAIL_K = X.M_TAILS, X.N_TAILS, 256  # one K-tile
SCHED = tuple((M, N, 2 * K) for M, N, K in X.SCHED)  # mx_ref's two shapes at the same numbers of K-tiles: K = 256 and 512
DEEP = X.DEEP  # K = 13824: 54 K-tiles
EPI_SHAPES = ((257, 264, 512), (255, 248, 256), (1, 8, 256))
AUTO = ((3073, 4096, 1536), (3073, 4096, 1280))  # 13 x 16 = 208 tiles of 256: 6 K-tiles of 256 -> the 256x256 body, 5 -> the 128x128 body
QUANT_GRID = ((2050, 8192),)  # M K / 16 = 1_049_600 chunks: past the 4096 x 256 threads of the capped grid
ACCEPT = ((257, 1536, 1536), (512, 8960, 1536))  # (m, k, n)


def family_i_shapes():
    """Every (M, N, K) at which the GPU module runs family I."""
    s = [(X.K_TILES_MN[0], X.K_TILES_MN[1], nk * KTILE4) for nk in K_TILES] + [(M, 136, TAIL_K) for M in M_TAILS] + [(129, N, TAIL_K) for N in N_TAILS]
    return list(dict.fromkeys(s + list(SCHED) + list(DEEP) + list(EPI_SHAPES) + list(AUTO)))


def auto_body(M, N, K):
    """The body variant 0 takes without an epilogue (mx.hip mx_body: MXFP8's rule on the K-tiles of 256, from 6 K-tiles on instead of 8;
    row strides far below 2^24)."""
    return 2 if -(-M // 256) * -(-N // 256) >= 192 and K // KTILE4 >= 6 else 1
