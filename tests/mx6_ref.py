"""float64 references, seeded inputs and fp32 emulations for the MXFP6-weight path: quant_mx_kernel<2> (lightx2v_amd/csrc/mx.hip) and the MXM = 2
instantiations of gemm_kernel (gemm.hip, 128x128) — MXFP6 (e3m2) weights x MXFP8 (e4m3) activations.  Plain PyTorch on float64; nothing here imports
the library or oracle/.  The scale rule, the table layout, family I / R, Expect, Case, the epilogue chains and both acceptance rules are
tests/mx_ref.py's and tests/gemm_ref.py's; this module adds the 6-bit element, its packing and the inputs whose b is e3m2.  Shared by
tests/test_mx6_ref_host.py (the yardstick checked without a GPU) and tests/test_gpu_mx6.py (the kernels checked against it).

The references restate include/x2v.h:
  e3m2        code = s << 5 | e << 2 | m: 1 sign, 3 exponent bits (bias 3), 2 mantissa bits; e = 0: m * 2^-4, else (4 + m) * 2^(e - 5); largest 28
  packing     the dense little-endian 6-bit string: code j of a row at bits 6 j .. 6 j + 5 of the row's bytes (4 codes = 3 bytes)
  quantiser   mx_ref's with 28 in place of 448: scale byte = biased exponent of the smallest power of two >= max|x| / 28 (fp32 quotient with
              denormals, saturating at 254, all-zero block -> 0); code = e3m2(x * 2^(127 - byte)), one rounding to nearest-even, saturating at
              +/-28, sign of zero kept
  GEMM        mx_ref's chain with deq(b) = e3m2 value * 2^(scale byte - 127)

Family I carries over unchanged: every integer in [-7, 7] is an e3m2 number, W codes are the integers in [-4, 4], so the product, the premises and
the float64 chain are those of the MXFP8 input of the same seed.  Family R quantises the same ramped weights with quant6."""
import copy

import torch

from tests import gemm_ref as G
from tests import mx_ref as X
from tests.gemm_ref import BF16, F32, F64
from tests.mx_ref import BLOCK, I64, U8, floor_log2, pow2, round_fp32

DIVISOR = 28.0  # the largest e3m2 number


# ------------------------------------------------------------------------------------------------------------------- float64 pieces
def e8m0_byte(amax, mode="ceil", divisor=DIVISOR):
    """Block maxima (float64, finite, >= 0) -> scale bytes (int64): mx_ref.e8m0_byte with the divisor 28 (= 7 * 4: the float64 quotient of an
    8-bit significand by 7 is periodic, so it rounds to fp32 as the exact one does).  divisor 448 and mode 'floor' are the host module's mutations."""
    sf = round_fp32(amax / divisor)
    e = floor_log2(sf)
    up = (sf != pow2(e.clamp_min(-1022))) & (sf > 0) if mode == "ceil" else torch.zeros_like(sf, dtype=torch.bool)
    return torch.where(sf > 0, (e + up.to(I64) + 127).clamp(0, 254), torch.zeros_like(e))


def e3m2_codes(v, rnd="rne", neg_zero=True):
    """float64 -> e3m2 codes (uint8, 0..63): 3 significant bits, least exponent -2 (steps of 2^-4 below 2^-2), one rounding, saturating at 28 (0x1F).
    rnd 'trunc' and neg_zero=False ('-0 -> +0') are the host module's mutations."""
    a = v.abs()
    e = floor_log2(a).clamp(-2, 4)
    r = a * pow2(2 - e)  # exact; [4, 8) in the normal range, [0, 4) below 2^-2
    r = (torch.round(r) if rnd == "rne" else torch.trunc(r)).to(I64)
    code = (((e + 3) << 2) + r - 4).clamp(0, 0x1F)  # r = 8 carries into the exponent field by itself
    sign = torch.signbit(v) if neg_zero else torch.signbit(v) & (code != 0)
    return (code + (sign.to(I64) << 5)).to(U8)


def e3m2_values(code):
    """e3m2 codes -> float64."""
    c = code.to(I64)
    e, m = (c >> 2) & 7, c & 3
    mag = torch.where(e == 0, m.to(F64) * 2.0 ** -4, (4 + m).to(F64) * pow2(e - 5))
    return torch.where(((c >> 5) & 1) == 1, -mag, mag)


def e2m3_values(code):
    """The OTHER 6-bit format of the matrix instruction (format code 2, 'fp6': 2 exponent bits of bias 1, 3 mantissa bits) — what a kernel with the
    wrong format code decodes: the host module's mutation."""
    c = code.to(I64)
    e, m = (c >> 3) & 3, c & 7
    mag = torch.where(e == 0, m.to(F64) * 2.0 ** -3, (8 + m).to(F64) * pow2(e - 4))
    return torch.where(((c >> 5) & 1) == 1, -mag, mag)


def pack6(codes, endian="little"):
    """Codes uint8 [rows, K] (0..63) -> bytes uint8 [rows, 3 K / 4]: code j of a row at bits 6 j .. 6 j + 5.  endian 'big' (the first code of four in
    the high bits of the first byte) is the host module's mutation."""
    rows, K = codes.shape
    assert K % 4 == 0 and int(codes.max()) < 64
    c = codes.to(I64).reshape(rows, K // 4, 4)
    if endian == "little":
        w = c[..., 0] | (c[..., 1] << 6) | (c[..., 2] << 12) | (c[..., 3] << 18)
        b = torch.stack([w & 255, (w >> 8) & 255, (w >> 16) & 255], -1)
    else:
        w = (c[..., 0] << 18) | (c[..., 1] << 12) | (c[..., 2] << 6) | c[..., 3]
        b = torch.stack([(w >> 16) & 255, (w >> 8) & 255, w & 255], -1)
    return b.to(U8).reshape(rows, K // 4 * 3)


def unpack6(packed):
    """Bytes uint8 [rows, 3 K / 4] -> codes uint8 [rows, K]."""
    rows, nb = packed.shape
    assert nb % 3 == 0
    b = packed.to(I64).reshape(rows, nb // 3, 3)
    w = b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16)
    return torch.stack([w & 63, (w >> 6) & 63, (w >> 12) & 63, (w >> 18) & 63], -1).to(U8).reshape(rows, nb // 3 * 4)


def quant6(x, e8m0="ceil", rnd="rne", neg_zero=True, divisor=DIVISOR, rows_per_step=1024):
    """x bf16 [M, K] (finite) -> (e3m2 codes uint8 [M, K], UNPACKED, scale bytes uint8 [M, K / 32]), row-major; pack6 gives the kernel's bytes."""
    M, K = x.shape
    assert K % BLOCK == 0 and x.dtype == BF16
    q, sc = torch.empty(M, K, dtype=U8, device=x.device), torch.empty(M, K // BLOCK, dtype=U8, device=x.device)
    for r0 in range(0, M, rows_per_step):
        xb = x[r0 : r0 + rows_per_step].to(F32).to(F64).reshape(-1, K // BLOCK, BLOCK)
        byte = e8m0_byte(xb.abs().amax(-1), e8m0, divisor)
        q[r0 : r0 + rows_per_step] = e3m2_codes(xb * pow2(127 - byte).unsqueeze(-1), rnd, neg_zero).reshape(-1, K)
        sc[r0 : r0 + rows_per_step] = byte.to(U8)
    return q, sc


def dequant6(code, sc):
    """e3m2 codes [rows, K] (unpacked) and scale bytes [rows, K / 32] -> float64 [rows, K] (exact)."""
    rows, K = code.shape
    return (e3m2_values(code).reshape(rows, K // BLOCK, BLOCK) * pow2(sc.to(I64) - 127).unsqueeze(-1)).reshape(rows, K)


# ------------------------------------------------------------------------------------------------------------------- inputs
class Inputs(X.Inputs):
    """mx_ref.Inputs whose b is e3m2: `b` the unpacked codes [N, K] (0..63), `b_packed` the kernel's bytes [N, 3 K / 4].  Family I: the codes of the
    same integers in [-4, 4] (acc, units, bias, resid and the premises are the parent's, unchanged).  Family R: quant6 of the parent's ramped
    weights, drawn again from the parent's seed; acc and absacc recomputed."""

    dtype = "mxfp8"  # Expect: the w8a8 term K + 3 (fp32 accumulation of exact products, as MXFP8)

    def __init__(self, family, M, N, K, seed=0, flat_a=False, device="cpu"):
        super().__init__(family, M, N, K, seed, flat_a, device)
        if family == "I":
            vals = X.e4m3_values(self.b)
            assert float(vals.abs().max()) <= 4 and bool((vals == vals.round()).all())
            self.b = e3m2_codes(vals)
            assert torch.equal(e3m2_values(self.b), vals)
        else:
            g = G._gen(77, 1, M, N, K, seed, int(flat_a))  # the parent's draws, in its order: alpha, x, w
            torch.randint(0, 2, (1,), generator=g)
            torch.randn(M, K, generator=g)
            ramp = torch.logspace(-3, 3, K // BLOCK).repeat_interleave(BLOCK)
            w = ((torch.randn(N, K, generator=g) / K ** 0.5).to(BF16).to(F32) / ramp).to(BF16)
            b, sb = quant6(w)
            self.b, self.sb = b.to(device), sb.to(device)
            a64, b64 = X.dequant(self.a, self.sa), dequant6(self.b, self.sb)
            self.acc = self.acc0 = a64 @ b64.T
            self.absacc = self.absacc0 = a64.abs() @ b64.abs().T
        self.b_packed = pack6(self.b)

    @property
    def name(self):
        return super().name.replace(" mxfp8 ", " mxfp6xmxfp8 ")


# ------------------------------------------------------------------------------------------------------------------- emulations
GEMM6_MUTATIONS = ("e2m3_decoding", "big_endian_packing", "fragment_halves_swapped")  # each rejected under EPI_NONE, next to mx_ref.GEMM_MUTATIONS
QUANT6_MUTATIONS = {"divisor_448": dict(divisor=448.0), "e8m0_floor": dict(e8m0="floor"), "e3m2_trunc": dict(rnd="trunc"), "neg_zero_to_zero": dict(neg_zero=False)}


def emulate(v, epi, use_bias=True, use_gate=True, truncating=False, mut=None):
    """mx_ref.emulate — a correct kernel in fp32 torch, block-ordered accumulation — on the e3m2 weights: every e3m2 (and e2m3) number is an e4m3
    number, so the view's b goes in as the e4m3 codes of the same values.  mut: one of mx_ref.GEMM_MUTATIONS, or of GEMM6_MUTATIONS:
      e2m3_decoding            the instruction's other 6-bit format (format code 2 instead of 3)
      big_endian_packing       the weight bytes written with the first code of four in the high bits, read as the little-endian string
      fragment_halves_swapped  the two 16-code pieces of a lane's fragment exchanged: k and k ^ 32 of the weight trade places, scales stay"""
    w = copy.copy(v)
    codes = v.b.cpu()
    if mut == "big_endian_packing":
        codes = unpack6(pack6(codes, "big"))
    vals = e2m3_values(codes) if mut == "e2m3_decoding" else e3m2_values(codes)
    if mut == "fragment_halves_swapped":
        vals = vals[:, torch.arange(v.K) ^ 32]
    w.b = X.e4m3_codes(vals)
    assert torch.equal(X.e4m3_values(w.b), vals)
    return X.emulate(w, epi, use_bias, use_gate, truncating, None if mut in GEMM6_MUTATIONS else mut)


# ------------------------------------------------------------------------------------------------------------------- quantiser inputs
PINS = {f"{m}*2^{k}": X._pin(m * 2.0 ** k) for k in (0, -60, 60) for m in (27.875, 28, 28.125)}  # at, one bf16 step below and one above 28 * 2^k
PINS.update({"1.75*2^-123 - 1 step": X._pin(1.75 * 2.0 ** -123) - 1, "1.75*2^-123": X._pin(1.75 * 2.0 ** -123), "1.75*2^-123 + 1 step": X._pin(1.75 * 2.0 ** -123) + 1,
             "2^-126": X._pin(2.0 ** -126), "least subnormal": 1, "largest finite": 0x7F7F})  # max / 28 = 2^-127: the ex == 0 branch of e8m0_ceil


def quant_input(M, K, seed=0):
    """mx_ref.quant_input with the block at the format's largest number (28) in place of 448."""
    x = X.quant_input(M, K, seed)
    x[0, :32] = 28.0
    return x


QUANT_GRID = ((2050, 8192),)  # M K / 16 = 1_049_600 chunks: past the 4096 x 256 threads of the capped grid
ACCEPT = ((257, 1536, 1536), (512, 8960, 1536))  # (m, k, n) of the reference's own acceptance test run here
