"""float64 / NumPy restatement of the block-scaled fp8 self-attention contract of include/x2v.h (x2v_attn_mx_*; kernels in
lightx2v_amd/csrc/attn_mx.hip), written from that contract.  Plain NumPy and PyTorch on the CPU; nothing here imports the library or the oracle.
Shared by tests/test_attn_mx_host.py (the yardstick checked without a GPU) and tests/test_gpu_attn_mx.py (the kernels checked against it).

Tensors are head-major: q [H, Sq, 128], k / v [H, Sk, 128], bf16 (tests/attn_ref.py's convention).  Scores are in base 2.

  kmean32        the fp32 column mean of k in the contract's summation order (256-token chunks in token order, then the chunk sums in chunk order)
  quant_rows     MXFP8 along the last axis: scale bytes and e4m3 codes of fp32 values, bit level
  quant_qk       Q^ / K^ in the device layout (codes [H, S_pad, 128], scale bytes [H, S_pad, 4], padding rows zero)
  quant_vt       V^T^ in the device layout (codes [H, NT, 128 dv, 128 keys], scale bytes [H, NT, 128, 4]), keys >= Sk as code 0
  deq_qk, deq_vt dequantisers of those layouts -> float64 [H, S, 128] (so a test can read the DEVICE buffers)
  exact          float64 softmax attention over dequantised operands: o, A = sum_j w_j |v^_jd|, and the flush term F
  emulate        the kernel's arithmetic on dequantised operands: fp32 scores, exact running max per 128-key tile, P^ = e4m3(P * 2^8), fp32 row sum of the
                 unrounded P, one rounding of o to bf16
  pipeline       bf16 q, k, v -> everything above in one object (Restated)

Element bound of the GPU test (derivation in tests/test_gpu_attn_mx.py): |got - o| <= 2^-7 |o| + 1.05 * 2^-4 * A + F,
F_d = 2^-18 / l * sum over the keys j with P_j < 2^-14 of |v^_jd|, P_j = 2^(s_j - max_j s_j), l = sum_j P_j."""
import math

import numpy as np
import torch

from tests import attn_ref as A

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
D = 128
TILE = 128  # keys per tile and per V^T^ tile
MEAN_CHUNK = 256
P_SHIFT = 8  # P^ = e4m3(P * 2^8)
P_MIN_NORMAL = 2.0 ** (-6 - P_SHIFT)  # the smallest P with a normal e4m3 code: relative half-ulp 2^-4 from here up
P_HALF_STEP = 2.0 ** (-9 - P_SHIFT - 1)  # half the spacing of the subnormal codes (smallest positive code 2^-9 -> P = 2^-17): absolute error below P_MIN_NORMAL
E4M3_HALF_ULP = 2.0 ** -4
ULP = 2.0 ** -7
MARGIN = 1.05
TRIANGLE = 1.5
FAMILIES = ("R", "N", "H", "U", "sea", "offset")
SEA_BINADES = 10


def q_scale(scale=0.0, prescaled=False):
    """The fp32 the q quantiser multiplies by: 1 for a q that carries the scale, else the fp32 nearest to softmax scale * log2(e)."""
    if prescaled:
        return np.float32(1.0)
    return np.float32(scale * 1.4426950408889634 if scale > 0 else 1.4426950408889634 / math.sqrt(128.0))


# ------------------------------------------------------------------------------------------------------------------- number formats
def e8m0_byte(amax):
    """float32 array (>= 0) -> uint8: biased exponent of the smallest power of two >= amax / 448 (fp32 quotient), 0 for 0, at most 254."""
    sf = (amax.astype(np.float32) / np.float32(448.0)).astype(np.float32)
    m, e = np.frexp(sf.astype(np.float64))  # sf = m * 2^e, m in [0.5, 1)
    ex = np.where(m == 0.5, e - 1, e)
    return np.where(sf == 0, 0, np.clip(ex + 127, 0, 254)).astype(np.uint8)


def e4m3_codes(a):
    """float64 array, |a| <= 448 -> uint8 e4m3fn codes, round to nearest even, the sign of a zero kept."""
    a = np.asarray(a, dtype=np.float64)
    sign = np.signbit(a).astype(np.uint8) << 7
    m = np.abs(a)
    _, e = np.frexp(m)
    e = np.maximum(e - 1, -6)  # floor(log2 m), held at the subnormal exponent
    n = np.rint(np.ldexp(m, 3 - e))  # multiples of 2^(e - 3): 8..15 for a normal number, 0..7 below 2^-6; 16 = carry
    carry = n == 16
    e = np.where(carry, e + 1, e)
    n = np.where(carry, 8, n).astype(np.int64)
    code = np.where(n < 8, n, ((e + 7) << 3) | (n - 8))
    return (np.minimum(code, 0x7E).astype(np.uint8) | sign).astype(np.uint8)


def e4m3_values(code):
    code = np.asarray(code, dtype=np.uint8)
    e, m = ((code >> 3) & 15).astype(np.int64), (code & 7).astype(np.float64)
    v = np.where(e == 0, np.ldexp(m, -9), np.ldexp(1.0 + m / 8.0, e - 7))
    return np.where(code >> 7 == 1, -v, v)


def quant_rows(x):
    """x float32 [..., 32 n]: MXFP8 along the last axis.  Returns (codes uint8 [..., 32 n], scale bytes uint8 [..., n])."""
    x = np.asarray(x, dtype=np.float32)
    b = x.reshape(*x.shape[:-1], x.shape[-1] // 32, 32)
    byte = e8m0_byte(np.abs(b).max(-1))
    scaled = np.ldexp(b.astype(np.float64), (127 - byte.astype(np.int64))[..., None])
    return e4m3_codes(scaled).reshape(x.shape), byte


def deq_rows(codes, byte):
    v = e4m3_values(codes)
    b = v.reshape(*v.shape[:-1], v.shape[-1] // 32, 32)
    return np.ldexp(b, (np.asarray(byte).astype(np.int64) - 127)[..., None]).reshape(v.shape)


# ------------------------------------------------------------------------------------------------------------------- the three preparation steps
def kmean32(k):
    """k bf16 [H, Sk, 128] -> float32 [H, 128] in the contract's order."""
    x = k.to(F32).numpy()
    H, Sk, _ = x.shape
    nch = (Sk + MEAN_CHUNK - 1) // MEAN_CHUNK
    pad = np.zeros((H, nch * MEAN_CHUNK, D), dtype=np.float32)  # adding +0 behind a chunk's last token changes nothing
    pad[:, :Sk] = x
    c = pad.reshape(H, nch, MEAN_CHUNK, D)
    s = c[:, :, 0].copy()
    for t in range(1, MEAN_CHUNK):
        s = (s + c[:, :, t]).astype(np.float32)
    tot = s[:, 0].copy()
    for i in range(1, nch):
        tot = (tot + s[:, i]).astype(np.float32)
    return (tot / np.float32(Sk)).astype(np.float32)


def quant_qk(x, mean=None, scale=np.float32(1.0), S_pad=None):
    """x bf16 [H, S, 128]; mean float32 [H, 128] or None -> (codes [H, S_pad, 128], scale bytes [H, S_pad, 4]); rows past S are zero."""
    xf = x.to(F32).numpy()
    H, S, _ = xf.shape
    m = np.zeros((H, 1, D), dtype=np.float32) if mean is None else np.asarray(mean, dtype=np.float32).reshape(H, 1, D)
    xp = ((xf - m).astype(np.float32) * np.float32(scale)).astype(np.float32)
    codes, byte = quant_rows(xp)
    S_pad = S if S_pad is None else S_pad
    c = np.zeros((H, S_pad, D), dtype=np.uint8)
    b = np.zeros((H, S_pad, 4), dtype=np.uint8)
    c[:, :S], b[:, :S] = codes, byte
    return c, b


def quant_vt(v):
    """v bf16 [H, Sk, 128] -> (codes [H, NT, 128 dv, 128 keys], scale bytes [H, NT, 128 dv, 4])."""
    vf = v.to(F32).numpy()
    H, Sk, _ = vf.shape
    nt = (Sk + TILE - 1) // TILE
    pad = np.zeros((H, nt * TILE, D), dtype=np.float32)
    pad[:, :Sk] = vf  # keys >= Sk are zeros: code 0, no share in a block's amax
    vt = pad.reshape(H, nt, TILE, D).transpose(0, 1, 3, 2)  # [H, NT, dv, key]
    codes, byte = quant_rows(np.ascontiguousarray(vt))
    return codes, byte


def deq_qk(codes, byte, S):
    """Device layout -> float64 tensor [H, S, 128]."""
    return torch.from_numpy(deq_rows(np.asarray(codes), np.asarray(byte))[:, :S].copy())


def deq_vt(codes, byte, Sk):
    v = deq_rows(np.asarray(codes), np.asarray(byte))  # [H, NT, dv, key]
    H, nt = v.shape[:2]
    return torch.from_numpy(v.transpose(0, 1, 3, 2).reshape(H, nt * TILE, D)[:, :Sk].copy())


# ------------------------------------------------------------------------------------------------------------------- attention on dequantised operands
def exact(qd, kd, vd):
    """float64 softmax attention (base 2) of dequantised operands.  Returns (o, A, F), all [H, Sq, 128]."""
    s = qd @ kd.transpose(-1, -2)
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    l = p.sum(-1, keepdim=True)
    va = vd.abs()
    o, Aw = (p @ vd) / l, (p @ va) / l
    F = P_HALF_STEP * ((p < P_MIN_NORMAL).to(F64) @ va) / l
    return o, Aw, F


def tol(o, Aw, F):
    return ULP * o.abs() + MARGIN * E4M3_HALF_ULP * Aw + F


def emulate(qd, kd, vd):
    """The kernel's arithmetic: fp32 scores per 128-key tile relative to the running max, exact running max, P^ rounded to e4m3 after the 2^8
    shift for the PV product only, fp32 row sum of the unrounded P, fp32 O, one rounding to bf16."""
    H, Sq, _ = qd.shape
    Sk = kd.shape[1]
    s_all = (qd @ kd.transpose(-1, -2)).to(F32)  # the MFMA's fp32 result of exact products
    m = torch.zeros(H, Sq, dtype=F32)
    l = torch.zeros(H, Sq, dtype=F32)
    o = torch.zeros(H, Sq, D, dtype=F32)
    for t0 in range(0, Sk, TILE):
        st = s_all[..., t0 : t0 + TILE] - m.unsqueeze(-1)
        mx = st.amax(-1)
        d = mx if t0 == 0 else mx.clamp_min(0.0)
        if t0 > 0:
            al = torch.exp2(-d)
            l, o = l * al, o * al.unsqueeze(-1)
        m = m + d
        p = torch.exp2(st - d.unsqueeze(-1))
        l = l + p.sum(-1)
        ph = torch.from_numpy(e4m3_values(e4m3_codes(p.to(F64).numpy() * 2.0 ** P_SHIFT))) * 2.0 ** -P_SHIFT
        o = o + (ph @ vd[:, t0 : t0 + TILE]).to(F32)
    return (o / l.unsqueeze(-1)).to(BF16)


class Restated:
    """bf16 q, k, v -> the restated operands, their dequantised values, the exact attention over them (o, A, F), the emulation and its Y."""

    def __init__(self, q, k, v, prescaled=False, smooth_k=True, scale=0.0, kmean=None):
        Sq, Sk = q.shape[1], k.shape[1]
        self.kmean = (kmean32(k) if kmean is None else np.asarray(kmean, dtype=np.float32)) if smooth_k else None
        self.q_codes, self.q_scales = quant_qk(q, None, q_scale(scale, prescaled))
        self.k_codes, self.k_scales = quant_qk(k, self.kmean, np.float32(1.0), (Sk + TILE - 1) // TILE * TILE)
        self.vt_codes, self.vt_scales = quant_vt(v)
        self.qd, self.kd, self.vd = deq_qk(self.q_codes, self.q_scales, Sq), deq_qk(self.k_codes, self.k_scales, Sk), deq_vt(self.vt_codes, self.vt_scales, Sk)
        self.o, self.A, self.F = exact(self.qd, self.kd, self.vd)
        self.emulated = emulate(self.qd, self.kd, self.vd)
        self.Y = A.rel_l2(self.emulated, self.o)

    def tol(self):
        return tol(self.o, self.A, self.F)


# ------------------------------------------------------------------------------------------------------------------- inputs
class MxInputs:
    """attn_ref.Inputs plus the two families of this contract.
    sea:    Sk - 1 equal keys u and ONE key (in the middle) whose score is 10 base-2 units above theirs for every query (q's channel 0 is the
            constant 4, the spike is u + 19.625 e_0: 4 * 19.625 / sqrt(128) * log2(e) = 10.01).  With Sk - 1 > 2^10 the sea holds most of the weight;
            a P operand whose tail is flushed at 2^-9 instead of 2^-17 loses the whole sea.  The sea's v rows are one vector w plus noise of size 0.25 and
            the spike's v row is unrelated, so the sea's share of the output does not average out.
    offset: k = a per-channel constant of size ~8 plus a variation of size 0.25: what K smoothing is for."""

    def __init__(self, family, Sq, Sk, H, spike="none", seed=0):
        assert family in FAMILIES
        self.family, self.Sq, self.Sk, self.H, self.spike, self.seed = family, Sq, Sk, H, spike, seed
        if family in A.FAMILIES:
            base = A.Inputs(family, Sq, Sk, H, spike, seed)
            self.q, self.k, self.v = base.q, base.k, base.v
            return
        g = torch.Generator().manual_seed(7919 * FAMILIES.index(family) + 31 * Sq + 17 * Sk + H + 1000 * seed)
        rn = lambda *shape: torch.randn(*shape, generator=g)
        if family == "sea":
            q = rn(H, Sq, D)
            q[..., 0] = 4.0
            u = rn(H, 1, D)
            k = u.expand(H, Sk, D).clone()
            k[:, Sk // 2, 0] += 19.625
            v = rn(H, 1, D) + 0.25 * rn(H, Sk, D)  # the sea's values agree (w + noise), so losing the sea moves the output; the spike's own row is apart
            v[:, Sk // 2] = rn(H, D)
            self.q, self.k, self.v = q.to(BF16), k.to(BF16), v.to(BF16)
        else:
            self.q, self.k, self.v = rn(H, Sq, D).to(BF16), (8.0 * rn(H, 1, D) + 0.25 * rn(H, Sk, D)).to(BF16), rn(H, Sk, D).to(BF16)

    @property
    def name(self):
        return f"{self.family}{'' if self.spike == 'none' else '-' + self.spike} Sq={self.Sq} Sk={self.Sk} H={self.H}"


def families():
    return [("R", s) for s in A.SPIKES] + [("N", "none"), ("H", "none"), ("U", "none"), ("sea", "none"), ("offset", "none")]


SK_SWEEP = (1, 31, 32, 33, 127, 128, 129, 200, 296, 1576)  # Sq = Sk
RECT_SQ, RECT_SK = (1, 33, 255, 256, 257), (200, 1576)
H_TEST = 2

_RESTATED = {}


def restated(inp, prescaled=False, smooth_k=True):
    """Restated(...) of a seeded case, computed once per run and shared by the tests that need it (the GPU module passes the kernel's own kmean
    to the bit comparison separately)."""
    key = (inp.family, inp.Sq, inp.Sk, inp.H, inp.spike, inp.seed, prescaled, smooth_k)
    if key not in _RESTATED:
        q = A.prescale_q(inp.q) if prescaled else inp.q
        _RESTATED[key] = Restated(q, inp.k, inp.v, prescaled, smooth_k)
    return _RESTATED[key]


def exact_bf16(inp):
    """Exact float64 attention on the bf16 inputs themselves (no quantisation): what `hip_flash` approximates."""
    return A.ref64(inp.q, inp.k, inp.v)[0]
