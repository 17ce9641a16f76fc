"""float64 references, seeded inputs, fp32 emulations and the acceptance rules for the VAE convolution family of lightx2v_amd/csrc (vae.hip's per-tap
kernel in fp32 and fp16 and its 64-pixel halo kernel, vae16g.hip's 128-pixel kernel, vae_enc.hip's stride-2 kernel).  Plain PyTorch; nothing here imports
the library or the oracle.  Shared by tests/test_vae_conv_ref_host.py (the yardstick checked without a GPU) and tests/test_gpu_vae_conv_fp64.py (the
kernels checked against it), which take their cases from the lists at the end of this file.

The reference restates the contracts of include/x2v.h (x2v_vae_conv_f32, x2v_vae_conv_f16, x2v_vae_conv_f16_cached, x2v_vae_conv_s2_f16), not a kernel:
  t = sum over taps (dt, dh, dw) of x[window of the tap] . w[tap]^T + bias + resid        in float64, one matmul per tap on a shifted view (conv64)
  then the clamp to [-1, 1] (VCONV_CLAMP), then the time-split (VCONV_TSPLIT: channel block j of frame t -> frame 2t + j); the stride-2 form reads
  x[t, 2 oy + dh, 2 ox + dw] with a zero row below and a zero column right of the image.  The kt - 1 leading frames of the input are the causal
  convolution's cache, in front of the frames or (the separate-cache form) in a tensor of their own: the same numbers either way.

Two input families, the same for every kernel body:

  I  small integers: x in [-8, 8], w in [-4, 4], bias and resid in [-200, 200].  Every value is exact in fp16 and fp32 and every partial sum is exact
     in fp32 (8 * 4 * K + 400 < 2^24 is asserted), so any correct kernel, whatever its order, gives t itself: Case.check_exact asks for
     torch.equal(got, t.float()) on every element.  A tap, slab, halo row or weight row that is dropped, doubled or shifted changes the integer.
     With VCONV_CLAMP the residual is steered (inside its range) so that both clamp sides and the interior occur; Inputs asserts that they do.

  R  x ~ N(0, 1), w ~ N(0, 1) / sqrt(K), bias, resid ~ N(0, 1); fp32 for the fp32 body, fp16-rounded for the 16-bit bodies (products exact in fp32).
     Case.check_bound applies two rules, no share of elements left out of either, no constant fitted to a kernel:
       per element   |got - t| <= (K + 2) 2^-23 (|x| . |w|^T + |bias| + |resid|), K = taps * Cin: the a-priori bound of an fp32 accumulation of K
                     products, a bias and a residual in any order, with the unit 2^-23 = twice the round-to-nearest unit roundoff so that a matrix
                     unit that truncates when it aligns addends is covered (the clamp is 1-Lipschitz and the time-split a permutation);
       yardstick     relL2(got, t) <= 1.5 Y, Y = the largest relative L2 error against the same t of fp32 emulations of a correct kernel on the same
                     operands: a strictly sequential fp32 chain over (tap, channel), and the documented order of the kernels — exact partial dot
                     products over a 32- or 64-channel slab of one tap, each rounded to fp32 once and chained.  Y never comes from a kernel.

Split mode (conv16="split"): activations [hi | hi 2^-12 | lo], weights [hi | lo 2^12 | hi] (split_x / split_w restate both).  The convolution of
those planes is an ordinary 16-bit case; the end-to-end claim "fp32-grade" is relL2 against the float64 convolution of the UNROUNDED operands
<= 1.5 Y with Y the fp32 chain on the unrounded operands (Inputs.t_unrounded / yardstick_unrounded)."""
import math
from collections import namedtuple

import torch

F64, F32, F16 = torch.float64, torch.float32, torch.float16
CLAMP, TSPLIT, PER_TAP, HALO64, ZERO_TAIL32 = 1, 2, 4, 8, 16  # x2v.h X2V_VCONV_* and the kernel-choice / zero-tail flags of x2v_vae_conv_f16
UNIT = 2.0 ** -23
MARGIN = 1.5  # the attention suite's margin over its yardstick
ON_DEVICE_ABOVE = 1 << 19  # outputs above which the float64 side runs on the device


def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 31) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def rel_l2(got, ref):
    return float((got.to(F64) - ref).norm() / ref.norm().clamp_min(1e-300))


# ------------------------------------------------------------------------------------------------------------------- cases
S2_OPS = ("s2", "p32")  # the stride-2 contract: the 16-bit kernel, and the fp32 polyphase decomposition of lightx2v_amd/vae_enc.py (four x2v_vae_conv_f32 calls)
_Spec = namedtuple("Spec", "op T H W Cin Cout k flags bias resid cache tail C")


def Spec(op, T, H, W, Cin, Cout, k=(1, 1, 1), flags=0, bias=True, resid=True, cache=False, tail=0, C=0):
    """One call.  op 'f32' (x2v_vae_conv_f32), 'f16' (x2v_vae_conv_f16[_cached]), 's2' (x2v_vae_conv_s2_f16: H, W are the INPUT's, no residual) or 'p32'
    (the same stride-2 convolution on fp32 operands).
    tail: trailing channels of Cin that are zero in both operands (with ZERO_TAIL32 the device buffers hold loud values there instead).
    C > 0: split operands of C fp32 channels in the first 3 C of Cin.  cache: the separate-cache form."""
    if op in S2_OPS:
        k, resid = (1, 3, 3), False
    if flags & TSPLIT:
        resid = False
    assert not (flags & ZERO_TAIL32) or tail == 32
    assert not C or tail == Cin - 3 * C
    return _Spec(op, T, H, W, Cin, Cout, tuple(k), flags, bias, resid, cache, tail, C)


def out_hw(sp):
    return (sp.H // 2, sp.W // 2) if sp.op in S2_OPS else (sp.H, sp.W)


def n_out(sp):
    ho, wo = out_hw(sp)
    return sp.T * ho * wo * sp.Cout


def name_of(sp):
    kt, kh, kw = sp.k
    return (f"{sp.op} {sp.T}x{sp.H}x{sp.W} {sp.Cin}->{sp.Cout} k{kt}{kh}{kw} f{sp.flags}" + ("" if sp.bias else " nobias") + (" resid" if sp.resid else "") +
            (" cache" if sp.cache else "") + (f" tail{sp.tail}" if sp.tail else "") + (f" split{sp.C}" if sp.C else ""))


def nf_of(Cout):
    """32-cout blocks per workgroup of the per-tap and 64-pixel halo kernels (vae.hip with_vconv_nf)."""
    if Cout <= 32:
        return 1
    if Cout % 128 != 0 and Cout % 96 == 0:
        return 3
    return 2 if Cout <= 64 else 4


def body_of(op, W, Cin, Cout, k, flags):
    """The kernel body a call reaches under the default dispatch (vae.hip x2v_vae_conv_f32 / vae_conv_f16_impl, vae16g.hip vae_conv16g_ok)."""
    kt, kh, kw = k
    if op == "s2":
        return "s2 16x16x96"
    if op in ("f32", "p32"):
        return f"pertap f32 NF{nf_of(Cout)} KC{32 if Cin % 32 == 0 else 16}"
    g_ok = (Cout % 96 == 0 or Cout % 128 == 0 or Cout <= 16) and Cin % 32 == 0 and W >= 16
    if kh == 3 and kw == 3 and not flags & (TSPLIT | PER_TAP | HALO64) and g_ok:
        return f"halo128 NCB{6 if Cout % 96 == 0 else 8 if Cout % 128 == 0 else 1}"
    if kh == 3 and kw == 3 and not flags & (TSPLIT | PER_TAP) and W >= 16:
        return f"halo64 NF{nf_of(Cout)}"
    return f"pertap f16 NF{nf_of(Cout)} KC64"


def body(sp):
    return body_of(sp.op, sp.W, sp.Cin, sp.Cout, sp.k, sp.flags)


def slab_of(sp):
    """Channels of one K step of the body (the documented reduction orders: vae.hip, vae16g.hip, vae_enc.hip)."""
    b = body(sp)
    return 32 if b.startswith(("halo128", "s2")) else 64 if sp.op == "f16" else (32 if sp.Cin % 32 == 0 else 16)


def n_slabs(sp):
    """K steps of the 128-pixel body: kt x 32-channel slabs, the zero tail skipped with ZERO_TAIL32."""
    return sp.k[0] * (sp.Cin - (32 if sp.flags & ZERO_TAIL32 else 0)) // 32


def cached_ok(sp):
    """x2v_vae_conv_f16_cached_ok restated."""
    return sp.op == "f16" and sp.k[0] > 1 and body(sp).startswith("halo128")


# ------------------------------------------------------------------------------------------------------------------- float64 pieces
def conv64(xpad, w, T, H, W, stride=1):
    """sum over taps of xpad[dt : dt + T, dh : dh + stride H : stride, dw : dw + stride W : stride] . w[:, dt, dh, dw]^T — xpad [>= T + kt - 1, Hp, Wp, C]
    with its zero border in place, w [Cout, kt, kh, kw, C]; both float64, on any device.  Returns [T, H, W, Cout]."""
    assert xpad.dtype == F64 and w.dtype == F64
    Cout, kt, kh, kw, C = w.shape
    acc = torch.zeros(T * H * W, Cout, dtype=F64, device=xpad.device)
    for dt in range(kt):
        for dh in range(kh):
            for dw in range(kw):
                v = xpad[dt : dt + T, dh : dh + stride * (H - 1) + 1 : stride, dw : dw + stride * (W - 1) + 1 : stride]
                assert v.shape[:3] == (T, H, W)
                acc += v.reshape(-1, C) @ w[:, dt, dh, dw].T
    return acc.view(T, H, W, Cout)


def pad_frames(x, k, stride=1):
    """The zero border of the convolution around frames x [F, H, W, C]: kh // 2 rows and kw // 2 columns on every side (stride 1), or one row below and
    one column right (the stride-2 form's ZeroPad2d((0, 1, 0, 1)))."""
    kt, kh, kw = k
    F, H, W, C = x.shape
    if stride == 2:
        out = x.new_zeros(F, H + 1, W + 1, C)
        out[:, :H, :W] = x
        return out
    ph, pw = kh // 2, kw // 2
    out = x.new_zeros(F, H + 2 * ph, W + 2 * pw, C)
    out[:, ph : ph + H, pw : pw + W] = x
    return out


def time_split(v):
    """[T, H, W, 2 C] -> [2 T, H, W, C]: channel block j of frame t -> frame 2 t + j."""
    T, H, W, C2 = v.shape
    return v.reshape(T, H, W, 2, C2 // 2).permute(0, 3, 1, 2, 4).reshape(2 * T, H, W, C2 // 2)


def finish(v, flags):
    """The epilogue behind acc + bias + resid: clamp, then the time-split permutation."""
    if flags & CLAMP:
        v = v.clamp(-1.0, 1.0)
    return time_split(v) if flags & TSPLIT else v


def split_x(x):
    """fp32 activations [..., C] -> fp16 planes [..., 3 C] = [hi | hi 2^-12 | lo] (x2v_vae_prep_split_f16 restated in float64 / fp16: hi saturates at the
    fp16 range, lo = fp16(x - hi) with x clamped to twice that range)."""
    o = x.to(F64).clamp(-131008.0, 131008.0)
    hi = o.clamp(-65504.0, 65504.0).to(F16)
    return torch.cat([hi, (hi.to(F64) * 2.0 ** -12).to(F16), (o - hi.to(F64)).to(F16)], dim=-1)


def split_w(w):
    """fp32 weights [..., C] -> fp16 [..., 3 C] = [hi | lo 2^12 | hi] (lightx2v_amd.vae._split16 restated)."""
    hi = w.to(F16)
    return torch.cat([hi, ((w.to(F64) - hi.to(F64)) * 4096.0).to(F16), hi], dim=-1)


# ------------------------------------------------------------------------------------------------------------------- inputs
class Inputs:
    """One seeded case on `device`.  x [kt - 1 + T, H, W, Cin] (the leading kt - 1 frames are the cache; 's2': [T, Hin, Win, Cin]), w [Cout, kt, kh, kw, Cin],
    bias [Cout], resid [T, H, W, Cout] fp32 or None; x and w in fp32 ('f32') or fp16.  t, tol: the float64 result behind the epilogue and the
    per-element bound (family R).  scale (split, family R): 'n3' = N(0, 1) * 3, 'small' = |x| in [1e-3, 0.25] with a random sign."""

    def __init__(self, family, spec, seed=0, device="cpu", scale="n1"):
        assert family in ("I", "R")
        sp = self.spec = spec
        self.family, self.seed, self.device = family, seed, device
        kt, kh, kw = sp.k
        taps = kt * kh * kw
        live = sp.Cin - sp.tail
        self.K = taps * live
        self.stride = 2 if sp.op in S2_OPS else 1
        self.Ho, self.Wo = out_hw(sp)
        F = sp.T + kt - 1
        g = _gen("IR".index(family), ("f32", "f16", "s2", "p32").index(sp.op), sp.T, sp.H, sp.W, sp.Cin, sp.Cout, kt, kh, kw, sp.flags, sp.tail, sp.C, seed)
        ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).to(F32)
        rn = lambda *shape: torch.randn(*shape, generator=g)
        od = F32 if sp.op in ("f32", "p32") else F16
        x, w = torch.zeros(F, sp.H, sp.W, sp.Cin, dtype=od), torch.zeros(sp.Cout, kt, kh, kw, sp.Cin, dtype=od)
        self.x32 = self.w32 = None
        if family == "I":
            assert 8 * 4 * self.K + 400 < 2 ** 24
            x[..., :live], w[..., :live] = ri(-8, 8, F, sp.H, sp.W, live).to(od), ri(-4, 4, sp.Cout, kt, kh, kw, live).to(od)
            bias, resid = ri(-200, 200, sp.Cout), ri(-200, 200, sp.T, self.Ho, self.Wo, sp.Cout)
            self.w_behind = ri(-4, 4, kt, kh, kw, sp.Cin)  # a weight row behind the last one, for the host module's mutation
        else:
            if sp.C:
                C = sp.C
                if scale == "small":
                    x32 = (torch.rand(F, sp.H, sp.W, C, generator=g) * (0.25 - 1e-3) + 1e-3) * (torch.randint(0, 2, (F, sp.H, sp.W, C), generator=g) * 2 - 1)
                else:
                    x32 = rn(F, sp.H, sp.W, C) * {"n1": 1.0, "n3": 3.0}[scale]
                w32 = rn(sp.Cout, kt, kh, kw, C) / math.sqrt(taps * C)
                self.x32, self.w32 = x32.to(device), w32.to(device)
                x[..., : 3 * C], w[..., : 3 * C] = split_x(x32), split_w(w32)
            else:
                x[..., :live], w[..., :live] = rn(F, sp.H, sp.W, live).to(od), (rn(sp.Cout, kt, kh, kw, live) / math.sqrt(self.K)).to(od)
            bias, resid = rn(sp.Cout), rn(sp.T, self.Ho, self.Wo, sp.Cout)
            self.w_behind = rn(kt, kh, kw, sp.Cin) / math.sqrt(self.K)
        self.xp_lead = x[: kt - 1].roll(1, 2).clone() if sp.cache else None  # what a kernel that ignored `cache` would find in xp's leading frames (host mutation)
        self.x, self.w = x.to(device), w.to(device)
        self.bias = bias.to(device) if sp.bias else None
        self.resid = resid.to(device) if sp.resid else None
        self.acc = conv64(self.xpad(), self.w.to(F64), sp.T, self.Ho, self.Wo, self.stride)
        if family == "I" and sp.flags & CLAMP and sp.resid:  # steer the residual, inside [-200, 200], so that acc + bias + resid lands in [-3, 3] where it can
            s = self.acc + (self.bias.to(F64) if sp.bias else 0.0)
            near = ri(-3, 3, sp.T, self.Ho, self.Wo, sp.Cout).to(device).to(F64) - s
            self.resid = torch.where(near.abs() <= 200, near, self.resid.to(F64)).to(F32)
        pre = self.acc.clone()
        if sp.bias:
            pre += self.bias.to(F64)
        if sp.resid:
            pre += self.resid.to(F64)
        self.pre = pre
        self.t = finish(pre, sp.flags)
        self.tol = None
        if family == "R":
            S = conv64(self.xpad().abs(), self.w.to(F64).abs(), sp.T, self.Ho, self.Wo, self.stride)
            if sp.bias:
                S += self.bias.to(F64).abs()
            if sp.resid:
                S += self.resid.to(F64).abs()
            self.tol = finish_perm((self.K + 2) * UNIT * S, sp.flags)
        self._Y = self._Yu = self._tu = self._emu = None

    @property
    def name(self):
        return f"{self.family} {name_of(self.spec)}"

    def xpad(self, x=None):
        return pad_frames((self.x if x is None else x).to(F64), self.spec.k, self.stride)

    def assert_premises(self):
        """Family I: t is an fp32 integer below 2^24.  With the clamp (either family): both sides and the interior occur.  Returns the three shares."""
        sp = self.spec
        if self.family == "I":
            assert float(self.pre.abs().max()) < 2.0 ** 24 and torch.equal(self.pre, self.pre.round()), f"{self.name}: t is not an integer below 2^24"
        if not sp.flags & CLAMP:
            return None
        lo, hi = float((self.pre < -1).double().mean()), float((self.pre > 1).double().mean())
        mid = float((self.pre.abs() < 1).double().mean())
        assert lo > 0 and hi > 0 and mid > 0, f"{self.name}: clamp shares below / inside / above = {lo:.4f} / {mid:.4f} / {hi:.4f}"
        return lo, mid, hi

    # ---- yardsticks (family R)
    def emulations(self):
        """The fp32 emulations of a correct kernel on these operands, made once: the sequential chain and the slab orders."""
        if self._emu is None:
            slabs = sorted(s for s in {32, 64, slab_of(self.spec)} if self.spec.Cin % s == 0)
            self._emu = {"chain": emulate(self, "chain"), **{f"slab{s}": emulate(self, "slab", s) for s in slabs}}
        return self._emu

    def yardstick(self):
        """Y: the largest relative L2 error against t of the emulations."""
        if self._Y is None:
            self._Y = max(rel_l2(e, self.t) for e in self.emulations().values())
            self._emu = {k: None for k in self._emu} if n_out(self.spec) > ON_DEVICE_ABOVE else self._emu  # the large cases keep the number only
        return self._Y

    @property
    def t_unrounded(self):
        """Split operands: the float64 result of the UNROUNDED fp32 activations and weights."""
        if self._tu is None:
            sp = self.spec
            acc = conv64(self.xpad(self.x32), self.w32.to(F64), sp.T, self.Ho, self.Wo, self.stride)
            if sp.bias:
                acc += self.bias.to(F64)
            if sp.resid:
                acc += self.resid.to(F64)
            self._tu = finish(acc, sp.flags)
        return self._tu

    def yardstick_unrounded(self):
        """Y of the end-to-end split claim: the strictly sequential fp32 chain of an fp32 convolution on the unrounded operands."""
        if self._Yu is None:
            self._Yu = rel_l2(emulate(self, "chain", operands=(self.x32, self.w32)), self.t_unrounded)
        return self._Yu


def finish_perm(v, flags):
    """finish() for a bound: the permutation only (the clamp does not widen a distance)."""
    return time_split(v) if flags & TSPLIT else v


# ------------------------------------------------------------------------------------------------------------------- emulations
STRUCTURAL = ("drop_tap", "drop_last_slab", "slab_twice", "halo_shift", "below_next_frame", "w_row_leak", "bias_shift", "resid_shift", "clamp_before_resid",
              "tsplit_swapped", "cache_from_xp", "tail_not_skipped")  # family I must reject these
PRECISION = ("x_fp16", "acc_fp16", "split_drop")  # family R must reject these
HALO_TW = 32  # tile width of both halo kernels


def applicable(mut, sp):
    """Whether the wrong kernel `mut` can occur at this case."""
    kt, kh, kw = sp.k
    steps = kt * kh * kw * max(1, (sp.Cin - sp.tail) // slab_of(sp))
    edge_only = (sp.H == 1 and kh == 3) or (sp.W == 1 and kw == 3) or (sp.op == "s2" and 2 in (sp.H, sp.W))  # the first and last taps read nothing but the zero border
    return {"drop_tap": True, "drop_last_slab": not edge_only, "slab_twice": steps >= 2 and not edge_only, "halo_shift": kw == 3 and sp.op not in S2_OPS and sp.W >= 2,
            "below_next_frame": sp.op == "s2" and sp.H % 2 == 0 and sp.T >= 2,  # only the stride-2 kernel reads a buffer without a border; odd Hin never reaches the pad row
            "w_row_leak": True, "bias_shift": sp.bias, "resid_shift": sp.resid, "clamp_before_resid": bool(sp.flags & CLAMP) and sp.resid,
            "tsplit_swapped": bool(sp.flags & TSPLIT), "cache_from_xp": sp.cache, "tail_not_skipped": bool(sp.flags & ZERO_TAIL32),
            "x_fp16": sp.op == "f32", "acc_fp16": True, "split_drop": sp.C > 0}[mut]


def _accumulate(xpad, w, T, H, W, stride, order, slab, mut=None, exact=False):
    """fp32 accumulation of the taps in the order (tap, channel): 'chain' one product at a time, 'slab' exact partial dot products over `slab` channels
    (float64, rounded to fp32 once) chained in fp32.  exact (family I, where no step rounds): one float64 matmul per tap, the steps a mutation touches
    rewritten in the tap's operand."""
    Cout, kt, kh, kw, C = w.shape
    acc = torch.zeros(T * H * W, Cout, dtype=F32, device=xpad.device)
    taps = [(dt, dh, dw) for dt in range(kt) for dh in range(kh) for dw in range(kw)]
    step, first, last_step = 0, None, len(taps) * (C // slab if order == "slab" else 1) - 1
    if exact and order == "slab" and mut != "acc_fp16":
        acc, per_tap = acc.to(F64), C // slab
        for tap, (dt, dh, dw) in enumerate(taps):
            v = xpad[dt : dt + T, dh : dh + stride * (H - 1) + 1 : stride, dw : dw + stride * (W - 1) + 1 : stride].reshape(-1, C)
            if tap == 0:
                first = v[:, :slab]
            if mut == "drop_tap" and tap == len(taps) // 2:
                continue
            if mut == "drop_last_slab" and tap == len(taps) - 1:
                v = v.clone()
                v[:, C - slab :] = 0
            if mut == "slab_twice" and 1 // per_tap == tap:  # step 1 reads step 0's buffer
                v = v.clone()
                v[:, (1 % per_tap) * slab : (1 % per_tap + 1) * slab] = first
            acc += v.to(F64) @ w[:, dt, dh, dw].to(F64).T
        return acc.to(F32).view(T, H, W, Cout)
    for tap, (dt, dh, dw) in enumerate(taps):
        v = xpad[dt : dt + T, dh : dh + stride * (H - 1) + 1 : stride, dw : dw + stride * (W - 1) + 1 : stride].reshape(-1, C)
        wt = w[:, dt, dh, dw]
        if order == "chain":
            v32, w32 = v.to(F32).T.contiguous().unsqueeze(2), wt.to(F32).T.contiguous().unsqueeze(1)  # [C, pixels, 1] and [C, 1, Cout]
            for c in range(C):
                acc.addcmul_(v32[c], w32[c])
            continue
        for c0 in range(0, C, slab):
            xs = v[:, c0 : c0 + slab]
            if step == 0:
                first = xs
            if mut == "slab_twice" and step == 1:
                xs = first  # the first step's buffer read again
            skip = (mut == "drop_tap" and tap == len(taps) // 2) or (mut == "drop_last_slab" and step == last_step)
            if not skip:
                acc += (xs.to(F64) @ wt[:, c0 : c0 + slab].to(F64).T).to(F32)
            if mut == "acc_fp16":
                acc = acc.to(F16).to(F32)
            step += 1
    return acc.view(T, H, W, Cout)


def emulate(inp, order="slab", slab=None, mut=None, operands=None):
    """A correct kernel in fp32 torch: the accumulation of _accumulate, then + bias + resid in fp32, the clamp and the time-split.  operands: (x, w)
    to run instead of the case's own (the unrounded fp32 pair of a split case).  mut: one of STRUCTURAL / PRECISION — a subtly WRONG kernel, for the
    host module's rejection tests.  Returns fp32 [T, H, W, Cout] (time-split: [2 T, H, W, Cout / 2])."""
    sp = inp.spec
    kt = sp.k[0]
    slab = slab or slab_of(sp)
    x, w = (inp.x, inp.w) if operands is None else operands
    x, w = x.clone(), w.clone()
    if operands is None and mut != "tail_not_skipped":  # whole slabs of zero padding are no step of the loop: the last slab is the last live one
        live = -(-(sp.Cin - sp.tail) // slab) * slab
        x, w = x[..., :live], w[..., :live]
    if mut == "x_fp16":
        x = x.to(F16).to(x.dtype)
    if mut == "split_drop":
        x[..., sp.C : 2 * sp.C] = 0  # x_hi 2^-12 . w_lo 2^12 never added
    if mut == "cache_from_xp":
        x[: kt - 1] = inp.xp_lead.to(x.device)[..., : x.shape[-1]]
    if mut == "tail_not_skipped":  # what the device buffers hold behind the live channels
        x[..., sp.Cin - sp.tail :], w[..., sp.Cin - sp.tail :] = 3.0, 2.0
    if mut == "w_row_leak":
        w[-1] += inp.w_behind.to(w.dtype).to(w.device)[..., : w.shape[-1]]
    dt_ = F32 if order == "chain" else F64
    xpad = pad_frames(x.to(dt_), sp.k, inp.stride)
    if mut == "below_next_frame":
        xpad[:-1, sp.H] = xpad[1:, 0]  # the row below frame f is frame f + 1's first row in memory
    args = (sp.T, inp.Ho, inp.Wo, inp.stride, order, slab)
    exact = inp.family == "I" and operands is None
    acc = _accumulate(xpad, w.to(dt_), *args, mut=mut, exact=exact)
    if mut == "halo_shift":  # the last tile column reads its halo one pixel to the right
        c0 = (sp.W - 1) // HALO_TW * HALO_TW
        acc[:, :, c0:] = _accumulate(xpad.roll(-1, 2), w.to(dt_), *args, exact=exact)[:, :, c0:]
    bias, resid = inp.bias, inp.resid
    if mut == "bias_shift":
        bias = bias.roll(1)
    if mut == "resid_shift":
        resid = resid.roll(1, -1)
    if bias is not None:
        acc = acc + bias
    if mut == "clamp_before_resid":
        acc = acc.clamp(-1.0, 1.0)
    if resid is not None:
        acc = acc + resid
    out = finish(acc, sp.flags & ~(CLAMP if mut == "clamp_before_resid" else 0))
    if mut == "tsplit_swapped":
        out = out.view(sp.T, 2, *out.shape[1:]).flip(1).reshape(out.shape)
    return out


# ------------------------------------------------------------------------------------------------------------------- acceptance
class Reject(AssertionError):
    def __init__(self, criterion, msg):
        super().__init__(msg)
        self.criterion = criterion


class Case:
    """The checks of one test: (case, body, what, rule, numbers, elements compared)."""

    def __init__(self, name, record=True):
        self.name, self.record, self.rows = name, record, []

    def _row(self, inp, body_, what, rule, nums, n):
        self.rows.append((inp.name, body_, what, rule, nums, n))
        if self.record:
            from tests.util import record as rec

            rec(f"vae_conv_fp64 {self.name} {inp.name} {body_} {what}", rule=rule, elements=n, **nums)

    def check(self, got, inp, body_="", what=""):
        return self.check_exact(got, inp, body_, what) if inp.family == "I" else self.check_bound(got, inp, body_, what)

    def check_exact(self, got, inp, body_="", what="", want=None):
        """Family I: got (fp32) equals t on every element."""
        want = (inp.t if want is None else want).to(F32)
        tag = f"{self.name} {inp.name} {body_} {what}"
        if got.shape != want.shape or got.dtype != F32:
            raise Reject("shape", f"{tag}: {tuple(got.shape)} {got.dtype} vs {tuple(want.shape)}")
        want = want.to(got.device)
        ne = ~((got == want) | (torch.isnan(got) & torch.isnan(want)))
        bad = int(ne.sum())
        self._row(inp, body_, what, "exact", {"unequal": bad}, got.numel())
        if bad:
            idx = ne.nonzero()
            i = tuple(int(v) for v in idx[0])
            lo, hi = idx.min(0).values.tolist(), idx.max(0).values.tolist()
            raise Reject("exact", f"{tag}: {bad} of {got.numel()} elements differ from the float64 result; first at {i}: got {float(got[i])} want {float(want[i])}; "
                                  f"indices span {lo} .. {hi}")
        return 0

    def check_bound(self, got, inp, body_="", what="", t=None, tol=None, Y=None):
        """Family R: |got - t| <= tol on every element and relL2(got, t) <= 1.5 Y.  tol = None: the yardstick alone (the end-to-end split claim)."""
        t = inp.t if t is None else t
        tol = inp.tol if (tol is None and t is inp.t) else tol
        Y = inp.yardstick() if Y is None else Y
        tag = f"{self.name} {inp.name} {body_} {what}"
        g = got.to(t.device).to(F64)
        if g.shape != t.shape:
            raise Reject("shape", f"{tag}: {tuple(g.shape)} vs {tuple(t.shape)}")
        if not bool(torch.isfinite(g).all()):
            raise Reject("finite", f"{tag}: non-finite output")
        err = (g - t).abs()
        worst = 0.0
        if tol is not None:
            ratio = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
            worst = float(ratio.max())
        r = rel_l2(g, t)
        self._row(inp, body_, what, "bound", {"bounded": tol is not None, "d_over_bound": worst, "rel_l2": r, "Y": Y, "rel_l2_over_Y": r / Y if Y > 0 else (0.0 if r == 0 else math.inf)}, g.numel())
        if worst > 1.0:
            i = tuple(int(v) for v in (ratio == ratio.max()).nonzero()[0])
            over = ratio > 1.0
            raise Reject("bound", f"{tag}: {int(over.sum())} of {g.numel()} elements ({float(over.double().mean()):.2%}) outside the bound; worst |d| / bound {worst:.3f} at {i}: "
                                  f"got {float(g[i]):.9g} ref {float(t[i]):.9g} bound {float(tol[i]):.3g}")
        if r > MARGIN * Y:
            raise Reject("yardstick", f"{tag}: relL2 {r:.3e} > {MARGIN} x Y = {MARGIN * Y:.3e} (relL2 / Y = {r / Y if Y > 0 else math.inf:.3f})")
        return worst

    @property
    def worst_bound(self):
        return max((r[4]["d_over_bound"] for r in self.rows if r[3] == "bound"), default=0.0)

    @property
    def worst_yardstick(self):
        return max((r[4]["rel_l2_over_Y"] for r in self.rows if r[3] == "bound"), default=0.0)

    def table(self):
        return [f"{self.name:<22} {case:<58} {body_:<22} {what:<14} " +
                ((f"d/bound {nums['d_over_bound']:5.3f}" if nums["bounded"] else "d/bound     -") + f"  relL2 {nums['rel_l2']:.3e}  Y {nums['Y']:.3e}  relL2/Y {nums['rel_l2_over_Y']:5.3f}" if rule == "bound" else f"unequal {nums['unequal']}") +
                f"  n={n}" for case, body_, what, rule, nums, n in self.rows]

    def header(self):
        nb, ne = sum(r[3] == "bound" for r in self.rows), sum(r[3] == "exact" for r in self.rows)
        return (f"# {self.name}: {len(self.rows)} checks ({ne} bit for bit, {nb} bounded)" +
                (f", largest |d| / bound = {self.worst_bound:.3f}, largest relL2 / Y = {self.worst_yardstick:.3f}" if nb else ""))


# ------------------------------------------------------------------------------------------------------------------- the GPU module's lists
PIXEL_TAILS = ((1, 1), (17, 15), (16, 16), (257, 1), (23, 11), (24, 11))  # H x W = 1, 255, 256, 257 pixels against the 256-pixel tile, and W = 11 with 253 / 264: a tile that spans image rows
COUT_TAILS = (3, 6, 40, 100, 132)  # element-wise stores, a masked weight-row tail inside the last 32-block, a second column tile of four rows
NF_COUTS = (32, 64, 96, 128)  # NF 1, 2, 3, 4
EPILOGUES = ((0, False, False), (0, True, False), (0, True, True), (CLAMP, True, True))  # (flags, bias?, resid?); the time-split + clamp has cases of its own

# per-tap fp32 body
F32_INSTANCES = [Spec("f32", 2, 9, 11, cin, cout, (1, 3, 3)) for cout in NF_COUTS for cin in (48, 64)]  # NF 1..4 x KC 16, 32
F32_K_LOOP = [Spec("f32", 2, 9, 11, cin, 40, k) for k, cin in (((1, 1, 1), 16), ((1, 1, 1), 32), ((1, 1, 1), 64), ((1, 1, 1), 48), ((3, 1, 1), 32), ((1, 3, 3), 16), ((1, 3, 3), 32),
                                                               ((3, 3, 3), 32), ((3, 3, 3), 48))]  # 1, 1, 2, 3, 3, 9, 9, 27 and 81 steps
F32_PIXELS = [Spec("f32", 2, h, w, 32, 32, (1, 3, 3)) for h, w in PIXEL_TAILS]
F32_COUTS = [Spec("f32", 2, 9, 11, 32, cout, (1, 3, 3)) for cout in COUT_TAILS]
F32_GRIDS = [Spec("f32", 2, 24, 11, 32, 132, (1, 3, 3)), Spec("f32", 1, 9, 11, 32, 32, (1, 3, 3)), Spec("f32", 5, 9, 11, 32, 64, (3, 1, 1)),
             Spec("f32", 9, 5, 7, 16, 100, (1, 1, 1)), Spec("f32", 13, 5, 7, 32, 40, (1, 3, 3))]  # 8, 1, 5, 9 and 13 workgroups: % 8 = 0, 1, 5, 1, 5
F32_EPILOGUES = [Spec("f32", 2, 9, 11, 32, cout, (3, 3, 3), flags=f, bias=b, resid=r) for cout in (40, 6) for f, b, r in EPILOGUES]
F32_TSPLIT = [Spec("f32", 2, 9, 11, cin, cout, (3, 1, 1), flags=TSPLIT | CLAMP) for cin, cout in ((32, 64), (48, 40), (64, 192))] + \
             [Spec("f32", 2, 9, 11, 32, 64, (3, 1, 1), flags=TSPLIT)]
F32_SPECS = F32_INSTANCES + F32_K_LOOP + F32_PIXELS + F32_COUTS + F32_GRIDS + F32_EPILOGUES + F32_TSPLIT
QK_CASES = ((32, 48), (48, 32), (64, 80))  # (c, npad): q . k^T with cin = c inside a 3 c pixel
PV_CASES = ((32, 64), (48, 96))  # (npad, C): scores . V^T with Cin = npad
POLYPHASE = ((2, 6, 8, 32, 40), (2, 7, 9, 32, 32), (2, 6, 9, 48, 96), (2, 7, 8, 16, 6))  # (T, Hin, Win, C, Cout): even and odd H and W

# per-tap 16-bit body: by flag, by kernel size, by width below the 16-pixel threshold, by the time-split
PT16_SPECS = ([Spec("f16", 2, 9, 11, cin, cout, (1, 3, 3)) for cout in NF_COUTS for cin in (64, 192)] +
              [Spec("f16", 2, 9, 11, cin, 40, (3, 1, 1)) for cin in (64, 192)] +
              [Spec("f16", 2, 9, 20, 64, cout, (3, 3, 3), flags=PER_TAP) for cout in (96, 40)] +
              [Spec("f16", 2, 9, 20, cin, cout, (3, 1, 1), flags=TSPLIT | CLAMP) for cin, cout in ((64, 64), (192, 192))] + [Spec("f16", 2, 9, 20, 64, 40, (3, 1, 1), flags=TSPLIT)] +
              [Spec("f16", 2, h, w, 64, 32, (1, 3, 3), flags=PER_TAP if w >= 16 else 0) for h, w in PIXEL_TAILS] + [Spec("f16", 2, 9, 11, 64, cout, (1, 3, 3)) for cout in COUT_TAILS] +
              [Spec("f16", 2, 9, 11, 64, 40, (1, 3, 3), flags=f, bias=b, resid=r) for f, b, r in EPILOGUES])

# 64-pixel halo body (8 x 32 tile)
HALO64_HW = tuple((h, w) for h in (8, 9, 17) for w in (16, 32, 33, 70))
HALO64_SPECS = ([Spec("f16", 2, 9, 33, 64, cout, (3, 3, 3), flags=0 if body_of("f16", 33, 64, cout, (3, 3, 3), 0).startswith("halo64") else HALO64) for cout in NF_COUTS + (40, 100, 6)] +
                [Spec("f16", 2, 9, 33, cin, 40, (kt, 3, 3)) for cin in (64, 128, 192) for kt in (1, 3)] +  # 9, 27, 18, 54, 27, 81 steps through the ring of four
                [Spec("f16", 2, h, w, 64, 64, (1, 3, 3)) for h, w in HALO64_HW] +
                [Spec("f16", 2, 9, 33, 64, 40, (1, 3, 3), flags=f, bias=b, resid=r) for f, b, r in EPILOGUES])

# 128-pixel body (16 x 32 tile): NCB 6 / 8 / 1; nslabs 1, 2, 3, 4, 9 from kt and the zero-tail flag
_SLABS = ((64, 1, True), (64, 1, False), (64, 3, True), (128, 1, False), (128, 3, True))  # (Cin, kt, zero tail) -> 1, 2, 3, 4, 9 slabs
HALO128_HW = tuple((h, w) for h in (16, 17, 33) for w in (16, 32, 33, 70))
HALO128_SPECS = ([Spec("f16", 1, 17, 20, cin, cout, (kt, 3, 3), flags=ZERO_TAIL32 if tail else 0, tail=32 if tail else 0) for cout in (96, 128) for cin, kt, tail in _SLABS] +
                 [Spec("f16", 1, 17, 20, cin, cout, (kt, 3, 3), flags=ZERO_TAIL32 if tail else 0, tail=32 if tail else 0) for cout, (cin, kt, tail) in
                  ((192, _SLABS[0]), (192, _SLABS[2]), (256, _SLABS[1]), (256, _SLABS[4]), (3, _SLABS[0]), (4, _SLABS[2]), (12, _SLABS[3]), (16, _SLABS[4]), (3, _SLABS[1]))] +
                 [Spec("f16", 2, h, w, 64, cout, (1, 3, 3)) for (h, w), cout in zip(HALO128_HW, (96, 128, 12, 192, 256, 3, 128, 96, 4, 96, 16, 128))] +
                 [Spec("f16", 1, 17, 33, 64, cout, (3, 3, 3), flags=f, bias=b, resid=r) for cout in (96, 3) for f, b, r in EPILOGUES])
HALO128_CACHED = [Spec("f16", 4, 17, 20, cin, cout, (3, 3, 3), flags=CLAMP | (ZERO_TAIL32 if tail else 0), cache=True, tail=tail)
                  for cin, cout, tail in ((64, 96, 0), (64, 128, 32), (128, 192, 32), (64, 3, 0), (64, 256, 0))]
FRAME_BATCH = Spec("f16", 3, 17, 33, 64, 96, (3, 3, 3))

# stride-2 body (16 x 16 output tile x 96 couts): one output, exact tiles, the zero row / column that is read and the odd row / column that is not
S2_SPECS = [Spec("s2", 2, h, w, cin, cout) for (h, w), cin, cout in zip(((2, 2), (3, 3), (32, 35), (33, 34), (34, 33), (35, 32), (2, 35), (34, 3), (32, 32), (35, 35)),
                                                                         (32, 96, 32, 96, 32, 96, 96, 32, 96, 32), (4, 96, 100, 192, 192, 4, 100, 96, 96, 100))]
S2_SPLIT = [Spec("s2", 2, h, w, 96, cout, C=32) for h, w, cout in ((33, 34, 96), (34, 33, 4))] + [Spec("s2", 2, 32, 35, 64, 100, tail=16, C=16)]

# split, end to end: one case per 16-bit body
SPLIT_E2E = (Spec("f16", 2, 9, 11, 320, 96, (3, 3, 3), tail=32, C=96),  # per-tap (W < 16)
             Spec("f16", 2, 9, 33, 192, 40, (3, 3, 3), C=64),  # 64-pixel halo
             Spec("f16", 2, 17, 33, 320, 96, (3, 3, 3), flags=ZERO_TAIL32, tail=32, C=96),  # 128-pixel, the decoder's 96-channel stage: nine slabs and a skipped tenth
             Spec("s2", 2, 33, 34, 96, 96, C=32))
SPLIT_SCALES = ("n3", "small")

ALL_SPECS = F32_SPECS + PT16_SPECS + HALO64_SPECS + HALO128_SPECS + HALO128_CACHED + [FRAME_BATCH] + S2_SPECS + S2_SPLIT + list(SPLIT_E2E)
# K = 27 * 512 = 13824 (s2: 9 * 512), family I: a step dropped, doubled or read from the wrong slot anywhere in a long loop changes the integer
DEEP_SPECS = (Spec("f32", 1, 5, 7, 512, 32, (3, 3, 3)), Spec("f16", 1, 5, 20, 512, 32, (3, 3, 3), flags=PER_TAP), Spec("f16", 1, 9, 20, 512, 32, (3, 3, 3)),
              Spec("f16", 1, 17, 20, 512, 96, (3, 3, 3)), Spec("f16", 1, 17, 20, 512, 128, (3, 3, 3)), Spec("s2", 1, 6, 8, 512, 96))
LARGEST_K = max(sp.k[0] * sp.k[1] * sp.k[2] * (sp.Cin - sp.tail) for sp in ALL_SPECS + list(DEEP_SPECS))


def persistent_specs(cus, which):
    """cus + 1 and 2 cus + 3 tiles (at least) on the persistent grids, from the smallest Cin: the 64-pixel halo body, and the 128-pixel body with kt = 3 and
    the separate cache so that one workgroup walks from a frame-0 tile (two cached frames) to later frames' tiles (one, none)."""
    out = []
    for tiles in (cus + 1, 2 * cus + 3):
        if which == "halo64":  # 17 x 33: 3 x 2 tiles of 8 x 32 per frame
            out.append(Spec("f16", -(-tiles // 6), 17, 33, 64, 32, (1, 3, 3)))
        else:  # 33 x 33: 3 x 2 tiles of 16 x 32 per frame
            out.append(Spec("f16", -(-tiles // 6), 33, 33, 64, 96, (3, 3, 3), cache=True))
    return out
