"""x2v_conv2d_bf16 and x2v_taehv_clamp_bf16 (csrc/taehv.hip) against float64, by the method of tests/test_gpu_vae_conv_fp64.py, at the smallest shapes at which each
edge exists: every (Cin, Cout) pair of the TAEHV decoder (16 -> 256, 2 x 256 -> 256, 256 -> 256, 256 -> 128, 2 x 128 -> 128, 128 -> 128, 128 -> 64, 2 x 64 -> 64,
64 -> 64, 64 -> 3), the 1x1 forms (256 -> 256, 128 -> 256, 64 -> 128), widths 1, 2, 7, 17 (= the 16-pixel tile + 1) and 33, heights 1, 3 and 17, T = 1 and 3, the
two-source form with zero memory, with a carried memory frame and with t - 1 inside the buffer, upsample-read at odd output sizes, the time-split order, every
epilogue, the head's channel-first store with a trim offset, and Clamp.

Operands are windows inside LOUD buffers (the frames in front of and behind the window — frame -1 of the two-source form included —, a ring of pixels around every
frame, the channels behind Cin of every pixel, the weight rows around the weights hold 2^15), outputs sit inside NaN-guarded allocations, and every operand must come
back unchanged.

The float64 reference: acc = F.conv2d in float64 of the operands the contract names (include/x2v.h), then the epilogue with its bf16 roundings (RN):
v = RN(acc + bias); resid: v = RN(v + resid); head: v = RN(2 v - 1); ReLU.

Family I (x in [-8, 8], w in [-4, 4], bias and resid in [-200, 200], all integers): every product and partial sum is an integer below 2^24 (asserted), exact in fp32
in any order, so the output must EQUAL the reference on every element.

Family R (x ~ N(0, 1), w ~ N(0, 1) / sqrt(K), bias, resid ~ N(0, 1), rounded to bf16; K = taps x channels summed): a bf16 x bf16 product has 16 significant bits and
is exact in fp32.  Summing K exact products and the bias in fp32 in ANY order makes at most K rounding errors, each at most u |partial sum| <= u S with
S = sum |x w| + |bias|; first order gives gamma_K = K u / (1 - K u) <= (K + 1) u for K u < 1e-3.  With u = 2^-23 (twice the round-to-nearest unit, so that a matrix
unit that truncates when it aligns addends is covered, as in tests/vae_conv_ref.py) the accumulator differs from the float64 one by at most d0 = (K + 1) 2^-23 S.
A rounding RN(t') of a value t' within d of the reference's t obeys |RN(t') - RN(t)| <= d + ulp(|RN(t)| + d) (half an ulp at either end), so through the epilogue
d1 = d0 + ulp(|v1| + d0), resid: d2 = d1 + ulp(|v2| + d1), head: d3 = 2 d2 + ulp(|v3| + 2 d2), ulp(a) = 2^(floor(log2 a) - 7); ReLU is 1-Lipschitz.  The bound holds
on EVERY element.  Second rule: the relative L2 error against the float64 result WITHOUT the roundings is at most 1.5 x the same figure of a float32 F.conv2d of the
same operands pushed through the same roundings — no constant comes from the kernel."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
BF, F64 = torch.bfloat16, torch.float64
LOUD, GUARD = 32768.0, 256
RELU, UPS, TWO, HEAD = 1, 2, 4, 8


def rn(v):
    """One rounding to bf16 of a float64 tensor (through fp32: exact for the integers of family I)."""
    return v.float().to(BF).to(F64)


def ulp(a):
    return torch.exp2(torch.floor(torch.log2(a.clamp_min(2.0**-126))) - 7)


def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 17) % (2**31 - 1)
    return torch.Generator().manual_seed(seed)


class Conv:
    """One seeded call: operands (CPU, bf16-exact values held in float64), the float64 reference, the bound and the fp32 yardstick."""

    def __init__(self, family, T, H, W, Cin, Cout, k=3, flags=0, bias=True, resid=False, mem="zero", tsplit=1, trim=0, channel_first=False):
        self.__dict__.update(family=family, T=T, H=H, W=W, Cin=Cin, Cout=Cout, k=k, flags=flags, tsplit=tsplit, trim=trim, channel_first=channel_first)
        up, two = 1 if flags & UPS else 0, bool(flags & TWO)
        self.Hin, self.Win, self.Ctot = (H + up) >> up, (W + up) >> up, (2 if two else 1) * Cin
        K = self.K = k * k * self.Ctot
        g = _gen("IR".index(family), T, H, W, Cin, Cout, k, flags, tsplit, trim, bias, resid, len(mem))
        if family == "I":
            assert 8 * 4 * K + 400 < 2**24
            ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).to(F64)
            x, w, b, r, m = ri(-8, 8, T, self.Hin, self.Win, Cin), ri(-4, 4, Cout, k, k, self.Ctot), ri(-200, 200, Cout), ri(-200, 200, T, H, W, Cout), ri(-8, 8, self.Hin, self.Win, Cin)
        else:
            rr = lambda *s: torch.randn(*s, generator=g).to(BF).to(F64)
            x, w, b, r, m = rr(T, self.Hin, self.Win, Cin), (torch.randn(Cout, k, k, self.Ctot, generator=g) / math.sqrt(K)).to(BF).to(F64), rr(Cout), rr(T, H, W, Cout), rr(self.Hin, self.Win, Cin)
        self.x, self.w, self.bias, self.resid, self.mem = x, w, (b if bias else None), (r if resid else None), (m if two and mem == "carried" else None)
        self.name = f"{family} {T}x{H}x{W} {'2x' if two else ''}{Cin}->{Cout} k{k} f{flags} ts{tsplit} trim{trim}" + (" resid" if resid else "") + (" mem" if self.mem is not None else "") + (" cf" if channel_first else "")

    def _operand(self, dt):
        """[T, Ctot, H, W]: the upsampled frames, and behind them the frames t - 1 (mem or zero in front)."""
        x = self.x.to(dt).permute(0, 3, 1, 2)
        if self.flags & TWO:
            first = torch.zeros_like(x[:1]) if self.mem is None else self.mem.to(dt).permute(2, 0, 1)[None]
            x = torch.cat([x, torch.cat([first, x[:-1]], 0)], 1)
        if self.flags & UPS:
            x = x.repeat_interleave(2, -2).repeat_interleave(2, -1)[..., : self.H, : self.W]
        return x

    def _epilogue(self, acc, bound=None):
        """acc [T, H, W, Cout] float64 -> the output layout; with `bound` (d0) also the per-element bound."""
        d = bound
        v = rn(acc + (self.bias if self.bias is not None else 0.0))
        if d is not None:
            d = d + ulp(v.abs() + d)
        if self.resid is not None:
            v = rn(v + self.resid)
            if d is not None:
                d = d + ulp(v.abs() + d)
        if self.flags & HEAD:
            v = rn(2 * v - 1)
            if d is not None:
                d = 2 * d + ulp(v.abs() + 2 * d)
        if self.flags & RELU:
            v = v.clamp_min(0.0)
        return self._layout(v), (None if d is None else self._layout(d))

    def _layout(self, v):
        T, H, W, Cout = v.shape
        v = v[self.trim :]
        if self.tsplit > 1:
            v = v.reshape(T - self.trim, H, W, self.tsplit, Cout // self.tsplit).permute(0, 3, 1, 2, 4).reshape((T - self.trim) * self.tsplit, H, W, Cout // self.tsplit)
        return v.permute(3, 0, 1, 2).contiguous() if self.channel_first else v.contiguous()

    def reference(self):
        w = self.w.permute(0, 3, 1, 2)
        acc = F.conv2d(self._operand(F64), w, None, padding=self.k // 2).permute(0, 2, 3, 1)
        if self.family == "I":
            assert float(acc.abs().max()) + 400 < 2**24 and torch.equal(acc, acc.round())
            return self._epilogue(acc)[0], None, None, None
        S = F.conv2d(self._operand(F64).abs(), w.abs(), None, padding=self.k // 2).permute(0, 2, 3, 1) + (self.bias.abs() if self.bias is not None else 0.0)
        ref, tol = self._epilogue(acc, (self.K + 1) * 2.0**-23 * S)
        # the unrounded float64 result, and the float32 F.conv2d of the same operands pushed through the same roundings
        exact = acc + (self.bias if self.bias is not None else 0.0) + (self.resid if self.resid is not None else 0.0)
        exact = self._layout((2 * exact - 1 if self.flags & HEAD else exact).clamp_min(0.0 if self.flags & RELU else -math.inf))
        acc32 = F.conv2d(self._operand(torch.float32), w.float(), None, padding=self.k // 2).permute(0, 2, 3, 1)
        y32 = self._epilogue(acc32.to(F64))[0]  # (the bias joins in float64: one fp32 addition less than a kernel makes, the stricter yardstick)
        return ref, tol, exact, float((y32 - exact).norm() / exact.norm())


def run(lib, c):
    """The call on the device inside loud / guarded buffers -> the output (CPU float64) in the reference's layout."""
    dev = "cuda"
    ps = c.Cin + 8
    xbig = torch.full((c.T + 2, c.Hin + 2, c.Win + 2, ps), LOUD, dtype=BF, device=dev)
    xwin = xbig[1 : c.T + 1, 1 : c.Hin + 1, 1 : c.Win + 1, : c.Cin]
    xwin.copy_(c.x.to(BF))
    wbig = torch.full((c.Cout + 2, c.k, c.k, c.Ctot), LOUD, dtype=BF, device=dev)
    wbig[1 : c.Cout + 1] = c.w.to(BF).to(dev)
    mbig = mem = None
    if c.mem is not None:
        mbig = torch.full((c.Hin + 2, c.Win + 2, ps), LOUD, dtype=BF, device=dev)
        mem = mbig[1 : c.Hin + 1, 1 : c.Win + 1, : c.Cin]
        mem.copy_(c.mem.to(BF))
    bias = None if c.bias is None else c.bias.to(BF).to(dev)
    To, Cb = (c.T - c.trim) * c.tsplit, c.Cout // c.tsplit
    n = To * c.H * c.W * Cb
    whole = torch.full((GUARD + n + GUARD,), float("nan"), dtype=BF, device=dev)
    flat = whole[GUARD : GUARD + n]
    resid = rwhole = None
    if c.resid is not None:
        rwhole = torch.full((GUARD + n + GUARD,), LOUD, dtype=BF, device=dev)
        resid = rwhole[GUARD : GUARD + n].view(To, c.H, c.W, Cb)
        resid.copy_(c.resid.to(BF))
    keep = [(t, t.clone()) for t in (xbig, wbig, mbig, bias, rwhole) if t is not None]
    if c.channel_first:
        out = flat.view(Cb, To, c.H, c.W)
        lib.conv2d_bf16(xwin, wbig[1 : c.Cout + 1], out, c.H, c.W, bias=bias, mem=mem, flags=c.flags, tsplit=c.tsplit, frame_trim=c.trim,
                        out_strides=(out.stride(1), out.stride(2), out.stride(3), out.stride(0)))
    else:
        out = flat.view(To, c.H, c.W, Cb)
        lib.conv2d_bf16(xwin, wbig[1 : c.Cout + 1], out, c.H, c.W, bias=bias, resid=resid, mem=mem, flags=c.flags, tsplit=c.tsplit, frame_trim=c.trim)
    torch.cuda.synchronize()
    assert torch.isnan(whole[:GUARD]).all() and torch.isnan(whole[GUARD + n :]).all(), f"{c.name}: wrote outside its output"
    for t, before in keep:
        assert torch.equal(t.view(torch.int16), before.view(torch.int16)), f"{c.name}: an operand was modified"
    assert not torch.isnan(out).any(), f"{c.name}: output elements left unwritten"
    return out.cpu().to(F64)


def check(lib, c):
    from tests.util import record

    ref, tol, exact, y32 = c.reference()
    got = run(lib, c)
    assert got.shape == ref.shape
    if c.family == "I":
        ne = got != ref
        assert not ne.any(), f"{c.name}: {int(ne.sum())} of {got.numel()} elements differ from the float64 result; first at {tuple(int(i) for i in ne.nonzero()[0])}"
        return
    err = (got - ref).abs()
    worst = float((err / tol).max())
    e = float((got - exact).norm() / exact.norm())
    print(f"{c.name}: worst |d| / bound {worst:.3f}; relL2 vs float64 {e:.3e}, float32 F.conv2d {y32:.3e} (ratio {e / y32:.3f})")
    record(f"taehv_conv_fp64 {c.name}", d_over_bound=worst, rel_l2=e, rel_l2_f32=y32)
    assert worst <= 1.0, f"{c.name}: {int((err > tol).sum())} of {got.numel()} elements outside the bound; worst |d| / bound {worst:.3f}"
    assert e <= 1.5 * y32, f"{c.name}: relL2 {e:.3e} > 1.5 x {y32:.3e} (float32 F.conv2d)"


@pytest.fixture(scope="module")
def lib():
    from lightx2v_amd import lib as L

    L.init()
    return L


# (T, H, W, Cin, Cout, keyword arguments): the decoder's pairs, each at another edge of the pixel tile / frame count / epilogue
SPECS = {
    "first 16->256 relu, one pixel": (1, 1, 1, 16, 256, dict(flags=RELU)),
    "first 16->256 relu, 3 frames x 3 x 17": (3, 3, 17, 16, 256, dict(flags=RELU)),
    "mem0 2x256->256 zero memory, t-1 inside": (3, 3, 7, 256, 256, dict(flags=RELU | TWO)),
    "mid 256->256 relu": (1, 3, 2, 256, 256, dict(flags=RELU)),
    "tail 256->256 resid relu": (1, 1, 17, 256, 256, dict(flags=RELU, resid=True)),
    "stage 256->128 upsample-read 3x7": (1, 3, 7, 256, 128, dict(flags=UPS, bias=False)),
    "mem0 2x128->128 carried memory": (1, 3, 17, 128, 128, dict(flags=RELU | TWO, mem="carried")),
    "plain 128->128 bias only": (3, 1, 2, 128, 128, dict()),
    "tail 128->128 resid, no relu": (1, 3, 7, 128, 128, dict(resid=True)),
    "stage 128->64 upsample-read 3x17": (3, 3, 17, 128, 64, dict(flags=UPS, bias=False)),
    "mem0 2x64->64 carried memory and t-1 inside": (3, 3, 17, 64, 64, dict(flags=RELU | TWO, mem="carried")),
    "mem0 2x64->64 one pixel wide": (3, 3, 1, 64, 64, dict(flags=RELU | TWO)),
    "stage 64->64 upsample-read relu 17x33": (1, 17, 33, 64, 64, dict(flags=UPS | RELU, bias=False)),
    "tail 64->64 resid relu": (3, 3, 17, 64, 64, dict(flags=RELU, resid=True)),
    "head 64->3 channel-first, trim 1": (3, 3, 17, 64, 3, dict(flags=HEAD, trim=1, channel_first=True)),
    "head 64->3 channel-first, no x2-1, trim 2 of 3": (3, 17, 7, 64, 3, dict(trim=2, channel_first=True)),
    "head 64->3 channels-last": (1, 3, 2, 64, 3, dict(flags=HEAD)),
    "tgrow 1x1 256->256": (3, 3, 7, 256, 256, dict(k=1, bias=False)),
    "tgrow 1x1 128->256 time-split": (3, 1, 17, 128, 256, dict(k=1, bias=False, tsplit=2)),
    "tgrow 1x1 64->128 time-split": (1, 3, 2, 64, 128, dict(k=1, bias=False, tsplit=2)),
    "tgrow 1x1 64->128 time-split 17x33": (3, 17, 33, 64, 128, dict(k=1, bias=False, tsplit=2)),
    "general 40->20 (channel and cout tails)": (3, 3, 17, 40, 20, dict(flags=RELU)),
}


@pytest.mark.parametrize("family", ["I", "R"])
@pytest.mark.parametrize("spec", sorted(SPECS))
def test_conv2d_bf16(lib, spec, family):
    T, H, W, Cin, Cout, kw = SPECS[spec]
    check(lib, Conv(family, T, H, W, Cin, Cout, **kw))


def test_two_source_memory_forms_agree(lib):
    """Frames 1 .. 2 of a 3-frame call equal a 2-frame call on x[1:] with x[0] as the carried memory, bit for bit (what the chunked decode relies on), and
    differ from the same call with zero memory."""
    c = Conv("R", 3, 3, 17, 64, 64, flags=RELU | TWO)
    whole = run(lib, c)
    tail = Conv("R", 2, 3, 17, 64, 64, flags=RELU | TWO, mem="carried")
    tail.x, tail.w, tail.bias, tail.mem = c.x[1:], c.w, c.bias, c.x[0]
    assert torch.equal(run(lib, tail), whole[1:])
    tail.mem = None
    assert not torch.equal(run(lib, tail)[0], whole[1])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_clamp(lib, dtype):
    """x2v_taehv_clamp_bf16 vs float64 tanh with the three roundings behind the input's: RN(RN(tanh(RN(RN(z) / 3))) * 3), z ~ 2.5 N(0, 1) (the curved range) on a
    strided [16, T, h, w] view.  The kernel's division is correctly rounded and its fp32 tanh is within a few 2^-24: against the 2^-9 half-spacing of bf16 a share of
    ~2^-13 of the tanh roundings can land on the other side, one ulp away — at most 2e-3 of the elements (the project's share for rounding-boundary flips) may differ,
    none by more than one bf16 ulp (2^-7 relative)."""
    from tests.util import record

    g = torch.Generator().manual_seed(5)
    T, h, w = 3, 5, 7
    big = (torch.randn(16, T + 2, h, w, generator=g) * 2.5).to(dtype).cuda()
    z = big[:, 1 : T + 1]
    whole = torch.full((GUARD + T * h * w * 16 + GUARD,), float("nan"), dtype=BF, device="cuda")
    out = whole[GUARD:-GUARD].view(T, h, w, 16)
    before = big.clone()
    lib.taehv_clamp(z, out)
    torch.cuda.synchronize()
    assert torch.isnan(whole[:GUARD]).all() and torch.isnan(whole[-GUARD:]).all() and torch.equal(big, before)
    ref = rn(rn(torch.tanh(rn(rn(z.cpu().to(F64)) / 3))) * 3).permute(1, 2, 3, 0)
    got = out.cpu().to(F64)
    share = float((got != ref).double().mean())
    worst = float(((got - ref).abs() / ref.abs().clamp_min(2.0**-126)).max())
    print(f"clamp {dtype}: share of unequal elements {share:.2e}, worst relative difference {worst:.3e}")
    record(f"taehv_clamp {dtype}", share_unequal=share, worst_rel=worst)
    assert float(ref.abs().max()) > 2.5 and float(ref.abs().min()) < 0.1
    assert share <= 2e-3 and worst <= 2.0**-7
