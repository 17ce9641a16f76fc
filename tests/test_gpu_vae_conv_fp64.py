"""Every VAE convolution kernel body — vae.hip's per-tap kernel in fp32 (NF 1..4 x KC 16, 32) and fp16 (NF 1..4), its 64-pixel halo kernel (NF 1..4),
vae16g.hip's 128-pixel kernel (96-, 128- and 16-cout forms) and vae_enc.hip's stride-2 kernel — at the smallest shapes at which each edge exists,
against the float64 references of tests/vae_conv_ref.py: the K loop at 1..81 steps and 1..9 slabs, pixel tiles that end inside an image row, cout
tails, the XCD remap at ragged workgroup counts, every epilogue, the GEMM roles of the attention block, the encoder's polyphase stride-2 path, the
separate cache with a persistent workgroup walking from a frame-0 tile to later frames, the zero-tail flag over LOUD values, and the hi/lo split end
to end.  Family I (integers) must EQUAL the float64 result on every element, family R must hold the derived per-element bound on every element and
relL2 <= 1.5 Y; tests/test_vae_conv_ref_host.py shows which subtly wrong kernels this rejects.

Every call reads its operands as windows of loud buffers (channels >= Cin of every pixel, the frames in front of and behind the window, the weight
row's tail behind taps * Cin and the rows around the weights hold 3e4) and writes a view inside a NaN-filled allocation whose guards are checked
afterwards; operands, residual and cache must come back unchanged, so the zero border stays zero.  The entries are called through lib._lib
directly (the wrappers take dense weights).  The suite assumes the default dispatch and forces kernels by flag; X2V_VAE_CONV_PARITY_TABLE names a
file to write the table of measured ratios to (profiles/vae_conv_fp64_parity.txt is one run's)."""
import os

import pytest
import torch

from tests import vae_conv_ref as V

pytestmark = pytest.mark.gpu
LOUD = 3.0e4  # exact in fp16
GUARD = 256  # floats in front of and behind every output (a multiple of 4: the view stays 16-byte aligned)
CASES, _INPUTS = {}, {}


@pytest.fixture(scope="module")
def lib():
    from lightx2v_amd import lib as L

    if L._VCONV16_FORCE != 0:
        pytest.fail("X2V_VAE_CONV16 is set: this module assumes the default dispatch of x2v_vae_conv_f16 and forces kernels by flag")
    L.init()
    yield L
    path = os.environ.get("X2V_VAE_CONV_PARITY_TABLE")
    if not path:
        return
    try:
        with open(path, "w") as f:
            for name in sorted(CASES):
                f.write(CASES[name].header() + "\n")
            for name in sorted(CASES):
                f.write("\n".join(CASES[name].table()) + "\n")
    except OSError:
        pass


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def case(name):
    return CASES.setdefault(name, V.Case(name))


# ------------------------------------------------------------------------------------------------------------------- buffers
def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def weight_window(w2d, tail=0, cin=0):
    """w2d [Cout, K] as rows 1 .. Cout of a loud [Cout + 2, K + pad] buffer (16 bytes of pad and more: w_row_stride > K).  tail: the last `tail` of every
    `cin` channels loud as well."""
    Cout, K = w2d.shape
    big = torch.full((Cout + 2, K + 32 // w2d.element_size()), LOUD, dtype=w2d.dtype, device="cuda")
    win = big[1 : Cout + 1, :K]
    win.copy_(w2d)
    if tail:
        win.view(Cout, K // cin, cin)[..., cin - tail :] = LOUD
    assert win.data_ptr() % 16 == 0 and win.stride(0) > K
    return big, win


def guarded_out(shape):
    n = 1
    for s in shape:
        n *= s
    whole = torch.full((GUARD + n + GUARD,), float("nan"), device="cuda")
    return whole, whole[GUARD : GUARD + n].view(*shape)


def guard_intact(whole):
    return bool(torch.isnan(whole[:GUARD]).all() and torch.isnan(whole[-GUARD:]).all())


class Dev:
    """The device side of an Inputs: the operand window [kt - 1 + T frames][H + 2 ph][W + 2 pw][px_stride > Cin] one frame inside a loud buffer (the
    stride-2 entry: no border), the weights, bias and residual.  separate: the cache frames in a tensor of their own and NaN in xp's leading frames.
    loud_tail: the zero tail of Cin holds loud values in both operands (what ZERO_TAIL32 must skip)."""

    def __init__(self, inp, separate=None, loud_tail=None, planes=None):
        sp = self.sp = inp.spec
        self.inp = inp
        kt, kh, kw = sp.k
        s2 = sp.op == "s2"
        self.separate = sp.cache if separate is None else separate
        loud_tail = bool(sp.flags & V.ZERO_TAIL32) if loud_tail is None else loud_tail
        od = torch.float32 if sp.op == "f32" else torch.float16
        ph, pw = (0, 0) if s2 else (kh // 2, kw // 2)
        L = kt - 1
        self.ps = ps = sp.Cin + 32 // (4 if od == torch.float32 else 2)
        Hp, Wp = sp.H + 2 * ph, sp.W + 2 * pw
        self.big = torch.full((1 + L + sp.T + 1, Hp, Wp, ps), LOUD, dtype=od, device="cuda")
        self.win = win = self.big[1 : 1 + L + sp.T]
        win[..., : sp.Cin] = 0
        self.interior = win[:, ph : ph + sp.H, pw : pw + sp.W]
        self.strides = (Hp * Wp * ps, Wp * ps, ps)
        if planes is None:
            self.interior[..., : sp.Cin] = inp.x.to("cuda")
        else:
            planes(self)
        if loud_tail:
            win[..., sp.Cin - sp.tail : sp.Cin] = LOUD
        self.cache = None
        if self.separate:
            self.cache = win[:L].clone()
            win[:L] = float("nan")
            self.cache_copy = self.cache.clone()
        self.wbig, self.w = weight_window(inp.w.reshape(sp.Cout, -1).to("cuda"), sp.tail if loud_tail else 0, sp.Cin)
        self.bias = None if inp.bias is None else inp.bias.to("cuda").contiguous()
        self.resid = None if inp.resid is None else inp.resid.to("cuda").contiguous()
        self.resid_copy = None if self.resid is None else self.resid.clone()
        self.big_copy, self.wbig_copy = self.big.clone(), self.wbig.clone()
        assert win.data_ptr() % 16 == 0 and ps > sp.Cin

    def run(self, lib, flags=None, frames=None):
        """One call; frames = (first, count): that many output frames from frame `first` on.  Returns the output view; guards and operands are checked."""
        sp = self.sp
        kt, kh, kw = sp.k
        flags = sp.flags if flags is None else flags
        f0, T = frames or (0, sp.T)
        ho, wo = V.out_hw(sp)
        shape = (2 * T, ho, wo, sp.Cout // 2) if flags & V.TSPLIT else (T, ho, wo, sp.Cout)
        whole, out = guarded_out(shape)
        xp = self.win[f0:]
        fs, rs, ps = self.strides
        p, L_ = lib._p, lib._lib
        resid = None if self.resid is None else self.resid[f0:]
        if sp.op == "f32":
            rc = L_.x2v_vae_conv_f32(p(xp), fs, rs, ps, p(self.w), self.w.stride(0), p(self.bias), p(resid), p(out), T, sp.H, sp.W, sp.Cin, sp.Cout, kt, kh, kw, flags, lib._stream())
        elif sp.op == "s2":
            rc = L_.x2v_vae_conv_s2_f16(p(xp), fs, rs, ps, p(self.w), self.w.stride(0), p(self.bias), p(out), T, sp.H, sp.W, sp.Cin, sp.Cout, 0, lib._stream())
        elif self.separate:
            assert f0 == 0
            rc = L_.x2v_vae_conv_f16_cached(p(xp), p(self.cache), fs, rs, ps, p(self.w), self.w.stride(0), p(self.bias), p(resid), p(out), T, sp.H, sp.W, sp.Cin, sp.Cout, kt, kh, kw,
                                            flags, lib._stream())
        else:
            rc = L_.x2v_vae_conv_f16(p(xp), fs, rs, ps, p(self.w), self.w.stride(0), p(self.bias), p(resid), p(out), T, sp.H, sp.W, sp.Cin, sp.Cout, kt, kh, kw, flags, lib._stream())
        lib._check(rc, V.name_of(sp))
        assert guard_intact(whole), f"{V.name_of(sp)}: wrote outside its output"
        assert torch.equal(bits(self.big), bits(self.big_copy)) and torch.equal(bits(self.wbig), bits(self.wbig_copy)), f"{V.name_of(sp)}: an operand buffer was written"
        assert self.resid is None or torch.equal(self.resid, self.resid_copy), f"{V.name_of(sp)}: resid was written"
        assert self.cache is None or torch.equal(bits(self.cache), bits(self.cache_copy)), f"{V.name_of(sp)}: the cache was written"
        return out


def inputs(family, sp, scale="n1"):
    """The Inputs of a case, made once per module run; the float64 side of the large cases lives on the device (rocBLAS's float64 matmul and torch's
    elementwise kernels are independent of the kernels under test) and is used by one test, the small ones' on the CPU."""
    key = (family, sp, scale)
    big = V.n_out(sp) > V.ON_DEVICE_ABOVE
    if key not in _INPUTS:
        inp = V.Inputs(family, sp, device="cuda" if big else "cpu", scale=scale)
        inp.assert_premises()
        if big:
            return inp
        _INPUTS[key] = inp
    return _INPUTS[key]


def assert_body(lib, sp):
    """What the ABI can tell about the dispatch: x2v_vae_conv_f16_cached_ok is 1 exactly where the 128-pixel body runs."""
    if sp.op == "f16":
        kt, kh, kw = sp.k
        ok = lib._lib.x2v_vae_conv_f16_cached_ok(sp.W, sp.Cin, sp.Cout, kh, kw, sp.flags) == 1
        assert ok == V.body(sp).startswith("halo128"), f"{V.name_of(sp)}: the library does not send this to {V.body(sp)}"
    return V.body(sp)


def run_spec(lib, name, sp, families=("I", "R"), want_body=None):
    b = assert_body(lib, sp)
    assert want_body is None or b.startswith(want_body), f"{V.name_of(sp)} reaches {b}, the test is written for {want_body}"
    for family in families:
        inp = inputs(family, sp)
        d = Dev(inp)
        got = d.run(lib)
        case(name).check(got, inp, b)
        if sp.flags & V.ZERO_TAIL32:  # the skipped slab over loud values = the multiplied slab over zeros, bit for bit
            plain = Dev(inp, loud_tail=False).run(lib, flags=sp.flags & ~V.ZERO_TAIL32)
            assert torch.equal(got, plain), f"{inp.name}: skipping the loud tail differs from multiplying a zero tail"
        if sp.cache:  # ... and the separate cache = the same frames in front of xp
            front = Dev(inp, separate=False).run(lib)
            assert torch.equal(got, front), f"{inp.name}: the separate-cache form differs from the cache in front of the frames"


def chunks(specs, n):
    return [specs[i : i + n] for i in range(0, len(specs), n)]


def ids(groups):
    return [V.name_of(g[0]).replace(" ", "_") + f"+{len(g) - 1}" for g in groups]


# ------------------------------------------------------------------------------------------------------------------- per-tap fp32 body
F32_GROUPS = {"instances": V.F32_INSTANCES, "k loop": V.F32_K_LOOP, "pixel tails": V.F32_PIXELS, "cout tails": V.F32_COUTS, "grids": V.F32_GRIDS, "epilogues": V.F32_EPILOGUES,
              "time-split": V.F32_TSPLIT}


@pytest.mark.parametrize("group", list(F32_GROUPS))
def test_pertap_f32(lib, group):
    """All eight NF x KC instantiations; 1, 2, 3, 9, 27 and 81 K steps; 1, 255, 256 and 257 pixels and W = 11 (a 256-pixel tile across image rows);
    Cout 3, 6, 40, 100, 132; 8, 1, 5, 9 and 13 workgroups through the XCD remap; every epilogue."""
    for sp in F32_GROUPS[group]:
        run_spec(lib, "pertap f32 " + group, sp, want_body="pertap f32")
    if group == "instances":
        assert {V.body(sp) for sp in V.F32_INSTANCES} == {f"pertap f32 NF{nf} KC{kc}" for nf in (1, 2, 3, 4) for kc in (16, 32)}


@pytest.mark.parametrize("c,npad", V.QK_CASES)
def test_pertap_f32_q_kt(lib, c, npad):
    """The attention block's S = Q K^T (lightx2v_amd/vae.py, hunyuan_vae.py): "pixels" = query tokens and "weights" = key rows of ONE [npad, 3 c] buffer —
    cin = c inside a 3 c pixel, w_row_stride = 3 c, the weights c floats into the buffer x starts at; V's third holds loud values."""
    sp = V.Spec("f32", 1, 1, npad, c, npad, bias=False, resid=False)
    for family in ("I", "R"):
        inp = inputs(family, sp)
        big = torch.full((npad + 2, 3 * c), LOUD, device="cuda")
        qkv = big[1 : npad + 1]
        qkv[:, :c], qkv[:, c : 2 * c] = inp.x.reshape(npad, c).cuda(), inp.w.reshape(npad, c).cuda()
        copy = big.clone()
        whole, out = guarded_out((1, 1, npad, npad))
        k = qkv[:, c:]
        lib._check(lib._lib.x2v_vae_conv_f32(lib._p(qkv), npad * 3 * c, npad * 3 * c, 3 * c, lib._p(k), 3 * c, None, None, lib._p(out), 1, 1, npad, c, npad, 1, 1, 1, 0, lib._stream()), "q k^T")
        assert guard_intact(whole) and torch.equal(big, copy)
        case("pertap f32 gemm roles").check(out, inp, V.body(sp), "q.k^T")


@pytest.mark.parametrize("npad,C", V.PV_CASES)
def test_pertap_f32_scores_v(lib, npad, C):
    """O = scores . V^T-transposed: Cin = npad keys, the reduction index contiguous in both operands."""
    run_spec(lib, "pertap f32 gemm roles", V.Spec("f32", 1, 1, npad, npad, C, bias=False, resid=False), want_body="pertap f32")


@pytest.mark.parametrize("T,Hin,Win,C,Cout", V.POLYPHASE)
def test_pertap_f32_polyphase_stride_2(lib, T, Hin, Win, C, Cout):
    """The encoder's fp32 downsampling (lightx2v_amd/vae_enc.py _down2d): four phase convolutions (2x2, 2x1, 1x2, 1x1 kernels) over the rows a::2 and columns
    b::2 of the frame with one zero row and column behind it — strides (fs, 2 rs, 2 ps) — chained through resid, against the stride-2 reference."""
    sp = V.Spec("p32", T, Hin, Win, C, Cout)
    ho, wo = Hin // 2, Win // 2
    hp, wp, ps = 2 * ho + 1, 2 * wo + 1, C + 8
    for family in ("I", "R"):
        inp = inputs(family, sp)
        big = torch.full((T + 2, hp, wp, ps), LOUD, device="cuda")
        buf = big[1 : T + 1]
        buf[..., :C] = 0
        buf[:, : min(Hin, hp), : min(Win, wp), :C] = inp.x.cuda()[:, :hp, :wp]
        copy = big.clone()
        fs, rs = hp * wp * ps, wp * ps
        acc, bias = None, inp.bias.cuda()
        for a in (0, 1):
            for b in (0, 1):
                wph = inp.w[:, 0, a::2, b::2].cuda()  # [Cout, kh', kw', C]
                kh, kw = wph.shape[1:3]
                wbig, w = weight_window(wph.reshape(Cout, -1))
                whole, out = guarded_out((T, ho, wo, Cout))
                prev = None if acc is None else acc.clone()
                lib._check(lib._lib.x2v_vae_conv_f32(lib._p(buf[:, a:, b:]), fs, 2 * rs, 2 * ps, lib._p(w), w.stride(0), lib._p(bias) if acc is None else None, lib._p(acc), lib._p(out),
                                                     T, ho, wo, C, Cout, 1, kh, kw, 0, lib._stream()), "polyphase")
                assert guard_intact(whole) and torch.equal(big, copy) and (prev is None or torch.equal(acc, prev))
                acc = out
        case("pertap f32 polyphase").check(acc, inp, V.body(sp), "4 phases")


# ------------------------------------------------------------------------------------------------------------------- 16-bit bodies
@pytest.mark.parametrize("group", chunks(V.PT16_SPECS, 8), ids=ids(chunks(V.PT16_SPECS, 8)))
def test_pertap_f16(lib, group):
    """NF 1..4 x Cin 64, 192; (3, 1, 1), (1, 3, 3) below the 16-pixel threshold, (3, 3, 3) by flag, the time-split; the fp32 body's pixel and cout tails."""
    for sp in group:
        run_spec(lib, "pertap f16", sp, want_body="pertap f16")


@pytest.mark.parametrize("group", chunks(V.HALO64_SPECS, 8), ids=ids(chunks(V.HALO64_SPECS, 8)))
def test_halo64(lib, group):
    """NF 1..4; 9, 18, 27, 54 and 81 steps through the ring of four slots; tiles ragged in H and W (8 x 32); every epilogue."""
    for sp in group:
        run_spec(lib, "halo64", sp, want_body="halo64")


@pytest.mark.parametrize("group", chunks(V.HALO128_SPECS, 8), ids=ids(chunks(V.HALO128_SPECS, 8)))
def test_halo128(lib, group):
    """The 96-, 128- and 16-cout forms at 1, 2, 3, 4 and 9 slabs (prologue only, the `h += 2` tail, the odd last slab), the zero-tail flag over loud values
    equal to the zero-padded buffer bit for bit, tiles ragged in H and W (16 x 32), every epilogue."""
    for sp in group:
        run_spec(lib, "halo128", sp, want_body="halo128")


def test_halo128_separate_cache(lib):
    """T = 4, kt = 3: frames 0, 1 and 2 read 2, 1 and 0 frames from `cache`; xp's own leading frames hold NaN."""
    for sp in V.HALO128_CACHED:
        assert V.cached_ok(sp)
        run_spec(lib, "halo128 cache", sp, want_body="halo128")


def test_halo128_frame_batching_is_bit_identical(lib):
    """A launch over T frames = T one-frame launches, bit for bit (family R), and both against float64."""
    sp = V.FRAME_BATCH
    inp = inputs("R", sp)
    d = Dev(inp)
    whole = d.run(lib)
    case("halo128 frames").check(whole, inp, assert_body(lib, sp), "T frames")
    for t in range(sp.T):
        assert torch.equal(d.run(lib, frames=(t, 1))[0], whole[t]), t


@pytest.mark.parametrize("which", ("halo64", "halo128"))
def test_persistent_later_tiles(lib, cus, which):
    """cus + 1 and 2 cus + 3 tiles on the persistent grids: some workgroups run a second and a third tile.  The 128-pixel body with kt = 3 and the separate
    cache: a workgroup's later tiles lie in later frames, so n_cached changes between its tiles."""
    for sp, tiles in zip(V.persistent_specs(cus, which), (cus + 1, 2 * cus + 3)):
        assert sp.T * 6 >= tiles and sp.T > 3
        for family in ("I", "R"):
            inp = inputs(family, sp)
            got = Dev(inp).run(lib)
            case("persistent " + which).check(got, inp, assert_body(lib, sp), f">= {tiles} tiles")
            del inp, got


@pytest.mark.parametrize("group", chunks(V.S2_SPECS + V.S2_SPLIT, 7), ids=ids(chunks(V.S2_SPECS + V.S2_SPLIT, 7)))
def test_stride_2(lib, group):
    """Cin 32, 96 x Cout 4, 96, 100, 192 at Hin, Win in {2, 3, 32, 33, 34, 35}: one output, exact tiles, the zero row / column that is read (even sizes) and the
    last row / column that no output reads (odd sizes); pixel stride > Cin; plain and split operands."""
    for sp in group:
        run_spec(lib, "stride 2", sp, want_body="s2")


@pytest.mark.parametrize("sp", V.DEEP_SPECS, ids=[V.body(sp).replace(" ", "_") for sp in V.DEEP_SPECS])
def test_deep_k(lib, sp):
    """K = 27 * 512 = 13824 on every body (the stride-2 body: 9 * 512), family I."""
    run_spec(lib, "deep k", sp, families=("I",))


# ------------------------------------------------------------------------------------------------------------------- split, end to end
@pytest.mark.parametrize("scale", V.SPLIT_SCALES)
@pytest.mark.parametrize("sp", V.SPLIT_E2E, ids=[V.body(sp).replace(" ", "_") for sp in V.SPLIT_E2E])
def test_split_end_to_end(lib, sp, scale):
    """conv16="split": the device's planes (lib.vae_prep(split=True)) and weights (lightx2v_amd.vae._split16) equal the restatement bit for bit; their
    convolution holds both rules of family R as a 16-bit case, and is fp32-grade end to end: relL2 against float64 of the UNROUNDED operands <= 1.5 Y,
    Y the fp32 chain on the unrounded operands — at N(0, 1) * 3 and at |x| in [1e-3, 0.25], where the middle plane is an fp16 subnormal."""
    from lightx2v_amd import vae

    inp = inputs("R", sp, scale)
    C = sp.C
    if scale == "small":
        mid = inp.x[..., C : 2 * C].float().abs()
        assert float(((mid > 0) & (mid < 2.0 ** -14)).float().mean()) > 0.95, "this case must put the middle plane into the fp16 subnormal range"

    def planes(d):
        y = d.interior
        lib.vae_prep(inp.x32.cuda().contiguous(), y, d.strides[:2], split=True)
        assert torch.equal(bits(y[..., : sp.Cin]), bits(inp.x.cuda())), "the device's split planes differ from the restatement"

    w16 = vae._split16(inp.w32.cuda(), sp.Cin, True)
    assert torch.equal(bits(w16), bits(inp.w.cuda())), "_split16 differs from the restatement"
    d = Dev(inp, planes=planes)
    got = d.run(lib)
    b = assert_body(lib, sp)
    case("split").check(got, inp, b, f"planes {scale}")
    case("split").check_bound(got, inp, b, f"e2e {scale}", t=inp.t_unrounded, Y=inp.yardstick_unrounded())
