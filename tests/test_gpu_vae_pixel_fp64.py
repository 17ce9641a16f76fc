"""The kernels between the VAE convolutions — vae.hip's pixel-wise producers (vae_prep in fp32, fp16 and the hi/lo split; vae_prep_ex in fp32 and fp16),
replicate padding, GroupNorm's statistics, the two row softmaxes and the axis blend, vae_enc.hip's video producer — at the smallest shapes at which each
dispatch arm, loop pass and layout edge exists, against the float64 references of tests/vae_pixel_ref.py (its docstring lists what each case reaches
and derives every bound).  Family I must EQUAL the float64 result on every element; family R must hold the per-element bound on every element and
relL2 <= 1.5 Y; tests/test_vae_pixel_ref_host.py shows which subtly wrong kernels this rejects.

Every output is the interior of a sentinel-filled buffer (a 1-pixel border, 0..2 frames in front, pad channels where the pixel stride exceeds what
is written, ld - N columns behind a softmax row, a row above and below); afterwards the sentinel must be intact and the inputs unchanged.  Upsampled
outputs are compared pixel by pixel with the reference's.  Everything is called through lightx2v_amd.lib."""
import math

import pytest
import torch

from tests import vae_pixel_ref as P
from tests.vae_pixel_ref import F16, F32

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from lightx2v_amd import lib as L

    L.init()
    return L


def dev(t):
    return None if t is None else t.cuda()


def unchanged(pairs, what):
    for d, h in pairs:
        assert d is None or torch.equal(d.cpu(), h), f"{what}: an input was written"


# ------------------------------------------------------------------------------------------------------------------- producers
def run_prep(lib, kind, x, gamma, a, b, mode, ps, lead):
    T, H, W, C = x.shape
    k = 2 if mode.up else 1
    written = C * (3 if kind == "split" else 1)
    buf, view = P.framed(T, H * k, W * k, ps, lead, F32 if kind == "f32" else F16, "cuda")
    xd, gd, ad, bd = dev(x), dev(gamma), dev(a), dev(b)
    lib.vae_prep(xd, view, (buf.stride(0), buf.stride(1)), gamma=gd, a=ad, b=bd, silu=mode.silu, upsample=mode.up, split=kind == "split")
    torch.cuda.synchronize()
    what = f"vae_prep {kind} C={C} {(T, H, W)} {P.mode_name(mode)} stride {ps}"
    assert P.frame_intact(buf, lead, written), f"{what}: wrote outside the interior's first {written} channels"
    unchanged(((xd, x), (gd, gamma), (ad, a), (bd, b)), what)
    return view[..., :written].cpu()


def prep_cases(lib, kind, C, strides, modes_i, modes_r):
    n = 0
    for ps in strides:
        for geom in P.GEOMS:
            for family, modes in (("I", modes_i), ("R", modes_r)):
                for mode in modes:
                    x, gamma, a, b = P.prep_inputs(family, C, geom, mode)
                    got = run_prep(lib, kind, x, gamma, a, b, mode, ps, n % 3)
                    P.accept_prep(kind, family, C, geom, mode, got=got)
                    if mode.gamma:  # the all-zero pixel: exactly 0 through the norm and SiLU
                        k = 2 if mode.up else 1
                        assert bool((got[0, :k, :k] == 0).all()), f"vae_prep {kind} C={C}: the zero pixel came out as {got[0, 0, 0, :4].tolist()}"
                    n += 1
    return n


@pytest.mark.parametrize("C", P.PREP_F32_C)
def test_vae_prep_f32(lib, C):
    assert prep_cases(lib, "f32", C, (C,), P.PREP_MODES_I, P.PREP_MODES_R) == 3 * (len(P.PREP_MODES_I) + len(P.PREP_MODES_R))


@pytest.mark.parametrize("kind", ["f16", "split"])
@pytest.mark.parametrize("C", P.PREP_F16_C)
def test_vae_prep_f16(lib, C, kind):
    w = C * (3 if kind == "split" else 1)
    if w % 8:  # strides are multiples of 8 halves: a pixel stride of 4 / 12 halves is refused, not run
        buf, view = P.framed(1, 1, 1, w, 0, F16, "cuda")
        with pytest.raises(lib.X2VError):
            lib.vae_prep(torch.zeros(1, 1, 1, C, device="cuda"), view, (buf.stride(0), buf.stride(1)), split=kind == "split")
        assert P.frame_intact(buf, 0, 0)
    prep_cases(lib, kind, C, ((w,) if w % 8 == 0 else ()) + (P.next64(w),), P.PREP16_MODES_I, P.PREP16_MODES_R)


@pytest.mark.parametrize("up", [False, True])
def test_vae_prep_split_saturates(lib, up):
    """+-65504, 65519, 65520, 1e5, 131008, 2e5, inf, 2^-14, 2^-24, 2^-25: hi saturates, lo carries the remainder, mid = hi 2^-12 in fp16 exactly."""
    mode, geom = P.Mode(up=up), (2, 3, 5)
    for C, ps in ((96, 288), (96, 320), (4, 64)):
        x = P.with_specials(P.prep_inputs("I", C, geom, mode)[0])
        got = run_prep(lib, "split", x, None, None, None, mode, ps, 1)
        P.check_exact(got, P.vae_prep_split_f16(x, upsample=up), f"split specials C={C} stride {ps}")
        assert bool(torch.isfinite(got).all())
        P.check_exact(got[..., C : 2 * C], (got[..., :C].double() * 2.0 ** -12).to(F16), "mid plane = hi 2^-12")
        P.check_exact(run_prep(lib, "f16", x, None, None, None, mode, P.next64(C), 1), P.vae_prep_f16(x, upsample=up), f"fp16 specials C={C}")


def run_ex(lib, kind, x, mul, add, ex, lead):
    T, H, W, C = x.shape
    k = 2 if ex.up_hw else 1
    To = 2 * T - 1 if ex.up_t else T
    buf, view = P.framed(To, H * k, W * k, C, lead, F32 if kind == "f32" else F16, "cuda")
    xd, md, ad = dev(x), dev(mul), dev(add)
    lib.vae_prep_ex(xd, view, (buf.stride(0), buf.stride(1)), mul=md, add=ad, silu=ex.silu, clamp01=ex.clamp, up_hw=ex.up_hw, up_t=ex.up_t)
    torch.cuda.synchronize()
    what = f"vae_prep_ex {kind} C={C} {(T, H, W)} {P.mode_name(ex)}"
    assert P.frame_intact(buf, lead, C), f"{what}: wrote outside the interior"
    unchanged(((xd, x), (md, mul), (ad, add)), what)
    return view.cpu()


@pytest.mark.parametrize("kind,C", [("f32", C) for C in P.EX_F32_C] + [("f16", C) for C in P.EX_F16_C])
def test_vae_prep_ex(lib, kind, C):
    n = 0
    for geom in P.GEOMS:
        for family, exs in (("I", P.EX_I), ("R", P.EX_R)):
            for ex in exs:
                x, mul, add = P.ex_inputs(family, C, geom, ex)
                P.accept_ex(kind, family, C, geom, ex, got=run_ex(lib, kind, x, mul, add, ex, n % 3))
                n += 1


@pytest.mark.parametrize("which", ["prep f32", "prep f16", "ex f32", "ex f16"])
def test_producer_grid_stride(lib, which):
    """8 * 262144 + 11 pixels: behind the grid cap of 65536 * 4 blocks x 8 pixel groups a second sweep has 11 live groups, so groups of one wave leave
    the loop at different trip counts.  Family I (a power of two, b an integer), compared on the device."""
    C = 8 if which == "ex f16" else 4
    g = P._gen(P.GRID_NPIX, C, 18)
    x = torch.randint(-8, 9, (1, 1, P.GRID_NPIX, C), generator=g, dtype=torch.int8).to(F32)
    a, b = torch.exp2(torch.randint(-2, 3, (C,), generator=g).to(F32)), torch.randint(-16, 17, (C,), generator=g).to(F32)
    f16 = which.endswith("f16")
    ps = 8 if f16 else C
    buf, view = P.framed(1, 1, P.GRID_NPIX, ps, 0, F16 if f16 else F32, "cuda")
    xd, ad, bd = x.cuda(), a.cuda(), b.cuda()
    if which.startswith("prep"):
        lib.vae_prep(xd, view, (buf.stride(0), buf.stride(1)), a=ad, b=bd)
        want = P.vae_prep(x, None, a, b, dtype=F32)  # exact in fp32: integers over powers of two plus integers
    else:
        lib.vae_prep_ex(xd, view, (buf.stride(0), buf.stride(1)), mul=ad, add=bd)
        want = P.vae_prep_ex(x, a, b, dtype=F32)
    torch.cuda.synchronize()
    assert P.frame_intact(buf, 0, C), f"{which}: wrote outside the interior"
    P.check_exact(view[..., :C], want.to(buf.dtype).cuda(), f"grid-stride {which}")
    assert torch.equal(xd.cpu(), x)


# ------------------------------------------------------------------------------------------------------------------- replicate padding
def test_replicate_border(lib):
    cases = [(c, 32) for c in P.BORDER_CASES] + [((lead, pad, 2 * pad + dh, 2 * pad + dw, hv), 16) for lead, pad in ((0, 1), (2, 2), (1, 0)) for dh, dw in ((1, 1), (3, 4))
                                                  for hv in P.BORDER_F16_HALVES]
    for case, bits in cases:
        before, want = P.border_buffers(*case, bits=bits)
        buf = before.view(F32 if bits == 32 else F16).cuda()
        lib.vae_replicate_border_(buf, case[0], case[1])
        P.check_bits(buf.cpu().view(before.dtype), want, f"replicate_border (lead, pad, Hp, Wp, C) = {case} {bits}-bit")


# ------------------------------------------------------------------------------------------------------------------- GroupNorm
def run_groupnorm(lib, family, C, G, npix, offset=False, seed=0):
    x, gamma, beta, eps = P.groupnorm_inputs(family, C, G, npix, seed, offset)
    xd, gd, bd = x.cuda(), gamma.cuda(), beta.cuda()
    mul, add = lib.groupnorm_affine(xd, G, gd, bd, eps)
    got = (mul.cpu(), add.cpu())
    unchanged(((xd, x), (gd, gamma), (bd, beta)), f"groupnorm C={C} G={G}")
    return P.accept_groupnorm(family, C, G, npix, offset, got=got, seed=seed)


@pytest.mark.parametrize("C,G", P.GN_SHAPES)
def test_groupnorm_affine(lib, C, G):
    for npix in P.GN_NPIX:
        run_groupnorm(lib, "I", C, G, npix)
        run_groupnorm(lib, "R", C, G, npix)
        run_groupnorm(lib, "R", C, G, npix, offset=True)
        run_groupnorm(lib, "R", C, G, npix, seed=1)  # the same shape again on fresh inputs: the workspace is re-zeroed


def test_groupnorm_affine_block_cap(lib):
    C, G, npix = P.GN_CAP
    assert npix * (C // 4) > 2048 * 256
    run_groupnorm(lib, "I", C, G, npix)
    run_groupnorm(lib, "R", C, G, npix, offset=True)


# ------------------------------------------------------------------------------------------------------------------- softmax
def window(M, N, ld):
    """A sentinel [M + 2, ld] buffer and its [M, N] window (rows 1 .. M)."""
    big = torch.full((M + 2, ld), P.SENTINEL, device="cuda")
    return big, big[1 : M + 1, :N]


def window_intact(big, M, N):
    return bool((big[0] == P.SENTINEL).all() and (big[M + 1] == P.SENTINEL).all() and (big[1 : M + 1, N:] == P.SENTINEL).all())


def run_softmax(lib, s, scale, ld, causal=None):
    M, N = s.shape
    big, v = window(M, N, ld)
    v.copy_(s)
    if causal is None:
        lib.softmax_rows_(v, scale)
    else:
        lib.softmax_rows_causal_(v, scale, causal[0], n_keys=causal[1])
    torch.cuda.synchronize()
    assert window_intact(big, M, N), f"softmax N={N} ld={ld}: wrote outside the rows"
    return v.cpu()


@pytest.mark.parametrize("N", P.SOFTMAX_N)
def test_softmax_rows(lib, N):
    for M in P.SOFTMAX_M:
        for ld in (N, N + 12):
            for scale in P.SOFTMAX_SCALES:
                for A in P.SOFTMAX_A:
                    s = P.softmax_inputs(M, N, scale, A)
                    P.accept_softmax(s, scale, None, f"softmax_rows N={N} M={M} ld={ld} scale={scale:.4f} A={A}", got=run_softmax(lib, s, scale, ld))
    for c in (0.0, 3.0, -1000.0):  # constant rows, scale a power of two: every entry is fp32(1) / fp32(N)
        got = run_softmax(lib, torch.full((2, N), c), 0.25, N + 12)
        P.check_exact(got, (torch.tensor(1.0) / torch.tensor(float(N))).expand(2, N).contiguous(), f"softmax_rows N={N}: constant rows of {c}")
    s = torch.randn(2, N, generator=P._gen(N, 19))
    s[:, N // 2] += 1e4
    want = torch.zeros(2, N)
    want[:, N // 2] = 1.0
    P.check_exact(run_softmax(lib, s, 0.25, N), want, f"softmax_rows N={N}: one entry 1e4 above the rest")


@pytest.mark.parametrize("hw,frames,N,n_keys,ld", P.CAUSAL_CASES)
def test_softmax_rows_causal(lib, hw, frames, N, n_keys, ld):
    valid = P.causal_valid(N, N, hw, n_keys)
    dead = torch.arange(N)[None, :] >= valid[:, None]
    for scale, A in ((0.25, 40), (1 / math.sqrt(384), 3)):
        s = P.causal_inputs(hw, frames, N, n_keys, scale, A)
        got = run_softmax(lib, s, scale, ld, (hw, n_keys))
        assert bool(torch.isfinite(got).all()), "non-finite entries (padded rows included)"
        assert bool((got[dead] == 0).all()), "a column >= valid is not exactly 0"
        P.accept_softmax(s, scale, valid, f"softmax_rows_causal hw={hw} frames={frames} N={N} n_keys={n_keys} ld={ld} A={A}", got=got)
    s = torch.full((N, N), 3.0)
    s[:, n_keys:] = P.LOUD
    want = torch.where(dead, torch.zeros(()), (torch.tensor(1.0) / valid.to(F32))[:, None].expand(N, N))
    P.check_exact(run_softmax(lib, s, 0.25, ld, (hw, n_keys)), want, "constant rows: fp32(1) / fp32(valid), 0 behind")
    s = torch.randn(N, N, generator=P._gen(N, hw, 20))
    s[:, 0] += 1e4
    want = torch.zeros(N, N)
    want[:, 0] = 1.0
    got = run_softmax(lib, s, 0.25, ld, (hw, n_keys))
    P.check_exact(got, want, "column 0 1e4 above the rest")
    if hw == 1:
        assert float(run_softmax(lib, torch.randn(N, N, generator=P._gen(N, 21)), 0.25, ld, (hw, n_keys))[0, 0]) == 1.0, "hw = 1: row 0 sees one key"


@pytest.mark.parametrize("scale", [0.0, -0.25, float("nan")])
def test_softmax_refuses_scale_not_above_zero(lib, scale):
    """The stabiliser is max(s) * scale: the maximum of the scaled row only for scale > 0.  Both entries refuse anything else before any launch."""
    s = torch.randn(4, 8, generator=P._gen(22))
    for causal in (None, (2, 8)):
        big, v = window(4, 8, 8)
        v.copy_(s)
        with pytest.raises(lib.X2VError):
            lib.softmax_rows_(v, scale) if causal is None else lib.softmax_rows_causal_(v, scale, causal[0], n_keys=causal[1])
        torch.cuda.synchronize()
        assert torch.equal(v.cpu(), s) and window_intact(big, 4, 8), "a refused call wrote"


# ------------------------------------------------------------------------------------------------------------------- blend
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_blend_axis(lib, axis):
    for family, extents in (("I", P.BLEND_EXTENTS_I), ("R", P.BLEND_EXTENTS_R)):
        for e in extents:
            a, b = P.blend_inputs(family, axis, e)
            ad, bd = a.cuda(), b.cuda()
            out = lib.blend_axis_(ad, bd, axis, e)
            assert out.data_ptr() == bd.data_ptr()
            got = bd.cpu()
            P.accept_blend(family, axis, e, got=got)
            ee = min(e, a.shape[axis], b.shape[axis])
            P.check_bits(got.narrow(axis, ee, b.shape[axis] - ee), b.narrow(axis, ee, b.shape[axis] - ee), f"blend_axis axis={axis} extent={e}: b beyond the extent")
            P.check_bits(ad.cpu(), a, f"blend_axis axis={axis} extent={e}: a")


# ------------------------------------------------------------------------------------------------------------------- video producer
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_video_prep(lib, mode):
    big, crop = P.video_inputs()
    T, H, W = P.VIDEO_GEOM
    written = 9 if mode == 2 else 3
    for ps in P.VIDEO_STRIDES[mode]:
        bigd = big.cuda()
        vd = P.video_crop(bigd)
        assert vd.stride() == crop.stride() and vd.stride(0) > T * vd.stride(1) > T * H * vd.stride(2) > T * H * W
        buf, view = P.framed(T, H, W, ps, 1, F32 if mode == 0 else F16, "cuda")
        lib.vae_video_prep(vd, view, split=mode == 2)
        torch.cuda.synchronize()
        assert P.frame_intact(buf, 1, written), f"video_prep mode {mode} stride {ps}: wrote outside its channels"
        P.check_bits(bigd.cpu(), big, "the video")
        want, got = P.video_prep(crop, mode), view[..., :written].cpu()
        P.check_bits(got, want, f"video_prep mode {mode} stride {ps}") if mode == 0 else P.check_exact(got, want, f"video_prep mode {mode} stride {ps}")
