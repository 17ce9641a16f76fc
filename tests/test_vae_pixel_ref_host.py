"""The yardstick of tests/test_gpu_vae_pixel_fp64.py checked without a GPU: every float64 restatement of tests/vae_pixel_ref.py against an independently
written torch form, the fp32 restatement exact on every family-I case and within HALF of the per-element bound on every family-R case (the bounds
are satisfiable by a correct kernel), and subtly wrong fp32 kernels each rejected by the acceptance on a named case of the GPU module's lists."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import vae_pixel_ref as P
from tests.vae_pixel_ref import F16, F32, F64

def close(a, b, rtol=1e-13):
    return bool(((a - b).abs() <= rtol * b.abs() + 1e-300).all())


# ------------------------------------------------------------------------------------------------------------------- independent forms
def test_float64_restatements_against_torch_forms():
    g = torch.Generator().manual_seed(5)
    T, H, W, C = 3, 2, 5, 12
    x, gamma = torch.randn(T, H, W, C, generator=g, dtype=F64), torch.randn(C, generator=g, dtype=F64)
    a, b = torch.rand(C, generator=g, dtype=F64) + 0.5, torch.randn(C, generator=g, dtype=F64)
    assert close(P.vae_prep(x, gamma), F.normalize(x, dim=-1) * math.sqrt(C) * gamma)
    assert close(P.vae_prep(x, gamma, silu_=True), F.silu(F.normalize(x, dim=-1) * math.sqrt(C) * gamma))
    assert close(P.vae_prep(x, None, a, b), x / a + b) and torch.equal(P.vae_prep(x), x)
    nearest = lambda v: F.interpolate(v.permute(0, 3, 1, 2), scale_factor=2.0, mode="nearest").permute(0, 2, 3, 1)  # noqa: E731
    assert torch.equal(P.vae_prep(x, upsample=True), nearest(x))
    v = x * a + b
    assert close(P.vae_prep_ex(x, a, b), v) and close(P.vae_prep_ex(x, a, b, True, True), F.silu(v).clamp(0, 1))
    cf = v.permute(3, 0, 1, 2)  # [C, T, H, W]: the frame-0 rule of UpsampleCausal3D
    first = F.interpolate(cf[:, :1].permute(1, 0, 2, 3), scale_factor=(2.0, 2.0), mode="nearest").permute(1, 0, 2, 3)
    other = F.interpolate(cf[:, 1:].unsqueeze(0), scale_factor=(2.0, 2.0, 2.0), mode="nearest")[0]
    assert torch.equal(P.vae_prep_ex(x, a, b, up_hw_=True, up_t_=True), torch.cat((first, other), 1).permute(1, 2, 3, 0))
    other_t = F.interpolate(cf[:, 1:].unsqueeze(0), scale_factor=(2.0, 1.0, 1.0), mode="nearest")[0]
    assert torch.equal(P.vae_prep_ex(x, a, b, up_t_=True), torch.cat((cf[:, :1], other_t), 1).permute(1, 2, 3, 0))
    assert P.vae_prep_ex(x[:1], up_t_=True).shape[0] == 1
    for lead, pad in ((0, 0), (2, 1), (1, 2)):
        inner = torch.randn(2, 3, 4, C, generator=g, dtype=F64)
        buf = torch.full((lead + 2, 3 + 2 * pad, 4 + 2 * pad, C), 9.0, dtype=F64)
        buf[lead:, pad : pad + 3, pad : pad + 4] = inner
        want = F.pad(inner.permute(3, 0, 1, 2).unsqueeze(0), (pad, pad, pad, pad, lead, 0), mode="replicate")[0].permute(1, 2, 3, 0)
        assert torch.equal(P.replicate_border(buf, lead, pad), want)
    xg = torch.randn(50, 24, generator=g, dtype=F64) * 2 + 0.7
    gm, bt = torch.randn(24, generator=g, dtype=F64), torch.randn(24, generator=g, dtype=F64)
    for G in (1, 3, 6):
        mul, add = P.groupnorm_affine(xg, G, gm, bt, 1e-6)
        assert close(xg * mul + add, F.group_norm(xg.T.unsqueeze(0), G, gm, bt, P.f32_scalar(1e-6))[0].T, 1e-11)
    s = torch.randn(12, 16, generator=g, dtype=F64) * 5
    assert close(P.softmax_rows(s, 0.25), (s * 0.25).softmax(-1))
    hw, n = 3, 11
    valid = P.causal_valid(12, 16, hw, n)
    col, row_fr = torch.arange(16), torch.arange(12) // hw
    mask = (col[None, :] // hw <= row_fr[:, None]) & (col[None, :] < n)
    assert torch.equal(valid, mask.sum(1))
    assert close(P.softmax_rows(s, 0.3, valid), (s * P.f32_scalar(0.3)).masked_fill(~mask, -math.inf).softmax(-1))
    for axis, e in ((0, 2), (1, 3), (2, 5), (1, 99)):
        sa, sb = [4, 6, 7, 3], [4, 6, 7, 3]
        sa[axis] += 1
        A, B = torch.randn(sa, generator=g, dtype=F64), torch.randn(sb, generator=g, dtype=F64)
        want, ee = B.clone().movedim(axis, 0), min(e, sa[axis], sb[axis])
        Am = A.movedim(axis, 0)
        for y in range(ee):  # blend_v / blend_h / blend_t of the reference
            want[y] = Am[-ee + y] * (1 - y / ee) + want[y] * (y / ee)
        assert close(P.blend_axis(A, B, axis, e), want.movedim(0, axis))
    vid = torch.randn(3, 2, 3, 4, generator=g)
    assert torch.equal(P.video_prep(vid, 0), torch.stack([vid[0], vid[1], vid[2]], -1)) and P.video_prep(vid, 2).shape[-1] == 9


def test_half_ulp16_and_split():
    r = torch.tensor([1.0, 1.5, 2.0, 1000.0, 2.0 ** -14, 2.0 ** -20, 0.0], dtype=F64)
    assert torch.equal(P.half_ulp16(r), torch.tensor([2.0 ** -11, 2.0 ** -11, 2.0 ** -10, 2.0 ** -2, 2.0 ** -25, 2.0 ** -25, 2.0 ** -25], dtype=F64))
    x = P.with_specials(torch.zeros(1, 1, 1, 96))
    sp = P.split_planes(x)
    assert bool(torch.isfinite(sp).all()) and float(sp[..., :96].abs().max()) == 65504.0
    assert torch.equal(sp[0, 0, 0, :4], torch.tensor([65504.0, -65504.0, 65504.0, -65504.0], dtype=F16))
    assert torch.equal(sp[0, 0, 0, 192:198], torch.tensor([0.0, 0.0, 15.0, -15.0, 16.0, -16.0], dtype=F16))


# ------------------------------------------------------------------------------------------------------------------- the restatement on every case
@pytest.mark.parametrize("kind", ["f32", "f16", "split"])
def test_vae_prep_restatement(kind):
    Y = 0.0
    cs, mi, mr = (P.PREP_F32_C, P.PREP_MODES_I, P.PREP_MODES_R) if kind == "f32" else (P.PREP_F16_C, P.PREP16_MODES_I, P.PREP16_MODES_R)
    for C in cs:
        for geom in P.GEOMS:
            for mode in mi:
                P.accept_prep(kind, "I", C, geom, mode)
            for mode in mr:
                worst, y = P.accept_prep(kind, "R", C, geom, mode, share=1.0 if kind == "f32" else 0.5)
                assert worst <= (0.5 if kind == "f32" else 1.0), f"vae_prep {kind} C={C} {geom} {P.mode_name(mode)}: the fp32 restatement reaches {worst:.3f} of its bound"
                Y = max(Y, y)
                if mode.gamma:  # the zero pixel comes out exactly 0
                    x, gamma, a, b = P.prep_inputs("R", C, geom, mode)
                    out = P.prep_eval(kind, x, gamma, a, b, mode, F32)
                    assert bool((out[0, : 2 if mode.up else 1, : 2 if mode.up else 1] == 0).all())
    print(f"vae_prep {kind}: Y = {Y:.2e}")
    assert 0 < Y < (1e-3 if kind == "f16" else 3e-7)


def test_split_specials_exact():
    for up in (False, True):
        x = P.with_specials(P.prep_inputs("I", 96, (2, 3, 5), P.Mode(up=up))[0])
        want, got = P.vae_prep_split_f16(x, upsample=up), P.vae_prep_split_f16(x, upsample=up, dtype=F32)
        P.check_exact(got, want, "split specials")
        assert torch.equal(got[..., 96:192], (got[..., :96].to(F64) * 2.0 ** -12).to(F16)) and bool(torch.isfinite(got).all())


@pytest.mark.parametrize("kind", ["f32", "f16"])
def test_vae_prep_ex_restatement(kind):
    Y, sides = 0.0, [0, 0, 0]
    for C in (P.EX_F32_C if kind == "f32" else P.EX_F16_C):
        for geom in P.GEOMS:
            for ex in P.EX_I:
                P.accept_ex(kind, "I", C, geom, ex)
                if ex.clamp:
                    x, mul, add = P.ex_inputs("I", C, geom, ex)
                    v = P.vae_prep_ex(x, mul, add)
                    sides = [sides[0] + int((v < 0).sum()), sides[1] + int(((v > 0) & (v < 1)).sum()), sides[2] + int((v > 1).sum())]
            for ex in P.EX_R:
                worst, y = P.accept_ex(kind, "R", C, geom, ex, share=1.0 if kind == "f32" else 0.5)
                assert worst <= (0.5 if kind == "f32" else 1.0), f"vae_prep_ex {kind} C={C} {geom} {P.mode_name(ex)}: the fp32 restatement reaches {worst:.3f} of its bound"
                Y = max(Y, y)
    assert min(sides) > 0, f"clamp01 of family I: below / inside / above = {sides}"
    print(f"vae_prep_ex {kind}: Y = {Y:.2e}")
    assert 0 < Y < (1e-3 if kind == "f16" else 3e-7)


def test_silu_form_on_its_range():
    v = torch.linspace(-80, 80, 200001, dtype=F32)
    ref = P.silu(v.to(F64))
    r = ((P.silu(v).to(F64) - ref).abs() / ((4 + 1.5 * v.to(F64).abs()) * P.UNIT * ref.abs() + P.TINY)).max()
    print(f"SiLU form on [-80, 80]: the fp32 restatement reaches {float(r):.3f}")
    assert float(r) <= 0.5


def test_groupnorm_restatement():
    Y = [0.0, 0.0]
    for C, G in P.GN_SHAPES:
        for npix in P.GN_NPIX:
            P.accept_groupnorm("I", C, G, npix)
            x, gamma, beta, _ = P.groupnorm_inputs("I", C, G, npix)
            mean, var = P.groupnorm_stats(x, G)
            assert bool((var.sqrt().log2() == var.sqrt().log2().round()).all()) and bool((mean == mean.round()).all()), "family I: mean an integer, sigma a power of two"
            for offset in (False, True):
                worst, y = P.accept_groupnorm("R", C, G, npix, offset)
                assert max(worst) <= 0.5
                Y = [max(a, b) for a, b in zip(Y, y)]
    print(f"groupnorm: Y mul = {Y[0]:.2e}, add = {Y[1]:.2e}")
    assert 0 < max(Y) < 3e-7


def test_softmax_restatement():
    Y, worst_of = 0.0, {}
    for N in P.SOFTMAX_N:
        for M in P.SOFTMAX_M:
            for scale in P.SOFTMAX_SCALES:
                for A in P.SOFTMAX_A:
                    worst, y = P.accept_softmax(P.softmax_inputs(M, N, scale, A), scale, None, f"softmax_rows N={N} M={M} scale={scale:.4f} A={A}", every=True)
                    assert worst <= 0.5
                    Y, worst_of[(N, A)] = max(Y, y), max(worst, worst_of.get((N, A), 0.0))
    print("softmax_rows: Y = %.2e; worst |d| / bound by (N, A): %s" % (Y, {k: round(v, 3) for k, v in worst_of.items()}))
    assert 0 < Y < 3e-6
    Yc = 0.0
    for hw, frames, N, n_keys, _ in P.CAUSAL_CASES:
        for scale, A in ((0.25, 40), (1 / math.sqrt(384), 3)):
            worst, y = P.accept_softmax(P.causal_inputs(hw, frames, N, n_keys, scale, A), scale, P.causal_valid(N, N, hw, n_keys), f"causal hw={hw} frames={frames} N={N}", every=True)
            assert worst <= 0.5
            Yc = max(Yc, y)
    print(f"softmax_rows_causal: Y = {Yc:.2e}")
    assert 0 < Yc < 3e-6


def test_softmax_family_I():
    for N, valid in ((64, 64), (1028, 1028), (608, 300), (15, 5)):
        for c in (0.0, 3.0, -1000.0):
            s = torch.full((2, N), c)
            s[:, valid:] = P.LOUD
            v = torch.full((2,), valid)
            out = P.softmax_rows(s, 0.25, v, dtype=F32)
            want = torch.zeros(2, N)
            want[:, :valid] = torch.tensor(1.0) / torch.tensor(float(valid))
            assert torch.equal(out, want) and torch.equal(P.softmax_rows(s, 0.25, v).to(F32), want)
        s = torch.randn(2, N)
        s[:, valid // 2] += 1e4
        out = P.softmax_rows(s, 0.25, torch.full((2,), valid), dtype=F32)
        want = torch.zeros(2, N)
        want[:, valid // 2] = 1.0
        assert torch.equal(out, want)
    s = torch.randn(5, 16)
    assert float(P.softmax_rows(s, 0.25, P.causal_valid(5, 16, 1, 5), dtype=F32)[0, 0]) == 1.0


def test_blend_restatement():
    Y = 0.0
    for axis in (0, 1, 2):
        for e in P.BLEND_EXTENTS_I:
            P.accept_blend("I", axis, e)
        for e in P.BLEND_EXTENTS_R:
            worst, y = P.accept_blend("R", axis, e)
            assert worst <= 0.5
            Y = max(Y, y)
    print(f"blend_axis: Y = {Y:.2e}")
    assert 0 < Y < 1e-7


# ------------------------------------------------------------------------------------------------------------------- wrong kernels
def rejected(fn, case):
    with pytest.raises(P.Reject):
        fn()
        pytest.fail(f"the wrong kernel passes on {case}")


def test_wrong_kernels_are_rejected():
    geom = (2, 3, 5)
    # the fourth chunk step dropped
    m = P.Mode(a=True, b=True)
    x, gamma, a, b = P.prep_inputs("I", 1024, geom, m)
    assert P.lpp_of(1024, False) == 64 and P.lpp_of(128, False) == 32 and [P.lpp_of(c, True) for c in (96, 192, 384)] == [8, 16, 32]
    rejected(lambda: P.accept_prep("f32", "I", 1024, geom, m, got=P.vae_prep(x, gamma, a, b, dtype=F32, mut="drop_k3", lpp=64)), "vae_prep f32 I C=1024 a+b")
    mg = P.Mode(gamma=True)
    x, gamma, a, b = P.prep_inputs("R", 1020, geom, mg)
    rejected(lambda: P.accept_prep("f32", "R", 1020, geom, mg, got=P.vae_prep(x, gamma, dtype=F32, mut="drop_k3", lpp=64)), "vae_prep f32 R C=1020 gamma")
    # upsample writes 3 of the 4 pixels
    mu = P.Mode(up=True)
    x, gamma, a, b = P.prep_inputs("I", 16, geom, mu)
    rejected(lambda: P.accept_prep("f32", "I", 16, geom, mu, got=P.vae_prep(x, upsample=True, dtype=F32, mut="up3")), "vae_prep f32 I C=16 up")
    # up_t duplicates frame 0
    ex = P.Ex(add=True, up_t=True)
    x, mul, add = P.ex_inputs("I", 8, geom, ex)
    rejected(lambda: P.accept_ex("f32", "I", 8, geom, ex, got=P.vae_prep_ex(x, mul, add, up_t_=True, dtype=F32, mut="up_t_dup0")), "vae_prep_ex f32 I C=8 (2,3,5) add+up_t")
    # pad channels zero-filled
    x, gamma, a, b = P.prep_inputs("I", 96, geom, P.Mode())
    buf, view = P.framed(*geom, 128, 1, F16)
    view[..., :96] = P.vae_prep_f16(x, dtype=F32)
    assert P.frame_intact(buf, 1, 96)
    view[..., 96:] = 0
    assert not P.frame_intact(buf, 1, 96), "the wrong kernel passes on vae_prep f16 C=96 pixel stride 128"
    # split without saturation
    xs = P.with_specials(x)
    rejected(lambda: P.check_exact(P.vae_prep_split_f16(xs, dtype=F32, mut="split_nosat"), P.vae_prep_split_f16(xs), "split"), "vae_prep split I C=96 specials")
    # causal softmax
    hw, frames, N, n_keys, _ = P.CAUSAL_CASES[1]
    s, valid = P.causal_inputs(hw, frames, N, n_keys, 0.25, 40), P.causal_valid(N, N, hw, n_keys)
    for mut in ("valid_frame", "valid_key"):
        wrong = P.softmax_rows(s, 0.25, P.causal_valid(N, N, hw, n_keys, mut), dtype=F32)
        rejected(lambda: P.accept_softmax(s, 0.25, valid, mut, got=wrong), f"softmax_rows_causal (6, 3, 32, 18, 32): {mut}")
    for mut in ("max_all", "masked_unnormalised"):
        wrong = P.softmax_rows(s, 0.25, valid, dtype=F32, mut=mut)
        rejected(lambda: P.accept_softmax(s, 0.25, valid, mut, got=wrong), f"softmax_rows_causal (6, 3, 32, 18, 32): {mut}")
    # GroupNorm
    for mut, (C, G, npix) in (("grp_shift", (128, 32, 7)), ("count_pad", (96, 8, 7))):
        x, gamma, beta, eps = P.groupnorm_inputs("I", C, G, npix)
        wrong = P.groupnorm_affine(x, G, gamma, beta, eps, dtype=F32, mut=mut)
        rejected(lambda: P.accept_groupnorm("I", C, G, npix, got=wrong), f"groupnorm I C={C} G={G} npix={npix}: {mut}")
    x, gamma, beta, eps = P.groupnorm_inputs("R", 96, 8, 1000, offset=True)
    wrong = P.groupnorm_affine(x, 8, gamma, beta, eps, dtype=F32, mut="acc_fp32")
    rejected(lambda: P.accept_groupnorm("R", 96, 8, 1000, True, got=wrong), "groupnorm R C=96 G=8 npix=1000 offset: fp32 accumulation")
    # blend
    for mut in ("w_extent_m1", "src_m1"):
        a_, b_ = P.blend_inputs("I", 1, 4)
        rejected(lambda: P.accept_blend("I", 1, 4, got=P.blend_axis(a_, b_, 1, 4, dtype=F32, mut=mut)), f"blend_axis I axis=1 extent=4: {mut}")
    # replicate border
    for mut, case in (("lead_from_0", (1, 1, 5, 6, 4)), ("border_far", (0, 1, 5, 6, 4))):
        before, want = P.border_buffers(*case)
        P.check_bits(P.replicate_border(before, case[0], case[1]), want, "replicate_border")
        rejected(lambda: P.check_bits(P.replicate_border(before, case[0], case[1], mut), want, mut), f"replicate_border {case}: {mut}")
