"""tests/vae_conv_ref.py checked without a GPU: the float64 reference against F.conv3d / F.conv2d(stride=2) in float64 for every kernel size, epilogue and
flag of the GPU module (time-split, polyphase decomposition and separate cache included), the hi/lo split restated by hand, the premises of family I
(integers below 2^24, both clamp sides and the interior), the fp32 emulations of a correct kernel inside both rules of family R, and fourteen
kinds of subtly WRONG kernel (fifteen emulations: bias and resid shift separately), each rejected at every case of the GPU module at which it can occur — the structural ones by family I, the
precision ones by family R.  These rejections are the evidence that tests/test_gpu_vae_conv_fp64.py would fail on such a kernel: deliberately
broken kernels are never run on a GPU."""
import pytest
import torch
import torch.nn.functional as F

from tests import vae_conv_ref as V

_INPUTS = {}


def inputs(family, sp, scale="n1"):
    key = (family, sp, scale)
    if key not in _INPUTS:
        _INPUTS[key] = V.Inputs(family, sp, scale=scale)
    return _INPUTS[key]


def _conv3d_ref(inp):
    """The case through torch's own convolution in float64 (NCDHW), the epilogue written out as the existing GPU tests do."""
    sp = inp.spec
    kt, kh, kw = sp.k
    x, w = inp.x.double(), inp.w.double().permute(0, 4, 1, 2, 3)  # [Cout, Cin, kt, kh, kw]
    if sp.op in V.S2_OPS:
        y = F.conv2d(F.pad(x.permute(0, 3, 1, 2), (0, 1, 0, 1)), w[:, :, 0], stride=2).permute(0, 2, 3, 1)
    else:
        xin = F.pad(x.permute(3, 0, 1, 2), (kw // 2, kw // 2, kh // 2, kh // 2, 0, 0))
        y = F.conv3d(xin.unsqueeze(0), w)[0].permute(1, 2, 3, 0)
    if sp.bias:
        y = y + inp.bias.double()
    if sp.resid:
        y = y + inp.resid.double()
    if sp.flags & V.CLAMP:
        y = y.clamp(-1, 1)
    if sp.flags & V.TSPLIT:
        C = sp.Cout // 2
        y = y.permute(3, 0, 1, 2).reshape(2, C, sp.T, *y.shape[1:3])
        y = torch.stack((y[0], y[1]), dim=2).reshape(C, 2 * sp.T, *y.shape[3:]).permute(1, 2, 3, 0)
    return y


def test_reference_equals_torch_convolutions():
    """One case of every (entry, kernel size, flags, bias?, resid?, cache?) of the GPU module, family R: 1e-12 of the largest |t|."""
    seen = set()
    for sp in V.ALL_SPECS:
        key = (sp.op, sp.k, sp.flags & (V.CLAMP | V.TSPLIT), sp.bias, sp.resid, sp.cache, bool(sp.C))
        if key in seen or V.n_out(sp) > 60000:
            continue
        seen.add(key)
        inp = inputs("R", sp)
        ref = _conv3d_ref(inp)
        assert ref.shape == inp.t.shape
        assert float((ref - inp.t).abs().max()) <= 1e-12 * max(1.0, float(inp.pre.abs().max())), V.name_of(sp)
    assert len(seen) >= 20 and {k[1] for k in seen} >= {(1, 1, 1), (3, 1, 1), (1, 3, 3), (3, 3, 3)}


def test_separate_cache_is_the_same_convolution():
    """cache [kt - 1 frames] + frames [T] is the convolution of their concatenation, and frame f reads 2, 1, 0 cached frames for f = 0, 1, 2."""
    sp = V.HALO128_CACHED[0]
    inp = inputs("R", sp)
    cache, frames = inp.x[:2].double(), inp.x[2:].double()
    xin = F.pad(torch.cat([cache, frames]).permute(3, 0, 1, 2), (1, 1, 1, 1, 0, 0))
    ref = (F.conv3d(xin.unsqueeze(0), inp.w.double().permute(0, 4, 1, 2, 3))[0].permute(1, 2, 3, 0) + inp.bias.double() + inp.resid.double()).clamp(-1, 1)
    assert float((ref - inp.t).abs().max()) <= 1e-12 * float(inp.pre.abs().max())
    other = V.emulate(inp, mut="cache_from_xp").double()
    differs = [(other[f] != V.emulate(inp)[f].double()).any().item() for f in range(sp.T)]
    assert differs == [True, True, False, False]


def test_polyphase_decomposition_equals_the_stride_2_convolution():
    """vae_enc.py's four phase convolutions (2x2, 2x1, 1x2, 1x1 kernels over the rows a::2 and columns b::2 of the zero-padded frame) summed."""
    for T, Hin, Win, C, Cout in V.POLYPHASE:
        inp = inputs("R", V.Spec("p32", T, Hin, Win, C, Cout))
        ho, wo = Hin // 2, Win // 2
        buf = torch.zeros(T, 2 * ho + 1, 2 * wo + 1, C, dtype=V.F64)
        buf[:, : min(Hin, 2 * ho + 1), : min(Win, 2 * wo + 1)] = inp.x.double()[:, : 2 * ho + 1, : 2 * wo + 1]
        total = inp.bias.double().expand(T, ho, wo, Cout).clone()
        for a in (0, 1):
            for b in (0, 1):
                wph = inp.w.double()[:, :, a::2, b::2]
                total += V.conv64(buf[:, a::2, b::2], wph, T, ho, wo)
        assert float((total - inp.t).abs().max()) <= 1e-12 * float(inp.pre.abs().max()), (Hin, Win)


def test_split_restated_by_hand():
    x = torch.tensor([1.0 + 2.0 ** -12, 0.1, -3.3, 7.0e4, -2.0e5, 2.0 ** -20])
    p = V.split_x(x)
    hi = x.clamp(-65504, 65504).half()
    assert torch.equal(p[:6], hi) and float(p[0]) == 1.0 and float(p[3]) == 65504.0 and float(p[4]) == -65504.0
    assert torch.equal(p[6:12], (hi.float() / 4096).half()) and float(p[6]) == 2.0 ** -12
    assert torch.equal(p[12:], (x.clamp(-131008, 131008) - hi.float()).half()) and float(p[12]) == 2.0 ** -12 and float(p[16]) == -65504.0
    w = torch.tensor([0.3, -0.01, 1.0 + 2.0 ** -13])
    q = V.split_w(w)
    assert torch.equal(q[:3], w.half()) and torch.equal(q[6:], w.half()) and torch.equal(q[3:6], ((w - w.half().float()) * 4096).half()) and float(q[5]) == 0.5
    # hi + lo carries ~22 bits: the three products of the planes restore x . w to 2^-21
    got = (p[:3].double() * q[:3].double() + p[6:9].double() * q[3:6].double() + p[12:15].double() * q[6:9].double())
    assert float(((got - x[:3].double() * w.double()) / (x[:3].double() * w.double())).abs().max()) < 2.0 ** -20


def test_dispatch_restated():
    B = V.body_of
    assert B("f16", 33, 64, 96, (3, 3, 3), 0) == "halo128 NCB6" and B("f16", 33, 64, 256, (1, 3, 3), V.CLAMP) == "halo128 NCB8" and B("f16", 16, 64, 3, (1, 3, 3), 16) == "halo128 NCB1"
    assert B("f16", 33, 64, 96, (3, 3, 3), V.HALO64) == "halo64 NF3" and B("f16", 33, 64, 40, (3, 3, 3), 0) == "halo64 NF2" and B("f16", 16, 64, 100, (1, 3, 3), 0) == "halo64 NF4"
    assert B("f16", 15, 64, 96, (3, 3, 3), 0) == "pertap f16 NF3 KC64" and B("f16", 33, 64, 64, (3, 1, 1), V.TSPLIT) == "pertap f16 NF2 KC64"
    assert B("f16", 33, 64, 128, (3, 3, 3), V.PER_TAP) == "pertap f16 NF4 KC64" and B("f32", 5, 48, 32, (1, 1, 1), 0) == "pertap f32 NF1 KC16"
    want = {f"pertap f32 NF{nf} KC{kc}" for nf in (1, 2, 3, 4) for kc in (16, 32)} | {f"pertap f16 NF{nf} KC64" for nf in (1, 2, 3, 4)} | \
           {f"halo64 NF{nf}" for nf in (1, 2, 3, 4)} | {f"halo128 NCB{n}" for n in (6, 8, 1)} | {"s2 16x16x96"}
    assert {V.body(sp) for sp in V.ALL_SPECS} == want
    for ncb in (6, 8):
        assert {V.n_slabs(sp) for sp in V.HALO128_SPECS if V.body(sp) == f"halo128 NCB{ncb}"} >= {1, 2, 3, 4, 9}
    assert all(V.cached_ok(sp) for sp in V.HALO128_CACHED)


def test_dispatch_of_the_released_vaes():
    """Every 16-bit 3x3 convolution of the Wan decoder and encoder (dim 96, split operands: 3 C planes in a 64-channel-padded pixel, vae.py Decoder3d._setup)
    and of the HunyuanVideo decoder (fp16 operands, hunyuan_vae.py) at the 720p widths of its stage takes the 128-pixel body — but the Wan encoder's head
    (384 -> 32 couts), the one launch of the 64-pixel body in a released model."""
    from lightx2v_amd import synth

    W0 = 1280 // 8  # the latent's width
    split = lambda c: (3 * c + 63) // 64 * 64
    convs = []  # (name, W, Cin of the operand buffer, Cout, k)

    def wan_res(name, w, cin, cout):
        convs.extend([(name + "residual.2", w, split(cin), cout, (3, 3, 3)), (name + "residual.6", w, split(cout), cout, (3, 3, 3))])

    dims, plan = synth.wan_vae_decoder_plan(96)  # conv1 (Cin = 16) is an fp32 convolution
    w = W0
    for m in (0, 2):
        wan_res(f"decoder.middle.{m}.", w, dims[0], dims[0])
    for idx, kind, cin, cout in plan:
        if kind == "res":
            wan_res(f"decoder.upsamples.{idx}.", w, cin, cout)
        else:  # nearest upsampling, then a 3x3 convolution per frame (the time_conv is 3x1x1)
            w *= 2
            convs.append((f"decoder.upsamples.{idx}.resample.1", w, split(cin), cin // 2, (1, 3, 3)))
    convs.append(("decoder.head.2", w, split(dims[-1]), 3, (3, 3, 3)))
    assert w == 1280

    dims, plan = synth.wan_vae_encoder_plan(96)
    convs.append(("encoder.conv1", w, 64, dims[0], (3, 3, 3)))
    for idx, kind, cin, cout in plan:
        if kind == "res":
            wan_res(f"encoder.downsamples.{idx}.", w, cin, cout)
        else:  # the stride-2 kernel (and a 3x1x1 time_conv)
            w //= 2
    for m in (0, 2):
        wan_res(f"encoder.middle.{m}.", w, dims[-1], dims[-1])
    head = ("encoder.head.2", w, split(dims[-1]), 32, (3, 3, 3))
    convs.append(head)
    assert w == W0

    def hy_res(name, w, cin, cout):
        convs.extend([(name + "conv1", w, cin, cout, (3, 3, 3)), (name + "conv2", w, cout, cout, (3, 3, 3))])

    cfg = synth.HUNYUAN_VAE_CFG  # conv_in (Cin = 16) is an fp32 convolution
    top = cfg["block_out_channels"][-1]
    for m in (0, 1):
        hy_res(f"decoder.mid_block.resnets.{m}.", w, top, top)
    for i, (cin, cout, _, fhw, has_up) in enumerate(synth.hunyuan_vae_up_plan(cfg)):
        for j in range(cfg["layers_per_block"] + 1):
            hy_res(f"decoder.up_blocks.{i}.resnets.{j}.", w, cin if j == 0 else cout, cout)
        if has_up:
            w *= fhw
            convs.append((f"decoder.up_blocks.{i}.upsamplers.0", w, cout, cout, (3, 3, 3)))
    convs.append(("decoder.conv_out", w, cfg["block_out_channels"][0], 3, (3, 3, 3)))
    assert w == 1280

    assert len(convs) == (2 * 14 + 3 + 1) + (1 + 2 * 10 + 1) + (2 * 14 + 3 + 1)  # residual blocks x 2, upsamplers, conv1 / heads
    bodies = {c[0]: V.body_of("f16", *c[1:], 0) for c in convs if c is not head}
    assert set(bodies.values()) == {"halo128 NCB6", "halo128 NCB8", "halo128 NCB1"}, {n: b for n, b in bodies.items() if not b.startswith("halo128")}
    assert all(c[2] % 64 == 0 for c in convs) and V.body_of("f16", *head[1:], 0) == "halo64 NF1"


def test_family_i_premises_and_emulations_at_the_largest_k():
    for sp in V.ALL_SPECS:
        inputs("I", sp).assert_premises()
    assert V.LARGEST_K == 27 * 512 and 8 * 4 * V.LARGEST_K + 400 < 2 ** 24
    for sp in V.DEEP_SPECS:
        inp = inputs("I", sp)
        inp.assert_premises()
        assert inp.K == V.LARGEST_K or sp.op == "s2"
        fp32_steps = V._accumulate(inp.xpad(), inp.w.to(V.F64), sp.T, inp.Ho, inp.Wo, inp.stride, "slab", V.slab_of(sp)) + inp.bias + inp.resid if sp.resid else None
        assert torch.equal(V.emulate(inp, "chain"), inp.t.float()) and torch.equal(V.emulate(inp, "slab"), inp.t.float()) and (fp32_steps is None or torch.equal(fp32_steps, inp.t.float()))
        for mut in ("drop_last_slab", "slab_twice"):
            assert not torch.equal(V.emulate(inp, mut=mut), inp.t.float())
    with pytest.raises(AssertionError):
        V.Inputs("I", V.Spec("f32", 1, 2, 2, 2 ** 19, 4))  # 8 * 4 * K reaches 2^24


def test_family_r_emulations_pass_both_rules():
    """Every emulation of a correct kernel, at every case: inside the per-element bound (the yardstick is their own maximum); the clamp cases hold
    both sides and the interior."""
    c = V.Case("host", record=False)
    for sp in V.ALL_SPECS:
        inp = inputs("R", sp)
        inp.assert_premises()
        for order, got in inp.emulations().items():
            c.check_bound(got, inp, V.body(sp), order)
    assert 0 < c.worst_bound < 0.5 and 0 < c.worst_yardstick <= 1.0
    # the yardstick grows with K like an fp32 chain's error does
    ys = {inputs("R", sp).K: inputs("R", sp).yardstick() for sp in (V.F32_K_LOOP[1], V.HALO128_CACHED[2])}
    assert ys[32] < 2e-7 and 4e-7 < ys[2592] < 2e-6


@pytest.mark.parametrize("mut", V.STRUCTURAL)
def test_family_i_rejects_structural_mutations(mut):
    n = 0
    for sp in V.ALL_SPECS:
        if not V.applicable(mut, sp):
            continue
        inp = inputs("I", sp)
        with pytest.raises(V.Reject) as e:
            V.Case("host", record=False).check_exact(V.emulate(inp, mut=mut), inp, V.body(sp), mut)
        assert e.value.criterion == "exact", (mut, V.name_of(sp))
        n += 1
    assert n >= 3, f"{mut} occurs at {n} cases only"


@pytest.mark.parametrize("mut", V.PRECISION)
def test_family_r_rejects_precision_mutations(mut):
    n, ratios = 0, []
    for sp in V.ALL_SPECS:
        if not V.applicable(mut, sp):
            continue
        inp = inputs("R", sp)
        c = V.Case("host", record=False)
        with pytest.raises(V.Reject) as e:
            c.check_bound(V.emulate(inp, mut=mut), inp, V.body(sp), mut)
        assert e.value.criterion in ("bound", "yardstick"), (mut, V.name_of(sp))
        ratios.append(c.worst_yardstick)
        n += 1
    assert n >= 3 and min(ratios) > 10 * V.MARGIN, f"{mut}: {n} cases, smallest relL2 / Y = {min(ratios):.1f}"


@pytest.mark.parametrize("scale", V.SPLIT_SCALES)
def test_split_end_to_end_yardstick_and_its_mutation(scale):
    """The planes' convolution is fp32-grade against the UNROUNDED operands' float64 result; without the x_hi . w_lo term it is 100 x off."""
    for sp in V.SPLIT_E2E:
        inp = inputs("R", sp, scale)
        if scale == "small":
            mid = inp.x[..., sp.C : 2 * sp.C].float().abs()
            assert float(((mid > 0) & (mid < 2.0 ** -14)).float().mean()) > 0.95
        Y, c = inp.yardstick_unrounded(), V.Case("host", record=False)
        c.check_bound(V.emulate(inp), inp, V.body(sp), "e2e", t=inp.t_unrounded, Y=Y)
        with pytest.raises(V.Reject) as e:
            c.check_bound(V.emulate(inp, mut="split_drop"), inp, V.body(sp), "e2e", t=inp.t_unrounded, Y=Y)
        assert e.value.criterion == "yardstick" and c.rows[-1][4]["rel_l2_over_Y"] > 50


def test_a_structural_mutation_is_also_outside_family_r():
    """A dropped tap is no rounding error: family R's bound sees it too (family I is what guarantees it)."""
    sp = V.HALO64_SPECS[0]
    inp = inputs("R", sp)
    with pytest.raises(V.Reject):
        V.Case("host", record=False).check_bound(V.emulate(inp, mut="drop_tap"), inp)
