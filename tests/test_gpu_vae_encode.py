"""Wan VAE encode on the HIP kernels (csrc/vae_enc.hip, lightx2v_amd/vae_enc.py) against
  * torch's conv2d / conv3d (fp64) for the stride-2 kernel, the video producer and the time convolution,
  * the fixture generated from the unmodified reference (tests/golden/wan_vae_encode_tiny.*.safetensors),
  * the CPU restatement (tests/wan_vae_encode_restatement.py, pinned to that fixture) at the released widths.
The encoder is fp32 in the reference (vae.py:794); the default hi/lo split mode is held to the decode's fp32-grade bar: |d| <= 2e-3 and relative
L2 <= 1e-3 on the latents, atol 2e-5 / relative L2 2e-6 on a single split convolution."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _check(got, ref, what, atol=2e-3, rel=1e-3):
    got, ref = got.float().cpu(), ref.float().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite values"
    d = (got - ref).abs().max().item()
    r = ((got - ref).norm() / ref.norm().clamp_min(1e-30)).item()
    assert d <= atol and r <= rel, f"{what}: max abs {d:.3e}, rel L2 {r:.3e}"


def _s2_case(x, w, b, split=True):
    """x [T, H, W, C] fp32 (CPU), w [Cout, C, 3, 3] → (HIP output, fp64 reference); the output goes into an oversized NaN-poisoned buffer whose tail must
    stay untouched."""
    from lightx2v_amd import lib
    from lightx2v_amd.vae import _split16

    T, H, W, C = x.shape
    cout = w.shape[0]
    ref = F.conv2d(F.pad(x.permute(0, 3, 1, 2).double(), (0, 1, 0, 1)), w.double(), b.double(), stride=2).permute(0, 2, 3, 1).float()
    cs = ((3 * C if split else C) + 31) // 32 * 32
    buf = torch.zeros(T, H, W, cs, dtype=torch.float16, device="cuda")
    lib.vae_prep(x.cuda(), buf, (H * W * cs, W * cs), split=split)
    w16 = _split16(w.permute(0, 2, 3, 1).contiguous().cuda(), cs, split)
    n = T * (H // 2) * (W // 2) * cout
    store = torch.full((n + 4096,), float("nan"), device="cuda")
    out = store[:n].view(T, H // 2, W // 2, cout)
    lib.vae_conv_s2(buf, w16, out, bias=b.cuda())
    torch.cuda.synchronize()
    assert torch.isnan(store[n:]).all(), "the stride-2 kernel wrote past its output"
    return out, ref


def test_conv_s2_matches_conv2d():
    """x2v_vae_conv_s2_f16 in the hi/lo split mode vs F.conv2d(F.pad(x, (0, 1, 0, 1)), w, stride=2) in fp64: Cout 96 / 192 / 384, a Cout tail (100), even and odd
    H, W, one to three frames, and activations whose middle plane hi * 2^-12 is an fp16 subnormal; plain fp16 operands at their own bar."""
    g = torch.Generator().manual_seed(3)
    for T, H, W, C, cout in [(2, 36, 64, 96, 96), (1, 37, 45, 96, 96), (3, 20, 33, 192, 192), (1, 18, 22, 384, 384), (2, 9, 17, 32, 100), (1, 2, 2, 64, 96),
                             (1, 70, 35, 96, 96)]:
        x = torch.randn(T, H, W, C, generator=g) * 2
        w = torch.randn(cout, C, 3, 3, generator=g) / (9 * C) ** 0.5
        b = torch.randn(cout, generator=g)
        out, ref = _s2_case(x, w, b)
        _check(out, ref, f"stride-2 split conv T={T} {H}x{W} C={C} Cout={cout}", atol=2e-5, rel=2e-6)
    T, H, W, C, cout = 2, 17, 40, 96, 96
    x = (torch.rand(T, H, W, C, generator=g) * (0.25 - 1e-3) + 1e-3) * (torch.randint(0, 2, (T, H, W, C), generator=g) * 2 - 1)
    w = torch.randn(cout, C, 3, 3, generator=g) / (9 * C) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    out, ref = _s2_case(x, w, b)
    _check(out, ref, "stride-2 split conv, subnormal middle plane", atol=2e-5, rel=2e-6)
    x = torch.randn(1, 21, 30, 96, generator=g)
    out, ref = _s2_case(x, torch.randn(96, 96, 3, 3, generator=g) / 864**0.5, torch.randn(96, generator=g), split=False)
    _check(out, ref, "stride-2 fp16 conv", atol=2e-2, rel=2e-3)


def test_video_prep_conv1_and_time_conv():
    """conv1 (Cin = 3) from the caller's [3, T, H, W] video through x2v_vae_video_prep (split into a 64-channel pixel, the zero tail skipped; fp32 into 16
    channels) vs F.conv3d with the causal zero pad; the (3,1,1) stride-2 time convolution as one launch per output frame vs F.conv3d(stride=(2, 1, 1))."""
    from lightx2v_amd import lib
    from lightx2v_amd.vae import _split16

    g = torch.Generator().manual_seed(4)
    T, H, W = 5, 20, 36
    video = torch.rand(3, T, H, W, generator=g) * 2 - 1
    w = torch.randn(96, 3, 3, 3, 3, generator=g) / 81**0.5
    b = torch.randn(96, generator=g) * 0.1
    ref = F.conv3d(F.pad(video, (1, 1, 1, 1, 2, 0)).unsqueeze(0).double(), w.double(), b.double())[0].permute(1, 2, 3, 0).float()
    wcl = w.permute(0, 2, 3, 4, 1).contiguous().cuda()
    vcuda = torch.zeros(3, T, H, W + 8, device="cuda")[..., :W]  # a strided view: the producer reads the video in place
    vcuda.copy_(video)
    for mode in ("split", "fp32"):
        c = 64 if mode == "split" else 16
        dt = torch.float16 if mode == "split" else torch.float32
        buf = torch.zeros(2 + T, H + 2, W + 2, c, dtype=dt, device="cuda")
        strides = ((H + 2) * (W + 2) * c, (W + 2) * c, c)
        lib.vae_video_prep(vcuda, buf[2:, 1 : 1 + H, 1 : 1 + W], split=mode == "split")
        out = torch.full((T, H, W, 96), float("nan"), device="cuda")
        if mode == "split":
            hi = video.permute(1, 2, 3, 0).half()
            got = buf[2:, 1 : 1 + H, 1 : 1 + W].cpu()
            assert torch.equal(got[..., :3], hi) and torch.equal(got[..., 3:6], (hi.float() / 4096).half())
            assert torch.equal(got[..., 6:9], (video.permute(1, 2, 3, 0) - hi.float()).half()) and not got[..., 9:].any()
            lib.vae_conv16(buf, strides, _split16(wcl, 64, True), out, T, H, W, bias=b.cuda(), flags=lib.VCONV_ZERO_TAIL32)
        else:
            assert torch.equal(buf[2:, 1 : 1 + H, 1 : 1 + W, :3].cpu(), video.permute(1, 2, 3, 0))
            lib.vae_conv(buf, strides, F.pad(wcl, (0, 13)).contiguous(), out, T, H, W, bias=b.cuda())
        _check(out, ref, f"conv1 from the video, {mode}", atol=2e-5, rel=2e-6)
    # time conv: [cache frame | 4 frames] → 2 frames
    T, H, W, C = 4, 6, 20, 192
    x = torch.randn(1 + T, H, W, C, generator=g)
    w = torch.randn(C, C, 3, 1, 1, generator=g) / (3 * C) ** 0.5
    b = torch.randn(C, generator=g)
    ref = F.conv3d(x.permute(3, 0, 1, 2).unsqueeze(0).double(), w.double(), b.double(), stride=(2, 1, 1))[0].permute(1, 2, 3, 0).float()
    cp = 3 * C
    buf = torch.zeros(1 + T, H, W, cp, dtype=torch.float16, device="cuda")
    strides = (H * W * cp, W * cp, cp)
    lib.vae_prep(x.cuda(), buf, strides[:2], split=True)
    w16 = _split16(w.permute(0, 2, 3, 4, 1).contiguous().cuda(), cp, True)
    out = torch.full((T // 2, H, W, C), float("nan"), device="cuda")
    for j in range(T // 2):
        lib.vae_conv16(buf[2 * j :], strides, w16, out[j : j + 1], 1, H, W, bias=b.cuda())
    _check(out, ref, "time conv (3,1,1) stride 2", atol=2e-5, rel=2e-6)


@pytest.fixture(scope="module")
def gold():
    from tests.util import load_golden

    return load_golden("wan_vae_encode_tiny")


def _tiny_sd(gold):
    from lightx2v_amd import synth

    return synth.synth_wan_vae_encoder_weights(dim=int(gold["dim"][0]), seed=int(gold["seed"][0])), int(gold["dim"][0])


def _inputs(gold):
    img = gold["image"]
    return {"video": gold["video"], "i2v": torch.cat([img[:, None], torch.zeros(3, 8, *img.shape[1:])], dim=1), "odd": gold["odd"]}


@pytest.mark.parametrize("conv16", ["split", False])
def test_encode_matches_reference_fixture(gold, conv16):
    """WanVAE.encode (default split mode, and the fp32 opt-in) vs the reference's fp32 WanVAE_.encode at dim 32 on the three fixture inputs (a 9-frame video,
    an i2v-shaped one, an odd-sized one): the decode's fp32-grade bar, |d| <= 2e-3 and relative L2 <= 1e-3."""
    from lightx2v_amd import vae

    sd, dim = _tiny_sd(gold)
    m = vae.WanVAE(sd, dim=dim, conv16=conv16)
    for name, x in _inputs(gold).items():
        z = m.encode([x.cuda()])
        assert isinstance(z, list) and len(z) == 1 and z[0].dtype == torch.float32
        _check(z[0], gold[f"mu_{name}"], f"encode {name} (conv16={conv16})")


def test_encode_fp16_operands_opt_in(gold):
    """conv16=True (fp16 operands, opt-in): the fp16 class of tolerance."""
    from lightx2v_amd import vae

    sd, dim = _tiny_sd(gold)
    z = vae.WanVAE(sd, dim=dim, conv16=True).encode([gold["video"].cuda()])[0]
    _check(z, gold["mu_video"], "encode, fp16 operands", atol=5e-2, rel=2e-2)


def test_encode_chunking_is_bit_identical(gold):
    """1 frame, then k frames per pass: k = 4 (the reference's), 8 and 16 give the same bits (time_conv sees the same windows; every kernel's reduction
    order is independent of the frames per launch).  Frames behind the last group of 4 are dropped, as by the reference."""
    from lightx2v_amd import vae

    sd, dim = _tiny_sd(gold)
    x = (torch.rand(3, 35, 48, 40, generator=torch.Generator().manual_seed(5)) * 2 - 1).cuda()
    m = vae.WanVAE(sd, dim=dim)
    outs = [m.model.encode(x[:, :33].unsqueeze(0), m.scale, chunk_frames=k) for k in (4, 8, 16)]
    assert outs[0].shape == (1, 16, 9, 6, 5)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert torch.equal(m.model.encode(x.unsqueeze(0), m.scale), outs[0])


def test_encode_real_widths_vs_restatement():
    """dim 96 (the released channel plan 96 / 96 / 192 / 384 / 384) on [3, 9, 128, 128] vs the CPU restatement: fp32-grade bar."""
    from lightx2v_amd import synth, vae
    from tests import wan_vae_encode_restatement as R

    sd = synth.synth_wan_vae_encoder_weights(dim=96, seed=2)
    x = torch.rand(3, 9, 128, 128, generator=torch.Generator().manual_seed(6)) * 2 - 1
    m = vae.WanVAE(sd, dim=96)
    with torch.no_grad():
        ref = R.encode(sd, x, m.mean.cpu(), m.inv_std.cpu(), dim=96)
    _check(m.encode([x.cuda()])[0], ref, "encode dim 96, 9 x 128 x 128")


def test_encode_720p_81f():
    """One 720p x 81-frame encode: [16, 21, 90, 160], finite; latent frame 0 depends on input frame 0 only (causal), so it must match the CPU restatement's
    encode of that frame alone."""
    from lightx2v_amd import synth, vae
    from tests import wan_vae_encode_restatement as R

    sd = synth.synth_wan_vae_encoder_weights(dim=96, seed=0)
    x = torch.rand(3, 81, 720, 1280, generator=torch.Generator().manual_seed(8)) * 2 - 1
    m = vae.WanVAE(sd, dim=96)
    z = m.encode([x.cuda()])[0]
    assert z.shape == (16, 21, 90, 160)
    assert torch.isfinite(z).all()
    with torch.no_grad():
        ref0 = R.encode(sd, x[:, :1].contiguous(), m.mean.cpu(), m.inv_std.cpu(), dim=96)
    _check(z[:, :1], ref0, "720p latent frame 0")


def test_i2v_conditioning_from_an_image_drives_the_tiny_model(gold):
    """run_vae_encoder's mirror on an image: mask in channels 0-3, encode() of [resized image | zero frames] in channels 4-19, bf16 — and it drives one
    wan-tiny-i2v forward."""
    from lightx2v_amd import scheduler, synth, vae, vae_enc, wan

    sd, dim = _tiny_sd(gold)
    m = vae.WanVAE(sd, dim=dim)
    dims = synth.WAN_DIMS["wan-tiny-i2v"]
    ts, frames = (16, 3, 8, 8), 9
    img = torch.rand(3, 50, 50, generator=torch.Generator().manual_seed(9)) * 2 - 1
    out, lat_h, lat_w = vae_enc.run_vae_encoder(m, img, target_height=64, target_width=64, target_video_length=frames)
    assert (lat_h, lat_w) == (8, 8) and out.shape == (20, 3, 8, 8) and out.dtype == torch.bfloat16
    assert torch.equal(out[:4].float().cpu(), vae_enc.i2v_first_frame_mask(frames, 8, 8))
    z = m.encode([vae_enc.i2v_video(img, frames, 8, 8, (4, 8, 8)).cuda()])[0]
    assert torch.equal(out[4:], z.to(torch.bfloat16))
    wd = {k: v.cuda() for k, v in synth.synth_wan_i2v_weights(dims, seed=0).items()}
    lat, ctx, ctx_null = synth.synth_inputs(dims, ts)
    image = {"clip_encoder_out": synth.synth_i2v_inputs(dims, ts)["clip_encoder_out"].cuda(), "vae_encode_out": out}
    cfg = wan.default_config(dims, task="i2v", in_dim=36, cross_attn_2_type="hip_flash", target_shape=ts, target_video_length=frames, infer_steps=2)
    model = wan.WanModel(cfg, wd)
    sch = scheduler.WanScheduler(cfg, device="cuda")
    sch.prepare(latents=lat)
    model.set_scheduler(sch)
    inputs = {"text_encoder_output": {"context": [c.cuda() for c in ctx], "context_null": [c.cuda() for c in ctx_null]}, "image_encoder_output": image}
    sch.step_pre(0)
    model.infer(inputs)
    assert torch.isfinite(sch.noise_pred.float()).all()
