"""The fused fp16 wide-head attention of the HunyuanVideo VAE mid block (csrc/vae_attn.hip, lib.vae_attention16) against a float64 masked softmax over
the fp16-rounded operands, and the decoder with attn16=True against the reference-generated fixture and the CPU oracle.
Bound of the kernel test: max |out - ref| <= 2^-10 max |v| — each p is rounded to fp16 (relative error <= 2^-11) and a row of the output is a convex
combination of v rows, so P contributes <= 2^-11 max |v|; the second factor of two covers fp32 accumulation and the hardware exp2.  A wrong mask or a
dropped tile is an O(1) error."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

CASES = [(128, 24, 3), (512, 24, 3), (512, 64, 2), (512, 288, 2), (512, 40, 1), (128, 5, 7), (512, 100, 3)]  # (C, hw, frames)


@pytest.mark.parametrize("gain", [1.0, 6.0])
@pytest.mark.parametrize("C,hw,frames", CASES)
def test_vae_attention16_vs_float64(C, hw, frames, gain):
    from lightx2v_amd import lib

    n = hw * frames
    qkv = torch.randn(n, 3 * C, generator=torch.Generator().manual_seed(C + hw + frames))
    qkv[n - hw :, C : 2 * C] *= gain  # the keys of the last frame: the running maximum rises late in the walk
    q, k, v = (t.half().double() for t in qkv.split(C, dim=1))
    frame = torch.arange(n) // hw
    s = (q @ k.t()) / math.sqrt(C)
    ref = torch.where(frame[None, :] <= frame[:, None], s, torch.tensor(float("-inf"), dtype=torch.float64)).softmax(-1) @ v

    bufs = lib.vae_attention16_buffers(n, C, "cuda")
    for b in bufs:
        b.fill_(float("nan"))
    out = torch.full((n, C), float("nan"), device="cuda")
    lib.vae_attention16(qkv.cuda(), n, C, hw, 1.0 / math.sqrt(C), out, buffers=bufs)
    got = out.double().cpu()
    assert torch.isfinite(got).all()
    d = (got - ref).abs().max().item()
    bound = 2.0**-10 * v.abs().max().item()
    print(f"vae_attention16 C={C} hw={hw} frames={frames} gain={gain:g}: max|d| {d:.3e} (bound {bound:.3e}) rel L2 {((got - ref).norm() / ref.norm()).item():.3e}")
    assert d <= bound


def _check(got, ref, what, atol=1e-2, rel=5e-3):  # the project's stated tolerance of its fp16-operand mode (tests/test_gpu_hunyuan_vae.py)
    got, ref = got.float().cpu(), ref.float().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    d = (got - ref).abs().max().item()
    r = ((got - ref).norm() / ref.norm().clamp_min(1e-30)).item()
    print(f"{what}: max abs {d:.3e}, rel L2 {r:.3e}")
    assert d <= atol and r <= rel, f"{what}: max abs {d:.3e}, rel L2 {r:.3e}"


def test_hunyuan_vae_attn16_vs_reference_fixture():
    from tests.util import load_golden

    from lightx2v_amd import hunyuan_vae, synth

    gld = load_golden("hunyuan_vae_tiny")
    cfg = synth.HUNYUAN_VAE_TINY_CFG
    vae = hunyuan_vae.VideoEncoderKLCausal3DModel(synth.synth_hunyuan_vae_weights(cfg, seed=1), cfg, conv16=False, attn16=True)
    _check(vae.decode(gld["z_tiled"].cuda()), gld["image_tiled"], "Hunyuan VAE tiled decode (attn16) vs reference fixture")
    assert vae.model.decoder.attn_ran == "fused-fp16"
    _check(vae.decode(gld["z_single"].cuda()), gld["image_single"], "Hunyuan VAE single-tile decode (attn16) vs reference fixture")


def test_hunyuan_vae_attn16_real_widths_vs_oracle():
    from lightx2v_amd import hunyuan_vae, synth
    from oracle import hunyuan_vae_oracle as V

    cfg = synth.HUNYUAN_VAE_CFG
    sd = synth.synth_hunyuan_vae_weights(cfg, seed=2)
    z = torch.randn(1, 16, 2, 4, 8, generator=torch.Generator().manual_seed(4)) * 0.5
    with torch.no_grad():
        ref = V.vae_decode(sd, z, cfg)
    vae = hunyuan_vae.VideoEncoderKLCausal3DModel(sd, cfg, attn16=True)
    _check(vae.decode(z.cuda()), ref, "Hunyuan VAE decode (released widths, attn16)")
    assert vae.model.decoder.attn_ran == "fused-fp16"
