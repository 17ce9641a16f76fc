"""Wan VAE encode, host side (no GPU): the CPU restatement against the reference fixture, run_vae_encoder's latent size and first-frame mask,
the chunk plan, and the new C-ABI entries' argument checks."""
import ctypes

import pytest
import torch

from lightx2v_amd import lib, synth, vae, vae_enc
from tests import wan_vae_encode_restatement as R
from tests.util import load_golden


@pytest.fixture(scope="module")
def gold():
    return load_golden("wan_vae_encode_tiny")


def _sd(gold):
    dim, seed = int(gold["dim"][0]), int(gold["seed"][0])
    sd = synth.synth_wan_vae_encoder_weights(dim=dim, seed=seed)
    checksum = sum((sd[k].double().abs().sum() for k in sorted(sd)), torch.zeros((), dtype=torch.float64)).reshape(1)  # oracle/gen_golden.py::weights_checksum
    assert torch.equal(checksum, gold["weights_checksum"]), "synth_wan_vae_encoder_weights drifted from the fixture"
    return sd, dim


@pytest.mark.parametrize("name", ["video", "i2v", "odd"])
def test_restatement_matches_reference_fixture(gold, name):
    sd, dim = _sd(gold)
    x = gold[name] if name != "i2v" else torch.cat([gold["image"][:, None], torch.zeros(3, 8, *gold["image"].shape[1:])], dim=1)
    with torch.no_grad():
        mu = R.encode(sd, x, gold["mean"], gold["inv_std"], dim=dim)
    ref = gold[f"mu_{name}"]
    assert mu.shape == ref.shape
    assert (mu - ref).abs().max().item() <= 1e-5


def test_encoder_plan_is_the_reference_module_tree():
    dims, plan = synth.wan_vae_encoder_plan(96)
    assert dims == [96, 96, 192, 384, 384]
    assert [k for _, k, _, _ in plan] == ["res", "res", "downsample2d", "res", "res", "downsample3d", "res", "res", "downsample3d", "res", "res"]
    assert [(i, ci, co) for i, _, ci, co in plan][3] == (3, 96, 192)
    sd = synth.synth_wan_vae_encoder_weights(dim=96)
    assert sd["encoder.downsamples.2.resample.1.weight"].shape == (96, 96, 3, 3) and "encoder.downsamples.2.time_conv.weight" not in sd
    assert sd["encoder.downsamples.5.time_conv.weight"].shape == (192, 192, 3, 1, 1)
    assert sd["encoder.head.2.weight"].shape == (32, 384, 3, 3, 3) and sd["conv1.weight"].shape == (32, 32, 1, 1, 1)
    assert not set(sd) & set(synth.synth_wan_vae_weights(dim=32))  # a separate stream from the decoder's weights


@pytest.mark.parametrize(
    "img_hw, target, lat",
    [
        ((720, 1280), (720, 1280), (90, 160)),  # 720p: sqrt(921600 * 0.5625) = 720 → 90; sqrt(921600 / 0.5625) = 1280 → 160
        # 480p: sqrt(399360 * (480 / 832)) is 479.99999999999994 in float64 → // 8 = 59 → 58 (patch 2): the reference's formula gives 58, not 60
        ((480, 832), (480, 832), (58, 104)),
        ((1000, 1000), (720, 1280), (120, 120)),  # square image at 720p: sqrt(921600) = 960 → 120
        ((600, 1000), (480, 832), (60, 100)),  # 489.5 // 8 = 61 → 60 (patch 2); 815.8 // 8 = 101 → 100
    ],
)
def test_i2v_latent_size(img_hw, target, lat):
    assert vae_enc.i2v_latent_hw(*img_hw, *target, (4, 8, 8), (1, 2, 2)) == lat


@pytest.mark.parametrize("frames, lat_hw", [(81, (90, 160)), (81, (58, 104)), (9, (4, 6))])
def test_i2v_first_frame_mask(frames, lat_hw):
    msk = vae_enc.i2v_first_frame_mask(frames, *lat_hw)
    t_lat = 1 + (frames - 1) // 4
    assert msk.shape == (4, t_lat, *lat_hw)
    want = torch.zeros(4, t_lat, *lat_hw)
    want[:, 0] = 1.0  # the 4 sub-frames of latent frame 0 are the given image (repeat_interleave of frame 0); every other frame is free
    assert torch.equal(msk, want)


def test_i2v_video_is_resized_image_plus_zero_frames():
    img = torch.rand(3, 37, 53) * 2 - 1
    v = vae_enc.i2v_video(img, 9, 4, 6, (4, 8, 8))
    assert v.shape == (3, 9, 32, 48) and v.dtype == torch.float32
    assert torch.equal(v[:, 0], torch.nn.functional.interpolate(img[None], size=(32, 48), mode="bicubic")[0])
    assert not v[:, 1:].any()


def test_encode_chunk_bounds():
    assert vae_enc.encode_chunk_bounds(1, 4) == [(0, 1)]
    assert vae_enc.encode_chunk_bounds(9, 4) == [(0, 1), (1, 5), (5, 9)]
    assert vae_enc.encode_chunk_bounds(81, 16)[:3] == [(0, 1), (1, 17), (17, 33)] and vae_enc.encode_chunk_bounds(81, 16)[-1] == (65, 81)
    assert vae_enc.encode_chunk_bounds(13, 8) == [(0, 1), (1, 9), (9, 13)]
    # as the reference (1 + (T - 1) // 4 passes): trailing frames behind the last whole group of 4 are not encoded
    assert vae_enc.encode_chunk_bounds(12, 4) == [(0, 1), (1, 5), (5, 9)] and vae_enc.encode_chunk_bounds(4, 4) == [(0, 1)]
    for bad in ((9, 6), (9, 0), (0, 4)):
        with pytest.raises(lib.X2VError):
            vae_enc.encode_chunk_bounds(*bad)


def test_encode_flops_720p():
    f = sum(vae_enc.encode_flops(81, 720, 1280).values())
    assert 3.7e14 < f < 3.9e14  # the issue's shape count: ~3.8e14


def test_encode_refusals_need_no_gpu():
    enc_sd = synth.synth_wan_vae_encoder_weights(dim=32)
    video = torch.zeros(3, 1, 16, 16)
    with pytest.raises(lib.X2VError, match="not built"):
        vae.WanVAE(enc_sd, dim=32, device="cpu", use_tiling=True).encode([video])
    with pytest.raises(lib.X2VError, match="no encoder"):  # a decode-only state dict
        vae.WanVAE(synth.synth_wan_vae_weights(dim=32), dim=32, device="cpu").encode([video])
    with pytest.raises(lib.X2VError, match="no decoder"):  # an encoder-only one
        vae.WanVAE(enc_sd, dim=32, device="cpu").decode(torch.zeros(16, 1, 2, 2))


def test_encoder_abi_argument_validation_needs_no_gpu():
    L = lib._lib
    a = ctypes.c_void_p(4096)
    # x2v_vae_conv_s2_f16(xp, fs, rs, ps, w, wrs, bias, y, T, Hin, Win, Cin, Cout, flags, stream)
    assert L.x2v_vae_conv_s2_f16(None, 4096, 512, 32, a, 288, None, a, 1, 8, 8, 32, 96, 0, None) == -5  # null
    assert L.x2v_vae_conv_s2_f16(a, 4096, 512, 32, a, 288, None, a, 1, 8, 8, 32, 96, 1, None) == -5  # flags
    assert L.x2v_vae_conv_s2_f16(a, 6144, 768, 48, a, 432, None, a, 1, 8, 8, 48, 96, 0, None) == -1  # Cin % 32
    assert b"Cin=48" in L.x2v_last_error()
    assert L.x2v_vae_conv_s2_f16(a, 4096, 512, 32, a, 288, None, a, 1, 8, 8, 32, 98, 0, None) == -1  # Cout % 4
    assert L.x2v_vae_conv_s2_f16(a, 4096, 512, 32, a, 288, None, a, 1, 1, 8, 32, 96, 0, None) == -1  # Hin < 2
    assert L.x2v_vae_conv_s2_f16(a, 4096, 256, 32, a, 288, None, a, 1, 8, 9, 32, 96, 0, None) == -2  # row stride below the extent
    assert L.x2v_vae_conv_s2_f16(a, 4096, 512, 32, a, 280, None, a, 1, 8, 8, 32, 96, 0, None) == -2  # weight row below 9 taps
    assert L.x2v_vae_conv_s2_f16(ctypes.c_void_p(4098), 4096, 512, 32, a, 288, None, a, 1, 8, 8, 32, 96, 0, None) == -2  # alignment
    # x2v_vae_video_prep(video, cs, ts, rs, T, H, W, y, yfs, yrs, yps, mode, stream)
    assert L.x2v_vae_video_prep(None, 64, 64, 8, 1, 8, 8, a, 4096, 512, 64, 2, None) == -5
    assert L.x2v_vae_video_prep(a, 64, 64, 8, 1, 8, 8, a, 4096, 512, 64, 3, None) == -5  # mode
    assert L.x2v_vae_video_prep(a, 64, 64, 8, 1, 8, 8, a, 4096, 512, 8, 2, None) == -1  # split needs 9 channels per pixel
    assert L.x2v_vae_video_prep(a, 64, 32, 8, 1, 8, 8, a, 4096, 512, 64, 2, None) == -1  # frame stride below H rows
    assert L.x2v_vae_video_prep(a, 64, 64, 8, 0, 8, 8, a, 4096, 512, 64, 2, None) == -1
