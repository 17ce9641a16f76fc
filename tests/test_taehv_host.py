"""The tiny VAE (TAEHV) without a GPU: the plain-PyTorch restatement (tests/taehv_restatement.py) against the fixture generated from the unmodified reference
(tests/golden/taehv_tiny.*.safetensors, tools/gen_golden_taehv.py: bf16 on CPU, parallel=False) — BIT-EQUAL, cases A-D and the four stage outputs of A: PyTorch's
CPU bf16 convolution gave the same bits for the reference's frame-by-frame modules and for F.conv2d over all frames where the fixture was generated; chunked
restatement == whole clip; the frame and shape plan; the seeded weights' checksum; the argument checks of the new C entries; import and the loud failure without a GPU."""
import ctypes

import pytest
import torch

from tests import taehv_restatement as R

CASES = {"a": ("z_a", (True, True)), "b": ("z_b", (True, True)), "c": ("z_c", (True, True)), "d": ("z_a", (False, True))}


@pytest.fixture(scope="module")
def gold():
    from tests.util import load_golden

    return load_golden("taehv_tiny")


@pytest.fixture(scope="module")
def sd(gold):
    from lightx2v_amd import synth

    return synth.synth_taehv_weights(seed=int(gold["seed"][0]))


def test_weight_checksum(gold, sd):
    acc = torch.zeros((), dtype=torch.float64)
    for k in sorted(sd):
        assert sd[k].dtype == torch.bfloat16
        acc += sd[k].double().abs().sum()
    assert torch.equal(acc.reshape(1), gold["weights_checksum"]), "synth_taehv_weights drifted from the fixture's weights"
    assert sd["decoder.13.conv.weight"].shape[0] == 256 and sd["decoder.19.conv.weight"].shape[0] == 128 and sd["decoder.7.conv.weight"].shape[0] == 256
    assert "decoder.8.bias" not in sd and "decoder.22.bias" in sd
    assert sum(v.numel() for v in sd.values()) > 9_000_000


@pytest.mark.parametrize("case", sorted(CASES))
def test_restatement_equals_reference_fixture(gold, sd, case):
    zkey, tu = CASES[case]
    stages = {} if case == "a" else None
    got = R.wan_decode(sd, gold[zkey], time_upscale=tu, stages=stages)
    want = gold[f"video_{case}"]
    assert got.dtype == torch.bfloat16 and got.shape == want.shape
    assert torch.equal(got, want), f"case {case}: {(got != want).sum().item()} of {got.numel()} elements differ from the reference's bits"
    if stages is not None:
        for i in R.STAGE_ENDS:
            assert torch.equal(stages[i], gold[f"stage{i}_a"]), f"stage ending at block {i} differs from the reference's bits"


@pytest.mark.parametrize("chunk", [1, 2])
def test_restatement_chunked_equals_whole_clip(gold, sd, chunk):
    whole = R.wan_decode(sd, gold["z_a"])
    assert torch.equal(R.wan_decode(sd, gold["z_a"], chunk_frames=chunk), whole)
    assert torch.equal(R.wan_decode(sd, gold["z_a"], chunk_frames=chunk, time_upscale=(False, True)), gold["video_d"])


def test_restatement_wrong_decoders_differ(gold, sd):
    """The planted wrong decoders are other decoders in bf16 as well (the generator asserts the margin in float64)."""
    want = gold["video_a"]
    for mut in R.MUTATIONS:
        assert not torch.equal(R.wan_decode(sd, gold["z_a"], mutate=mut), want), mut


def test_frame_and_shape_plan(sd):
    from lightx2v_amd import vae_tiny

    for T in (1, 2, 5, 21):
        for tu, scale, trim in (((True, True), 4, 3), ((False, True), 2, 1), ((True, False), 2, 1), ((False, False), 1, 0)):
            plan = vae_tiny.frame_plan(T, (5, 7), tu)
            assert plan["trim"] == trim == R.frames_to_trim(tu)
            assert plan["out"] == (scale * T - trim, 40, 56) and plan["out"][0] == R.out_frames(T, tu)
            assert plan["stages"][0] == (T, 5, 7) and plan["stages"][3] == (scale * T, 40, 56)
    assert vae_tiny.frame_plan(21, (90, 160))["out"] == (81, 720, 1280)
    assert vae_tiny.frame_plan(3, (5, 7), decoder_space_upscale=(True, False, True))["out"] == (9, 20, 28)
    # patch_tgrow_layers: the LAST stride * C rows
    w = sd["decoder.13.conv.weight"]
    assert torch.equal(R.tgrow_rows(w, 128, 1), w[128:]) and torch.equal(R.tgrow_rows(w, 128, 2), w)


def test_argument_validation_needs_no_gpu():
    """Null operands, unsupported kernel sizes and misaligned strides are reported before any HIP call."""
    from lightx2v_amd import lib

    L = lib._lib
    a = ctypes.c_void_p(4096)

    def conv(x=a, mem=None, xs=(64 * 64, 8 * 64, 64), w=a, bias=None, resid=None, y=a, ys=(64 * 64, 8 * 64, 64, 1), T=1, H=8, W=8, Cin=64, Cout=64, k=3, flags=0, tsplit=1, trim=0):
        return L.x2v_conv2d_bf16(x, mem, *xs, w, bias, resid, y, *ys, T, H, W, Cin, Cout, k, flags, tsplit, trim, None)

    assert conv(x=None) == -5 and b"null operand" in L.x2v_last_error()
    assert conv(w=None) == -5 and conv(y=None) == -5
    assert conv(k=5) == -1 and b"kernel size 5" in L.x2v_last_error()
    assert conv(k=2) == -1
    assert conv(xs=(64 * 64, 8 * 64 + 4, 64)) == -2 and b"strides" in L.x2v_last_error()
    assert conv(xs=(64 * 64, 8 * 64, 32)) == -2  # pixel stride below Cin
    assert conv(x=ctypes.c_void_p(4104)) == -2
    assert conv(Cin=12) == -1
    assert conv(flags=lib.C2D_TWO_SOURCE, Cin=16, xs=(16 * 64, 8 * 16, 16)) == -1  # the two-source form steps in whole 32-channel chunks per source
    assert conv(mem=a) == -5  # mem without the two-source flag
    assert conv(flags=64) == -5
    assert conv(tsplit=3) == -1 and conv(tsplit=2, resid=a) == -5
    assert conv(trim=2) == -1
    assert conv(T=0) == 0  # no frames: nothing launched
    assert conv(T=3, trim=3) == 0
    assert L.x2v_taehv_clamp_bf16(None, 1, 64, 64, a, 1, 8, 8, 16, None) == -5
    assert L.x2v_taehv_clamp_bf16(a, 1, 64, 64, a, 1, 8, 8, 12, None) == -1 and b"C=12" in L.x2v_last_error()
    assert L.x2v_taehv_clamp_bf16(a, 2, 64, 64, a, 1, 8, 8, 16, None) == -5
    assert L.x2v_taehv_clamp_bf16(a, 1, 64, 64, ctypes.c_void_p(4100), 1, 8, 8, 16, None) == -2
    assert L.x2v_taehv_clamp_bf16(a, 1, 64, 64, a, 0, 8, 8, 16, None) == 0


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU failure mode")
def test_import_works_and_decode_fails_loudly_without_gpu(gold, sd):
    from lightx2v_amd import lib, vae_tiny

    vae = vae_tiny.WanVAE_tiny(sd, device="cpu")
    assert vae.temperal_downsample == [True, True, False] and vae.config.z_dim == 16 and vae.config.scaling_factor == 1.0
    assert vae.taehv.frames_to_trim == 3
    with pytest.raises(lib.X2VError):
        vae.decode(gold["z_b"])
    with pytest.raises(lib.X2VError):
        vae.taehv.decode_video(gold["z_b"].unsqueeze(0).transpose(1, 2))
    with pytest.raises(KeyError):
        vae_tiny.TAEHV({k: v for k, v in sd.items() if k != "decoder.8.weight"}, device="cpu")
