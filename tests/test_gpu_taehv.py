"""The tiny VAE (TAEHV) decoder on the HIP kernels (lightx2v_amd/vae_tiny.py, csrc/taehv.hip) against the fixture generated from the unmodified reference
(tests/golden/taehv_tiny.*.safetensors: bf16 on CPU, parallel=False) with the project's fp32 triangle, as in tests/test_gpu_t5.py: truth = the plain-PyTorch restatement
(tests/taehv_restatement.py, pinned to the fixture bit for bit by tests/test_taehv_host.py) in float64 on the bf16 weights, computed here on the CPU;
bar: relL2(HIP, truth) <= 1.5 x relL2(reference bf16, truth) — for the video of cases A-D and for the four stage outputs of case A, so that a failure names its
stage.  Where the fixture was generated the reference's own error was 5.7e-3 (A), 1.7e-3 (B), 3.6e-3 (C), 5.4e-3 (D); a decoder with a wrong past frame, swapped
TGrow frames or a trim from the wrong end is off by 0.33 .. 0.52 (tools/gen_golden_taehv.py asserts more than ten bars).  Chunked decodes must give the whole clip's
bits.  Measured numbers go to the parity summary (tests/util.py::record)."""
import pytest
import torch

from tests import taehv_restatement as R

pytestmark = pytest.mark.gpu
CASES = {"a": ("z_a", (True, True)), "b": ("z_b", (True, True)), "c": ("z_c", (True, True)), "d": ("z_a", (False, True))}


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


@pytest.fixture(scope="module")
def gold():
    from tests.util import load_golden

    return load_golden("taehv_tiny")


@pytest.fixture(scope="module")
def sd(gold):
    from lightx2v_amd import synth

    return synth.synth_taehv_weights(seed=int(gold["seed"][0]))


@pytest.fixture(scope="module")
def truth(gold, sd):
    """float64 restatement per case, made once: (video, stages)."""
    out = {}
    for case, (zkey, tu) in CASES.items():
        stages = {}
        out[case] = (R.wan_decode(sd, gold[zkey], dtype=torch.float64, time_upscale=tu, stages=stages), stages)
    return out


def _triangle(hip, ref16, tr, what):
    from tests.util import record

    e_hip, e_ref, e_pair = _rel(hip, tr), _rel(ref16, tr), _rel(hip, ref16)
    print(f"{what}: HIP vs truth {e_hip:.3e}; reference bf16 vs truth {e_ref:.3e}; HIP vs reference bf16 {e_pair:.3e}")
    record(what, hip_vs_truth=e_hip, ref_bf16_vs_truth=e_ref, hip_vs_ref_bf16=e_pair)
    assert torch.isfinite(hip.float()).all(), f"{what}: non-finite output"
    assert e_hip <= 1.5 * e_ref, f"{what}: err(HIP) {e_hip:.3e} > 1.5 x err(reference bf16) {e_ref:.3e}"


@pytest.mark.parametrize("case", sorted(CASES))
def test_decode_vs_reference_fixture(gold, sd, truth, case):
    from lightx2v_amd import vae_tiny

    zkey, tu = CASES[case]
    z = gold[zkey].cuda()
    if case == "d":
        dec = vae_tiny.TAEHV(sd, decoder_time_upscale=tu)
        assert dec.frames_to_trim == 1 and dec.w["decoder.13.conv"].shape[0] == 128
        got = dec._decode(z, head=True)
    else:
        got = vae_tiny.WanVAE_tiny(sd).decode(z)
    want = gold[f"video_{case}"]
    assert got.dtype == torch.bfloat16 and got.is_cuda and got.shape == want.shape
    _triangle(got, want, truth[case][0], f"taehv case {case} video {tuple(want.shape)}")


def test_stage_outputs_case_a(gold, sd, truth):
    from lightx2v_amd import vae_tiny

    dec = vae_tiny.TAEHV(sd)
    stages = {}
    video = dec.decode_video(gold["z_a"].cuda().unsqueeze(0).transpose(1, 2), stages=stages)
    assert tuple(video.shape) == (1, 9, 3, 40, 56) and video.dtype == torch.bfloat16
    for i in R.STAGE_ENDS:
        assert stages[i].shape == gold[f"stage{i}_a"].shape
        _triangle(stages[i], gold[f"stage{i}_a"], truth["a"][1][i], f"taehv case a stage ending at block {i}")
    # decode_video is the video before x 2 - 1: WanVAE_tiny.decode's result is one more rounding of it
    full = vae_tiny.WanVAE_tiny(sd).decode(gold["z_a"].cuda())
    assert torch.equal(video.transpose(1, 2).mul(2).sub(1), full)


@pytest.mark.parametrize("chunk", [1, 2])
def test_chunked_decode_is_bit_equal(gold, sd, chunk):
    from lightx2v_amd import vae_tiny

    z = gold["z_a"].cuda()
    whole = vae_tiny.WanVAE_tiny(sd).decode(z)
    assert torch.equal(vae_tiny.WanVAE_tiny(sd, chunk_frames=chunk).decode(z), whole)
    tu = (False, True)
    assert torch.equal(vae_tiny.TAEHV(sd, decoder_time_upscale=tu, chunk_frames=chunk)._decode(z, head=True), vae_tiny.TAEHV(sd, decoder_time_upscale=tu)._decode(z, head=True))


def test_decode_contract(gold, sd):
    """[16, T, h, w] in, [1, 3, 4 T - 3, 8 h, 8 w] bf16 out; the input is not modified; a second call gives the same bits, also behind a clip of another size and
    behind a chunked decoder's carried frames (no state leaks between clips); fp32 and bf16 latents of the same values agree."""
    from lightx2v_amd import vae_tiny

    vae = vae_tiny.WanVAE_tiny(sd, chunk_frames=2)
    z = gold["z_a"].cuda()
    before = z.clone()
    first = vae.decode(z)
    assert tuple(first.shape) == (1, 3, 9, 40, 56) and first.dtype == torch.bfloat16 and first.is_contiguous()
    assert torch.equal(z, before)
    other = vae.decode(gold["z_c"].cuda())
    assert tuple(other.shape) == (1, 3, 1, 24, 16)
    assert torch.equal(vae.decode(z), first)
    assert torch.equal(vae.decode(z.to(torch.bfloat16)), first)
    assert vae.temperal_downsample == [True, True, False] and vae.config.z_dim == 16


def test_wide_row_sampled_pixels(sd):
    """Latent (16, 2, 4, 160): a 1280-pixel output row with 32 rows, 80 pixel tiles across at the full-resolution stage.  Sampled pixels (row ends, both sides of
    tile seams, the interior) against the float64 restatement; bar: the triangle with the restatement's own bf16 run on the CPU (the reference's bits,
    tests/test_taehv_host.py) on the same samples."""
    from lightx2v_amd import vae_tiny

    z = torch.randn(16, 2, 4, 160, generator=torch.Generator().manual_seed(77)) * 2.5
    got = vae_tiny.WanVAE_tiny(sd).decode(z.cuda())
    assert tuple(got.shape) == (1, 3, 5, 32, 1280)
    tr = R.wan_decode(sd, z, dtype=torch.float64)
    ref16 = R.wan_decode(sd, z)
    cols = torch.tensor(sorted({0, 1, 15, 16, 17, 31, 32, 639, 640, 641, 1263, 1264, 1278, 1279} | set(range(5, 1280, 97))))
    rows = torch.tensor([0, 1, 15, 16, 17, 31])
    pick = lambda v: v.cpu()[..., rows[:, None], cols[None, :]]
    _triangle(pick(got), pick(ref16), pick(tr), f"taehv wide row 32 x 1280, {rows.numel() * cols.numel()} sampled pixels x 5 frames x 3 channels")
