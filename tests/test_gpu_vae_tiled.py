"""Wan VAE use_tiling on the HIP path (lightx2v_amd/vae.py tile driver, x2v_vae_tile_compose_f32) against
  * the reference's sequential blend loops in torch fp32 on the CPU (tests/wan_vae_tiled_restatement.py) — bit for bit for the one-pass compose kernel,
  * the fixture generated from the unmodified reference's tiled_decode / tiled_encode (tests/golden/wan_vae_tiled_tiny.*.safetensors),
  * the CPU restatement (pinned to that fixture by tests/test_vae_tiled_host.py) at the released widths and at the default 256 / 192 px geometry.
Decode and encode bars are those of test_gpu_vae.py / test_gpu_vae_encode.py: |d| <= 2e-3 and relative L2 <= 1e-3 — blending is a convex combination of
tile values and does not widen them."""
import pytest
import torch

from tests import wan_vae_tiled_restatement as R
from tests.test_vae_tiled_host import GEOMETRIES, raw_tiles, tiny_sd

pytestmark = pytest.mark.gpu


def _check(got, ref, what, atol=2e-3, rel=1e-3):
    got, ref = got.float().cpu(), ref.float().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite values"
    d = (got - ref).abs().max().item()
    r = ((got - ref).norm() / ref.norm().clamp_min(1e-30)).item()
    print(f"{what}: max abs {d:.3e}, rel L2 {r:.3e}")
    assert d <= atol and r <= rel, f"{what}: max abs {d:.3e}, rel L2 {r:.3e}"


@pytest.fixture(scope="module")
def gold():
    from tests.util import load_golden

    return load_golden("wan_vae_tiled_tiny")


def _vae(sd, dim, tile=(64, 48), **kw):
    from lightx2v_amd import vae

    m = vae.WanVAE(sd, dim=dim, **kw)
    if tile is not None:
        m.model.tile_sample_min_height = m.model.tile_sample_min_width = tile[0]
        m.model.tile_sample_stride_height = m.model.tile_sample_stride_width = tile[1]
    return m


def _compose_on_gpu(raw, h, w, mn, st, clamp):
    """raw: rows of CPU tiles [C, T, th, tw] → the driver's composition on the GPU, [C, T, h, w] inside an oversized NaN-poisoned buffer whose tail must stay NaN."""
    from lightx2v_amd import vae

    plan = vae.tile_plan(h, w, mn, mn, st, st)
    flat = [t.permute(1, 2, 3, 0).contiguous().cuda() for r in raw for t in r]  # channels-last [T, th, tw, C]
    c, t = raw[0][0].shape[:2]
    n = c * t * h * w
    store = torch.full((n + 4096,), float("nan"), device="cuda")
    out = store[:n].view(c, t, h, w)
    vae.compose_tiles(plan, flat, out, clamp=clamp)
    torch.cuda.synchronize()
    assert torch.isnan(store[n:]).all(), "the compose kernel wrote past its output"
    assert not torch.isnan(out).any(), "the compose kernel left part of the image unwritten"
    return plan, out.cpu()


@pytest.mark.parametrize("geom", GEOMETRIES)
def test_compose_kernel_equals_the_reference_loops(geom):
    """x2v_vae_tile_compose_f32, one launch per output tile on raw tiles in [-2, 2], vs the reference's in-place row-major blend_v / blend_h + crop + cat on the
    CPU: torch.equal, for C = 3 and 16, T = 1 and 5, with and without the clamp (weights double-derived, products and sums rounded one by one)."""
    h, w, mn, st = geom
    b = mn - st
    for c in (3, 16):
        for t in (1, 5):
            raw = raw_tiles(h, w, mn, st, lead=(c, t), seed=c + t)
            ref = R.compose_sequential([[x.clone() for x in r] for r in raw], b, b, st, st, h, w)
            for clamp in (False, True):
                plan, out = _compose_on_gpu(raw, h, w, mn, st, clamp)
                assert plan["mode"] == "fused"
                want = ref.clamp(-1, 1) if clamp else ref
                assert torch.equal(out, want), f"{geom} C={c} T={t} clamp={clamp}: max |d| {(out - want).abs().max().item():.3e}"


def test_sequential_path_for_blend_beyond_stride():
    """(19, 13) at 8 / 3: blend 5 > stride 3 — the driver blends in place in tile order with x2v_blend_axis_f32 (fp32-derived weights, contracted sums) and
    stores through the compose kernel: the existing blend test's bar, atol 1e-6 / relative L2 1e-6."""
    h, w, mn, st = 19, 13, 8, 3
    for c, t in ((3, 2), (16, 1)):
        raw = raw_tiles(h, w, mn, st, lead=(c, t), seed=7)
        ref = R.compose_sequential([[x.clone() for x in r] for r in raw], 5, 5, st, st, h, w)
        for clamp in (False, True):
            plan, out = _compose_on_gpu(raw, h, w, mn, st, clamp)
            assert plan["mode"] == "sequential"
            _check(out, ref.clamp(-1, 1) if clamp else ref, f"sequential compose C={c} clamp={clamp}", atol=1e-6, rel=1e-6)


@pytest.mark.parametrize("conv16", [False, "split"])
def test_tiled_decode_matches_reference_fixture(gold, conv16):
    """WanVAE(use_tiling=True).decode at 64 / 48 px tiles vs the reference's tiled_decode (+ WanVAE.decode's clamp) on both fixture latents — 3 x 2 tiles with
    2-row / 5-column edge tiles, and a one-latent-row sliver shorter than the blend.  The fixture's seams hold values beyond [-1, 1]: a head that clamped
    before the blend misses by 0.085 / 0.025.  A second call and every tile_chunk_frames give the same bits."""
    sd, dim = tiny_sd(gold)
    m = _vae(sd, dim, conv16=conv16, use_tiling=True)
    for name in ("a", "b"):
        z = gold[f"z_{name}"].cuda()
        out = m.decode(z)
        assert out.shape == (1, *gold[f"dec_{name}"].shape) and out.dtype == torch.float32
        _check(out[0], gold[f"dec_{name}"].clamp(-1, 1), f"tiled decode {name} (conv16={conv16})")
        assert out.abs().max().item() <= 1.0
        assert torch.equal(m.decode(z), out)
        for k in (1, 2):
            m.tile_chunk_frames = k
            assert torch.equal(m.decode(z), out), f"tile_chunk_frames={k}"
        m.tile_chunk_frames = None


def test_tiled_decode_frame_chunking_is_bit_identical(gold):
    """Four latent frames, where tile_chunk_frames = 1, 2 and None really are different passes (1+1+1+1, 1+2+1, 1+3), 2 x 2 tiles."""
    sd, dim = tiny_sd(gold)
    z = torch.randn(16, 4, 8, 11, generator=torch.Generator().manual_seed(41)).cuda()
    outs = []
    for k in (None, 1, 2):
        outs.append(_vae(sd, dim, use_tiling=True, tile_chunk_frames=k).decode(z))
    assert outs[0].shape == (1, 3, 13, 64, 88)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


@pytest.mark.parametrize("conv16", [False, "split"])
def test_tiled_encode_matches_reference_fixture(gold, conv16):
    sd, dim = tiny_sd(gold)
    m = _vae(sd, dim, conv16=conv16, use_tiling=True)
    z = m.encode([gold["video"].cuda()])
    assert isinstance(z, list) and len(z) == 1 and z[0].dtype == torch.float32
    _check(z[0], gold["mu_video"], f"tiled encode (conv16={conv16})")
    assert torch.equal(m.encode([gold["video"].cuda()])[0], z[0])


def test_single_tile_equals_the_plain_paths(gold):
    """h, w <= stride: one tile, no seam — the unclamped head + the compose kernel's clamp must give the plain decode's fused clamp bit for bit, and the tiled
    encode the plain encode."""
    sd, dim = tiny_sd(gold)
    g = torch.Generator().manual_seed(42)
    z = (torch.randn(16, 2, 6, 5, generator=g) * 1.5).cuda()
    video = (torch.rand(3, 5, 48, 40, generator=g) * 2 - 1).cuda()
    tiled, plain = _vae(sd, dim, use_tiling=True), _vae(sd, dim)
    out = plain.decode(z)
    assert out.abs().max().item() == 1.0, "the clamp must bite for this check to mean something"
    assert torch.equal(tiled.decode(z), out)
    assert torch.equal(tiled.encode([video])[0], plain.encode([video])[0])


def test_tiled_real_widths_vs_restatement():
    """dim 96 (the released channel plan) with 32 / 24 px tiles: latent (16, 2, 5, 7) = 2 x 3 tiles with a 1-column sliver; video (3, 5, 40, 56)."""
    from lightx2v_amd import synth

    sd = dict(synth.synth_wan_vae_weights(dim=96, seed=3))
    sd.update(synth.synth_wan_vae_encoder_weights(dim=96, seed=2))
    g = torch.Generator().manual_seed(43)
    z = torch.randn(16, 2, 5, 7, generator=g)
    video = torch.rand(3, 5, 40, 56, generator=g) * 2 - 1
    m = _vae(sd, 96, tile=(32, 24), use_tiling=True)
    mean, inv_std = m.mean.cpu(), m.inv_std.cpu()
    _check(m.decode(z.cuda())[0], R.tiled_decode(sd, z, mean, inv_std, dim=96, tile_min=32, tile_stride=24), "tiled decode dim 96")
    _check(m.encode([video.cuda()])[0], R.tiled_encode(sd, video, mean, inv_std, dim=96, tile_min=32, tile_stride=24), "tiled encode dim 96")


def test_tiled_default_geometry_vs_restatement(gold):
    """The attributes left at 256 / 192 px: latent (16, 2, 34, 26) = tiles of 32 x 26 latents with edge tiles of 10 rows and 2 columns, a 64-px blend."""
    sd, dim = tiny_sd(gold)
    z = torch.randn(16, 2, 34, 26, generator=torch.Generator().manual_seed(44))
    m = _vae(sd, dim, tile=None, use_tiling=True)
    assert m.model.tile_geometry() == (32, 32, 24, 24)
    _check(m.decode(z.cuda())[0], R.tiled_decode(sd, z, m.mean.cpu(), m.inv_std.cpu(), dim=dim), "tiled decode, default geometry")


def test_parallel_keeps_precedence_and_refusals_stay(gold, monkeypatch):
    """parallel=True on a one-rank group ignores use_tiling, as the reference's decode does (vae.py:935-949): the result is the plain decode's, not the tiled
    one's.  A decode-only state dict still refuses to encode, tiled or not."""
    import torch.distributed as dist

    from lightx2v_amd import lib, synth

    sd, dim = tiny_sd(gold)
    z = gold["z_a"].cuda()
    plain, tiled = _vae(sd, dim).decode(z), _vae(sd, dim, use_tiling=True).decode(z)
    assert not torch.equal(plain, tiled)
    own_group = not dist.is_initialized()
    if own_group:
        dist.init_process_group("gloo", store=dist.HashStore(), rank=0, world_size=1)
    try:
        gather = dist.all_gather_into_tensor
        monkeypatch.setattr(dist, "all_gather_into_tensor", lambda out, inp, *a, **kw: out.copy_(_host(gather, out, inp, *a, **kw)))
        assert torch.equal(_vae(sd, dim, use_tiling=True, parallel=True).decode(z), plain)
    finally:
        if own_group:
            dist.destroy_process_group()
    with pytest.raises(lib.X2VError, match="no encoder"):
        _vae(synth.synth_wan_vae_weights(dim=dim, seed=3), dim, use_tiling=True).encode([gold["video"].cuda()])


def _host(gather, out, inp, *a, **kw):
    """The gloo group gathers host tensors: stage through the CPU (one rank: a copy)."""
    o = torch.empty(out.shape, dtype=out.dtype)
    gather(o, inp.cpu(), *a, **kw)
    return o
