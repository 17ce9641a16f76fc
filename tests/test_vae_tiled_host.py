"""Wan VAE tiling, host side (no GPU): the CPU restatement of tiled_decode / tiled_encode against the reference fixture (and live against the reference where
it is present), the tile plan against hand-written expectations, the fused four-tile expression against the reference's sequential loops, and the
argument checks of x2v_vae_tile_compose_f32."""
import ctypes

import pytest
import torch

from lightx2v_amd import lib, synth, vae
from tests import wan_vae_tiled_restatement as R
from tests.util import load_golden

# (H, W, min, stride) on which the fused expression was derived: non-power-of-two extents, blend = stride, one-pixel slivers, truncated neighbours
GEOMETRIES = [(20, 14, 8, 6), (19, 13, 8, 6), (25, 7, 8, 6), (30, 40, 8, 6), (17, 22, 8, 4), (13, 19, 12, 9), (21, 21, 16, 10)]


@pytest.fixture(scope="module")
def gold():
    return load_golden("wan_vae_tiled_tiny")


def tiny_sd(gold):
    dim, seed = int(gold["dim"][0]), int(gold["seed"][0])
    sd = dict(synth.synth_wan_vae_weights(dim=dim, seed=seed))
    sd.update(synth.synth_wan_vae_encoder_weights(dim=dim))
    checksum = sum((sd[k].double().abs().sum() for k in sorted(sd)), torch.zeros((), dtype=torch.float64)).reshape(1)  # oracle/gen_golden.py::weights_checksum
    assert torch.equal(checksum, gold["weights_checksum"]), "the synthetic Wan VAE weights drifted from the fixture"
    return sd, dim


def raw_tiles(h, w, mn, st, lead=(2, 3), seed=0):
    """Seeded raw tiles in about [-2, 2] for an h x w image cut into mn-sized tiles at stride st: rows of [*lead, th, tw]."""
    g = torch.Generator().manual_seed(seed + 1000 * h + w)
    return [[torch.randn(*lead, min(mn, h - i), min(mn, w - j), generator=g).clamp_(-2, 2) for j in range(0, w, st)] for i in range(0, h, st)]


@pytest.mark.parametrize("name", ["a", "b"])
def test_decode_restatement_equals_reference_fixture(gold, name):
    """Both forms of the restatement, bit for bit, on the fixture's latents: (16, 2, 14, 11) = 3 x 2 tiles with a 2-row and a 5-column edge tile, and
    (16, 2, 13, 8) with a one-latent-row sliver tile shorter than the blend.  The fixture holds tiled_decode's own, unclamped, return value."""
    sd, dim = tiny_sd(gold)
    mn, st = (int(v) for v in gold["tile"])
    for fused in (False, True):
        out = R.tiled_decode(sd, gold[f"z_{name}"], gold["mean"], gold["inv_std"], dim=dim, tile_min=mn, tile_stride=st, clamp=False, fused=fused)
        assert torch.equal(out, gold[f"dec_{name}"]), f"fused={fused}: max |d| {(out - gold[f'dec_{name}']).abs().max().item():.3e}"
    assert gold[f"dec_{name}"].abs().max().item() > 1.0  # the clamp behind the blend has something to do


def test_encode_restatement_equals_reference_fixture(gold):
    sd, dim = tiny_sd(gold)
    mn, st = (int(v) for v in gold["tile"])
    for fused in (False, True):
        mu = R.tiled_encode(sd, gold["video"], gold["mean"], gold["inv_std"], dim=dim, tile_min=mn, tile_stride=st, fused=fused)
        assert torch.equal(mu, gold["mu_video"]), f"fused={fused}"


def test_restatement_equals_the_reference_live(gold):
    """One more shape per direction against the unmodified reference itself, where it is present: latent (16, 2, 12, 7) (a 1-column sliver beside full rows)
    and video (3, 5, 104, 56)."""
    from oracle import ref_import

    if not ref_import.reference_available():
        pytest.skip("reference checkout not present (authoring container only)")
    ref_import.patch_and_import()
    from lightx2v.models.video_encoders.hf.wan.vae import WanVAE_

    sd, dim = tiny_sd(gold)
    m = WanVAE_(dim=dim, z_dim=16, dim_mult=[1, 2, 4, 4], num_res_blocks=2, attn_scales=[], temperal_downsample=[False, True, True], dropout=0.0).eval()
    m.load_state_dict(sd, strict=False)
    m.tile_sample_min_height = m.tile_sample_min_width = 64
    m.tile_sample_stride_height = m.tile_sample_stride_width = 48
    scale = [gold["mean"], gold["inv_std"]]
    g = torch.Generator().manual_seed(31)
    z = torch.randn(16, 2, 12, 7, generator=g)
    video = torch.rand(3, 5, 104, 56, generator=g) * 2 - 1
    with torch.no_grad():
        ref_dec = m.tiled_decode(z.unsqueeze(0), scale)[0]
        ref_enc = m.tiled_encode(video.unsqueeze(0), scale)[0]
    assert torch.equal(R.tiled_decode(sd, z, *scale, dim=dim, tile_min=64, tile_stride=48, clamp=False), ref_dec)
    assert torch.equal(R.tiled_encode(sd, video, *scale, dim=dim, tile_min=64, tile_stride=48), ref_enc)


def _sizes(plan, key, axis):
    return [p[key] for p in plan["tiles"] if p["j" if axis == "i" else "i"] == 0]


def test_tile_plan_default_geometry():
    """720p and 480p latents at the reference's 256 / 192 px (32 / 24 latents, blend 8): 4 x 7 tiles with 18-row / 16-column edge tiles, 3 x 5 with 12 / 8."""
    for (h, w), (rows, cols), (eh_, ew_) in [((90, 160), (4, 7), (18, 16)), ((60, 104), (3, 5), (12, 8))]:
        plan = vae.tile_plan(h, w, 32, 32, 24, 24)
        assert (plan["mode"], plan["rows"], plan["cols"], plan["blend"]) == ("fused", rows, cols, (8, 8))
        assert len(plan["tiles"]) == rows * cols and [(p["i"], p["j"]) for p in plan["tiles"]] == [(i, j) for i in range(rows) for j in range(cols)]
        assert _sizes(plan, "y0", "i") == [24 * i for i in range(rows)] and _sizes(plan, "x0", "j") == [24 * j for j in range(cols)]
        assert _sizes(plan, "th", "i") == [32] * (rows - 1) + [eh_] and _sizes(plan, "tw", "j") == [32] * (cols - 1) + [ew_]
        assert _sizes(plan, "ev", "i") == [0] + [8] * (rows - 1) and _sizes(plan, "eh", "j") == [0] + [8] * (cols - 1)
        assert _sizes(plan, "rh", "i") == [24] * (rows - 1) + [eh_] and _sizes(plan, "rw", "j") == [24] * (cols - 1) + [ew_]
        assert sum(_sizes(plan, "rh", "i")) == h and sum(_sizes(plan, "rw", "j")) == w  # the regions tile the image
    last = vae.tile_plan(90, 160, 32, 32, 24, 24)["tiles"][-1]
    assert last == dict(i=3, j=6, y0=72, x0=144, th=18, tw=16, ev=8, eh=8, rh=18, rw=16)


def test_tile_plan_slivers_and_modes():
    """13 x 8 at 8 / 6: rows start at 0, 6, 12 — the last tile is ONE row, shorter than the blend of 2: its extent is min(8, 1, 2) = 1; columns 0, 6 with a
    2-column edge tile.  A single tile when the image fits one stride.  min > 2 stride: sequential."""
    plan = vae.tile_plan(13, 8, 8, 8, 6, 6)
    assert (plan["rows"], plan["cols"], plan["mode"]) == (3, 2, "fused")
    assert _sizes(plan, "th", "i") == [8, 7, 1] and _sizes(plan, "ev", "i") == [0, 2, 1] and _sizes(plan, "rh", "i") == [6, 6, 1]
    assert _sizes(plan, "tw", "j") == [8, 2] and _sizes(plan, "eh", "j") == [0, 2] and _sizes(plan, "rw", "j") == [6, 2]
    one = vae.tile_plan(6, 5, 8, 8, 6, 6)
    assert one["tiles"] == [dict(i=0, j=0, y0=0, x0=0, th=6, tw=5, ev=0, eh=0, rh=6, rw=5)]
    assert vae.tile_plan(19, 13, 8, 8, 3, 3)["mode"] == "sequential"  # blend 5 > stride 3
    assert vae.tile_plan(19, 13, 8, 8, 4, 3)["mode"] == "sequential" and vae.tile_plan(19, 13, 8, 8, 4, 4)["mode"] == "fused"  # blend = stride is still fused
    assert vae.tile_plan(9, 9, 6, 6, 6, 6)["blend"] == (0, 0)  # min = stride: no blending, the reference's range(0) loops
    for bad in ((0, 4, 8, 8, 6, 6), (4, 4, 8, 8, 0, 6), (4, 4, 4, 8, 6, 6)):
        with pytest.raises(lib.X2VError):
            vae.tile_plan(*bad)


def test_tile_attributes_are_the_references():
    m = vae.WanVAE_({}, dim=16, device="cpu")
    assert (m.tile_sample_min_height, m.tile_sample_min_width, m.tile_sample_stride_height, m.tile_sample_stride_width) == (256, 256, 192, 192)
    assert m.tile_geometry() == (32, 32, 24, 24)
    m.tile_sample_min_height = m.tile_sample_min_width = 64
    m.tile_sample_stride_height = m.tile_sample_stride_width = 48
    assert m.tile_geometry() == (8, 8, 6, 6)
    m.tile_sample_stride_width = 44
    with pytest.raises(lib.X2VError, match="multiples of 8"):
        m.tile_geometry()


@pytest.mark.parametrize("geom", GEOMETRIES)
def test_fused_expression_equals_the_sequential_loops(geom):
    """compose_fused (what the HIP kernel computes, per output tile from at most four raw tiles) vs the reference's in-place loops: bit-equal on the seven
    geometries with blend <= stride, and the plan of each says "fused"."""
    h, w, mn, st = geom
    raw = raw_tiles(h, w, mn, st)
    b = mn - st
    seq = R.compose_sequential([[t.clone() for t in r] for r in raw], b, b, st, st, h, w)
    assert torch.equal(R.compose_fused(raw, b, b, st, st, h, w), seq)
    plan = vae.tile_plan(h, w, mn, mn, st, st)
    assert plan["mode"] == "fused" and (plan["rows"], plan["cols"]) == (len(raw), len(raw[0]))
    for p, t in zip(plan["tiles"], [t for r in raw for t in r]):
        assert (p["th"], p["tw"]) == tuple(t.shape[-2:])


def test_fused_expression_is_not_for_blend_beyond_stride():
    """(19, 13, 8, 3): blend 5 > stride 3 — a tile reads rows of its neighbour that the neighbour's own blend already changed, the four-raw-tile
    expression is another function; the plan routes it to the sequential path."""
    raw = raw_tiles(19, 13, 8, 3)
    seq = R.compose_sequential([[t.clone() for t in r] for r in raw], 5, 5, 3, 3, 19, 13)
    assert not torch.equal(R.compose_fused(raw, 5, 5, 3, 3, 19, 13), seq)
    assert vae.tile_plan(19, 13, 8, 8, 3, 3)["mode"] == "sequential"


def test_tiled_entry_points_refuse_a_cpu_device_first():
    """The product has no CPU path: with use_tiling both entry points say so before they look at the state dict (an empty one here)."""
    m = vae.WanVAE({}, dim=16, device="cpu", use_tiling=True)
    with pytest.raises(lib.X2VError, match="not built for device"):
        m.decode(torch.zeros(16, 1, 2, 2))
    with pytest.raises(lib.X2VError, match="not built for device"):
        m.encode([torch.zeros(3, 1, 16, 16)])


def test_tile_compose_abi_argument_validation_needs_no_gpu():
    L = lib._lib
    a = ctypes.c_void_p(4096)
    # x2v_vae_tile_compose_f32(center, up, left, up_left, T, C, ch, cw, uh, lw, ev, eh, rh, rw, out, out_c_stride, out_t_stride, out_row_stride, clamp, stream)
    ok = (a, a, a, a, 2, 3, 8, 8, 8, 8, 2, 2, 6, 6, a, 4096, 256, 16, 1, None)

    def call(**kw):
        names = ["center", "up", "left", "up_left", "T", "C", "ch", "cw", "uh", "lw", "ev", "eh", "rh", "rw", "out", "ocs", "ots", "ors", "clamp", "stream"]
        args = dict(zip(names, ok))
        args.update(kw)
        return L.x2v_vae_tile_compose_f32(*[args[n] for n in names])

    assert call(center=None) == -5  # null centre tile
    assert b"vae_tile_compose" in L.x2v_last_error()
    assert call(out=None) == -5
    assert call(clamp=2) == -5
    assert call(up_left=None) == -5  # both extents set, no corner tile
    for bad in (dict(T=0), dict(C=0), dict(ch=0), dict(cw=-1), dict(rh=0), dict(rw=-3)):  # zero or negative sizes
        assert call(**bad) == -1, bad
    assert call(rh=9) == -1 and call(rw=9) == -1  # region beyond the centre tile
    assert call(ev=9) == -1 and call(eh=9) == -1  # extent larger than the centre tile
    assert call(uh=1) == -1 and call(lw=1) == -1  # ... than the neighbour
    assert call(ev=-1) == -1
    assert call(up=None) == -1 and call(left=None) == -1  # an extent without its neighbour
    assert call(ors=5) == -1  # output rows shorter than the region
    assert call(center=ctypes.c_void_p(4098)) == -2 and call(out=ctypes.c_void_p(4097)) == -2  # misalignment
    # a first-row, first-column tile needs no neighbour at all — and these all return before any HIP call
    assert call(up=None, left=None, up_left=None, ev=0, eh=0, uh=0, lw=0, T=0) == -1
