"""TEST INFRASTRUCTURE ONLY — CPU fp32 restatement of the reference's tiled Wan VAE paths, the checker of lightx2v_amd/vae.py's tile driver.

reference: lightx2v/models/video_encoders/hf/wan/vae.py — blend_v / blend_h :556-566 · tiled_encode :568-629 · tiled_decode :631-682 · the clamp behind
tiled_decode, WanVAE.decode :949.  The tile loops are the reference's, run around the decode restatement without its clamp
(oracle/wan_vae_oracle.py::wan_vae_decode(clamp=False)) and the encode restatement (tests/wan_vae_encode_restatement.py).  Pinned to
tests/golden/wan_vae_tiled_tiny.*.safetensors (tools/gen_golden_vae_tiled.py, generated from the unmodified reference) by tests/test_vae_tiled_host.py.

Two forms of the blending stand side by side:
  * `compose_sequential`: the reference's loops — in place, row-major, blend_v then blend_h, crop to the stride, cat, crop to the image;
  * `compose_fused`: the four-raw-tile expression of x2v_vae_tile_compose_f32 (include/x2v.h) in torch fp32, which equals the loops bit for bit whenever
    blend <= stride on both axes.
Tiles are [C, T, h, w] (batch 1 dropped); the blended axes are the last two.  Not for shapes with a 1 x 1-latent tile: the CPU convolution library takes
another path there and the per-tile decode differs from the reference's by 2.4e-7.
"""
import torch

from oracle.wan_vae_oracle import wan_vae_decode
from tests import wan_vae_encode_restatement as E


def blend(a, b, extent, dim):
    """blend_v (dim = -2) / blend_h (dim = -1), vae.py:556-566: in place on b."""
    extent = min(a.shape[dim], b.shape[dim], extent)
    for y in range(extent):
        ia, ib = [slice(None)] * a.dim(), [slice(None)] * b.dim()
        ia[dim], ib[dim] = -extent + y, y
        b[tuple(ib)] = a[tuple(ia)] * (1 - y / extent) + b[tuple(ib)] * (y / extent)
    return b


def compose_sequential(rows, blend_h, blend_w, stride_h, stride_w, height, width):
    """vae.py:615-629 / 667-680 on `rows` (list of rows of tiles).  The tiles are blended IN PLACE, as in the reference: pass clones to keep them."""
    result_rows = []
    for i, row in enumerate(rows):
        result_row = []
        for j, tile in enumerate(row):
            if i > 0:
                tile = blend(rows[i - 1][j], tile, blend_h, -2)
            if j > 0:
                tile = blend(row[j - 1], tile, blend_w, -1)
            result_row.append(tile[..., :stride_h, :stride_w])
        result_rows.append(torch.cat(result_row, dim=-1))
    return torch.cat(result_rows, dim=-2)[..., :height, :width]


def _w(k, n):
    """The two weights of index k of an extent n as torch applies its Python-float scalars to an fp32 tensor: formed in double, rounded once."""
    return torch.tensor(1 - k / n, dtype=torch.float64).float(), torch.tensor(k / n, dtype=torch.float64).float()


def compose_fused(rows, blend_h, blend_w, stride_h, stride_w, height, width):
    """The expression of x2v_vae_tile_compose_f32 on the RAW tiles (nothing is modified): per output tile, centre / up / left / up-left."""
    lead = rows[0][0].shape[:-2]
    out = torch.zeros((*lead, height, width), dtype=torch.float32)
    for i, row in enumerate(rows):
        for j, c in enumerate(row):
            th, tw = c.shape[-2:]
            up, left = (rows[i - 1][j] if i else None), (row[j - 1] if j else None)
            ul = rows[i - 1][j - 1] if i and j else None
            ev = min(up.shape[-2], th, blend_h) if i else 0
            eh = min(left.shape[-1], tw, blend_w) if j else 0
            rh, rw = min(th, stride_h, height - i * stride_h), min(tw, stride_w, width - j * stride_w)
            v = c[..., :rh, :rw].clone()
            for y in range(min(ev, rh)):
                wy1, wy = _w(y, ev)
                u = up[..., up.shape[-2] - ev + y, :rw].clone()
                for x in range(min(eh, rw)):
                    wx1, wx = _w(x, eh)
                    u[..., x] = ul[..., ul.shape[-2] - ev + y, ul.shape[-1] - eh + x] * wx1 + u[..., x] * wx
                v[..., y, :] = u * wy1 + v[..., y, :] * wy
            for x in range(min(eh, rw)):
                wx1, wx = _w(x, eh)
                col = left[..., :rh, left.shape[-1] - eh + x].clone()
                for y in range(min(ev, rh)):
                    wy1, wy = _w(y, ev)
                    col[..., y] = ul[..., ul.shape[-2] - ev + y, ul.shape[-1] - eh + x] * wy1 + col[..., y] * wy
                v[..., :, x] = col * wx1 + v[..., :, x] * wx
            out[..., i * stride_h : i * stride_h + rh, j * stride_w : j * stride_w + rw] = v
    return out


def decode_tiles(sd, z, mean, inv_std, dim, tile_min, tile_stride):
    """The decoding half of tiled_decode (vae.py:649-665): z [16, T, h, w]; tile_min / tile_stride in PIXELS → rows of raw (unclamped) tiles [3, T', 8th, 8tw]."""
    lm, ls = tile_min // 8, tile_stride // 8
    with torch.no_grad():
        return [[wan_vae_decode(sd, z[:, :, i : i + lm, j : j + lm].contiguous(), mean, inv_std, dim=dim, clamp=False) for j in range(0, z.shape[3], ls)]
                for i in range(0, z.shape[2], ls)]


def tiled_decode(sd, z, mean, inv_std, dim=96, tile_min=256, tile_stride=192, clamp=True, fused=False):
    """WanVAE_.tiled_decode (vae.py:631-682) + the clamp of WanVAE.decode (vae.py:949): z [16, T, h, w] → [3, 1 + 4 (T - 1), 8h, 8w]."""
    rows = decode_tiles(sd, z, mean, inv_std, dim, tile_min, tile_stride)
    b = tile_min - tile_stride
    out = (compose_fused if fused else compose_sequential)(rows, b, b, tile_stride, tile_stride, 8 * z.shape[2], 8 * z.shape[3])
    return out.float().clamp_(-1, 1) if clamp else out


def tiled_encode(sd, video, mean, inv_std, dim=96, tile_min=256, tile_stride=192, fused=False):
    """WanVAE_.tiled_encode (vae.py:568-629): video [3, T, H, W] → normalised mu [16, 1 + (T - 1) // 4, H // 8, W // 8]; tiles in pixels, blending in latents."""
    with torch.no_grad():
        rows = [[E.encode(sd, video[:, :, i : i + tile_min, j : j + tile_min].contiguous(), mean, inv_std, dim=dim) for j in range(0, video.shape[3], tile_stride)]
                for i in range(0, video.shape[2], tile_stride)]
    b, s = tile_min // 8 - tile_stride // 8, tile_stride // 8
    return (compose_fused if fused else compose_sequential)(rows, b, b, s, s, video.shape[2] // 8, video.shape[3] // 8)
