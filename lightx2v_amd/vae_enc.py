"""Wan VAE encode on the HIP kernels — host-side mirror of the reference's encode path (the i2v conditioning latents).

reference: lightx2v/models/video_encoders/hf/wan/vae.py — WanVAE.encode :867-881 → WanVAE_.encode :684-711 → Encoder3d.forward :322-374 →
ResidualBlock :185-223 / AttentionBlock :226-262 / Resample downsample2d, downsample3d :96-100,141-158 / CausalConv3d :19-44;
runners/wan/wan_runner.py:204-248 (run_vae_encoder: latent size, bicubic resize, zero frames, first-frame mask).

The encoder is the decoder's machinery run the other way: it subclasses `vae.Decoder3d` for the cache-carrying convolution buffers (`_ConvInput`,
shared frame pools), the RMS_norm + SiLU producers, the residual block and the attention block, and adds the parts only an encoder has:
  * conv1 reads the caller's [3, T, H, W] fp32 video in place (x2v_vae_video_prep writes the zero-bordered channels-last operand buffer, 9 split
    channels in a 64-channel pixel whose last 32 the 128-pixel kernel skips); the video is resident, so the 2-frame cache is the usual buffer head;
  * Resample downsample2d / 3d: nn.ZeroPad2d((0, 1, 0, 1)) + 3x3 stride-2 Conv2d on x2v_vae_conv_s2_f16 (the pad is the kernel's bounded read), then
    for 3d the (3,1,1) stride-2 time convolution as one x2v_vae_conv_f16 launch (kt = 3, kh = kw = 1, T = 1) per output frame over the buffer
    [last frame of the previous chunk | this chunk's frames] — on the first chunk the reference skips it and only caches (vae.py:144-158);
  * the head's 32 channels, then conv1 (1x1, 32 → 32) of which only mu is computed, with the (mu - mean) * inv_std normalisation folded into its
    weights (vae.py:706-710).
Like the decoder's, every kernel reduces each output value in an order that does not depend on the launch's frame count, so any `chunk_frames`
(1 frame, then k frames per pass, k a multiple of 4) gives bit-identical latents; the reference's is 4 (vae.py:687-705).
"""
import torch

from . import lib, synth
from .vae import Decoder3d, _split16


class Encoder3d(Decoder3d):
    """reference: vae.py:265-374."""

    def __init__(self, sd, dim, image_hw, device, conv16="split", share=None):
        self._setup(sd, "encoder.", image_hw, device, conv16, share)  # conv16 as in Decoder3d; _rep here: downsample3d's "first chunk has passed" (vae.py:146-149)
        self.dims, self.plan = synth.wan_vae_encoder_plan(dim)
        if share is not None:  # another tile geometry of the same encoder (tiled_encode): the converted weights, the stride-2 and conv1 forms included
            self.w_s2 = share.w_s2
            return
        # the stride-2 kernel's weights: fp16 / split operands in 32-channel slabs, [Cout, 3, 3, Cs] (fp32 mode: the polyphase convolutions of _down2d)
        self.w_s2 = {}
        if conv16:
            for k, v in self.w.items():
                if k.endswith("resample.1.weight"):
                    self.w16.pop(k, None)
                    cin = v.shape[4]
                    self.w_s2[k] = _split16(v[:, 0], ((3 * cin if self.split else cin) + 31) // 32 * 32, self.split)
        # conv1 (Cin = 3): fp16 / split operands in a 64-channel pixel (9 split channels, the last 32 skipped by the 128-pixel kernel); fp32: 16 channels
        w1 = self.w["encoder.conv1.weight"]
        if conv16:
            self.w16["encoder.conv1.weight"] = _split16(w1, 64, self.split)
            self.w16_tail["encoder.conv1.weight"] = 64 - (9 if self.split else 3)
        else:
            self.w["encoder.conv1.weight"] = torch.nn.functional.pad(w1, (0, 13)).contiguous()

    # ---- layers -------------------------------------------------------------------------------------------------------
    def conv1(self, video):
        """Encoder3d.conv1 (vae.py:286,323-336) on video [3, T, H, W] fp32 (a device view, read in place) → [T, H, W, dims[0]]."""
        _, t, h, w = video.shape
        name = "encoder.conv1"
        w16 = self.w16.get(name + ".weight")
        wt = self.w[name + ".weight"]
        cout = wt.shape[0]
        flags = lib.VCONV_ZERO_TAIL32 if w16 is not None and self.w16_tail[name + ".weight"] >= 32 else 0
        sep = w16 is not None and lib.vae_conv16_cached_ok(w, w16, flags)
        if w16 is not None:
            b = self._input("conv1", t, h, w, 3, 3, 1, torch.float16, copy_cache=not sep)
        else:
            b = self._input("conv1", t, h, w, 16, 3, 1, torch.float32)
        lib.vae_video_prep(video, b.interior()[:t, :h, :w], split=self.split)
        out = torch.empty((t, h, w, cout), dtype=torch.float32, device=video.device)
        if w16 is not None:
            lib.vae_conv16(b.buf, b.strides, w16, out, t, h, w, bias=self.w[name + ".bias"], flags=flags, cache=b.cache if sep else None)
        else:
            lib.vae_conv(b.buf, b.strides, wt, out, t, h, w, bias=self.w[name + ".bias"])
        b.roll(t, head_valid=not sep)
        return out

    def _down2d(self, name, x):
        """nn.ZeroPad2d((0, 1, 0, 1)) + nn.Conv2d(C, C, 3, stride=2) per frame (vae.py:96-100) on x [T, H, W, C] → [T, H // 2, W // 2, C]."""
        t, h, w, c = x.shape
        wt = self.w[name + ".weight"]  # [C, 1, 3, 3, C]
        cout = wt.shape[0]
        out = torch.empty((t, h // 2, w // 2, cout), dtype=torch.float32, device=x.device)
        bias = self.w[name + ".bias"]
        w_s2 = self.w_s2.get(name + ".weight")
        if w_s2 is not None:
            cs = w_s2.shape[-1]
            key = ("s2", t, h, w, cs, c)
            buf = self._pool.get(key)
            if buf is None:  # pad channels (none at the Wan widths) are never written and stay zero
                buf = self._pool[key] = torch.zeros((t, h, w, cs), dtype=torch.float16, device=x.device)
            lib.vae_prep(x, buf, (h * w * cs, w * cs), split=self.split)
            return lib.vae_conv_s2(buf, w_s2, out, bias=bias)
        # fp32 mode: four polyphase convolutions on the fp32 matrix instruction — input phase (a, b) = rows a::2, columns b::2 of the zero-padded frame
        # meets taps dh = a, a + 2 and dw = b, b + 2; the phases accumulate through the residual input
        ho, wo = h // 2, w // 2
        hp, wp = 2 * ho + 1, 2 * wo + 1
        key = ("s2f32", t, hp, wp, c)
        buf = self._pool.get(key)
        if buf is None:
            buf = self._pool[key] = torch.zeros((t, hp, wp, c), dtype=torch.float32, device=x.device)
        buf[:, : min(h, hp), : min(w, wp)].copy_(x[:, :hp, :wp])
        fs, rs, ps = hp * wp * c, wp * c, c
        acc = None
        for a in (0, 1):
            for bb in (0, 1):
                wph = wt[:, :, a::2, bb::2].contiguous()
                nxt = torch.empty_like(out) if acc is not None else out
                lib.vae_conv(buf[:, a:, bb:], (fs, 2 * rs, 2 * ps), wph, nxt, t, ho, wo, bias=bias if acc is None else None, resid=acc)
                acc = nxt
        return acc

    def resample_down(self, p, x, mode):
        """Resample.forward, downsample2d / downsample3d (vae.py:141-158)."""
        x = self._down2d(p + "resample.1", x)
        if mode != "downsample3d":
            return x
        t, h, w, c = x.shape
        name = p + "time_conv"
        w16 = self.w16.get(name + ".weight")
        dt = torch.float16 if w16 is not None else torch.float32
        # [cache | x]: the buffer's one leading frame is the reference's feat_cache entry x[:, :, -1:] of the previous chunk (lead = kt - 1 = 1 with kt = 2)
        b = self._input(p + "time", t, h, w, c, 2, 0, dt)
        lib.vae_prep(x, b.interior()[:t], b.strides[:2], split=self.split and w16 is not None)
        if not self._rep.get(p, False):
            self._rep[p] = True  # first chunk: cache the frame, no time_conv (vae.py:146-149)
            b.roll(t)
            return x
        wt = self.w[name + ".weight"]
        out = torch.empty((t // 2, h, w, wt.shape[0]), dtype=torch.float32, device=x.device)
        for j in range(t // 2):  # output frame j reads input frames 2j, 2j + 1, 2j + 2 of [cache | x] (stride 2, no pad)
            src = b.buf[2 * j :]
            if w16 is not None:
                lib.vae_conv16(src, b.strides, w16, out[j : j + 1], 1, h, w, bias=self.w[name + ".bias"])
            else:
                lib.vae_conv(src, b.strides, wt, out[j : j + 1], 1, h, w, bias=self.w[name + ".bias"])
        b.roll(t)
        return out

    def forward(self, video):
        """One chunk: video [3, T, H, W] fp32 (device view) → head output [T', H / 8, W / 8, 2 z_dim] (vae.py:322-374)."""
        x = self.conv1(video)
        for idx, kind, _, _ in self.plan:
            p = f"encoder.downsamples.{idx}."
            x = self.residual_block(p, x) if kind == "res" else self.resample_down(p, x, kind)
        x = self.residual_block("encoder.middle.0.", x)
        x = self.attention_block("encoder.middle.1.", x)
        x = self.residual_block("encoder.middle.2.", x)
        return self._conv_cached("head", "encoder.head.2", x, gamma=self.w["encoder.head.0.gamma"], silu=True)


def encode_chunk_bounds(t, chunk_frames):
    """[a, b) video-frame ranges of the encoder passes: the first frame alone, then `chunk_frames` (a multiple of 4) at a time (vae.py:687-705).
    Like the reference, frames behind the last whole group of 4 (T - 1 not a multiple of 4) are not encoded."""
    if chunk_frames < 4 or chunk_frames % 4:
        raise lib.X2VError(f"encode: chunk_frames must be a positive multiple of 4, got {chunk_frames}")
    if t < 1:
        raise lib.X2VError("encode: the video has no frames")
    t = 1 + (t - 1) // 4 * 4
    edges = [0, 1] + list(range(1 + chunk_frames, t, chunk_frames)) + ([t] if t > 1 else [])
    return list(zip(edges[:-1], edges[1:]))


def _check_video(model, x, chunk_frames):
    if x.dim() != 5 or x.shape[0] != 1 or x.shape[1] != 3:
        raise lib.X2VError(f"encode: expected a [1, 3, T, H, W] video, got {tuple(x.shape)}")
    chunk_frames = model.encode_chunk_frames if chunk_frames is None else int(chunk_frames)
    bounds = encode_chunk_bounds(x.shape[2], chunk_frames)
    if "encoder.conv1.weight" not in model.sd or "conv1.weight" not in model.sd:
        raise lib.X2VError("encode: the state dict holds no encoder (encoder.* / conv1.* tensors)")
    video = x[0].to(device=model.device, dtype=torch.float32)
    return (video if video.stride(3) == 1 else video.contiguous()), bounds


def _mu(model, enc, video, bounds, scale):
    """Encoder passes over `video` [3, T, H, W] (a device view) + conv1 → normalised mu, channels-last [T_lat, H / 8, W / 8, z_dim]."""
    sd = model.sd
    enc.clear_cache()
    outs = [enc.forward(video[:, a:b]) for a, b in bounds]
    enc.clear_cache()
    z2 = model.z_dim
    feat = torch.cat(outs, dim=0) if len(outs) > 1 else outs[0]  # [T_lat, h, w, 2 z_dim]
    tl, hl, wl, _ = feat.shape
    # conv1 (1x1, vae.py:706) keeping mu only, (mu - mean) * inv_std folded in (vae.py:707-710)
    mean, inv_std = (s.to(device=model.device, dtype=torch.float32).reshape(-1) for s in scale)
    w1 = sd["conv1.weight"].to(device=model.device, dtype=torch.float32).reshape(2 * z2, 2 * z2)[:z2]
    b1 = sd["conv1.bias"].to(device=model.device, dtype=torch.float32)[:z2]
    wf = (w1 * inv_std[:, None]).contiguous()
    bf = ((b1 - mean) * inv_std).contiguous()
    mu = torch.empty((tl, hl, wl, z2), dtype=torch.float32, device=model.device)
    lib.vae_conv(feat, (hl * wl * 2 * z2, wl * 2 * z2, 2 * z2), wf, mu, tl, hl, wl, bias=bf)
    return mu


def encode(model, x, scale, chunk_frames=None):
    """WanVAE_.encode (vae.py:684-711) for vae.WanVAE_ `model`: x [1, 3, T, H, W] → mu [1, z_dim, 1 + (T - 1) // 4, H / 8, W / 8] fp32, normalised."""
    video, bounds = _check_video(model, x, chunk_frames)
    h, w = video.shape[2:]
    enc = model.encoder
    if enc is None or (enc.h0, enc.w0) != (h, w):
        enc = model.encoder = Encoder3d(model.sd, model.dim, (h, w), model.device, conv16=model.conv16)
    return _mu(model, enc, video, bounds, scale).permute(3, 0, 1, 2).unsqueeze(0).contiguous()


def tiled_encode(model, x, scale, chunk_frames=None):
    """WanVAE_.tiled_encode (vae.py:568-629): every 256 x 256 px tile of the video (a strided view of the resident video, read in place by conv1's producer)
    goes through the encoder of its geometry with a cleared cache, in the usual frame chunks; the tiles' normalised mu [T_lat, th, tw, z_dim] are blended
    in latent units, cropped to the stride and stored channel-first by x2v_vae_tile_compose_f32 (no clamp).  H and W must be multiples of 8: the tile
    starts are multiples of the 8-aligned stride, and a tile of fewer than 8 rows or columns has no latent."""
    from .vae import compose_tiles, tile_plan

    video, bounds = _check_video(model, x, chunk_frames)
    _, t, h, w = video.shape
    if h % 8 or w % 8:
        raise lib.X2VError(f"tiled encode: the video's height and width must be multiples of 8, got {h}x{w}")
    plan = tile_plan(h // 8, w // 8, *model.tile_geometry())
    raw = []
    for p in plan["tiles"]:
        hw = (8 * p["th"], 8 * p["tw"])
        enc = model._tile_module(Encoder3d, model._tile_encoders, model.encoder, (h, w), hw)
        raw.append(_mu(model, enc, video[:, :, 8 * p["y0"] : 8 * p["y0"] + hw[0], 8 * p["x0"] : 8 * p["x0"] + hw[1]], bounds, scale))
    out = torch.empty((1, model.z_dim, raw[0].shape[0], h // 8, w // 8), dtype=torch.float32, device=model.device)
    compose_tiles(plan, raw, out[0])
    return out


def i2v_latent_hw(img_h, img_w, target_height, target_width, vae_stride, patch_size):
    """run_vae_encoder's latent size (wan_runner.py:207-213): (lat_h, lat_w)."""
    import numpy as np

    aspect_ratio = img_h / img_w
    max_area = target_height * target_width
    lat_h = round(np.sqrt(max_area * aspect_ratio) // vae_stride[1] // patch_size[1] * patch_size[1])
    lat_w = round(np.sqrt(max_area / aspect_ratio) // vae_stride[2] // patch_size[2] * patch_size[2])
    return int(lat_h), int(lat_w)


def i2v_first_frame_mask(target_video_length, lat_h, lat_w, device="cpu"):
    """run_vae_encoder's mask (wan_runner.py:218-229): [4, 1 + (T - 1) / 4, lat_h, lat_w], ones on the frames of latent frame 0."""
    msk = torch.ones(1, target_video_length, lat_h, lat_w, device=device)
    msk[:, 1:] = 0
    msk = torch.concat([torch.repeat_interleave(msk[:, 0:1], repeats=4, dim=1), msk[:, 1:]], dim=1)
    msk = msk.view(1, msk.shape[1] // 4, 4, lat_h, lat_w)
    return msk.transpose(1, 2)[0]


def i2v_video(img, target_video_length, lat_h, lat_w, vae_stride):
    """The encoder's input of run_vae_encoder (wan_runner.py:230-241): img [3, h, w] in [-1, 1] resized bicubically ON THE CPU to the latent grid's
    pixel size, followed by target_video_length - 1 zero frames → [3, T, H, W] fp32 (CPU)."""
    h, w = lat_h * vae_stride[1], lat_w * vae_stride[2]
    first = torch.nn.functional.interpolate(img[None].float().cpu(), size=(h, w), mode="bicubic").transpose(0, 1)
    return torch.concat([first, torch.zeros(3, target_video_length - 1, h, w)], dim=1)


def run_vae_encoder(vae, img, target_height, target_width, target_video_length, vae_stride=(4, 8, 8), patch_size=(1, 2, 2), args=None):
    """WanRunner.run_vae_encoder after the PIL → tensor step (wan_runner.py:204-248): img [3, h, w] in [-1, 1] → (vae_encode_out
    [4 + z_dim, 1 + (T - 1) / 4, lat_h, lat_w] bf16 on the VAE's device, lat_h, lat_w) with `vae` a vae.WanVAE holding encoder weights."""
    lat_h, lat_w = i2v_latent_hw(img.shape[1], img.shape[2], target_height, target_width, vae_stride, patch_size)
    video = i2v_video(img, target_video_length, lat_h, lat_w, vae_stride)
    msk = i2v_first_frame_mask(target_video_length, lat_h, lat_w, device=vae.device)
    z = vae.encode([video.to(vae.device)], args)[0]
    return torch.concat([msk, z]).to(torch.bfloat16), lat_h, lat_w


def encode_flops(t, h, w, dim=96, z_dim=16):
    """Convolution / attention FLOP of one encode of a [3, t, h, w] video counted from the shapes (2 per multiply-add; the algorithmic fp32 count —
    the split mode multiplies three 16-bit products per fp32 one).  {stage name: FLOP}."""
    dims, plan = synth.wan_vae_encoder_plan(dim)
    f = {}

    def add(k, v):
        f[k] = f.get(k, 0) + v

    add("conv1", 2 * t * h * w * dims[0] * 3 * 27)
    for _, kind, cin, cout in plan:
        if kind == "res":
            add(f"res {cout}@{h}x{w}", 2 * t * h * w * cout * (cin + cout) * 27 + (2 * t * h * w * cout * cin if cin != cout else 0))
        else:
            h, w = h // 2, w // 2
            add(f"down {cout}@{h}x{w}", 2 * t * h * w * cout * cin * 9)
            if kind == "downsample3d":
                t_new = 1 + (t - 1) // 2
                add(f"down {cout}@{h}x{w}", 2 * (t_new - 1) * h * w * cout * cin * 3)
                t = t_new
    c = dims[-1]
    add(f"middle {c}@{h}x{w}", 2 * (2 * t * h * w * c * c * 27 * 2))
    n = h * w
    add(f"middle {c}@{h}x{w}", t * (2 * n * c * 3 * c + 2 * 2 * n * n * c + 2 * n * c * c))
    add(f"head {2 * z_dim}@{h}x{w}", 2 * t * h * w * 2 * z_dim * c * 27 + 2 * t * h * w * z_dim * 2 * z_dim)
    return f


__all__ = ["Encoder3d", "encode", "tiled_encode", "encode_chunk_bounds", "encode_flops", "i2v_first_frame_mask", "i2v_latent_hw", "i2v_video", "run_vae_encoder"]
