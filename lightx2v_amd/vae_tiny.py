"""Wan tiny VAE (TAEHV) decode on the HIP kernels of csrc/taehv.hip — host-side mirror of the reference's `tiny_vae` decoder.

reference: lightx2v/models/video_encoders/hf/tae.py — TAEHV :158-259 (decoder :193-217, patch_tgrow_layers :221-234, decode_video :248-259), MemBlock :24-32,
TGrow :46-55, Clamp :19-21; lightx2v/models/video_encoders/hf/wan/vae_tiny.py — WanVAE_tiny :12-27.  Same class names, same state-dict tensor names
(`decoder.{i}.weight`, `decoder.{i}.conv.{0,2,4}.{weight,bias}`, `decoder.{i}.conv.weight`), all bf16 like the reference.

What is laid out differently for the MI355X:
  * activations are channels-last [T, H, W, C] bf16; every layer is ONE launch of x2v_conv2d_bf16 over all frames of the pass: ReLU, the bias, MemBlock's residual
    add and its cat([x_t, x_{t-1}]) (a K loop over two frames, no concatenated tensor), TGrow's channel -> frame interleave, nn.Upsample (the next 3x3 reads at
    (h >> 1, w >> 1); the upsampled tensor is never written, and TGrow's 1x1 runs at the low resolution, which is the same bits) and the head's x 2 - 1 with the
    channel-first store and the frame trim are read sides and epilogues of the convolutions;
  * Clamp reads the caller's [16, T, h, w] latent and writes the first convolution's channels-last operand;
  * the reference walks the graph one frame at a time (parallel=False) to bound memory; here the whole clip goes through each layer in one pass by default, or
    `chunk_frames` latent frames at a time with each MemBlock's last input frame carried over — every kernel reduces an output value in an order that does not
    depend on the frame, so both give the same bits.
Torch is used for allocation, views and the one-frame memory copies of the chunked decode — memory plumbing, no arithmetic."""
import torch

from . import lib

LATENT_CHANNELS, IMAGE_CHANNELS = 16, 3
WIDTHS = (256, 128, 64, 64)  # tae.py:191
MEMBLOCKS = ((3, 4, 5), (9, 10, 11), (15, 16, 17))
STAGE_ENDS = (5, 11, 17, 21)


class DotDict(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def frame_plan(T, hw, decoder_time_upscale=(True, True), decoder_space_upscale=(True, True, True)):
    """Frames and image size behind each of the four stages for T latent frames of hw = (h, w), the frames to trim, and the output (frames, H, W)."""
    strides = (1, 2 if decoder_time_upscale[0] else 1, 2 if decoder_time_upscale[1] else 1)
    h, w = hw
    stages = [(T, h, w)]
    for s in range(3):
        T, h, w = T * strides[s], h << int(bool(decoder_space_upscale[s])), w << int(bool(decoder_space_upscale[s]))
        stages.append((T, h, w))
    trim = 2 ** sum(bool(u) for u in decoder_time_upscale) - 1
    return dict(stages=stages, strides=strides, trim=trim, out=(max(T - trim, 0), h, w))


class TAEHV:
    """reference: tae.py:158-259 (the decoder; encoder tensors in the state dict are ignored)."""

    latent_channels = LATENT_CHANNELS
    image_channels = IMAGE_CHANNELS

    def __init__(self, sd, device="cuda", decoder_time_upscale=(True, True), decoder_space_upscale=(True, True, True), chunk_frames=None):
        """chunk_frames: latent frames per pass (None: the whole clip).  Weights are converted once: [Cout, C, k, k] -> channels-last [Cout, k, k, C] bf16 (a MemBlock's
        first convolution keeps the reference's channel order, frame t then frame t - 1, which is the kernel's source order); TGrow keeps the last stride * C rows."""
        if chunk_frames is not None and chunk_frames < 1:
            raise ValueError(f"chunk_frames={chunk_frames}")
        self.device, self.chunk_frames = torch.device(device), chunk_frames
        self.time_upscale, self.space_upscale = tuple(bool(u) for u in decoder_time_upscale), tuple(bool(u) for u in decoder_space_upscale)
        self.frames_to_trim = 2 ** sum(self.time_upscale) - 1
        self.strides = (1, 2 if self.time_upscale[0] else 1, 2 if self.time_upscale[1] else 1)
        self.w, self.b = {}, {}

        def take(key, rows=None):
            if key + ".weight" not in sd:
                raise KeyError(f"TAEHV: {key}.weight is missing from the state dict")
            w = sd[key + ".weight"]
            if rows is not None:
                if w.shape[0] < rows:
                    raise ValueError(f"TAEHV: {key}.weight has {w.shape[0]} rows, {rows} are needed")
                w = w[w.shape[0] - rows :]  # patch_tgrow_layers: the last-timestep output channels
            self.w[key] = w.to(device=self.device, dtype=torch.bfloat16).permute(0, 2, 3, 1).contiguous()
            bias = sd.get(key + ".bias")
            self.b[key] = None if bias is None else bias.to(device=self.device, dtype=torch.bfloat16).contiguous()

        take("decoder.1")
        for s, blocks in enumerate(MEMBLOCKS):
            for i in blocks:
                for j in (0, 2, 4):
                    take(f"decoder.{i}.conv.{j}")
            take(f"decoder.{blocks[2] + 2}.conv", rows=self.strides[s] * WIDTHS[s])
            take(f"decoder.{blocks[2] + 3}")
        take("decoder.22")
        self.mem = {}  # chunked decode: MemBlock index -> its last input frame

    def _pass(self, z, t0, t1, out, first, head, stages):
        """Latent frames t0 .. t1 - 1 of z [16, T, h, w] through every layer; the video frames go to `out` [3, T_out, H, W]."""
        conv = lib.conv2d_bf16
        k, (h, w) = t1 - t0, z.shape[2:]
        dev, bf = self.device, torch.bfloat16
        carried = self.chunk_frames is not None
        c0 = lib.taehv_clamp(z[:, t0:t1], torch.empty((k, h, w, LATENT_CHANNELS), dtype=bf, device=dev))
        x = conv(c0, self.w["decoder.1"], torch.empty((k, h, w, WIDTHS[0]), dtype=bf, device=dev), h, w, bias=self.b["decoder.1"], flags=lib.C2D_RELU)
        del c0
        T = k
        for s, blocks in enumerate(MEMBLOCKS):
            a, b = torch.empty_like(x), torch.empty_like(x)
            for i in blocks:
                p = f"decoder.{i}.conv."
                conv(x, self.w[p + "0"], a, h, w, bias=self.b[p + "0"], mem=None if first else self.mem[i], flags=lib.C2D_RELU | lib.C2D_TWO_SOURCE)
                conv(a, self.w[p + "2"], b, h, w, bias=self.b[p + "2"], flags=lib.C2D_RELU)
                conv(b, self.w[p + "4"], a, h, w, bias=self.b[p + "4"], resid=x, flags=lib.C2D_RELU)
                if carried:
                    if i not in self.mem or self.mem[i].shape != x.shape[1:]:
                        self.mem[i] = torch.empty_like(x[0])
                    self.mem[i].copy_(x[-1])
                x, a = a, x
            if stages is not None:
                stages.setdefault(blocks[2], []).append(x.permute(0, 3, 1, 2).clone())
            del a, b
            # nn.Upsample, TGrow, conv: the 1x1 at the low resolution with the time-split, the 3x3 reads it at (h >> 1, w >> 1)
            st, up = self.strides[s], self.space_upscale[s]
            g = conv(x, self.w[f"decoder.{blocks[2] + 2}.conv"], torch.empty((T * st, h, w, WIDTHS[s]), dtype=bf, device=dev), h, w, tsplit=st)
            T, h, w = T * st, h << int(up), w << int(up)
            x = conv(g, self.w[f"decoder.{blocks[2] + 3}"], torch.empty((T, h, w, WIDTHS[s + 1]), dtype=bf, device=dev), h, w,
                     flags=(lib.C2D_UPSAMPLE_READ if up else 0) | (lib.C2D_RELU if s == 2 else 0))
            del g
        if stages is not None:
            stages.setdefault(21, []).append(x.permute(0, 3, 1, 2).clone())
        scale = T // k
        trim = self.frames_to_trim if t0 == 0 else 0
        f0 = 0 if t0 == 0 else t0 * scale - self.frames_to_trim
        if T - trim > 0:
            dst = out[:, f0:]
            conv(x, self.w["decoder.22"], dst, h, w, bias=self.b["decoder.22"], flags=lib.C2D_HEAD if head else 0, frame_trim=trim,
                 out_strides=(dst.stride(1), dst.stride(2), dst.stride(3), dst.stride(0)))

    def _decode(self, z, head, stages=None):
        """z [16, T, h, w] fp32 or bf16 on the device -> [1, 3, T_out, H, W] bf16."""
        if z.dim() != 4 or z.shape[0] != LATENT_CHANNELS:
            raise lib.X2VError(f"TAEHV: expected a [16, T, h, w] latent, got {tuple(z.shape)}")
        if not z.is_cuda:
            raise lib.X2VError(f"TAEHV: the latent is on {z.device}; the x2v HIP path has no CPU fallback")
        lib.init()
        if z.dtype not in (torch.float32, torch.bfloat16):
            z = z.float()
        z = z.contiguous()
        T = z.shape[1]
        plan = frame_plan(T, tuple(z.shape[2:]), self.time_upscale, self.space_upscale)
        To, H, W = plan["out"]
        out = torch.empty((1, IMAGE_CHANNELS, To, H, W), dtype=torch.bfloat16, device=self.device)
        k = T if self.chunk_frames is None else self.chunk_frames
        parts = {} if stages is not None else None
        for t0 in range(0, T, max(k, 1)):
            self._pass(z, t0, min(T, t0 + k), out[0], t0 == 0, head, parts)
        self.mem = {}  # nothing is carried from one clip to the next
        if stages is not None:
            stages.update({i: torch.cat(v, 0) for i, v in parts.items()})
        return out

    def decode_video(self, x, parallel=True, show_progress_bar=False, stages=None):
        """tae.py:248-259: x NTCHW (N = 1) latent -> NTCHW bf16 video in ~[0, 1], the first frames_to_trim frames dropped.  `parallel` is accepted and ignored: the
        pass size is `chunk_frames`, the bits do not depend on it.  stages: a dict that receives the untrimmed outputs of blocks 5, 11, 17, 21 as [T, C, H, W]."""
        if x.dim() != 5 or x.shape[0] != 1:
            raise lib.X2VError(f"TAEHV operates on NTCHW tensors with N = 1, got {tuple(x.shape)}")
        return self._decode(x[0].transpose(0, 1), head=False, stages=stages).transpose(1, 2)


class WanVAE_tiny:
    """reference: wan/vae_tiny.py:12-27 (what WanRunner.load_vae_decoder builds when the config sets `tiny_vae`)."""

    def __init__(self, vae_pth="taew2_1.pth", dtype=torch.bfloat16, device="cuda", chunk_frames=None):
        """vae_pth: a state dict, or the path of the released checkpoint (torch.load, or safetensors by its suffix)."""
        if dtype != torch.bfloat16:
            raise lib.X2VError(f"WanVAE_tiny: the HIP decoder is bf16 (the reference's dtype), got {dtype}")
        self.dtype, self.device = dtype, torch.device(device)
        if isinstance(vae_pth, dict):
            sd = vae_pth
        elif str(vae_pth).endswith(".safetensors"):
            from safetensors.torch import load_file

            sd = load_file(vae_pth)
        else:
            sd = torch.load(vae_pth, map_location="cpu", weights_only=True)
        self.taehv = TAEHV(sd, device=device, chunk_frames=chunk_frames)
        self.temperal_downsample = [True, True, False]
        self.config = DotDict(scaling_factor=1.0, latents_mean=torch.zeros(16), z_dim=16, latents_std=torch.ones(16))

    @torch.no_grad()
    def decode(self, latents, generator=None, return_dict=None, config=None):
        """latents [16, T, h, w] -> [1, 3, 4 T - 3, 8 h, 8 w] bf16 = decode_video(...) * 2 - 1 (the head's epilogue).  The input is not modified."""
        return self.taehv._decode(latents, head=True)
