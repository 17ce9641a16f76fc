"""The TAEHV decoder (the Wan runner's tiny VAE) written from scratch on torch.nn.functional: test infrastructure, pinned to the fixture generated from the unmodified
reference (tests/golden/taehv_tiny.*.safetensors, tests/test_taehv_host.py) and, in float64, the truth of the GPU tests.  Nothing here imports the library.

The graph, by the released checkpoint's indices (state dict `decoder.<i>...`):
   0 Clamp tanh(x / 3) * 3            1 conv3 16 -> 256 + bias, 2 ReLU
   3, 4, 5 MemBlock(256)              6 nearest x2      7 TGrow(256, 1)      8 conv3 256 -> 128
   9, 10, 11 MemBlock(128)           12 nearest x2     13 TGrow(128, 1 | 2) 14 conv3 128 -> 64
  15, 16, 17 MemBlock(64)            18 nearest x2     19 TGrow(64, 1 | 2)  20 conv3 64 -> 64, 21 ReLU      22 conv3 64 -> 3 + bias
MemBlock(x_t) = relu(conv4(relu(conv2(relu(conv0(cat([x_t, x_{t-1}], channels)))))) + x_t), x_{-1} = 0.  TGrow(C, s) = a bias-free 1x1 convolution C -> s C whose
channel block j of frame t becomes frame s t + j; a checkpoint with more rows than s C keeps its LAST s C rows.  The first 2^(time upscales) - 1 output frames are dropped.
Stage boundaries (`stages`): the outputs of blocks 5, 11, 17 and 21.

Every frame is independent except through x_{t-1}, so a clip can be decoded `chunk_frames` latent frames at a time with each MemBlock's last input frame carried over."""
import torch
import torch.nn.functional as F

MEMBLOCKS = (3, 4, 5, 9, 10, 11, 15, 16, 17)
STAGE_ENDS = (5, 11, 17, 21)
WIDTHS = (256, 128, 64, 64)
MUTATIONS = ("zero_past", "future_frame", "tgrow_swapped", "trim_from_end")  # wrong decoders the fixture must tell apart (tools/gen_golden_taehv.py)


def frames_to_trim(time_upscale=(True, True)):
    return 2 ** sum(bool(u) for u in time_upscale) - 1


def out_frames(T, time_upscale=(True, True)):
    return T * 2 ** sum(bool(u) for u in time_upscale) - frames_to_trim(time_upscale)


def tgrow_rows(w, C, stride):
    """patch_tgrow_layers: the last stride * C rows of a TGrow weight."""
    assert w.shape[0] >= stride * C and w.shape[0] % C == 0
    return w[w.shape[0] - stride * C :]


def _memblock(x, sd, i, carry, mutate):
    """x [T, C, H, W]; carry = the frame in front of x[0] or None.  Returns (out, x[-1])."""
    zero = torch.zeros_like(x[:1])
    if mutate == "zero_past":
        past = torch.zeros_like(x)
    elif mutate == "future_frame":
        past = torch.cat([x[1:], zero], 0)
    else:
        past = torch.cat([zero if carry is None else carry[None], x[:-1]], 0)
    p = f"decoder.{i}.conv."
    h = F.relu(F.conv2d(torch.cat([x, past], 1), sd[p + "0.weight"], sd[p + "0.bias"], padding=1))
    h = F.relu(F.conv2d(h, sd[p + "2.weight"], sd[p + "2.bias"], padding=1))
    h = F.conv2d(h, sd[p + "4.weight"], sd[p + "4.bias"], padding=1)
    return F.relu(h + x), x[-1]


def _tgrow(x, w, stride, mutate):
    T, C, H, W = x.shape
    y = F.conv2d(x, tgrow_rows(w, C, stride)).reshape(T, stride, C, H, W)
    if mutate == "tgrow_swapped":
        y = y.flip(1)
    return y.reshape(T * stride, C, H, W)


def _up(x, on):
    return x.repeat_interleave(2, dim=-2).repeat_interleave(2, dim=-1) if on else x


def _run(x, sd, carry, time_upscale, space_upscale, stages, mutate):
    """Frames x [T, 16, h, w] (already in the compute dtype) through blocks 0 .. 22; carry: {block index: frame} updated in place."""
    strides = (1, 2 if time_upscale[0] else 1, 2 if time_upscale[1] else 1)
    x = torch.tanh(x / 3) * 3
    x = F.relu(F.conv2d(x, sd["decoder.1.weight"], sd["decoder.1.bias"], padding=1))
    i = 3
    for stage in range(3):
        for b in range(3):
            x, carry[i + b] = _memblock(x, sd, i + b, carry.get(i + b), mutate)
        if stages is not None:
            stages.setdefault(i + 2, []).append(x)
        x = _tgrow(_up(x, space_upscale[stage]), sd[f"decoder.{i + 4}.conv.weight"], strides[stage], mutate)
        x = F.conv2d(x, sd[f"decoder.{i + 5}.weight"], None, padding=1)
        i += 6
    x = F.relu(x)
    if stages is not None:
        stages.setdefault(21, []).append(x)
    return F.conv2d(x, sd["decoder.22.weight"], sd["decoder.22.bias"], padding=1)


def decode_video(sd, x, dtype=torch.bfloat16, time_upscale=(True, True), space_upscale=(True, True, True), chunk_frames=None, stages=None, mutate=None):
    """TAEHV.decode_video: x NTCHW with N = 1 (rounded to bf16 first, as WanVAE_tiny.decode hands it over) -> NTCHW in `dtype`.
    stages: a dict that receives {5, 11, 17, 21: [T_stage, C, H, W]} (untrimmed).  mutate: one of MUTATIONS — a WRONG decoder."""
    assert x.dim() == 5 and x.shape[0] == 1 and x.shape[2] == 16 and (mutate is None or mutate in MUTATIONS)
    sd = {k: v.to(dtype) for k, v in sd.items() if k.startswith("decoder.")}
    x = x[0].to(torch.bfloat16).to(dtype)
    T = x.shape[0]
    k = T if chunk_frames is None else chunk_frames
    carry, parts, out = {}, {}, []
    with torch.no_grad():
        for t0 in range(0, T, k):
            out.append(_run(x[t0 : t0 + k], sd, carry, time_upscale, space_upscale, parts if stages is not None else None, mutate))
    if stages is not None:
        stages.update({i: torch.cat(v, 0) for i, v in parts.items()})
    y = torch.cat(out, 0)
    trim = frames_to_trim(time_upscale)
    return (y[: y.shape[0] - trim] if mutate == "trim_from_end" else y[trim:])[None]


def wan_decode(sd, latents, dtype=torch.bfloat16, **kw):
    """WanVAE_tiny.decode (vae_tiny.py:21-27): latents [16, T, h, w] -> [1, 3, 4 T - 3, 8 h, 8 w], decode_video's result times 2 minus 1, each rounded in `dtype`."""
    v = decode_video(sd, latents.unsqueeze(0).transpose(1, 2), dtype=dtype, **kw)
    return v.transpose(1, 2).mul(2).sub(1)
