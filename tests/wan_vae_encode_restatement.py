"""TEST INFRASTRUCTURE ONLY — CPU fp32 restatement of the reference's Wan VAE *encode* path, the checker of lightx2v_amd/vae_enc.py.

reference: lightx2v/models/video_encoders/hf/wan/vae.py — Resample downsample2d / downsample3d :96-100,141-158 · Encoder3d :265-374 ·
WanVAE_.encode :684-711.  The shared layers (causal conv with its 2-frame cache, RMS_norm, ResidualBlock, AttentionBlock) are the decode
restatement's (oracle/wan_vae_oracle.py).  Pinned to tests/golden/wan_vae_encode_tiny.*.safetensors (tools/gen_golden_vae_encode.py, generated
from the unmodified reference) by tests/test_vae_encode_host.py.  Tensors are [C, T, H, W] (batch 1 dropped).
"""
import torch
import torch.nn.functional as F

from lightx2v_amd import synth
from oracle.wan_vae_oracle import _Cache, attention_block, residual_block, rms_norm


def resample_down(sd, p, x, cache, mode):
    """vae.py:141-158: ZeroPad2d((0, 1, 0, 1)) + Conv2d(3, stride 2) per frame; downsample3d: the first chunk is cached as is, every later one
    runs time_conv (3,1,1), stride 2, no pad, over [last cached frame | x] and caches x[:, -1:]."""
    xf = F.pad(x.permute(1, 0, 2, 3), (0, 1, 0, 1))
    x = F.conv2d(xf, sd[p + "resample.1.weight"], sd[p + "resample.1.bias"], stride=2).permute(1, 0, 2, 3)
    if mode == "downsample3d":
        key = p + "time"
        state = cache.slots.get(key)
        if state is None:
            cache.slots[key] = x.clone()
        else:
            keep = x[:, -1:].clone()
            x = F.conv3d(torch.cat([state[:, -1:], x], 1).unsqueeze(0), sd[p + "time_conv.weight"], sd[p + "time_conv.bias"], stride=(2, 1, 1)).squeeze(0)
            cache.slots[key] = keep
    return x


def encoder_forward(sd, x, cache, dim):
    """Encoder3d.forward (vae.py:322-374) on one chunk x [3, T, H, W] → [2 z_dim, T', H / 8, W / 8]."""
    _, plan = synth.wan_vae_encoder_plan(dim)
    x = cache.conv("conv1", x, sd["encoder.conv1.weight"], sd["encoder.conv1.bias"])
    for idx, kind, _, _ in plan:
        p = f"encoder.downsamples.{idx}."
        x = residual_block(sd, p, x, cache) if kind == "res" else resample_down(sd, p, x, cache, kind)
    x = residual_block(sd, "encoder.middle.0.", x, cache)
    x = attention_block(sd, "encoder.middle.1.", x)
    x = residual_block(sd, "encoder.middle.2.", x, cache)
    x = F.silu(rms_norm(x, sd["encoder.head.0.gamma"]))
    return cache.conv("head", x, sd["encoder.head.2.weight"], sd["encoder.head.2.bias"])


def encode(sd, video, mean, inv_std, dim=96, z_dim=16):
    """WanVAE_.encode (vae.py:684-711): video [3, T, H, W] in chunks of 1, 4, 4, ... frames → normalised mu [z_dim, 1 + (T - 1) / 4, H / 8, W / 8]."""
    cache = _Cache()
    t = video.shape[1]
    outs = [encoder_forward(sd, video[:, :1], cache, dim)]
    for i in range(1, 1 + (t - 1) // 4):
        outs.append(encoder_forward(sd, video[:, 1 + 4 * (i - 1) : 1 + 4 * i], cache, dim))
    out = torch.cat(outs, 1)
    mu = F.conv3d(out.unsqueeze(0), sd["conv1.weight"], sd["conv1.bias"]).squeeze(0)[:z_dim]
    return (mu - mean.reshape(-1, 1, 1, 1)) * inv_std.reshape(-1, 1, 1, 1)
