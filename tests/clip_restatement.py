"""TEST INFRASTRUCTURE ONLY — plain-PyTorch restatement of the reference's CLIP image tower, the checker of lightx2v_amd/clip.py.

reference: lightx2v/models/input_encoders/hf/xlm_roberta/model.py — CLIPModel.visual :436-450 (bicubic resize to 224 x 224, x * 0.5 + 0.5,
Normalize with the constants of :379-380, the forward under fp16 autocast) · VisionTransformer.forward(use_31_block=True) :274-295 (patch
embedding, class token, pos_embedding, pre_norm, transformer[:-1]; no post_norm, no head) · AttentionBlock.forward :157-164 (pre-norm form) ·
SelfAttention.forward :75-91 (one to_qkv Linear viewed (b, s, 3, n, d), non-causal SDPA, proj) · LayerNorm.forward :47-49 (fp32, cast back) ·
nn.GELU() (exact).  `dtype` is the model's: torch.float32 (the truth) or torch.float16 (what the reference runs: fp16 weights and activations,
LayerNorm in fp32 with fp32 parameters — what CUDA / CPU autocast makes of the module).  Pinned to tests/golden/clip_visual_tiny.*.safetensors
(tools/gen_golden_clip.py, generated from the unmodified reference) by tests/test_clip_host.py.
"""
import functools

import torch
import torch.nn.functional as F

from lightx2v_amd import synth


@functools.lru_cache(maxsize=None)
def _mean_std(mean, std, dtype, device):
    return torch.tensor(mean, dtype=dtype, device=device).view(1, 3, 1, 1), torch.tensor(std, dtype=dtype, device=device).view(1, 3, 1, 1)


def preprocess(videos, image_size=224, mean=synth.CLIP_MEAN, std=synth.CLIP_STD):
    """model.py:440-442: list of [3, T, H, W] in [-1, 1] → [sum T, 3, S, S] fp32.  The two constant tensors are built once per device."""
    x = torch.cat([F.interpolate(u.float().transpose(0, 1), size=(image_size, image_size), mode="bicubic", align_corners=False) for u in videos])
    x = x.mul(0.5).add(0.5)
    m, s = _mean_std(tuple(mean), tuple(std), x.dtype, x.device)
    return x.sub(m).div(s)  # torchvision's Normalize: tensor.sub_(mean).div_(std)


class Prepared(dict):
    """A weight dict as the module holds it: see prepare()."""


def prepare(sd, dtype, device):
    """The visual parameters on `device` as the reference module holds them under autocast: `dtype` everywhere except the LayerNorm parameters, which
    stay fp32 (LayerNorm.forward :47-49 computes in fp32).  forward() does this itself for a plain dict; a caller that times repeated forwards prepares
    once, as a loaded module would."""
    return Prepared({k: (v.to(device=device, dtype=torch.float32 if "norm" in k else dtype) if v.is_floating_point() else v) for k, v in sd.items() if k.startswith("visual.")})


def layer_norm(w, p, x, eps=1e-5):
    return F.layer_norm(x.float(), (x.shape[-1],), w[p + ".weight"], w[p + ".bias"], eps).type_as(x)


def forward(sd, x, dtype=torch.float32, num_heads=None, blocks=None, eps=1e-5):
    """VisionTransformer.forward(x, use_31_block=True) on preprocessed x [B, 3, S, S]; `blocks`: how many to run (default: all but the last)."""
    w = sd if isinstance(sd, Prepared) else prepare(sd, dtype, x.device)
    dim = w["visual.patch_embedding.weight"].shape[0]
    n = num_heads or dim // 80
    layers = 1 + max(int(k.split(".")[2]) for k in w if k.startswith("visual.transformer."))
    blocks = layers - 1 if blocks is None else blocks
    b = x.shape[0]
    x = F.conv2d(x.to(dtype), w["visual.patch_embedding.weight"], stride=w["visual.patch_embedding.weight"].shape[-1]).flatten(2).permute(0, 2, 1)
    x = torch.cat([w["visual.cls_embedding"].expand(b, -1, -1), x], dim=1)
    x = x + w["visual.pos_embedding"]
    x = layer_norm(w, "visual.pre_norm", x, eps)
    for i in range(blocks):
        p = f"visual.transformer.{i}."
        h = layer_norm(w, p + "norm1", x, eps)
        s = h.shape[1]
        q, k, v = F.linear(h, w[p + "attn.to_qkv.weight"], w[p + "attn.to_qkv.bias"]).view(b, s, 3, n, dim // n).unbind(2)
        a = F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)).transpose(1, 2).reshape(b, s, dim)
        x = x + F.linear(a, w[p + "attn.proj.weight"], w[p + "attn.proj.bias"])
        h = layer_norm(w, p + "norm2", x, eps)
        h = F.gelu(F.linear(h, w[p + "mlp.0.weight"], w[p + "mlp.0.bias"]))
        x = x + F.linear(h, w[p + "mlp.2.weight"], w[p + "mlp.2.bias"])
    return x


def visual(sd, videos, dtype=torch.float32, device="cpu", num_heads=None):
    """CLIPModel.visual(videos, args) → [B, tokens, dim] in `dtype`."""
    grid = int(round((sd["visual.pos_embedding"].shape[1] - 1) ** 0.5))
    size = grid * sd["visual.patch_embedding.weight"].shape[-1]
    with torch.no_grad():
        return forward(sd, preprocess([u.to(device) for u in videos], size), dtype=dtype, num_heads=num_heads)
