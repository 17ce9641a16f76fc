"""Plain-PyTorch restatement of what the reference's TextEncoderHFLlamaModel.infer computes after tokenisation (lightx2v/models/input_encoders/hf/llama/
model.py:54-63 around transformers' LlamaModel): the decoder stack on a name → tensor state dict (LlamaModel.state_dict() names) and a dims dict
(synth.LLAMA_DIMS keys), up to hidden_states[-(skip + 1)], cropped.

dtype is a parameter: float64 is the truth the HIP tower and the reference's fp16 output are measured against, float32 / float16 run the same statements
with torch's own rounding of each op.  It is not expected to equal transformers bit for bit in fp16 (sdpa and eager differ from each other there too); the
fixture test holds it to the reference within a bound that separates every single slip listed in tests/test_hunyuan_text_host.py (`slip`)."""
import torch
import torch.nn.functional as F

SLIPS = ("interleaved_rope", "skip_one_layer_less", "kv_head_modulo", "final_norm", "non_causal")


def rms_norm(x, weight, eps):
    stat = torch.float64 if x.dtype == torch.float64 else torch.float32
    v = x.to(stat)
    v = v * torch.rsqrt(v.pow(2).mean(-1, keepdim=True) + eps)
    return weight * v.to(x.dtype)


def rope_cos_sin(n, head_dim, theta, dtype, device):
    """cos / sin [n, head_dim] of pos * theta^(-2i / head_dim), the head_dim / 2 angles repeated over both halves."""
    inv = torch.tensor(float(theta), dtype=torch.float64) ** (-torch.arange(0, head_dim, 2, dtype=torch.float64) / head_dim)
    ang = torch.arange(n, dtype=torch.float64)[:, None] * inv[None]
    ang = torch.cat([ang, ang], dim=-1)
    return ang.cos().to(device=device, dtype=dtype), ang.sin().to(device=device, dtype=dtype)


def rotate_half(t):
    h = t.shape[-1] // 2
    return torch.cat([-t[..., h:], t[..., :h]], dim=-1)


def rotate_pairs(t):
    """The interleaved-pair rotation (the slip): (t0, t1) -> (-t1, t0) on adjacent elements."""
    return torch.stack([-t[..., 1::2], t[..., 0::2]], dim=-1).flatten(-2)


def decoder(sd, dims, ids, mask, dtype=torch.float64, device="cpu", skip=2, slip=None):
    """ids, mask [B, L] (right-padded) → hidden_states[-(skip + 1)] [B, L, dim] in `dtype`: the residual stream after layer L - skip, no final norm.
    Keys of padded tokens are masked as LlamaModel's padding mask does."""
    assert slip is None or slip in SLIPS
    sd = {k: v.to(device=device, dtype=dtype) for k, v in sd.items()}
    ids, mask = ids.to(device), mask.to(device)
    H, Hkv, d, eps = dims["heads"], dims["kv_heads"], dims["head_dim"], dims["eps"]
    group = H // Hkv
    if slip == "skip_one_layer_less":
        skip -= 1
    B, L = ids.shape
    x = F.embedding(ids, sd["embed_tokens.weight"])
    cos, sin = rope_cos_sin(L, d, dims["rope_theta"], dtype, device)
    allowed = mask.gt(0)[:, None, None, :].expand(B, 1, L, L)
    if slip != "non_causal":
        allowed = allowed & torch.ones(L, L, dtype=torch.bool, device=device).tril()
    neg = torch.finfo(dtype).min
    rot = rotate_pairs if slip == "interleaved_rope" else rotate_half
    for i in range(dims["layers"] - skip):
        p = f"layers.{i}."
        h = rms_norm(x, sd[p + "input_layernorm.weight"], eps)
        q = F.linear(h, sd[p + "self_attn.q_proj.weight"]).view(B, L, H, d).transpose(1, 2)
        k = F.linear(h, sd[p + "self_attn.k_proj.weight"]).view(B, L, Hkv, d).transpose(1, 2)
        v = F.linear(h, sd[p + "self_attn.v_proj.weight"]).view(B, L, Hkv, d).transpose(1, 2)
        q, k = q * cos + rot(q) * sin, k * cos + rot(k) * sin
        kv_of = [(hh % Hkv) if slip == "kv_head_modulo" else hh // group for hh in range(H)]
        k, v = k[:, kv_of], v[:, kv_of]
        s = (q @ k.transpose(-1, -2)) * d**-0.5
        s = s.masked_fill(~allowed, neg)
        pr = torch.softmax(s.double() if dtype == torch.float64 else s.float(), dim=-1).to(dtype)
        a = (pr @ v).transpose(1, 2).reshape(B, L, H * d)
        x = x + F.linear(a, sd[p + "self_attn.o_proj.weight"])
        h = rms_norm(x, sd[p + "post_attention_layernorm.weight"], eps)
        x = x + F.linear(F.silu(F.linear(h, sd[p + "mlp.gate_proj.weight"])) * F.linear(h, sd[p + "mlp.up_proj.weight"]), sd[p + "mlp.down_proj.weight"])
    if slip == "final_norm":
        x = rms_norm(x, sd["norm.weight"], eps)
    return x


def infer_ids(sd, dims, ids, mask, dtype=torch.float64, device="cpu", skip=2, crop_start=95, slip=None):
    """TextEncoderHFLlamaModel.infer after tokenisation: (hidden_states[-(skip + 1)][:, crop_start:], mask[:, crop_start:])."""
    return decoder(sd, dims, ids, mask, dtype, device, skip, slip)[:, crop_start:], mask[:, crop_start:]
