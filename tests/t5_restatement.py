"""Plain-PyTorch restatement of the reference's umT5 encoder (lightx2v/models/input_encoders/hf/t5/model.py: T5Encoder.forward :314-347, T5SelfAttention
:190-205, T5Attention :99-136, T5FeedForward :158-170, GELU :58, T5LayerNorm :68-72, T5RelativeEmbedding :255-281) on a name → tensor state dict.

dtype=torch.bfloat16 follows the reference's op and rounding order exactly, padding and key mask included: it equals tests/golden/t5_encoder_tiny (generated
from the unmodified reference) bit for bit (tests/test_t5_host.py).  dtype=torch.float32 / float64 drop every bf16 cast and are the truth the HIP encoder is
measured against (the reference's own fp32 build does not run: :128 casts P to bf16 unconditionally)."""
import math

import torch
import torch.nn.functional as F

from lightx2v_amd.t5 import relative_position_bucket


def gelu(x):
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * torch.pow(x, 3.0))))


def layer_norm(x, weight, eps=1e-6):
    stat = torch.float64 if x.dtype == torch.float64 else torch.float32
    x = x * torch.rsqrt(x.to(stat).pow(2).mean(dim=-1, keepdim=True) + eps)
    if weight.dtype in (torch.float16, torch.bfloat16):
        x = x.type_as(weight)
    return weight * x


def bucket_map(length, num_buckets=32, device="cpu"):
    """[length, length] buckets of key position - query position (T5RelativeEmbedding.forward :259-260) on `device`.  The map is evaluated by the host
    function the HIP path builds its tables from (on the CPU the reference's own expression, bit for bit) and moved: the reference evaluates it on its
    device once per block, so a caller that times this restatement passes the map in (`rel_buckets`) and leaves that work out of the clock."""
    rel = torch.arange(length).unsqueeze(0) - torch.arange(length).unsqueeze(1)
    return relative_position_bucket(rel, num_buckets).to(device)


def encoder(sd, ids, mask, dtype=torch.bfloat16, device="cpu", rel_buckets=None):
    """ids, mask [B, L] → [B, L, dim] (bf16 in the bf16 mode, as T5Encoder.forward returns it; `dtype` otherwise), padded rows included.
    rel_buckets: bucket_map(L, buckets, device) computed by the caller (default: computed here, once per call)."""
    sd = {k: v.to(device=device, dtype=dtype) for k, v in sd.items()}
    ids, mask = ids.to(device), mask.to(device)
    heads = sd["blocks.0.pos_embedding.embedding.weight"].shape[1]
    layers = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
    p_dtype = torch.bfloat16 if dtype == torch.bfloat16 else dtype  # :128 `.to(torch.bfloat16)`
    x = F.embedding(ids, sd["token_embedding.weight"])
    b, L = ids.shape
    if rel_buckets is None:
        rel_buckets = bucket_map(L, sd["blocks.0.pos_embedding.embedding.weight"].shape[0], device)
    for i in range(layers):
        p = f"blocks.{i}."
        emb = sd[p + "pos_embedding.embedding.weight"]
        e = F.embedding(rel_buckets, emb).permute(2, 0, 1).unsqueeze(0).contiguous()  # [1, N, Lq, Lk]: on the device, per block, as the reference
        h = layer_norm(x, sd[p + "norm1.weight"])
        c = sd[p + "attn.q.weight"].shape[0] // heads
        q = F.linear(h, sd[p + "attn.q.weight"]).view(b, -1, heads, c)
        k = F.linear(h, sd[p + "attn.k.weight"]).view(b, -1, heads, c)
        v = F.linear(h, sd[p + "attn.v.weight"]).view(b, -1, heads, c)
        attn_bias = h.new_zeros(b, heads, L, L)
        attn_bias += e
        attn_bias.masked_fill_(mask.view(b, 1, 1, -1) == 0, torch.finfo(h.dtype).min)
        attn = torch.einsum("binc,bjnc->bnij", q, k) + attn_bias
        attn = F.softmax(attn.double() if dtype == torch.float64 else attn.float(), dim=-1).to(p_dtype)
        a = torch.einsum("bnij,bjnc->binc", attn, v).reshape(b, -1, heads * c)
        x = x + F.linear(a, sd[p + "attn.o.weight"])
        h = layer_norm(x, sd[p + "norm2.weight"])
        x = x + F.linear(F.linear(h, sd[p + "ffn.fc1.weight"]) * gelu(F.linear(h, sd[p + "ffn.gate.0.weight"])), sd[p + "ffn.fc2.weight"])
    x = layer_norm(x, sd["norm.weight"])
    return x.to(torch.bfloat16) if dtype == torch.bfloat16 else x


def infer_ids(sd, ids, mask, dtype=torch.bfloat16, device="cpu", rel_buckets=None):
    """T5EncoderModel.infer after tokenisation (:588-601): the valid rows of each prompt."""
    out = encoder(sd, ids, mask, dtype, device, rel_buckets)
    return [u[:n] for u, n in zip(out, mask.gt(0).sum(dim=1).tolist())]


def pad_to(ids, mask, length):
    """Right-pad [B, L] ids / mask with zeros to `length` columns (the tokenizer's padding="max_length")."""
    return F.pad(ids, (0, length - ids.shape[1])), F.pad(mask, (0, length - mask.shape[1]))
