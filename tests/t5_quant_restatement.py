"""Plain-PyTorch restatement of the reference's QUANTISED umT5 encoder: tests/t5_restatement.py::encoder with every F.linear of T5Attention / T5FeedForward
replaced by what QuantLinearInt8 / QuantLinearFp8 compute (lightx2v/models/input_encoders/hf/q_linear.py:20-39, 69-87): the per-token dynamic activation
quantiser (vLLM's scaled_int8_quant / scaled_fp8_quant, restated as in include/x2v.h), the product of the codes, the two scales, one rounding to the
activation dtype.  The state dict is the quantised layout (`<name>.weight` codes, `<name>.weight_scale` [N, 1] fp32; lightx2v_amd.t5.quantize_state_dict).

dtype=torch.bfloat16 follows the reference's op and rounding order (bf16 activations, fp32 quantiser arithmetic, bf16 Linear outputs); float32 / float64 drop
every bf16 cast and evaluate the quantiser in that precision: float64 is the truth the HIP path is measured against, float32 (an exact int8 product, an
fp32-accumulated e4m3 product) the stand-in for a correct kernel path."""
import torch
import torch.nn.functional as F

from tests.t5_restatement import bucket_map, gelu, layer_norm


def act_quant(h, scheme, stat):
    """Per-token codes (as `stat` values) and scales [.., 1] of h: the contracts of x2v_quant_int8_rowwise / x2v_quant_fp8_rowwise."""
    hf = h.to(stat)
    amax = hf.abs().amax(dim=-1, keepdim=True)
    if scheme == "int8":
        inv = torch.where(amax > 0, torch.tensor(127.0, dtype=stat) / amax, torch.zeros_like(amax))
        return torch.clamp(torch.round(hf * inv), -128, 127), amax / torch.tensor(127.0, dtype=stat)
    sx = torch.clamp(amax / torch.tensor(448.0, dtype=stat), min=1.0 / (448.0 * 512.0))
    return torch.clamp(hf / sx, -448, 448).float().to(torch.float8_e4m3fn).to(stat), sx


def qlinear(h, wq, sw, scheme, dtype):
    stat = torch.float64 if dtype == torch.float64 else torch.float32
    q, sx = act_quant(h, scheme, stat)
    acc = (q.double() @ wq.double().t()).to(stat) if scheme == "int8" or stat == torch.float64 else q @ wq.to(stat).t()  # int8: the exact sum, converted once
    return ((acc * sx) * sw.to(stat).view(-1)).to(dtype)


def encoder(sd, ids, mask, scheme, dtype=torch.bfloat16, device="cpu"):
    """ids, mask [B, L] → [B, L, dim], padded rows included (t5_restatement.encoder's contract)."""
    sd = {k: v.to(device) if k.endswith("weight_scale") or v.dtype in (torch.int8, torch.float8_e4m3fn) else v.to(device=device, dtype=dtype) for k, v in sd.items()}
    ids, mask = ids.to(device), mask.to(device)
    heads = sd["blocks.0.pos_embedding.embedding.weight"].shape[1]
    layers = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
    p_dtype = torch.bfloat16 if dtype == torch.bfloat16 else dtype
    x = F.embedding(ids, sd["token_embedding.weight"])
    b, L = ids.shape
    rel_buckets = bucket_map(L, sd["blocks.0.pos_embedding.embedding.weight"].shape[0], device)

    def lin(h, name):
        return qlinear(h, sd[name + ".weight"], sd[name + ".weight_scale"], scheme, dtype)

    for i in range(layers):
        p = f"blocks.{i}."
        e = F.embedding(rel_buckets, sd[p + "pos_embedding.embedding.weight"]).permute(2, 0, 1).unsqueeze(0).contiguous()
        h = layer_norm(x, sd[p + "norm1.weight"])
        c = sd[p + "attn.q.weight"].shape[0] // heads
        q, k, v = (lin(h, p + "attn." + n).view(b, -1, heads, c) for n in "qkv")
        attn_bias = h.new_zeros(b, heads, L, L)
        attn_bias += e
        attn_bias.masked_fill_(mask.view(b, 1, 1, -1) == 0, torch.finfo(h.dtype).min)
        attn = torch.einsum("binc,bjnc->bnij", q, k) + attn_bias
        attn = F.softmax(attn.double() if dtype == torch.float64 else attn.float(), dim=-1).to(p_dtype)
        x = x + lin(torch.einsum("bnij,bjnc->binc", attn, v).reshape(b, -1, heads * c), p + "attn.o")
        h = layer_norm(x, sd[p + "norm2.weight"])
        x = x + lin(lin(h, p + "ffn.fc1") * gelu(lin(h, p + "ffn.gate.0")), p + "ffn.fc2")
    x = layer_norm(x, sd["norm.weight"])
    return x.to(torch.bfloat16) if dtype == torch.bfloat16 else x


def infer_ids(sd, ids, mask, scheme, dtype=torch.bfloat16, device="cpu"):
    out = encoder(sd, ids, mask, scheme, dtype, device)
    return [u[:n] for u, n in zip(out, mask.gt(0).sum(dim=1).tolist())]
