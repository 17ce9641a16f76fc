"""Plain-PyTorch restatement of what the reference's TextEncoderHFClipModel.infer computes after tokenisation (lightx2v/models/input_encoders/hf/clip/
model.py:41-47 around transformers' CLIPTextModel): pooler_output on a name → tensor state dict (CLIPTextModel names, with or without `text_model.`) and
a dims dict (synth.CLIP_TEXT_DIMS keys).

dtype is a parameter: float64 is the truth, float32 / float16 run the same statements with torch's own rounding of each op (see tests/llama_restatement.py
on what that does and does not promise).  `slip` applies one of the single mistakes tests/test_hunyuan_text_host.py must be able to tell from the truth."""
import torch
import torch.nn.functional as F

from lightx2v_amd.clip_text import eos_position

SLIPS = ("pool_last", "exact_gelu", "non_causal")


def quick_gelu(v):
    return v * torch.sigmoid(1.702 * v)


def text_model(sd, dims, ids, mask, dtype=torch.float64, device="cpu", slip=None):
    """ids, mask [B, L] → final_layer_norm(x) [B, L, dim] in `dtype`."""
    assert slip is None or slip in SLIPS
    sd = {(k[len("text_model."):] if k.startswith("text_model.") else k): v.to(device=device, dtype=dtype) for k, v in sd.items()}
    ids, mask = ids.to(device), mask.to(device)
    H, eps = dims["heads"], dims["eps"]
    B, L = ids.shape
    D = dims["dim"]
    d = D // H
    x = F.embedding(ids, sd["embeddings.token_embedding.weight"]) + sd["embeddings.position_embedding.weight"][:L]
    allowed = mask.gt(0)[:, None, None, :].expand(B, 1, L, L)
    if slip != "non_causal":
        allowed = allowed & torch.ones(L, L, dtype=torch.bool, device=device).tril()
    neg = torch.finfo(dtype).min
    act = F.gelu if slip == "exact_gelu" else quick_gelu

    def lin(t, name):
        return F.linear(t, sd[name + ".weight"], sd[name + ".bias"])

    def ln(t, name):
        return F.layer_norm(t, (D,), sd[name + ".weight"], sd[name + ".bias"], eps)

    for i in range(dims["layers"]):
        p = f"encoder.layers.{i}."
        h = ln(x, p + "layer_norm1")
        q, k, v = (lin(h, p + "self_attn." + n).view(B, L, H, d).transpose(1, 2) for n in ("q_proj", "k_proj", "v_proj"))
        s = (q @ k.transpose(-1, -2)) * d**-0.5
        s = s.masked_fill(~allowed, neg)
        pr = torch.softmax(s.double() if dtype == torch.float64 else s.float(), dim=-1).to(dtype)
        x = x + lin((pr @ v).transpose(1, 2).reshape(B, L, D), p + "self_attn.out_proj")
        x = x + lin(act(lin(ln(x, p + "layer_norm2"), p + "mlp.fc1")), p + "mlp.fc2")
    return ln(x, "final_layer_norm")


def infer_ids(sd, dims, ids, mask, dtype=torch.float64, device="cpu", slip=None):
    """TextEncoderHFClipModel.infer after tokenisation: (pooler_output [B, dim], mask)."""
    x = text_model(sd, dims, ids, mask, dtype, device, slip)
    pos = torch.full((ids.shape[0],), ids.shape[1] - 1) if slip == "pool_last" else eos_position(ids, dims["eos_token_id"])
    return x[torch.arange(ids.shape[0]), pos.to(x.device)], mask
