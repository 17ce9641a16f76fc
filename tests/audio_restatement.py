"""float64 restatement of the audio adapter's layer (PerceiverAttentionCA.forward) and of modify_hidden_states on one GPU, written fresh from the
contract in lightx2v_amd/audio.py: plain PyTorch on the CPU, nothing here imports the library.  flash_attn is not available where the fixtures of this
suite are made, so there is NO reference-generated fixture for the adapter: this restatement is the yardstick.

Nothing between the inputs and the result is rounded, except the three [1, D] rows the driver makes on the host once per step and layer, which are
inputs of the kernels: shift, scale = bf16(t_emb + shift_scale_gate)[0, 1], gate = bf16((t_emb + shift_scale_gate)[2] * weight).

Bar (`check`): got = bf16(x + r) where the residual r has passed six bf16 roundings (norm_kv's output, K / V, the adaLN output, q, the attention's P and
O, the gated product in the epilogue), each <= 2^-8 relative per element; the score errors they cause reach the result through the softmax, d w / w <=
ln 2 |d s| with |s| of a few base-2 units.  Allowed: ||got - ref|| <= 2^-8 ||ref|| (the last rounding of x + r) + 8 * 2^-8 ||r|| (six roundings and
the softmax's share).  A residual from the wrong frame's audio, or a missing one, is off by ~||r||: 32 times the second term."""
import torch

F64 = torch.float64


def layer_norm(x, w=None, b=None, eps=1e-5):
    y = (x - x.mean(-1, keepdim=True)) / torch.sqrt(x.var(-1, unbiased=False, keepdim=True) + eps)
    return y if w is None else y * w + b


def params(ca_block):
    """The layer's tensors in float64 on the CPU, by state-dict name (+ the non-persistent constant shift_scale_gate)."""
    p = {k: v.detach().to("cpu", F64) for k, v in ca_block.state_dict().items()}
    p["shift_scale_gate"] = ca_block.shift_scale_gate.detach().to("cpu", F64)
    return p


def rows(p, t_emb, weight):
    ssg = t_emb.detach().to("cpu", F64) + p["shift_scale_gate"]
    bf = lambda t: t.to(torch.bfloat16).to(F64)
    return bf(ssg[:, 0]), bf(ssg[:, 1]), bf(ssg[:, 2] * float(weight))


def residual(xa, tokens, p, t_emb, weight, heads, rows_per_frame):
    """xa [n, D] (row r of frame r // rows_per_frame), tokens [f, Kf, C] -> gate * weight * to_out(attention(to_q(adaLN(xa)), K_t, V_t)) [n, D]."""
    xa, tokens = xa.to("cpu", F64), tokens.to("cpu", F64)
    shift, scale, gate = rows(p, t_emb, weight)
    kv = layer_norm(tokens, p["norm_kv.weight"], p["norm_kv.bias"]) @ p["to_kv.weight"].T + p["to_kv.bias"]
    k, v = kv.chunk(2, dim=-1)  # [f, Kf, D]
    q = (layer_norm(xa, p.get("norm_q.weight"), p.get("norm_q.bias")) * (1 + scale) + shift) @ p["to_q.weight"].T + p["to_q.bias"]
    n, d = xa.shape[0], xa.shape[1] // heads
    out = torch.empty_like(xa)
    for t in range((n + rows_per_frame - 1) // rows_per_frame):
        r = slice(t * rows_per_frame, min((t + 1) * rows_per_frame, n))
        for h in range(heads):
            c = slice(h * d, (h + 1) * d)
            out[r, c] = torch.softmax(q[r, c] @ k[t][:, c].T / d ** 0.5, dim=-1) @ v[t][:, c]
    return (out @ p["to_out.weight"].T + p["to_out.bias"]) * gate


def modify_hidden_states(hidden, grid, tokens, p, t_emb, weight, heads):
    """hidden [rows, D]: the first f h w rows get the residual, the tail stays.  Returns (result, residual), float64."""
    f, h, w = grid
    out = hidden.to("cpu", F64).clone()
    r = residual(out[: f * h * w], tokens, p, t_emb, weight, heads, h * w)
    out[: f * h * w] += r
    return out, r


def check(got, ref, r, what=""):
    err, bar = float((got.to("cpu", F64) - ref).norm()), 2.0 ** -8 * float(ref.norm()) + 2.0 ** -5 * float(r.norm())
    print(f"audio {what}: ||got - ref|| {err:.4e}  bar {bar:.4e}  ||r|| {float(r.norm()):.4e}  ||ref|| {float(ref.norm()):.4e}")
    assert err <= bar, f"{what}: ||got - ref|| = {err:.4e} > {bar:.4e}"
