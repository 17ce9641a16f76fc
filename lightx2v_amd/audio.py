"""The audio adapter of the audio-driven Wan model (reference: wan/audio_adapter.py AudioAdapter / PerceiverAttentionCA; wan/audio_model.py hands its
`forward` result to the block stack as `audio_dit_blocks`).  After a DiT block, each latent frame's h w tokens cross-attend that frame's own 128 audio
tokens and the result is added to the residual stream, gated.

Same parameter names and state-dict keys as the reference (`ca.{i}.norm_kv`, `norm_q`, `to_q`, `to_kv`, `to_out`, `shift_scale_gate`, `audio_pe`,
`time_embedding.*`, `audio_proj.*`), and `forward` returns the same {block_idx: {"modify_func", "kwargs"}} dict, so both this project's Wan driver
(wan.WanTransformerInfer) and the reference's WanAudioModel through the plugin can consume it.

What runs where:
  once per video   audio_proj (interpolation, transformer decoder, MLP, LayerNorm), the frame regrouping and `+ audio_pe` — PyTorch-ROCm plumbing, off
                   the hot path — then per adapter layer K, V = to_kv(norm_kv(audio tokens)) through lib.layernorm / lib.gemm.  None of it depends on
                   the timestep: computed on first use and cached, keyed on the audio tensor object (and its version) and latent_frame.
  per step         time_embedding(timestep) -> t_emb [1, 3, D] (three 1-row linears: plumbing), per layer shift, scale, gate = t_emb + shift_scale_gate.
  per layer        on the first n_query_tokens rows of x: lib.layernorm with adaLN scale / shift, the to_q GEMM, lib.attention_frames (the per-frame
                   kernel, attn_frames.hip), the to_out GEMM with the gated-residual epilogue (resid = x, gate = gate * weight) IN PLACE: the tail
                   rows (reference-image tokens, padding) are never touched, and the residual add costs no pass of its own.

LIMIT: single GPU only.  There is no multi-GPU driver for the audio model (as with radial and mxfp8 attention): rows are frame-aligned from row 0
(`sp_rank = 0` in the reference's terms); the kernel's row0 / partial-frame form is covered by the kernel tests only.  A rank without query rows
(n_query_tokens == 0) is a no-op here, not the reference's fake attention (which exists for FSDP)."""
import math

import torch
import torch.nn.functional as F
from torch import nn

from . import lib

LN_EPS = 1e-5  # nn.LayerNorm's default: norm_kv, norm_q, audio_proj.norm


class AudioProjection(nn.Module):
    """audio features [B, L, C] -> [B, video_frame, num_tokens, mlp_dims[-1] / num_tokens]: resample to one feature per video frame, refine against
    the original sequence (transformer decoder), gather each frame's (left, right) neighbours, MLP, split into tokens, LayerNorm."""

    def __init__(self, audio_feature_dim=768, n_neighbors=(2, 2), num_tokens=32, mlp_dims=(1024, 1024, 32 * 768), transformer_layers=4):
        super().__init__()
        self.left, self.right = n_neighbors
        self.audio_frames, self.num_tokens = sum(n_neighbors) + 1, num_tokens
        dims, layers = (audio_feature_dim * self.audio_frames, *mlp_dims), []
        for i in range(len(mlp_dims)):
            layers += [nn.Linear(dims[i], dims[i + 1])] + ([nn.ReLU()] if i + 1 < len(mlp_dims) else [])
        self.mlp = nn.Sequential(*layers)
        self.norm = nn.LayerNorm(mlp_dims[-1] // num_tokens)
        self.transformer_decoder = None
        if transformer_layers > 0:
            layer = nn.TransformerDecoderLayer(d_model=audio_feature_dim, nhead=audio_feature_dim // 64, dim_feedforward=4 * audio_feature_dim, dropout=0.0, batch_first=True)
            self.transformer_decoder = nn.TransformerDecoder(layer, num_layers=transformer_layers)

    def forward(self, audio_feature, latent_frame):
        video_frame = (latent_frame - 1) * 4 + 1
        x = F.interpolate(audio_feature.transpose(1, 2), size=video_frame, mode="linear", align_corners=False).transpose(1, 2)
        if self.transformer_decoder is not None:
            x = self.transformer_decoder(x, audio_feature)
        x = F.pad(x.transpose(1, 2), (self.left, self.right), mode="replicate").transpose(1, 2)
        x = x.unfold(1, self.audio_frames, 1)  # [B, T, C, W]
        x = self.mlp(x.permute(0, 1, 3, 2).flatten(2))
        return self.norm(x.unflatten(2, (self.num_tokens, -1)))


class TimeEmbedding(nn.Module):
    """timestep -> [B, time_proj_dim]: sinusoid (cos first, no frequency shift), Linear, SiLU, Linear, SiLU, Linear."""

    def __init__(self, dim, time_freq_dim, time_proj_dim):
        super().__init__()
        self.time_freq_dim = time_freq_dim
        self.time_embedder = nn.ModuleDict({"linear_1": nn.Linear(time_freq_dim, dim), "linear_2": nn.Linear(dim, dim)})
        self.time_proj = nn.Linear(dim, time_proj_dim)

    def forward(self, timestep):
        half = self.time_freq_dim // 2
        freqs = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float32, device=timestep.device) / half)
        ang = timestep.reshape(-1, 1).float() * freqs
        emb = torch.cat([ang.cos(), ang.sin()], dim=-1).to(self.time_proj.weight.dtype)
        t = self.time_embedder["linear_2"](F.silu(self.time_embedder["linear_1"](emb)))
        return self.time_proj(F.silu(t))


class PerceiverAttentionCA(nn.Module):
    """One adapter layer.  The module holds the parameters; `apply_` is the hot path."""

    def __init__(self, dim_head=128, heads=16, kv_dim=2048, adaLN=False):
        super().__init__()
        if dim_head != 128:
            raise NotImplementedError(f"PerceiverAttentionCA: dim_head={dim_head} (the per-frame attention kernel is built for 128)")
        self.dim_head, self.heads = dim_head, heads
        inner = dim_head * heads
        self.norm_kv = nn.LayerNorm(inner if kv_dim is None else kv_dim)
        self.norm_q = nn.LayerNorm(inner, elementwise_affine=not adaLN)
        self.to_q = nn.Linear(inner, inner)
        self.to_kv = nn.Linear(inner if kv_dim is None else kv_dim, inner * 2)
        self.to_out = nn.Linear(inner, inner)
        if adaLN:
            self.shift_scale_gate = nn.Parameter(torch.randn(1, 3, inner) / inner ** 0.5)
        else:  # constant: no shift, no scale, gate 1
            self.register_buffer("shift_scale_gate", torch.tensor([0.0, 0.0, 1.0]).view(1, 3, 1).repeat(1, 1, inner), persistent=False)
        self._kv = None  # (audio tokens, version, k, v)

    def kv(self, x):
        """K, V [f * 128, H * 128] of the audio tokens x [1, f, 128, C]: step-invariant, computed once per x object."""
        hit = self._kv
        if hit is None or hit[0] is not x or hit[1] != x._version:
            kv = self.compute_kv(x)
            inner = self.heads * self.dim_head
            hit = self._kv = (x, x._version, kv[:, :inner], kv[:, inner:])
        return hit[2], hit[3]

    def compute_kv(self, x):
        n = lib.layernorm(x.reshape(-1, x.shape[-1]), self.norm_kv.weight, self.norm_kv.bias, eps=LN_EPS)
        return lib.gemm(n, self.to_kv.weight, self.to_kv.bias)

    def apply_(self, xa, rows_per_frame, x, t_emb, weight):
        """xa [n, D] <- xa + gate * weight * to_out(attention(to_q(adaLN(xa)), K, V)), in place; row r belongs to frame r // rows_per_frame."""
        ssg = t_emb.float() + self.shift_scale_gate.float()  # [1, 3, D]
        shift, scale = ssg[:, 0].to(xa.dtype), ssg[:, 1].to(xa.dtype)
        gate = (ssg[:, 2] * float(weight)).to(xa.dtype)  # one [1, D] row: the residual add rides the to_out epilogue
        k, v = self.kv(x)
        n = lib.layernorm(xa, self.norm_q.weight, self.norm_q.bias, scale=scale, shift=shift, eps=LN_EPS)
        q = lib.gemm(n, self.to_q.weight, self.to_q.bias)
        a = lib.attention_frames(q, k, v, self.heads, rows_per_frame, keys_per_frame=x.shape[2])
        return lib.gemm(a, self.to_out.weight, self.to_out.bias, epilogue=lib.EPI_RESIDUAL, resid=xa, gate=gate)


def modify_hidden_states(hidden_states, grid_sizes, ca_block, x, t_emb, dtype, weight):
    """The reference's modify_func contract (audio_adapter.py:265-310) on one GPU: the first n_query_tokens rows of hidden_states — the f h w video
    tokens; reference-image tokens and padding behind them are the tail — get the adapter layer's residual, in place.  Returns hidden_states."""
    hs = hidden_states[0] if hidden_states.dim() == 3 else hidden_states
    if hidden_states.dim() == 3 and hidden_states.shape[0] != 1:
        raise NotImplementedError("audio adapter: batch size 1 only")
    t, h, w = (int(g) for g in grid_sizes[0].tolist())
    n_query = t * h * w  # = n_tokens_per_rank - tail_length on the one rank there is
    if hs.shape[0] < n_query:
        raise NotImplementedError("audio adapter: a token shard that ends inside the video (sequence parallelism) has no driver")
    if n_query > 0:  # no query rows: a no-op
        ca_block.apply_(hs[:n_query], h * w, x, t_emb, weight)
    return hidden_states


class AudioAdapter(nn.Module):
    def __init__(self, attention_head_dim=128, num_attention_heads=40, base_num_layers=30, interval=1, audio_feature_dim=768, num_tokens=32,
                 mlp_dims=(1024, 1024, 32 * 768), time_freq_dim=256, projection_transformer_layers=4):
        super().__init__()
        self.audio_proj = AudioProjection(audio_feature_dim, (2, 2), num_tokens, mlp_dims, projection_transformer_layers)
        self.num_tokens_x4 = num_tokens * 4
        kv_dim = mlp_dims[-1] // num_tokens
        self.audio_pe = nn.Parameter(torch.randn(self.num_tokens_x4, kv_dim) * 0.02)
        self.base_num_layers, self.interval = base_num_layers, interval
        self.ca = nn.ModuleList(PerceiverAttentionCA(attention_head_dim, num_attention_heads, kv_dim, adaLN=time_freq_dim > 0)
                                for _ in range(math.ceil(base_num_layers / interval)))
        self.dim = attention_head_dim * num_attention_heads
        self.time_embedding = TimeEmbedding(self.dim, time_freq_dim, self.dim * 3) if time_freq_dim > 0 else None
        self._tokens = None  # (audio_feat, version, latent_frame, tokens)

    @classmethod
    def from_transformer(cls, transformer, audio_feature_dim=1024, interval=1, time_freq_dim=256, projection_transformer_layers=4):
        c = transformer.config
        return cls(c["dim"] // c["num_heads"], c["num_heads"], c["num_layers"], interval=interval, audio_feature_dim=audio_feature_dim, time_freq_dim=time_freq_dim,
                   projection_transformer_layers=projection_transformer_layers, mlp_dims=(1024, 1024, 32 * audio_feature_dim))

    def rearange_audio_features(self, audio_feature):
        """[B, video_frame, N, C] -> [B, latent_frame, 4 N, C]: the first video frame four times (it is a latent frame of its own), then groups of 4."""
        x = torch.cat([audio_feature[:, :1].expand(-1, 4, -1, -1), audio_feature[:, 1:]], dim=1)
        return x.reshape(x.shape[0], x.shape[1] // 4, 4 * x.shape[2], x.shape[3])

    def audio_tokens(self, audio_feat, latent_frame):
        """The step-invariant audio tokens [1, latent_frame, 128, C] in the adapter's dtype: the SAME tensor object for the same audio_feat object
        (and version) and latent_frame, which is what keeps every layer's K / V cached across the denoise loop."""
        hit = self._tokens
        if hit is None or hit[0] is not audio_feat or hit[1] != audio_feat._version or hit[2] != latent_frame:
            p = self.audio_pe
            x = self.rearange_audio_features(self.audio_proj(audio_feat.to(p.dtype), latent_frame)) + p
            if x.shape[0] != 1:
                raise NotImplementedError("audio adapter: batch size 1 only")
            hit = self._tokens = (audio_feat, audio_feat._version, latent_frame, x.contiguous())
        return hit[3]

    @torch.no_grad()
    def forward(self, audio_feat, timestep, latent_frame, weight=1.0):
        x = self.audio_tokens(audio_feat, latent_frame)
        if self.time_embedding is not None:
            t_emb = self.time_embedding(timestep).unflatten(1, (3, -1))
        else:
            t_emb = torch.zeros((1, 3, self.dim), device=x.device, dtype=x.dtype)
        return {base_idx: {"modify_func": modify_hidden_states, "kwargs": {"ca_block": self.ca[i], "x": x, "weight": weight, "t_emb": t_emb, "dtype": x.dtype}}
                for i, base_idx in enumerate(range(0, self.base_num_layers, self.interval))}
