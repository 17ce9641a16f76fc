"""HunyuanVideo's Llama text tower on the HIP kernels (csrc/txt_enc.hip) — the producer of `text_encoder_output["text_encoder_1_text_states"]` and
`["text_encoder_1_attention_mask"]` for t2v.

reference: lightx2v/models/input_encoders/hf/llama/model.py — TextEncoderHFLlamaModel (init :12-25, infer :39-66), which runs transformers' LlamaModel
(AutoModel.from_pretrained(...).to(torch.float16)) on the prompt padded to max_length and returns hidden_states[-(hidden_state_skip_layer + 1)][:, crop_start:]
with the mask cropped the same way; runners/hunyuan/hunyuan_runner.py:30-37 (load_text_encoder), :58-67 (run_text_encoder).

hidden_states[-3] is the residual stream after layer L - 2, without the final norm: only the first L - 2 layers are loaded and run, norm.weight is never
used.  The prompt is right-padded and the attention is causal, so a valid row never sees a padded key: this path runs the n valid tokens only and returns
[1, L - crop_start, D] with the rows from n - crop_start on ZERO (the reference leaves what the model computed on pad tokens there; its consumers read those
rows only through the mask, hunyuan/infer/pre_infer.py:46-47,85-86,98-101).  Per layer 7 launches on one stream — RMSNorm, fused q | k | v GEMM, causal
grouped-query attention with the rotary embedding inside, o GEMM + residual, RMSNorm, gate | up GEMM with the SwiGLU epilogue, down GEMM + residual; one
workspace, sized to the largest n seen.  fp16 activations and weights, fp32 accumulation and statistics, as the reference's fp16 model.  Where it rounds
differently: the norm rounds once (LlamaRMSNorm rounds x * rsqrt(...) to fp16 and the weight product again), q and k are rotated in fp32 and rounded once
(apply_rotary_pos_emb rounds both products and their sum, with cos / sin themselves rounded to fp16), scores and probabilities stay fp32 up to the PV operand
(sdpa / eager round the scores to fp16), SiLU and its product are fp32 on the two fp16 Linear outputs.  The LLaVA tower of i2v, quantised Linears and
cpu_offload are not built.
"""
import json
import os

import torch

from . import lib
from .packed import MAX_PLANS, PackedTower  # noqa: F401

HEAD_DIM = 128  # the rotary form of x2v_attn_f16_causal
MAX_LEN = lib.ATTN_CAUSAL_MAX_LEN


def load_hf_dir(path):
    """(name → tensor dict, config dict) of a transformers model directory: config.json and every *.safetensors shard (by the index file if there is one)."""
    from safetensors.torch import load_file

    cfg_path = os.path.join(path, "config.json")
    if not os.path.isfile(cfg_path):
        raise lib.X2VError(f"{path}: no config.json (a transformers model directory is expected)")
    with open(cfg_path) as f:
        cfg = json.load(f)
    index = os.path.join(path, "model.safetensors.index.json")
    if os.path.isfile(index):
        with open(index) as f:
            files = sorted(set(json.load(f)["weight_map"].values()))
    else:
        files = sorted(f for f in os.listdir(path) if f.endswith(".safetensors"))
    if not files:
        raise lib.X2VError(f"{path}: no *.safetensors file")
    sd = {}
    for f in files:
        sd.update(load_file(os.path.join(path, f)))
    return sd, cfg


def strip_prefix(sd, prefix, probe):
    """The dict with `prefix` removed from every name that carries it, if `prefix + probe` is a name (checkpoints come with or without it)."""
    if prefix + probe in sd:
        return {(k[len(prefix):] if k.startswith(prefix) else k): v for k, v in sd.items()}
    return sd


def rope_tables(theta, head_dim=HEAD_DIM, positions=MAX_LEN):
    """(cos, sin) [positions, head_dim / 2] fp32 of pos * theta^(-2i / head_dim) (transformers' LlamaRotaryEmbedding, rope_type "default"), evaluated in
    fp64 on the host and rounded once."""
    inv = torch.tensor(float(theta), dtype=torch.float64) ** (-torch.arange(0, head_dim, 2, dtype=torch.float64) / head_dim)
    ang = torch.arange(positions, dtype=torch.float64)[:, None] * inv[None]
    return ang.cos().float().contiguous(), ang.sin().float().contiguous()


def interleave_rows(a, b):
    """[2N, K]: row 2n = a[n], row 2n + 1 = b[n] (the operand of the gated GEMM epilogues)."""
    return torch.stack([a, b], dim=1).reshape(2 * a.shape[0], a.shape[1]).contiguous()


def dims_from_config(cfg):
    """The dims dict (synth.LLAMA_DIMS keys) of a transformers Llama config.json."""
    if cfg.get("hidden_act", "silu") != "silu":
        raise lib.X2VError(f"TextEncoderHFLlamaModel: hidden_act {cfg.get('hidden_act')!r}; the SwiGLU epilogue is silu")
    rope = cfg.get("rope_parameters") or cfg.get("rope_scaling") or {}
    if rope.get("rope_type", rope.get("type", "default")) != "default":
        raise lib.X2VError(f"TextEncoderHFLlamaModel: rope scaling {rope} is not built (rope_type: default only)")
    if cfg.get("attention_bias") or cfg.get("mlp_bias"):
        raise lib.X2VError("TextEncoderHFLlamaModel: Linear biases are not built (the released text_encoder has none)")
    heads = int(cfg["num_attention_heads"])
    return dict(vocab=int(cfg["vocab_size"]), dim=int(cfg["hidden_size"]), heads=heads, kv_heads=int(cfg.get("num_key_value_heads") or heads),
                head_dim=int(cfg.get("head_dim") or cfg["hidden_size"] // heads), ffn=int(cfg["intermediate_size"]), layers=int(cfg["num_hidden_layers"]),
                rope_theta=float(rope.get("rope_theta", cfg.get("rope_theta", 10000.0))), eps=float(cfg.get("rms_norm_eps", 1e-6)))


class TextEncoderHFLlamaModel(PackedTower):
    """Same constructor, attributes, `infer`, `to_cuda` and `to_cpu` as the reference's TextEncoderHFLlamaModel; `model_path` may also be a
    (name → tensor dict, dims dict) pair (dims: the keys of synth.LLAMA_DIMS)."""

    def __init__(self, model_path, device):
        self.device, self.model_path = torch.device(device), model_path
        self.init()
        if isinstance(model_path, (tuple, list)):
            sd, dims = model_path[0], dict(model_path[1])
        else:
            sd, cfg = load_hf_dir(str(model_path))
            dims = dims_from_config(cfg)
        self.load(strip_prefix(sd, "model.", "embed_tokens.weight"), dims)

    def init(self):
        self.max_length = 351
        self.hidden_state_skip_layer = 2
        self.crop_start = 95
        self.prompt_template = (
            "<|start_header_id|>system<|end_header_id|>\n\nDescribe the video by detailing the following aspects: "
            "1. The main content and theme of the video."
            "2. The color, shape, size, texture, quantity, text, and spatial relationships of the objects."
            "3. Actions, events, behaviors temporal relationships, physical movement changes of the objects."
            "4. background environment, light, style and atmosphere."
            "5. camera angles, movements, and transitions used in the video:<|eot_id|>"
            "<|start_header_id|>user<|end_header_id|>\n\n{}<|eot_id|>"
        )

    def load(self, sd, dims):
        who = "TextEncoderHFLlamaModel"
        self.dims = dims
        self.vocab, self.dim, self.num_heads, self.num_kv_heads, self.head_dim, self.dim_ffn = (int(dims[k]) for k in ("vocab", "dim", "heads", "kv_heads", "head_dim", "ffn"))
        self.norm_eps, self.rope_theta = float(dims["eps"]), float(dims["rope_theta"])
        self.num_layers = int(dims["layers"]) - self.hidden_state_skip_layer  # hidden_states[-(skip + 1)]: the stream after layer L - skip
        if self.num_layers < 1:
            raise lib.X2VError(f"{who}: {dims['layers']} layers leave none to run before hidden_states[-{self.hidden_state_skip_layer + 1}]")
        if self.head_dim != HEAD_DIM or self.num_heads % self.num_kv_heads:
            raise lib.X2VError(f"{who}: head_dim {self.head_dim} / {self.num_heads} query heads over {self.num_kv_heads} key/value heads; the attention kernel's rotary "
                               f"form takes head_dim {HEAD_DIM} and a whole number of query heads per key/value head")
        if self.dim % 32 or self.dim_ffn % 32:
            raise lib.X2VError(f"{who}: dim {self.dim} and ffn {self.dim_ffn} must be multiples of 32 (the GEMM's k-step)")
        A, KV = self.num_heads * HEAD_DIM, self.num_kv_heads * HEAD_DIM
        self.dim_attn, self.dim_qkv = A, A + 2 * KV

        def w(k, shape):
            if k not in sd:
                raise lib.X2VError(f"{who}: the checkpoint lacks {k}")
            if tuple(sd[k].shape) != shape:
                raise lib.X2VError(f"{who}: {k} is {tuple(sd[k].shape)} but the config gives {shape}")
            return sd[k].to(device=self.device, dtype=torch.float16).contiguous()

        self.embedding = w("embed_tokens.weight", (self.vocab, self.dim))
        self.blocks = []
        for i in range(self.num_layers):
            p = f"layers.{i}."
            self.blocks.append(dict(
                n1=w(p + "input_layernorm.weight", (self.dim,)), n2=w(p + "post_attention_layernorm.weight", (self.dim,)),
                qkv=torch.cat([w(p + "self_attn.q_proj.weight", (A, self.dim)), w(p + "self_attn.k_proj.weight", (KV, self.dim)),
                               w(p + "self_attn.v_proj.weight", (KV, self.dim))]).contiguous(),
                o=w(p + "self_attn.o_proj.weight", (self.dim, A)),
                swiglu=interleave_rows(w(p + "mlp.gate_proj.weight", (self.dim_ffn, self.dim)), w(p + "mlp.up_proj.weight", (self.dim_ffn, self.dim))),
                down=w(p + "mlp.down_proj.weight", (self.dim, self.dim_ffn))))
        self.rope = tuple(t.to(self.device) for t in rope_tables(self.rope_theta))
        self._init_plumbing()

    # ---- plumbing (packed.PackedTower: one workspace, the plan cache) --------------------------------------------------
    def weight_bytes(self):
        """Bytes of Linear weights one forward streams (the launch floor of the tower)."""
        return sum(b[k].numel() * 2 for b in self.blocks for k in ("qkv", "o", "swiglu", "down"))

    def launches(self):
        return 7 * self.num_layers

    def _buffers(self):
        return dict(x=self.dim, h=self.dim, qkv=self.dim_qkv, att=self.dim_attn, f=self.dim_ffn)

    def _launches(self, p, M, cu_arr, batch, stream):
        L, D, A, Q, F, eps = lib._lib, self.dim, self.dim_attn, self.dim_qkv, self.dim_ffn, self.norm_eps
        cos, sin = (t.data_ptr() for t in self.rope)
        plan = []

        def norm(wt):
            plan.append((L.x2v_rmsnorm_f16, (p["x"], D, wt.data_ptr(), p["h"], D, M, D, eps, stream)))

        def gemm(x, wt, y, n, k, epi, ldy, resid=None):
            plan.append((L.x2v_gemm_f16, (p[x], k, wt.data_ptr(), k, None, p[y], ldy, M, n, k, epi, None if resid is None else p[resid], 0 if resid is None else ldy, stream)))

        for b in self.blocks:
            norm(b["n1"])
            gemm("h", b["qkv"], "qkv", Q, D, lib.EPI16_NONE, Q)
            plan.append((L.x2v_attn_f16_causal, (p["qkv"], Q, p["att"], A, cu_arr, batch, self.num_heads, self.num_kv_heads, HEAD_DIM, cos, sin, 0.0, stream)))
            gemm("att", b["o"], "x", D, A, lib.EPI16_RESIDUAL, D, "x")
            norm(b["n2"])
            gemm("h", b["swiglu"], "f", F, D, lib.EPI16_SWIGLU, F)
            gemm("f", b["down"], "x", D, F, lib.EPI16_RESIDUAL, D, "x")
        return plan

    def forward_packed(self, lens):
        """The L - skip layers on the workspace of these lengths (`x` holds the packed token embeddings): → the residual stream [sum(lens), dim] (the workspace)."""
        M = self._run_packed(lens)
        return self._bufs["x"][:M]

    # ---- the reference's interface -------------------------------------------------------------------------------------
    def _valid_length(self, ids, mask):
        who = "TextEncoderHFLlamaModel.infer_ids"
        if ids.dim() != 2 or ids.shape[0] != 1 or tuple(mask.shape) != tuple(ids.shape):
            raise lib.X2VError(f"{who}: ids {tuple(ids.shape)} and mask {tuple(mask.shape)} must both be [1, L]")
        Lp = ids.shape[1]
        if not 1 <= Lp <= MAX_LEN:
            raise lib.X2VError(f"{who}: L = {Lp}; the attention kernel takes at most {MAX_LEN} tokens")
        valid = mask.gt(0).cpu()[0]
        n = int(valid.sum())
        if not bool(valid[:n].all()):
            raise lib.X2VError(f"{who}: the mask must mark a prefix of the row (padding_side=\"right\", llama/model.py:29)")
        if n <= self.crop_start:
            raise lib.X2VError(f"{who}: {n} valid tokens leave no row after crop_start = {self.crop_start} (the prompt template alone is longer)")
        idc = ids.cpu()[0, :n]
        if int(idc.min()) < 0 or int(idc.max()) >= self.vocab:
            raise lib.X2VError(f"{who}: token ids outside the vocabulary of {self.vocab}")
        return n

    def infer_ids(self, ids, mask):
        """ids, mask [1, L] (L <= 512; the mask marks a prefix, as right padding does) → (states [1, L - crop_start, dim] fp16 with the rows of padded
        tokens zero, mask[:, crop_start:]): what TextEncoderHFLlamaModel.infer returns for these ids (llama/model.py:54-63) on the valid rows."""
        n = self._valid_length(ids, mask)
        lib.init()
        tok = ids[0, :n].to(device=self.device, dtype=torch.long)
        torch.index_select(self.embedding, 0, tok, out=self._workspace(n)["x"])  # embed_tokens(ids): a gather (plumbing)
        x = self.forward_packed((n,))
        out = torch.zeros((1, ids.shape[1] - self.crop_start, self.dim), dtype=torch.float16, device=self.device)
        out[0, : n - self.crop_start] = x[self.crop_start : n]
        return out, mask[:, self.crop_start :]

    def _tokenize(self, text):
        if self._tokenizer is None:
            try:
                from transformers import AutoTokenizer

                self._tokenizer = AutoTokenizer.from_pretrained(self.model_path, local_files_only=True, padding_side="right")
            except Exception as e:
                raise lib.X2VError(f"TextEncoderHFLlamaModel.infer: no tokenizer could be loaded from {self.model_path!r} ({e}); pass token ids to infer_ids") from e
        tokens = self._tokenizer(text, return_length=False, return_overflowing_tokens=False, return_attention_mask=True, truncation=True, max_length=self.max_length,
                                 padding="max_length", return_tensors="pt")
        return tokens["input_ids"], tokens["attention_mask"]

    def infer(self, text, config=None):
        """text → (states [1, max_length - crop_start, dim] fp16, mask) (llama/model.py:39-66)."""
        if config is not None and config.get("cpu_offload", False):
            raise NotImplementedError("TextEncoderHFLlamaModel: cpu_offload is not built on the HIP path (the weights live on the device)")
        ids, mask = self._tokenize(self.prompt_template.format(text))
        states, mask = self.infer_ids(ids, mask)
        return states, mask.to(self.device)

    def to_cuda(self):
        pass  # weights live on the device (no cpu_offload on this path)

    def to_cpu(self):
        pass


def encoder_flops(model, lens):
    """Multiply-add FLOP (2 per) of one forward over prompts of these valid lengths, from the shapes (the causal attention counts keys <= query)."""
    M, D, A, Q, F = sum(lens), model.dim, model.dim_attn, model.dim_qkv, model.dim_ffn
    per_block = 2 * M * (D * Q + A * D + 2 * D * F + F * D) + 4 * model.num_heads * model.head_dim * sum(n * (n + 1) // 2 for n in lens)
    return per_block * model.num_layers


def run_text_encoder(encoders, ids_1, mask_1, ids_2, mask_2):
    """HunyuanRunner.run_text_encoder after tokenisation (hunyuan_runner.py:58-67): `encoders` = [Llama tower, CLIP text tower], their ids and masks →
    the dict HunyuanPreInfer consumes, states cast to bf16 as the runner does."""
    out = {}
    for i, (enc, ids, mask) in enumerate(((encoders[0], ids_1, mask_1), (encoders[1], ids_2, mask_2))):
        states, m = enc.infer_ids(ids, mask)
        out[f"text_encoder_{i + 1}_text_states"] = states.to(dtype=torch.bfloat16)
        out[f"text_encoder_{i + 1}_attention_mask"] = m.to(states.device)
    return out


__all__ = ["TextEncoderHFLlamaModel", "run_text_encoder", "encoder_flops", "rope_tables", "interleave_rows", "dims_from_config", "load_hf_dir", "strip_prefix"]
