"""HunyuanVideo's CLIP-L text tower on the HIP kernels (csrc/txt_enc.hip, csrc/clip.hip) — the producer of `text_encoder_output["text_encoder_2_text_states"]`.

reference: lightx2v/models/input_encoders/hf/clip/model.py — TextEncoderHFClipModel (init :12-13, infer :27-50), which runs transformers' CLIPTextModel in
fp16 on the prompt padded to 77 tokens and returns pooler_output [1, dim] with the uncropped mask; runners/hunyuan/hunyuan_runner.py:30-37,58-67.

pooler_output is final_layer_norm(x)[p], p the end token's position (eos_position).  The attention is causal, so rows <= p never see what follows them:
this path runs the first p + 1 tokens only, and the final norm on row p alone.  Per layer 7 launches — LayerNorm, fused q | k | v GEMM (+ bias), causal
head-dim-64 attention, out_proj GEMM + bias + residual, LayerNorm, fc1 GEMM + bias + quick-GELU, fc2 GEMM + bias + residual — plus the final norm; the
token + position add is torch glue.  fp16 activations and weights, fp32 accumulation, statistics and LayerNorm parameters.  Where it rounds differently from
the reference's fp16 model: q is not scaled before the product (the softmax scale is applied to the fp32 scores), scores and probabilities stay fp32 up to
the PV operand, the quick-GELU is evaluated in fp32 on the fp32 accumulator + bias and rounded once.  cpu_offload is not built.
"""
import torch

from . import lib
from .llama import load_hf_dir, strip_prefix
from .packed import MAX_PLANS, PackedTower  # noqa: F401

HEAD_DIM = 64


def eos_position(ids, eos_token_id):
    """The pooled position of each row of ids [B, L] → [B] (CLIPTextModel.forward): with the legacy eos_token_id == 2 the first position of the row's
    largest id, otherwise the first position holding eos_token_id (0 where the row has none: the argmax of an all-zero row)."""
    ids = ids.cpu().to(torch.int)
    if eos_token_id == 2:
        return ids.argmax(dim=-1)
    return (ids == eos_token_id).int().argmax(dim=-1)


def dims_from_config(cfg):
    """The dims dict (synth.CLIP_TEXT_DIMS keys) of a transformers CLIPTextModel config.json (a full CLIP config carries it under text_config)."""
    cfg = cfg.get("text_config") or cfg
    if cfg.get("hidden_act", "quick_gelu") != "quick_gelu":
        raise lib.X2VError(f"TextEncoderHFClipModel: hidden_act {cfg.get('hidden_act')!r}; the GEMM epilogue is quick_gelu")
    heads = int(cfg["num_attention_heads"])
    return dict(vocab=int(cfg["vocab_size"]), dim=int(cfg["hidden_size"]), heads=heads, head_dim=int(cfg["hidden_size"]) // heads, ffn=int(cfg["intermediate_size"]),
                layers=int(cfg["num_hidden_layers"]), positions=int(cfg.get("max_position_embeddings", 77)), eps=float(cfg.get("layer_norm_eps", 1e-5)),
                eos_token_id=int(cfg.get("eos_token_id", 2)))


class TextEncoderHFClipModel(PackedTower):
    """Same constructor, attributes, `infer`, `to_cuda` and `to_cpu` as the reference's TextEncoderHFClipModel; `model_path` may also be a
    (name → tensor dict, dims dict) pair (dims: the keys of synth.CLIP_TEXT_DIMS)."""

    def __init__(self, model_path, device):
        self.device, self.model_path = torch.device(device), model_path
        self.init()
        if isinstance(model_path, (tuple, list)):
            sd, dims = model_path[0], dict(model_path[1])
        else:
            sd, cfg = load_hf_dir(str(model_path))
            dims = dims_from_config(cfg)
        self.load(strip_prefix(sd, "text_model.", "embeddings.token_embedding.weight"), dims)

    def init(self):
        self.max_length = 77

    def load(self, sd, dims):
        who = "TextEncoderHFClipModel"
        self.dims = dims
        self.vocab, self.dim, self.num_heads, self.dim_ffn, self.num_layers, self.positions = (int(dims[k]) for k in ("vocab", "dim", "heads", "ffn", "layers", "positions"))
        self.norm_eps, self.eos_token_id = float(dims["eps"]), int(dims["eos_token_id"])
        if int(dims["head_dim"]) != HEAD_DIM or self.dim != self.num_heads * HEAD_DIM:
            raise lib.X2VError(f"{who}: dim {self.dim} / {self.num_heads} heads is not the head dim {HEAD_DIM} this tower's attention kernel is instantiated for")
        if self.dim % 32 or self.dim_ffn % 32 or self.dim > 2048:
            raise lib.X2VError(f"{who}: dim {self.dim} and ffn {self.dim_ffn} must be multiples of 32 (the GEMM's k-step), dim at most 2048 (the LayerNorm kernel)")
        D, F = self.dim, self.dim_ffn

        def w(k, shape, dtype=torch.float16):
            if k not in sd:
                raise lib.X2VError(f"{who}: the checkpoint lacks {k}")
            if tuple(sd[k].shape) != shape:
                raise lib.X2VError(f"{who}: {k} is {tuple(sd[k].shape)} but the config gives {shape}")
            return sd[k].to(device=self.device, dtype=dtype).contiguous()

        def ln(k):
            return w(k + ".weight", (D,), torch.float32), w(k + ".bias", (D,), torch.float32)

        self.token_embedding, self.position_embedding = w("embeddings.token_embedding.weight", (self.vocab, D)), w("embeddings.position_embedding.weight", (self.positions, D))
        self.blocks = []
        for i in range(self.num_layers):
            p = f"encoder.layers.{i}."
            a = p + "self_attn."
            self.blocks.append(dict(
                ln1=ln(p + "layer_norm1"), ln2=ln(p + "layer_norm2"),
                qkv=torch.cat([w(a + n + ".weight", (D, D)) for n in ("q_proj", "k_proj", "v_proj")]).contiguous(),
                qkv_b=torch.cat([w(a + n + ".bias", (D,)) for n in ("q_proj", "k_proj", "v_proj")]).contiguous(),
                o=w(a + "out_proj.weight", (D, D)), o_b=w(a + "out_proj.bias", (D,)),
                fc1=w(p + "mlp.fc1.weight", (F, D)), fc1_b=w(p + "mlp.fc1.bias", (F,)), fc2=w(p + "mlp.fc2.weight", (D, F)), fc2_b=w(p + "mlp.fc2.bias", (D,))))
        self.final_ln = ln("final_layer_norm")
        self._init_plumbing()

    # ---- plumbing (packed.PackedTower: one workspace, the plan cache) --------------------------------------------------
    def weight_bytes(self):
        """Bytes of Linear weights one forward streams (the launch floor of the tower)."""
        return sum(b[k].numel() * 2 for b in self.blocks for k in ("qkv", "o", "fc1", "fc2"))

    def launches(self):
        return 7 * self.num_layers + 1

    def _buffers(self):
        return dict(x=self.dim, h=self.dim, qkv=3 * self.dim, att=self.dim, f=self.dim_ffn, pooled=(self.dim, 1))

    def _launches(self, p, M, cu_arr, batch, stream):
        """The final norm reads the last row of the single sequence."""
        L, D, F, eps = lib._lib, self.dim, self.dim_ffn, self.norm_eps
        plan = []

        def norm(wb):
            plan.append((L.x2v_layernorm_f16, (p["x"], D, wb[0].data_ptr(), wb[1].data_ptr(), p["h"], D, M, D, eps, stream)))

        def gemm(x, wt, bias, y, n, k, epi, resid=None):
            plan.append((L.x2v_gemm_f16, (p[x], k, wt.data_ptr(), k, bias.data_ptr(), p[y], n, M, n, k, epi, None if resid is None else p[resid], 0 if resid is None else n, stream)))

        for b in self.blocks:
            norm(b["ln1"])
            gemm("h", b["qkv"], b["qkv_b"], "qkv", 3 * D, D, lib.EPI16_NONE)
            plan.append((L.x2v_attn_f16_causal, (p["qkv"], 3 * D, p["att"], D, cu_arr, batch, self.num_heads, self.num_heads, HEAD_DIM, None, None, 0.0, stream)))
            gemm("att", b["o"], b["o_b"], "x", D, D, lib.EPI16_RESIDUAL, "x")
            norm(b["ln2"])
            gemm("h", b["fc1"], b["fc1_b"], "f", F, D, lib.EPI16_QUICK_GELU)
            gemm("f", b["fc2"], b["fc2_b"], "x", D, F, lib.EPI16_RESIDUAL, "x")
        plan.append((L.x2v_layernorm_f16, (p["x"] + (M - 1) * D * 2, D, self.final_ln[0].data_ptr(), self.final_ln[1].data_ptr(), p["pooled"], D, 1, D, eps, stream)))
        return plan

    def forward_packed(self, lens):
        """Layers + the final norm of the last row on the workspace (`x` holds token + position embeddings of one sequence): → pooled [1, dim] (the workspace)."""
        self._run_packed(lens)
        return self._bufs["pooled"]

    # ---- the reference's interface -------------------------------------------------------------------------------------
    def _pooled_position(self, ids, mask):
        who = "TextEncoderHFClipModel.infer_ids"
        if ids.dim() != 2 or ids.shape[0] != 1 or tuple(mask.shape) != tuple(ids.shape):
            raise lib.X2VError(f"{who}: ids {tuple(ids.shape)} and mask {tuple(mask.shape)} must both be [1, L]")
        if not 1 <= ids.shape[1] <= self.positions:
            raise lib.X2VError(f"{who}: L = {ids.shape[1]}; the tower has {self.positions} positions")
        idc = ids.cpu()
        if int(idc.min()) < 0 or int(idc.max()) >= self.vocab:
            raise lib.X2VError(f"{who}: token ids outside the vocabulary of {self.vocab}")
        p = int(eos_position(idc, self.eos_token_id)[0])
        valid = mask.gt(0).cpu()[0]
        n = int(valid.sum())
        if not bool(valid[:n].all()) or n < p + 1:
            raise lib.X2VError(f"{who}: the mask must mark a prefix of the row that reaches the end token at position {p} (padding_side=\"right\", clip/model.py:17)")
        return p

    def infer_ids(self, ids, mask):
        """ids, mask [1, L <= 77] → (pooler_output [1, dim] fp16, mask): what TextEncoderHFClipModel.infer returns for these ids (clip/model.py:41-50)."""
        p = self._pooled_position(ids, mask)
        lib.init()
        tok = ids[0, : p + 1].to(device=self.device, dtype=torch.long)
        ws = self._workspace(p + 1)
        torch.add(self.token_embedding[tok], self.position_embedding[: p + 1], out=ws["x"])  # CLIPTextEmbeddings.forward: the fp16 add (glue)
        return self.forward_packed((p + 1,)).clone(), mask

    def _tokenize(self, text):
        if self._tokenizer is None:
            try:
                from transformers import AutoTokenizer

                self._tokenizer = AutoTokenizer.from_pretrained(self.model_path, local_files_only=True, padding_side="right")
            except Exception as e:
                raise lib.X2VError(f"TextEncoderHFClipModel.infer: no tokenizer could be loaded from {self.model_path!r} ({e}); pass token ids to infer_ids") from e
        tokens = self._tokenizer(text, return_length=False, return_overflowing_tokens=False, return_attention_mask=True, truncation=True, max_length=self.max_length,
                                 padding="max_length", return_tensors="pt")
        return tokens["input_ids"], tokens["attention_mask"]

    def infer(self, text, config=None):
        """text → (pooler_output [1, dim] fp16, mask) (clip/model.py:27-50)."""
        if config is not None and config.get("cpu_offload", False):
            raise NotImplementedError("TextEncoderHFClipModel: cpu_offload is not built on the HIP path (the weights live on the device)")
        pooled, mask = self.infer_ids(*self._tokenize(text))
        return pooled, mask.to(self.device)

    def to_cuda(self):
        pass  # weights live on the device (no cpu_offload on this path)

    def to_cpu(self):
        pass


def encoder_flops(model, lens):
    """Multiply-add FLOP (2 per) of one forward over these run lengths (p + 1 tokens each), from the shapes."""
    M, D, F = sum(lens), model.dim, model.dim_ffn
    per_block = 2 * M * (4 * D * D + 2 * D * F) + 4 * D * sum(n * (n + 1) // 2 for n in lens)
    return per_block * model.num_layers


__all__ = ["TextEncoderHFClipModel", "eos_position", "encoder_flops", "dims_from_config"]
