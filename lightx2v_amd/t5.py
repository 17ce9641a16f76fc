"""umT5-XXL text encoder on the HIP kernels (csrc/t5.hip) — the producer of Wan's `text_encoder_output["context"]` / `["context_null"]`.

reference: lightx2v/models/input_encoders/hf/t5/model.py — T5EncoderModel :515-601 (infer :581-601), T5Encoder.forward :314-347, T5SelfAttention :190-205,
T5Attention :99-136, T5FeedForward :158-170, T5LayerNorm :68-72, T5RelativeEmbedding :255-281, umt5_xxl :498-512; runners/wan/wan_runner.py:178-191
(run_text_encoder).

The encoder runs in bf16 as the reference does: bf16 activations and Linear weights, fp32 accumulation, fp32 norm statistics.  The reference pads every
prompt to text_len tokens, masks the padded keys with the dtype's minimum (probability exactly 0) and returns the valid rows only, so valid rows never depend
on padding: this path runs on the valid tokens alone, all prompts packed into one M = sum(seq_len) pass, the attention kernel keeping each query inside its
own sequence.  Per block 7 launches on one stream — norm, fused q | k | v GEMM, attention with the block's relative-position bias, o GEMM + residual, norm,
fc1 / gate GEMM with the GEGLU epilogue, fc2 GEMM + residual — plus the final norm; one workspace, sized to the largest M seen, serves every pass.  Where it rounds differently from
the reference: scores and score + bias stay fp32 (the reference rounds both to bf16 before its fp32 softmax), the GELU is evaluated in fp32 on the bf16 gate
output (the reference's GELU module rounds every op), the norm rounds once (X2V_ROUND_FP32).  The quantised Linear path (q_linear.py) and cpu_offload are
not built.
"""
import math

import torch

from . import lib
from .packed import MAX_PLANS, PackedTower  # noqa: F401

HEAD_DIM = 64  # x2v_attn_bf16_d64_relbias
MAX_BATCH, MAX_LEN = lib.ATTN_D64_MAX_BATCH, lib.ATTN_D64_MAX_LEN


def relative_position_bucket(rel_pos, num_buckets=32, max_dist=128):
    """T5RelativeEmbedding._relative_position_bucket (model.py:265-281) with bidirectional=True, the same torch expression on the CPU: an fp32 log
    followed by .long() truncation (pinned to the reference by tests/golden/t5_encoder_tiny)."""
    rel_pos = rel_pos.cpu()
    num_buckets = num_buckets // 2
    rel_buckets = (rel_pos > 0).long() * num_buckets
    rel_pos = torch.abs(rel_pos)
    max_exact = num_buckets // 2
    rel_pos_large = max_exact + (torch.log(rel_pos.float() / max_exact) / math.log(max_dist / max_exact) * (num_buckets - max_exact)).long()
    rel_pos_large = torch.min(rel_pos_large, torch.full_like(rel_pos_large, num_buckets - 1))
    rel_buckets += torch.where(rel_pos < max_exact, rel_pos, rel_pos_large)
    return rel_buckets


def bias_table(embedding, max_dist=128):
    """[H, 1023] fp32: entry [h][d + 511] = embedding[bucket(d)][h] for d = key position - query position (T5RelativeEmbedding.forward :255-263)."""
    emb = embedding.detach().float().cpu()
    buckets = relative_position_bucket(torch.arange(-(MAX_LEN - 1), MAX_LEN), emb.shape[0], max_dist)
    return emb[buckets].t().contiguous()


def _load_state(src):
    if isinstance(src, dict):
        return src
    path = str(src)
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file

        return load_file(path)
    return torch.load(path, map_location="cpu", weights_only=True)


class T5EncoderModel(PackedTower):
    """Same constructor keywords, `infer`, `to_cuda` and `to_cpu` as the reference's T5EncoderModel; `checkpoint_path` may also be a name → tensor dict."""

    def __init__(self, text_len, dtype=torch.bfloat16, device="cuda", checkpoint_path=None, tokenizer_path=None, shard_fn=None, cpu_offload=False, offload_granularity="model",
                 t5_quantized=False, t5_quantized_ckpt=None, quant_scheme=None):
        if t5_quantized:
            raise NotImplementedError("T5EncoderModel: t5_quantized (the int8 / fp8 Linear classes of q_linear.py) is not built on the HIP path; load the bf16 checkpoint")
        if dtype != torch.bfloat16:
            raise lib.X2VError(f"T5EncoderModel: the HIP encoder is bf16 (the reference's dtype), got {dtype}")
        if cpu_offload or shard_fn is not None:
            raise NotImplementedError("T5EncoderModel: cpu_offload / shard_fn are not built on the HIP path (the weights live on the device)")
        if not 1 <= int(text_len) <= MAX_LEN:
            raise lib.X2VError(f"T5EncoderModel: text_len {text_len} is outside 1..{MAX_LEN} (the attention kernel's key capacity)")
        self.text_len, self.dtype, self.device = int(text_len), dtype, torch.device(device)
        self.checkpoint_path, self.tokenizer_path, self.offload_granularity, self.cpu_offload = checkpoint_path, tokenizer_path, offload_granularity, False
        sd = _load_state(checkpoint_path)
        need = ["token_embedding.weight", "norm.weight", "blocks.0.attn.q.weight", "blocks.0.ffn.fc1.weight", "blocks.0.pos_embedding.embedding.weight"]
        missing = [k for k in need if k not in sd]
        if missing:
            raise lib.X2VError(f"T5EncoderModel: the checkpoint lacks {missing} (an encoder with per-block position tables, shared_pos=False)")
        self.vocab, self.dim = (int(s) for s in sd["token_embedding.weight"].shape)
        self.dim_attn, self.dim_ffn = int(sd["blocks.0.attn.q.weight"].shape[0]), int(sd["blocks.0.ffn.fc1.weight"].shape[0])
        self.num_buckets, self.num_heads = (int(s) for s in sd["blocks.0.pos_embedding.embedding.weight"].shape)
        if self.dim_attn != self.num_heads * HEAD_DIM:
            raise lib.X2VError(f"T5EncoderModel: dim_attn {self.dim_attn} / {self.num_heads} heads is not the head dim {HEAD_DIM} this encoder's attention kernel is written for")
        if self.dim % 32 or self.dim_ffn % 32:
            raise lib.X2VError(f"T5EncoderModel: dim {self.dim} and dim_ffn {self.dim_ffn} must be multiples of 32 (the GEMM's k-step)")
        self.num_layers = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
        self.norm_eps = 1e-6

        def w(k):
            return sd[k].to(device=self.device, dtype=torch.bfloat16).contiguous()

        self.embedding, self.norm = w("token_embedding.weight"), w("norm.weight")
        self.blocks = []
        for i in range(self.num_layers):
            p = f"blocks.{i}."
            fc1, gate = w(p + "ffn.fc1.weight"), w(p + "ffn.gate.0.weight")
            self.blocks.append(dict(
                n1=w(p + "norm1.weight"), n2=w(p + "norm2.weight"),
                qkv=torch.cat([w(p + "attn.q.weight"), w(p + "attn.k.weight"), w(p + "attn.v.weight")]).contiguous(), o=w(p + "attn.o.weight"),
                geglu=torch.stack([fc1, gate], dim=1).reshape(2 * self.dim_ffn, self.dim).contiguous(),  # row 2n = fc1 row n, row 2n + 1 = gate.0 row n
                fc2=w(p + "ffn.fc2.weight"), bias=bias_table(sd[p + "pos_embedding.embedding.weight"]).to(self.device)))
        self._init_plumbing()

    # ---- plumbing (packed.PackedTower: one workspace, the plan cache) --------------------------------------------------
    DTYPE = torch.bfloat16

    def weight_bytes(self):
        """Bytes of Linear weights one forward streams (the launch floor of the encoder)."""
        return sum(b[k].numel() * 2 for b in self.blocks for k in ("qkv", "o", "geglu", "fc2"))

    def _buffers(self):
        return dict(x=self.dim, h=self.dim, qkv=3 * self.dim_attn, att=self.dim_attn, f=self.dim_ffn, out=self.dim)

    def _launches(self, p, M, cu_arr, batch, stream):
        L, D, A, F, eps = lib._lib, self.dim, self.dim_attn, self.dim_ffn, self.norm_eps
        plan = []

        def norm(x, wt, y):
            plan.append((L.x2v_rmsnorm_bf16, (p[x], D, wt.data_ptr(), p[y], D, M, D, eps, lib.ROUND_FP32, stream)))

        def gemm(x, wt, y, n, k, epi, resid=None):
            plan.append((L.x2v_gemm_rows_bf16, (p[x], k, wt.data_ptr(), k, p[y], n, M, n, k, epi, None if resid is None else p[resid], 0 if resid is None else n, stream)))

        for b in self.blocks:
            norm("x", b["n1"], "h")
            gemm("h", b["qkv"], "qkv", 3 * A, D, lib.EPIR_NONE)
            plan.append((L.x2v_attn_bf16_d64_relbias, (p["qkv"], 3 * A, b["bias"].data_ptr(), p["att"], A, cu_arr, batch, self.num_heads, 1.0, stream)))
            gemm("att", b["o"], "x", D, A, lib.EPIR_RESIDUAL, "x")
            norm("x", b["n2"], "h")
            gemm("h", b["geglu"], "f", F, D, lib.EPIR_GEGLU)
            gemm("f", b["fc2"], "x", D, F, lib.EPIR_RESIDUAL, "x")
        norm("x", self.norm, "out")
        return plan

    def forward_packed(self, lens):
        """Blocks + final norm on the workspace of these lengths (`x` holds the packed token embeddings): → out [sum(lens), dim] (the workspace)."""
        M = self._run_packed(lens)
        return self._bufs["out"][:M]

    # ---- the reference's interface -------------------------------------------------------------------------------------
    def infer_ids(self, ids, mask):
        """ids, mask [B, L] (L <= 512, B <= 8; the mask marks a prefix of each row, as the tokenizer's padding does) → list of [seq_len_b, dim] bf16
        device tensors: what T5EncoderModel.infer returns for these ids (model.py:588-601)."""
        if ids.dim() != 2 or tuple(mask.shape) != tuple(ids.shape):
            raise lib.X2VError(f"T5EncoderModel.infer_ids: ids {tuple(ids.shape)} and mask {tuple(mask.shape)} must both be [B, L]")
        B, Lp = ids.shape
        if not 1 <= B <= MAX_BATCH or not 1 <= Lp <= MAX_LEN:
            raise lib.X2VError(f"T5EncoderModel.infer_ids: [B, L] = {(B, Lp)}; one pass takes at most {MAX_BATCH} prompts of at most {MAX_LEN} tokens")
        valid = mask.gt(0).cpu()
        lens = [int(n) for n in valid.sum(dim=1)]
        if min(lens) < 1:
            raise lib.X2VError(f"T5EncoderModel.infer_ids: prompt {lens.index(min(lens))} has no valid token (the tokenizer always emits </s>)")
        if any(not bool(valid[b, :n].all()) for b, n in enumerate(lens)):
            raise lib.X2VError("T5EncoderModel.infer_ids: the mask must mark a prefix of each row (infer returns the first seq_len rows, model.py:601)")
        ids = ids.cpu()
        if int(ids.min()) < 0 or int(ids.max()) >= self.vocab:
            raise lib.X2VError(f"T5EncoderModel.infer_ids: token ids outside the vocabulary of {self.vocab}")
        lib.init()
        packed = torch.cat([ids[b, :n] for b, n in enumerate(lens)]).to(device=self.device, dtype=torch.long)
        torch.index_select(self.embedding, 0, packed, out=self._workspace(sum(lens))["x"])  # token_embedding(ids): a gather (plumbing)
        out = self.forward_packed(lens)
        return [u.clone() for u in out.split(lens)]

    def _tokenize(self, texts):
        if self._tokenizer is None:
            try:
                import ftfy  # noqa: F401
            except ImportError as e:
                raise lib.X2VError("T5EncoderModel.infer: the `ftfy` package (the reference tokenizer's basic_clean) is not installed; pass token ids to infer_ids") from e
            try:
                from transformers import AutoTokenizer

                self._tokenizer = AutoTokenizer.from_pretrained(self.tokenizer_path, local_files_only=True)
            except Exception as e:
                raise lib.X2VError(f"T5EncoderModel.infer: no tokenizer could be loaded from tokenizer_path={self.tokenizer_path!r} ({e}); pass token ids to infer_ids") from e
        import html
        import re

        import ftfy

        def clean(t):  # clean="whitespace" (tokenizer.py:12-21,74-76)
            t = html.unescape(html.unescape(ftfy.fix_text(t))).strip()
            return re.sub(r"\s+", " ", t).strip()

        enc = self._tokenizer([clean(t) for t in ([texts] if isinstance(texts, str) else texts)], return_tensors="pt", padding="max_length", truncation=True,
                              max_length=self.text_len, add_special_tokens=True)
        return enc.input_ids, enc.attention_mask

    def infer(self, texts):
        """texts → list of [seq_len, dim] bf16 (model.py:581-601)."""
        return self.infer_ids(*self._tokenize(texts))

    def to_cuda(self):
        pass  # weights live on the device (no cpu_offload on this path)

    def to_cpu(self):
        pass


def run_text_encoder(model, ids, mask, ids_null, mask_null):
    """WanRunner.run_text_encoder after tokenisation (wan_runner.py:178-191): the prompt's and the negative prompt's [B, L] ids and masks →
    {"context": [...], "context_null": [...]} from ONE packed pass (the reference runs the encoder twice)."""
    if ids.dim() != 2 or ids_null.dim() != 2:
        raise lib.X2VError("run_text_encoder: ids and ids_null must be [B, L]")
    Lp = max(ids.shape[1], ids_null.shape[1])

    def pad(t):
        return torch.nn.functional.pad(t.cpu(), (0, Lp - t.shape[1]))

    out = model.infer_ids(torch.cat([pad(ids), pad(ids_null)]), torch.cat([pad(mask), pad(mask_null)]))
    return {"context": out[: ids.shape[0]], "context_null": out[ids.shape[0] :]}


def encoder_flops(model, lens):
    """Multiply-add FLOP (2 per) of one packed forward over prompts of these lengths, from the shapes."""
    M, D, A, F = sum(lens), model.dim, model.dim_attn, model.dim_ffn
    per_block = 2 * M * (D * 3 * A + A * D + 2 * D * F + F * D) + 4 * model.num_heads * HEAD_DIM * sum(n * n for n in lens)
    return per_block * model.num_layers


__all__ = ["T5EncoderModel", "run_text_encoder", "encoder_flops", "relative_position_bucket", "bias_table"]
