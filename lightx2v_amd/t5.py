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
output (the reference's GELU module rounds every op), the norm rounds once (X2V_ROUND_FP32).  cpu_offload is not built.

The quantised encoder (t5_quantized=True with t5_quantized_ckpt and quant_scheme "int8" | "fp8"; the reference's QuantLinearInt8 / QuantLinearFp8,
models/input_encoders/hf/q_linear.py, chosen by t5/model.py:84-96, 145-155, 533-534) loads `<name>.weight` as [N, K] int8 / float8_e4m3fn codes with
`<name>.weight_scale` [N, 1] fp32 and runs 9 launches per block: norm + per-token quantiser in one kernel (x2v_rmsnorm_quant_*; q, k and v read the one
quantised h, which is what three QuantLinears make of the same input), q | k | v GEMM on the codes (x2v_gemm_rows_w8a8), attention, quantiser, o GEMM +
residual, norm + quantiser, fc1 / gate GEMM with GEGLU, quantiser, fc2 GEMM + residual.  Embedding, norms and position tables stay bf16.
`quantize_state_dict` makes that layout from a bf16 checkpoint.  On-the-fly quantisation inside the constructor is not built.
"""
import math

import torch

from . import checkpoint, lib
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


QUANT_SCHEMES = {"int8": torch.int8, "fp8": torch.float8_e4m3fn}


def _scheme_dtype(scheme, who):
    if scheme not in QUANT_SCHEMES:
        raise lib.X2VError(f"{who}: unknown quant_scheme {scheme!r} (the reference's t5_quant_scheme is one of {sorted(QUANT_SCHEMES)})")
    return QUANT_SCHEMES[scheme]


def quantize_state_dict(sd, scheme):
    """A bf16 encoder state dict → the reference's quantised layout (tools/convert/converter.py with model_type wan_t5): every Linear of attn / ffn as
    `<name>.weight` [N, K] int8 or float8_e4m3fn with `<name>.weight_scale` [N, 1] fp32 — per output channel max(amax, 1e-5) / qmax, round to nearest, clamp
    (checkpoint.quantize_tensor, the routine tools/convert_ckpt.py runs) — and everything else bf16.  Returns a new dict."""
    dtype = _scheme_dtype(scheme, "quantize_state_dict")
    sel = checkpoint.MODEL_TYPE_KEYS["wan_t5"]
    out = {}
    for k, v in sd.items():
        parts = k.split(".")
        if v.dim() == 2 and len(parts) > sel["key_idx"] and parts[sel["key_idx"]] in sel["target_keys"]:  # converter.py's rule for which tensors are Linears
            out[k], out[k + "_scale"] = checkpoint.quantize_tensor(v.float(), dtype)
        else:
            out[k] = v.to(torch.bfloat16)
    return out


class T5EncoderModel(PackedTower):
    """Same constructor keywords, `infer`, `to_cuda` and `to_cpu` as the reference's T5EncoderModel; `checkpoint_path` may also be a name → tensor dict."""

    def __init__(self, text_len, dtype=torch.bfloat16, device="cuda", checkpoint_path=None, tokenizer_path=None, shard_fn=None, cpu_offload=False, offload_granularity="model",
                 t5_quantized=False, t5_quantized_ckpt=None, quant_scheme=None):
        self.quantized = bool(t5_quantized) and t5_quantized_ckpt is not None  # the reference's rule (model.py:533-534)
        if t5_quantized and not self.quantized:
            raise NotImplementedError("T5EncoderModel: t5_quantized without t5_quantized_ckpt: on-the-fly quantisation of a bf16 checkpoint is not built on the HIP path; "
                                      "pass t5_quantized_ckpt (quantize_state_dict makes one)")
        self.quant_scheme = quant_scheme if self.quantized else None
        self.code_dtype = _scheme_dtype(quant_scheme, "T5EncoderModel") if self.quantized else None
        if dtype != torch.bfloat16:
            raise lib.X2VError(f"T5EncoderModel: the HIP encoder is bf16 (the reference's dtype), got {dtype}")
        if cpu_offload or shard_fn is not None:
            raise NotImplementedError("T5EncoderModel: cpu_offload / shard_fn are not built on the HIP path (the weights live on the device)")
        if not 1 <= int(text_len) <= MAX_LEN:
            raise lib.X2VError(f"T5EncoderModel: text_len {text_len} is outside 1..{MAX_LEN} (the attention kernel's key capacity)")
        self.text_len, self.dtype, self.device = int(text_len), dtype, torch.device(device)
        self.checkpoint_path, self.tokenizer_path, self.offload_granularity, self.cpu_offload = checkpoint_path, tokenizer_path, offload_granularity, False
        sd = _load_state(t5_quantized_ckpt if self.quantized else checkpoint_path)
        need = ["token_embedding.weight", "norm.weight", "blocks.0.attn.q.weight", "blocks.0.ffn.fc1.weight", "blocks.0.pos_embedding.embedding.weight"]
        missing = [k for k in need if k not in sd]
        if missing:
            raise lib.X2VError(f"T5EncoderModel: the checkpoint lacks {missing} (an encoder with per-block position tables, shared_pos=False)")
        self.vocab, self.dim = (int(s) for s in sd["token_embedding.weight"].shape)
        self.dim_attn, self.dim_ffn = int(sd["blocks.0.attn.q.weight"].shape[0]), int(sd["blocks.0.ffn.fc1.weight"].shape[0])
        self.num_buckets, self.num_heads = (int(s) for s in sd["blocks.0.pos_embedding.embedding.weight"].shape)
        if self.dim_attn != self.num_heads * HEAD_DIM:
            raise lib.X2VError(f"T5EncoderModel: dim_attn {self.dim_attn} / {self.num_heads} heads is not the head dim {HEAD_DIM} this encoder's attention kernel is written for")
        kstep = {None: 32, torch.int8: 64, torch.float8_e4m3fn: 128}[self.code_dtype]
        if self.dim % kstep or self.dim_ffn % kstep:
            raise lib.X2VError(f"T5EncoderModel: dim {self.dim} and dim_ffn {self.dim_ffn} must be multiples of {kstep} (the GEMM's k-step)")
        self.num_layers = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
        self.norm_eps = 1e-6

        def w(k):
            return sd[k].to(device=self.device, dtype=torch.bfloat16).contiguous()

        def lin(k):
            """One Linear → [(weight [N, K], scales [N] fp32 or None)]: bf16, or the codes with their per-channel scales."""
            if not self.quantized:
                return w(k + ".weight"), None
            wq, sc = sd[k + ".weight"], sd.get(k + ".weight_scale")
            if wq.dtype != self.code_dtype:
                raise lib.X2VError(f"T5EncoderModel: {k}.weight is {wq.dtype}, but quant_scheme {self.quant_scheme!r} reads {self.code_dtype}")
            if sc is None or sc.numel() != wq.shape[0]:
                raise lib.X2VError(f"T5EncoderModel: the quantised checkpoint lacks {k}.weight_scale [{wq.shape[0]}, 1]")
            return wq.to(self.device).contiguous(), sc.to(device=self.device, dtype=torch.float32).reshape(-1).contiguous()

        def fuse(parts, interleave=False):
            """Rows of several Linears as one weight, their scales alongside: one after the other (q | k | v), or row by row (fc1 / gate.0)."""
            ws, ss = zip(*parts)
            if interleave:
                return torch.stack(ws, dim=1).flatten(0, 1).contiguous(), None if ss[0] is None else torch.stack(ss, dim=1).flatten().contiguous()
            return torch.cat(ws).contiguous(), None if ss[0] is None else torch.cat(ss).contiguous()

        self.embedding, self.norm = w("token_embedding.weight"), w("norm.weight")
        self.blocks = []
        for i in range(self.num_layers):
            p = f"blocks.{i}."
            (qkv, qkv_s), (o, o_s) = fuse([lin(p + "attn.q"), lin(p + "attn.k"), lin(p + "attn.v")]), lin(p + "attn.o")
            (geglu, geglu_s), (fc2, fc2_s) = fuse([lin(p + "ffn.fc1"), lin(p + "ffn.gate.0")], interleave=True), lin(p + "ffn.fc2")  # row 2n = fc1 row n, row 2n + 1 = gate.0 row n
            self.blocks.append(dict(n1=w(p + "norm1.weight"), n2=w(p + "norm2.weight"), qkv=qkv, o=o, geglu=geglu, fc2=fc2, qkv_s=qkv_s, o_s=o_s, geglu_s=geglu_s, fc2_s=fc2_s,
                                    bias=bias_table(sd[p + "pos_embedding.embedding.weight"]).to(self.device)))
        self._init_plumbing()

    # ---- plumbing (packed.PackedTower: one workspace, the plan cache) --------------------------------------------------
    DTYPE = torch.bfloat16

    def weight_bytes(self):
        """Bytes of Linear weights one forward streams (the launch floor of the encoder)."""
        return sum(b[k].numel() * b[k].element_size() for b in self.blocks for k in ("qkv", "o", "geglu", "fc2"))

    def _buffers(self):
        if self.quantized:  # no bf16 h: the norm writes codes.  One code buffer and one scale column serve the three quantised activations in turn
            return dict(x=self.dim, qkv=3 * self.dim_attn, att=self.dim_attn, f=self.dim_ffn, out=self.dim, codes=(max(self.dim, self.dim_attn, self.dim_ffn), None, torch.uint8),
                        sx=(1, None, torch.float32))
        return dict(x=self.dim, h=self.dim, qkv=3 * self.dim_attn, att=self.dim_attn, f=self.dim_ffn, out=self.dim)

    def _launches_quantized(self, p, M, cu_arr, batch, stream):
        L, D, A, F, eps = lib._lib, self.dim, self.dim_attn, self.dim_ffn, self.norm_eps
        i8 = self.code_dtype == torch.int8
        kind = lib.W8A8_INT8 if i8 else lib.W8A8_E4M3
        norm_quant, quant = (L.x2v_rmsnorm_quant_int8, L.x2v_quant_int8_rowwise) if i8 else (L.x2v_rmsnorm_quant_fp8, L.x2v_quant_fp8_rowwise)
        codes, sx = p["codes"], p["sx"]
        plan = []

        def gemm(b, name, y, n, k, epi, resid=None):  # on the codes of the launch in front (rows of k bytes)
            plan.append((L.x2v_gemm_rows_w8a8, (codes, k, sx, b[name].data_ptr(), k, b[name + "_s"].data_ptr(), p[y], n, M, n, k, kind, epi, None if resid is None else p[resid],
                                                0 if resid is None else n, stream)))

        for b in self.blocks:
            plan.append((norm_quant, (p["x"], D, b["n1"].data_ptr(), codes, D, sx, M, D, eps, stream)))
            gemm(b, "qkv", "qkv", 3 * A, D, lib.EPIR_NONE)
            plan.append((L.x2v_attn_bf16_d64_relbias, (p["qkv"], 3 * A, b["bias"].data_ptr(), p["att"], A, cu_arr, batch, self.num_heads, 1.0, stream)))
            plan.append((quant, (p["att"], A, codes, A, sx, M, A, stream)))
            gemm(b, "o", "x", D, A, lib.EPIR_RESIDUAL, "x")
            plan.append((norm_quant, (p["x"], D, b["n2"].data_ptr(), codes, D, sx, M, D, eps, stream)))
            gemm(b, "geglu", "f", F, D, lib.EPIR_GEGLU)
            plan.append((quant, (p["f"], F, codes, F, sx, M, F, stream)))
            gemm(b, "fc2", "x", D, F, lib.EPIR_RESIDUAL, "x")
        plan.append((L.x2v_rmsnorm_bf16, (p["x"], D, self.norm.data_ptr(), p["out"], D, M, D, eps, lib.ROUND_FP32, stream)))
        return plan

    def _launches(self, p, M, cu_arr, batch, stream):
        if self.quantized:
            return self._launches_quantized(p, M, cu_arr, batch, stream)
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


__all__ = ["T5EncoderModel", "run_text_encoder", "encoder_flops", "relative_position_bucket", "bias_table", "quantize_state_dict", "QUANT_SCHEMES"]
