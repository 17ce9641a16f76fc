"""CLIP ViT-H/14 image tower on the HIP kernels (csrc/clip.hip) — the producer of i2v's `clip_encoder_out`.

reference: lightx2v/models/input_encoders/hf/xlm_roberta/model.py — CLIPModel :411-456 (visual :436-450), VisionTransformer.forward :274-295
(use_31_block=True: all blocks but the last, no post_norm, no head), AttentionBlock :157-164, SelfAttention :75-91, LayerNorm :47-49;
runners/wan/wan_runner.py:52-84 (load_image_encoder), :193-202 (run_image_encoder).

The tower runs in fp16 as the reference does (CLIPModel(dtype=torch.float16)): fp16 activations and Linear weights, fp32 accumulation, fp32
LayerNorm statistics and parameters.  Per image batch it is 2 + 7 x (layers - 1) launches on one stream behind one x2v_clip_preprocess_f16 per
image; every buffer is allocated once per batch size, so `graph = True` can replay the chain as one captured HIP graph (a single chain: no
parallel branches).  Only the visual half of the checkpoint is read; the quantised Linear path (q_linear.py) is not built.
"""
import math

import torch

from . import lib, synth
from .packed import run_plan

HEAD_DIM = 80  # x2v_attn_f16_d80


def _load_state(src):
    if isinstance(src, dict):
        return src
    path = str(src)
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file

        return load_file(path)
    return torch.load(path, map_location="cpu", weights_only=True)


class CLIPModel:
    """Same constructor and `visual` as the reference's CLIPModel; `checkpoint_path` may also be a name → tensor dict."""

    def __init__(self, dtype, device, checkpoint_path, clip_quantized, clip_quantized_ckpt, quant_scheme):
        if clip_quantized:
            raise NotImplementedError("CLIPModel: clip_quantized (the int8 / fp8 Linear classes of q_linear.py) is not built on the HIP path; load the fp16 checkpoint")
        if dtype != torch.float16:
            raise lib.X2VError(f"CLIPModel: the HIP tower is fp16 (the reference's dtype), got {dtype}")
        self.dtype, self.device, self.quantized, self.checkpoint_path = dtype, torch.device(device), False, checkpoint_path
        self.graph = False  # replay the tower as a captured HIP graph (one per batch size)
        self.mean, self.std = list(synth.CLIP_MEAN), list(synth.CLIP_STD)
        sd = {k: v for k, v in _load_state(checkpoint_path).items() if "textual" not in k}  # model.py:428-430
        need = ["visual.patch_embedding.weight", "visual.cls_embedding", "visual.pos_embedding", "visual.pre_norm.weight", "visual.pre_norm.bias"]
        missing = [k for k in need if k not in sd]
        if missing:
            raise lib.X2VError(f"CLIPModel: the checkpoint lacks {missing}")
        pw = sd["visual.patch_embedding.weight"]
        self.dim, self.patch_size = int(pw.shape[0]), int(pw.shape[-1])
        self.tokens = int(sd["visual.pos_embedding"].shape[1])
        grid = math.isqrt(self.tokens - 1)
        if grid * grid != self.tokens - 1 or tuple(pw.shape) != (self.dim, 3, self.patch_size, self.patch_size):
            raise lib.X2VError(f"CLIPModel: pos_embedding {tuple(sd['visual.pos_embedding'].shape)} / patch_embedding {tuple(pw.shape)} are not a class token + square grid")
        if self.dim % HEAD_DIM:
            raise lib.X2VError(f"CLIPModel: dim {self.dim} is not a multiple of the head dim {HEAD_DIM} this tower's attention kernel is written for")
        self.image_size, self.num_heads = grid * self.patch_size, self.dim // HEAD_DIM
        self.num_layers = 1 + max(int(k.split(".")[2]) for k in sd if k.startswith("visual.transformer."))
        self.norm_eps = 1e-5

        def f16(k):
            return sd[k].to(device=self.device, dtype=torch.float16).contiguous()

        def f32(k):
            return sd[k].to(device=self.device, dtype=torch.float32).contiguous()

        kk = 3 * self.patch_size**2
        self.k_pad = (kk + 31) // 32 * 32  # the patch GEMM's K: 588 → 608
        self.w_patch = torch.zeros((self.dim, self.k_pad), dtype=torch.float16, device=self.device)
        self.w_patch[:, :kk] = f16("visual.patch_embedding.weight").reshape(self.dim, kk)
        self.cls, self.pos = f16("visual.cls_embedding").reshape(-1), f16("visual.pos_embedding").reshape(self.tokens, self.dim)
        self.pre_norm = (f32("visual.pre_norm.weight"), f32("visual.pre_norm.bias"))
        self.blocks = []
        for i in range(self.num_layers - 1):  # use_31_block: transformer[:-1]
            p = f"visual.transformer.{i}."
            self.blocks.append(dict(
                n1=(f32(p + "norm1.weight"), f32(p + "norm1.bias")), n2=(f32(p + "norm2.weight"), f32(p + "norm2.bias")),
                qkv=(f16(p + "attn.to_qkv.weight"), f16(p + "attn.to_qkv.bias")), proj=(f16(p + "attn.proj.weight"), f16(p + "attn.proj.bias")),
                fc1=(f16(p + "mlp.0.weight"), f16(p + "mlp.0.bias")), fc2=(f16(p + "mlp.2.weight"), f16(p + "mlp.2.bias"))))
        self.mlp_dim = int(self.blocks[0]["fc1"][0].shape[0]) if self.blocks else 4 * self.dim
        self._ws, self._plans, self._graphs = {}, {}, {}

    # ---- plumbing ------------------------------------------------------------------------------------------------------
    def weight_bytes(self):
        """Bytes of Linear weights one forward streams (the launch floor of the tower)."""
        return self.w_patch.numel() * 2 + sum(b[k][0].numel() * 2 for b in self.blocks for k in ("qkv", "proj", "fc1", "fc2"))

    def _workspace(self, B):
        ws = self._ws.get(B)
        if ws is None:
            M, D = B * self.tokens, self.dim

            def buf(r, c):
                return torch.empty((r, c), dtype=torch.float16, device=self.device)

            ws = self._ws[B] = dict(xa=buf(B * (self.tokens - 1), self.k_pad), patches=buf(B * (self.tokens - 1), D), x=buf(M, D), h=buf(M, D), qkv=buf(M, 3 * D),
                                    att=buf(M, D), f=buf(M, self.mlp_dim))
        return ws

    def _plan(self, B, stream):
        """The tower as a list of (C entry, raw arguments): pointers, strides and the stream are fixed per (batch size, stream)."""
        key = (B, stream)
        plan = self._plans.get(key)
        if plan is not None:
            return plan
        L, ws = lib._lib, self._workspace(B)
        M, D, F, T, eps = B * self.tokens, self.dim, self.mlp_dim, self.tokens, self.norm_eps
        p = {k: v.data_ptr() for k, v in ws.items()}
        plan = [(L.x2v_gemm_f16, (p["xa"], self.k_pad, self.w_patch.data_ptr(), self.k_pad, None, p["patches"], D, B * (T - 1), D, self.k_pad, lib.EPI16_NONE, None, 0, stream)),
                (L.x2v_clip_embed_f16, (p["patches"], D, self.cls.data_ptr(), self.pos.data_ptr(), self.pre_norm[0].data_ptr(), self.pre_norm[1].data_ptr(), p["x"], D, B, T, D, eps,
                                        stream))]

        def gemm(x, w, y, n, k, epi, resid=None):
            plan.append((L.x2v_gemm_f16, (p[x], k, w[0].data_ptr(), k, w[1].data_ptr(), p[y], n, M, n, k, epi, None if resid is None else p[resid], n, stream)))

        for b in self.blocks:
            plan.append((L.x2v_layernorm_f16, (p["x"], D, b["n1"][0].data_ptr(), b["n1"][1].data_ptr(), p["h"], D, M, D, eps, stream)))
            gemm("h", b["qkv"], "qkv", 3 * D, D, lib.EPI16_NONE)
            plan.append((L.x2v_attn_f16_d80, (p["qkv"], 3 * D, p["att"], D, B, T, self.num_heads, 0.0, stream)))
            gemm("att", b["proj"], "x", D, D, lib.EPI16_RESIDUAL, "x")
            plan.append((L.x2v_layernorm_f16, (p["x"], D, b["n2"][0].data_ptr(), b["n2"][1].data_ptr(), p["h"], D, M, D, eps, stream)))
            gemm("h", b["fc1"], "f", F, D, lib.EPI16_GELU_ERF)
            gemm("f", b["fc2"], "x", D, F, lib.EPI16_RESIDUAL, "x")
        self._plans[key] = plan
        return plan

    def _run_plan(self, B):
        run_plan(self._plan(B, lib._stream()))

    def preprocess(self, videos):
        """CLIPModel.visual's resize + normalise (model.py:440-442), written as the patch GEMM's operand: → (B, workspace)."""
        imgs = []
        for u in videos:
            if u.dim() != 4 or u.shape[0] != 3:
                raise lib.X2VError(f"CLIPModel.visual: expected [3, T, H, W] entries, got {tuple(u.shape)}")
            u = u.to(device=self.device, dtype=torch.float32)
            imgs += [u[:, t] if u.stride(3) == 1 else u[:, t].contiguous() for t in range(u.shape[1])]  # u.transpose(0, 1): one image per frame
        if not imgs:
            raise lib.X2VError("CLIPModel.visual: no image")
        lib.init()
        B, n = len(imgs), self.tokens - 1
        ws = self._workspace(B)
        for i, im in enumerate(imgs):
            lib.clip_preprocess(im, ws["xa"][i * n : (i + 1) * n], self.image_size, self.patch_size, self.mean, self.std)
        return B, ws

    def forward_tokens(self, B):
        """Patch embedding → block 30's output on the workspace of batch size B (the operand buffer `xa` is filled): → x [B * tokens, dim] (the workspace)."""
        if not self.graph:
            self._run_plan(B)
            return self._ws[B]["x"]
        g = self._graphs.get(B)
        if g is None:
            self._run_plan(B)  # first touch outside the capture (kernel attributes, lazy module load)
            torch.cuda.synchronize()
            g = self._graphs[B] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._run_plan(B)
        g.replay()
        return self._ws[B]["x"]

    # ---- the reference's interface -------------------------------------------------------------------------------------
    def visual(self, videos, args):
        """videos: list of [3, T, H, W] in [-1, 1] → [sum T, tokens, dim] fp16 (model.py:436-450)."""
        B, _ = self.preprocess(videos)
        return self.forward_tokens(B).view(B, self.tokens, self.dim).clone()

    def to_cuda(self):
        pass  # weights live on the device (no cpu_offload on this path)

    def to_cpu(self):
        pass


def run_image_encoder(model, img, args=None):
    """WanRunner.run_image_encoder after the PIL → tensor step (wan_runner.py:196-197): img [3, H, W] in [-1, 1] → clip_encoder_out [257, dim] bf16."""
    return model.visual([img[:, None, :, :]], args).squeeze(0).to(torch.bfloat16)


def tower_flops(model, B=1):
    """Multiply-add FLOP (2 per) of one forward of B images, from the shapes."""
    M, D, F, T = B * model.tokens, model.dim, model.mlp_dim, model.tokens
    per_block = 2 * M * D * (3 * D + D + 2 * F) + 4 * B * model.num_heads * T * T * HEAD_DIM
    return 2 * B * (T - 1) * D * 3 * model.patch_size**2 + per_block * len(model.blocks)


__all__ = ["CLIPModel", "run_image_encoder", "tower_flops"]
