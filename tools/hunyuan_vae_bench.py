#!/usr/bin/env python
"""Times the HunyuanVideo VAE decode (HIP path) on one full-size tile and, with --full, on the whole 720p x 129-frame latent.
    python tools/hunyuan_vae_bench.py [--full] [--fp32] [--attn16]      (default: fp16 convolution operands, the reference's precision)
--attn16: the mid-block attention as the fused fp16 kernel.  --attn-only: times that attention alone on one full latent tile (17 x 32 x 32 tokens of
width 512), fp32-score path and fused path alternating in one process (A-B-A-B, device events, median of 7)."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lightx2v_amd import hunyuan_vae, lib, synth  # noqa: E402


def attn_only(cfg):
    sd = synth.synth_hunyuan_vae_weights(cfg, seed=0)
    decs = {a: hunyuan_vae.DecoderCausal3D(sd, cfg, "cuda", attn16=a) for a in (False, True)}
    t, h, w, c = 17, 32, 32, cfg["block_out_channels"][-1]
    x = torch.randn(t, h, w, c, generator=torch.Generator().manual_seed(1)).cuda()
    p = "decoder.mid_block.attentions.0."
    outs = {a: d.mid_attention(p, x) for a, d in decs.items()}  # warm-up, and the two paths' outputs on the same input
    ms = {False: [], True: []}
    for _ in range(7):
        for a in (False, True):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            decs[a].mid_attention(p, x)
            e1.record()
            e1.synchronize()
            ms[a].append(e0.elapsed_time(e1))
    med = {a: sorted(v)[3] for a, v in ms.items()}
    n, hw = t * h * w, h * w
    blocks = sum(-(-min(n, ((min(64 * b + 63, n - 1)) // hw + 1) * hw) // 64) for b in range(-(-n // 64)))  # 64 x 64 blocks the fused kernel walks
    flop = 4.0 * 64 * 64 * c * blocks
    d = (outs[True] - outs[False]).abs().max().item()
    print(json.dumps({"workload": f"hunyuan_vae mid_attention x[{t},{h},{w},{c}] ({n} tokens)", "ms_fp32_scores": med[False], "ms_fused_fp16": med[True],
                      "all_ms_fp32_scores": ms[False], "all_ms_fused_fp16": ms[True], "attended_blocks_64x64": blocks, "attended_tflop": flop / 1e12,
                      "fused_tflops_per_s_whole_method": flop / med[True] / 1e9, "max_abs_diff_between_paths": d}))


def main():
    full = "--full" in sys.argv
    lib.init(0)
    cfg = synth.HUNYUAN_VAE_CFG
    if "--attn-only" in sys.argv:
        return attn_only(cfg)
    conv16 = "--fp32" not in sys.argv
    attn16 = "--attn16" in sys.argv
    m = hunyuan_vae.VideoEncoderKLCausal3DModel(synth.synth_hunyuan_vae_weights(cfg, seed=0), cfg, conv16=conv16, attn16=attn16)
    shape = (1, 16, 33, 90, 160) if full else (1, 16, 17, 32, 32)
    z = (torch.randn(*shape, generator=torch.Generator().manual_seed(1)) * 0.5).cuda()
    flops = [0.0]
    orig = lib.vae_conv

    def counted(xp, strides, weight, out, T, H, W, **kw):
        cin = kw.get("cin") or (weight.shape[-1] if weight.dim() == 5 else weight.shape[1])
        taps = weight.shape[1] * weight.shape[2] * weight.shape[3] if weight.dim() == 5 else 1
        flops[0] += 2.0 * T * H * W * weight.shape[0] * cin * taps
        return orig(xp, strides, weight, out, T, H, W, **kw)

    orig16 = lib.vae_conv16

    per_tap = "--per-tap" in sys.argv  # force the per-tap 16-bit kernel (flag 4) instead of the halo-tiled one

    def counted16(xp, strides, weight, out, T, H, W, **kw):
        if per_tap:
            kw["flags"] = kw.get("flags", 0) | 4
        flops[0] += 2.0 * T * H * W * weight.shape[0] * weight.shape[4] * 27
        flops16[0] += 2.0 * T * H * W * weight.shape[0] * weight.shape[4] * 27
        return orig16(xp, strides, weight, out, T, H, W, **kw)

    flops16 = [0.0]
    hunyuan_vae.lib.vae_conv = counted
    hunyuan_vae.lib.vae_conv16 = counted16
    if not full:
        m.decode(z)  # warm-up
        flops[0] = flops16[0] = 0.0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = m.decode(z)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert torch.isfinite(out).all()
    print(json.dumps({"workload": f"hunyuan_vae_decode z{list(shape)} -> {list(out.shape)}", "conv_operands": "fp16" if conv16 else "fp32", "attention": m.model.decoder.attn_ran,
                      "seconds": dt,
                      "conv_tflop": flops[0] / 1e12, "conv_tflop_on_fp16_kernel": flops16[0] / 1e12, "tflops_per_s": flops[0] / dt / 1e12,
                      "hbm_gb": torch.cuda.max_memory_allocated() / 1e9}))


if __name__ == "__main__":
    main()
