#!/usr/bin/env python
"""Times the CLIP ViT-H/14 image tower on the HIP kernels (lightx2v_amd/clip.py: released dims, seeded weights, a seeded 720p image) per batch of
B = 1 and B = 4 images — warmed up, HIP events, best of 3 — as eager launches and as one captured graph, and in the same process the same tower run in
fp16 through plain PyTorch on the same GPU (tests/clip_restatement.py; the role torch.nn.functional plays in tools/vae_encode_bench.py).  Also the
launch times of the tower's GEMM shapes and of its attention, and the floor of streaming the fp16 weights once at DESIGN §4's 6.29 TB/s.  One JSON line.
    python tools/clip_encode_bench.py [--reps 3] [--batches 1,4]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lightx2v_amd import clip, lib, synth  # noqa: E402

HBM_TBS = 6.29


def best_ms(fn, reps, inner=1):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b) / inner)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batches", default="1,4")
    a = ap.parse_args()
    from tests import clip_restatement as R

    lib.init(0)
    sd = synth.synth_clip_weights(synth.CLIP_DIMS["clip-vit-h-14"], seed=0, device="cuda")
    m = clip.CLIPModel(torch.float16, "cuda", sd, False, None, None)
    w16 = R.prepare(sd, torch.float16, "cuda")  # the baseline's parameters as a loaded module holds them (LayerNorm in fp32): no casts inside the timed forward
    g = torch.Generator().manual_seed(4)
    floor_ms = m.weight_bytes() / (HBM_TBS * 1e12) * 1e3
    res = {"workload": "clip ViT-H/14 image tower, 31 blocks, 720p image -> [B, 257, 1280] fp16", "weight_bytes": m.weight_bytes(), "weight_stream_floor_ms": floor_ms,
           "launches_per_forward": 2 + 7 * len(m.blocks)}
    for B in (int(v) for v in a.batches.split(",")):
        imgs = [(torch.rand(3, 1, 720, 1280, generator=g) * 2 - 1).cuda() for _ in range(B)]
        m.graph = False
        eager = best_ms(lambda: m.visual(imgs, None), a.reps)
        tower = best_ms(lambda: m.forward_tokens(B), a.reps)  # without the front end and the output copy
        m.graph = True
        graph = best_ms(lambda: m.visual(imgs, None), a.reps)
        tower_graph = best_ms(lambda: m.forward_tokens(B), a.reps)
        torch_ms = best_ms(lambda: R.visual(w16, imgs, dtype=torch.float16, device="cuda"), a.reps)
        res[f"B{B}"] = {"hip_visual_ms": eager, "hip_visual_graph_ms": graph, "hip_tower_only_ms": tower, "hip_tower_only_graph_ms": tower_graph, "torch_fp16_visual_ms": torch_ms,
                        "hip_ms_per_image": min(eager, graph) / B, "torch_over_hip": torch_ms / min(eager, graph), "hip_over_weight_floor": min(tower, tower_graph) / floor_ms,
                        "tflops_per_s": clip.tower_flops(m, B) / min(tower, tower_graph) / 1e9}
    # per-kernel launch times at B = 1 (back-to-back launches of one kernel: W stays in the 256 MiB cache between them, so these are lower bounds of the in-tower times)
    M, D, F = 257, 1280, 5120
    kern = {}
    x, f = torch.randn(M, D, device="cuda").half(), torch.randn(M, F, device="cuda").half()
    b0 = m.blocks[0]
    for name, inp, (w, bias), epi in (("qkv 3840x1280", x, b0["qkv"], lib.EPI16_NONE), ("proj 1280x1280", x, b0["proj"], lib.EPI16_RESIDUAL), ("fc1 5120x1280", x, b0["fc1"], lib.EPI16_GELU_ERF),
                                      ("fc2 1280x5120", f, b0["fc2"], lib.EPI16_RESIDUAL)):
        out = torch.empty(M, w.shape[0], dtype=torch.float16, device="cuda")
        resid = torch.zeros_like(out) if epi == lib.EPI16_RESIDUAL else None
        ms = best_ms(lambda: lib.gemm_f16(inp, w, bias, epilogue=epi, resid=resid, out=out), a.reps, inner=20)
        kern[f"gemm {name}"] = {"ms": ms, "weight_floor_ms": w.numel() * 2 / (HBM_TBS * 1e12) * 1e3, "tile": lib.gemm_f16_tile_choice(M, w.shape[0])}
    qkv = torch.randn(M, 3 * D, device="cuda").half()
    att = torch.empty(M, D, dtype=torch.float16, device="cuda")
    kern["attention 16 heads x 257"] = {"ms": best_ms(lambda: lib.attention_f16_d80(qkv, 1, 16, out=att), a.reps, inner=20)}
    kern["layernorm 257x1280"] = {"ms": best_ms(lambda: lib.layernorm_f16(x, b0["n1"][0], b0["n1"][1], out=att), a.reps, inner=20)}
    img = torch.rand(3, 720, 1280, device="cuda") * 2 - 1
    xa = torch.empty(256, 608, dtype=torch.float16, device="cuda")
    kern["front end 720p"] = {"ms": best_ms(lambda: lib.clip_preprocess(img, xa, 224, 14, synth.CLIP_MEAN, synth.CLIP_STD), a.reps, inner=20)}
    res["kernels_B1"] = kern
    res["per_block_kernel_sum_ms"] = sum(v["ms"] for k, v in kern.items() if k.startswith("gemm") or k.startswith("attention")) + 2 * kern["layernorm 257x1280"]["ms"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
