#!/usr/bin/env python
"""Times WanVAE.encode (HIP path) on a synthetic video of the i2v shape (720p x 81 frames: [3, 81, 720, 1280]; --video 3,81,480,832 for 480p) and
reports the encoder's algorithmic TFLOP/s counted from the shapes (lightx2v_amd.vae_enc.encode_flops: 2 per fp32 multiply-add; the split mode
multiplies three 16-bit products per fp32 one).  One JSON line.
    python tools/vae_encode_bench.py [--video 3,81,720,1280] [--reps 3] [--chunk-frames 4] [--conv16 split|fp16|fp32] [--tiled] [--torch]
--tiled also times, in the same process and on the same video, the use_tiling encode (256 / 192 px tiles, WanVAE_.tiled_encode) with its peak memory.
--torch also times the same encoder written with torch.nn.functional fp32 convolutions (tests/wan_vae_encode_restatement.py) on the same GPU, for scale."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lightx2v_amd import lib, synth, vae, vae_enc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--video", default="3,81,720,1280")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--chunk-frames", type=int, default=4, help="video frames per encoder pass after the first (a multiple of 4; 4 = the reference's)")
    ap.add_argument("--conv16", default="split", choices=["split", "fp16", "fp32"])
    ap.add_argument("--tiled", action="store_true", help="also time the use_tiling encode (fields tiled_*)")
    ap.add_argument("--tiled-chunk-frames", type=int, default=0, help="--tiled: video frames per encoder pass inside a tile (0 = --chunk-frames; the whole clip fits: a tile is 256 x 256 px)")
    ap.add_argument("--torch", action="store_true", help="also time the torch.nn.functional fp32 encoder on the same GPU")
    a = ap.parse_args()
    shape = tuple(int(v) for v in a.video.split(","))
    lib.init(0)
    sd = synth.synth_wan_vae_encoder_weights(dim=96, seed=0)
    m = vae.WanVAE(sd, dim=96, conv16={"split": "split", "fp16": True, "fp32": False}[a.conv16], encode_chunk_frames=a.chunk_frames)
    x = (torch.rand(*shape, generator=torch.Generator().manual_seed(5)) * 2 - 1).cuda()
    for _ in range(a.warmup):  # allocates every buffer
        out = m.encode([x])[0]
    torch.cuda.synchronize()
    times = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        out = m.encode([x])[0]
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    assert torch.isfinite(out).all()
    flop = sum(vae_enc.encode_flops(shape[1], shape[2], shape[3]).values())
    dt = min(times)
    res = {"workload": f"wan_vae_encode video{list(shape)} -> {list(out.shape)}", "conv_operands": a.conv16, "chunk_frames": a.chunk_frames, "seconds": dt,
           "seconds_all": times, "tflop": flop / 1e12, "tflops_per_s": flop / dt / 1e12, "max_memory_allocated_gb": torch.cuda.max_memory_allocated() / 1e9}
    if a.tiled:
        conv16 = m.model.conv16
        del m
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        m = vae.WanVAE(sd, dim=96, conv16=conv16, encode_chunk_frames=a.tiled_chunk_frames or a.chunk_frames, use_tiling=True)
        for _ in range(max(a.warmup, 1)):  # builds the (at most four) tile encoders and their buffers
            tiled = m.encode([x])[0]
        torch.cuda.synchronize()
        ttimes = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            tiled = m.encode([x])[0]
            torch.cuda.synchronize()
            ttimes.append(time.perf_counter() - t0)
        assert torch.isfinite(tiled).all() and tiled.shape == out.shape
        plan = vae.tile_plan(shape[2] // 8, shape[3] // 8, *m.model.tile_geometry())
        res.update(tiled_chunk_frames=a.tiled_chunk_frames or a.chunk_frames, tiled_seconds=min(ttimes), tiled_seconds_all=ttimes, tiled_ratio_to_plain=min(ttimes) / dt, tiles=[plan["rows"], plan["cols"]],
                   pixel_ratio_tiles_to_image=sum(p["th"] * p["tw"] for p in plan["tiles"]) / float((shape[2] // 8) * (shape[3] // 8)),
                   tiled_max_memory_allocated_gb=(torch.cuda.max_memory_allocated() - base) / 1e9,
                   tiled_rel_l2_vs_plain=((tiled - out).norm() / out.norm()).item())
    if a.torch:
        from tests import wan_vae_encode_restatement as R

        mean, inv_std = m.mean, m.inv_std
        del m
        torch.cuda.empty_cache()
        sdg = {k: v.cuda() for k, v in sd.items()}
        with torch.no_grad():
            R.encode(sdg, x[:, :5], mean, inv_std)  # warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ref = R.encode(sdg, x, mean, inv_std)
            torch.cuda.synchronize()
        res["torch_fp32_seconds"] = time.perf_counter() - t0
        res["torch_fp32_rel_l2_vs_hip"] = ((out - ref).norm() / ref.norm()).item()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
