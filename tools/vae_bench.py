#!/usr/bin/env python
"""Times WanVAE.decode (HIP path) on a synthetic latent of the BASELINE shape (720p x 81 frames: z [16,21,90,160]) and
reports the convolution kernel's algorithmic TFLOP/s (2*T*H*W*Cout*Cin*taps per launch, summed over launches).
    python tools/vae_bench.py [--latent 16,21,90,160] [--reps 1] [--tiled]
--tiled adds, in the same process and on the same latent, the use_tiling decode (256 / 192 px tiles, WanVAE_.tiled_decode) with its peak memory, and times
the one-pass tile composition (x2v_vae_tile_compose_f32) against the sequential blend_axis_ path on the same raw tiles: a second JSON line.
    python tools/vae_bench.py --tiny [--tiny-latents "16,21,90,160;16,21,60,104"] [--out profiles/taehv_bench.json]
--tiny measures the tiny VAE (TAEHV, lightx2v_amd/vae_tiny.py) instead: per latent shape the HIP decode of the whole clip and with chunk_frames=4 (with peak memory),
the full Wan decode (this tool's default leg) in the same process, and the same TAEHV graph through plain PyTorch bf16 on the same GPU (tests/taehv_restatement.py on
F.conv2d, whole clip), with the box calibration (lib.mfma_probe) before and after; one JSON document, printed and written to --out."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lightx2v_amd import lib, synth, vae  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--latent", default="16,21,90,160")
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--conv16", action="store_true", help="opt-in fp16 convolution operands")
    ap.add_argument("--split", action="store_true", help="hi/lo fp16 split of the convolution operands (fp32-grade; WanVAE's default)")
    ap.add_argument("--chunk-frames", type=int, default=4, help="latent frames per decoder pass (1 = the reference's chunking)")
    ap.add_argument("--tiled", action="store_true", help="also time the use_tiling decode and the tile composition (second JSON line)")
    ap.add_argument("--tile-chunk-frames", default="none", help="--tiled: latent frames per decoder pass inside a tile, comma-separated values each timed in turn (none = the whole clip, WanVAE's default)")
    ap.add_argument("--tiny", action="store_true", help="measure the tiny VAE (TAEHV) against the full decode and plain PyTorch bf16")
    ap.add_argument("--tiny-latents", default="16,21,90,160;16,21,60,104", help="--tiny: latent shapes, ';'-separated (720p x 81f; 480p x 81f)")
    ap.add_argument("--tiny-legs", default="hip,full,torch", help="--tiny: which legs to run")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "taehv_bench.json"))
    a = ap.parse_args()
    if a.tiny:
        return tiny_main(a)
    shape = tuple(int(v) for v in a.latent.split(","))
    lib.init(0)
    sd = synth.synth_wan_vae_weights(dim=96, seed=0)
    m = vae.WanVAE(sd, dim=96, conv16=("split" if a.split else a.conv16), chunk_frames=a.chunk_frames)
    z = torch.randn(*shape, generator=torch.Generator().manual_seed(5)).cuda()
    flops = [0.0]
    orig = lib.vae_conv

    def counted(xp, strides, weight, out, T, H, W, **kw):
        cin = kw.get("cin") or (weight.shape[-1] if weight.dim() == 5 else weight.shape[1])
        taps = weight.shape[1] * weight.shape[2] * weight.shape[3] if weight.dim() == 5 else 1
        flops[0] += 2.0 * T * H * W * weight.shape[0] * cin * taps
        return orig(xp, strides, weight, out, T, H, W, **kw)

    orig16 = lib.vae_conv16

    def counted16(xp, strides, weight, out, T, H, W, **kw):
        cin = weight.shape[4] - (32 if kw.get("flags", 0) & lib.VCONV_ZERO_TAIL32 else 0)  # channels multiplied (the 32-channel-slab kernel skips a zero tail)
        flops[0] += 2.0 * T * H * W * weight.shape[0] * cin * weight.shape[1] * weight.shape[2] * weight.shape[3]
        return orig16(xp, strides, weight, out, T, H, W, **kw)

    lib.vae_conv = counted
    vae.lib.vae_conv = counted
    vae.lib.vae_conv16 = counted16
    out = m.decode(z)  # warm-up: allocates every buffer
    torch.cuda.synchronize()
    f1 = flops[0]
    t0 = time.perf_counter()
    for _ in range(a.reps):
        out = m.decode(z)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.reps
    assert torch.isfinite(out).all()
    print(json.dumps({"workload": f"wan_vae_decode z{list(shape)} -> {list(out.shape)}", "conv_operands": "fp16 hi/lo split" if a.split else "fp16" if a.conv16 else "fp32", "chunk_frames": a.chunk_frames, "seconds": dt, "conv_tflop": f1 / 1e12, "tflops_per_s": f1 / dt / 1e12,
                      "frac_of_fp32_mfma_peak_157": f1 / dt / 1e12 / 157.3, "hbm_gb_allocated": torch.cuda.max_memory_allocated() / 1e9}))
    if a.tiled:
        vae.lib.vae_conv, vae.lib.vae_conv16 = orig, orig16
        del m, out
        torch.cuda.empty_cache()
        for k in a.tile_chunk_frames.split(","):
            print(json.dumps(tiled_leg(sd, z, a, dt, f1, None if k == "none" else int(k))))


def _timed(fn, reps):
    """Warm-up call, then `reps` calls timed one by one with a device synchronisation behind each -> (last result, seconds each)."""
    out = fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return out, times


def tiny_main(a):
    from lightx2v_amd import vae_tiny
    from tests import taehv_restatement as R

    lib.init(0)
    legs = a.tiny_legs.split(",")
    reps = max(a.reps, 3)
    sd = synth.synth_taehv_weights(seed=0)
    doc = {"tool": "tools/vae_bench.py --tiny", "weights": "synth.synth_taehv_weights(seed=0)", "reps": reps, "timing": "wall clock around decode + synchronize, warm-up outside; min and all reps",
           "box_calibration": {"kernel": "v_mfma_f32_16x16x32_bf16 (x2v_mfma_probe_bf16)", "mfma_probe_tflops_before": lib.mfma_probe(500)}, "shapes": []}
    flops = [0.0]
    orig = lib.conv2d_bf16

    def counted(x, weight, out, H, W, **kw):
        flops[0] += 2.0 * (x.shape[0] - kw.get("frame_trim", 0)) * H * W * weight.numel()
        return orig(x, weight, out, H, W, **kw)

    for spec in a.tiny_latents.split(";"):
        shape = tuple(int(v) for v in spec.split(","))
        z = (torch.randn(*shape, generator=torch.Generator().manual_seed(5)) * 2.5).cuda()
        rec = {"latent": list(shape)}
        if "hip" in legs:
            for name, chunk in (("hip_whole_clip", None), ("hip_chunk_frames_4", 4)):
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                m = vae_tiny.WanVAE_tiny(sd, chunk_frames=chunk)
                vae_tiny.lib.conv2d_bf16, flops[0] = counted, 0.0
                m.decode(z)
                vae_tiny.lib.conv2d_bf16 = orig
                out, times = _timed(lambda: m.decode(z), reps)
                assert torch.isfinite(out.float()).all()
                rec[name] = {"seconds": min(times), "seconds_all": times, "conv_tflop": flops[0] / 1e12, "tflops_per_s": flops[0] / min(times) / 1e12,
                             "hbm_gb_peak": (torch.cuda.max_memory_allocated() - base) / 1e9, "video": list(out.shape)}
                del m, out
        if "full" in legs:
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            full = vae.WanVAE(synth.synth_wan_vae_weights(dim=96, seed=0), dim=96, conv16="split", chunk_frames=4)
            zf = torch.randn(*shape, generator=torch.Generator().manual_seed(5)).cuda()
            out, times = _timed(lambda: full.decode(zf), 1 if shape[1] * shape[2] * shape[3] > 100000 else reps)
            rec["full_wan_vae_split_chunk4"] = {"seconds": min(times), "seconds_all": times, "hbm_gb_peak": (torch.cuda.max_memory_allocated() - base) / 1e9}
            del full, out, zf
        if "torch" in legs:
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            sdg = {k: v.cuda() for k, v in sd.items()}
            try:
                out, times = _timed(lambda: R.wan_decode(sdg, z), reps)
                rec["torch_bf16_f_conv2d_whole_clip"] = {"seconds": min(times), "seconds_all": times, "hbm_gb_peak": (torch.cuda.max_memory_allocated() - base) / 1e9}
                del out
            except RuntimeError as e:  # reported as it comes out (an out-of-memory or a MIOpen refusal at this size is a result)
                rec["torch_bf16_f_conv2d_whole_clip"] = {"error": str(e)[:300]}
        if "hip_whole_clip" in rec and "full_wan_vae_split_chunk4" in rec:
            rec["tiny_over_full"] = rec["hip_whole_clip"]["seconds"] / rec["full_wan_vae_split_chunk4"]["seconds"]
        if "hip_whole_clip" in rec and "seconds" in rec.get("torch_bf16_f_conv2d_whole_clip", {}):
            rec["hip_over_torch"] = rec["hip_whole_clip"]["seconds"] / rec["torch_bf16_f_conv2d_whole_clip"]["seconds"]
        doc["shapes"].append(rec)
        print(json.dumps(rec), flush=True)
    doc["box_calibration"]["mfma_probe_tflops_after"] = lib.mfma_probe(500)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


def compose_bytes(plan, t, c, scale):
    """Bytes the composition has to move: every output value once out, and in the raw values it is made of (centre, and up / left / up-left inside the blend zones)."""
    n = sum(2 * p["rh"] * p["rw"] + p["ev"] * p["rw"] + p["rh"] * p["eh"] + p["ev"] * p["eh"] for p in plan["tiles"])
    return 4.0 * t * c * scale * scale * n


def tiled_leg(sd, z, a, plain_s, plain_flop, tile_chunk_frames):
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    m = vae.WanVAE(sd, dim=96, conv16=("split" if a.split else a.conv16), use_tiling=True, tile_chunk_frames=tile_chunk_frames)
    out = m.decode(z)  # warm-up: builds the (at most four) tile decoders and their buffers
    torch.cuda.synchronize()
    times = []
    for _ in range(max(a.reps, 2)):
        t0 = time.perf_counter()
        out = m.decode(z)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    assert torch.isfinite(out).all() and out.abs().max().item() <= 1.0
    peak = (torch.cuda.max_memory_allocated() - base) / 1e9
    _, t, h, w = z.shape
    plan = vae.tile_plan(h, w, *m.model.tile_geometry())
    t_out = out.shape[2]
    px_tiles = sum(64 * p["th"] * p["tw"] for p in plan["tiles"])
    # the composition alone, fused vs sequential, on raw tiles of the decode's shapes, alternating
    g = torch.Generator(device="cuda").manual_seed(1)
    raw = [torch.randn(t_out, 8 * p["th"], 8 * p["tw"], 3, device="cuda", generator=g) for p in plan["tiles"]]
    seq_plan = dict(plan, mode="sequential")  # the in-place path takes any geometry (it blends the tiles it is given: values drift over the reps, the work does not)
    img = torch.empty_like(out[0])
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    res = {"fused": [], "sequential": []}
    for rep in range(6):
        for name, pl in (("fused", plan), ("sequential", seq_plan)):
            ev[0].record()
            vae.compose_tiles(pl, raw, img, scale=8, clamp=True)
            ev[1].record()
            torch.cuda.synchronize()
            if rep:  # the first pass of either is the warm-up
                res[name].append(ev[0].elapsed_time(ev[1]) * 1e-3)
    nbytes = compose_bytes(plan, t_out, 3, 8)
    fused_s, seq_s = min(res["fused"]), min(res["sequential"])
    dt = min(times)
    return {"workload": f"wan_vae_tiled_decode z{list(z.shape)} -> {list(out.shape)}", "tiles": [plan["rows"], plan["cols"]], "tile_px": [m.model.tile_sample_min_height, m.model.tile_sample_stride_height],
            "tile_chunk_frames": tile_chunk_frames, "seconds": dt, "seconds_all": times, "plain_seconds": plain_s, "ratio_to_plain": dt / plain_s, "pixel_ratio_tiles_to_image": px_tiles / (64.0 * h * w),
            "plain_conv_tflop": plain_flop / 1e12, "hbm_gb_peak_tiled": peak, "compose_fused_s": fused_s, "compose_fused_s_all": res["fused"], "compose_sequential_s": seq_s,
            "compose_sequential_s_all": res["sequential"], "compose_gb_moved": nbytes / 1e9, "compose_fused_tb_per_s": nbytes / fused_s / 1e12,
            "compose_share_of_tiled_decode": fused_s / dt}


if __name__ == "__main__":
    main()
