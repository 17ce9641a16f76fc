"""Per-frame cross-attention (x2v_attn_frames_fwd_bf16) against what the tree could do before it for the whole-frame case: x2v_attn_fwd_bf16_vt_batched
with B = frames, Sq = rows per frame, Sk = 128, its V^T preparation (x2v_transpose_heads_bf16) timed separately.

Method: one process, both kernels warmed up, then 7 rounds of A-B (so A-B-A-B-...), each timing `--launches` back-to-back launches between two
device events; the figure is the median of the 7 per-launch times.  Bytes = q in + o out + K + V, counted from the shapes; GB/s = bytes / time; the
byte floor is taken at 5 TB/s.  The two outputs are compared (same inputs) before anything is timed.

    python tools/audio_attn_bench.py --out profiles/audio_attn_bench.json"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lightx2v_amd import lib  # noqa: E402

SHAPES = ((21, 3600, 40), (21, 1560, 40), (13, 1560, 12))  # (frames, rows per frame, heads): 14B 720p, 14B 480p, 1.3B 480p x 49 f
KF = 128
FLOOR_BPS = 5e12


def timed(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / launches


def bench(frames, rpf, H, launches, rounds=7):
    W, g = H * 128, torch.Generator(device="cuda").manual_seed(frames * rpf + H)
    rn = lambda rows: torch.randn(rows, W, generator=g, device="cuda", dtype=torch.float32).to(torch.bfloat16)
    q, k, v = rn(frames * rpf), rn(frames * KF), rn(frames * KF)
    o_new, o_old = torch.empty_like(q), torch.empty_like(q)
    vt = lib.transpose_heads(v, H)
    new = lambda: lib.attention_frames(q, k, v, H, rpf, keys_per_frame=KF, out=o_new)

    def old():
        lib._check(lib._lib.x2v_attn_fwd_bf16_vt_batched(q.data_ptr(), W, rpf * W, k.data_ptr(), W, KF * W, vt.data_ptr(), frames * KF, KF * 128, o_old.data_ptr(), W, rpf * W, rpf, KF,
                                                         H, frames, 128, 0.0, 0, lib._stream()), "attn_fwd_vt_batched")

    prep = lambda: lib.transpose_heads(v, H)
    for fn in (new, old, prep):
        timed(fn, 3)
    diff = float((o_new.float() - o_old.float()).abs().max())
    t = {"new": [], "old": [], "prep": []}
    for _ in range(rounds):
        t["new"].append(timed(new, launches))
        t["old"].append(timed(old, launches))
        t["prep"].append(timed(prep, launches))
    med = {n: statistics.median(x) for n, x in t.items()}
    nbytes = 2 * (2 * frames * rpf * W + 2 * frames * KF * W)
    return {"frames": frames, "rows_per_frame": rpf, "heads": H, "bytes": nbytes, "max_abs_diff_new_vs_batched": diff,
            "attn_frames_ms": med["new"], "batched_vt_ms": med["old"], "vt_prep_ms": med["prep"], "ratio_batched_over_frames": med["old"] / med["new"],
            "attn_frames_GBps": nbytes / med["new"] / 1e6, "batched_vt_GBps": nbytes / med["old"] / 1e6, "byte_floor_ms_at_5TBps": nbytes / FLOOR_BPS * 1e3,
            "attn_frames_fraction_of_floor": nbytes / FLOOR_BPS * 1e3 / med["new"], "spread_ms": {n: [min(x), max(x)] for n, x in t.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/audio_attn_bench.json")
    ap.add_argument("--launches", type=int, default=40)
    args = ap.parse_args()
    lib.init()
    res = {"device": torch.cuda.get_device_name(0), "calibration_mfma_bf16_tflops": lib.mfma_probe(), "method": "A-B-A-B in one process, device events, median of 7",
           "shapes": [bench(*s, args.launches) for s in SHAPES]}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
