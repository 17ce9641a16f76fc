"""How often the sum guard of the ping-pong attention kernels' softmax half-step (A9_SOFTMAX, lightx2v_amd/csrc/attn.hip) fires without cause on the
synthetic headline workload: the q and k that block 0's self-attention launch receives (normed, RoPE'd, q prescaled) are captured from the first
denoise step, and the lazy-rescale walk of tests/attn_guard_ref.py (fp32 torch, the kernel's lane map and sum association) is run over every
key tile for evenly spaced waves of some heads.  Prints one JSON line: tiles walked, tiles on which the guard fires, on which the exact condition
holds, and the false positives (guard without the condition) — DESIGN.md §4.1 quotes the rate.

    python tools/attn_guard_rate.py [--workload wan14b_720px81f] [--waves 64] [--heads 0,20]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lightx2v_amd import lib, scheduler, synth, wan  # noqa: E402
from tests import attn_guard_ref as G  # noqa: E402


class Captured(Exception):
    pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="wan14b_720px81f")
    ap.add_argument("--waves", type=int, default=64)
    ap.add_argument("--heads", default="0,20")
    args = ap.parse_args()
    lib.init(0)
    wl = synth.WORKLOADS[args.workload]
    dims = synth.WAN_DIMS[wl["model"]]
    extra = {k: wl[k] for k in ("sample_guide_scale", "sample_shift") if k in wl}
    cfg = wan.default_config(dims, target_shape=wl["target_shape"], target_video_length=wl["frames"], infer_steps=wl.get("infer_steps", 50), enable_cfg=True, cfg_pair="auto", **extra)
    _, _, wd, lat, inputs = synth.workload_setup(args.workload, seed=0, device="cuda")
    model = wan.WanModel(cfg, wd)
    del wd
    sch = scheduler.WanScheduler(cfg, device="cuda")
    sch.prepare(latents=lat)
    model.set_scheduler(sch)
    got = {}

    def batched(q, k, vt, num_heads, nb, Sp, S, **kw):
        got.update(q=q[:S].clone(), k=k[:S].clone(), H=num_heads, prescaled=bool(kw.get("prescaled")))
        raise Captured

    def single(q, k, v, num_heads, head_dim=128, **kw):
        got.update(q=q.clone(), k=k.clone(), H=num_heads, prescaled=bool(kw.get("variant", 0) & lib.ATTN_Q_PRESCALED))
        raise Captured

    lib.attention_batched, lib.attention = batched, single
    sch.step_pre(0)
    try:
        model.infer(inputs)
    except Captured:
        pass
    assert got and got["prescaled"], "no prescaled self-attention launch was captured"
    torch.cuda.synchronize()
    q, k, H = got["q"], got["k"], got["H"]
    del model, inputs
    torch.cuda.empty_cache()
    S = q.shape[0]
    heads = [int(h) for h in args.heads.split(",")]
    nwaves = S // 32
    picks = [round(i * (nwaves - 1) / (args.waves - 1)) for i in range(args.waves)]
    rows = torch.cat([torch.arange(32 * w, 32 * w + 32) for w in picks]).cuda()
    qh = q.reshape(S, H, 128)[rows][:, heads].permute(1, 0, 2).float()
    kh = k.reshape(S, H, 128)[:, heads].permute(1, 0, 2).float()
    s = qh @ kh.transpose(-1, -2)  # fp32 products of bf16 values, fp32 accumulation: the MFMA's scores up to summation order
    trace = []
    G.emulate_guarded(s, torch.zeros(len(heads), S, 128, device="cuda"), trace=trace)
    guard = sum(int(t["guard"].sum()) for t in trace)
    exact = sum(int(t["exact"].sum()) for t in trace)
    false_pos = sum(int((t["guard"] & ~t["exact"]).sum()) for t in trace)
    missed = sum(int((t["exact"] & ~t["guard"]).sum()) for t in trace)
    tiles = len(trace) * len(heads) * args.waves
    print(json.dumps({"workload": args.workload, "tokens": S, "heads": heads, "waves": args.waves, "tiles_after_the_first": tiles, "guard_fires": guard,
                      "exact_condition_holds": exact, "false_positives": false_pos, "false_positive_rate": false_pos / tiles, "cold_branch_rate": guard / tiles,
                      "exact_without_guard": missed, "largest_lane_sum_on_a_quiet_tile": max(float(t["lane_sum"][~t["guard"]].max()) for t in trace if (~t["guard"]).any())}))


if __name__ == "__main__":
    main()
