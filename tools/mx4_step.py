#!/usr/bin/env python
"""One Wan denoise step with MXFP4 x MXFP4 block linears (`mm_type` W-mxfp4-A-mxfp4-dynamic-Hip, what `tools/e2e.py --mxfp4` configures) against the
bf16 step, two models on the same seeded synthetic weights and inputs in one process: rel L2 of the first forward's noise prediction against the
bf16 model's, and the step time A-B-A-B, median of --rounds.  Other mm_types can be named with --mm.  One JSON line, also written to --out."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lightx2v_amd import lib, scheduler, synth, wan  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="wan1.3b_480px49f")
    ap.add_argument("--mm", default="W-mxfp4-A-mxfp4-dynamic-Hip,W-mxfp8-A-mxfp8-dynamic-Hip")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lib.init()
    wl = synth.WORKLOADS[a.workload]
    dims = synth.WAN_DIMS[wl["model"]]
    _, overrides, wd, lat, inputs = synth.workload_setup(a.workload, seed=0, device="cuda")
    models = {}
    for mm in ["Hip-bf16"] + a.mm.split(","):
        extra = dict(overrides)
        if mm != "Hip-bf16":
            extra["mm_config"] = {"mm_type": mm, "weight_auto_quant": True}
        cfg = wan.default_config(dims, target_shape=wl["target_shape"], target_video_length=wl["frames"], infer_steps=4, **extra)
        model = wan.WanModel(cfg, wd)
        sch = scheduler.WanScheduler(cfg, device="cuda")
        sch.prepare(latents=lat)
        model.set_scheduler(sch)
        models[mm] = (model, sch)
    del wd

    def step(mm):
        model, sch = models[mm]
        sch.step_pre(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.infer(inputs)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, sch.noise_pred.float()

    first = {mm: step(mm)[1].clone() for mm in models}  # also the warm-up
    ref = first["Hip-bf16"].double()
    ms = {mm: [] for mm in models}
    for _ in range(a.rounds):
        for mm in models:
            ms[mm].append(step(mm)[0])
    out = {"tool": "mx4_step", "workload": a.workload, "rounds": a.rounds, "cfg": True, "data": "synthetic weights / latents / text embeddings", "box_mfma_bf16_tflops": lib.mfma_probe(500),
           "step_ms": {mm: statistics.median(v) for mm, v in ms.items()}, "step_ms_all": ms,
           "step_over_bf16": {mm: statistics.median(v) / statistics.median(ms["Hip-bf16"]) for mm, v in ms.items()},
           "rel_l2_of_one_forward_vs_bf16": {mm: float((first[mm].double() - ref).norm() / ref.norm()) for mm in models if mm != "Hip-bf16"}}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
