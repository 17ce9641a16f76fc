#!/usr/bin/env python
"""The fp8 block-128 GEMM and quantiser (gemm_b128.hip) against the per-channel fp8 pair (x2v_gemm_fp8 / x2v_quant_fp8_rowwise) in one process, at the
Wan2.1-14B 720p and 1.3B 480p linear-layer shapes.  Each pair is timed A-B-A-B with one pair of device events per call, median of --rounds (7)
rounds, on random (not zero) operands.  The line carries the box probe (bare bf16 MFMA TFLOP/s, lib.mfma_probe) before and after: compare numbers
inside one file only.  One JSON line, also written to --out (profiles/gemm_block128_bench.json is one run's)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lightx2v_amd import lib, ops  # noqa: E402

QUANT_SHAPES = ((75600, 5120), (75600, 13824), (20280, 1536))  # M, K
GEMM_SHAPES = ((75600, 5120, 5120), (75600, 13824, 5120), (75600, 5120, 13824), (20280, 1536, 1536), (20280, 8960, 1536), (20280, 1536, 8960))  # M, N, K


def abab(fns, rounds):
    """{name: median ms} of the callables, interleaved: one call of each per round, each between its own pair of events."""
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            f()
            e.record()
            torch.cuda.synchronize()
            ms[k].append(s.elapsed_time(e))
    return {k: statistics.median(v) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lib.init()
    out = {"tool": "gemm_block128_bench", "method": "A-B-A-B in one process, device events, median of rounds", "rounds": a.rounds,
           "box_mfma_bf16_tflops_before": lib.mfma_probe(500), "quant": [], "gemm": []}
    for M, K in QUANT_SHAPES:
        x = torch.randn(M, K, dtype=torch.bfloat16, device="cuda")
        t = abab({"group128": lambda: lib.quant_fp8_group128(x), "rowwise": lambda: lib.quant_fp8_rowwise(x)}, a.rounds)
        bg, br = M * K * (3 + 4 / 128), M * K * 3 + 4 * M  # bytes read + written
        out["quant"].append({"M": M, "K": K, "group128_ms": t["group128"], "group128_GB/s": bg / t["group128"] / 1e6, "rowwise_ms": t["rowwise"],
                             "rowwise_GB/s": br / t["rowwise"] / 1e6, "group128_over_rowwise": t["group128"] / t["rowwise"]})
        del x
    for M, N, K in GEMM_SHAPES:
        x = torch.randn(M, K, dtype=torch.bfloat16, device="cuda")
        w = (torch.randn(N, K, dtype=torch.float32, device="cuda") / K ** 0.5).to(torch.bfloat16)
        (xg, sg), (xr, sr) = lib.quant_fp8_group128(x), lib.quant_fp8_rowwise(x)
        wb, swb = ops.MMWeightFp8Block128Hip.per_block_cast_to_fp8(w)
        pc = ops.MMWeightFp8Hip("w.weight", None)
        pc.load({"w.weight": w})
        del x, w
        y = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
        t = abab({"block128": lambda: lib.gemm_fp8_block128(xg, sg, wb, swb, out=y), "per_channel": lambda: lib.gemm_fp8(xr, sr, pc.weight, pc.weight_scale, out=y)}, a.rounds)
        fl = 2.0 * M * N * K
        out["gemm"].append({"M": M, "N": N, "K": K, "block128_ms": t["block128"], "block128_TFLOP/s": fl / t["block128"] / 1e9, "block128_frac_of_5000": fl / t["block128"] / 1e9 / 5000,
                            "per_channel_ms": t["per_channel"], "per_channel_TFLOP/s": fl / t["per_channel"] / 1e9, "block128_over_per_channel": t["block128"] / t["per_channel"]})
        del xg, sg, xr, sr, wb, swb, pc, y
    out["box_mfma_bf16_tflops_after"] = lib.mfma_probe(500)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
