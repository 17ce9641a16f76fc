#!/usr/bin/env python
"""MXFP4 x MXFP4 against MXFP8 x MXFP8 in one process: the quantisers (HBM-bound) and the GEMMs per body and automatic (MFMA-bound: 10 PFLOP/s
for two 4-bit operands, 5 for fp8) at the Wan2.1-14B 720p and 1.3B 480p shapes, and the accuracy that 4 bits cost at two small shapes.  Each pair
is timed A-B-A-B with one pair of device events per call, median of --rounds (7) rounds, on random (not zero) operands.  The line carries the
box probe (bare bf16 MFMA TFLOP/s, lib.mfma_probe) before and after: compare numbers inside one file only.  One JSON line, also written to --out."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lightx2v_amd import lib  # noqa: E402

QUANT_SHAPES = ((75600, 5120), (75600, 13824), (20280, 1536))  # M, K
GEMM_SHAPES = ((75600, 5120, 5120), (75600, 5120, 13824), (75600, 13824, 5120), (20280, 1536, 8960))  # M, K, N
PARITY_SHAPES = ((257, 1536, 1536), (512, 8960, 1536))  # m, k, n


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


def rel_l2(got, ref):
    return float((got.double() - ref.double()).norm() / ref.double().norm())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lib.init()
    out = {"tool": "mx4_bench", "rounds": a.rounds, "box_mfma_bf16_tflops_before": lib.mfma_probe(500), "quant": [], "gemm": [], "parity": []}
    for M, K in QUANT_SHAPES:
        x = torch.randn(M, K, dtype=torch.bfloat16, device="cuda")
        t = abab({"mxfp4": lambda: lib.quant_mxfp4(x), "mxfp8": lambda: lib.quant_mxfp8(x)}, a.rounds)
        b4, b8 = M * K * (2 + 0.5 + 1 / 32), M * K * (2 + 1 + 1 / 32)
        out["quant"].append({"M": M, "K": K, "mxfp4_ms": t["mxfp4"], "mxfp4_GB/s": b4 / t["mxfp4"] / 1e6, "mxfp4_frac_of_6290": b4 / t["mxfp4"] / 1e6 / 6290, "mxfp8_ms": t["mxfp8"],
                             "mxfp8_GB/s": b8 / t["mxfp8"] / 1e6, "mxfp8_frac_of_6290": b8 / t["mxfp8"] / 1e6 / 6290, "mxfp4_over_mxfp8": t["mxfp4"] / t["mxfp8"]})
        del x
    for M, K, N in GEMM_SHAPES:
        x, w = torch.randn(M, K, dtype=torch.bfloat16, device="cuda"), torch.randn(N, K, dtype=torch.bfloat16, device="cuda")
        (a4, sa4), (w4, sw4) = lib.quant_mxfp4(x), lib.quant_mxfp4(w)
        (a8, sa8), (w8, sw8) = lib.quant_mxfp8(x), lib.quant_mxfp8(w)
        del x, w
        y = torch.empty(M, N, dtype=torch.bfloat16, device="cuda")
        fns = {}
        for v, tag in ((1, "tile128"), (2, "tile256"), (0, "auto")):
            fns[f"mxfp4_{tag}"] = lambda v=v: lib.gemm_mxfp4(a4, sa4, w4, sw4, out=y, variant=v)
            fns[f"mxfp8_{tag}"] = lambda v=v: lib.gemm_mxfp8(a8, sa8, w8, sw8, out=y, variant=v)
        t = abab(fns, a.rounds)
        row = {"M": M, "K": K, "N": N}
        for tag in ("tile128", "tile256", "auto"):
            t4, t8 = t[f"mxfp4_{tag}"], t[f"mxfp8_{tag}"]
            tf4, tf8 = 2.0 * M * N * K / t4 / 1e9, 2.0 * M * N * K / t8 / 1e9
            row.update({f"mxfp4_{tag}_ms": t4, f"mxfp4_{tag}_TFLOP/s": tf4, f"mxfp4_{tag}_frac_of_10000": tf4 / 10000, f"mxfp8_{tag}_ms": t8, f"mxfp8_{tag}_TFLOP/s": tf8,
                        f"mxfp8_{tag}_frac_of_5000": tf8 / 5000, f"mxfp4_over_mxfp8_{tag}": t4 / t8})
        out["gemm"].append(row)
        del a4, sa4, w4, sw4, a8, sa8, w8, sw8, y
    for m, k, n in PARITY_SHAPES:  # relL2 of the GEMM output against the exact (float64) product of the bf16 inputs
        g = torch.Generator(device="cuda").manual_seed(m)
        x, w = torch.randn(m, k, dtype=torch.bfloat16, device="cuda", generator=g), torch.randn(n, k, dtype=torch.bfloat16, device="cuda", generator=g)
        ref = x.double() @ w.double().T
        (a4, sa4), (w4, sw4), (a8, sa8), (w8, sw8), (w6, sw6) = lib.quant_mxfp4(x), lib.quant_mxfp4(w), lib.quant_mxfp8(x), lib.quant_mxfp8(w), lib.quant_mxfp6(w)
        out["parity"].append({"m": m, "k": k, "n": n, "rel_l2_mxfp4": rel_l2(lib.gemm_mxfp4(a4, sa4, w4, sw4), ref), "rel_l2_mxfp6_mxfp8": rel_l2(lib.gemm_mxfp6_mxfp8(a8, sa8, w6, sw6), ref),
                              "rel_l2_mxfp8": rel_l2(lib.gemm_mxfp8(a8, sa8, w8, sw8), ref), "rel_l2_bf16": rel_l2(lib.gemm(x, w), ref)})
    out["box_mfma_bf16_tflops_after"] = lib.mfma_probe(500)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
