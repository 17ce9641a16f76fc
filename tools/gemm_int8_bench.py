#!/usr/bin/env python
"""Times the int8 w8a8 GEMM against the existing fp8 kernel (x2v_gemm_fp8, variant 0) in one process, alternating a/b/a/b, at the six GEMM shapes
of a Wan2.1-14B 720p x 81-frame step (BASELINE config #4: M = 75 600; K, N in {5120, 13824}) with the plain, GELU and gated-residual epilogues.
Same bytes moved, same staging pipeline, a matrix instruction of the same nominal class: fp8 is the yardstick, parity (within 5 %) the target.

Every variant of a shape is warmed up, then each is timed `--rounds` times in turn with device events around `--iters` back-to-back launches;
the median round is reported.  Results that must agree (int8 variants among themselves) are compared on the timed operands first.  The fp8 mode of
the 128x128 kernel (fp8 v1) is timed too, to tell what the tile costs from what the instruction costs.

    python tools/gemm_int8_bench.py [--rounds 5] [--iters 10] [--out profiles/int8_gemm_bench.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lightx2v_amd import lib  # noqa: E402

M = 75600
SHAPES = (  # (name, K, N, epilogue) — the step's linear layers (self/cross-attention projections, ffn_0 with GELU, ffn_2 / o with the gated residual)
    ("q/k/v/o plain", 5120, 5120, "plain"),
    ("o gated residual", 5120, 5120, "residual"),
    ("ffn_0 plain", 5120, 13824, "plain"),
    ("ffn_0 GELU", 5120, 13824, "gelu"),
    ("ffn_2 plain", 13824, 5120, "plain"),
    ("ffn_2 gated residual", 13824, 5120, "residual"),
)
INT8_VARIANTS = (1, 5, 0)  # the 128x128 kernel, the continuous 256x256 kernel, the dispatcher's choice


def time_ms(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "int8_gemm_bench.json"))
    a = ap.parse_args()
    lib.init()
    g = torch.Generator(device="cuda").manual_seed(0)
    rows = []
    for name, K, N, epi in SHAPES:
        x = torch.randn(M, K, generator=g, device="cuda", dtype=torch.bfloat16)
        w = (torch.randn(N, K, generator=g, device="cuda", dtype=torch.bfloat16) / K**0.5)
        bias = torch.randn(N, generator=g, device="cuda", dtype=torch.bfloat16) * 0.1
        gate = torch.randn(N, generator=g, device="cuda", dtype=torch.bfloat16)
        ops = {"fp8": (lib.gemm_fp8, *lib.quant_fp8_rowwise(x), *lib.quant_fp8_rowwise(w)), "int8": (lib.gemm_int8, *lib.quant_int8_rowwise(x), *lib.quant_int8_rowwise(w))}
        del x, w
        y = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
        resid = torch.zeros(M, N, device="cuda", dtype=torch.bfloat16)

        def call(kind, variant):
            fn, xq, sx, wq, sw = ops[kind]
            if epi == "residual":  # in place on resid, as the block driver runs it
                return fn(xq, sx, wq, sw, bias, epilogue=lib.EPI_RESIDUAL, resid=resid, gate=gate, variant=variant)
            return fn(xq, sx, wq, sw, bias, epilogue=lib.EPI_GELU_TANH if epi == "gelu" else lib.EPI_NONE, out=y, variant=variant)

        # fp8 v1 = the fp8 mode of the same 128x128 kernel: int8 v1 against it is the instruction alone, against fp8 v0 instruction and tile
        runs = [("fp8 v0", "fp8", 0), ("fp8 v1", "fp8", 1)] + [(f"int8 v{v}", "int8", v) for v in INT8_VARIANTS]
        outs = {}
        for label, kind, v in runs:  # warm-up, and the results the int8 variants must share
            resid.zero_()
            outs[label] = call(kind, v).clone()
        torch.cuda.synchronize()
        equal = all(torch.equal(outs["int8 v1"], outs[f"int8 v{v}"]) for v in INT8_VARIANTS)
        del outs
        times = {label: [] for label, _, _ in runs}
        for _ in range(a.rounds):
            for label, kind, v in runs:
                times[label].append(time_ms(lambda: call(kind, v), a.iters))
        med = {label: statistics.median(t) for label, t in times.items()}
        row = {"layer": name, "M": M, "K": K, "N": N, "epilogue": epi, "int8_variant0_kernel": lib.gemm_int8_kernel_choice(M, N, K, with_form=True),
               "fp8_variant0_kernel": lib.gemm_kernel_choice(M, N, K, fp8=True, with_form=True), "int8_variants_bit_equal": equal,
               "ms": {k: round(v, 4) for k, v in med.items()}, "ms_min_max": {k: [round(min(t), 4), round(max(t), 4)] for k, t in times.items()},
               "tops": {k: round(2.0 * M * N * K / (v * 1e-3) / 1e12, 1) for k, v in med.items()},
               "int8_over_fp8_time": {k: round(v / med["fp8 v0"], 3) for k, v in med.items() if k != "fp8 v0"}}
        rows.append(row)
        print(json.dumps(row), flush=True)
    rec = {"tool": "tools/gemm_int8_bench.py", "device": torch.cuda.get_device_name(), "rounds": a.rounds, "iters": a.iters, "timing": "device events, median of rounds, a/b/a/b",
           "switches": lib.switches(), "shapes": rows}
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
