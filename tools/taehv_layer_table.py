#!/usr/bin/env python
"""Per-layer table of one tiny VAE (TAEHV) decode from a `rocprofv3 --kernel-trace` CSV: the operations and bytes each launch needs, counted from the shapes, over
its kernel time (profiles/taehv_rocprof_layers.txt is one run's).
    python tools/taehv_layer_table.py TRACE.csv [--latent 16,21,90,160] [--decodes 3]
The trace must hold `--decodes` whole-clip decodes of that latent by WanVAE_tiny and nothing else on the taehv kernels; the LAST decode's 36 launches are listed.
GFLOP = 2 x frames x H x W x Cout x Ctot x k^2; GB = the operand read once at its own resolution + the output written + the residual read, bf16 (halo re-reads and
weights are not counted; Clamp reads fp32)."""
import argparse
import csv

WIDTHS, STRIDES = (256, 128, 64, 64), (1, 2, 2)


def layer_plan(T, h, w):
    """(name, frames, H, W, Ctot, Cout, k, share of the output pixels the operand holds, residual?) in launch order."""
    plan = [("0 Clamp 16", T, h, w, 0, 16, 0, 1, False), ("1 conv3 16->256 +ReLU", T, h, w, 16, 256, 3, 1, False)]
    idx = 3
    for s in range(3):
        c = WIDTHS[s]
        for b in range(3):
            plan.append((f"{idx + b}.0 conv3 2x{c}->{c} +ReLU (two-source)", T, h, w, 2 * c, c, 3, 1, False))
            plan.append((f"{idx + b}.2 conv3 {c}->{c} +ReLU", T, h, w, c, c, 3, 1, False))
            plan.append((f"{idx + b}.4 conv3 {c}->{c} +x +ReLU", T, h, w, c, c, 3, 1, True))
        plan.append((f"{idx + 4} TGrow 1x1 {c}->{STRIDES[s] * c} (time-split)", T, h, w, c, STRIDES[s] * c, 1, 1, False))
        T, h, w = T * STRIDES[s], 2 * h, 2 * w
        plan.append((f"{idx + 5} conv3 {c}->{WIDTHS[s + 1]} (upsample-read)" + (" +ReLU" if s == 2 else ""), T, h, w, c, WIDTHS[s + 1], 3, 0.25, False))
        idx += 6
    plan.append(("22 conv3 64->3 head (x2-1, channel-first, trim 3)", T - 3, h, w, 64, 3, 3, 1, False))
    return plan


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--latent", default="16,21,90,160")
    ap.add_argument("--decodes", type=int, default=3)
    a = ap.parse_args()
    _, T, h, w = (int(v) for v in a.latent.split(","))
    rows = [r for r in csv.DictReader(open(a.trace)) if "x2v::taehv" in r["Kernel_Name"]]
    plan = layer_plan(T, h, w)
    assert len(rows) == a.decodes * len(plan), f"{len(rows)} taehv launches in the trace, {a.decodes} x {len(plan)} expected"
    tot_t = tot_f = tot_b = 0.0
    print(f"{'layer':58} {'frames x H x W':>16} {'GFLOP':>9} {'GB':>7} {'ms':>7} {'TFLOP/s':>8} {'TB/s':>6}")
    for (name, T_, H, W, ct, co, k, share, resid), r in zip(plan, rows[-len(plan):]):
        ms = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
        px = T_ * H * W
        fl = 2.0 * px * ct * co * k * k
        by = px * 16 * (4 + 2) if k == 0 else px * 2 * (ct * share + co + (co if resid else 0))
        tot_t, tot_f, tot_b = tot_t + ms, tot_f + fl, tot_b + by
        print(f"{name:58} {f'{T_}x{H}x{W}':>16} {fl / 1e9:9.1f} {by / 1e9:7.3f} {ms:7.3f} {fl / ms / 1e9:8.1f} {by / ms / 1e9:6.2f}")
    print(f"{'total':58} {'':>16} {tot_f / 1e9:9.1f} {tot_b / 1e9:7.3f} {tot_t:7.3f} {tot_f / tot_t / 1e9:8.1f} {tot_b / tot_t / 1e9:6.2f}")


if __name__ == "__main__":
    main()
