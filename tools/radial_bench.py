#!/usr/bin/env python
"""Block-sparse (radial) self-attention against the dense launch, one process, device events.

Per shape — the token grids of the three benchmark workloads with their head counts — the dense x2v_attn_fwd_bf16_vt launch (A) and the sparse
x2v_attn_bsr_fwd_bf16_vt launch (B) on the same seeded q / k / V^T (q prescaled, as the Wan driver hands it over) with the radial mask of
lightx2v_amd.radial.MaskMap (wan, decay_factor 1).  All shapes are warmed first; timed runs alternate A-B-A-B; a launch's time is one pair of
device events.  Writes profiles/radial_attn_bench.json: per shape the mask density, the density of the union over pairs of block rows (what a
256-row workgroup walks), median / min / max of both launches, sparse / dense, and PFLOP/s over the attended blocks (4 * 128 * attended (row, key)
pairs * H FLOP) — the ideal ratio is the density.

    python tools/radial_bench.py [--rounds 7] [--out profiles/radial_attn_bench.json] [--shapes 3600x21x40,1560x21x40,1560x13x12]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lightx2v_amd import lib, radial  # noqa: E402


def setup(tpf, frames, H):
    S = tpf * frames
    g = torch.Generator(device="cuda").manual_seed(S + H)
    rn = lambda *shape: torch.randn(*shape, generator=g, device="cuda", dtype=torch.float32)
    q = (rn(S, H * 128) * lib.ATTN_PRESCALE).to(torch.bfloat16)
    k = rn(S, H * 128).to(torch.bfloat16)
    vt = lib.transpose_heads(rn(S, H * 128).to(torch.bfloat16), H)
    t0 = time.perf_counter()

    class Rows:
        shape = ((S + 127) // 128 * 128,)

    mask = radial.MaskMap(S, frames).queryLogMask(Rows, "radial", block_size=128, decay_factor=1, model_type="wan")
    t1 = time.perf_counter()
    plan = lib.attn_block_plan(mask, S, S)
    t2 = time.perf_counter()
    nb = mask.shape[0]
    pad = torch.zeros(nb % 2, nb, dtype=torch.bool)
    union = torch.cat([mask, pad]).view(-1, 2, nb).any(1)
    rows_in = torch.full((nb,), 128.0)
    rows_in[-1] = S - 128 * (nb - 1)
    attended = float((mask.float() * rows_in.view(-1, 1) * rows_in.view(1, -1)).sum())  # (query row, key) pairs inside the sequence
    out = torch.empty(S, H * 128, dtype=torch.bfloat16, device="cuda")
    per_row = mask.sum(1)
    info = dict(tokens_per_frame=tpf, frames=frames, heads=H, seq_len=S, blocks_per_side=nb, mask_density=float(mask.float().mean()), union_density=float(union.float().mean()),
                blocks_per_row_min=int(per_row.min()), blocks_per_row_max=int(per_row.max()), mask_seconds_cpu=round(t1 - t0, 3), plan_seconds_cpu=round(t2 - t1, 3),
                plan_table_bytes=int(plan.table.nbytes), attended_pair_fraction=attended / (float(S) * S))
    dense = lambda: lib.attention(q, k, None, H, out=out, variant=lib.ATTN_FAST | lib.ATTN_Q_PRESCALED, vt=vt)
    sparse = lambda: lib.attention_block_sparse(q, k, vt, H, plan, prescaled=True, out=out)
    return info, dense, sparse, attended


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), runs=len(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--shapes", default="3600x21x40,1560x21x40,1560x13x12")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "radial_attn_bench.json"))
    a = ap.parse_args()
    lib.init()
    cases = [setup(*(int(x) for x in s.split("x"))) for s in a.shapes.split(",")]
    for _, dense, sparse, _ in cases:  # every shape warmed before any is timed
        dense()
        sparse()
    torch.cuda.synchronize()
    results = []
    for info, dense, sparse, attended in cases:
        td, ts = [], []
        for _ in range(a.rounds):
            td.append(timed(dense))
            ts.append(timed(sparse))
        d, s = stats(td), stats(ts)
        S, H = info["seq_len"], info["heads"]
        rec = dict(info, dense=d, sparse=s, sparse_over_dense=s["median_ms"] / d["median_ms"], ideal_ratio=info["mask_density"],
                   dense_pflops=4.0 * 128 * S * S * H / (d["median_ms"] * 1e-3) / 1e15, sparse_pflops_attended=4.0 * 128 * attended * H / (s["median_ms"] * 1e-3) / 1e15)
        results.append(rec)
        print(json.dumps(rec), flush=True)
    doc = dict(tool="tools/radial_bench.py", device=torch.cuda.get_device_name(0), library=lib.version(), method="A-B-A-B in one process, one device-event pair per launch, all shapes warmed first",
               rounds=a.rounds, shapes=results)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
