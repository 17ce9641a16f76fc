#!/usr/bin/env python
"""Block-scaled fp8 self-attention (hip_mxfp8) against the dense launch, one process, device events.

Per shape — the token counts of the benchmark workloads with their head counts — on the same seeded q / k / v (q prescaled, as the Wan driver hands it
over): A = the dense x2v_attn_fwd_bf16_vt launch on a pre-transposed V (what hip_flash runs; its V^T comes from the v projection's epilogue, so no
transposition is charged to it), B = the x2v_attn_mx_fwd launch on prepared operands, and B's preparation passes each on their own (column mean of
k, q quantiser, k quantiser, V quantiser) and all four together.  All shapes are warmed first; timed runs alternate A-B-A-B; a launch's time is one
pair of device events; medians of --rounds runs.  The box probe (bare bf16 MFMA TFLOP/s, lib.mfma_probe) is taken before and after: compare
numbers inside one file only.  Writes profiles/attn_mx_bench.json.

    python tools/attn_mx_bench.py [--rounds 7] [--out profiles/attn_mx_bench.json] [--shapes 75600x40,32760x40,20280x12]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lightx2v_amd import lib  # noqa: E402
from lightx2v_amd.lib import _check, _lib, _p, _stream  # noqa: E402


def setup(S, H):
    g = torch.Generator(device="cuda").manual_seed(S + H)
    rn = lambda *shape: torch.randn(*shape, generator=g, device="cuda", dtype=torch.float32)
    q = (rn(S, H * 128) * lib.ATTN_PRESCALE).to(torch.bfloat16)
    k = rn(S, H * 128).to(torch.bfloat16)
    v = rn(S, H * 128).to(torch.bfloat16)
    vt = lib.transpose_heads(v, H)
    ops = lib.attention_mx_prepare(q, k, v, H, prescaled=True)
    out = torch.empty(S, H * 128, dtype=torch.bfloat16, device="cuda")
    nt = (S + 127) // 128
    passes = {
        "kmean": lambda: _check(_lib.x2v_attn_mx_kmean_f32(_p(k), k.stride(0), _p(ops.kmean_buf), S, H, _stream()), "kmean"),
        "quant_q": lambda: _check(_lib.x2v_attn_mx_quant_qk(_p(q), q.stride(0), None, 0, 1.0, _p(ops.q_codes), _p(ops.q_scales), S, S, H, _stream()), "quant q"),
        "quant_k": lambda: _check(_lib.x2v_attn_mx_quant_qk(_p(k), k.stride(0), _p(ops.kmean), 1, 1.0, _p(ops.k_codes), _p(ops.k_scales), S, nt * 128, H, _stream()), "quant k"),
        "quant_vt": lambda: _check(_lib.x2v_attn_mx_quant_vt(_p(v), v.stride(0), _p(ops.vt_codes), _p(ops.vt_scales), S, H, _stream()), "quant vt"),
    }
    prepare = lambda: [f() for f in passes.values()]
    dense = lambda: lib.attention(q, k, None, H, out=out, variant=lib.ATTN_FAST | lib.ATTN_Q_PRESCALED, vt=vt)
    mx = lambda: lib.attention_mx(None, None, None, H, out=out, prepared=ops)
    return dict(seq_len=S, heads=H), dense, mx, passes, prepare


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
    ap.add_argument("--shapes", default="75600x40,32760x40,20280x12")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_mx_bench.json"))
    a = ap.parse_args()
    lib.init()
    box_before = lib.mfma_probe(500)
    cases = [setup(*(int(x) for x in s.split("x"))) for s in a.shapes.split(",")]
    for _, dense, mx, _, prepare in cases:  # every shape warmed before any is timed
        dense()
        mx()
        prepare()
    torch.cuda.synchronize()
    results = []
    for info, dense, mx, passes, prepare in cases:
        td, tm, tp = [], [], []
        each = {n: [] for n in passes}
        for _ in range(a.rounds):
            td.append(timed(dense))
            tm.append(timed(mx))
            tp.append(timed(prepare))
            for n, f in passes.items():
                each[n].append(timed(f))
        d, m, p = stats(td), stats(tm), stats(tp)
        S, H = info["seq_len"], info["heads"]
        flop = 4.0 * 128 * S * S * H
        rec = dict(info, dense=d, mx=m, prepare_total=p, prepare_passes={n: stats(v) for n, v in each.items()}, mx_over_dense=m["median_ms"] / d["median_ms"],
                   mx_with_prepare_over_dense=(m["median_ms"] + p["median_ms"]) / d["median_ms"], dense_pflops=flop / (d["median_ms"] * 1e-3) / 1e15,
                   mx_pflops=flop / (m["median_ms"] * 1e-3) / 1e15)
        results.append(rec)
        print(json.dumps(rec), flush=True)
    doc = dict(tool="tools/attn_mx_bench.py", device=torch.cuda.get_device_name(0), library=lib.version(),
               method="A-B-A-B in one process, one device-event pair per launch, all shapes warmed first, medians", rounds=a.rounds,
               box_mfma_bf16_tflops_before=box_before, box_mfma_bf16_tflops_after=lib.mfma_probe(500), shapes=results)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
