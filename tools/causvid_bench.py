#!/usr/bin/env python
"""The V^T cache append and the attention over the cache at the shapes of the reference's CausVid configuration on Wan-1.3B 480p: blocks of 3 latent
frames = 4680 tokens, 12 heads, a cache of 21 frames = 32 760 keys.  One process, device events, A-B-A-B, median of `--rounds` (7); a sample is
`--inner` (20) back-to-back launches inside one event pair divided by their number (one launch is a few microseconds).  All shapes are warmed first.

  append_vs_same_rows     x2v_transpose_heads_append_bf16 of 4680 rows at key0 in {0, 4680, 28 080} and at the odd offset 4681 (B) against
                          x2v_transpose_heads_bf16 of the same 4680 rows into a V^T of its own (A); the A samples of the first and the second half of each
                          round are kept apart (two A legs: their difference is the spread a ratio has to exceed); GB/s over bytes read plus written.
  append_vs_retranspose   the append of a block's 4680 rows (B) against what a driver without it would do — transpose_heads of v[:kv_end] (A) — at
                          kv_end 4680, 18 720 and 32 760.
  attention               lib.attention_cached of 4680 queries over the first kv_end keys, same three kv_end; workgroups and PFLOP/s.
  e2e                     tools/e2e.py --causvid --workload wan1.3b_480px81f in a child process: the whole 7-block run, per-block seconds.

    python tools/causvid_bench.py [--rounds 7] [--inner 20] [--out profiles/causvid_bench.json] [--no-e2e]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lightx2v_amd import lib  # noqa: E402

H, BLOCK, CAPACITY = 12, 4680, 32760


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def stats(ms):
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), runs=len(ms))


def abab(fa, fb, rounds, inner):
    """A-B-A-B per round; returns (A first legs, A second legs, B both legs)."""
    a1, a2, b = [], [], []
    for _ in range(rounds):
        a1.append(timed(fa, inner))
        b.append(timed(fb, inner))
        a2.append(timed(fa, inner))
        b.append(timed(fb, inner))
    return a1, a2, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "causvid_bench.json"))
    a = ap.parse_args()
    lib.init()
    g = torch.Generator(device="cuda").manual_seed(5)
    rn = lambda *shape: torch.randn(*shape, generator=g, device="cuda", dtype=torch.float32)  # noqa: E731
    W = H * 128
    v_all = rn(CAPACITY, W).to(torch.bfloat16)
    k_cache = rn(CAPACITY, W).to(torch.bfloat16)
    q = (rn(BLOCK, W) * lib.ATTN_PRESCALE).to(torch.bfloat16)
    tiles = (CAPACITY + 63) // 64
    vt_cache = torch.zeros((H, tiles, 128, 64), dtype=torch.bfloat16, device="cuda")
    lib.transpose_heads_append(v_all, vt_cache, 0)  # a full cache: every attention below reads real values
    v_blk = v_all[:BLOCK]
    blk_tiles = (BLOCK + 63) // 64
    vt_blk = torch.empty((H, blk_tiles, 128, 64), dtype=torch.bfloat16, device="cuda")
    vt_full = torch.empty((H, tiles, 128, 64), dtype=torch.bfloat16, device="cuda")
    out = torch.empty(BLOCK, W, dtype=torch.bfloat16, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    L = lib._lib

    # Both legs call the C entry with prepared arguments: a launch is 7-10 us of GPU time, so a Python wrapper's checks on one leg only (the first form
    # of this tool) would time the host, not the kernel.
    def transpose_rows(n, dst):  # x2v_transpose_heads_bf16 of v_all[:n] into a preallocated V^T
        args = (v_all.data_ptr(), W, dst.data_ptr(), (n + 63) // 64 * 64, n, H, st)
        return lambda: L.x2v_transpose_heads_bf16(*args)

    def append_at(key0):
        args = (v_blk.data_ptr(), W, vt_cache.data_ptr(), tiles * 64, key0, BLOCK, H, st)
        return lambda: L.x2v_transpose_heads_append_bf16(*args)

    def attend(kv_end):
        return lambda: lib.attention_cached(q, k_cache, vt_cache, kv_end, H, out=out, prescaled=True)

    key0s, kv_ends = [0, 4680, 28080, 4681], [4680, 18720, 32760]
    for f in [transpose_rows(BLOCK, vt_blk)] + [append_at(k) for k in key0s] + [transpose_rows(n, vt_full) for n in kv_ends] + [attend(n) for n in kv_ends]:
        f()  # every shape warmed before any is timed
    torch.cuda.synchronize()

    row_bytes = W * 2
    doc = dict(tool="tools/causvid_bench.py", device=torch.cuda.get_device_name(0), library=lib.version(), rounds=a.rounds, inner_launches_per_sample=a.inner,
               method="A-B-A-B in one process, one device-event pair per sample of `inner` back-to-back launches, all shapes warmed first; medians; the append and transpose legs call the C entries with prepared arguments",
               shape=dict(heads=H, block_tokens=BLOCK, cache_keys=CAPACITY))
    same = []
    for key0 in key0s:
        a1, a2, b = abab(transpose_rows(BLOCK, vt_blk), append_at(key0), a.rounds, a.inner)
        m1, m2, mb = statistics.median(a1), statistics.median(a2), statistics.median(b)
        ma = statistics.median(a1 + a2)
        first, last = key0 // 64, (key0 + BLOCK - 1) // 64
        rec = dict(key0=key0, key0_mod_64=key0 % 64, edge_kernel=bool(key0 % 8 or (key0 + BLOCK) % 8), tiles_touched=last - first + 1, transpose_same_rows=stats(a1 + a2),
                   transpose_leg1_median_ms=m1, transpose_leg2_median_ms=m2, a_leg_spread=abs(m1 - m2) / ma, append=stats(b), append_over_transpose=mb / ma,
                   append_gbps=2 * BLOCK * row_bytes / (mb * 1e-3) / 1e9, transpose_gbps=(BLOCK + blk_tiles * 64) * row_bytes / (ma * 1e-3) / 1e9)
        same.append(rec)
        print(json.dumps(rec), flush=True)
    doc["append_vs_same_rows"] = same
    retr = []
    for kv_end in kv_ends:
        a1, a2, b = abab(transpose_rows(kv_end, vt_full), append_at(kv_end - BLOCK), a.rounds, a.inner)
        ma, mb = statistics.median(a1 + a2), statistics.median(b)
        rec = dict(kv_end=kv_end, key0=kv_end - BLOCK, retranspose_whole_cache=stats(a1 + a2), append=stats(b), append_over_retranspose=mb / ma,
                   a_leg_spread=abs(statistics.median(a1) - statistics.median(a2)) / ma)
        retr.append(rec)
        print(json.dumps(rec), flush=True)
    doc["append_vs_retranspose"] = retr
    lib.transpose_heads_append(v_all, vt_cache, 0)  # the appends above wrote block 0's rows elsewhere: restore the cache the attention reads
    att = []
    for kv_end in kv_ends:
        ms = [timed(attend(kv_end), max(1, a.inner // 4)) for _ in range(a.rounds)]
        s = stats(ms)
        rec = dict(kv_end=kv_end, queries=BLOCK, workgroups=((BLOCK + 255) // 256) * H, attention=s, pflops=4.0 * 128 * BLOCK * kv_end * H / (s["median_ms"] * 1e-3) / 1e15)
        att.append(rec)
        print(json.dumps(rec), flush=True)
    doc["attention"] = att
    if not a.no_e2e:
        del v_all, k_cache, vt_cache, vt_full
        torch.cuda.empty_cache()
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "e2e.py"), "--causvid", "--workload", "wan1.3b_480px81f"], capture_output=True, text=True, timeout=900)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        if p.returncode != 0 or not lines:
            raise SystemExit(f"tools/e2e.py --causvid failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
        doc["e2e"] = json.loads(lines[-1])
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
