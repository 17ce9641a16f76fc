#!/usr/bin/env python
"""What ONE rank launches per self-attention under ring attention against what it launches under Ulysses, for the same share of the work, on one GPU.

Per shape (S tokens, H heads, N ranks): ring (A) = N carry launches (x2v_attn_fwd_bf16_vt_carry: CARRY_OUT, CARRY_IN | CARRY_OUT ..., CARRY_IN) with
Sq = Sk = S / N and all H heads; Ulysses (B) = one x2v_attn_fwd_bf16_vt launch with Sq = Sk = S and H / N heads.  Same FLOP; the ring's N chunks are
one seeded k / V^T chunk re-read N times (the kernel does not care where a chunk came from).  q prescaled, as the Wan driver hands it over.  All shapes
are warmed first; timed runs alternate A-B-A-B; a side's time is one pair of device events around all of its launches; median of --rounds.
Also reported: the bytes a rank sends per attention — ring: (N - 1) hops of the K chunk and the V^T chunk (padded to whole 64-key tiles); Ulysses: q, k, v
seq->head and o head->seq, (N - 1) / N of four [S / N, H * 128] bf16 tensors.
Nothing here measures communication: no transfer runs, exposed or hidden, and no multi-GPU figure follows from it.

    python tools/ring_bench.py [--rounds 7] [--out profiles/ring_attn_bench.json] [--shapes 75600x40x8,20280x12x4]
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


def setup(S, H, N):
    assert S % N == 0 and H % N == 0, "the comparison needs a shape both schemes can run"
    sl, hl = S // N, H // N
    g = torch.Generator(device="cuda").manual_seed(S + H + N)
    rn = lambda *shape: torch.randn(*shape, generator=g, device="cuda", dtype=torch.float32)  # noqa: E731
    # ring: this rank's query rows, all heads; one chunk of keys
    rq = (rn(sl, H * 128) * lib.ATTN_PRESCALE).to(torch.bfloat16)
    rk = rn(sl, H * 128).to(torch.bfloat16)
    rvt = lib.transpose_heads(rn(sl, H * 128).to(torch.bfloat16), H)
    rout = torch.empty(sl, H * 128, dtype=torch.bfloat16, device="cuda")
    state = lib.AttnCarryState.alloc(sl, H, "cuda")
    # Ulysses: all rows, this rank's heads
    uq = (rn(S, hl * 128) * lib.ATTN_PRESCALE).to(torch.bfloat16)
    uk = rn(S, hl * 128).to(torch.bfloat16)
    uvt = lib.transpose_heads(rn(S, hl * 128).to(torch.bfloat16), hl)
    uout = torch.empty(S, hl * 128, dtype=torch.bfloat16, device="cuda")

    def ring():
        st = state.reset()
        for s in range(N):
            lib.attention_carry(rq, rk, rvt, H, state=st, last=s == N - 1, prescaled=True, out=rout if s == N - 1 else None)

    ulysses = lambda: lib.attention(uq, uk, None, hl, out=uout, variant=lib.ATTN_FAST | lib.ATTN_Q_PRESCALED, vt=uvt)  # noqa: E731
    ring_bytes = (N - 1) * (sl * H * 128 + H * ((sl + 63) // 64) * 64 * 128) * 2
    uly_bytes = 4 * (N - 1) * sl * (H // N) * 128 * 2
    info = dict(seq_len=S, heads=H, ranks=N, ring=dict(launches=N, Sq=sl, Sk=sl, heads=H, xcd_remap=lib.attn_vt_launch_plan(sl, sl, H, one_walk=True)[0]),
                ulysses=dict(launches=1, Sq=S, Sk=S, heads=hl, xcd_remap=lib.attn_vt_launch_plan(S, S, hl)[0]), flop=4.0 * 128 * S * sl * H,
                ring_bytes_sent_per_attention=ring_bytes, ulysses_bytes_sent_per_attention=uly_bytes, ring_state_bytes=sl * H * 128 * 4 + H * sl * 4)
    return info, ring, ulysses


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
    ap.add_argument("--shapes", default="75600x40x8,20280x12x4", help="SxHxN: Wan-14B 720p x 81f at N = 8, Wan-1.3B 480p x 49f at N = 4")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ring_attn_bench.json"))
    a = ap.parse_args()
    lib.init()
    cases = [setup(*(int(x) for x in s.split("x"))) for s in a.shapes.split(",")]
    for _, ring, ulysses in cases:  # every shape warmed before any is timed
        ring()
        ulysses()
    torch.cuda.synchronize()
    results = []
    for info, ring, ulysses in cases:
        tr, tu = [], []
        for _ in range(a.rounds):
            tr.append(timed(ring))
            tu.append(timed(ulysses))
        r, u = stats(tr), stats(tu)
        rec = dict(info, ring_time=r, ulysses_time=u, ring_over_ulysses=r["median_ms"] / u["median_ms"], ring_pflops=info["flop"] / (r["median_ms"] * 1e-3) / 1e15,
                   ulysses_pflops=info["flop"] / (u["median_ms"] * 1e-3) / 1e15)
        results.append(rec)
        print(json.dumps(rec), flush=True)
    doc = dict(tool="tools/ring_bench.py", device=torch.cuda.get_device_name(0), library=lib.version(),
               method="A-B-A-B in one process, one device-event pair around a side's launches, all shapes warmed first",
               not_measured="communication (no transfer runs here), its overlap with the launches, and any multi-GPU figure: the ring has never run over xGMI",
               rounds=a.rounds, shapes=results)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
