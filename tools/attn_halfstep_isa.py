"""Counts what a softmax half-step of the ping-pong attention kernels (A9_SOFTMAX, lightx2v_amd/csrc/attn.hip) costs in vector instructions, from the
ISA that `hipcc -S` wrote.  From every s_barrier every way through the conditional branches up to the next barrier is walked; where some path runs
the 32 exp2 and the 16 packs exactly once (no cold code), the one with the fewest vector instructions is the half-step's hot path.  Printed per
half-step: the VALU mnemonics, the s_nop, and two hazards the source is written around: a v_pk_add_f32 in the half-step, and a v_exp_f32 directly followed by an instruction that names its destination.

    python tools/attn_halfstep_isa.py attn.s [--kernel 'attn_fwd_v9_kernelILi8ELi8ELb1ELb0E'] [--list]"""
import argparse
import collections
import re
import sys

INST = re.compile(r"^\s+([a-z_0-9]+)\s*(.*?)\s*(?:;.*)?$")
LABEL = re.compile(r"^(\.LBB[0-9_]+):")


def kernel_lines(text, key):
    out, on = [], False
    for ln in text.splitlines():
        if not on and re.match(r"^_Z\w*" + re.escape(key) + r"\w*:", ln):
            on = True
            continue
        if on:
            if ln.startswith(".Lfunc_end"):
                break
            out.append(ln)
    return out


def parse(lines):
    """-> list of (mnemonic, operands) with labels as ('label', name)"""
    prog = []
    for ln in lines:
        m = LABEL.match(ln)
        if m:
            prog.append(("label", m.group(1)))
            continue
        if ln.strip().startswith((";", ".", "//")) or not ln.strip():
            continue
        m = INST.match(ln)
        if m:
            prog.append((re.sub(r"_(e32|e64|dpp|sdwa)$", "", m.group(1)), m.group(2)))
    return prog


def is_valu(mn):
    return mn.startswith("v_") and not mn.startswith(("v_mfma", "v_accvgpr", "v_readfirstlane", "v_readlane"))


def walk(prog, start, labels, take):
    """From `start` (just behind a barrier) to the next s_barrier.  take: set of branch positions whose jump is followed."""
    path, i, seen = [], start, 0
    while i < len(prog) and seen < 5000:
        mn, ops = prog[i]
        seen += 1
        if mn == "s_barrier":
            return path, i
        if mn == "s_branch":
            i = labels[ops.strip()]
            continue
        if mn.startswith("s_cbranch"):
            path.append((i, mn, ops))
            if i in take:
                i = labels[ops.strip()]
                continue
        elif mn != "label":
            path.append((i, mn, ops))
        i += 1
    return path, None


def hot_path(prog, start, labels):
    """Every combination of taken / not taken over the conditional branches met on the way (at most ten) is walked; of the paths that hold the 32
    exp2 and the 16 packs once, the one that issues the most LDS-DMA (the late role's half-step in the middle of the key walk) with the fewest VALU is the hot one."""
    best, seen, todo = None, set(), [frozenset()]
    while todo:
        take = todo.pop()
        if take in seen:
            continue
        seen.add(take)
        p, end = walk(prog, start, labels, take)
        for b in [i for i, mn, _ in p if mn.startswith("s_cbranch")][:10]:
            if b not in take and len(seen) + len(todo) < 4096:
                todo.append(take | {b})
        if end is None or sum(mn == "v_exp_f32" for _, mn, _ in p) != 32 or sum(mn == "v_cvt_pk_bf16_f32" for _, mn, _ in p) != 16:
            continue
        key = (-sum(mn.startswith("buffer_load") for _, mn, _ in p), sum(is_valu(mn) for _, mn, _ in p))
        if best is None or key < best[0]:
            best = (key, p, end)
    return None if best is None else (best[0][1], best[1], best[2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("--kernel", default="attn_fwd_v9_kernelILi8ELi8ELb1ELb0E")
    ap.add_argument("--list", action="store_true", help="print the instructions of every half-step found")
    a = ap.parse_args()
    prog = parse(kernel_lines(open(a.asm).read(), a.kernel))
    if not prog:
        sys.exit(f"no kernel matching {a.kernel}")
    labels = {ops: i for i, (mn, ops) in enumerate(prog) if mn == "label"}
    n = 0
    for i, (mn, _) in enumerate(prog):
        if mn != "s_barrier":
            continue
        got = hot_path(prog, i + 1, labels)
        if got is None:
            continue
        valu, path, end = got
        n += 1
        tally = collections.Counter(m for _, m, _ in path if is_valu(m))
        nops = [o for _, m, o in path if m == "s_nop"]
        mfma = sum(m.startswith("v_mfma") for _, m, _ in path)
        dma = sum(m.startswith("buffer_load") for _, m, _ in path)
        bad = []
        for (_, m0, o0), (_, m1, o1) in zip(path, path[1:]):
            if m0 == "v_exp_f32":
                dst = o0.split(",")[0].strip()
                if re.search(r"\b" + re.escape(dst) + r"\b", o1) or any(dst == f"v{k}" for k in _range_regs(o1)):
                    bad.append(f"{m0} {o0} -> {m1} {o1}")
        print(f"half-step {n}: instructions {path[0][0]}..{end}  VALU {valu}  ({', '.join(f'{c} {m}' for m, c in tally.most_common())})  "
              f"s_nop {len(nops)} (wait states {sum(int(o) + 1 for o in nops)})  MFMA {mfma}  LDS-DMA {dma}  "
              f"v_pk_add_f32 {tally.get('v_pk_add_f32', 0)}  exp-then-reader {len(bad)}")
        for b in bad:
            print("   HAZARD", b)
        if a.list:
            for _, m, o in path:
                print("      ", m, o)
    if n == 0:
        sys.exit("no softmax half-step found")


def _range_regs(ops):
    for lo, hi in re.findall(r"v\[(\d+):(\d+)\]", ops):
        yield from range(int(lo), int(hi) + 1)


if __name__ == "__main__":
    main()
