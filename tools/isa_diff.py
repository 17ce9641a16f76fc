#!/usr/bin/env python3
"""Per-kernel comparison of two device assemblies of the same source file (hipcc <build flags> --cuda-device-only -S), e.g. of a commit and its parent:
for every kernel its register counts, scratch and static LDS on both sides, whether the whole instruction stream is identical and, if not, whether it
is identical from the kernel's entry to the end of its K loop (the last s_barrier), followed by the differing instructions.  Comment lines, the
compile-unit id and basic-block numbering are ignored.  Kernel names are demangled with llvm-cxxfilt or c++filt; --rename REGEX=REPLACEMENT (repeatable) maps
the OLD side's names onto the new ones where a kernel was renamed.  An OLD argument may name several files joined with '+' (OLDa.s+OLDb.s): their
kernels are taken together, for two files that were merged into the one NEW file; a NEW argument may do the same, for a kernel that moved from one
file to another.  Also reports the accumulator AUDIT rule of the single-stream GEMM kernels on the
NEW side: no v_accvgpr_* and no a[..] operand outside ;;#ASMSTART / ;;#ASMEND.
usage: isa_diff.py [--rename REGEX=REPLACEMENT ...] OLD.s[+OLDb.s] NEW.s[+NEWb.s] [OLD2.s NEW2.s ...] > profiles/<what>_isa.txt"""
import difflib
import os
import re
import shutil
import subprocess
import sys

FIELDS = ("sgpr_count", "vgpr_count", "agpr_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")
CXXFILT = os.environ.get("CXXFILT") or shutil.which("llvm-cxxfilt") or shutil.which("llvm-cxxfilt", path="/opt/rocm/llvm/bin") or "c++filt"


def demangle(syms):
    """{symbol: name<template args>} — return type and parameter list dropped"""
    out = subprocess.run([CXXFILT], input="\n".join(syms), capture_output=True, text=True, check=True).stdout.split("\n")
    names = {}
    for sym, full in zip(syms, out):
        full = re.sub(r"^void ", "", full)
        depth, end = 0, len(full)
        for i, ch in enumerate(full):  # the parameter list starts at the first '(' outside template brackets that does not open "(anonymous namespace)"
            depth += ch == "<"
            depth -= ch == ">"
            if ch == "(" and depth == 0 and not full.startswith("(anonymous namespace)", i):
                end = i
                break
        names[sym] = full[:end]
    return names


def kernels(path, renames=()):
    """{name: (instruction lines, {field: value}, accumulator operands outside inline asm)}"""
    text = open(path).read()
    meta = {}
    for entry in re.split(r"^  - ", text[text.index("amdhsa.kernels:"):text.index("amdhsa.target:")], flags=re.M)[1:]:
        sym = re.search(r"^    \.name:\s+(\S+)", entry, flags=re.M).group(1)
        meta[sym] = {f: int(re.search(rf"^ *\.{f}:\s+(\d+)", entry, flags=re.M).group(1)) for f in FIELDS}
    names = demangle(list(meta))
    out = {}
    for sym, m in meta.items():
        body = text[text.index(f"\n{sym}:") + len(sym) + 2:]
        body = body[: body.index(".Lfunc_end")]
        lines, in_asm, stray = [], False, 0
        for ln in body.split("\n"):
            if "#ASMSTART" in ln or "#ASMEND" in ln:
                in_asm = "#ASMSTART" in ln
                continue
            ln = re.sub(r"\s*;.*", "", ln).strip()  # comments: whole lines and trailing
            if not ln or "__hip_cuid" in ln or (ln.startswith(".") and not ln.endswith(":")):  # directives (they carry the kernel's own name)
                continue
            stray += (not in_asm) and bool(re.search(r"v_accvgpr|\ba\[?\d", ln))
            lines.append(re.sub(r"\.LBB\d+_", ".LBB_", ln))
        name = names[sym]
        for pat, repl in renames:
            name = re.sub(pat, repl, name)
        out[name] = (lines, m, stray)
    return out


def k_loop(lines):
    last = max((i for i, ln in enumerate(lines) if ln.startswith("s_barrier")), default=-1)
    return lines[: last + 1]


def main(argv):
    renames = []
    while argv and argv[0] == "--rename":
        renames.append(tuple(argv[1].split("=", 1)))
        argv = argv[2:]
    print(f"{'kernel':64s} {'identical':10s} {'to K-loop end':13s} sgpr / vgpr / agpr / spilled vgprs / scratch / static LDS   old -> new")
    bad = stray_total = count = 0
    for old_path, new_path in zip(argv[0::2], argv[1::2]):
        old, new = {}, {}
        for part in old_path.split("+"):
            old.update(kernels(part, renames))
        for part in new_path.split("+"):
            new.update(kernels(part))
        for name in sorted(set(old) | set(new)):
            if name not in old or name not in new:
                print(f"{name:64s} only in {'old' if name in old else 'new'}")
                bad += 1
                continue
            (lo, mo, _), (ln, mn, stray) = old[name], new[name]
            same, loop_same = lo == ln, k_loop(lo) == k_loop(ln)
            ops = [] if same else [o for o in difflib.SequenceMatcher(None, lo, ln, autojunk=False).get_opcodes() if o[0] != "equal"]
            moved = sum(max(i2 - i1, j2 - j1) for _, i1, i2, j1, j2 in ops if i1 <= len(k_loop(lo)))  # differ or sit elsewhere, entry .. end of the K loop
            nums = " / ".join(str(mo[f]) for f in FIELDS) + "  ->  " + " / ".join(str(mn[f]) for f in FIELDS)
            bad += (mo != mn) or not loop_same
            stray_total += stray
            count += 1
            print(f"{name:64s} {'yes' if same else 'NO':10s} {'yes' if loop_same else f'NO ({moved})':13s} {nums}{'' if mo == mn else '   COUNTS DIFFER'}")
            for _, i1, i2, j1, j2 in ops:
                print(f"    old {i1}..{i2}: " + " | ".join(lo[i1:i2]))
                print(f"    new {j1}..{j2}: " + " | ".join(ln[j1:j2]))
    print(f"\n{count} kernel(s) compared; {bad} with differing counts or a differing stream up to the end of the K loop")
    print(f"AUDIT (new side): {stray_total} instruction(s) with v_accvgpr_* or an a[..] operand outside ;;#ASMSTART / ;;#ASMEND")
    return 1 if bad or stray_total else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
