#!/usr/bin/env python3
"""Per-kernel comparison of two device assemblies of csrc/vae.hip or csrc/vae16g.hip (hipcc <build flags> --cuda-device-only -S): for every kernel its
register counts, scratch and static LDS on both sides, whether the whole instruction stream is identical and, if not, whether it is identical from the
kernel's entry to the end of its K loop (the last s_barrier; else the number of instructions that differ or moved).  Comment lines, the compile-unit id and basic-block numbering are ignored; the per-tap
kernels' names of before the merge (vae_conv_kernel<NF, KC>, vae_conv16_kernel<NF>) are mapped onto vae_conv_kernel<OP, NF, KC>.
usage: vae_conv_isa_diff.py OLD.s NEW.s [OLD2.s NEW2.s ...] > profiles/vae_conv_refactor_isa.txt"""
import difflib
import re
import sys

FIELDS = ("sgpr_count", "vgpr_count", "agpr_count", "private_segment_fixed_size", "group_segment_fixed_size")


def canonical(sym):
    """_ZN3x2v<len><name>[I<template args>E]... -> name<args> (Itanium mangling of int / float / _Float16 template arguments only)"""
    m = re.match(r"_ZN3x2v(\d+)", sym)
    name, rest = sym[m.end():][: int(m.group(1))], sym[m.end() + int(m.group(1)):]
    if rest.startswith("I"):
        args = re.findall(r"Li(\d+)E|(f)|(DF16_)", re.match(r"I((?:Li\d+E|f|DF16_)+)E", rest).group(1))
        name += "<" + ", ".join(i or ("float" if f else "_Float16") for i, f, h in args) + ">"
    name = re.sub(r"^vae_conv_kernel<(\d), (\d+)>", r"vae_conv_kernel<float, \1, \2>", name)
    return re.sub(r"^vae_conv16_kernel<(\d)>", r"vae_conv_kernel<_Float16, \1, 64>", name)


def kernels(path):
    """{canonical name: (instruction lines, {field: value})}"""
    text = open(path).read()
    meta = {}
    for entry in re.split(r"^  - ", text[text.index("amdhsa.kernels:"):text.index("amdhsa.target:")], flags=re.M)[1:]:
        sym = re.search(r"^    \.name:\s+(\S+)", entry, flags=re.M).group(1)
        meta[sym] = {f: int(re.search(rf"^ *\.{f}:\s+(\d+)", entry, flags=re.M).group(1)) for f in FIELDS}
    out = {}
    for sym, m in meta.items():
        body = text[text.index(f"\n{sym}:") + len(sym) + 2:]
        body = body[: body.index(".Lfunc_end")]
        lines = []
        for ln in body.split("\n"):
            ln = re.sub(r"\s*;.*", "", ln).strip()  # comments: whole lines and trailing
            if not ln or "__hip_cuid" in ln or (ln.startswith(".") and not ln.endswith(":")):  # directives (they carry the kernel's own name)
                continue
            lines.append(re.sub(r"\.LBB\d+_", ".LBB_", ln))
        out[canonical(sym)] = (lines, m)
    return out


def k_loop(lines):
    last = max((i for i, ln in enumerate(lines) if ln.startswith("s_barrier")), default=-1)
    return lines[: last + 1]


def main(argv):
    print(f"{'kernel':52s} {'identical':10s} {'to K-loop end':13s} sgpr / vgpr / agpr / scratch / static LDS   old -> new")
    bad = 0
    for old_path, new_path in zip(argv[0::2], argv[1::2]):
        old, new = kernels(old_path), kernels(new_path)
        for name in sorted(set(old) | set(new)):
            if name not in old or name not in new:
                print(f"{name:52s} only in {'old' if name in old else 'new'}")
                bad += 1
                continue
            (lo, mo), (ln, mn) = old[name], new[name]
            same, loop_same = lo == ln, k_loop(lo) == k_loop(ln)
            ops = [] if loop_same else [o for o in difflib.SequenceMatcher(None, k_loop(lo), k_loop(ln), autojunk=False).get_opcodes() if o[0] != "equal"]
            moved = sum(max(i2 - i1, j2 - j1) for _, i1, i2, j1, j2 in ops)  # instructions that differ or sit elsewhere, entry .. end of the K loop
            nums = " / ".join(str(mo[f]) for f in FIELDS) + "  ->  " + " / ".join(str(mn[f]) for f in FIELDS)
            bad += (mo != mn) or not loop_same
            print(f"{name:52s} {'yes' if same else 'NO':10s} {'yes' if loop_same else f'NO ({moved})':13s} {nums}{'' if mo == mn else '   COUNTS DIFFER'}")
    print(f"\n{bad} kernel(s) with differing counts or a differing stream up to the end of the K loop")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
