#!/usr/bin/env python3
"""Kernel-by-kernel comparison of two `hipcc --cuda-device-only -S` listings of sa_gemm.hip: the listing of a commit whose kernels
carried the main loop as one integer code (OLD) against one whose kernels carry the loop kind and the k-group count — the distance
matrix's also which operands it reads in fragment order — (NEW).
One line per kernel: old name, new name, `identical` / `DIFFERENT`, instructions.  Identical = the instruction text and the
.amdhsa_* block are the same once the kernel's own symbol and the listing's basic-block numbering are replaced by placeholders.

    python scripts/kernel_identity.py OLD.s NEW.s > profiles/r10_kernel_identity.txt      (exit status 1 on any difference)
"""
import re
import subprocess
import sys

LOOPS = ("staged", "ring", "ksplit", "direct", "ks128")   # SaLoop (sa_tile_plan.h)


def kernels(path):
    """{demangled name: (instructions + .amdhsa block, instruction count)}"""
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^\t\.amdhsa_kernel (\S+)\n(.*?)^\t\.end_amdhsa_kernel", text, re.M | re.S):
        sym, hsa = m.group(1), m.group(2)
        body = re.search(r"^%s:.*?\n(.*?)^\.Lfunc_end" % re.escape(sym), text, re.M | re.S).group(1)
        lines = [l for l in (re.sub(r"\s*;.*$", "", l) for l in body.split("\n")) if l.strip()]   # (the listing's comments name blocks by number)
        norm = re.sub(r"\.LBB\d+_", ".LBB_", "\n".join(lines) + "\n" + hsa).replace(sym, "<kernel>")
        n = sum(1 for l in lines if re.match(r"\t[a-z]", l))
        out[sym] = (norm, n)
    names = subprocess.run(["c++filt"], input="\n".join(out), capture_output=True, text=True, check=True).stdout.split("\n")
    short = lambda d: re.sub(r"^void ", "", d[:d.rindex(">") + 1] if ">" in d else d[:d.index("(")])   # (without the parameter list)
    return {short(d): v for d, v in zip(names, out.values())}


def renamed(old):
    """The new name of an old kernel: the integer code spelled out as (loop, k-groups); k_frame_visual loses its leading 1."""
    m = re.match(r"(k_visual_cosine|k_cosine_matrix)<(\d+), (\d+), (\d+)(.*)>$", old)
    if m:
        k, code = m.group(1), int(m.group(4))
        loop, kg = {0: ("ring", 1), 9: ("ksplit", 1), 10: ("ksplit", 1), 13: ("ksplit", 1), 15: ("direct", 1), 17: ("ks128", 1)}.get(code, ("staged", code))
        frag = "" if k == "k_visual_cosine" else ", %s, %s" % (str(code in (10, 13, 15, 17)).lower(), str(code == 13).lower())   # B, A in fragment order
        return "%s<%s, %s, (SaLoop)%d, %d%s%s>" % (k, m.group(2), m.group(3), LOOPS.index(loop), kg, frag, m.group(5))
    return re.sub(r"^k_frame_visual<1, ", "k_frame_visual<", old)


def with_tail(name):
    """k_frame_visual before it had the TAIL parameter (six arguments) -> the same form of the seven-argument kernel."""
    m = re.match(r"k_frame_visual<([^<>]*)>$", name)
    return "k_frame_visual<%s, false>" % m.group(1) if m and m.group(1).count(",") == 5 else name


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = len(old) != len(new)
    print("# %d kernels in %s, %d in %s" % (len(old), sys.argv[1].split("/")[-1], len(new), sys.argv[2].split("/")[-1]))
    left = set(new)
    for o in sorted(old):
        n = renamed(o)
        if n not in left:
            n = with_tail(n)
        if n not in left:
            print(o, "->", "MISSING")
            bad = True
            continue
        left.discard(n)
        same = old[o][0] == new[n][0]
        bad |= not same
        print("%s -> %s %s %d" % (o, n, "identical" if same else "DIFFERENT", new[n][1]))
    for n in sorted(left):
        print("NEW ONLY", n)
        bad = True
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
