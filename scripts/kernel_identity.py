#!/usr/bin/env python3
"""Kernel-by-kernel comparison of two `hipcc --cuda-device-only -S` listings of one source file (sa_gemm.hip, sa_search.hip,
sa_gallery.hip, sa_upkeep.hip): the listing of an older commit (OLD) against one in which kernels were renamed (NEW).  renamed() knows the renames so far:
the contraction's main loop, once one integer code, as the loop kind and the k-group count — the distance matrix's also which operands
it reads in fragment order —, the track search's kernels, once one name per form, as template arguments (TRACK_SEARCH), and the
frame-preprocessing kernels (FRAMES), whose *_set forms took the plain names when the single-scene kernels of those names were retired:
an old kernel whose name a renamed one takes over is listed as RETIRED and compared with nothing.
One line per kernel: old name, new name, `identical` / `DIFFERENT`, instructions.  Identical = the instruction text and the
.amdhsa_* block are the same once the kernel's own symbol and the listing's basic-block numbering are replaced by placeholders
(section directives are left out: a template's code lies in a section named after it).

    python scripts/kernel_identity.py OLD.s NEW.s > profiles/r12_kernel_identity_gemm.txt      (exit status 1 on any difference)
"""
import re
import subprocess
import sys

LOOPS = ("staged", "ring", "ksplit", "direct", "ks128")   # SaLoop (sa_tile_plan.h)

# track search: one kernel template per job (k_search_tile<EU, JOIN, COMPAT>, k_topn<JOIN>, k_gather<ATTRS>) where each form had a name
_B = ("false", "true")
TRACK_SEARCH = {"k_%s_%s%s" % (("search", "join")[j], ("cosine", "euclid")[e], ("", "_compat")[c]): "k_search_tile<%s, %s, %s>" % (_B[e], _B[j], _B[c])
                for e in (0, 1) for j in (0, 1) for c in (0, 1)}
TRACK_SEARCH.update({"k_search_topn": "k_topn<false>", "k_join_topn": "k_topn<true>",
                     "k_gather_queries": "k_gather<>", "k_gather_queries_attrs": "k_gather<sa_track_attrs const, sa_track_attrs>"})

# frame preprocessing: the segment-table forms are the only forms (k_nms_sweep_set<S> -> k_nms_sweep<S>)
FRAMES = ("k_nms_mask", "k_nms_sweep", "k_own_area", "k_own_area_big")


def kernels(path):
    """{demangled name: (instructions + .amdhsa block, instruction count)}"""
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^\t\.amdhsa_kernel (\S+)\n(.*?)^\t\.end_amdhsa_kernel", text, re.M | re.S):
        sym, hsa = m.group(1), m.group(2)
        body = re.search(r"^%s:.*?\n(.*?)^\.Lfunc_end" % re.escape(sym), text, re.M | re.S).group(1)
        lines = [l for l in (re.sub(r"\s*;.*$", "", l) for l in body.split("\n")) if l.strip()]   # (the listing's comments name blocks by number)
        lines = [l for l in lines if not re.match(r"\t\.(text|section)\b", l)]   # (a template's code lies in a section of its own name)
        norm = re.sub(r"\.LBB\d+_", ".LBB_", "\n".join(lines) + "\n" + hsa).replace(sym, "<kernel>")
        n = sum(1 for l in lines if re.match(r"\t[a-z]", l))
        out[sym] = (norm, n)
    names = subprocess.run(["c++filt"], input="\n".join(out), capture_output=True, text=True, check=True).stdout.split("\n")

    def short(d):   # without the parameter list: up to the bracket that pairs with the last one (a parameter may be a template itself)
        depth = 0
        for i in range(len(d) - 1, -1, -1):
            depth += (d[i] == ")") - (d[i] == "(")
            if depth == 0:
                return re.sub(r"^void ", "", d[:i])
    return {short(d): v for d, v in zip(names, out.values())}


def renamed(old):
    """The new name of an old kernel: the integer code spelled out as (loop, k-groups); k_frame_visual loses its leading 1; the track
    search's names (inside or outside an anonymous namespace) from TRACK_SEARCH; the frame-preprocessing kernels lose their _set."""
    m = re.match(r"(k_visual_cosine|k_cosine_matrix)<(\d+), (\d+), (\d+)(.*)>$", old)
    if m:
        k, code = m.group(1), int(m.group(4))
        loop, kg = {0: ("ring", 1), 9: ("ksplit", 1), 10: ("ksplit", 1), 13: ("ksplit", 1), 15: ("direct", 1), 17: ("ks128", 1)}.get(code, ("staged", code))
        frag = "" if k == "k_visual_cosine" else ", %s, %s" % (str(code in (10, 13, 15, 17)).lower(), str(code == 13).lower())   # B, A in fragment order
        return "%s<%s, %s, (SaLoop)%d, %d%s%s>" % (k, m.group(2), m.group(3), LOOPS.index(loop), kg, frag, m.group(5))
    ns, bare = re.match(r"(\(anonymous namespace\)::)?(.*)$", old).groups()
    if bare in TRACK_SEARCH:
        return (ns or "") + TRACK_SEARCH[bare]
    m = re.match(r"(\w+)_set(<\d+>)?$", old)
    if m and m.group(1) in FRAMES:
        return m.group(1) + (m.group(2) or "")
    return re.sub(r"^k_frame_visual<1, ", "k_frame_visual<", old)


def with_tail(name):
    """k_frame_visual before it had the TAIL parameter (six arguments) -> the same form of the seven-argument kernel."""
    m = re.match(r"k_frame_visual<([^<>]*)>$", name)
    return "k_frame_visual<%s, false>" % m.group(1) if m and m.group(1).count(",") == 5 else name


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    retired = {renamed(o) for o in old if renamed(o) != o} & set(old)   # old kernels whose names now belong to renamed ones
    bad = len(old) - len(retired) != len(new)
    print("# %d kernels in %s, %d in %s" % (len(old), sys.argv[1].split("/")[-1], len(new), sys.argv[2].split("/")[-1]))
    left = set(new)
    for o in sorted(old):
        if o in retired:
            print(o, "->", "RETIRED")
            continue
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
