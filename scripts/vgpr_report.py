"""Register report of the kernels in a device assembly file:
    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S -I include -o k.s csrc/probe.hip
    python scripts/vgpr_report.py k.s [name-substring]
prints VGPRs, SGPRs, SGPR spills into VGPR lanes (v_writelane) and scratch use per kernel --
the probe's occupancy hinges on it (5 waves/SIMD up to 96 VGPRs, 3 at 154).

Comparison of two builds (a refactor that must leave the generated code alone):
    python scripts/vgpr_report.py --compare old.s new.s [name-substring]
pairs the functions of both files by name, and the ones whose name exists in one file only
(a kernel whose template parameters changed) by content, and prints per function whether the
instruction text is the same -- comments dropped, local label numbers and the function's own
symbol normalised -- with the VGPR / SGPR / scratch / LDS numbers of both builds.  Exit status
1 when a paired function differs or a function is left unpaired."""
import re
import sys
from collections import defaultdict

KEYS = ("num_vgpr", "numbered_sgpr", "private_seg_size")


def functions(src):
    """name -> text from the function's label to its .Lfunc_end (for a kernel that includes
    its descriptor)"""
    out = {}
    for m in re.finditer(r"^(_Z\S+):\s*;\s*@", src, re.M):
        out[m.group(1)] = src[m.end():src.find(".Lfunc_end", m.end())]
    return out


def meta(src, name, key):
    r = re.search(r"\.set " + re.escape(name) + r"\." + key + r", (\d+)", src)
    return r.group(1) if r else "?"


def lds(body):
    r = re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", body)
    return r.group(1) if r else "-"  # not a kernel


def normalised(name, body):
    lines = []
    for ln in body.replace(name, "SELF").splitlines():
        ln = ln.split(";", 1)[0].rstrip()
        if ln:
            lines.append(re.sub(r"\.L([A-Za-z_]+)\d+_", r".L\1_", ln))
    return "\n".join(lines)


def report(path, pat):
    src = open(path).read()
    for name, body in functions(src).items():
        if pat not in name:
            continue
        print(f"{name[:70]:70s} vgpr {meta(src, name, 'num_vgpr'):>4s} sgpr {meta(src, name, 'numbered_sgpr'):>4s} "
              f"writelane {body.count('v_writelane_b32'):4d} scratch {meta(src, name, 'private_seg_size'):>4s}")


def compare(path_a, path_b, pat):
    src = [open(path_a).read(), open(path_b).read()]
    fn = [functions(s) for s in src]

    def numbers(side, name):
        return tuple(meta(src[side], name, k) for k in KEYS) + (lds(fn[side][name]),)

    pairs = [(n, n) for n in fn[0] if n in fn[1]]
    only = [[n for n in fn[side] if n not in fn[1 - side]] for side in (0, 1)]
    # renamed functions: the same normalised text under another name
    by_text = defaultdict(list)
    for n in only[1]:
        by_text[normalised(n, fn[1][n])].append(n)
    left = []
    for n in only[0]:
        same = by_text.get(normalised(n, fn[0][n]))
        if same:
            pairs.append((n, same.pop(0)))
        else:
            left.append(n)
    unpaired_b = [n for names in by_text.values() for n in names]
    ident = differ = 0
    for a, b in pairs:
        if pat not in a and pat not in b:
            continue
        same = normalised(a, fn[0][a]) == normalised(b, fn[1][b])
        ident += same
        differ += not same
        na, nb = numbers(0, a), numbers(1, b)
        line = f"{'same' if same else 'DIFF':4s} {a[:90]:90s} vgpr/sgpr/scratch/lds {'/'.join(na)}"
        if nb != na:
            line += f" -> {'/'.join(nb)}"
        if a != b:
            line += f"\n     renamed to {b}"
        if not same or a != b or pat:
            print(line)
    for side, names in ((0, left), (1, unpaired_b)):
        for n in names:
            if pat in n:
                print(f"only in {(path_a, path_b)[side]}: {n}  vgpr/sgpr/scratch/lds {'/'.join(numbers(side, n))}")
    nl = sum(pat in n for n in left)
    nr = sum(pat in n for n in unpaired_b)
    kern = [sum(lds(b) != "-" for b in f.values()) for f in fn]
    print(f"{len(fn[0])} functions ({kern[0]} kernels) in {path_a}, {len(fn[1])} ({kern[1]}) in {path_b}: "
          f"{ident} identical ({sum(a != b for a, b in pairs)} of the pairs under a new name), {differ} differ, "
          f"{nl} only in the first, {nr} only in the second")
    return 1 if differ or nl or nr else 0


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3], sys.argv[4] if len(sys.argv) > 4 else ""))
    report(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else "")
