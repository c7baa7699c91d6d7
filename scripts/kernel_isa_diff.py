#!/usr/bin/env python3
"""usage: scripts/kernel_isa_diff.py A/libstage_hip.so B/libstage_hip.so

Compares the gfx950 device code of two built libraries symbol by symbol: the text of
`llvm-objdump -d` and the kernel descriptor fields of the code objects' metadata.  What depends
on where the linker put a function is taken out of the text: addresses and encodings, the
padding after a function's last instruction, and a pc-relative offset to another function
(replaced by that function's name).  A device function whose name changed but whose body did not
-- a symbol only in A and one only in B with equal text -- is paired, and B's name is read as A's
in the callers.  Prints one line per symbol -- same, same (renamed), differs (n lines), only in A,
only in B -- then every descriptor field that differs, and exits 1 if anything but a rename does.
Text only: it says whether two builds hold the same instructions, not what they are."""
import difflib
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "tests"), os.path.join(REPO, "stage-indexorganized_amd")]
from test_dispatch_rule import LLVM, gfx950_code_objects  # noqa: E402
from test_probe_form_rule import kernels  # noqa: E402


def functions(co):
    """symbol -> its disassembly lines, placement-independent (see above)"""
    with tempfile.NamedTemporaryFile(suffix=".o") as f:
        f.write(co)
        f.flush()
        text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", f.name], check=True,
                              capture_output=True, text=True).stdout
    starts = {int(m.group(1), 16): m.group(2) for m in re.finditer(r"^([0-9a-f]+) <(.+)>:$", text, re.M)}
    out, cur, pc = {}, None, None
    for line in text.splitlines():
        m = re.match(r"[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur, pc = out.setdefault(m.group(1), []), None
            continue
        if cur is None or not line.strip():
            continue
        ins, _, where = line.partition("//")
        ins = ins.strip()
        lit = re.search(r"0x[0-9a-f]+$", ins)
        if pc is not None and lit:  # an offset from the pc just read: name the function it reaches
            ins = ins[:lit.start()] + starts.get((pc + int(lit.group(), 16)) & 0xFFFFFFFF, "pc+" + lit.group())
        pc = int(where.split(":")[0], 16) + 4 if ins.startswith("s_getpc_b64") else None
        cur.append(ins)
    for body in out.values():  # the padding between functions and at the end of a code object
        while body and body[-1] in ("s_nop 0", "..."):
            body.pop()
    return out


def library(path):
    """symbol -> [disassembly per code object holding it], kernel name -> descriptor fields"""
    funcs, descs = {}, {}
    for co in gfx950_code_objects(path):
        for name, body in functions(co).items():
            funcs.setdefault(name, []).append(body)
        descs.update(kernels(co))
    return {k: sorted(v) for k, v in funcs.items()}, descs


def pair_renamed(fa, fb):
    """A's name -> B's name of the one-sided symbols with equal bodies; fb's callers then name A's"""
    pairs = {}
    while True:
        new = {}
        for nb in sorted(set(fb) - set(fa)):
            na = next((n for n in sorted(set(fa) - set(fb)) if n not in new and fa[n] == fb[nb]), None)
            if na is not None:
                new[na] = nb
        if not new:
            return pairs
        back = {nb: na for na, nb in new.items()}
        for name, bodies in list(fb.items()):  # a call ends in the callee's name (functions())
            fb[back.get(name, name)] = sorted(
                [next((ins[:-len(nb)] + na for nb, na in back.items() if ins.endswith(nb)), ins) for ins in body]
                for body in bodies)
            if name in back:
                del fb[name]
        pairs.update(new)


def main(a, b):
    (fa, da), (fb, db) = library(a), library(b)
    renamed = pair_renamed(fa, fb)
    changed = 0
    for name in sorted(set(fa) | set(fb)):
        if name in renamed:
            print(f"{'same (renamed)':12s} {name} -> {renamed[name]}")
            continue
        if name not in fb or name not in fa:
            verdict = "only in A" if name in fa else "only in B"
        elif fa[name] == fb[name]:
            verdict = "same"
        else:
            la, lb = sum(fa[name], []), sum(fb[name], [])
            n = sum(1 for d in difflib.unified_diff(la, lb, lineterm="", n=0) if d[0] in "+-" and d[:3] not in ("+++", "---"))
            verdict = f"differs ({n} lines of {len(la)} / {len(lb)})"
        changed += verdict != "same"
        print(f"{verdict:12s} {name}")
    for name in sorted(set(da) & set(db)):
        for k in sorted(set(da[name]) | set(db[name])):
            if da[name].get(k) != db[name].get(k):
                changed += 1
                print(f"descriptor   {name} {k}: {da[name].get(k)} -> {db[name].get(k)}")
    print(f"{len(set(fa) | set(fb))} symbols, {len(set(da) | set(db))} kernel descriptors, {changed} differences")
    return 1 if changed else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
