#!/usr/bin/env python3
"""Compare the device code of two -S outputs of hipfeat.hip kernel by kernel (no GPU needed): the gate of a refactor that must not
change what the kernels compile to.  Build both with the compile line of tools/isa_hist.py (add the experiment macro under test):

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -DHIPFEAT_BUILD -Iinclude --cuda-device-only -S lhotse_amd/csrc/hipfeat.hip -o /tmp/hf.s
    python tools/isa_diff.py /tmp/parent.s /tmp/branch.s [-v]

A kernel's text runs from its label to .Lfunc_end; comments and blank lines are dropped and the numbered local labels (.LBB<n>_<m>,
.Ltmp<n>, .Lfunc_end<n>) become fixed tokens, since their numbers count functions of the whole file.  The .amdhsa_* descriptor lines
(registers, LDS, scratch) are compared separately.  Exit status 1 if any kernel differs or exists on one side only; -v prints a diff.
"""
import difflib, re, sys

LABEL = re.compile(r"\.LBB\d+_(\d+)|\.Ltmp\d+|\.Lfunc_(?:begin|end)\d+")


def norm(line):
    line = line.split(";", 1)[0].rstrip()
    return LABEL.sub(lambda m: ".LBB_" + m.group(1) if m.group(1) else m.group(0).rstrip("0123456789"), line)


def kernels(path):
    """name -> (instruction lines, descriptor lines)"""
    lines = open(path).read().split("\n")
    names = [m.group(1) for l in lines if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l))]
    start = {m.group(1): i for i, l in enumerate(lines) if (m := re.match(r"([A-Za-z_$][\w$.]*):", l))}
    desc_at = {m.group(1): i for i, l in enumerate(lines) if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l))}
    out = {}
    for name in names:
        a = start[name]
        b = next(i for i in range(a, len(lines)) if lines[i].startswith(".Lfunc_end"))
        d = desc_at[name]
        e = next(i for i in range(d, len(lines)) if ".end_amdhsa_kernel" in lines[i])
        out[name] = ([t for l in lines[a:b] if (t := norm(l)).strip()], [l.strip() for l in lines[d + 1:e] if ".amdhsa_" in l])
    return out


verbose = "-v" in sys.argv
pa, pb = [a for a in sys.argv[1:] if a != "-v"]
A, B = kernels(pa), kernels(pb)
bad = 0
for name in sorted(set(A) | set(B)):
    if name not in A or name not in B:
        print(f"ONLY IN {pb if name in B else pa}: {name}")
        bad += 1
        continue
    text, desc = A[name][0] == B[name][0], A[name][1] == B[name][1]
    if not (text and desc):
        bad += 1
        print(f"DIFFERS ({'text ' if not text else ''}{'descriptor' if not desc else ''}): {name}  [{len(A[name][0])} -> {len(B[name][0])} lines]")
        if verbose:
            for k in (0, 1):
                print("\n".join(list(difflib.unified_diff(A[name][k], B[name][k], "parent", "branch", lineterm="", n=2))[:80]))
print(f"{len(set(A) | set(B))} kernels compared: {len(set(A) | set(B)) - bad} identical in instruction text and descriptors, {bad} not")
sys.exit(1 if bad else 0)
