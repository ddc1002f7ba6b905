#!/usr/bin/env python3
"""Kernel by kernel comparison of two -S gfx950 listings of one translation unit (isa_kernel_stats.py counts, this one
compares): which kernels have the same instruction stream in both.  Comments and directives are dropped.  With
--normalise, two things that move without any instruction changing are masked: the numbers of local labels (.LBBn_m:
n is the function's position in the file) and the displacements of scalar loads from the kernel-argument pointer
s[0:1] (an argument struct that grew at its end moves what is passed behind it).

    python tools/isa_kernel_diff.py parent.s new.s [--normalise] [substring of the demangled name]
"""
import re
import subprocess
import sys


def bodies(path, normalise):
    out = {}
    for f in re.split(r"\n(?=_Z\w+:)", open(path).read()):
        m = re.match(r"(_Z\w+):", f)
        if not (m and "s_endpgm" in f):
            continue
        lines = [l.strip() for l in f.split(".Lfunc_end")[0].split("\n")[1:]]
        lines = [l for l in lines if l and not l.startswith((";", "."))] + [l for l in lines if l.startswith(".LBB")]
        if normalise:
            lines = [re.sub(r"\.LBB\d+_", ".LBB_", l) for l in lines]
            lines = [re.sub(r"^(s_load_\w+ \S+ s\[0:1\],) 0x[0-9a-f]+", r"\1 <kernarg>", l) for l in lines]
        out[m.group(1)] = lines
    return out


def main():
    args = [a for a in sys.argv[1:] if a != "--normalise"]
    normalise = "--normalise" in sys.argv
    a, b = bodies(args[0], normalise), bodies(args[1], normalise)
    sub = args[2] if len(args) > 2 else ""
    names = sorted(set(a) | set(b))
    dem = dict(zip(names, subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")))
    same = 0
    for n in sorted(names, key=lambda k: dem[k]):
        dn = re.sub(r"[(].*", "", dem[n].replace("pm::", ""))
        if sub not in dn:
            continue
        if n not in a or n not in b:
            print(f"only in {'the first' if n in a else 'the second'}: {dn}")
        elif a[n] == b[n]:
            same += 1
        else:
            changed = sum(x != y for x, y in zip(a[n], b[n])) + abs(len(a[n]) - len(b[n]))
            print(f"differs: {dn}; {len(a[n])} -> {len(b[n])} lines, {changed} changed")
    print(f"{same} kernels identical")


if __name__ == "__main__":
    main()
