#!/usr/bin/env python3
"""Whole-kernel static counts from a -S / -save-temps gfx950 listing: for every kernel whose demangled name contains
the given substring, the number of v_mad_u64_u32, of VALU instructions (v_*), of s_load_* and the .vgpr_count /
.sgpr_count / scratch bytes of its metadata.  (isa_count.py counts the timed loop of a micro-benchmark; the pass
kernels are straight-line code with untaken branches, so the whole body is what can be compared between builds.)

    python tools/isa_kernel_stats.py build/ntt4-hip-amdgcn-amd-amdhsa-gfx950.s 'ntt_pass4_kernel<10, 1,'
"""
import re
import subprocess
import sys


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return dict(zip(names, out))


def main():
    path, sub = sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else ""
    text = open(path).read()
    bodies = {}
    for f in re.split(r"\n(?=_Z\w+:)", text):
        m = re.match(r"(_Z\w+):", f)
        if m and "s_endpgm" in f:
            bodies[m.group(1)] = f.split(".Lfunc_end")[0]
    meta = {}
    for blk in re.split(r"\n  - \.agpr_count:", text)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        if not name:
            continue
        get = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))
        meta[name.group(1)] = (get("vgpr_count"), get("sgpr_count"), get("private_segment_fixed_size"))
    names = demangle(sorted(bodies))
    print("# kernel; v_mad_u64_u32; VALU; s_load; vgpr_count; sgpr_count; scratch_bytes")
    for mangled in sorted(bodies, key=lambda k: names[k]):
        dn = names[mangled].replace("pm::", "").replace("(anonymous namespace)::", "")
        if sub not in dn or mangled not in meta:
            continue
        ops = re.findall(r"^\s+([vs]_\w+)", bodies[mangled], re.M)
        mads = sum(o == "v_mad_u64_u32" for o in ops)
        valu = sum(o.startswith("v_") for o in ops)
        sld = sum(o.startswith("s_load_") for o in ops)
        vg, sg, scr = meta[mangled]
        print(f"{re.sub(r'[(].*', '', dn)}; {mads}; {valu}; {sld}; {vg}; {sg}; {scr}")


if __name__ == "__main__":
    main()
