#!/usr/bin/env python3
"""Phase timeline of the radix-4 passes of one forward 2^20 Fr transform, from the stamps of a diagnostic build
(make -C plonk-prototype_amd/csrc ntt-phase-timeline-lib, i.e. EXTRA=-DPM_DEV_STAMPS; csrc/ntt_kernels4.hip.h: ntt_stamp).

    python tools/ntt_phase_timeline.py --lib build_ab/stamps/libplonk_mi355x.so [--prio V] [--log-n 20] > profiles/FILE.txt

After a short warm-up without stamps, ONE transform runs with a stamp buffer.  Lane 0 of every wave has left s_memtime and
s_memrealtime at kernel entry, when its entry loads were back, in every step after its LDS reads, after its last product and
after its second barrier, and after its last store was issued, together with HW_ID and XCC_ID.  From those the waves are put
on their CUs and SIMDs and the workgroups of a CU are paired, the older being the one that entered first.  Reported per pass
role, as the distribution over CUs (min / median / 90 % / max, shader cycles):
  (a) when the older and the younger workgroup finish each step, counted from the older one's entry;
  (b) the younger one's lag at each step, in cycles and in steps it is behind when the older one finishes that step;
  (c) how long the last workgroup of a CU runs with no co-resident partner;
  (d) the in-kernel clock, Δs_memtime / Δs_memrealtime x 100 MHz.
The stamps perturb the kernel (each one drains the scalar and LDS counters): this is evidence about ORDER, not a timing."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

WORDS = 40   # NTT_STAMP_WORDS


def dist(v):
    v = np.asarray(v, dtype=np.float64)
    if v.size == 0:
        return "      -       -       -       -"
    return " ".join(f"{x:7.0f}" for x in (v.min(), np.median(v), np.percentile(v, 90), v.max()))


def report(name, st, nsteps):
    st = st[st[:, 0] != 0]                       # waves that stamped
    k_end = 2 + 3 * nsteps
    t = st[:, 0:2 * (k_end + 1):2].astype(np.int64)
    r = st[:, 1:2 * (k_end + 1):2].astype(np.int64)
    hw, xcc = st[:, 36] & 0xFFFFFFFF, st[:, 36] >> 32
    block = (st[:, 37] & 0xFFFFFFFF).astype(np.int64)
    cu = ((xcc.astype(np.int64) << 8) | (((hw >> 12) & 15).astype(np.int64) << 4) | ((hw >> 8) & 15).astype(np.int64))
    simd = ((hw >> 4) & 3).astype(np.int64)
    print(f"== {name}: {st.shape[0]} waves, {len(np.unique(block))} workgroups of {st.shape[0] // len(np.unique(block))} waves, {len(np.unique(cu))} CUs, "
          f"{nsteps} steps")
    per_simd = np.unique(cu * 4 + simd, return_counts=True)[1]
    print(f"   waves per SIMD over the launch: min {per_simd.min()} median {int(np.median(per_simd))} max {per_simd.max()}")
    # (d) clock, per wave over the whole kernel
    dr = r[:, k_end] - r[:, 0]
    ok = dr > 0
    clk = (t[ok, k_end] - t[ok, 0]) / dr[ok] * 100.0
    print(f"   (d) in-kernel clock, MHz: median {np.median(clk):.0f}  (5 % {np.percentile(clk, 5):.0f}, 95 % {np.percentile(clk, 95):.0f});"
          f" a wave's kernel: median {np.median(t[:, k_end] - t[:, 0]):.0f} cycles = {np.median(dr) / 100.0:.2f} us")
    # per workgroup: entry = first wave in, step s finished = its last wave past the step's second barrier (last step: stores issued)
    fin_idx = [2 + 3 * s + 2 for s in range(nsteps - 1)] + [k_end]
    wgs = {}
    for b in np.unique(block):
        m = block == b
        cus = np.unique(cu[m])
        if len(cus) != 1:
            continue
        wgs[b] = (int(cus[0]), int(t[m, 0].min()), np.array([int(t[m, k].max()) for k in fin_idx]))
    by_cu = {}
    for b, (c, start, fin) in wgs.items():
        by_cu.setdefault(c, []).append((start, fin))
    counts = np.unique([len(v) for v in by_cu.values()], return_counts=True)
    print("   workgroups per CU: " + ", ".join(f"{n} on {c} CUs" for n, c in zip(*counts)))
    older, younger, lag, behind, tail, span, entry_gap = [], [], [], [], [], [], []
    for c, v in by_cu.items():
        if len(v) != 2:
            continue
        v.sort(key=lambda e: e[0])
        (s0, f0), (s1, f1) = v
        if s1 >= f0[-1]:
            continue                              # one after the other: not co-resident
        older.append(f0 - s0)
        younger.append(f1 - s0)
        lag.append(f1 - f0)
        behind.append([s + 1 - int((f1 <= f0[s]).sum()) for s in range(nsteps)])
        tail.append(abs(int(f1[-1]) - int(f0[-1])))
        span.append(max(f0[-1], f1[-1]) - s0)
        entry_gap.append(s1 - s0)
    older, younger, lag, behind = (np.array(x) for x in (older, younger, lag, behind))
    print(f"   paired CUs (two co-resident workgroups): {len(tail)};  the younger enters behind the older by {dist(entry_gap)}")
    print("   cycles from the older workgroup's entry          min  median    90 %     max")
    for s in range(nsteps):
        print(f"   (a) step {s} finished, older                  {dist(older[:, s])}")
        print(f"   (a) step {s} finished, younger                {dist(younger[:, s])}")
        print(f"   (b) step {s} lag of the younger, cycles       {dist(lag[:, s])}")
        print(f"   (b) step {s} steps the younger is behind      " + " ".join(f"{x:7.2f}" for x in (
            behind[:, s].min(), np.mean(behind[:, s]), np.percentile(behind[:, s], 90), behind[:, s].max())) + "   (min mean 90 % max)")
    print(f"   (c) last workgroup alone on its CU, cycles    {dist(tail)}")
    print(f"   (c) ... as a share of the CU's busy span, %   " + " ".join(f"{x:7.1f}" for x in (
        np.min(np.array(tail) / span * 100), np.median(np.array(tail) / span * 100), np.percentile(np.array(tail) / span * 100, 90),
        np.max(np.array(tail) / span * 100))))
    print(f"   CU busy span (older entry to last store issued) {dist(span)}")
    # where a wave's time goes: the three parts of a step, median over waves
    parts = []
    for s in range(nsteps):
        a, b = 2 + 3 * s, 2 + 3 * s + 1
        prev = 1 if s == 0 else 2 + 3 * (s - 1) + 2
        seg = [np.median(t[:, a] - t[:, prev]), np.median(t[:, b] - t[:, a])]
        if s < nsteps - 1:
            seg.append(np.median(t[:, b + 1] - t[:, b]))
        parts.append("/".join(f"{x:.0f}" for x in seg))
    print(f"   a wave's entry loads: median {np.median(t[:, 1] - t[:, 0]):.0f} cycles; steps (LDS reads / products / exchange): "
          + "  ".join(parts) + f";  stores {np.median(t[:, k_end] - t[:, k_end - 2]):.0f}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", default=None, help="the stamped build of the library (default: PM_LIB_PATH or the tree's)")
    ap.add_argument("--prio", type=int, default=None, help="value of the option ntt_step_prio (default: the library's)")
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=50)
    args = ap.parse_args()
    if args.lib:
        os.environ["PM_LIB_PATH"] = os.path.abspath(args.lib)
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import plonk_prototype_amd as pa
    from plonk_prototype_amd import _lib

    lib = _lib.load()
    if not hasattr(lib, "pm_dev_ntt_stamps"):
        sys.exit("this library has no stamps: build it with EXTRA=-DPM_DEV_STAMPS")
    lib.pm_dev_ntt_stamps.restype = C.c_int
    lib.pm_dev_ntt_stamps.argtypes = [C.c_void_p, C.c_size_t]
    k = args.log_n
    n = 1 << k
    plan = (C.c_uint32 * 4)()
    npass = C.c_uint32(0)
    assert lib.pm_ntt_plan(k, plan, C.byref(npass)) == 0
    radices = list(plan)[: npass.value]
    ctx = pa.Context(0)
    if args.prio is not None:
        ctx.set_option("ntt_step_prio", args.prio)
    rng = np.random.default_rng(7)
    a = torch.from_numpy(rng.integers(0, 1 << 62, size=(n, 4), dtype=np.uint64).view(np.int64)).cuda()
    b = torch.empty_like(a)
    for _ in range(args.warmup):
        ctx.fr_ntt_dev(a.data_ptr(), n, b.data_ptr(), k, 0)
    ctx.sync()
    waves = n // 4 // 64                         # a thread keeps four elements
    buf = torch.zeros((len(radices), waves, WORDS), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert lib.pm_dev_ntt_stamps(C.c_void_p(buf.data_ptr()), len(radices) * waves) == 0
    ctx.fr_ntt_dev(a.data_ptr(), n, b.data_ptr(), k, 0)
    ctx.sync()
    assert lib.pm_dev_ntt_stamps(None, 0) == 0
    st = buf.cpu().numpy().view(np.uint64)
    print(f"# one forward 2^{k} transform, passes {radices}, ntt_step_prio = {args.prio if args.prio is not None else 'default'}, "
          f"after {args.warmup} unstamped transforms; shader cycles")
    roles = ["single"] if len(radices) == 1 else ["first"] + ["middle"] * (len(radices) - 2) + ["last"]
    for i, (S, role) in enumerate(zip(radices, roles)):
        report(f"pass {i} ({role}, radix 2^{S})", st[i], (S + 1) // 2)
    ctx.close()


if __name__ == "__main__":
    main()
