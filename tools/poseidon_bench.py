#!/usr/bin/env python3
"""Native Poseidon: permutations per second of pm_hades_permute_dev at dusk's size (67 rounds, 8 full,
one matrix) in the THREAD form, the WAVE form and AUTO, and an arity-4 Merkle tree of height 10 end to end.  A developer tool:
one GPU, one process.

For n = 1, 2^6, 2^10, 2^14, 2^18 and 2^20 random states, permuted in place (a permuted state is a valid input again).  Before
anything is timed, 64 states are compared with pm_hades_permute_host in all three forms.  The arms alternate call by call after
one warm-up round; each call is timed by the library's device events around its launch (the profile scope of the entry point);
a point reports the median of CALLS calls per arm and the spread (max - min) / median.  ``auto_over_best`` is AUTO's time over
the better forced form's: the crossover in csrc/hades.hip is right while it stays below 1.10 at every n.

    python tools/poseidon_bench.py [--sizes 1,64,1024,16384,262144,1048576] [--height 10] [--out profiles/poseidon_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (before the library: one HIP runtime per process, as in bench.py)
import plonk_prototype_amd as pa  # noqa: E402

ROUNDS, FULL = 67, 8
CALLS = 5
FORMS = ("thread", "wave", "auto")


def random_elements(rng, count):
    """canonical Montgomery limbs: any value below 2^254 is below the modulus"""
    a = rng.integers(0, 1 << 63, size=(count, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(count, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64(0x3fffffffffffffff)
    return a


def spread(xs):
    return round((max(xs) - min(xs)) / statistics.median(xs), 4)


def timed(ctx, scope, arms, calls):
    """arms: {name: callable}; -> {name: [ms] x calls}, the arms alternating, round 0 dropped"""
    ctx.profile(True, only=scope)
    times, seen, launches = {k: [] for k in arms}, 0.0, 0
    for k in range(calls + 1):
        for name, fn in arms.items():
            fn()
            ctx.sync()
            count, total = ctx.profile_read()[scope]
            launches += 1
            assert count == launches
            if k:
                times[name].append(total - seen)
            seen = total
    ctx.profile(False)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,64,1024,16384,262144,1048576")
    ap.add_argument("--height", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poseidon_bench.json"))
    args = ap.parse_args()
    ctx = pa.Context(0)
    rng = np.random.default_rng(2025)
    ark, mds = random_elements(rng, 5 * ROUNDS), random_elements(rng, 25)
    h = pa.Hades(ctx, ark, mds, ROUNDS, FULL)
    check = random_elements(rng, 5 * 64).reshape(64, 5, 4)
    want = np.stack([pa.hades_permute_host(ark, mds, s, ROUNDS, FULL) for s in check])
    for form in FORMS:
        assert h.permute(check, form=form).tobytes() == want.tobytes(), f"the {form} form disagrees with the host form"
    rec = {"what": "poseidon_native", "rounds": ROUNDS, "full_rounds": FULL, "calls_per_arm": CALLS, "points": []}
    for n in [int(x) for x in args.sizes.split(",")]:
        d = pa.DeviceVector.from_host(ctx, random_elements(rng, 5 * n))
        times = timed(ctx, "hades_permute", {f: (lambda f=f: h.permute_dev(d.ptr, n, form=f)) for f in FORMS}, CALLS)
        med = {f: statistics.median(times[f]) for f in FORMS}
        best = min(med["thread"], med["wave"])
        point = {"n": n}
        for f in FORMS:
            point.update({f"{f}_ms": round(med[f], 4), f"{f}_spread": spread(times[f]), f"{f}_perm_per_s": round(n / med[f] * 1e3)})
        point["auto_over_best"] = round(med["auto"] / best, 3)
        rec["points"].append(point)
        print(json.dumps(point), flush=True)
        d.free()
    leaves = pa.DeviceVector.from_host(ctx, random_elements(rng, 4 ** args.height))
    tree = pa.DeviceVector(ctx, (4 ** args.height - 1) // 3)
    times = timed(ctx, "poseidon_merkle", {f: (lambda f=f: h.merkle_dev(leaves.ptr, args.height, tree.ptr, form=f)) for f in ("auto", "thread")},
                  CALLS)
    nodes = (4 ** args.height - 1) // 3
    rec["merkle"] = {"height": args.height, "nodes": nodes}
    for f in ("auto", "thread"):
        ms = statistics.median(times[f])
        rec["merkle"].update({f"{f}_ms": round(ms, 4), f"{f}_spread": spread(times[f]), f"{f}_perm_per_s": round(nodes / ms * 1e3)})
    print(json.dumps(rec["merkle"]), flush=True)
    h.free()
    ctx.close()
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
