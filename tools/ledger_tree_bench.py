#!/usr/bin/env python3
"""The append-only Poseidon tree at dusk's size (67 rounds, 8 full, one matrix).  A developer tool: one
GPU, one process.  The method is that of tools/merkle_update_bench.py: every arm is one call that ends in a wait for the stream,
timed by the host clock around it; what restores an arm's starting state (a truncate before an append, an append before a
truncate) runs before the clock starts; the arms alternate call by call after one warm-up round; a point reports the median of
CALLS calls per arm and the spread (max - min) / median.  Every arm's result is compared byte by byte before it is timed.

  append   k leaves appended to a half-full ledger tree of height H against pm_poseidon_merkle_update_dev over the same
           contiguous indices of the dense tree, and against the dense rebuild, in the same run.
  single   one leaf appended, and a truncate by one leaf, on a tree of 1000 leaves at ledger heights.
  scale    one append of 2^20 leaves into an empty tree of height 17, and 2^12 paths out of it.

    python tools/ledger_tree_bench.py [--heights 10,12] [--ks 1,64,4096,65536] [--single-heights 17,31]
                                      [--out profiles/ledger_tree_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (before the library: one HIP runtime per process, as in bench.py)
import plonk_prototype_amd as pa  # noqa: E402
from plonk_prototype_amd.poseidon import _upload_words  # noqa: E402

ROUNDS, FULL = 67, 8
CALLS = 5


def random_elements(rng, count):
    """canonical Montgomery limbs: any value below 2^254 is below the modulus"""
    a = rng.integers(0, 1 << 63, size=(count, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(count, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64(0x3fffffffffffffff)
    return a


def spread(xs):
    return round((max(xs) - min(xs)) / statistics.median(xs), 4)


def timed(ctx, arms, calls=CALLS):
    """arms: {name: (prepare, call)}; prepare runs and is waited for outside the clock, call ends in a wait for the stream
    -> {name: [ms] x calls}, alternating, round 0 dropped"""
    times = {k: [] for k in arms}
    for k in range(calls + 1):
        for name, (prepare, call) in arms.items():
            prepare()
            ctx.sync()
            t0 = time.perf_counter()
            call()
            dt = (time.perf_counter() - t0) * 1e3
            if k:
                times[name].append(dt)
    return times


def report(point, times):
    for name, ts in times.items():
        point.update({f"{name}_ms": round(statistics.median(ts), 4), f"{name}_spread": spread(ts)})
    print(json.dumps(point), flush=True)
    return point


def append_points(ctx, h, rng, height, ks):
    count = 4 ** height
    half = count // 2
    leaves = np.zeros((count, 4), np.uint64)                                   # the empty leaf is zero
    leaves[:half] = random_elements(rng, half)
    dense = h.merkle(leaves)
    ledger = h.ledger(height, reserve=count)
    ledger.append(leaves[:half])
    points = []
    for k in [k for k in ks if k <= half]:
        values = random_elements(rng, k)
        d_vals, d_idx = pa.DeviceVector.from_host(ctx, values), _upload_words(ctx, np.arange(half, half + k, dtype=np.uint64))
        work = pa.DeviceVector(ctx, (ctx._lib.pm_poseidon_merkle_update_work_bytes(k) + 31) // 32)

        def rebuild():
            h.merkle_dev(dense.leaves.ptr, height, dense.nodes.ptr)
            ctx.sync()

        def update():
            dense.update_dev(d_idx.ptr, d_vals.ptr, k, work.ptr)                # waits for the stream itself

        def append():
            ledger.append_dev(d_vals.ptr, k)
            ctx.sync()
        hashed = ledger.append_dev(d_vals.ptr, k)                               # checked before it is timed
        assert dense.update_dev(d_idx.ptr, d_vals.ptr, k, work.ptr) == hashed
        for l in range(height + 1):
            stored = ledger.level(l)
            assert stored.to_host().tobytes() == dense.level(l).view(0, stored.n).to_host().tobytes(), ("level", l)
        assert ledger.root.tobytes() == dense.root.tobytes()
        arms = {"append": (lambda: ledger.truncate(half), append), "update": (lambda: None, update), "rebuild": (lambda: None, rebuild)}
        point = report({"what": "append", "height": height, "count": half, "k": k, "hashed": hashed,
                        "rebuild_hashed": (count - 1) // 3}, timed(ctx, arms))
        slack = max(point["append_spread"] * point["append_ms"], point["update_spread"] * point["update_ms"])
        point["append_over_update"] = round(point["append_ms"] / point["update_ms"], 4)
        point["append_slower_than_update"] = bool(point["append_ms"] > point["update_ms"] + slack)
        points.append(point)
        ledger.truncate(half)
        for d in (d_vals, d_idx, work):
            d.free()
    ledger.free(), dense.free()
    return points


def single_point(ctx, h, rng, height, filled=1000):
    t = h.ledger(height, reserve=2 * filled)
    t.append(random_elements(rng, filled))
    d_val = pa.DeviceVector.from_host(ctx, random_elements(rng, 1))
    before = t.root.tobytes()
    assert t.append_dev(d_val.ptr, 1) == height and t.truncate(filled) == height
    assert t.root.tobytes() == before, "a truncate does not undo an append"

    def waited(call):
        def run():
            call()
            ctx.sync()
        return run
    arms = {"append": (lambda: t.truncate(filled), waited(lambda: t.append_dev(d_val.ptr, 1))),
            "truncate": (lambda: (t.truncate(filled), t.append_dev(d_val.ptr, 1)), waited(lambda: t.truncate(filled)))}
    point = report({"what": "single", "height": height, "count": filled}, timed(ctx, arms))
    d_val.free(), t.free()
    return point


def scale_point(ctx, h, rng, height=17, log_k=20, n_paths=1 << 12):
    k = 1 << log_k
    values = random_elements(rng, k)
    d_vals = pa.DeviceVector.from_host(ctx, values)
    t = h.ledger(height, reserve=k)
    hashed = t.append_dev(d_vals.ptr, k)
    dense = h.merkle(values)                                                    # 4^10 = 2^20: the dense tree is its first 10 levels
    for l in range(log_k // 2 + 1):
        assert t.level(l).to_host().tobytes() == dense.level(l).to_host().tobytes(), ("level", l)
    dense.free()
    idx = rng.integers(0, k, size=n_paths, dtype=np.uint64)
    d_idx, d_paths = _upload_words(ctx, idx), pa.DeviceVector(ctx, n_paths * height * 4)
    t.paths_dev(d_idx.ptr, n_paths, d_paths.ptr)
    assert not t.verify(d_paths.to_host().reshape(n_paths, height, 4, 4), idx).any(), "a path of the tree itself does not verify"

    def append():
        t.append_dev(d_vals.ptr, k)
        ctx.sync()
    arms = {"append": (lambda: t.truncate(0), append), "paths": (lambda: None, lambda: t.paths_dev(d_idx.ptr, n_paths, d_paths.ptr))}
    point = report({"what": "scale", "height": height, "k": k, "hashed": hashed, "paths": n_paths}, timed(ctx, arms))
    point["permutations_per_second"] = round(hashed / (point["append_ms"] * 1e-3))
    for d in (d_vals, d_idx, d_paths):
        d.free()
    t.free()
    return point


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--heights", default="10,12")
    ap.add_argument("--ks", default="1,64,4096,65536")
    ap.add_argument("--single-heights", default="17,31")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ledger_tree_bench.json"))
    args = ap.parse_args()
    ctx = pa.Context(0)
    rng = np.random.default_rng(2026)
    h = pa.Hades(ctx, random_elements(rng, 5 * ROUNDS), random_elements(rng, 25), ROUNDS, FULL)
    rec = {"what": "poseidon_ledger_tree", "rounds": ROUNDS, "full_rounds": FULL, "calls_per_arm": CALLS,
           "device": torch.cuda.get_device_name(0), "append": [], "single": []}
    for height in [int(x) for x in args.single_heights.split(",") if x]:
        rec["single"].append(single_point(ctx, h, rng, height))
    for height in [int(x) for x in args.heights.split(",") if x]:
        rec["append"] += append_points(ctx, h, rng, height, sorted(int(x) for x in args.ks.split(",")))   # ascending: see the check
    rec["scale"] = scale_point(ctx, h, rng)
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
