#!/usr/bin/env python3
"""The incremental Poseidon tree at dusk's size (67 rounds, 8 full, one matrix): what an update of k
leaves costs against the full rebuild of the same tree, and what verifying a path costs against the bare hash chain.  A
developer tool: one GPU, one process.

Update: on a tree of 4^height leaves, pm_poseidon_merkle_update_dev for k random leaves and for k contiguous leaves (starting at
an index that is no multiple of 4) in the THREAD form, the WAVE form and AUTO, against pm_poseidon_merkle_dev (AUTO) over the
same leaves, measured in the same run.  Every arm is one call that ends in a wait for the stream, timed by the host clock
around it; the arms alternate call by call after one warm-up round; a point reports the median of CALLS calls per arm and the
spread (max - min) / median.  Before anything is timed the updated tree is compared with a rebuild, byte by byte.  The tool
reports between which two measured k the AUTO update stops being cheaper than the rebuild.

Verify: pm_poseidon_merkle_verify_dev on n paths (AUTO and THREAD) against `height` calls of pm_poseidon_hash_dev on n messages
of four -- the same permutations without the path logic -- and the ratio of the two.

    python tools/merkle_update_bench.py [--heights 10,12] [--ks 1,64,4096,16384,65536,262144] [--paths 1024,4096,16384,65536,262144]
                                        [--out profiles/merkle_update_bench.json]
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
FORMS = ("thread", "wave", "auto")


def random_elements(rng, count):
    """canonical Montgomery limbs: any value below 2^254 is below the modulus"""
    a = rng.integers(0, 1 << 63, size=(count, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(count, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64(0x3fffffffffffffff)
    return a


def spread(xs):
    return round((max(xs) - min(xs)) / statistics.median(xs), 4)


def timed(ctx, arms, calls=CALLS):
    """arms: {name: callable that ends in a wait for the stream}; -> {name: [ms] x calls}, alternating, round 0 dropped"""
    times = {k: [] for k in arms}
    ctx.sync()
    for k in range(calls + 1):
        for name, fn in arms.items():
            t0 = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t0) * 1e3
            if k:
                times[name].append(dt)
    return times


def update_points(ctx, h, rng, height, ks):
    count = 4 ** height
    leaves = random_elements(rng, count)
    tree = h.merkle(leaves)
    nodes = (count - 1) // 3

    def rebuild():
        h.merkle_dev(tree.leaves.ptr, height, tree.nodes.ptr)
        ctx.sync()
    points = []
    for k in [k for k in ks if k <= count]:
        for pattern in ("random", "contiguous"):
            if pattern == "random":
                idx = np.sort(rng.choice(count, size=k, replace=False).astype(np.uint64))
            else:
                first = min(count - k, (count // 3) | 1)
                idx = np.arange(first, first + k, dtype=np.uint64)
            d_idx, d_vals = _upload_words(ctx, idx), pa.DeviceVector.from_host(ctx, random_elements(rng, k))
            work = pa.DeviceVector(ctx, (ctx._lib.pm_poseidon_merkle_update_work_bytes(k) + 31) // 32)
            hashed = tree.update_dev(d_idx.ptr, d_vals.ptr, k, work.ptr)                      # checked before it is timed
            after = tree.nodes.to_host().tobytes()
            rebuild()
            assert tree.nodes.to_host().tobytes() == after, "the update disagrees with the rebuild"
            arms = {f: (lambda f=f: tree.update_dev(d_idx.ptr, d_vals.ptr, k, work.ptr, form=f)) for f in FORMS}
            arms["rebuild"] = rebuild
            times = timed(ctx, arms)
            point = {"height": height, "k": k, "pattern": pattern, "hashed": hashed, "rebuild_hashed": nodes}
            for name in arms:
                point.update({f"{name}_ms": round(statistics.median(times[name]), 4), f"{name}_spread": spread(times[name])})
            point["auto_over_best"] = round(point["auto_ms"] / min(point["thread_ms"], point["wave_ms"]), 3)
            point["auto_over_rebuild"] = round(point["auto_ms"] / point["rebuild_ms"], 4)
            points.append(point)
            print(json.dumps(point), flush=True)
            d_idx.free(), d_vals.free(), work.free()
    cross = {}
    for pattern in ("random", "contiguous"):
        mine = [p for p in points if p["pattern"] == pattern]
        below = [p["k"] for p in mine if p["auto_over_rebuild"] < 1]
        above = [p["k"] for p in mine if p["auto_over_rebuild"] >= 1]
        cross[pattern] = {"update_cheaper_up_to_k": max(below) if below else None,
                          "rebuild_cheaper_from_k": min(above) if above else None}
    tree.free()
    return points, cross


def verify_points(ctx, h, rng, height, sizes):
    count = 4 ** height
    tree = h.merkle(random_elements(rng, count))
    root = tree.level(height)
    points = []
    for n in sizes:
        idx = rng.integers(0, count, size=n, dtype=np.uint64)
        d_idx = _upload_words(ctx, idx)
        paths, status = pa.DeviceVector(ctx, n * height * 4), pa.DeviceVector(ctx, (n + 7) // 8)
        hashes = pa.DeviceVector(ctx, n)
        tree.paths_dev(d_idx.ptr, n, paths.ptr)
        for form in ("auto", "thread"):
            h.verify_paths_dev(paths.ptr, d_idx.ptr, n, height, root.ptr, status.ptr, form=form)
            ctx.sync()
            assert not status.to_host().view(np.uint32).reshape(-1)[:n].any(), "a path of the tree itself does not verify"

        def verify(form):
            h.verify_paths_dev(paths.ptr, d_idx.ptr, n, height, root.ptr, status.ptr, form=form)
            ctx.sync()

        def chain(form):                                     # `height` hashes of n messages of four: the permutations alone
            for l in range(height):
                h.hash_dev(paths.ptr + 128 * l, 4, n, hashes.ptr, msg_stride=4 * height, form=form)   # level l of every path
            ctx.sync()
        times = timed(ctx, {"verify_auto": lambda: verify("auto"), "chain_auto": lambda: chain("auto"),
                            "verify_thread": lambda: verify("thread"), "chain_thread": lambda: chain("thread")})
        point = {"height": height, "paths": n}
        for name, ts in times.items():
            point.update({f"{name}_ms": round(statistics.median(ts), 4), f"{name}_spread": spread(ts)})
        point["verify_over_chain_auto"] = round(point["verify_auto_ms"] / point["chain_auto_ms"], 3)
        point["verify_over_chain_thread"] = round(point["verify_thread_ms"] / point["chain_thread_ms"], 3)
        point["us_per_path_auto"] = round(point["verify_auto_ms"] * 1e3 / n, 4)
        points.append(point)
        print(json.dumps(point), flush=True)
        for d in (d_idx, paths, status, hashes):
            d.free()
    tree.free()
    return points


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--heights", default="10,12")
    ap.add_argument("--ks", default="1,64,4096,16384,65536,262144")
    ap.add_argument("--paths", default="1024,4096,16384,65536,262144")
    ap.add_argument("--verify-height", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merkle_update_bench.json"))
    args = ap.parse_args()
    ctx = pa.Context(0)
    rng = np.random.default_rng(2026)
    h = pa.Hades(ctx, random_elements(rng, 5 * ROUNDS), random_elements(rng, 25), ROUNDS, FULL)
    rec = {"what": "poseidon_merkle_update", "rounds": ROUNDS, "full_rounds": FULL, "calls_per_arm": CALLS,
           "device": torch.cuda.get_device_name(0), "update": [], "crossover": {}}
    for height in [int(x) for x in args.heights.split(",")]:
        points, cross = update_points(ctx, h, rng, height, [int(x) for x in args.ks.split(",")])
        rec["update"] += points
        rec["crossover"][str(height)] = cross
        print(json.dumps({"height": height, "crossover": cross}), flush=True)
    rec["verify"] = verify_points(ctx, h, rng, args.verify_height, [int(x) for x in args.paths.split(",")])
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
