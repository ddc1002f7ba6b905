#!/usr/bin/env python3
"""Native JubJub: time per multiplication of pm_jubjub_fixed_mul_dev, pm_jubjub_commit_dev (two
multiplications an output) and pm_jubjub_mul_dev at n = 2^10, 2^14, 2^18 and 2^20, beside the two routes that existed before:
pm_jubjub_mul_host on one host thread, and the same multiplications done as FIXED_BASE gadgets of 256 rounds through
pk.fill_gadgets (16 gadgets a circuit, batches of 1, 16 and 64 proofs: 16, 256 and 1024 multiplications a call).  A developer
tool: one GPU, one process.

Before anything is timed, 64 outputs of each device call are compared with the host form, and the gadget's last row with the
native product of the key's own base.  The arms alternate call by call after one warm-up round; each call is timed by the
library's device events around its launches (the profile scope of the entry point); a point reports the median of CALLS calls
per arm and the spread (max - min) / median.  The host form is timed by the host clock over 32 calls.

    python tools/jubjub_bench.py [--sizes 1024,16384,262144,1048576] [--batches 1,16,64] [--out profiles/jubjub_bench.json]
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402,F401  (before the library: one HIP runtime per process, as in bench.py)
import gadget_model as M  # noqa: E402
import plonk_prototype_amd as pa  # noqa: E402

CALLS = 5
ROUNDS, GADGETS = 256, 16
SCOPES = {"fixed": "jubjub_fixed_mul", "commit": "jubjub_commit", "variable": "jubjub_mul"}


def random_elements(rng, count):
    """canonical Montgomery limbs: any value below 2^254 is below the modulus"""
    a = rng.integers(0, 1 << 63, size=(count, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(count, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64(0x3fffffffffffffff)
    return a


def spread(xs):
    return round((max(xs) - min(xs)) / statistics.median(xs), 4)


def timed(ctx, arms, calls):
    """arms: {name: (scope, callable)}; -> {name: [ms] x calls}, the arms alternating, round 0 dropped"""
    times = {k: [] for k in arms}
    ctx.profile(True)
    seen = {}
    for k in range(calls + 1):
        for name, (scope, fn) in arms.items():
            fn()
            ctx.sync()
            _, total = ctx.profile_read()[scope]
            if k:
                times[name].append(total - seen.get(scope, 0.0))
            seen[scope] = total
    ctx.profile(False)
    return times


def gadget_route(ctx, batches):
    """GADGETS fixed-base gadgets of ROUNDS rounds from the identity; -> [{multiplications, fill_ms, us_per_mul}]"""
    b = M.Builder(1 << (GADGETS * (ROUNDS + 1)).bit_length())
    one = b.var(True)
    svars = [b.var(True) for _ in range(GADGETS)]
    outs = [b.fixed_base(s, ROUNDS, (0, one)) for s in svars]
    arith = b.fill_arithmetic(1)
    rng = random.Random(16)
    scalars = [rng.getrandbits(250) for _ in range(GADGETS)]
    only, _, reasons = b.model({one: 1, **dict(zip(svars, scalars)), **arith})
    assert not reasons
    pk = pa.preprocess(b.circuit(), ctx)
    pk.set_gadgets(b.gadget_records())
    nv = b.num_vars
    base = pa.JubJubBase.from_key(pk, 0)
    filled, reps = pk.fill_gadgets(M.to_limbs(only))
    filled = filled.reshape(-1, nv, 4)[0]
    native = base.mul(scalars)
    assert all(r.ok for r in reps)
    for k, (x, y) in enumerate(outs):
        assert filled[x].tobytes() == native[k, 0].tobytes() and filled[y].tobytes() == native[k, 1].tobytes(), "gadget != native"
    points = []
    for B in batches:
        d = pa.DeviceVector.from_host(ctx, np.tile(M.to_limbs(only), (B, 1)))
        raws = (pa._lib.GadgetReport * B)()
        call = lambda: ctx._check(ctx._lib.pm_plonk_fill_gadgets_dev(ctx._h, pk._h, d._p, nv, B, raws, None))   # noqa: E731
        t = timed(ctx, {"fill": ("plonk_gadget_fill", call)}, CALLS)["fill"]
        ms = statistics.median(t)
        points.append({"multiplications": GADGETS * B, "batch": B, "fill_ms": round(ms, 4), "fill_spread": spread(t),
                       "us_per_mul": round(ms * 1e3 / (GADGETS * B), 3)})
        print(json.dumps(points[-1]), flush=True)
        d.free()
    base.free()
    pk.free()
    return points


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,16384,262144,1048576")
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jubjub_bench.json"))
    args = ap.parse_args()
    ctx = pa.Context(0)
    rng = np.random.default_rng(2026)
    G, H = pa.JUBJUB_GENERATOR, M.curve_point(0x14)
    g, h = pa.JubJubBase(ctx, G), pa.JubJubBase(ctx, H)
    # ---- correctness first: 64 outputs of each call against the host form
    s64, b64 = random_elements(rng, 64), random_elements(rng, 64)
    fixed = g.mul(s64)
    want = np.stack([pa.jubjub_mul_host(G, s) for s in s64])
    assert fixed.tobytes() == want.tobytes(), "fixed base disagrees with the host form"
    want_c = np.stack([pa.jubjub_add_host(w, pa.jubjub_mul_host(H, b)) for w, b in zip(want, b64)])
    assert pa.jubjub_commit(g, h, s64, b64).tobytes() == want_c.tobytes(), "commit disagrees with the host form"
    assert pa.jubjub_mul(ctx, want, b64).tobytes() == np.stack([pa.jubjub_mul_host(w, b) for w, b in zip(want, b64)]).tobytes(), \
        "variable base disagrees with the host form"
    # ---- the host form, one thread
    t0 = time.perf_counter()
    for s in s64[:32]:
        pa.jubjub_mul_host(G, s)
    host_us = (time.perf_counter() - t0) / 32 * 1e6
    rec = {"what": "jubjub_native", "calls_per_arm": CALLS, "host_us_per_mul": round(host_us, 1), "points": []}
    print(json.dumps({"host_us_per_mul": rec["host_us_per_mul"]}), flush=True)
    for n in [int(x) for x in args.sizes.split(",")]:
        ds, db = pa.DeviceVector.from_host(ctx, random_elements(rng, n)), pa.DeviceVector.from_host(ctx, random_elements(rng, n))
        dp, out = pa.DeviceVector(ctx, 2 * n), pa.DeviceVector(ctx, 2 * n)
        g.mul_dev(db.ptr, n, dp.ptr)                      # n points of the curve for the variable-base arm
        arms = {"fixed": (SCOPES["fixed"], lambda: g.mul_dev(ds.ptr, n, out.ptr)),
                "commit": (SCOPES["commit"], lambda: pa.jubjub_commit_dev(g, h, ds.ptr, db.ptr, n, out.ptr)),
                "variable": (SCOPES["variable"], lambda: pa.jubjub_mul_dev(ctx, dp.ptr, ds.ptr, n, out.ptr))}
        times = timed(ctx, arms, CALLS)
        point = {"n": n}
        for name in arms:
            ms = statistics.median(times[name])
            per = 2 * n if name == "commit" else n       # a commitment is two multiplications
            point.update({f"{name}_ms": round(ms, 4), f"{name}_spread": spread(times[name]),
                          f"{name}_us_per_mul": round(ms * 1e3 / per, 4)})
        rec["points"].append(point)
        print(json.dumps(point), flush=True)
        for x in (ds, db, dp, out):
            x.free()
    rec["gadget_route"] = {"rounds": ROUNDS, "gadgets_per_circuit": GADGETS,
                           "points": gadget_route(ctx, [int(x) for x in args.batches.split(",")])}
    g.free(), h.free()
    ctx.close()
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
