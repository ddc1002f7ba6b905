#!/usr/bin/env python3
"""JubJub MSM and batch Schnorr verification: milliseconds per pm_jubjub_msm_dev over n points for
uniform and for witness-like scalars (90 % below 2^16, 5 % zero, 1 % one), the window width the rule chose beside a sweep of
forced widths, and -- in the same run, on the same points and scalars -- pm_jubjub_mul_dev, the only route to the same sum
before (its n products still have to be added up); then pm_schnorr_verify_batch_dev against pm_schnorr_verify_dev on the same
signatures.  A developer tool: one GPU, one process.

Before anything is timed the MSM of 64 points is compared with the host form and a valid batch must be accepted.  The arms
alternate call by call after one warm-up round; each call is timed by the library's device events around its launches (the
profile scope of the entry point: allocation and the final wait are outside it); a point reports the median of CALLS calls per
arm and the spread (max - min) / median.

    python tools/jubjub_msm_bench.py [--sizes 64,...,1048576] [--sweep 1024,16384,65536,262144,1048576] [--out profiles/jubjub_msm_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402,F401  (before the library: one HIP runtime per process, as in bench.py)
import gadget_model as M  # noqa: E402
import schnorr_model as S  # noqa: E402
import plonk_prototype_amd as pa  # noqa: E402
from plonk_prototype_amd import _lib  # noqa: E402

CALLS = 5
CANON = _lib.SCALAR_CANONICAL
WIDTHS = (6, 8, 10, 11, 12, 13, 14, 15, 16)


def uniform_scalars(rng, count):
    """canonical integers below 2^254 < r"""
    a = rng.integers(0, 1 << 63, size=(count, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(count, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64(0x3fffffffffffffff)
    return a


def witness_scalars(rng, count):
    a = uniform_scalars(rng, count)
    t = rng.random(count)
    small = t < 0.96
    a[small, 1:] = 0
    a[small, 0] &= np.uint64(0xffff)
    a[t < 0.06, 0] = 1
    a[t < 0.05, 0] = 0
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


def med(ts):
    return round(statistics.median(ts), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default=",".join(str(1 << k) for k in (6, 7, 8, 9, 10, 12, 14, 16, 18, 20)))
    ap.add_argument("--sweep", default="1024,16384,65536,262144,1048576")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jubjub_msm_bench.json"))
    args = ap.parse_args()
    sizes, sweep = [int(x) for x in args.sizes.split(",")], {int(x) for x in args.sweep.split(",") if x}
    ctx = pa.Context(0)
    lib = ctx._lib
    rng = np.random.default_rng(2027)
    g = pa.JubJubBase(ctx, pa.JUBJUB_GENERATOR)
    hm = S.Hades("67_8_one_matrix")
    hades = pa.Hades(ctx, M.to_limbs(hm.flat_ark), M.to_limbs(hm.flat_mds), hm.rounds, hm.full)
    sch = pa.Schnorr(g, hades)
    # ---- correctness first
    k64, s64 = uniform_scalars(rng, 64), uniform_scalars(rng, 64)
    p64 = g.mul([int.from_bytes(r.tobytes(), "little") for r in k64])
    ints = [int.from_bytes(r.tobytes(), "little") for r in s64]
    assert pa.jubjub_msm(ctx, p64, ints).tobytes() == pa.jubjub_msm_host(p64.reshape(-1, 2, 4), ints).tobytes(), "MSM disagrees with the host form"
    rec = {"what": "jubjub_msm", "calls_per_arm": CALLS, "points": [], "schnorr": []}
    plan = np.zeros(8, np.uint64)
    for n in sizes:
        dk = pa.DeviceVector.from_host(ctx, uniform_scalars(rng, n))
        dp, prod, out = pa.DeviceVector(ctx, 2 * n), pa.DeviceVector(ctx, 2 * n), pa.DeviceVector(ctx, 2)
        g.mul_dev(dk.ptr, n, dp.ptr, CANON)                   # n points of the curve
        assert lib.pm_test_jubjub_msm_plan(n, 1, 0, 0, plan.ctypes.data_as(_lib.u64p)) == 0
        point = {"n": n, "rule_c": int(plan[0])}
        for label, make in (("uniform", uniform_scalars), ("witness", witness_scalars)):
            ds = pa.DeviceVector.from_host(ctx, make(rng, n))
            arms = {"msm": ("jubjub_msm", lambda: pa.jubjub_msm_dev(ctx, dp.ptr, ds.ptr, n, out.ptr, 1, None, CANON)),
                    "mul": ("jubjub_mul", lambda: pa.jubjub_mul_dev(ctx, dp.ptr, ds.ptr, n, prod.ptr, CANON))}
            t = timed(ctx, arms, CALLS)
            point.update({f"{label}_msm_ms": med(t["msm"]), f"{label}_msm_spread": spread(t["msm"]),
                          f"{label}_mul_ms": med(t["mul"]), f"{label}_mul_spread": spread(t["mul"])})
            if n in sweep:
                widths = {}
                for c in WIDTHS:
                    ctx.set_option("jubjub_msm_window_bits", c)
                    rc = lib.pm_test_jubjub_msm_plan(n, 1, c, 0, plan.ctypes.data_as(_lib.u64p))
                    if rc == 0:
                        widths[str(c)] = med(timed(ctx, {"msm": arms["msm"]}, 3)["msm"])
                ctx.set_option("jubjub_msm_window_bits", 0)
                point[f"{label}_sweep_ms"] = widths
            ds.free()
        rec["points"].append(point)
        print(json.dumps(point), flush=True)
        # ---- signatures over the same n: public keys sk G, signatures made on the device
        dsk, dno, dm = (pa.DeviceVector.from_host(ctx, uniform_scalars(rng, n)) for _ in range(3))
        dpk, dsig = pa.DeviceVector(ctx, 2 * n), pa.DeviceVector(ctx, 3 * n)
        w = rng.integers(1, 1 << 63, size=(2 * ((n + 1) // 2), 2), dtype=np.uint64)      # z_i in [1, 2^127): fresh per run
        dw = pa.DeviceVector.from_host(ctx, w.reshape(-1, 4))
        g.mul_dev(dsk.ptr, n, dpk.ptr, CANON)
        sch.sign_dev(dsk.ptr, dno.ptr, dm.ptr, n, dsig.ptr, CANON)
        assert sch.verify_dev(dpk.ptr, dm.ptr, dsig.ptr, n, 0, True, CANON) == n, "a signature made here does not verify"
        assert sch.verify_batch_dev(dpk.ptr, dm.ptr, dsig.ptr, dw.ptr, n, 0, CANON) == (0, n), "the batch is not accepted"
        arms = {"verify": ("schnorr_verify", lambda: sch.verify_dev(dpk.ptr, dm.ptr, dsig.ptr, n, 0, True, CANON)),
                "batch": ("schnorr_verify_batch", lambda: sch.verify_batch_dev(dpk.ptr, dm.ptr, dsig.ptr, dw.ptr, n, 0, CANON))}
        t = timed(ctx, arms, CALLS)
        spoint = {"n": n, "verify_ms": med(t["verify"]), "verify_spread": spread(t["verify"]),
                  "batch_ms": med(t["batch"]), "batch_spread": spread(t["batch"])}
        rec["schnorr"].append(spoint)
        print(json.dumps(spoint), flush=True)
        for x in (dk, dp, prod, out, dsk, dno, dm, dpk, dsig, dw):
            x.free()
    g.free(), hades.free()
    ctx.close()
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
