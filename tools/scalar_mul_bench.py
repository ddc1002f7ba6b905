"""Per-point G1 scalar multiplication and the flagged Lagrange conversion, measured in one process; writes one JSON file.

For each --logs size, on the 2^log_n powers made by CommitKey.setup and as many uniform scalars:
  scalar_mul_plain / scalar_mul_glv   pm_g1_scalar_mul_dev without and with PM_G1_POINTS_IN_SUBGROUP (event pair "g1_scalar_mul")
  fixed_base_mul                      pm_g1_fixed_base_mul_dev on the same scalars, the yardstick ("g1_fixed_base_mul")
  lagrange_plain / lagrange_glv       pm_g1_bases_lagrange against pm_g1_bases_lagrange_ex with the flag ("g1_ec_ntt"); the
                                      unflagged call is the baseline
All arms run in this one process, alternated round by round after one warm-up round; per arm the median of --reps runs,
min, max and the spread (max - min) / median of the device time from the library's event pairs.  A flagged arm counts as a
gain only if its median is below its baseline's by more than the larger of the two spreads (`gain` in the output); the two
Lagrange results are also compared byte for byte.

usage: python tools/scalar_mul_bench.py [--logs 16,20] [--reps 5] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch  # noqa: F401  (first: one HIP runtime in the process)
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import plonk_prototype_amd as pa  # noqa: E402
from plonk_prototype_amd import _lib  # noqa: E402
from plonk_prototype_amd.field import fr_to_limbs  # noqa: E402
from plonk_prototype_amd.host import G1_GENERATOR, _p  # noqa: E402

TAU = fr_to_limbs(0x5DEECE66D1234567890ABCDEF0123456789ABCDEF)
SEED = fr_to_limbs(0x243F6A8885A308D313198A2E03707344A4093822299F31D0082EFA98EC4E6C89)


def summary(v):
    med = statistics.median(v)
    return {"median_ms": med, "min_ms": min(v), "max_ms": max(v), "spread": (max(v) - min(v)) / med, "n": len(v)}


def verdict(base, arm):
    """the flagged arm gains only if its median is below the baseline's by more than the larger of the two spreads"""
    margin = max(base["spread"], arm["spread"])
    return {"speedup": base["median_ms"] / arm["median_ms"], "margin": margin,
            "gain": bool(arm["median_ms"] < base["median_ms"] * (1 - margin))}


def one_size(ctx, log_n, reps):
    n = 1 << log_n
    ck = pa.CommitKey.setup(n - 1, TAU, ctx)
    pts, out = pa.DeviceVector(ctx, 3 * n), pa.DeviceVector(ctx, 3 * n)
    lag = [pa.DeviceVector(ctx, 3 * n), pa.DeviceVector(ctx, 3 * n)]
    sc = pa.DeviceVector(ctx, n)
    ctx._check(ctx._lib.pm_g1_bases_to_dev(ctx._h, ck._bases._h, pts._p, None))
    # uniform scalars: the powers of a fixed full-width element, then squared elementwise so no short run of them is special
    ctx.fr_powers(SEED, SEED, n, sc.ptr)
    ctx.fr_vec_op(2, sc.ptr, sc.ptr, n, sc.ptr, n)
    arms = {
        "scalar_mul_plain": ("g1_scalar_mul", lambda: ctx.g1_scalar_mul_dev(pts.ptr, sc.ptr, n, out.ptr, _lib.SCALAR_MONTGOMERY, False)),
        "scalar_mul_glv": ("g1_scalar_mul", lambda: ctx.g1_scalar_mul_dev(pts.ptr, sc.ptr, n, out.ptr, _lib.SCALAR_MONTGOMERY, True)),
        "fixed_base_mul": ("g1_fixed_base_mul", lambda: ctx._check(ctx._lib.pm_g1_fixed_base_mul_dev(
            ctx._h, _p(G1_GENERATOR), sc._p, n, _lib.SCALAR_MONTGOMERY, out._p, None))),
        "lagrange_plain": ("g1_ec_ntt", lambda: ctx._check(ctx._lib.pm_g1_bases_lagrange(ctx._h, ck._bases._h, log_n, lag[0]._p, None))),
        "lagrange_glv": ("g1_ec_ntt", lambda: ctx._check(ctx._lib.pm_g1_bases_lagrange_ex(
            ctx._h, ck._bases._h, log_n, _lib.G1_POINTS_IN_SUBGROUP, lag[1]._p, None))),
    }
    times = {name: [] for name in arms}
    for it in range(reps + 1):                     # round 0 warms every arm up
        for name, (event, fn) in arms.items():
            ctx.profile(True, event)
            fn()
            ctx.sync()
            ms = ctx.profile_read().get(event, (0, float("nan")))[1]
            ctx.profile(False)
            if it:
                times[name].append(ms)
    res = {"log_n": log_n, **{name: summary(v) for name, v in times.items()}}
    res["lagrange_bytes_equal"] = bool(np.array_equal(lag[0].to_host(), lag[1].to_host()))
    res["scalar_mul_glv_vs_plain"] = verdict(res["scalar_mul_plain"], res["scalar_mul_glv"])
    res["lagrange_glv_vs_plain"] = verdict(res["lagrange_plain"], res["lagrange_glv"])
    res["scalar_mul_glv_over_fixed_base"] = res["scalar_mul_glv"]["median_ms"] / res["fixed_base_mul"]["median_ms"]
    for v in (pts, out, sc, *lag):
        v.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", default="16,20")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "scalar_mul_bench.json"))
    a = ap.parse_args()
    ctx = pa.Context(0)
    out = {"sizes": []}
    for k in [int(x) for x in a.logs.split(",") if x]:
        out["sizes"].append(one_size(ctx, k, a.reps))
        print(json.dumps(out["sizes"][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
