"""Checked commit-key loading, measured in one process; writes one JSON file.

For each --logs size, on the 2^log_n powers made by CommitKey.setup:
  compress / decompress / subgroup_check / curve_check
               device time from the library's event pairs around the launches (ctx.profile; the ProfScope names
               g1_compress, g1_decompress, g1_subgroup_check, g1_curve_check), median of --reps runs after one warm-up
  from_bytes   wall time of the whole CommitKey.from_bytes (upload of n x 48 bytes, decode, subgroup check, the
               conversion into resident bases), with and without the subgroup check
  yardstick    pm_g1_fixed_base_mul_dev on as many points in the same run (event pair "g1_fixed_base_mul"), and the
               ratios decompress / yardstick and subgroup_check / decompress
  host         pm_g1_decompress with the subgroup flag on --host-points points, one CPU thread, and its EXTRAPOLATION
               (labelled as one) to 2^20 points

usage: python tools/srs_load_bench.py [--logs 16,20] [--reps 5] [--host-points 256] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch  # noqa: F401  (first: one HIP runtime in the process)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import plonk_prototype_amd as pa  # noqa: E402
from plonk_prototype_amd.field import fr_to_limbs  # noqa: E402

TAU = fr_to_limbs(0x5DEECE66D1234567890ABCDEF0123456789ABCDEF)


def timed(ctx, name, fn, reps):
    """median device ms of the event pair `name` over reps runs of fn (one warm-up first)"""
    fn()
    out = []
    for _ in range(reps):
        ctx.profile(True, name)
        fn()
        ctx.sync()
        out.append(ctx.profile_read().get(name, (0, float("nan")))[1])
        ctx.profile(False)
    return {"median_ms": statistics.median(out), "min_ms": min(out), "max_ms": max(out), "n": len(out)}


def one_size(ctx, log_n, reps):
    n = 1 << log_n
    ctx.profile(True, "g1_fixed_base_mul")
    ck = pa.CommitKey.setup(n - 1, TAU, ctx, host_copy=True)
    ctx.profile(False)
    yard = []
    for _ in range(reps):
        ctx.profile(True, "g1_fixed_base_mul")
        pa.CommitKey.setup(n - 1, TAU, ctx)
        yard.append(ctx.profile_read().get("g1_fixed_base_mul", (0, float("nan")))[1])
        ctx.profile(False)
    d_xy = pa.DeviceVector.from_host(ctx, ck.powers_of_g.reshape(-1, 4))
    d_bytes, d_back = pa.DeviceVector(ctx, (3 * n + 1) // 2), pa.DeviceVector(ctx, 3 * n)
    res = {"log_n": log_n,
           "yardstick_fixed_base_mul": {"median_ms": statistics.median(yard), "min_ms": min(yard), "max_ms": max(yard), "n": len(yard)}}
    res["compress"] = timed(ctx, "g1_compress", lambda: ctx.g1_compress_dev(d_xy.ptr, n, d_bytes.ptr), reps)
    res["decompress"] = timed(ctx, "g1_decompress", lambda: ctx.g1_decompress_dev(d_bytes.ptr, n, d_back.ptr, False), reps)
    res["subgroup_check"] = timed(ctx, "g1_subgroup_check", lambda: ctx.g1_check_dev(d_xy.ptr, n, True), reps)
    res["curve_check"] = timed(ctx, "g1_curve_check", lambda: ctx.g1_check_dev(d_xy.ptr, n, False), reps)
    data = d_bytes.to_host().tobytes()[:48 * n]
    assert data == ck.to_bytes(), "device encoding of the array and of the resident bases differ"
    for check in (True, False):
        walls = []
        for _ in range(reps + 1):
            ctx.sync()
            t0 = time.perf_counter()
            k = pa.CommitKey.from_bytes(data, ctx, check_subgroup=check)
            walls.append((time.perf_counter() - t0) * 1e3)
            k._bases.free()
        walls = walls[1:]
        res["from_bytes_checked_wall" if check else "from_bytes_unchecked_subgroup_wall"] = {
            "median_ms": statistics.median(walls), "min_ms": min(walls), "max_ms": max(walls), "n": len(walls)}
    y = res["yardstick_fixed_base_mul"]["median_ms"]
    res["ratio_decompress_to_yardstick"] = res["decompress"]["median_ms"] / y
    res["ratio_subgroup_to_decompress"] = res["subgroup_check"]["median_ms"] / res["decompress"]["median_ms"]
    for v in (d_xy, d_bytes, d_back):
        v.free()
    return res, data


def host_rate(data, points):
    t0 = time.perf_counter()
    for i in range(points):
        pa.g1_decompress(data[48 * i:48 * i + 48], check_subgroup=True)
    per = (time.perf_counter() - t0) / points
    return {"points": points, "ms_per_point": per * 1e3, "EXTRAPOLATED_seconds_for_2^20_points_one_thread": per * (1 << 20)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", default="16,20")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-points", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "srs_load_bench.json"))
    a = ap.parse_args()
    ctx = pa.Context(0)
    out = {"sizes": [], "host": None}
    data = b""
    for k in [int(x) for x in a.logs.split(",") if x]:
        res, data = one_size(ctx, k, a.reps)
        out["sizes"].append(res)
        print(json.dumps(res), flush=True)
    if a.host_points and data:
        out["host"] = host_rate(data, min(a.host_points, len(data) // 48))
        print(json.dumps(out["host"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
