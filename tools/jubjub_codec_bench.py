#!/usr/bin/env python3
"""The JubJub wire format: device time per element of pm_fr_sqrt_dev, pm_jubjub_decompress_dev with and
without PM_JUBJUB_CHECK_SUBGROUP and pm_jubjub_compress_dev at n = 2^10 .. 2^20, and what decoding adds to a scan:

    host         pm_jubjub_decompress on one host thread over HOST_POINTS encodings: what a caller had before the device call
    scan         pm_poseidon_cipher_scan_dev on already-decoded ephemeral keys
    scan_bytes   pm_jubjub_decompress_dev on the 32-byte keys, then the same scan on its output

A developer tool: one GPU, one process.  Before anything is timed the encodings -- the device's own compress of R_i = e_i G --
are decoded both ways: every status is 0, the points are the ones encoded, with and without the flag, and 64 of them agree with
the host form; the roots of n random elements are squared on the host for 64 of them.  The arms alternate call by call after
one warm-up round; each call is timed by the library's device events around its launches (the profile scopes of the entry
points).  A point reports the median of CALLS calls per arm and the spread (max - min) / median.

    python tools/jubjub_codec_bench.py [--sizes 1024,4096,16384,65536,262144,1048576] [--out profiles/jubjub_codec_bench.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402,F401  (before the library: one HIP runtime per process, as in bench.py)
import poseidon_model as PM  # noqa: E402
import plonk_prototype_amd as pa  # noqa: E402
from plonk_prototype_amd.field import R_MOD, fr_from_limbs  # noqa: E402

CALLS = 5
ROUNDS, FULL, MSG_LEN = 67, 8, 2
HOST_POINTS = 512


def random_elements(rng, count):
    """canonical Montgomery limbs: any value below 2^254 is below the modulus"""
    a = rng.integers(0, 1 << 63, size=(count, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(count, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64(0x3fffffffffffffff)
    return a


def spread(xs):
    return round((max(xs) - min(xs)) / statistics.median(xs), 4)


def timed(ctx, arms, calls):
    """arms: {name: (scopes, callable)}; -> {name: [device ms]}, the arms alternating, round 0 dropped"""
    dev = {k: [] for k in arms}
    ctx.profile(True)
    seen = {}
    for k in range(calls + 1):
        for name, (scopes, fn) in arms.items():
            ctx.sync()
            fn()
            ctx.sync()
            read = ctx.profile_read()
            total = 0.0
            for scope in scopes:
                now = read[scope][1]
                total += now - seen.get(scope, 0.0)
                seen[scope] = now
            if k:
                dev[name].append(total)
    ctx.profile(False)
    return dev


def host_decode_us(data):
    """microseconds a point of pm_jubjub_decompress on this thread, the ctypes call included"""
    rows = [data[i].tobytes() for i in range(data.shape[0])]
    t0 = time.perf_counter()
    for row in rows:
        pa.jubjub_decompress_host(row)
    return (time.perf_counter() - t0) * 1e6 / len(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096,16384,65536,262144,1048576")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jubjub_codec_bench.json"))
    args = ap.parse_args()
    L = MSG_LEN   # noqa: N806
    ctx = pa.Context(0)
    rng = np.random.default_rng(2027)
    ark, mds = PM.constants(ROUNDS, 1, 0xC1F)
    flat_ark, flat_mds, _ = PM.flat(ark, mds)
    hades = pa.Hades(ctx, flat_ark, flat_mds, ROUNDS, FULL)
    cipher = pa.PoseidonCipher(hades, L)
    g = pa.JubJubBase(ctx, pa.JUBJUB_GENERATOR)
    vk = random_elements(rng, 1)
    rec = {"what": "jubjub_codec", "calls_per_arm": CALLS, "host_points": HOST_POINTS, "points": []}
    for n in [int(x) for x in args.sizes.split(",")]:
        d_e, d_k, d_c, d_a = (pa.DeviceVector.from_host(ctx, random_elements(rng, m)) for m in (n, n, (L + 1) * n, n))
        d_r, d_p, d_root = pa.DeviceVector(ctx, 2 * n), pa.DeviceVector(ctx, 2 * n), pa.DeviceVector(ctx, n)
        d_b, d_b2, d_out = pa.DeviceVector(ctx, n), pa.DeviceVector(ctx, n), pa.DeviceVector(ctx, L * n)
        d_st, d_fl = pa.DeviceVector(ctx, (n + 7) // 8), pa.DeviceVector(ctx, (n + 7) // 8)
        # ---- the encodings: R_i = e_i G, compressed by the device
        g.mul_dev(d_e.ptr, n, d_r.ptr)
        pa.jubjub_compress_dev(ctx, d_r.ptr, n, d_b.ptr)
        # ---- correctness first
        points = d_r.to_host()
        for flag in (False, True):
            assert pa.jubjub_decompress_dev(ctx, d_b.ptr, n, d_p.ptr, d_st.ptr, flag) == n, (n, flag)
            assert d_p.to_host().tobytes() == points.tobytes(), "decode-then-encode is not the identity"
        data = d_b.to_host().view(np.uint8).reshape(n, 32)
        for i in range(min(n, 64)):
            p, s = pa.jubjub_decompress_host(data[i].tobytes())
            assert s == 0 and p.tobytes() == points.reshape(n, 2, 4)[i].tobytes(), "the host form disagrees"
        squares = pa.fr_sqrt_dev(ctx, d_a.ptr, n, d_root.ptr, d_fl.ptr, want_count=True)
        vals, roots, flags = d_a.to_host(), d_root.to_host(), d_fl.to_host().view(np.uint32).reshape(-1)[:n]
        for i in range(min(n, 64)):
            x = fr_from_limbs(roots[i])
            assert x % 2 == 0 and (x * x % R_MOD == fr_from_limbs(vals[i]) if flags[i] else x == 0), "a root is wrong"
        host_us = host_decode_us(data[:min(n, HOST_POINTS)])

        def scan(d_keys):
            cipher.scan_dev(vk, d_keys, d_k.ptr, d_c.ptr, n, d_out.ptr, d_st.ptr, want_n_ok=False)

        def scan_bytes():
            pa.jubjub_decompress_dev(ctx, d_b.ptr, n, d_p.ptr, want_n_ok=False)
            scan(d_p.ptr)

        arms = {"fr_sqrt": (("fr_sqrt",), lambda: pa.fr_sqrt_dev(ctx, d_a.ptr, n, d_root.ptr, d_fl.ptr)),
                "decompress": (("jubjub_decompress",), lambda: pa.jubjub_decompress_dev(ctx, d_b.ptr, n, d_p.ptr, d_st.ptr, want_n_ok=False)),
                "decompress_subgroup": (("jubjub_decompress",),
                                        lambda: pa.jubjub_decompress_dev(ctx, d_b.ptr, n, d_p.ptr, d_st.ptr, True, want_n_ok=False)),
                "compress": (("jubjub_compress",), lambda: pa.jubjub_compress_dev(ctx, d_r.ptr, n, d_b2.ptr)),
                "scan": (("poseidon_cipher_scan",), lambda: scan(d_r.ptr)),
                "scan_bytes": (("jubjub_decompress", "poseidon_cipher_scan"), scan_bytes)}
        dev = timed(ctx, arms, CALLS)
        point = {"n": n, "squares": squares, "host_decompress_us_per_point": round(host_us, 2)}
        for name in arms:
            ms = statistics.median(dev[name])
            point.update({f"{name}_ms": round(ms, 4), f"{name}_spread": spread(dev[name]), f"{name}_ns_per_element": round(ms * 1e6 / n, 2)})
        point["host_over_device_decompress"] = round(host_us * 1e3 / point["decompress_ns_per_element"], 1)
        point["scan_bytes_over_scan"] = round(point["scan_bytes_ms"] / point["scan_ms"], 4)
        point["decompress_over_scan"] = round(point["decompress_ms"] / point["scan_ms"], 4)
        rec["points"].append(point)
        print(json.dumps(point), flush=True)
        for x in (d_e, d_k, d_c, d_a, d_r, d_p, d_root, d_b, d_b2, d_out, d_st, d_fl):
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
