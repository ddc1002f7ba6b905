#!/usr/bin/env python3
"""Native Schnorr signatures: time per signature of pm_schnorr_sign_dev (a) and pm_schnorr_verify_dev
(b) at n = 2^10, 2^14, 2^18 and 2^20, beside (c) the composed route the library offered before for a verification --
pm_poseidon_hash_dev over (R.x, R.y, m), pm_jubjub_fixed_mul_dev for u G and pm_jubjub_mul_dev for c PK -- and beside
pm_jubjub_fixed_mul_dev alone, the multiplication inside a signing.  A developer tool: one GPU, one process.

What arm (c) leaves out, all in its favour: the messages are already packed as (R.x, R.y, m); the multiplier of PK is the
untruncated hash (the library had no device call for the truncation; the work is the same); the range and point tests are not
done; and its closing step, one affine addition and a comparison per signature, is not a device call at all: it is timed on the
host over 64 signatures and reported separately (`composed_closing_host_us`).

Before anything is timed, 64 signatures of the device call are compared with pm_schnorr_sign_host and their 64 reasons, with one
signature spoiled, with pm_schnorr_verify_host.  The arms alternate call by call after one warm-up round; each call is timed by
the library's device events around its launches (the profile scope of the entry point); a point reports the median of CALLS
calls per arm and the spread (max - min) / median.

    python tools/schnorr_bench.py [--sizes 1024,16384,262144,1048576] [--out profiles/schnorr_bench.json]
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
import plonk_prototype_amd as pa  # noqa: E402
import poseidon_model as PM  # noqa: E402

CALLS = 7
SHAPE = (67, 8)


def random_elements(rng, count):
    """canonical Montgomery limbs: any value below 2^254 is below the modulus"""
    a = rng.integers(0, 1 << 63, size=(count, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(count, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64(0x3fffffffffffffff)
    return a


def spread(xs):
    return round((max(xs) - min(xs)) / statistics.median(xs), 4)


def timed(ctx, arms, calls):
    """arms: {name: (scopes, callable)}; -> {name: [ms] x calls}, the arms alternating, round 0 dropped"""
    times = {k: [] for k in arms}
    ctx.profile(True)
    seen = {}
    for k in range(calls + 1):
        for name, (scopes, fn) in arms.items():
            fn()
            ctx.sync()
            prof = ctx.profile_read()
            ms = 0.0
            for scope in scopes:
                total = prof[scope][1]
                ms += total - seen.get(scope, 0.0)
                seen[scope] = total
            if k:
                times[name].append(ms)
    ctx.profile(False)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,16384,262144,1048576")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "schnorr_bench.json"))
    args = ap.parse_args()
    ctx = pa.Context(0)
    rng = np.random.default_rng(2026)
    ark, mds = PM.constants(SHAPE[0], 1, 67)
    flat_ark, flat_mds, _ = PM.flat(ark, mds)
    a_l, m_l = PM.to_limbs(flat_ark), PM.to_limbs(flat_mds)
    G = pa.JUBJUB_GENERATOR
    g, hades = pa.JubJubBase(ctx, G), pa.Hades(ctx, a_l, m_l, *SHAPE)
    s = pa.Schnorr(g, hades)
    # ---- correctness first: 64 signatures and 64 reasons against the host forms
    sk, k, m = (random_elements(rng, 64) for _ in range(3))
    sig, pk = s.sign(sk, m, k), s.public_keys(sk)
    want = np.stack([pa.schnorr_sign_host(G, a_l, m_l, sk[i:i + 1], k[i:i + 1], m[i], rounds=SHAPE[0], full_rounds=SHAPE[1])
                     for i in range(64)])
    assert sig.tobytes() == want.tobytes(), "the device's signatures disagree with the host form"
    spoiled = m.copy()
    spoiled[9] = m[10]
    got = s.verify(pk, spoiled, sig)
    host = [pa.schnorr_verify_host(G, a_l, m_l, pk[i], spoiled[i], sig[i], rounds=SHAPE[0], full_rounds=SHAPE[1]) for i in range(64)]
    assert got.tolist() == host == [0] * 9 + [4] + [0] * 54, "the device's reasons disagree with the host form"
    # ---- the closing step of the composed route, on the host
    pts = pa.jubjub_mul(ctx, pk, k)
    t0 = time.perf_counter()
    for i in range(64):
        _ = pa.jubjub_add_host(pk[i], pts[i]).tobytes() == sig[i, 1:].tobytes()
    closing_us = (time.perf_counter() - t0) / 64 * 1e6
    rec = {"what": "schnorr_native", "hades_shape": list(SHAPE), "calls_per_arm": CALLS,
           "composed_closing_host_us": round(closing_us, 1), "points": []}
    print(json.dumps({"composed_closing_host_us": rec["composed_closing_host_us"]}), flush=True)
    cap = np.zeros(4, np.uint64)
    for n in [int(x) for x in args.sizes.split(",")]:
        dsk, dk, dm = (pa.DeviceVector.from_host(ctx, random_elements(rng, n)) for _ in range(3))
        dsig, dpk, dr = pa.DeviceVector(ctx, 3 * n), pa.DeviceVector(ctx, 2 * n), pa.DeviceVector(ctx, (n + 7) // 8)
        dh, dug, dcp = pa.DeviceVector(ctx, n), pa.DeviceVector(ctx, 2 * n), pa.DeviceVector(ctx, 2 * n)
        s.sign_dev(dsk.ptr, dk.ptr, dm.ptr, n, dsig.ptr)
        g.mul_dev(dsk.ptr, n, dpk.ptr)
        ctx.sync()
        sig_h = dsig.to_host().reshape(n, 3, 4)
        packed = pa.DeviceVector.from_host(ctx, np.concatenate([sig_h[:, 1:], dm.to_host().reshape(n, 1, 4)], axis=1).reshape(-1, 4))
        du = pa.DeviceVector.from_host(ctx, np.ascontiguousarray(sig_h[:, 0]))
        assert s.verify_dev(dpk.ptr, dm.ptr, dsig.ptr, n, dr.ptr) == n, "a signature made here does not verify"

        def composed():
            hades.hash_dev(packed.ptr, 3, n, dh.ptr, capacity=cap, form="thread")
            g.mul_dev(du.ptr, n, dug.ptr)
            pa.jubjub_mul_dev(ctx, dpk.ptr, dh.ptr, n, dcp.ptr)

        arms = {"sign": (("schnorr_sign",), lambda: s.sign_dev(dsk.ptr, dk.ptr, dm.ptr, n, dsig.ptr)),
                "verify": (("schnorr_verify",), lambda: s.verify_dev(dpk.ptr, dm.ptr, dsig.ptr, n, dr.ptr, want_first_bad=False)),
                "composed": (("poseidon_hash", "jubjub_fixed_mul", "jubjub_mul"), composed),
                "fixed": (("jubjub_fixed_mul",), lambda: g.mul_dev(dk.ptr, n, dug.ptr))}
        times = timed(ctx, arms, CALLS)
        point = {"n": n}
        for name in arms:
            ms = statistics.median(times[name])
            point.update({f"{name}_ms": round(ms, 4), f"{name}_spread": spread(times[name]), f"{name}_us_per_sig": round(ms * 1e3 / n, 4)})
        point["verify_over_composed"] = round(point["verify_ms"] / point["composed_ms"], 4)
        point["sign_over_fixed"] = round(point["sign_ms"] / point["fixed_ms"], 4)
        rec["points"].append(point)
        print(json.dumps(point), flush=True)
        for x in (dsk, dk, dm, dsig, dpk, dr, dh, dug, dcp, packed, du):
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
