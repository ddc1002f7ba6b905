#!/usr/bin/env python3
"""Scanning a ledger under K viewing keys: device time of ONE pm_poseidon_cipher_scan_keys_dev beside
the composition it replaces, K calls of pm_poseidon_cipher_scan_dev, for K in 1, 2, 4, 16, 64 and n = 2^10, 2^16, 2^20 notes,
Hades (67, 8), L = 2.

    a_table   one scan_keys call on its full-table path ("cipher_scan_keys_table_min" = 1): build, walk, open, emit
    a_ladder  one scan_keys call on its per-key path (= 65), for K <= 4: K ladders, open, emit
    b         K calls of pm_poseidon_cipher_scan_dev -- that entry is unchanged, so (b) is the parent's time

and, at n = 2^20 and K = 16, a_table under three scratch budgets ("cipher_scan_table_mb" = 0, 4096, 1024).

A developer tool by the rules of tools/cipher_bench.py: one GPU, one process.  The notes are made by the device's own encrypt:
one in eight is addressed to a key of the list, the rest to a stranger.  Before anything is timed every arm is run once: (a) on
either path and (b), combined as the header states, agree byte for byte in masks, status and messages, and every planted note
is found under its key.  The arms alternate call by call after one warm-up round; a call is timed by the library's device events
around its launches (the profile scopes of the entry points, which also give the split by kernel) and by the host clock around
the call and a synchronise, which adds the allocation and release of the scratch.  A point reports the median of CALLS calls per
arm and the spread (max - min) / median.

    python tools/cipher_scan_keys_bench.py [--sizes 1024,65536,1048576] [--keys 1,2,4,16,64] [--out profiles/cipher_scan_keys_bench.json]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402,F401  (before the library: one HIP runtime per process, as in bench.py)
import poseidon_model as PM  # noqa: E402
import plonk_prototype_amd as pa  # noqa: E402
from cipher_bench import random_elements, spread  # noqa: E402

CALLS = 5
ROUNDS, FULL = 67, 8
L = 2
TABLE_SCOPES = ("poseidon_cipher_scan_keys_build", "poseidon_cipher_scan_keys_walk", "poseidon_cipher_scan_keys_open",
                "poseidon_cipher_scan_keys_emit")
LADDER_SCOPES = ("poseidon_cipher_scan_keys_ladder", "poseidon_cipher_scan_keys_open", "poseidon_cipher_scan_keys_emit")
BUDGETS = (0, 4096, 1024)


def timed(ctx, arms, calls):
    """arms: {name: (scopes, callable)} -> {name: {"dev": [ms], "host": [ms], scope: [ms]}}, the arms alternating, round 0 dropped"""
    out = {k: {"dev": [], "host": [], **{s: [] for s in arms[k][0]}} for k in arms}
    ctx.profile(True)
    seen = {}
    for k in range(calls + 1):
        for name, (scopes, fn) in arms.items():
            ctx.sync()
            t0 = time.perf_counter()
            fn()
            ctx.sync()
            t1 = time.perf_counter()
            read = ctx.profile_read()
            total, parts = 0.0, {}
            for scope in scopes:
                now = read[scope][1]
                parts[scope] = now - seen.get(scope, 0.0)
                total += parts[scope]
                seen[scope] = now
            if k:
                out[name]["dev"].append(total)
                out[name]["host"].append((t1 - t0) * 1e3)
                for scope in scopes:
                    out[name][scope].append(parts[scope])
    ctx.profile(False)
    return out


def words32(v, n):
    return v.to_host().view(np.uint32).reshape(-1)[:n].copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,65536,1048576")
    ap.add_argument("--keys", default="1,2,4,16,64")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cipher_scan_keys_bench.json"))
    args = ap.parse_args()
    ctx = pa.Context(0)
    rng = np.random.default_rng(2027)
    ark, mds = PM.constants(ROUNDS, 1, 0xC1F)
    flat_ark, flat_mds, _ = PM.flat(ark, mds)
    hades = pa.Hades(ctx, flat_ark, flat_mds, ROUNDS, FULL)
    cipher = pa.PoseidonCipher(hades, L)
    g = pa.JubJubBase(ctx, pa.JUBJUB_GENERATOR)
    all_keys = random_elements(rng, 65)                       # Montgomery limbs; the last one is the stranger
    rec = {"what": "poseidon_cipher_scan_keys", "msg_len": L, "rounds": ROUNDS, "full_rounds": FULL, "calls_per_arm": CALLS, "points": []}
    for n in [int(x) for x in args.sizes.split(",")]:
        d_e, d_k, d_m = (pa.DeviceVector.from_host(ctx, x) for x in (random_elements(rng, n), random_elements(rng, n),
                                                                     random_elements(rng, L * n)))
        d_r, d_s, d_c = pa.DeviceVector(ctx, 2 * n), pa.DeviceVector(ctx, 2 * n), pa.DeviceVector(ctx, (L + 1) * n)
        d_out, d_st, d_mask = pa.DeviceVector(ctx, L * n), pa.DeviceVector(ctx, (n + 7) // 8), pa.DeviceVector(ctx, (n + 3) // 4)
        d_out_b, d_st_b = pa.DeviceVector(ctx, L * n), pa.DeviceVector(ctx, (n + 7) // 8)
        g.mul_dev(d_e.ptr, n, d_r.ptr)                        # R_i = e_i G
        msgs = d_m.to_host().reshape(n, L, 4)
        for K in [int(x) for x in args.keys.split(",")]:   # noqa: N806
            keys = all_keys[:K]
            planted = rng.random(n) < 0.125
            owner = np.where(planted, rng.integers(0, K, n), 64)
            d_vk = pa.DeviceVector.from_host(ctx, all_keys[owner])
            pa.jubjub_mul_dev(ctx, d_r.ptr, d_vk.ptr, n, d_s.ptr)   # S_i = vk_owner R_i
            cipher.encrypt_dev(d_s.ptr, d_k.ptr, d_m.ptr, n, d_c.ptr)
            d_vk.free()

            def scan_keys(table_min, budget=0):
                ctx.set_option("cipher_scan_keys_table_min", table_min)
                ctx.set_option("cipher_scan_table_mb", budget)
                return cipher.scan_keys_dev(keys, d_r.ptr, d_k.ptr, d_c.ptr, n, d_mask.ptr, d_out.ptr, d_st.ptr, want_n_hits=False)

            def composition():
                for k in range(K):
                    cipher.scan_dev(keys[k], d_r.ptr, d_k.ptr, d_c.ptr, n, d_out_b.ptr, d_st_b.ptr, want_n_ok=False)

            # ---- correctness first: (b) combined as the header states, then (a) on either path and under every budget
            want_mask, want_m = np.zeros(n, np.uint64), np.zeros((n, L, 4), np.uint64)
            for k in reversed(range(K)):
                cipher.scan_dev(keys[k], d_r.ptr, d_k.ptr, d_c.ptr, n, d_out_b.ptr, d_st_b.ptr, want_n_ok=False)
                st = words32(d_st_b, n)
                assert set(np.unique(st).tolist()) <= {0, 3}
                hit = st == 0
                want_mask[hit] |= np.uint64(1 << k)
                want_m[hit] = d_out_b.to_host().reshape(n, L, 4)[hit]
            want_st = np.where(want_mask != 0, 0, 3).astype(np.uint32)
            assert (want_mask[planted] == np.uint64(1) << owner[planted].astype(np.uint64)).all(), "a planted note was not found"
            assert not want_mask[~planted].any() and want_m[planted].tobytes() == msgs[planted].tobytes()
            paths = [(1, b) for b in (BUDGETS if (n, K) == (1 << 20, 16) else (0,))] + ([(65, 0)] if K <= 4 else [])
            for table_min, budget in paths:
                scan_keys(table_min, budget)
                ctx.sync()
                got = (d_mask.to_host().reshape(-1)[:n], d_out.to_host().reshape(n, L, 4), words32(d_st, n))
                assert all(a.tobytes() == b.tobytes() for a, b in zip(got, (want_mask, want_m, want_st))), (n, K, table_min, budget)

            # ---- then the time
            arms = {"a_table": (TABLE_SCOPES, lambda: scan_keys(1)), "b": (("poseidon_cipher_scan",), composition)}
            if K <= 4:
                arms["a_ladder"] = (LADDER_SCOPES, lambda: scan_keys(65))
            if (n, K) == (1 << 20, 16):
                for mb in BUDGETS[1:]:
                    arms[f"a_table_{mb}mb"] = (TABLE_SCOPES, lambda mb=mb: scan_keys(1, mb))
            res = timed(ctx, arms, CALLS)
            ctx.set_option("cipher_scan_keys_table_min", 0)
            ctx.set_option("cipher_scan_table_mb", 0)
            point = {"n": n, "keys": K, "planted": int(planted.sum())}
            for name, r in res.items():
                point[f"{name}_ms"] = round(statistics.median(r["dev"]), 4)
                point[f"{name}_spread"] = spread(r["dev"])
                point[f"{name}_host_ms"] = round(statistics.median(r["host"]), 4)
                if name != "b":
                    point[f"{name}_split_ms"] = {s.rsplit("_", 1)[1]: round(statistics.median(r[s]), 4) for s in arms[name][0]}
            for name in res:
                if name != "b":
                    point[f"{name}_over_b"] = round(point[f"{name}_ms"] / point["b_ms"], 3)
                    point[f"{name}_over_b_host"] = round(point[f"{name}_host_ms"] / point["b_host_ms"], 3)
            rec["points"].append(point)
            print(json.dumps(point), flush=True)
        for x in (d_e, d_k, d_m, d_r, d_s, d_c, d_out, d_st, d_mask, d_out_b, d_st_b):
            x.free()
    g.free(), hades.free()
    ctx.close()
    line = json.dumps(rec)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
