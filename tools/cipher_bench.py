#!/usr/bin/env python3
"""The Poseidon cipher on JubJub keys: device time per note of pm_poseidon_cipher_encrypt_dev,
pm_poseidon_cipher_decrypt_dev and pm_poseidon_cipher_scan_dev at n = 2^10 .. 2^20, each beside its yardstick:

    decrypt   two permutations as pm_hades_permute_dev's thread form runs them (two calls on n states)
    scan (a)  the call itself
    scan (b)  the composition that existed before it: pm_jubjub_mul_dev with the viewing key replicated n times, then
              pm_poseidon_cipher_decrypt_dev on the products

A developer tool: one GPU, one process.  Before anything is timed, the notes -- made by the device's own encrypt under
S_i = vk R_i -- are scanned both ways: every status is 0, the messages are the ones encrypted and (a) and (b) write the same
bytes; 64 ciphers are compared with the host form.  The arms alternate call by call after one warm-up round; each call is timed
by the library's device events around its launches (the profile scopes of the entry points) and, for the two scans, which
allocate and release their tables, by the host clock around the call and a synchronise as well.  A point reports the median of
CALLS calls per arm and the spread (max - min) / median.

    python tools/cipher_bench.py [--sizes 1024,4096,16384,65536,262144,1048576] [--msg-len 2] [--out profiles/cipher_bench.json]
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

CALLS = 5
ROUNDS, FULL = 67, 8


def random_elements(rng, count):
    """canonical Montgomery limbs: any value below 2^254 is below the modulus"""
    a = rng.integers(0, 1 << 63, size=(count, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(count, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64(0x3fffffffffffffff)
    return a


def spread(xs):
    return round((max(xs) - min(xs)) / statistics.median(xs), 4)


def timed(ctx, arms, calls):
    """arms: {name: (scopes, callable)}; -> ({name: [device ms]}, {name: [host ms]}), the arms alternating, round 0 dropped"""
    dev, wall = {k: [] for k in arms}, {k: [] for k in arms}
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
            total = 0.0
            for scope in scopes:
                now = read[scope][1]
                total += now - seen.get(scope, 0.0)
                seen[scope] = now
            if k:
                dev[name].append(total)
                wall[name].append((t1 - t0) * 1e3)
    ctx.profile(False)
    return dev, wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,4096,16384,65536,262144,1048576")
    ap.add_argument("--msg-len", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cipher_bench.json"))
    args = ap.parse_args()
    L = args.msg_len   # noqa: N806
    ctx = pa.Context(0)
    rng = np.random.default_rng(2026)
    ark, mds = PM.constants(ROUNDS, 1, 0xC1F)
    flat_ark, flat_mds, _ = PM.flat(ark, mds)
    hades = pa.Hades(ctx, flat_ark, flat_mds, ROUNDS, FULL)
    cipher = pa.PoseidonCipher(hades, L)
    g = pa.JubJubBase(ctx, pa.JUBJUB_GENERATOR)
    vk = random_elements(rng, 1)                              # Montgomery limbs
    rec = {"what": "poseidon_cipher", "msg_len": L, "rounds": ROUNDS, "full_rounds": FULL, "calls_per_arm": CALLS, "points": []}
    for n in [int(x) for x in args.sizes.split(",")]:
        d_e, d_k, d_m = (pa.DeviceVector.from_host(ctx, x) for x in (random_elements(rng, n), random_elements(rng, n),
                                                                     random_elements(rng, L * n)))
        d_vk = pa.DeviceVector.from_host(ctx, np.tile(vk, (n, 1)))
        d_r, d_s, d_s2 = pa.DeviceVector(ctx, 2 * n), pa.DeviceVector(ctx, 2 * n), pa.DeviceVector(ctx, 2 * n)
        d_c, d_out, d_out2 = pa.DeviceVector(ctx, (L + 1) * n), pa.DeviceVector(ctx, L * n), pa.DeviceVector(ctx, L * n)
        d_st, d_st2 = pa.DeviceVector(ctx, (n + 7) // 8), pa.DeviceVector(ctx, (n + 7) // 8)
        d_states = pa.DeviceVector.from_host(ctx, random_elements(rng, 5 * n))
        # ---- the notes: R_i = e_i G, S_i = vk R_i, c_i under S_i
        g.mul_dev(d_e.ptr, n, d_r.ptr)
        pa.jubjub_mul_dev(ctx, d_r.ptr, d_vk.ptr, n, d_s.ptr)
        cipher.encrypt_dev(d_s.ptr, d_k.ptr, d_m.ptr, n, d_c.ptr)
        # ---- correctness first
        ok_a = cipher.scan_dev(vk, d_r.ptr, d_k.ptr, d_c.ptr, n, d_out.ptr, d_st.ptr)
        pa.jubjub_mul_dev(ctx, d_r.ptr, d_vk.ptr, n, d_s2.ptr)
        ok_b = cipher.decrypt_dev(d_s2.ptr, d_k.ptr, d_c.ptr, n, d_out2.ptr, d_st2.ptr)
        assert ok_a == n and ok_b == n, (n, ok_a, ok_b)
        msgs = d_m.to_host()
        assert d_out.to_host().tobytes() == msgs.tobytes() and d_out2.to_host().tobytes() == msgs.tobytes(), "a scan's messages"
        assert not d_st.to_host().view(np.uint32).reshape(-1)[:n].any() and d_st.to_host().tobytes() == d_st2.to_host().tobytes()
        sec, non, cts = d_s.to_host().reshape(n, 2, 4), d_k.to_host(), d_c.to_host().reshape(n, L + 1, 4)
        for i in range(0, min(n, 64)):
            host = pa.poseidon_cipher_encrypt_host(flat_ark, flat_mds, sec[i], non[i], msgs.reshape(n, L, 4)[i], msg_len=L)
            assert host.tobytes() == cts[i].tobytes(), "encrypt disagrees with the host form"

        def two_permutations():
            hades.permute_dev(d_states.ptr, n, "thread")
            hades.permute_dev(d_states.ptr, n, "thread")

        def composition():
            pa.jubjub_mul_dev(ctx, d_r.ptr, d_vk.ptr, n, d_s2.ptr)
            cipher.decrypt_dev(d_s2.ptr, d_k.ptr, d_c.ptr, n, d_out2.ptr, d_st2.ptr, want_n_ok=False)

        arms = {"encrypt": (("poseidon_cipher_encrypt",), lambda: cipher.encrypt_dev(d_s.ptr, d_k.ptr, d_m.ptr, n, d_c.ptr)),
                "decrypt": (("poseidon_cipher_decrypt",),
                            lambda: cipher.decrypt_dev(d_s.ptr, d_k.ptr, d_c.ptr, n, d_out.ptr, d_st.ptr, want_n_ok=False)),
                "two_permutations": (("hades_permute",), two_permutations),
                "scan_a": (("poseidon_cipher_scan",),
                           lambda: cipher.scan_dev(vk, d_r.ptr, d_k.ptr, d_c.ptr, n, d_out.ptr, d_st.ptr, want_n_ok=False)),
                "scan_b": (("jubjub_mul", "poseidon_cipher_decrypt"), composition)}
        dev, wall = timed(ctx, arms, CALLS)
        point = {"n": n}
        for name in arms:
            ms = statistics.median(dev[name])
            point.update({f"{name}_ms": round(ms, 4), f"{name}_spread": spread(dev[name]), f"{name}_ns_per_note": round(ms * 1e6 / n, 2)})
        for name in ("scan_a", "scan_b"):
            point[f"{name}_host_ms"] = round(statistics.median(wall[name]), 4)
        point["decrypt_over_two_permutations"] = round(point["decrypt_ms"] / point["two_permutations_ms"], 3)
        point["scan_a_over_b"] = round(point["scan_a_ms"] / point["scan_b_ms"], 3)
        point["scan_a_over_b_host"] = round(point["scan_a_host_ms"] / point["scan_b_host_ms"], 3)
        rec["points"].append(point)
        print(json.dumps(point), flush=True)
        for x in (d_e, d_k, d_m, d_vk, d_r, d_s, d_s2, d_c, d_out, d_out2, d_st, d_st2, d_states):
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
