"""The Lagrange-form commit key, measured in one process; writes one JSON file.

  conversion   pm_g1_bases_lagrange at each --conv size: device time from the library's event pair around the launches
               (ctx.profile, kernel "g1_ec_ntt"), wall time around the call (it synchronises before returning), and the
               achieved group operations per second (~(n/2) log_n twiddle products of ~254 doublings + ~127 additions,
               + the n/2 log_n butterfly additions), set against the fixed-base SRS generation rate (pm_g1_fixed_base_mul_dev:
               <= 32 mixed additions per point) measured in the same run
  proof        prove() at --prove-log gates with and without the key attached, on chain_circuit (uniform witness) and
               boolean_circuit (bits): every shape warmed up, the two arms alternated, --reps proofs per arm; median,
               min, max and the spread (max - min) / median
  memory       HBM in use (hipMemGetInfo through torch) with the key attached, at each --mem size

usage: python tools/lagrange_bench.py [--conv 16,20,24] [--prove-log 20] [--reps 20] [--mem 20,24] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch  # noqa: F401  (first: one HIP runtime in the process)
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import plonk_prototype_amd as pa  # noqa: E402
import plonk_prototype_amd.prover as PR  # noqa: E402
from plonk_prototype_amd.field import fr_to_limbs  # noqa: E402

TAU = fr_to_limbs(0x5DEECE66D1234567890ABCDEF0123456789ABCDEF)


def hbm_used():
    free, total = torch.cuda.mem_get_info(0)
    return total - free


def conversion(ctx, log_n):
    n = 1 << log_n
    ck = pa.CommitKey.setup(n - 1, TAU, ctx)
    out = pa.DeviceVector(ctx, 3 * n)
    try:
        ctx.profile(True, "g1_ec_ntt")
        t0 = time.perf_counter()
        ctx._check(ctx._lib.pm_g1_bases_lagrange(ctx._h, ck._bases._h, log_n, out._p, None))
        ctx.sync()
        wall = time.perf_counter() - t0
        prof = ctx.profile_read()
        ctx.profile(False)
        dev_ms = prof.get("g1_ec_ntt", (0, float("nan")))[1]
    finally:
        out.free()
    # the fixed-base SRS generation of the same n, for the rate comparison
    ctx.profile(True, "g1_fixed_base_mul")
    ck2 = pa.CommitKey.setup(n - 1, TAU, ctx)
    fb_ms = ctx.profile_read().get("g1_fixed_base_mul", (0, float("nan")))[1]
    ctx.profile(False)
    del ck, ck2
    muls = (n // 2) * max(log_n - 1, 0) + n   # stages 2.. have twiddles (k = 0 skipped: ~half of stage 2's), last stage scales a too
    group_ops = muls * (254 + 127) + (n // 2) * log_n * 2
    return {"log_n": log_n, "device_ms": dev_ms, "wall_ms": wall * 1e3,
            "group_ops_estimate": group_ops, "group_ops_per_s": group_ops / (dev_ms * 1e-3),
            "fixed_base_srs_ms": fb_ms, "fixed_base_group_ops_per_s": n * 32 / (fb_ms * 1e-3)}


def proof_times(ctx, log_n, reps):
    n = 1 << log_n
    ck = pa.CommitKey.setup(n - 1, TAU, ctx, precompute=True)
    lck = ck.lagrange(log_n)
    res = {}
    for name, make in (("chain_circuit", pa.synthetic.chain_circuit), ("boolean_circuit", pa.synthetic.boolean_circuit)):
        circuit, wit, pub = make(n, 1)
        pk = PR.preprocess(circuit, ctx, ck)
        d_wit = pa.DeviceVector.from_host(ctx, np.ascontiguousarray(wit).reshape(4 * n, 4))
        times = {"plain": [], "lagrange": []}
        ref = None
        for it in range(reps + 3):                 # 3 warm-up rounds of both arms
            for arm in ("plain", "lagrange"):
                pk.use_lagrange(ck, lck if arm == "lagrange" else None)
                ctx.sync()
                t0 = time.perf_counter()
                p = PR.prove(pk, ck, d_wit, pub)
                ctx.sync()
                dt = (time.perf_counter() - t0) * 1e3
                ref = ref or p.native_bytes
                assert p.native_bytes == ref, "proof bytes differ between the arms"
                if it >= 3:
                    times[arm].append(dt)
        res[name] = {arm: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v),
                           "spread": (max(v) - min(v)) / statistics.median(v), "n": len(v)}
                     for arm, v in times.items()}
        res[name]["saving_ms_median"] = res[name]["plain"]["median_ms"] - res[name]["lagrange"]["median_ms"]
        pk.use_lagrange(ck, None)
        d_wit.free()
        pk.free()
    return res


def memory(ctx, log_n):
    n = 1 << log_n
    circuit, _, _ = pa.synthetic.boolean_circuit(n, 1)
    base = hbm_used()
    ck = pa.CommitKey.setup(n - 1, TAU, ctx, precompute=True)
    pk = PR.preprocess(circuit, ctx, ck)
    ctx.sync()
    without = hbm_used()
    lck = ck.lagrange(log_n)
    pk.use_lagrange(ck, lck)
    ctx.sync()
    with_key = hbm_used()
    pk.free()
    return {"log_n": log_n, "hbm_bytes_ck_and_prover_key": without - base, "hbm_bytes_with_lagrange_key": with_key - base,
            "lagrange_key_bytes": with_key - without}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--conv", default="16,20,24")
    ap.add_argument("--prove-log", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--mem", default="20,24")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "lagrange_bench.json"))
    a = ap.parse_args()
    ctx = pa.Context(0)
    out = {"conversion": [], "proof": None, "memory": []}
    for k in [int(x) for x in a.conv.split(",") if x]:
        out["conversion"].append(conversion(ctx, k))
        print(json.dumps(out["conversion"][-1]), flush=True)
    if a.prove_log:
        out["proof"] = {"log_n": a.prove_log, **proof_times(ctx, a.prove_log, a.reps)}
        print(json.dumps(out["proof"]), flush=True)
    for k in [int(x) for x in a.mem.split(",") if x]:
        out["memory"].append(memory(ctx, k))
        print(json.dumps(out["memory"][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
