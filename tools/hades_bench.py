#!/usr/bin/env python3
"""The HADES gadget: filling P Hades permutations of dusk's size (67 rounds, 8 full, 1302 rows each) on
the GPU, claimed as HADES gadgets (one wave each) and claimed as one ARITH run each (one thread each -- the kernel this
repository had before, unchanged: the yardstick).  A developer tool: one GPU, one process.

For P = 1, 8 and 32 permutations in one level (circuits of 2^11, 2^14 and 2^16 gates, arithmetic gates for the rest) and
B = 1, 16 and 64 proofs.  tests/hades_model.py lays the circuit out and gives the expected values: both forms are compared with
the big-integer model, byte for byte, before anything is timed.  Both keys hold the same rows; the arms alternate call by call
after one warm-up round, each call is timed by the library's device events around the fill's launches (its profile scope),
and a point reports the median of 5 calls per arm and the spread (max - min) / median.  prove_batch of the same circuit and
batch, by the host clock, is what the fill is read against.

    python tools/hades_bench.py [--perms 1,8,32] [--batches 1,16,64] [--out profiles/hades_gadget_bench.json]
"""
import argparse
import ctypes as C
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
import hades_model as HM  # noqa: E402
import plonk_prototype_amd as pa  # noqa: E402
from plonk_prototype_amd.field import fr_to_limbs  # noqa: E402

R = HM.R
TAU = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % R
ROUNDS, FULL = 67, 8
CALLS = 5


def circuit(perms, as_arith):
    rows = perms * HM.hades_rows(ROUNDS, FULL)
    b = HM.Builder(1 << max(11, rows.bit_length()))
    states = [[b.var(True) for _ in range(5)] for _ in range(perms)]
    for st in states:
        b.hades(st, ROUNDS, FULL, level=0, as_arith=as_arith)
    arith = b.fill_arithmetic(1)

    def inputs(seed):
        rng = random.Random(seed)
        return {**{v: rng.randrange(R) for st in states for v in st}, **arith}
    return b, inputs


def spread(xs):
    return round((max(xs) - min(xs)) / statistics.median(xs), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--perms", default="1,8,32")
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hades_gadget_bench.json"))
    args = ap.parse_args()
    ctx = pa.Context(0)
    rec = {"what": "hades_gadget_fill", "rounds": ROUNDS, "full_rounds": FULL, "rows_per_permutation": HM.hades_rows(ROUNDS, FULL),
           "calls_per_arm": CALLS, "points": []}
    for perms in [int(x) for x in args.perms.split(",")]:
        b, inputs = circuit(perms, False)
        b2, _ = circuit(perms, True)                  # the same rows and variable ids, claimed as ARITH runs
        assert b2.wires == b.wires and b2.sel == b.sel and b2.num_vars == b.num_vars
        n, nv = b.n, b.num_vars
        ck = pa.CommitKey.setup(n + 9, fr_to_limbs(TAU), ctx, precompute=True)
        pk = pa.preprocess(b.circuit(), ctx, ck)
        pk2 = pa.preprocess(b2.circuit(), ctx)
        table_bytes, table_bytes2 = pk.set_gadgets(b.gadget_records()), pk2.set_gadgets(b2.gadget_records())
        models = [b.model(inputs(k)) for k in range(2)]
        for B in [int(x) for x in args.batches.split(",")]:
            only = np.ascontiguousarray(np.stack([HM.to_limbs(models[k % 2][0]) for k in range(B)])).reshape(B * nv, 4)
            full = np.ascontiguousarray(np.stack([HM.to_limbs(models[k % 2][1]) for k in range(B)])).reshape(B * nv, 4)
            d, d2 = pa.DeviceVector(ctx, B * nv), pa.DeviceVector(ctx, B * nv)
            raws = (pa._lib.GadgetReport * B)()
            for dv, key, name in ((d, pk, "HADES"), (d2, pk2, "ARITH")):
                ctx._check(ctx._lib.pm_dev_upload(ctx._h, dv._p, only.ctypes.data_as(C.c_void_p), only.shape[0] * 32))
                _, reps = key.fill_gadgets(dv)
                assert all(r.ok for r in reps) and np.array_equal(dv.to_host(), full), f"the {name} form disagrees with the model"

            def call(key, dv):
                ctx._check(ctx._lib.pm_plonk_fill_gadgets_dev(ctx._h, key._h, dv._p, nv, B, raws, None))   # waits for the stream

            ctx.profile(True, only="plonk_gadget_fill")
            times, seen, launches = {"hades": [], "arith": []}, 0.0, 0
            for k in range(CALLS + 1):                # round 0 warms both arms up and is dropped
                for arm, key, dv in (("hades", pk, d), ("arith", pk2, d2)):
                    call(key, dv)
                    count, total = ctx.profile_read()["plonk_gadget_fill"]
                    launches += 1
                    assert count == launches
                    if k:
                        times[arm].append(total - seen)
                    seen = total
            ctx.profile(False)
            ws = pk.batch(B)
            prove = []
            for k in range(4):
                t0 = time.perf_counter()
                pa.prove_batch(pk, ck, variables=d, workspace=ws)
                prove.append((time.perf_counter() - t0) * 1e3)
            ws.free()
            d.free()
            d2.free()
            h, a = statistics.median(times["hades"]), statistics.median(times["arith"])
            rec["points"].append({"permutations": perms, "log_n": n.bit_length() - 1, "batch": B, "num_vars": nv,
                                  "hades_ms": round(h, 4), "hades_spread": spread(times["hades"]),
                                  "arith_ms": round(a, 4), "arith_spread": spread(times["arith"]),
                                  "arith_over_hades": round(a / h, 2),
                                  "gap_over_larger_spread": round((a - h) / max(max(times["hades"]) - min(times["hades"]),
                                                                                 max(times["arith"]) - min(times["arith"]), 1e-9), 1),
                                  "hades_table_bytes": table_bytes, "arith_table_bytes": table_bytes2,
                                  "prove_batch_ms": round(statistics.median(prove[1:]), 3),
                                  "hades_over_prove": round(h / statistics.median(prove[1:]), 5)})
            print(json.dumps(rec["points"][-1]), flush=True)
        pk.free()
        pk2.free()
    ctx.close()
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
