#!/usr/bin/env python3
"""The variable-base scalar multiplication gadget: filling M multiplications of dusk's size (252 rounds,
1512 rows each) on the GPU, claimed as gadgets of kind 10 (one wave each, one chain in extended coordinates, one inversion a
lane) and claimed in the composed form -- per round a CURVE_ADD, an ARITH run of 2 rows and a CURVE_ADD, on 504 levels, through
the kernels this repository had before, unchanged: the yardstick.  A developer tool: one GPU, one process.

For (M, B) = (1, 1), (3, 16) and (8, 64): M multiplications in one level (circuits of 2^11, 2^13 and 2^14 gates, arithmetic
gates for the rest) and B proofs.  tests/var_base_model.py lays the circuit out and gives the expected values: both forms are
compared with the big-integer model, byte for byte, before anything is timed.  Both keys hold the same rows; the arms alternate
call by call after one warm-up round, each call is timed by the library's device events around the fill's launches (its
profile scope), and a point reports the median of 5 calls per arm and the spread (max - min) / median.  prove_batch of the same
circuit and batch, by the host clock, is what the fill is read against.

    python tools/var_base_bench.py [--points 1:1,3:16,8:64] [--out profiles/var_base_gadget_bench.json]
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
import gadget_model as M  # noqa: E402
import var_base_model as VM  # noqa: E402
import plonk_prototype_amd as pa  # noqa: E402
from plonk_prototype_amd.field import fr_to_limbs  # noqa: E402

R = VM.R
TAU = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % R
ROUNDS = 252
CALLS = 5


def circuit(muls, as_composed):
    rows = muls * VM.ROWS_PER_ROUND * ROUNDS
    b = VM.Builder(1 << max(11, rows.bit_length()))
    one = b.var(True)
    points = [(b.var(True), b.var(True)) for _ in range(muls)]
    bits = [[b.var(True) for _ in range(ROUNDS)] for _ in range(muls)]
    for p, bv in zip(points, bits):
        b.var_base((0, one), bv, p, level=0, as_composed=as_composed)     # from the identity, as dusk starts
    arith = b.fill_arithmetic(1)

    def inputs(seed):
        rng = random.Random(seed)
        a = {one: 1, **arith}
        for p, bv in zip(points, bits):
            a.update(zip(p, M.curve_point(rng.randrange(R))))
            a.update(zip(bv, VM.scalar_bits(rng.randrange(1 << ROUNDS), ROUNDS)))
        return a
    return b, inputs


def spread(xs):
    return round((max(xs) - min(xs)) / statistics.median(xs), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", default="1:1,3:16,8:64")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "var_base_gadget_bench.json"))
    args = ap.parse_args()
    ctx = pa.Context(0)
    rec = {"what": "var_base_gadget_fill", "rounds": ROUNDS, "rows_per_multiplication": VM.ROWS_PER_ROUND * ROUNDS,
           "calls_per_arm": CALLS, "points": []}
    for muls, B in [tuple(int(x) for x in pt.split(":")) for pt in args.points.split(",")]:
        b, inputs = circuit(muls, False)
        b2, _ = circuit(muls, True)                   # the same rows and variable ids, claimed in the composed form
        assert b2.wires == b.wires and b2.sel == b.sel and b2.num_vars == b.num_vars
        n, nv = b.n, b.num_vars
        ck = pa.CommitKey.setup(n + 9, fr_to_limbs(TAU), ctx, precompute=True)
        pk = pa.preprocess(b.circuit(), ctx, ck)
        pk2 = pa.preprocess(b2.circuit(), ctx)
        recs2 = b2.gadget_records()
        table_bytes, table_bytes2 = pk.set_gadgets(b.gadget_records()), pk2.set_gadgets(recs2)
        models = [b.model(inputs(k)) for k in range(2)]
        only = np.ascontiguousarray(np.stack([VM.to_limbs(models[k % 2][0]) for k in range(B)])).reshape(B * nv, 4)
        full = np.ascontiguousarray(np.stack([VM.to_limbs(models[k % 2][1]) for k in range(B)])).reshape(B * nv, 4)
        d, d2 = pa.DeviceVector(ctx, B * nv), pa.DeviceVector(ctx, B * nv)
        raws = (pa._lib.GadgetReport * B)()
        for dv, key, name in ((d, pk, "variable-base"), (d2, pk2, "composed")):
            ctx._check(ctx._lib.pm_dev_upload(ctx._h, dv._p, only.ctypes.data_as(C.c_void_p), only.shape[0] * 32))
            _, reps = key.fill_gadgets(dv)
            assert all(r.ok for r in reps) and np.array_equal(dv.to_host(), full), f"the {name} form disagrees with the model"

        def call(key, dv):
            ctx._check(ctx._lib.pm_plonk_fill_gadgets_dev(ctx._h, key._h, dv._p, nv, B, raws, None))   # waits for the stream

        ctx.profile(True, only="plonk_gadget_fill")
        times, seen, launches = {"chain": [], "composed": []}, 0.0, 0
        for k in range(CALLS + 1):                # round 0 warms both arms up and is dropped
            for arm, key, dv in (("chain", pk, d), ("composed", pk2, d2)):
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
        h, a = statistics.median(times["chain"]), statistics.median(times["composed"])
        rec["points"].append({"multiplications": muls, "log_n": n.bit_length() - 1, "batch": B, "num_vars": nv,
                              "var_base_ms": round(h, 4), "var_base_spread": spread(times["chain"]),
                              "composed_ms": round(a, 4), "composed_spread": spread(times["composed"]),
                              "composed_levels": 1 + max(g.level for g in recs2), "composed_gadgets": len(recs2),
                              "composed_over_var_base": round(a / h, 2),
                              "gap_over_larger_spread": round((a - h) / max(max(times["chain"]) - min(times["chain"]),
                                                                             max(times["composed"]) - min(times["composed"]), 1e-9), 1),
                              "var_base_table_bytes": table_bytes, "composed_table_bytes": table_bytes2,
                              "prove_batch_ms": round(statistics.median(prove[1:]), 3),
                              "var_base_over_prove": round(h / statistics.median(prove[1:]), 5)})
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
