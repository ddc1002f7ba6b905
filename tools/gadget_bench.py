#!/usr/bin/env python3
"""Gadget witnesses: what filling the widget rows on the GPU costs, read against the proof of the same
batch in the same run.  A developer tool: one GPU, one process.

The circuit has 2^12 gates shaped like the reference's use of its gadgets: three 256-round fixed-base multiplications, one curve
addition of two of the results, two 64-bit ranges, arithmetic gates for the rest (tests/gadget_model.py lays it out and gives the
expected values: every filled assignment is compared with the big-integer model before anything is timed).

For B = 1, 16 and 64, after a warm-up:
  fill_event_ms       the launches of pm_plonk_fill_gadgets_dev by device events (the library's profile scope)
  fill_call_ms        the call with reports (it waits for the stream) by the host clock
  upload_full_ms      upload of B full assignments, B x num_vars x 32 bytes: what a caller sends today, with or without the fill
                      (the fill works in place on one value per variable)
  upload_inputs_ms    upload of as many bytes as the INPUTS of B assignments have (gadget inputs and the arithmetic gates'
                      variables, B x inputs x 32 bytes, one copy): what a caller whose inputs have the lowest ids could send
  prove_batch_ms      prove_batch of the same batch from filled device variables
  model_ms_per_witness  the big-integer model of this tool filling one assignment on one host core (Python integers: an upper
                      bound for a host implementation, not a baseline)

    python tools/gadget_bench.py [--seconds 0.5] [--out profiles/gadget_bench.json]
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
import plonk_prototype_amd as pa  # noqa: E402
from plonk_prototype_amd.field import fr_to_limbs  # noqa: E402

TAU = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % M.R


def circuit(n):
    b = M.Builder(n)
    sc = [b.var(True) for _ in range(3)]
    rv = [b.var(True) for _ in range(2)]
    one = b.var(True)                               # the y of the identity, shared by the three start points
    pts = [b.fixed_base(s, 256, (0, one), level=0, table_seed=0x1234567 + k) for k, s in enumerate(sc)]
    b.curve_add(pts[0], pts[1], level=1)
    for v in rv:
        b.equal(v, b.range(v, 8, level=2))
    arith = b.fill_arithmetic(1)

    def inputs(seed):
        rng = random.Random(seed)
        return {**{s: rng.randrange(M.R) for s in sc}, **{v: rng.getrandbits(64) for v in rv}, one: 1, **arith}
    return b, inputs, len(sc) + len(rv) + 1


def repeat(fn, seconds, least=10):
    fn()
    times = []
    t_end = time.perf_counter() + seconds
    while len(times) < least or time.perf_counter() < t_end:
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(times), 4), len(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--log-n", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gadget_bench.json"))
    args = ap.parse_args()
    n = 1 << args.log_n
    ctx = pa.Context(0)
    b, inputs, real_inputs = circuit(n)
    ck = pa.CommitKey.setup(n + 9, fr_to_limbs(TAU), ctx, precompute=True)
    pk = pa.preprocess(b.circuit(), ctx, ck)
    table_bytes = pk.set_gadgets(b.gadget_records())
    nv = b.num_vars
    t0 = time.perf_counter()
    models = [b.model(inputs(k)) for k in range(4)]
    model_ms = (time.perf_counter() - t0) * 1e3 / 4
    rec = {"what": "gadget_fill", "log_n": args.log_n, "num_vars": nv, "gadgets": len(b.gadgets), "table_bytes": table_bytes,
           "inputs_used": real_inputs, "arithmetic_inputs": len(b.inputs) - 1 - real_inputs,
           "model_ms_per_witness": round(model_ms, 2), "batches": []}
    for B in (1, 16, 64):
        only = np.ascontiguousarray(np.stack([M.to_limbs(models[k % 4][0]) for k in range(B)])).reshape(B * nv, 4)
        full = np.ascontiguousarray(np.stack([M.to_limbs(models[k % 4][1]) for k in range(B)])).reshape(B * nv, 4)
        d = pa.DeviceVector(ctx, B * nv)
        up = lambda a: ctx._check(ctx._lib.pm_dev_upload(ctx._h, d._p, a.ctypes.data_as(C.c_void_p), a.shape[0] * 32))   # noqa: E731
        up(only)
        _, reps = pk.fill_gadgets(d)
        assert all(r.ok for r in reps) and np.array_equal(d.to_host(), full), "the fill disagrees with the model"
        raws = (pa._lib.GadgetReport * B)()

        def fill():
            ctx._check(ctx._lib.pm_plonk_fill_gadgets_dev(ctx._h, pk._h, d._p, nv, B, raws, None))

        fill_call, calls = repeat(fill, args.seconds)
        ctx.profile(True, only="plonk_gadget_fill")
        repeat(fill, args.seconds)
        launches, total = ctx.profile_read()["plonk_gadget_fill"]
        ctx.profile(False)
        n_in = len(b.inputs)
        up_only, _ = repeat(lambda: (up(only[:B * n_in]), ctx.sync()), args.seconds)
        up_full, _ = repeat(lambda: (up(full), ctx.sync()), args.seconds)
        ws = pk.batch(B)
        prove, proofs = repeat(lambda: pa.prove_batch(pk, ck, variables=d, workspace=ws), max(args.seconds, 1.0), least=5)
        ws.free()
        d.free()
        rec["batches"].append({"batch": B, "fill_event_ms": round(total / launches, 4), "fill_call_ms": fill_call,
                               "fill_calls": calls, "upload_inputs_ms": up_only, "upload_full_ms": up_full,
                               "upload_full_bytes": B * nv * 32, "upload_inputs_bytes": B * n_in * 32,
                               "prove_batch_ms": prove, "prove_batch_calls": proofs,
                               "fill_over_prove": round(total / launches / prove, 4)})
    pk.free()
    ctx.close()
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
