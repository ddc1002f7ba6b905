#!/usr/bin/env python3
"""Composed gadget witnesses: what filling arithmetic-row gadgets on the GPU costs, read against the
upload it replaces and the proof of the same batch in the same run.  A developer tool: one GPU, one process.

The circuit has 2^12 gates: eight range checks between 64-bit bounds (two 64-bit decompositions with their comparisons and
three glue rows each) and one 255-bit decomposition, arithmetic gates for the rest (tests/composed_gadget_model.py lays it out
and gives the expected values: every filled assignment is compared with the big-integer model before anything is timed).

For B = 1, 16 and 64, after a warm-up, the median of at least 10:
  fill_event_ms         the launches of one pm_plonk_fill_gadgets_dev call by device events (the library's profile scope, read
                        after every call)
  fill_call_ms          the call with reports (it waits for the stream) by the host clock
  upload_full_ms        upload of B full assignments, B x num_vars x 32 bytes: what a caller sends without the fill
  upload_inputs_ms      upload of as many bytes as the INPUTS of B assignments have
  prove_batch_ms        prove_batch of the same batch from filled device variables
  arith_form_event_ms   the same circuit with every BITS gadget claimed as ONE ARITH run of its 2 B rows and the bits given as
                        inputs: the sequential form of the identical computation, by device events

    python tools/composed_gadget_bench.py [--seconds 0.5] [--out profiles/composed_gadget_bench.json]
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
import composed_gadget_model as CM  # noqa: E402
import plonk_prototype_amd as pa  # noqa: E402
from plonk_prototype_amd.field import fr_to_limbs  # noqa: E402

R = CM.R
TAU = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % R
LO, HI = 1000, (1 << 64) - 5


def circuit(n, as_arith):
    b = CM.Builder(n)
    b.bits_as_arith = as_arith
    xs = [b.var(True) for _ in range(8)]
    s = b.var(True)
    for x in xs:
        b.range_check(LO, HI, x, level=0)
    b.decomposition(s, 255, level=0)
    arith = b.fill_arithmetic(1)

    def inputs(seed):
        rng = random.Random(seed)
        return {**{x: rng.randrange(LO, HI) for x in xs}, s: rng.randrange(R), **arith}
    return b, inputs, len(xs) + 1


def repeat(fn, seconds, least=10):
    fn()
    times = []
    t_end = time.perf_counter() + seconds
    while len(times) < least or time.perf_counter() < t_end:
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(times), 4), len(times)


def event_ms(ctx, fn, seconds, least=10):
    """device time of the fill's launches in one call (the library's profile scope: events around the launches): the scope's
    running total is read after every call, the first call is a warm-up and dropped, the median of the rest is returned"""
    ctx.profile(True, only="plonk_gadget_fill")
    times, seen = [], 0.0
    t_end = time.perf_counter() + seconds
    while len(times) < least + 1 or time.perf_counter() < t_end:
        fn()                                          # the call with reports waits for the stream
        launches, total = ctx.profile_read()["plonk_gadget_fill"]
        assert launches == len(times) + 1
        times.append(total - seen)
        seen = total
    ctx.profile(False)
    return round(statistics.median(times[1:]), 4), len(times) - 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--log-n", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "composed_gadget_bench.json"))
    args = ap.parse_args()
    n = 1 << args.log_n
    ctx = pa.Context(0)
    b, inputs, real_inputs = circuit(n, False)
    b2, _, _ = circuit(n, True)                       # the same rows and variable ids, the bits as inputs of ARITH runs
    assert b2.num_vars == b.num_vars and b2.wires == b.wires and b2.bit_vars == b.bit_vars
    ck = pa.CommitKey.setup(n + 9, fr_to_limbs(TAU), ctx, precompute=True)
    pk = pa.preprocess(b.circuit(), ctx, ck)
    pk2 = pa.preprocess(b2.circuit(), ctx)
    table_bytes = pk.set_gadgets(b.gadget_records())
    table_bytes2 = pk2.set_gadgets(b2.gadget_records())
    nv = b.num_vars
    t0 = time.perf_counter()
    models = [b.model(inputs(k)) for k in range(4)]
    model_ms = (time.perf_counter() - t0) * 1e3 / 4
    kinds = {}
    for g in b.gadgets:
        kinds[g[0]] = kinds.get(g[0], 0) + 1
    rec = {"what": "composed_gadget_fill", "log_n": args.log_n, "num_vars": nv, "gadgets": kinds, "table_bytes": table_bytes,
           "arith_form_table_bytes": table_bytes2, "levels": len(set(g[1] for g in b.gadgets)),
           "inputs_used": real_inputs, "arithmetic_inputs": len(b.inputs) - 1 - real_inputs,
           "bit_variables": len(b.bit_vars), "model_ms_per_witness": round(model_ms, 2), "batches": []}
    for B in (1, 16, 64):
        only = np.ascontiguousarray(np.stack([CM.to_limbs(models[k % 4][0]) for k in range(B)])).reshape(B * nv, 4)
        full = np.ascontiguousarray(np.stack([CM.to_limbs(models[k % 4][1]) for k in range(B)])).reshape(B * nv, 4)
        with_bits = only.reshape(B, nv, 4).copy()     # the ARITH form's inputs: the bits too
        with_bits[:, b.bit_vars] = full.reshape(B, nv, 4)[:, b.bit_vars]
        with_bits = np.ascontiguousarray(with_bits).reshape(B * nv, 4)
        d = pa.DeviceVector(ctx, B * nv)
        up = lambda a: ctx._check(ctx._lib.pm_dev_upload(ctx._h, d._p, a.ctypes.data_as(C.c_void_p), a.shape[0] * 32))   # noqa: E731
        raws = (pa._lib.GadgetReport * B)()
        # the sequential form first: same bytes as the model
        up(with_bits)
        _, reps = pk2.fill_gadgets(d)
        assert all(r.ok for r in reps) and np.array_equal(d.to_host(), full), "the ARITH form disagrees with the model"
        arith_form, _ = event_ms(ctx, lambda: ctx._check(ctx._lib.pm_plonk_fill_gadgets_dev(ctx._h, pk2._h, d._p, nv, B, raws, None)),
                                 args.seconds)
        up(only)
        _, reps = pk.fill_gadgets(d)
        assert all(r.ok for r in reps) and np.array_equal(d.to_host(), full), "the fill disagrees with the model"

        def fill():
            ctx._check(ctx._lib.pm_plonk_fill_gadgets_dev(ctx._h, pk._h, d._p, nv, B, raws, None))

        fill_call, calls = repeat(fill, args.seconds)
        fill_event, event_calls = event_ms(ctx, fill, args.seconds)
        n_in = len(b.inputs)
        up_only, _ = repeat(lambda: (up(only[:B * n_in]), ctx.sync()), args.seconds)
        up_full, _ = repeat(lambda: (up(full), ctx.sync()), args.seconds)
        ws = pk.batch(B)
        prove, proofs = repeat(lambda: pa.prove_batch(pk, ck, variables=d, workspace=ws), max(args.seconds, 1.0), least=10)
        ws.free()
        d.free()
        rec["batches"].append({"batch": B, "fill_event_ms": fill_event, "fill_call_ms": fill_call, "fill_calls": calls, "fill_event_calls": event_calls,
                               "arith_form_event_ms": arith_form, "upload_inputs_ms": up_only, "upload_full_ms": up_full,
                               "upload_full_bytes": B * nv * 32, "upload_inputs_bytes": B * n_in * 32,
                               "prove_batch_ms": prove, "prove_batch_calls": proofs,
                               "fill_over_prove": round(fill_event / prove, 4),
                               "arith_form_over_fill": round(arith_form / fill_event, 2)})
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
