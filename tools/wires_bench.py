#!/usr/bin/env python3
"""Composer-form circuits: what the wire-variable path costs against the path it replaces.  A
developer tool: one GPU, one process, the measurements of a size alternate round by round and the medians are reported.

  (a) sigma_index on the host with numpy (synthetic._sigma_cycles) + pm_plonk_preprocess       -- the index path
  (b) pm_plonk_preprocess_wires                                                                -- the wire path
  (s) pm_plonk_sigma_from_wires_dev alone (device in, device out): the sort and the link
  (c) dense witness upload  vs  variable upload + pm_plonk_witness_from_vars_dev, B = 1 and 16 (n <= 2^20)

on two wire maps per size: the one of synthetic.wide_circuit (2n variables, every pool variable at 2-4 positions) and the
one of synthetic.boolean_circuit (n + 1 variables, one of them at about n positions).  Selectors are random limbs (wide) or
the boolean circuit's; the witness values are random limbs -- nothing here proves anything.

    python tools/wires_bench.py [--log-sizes 16 20 22] [--rounds 5] [--out profiles/wires_bench.txt]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import plonk_prototype_amd as pa  # noqa: E402
from plonk_prototype_amd.field import R_MOD, fr_to_limbs  # noqa: E402
from plonk_prototype_amd.synthetic import _random_fr, _sigma_cycles, boolean_circuit_wires  # noqa: E402


def wire_map(shape: str, n: int):
    """-> (selector dict, wire_vars [4, n] uint32, num_vars)"""
    if shape == "boolean":
        c, _, _ = boolean_circuit_wires(n, 1)
        return {k: getattr(c, k) for k in pa.prover.SELECTORS}, c.wire_vars, c.num_vars
    rng = np.random.default_rng(n)
    ar = np.arange(n, dtype=np.int64)
    var = np.concatenate([ar, (5 * ar + 1) % n, n + ar, ar // 2])
    sel = {k: _random_fr(rng, n) for k in ("q_m", "q_l", "q_r", "q_4", "q_c")}
    sel.update(q_o=np.tile(fr_to_limbs(R_MOD - 1), (n, 1)), q_arith=np.tile(fr_to_limbs(1), (n, 1)))
    return sel, var.astype(np.uint32).reshape(4, n), 2 * n


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-sizes", type=int, nargs="+", default=[16, 20, 22])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = pa.Context(0)
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    for log_n in args.log_sizes:
        n = 1 << log_n
        for shape in ("wide", "boolean"):
            sel, wv, num_vars = wire_map(shape, n)
            flat = wv.reshape(-1).astype(np.int64)
            t = {"numpy_sigma": [], "preprocess_index": [], "preprocess_wires": [], "sort_link": []}
            d_w, d_s = C.c_void_p(), C.c_void_p()
            ctx._check(ctx._lib.pm_dev_alloc(ctx._h, 4 * n * 4, C.byref(d_w)))
            ctx._check(ctx._lib.pm_dev_alloc(ctx._h, 4 * n * 8, C.byref(d_s)))
            ctx._check(ctx._lib.pm_dev_upload(ctx._h, d_w, wv.ctypes.data_as(C.c_void_p), 4 * n * 4))
            for rnd in range(args.rounds + 1):                 # round 0 warms up (module load, first allocations)
                ms_np, sigma = timed(lambda: _sigma_cycles(flat))
                ms_a, pk = timed(lambda: pa.ProverKey(pa.Circuit(sigma_index=sigma.reshape(4, n), **sel), ctx))
                pk.free()
                ms_b, pk = timed(lambda: pa.ProverKey(pa.Circuit(wire_vars=wv, num_vars=num_vars, **sel), ctx))
                pk.free()
                ms_s, rc = timed(lambda: ctx._lib.pm_plonk_sigma_from_wires_dev(ctx._h, d_w, num_vars, n, d_s, None))
                ctx._check(rc)
                if rnd:
                    for k, v in (("numpy_sigma", ms_np), ("preprocess_index", ms_a), ("preprocess_wires", ms_b), ("sort_link", ms_s)):
                        t[k].append(round(v, 3))
            ctx._lib.pm_dev_free(ctx._h, d_w)
            ctx._lib.pm_dev_free(ctx._h, d_s)
            med = {k: round(statistics.median(v), 3) for k, v in t.items()}
            emit({"what": "build", "log_n": log_n, "shape": shape, "num_vars": num_vars, "vars_per_position": num_vars / (4 * n),
                  "median_ms": dict(med, index_path=round(med["numpy_sigma"] + med["preprocess_index"], 3),
                                    wire_path=med["preprocess_wires"]), "rounds_ms": t})
            if log_n > 20:
                continue
            pk = pa.ProverKey(pa.Circuit(wire_vars=wv, num_vars=num_vars, **sel), ctx)
            rng = np.random.default_rng(log_n)
            for B in (1, 16):
                variables = _random_fr(rng, B * num_vars)
                dense = np.ascontiguousarray(variables.reshape(B, num_vars, 4)[:, wv.reshape(-1)]).reshape(B * 4 * n, 4)
                d_dense, d_vars, d_out = pa.DeviceVector(ctx, B * 4 * n), pa.DeviceVector(ctx, B * num_vars), pa.DeviceVector(ctx, B * 4 * n)
                up = lambda dst, a: ctx._check(ctx._lib.pm_dev_upload(ctx._h, dst._p, a.ctypes.data_as(C.c_void_p), a.shape[0] * 32))   # noqa: E731
                td, tv = [], []

                def from_vars():
                    up(d_vars, variables)
                    ctx._check(ctx._lib.pm_plonk_witness_from_vars_dev(ctx._h, pk._h, d_vars._p, num_vars, B, d_out._p, None))
                    ctx.sync()

                for rnd in range(args.rounds + 1):
                    ms_d, _ = timed(lambda: up(d_dense, dense))
                    ms_v, _ = timed(from_vars)
                    if rnd:
                        td.append(round(ms_d, 3))
                        tv.append(round(ms_v, 3))
                assert np.array_equal(d_out.to_host(), dense)
                for v in (d_dense, d_vars, d_out):
                    v.free()
                emit({"what": "witness", "log_n": log_n, "shape": shape, "batch": B, "vars_per_position": num_vars / (4 * n),
                      "dense_bytes": B * 4 * n * 32, "variable_bytes": B * num_vars * 32,
                      "median_ms": {"dense_upload": round(statistics.median(td), 3),
                                    "variables_upload_and_expand": round(statistics.median(tv), 3)},
                      "rounds_ms": {"dense_upload": td, "variables_upload_and_expand": tv}})
            pk.free()
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
