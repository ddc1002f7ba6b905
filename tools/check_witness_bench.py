"""GPU measurement (not a test): the witness check (pm_plonk_check_witness) beside the proof of the
same witness.  In one process, at 2^12, 2^16 and 2^20 gates, on wide_mixed_circuit (all four widgets: the all-widgets
kernel) and chain_circuit (arithmetic gates only: the kernel without widgets), witness resident on the device:

  check kernel     device events around the one launch of a check (the library's per-kernel timers)
  check call       host clock around pm_plonk_check_witness, which ends in a device synchronise (report download)
  quotient kernel  device events around pm_plonk_quotient_dev inside the proofs
  proof            host clock around pm_plonk_prove

Every arm is warmed up, then repeated until it has at least --seconds of timed calls (and at least 10 calls); the event-timed
runs are separate from the host-timed ones.  Also records the device bytes pm_plonk_key_enable_check holds and the bytes
the check kernel must move per row.  Writes profiles/check_witness_bench.json (or --out).

usage: python tools/check_witness_bench.py [--sizes 12 16 20] [--seconds 0.5] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

TAU = 0x1F2E3D4C5B6A79880123456789ABCDEF0FEDCBA9876543210A1B2C3D4E5F6071


def row_bytes(circuit) -> int:
    """Bytes one row of the check reads and writes: 4 wires + 3 next-row wires + 4 gathered wires + PI + the stored selectors
    (32 each), 4 permutation indices (4 each), 1 mask byte."""
    from plonk_prototype_amd.field import fr_to_limbs
    from plonk_prototype_amd.prover import SELECTORS
    present = {s: getattr(circuit, s) is not None and bool(np.asarray(getattr(circuit, s)).any()) for s in SELECTORS}
    stored = sum(present.values())
    if present["q_arith"] and (np.asarray(circuit.q_arith).reshape(-1, 4) == fr_to_limbs(1)).all():
        stored -= 1                                   # identically one: not stored
    widgets = any(present[s] for s in SELECTORS[7:])
    return 32 * (4 + (3 if widgets else 0) + 4 + 1 + stored) + 16 + 1


def timed(fn, seconds, least=10):
    """-> (seconds per call, calls): fn repeated for at least `seconds` and `least` calls; fn ends synchronised."""
    fn()
    calls, t0 = 0, time.perf_counter()
    while True:
        fn()
        calls += 1
        dt = time.perf_counter() - t0
        if dt >= seconds and calls >= least:
            return dt / calls, calls


def kernel_ms(ctx, name, fn, seconds, least=10):
    """Mean device-event time of the launches named `name` while fn is repeated (fn ends synchronised)."""
    fn()
    ctx.profile(True, only=name)
    calls, t0 = 0, time.perf_counter()
    while calls < least or time.perf_counter() - t0 < seconds:
        fn()
        calls += 1
    stats = ctx.profile_read()
    ctx.profile(False)
    launches, total = stats[name]
    return total / launches, launches


def measure(pa, ctx, ck, label, circuit, d_wit, pi, seconds):
    from plonk_prototype_amd import _lib
    n = circuit.n
    pk = pa.preprocess(circuit, ctx, ck)
    state_bytes = pk.enable_check()
    pos, val = pa.prover.sparse_public_inputs(pi)
    p_pos = pos.ctypes.data_as(_lib.u64p) if pos.size else None
    p_val = val.ctypes.data_as(_lib.u64p) if pos.size else None
    report, proof = _lib.WitnessReport(), _lib.PlonkProof()

    def check():
        ctx._check(ctx._lib.pm_plonk_check_witness(ctx._h, pk._h, d_wit._p, p_pos, p_val, pos.size, C.byref(report), None))

    def prove():
        ctx._check(ctx._lib.pm_plonk_prove(ctx._h, pk._h, ck._bases._h, d_wit._p, p_pos, p_val, pos.size, 0, C.byref(proof)))

    check()
    if report.failed_rows:
        raise SystemExit(f"{label}: the synthetic witness fails the check at row {report.first_row}")
    out = {"circuit": label, "log_n": n.bit_length() - 1, "row_bytes": row_bytes(circuit), "check_state_bytes": state_bytes}
    out["check_kernel_ms"], out["check_kernel_launches"] = kernel_ms(ctx, "plonk_check_witness", check, seconds)
    t, out["check_calls"] = timed(check, seconds)
    out["check_call_ms"] = 1e3 * t
    out["quotient_kernel_ms"], _ = kernel_ms(ctx, "plonk_quotient", prove, seconds, least=5)
    t, out["proofs"] = timed(prove, seconds, least=5)
    out["proof_ms"] = 1e3 * t
    out["check_kernel_gb_per_s"] = out["row_bytes"] * n / out["check_kernel_ms"] / 1e6
    pk.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[12, 16, 20])
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "check_witness_bench.json"))
    args = ap.parse_args()
    import torch  # noqa: F401  (before the library: one HIP runtime per process)
    import plonk_prototype_amd as pa
    ctx = pa.Context(0)
    rows = []
    for lg in sorted(args.sizes):
        n = 1 << lg
        ck = pa.CommitKey.setup(n - 1, pa.field.fr_to_limbs(TAU % pa.field.R_MOD), ctx, precompute=lg >= 10)
        circuit, d_wit, pi = pa.synthetic.wide_mixed_circuit(n, ctx, 1)
        rows.append(measure(pa, ctx, ck, "wide_mixed_circuit", circuit, d_wit, pi, args.seconds))
        d_wit.free()
        print(json.dumps(rows[-1]), flush=True)
        circuit, wit, pi = pa.synthetic.chain_circuit(n, 1)
        d_wit = pa.DeviceVector.from_host(ctx, np.ascontiguousarray(wit).reshape(4 * n, 4))
        rows.append(measure(pa, ctx, ck, "chain_circuit", circuit, d_wit, pi, args.seconds))
        d_wit.free()
        print(json.dumps(rows[-1]), flush=True)
        ck._bases.free()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"rows": rows, "seconds_per_arm": args.seconds}, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
