"""GPU measurement (not a test): zero-knowledge proofs (pm_plonk_prove_zk) against plain ones (pm_plonk_prove) on the same
key, witness and commit key, at 2^12, 2^16 and 2^20 gates of boolean_circuit.  Each arm is warmed up, then the two arms
alternate proof by proof until each has --proofs timed proofs; the ZK arm draws fresh blinders per proof (their upload is
part of the call).  Also records the device bytes pm_plonk_key_enable_zk adds.  Writes profiles/zk_bench.json (or --out).

--trace-only LOG_N runs a few ZK proofs at 2^LOG_N and nothing else: the process to put under
`rocprofv3 --kernel-trace --stats -- python tools/zk_bench.py --trace-only 20`.

usage: python tools/zk_bench.py [--sizes 12 16 20] [--proofs 20] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402,F401  (the library binds to torch's HIP runtime, as in bench.py)

import plonk_prototype_amd as pa  # noqa: E402
import plonk_prototype_amd.prover as PR  # noqa: E402
from plonk_prototype_amd.host import DeviceVector  # noqa: E402
from plonk_prototype_amd.field import fr_to_limbs  # noqa: E402

TAU = 0x1F2E3D4C5B6A79880F1E2D3C4B5A6978  # any scalar: timings do not depend on it


def setup(ctx, log_n):
    n = 1 << log_n
    circuit, wit, pub = pa.synthetic.boolean_circuit(n, 1)
    ck = pa.CommitKey.setup(n + 9, fr_to_limbs(TAU), ctx, precompute=True)
    pk = pa.preprocess(circuit, ctx, ck)
    ctx.sync()
    free0 = torch.cuda.mem_get_info(0)[0]
    added = pk.enable_zk()
    ctx.sync()
    used = free0 - torch.cuda.mem_get_info(0)[0]
    d_wit = DeviceVector.from_host(ctx, wit.reshape(4 * n, 4))
    return n, ck, pk, d_wit, pub, added, used


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms),
            "p10_ms": sorted(ms)[len(ms) // 10], "p90_ms": sorted(ms)[(9 * len(ms)) // 10], "count": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[12, 16, 20])
    ap.add_argument("--proofs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "zk_bench.json"))
    ap.add_argument("--trace-only", type=int, default=None)
    args = ap.parse_args()
    ctx = pa.Context(0)
    if args.trace_only is not None:
        n, ck, pk, d_wit, pub, _, _ = setup(ctx, args.trace_only)
        for _ in range(3):
            PR.prove(pk, ck, d_wit, pub, zero_knowledge=True)
        return
    rows = []
    for log_n in args.sizes:
        n, ck, pk, d_wit, pub, added, used = setup(ctx, log_n)
        arms = {"plain": lambda: PR.prove(pk, ck, d_wit, pub),
                "zk": lambda: PR.prove(pk, ck, d_wit, pub, zero_knowledge=True)}
        for f in arms.values():
            for _ in range(args.warmup):
                f()
        times = {k: [] for k in arms}
        for _ in range(args.proofs):
            for k, f in arms.items():
                t0 = time.perf_counter()
                f()
                times[k].append((time.perf_counter() - t0) * 1e3)
        row = {"log_n": log_n, "gates": n, "enable_zk_bytes": added, "device_bytes_taken": used,
               "plain": stats(times["plain"]), "zk": stats(times["zk"])}
        row["zk_over_plain"] = row["zk"]["median_ms"] / row["plain"]["median_ms"]
        print(json.dumps(row), flush=True)
        rows.append(row)
        d_wit.free()
        pk.free()
        del ck
    out = {"what": "pm_plonk_prove_zk vs pm_plonk_prove, boolean_circuit, one MI355X, wall time per call from the host",
           "proofs_per_arm": args.proofs, "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
