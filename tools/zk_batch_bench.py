"""GPU measurement (not a test): zero-knowledge proofs in the batch prover.  In one process, at 2^12, 2^14 and 2^16 gates:
sequential pm_plonk_prove_zk (what a caller had before), pm_plonk_prove_batch at B in {4, 16, 64} (the cost of blinding
inside a batch) and pm_plonk_prove_batch_zk at B in {1, 4, 16, 64}.  Witnesses: distinct boolean_circuit seeds of one
circuit, resident on the device.  Every zero-knowledge call gets fresh blinders (drawn before its timer starts: the draw is
the caller's work in every arm; their upload is part of the call).  Every arm is warmed up, then the arms alternate in
rounds until each has at least --seconds of timed calls; wall time per call from the host.  Also records the device bytes
pm_plonk_batch_enable_zk adds per proof.  Writes profiles/zk_batch_bench.json (or --out).

--trace-only LOG_N B CALLS runs the setup, CALLS zero-knowledge batches of B and nothing else: the process to put under
`rocprofv3 --kernel-trace --stats`; --trace-report A.csv B.csv C.csv turns the kernel_stats files of the runs
(B=16, 10 calls), (B=16, 5 calls), (B=4, 10 calls) into launches per call.

usage: python tools/zk_batch_bench.py [--sizes 12 14 16] [--seconds 1.0] [--out FILE]"""
import argparse
import csv
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

BATCHES = (1, 4, 16, 64)
PLAIN_BATCHES = (4, 16, 64)


def trace_report(files):
    def calls(path):
        with open(path) as f:
            return {r["Name"]: int(r["Calls"]) for r in csv.DictReader(f)}
    b16x10, b16x5, b4x10 = (calls(p) for p in files)
    names = sorted(set(b16x10) | set(b16x5) | set(b4x10))
    print("totals: B16x10 %d  B16x5 %d  B4x10 %d" % tuple(sum(d.values()) for d in (b16x10, b16x5, b4x10)))
    print("per call:  B=16    B=4   kernel")
    tot16 = tot4 = 0.0
    for nm in names:
        l16 = (b16x10.get(nm, 0) - b16x5.get(nm, 0)) / 5
        l4 = ((b4x10.get(nm, 0) - b16x5.get(nm, 0)) / 5 + l16) / 2
        tot16, tot4 = tot16 + l16, tot4 + l4
        if l16 or l4:
            print("        %6.1f %6.1f   %s" % (l16, l4, nm[:100]))
    print("all:    %6.1f %6.1f" % (tot16, tot4))


class Size:
    def __init__(self, pa, ctx, srs, log_n, bmax):
        from plonk_prototype_amd import _lib
        self.pa, self.lib, self.ctx = pa, _lib, ctx
        self.n, self.log_n, self.bmax = 1 << log_n, log_n, bmax
        n = self.n
        made = [pa.synthetic.boolean_circuit(n, s) for s in range(1, bmax + 1)]
        self.ck = pa.CommitKey(srs[:n + _lib.PLONK_ZK_EXTRA_BASES], ctx, precompute=True)
        self.key = pa.preprocess(made[0][0], ctx, self.ck)
        self.key.enable_zk()
        self.wits = pa.DeviceVector.from_host(ctx, np.concatenate([m[1].reshape(4 * n, 4) for m in made]))
        self.ws = self.key.batch(bmax)
        self.plain_bytes = self.ws.device_bytes()
        self.added_bytes = self.ws.enable_zk()
        self.raw = (_lib.PlonkProof * bmax)()
        self.cnt = (C.c_size_t * bmax)()

    def blinders(self, count):
        return self.pa.prover.random_blinders(count)

    def prove_zk_one(self, b, bl):
        c, raw = self.ctx, self.lib.PlonkProof()
        c._check(c._lib.pm_plonk_prove_zk(c._h, self.key._h, self.ck._bases._h, C.c_void_p(self.wits.ptr + 32 * 4 * self.n * b),
                                          None, None, 0, 0, bl.ctypes.data_as(self.lib.u64p), C.byref(raw)))
        return raw

    def prove_batch(self, B):
        c = self.ctx
        c._check(c._lib.pm_plonk_prove_batch(c._h, self.key._h, self.ws._h, self.ck._bases._h, B, self.wits._p, None, None,
                                             self.cnt, 0, self.raw))

    def prove_batch_zk(self, B, bl):
        c = self.ctx
        c._check(c._lib.pm_plonk_prove_batch_zk(c._h, self.key._h, self.ws._h, self.ck._bases._h, B, self.wits._p, None, None,
                                                self.cnt, 0, bl.ctypes.data_as(self.lib.u64p), self.raw))

    def check(self):
        """every member of a zero-knowledge batch equals its single zero-knowledge proof (first call of every batch size)"""
        for B in [b for b in BATCHES if b <= self.bmax]:
            bl = self.blinders(B)
            self.prove_batch_zk(B, bl)
            for b in range(B):
                assert bytes(self.raw[b]) == bytes(self.prove_zk_one(b, bl[b])), f"2^{self.log_n} B={B}: proof {b} differs"

    def free(self):
        self.ws.free()
        self.key.free()
        self.wits.free()


def arms(sz: Size):
    """name -> (prepare() -> argument drawn outside the timer, function of it, proofs per call)"""
    out = {}
    k_seq = min(16, sz.bmax)

    def seq(bl):
        for b in range(k_seq):
            sz.prove_zk_one(b, bl[b])
    out["sequential_zk"] = (lambda: sz.blinders(k_seq), seq, k_seq)
    for B in PLAIN_BATCHES:
        if B <= sz.bmax:
            out[f"plain_batch_{B}"] = (lambda: None, lambda _, B=B: sz.prove_batch(B), B)
    for B in BATCHES:
        if B <= sz.bmax:
            out[f"zk_batch_{B}"] = (lambda B=B: sz.blinders(B), lambda bl, B=B: sz.prove_batch_zk(B, bl), B)
    return out


def measure(sz: Size, seconds: float):
    a = arms(sz)
    for prep, fn, _ in a.values():          # warm-up: at least two calls and a quarter of a second per arm
        t0 = time.perf_counter()
        while True:
            fn(prep())
            fn(prep())
            if time.perf_counter() - t0 > 0.25:
                break
    sz.ctx.sync()
    tot = {k: 0.0 for k in a}
    cnt = {k: 0 for k in a}
    rounds = 0
    while min(tot.values()) < seconds:
        rounds += 1
        for name, (prep, fn, k) in a.items():          # alternate the arms
            arg = prep()                               # fresh blinders for every call
            t0 = time.perf_counter()
            fn(arg)
            tot[name] += time.perf_counter() - t0
            cnt[name] += k
    res = {name: {"proofs": cnt[name], "seconds": round(tot[name], 4), "ms_per_proof": round(1e3 * tot[name] / cnt[name], 4),
                  "proofs_per_s": round(cnt[name] / tot[name], 1)} for name in a}
    seq = res["sequential_zk"]["ms_per_proof"]
    for B in BATCHES:
        z = res.get(f"zk_batch_{B}")
        if z:
            z["speedup_over_sequential_zk"] = round(seq / z["ms_per_proof"], 3)
            p = res.get(f"plain_batch_{B}")
            if p:
                z["over_plain_batch"] = round(z["ms_per_proof"] / p["ms_per_proof"], 4)
    res["rounds"] = rounds
    res["workspace_n32_per_proof"] = {"plain": round(sz.plain_bytes / (sz.bmax * sz.n * 32), 2),
                                      "zk_added": round(sz.added_bytes / (sz.bmax * sz.n * 32), 2), "max_batch": sz.bmax}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[12, 14, 16])
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                   "zk_batch_bench.json"))
    ap.add_argument("--trace-only", type=int, nargs=3, metavar=("LOG_N", "B", "CALLS"), default=None)
    ap.add_argument("--trace-report", nargs=3, metavar=("B16x10", "B16x5", "B4x10"), default=None)
    args = ap.parse_args()
    if args.trace_report:
        trace_report(args.trace_report)
        return
    import torch  # noqa: F401  (the library binds to torch's HIP runtime, as in bench.py)
    import plonk_prototype_amd as pa
    from oracle.cpu_oracle import CpuOracle, ints_to_limbs
    orc = CpuOracle()
    sizes = [args.trace_only[0]] if args.trace_only else args.sizes
    srs = orc.g1_bases_arith(ints_to_limbs([0x1234567], 4)[0], ints_to_limbs([0x9E3779B9], 4)[0], (1 << max(sizes)) + 10, threads=16)
    ctx = pa.Context(0)
    if args.trace_only:
        lg, B, calls = args.trace_only
        sz = Size(pa, ctx, srs, lg, 16)        # the same setup whatever B is: the runs differ in their calls only
        for _ in range(calls):
            sz.prove_batch_zk(B, sz.blinders(B))
        sz.free()
        return
    report = {"device": torch.cuda.get_device_name(0), "witnesses": "boolean_circuit seeds 1..B (one circuit)",
              "arms": "sequential pm_plonk_prove_zk | pm_plonk_prove_batch B | pm_plonk_prove_batch_zk B; fresh blinders per call",
              "sizes": {}}
    for lg in sizes:
        sz = Size(pa, ctx, srs, lg, 64)
        sz.check()
        res = measure(sz, args.seconds)
        report["sizes"][f"2^{lg}"] = res
        print(f"2^{lg}: " + "  ".join(f"{k} {v['ms_per_proof']:.3f} ms ({v['proofs_per_s']:.0f}/s)"
                                      for k, v in res.items() if isinstance(v, dict) and "ms_per_proof" in v), flush=True)
        sz.free()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
