"""GPU measurement (not a test): many proofs of one circuit -- sequential pm_plonk_prove, four contexts from four host threads
(tools/multi_ctx_prover.py's arrangement: one resident SRS, a key and a workspace per context), and pm_plonk_prove_batch at
B in {1, 4, 16, 64} -- in one process, at 2^12, 2^14 and 2^16 gates (2^20 at B <= 4).  Witnesses: distinct
boolean_circuit seeds of one circuit, resident on the device.  Every arm is warmed up, then the arms alternate in rounds
until each has at least --seconds of timed proofs.  Writes profiles/prove_batch_bench.json (or --out).

usage: python tools/prove_batch_bench.py [--sizes 12 14 16 20] [--seconds 1.0] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import threading
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (the library binds to torch's HIP runtime, as in bench.py)

import plonk_prototype_amd as pa  # noqa: E402
from plonk_prototype_amd import _lib  # noqa: E402
from oracle.cpu_oracle import CpuOracle, ints_to_limbs  # noqa: E402

BATCHES = (1, 4, 16, 64)


class Size:
    def __init__(self, ctxs, srs, log_n, bmax):
        self.n, self.log_n, self.bmax = 1 << log_n, log_n, bmax
        n = self.n
        made = [pa.synthetic.boolean_circuit(n, s) for s in range(1, bmax + 1)]
        self.ctxs = ctxs
        self.cks, self.keys, self.wits = [], [], []
        ck0 = pa.CommitKey(srs[:n], ctxs[0], precompute=True)
        for i, c in enumerate(ctxs):
            if i == 0:
                ck = ck0
            else:
                ck = pa.CommitKey.__new__(pa.CommitKey)
                ck.__dict__.update(ck0.__dict__)                 # the same resident SRS table
            self.cks.append(ck)
            self.keys.append(pa.preprocess(made[0][0], c, ck))
            self.wits.append(pa.DeviceVector.from_host(c, np.concatenate([m[1].reshape(4 * n, 4) for m in made])))
        self.ws = self.keys[0].batch(bmax)
        self.raw = (_lib.PlonkProof * bmax)()
        self.cnt = (C.c_size_t * bmax)()

    def prove_one(self, i, b):
        """context i, witness b: one pm_plonk_prove"""
        c, w = self.ctxs[i], self.wits[i]
        raw = _lib.PlonkProof()
        c._check(c._lib.pm_plonk_prove(c._h, self.keys[i]._h, self.cks[i]._bases._h, C.c_void_p(w.ptr + 32 * 4 * self.n * b),
                                       None, None, 0, 0, C.byref(raw)))
        return raw

    def prove_batch(self, B):
        c = self.ctxs[0]
        c._check(c._lib.pm_plonk_prove_batch(c._h, self.keys[0]._h, self.ws._h, self.cks[0]._bases._h, B, self.wits[0]._p,
                                             None, None, self.cnt, 0, self.raw))

    def check(self):
        """the batch equals the single proofs (first call of every batch size, every proof)"""
        for B in [b for b in BATCHES if b <= self.bmax]:
            self.prove_batch(B)
            for b in range(B):
                one = self.prove_one(0, b)
                assert bytes(self.raw[b]) == bytes(one), f"2^{self.log_n} B={B}: proof {b} differs"

    def free(self):
        self.ws.free()
        for k in self.keys:
            k.free()
        for w in self.wits:
            w.free()


def arms(sz: Size):
    """name -> (function running some proofs, proofs per call)"""
    out = {}
    k_seq = max(1, min(16, sz.bmax))

    def seq():
        for b in range(k_seq):
            sz.prove_one(0, b % sz.bmax)
    out["sequential"] = (seq, k_seq)
    if len(sz.ctxs) >= 4 and sz.n <= (1 << 16):
        per = 4

        def four():
            def worker(i):
                for r in range(per):
                    sz.prove_one(i, (i * per + r) % sz.bmax)
            th = [threading.Thread(target=worker, args=(i,)) for i in range(4)]
            for t in th:
                t.start()
            for t in th:
                t.join()
        out["four_contexts"] = (four, 4 * per)
    for B in BATCHES:
        if B <= sz.bmax:
            out[f"batch_{B}"] = (lambda B=B: sz.prove_batch(B), B)
    return out


def measure(sz: Size, seconds: float):
    a = arms(sz)
    for fn, _ in a.values():          # warm-up: two calls of every arm, at least half a second in all
        t0 = time.perf_counter()
        while True:
            fn()
            fn()
            if time.perf_counter() - t0 > 0.25:
                break
    for c in sz.ctxs:
        c.sync()
    tot = {k: 0.0 for k in a}
    cnt = {k: 0 for k in a}
    rounds = 0
    while min(tot.values()) < seconds:
        rounds += 1
        for name, (fn, k) in a.items():          # alternate the arms
            t0 = time.perf_counter()
            fn()
            tot[name] += time.perf_counter() - t0
            cnt[name] += k
    res = {name: {"proofs": cnt[name], "seconds": round(tot[name], 4), "ms_per_proof": round(1e3 * tot[name] / cnt[name], 4),
                  "proofs_per_s": round(cnt[name] / tot[name], 1)} for name in a}
    res["rounds"] = rounds
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[12, 14, 16, 20])
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                   "prove_batch_bench.json"))
    args = ap.parse_args()
    orc = CpuOracle()
    nmax = 1 << max(args.sizes)
    srs = orc.g1_bases_arith(ints_to_limbs([0x1234567], 4)[0], ints_to_limbs([0x9E3779B9], 4)[0], nmax, threads=16)
    ctxs = [pa.Context(0) for _ in range(4)]
    report = {"device": torch.cuda.get_device_name(0), "witnesses": "boolean_circuit seeds 1..B (one circuit)",
              "arms": "sequential pm_plonk_prove | 4 contexts x 4 threads | pm_plonk_prove_batch B", "sizes": {}}
    for lg in args.sizes:
        bmax = 4 if lg >= 20 else 64
        sz = Size(ctxs if lg <= 16 else ctxs[:1], srs, lg, bmax)
        sz.check()
        res = measure(sz, args.seconds)
        report["sizes"][f"2^{lg}"] = res
        print(f"2^{lg}: " + "  ".join(f"{k} {v['ms_per_proof']:.3f} ms ({v['proofs_per_s']:.0f}/s)"
                                      for k, v in res.items() if k != "rounds"), flush=True)
        sz.free()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
