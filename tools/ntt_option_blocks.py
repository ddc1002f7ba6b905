#!/usr/bin/env python3
"""Forward + inverse 2^20 steps in blocks that alternate the option ntt_fixed_shape, for a kernel trace or a counters run of one
process that holds the generic and the fixed-shape kernels side by side (profiles/twiddle_prefetch_kernel_trace.txt, _pmc.txt).

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/ntt_option_blocks.py run 200 121212
    python tools/ntt_option_blocks.py report DIR 200 6

run STEPS ORDER: a warm-up of 4 x STEPS steps under option 1 and again under 2, then one block of STEPS steps per digit of ORDER with the
option at that digit; prints the device-event time per step of every block.  PM_LIB_PATH picks the library.
report DIR STEPS NBLOCKS: cuts the trace into the blocks by counting the dispatches of the pass kernels (four a step: forward first and
last pass, inverse first and last pass) and prints, per block, the mean time per launch of the first and of the last pass and which
kernel ran."""
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 20


def run(steps, order):
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    import plonk_prototype_amd as pa
    from oracle.cpu_oracle import INVERSE, CpuOracle

    n = 1 << K
    ctx = pa.Context(0)
    dev = torch.device("cuda:0")
    a = torch.from_numpy(CpuOracle().fr_sample(0x504C4F4E4B, n).view(np.int64)).to(dev)
    b, c = torch.empty_like(a), torch.empty_like(a)
    stream = torch.cuda.ExternalStream(ctx.stream_handle(), device=dev)

    def step():
        ctx.fr_ntt_dev(a.data_ptr(), n, b.data_ptr(), K, 0, stream=0)
        ctx.fr_ntt_dev(b.data_ptr(), n, c.data_ptr(), K, INVERSE, stream=0)

    for opt in (1, 2):   # tables, code load, clocks
        ctx.set_option("ntt_fixed_shape", opt)
        for _ in range(4 * steps):
            step()
        ctx.sync()
    blocks = []
    for opt in order:
        ctx.set_option("ntt_fixed_shape", opt)
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record(stream)
        for _ in range(steps):
            step()
        ev[1].record(stream)
        ctx.sync()
        torch.cuda.synchronize()
        assert torch.equal(c, a), "iNTT(NTT(a)) != a"
        blocks.append((opt, round(ev[0].elapsed_time(ev[1]) / steps * 1e3, 3)))
    print(json.dumps({"lib": os.environ.get("PM_LIB_PATH", "default"), "steps": steps, "us_per_step": blocks}))
    ctx.close()


def report(directory, steps, nblocks):
    path = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = [r for r in csv.DictReader(open(path)) if "ntt_pass4" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    print("# dispatches of pass kernels: %d, expected %d" % (len(rows), (8 + nblocks) * steps * 4))
    rows = rows[len(rows) - nblocks * steps * 4:]
    for i in range(nblocks):
        blk = rows[i * steps * 4:(i + 1) * steps * 4]
        out = []
        for pos, name in ((0, "first"), (1, "last")):
            sel = blk[pos::2]
            us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in sel]
            kinds = sorted({"fixed" if "fixed" in r["Kernel_Name"] else "generic" for r in sel})
            out.append("%s %s %.2f" % (name, "/".join(kinds), sum(us) / len(us)))
        span = (int(blk[-1]["End_Timestamp"]) - int(blk[0]["Start_Timestamp"])) / 1e3 / steps
        print("block %d: %s ; %s ; span per step %.2f us" % (i, out[0], out[1], span))


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(int(sys.argv[2]), [int(ch) for ch in sys.argv[3]])
    else:
        report(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
