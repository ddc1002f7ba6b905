"""`bench.py --full`: beyond the headline step it runs the roofline's profiled loop and the legs, with their in-bench checks
(a plain run, which leaves these fields null, is tested in test_bench_dump.py).  Small sizes: this checks what runs, not
how fast."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT


@pytest.mark.gpu
def test_full_run_carries_the_legs(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2", "--log-n", "12",
           "--full", "--msm-log-n", "12", "--msm-steps", "1", "--msm-large-log-n", "0", "--prover-log-n", "12",
           "--prover-large-log-n", "0", "--no-cpu-baseline"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout
    line = json.loads(lines[0])
    assert line["value"] > 0 and line["roofline"]["kernel"].startswith("ntt_pass")
    assert line["ntt_extra"]["fwd_inv_2^24"]["fourstep_world1"]["equals_single_gpu_plan"] is True
    assert line["msm"]["bit_exact_vs_oracle"] is True and line["next_rows"]["n"] == 1 << 22
    prover = line["prover"]
    assert prover["verifier_identity_holds"] and prover["kzg_opening_equation_holds"]
    assert prover["distributed"]["equals_the_replicated_prover_byte_for_byte"] is True
    assert line["cpu_baseline"] is None and line["msm_large"] is None
