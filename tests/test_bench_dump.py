"""`bench.py --dump-outputs DIR` and `--steps`: the dump is exact (32-bit halves of the Montgomery limbs in float64), the
row sample is fixed, the whole dump stays under 64 MB, a non-positive step count is refused, and on the GPU the files hold
the forward transform of the bench's seeded input and its inverse (= the input), as the CPU oracle computes them, from a
plain run that measures nothing but the headline step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _from_words(w):
    w = w.astype(np.uint64).reshape(w.shape[0], -1, 2)
    return w[..., 0] | (w[..., 1] << np.uint64(32))


def test_dump_is_exact_float64(tmp_path):
    a = np.random.default_rng(1).integers(0, 2**64 - 1, size=(100, 4), dtype=np.uint64, endpoint=True)
    a[0] = 2**64 - 1
    bench.write_dump(str(tmp_path / "d"), {"x": a})
    got = np.load(tmp_path / "d" / "x.npy")
    assert got.dtype == np.float64 and got.shape == (100, 8)
    assert np.all(got < 2**32) and np.array_equal(_from_words(got), a)


def test_dump_rows_fixed_and_bounded():
    assert np.array_equal(bench.dump_rows(1 << 12), np.arange(1 << 12))
    r = bench.dump_rows(1 << 20)
    assert len(r) == bench.DUMP_MAX_ROWS and len(np.unique(r)) == len(r) and np.all(np.diff(r) > 0)
    assert r[-1] < 1 << 20 and np.array_equal(r, bench.dump_rows(1 << 20))
    for log_n in (20, 24, 28):      # two outputs of the headline step at any size fit in 64 MB
        assert 2 * len(bench.dump_rows(1 << log_n)) * 8 * 8 <= 64 << 20


@pytest.mark.parametrize("steps", ["0", "-3"])
def test_steps_must_be_positive(steps):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", steps], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 2 and "--steps" in p.stderr and not p.stdout.strip()


@pytest.mark.gpu
def test_dump_outputs_on_the_gpu(tmp_path, oracle):
    k, steps = 12, 7
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "2",
           "--log-n", str(k), "--dump-outputs", str(tmp_path / "out")]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-4000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert line["steps"] == steps and line["ms_per_step"] > 0
    # a plain run (no --full) measures the headline step alone
    assert all(line[f] is None for f in ("roofline", "cpu_baseline", "ntt_extra", "ntt_fourstep", "msm", "msm_large",
                                         "next_rows", "prover")), line
    assert sorted(os.listdir(tmp_path / "out")) == ["ntt_forward.npy", "ntt_inverse.npy"]
    a = oracle.fr_sample(0x504C4F4E4B, 1 << k)                    # the bench's input on rank 0
    assert np.array_equal(_from_words(np.load(tmp_path / "out" / "ntt_forward.npy")), oracle.fr_ntt(a, k, 0))
    assert np.array_equal(_from_words(np.load(tmp_path / "out" / "ntt_inverse.npy")), a)
