"""examples/zk_batch_demo.cpp: zero-knowledge batches from C++ (BatchWorkspace::enable_zk / ProverKey::prove_batch_zk of
include/plonk_mi355x.hpp) -- no Python, no torch in the process.  CPU: it compiles, links and fails loudly without a device.
GPU: zero blinders reproduce prove_batch, every member of a blinded batch equals prove_zk of the same witness and blinders,
and two blinder sets give different proofs."""
import os
import subprocess

import pytest

from conftest import ROOT

LIBDIR = os.path.join(ROOT, "plonk-prototype_amd", "lib")


def _build(tmp_path):
    exe = str(tmp_path / "zk_batch_demo")
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Werror", os.path.join(ROOT, "examples", "zk_batch_demo.cpp"),
           "-I", os.path.join(ROOT, "include"), "-L", LIBDIR, "-lplonk_mi355x", f"-Wl,-rpath,{LIBDIR}", "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def test_zk_batch_demo_builds_and_fails_loudly_without_a_gpu(tmp_path):
    import torch
    exe = _build(tmp_path)
    if torch.cuda.is_available():
        return                    # the gpu-marked test runs the demo
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "Error -5" in r.stderr and "no CPU fallback" in r.stderr


@pytest.mark.gpu
def test_zk_batch_demo_runs_on_the_gpu(tmp_path):
    r = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "zk_batch_demo OK" in r.stdout
