"""Step twiddles kept in flight in the fixed-shape last pass of the plain 2^20 transform (csrc/ntt_kernels4.hip.h:
PM_NTT_FIXED_TW_PREFETCH, step4_tw_prefetch).  The kernel issues the loads of a step twiddle one product earlier than the
generic kernel does, and a step's first twiddle from the step before it; no product, table or bound changes.  So with
ntt_fixed_shape = 2 (both fixed kernels) a call must give the bytes of ntt_fixed_shape = 0 (generic kernels, the loads
where they always were): a prefetched entry of the wrong step block or digit would change almost every output.

    forward and inverse of a uniform sample           2 against 0, the forward one against the CPU oracle too
    a batch of three, strides n + 3, on the device    the uniform base moves, the lanes' offsets do not; gaps untouched
    every element r - 1                               the largest canonical words through every product
    the kernels a transform took under option 2       fixed, fixed; in a fresh context, what PM_NTT_FIXED_SHAPE_DEFAULT says
    registers of both fixed kernels (no GPU)          from the gfx950 listing: no scratch, at most 128 VGPRs

The variants exist at 2^20 only, which is also the smallest size that reaches this code."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle import bigint_oracle as B
from oracle.cpu_oracle import INVERSE, ints_to_limbs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 20
N = 1 << K
GENERIC, FIXED = 1, 2
SEED = 0x54575046


def _variants(ctx):
    out = (C.c_uint32 * 4)()
    ctx._check(ctx._lib.pm_test_ntt_last_variants(ctx._h, out))
    return list(out)


def _default_option():
    """PM_NTT_FIXED_SHAPE_DEFAULT of csrc/context.h: what a context starts with"""
    src = open(os.path.join(ROOT, "plonk-prototype_amd", "csrc", "context.h")).read()
    m = re.search(r"#define PM_NTT_FIXED_SHAPE_DEFAULT (\d)\n", src)
    assert m, "PM_NTT_FIXED_SHAPE_DEFAULT"
    return int(m.group(1))


def _under(ctx, option, call):
    """call() with ntt_fixed_shape = option, which goes back to the default; the result and the kernels the last transform took"""
    ctx.set_option("ntt_fixed_shape", option)
    try:
        return call(), _variants(ctx)
    finally:
        ctx.set_option("ntt_fixed_shape", _default_option())


def _fixed_against_generic(ctx, call):
    got2, v2 = _under(ctx, 2, call)
    got0, v0 = _under(ctx, 0, call)
    assert v2 == [FIXED, FIXED, 0, 0], v2
    assert v0 == [GENERIC, GENERIC, 0, 0], v0
    assert np.array_equal(got2, got0)
    return got2


@pytest.fixture(scope="module")
def sample(oracle):
    a = oracle.fr_sample(SEED, N)
    a.setflags(write=False)
    return a


@pytest.mark.gpu
def test_forward_is_the_generic_kernels_and_the_oracles(ctx, oracle, sample):
    got = _fixed_against_generic(ctx, lambda: ctx.fr_ntt(sample, K, 0))
    assert np.array_equal(got, oracle.fr_ntt(sample, K, 0))


@pytest.mark.gpu
def test_inverse_is_the_generic_kernels(ctx, sample):
    _fixed_against_generic(ctx, lambda: ctx.fr_ntt(sample, K, INVERSE))


@pytest.mark.gpu
def test_batch_of_three_with_strides(ctx, sample):
    """in_stride = out_stride = n + 3 elements: the vectors start at 32 (n + 3) b bytes, off every power of two"""
    import torch

    stride = N + 3
    host = np.full((3 * stride, 4), 0x5A5A5A5A5A5A5A5A, np.uint64)
    for b in range(3):
        host[b * stride:b * stride + N] = np.roll(sample, 7 * b, axis=0)   # three different vectors from one sample

    def call():
        src = torch.from_numpy(host.view(np.int64).copy()).cuda()
        dst = torch.from_numpy(host.view(np.int64).copy()).cuda()
        torch.cuda.synchronize()
        ctx.fr_ntt_dev(src.data_ptr(), N, dst.data_ptr(), K, 0, batch=3, in_stride=stride, out_stride=stride)
        ctx.sync()
        return dst.cpu().numpy().view(np.uint64)

    got = _fixed_against_generic(ctx, call)
    for b in range(3):
        assert np.array_equal(got[b * stride + N:(b + 1) * stride], host[b * stride + N:(b + 1) * stride]), b
    assert not np.array_equal(got[:N], got[stride:stride + N])


@pytest.mark.gpu
def test_every_element_r_minus_1(ctx):
    a = np.empty((N, 4), np.uint64)
    a[:] = ints_to_limbs([B.R_MOD - 1], 4)[0]
    _fixed_against_generic(ctx, lambda: ctx.fr_ntt(a, K, 0))


@pytest.mark.gpu
def test_a_fresh_context_takes_the_default_variants(sample):
    """no option set: the first pass's fixed kernel, and the last pass's where the default is 2"""
    import plonk_prototype_amd as pa

    default = _default_option()
    assert default in (1, 2)
    fresh = pa.Context(0)
    try:
        fresh.fr_ntt(sample, K, 0)
        assert _variants(fresh) == [FIXED, FIXED if default == 2 else GENERIC, 0, 0]
    finally:
        fresh.close()


def test_fixed_kernels_hold_128_vgprs_without_scratch(tmp_path):
    """the listing of csrc/ntt4_fixed.hip with the flags of csrc/Makefile, read by tools/isa_kernel_stats.py"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    assert os.path.exists(hipcc), "the build needs hipcc"
    listing = str(tmp_path / "ntt4_fixed.s")
    src = os.path.join(ROOT, "plonk-prototype_amd", "csrc", "ntt4_fixed.hip")
    subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-mllvm", "-pragma-unroll-threshold=1000000",
                    "-Wno-pass-failed", "--cuda-device-only", "-S", "-o", listing, src],
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_kernel_stats.py"), listing, "ntt_pass4_fixed_kernel<"],
                         check=True, capture_output=True, text=True).stdout
    rows = [line.split("; ") for line in out.splitlines() if line and not line.startswith("#")]
    assert sorted(r[0] for r in rows) == ["void ntt_pass4_fixed_kernel<10, 1, false, true, false, 20>",
                                          "void ntt_pass4_fixed_kernel<10, 1, true, false, true, 20>"], out
    for name, _mads, _valu, _sld, vgprs, _sgprs, scratch in rows:
        assert int(scratch) == 0, (name, scratch)
        assert int(vgprs) <= 128, (name, vgprs)
