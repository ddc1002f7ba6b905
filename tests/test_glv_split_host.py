"""The GLV split k = k1 + k2 z^2 of csrc/ec_mul.hip.h, compiled for the host (pm_test_host_glv_split), against Python's
divmod(k, z^2): the constants (z^2, the reciprocal of the division) and the correction step, on a machine without a GPU.
The device runs the same routine; tests/test_gpu_scalar_mul.py repeats the list there."""
import ctypes as C
import random

import numpy as np

from oracle import bigint_oracle as B
from oracle.cpu_oracle import ints_to_limbs

Z = -0xd201000000010000
Z2 = 0xac45a4010001a4020000000100000000
R = B.R_MOD


def split_cases():
    """the fixed list, the limb carries of the reciprocal product, and 2000 seeded random scalars, all below r"""
    ks = [0, 1, 2, Z2 - 1, Z2, Z2 + 1, 2 * Z2 - 1, 2 * Z2, R - 2, R - 1, (Z2 - 1) * Z2 - 1, 2**128 - 1, 2**128, 2**254]
    for j in (2**32 - 1, 2**32, 2**64 - 1, 2**64, 2**96, 2**127):
        ks += [j * Z2 - 1, j * Z2, j * Z2 + 1]
    rng = random.Random(0x474C56)
    ks += [rng.randrange(R) for _ in range(2000)]
    assert all(0 <= k < R for k in ks)
    return ks


def test_the_arithmetic_behind_the_split():
    assert Z2 == Z * Z and R == Z**4 - Z2 + 1 and R - 1 == Z2 * (Z2 - 1) and Z2.bit_length() == 128
    mu = (-Z2) % R
    assert mu != 1 and pow(mu, 3, R) == 1                      # a primitive cube root of unity mod r
    beta = pow(2, (B.P_MOD - 1) // 3, B.P_MOD)
    x, y = B.G1_GEN
    assert B.g1_mul(Z2, B.G1_GEN) == (beta * x % B.P_MOD, B.P_MOD - y)   # Q = (beta x, -y) = [z^2] P on the subgroup
    assert divmod(R - 1, Z2) == (Z2 - 1, 0)


def test_host_split_matches_divmod():
    import plonk_prototype_amd as pa
    lib = pa.load()
    u64p = C.POINTER(C.c_uint64)
    ks = split_cases()
    limbs = ints_to_limbs(ks, 4)
    out = np.zeros(4, np.uint64)
    for k, row in zip(ks, limbs):
        row = np.ascontiguousarray(row)
        assert lib.pm_test_host_glv_split(row.ctypes.data_as(u64p), out.ctypes.data_as(u64p)) == 0
        k1 = int(out[0]) | int(out[1]) << 64
        k2 = int(out[2]) | int(out[3]) << 64
        assert (k2, k1) == divmod(k, Z2), hex(k)
        assert k1 < Z2 and k2 < Z2
    assert lib.pm_test_host_glv_split(None, out.ctypes.data_as(u64p)) == -1


def test_new_names_are_bound():
    from plonk_prototype_amd import _lib, host
    for name in ("pm_g1_scalar_mul_dev", "pm_g1_bases_lagrange_ex", "pm_g1_bases_to_dev", "pm_test_glv_split",
                 "pm_test_host_glv_split"):
        assert name in _lib.SIGNATURES
    assert _lib.G1_POINTS_IN_SUBGROUP == 1 and _lib.GLV_Z2 == Z2
    assert hasattr(host.Context, "g1_scalar_mul_dev") and hasattr(host, "g1_scalar_mul") and hasattr(host.CommitKey, "update")
