"""Native JubJub without a device: the new exports are declared, bound, exported and documented; the two
host forms agree with the big-integer model of tests/jubjub_model.py on the edge scalars and points, in both scalar forms; and
they refuse what the header says they refuse."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jubjub_model as J  # noqa: E402

EXPORTS = ("pm_jubjub_base_create", "pm_jubjub_base_from_key", "pm_jubjub_base_point", "pm_jubjub_base_free",
           "pm_jubjub_fixed_mul_dev", "pm_jubjub_commit_dev", "pm_jubjub_mul_dev", "pm_jubjub_check_dev", "pm_jubjub_mul_host",
           "pm_jubjub_add_host")
PY_NAMES = ("JubJubBase", "JUBJUB_GENERATOR", "jubjub_commit", "jubjub_commit_dev", "jubjub_mul", "jubjub_mul_dev", "jubjub_check",
            "jubjub_mul_host", "jubjub_add_host")


def _u64p(a):
    from plonk_prototype_amd._lib import u64p
    return a.ctypes.data_as(u64p)


def _canonical(s: int) -> np.ndarray:
    return np.frombuffer(s.to_bytes(32, "little"), dtype=np.uint64).copy()


def test_exports_are_declared_bound_exported_and_documented():
    import plonk_prototype_amd as pa
    from plonk_prototype_amd import _lib
    header = open(os.path.join(ROOT, "include", "plonk_mi355x.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = C.CDLL(pa.LIB_PATH)
    for name in EXPORTS:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in the header"
        assert name in _lib.SIGNATURES, f"{name} has no binding"
        assert hasattr(lib, name), f"{name} is not exported by the library"
        assert "pub fn %s(" % name in doc, f"{name} is missing from INTEGRATION.md's extern block"
    for name in PY_NAMES:
        assert hasattr(pa, name), f"plonk_prototype_amd.{name} is not exported"
    assert "hardened against side channels" in header.replace("\n * ", " ")


def test_generator_and_the_model_itself():
    import plonk_prototype_amd as pa
    from plonk_prototype_amd.jubjub import JUBJUB_ORDER
    g = pa.JUBJUB_GENERATOR
    assert g == J.GENERATOR and JUBJUB_ORDER == J.Q
    assert g == pa.synthetic.jubjub_point(0x12) or (J.R - g[0], g[1]) == pa.synthetic.jubjub_point(0x12)
    assert J.on_curve(g) and J.mul(g, J.Q) == J.IDENTITY and J.mul(g, 8) != J.IDENTITY
    odd = J.M.curve_point(0x14)                       # outside the subgroup: the integer-multiplier rule is visible
    assert J.mul(odd, J.Q) != J.IDENTITY and J.mul(odd, 8 * J.Q) == J.IDENTITY
    assert J.mul((0, J.R - 1), 2) == J.IDENTITY and J.mul((J.SQRT_M1, 0), 4) == J.IDENTITY and J.mul((J.SQRT_M1, 0), 2) == (0, J.R - 1)
    # the projective ladder is the affine law
    for p in J.edge_points():
        for s in (0, 1, 2, 3, 17, J.Q + 1, J.edge_scalars()[-1]):
            assert J.mul(p, s) == J.mul_affine(p, s)


@pytest.fixture(scope="module")
def products():
    """the model's s * P for the edge scalars x the edge points, computed once"""
    pts, scs = J.edge_points(), J.edge_scalars()
    return pts, scs, [[J.mul(p, s) for s in scs] for p in pts]


def test_mul_host_agrees_with_the_model_in_both_forms(products):
    import plonk_prototype_amd as pa
    pts, scs, want = products
    for p, row in zip(pts, want):
        for s, w in zip(scs, row):
            w_l = J.to_limbs([w])[0]
            assert np.array_equal(pa.jubjub_mul_host(p, s), w_l), (p, hex(s), "canonical")
            assert np.array_equal(pa.jubjub_mul_host(J.to_limbs([p])[0], J.M.to_limbs([s])[0]), w_l), (p, hex(s), "montgomery")


def test_add_host_agrees_with_the_model():
    import plonk_prototype_amd as pa
    pts = J.edge_points()
    for p in pts:
        for q in pts:
            assert np.array_equal(pa.jubjub_add_host(p, q), J.to_limbs([J.add(p, q)])[0]), (p, q)


def test_host_refusals():
    from plonk_prototype_amd import _lib
    lib = _lib.load()
    BAD = _lib.PM_ERR_BAD_ARG
    g = J.to_limbs([J.GENERATOR])[0]
    out = np.zeros((2, 4), np.uint64)
    one = _canonical(1)
    assert lib.pm_jubjub_mul_host(_u64p(g), _u64p(one), _lib.SCALAR_CANONICAL, _u64p(out)) == _lib.PM_OK
    off = J.to_limbs([(J.GENERATOR[0], J.GENERATOR[1] + 1)])[0]
    assert not J.on_curve((J.GENERATOR[0], J.GENERATOR[1] + 1))
    big = g.copy()
    big[1] = _canonical(J.R)                           # y = r: a coordinate >= r
    for form in (_lib.SCALAR_CANONICAL, _lib.SCALAR_MONTGOMERY):
        assert lib.pm_jubjub_mul_host(_u64p(off), _u64p(one), form, _u64p(out)) == BAD            # off the curve
        assert lib.pm_jubjub_mul_host(_u64p(big), _u64p(one), form, _u64p(out)) == BAD            # coordinate >= r
        assert lib.pm_jubjub_mul_host(_u64p(g), _u64p(_canonical(J.R)), form, _u64p(out)) == BAD  # scalar >= r
        assert lib.pm_jubjub_mul_host(_u64p(g), _u64p(_canonical((1 << 256) - 1)), form, _u64p(out)) == BAD
        assert lib.pm_jubjub_mul_host(None, _u64p(one), form, _u64p(out)) == BAD
        assert lib.pm_jubjub_mul_host(_u64p(g), None, form, _u64p(out)) == BAD
        assert lib.pm_jubjub_mul_host(_u64p(g), _u64p(one), form, None) == BAD
    assert lib.pm_jubjub_mul_host(_u64p(g), _u64p(one), 2, _u64p(out)) == BAD                     # unknown scalar form
    assert lib.pm_jubjub_mul_host(_u64p(g), _u64p(one), 0xFFFFFFFF, _u64p(out)) == BAD
    # (0, r) reads as the identity modulo r but is not canonical
    ident_r = np.stack([_canonical(0), _canonical(J.R)])
    assert lib.pm_jubjub_add_host(_u64p(g), _u64p(ident_r), _u64p(out)) == BAD
    assert lib.pm_jubjub_add_host(_u64p(off), _u64p(g), _u64p(out)) == BAD
    assert lib.pm_jubjub_add_host(_u64p(g), _u64p(off), _u64p(out)) == BAD
    assert lib.pm_jubjub_add_host(None, _u64p(g), _u64p(out)) == BAD
    assert lib.pm_jubjub_add_host(_u64p(g), None, _u64p(out)) == BAD
    assert lib.pm_jubjub_add_host(_u64p(g), _u64p(g), None) == BAD
    assert lib.pm_jubjub_add_host(_u64p(g), _u64p(g), _u64p(out)) == _lib.PM_OK
    assert lib.pm_jubjub_base_point(None, _u64p(out)) == BAD
