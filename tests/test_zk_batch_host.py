"""Host-side ground for zero-knowledge batches (pm_plonk_prove_batch_zk): the new exports are in the
library and bound with the declared argument types, the Python entry points take the new keywords, and random_blinders
draws one independent set per proof.  No device compute here."""
import ctypes as C
import inspect

import numpy as np
import pytest

ZK_BATCH_EXPORTS = ("pm_plonk_batch_enable_zk", "pm_plonk_batch_zk_bytes", "pm_plonk_prove_batch_zk")


def test_zk_batch_symbols_exported_and_bound():
    import plonk_prototype_amd as pa
    from plonk_prototype_amd import _lib
    lib = C.CDLL(pa.LIB_PATH)
    for name in ZK_BATCH_EXPORTS:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    bound = pa.load()
    for name in ZK_BATCH_EXPORTS:
        assert getattr(bound, name).argtypes == _lib.SIGNATURES[name][1]
        assert getattr(bound, name).restype == _lib.SIGNATURES[name][0]
    res, args = _lib.SIGNATURES["pm_plonk_prove_batch_zk"]
    plain = _lib.SIGNATURES["pm_plonk_prove_batch"][1]
    assert res is C.c_int and args[:-2] == plain[:-1] and args[-2] is _lib.u64p and args[-1] is plain[-1]
    assert _lib.SIGNATURES["pm_plonk_batch_enable_zk"] == (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)])
    assert _lib.SIGNATURES["pm_plonk_batch_zk_bytes"] == (C.c_size_t, [C.c_void_p])
    assert bound.pm_plonk_batch_zk_bytes(None) == 0          # a null workspace holds nothing


def test_python_entry_points_take_the_new_keywords():
    import plonk_prototype_amd as pa
    sig = inspect.signature(pa.prove_batch)
    assert sig.parameters["zero_knowledge"].default is False and sig.parameters["blinders"].default is None
    assert inspect.signature(pa.ProverKey.batch).parameters["zero_knowledge"].default is False
    assert callable(pa.BatchWorkspace.enable_zk)
    assert inspect.signature(pa.prover.random_blinders).parameters["count"].default is None
    doc = pa.prove_batch.__doc__
    assert "tests only" in doc and "zero_knowledge" in doc


def test_random_blinders_per_proof():
    from plonk_prototype_amd.field import R_MOD, fr_from_limbs
    from plonk_prototype_amd.prover import random_blinders
    one = random_blinders()
    assert one.shape == (17, 4) and one.dtype == np.uint64          # the single prover's form is unchanged
    for count in (1, 5, 64):
        bl = random_blinders(count)
        assert bl.shape == (count, 17, 4) and bl.dtype == np.uint64
        vals = [[fr_from_limbs(bl[b, i]) for i in range(17)] for b in range(count)]
        assert all(0 <= v < R_MOD for row in vals for v in row)
        assert len({tuple(row) for row in vals}) == count, "every proof needs its own blinders"
        assert len({v for row in vals for v in row}) == 17 * count
    assert random_blinders(0).shape == (0, 17, 4)
    with pytest.raises(ValueError):
        random_blinders(-1)
