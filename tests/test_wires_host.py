"""Composer-form circuits, the parts that need no GPU: the new exports and their bindings, the
geometry of the sort behind pm_plonk_sigma_from_wires (pm_test_wire_sort_plan), the two forms of ``Circuit`` and the
wire-form synthetic generators against their dense twins."""
import ctypes as C
import os

import numpy as np
import pytest

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "plonk_mi355x.h")
WIRE_EXPORTS = ("pm_plonk_sigma_from_wires", "pm_plonk_sigma_from_wires_dev", "pm_plonk_preprocess_wires",
                "pm_plonk_key_num_vars", "pm_plonk_witness_from_vars_dev", "pm_test_wire_sort_plan")


def test_exports_bindings_and_header():
    import plonk_prototype_amd as pa
    from plonk_prototype_amd import _lib
    header = open(HEADER).read()
    raw = C.CDLL(pa.LIB_PATH)
    bound = pa.load()
    for name in WIRE_EXPORTS:
        assert hasattr(raw, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES, name
        assert name + "(" in header, name
        assert getattr(bound, name).argtypes == _lib.SIGNATURES[name][1]
        assert getattr(bound, name).restype == _lib.SIGNATURES[name][0]
    assert "#define PM_PLONK_NO_VAR 0xffffffffu" in header and _lib.PLONK_NO_VAR == 0xFFFFFFFF
    vp, sz = C.c_void_p, C.c_size_t
    assert _lib.SIGNATURES["pm_plonk_sigma_from_wires"] == (C.c_int, [vp, _lib.u32p, sz, sz, C.POINTER(C.c_int64)])
    assert _lib.SIGNATURES["pm_plonk_sigma_from_wires_dev"] == (C.c_int, [vp, vp, sz, sz, vp, vp])
    assert _lib.SIGNATURES["pm_plonk_preprocess_wires"] == (C.c_int, [vp, C.POINTER(_lib.u64p), _lib.u32p, sz, sz, C.POINTER(vp)])
    assert _lib.SIGNATURES["pm_plonk_key_num_vars"] == (sz, [vp])
    assert _lib.SIGNATURES["pm_plonk_witness_from_vars_dev"] == (C.c_int, [vp, vp, vp, sz, C.c_uint32, vp, vp])
    assert pa.sigma_from_wires is pa.prover.sigma_from_wires


def _plan(lib, n, num_vars):
    passes, tiles, scratch = C.c_uint32(), C.c_uint32(), C.c_size_t()
    rc = lib.pm_test_wire_sort_plan(n, num_vars, C.byref(passes), C.byref(tiles), C.byref(scratch))
    return rc, passes.value, tiles.value, scratch.value


def test_wire_sort_plan():
    import plonk_prototype_amd as pa
    from plonk_prototype_amd import _lib
    lib = pa.load()
    tile = _lib.WIRE_SORT_TILE
    for num_vars, want in ((256, 1), (257, 2), (65536, 2), (65537, 3), (1 << 24, 3), ((1 << 24) + 1, 4), ((1 << 32) - 1, 4)):
        assert _plan(lib, 1 << 10, num_vars)[:2] == (0, want), num_vars
    for num_vars in (0, 1):
        rc, passes, _, _ = _plan(lib, 1 << 10, num_vars)
        assert rc == 0 and passes >= 1
    last = 0
    for log_n in range(2, 25):
        n = 1 << log_n
        rc, passes, tiles, scratch = _plan(lib, n, n + 1)
        assert rc == 0 and tiles == -(-4 * n // tile) and passes == -(-(log_n + 1) // 8)     # ids up to n: log_n + 1 bits
        assert scratch > last and scratch >= 64 * n               # two pair buffers of 4n x 8 bytes, plus counts
        assert scratch <= 64 * n + 1024 * tiles + (1 << 16)
        last = scratch
    assert lib.pm_test_wire_sort_plan(1 << 10, 300, None, None, None) == 0
    for bad_n in (0, 1, 2, 3, 12, 1000, (1 << 30)):
        assert _plan(lib, bad_n, 10)[0] == _lib.PM_ERR_LENGTH, bad_n
    assert _plan(lib, 1 << 10, 1 << 32)[0] == _lib.PM_ERR_BAD_ARG      # ids are 32 bit and PM_PLONK_NO_VAR is no id


def test_circuit_takes_exactly_one_form_of_the_permutation():
    import plonk_prototype_amd as pa
    n = 8
    c, _, _ = pa.synthetic.chain_circuit(n, 3)
    sel = {k: getattr(c, k) for k in pa.prover.SELECTORS}
    wv = np.zeros((4, n), np.uint32)
    assert pa.Circuit(sigma_index=c.sigma_index, **sel).n == n
    w = pa.Circuit(wire_vars=wv, num_vars=1, **sel)
    assert w.n == n and w.sigma_index is None
    with pytest.raises(ValueError):
        pa.Circuit(sigma_index=c.sigma_index, wire_vars=wv, num_vars=1, **sel)
    with pytest.raises(ValueError):
        pa.Circuit(**sel)
    with pytest.raises(ValueError):
        pa.Circuit(wire_vars=wv, **sel)                           # the ids need their range
    assert pa.Circuit(**c.__dict__).sigma_index is c.sigma_index      # the copy idiom of the existing tests


@pytest.mark.parametrize("n,seed", [(4, 1), (64, 7), (1024, 3)])
def test_chain_circuit_wires_is_chain_circuit(n, seed):
    import plonk_prototype_amd as pa
    S = pa.synthetic
    rows = (0, n - 1)
    dense, wit, pi = S.chain_circuit(n, seed, public_rows=rows, zero_selectors=("q_r",))
    wires, variables, pi_w = S.chain_circuit_wires(n, seed, public_rows=rows, zero_selectors=("q_r",))
    assert wires.sigma_index is None and wires.num_vars == n + 1 == variables.shape[0]
    assert wires.wire_vars.shape == (4, n) and wires.wire_vars.dtype == np.uint32
    assert np.array_equal(variables[wires.wire_vars], wit) and np.array_equal(pi_w, pi)
    for k in pa.prover.SELECTORS:
        a, b = getattr(dense, k), getattr(wires, k)
        assert (a is None and b is None) or np.array_equal(a, b), k
    # the same copy classes as the dense circuit's sigma: following sigma never leaves a variable
    sig = dense.sigma_index.reshape(-1)
    flat = wires.wire_vars.reshape(-1)
    assert np.array_equal(flat[sig], flat)


@pytest.mark.parametrize("n,seed", [(8, 1), (64, 2), (4096, 5)])
def test_boolean_circuit_wires_is_boolean_circuit(n, seed):
    import plonk_prototype_amd as pa
    S = pa.synthetic
    dense, wit, pi = S.boolean_circuit(n, seed)
    wires, variables, pi_w = S.boolean_circuit_wires(n, seed)
    assert wires.num_vars == variables.shape[0] and int(wires.wire_vars.max()) == wires.num_vars - 1
    assert np.array_equal(variables[wires.wire_vars], wit) and np.array_equal(pi_w, pi)
    for k in pa.prover.SELECTORS:
        a, b = getattr(dense, k), getattr(wires, k)
        assert (a is None and b is None) or np.array_equal(a, b), k
    flat = wires.wire_vars.reshape(-1)
    assert np.array_equal(flat[dense.sigma_index.reshape(-1)], flat)
    # one id at about n positions: the shared zero of the d column
    assert np.bincount(flat).max() >= n * 7 // 8
