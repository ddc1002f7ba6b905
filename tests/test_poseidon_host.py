"""Host-side ground for the native Poseidon: the new exports are in the header, the ctypes table and
the Rust bindings, and the two pure-host forms (pm_hades_permute_host, pm_poseidon_hash_host: csrc/host_field.h, no context)
agree with the big-integer model of tests/poseidon_model.py on every shape, with one matrix and with one a round, on edge
states, on every message length around the rate, and refuse what the header says they refuse.  No device here."""
import ctypes as C
import os
import random
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import poseidon_model as PM  # noqa: E402
from conftest import ROOT  # noqa: E402

R = PM.R
EXPORTS = ("pm_hades_params_create", "pm_hades_params_from_key", "pm_hades_params_info", "pm_hades_params_free",
           "pm_hades_permute_dev", "pm_poseidon_hash_dev", "pm_poseidon_merkle_dev", "pm_poseidon_merkle_paths_dev",
           "pm_hades_permute_host", "pm_poseidon_hash_host")


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def _consts(shape, n_mds, seed):
    ark, mds = PM.constants(shape[0], n_mds, seed)
    a, m, k = PM.flat(ark, mds)
    return ark, mds, PM.to_limbs(a), PM.to_limbs(m), k


def test_exports_are_declared_bound_and_documented():
    import plonk_prototype_amd as pa
    from plonk_prototype_amd import _lib
    header = open(os.path.join(ROOT, "include", "plonk_mi355x.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = C.CDLL(pa.LIB_PATH)
    for name in EXPORTS:
        assert re.search(rf"\b{name}\(", header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert f"pub fn {name}(" in doc, name
    assert re.search(r"#define PM_HADES_FORM_AUTO 0u\n#define PM_HADES_FORM_THREAD 1u\n#define PM_HADES_FORM_WAVE 2u", header)
    assert (_lib.HADES_FORM_AUTO, _lib.HADES_FORM_THREAD, _lib.HADES_FORM_WAVE) == (0, 1, 2)
    assert "#define PM_POSEIDON_MERKLE_MAX_HEIGHT 15u" in header and _lib.POSEIDON_MERKLE_MAX_HEIGHT == 15
    for name in ("Hades", "MerkleTree", "hades_permute_host", "poseidon_hash_host"):
        assert hasattr(pa, name), name


@pytest.mark.parametrize("shape", PM.SHAPES)
@pytest.mark.parametrize("per_round", (False, True))
def test_permute_host_against_the_model(shape, per_round):
    import plonk_prototype_amd as pa
    rounds, full = shape
    ark, mds, a, m, k = _consts(shape, rounds if per_round else 1, 100 * rounds + per_round)
    assert k == (rounds if per_round else 1)
    rng = random.Random(rounds)
    states = [[rng.randrange(R) for _ in range(5)] for _ in range(4)]
    states += [[0] * 5, [R - 1] * 5, [0, R - 1, 0, R - 1, 0], [R - 1, 0, 0, 0, R - 1], [1, 0, R - 1, 2, R - 2]]
    lib = pa.load()
    for s in states:
        want = PM.HM.hades_model(s, ark, mds, rounds, full)
        buf = PM.to_limbs(s)
        assert lib.pm_hades_permute_host(rounds, full, _p(a), _p(m), k, _p(buf)) == 0
        assert buf.tobytes() == PM.to_limbs(want).tobytes(), (shape, per_round, s)
        got = pa.hades_permute_host(a, m, PM.to_limbs(s), rounds, full)                  # the Python wrapper, the same call
        assert got.tobytes() == buf.tobytes()


@pytest.mark.parametrize("capacity", (0, 0x1234567 << 200))
def test_hash_host_for_every_length_around_the_rate(capacity):
    import plonk_prototype_amd as pa
    lib = pa.load()
    cap = PM.to_limbs([capacity])
    for shape, per_round in (((5, 2), True), ((67, 8), False)):
        rounds, full = shape
        ark, mds, a, m, k = _consts(shape, rounds if per_round else 1, 7 + rounds)
        rng = random.Random(capacity % 1000 + rounds)
        for length in range(1, 10):
            msg = [rng.randrange(R) for _ in range(length)]
            if length == 4:
                msg = [0, R - 1, 0, R - 1]
            want = PM.sponge(msg, ark, mds, rounds, full, capacity)
            out = np.zeros(4, np.uint64)
            assert lib.pm_poseidon_hash_host(rounds, full, _p(a), _p(m), k, _p(cap), _p(PM.to_limbs(msg)), length, _p(out)) == 0
            assert out.tobytes() == PM.to_limbs([want]).tobytes(), (shape, length)
            assert pa.poseidon_hash_host(a, m, PM.to_limbs(msg), capacity, rounds, full).tobytes() == out.tobytes()


def test_the_sponge_is_the_modelled_circuits():
    """hades_circuits.sponge_case lays out two chunks (four inputs, then two and the padding) with FRESH constants for each
    permutation: chained by hand through hades_model it gives the circuit's hash variable, and with one set of constants the
    same chain is poseidon_model.sponge -- the absorption and the padding are the builder's."""
    import hades_circuits as HC
    b, inputs, out, _ = HC.sponge_case()
    a = inputs(1)
    _, full, reasons = b.model(a)
    assert not reasons
    (r0, _, _, ark1, mds1), (_, _, _, ark2, mds2) = b.permutations
    assert [(p[1], p[2]) for p in b.permutations] == [(5, 2), (5, 2)] and ark1 != ark2
    # the message: what the first absorption adds to the zero state, then the two inputs of the second chunk
    first = [full[b.wires[0][r0 + j]] for j in range(5)]                     # a of the first permutation's key rows
    assert first[0] == 0

    def chain(c1, c2, tail):
        s = PM.HM.hades_model(first, *c1, 5, 2)
        s = [s[0], (s[1] + tail[0]) % R, (s[2] + tail[1]) % R, (s[3] + 1) % R, s[4]]
        return PM.HM.hades_model(s, *c2, 5, 2)[1]

    r1 = b.permutations[1][0]
    second = [full[b.wires[0][r1 + j]] for j in range(5)]
    after1 = PM.HM.hades_model(first, ark1, mds1, 5, 2)
    tail = [(second[1] - after1[1]) % R, (second[2] - after1[2]) % R]
    assert second[3] == (after1[3] + 1) % R and second[0] == after1[0] and second[4] == after1[4]
    assert chain((ark1, mds1), (ark2, mds2), tail) == full[out]
    assert chain((ark1, mds1), (ark1, mds1), tail) == PM.sponge(first[1:] + tail, ark1, mds1, 5, 2)


def test_refusals():
    import plonk_prototype_amd as pa
    lib = pa.load()
    ark, mds, a, m, k = _consts((5, 2), 5, 3)
    _, _, a1, m1, _ = _consts((5, 2), 1, 3)
    state, out, cap = PM.to_limbs([1, 2, 3, 4, 5]), np.zeros(4, np.uint64), PM.to_limbs([0])
    msg = PM.to_limbs([9, 8, 7])

    def permute(rounds, full, a_, m_, k_, s_=state):
        return lib.pm_hades_permute_host(rounds, full, _p(a_), _p(m_), k_, _p(s_.copy()))

    def hash_(rounds, full, a_, m_, k_, cap_=cap, msg_=msg, length=3):
        return lib.pm_poseidon_hash_host(rounds, full, _p(a_), _p(m_), k_, _p(cap_), _p(msg_), length, _p(out))

    assert permute(5, 2, a, m, 5) == 0 and permute(5, 2, a1, m1, 1) == 0 and hash_(5, 2, a, m, 5) == 0
    for call in (permute, hash_):
        assert call(5, 3, a, m, 5) == -1            # F odd
        assert call(5, 6, a, m, 5) == -1            # F > R
        assert call(0, 0, a, m, 0) == -1            # R = 0
        assert call(0, 0, a, m, 1) == -1
        assert call(5, 2, a, m, 2) == -1            # n_mds neither 1 nor R
        assert call(5, 2, a, m, 0) == -1
        for bad_v in (R, R + 1, (1 << 256) - 1):    # a constant that is not below the modulus
            bad_a, bad_m = a.copy(), m.copy()
            bad_a[7] = np.frombuffer(bad_v.to_bytes(32, "little"), np.uint64)
            bad_m[100] = np.frombuffer(bad_v.to_bytes(32, "little"), np.uint64)
            assert call(5, 2, bad_a, m, 5) == -1 and call(5, 2, a, bad_m, 5) == -1
    assert hash_(5, 2, a, m, 5, length=0) == -1     # msg_len = 0
    bad = np.frombuffer(R.to_bytes(32, "little"), np.uint64).reshape(1, 4)
    assert hash_(5, 2, a, m, 5, cap_=bad) == -1 and hash_(5, 2, a, m, 5, msg_=np.concatenate([msg[:2], bad])) == -1
    bad_state = state.copy()
    bad_state[4] = bad[0]
    assert permute(5, 2, a, m, 5, bad_state) == -1
    assert lib.pm_hades_permute_host(5, 2, None, _p(m), 5, _p(state.copy())) == -1
    assert lib.pm_hades_permute_host(5, 2, _p(a), _p(m), 5, None) == -1
    assert lib.pm_hades_params_info(None, None, None, None) == -1
    with pytest.raises(ValueError):
        pa.hades_permute_host(a, m, state, 5, 3)
    with pytest.raises(ValueError):
        pa.poseidon_hash_host(a[:-1], m, msg, 0, 5, 2)
