"""The linearisation scalars (csrc/prover_rounds.h, linearise: the one copy behind pm_plonk_prove, pm_plonk_prove_batch and
pm_plonk_prove_dist) through the library's pure-host test hook -- no GPU: for random openings and challenges, every
present/absent combination of the four widget selectors and several circuit sizes, each coefficient equals the big-integer
oracle's and r(z) is the sum of coefficient x value at z."""
import ctypes as C
import random

import numpy as np
import pytest

from oracle import bigint_oracle as B
from oracle import plonk_rounds_oracle as P
from oracle.cpu_oracle import ints_to_limbs, limbs_to_ints

R = B.R_MOD
# the values r(z) needs beyond the proof's evaluations, in the hook's order
EXTRAS = ("q_m", "q_o", "q_4", "z", "sigma_4", "q_range", "q_logic", "q_fixed_group_add", "q_variable_group_add")
ROLE_Z, ROLE_SIGMA, ROLE_SELECTOR = 2, 3, 4


@pytest.fixture(scope="module")
def lib():
    from plonk_prototype_amd import _lib
    return _lib.load()


def _mont(vals):
    return np.ascontiguousarray(ints_to_limbs([B.fr_to_mont(v) for v in vals], 4))


def _linearise(lib, n, ev, extras, ch, mask):
    u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    e, x, c = _mont(ev), _mont(extras), _mont(ch)
    coeffs, roles = np.zeros((12, 4), np.uint64), np.zeros(12, np.uint32)
    count, r_z = C.c_uint32(0), np.zeros((1, 4), np.uint64)
    rc = lib.pm_test_plonk_linearise(n, e.ctypes.data_as(u64p), x.ctypes.data_as(u64p), c.ctypes.data_as(u64p), mask,
                                     coeffs.ctypes.data_as(u64p), roles.ctypes.data_as(u32p), C.byref(count),
                                     r_z.ctypes.data_as(u64p))
    assert rc == 0
    k = count.value
    got = [B.fr_from_mont(v) for v in limbs_to_ints(coeffs[:k])]
    return got, [int(r) for r in roles[:k]], B.fr_from_mont(limbs_to_ints(r_z)[0])


def _name(role):
    kind, index = role >> 8, role & 0xFF
    if kind == ROLE_SELECTOR:
        return P.SELECTORS[index]
    assert (kind, index) in ((ROLE_Z, 0), (ROLE_SIGMA, 3)), role
    return "z" if kind == ROLE_Z else "sigma_4"


@pytest.mark.parametrize("n", [4, 8, 1 << 12, 1 << 20, 1 << 26])
def test_linearise_matches_the_oracle(lib, n):
    rng = random.Random(0x4C494E + n)
    for widgets in range(16):                      # bit w: widget selector w (range, logic, fixed, variable) is in the circuit
        present = [s for w, s in enumerate(P.WIDGET_SELECTORS) if widgets >> w & 1]
        mask = 0x7F | sum(1 << P.SELECTORS.index(s) for s in present)
        ev = {k: rng.randrange(R) for k in P.TRANSCRIPT_EVALS}
        ch = {k: rng.randrange(R) for k in P.CHALLENGES}
        xs = {k: rng.randrange(R) for k in EXTRAS}
        for s in P.WIDGET_SELECTORS:
            if s not in present:
                xs[s] = 0                           # what the prover holds for a selector it does not open
        got, roles, r_z = _linearise(lib, n, [ev[k] for k in P.TRANSCRIPT_EVALS], [xs[k] for k in EXTRAS],
                                     [ch[k] for k in P.CHALLENGES], mask)
        names = [_name(r) for r in roles]
        want = P.linearisation_coeffs(ev, ch, n)
        # every polynomial of r once, the widget selectors exactly where the circuit has them
        assert sorted(names) == sorted(["q_m", "q_l", "q_r", "q_o", "q_4", "q_c", "z", "sigma_4"] + present), (n, widgets)
        for nm, c in zip(names, got):
            assert c == want[nm], (n, widgets, nm)
        value = dict(xs, q_l=ev["q_l"], q_r=ev["q_r"], q_c=ev["q_c"])
        assert r_z == sum(c * value[nm] for nm, c in zip(names, got)) % R, (n, widgets)


def test_linearise_rejects_bad_arguments(lib):
    u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    z17, z9, z10 = (np.zeros((k, 4), np.uint64) for k in (17, 9, 10))
    coeffs, roles, count, r_z = np.zeros((12, 4), np.uint64), np.zeros(12, np.uint32), C.c_uint32(0), np.zeros(4, np.uint64)

    def call(n, e):
        return lib.pm_test_plonk_linearise(n, e.ctypes.data_as(u64p), z9.ctypes.data_as(u64p), z10.ctypes.data_as(u64p), 0x7FF,
                                           coeffs.ctypes.data_as(u64p), roles.ctypes.data_as(u32p), C.byref(count),
                                           r_z.ctypes.data_as(u64p))
    assert call(0, z17) == -6                       # PM_ERR_LENGTH
    bad = z17.copy()
    bad[3] = np.uint64(0xFFFFFFFFFFFFFFFF)          # not below r
    assert call(4, bad) == -1                       # PM_ERR_BAD_ARG
    assert lib.pm_test_plonk_linearise(4, None, None, None, 0, None, None, None, None) == -1
