"""The binary-GCD inversion of csrc/field_inv.hip.h ON THE INTEGERS IT ITERATES ON.

The raw hooks (pm_test_field_raw_op, ops 20 - 22: fe_canon_limbs, fe_inv_int, fe_inv_dev) take radix-2^W limbs as they are,
so a case of tests/inv_cases.py is the integer y the GCD starts from -- not the Montgomery image of a small number.  The lists
reach every round count up to ROUNDS, the exact path and the sign repair of either row (tests/test_fe_inv_model.py asserts
that in the model); here the device must give the model's limbs (oracle/fe_model.py), and, independently of the model, a
number that inverts y.  The hook's blocks are single waves, 64 consecutive cases each, and fe_inv_int leaves through a vote of
the wave: every case is run in several companies -- a wave that leaves at the case's own round count, one that runs all
ROUNDS rounds, partial last waves -- and must come out the same limb for limb.  Then the production kernels with y chosen:
the elementwise inverse (pm_test_field_op 6 / 7) and the batch inversion.  Every comparison is exact."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inv_cases as IC  # noqa: E402
from oracle import bigint_oracle as B  # noqa: E402
from oracle import fe_model as M  # noqa: E402
from oracle.cpu_oracle import ints_to_limbs, limbs_to_ints  # noqa: E402

pytestmark = pytest.mark.gpu

FIELDS = IC.FIELDS
CANON_LIMBS, INV_INT, INV_DEV = 20, 21, 22                           # enum RawOp, csrc/test_hooks.hip
WAVE = 64                                                            # the hook's block: cases 64 k .. 64 k + 63 share a wave


@pytest.fixture(autouse=True)
def clean_log():
    M.VIOLATIONS.clear()
    yield
    M.VIOLATIONS.clear()


def val(f, l):
    return M.value_of(f, l)


def run(ctx, f, op, operands):
    """operands: one limb list per case, in launch order -> one tuple of result limbs per case, one launch"""
    x = np.array(operands, dtype=np.uint64)
    assert x.ndim == 2 and x.shape[1] == f.N and int(x.max()) <= M.M32
    out = ctx.field_raw_op(IC.FIELD_ID[f.name], op, x.astype(np.uint32).reshape(-1, 1, f.N), 1)
    return [tuple(r) for r in out.reshape(-1, f.N).tolist()]


def limbs_all(f, ys):
    return [M.limbs_of(f, y) for y in ys]


# ---------------------------------------------------------------------------- fe_inv_int
@pytest.mark.parametrize("f", FIELDS, ids=repr)
def test_inv_int_raw(ctx, f):
    """every case in natural order: the model's limbs; and v y = 1 (mod m) with v < 64 m, whatever the model says"""
    m = f.mod
    walked, violations = IC.walk(f)
    assert not violations, violations[:3]
    got = run(ctx, f, INV_INT, limbs_all(f, [y for y, _, _ in walked]))
    for (y, want, trace), g in zip(walked, got):
        assert g == want, f"y = {y:#x} ({trace['rounds']} rounds): {g} != {want}"
        assert val(f, g) * y % m == (1 if y else 0) and val(f, g) < 64 * m, hex(y)


@pytest.mark.parametrize("f", FIELDS, ids=repr)
def test_wave_company(ctx, f):
    """A round run after a lane's a has reached zero leaves its b and v as they are (field_inv.hip.h), so the result cannot
    depend on when the wave's vote ends the loop: every case alone among 63 zeros (the wave leaves at this lane's own round
    count), beside the full-round y (the wave runs all ROUNDS rounds), in natural order, and in a last partial wave of 1 and
    of 63 live lanes (the other lanes redo element n - 1 and store nothing) -- raw limbs equal in all of them."""
    walked, _ = IC.walk(f)
    ys = [y for y, _, _ in walked]
    limbs = limbs_all(f, ys)
    want = [w for _, w, _ in walked]
    zero, full = [0] * f.N, M.limbs_of(f, IC.FULL_ROUND[f.name])
    natural = run(ctx, f, INV_INT, limbs)
    # alone: case i in wave i, at lane i % 64
    ops = [zero] * (WAVE * len(ys))
    for i, l in enumerate(limbs):
        ops[WAVE * i + i % WAVE] = l
    got = run(ctx, f, INV_INT, ops)
    alone = [got[WAVE * i + i % WAVE] for i in range(len(ys))]
    zero_out = tuple(M.limbs_of(f, 32 * f.mod))                      # ... and the zeros beside it come out as 0 + 32 m
    assert all(got[WAVE * i + (i + 1) % WAVE] == zero_out for i in range(0, len(ys), 7))
    # 63 cases and the full-round y at the last lane of every wave
    ops, where = [], []
    for k in range(0, len(limbs), WAVE - 1):
        chunk = limbs[k:k + WAVE - 1]
        where += range(len(ops), len(ops) + len(chunk))
        ops += chunk + [zero] * (WAVE - 1 - len(chunk)) + [full]
    got = run(ctx, f, INV_INT, ops)
    beside_full = [got[j] for j in where]
    # last partial waves: n % 64 = 63 (63 cases a launch; the last launch takes the last 63), n % 64 = 1 (one launch a case)
    partial63 = [None] * len(ys)
    for k in list(range(0, len(ys) - (WAVE - 1), WAVE - 1)) + [len(ys) - (WAVE - 1)]:
        partial63[k:k + WAVE - 1] = run(ctx, f, INV_INT, limbs[k:k + WAVE - 1])
    partial1 = [run(ctx, f, INV_INT, [l])[0] for l in limbs]
    for i, y in enumerate(ys):
        seen = {"natural": natural[i], "alone": alone[i], "beside the full-round y": beside_full[i], "n % 64 = 63": partial63[i],
                "n % 64 = 1": partial1[i]}
        assert all(g == want[i] for g in seen.values()), f"y = {y:#x} ({walked[i][2]['rounds']} rounds): {seen}, model {want[i]}"


@pytest.mark.parametrize("f", FIELDS, ids=repr)
def test_all_zero_wave(ctx, f):
    """the vote lets an all-zero wave go before round 0: v = 0, which fe_inv_int hands back as 0 + 32 m (the model's limbs),
    and fe_inv_dev as a representative of 0; whole waves and a partial one"""
    n = 2 * WAVE + 5
    want = tuple(M.fe_inv_int(f, [0] * f.N))
    assert list(want) == M.limbs_of(f, 32 * f.mod)
    assert run(ctx, f, INV_INT, [[0] * f.N] * n) == [want] * n
    want = tuple(M.fe_inv_dev(f, [0] * f.N))
    assert val(f, want) in (0, f.mod)
    assert run(ctx, f, INV_DEV, [[0] * f.N] * n) == [want] * n
    assert not M.VIOLATIONS


# ---------------------------------------------------------------------------- fe_canon_limbs, fe_inv_dev
@pytest.mark.parametrize("f", FIELDS, ids=repr)
def test_canon_limbs_raw(ctx, f):
    """the members of its class (value < 2 m, limbs < 2^32 - 2^(32-W)): the canonical limbs of value mod m"""
    cases = IC.canon_cases(f)
    for l, g in zip(cases, run(ctx, f, CANON_LIMBS, [list(l) for l in cases])):
        assert list(g) == M.limbs_of(f, val(f, l) % f.mod) == M.fe_canon_limbs(f, list(l)), l
    assert not M.VIOLATIONS, M.VIOLATIONS[:3]


@pytest.mark.parametrize("f", FIELDS, ids=repr)
def test_inv_dev_raw(ctx, f):
    """x = y and y + m, normalised and in the most redundant limbs fe_canon_limbs admits (x = 0 and x = m among them): the
    model's limbs, in fe_mul's result class (limbs < 2^W, value < 2 m), with value * x = R'^2 (mod m), 0 for x = 0 (mod m).
    The model's fe_inv_dev is fe_mul(fe_inv_int(fe_canon_limbs(x)), 2^(3 W N) mod m); the four x of one y share the walk
    of fe_inv_int (their canonical limbs are asserted equal), and every 16th case walks fe_inv_dev whole."""
    m, r2, c = f.mod, f.RADIX * f.RADIX % f.mod, M.fe_pow2(f, 3 * f.W * f.N)
    walked, _ = IC.walk(f)
    ops, want = [], []
    for i, (y, v, _) in enumerate(walked):
        w = tuple(M.fe_mul(f, list(v), c))
        for x in (M.limbs_of(f, y), M.limbs_of(f, y + m), IC.redundant(f, y), IC.redundant(f, y + m)):
            assert M.fe_canon_limbs(f, x) == M.limbs_of(f, y)
            if i % 16 == 0:
                assert tuple(M.fe_inv_dev(f, x)) == w
            ops.append(x)
            want.append((y, w))
    assert not M.VIOLATIONS, M.VIOLATIONS[:3]
    for x, (y, w), g in zip(ops, want, run(ctx, f, INV_DEV, ops)):
        assert g == w, f"y = {y:#x}, x = {x}: {g} != {w}"
        assert M.in_class(f, g, 1, 2) and val(f, g) * val(f, x) % m == (r2 if y else 0), hex(y)


# ---------------------------------------------------------------------------- production kernels, the integer chosen
@pytest.mark.parametrize("f", FIELDS, ids=repr)
def test_field_op_inverse_of_chosen_integers(ctx, f):
    """pm_test_field_op 6 / 7 with y itself as the ABI limbs, no to_mont: field_op_kernel hands the loaded limbs to fe_inv_int
    as they are and multiplies by 2^(64 NS + W N) (with the product's 1 / R': the comment in api.hip reads "the integer inverse
    of x R is x^-1 / R; times R^2 R' ... = x^-1 R"), so the result is y^-1 * 2^(64 NS) mod m as a raw integer."""
    m, nl, op = f.mod, f.NS // 2, 6 if f is M.FR else 7
    ys = list(IC.cases(f))
    k = pow(2, 64 * f.NS, m)
    a = ints_to_limbs(ys, nl)
    got = limbs_to_ints(ctx.field_op(op, a, a))
    for y, g in zip(ys, got):
        assert g == (pow(y, -1, m) * k % m if y else 0), hex(y)


def test_batch_inverse_of_chosen_integers(ctx, oracle):
    """Polynomial.batch_inverse with n <= 256 and default options: one block of 256 threads, one quad a thread, so thread t holds
    element t alone and inverts abi_to_dev(a_t) = 32 a_t mod r.  With a_t = y / 32 mod r as raw limbs the GCD iterates on y.
    (A zero element is skipped by the kernel: its thread inverts fe_one.)  The Fr list in slices of 256, in natural order and
    dealt out so that every wave holds a zero element, the full-round y and cases of every round count; byte for byte against
    the C oracle."""
    import plonk_prototype_amd as pa
    f, r = M.FR, B.R_MOD
    walked, _ = IC.walk(f)
    inv32 = pow(32, -1, r)
    by_rounds = [y for y, _, t in sorted(walked, key=lambda c: (c[2]["rounds"], c[0])) if y]
    waves = -(-len(by_rounds) // (WAVE - 2))
    mixed = []
    for w in range(waves):                                           # wave w: a zero, the full-round y, then every waves-th case
        mixed += [0, IC.FULL_ROUND["fr"]] + by_rounds[w::waves]
        mixed += [1] * (-len(mixed) % WAVE)
    for order in (list(IC.cases(f)), mixed):
        for k in range(0, len(order), 256):
            ys = order[k:k + 256]
            a_int = [y * inv32 % r for y in ys]
            assert all(32 * a % r == y for a, y in zip(a_int, ys))
            a = ints_to_limbs(a_int, 4)
            got = pa.Polynomial.from_host(ctx, a).batch_inverse().to_host()
            want = oracle.fr_batch_inverse(a)
            bad = [hex(y) for y, g, w in zip(ys, got, want) if not np.array_equal(g, w)]
            assert not bad, bad[:5]
