"""The lazy forms of fe_mul_split (csrc/fields.hip.h, D = G: one reduction digit fewer) and the butterflies that take their
results (dft4s_lazy, csrc/ntt_kernels4.hip.h), on the big-integer model of oracle/fe_model.py -- no GPU, no library.

A lazy product keeps the residue and the normalised limbs of the (1, <2) forms and gives up only the size of the value:
below (ceil(9 / G) Bx (1 + 2^-28) + 1) r for data limbs below Bx 2^29.  The forms the radix-2^10 passes use:
    (5, 5)  step twiddles of the first pass   data (<5, .)  -> value < 11.01 r   121 limb products
    (3, 3)  step twiddles of the last pass    data (<5, .)  -> value < 16.01 r   105
    (1, 1)  w4, every step of both            data (4, .)   -> value < 37.01 r    89
The first part checks each at the limits of those classes: exact residue, no 64-bit column wraps, every limb below 2^29
(the top one too), the value under the stated bound.  The second part walks dft4s_lazy with the K constants read from the
kernel source, and then five consecutive steps of both <10, 1> passes, with worst-case members of every class: no routine
is handed an operand outside its precondition, everything a step leaves for the next (what goes to the LDS, to the wide
store, to the canonical exit) is (<5, <60), and 60 r < 2^261, the limit of fe_reduce_weak / fe_reduce_canon_pack."""
import os
import random
import re

import pytest

from oracle import fe_model as M
from oracle.fe_model import FR, MASK, N, R_MOD, RADIX, W, limbs, mul_split, rows_of, value

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RINV = pow(RADIX, -1, R_MOD)
# (G, D): data limb bound Bx, data value class V (the call site's; the routine itself takes any value), limb products
FORMS = {(5, 5): (5, 60, 121), (3, 3): (5, 60, 105), (1, 1): (4, 35, 89)}
STORED = (5, 60)                  # what a step leaves behind: limbs < 5 * 2^29, value < 60 r
assert STORED[1] * R_MOD < RADIX  # fe_reduce_weak / fe_reduce_canon_pack take values below 2^261


def value_bound_ok(r, G, Bx):
    """value < ceil(N / G) Bx (1 + 2^(1 - W)) m + m, in integers"""
    groups = (N + G - 1) // G
    return value(r) << (W - 1) < (groups * Bx * ((1 << (W - 1)) + 1) + (1 << (W - 1))) * R_MOD


def lazy_split(x, rows, G, Bx, what="fe_mul_split"):
    """the device routine with D = G; a violation is recorded for anything outside what its comment promises"""
    if max(x) >= Bx << W:
        M.flag(f"{what}<{G},{G}> precondition: data limbs")
    r, peak, _ = mul_split(x, rows, G, G)
    if peak > M.M64:
        M.flag(f"u64 wrap in {what}<{G},{G}> column")
    if any(v >> W for v in r) or not value_bound_ok(r, G, Bx):
        M.flag(f"{what}<{G},{G}> result class: value / r = {value(r) / R_MOD:.3f}")
    return r


@pytest.fixture(autouse=True)
def clean_log():
    M.VIOLATIONS.clear()
    yield
    M.VIOLATIONS.clear()


def check(x, rows, G, Bx, macs_expected):
    r, peak, macs = mul_split(x, rows, G, G)
    assert macs == macs_expected
    assert peak < 1 << 64, f"column overflow: {peak:#x}"
    assert all(v < 1 << W for v in r), r                               # the top limb too
    t = sum(value(x[j * G:(j + 1) * G]) * value(rows[j]) for j in range(len(rows)))
    assert (value(r) << (W * G)) % R_MOD == t % R_MOD
    assert value(r) << (W * G) >= t and value(r) < (t >> (W * G)) + R_MOD + 1
    assert value_bound_ok(r, G, Bx), value(r) / R_MOD
    return r


def data_members(Bx, V, n_random, seed):
    out = [M.all_max(FR, Bx, V), M.most_redundant(FR, V * R_MOD - 1, Bx), [(Bx << W) - 1] * N,   # the last: any value the limbs allow
           limbs(0), limbs(1), limbs(R_MOD - 1), M.limbs_of(FR, V * R_MOD - 1)]
    rng = random.Random(seed)
    return out + [M.random_member(FR, Bx, V, False, rng) for _ in range(n_random)]


@pytest.mark.parametrize("G,D", sorted(FORMS))
def test_lazy_forms_at_the_class_limits(G, D):
    Bx, V, macs = FORMS[(G, D)]
    groups = (N + G - 1) // G
    rng = random.Random(0x1A27 + G)
    xs = data_members(Bx, V, 300, 77 + G)
    biggest = 0
    for i, x in enumerate(xs):
        for w in (1, R_MOD - 1, 0, rng.randrange(R_MOD)):              # the twiddle, out of Montgomery form
            w_mont = w * RADIX % R_MOD
            r = check(x, rows_of(w_mont, G, D), G, Bx, macs)
            assert value(r) % R_MOD == value(x) * w_mont * RINV % R_MOD   # what fe_mul returns for the same operands
            biggest = max(biggest, value(r))
        if i < 8:
            check(x, [limbs(R_MOD - 1)] * groups, G, Bx, macs)          # every row at r - 1: the value bound
            peak = mul_split(x, [[MASK] * N] * groups, G, D)[1]         # rows the table never holds: the column bound alone
            assert peak < 1 << 64
    assert biggest > 2 * R_MOD                                         # the lazy class is really used: not a (1, <2) result


# ---------------------------------------------------------------------------- dft4s_lazy and the steps around it
def kernel_K():
    """the four BFLY constants of dft4s_lazy, from the kernel source"""
    src = open(os.path.join(ROOT, "plonk-prototype_amd", "csrc", "ntt_kernels4.hip.h")).read()
    body = src.split("PM_DEV void dft4s_lazy(")[1].split("\n}\n")[0]
    K = [int(k) for k in re.findall(r"BFLY\((\d+),", body)]
    assert len(K) == 4
    return K


def kernel_form(in_wide):
    src = open(os.path.join(ROOT, "plonk-prototype_amd", "csrc", "ntt_kernels4.hip.h")).read()
    m = re.search(r"return S == 10 && LT == 1 \? \(in_wide \? (\d) : (\d)\) : 0;", src)
    assert m, "step4_lazy_form"
    return int(m.group(1 if in_wide else 2))


def dft4s_lazy(K, a0, a1, a2, a3, w4_rows):
    f = FR
    M.expect(f, a0, 1, 2, False, "dft4s_lazy in a0")
    for i, a in enumerate((a1, a2, a3)):
        M.expect(f, a, 1, 17, False, f"dft4s_lazy in a{i + 1}")
    a0, a2 = M.bfly(K[0], a0, a2, "dft4s_lazy BFLY 0")
    a1, a3 = M.bfly(K[1], a1, a3, "dft4s_lazy BFLY 1")
    M.expect(f, a0, 2, 19, False, "dft4s_lazy a0")
    M.expect(f, a2, 4, 21, False, "dft4s_lazy a2")
    M.expect(f, a1, 2, 33, False, "dft4s_lazy a1")
    M.expect(f, a3, 4, 35, False, "dft4s_lazy a3")
    a3 = lazy_split(a3, w4_rows, 1, 4, "w4")
    a2 = M.fe_norm(f, a2)
    a0, a1 = M.bfly(K[2], a0, a1, "dft4s_lazy BFLY 2")
    a2, a3 = M.bfly(K[3], a2, a3, "dft4s_lazy BFLY 3")
    out = [a0, a2, a1, a3]
    for i, a in enumerate(out):
        M.expect(f, a, STORED[0], STORED[1], False, f"dft4s_lazy out X{i}")
    return out


def lazy_inputs(G, rng, worst):
    """a0 of (1, <2) and three results of the form's product at (or, worst = False, somewhere inside) the top of their class"""
    Bx = FORMS[(G, G)][0]
    a0 = M.all_max(FR, 1, 2) if worst else limbs(rng.randrange(2 * R_MOD))
    out = [a0]
    for _ in range(3):
        x = [(Bx << W) - 1 - (0 if worst else rng.randrange(1 << 20)) for _ in range(N)]
        out.append(lazy_split(x, rows_of(rng.randrange(R_MOD), G, G), G, Bx))
    return out


def test_dft4s_lazy_with_the_kernel_constants():
    K = kernel_K()
    rng = random.Random(0xD4)
    for G in (3, 5):
        for it in range(200):
            w4 = rows_of(R_MOD - 1 if it == 0 else rng.randrange(R_MOD), 1, 1)
            a = lazy_inputs(G, rng, worst=it < 20)
            want = [value(v) % R_MOD for v in a]
            out = dft4s_lazy(K, *a, w4)
            # the integers: a butterfly adds K r, the w4 product is exact modulo r
            w4v = value(w4[8]) * RINV % R_MOD                          # row 8 is the constant itself
            s0, d0, s1, d1 = want[0] + want[2], want[0] - want[2], want[1] + want[3], (want[1] - want[3]) * w4v
            assert [value(v) % R_MOD for v in out] == [(s0 + s1) % R_MOD, (d0 + d1) % R_MOD, (s0 - s1) % R_MOD, (d0 - d1) % R_MOD]
    # the products' largest possible values, as numbers rather than samples: the subtrahend bounds the K constants rest on
    assert 17 > 16.01 and K[0] - 1 >= 17 and K[1] - 1 >= 17            # twiddled inputs < 16.01 r
    assert K[2] - 1 >= 33                                              # a1 = sum of two of them < 32.02 r
    assert K[3] - 1 >= 38                                              # a3 < 37.01 r after w4
    # X3 = a2 - a3 + K3 r and X1 = a2 + a3 with a2 < (2 + K0) r; X2 = a0 - a1 + K2 r and X0 = a0 + a1 with a0 < (2 + 17) r
    assert max(2 + K[0] + K[3], 2 + K[0] + 38, 2 + 17 + K[2], 2 + 17 + 2 * 17) <= STORED[1]
    assert not M.VIOLATIONS, M.VIOLATIONS[:3]


def worst_stored(rng, i):
    """a member of what a step leaves behind, (<5, <60): the extremes first"""
    if i == 0:
        return M.all_max(FR, *STORED)
    if i == 1:
        return M.most_redundant(FR, STORED[1] * R_MOD - 1, STORED[0])
    return M.random_member(FR, STORED[0], STORED[1], False, rng)


@pytest.mark.parametrize("in_wide", [False, True], ids=["first_pass", "last_pass"])
def test_five_steps_of_a_radix_1024_pass(in_wide):
    """Steps 0 .. 4 as ntt_step4 runs them for <10, 1>: step 0 on (1, <2) inputs; the first-layer products through the (1, 2)
    head rows (behind step 0 in the last pass, at the top of step 1 in the first); steps 2 .. 4 with the pass's lazy form.  One
    chain hands every step the outputs of the one before (as if the exchange were the identity), a second one feeds every step
    the extremes of the stored class, whatever came before."""
    K, G = kernel_K(), kernel_form(in_wide)
    Bx = FORMS[(G, G)][0]
    rng = random.Random(0x57E9 + in_wide)
    w4 = rows_of(rng.randrange(R_MOD), 1, 1)
    for chain in range(40):
        x = [M.all_max(FR, 1, 2) if chain == 0 else limbs(rng.randrange(2 * R_MOD)) for _ in range(4)]   # loaded, or a (1, <2) product
        for step in range(5):
            inject = lambda: [worst_stored(rng, (chain // 2 + m) % 4) for m in range(4)]
            stored_in = step > 0 and not (in_wide and step == 1)       # step 1 of the last pass reads products, (1, <2)
            if stored_in and chain % 2 == 1:                           # the second kind of chain: the class limits, not the data
                x = inject()
            for v in x:
                if stored_in:
                    M.expect(FR, v, STORED[0], STORED[1], False, f"stored before step {step}")
            head = lambda v: M.fe_mul_split(v, rows_of(rng.randrange(R_MOD), 1, 2), 1, 2)      # (1, 2): flags anything outside (1, <2)
            if step == 1 and not in_wide:                              # L1_CONSUMER: the first pass multiplies at the top of step 1
                x = [M.fe_reduce_weak(FR, x[0])] + [head(v) for v in x[1:]]
            elif step >= 2:
                x = [M.fe_reduce_weak(FR, x[0])] + [lazy_split(v, rows_of(rng.randrange(R_MOD), G, G), G, Bx) for v in x[1:]]
            x = dft4s_lazy(K, *x, w4)
            if step == 0 and in_wide:                                  # L1_UNIFORM: the last pass multiplies behind step 0
                if chain % 2 == 1:
                    x = inject()
                x = [M.fe_reduce_weak(FR, x[0])] + [head(v) for v in x[1:]]
        for v in x:                                                    # the exits
            if in_wide:                                                # fe_reduce_canon_pack: weak reduction, then canonical
                weak = M.fe_reduce_weak(FR, v)
                assert value(weak) % R_MOD == value(v) % R_MOD and value(weak) < 2 * R_MOD
                assert M.fe_canon_pack(FR, weak) is not None
                scaled = M.fe_mul(FR, v, limbs(rng.randrange(R_MOD)))  # PASS_POST_SCALE / PASS_POST_COSET instead
            else:                                                      # the producer-side inter-pass product, canonical entry
                scaled = M.fe_mul(FR, v, limbs(rng.randrange(R_MOD)))
            assert M.in_class(FR, scaled, 1, 2)
    assert not M.VIOLATIONS, M.VIOLATIONS[:3]
