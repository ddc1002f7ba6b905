"""The circuits of tests/test_gpu_composed_gadgets.py, built once and shared with tests/test_composed_gadgets_host.py (which
checks that the model's own output satisfies them).  Each function returns the builder, the assignments of its inputs and what
else its test needs; nothing here touches the library."""
import functools
import random

import composed_gadget_model as CM
import gadget_model as M

R = M.R
ALT01, ALT0011 = int("01" * 128, 2) % R, int("0011" * 64, 2) % R
BITS_SMALL, BITS_FULL = (1, 2, 31, 32, 33, 64, 255), (256,)


def _bits_values(B, rng):
    vals = [0, 1, ((1 << B) - 1) % R, R - 1, ALT01, ALT0011]
    if (1 << B) < R:
        vals.append(1 << B)
    return vals


def bits_circuit(widths):
    """one BITS gadget per width whose sum starts from an INPUT variable (0, 1, r - 1 over the assignments), one more of the
    first width that starts from the zero variable.  64 assignments: every edge value with every start, then random ones."""
    b = CM.Builder(1024)
    start = b.var(True)
    vvars = []
    for B in widths:
        v = b.var(True)
        vvars.append(v)
        b.bits(v, B, acc0=start)
    v0 = b.var(True)
    b.bits(v0, widths[0], acc0=0)
    arith = b.fill_arithmetic(21)
    rng = random.Random(21)
    assignments = []
    for s in (0, 1, R - 1):
        for e in range(7):
            a = {start: s, v0: rng.randrange(R), **arith}
            for v, B in zip(vvars, widths):
                vals = _bits_values(B, rng)
                a[v] = vals[e % len(vals)]
            assignments.append(a)
    while len(assignments) < 64:
        assignments.append({start: rng.randrange(R), v0: rng.randrange(R), **{v: rng.randrange(R) for v in vvars}, **arith})
    return b, assignments


@functools.lru_cache(maxsize=None)
def bits_case(which):
    b, assignments = bits_circuit(BITS_SMALL if which == "small" else BITS_FULL)
    return b, assignments, [b.model(a) for a in assignments]


@functools.lru_cache(maxsize=None)
def maybe_equal_case():
    """65 gadgets in one level: a full wave and a partial one"""
    b = CM.Builder(256)
    pairs = [(b.var(True), b.var(True)) for _ in range(65)]
    outs = [b.maybe_equal(x, y)[0] for x, y in pairs]
    arith = b.fill_arithmetic(22)
    rng = random.Random(22)
    assignments = []
    for p in range(3):
        a = dict(arith)
        for g, (x, y) in enumerate(pairs):
            diff = (0, 1, R - 1, rng.randrange(R))[(g + p) % 4]
            a[y] = rng.randrange(R)
            a[x] = (a[y] + diff) % R
        assignments.append(a)
    return b, assignments, [b.model(a) for a in assignments], outs


@functools.lru_cache(maxsize=None)
def arith_case():
    """two independent runs in one level.  Run 1: every row reads the row before it, through a, then b, then d; a row whose d
    is no variable; a row with c = a.  Run 2: coefficients 0, 1, r - 1 and random ones in every position."""
    b = CM.Builder(64)
    rng = random.Random(23)
    x, y, w, flag = b.var(True), b.var(True), b.var(True), b.var(True)
    rnd = lambda: rng.randrange(R)   # noqa: E731
    full = lambda: dict(q_m=rnd(), q_l=rnd(), q_r=rnd(), q_4=rnd(), q_c=rnd())   # noqa: E731
    c0, c1, c2, c3 = b.var(), b.var(), b.var(), b.var()
    b.arith([(x, y, c0, w, full()),
             (c0, y, c1, w, full()),             # reads row 0 through a
             (x, c1, c2, w, full()),             # ... row 1 through b
             (x, y, c3, c2, full()),             # ... row 2 through d
             (c3, c3, None, None, full()),       # d is no variable: it reads as zero
             (flag, flag, flag, None, dict(q_m=1))])   # c = a: the boolean row
    pick = (0, 1, R - 1, None)
    chain, prev = [], x
    for _ in range(16):                          # run 2 chains through a
        q = {k: (rnd() if p is None else p) for k, p in ((k, rng.choice(pick)) for k in ("q_m", "q_l", "q_r", "q_4", "q_c"))}
        chain.append((prev, y, b.var(), w, q))
        prev = chain[-1][2]
    b.arith(chain)
    arith = b.fill_arithmetic(24)
    assignments = [{x: rnd(), y: rnd(), w: rnd(), flag: p & 1, **arith} for p in range(3)]
    assignments.append({x: 0, y: R - 1, w: 1, flag: 1, **arith})
    return b, assignments, [b.model(a) for a in assignments]


@functools.lru_cache(maxsize=None)
def cross_case(num_bits=255):
    """the same decomposition twice: as BITS + MAYBE_EQUAL, and with its bits as inputs and the 2 B rows as one ARITH run"""
    out = []
    rng = random.Random(25)
    values = [rng.randrange(R), R - 1, ((1 << num_bits) - 1) % R, (1 << 254) + 12345]
    for as_arith in (False, True):
        b = CM.Builder(1024)
        v = b.var(True)
        bit, acc = b.bits(v, num_bits, level=0, as_arith=as_arith)
        b.maybe_equal(acc[-1], v, level=1)
        arith = b.fill_arithmetic(26)
        assignments = []
        for val in values:
            a = {v: val, **arith}
            if as_arith:
                a.update({bv: (val >> k) & 1 for k, bv in enumerate(bit)})
            assignments.append(a)
        out.append((b, assignments, [b.model(a) for a in assignments]))
    return out


RANGE_MIN, RANGE_MAX = 1000, (1 << 64) - 5


@functools.lru_cache(maxsize=None)
def end_to_end_case():
    """a range check between 64-bit bounds (levels 0..3) beside a commitment: two 256-round fixed-base multiplications
    (level 0) and the addition of their results (level 1); n = 1024"""
    b = CM.Builder(1024)
    s1, s2, x = b.var(True), b.var(True), b.var(True)
    st = [b.var(True) for _ in range(4)]
    p1 = b.fixed_base(s1, 256, st[:2], level=0, table_seed=0x1234567)
    p2 = b.fixed_base(s2, 256, st[2:], level=0, table_seed=0x2345678)
    b.curve_add(p1, p2, level=1)
    out = b.range_check(RANGE_MIN, RANGE_MAX, x, level=0)
    arith = b.fill_arithmetic(27)
    rng = random.Random(27)

    def inputs(value):
        return {s1: rng.randrange(R), s2: rng.randrange(R), x: value % R, st[0]: 0, st[1]: 1, st[2]: 0, st[3]: 1, **arith}
    return b, inputs, out


def range_check_circuit(min_range, max_range):
    b = CM.Builder(1024)
    x = b.var(True)
    out = b.range_check(min_range, max_range, x)
    return b, x, out


@functools.lru_cache(maxsize=None)
def refusal_case():
    """a good table (ARITH, BITS 8, MAYBE_EQUAL, a range) and, beside it, rows that look like a gadget's but are wrong in ONE
    place; the good table never claims them"""
    b = CM.Builder(256)
    v, w = b.var(True), b.var(True)
    t = b.add(v, w, q_l=3, q_r=5, q_c=7, level=0)
    y, _ = b.decomposition(t, 8, level=1)
    b.equal(v, b.range(v, 2, level=0))
    decoys = {}

    def bits_like(name, spoil):
        r0 = b.row
        bit = [b.var() for _ in range(4)]
        acc = [b.var() for _ in range(4)]
        for k in range(4):
            b.gate(bit[k], bit[k], bit[k], q_m=1, q_o=R - 1)
            b.gate(bit[k], acc[k - 1] if k else 0, acc[k], q_l=1 << k, q_r=1, q_o=R - 1)
        spoil(r0)
        decoys[name] = r0

    def wrong_power(r0):
        b.sel["q_l"][r0 + 5] = 5                      # 2^2 expected
    bits_like("bits_q_l", wrong_power)

    def wrong_wire(r0):
        b.wires[2][r0 + 4] = b.var()                  # a != c on the boolean row of bit 2
    bits_like("bits_wire", wrong_wire)
    decoys["arith_q_o"] = b.gate(v, w, b.var(), q_l=1, q_r=1, q_o=1)
    r = b.gate(v, w, b.var(), q_l=1, q_r=1, q_o=R - 1)
    b.sel["q_arith"][r] = 0
    decoys["arith_off"] = r
    r = b.gate(v, w, b.var(), q_l=1, q_r=1, q_o=R - 1)        # a good ARITH row but for the widget selector beside q_arith
    b.sel["q_logic"][r] = 1
    decoys["arith_widget"] = r
    r0 = b.row
    u, z, yy = b.var(), b.var(), b.var()
    b.gate(v, w, u, q_l=1, q_r=R - 1, q_o=R - 1)
    b.gate(z, u, yy, q_m=R - 1, q_c=2, q_o=R - 1)     # q_c = 1 expected
    b.gate(yy, u, u, q_m=1)
    decoys["maybe_equal_q_c"] = r0
    arith = b.fill_arithmetic(28)
    rng = random.Random(28)
    return b, {v: rng.getrandbits(16), w: rng.getrandbits(4), **arith}, decoys


# ---------------------------------------------------------------------------------------------- every set-time rule, one decoy each
# What pm_plonk_key_set_gadgets checks on the rows a composed gadget claims.  On EVERY row: q_arith is not zero and the four
# widget selectors are zero.  Then, with the coefficients in the order q_m q_l q_r q_o q_c q_4:
#   ARITH, every row:              q_o = -1, c is a variable; nothing else
#   BITS, boolean row of bit k:    1 0 0 -1 0 0; a is a variable, b = a, c = a
#   BITS, sum row of bit k:        0 2^k 1 -1 0 0; c is a variable, a = the bit (a of the row before), and for k > 0
#                                  b = acc_(k-1) (c of the row two before); b of bit 0 is free: the start of the sum
#   MAYBE_EQUAL row 0 (u):         0 1 -1 -1 0 0; c is a variable
#   MAYBE_EQUAL row 1 (y):         -1 0 0 -1 1 0; a and c are variables, b = u
#   MAYBE_EQUAL row 2:             1 0 0 0 0 0; a = y, b = u
# d is never looked at, nor is c of the last MAYBE_EQUAL row.
COEFF_ORDER = ("q_m", "q_l", "q_r", "q_o", "q_c", "q_4")
_WIDGETS = ("q_range", "q_logic", "q_fixed_group_add", "q_variable_group_add")
DECOY_BITS = 2                                     # k = 0 and k > 0


def _wrong(x):
    return 2 if x % R == 1 else 1


@functools.lru_cache(maxsize=None)
def rule_decoys_case():
    """a good table (a glue row, two BITS, two MAYBE_EQUAL and two ARITH runs: the second of each kind sits at a non-zero
    offset of whatever is gathered for it) and, beside it, gadgets of DECOY_BITS bits, MAYBE_EQUALs and one-row ARITH runs that
    are wrong in ONE place of the list above; the good table never claims them.
    -> (builder, input assignment, {kind: {name: first row}}), an untouched "good" one of every kind among them"""
    b = CM.Builder(512)
    v, w, other = b.var(True), b.var(True), b.var(True)
    t = b.add(v, w, q_l=3, q_r=5, q_c=7, level=0)
    b.arith([(v, w, None, t, dict(q_m=2, q_l=3, q_r=5, q_4=11, q_c=7)), (w, v, None, None, dict(q_m=R - 1, q_c=1))], level=1)
    b.decomposition(t, 8, level=1)
    b.decomposition(w, 3, level=1)
    decoys = {"bits": {}, "maybe_equal": {}, "arith": {}}

    def no_var(r0, rows, row):
        """c of the row is no variable, and neither is any position of the gadget that names it"""
        x = b.wires[2][r0 + row]
        for j in range(4):
            for i in range(r0, r0 + rows):
                if b.wires[j][i] == x:
                    b.wires[j][i] = CM.NO_VAR

    def lay(kind):
        r0 = b.row
        if kind == "bits":
            bit, acc = [b.var() for _ in range(DECOY_BITS)], [b.var() for _ in range(DECOY_BITS)]
            for k in range(DECOY_BITS):
                b.gate(bit[k], bit[k], bit[k], q_m=1, q_o=R - 1)
                b.gate(bit[k], acc[k - 1] if k else v, acc[k], q_l=1 << k, q_r=1, q_o=R - 1)
        elif kind == "maybe_equal":
            u, z, y = b.var(), b.var(), b.var()
            b.gate(v, w, u, q_l=1, q_r=R - 1, q_o=R - 1)
            b.gate(z, u, y, q_m=R - 1, q_c=1, q_o=R - 1)
            b.gate(y, u, u, q_m=1)
        else:
            b.gate(v, w, b.var(), q_m=3, q_l=1, q_r=1, q_o=R - 1)
        return r0, b.row - r0

    def decoy(kind, name, spoil):
        r0, rows = lay(kind)
        before = ([list(x) for x in b.wires], {k: list(x) for k, x in b.sel.items()})
        spoil(r0, rows)
        assert name == "good" or before != ([list(x) for x in b.wires], {k: list(x) for k, x in b.sel.items()}), name
        assert name not in decoys[kind]
        decoys[kind][name] = r0

    def sel(key, row, value=None):
        return lambda r0, rows: b.sel[key].__setitem__(r0 + row, _wrong(b.sel[key][r0 + row]) if value is None else value)

    def wire(j, row, var=other):
        return lambda r0, rows: b.wires[j].__setitem__(r0 + row, var)

    for kind, rows in (("bits", 2 * DECOY_BITS), ("maybe_equal", 3), ("arith", 1)):
        decoy(kind, "good", lambda r0, rows: None)
        for row in range(rows):
            for q in (("q_o",) if kind == "arith" else COEFF_ORDER):      # ARITH: the other five are free
                if (kind, row, q) != ("maybe_equal", 2, "q_o"):
                    decoy(kind, f"row{row}_{q}", sel(q, row))
            decoy(kind, f"row{row}_no_arith", sel("q_arith", row, 0))
            decoy(kind, f"row{row}_widget", sel(_WIDGETS[row % 4], row, 1))
    decoy("maybe_equal", "row2_q_o", sel("q_o", 2, R - 1))               # 0 expected on this row, not -1
    decoy("bits", "row3_q_l_is_4", sel("q_l", 3, 4))                       # 2^1 expected, not the next power
    decoy("bits", "bool_b", wire(1, 2))
    decoy("bits", "bool_c", wire(2, 0))
    decoy("bits", "bool_no_var", lambda r0, rows: no_var(r0, rows, 2))    # a = b = c = a of the sum row: all no variable
    decoy("bits", "sum_bit_k0", wire(0, 1))
    decoy("bits", "sum_bit_k1", wire(0, 3))
    decoy("bits", "sum_link", wire(1, 3))
    decoy("bits", "sum_no_var_k0", lambda r0, rows: no_var(r0, rows, 1))
    decoy("bits", "sum_no_var_k1", lambda r0, rows: no_var(r0, rows, 3))
    decoy("maybe_equal", "no_var_u", lambda r0, rows: no_var(r0, rows, 0))
    decoy("maybe_equal", "no_var_z", wire(0, 1, CM.NO_VAR))
    decoy("maybe_equal", "no_var_y", lambda r0, rows: no_var(r0, rows, 1))
    decoy("maybe_equal", "row1_b", wire(1, 1))
    decoy("maybe_equal", "row2_a", wire(0, 2))
    decoy("maybe_equal", "row2_b", wire(1, 2))
    decoy("arith", "no_var", wire(2, 0, CM.NO_VAR))
    arith = b.fill_arithmetic(29)
    rng = random.Random(29)
    return b, {v: rng.getrandbits(16), w: rng.getrandbits(3), other: rng.randrange(R), **arith}, decoys
