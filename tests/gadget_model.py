"""Big-integer model of the four gadget definitions (include/plonk_mi355x.h, pm_plonk_gadget) and a small builder of
composer-form circuits that use them -- the reference of tests/test_gadgets_host.py and tests/test_gpu_gadgets.py.  Plain
Python integers throughout; nothing here touches the library's arithmetic."""
import random

import numpy as np

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
EDWARDS_D = (-(10240 * pow(10241, -1, R))) % R
NO_VAR = 0xFFFFFFFF
IDENTITY = (0, 1)
TOO_WIDE, SCALAR_TOO_LONG, DEGENERATE = "too_wide", "scalar_too_long", "degenerate"


def jubjub_add(p, q):
    (x1, y1), (x2, y2) = p, q
    k = EDWARDS_D * x1 % R * x2 % R * y1 % R * y2 % R
    return ((x1 * y2 + y1 * x2) * pow(1 + k, -1, R) % R, (y1 * y2 + x1 * x2) * pow(1 - k, -1, R) % R)


def on_curve(p):
    x, y = p
    return (-x * x + y * y - 1 - EDWARDS_D * x * x % R * y * y) % R == 0


# ------------------------------------------------------------------------------------------ the definitions
def naf_digits(s: int, rounds: int):
    """-> (e_0 .. e_(rounds-1), too_long): the width-2 non-adjacent form of s, least significant first."""
    e, k = [], s
    while k:
        if k & 1:
            d = 2 - k % 4
            k -= d
        else:
            d = 0
        e.append(d)
        k //= 2
    too_long = len(e) > rounds
    return (e + [0] * rounds)[:rounds], too_long


def range_model(v: int, m: int):
    """-> (acc_0 .. acc_4m, reason): accumulators of the low 8m bits of v, most significant quad first."""
    acc = [0]
    for k in range(4 * m):
        acc.append(4 * acc[-1] + ((v >> (2 * (4 * m - 1 - k))) & 3))
    return acc, (TOO_WIDE if v >> (8 * m) else None)


def logic_model(x: int, y: int, quads: int, xor: bool):
    """-> (A, B, D accumulators [quads + 1], products [quads], reason)."""
    A, Bc, D, prod = [0], [0], [0], []
    for k in range(quads):
        qx, qy = (x >> (2 * (quads - 1 - k))) & 3, (y >> (2 * (quads - 1 - k))) & 3
        A.append(4 * A[-1] + qx)
        Bc.append(4 * Bc[-1] + qy)
        D.append(4 * D[-1] + ((qx ^ qy) if xor else (qx & qy)))
        prod.append(qx * qy)
    return A, Bc, D, prod, (TOO_WIDE if (x >> (2 * quads)) or (y >> (2 * quads)) else None)


def fixed_base_model(s: int, rounds: int, start, table):
    """table[k] = (x_b, y_b) of row k.  -> (points [rounds + 1], c [rounds], d [rounds + 1], reason), sequentially as defined."""
    e, too_long = naf_digits(s, rounds)
    pts, c, d = [start], [], [0]
    for k in range(rounds):
        bit = e[rounds - 1 - k]
        xb, yb = table[k]
        c.append(bit * xb * yb % R)
        pts.append(jubjub_add(pts[-1], (bit * xb % R, (bit * bit * (yb - 1) + 1) % R)))
        d.append((2 * d[-1] + bit) % R)
    return pts, c, d, (SCALAR_TOO_LONG if too_long else None)


def curve_add_model(p, q):
    """-> (x3, y3, x1 y2, reason)"""
    (x1, y1), (x2, y2) = p, q
    k = EDWARDS_D * x1 % R * x2 % R * y1 % R * y2 % R
    if (1 + k) % R == 0 or (1 - k) % R == 0:
        return 0, 0, x1 * y2 % R, DEGENERATE
    x3, y3 = jubjub_add(p, q)
    return x3, y3, x1 * y2 % R, None


# ------------------------------------------------------------------------------------------ the widget identities, restated
def _delta(f):
    return f * (f - 1) * (f - 2) * (f - 3) % R


def range_summands(row, d_next):
    a, b, c, d = row
    return [_delta(c - 4 * d), _delta(b - 4 * c), _delta(a - 4 * b), _delta(d_next - 4 * a)]


def logic_summands(row, nxt, q_c):
    a, b, c, d = row
    qa, qb, qd = (nxt[0] - 4 * a) % R, (nxt[1] - 4 * b) % R, (nxt[3] - 4 * d) % R
    s = qa + qb
    f = c * (c * (4 * c - 18 * s + 81) + 18 * (qa * qa + qb * qb) - 81 * s + 83) % R
    e = 3 * (s + qd) - 2 * f
    return [_delta(qa), _delta(qb), _delta(qd), (c - qa * qb) % R, (q_c * (9 * qd - 3 * s) + e) % R]


def fixed_summands(row, nxt, table_point):
    a, b, c, d = row
    xb, yb = table_point
    bit = (nxt[3] - 2 * d) % R
    ya, xa = (bit * bit * (yb - 1) + 1) % R, xb * bit % R
    dxy = c * a % R * b % R * EDWARDS_D % R
    return [bit * (bit - 1) * (bit + 1) % R, (bit * xb * yb - c) % R, (nxt[0] + nxt[0] * dxy - (a * ya + b * xa)) % R,
            (nxt[1] - nxt[1] * dxy - (b * ya + a * xa)) % R]


def var_summands(row, nxt):
    a, b, c, d = row
    an, bn, dn = nxt[0], nxt[1], nxt[3]
    dd = dn * (b * c) % R * EDWARDS_D % R
    return [(a * d - dn) % R, (dn + b * c - (an + an * dd)) % R, (b * d + a * c - (bn - bn * dd)) % R]


# ------------------------------------------------------------------------------------------ points
def _sqrt(a):
    a %= R
    if a == 0:
        return 0
    if pow(a, (R - 1) // 2, R) != 1:
        return None
    s, q = 32, (R - 1) >> 32
    z = pow(7, q, R)
    m, c, t, r = s, z, pow(a, q, R), pow(a, (q + 1) // 2, R)
    while t != 1:
        i, t2 = 0, t
        while t2 != 1:
            t2 = t2 * t2 % R
            i += 1
        b = pow(c, 1 << (m - i - 1), R)
        m, c = i, b * b % R
        t, r = t * c % R, r * b % R
    return r


def curve_point(seed: int):
    y = seed % R
    while True:
        x = _sqrt((y * y - 1) * pow(1 + EDWARDS_D * y * y, -1, R))
        if x:
            assert on_curve((x, y))
            return x, y
        y += 1


_TABLES: dict = {}


def base_table(rounds: int, seed: int = 0x1234567):
    """[2^j B for j < rounds] by repeated jubjub_add."""
    key = seed
    if key not in _TABLES:
        _TABLES[key] = [curve_point(seed)]
    t = _TABLES[key]
    while len(t) < rounds:
        t.append(jubjub_add(t[-1], t[-1]))
    return t[:rounds]


# ------------------------------------------------------------------------------------------ the builder
SELECTORS = ("q_m", "q_l", "q_r", "q_o", "q_c", "q_4", "q_arith", "q_range", "q_logic", "q_fixed_group_add",
             "q_variable_group_add")


class Builder:
    """Lays out a composer-form circuit of n rows: selectors, wire_vars, the gadget records, the INPUT variables (what a
    caller provides) and, per assignment, the model's value of every variable.  Variable 0 is the zero variable; the
    accumulators a definition starts at zero name it.  Gadgets are appended in the order of the calls; ``gadgets`` holds
    (kind, level, first_row, count, param, in_vars) tuples, which the caller turns into ``Gadget`` records."""

    def __init__(self, n: int):
        self.n, self.row = n, 0
        self.sel = {k: [0] * n for k in SELECTORS}
        self.wires = [[NO_VAR] * n for _ in range(4)]
        self.num_vars = 1
        self.gadgets = []
        self.steps = []            # closures (values: list) -> reason or None, in level order of evaluation
        self.inputs = set([0])

    def var(self, is_input=False):
        v = self.num_vars
        self.num_vars += 1
        if is_input:
            self.inputs.add(v)
        return v

    def _rows(self, count):
        r = self.row
        self.row += count
        assert self.row <= self.n, "circuit too small"
        return r

    def _put(self, row, ids):
        for j, v in enumerate(ids):
            if v is not None:
                self.wires[j][row] = v

    def range(self, value_var, m, level=0):
        r0 = self._rows(m + 1)
        acc = [0] + [self.var() for _ in range(4 * m)]
        for i in range(m):
            self.sel["q_range"][r0 + i] = 1
            self._put(r0 + i, (acc[4 * i + 3], acc[4 * i + 2], acc[4 * i + 1], acc[4 * i]))
        self._put(r0 + m, (None, None, None, acc[4 * m]))
        idx = len(self.gadgets)
        self.gadgets.append(("range", level, r0, m, 0, (value_var,)))

        def step(val):
            a, reason = range_model(val[value_var], m)
            for v, x in zip(acc, a):
                val[v] = x % R
            return reason
        self.steps.append((level, idx, step))
        return acc[4 * m]

    def logic(self, x_var, y_var, quads, xor=False, level=0):
        r0 = self._rows(quads + 1)
        A = [0] + [self.var() for _ in range(quads)]
        Bc = [0] + [self.var() for _ in range(quads)]
        D = [0] + [self.var() for _ in range(quads)]
        P = [self.var() for _ in range(quads)]
        for k in range(quads):
            self.sel["q_logic"][r0 + k] = 1
            self.sel["q_c"][r0 + k] = R - 1 if xor else 1
            self._put(r0 + k, (A[k], Bc[k], P[k], D[k]))
        self._put(r0 + quads, (A[quads], Bc[quads], None, D[quads]))
        idx = len(self.gadgets)
        self.gadgets.append(("logic", level, r0, quads, 1 if xor else 0, (x_var, y_var)))

        def step(val):
            a, b, d, p, reason = logic_model(val[x_var], val[y_var], quads, xor)
            for ids, xs in ((A, a), (Bc, b), (D, d), (P, p)):
                for v, x in zip(ids, xs):
                    val[v] = x % R
            return reason
        self.steps.append((level, idx, step))
        return D[quads]

    def fixed_base(self, scalar_var, rounds, start_vars, level=0, table_seed=0x1234567):
        """start_vars: the two variables of the start point (inputs, or another gadget's outputs).  -> (x var, y var) of the result"""
        r0 = self._rows(rounds + 1)
        base = base_table(rounds, table_seed)
        table = [base[rounds - 1 - k] for k in range(rounds)]
        X = [start_vars[0]] + [self.var() for _ in range(rounds)]
        Y = [start_vars[1]] + [self.var() for _ in range(rounds)]
        Cc = [self.var() for _ in range(rounds)]
        Dd = [0] + [self.var() for _ in range(rounds)]
        for k in range(rounds):
            xb, yb = table[k]
            self.sel["q_fixed_group_add"][r0 + k] = 1
            self.sel["q_l"][r0 + k], self.sel["q_r"][r0 + k], self.sel["q_c"][r0 + k] = xb, yb, xb * yb % R
            self._put(r0 + k, (X[k], Y[k], Cc[k], Dd[k]))
        self._put(r0 + rounds, (X[rounds], Y[rounds], None, Dd[rounds]))
        idx = len(self.gadgets)
        self.gadgets.append(("fixed_base", level, r0, rounds, 0, (scalar_var,)))

        def step(val):
            pts, c, d, reason = fixed_base_model(val[scalar_var], rounds, (val[X[0]], val[Y[0]]), table)
            for k in range(1, rounds + 1):
                val[X[k]], val[Y[k]] = pts[k]
            for v, x in zip(Cc, c):
                val[v] = x
            for v, x in zip(Dd, d):
                val[v] = x
            return reason
        self.steps.append((level, idx, step))
        return X[rounds], Y[rounds]

    def curve_add(self, p_vars, q_vars, level=0):
        r0 = self._rows(2)
        self.sel["q_variable_group_add"][r0] = 1
        x3, y3, xy = self.var(), self.var(), self.var()
        self._put(r0, (p_vars[0], p_vars[1], q_vars[0], q_vars[1]))
        self._put(r0 + 1, (x3, y3, None, xy))
        idx = len(self.gadgets)
        self.gadgets.append(("curve_add", level, r0, 0, 0, ()))

        def step(val):
            val[x3], val[y3], val[xy], reason = curve_add_model((val[p_vars[0]], val[p_vars[1]]), (val[q_vars[0]], val[q_vars[1]]))
            return reason
        self.steps.append((level, idx, step))
        return x3, y3

    def equal(self, u, v):
        """one arithmetic row: u - v = 0"""
        r0 = self._rows(1)
        self.sel["q_arith"][r0], self.sel["q_l"][r0], self.sel["q_r"][r0] = 1, 1, R - 1
        self._put(r0, (u, v, None, None))

    def fill_arithmetic(self, seed=1):
        """the rest of the rows: a product chain a b - c = 0 whose variables are inputs (-> the values they take)"""
        rng = random.Random(seed)
        vals = {}
        prev = self.var(True)
        vals[prev] = rng.randrange(R)
        while self.row < self.n:
            r0 = self._rows(1)
            b, c = self.var(True), self.var(True)
            vals[b] = rng.randrange(R)
            vals[c] = vals[prev] * vals[b] % R
            self.sel["q_arith"][r0], self.sel["q_m"][r0], self.sel["q_o"][r0] = 1, 1, R - 1
            self._put(r0, (prev, b, c, None))
            prev = c
        return vals

    # ---- what the tests take
    def circuit(self):
        import plonk_prototype_amd as pa
        from plonk_prototype_amd.field import fr_vec_to_limbs
        sel = {k: fr_vec_to_limbs(v) for k, v in self.sel.items()}
        return pa.Circuit(wire_vars=np.array(self.wires, dtype=np.uint32), num_vars=self.num_vars, **sel)

    def gadget_records(self):
        import plonk_prototype_amd as pa
        out = []
        for kind, level, r0, count, param, iv in self.gadgets:
            if kind == "range":
                out.append(pa.Gadget.range(r0, count, iv[0], level=level))
            elif kind == "logic":
                out.append(pa.Gadget.logic(r0, count, iv[0], iv[1], xor=bool(param), level=level))
            elif kind == "fixed_base":
                out.append(pa.Gadget.fixed_base(r0, count, iv[0], level=level))
            else:
                out.append(pa.Gadget.curve_add(r0, level=level))
        return out

    def model(self, input_values: dict):
        """input_values: {input variable: int}.  -> (inputs-only list, model-filled list, {gadget index: reason})"""
        val = [0] * self.num_vars
        for v, x in input_values.items():
            assert v in self.inputs, v
            val[v] = x % R
        only = list(val)
        reasons = {}
        for _, idx, step in sorted(self.steps, key=lambda t: (t[0], t[1])):
            reason = step(val)
            if reason:
                reasons[idx] = reason
        return only, val, reasons

    def rows(self, val):
        """the four wire values of every row under an assignment"""
        return [[0 if self.wires[j][i] == NO_VAR else val[self.wires[j][i]] for j in range(4)] for i in range(self.n)]


def to_limbs(vals) -> np.ndarray:
    from plonk_prototype_amd.field import fr_vec_to_limbs
    return fr_vec_to_limbs(vals)
