"""Limb-exact big-integer model of the device field arithmetic (csrc/fields.hip.h), of the binary-GCD inversion
(csrc/field_inv.hip.h), of the butterfly networks built on it (dft8 / dft4, csrc/ntt_kernels.hip.h) and of the XYZZ group
law (csrc/ec.hip.h) -- plain Python, no GPU, no library.

Every routine walks the device code limb for limb: the same 32-bit limb sums, the same 64-bit column accumulators, the
same digits and shifts, for both parameter sets (FR: W = 29, N = 9; FP: W = 28, N = 14).  Python integers do not wrap, so
the model can see what the device cannot: whenever a 32-bit or 64-bit intermediate would wrap, whenever a routine is
handed an operand outside its documented precondition, and whenever a result leaves its documented class, a line is
appended to VIOLATIONS (the computation then goes on with the wrapped value, as the device would).  A walk with the
worst members of the classes the call sites document must leave VIOLATIONS empty.

Classes are written (B, V) as in the device comments: limbs < B * 2^W, value < V * m; "+" adds the slack a parallel carry
step (fe_norm) leaves, 2^(32 - W) ("++": twice that, the sum of two such operands).  An element is a list of N integers, least significant limb first.
"""
import functools
import random

from . import bigint_oracle as B

M32 = (1 << 32) - 1
M64 = (1 << 64) - 1

VIOLATIONS = []


def flag(msg):
    VIOLATIONS.append(msg)


class Field:
    def __init__(self, name, W, N, NS, mod):
        self.name, self.W, self.N, self.NS, self.mod = name, W, N, NS, mod
        self.MASK = (1 << W) - 1
        self.M = [(mod >> (W * i)) & self.MASK for i in range(N)]
        self.RADIX = 1 << (W * N)                                   # the device Montgomery radix R'
        self.RINV = pow(self.RADIX, -1, mod)
        self.NINV = (-pow(mod, -1, 1 << W)) % (1 << W)
        self.SLACK = 1 << (32 - W)

    def __repr__(self):
        return self.name


FR = Field("fr", 29, 9, 8, B.R_MOD)
FP = Field("fp", 28, 14, 12, B.P_MOD)


def limbs_of(f, v):
    """normalised limbs of v (the top limb keeps the rest)"""
    r = [(v >> (f.W * i)) & f.MASK for i in range(f.N)]
    r[f.N - 1] = v >> (f.W * (f.N - 1))
    return r


def value_of(f, l):
    return sum(x << (f.W * i) for i, x in enumerate(l))


def _u32(x, what):
    if not 0 <= x <= M32:
        flag(f"u32 wrap in {what}: {x:#x}")
    return x & M32


def _u64(x, what):
    if not 0 <= x <= M64:
        flag(f"u64 wrap in {what}: {x:#x}")
    return x & M64


def _i32(x, what):
    """an int32_t value: wraps to two's complement"""
    if not -(1 << 31) <= x < 1 << 31:
        flag(f"i32 wrap in {what}: {x:#x}")
        return ((x + (1 << 31)) & M32) - (1 << 31)
    return x


def _i64(x, what):
    """a long long value"""
    if not -(1 << 63) <= x < 1 << 63:
        flag(f"i64 wrap in {what}: {x:#x}")
        return ((x + (1 << 63)) & M64) - (1 << 63)
    return x


def in_class(f, x, Bl, V, plus=False):
    """limbs < Bl * 2^W (+ slack), value < V * m"""
    lim = Bl * (1 << f.W) + f.SLACK * int(plus)                     # plus = 2: the sum of two "+" operands
    return all(0 <= v < lim for v in x) and value_of(f, x) < V * f.mod


def expect(f, x, Bl, V, plus, what):
    """an annotated intermediate: record a violation if it is outside its class"""
    if not in_class(f, x, Bl, V, plus):
        flag(f"{what}: outside ({Bl}{'+' * int(plus)}, <{V}): max limb {max(x):#x}, value / m = {value_of(f, x) / f.mod:.3f}")
    return x


# ------------------------------------------------------------------ compile-time constants (struct Consts)
def k_mod(f, k):
    r, c = [0] * f.N, 0
    for i in range(f.N):
        t = f.M[i] * k + c
        r[i] = _u32(t, "k_mod top") if i == f.N - 1 else t & f.MASK
        c = t >> f.W
    return r


def sub_bias(f, K, E):
    r = k_mod(f, K)
    for i in range(f.N - 1):
        r[i] += 1 << (f.W + E)
        r[i + 1] -= 1 << E
    for i in range(f.N):
        if not 0 <= r[i] <= M32:
            flag(f"sub_bias<{K},{E}> limb {i} out of u32")
    return r


def rbar(f):
    r = [f.MASK - m for m in f.M]
    r[0] += 1
    return r


def fe_pow2(f, e):
    """Consts::pow2_mod: compile-time double-and-reduce"""
    return list(_pow2(f, e))


@functools.lru_cache(maxsize=None)
def _pow2(f, e):
    N, W, MASK = f.N, f.W, f.MASK
    x = [0] * N
    x[0] = 1
    for _ in range(e):
        c = 0
        for i in range(N):
            t = _u32(x[i] << 1, "pow2 shift") | c
            c = 0 if i == N - 1 else t >> W
            x[i] = t if i == N - 1 else t & MASK
        ge = True
        for i in range(N - 1, -1, -1):
            if x[i] != f.M[i]:
                ge = x[i] > f.M[i]
                break
        if ge:
            bw = 0
            for i in range(N):
                t = (x[i] - f.M[i] - bw) & M32
                bw = 0 if i == N - 1 else (t >> W) & 1
                x[i] = t if i == N - 1 else t & MASK
    return tuple(x)


def fe_one(f):
    return fe_pow2(f, f.W * f.N)


# ------------------------------------------------------------------ trivial ops
def fe_zero(f):
    return [0] * f.N


def fe_add(f, a, b):
    return [_u32(x + y, "fe_add") for x, y in zip(a, b)]


def fe_sub(f, K, E, a, b):
    """a - b + K m.  Precondition: b limbs <= 2^(W+E) - 2^E, b's top limb <= top(K m) - 2^E."""
    bias = sub_bias(f, K, E)
    lim = (1 << (f.W + E)) - (1 << E)
    if any(v > lim for v in b[:-1]) or b[-1] > bias[-1]:
        flag(f"fe_sub<{K},{E}> precondition: subtrahend limbs {max(b[:-1]):#x} (limit {lim:#x}), top {b[-1]:#x} (limit {bias[-1]:#x})")
    r = []
    for i in range(f.N):
        t = bias[i] - b[i]
        if t < 0:
            flag(f"fe_sub<{K},{E}> limb {i} goes negative")
        r.append(_u32(a[i] + (t & M32), "fe_sub sum") if t >= 0 else (a[i] + t) & M32)
    return r


def fe_norm(f, a):
    N, W, MASK = f.N, f.W, f.MASK
    r = [a[0] & MASK]
    for i in range(1, N - 1):
        r.append((a[i] & MASK) + (a[i - 1] >> W))
    r.append(_u32(a[N - 1] + (a[N - 2] >> W), "fe_norm top"))
    if any(v >= (1 << W) + f.SLACK for v in r[:-1]):
        flag("fe_norm result class")
    return r


def fe_norm_full(f, a):
    r, c = [], 0
    for i in range(f.N - 1):
        t = _u32(a[i] + c, "fe_norm_full")
        r.append(t & f.MASK)
        c = t >> f.W
    r.append(_u32(a[f.N - 1] + c, "fe_norm_full top"))
    return r


# ------------------------------------------------------------------ Montgomery products
def _mont_cols(f, K, prod, what):
    """fe_mont_cols: prod(k) lists (chain, x, y) limb products of column k.  Returns K results."""
    N, W, MASK = f.N, f.W, f.MASK
    q = [[0] * N for _ in range(K)]
    acc = [0] * K
    r = [[0] * N for _ in range(K)]
    total = [0] * K                                                 # the integer each chain reduces

    def mac(c, x, y):
        acc[c] = _u64(acc[c] + x * y, what + " column")

    for k in range(2 * N - 1):
        for c, x, y in prod(k):
            mac(c, x, y)
            total[c] += (x * y) << (W * k)
        if k < N:
            for i in range(k):
                for c in range(K):
                    mac(c, q[c][i], f.M[k - i])
            for c in range(K):
                if f.M[0] == 1:
                    q[c][k] = (-(acc[c] & M32)) & MASK
                    acc[c] = _u64(acc[c] + MASK, what + " digit")
                else:
                    q[c][k] = (((acc[c] & M32) * f.NINV) & M32) & MASK
                    mac(c, q[c][k], f.M[0])
                acc[c] >>= W
        else:
            for i in range(k - N + 1, N):
                for c in range(K):
                    mac(c, q[c][i], f.M[k - i])
            for c in range(K):
                r[c][k - N] = acc[c] & MASK
                acc[c] >>= W
    for c in range(K):
        r[c][N - 1] = _u32(acc[c], what + " top limb")
        # documented result: limbs < 2^W, value < T / R' + m, congruent to T / R'
        v = value_of(f, r[c])
        if any(x >> W for x in r[c]) or v * f.RADIX >= total[c] + f.mod * f.RADIX or (v * f.RADIX - total[c]) % f.mod:
            flag(what + " result class")
    return r


def _col_bound(f, pairs, what):
    """N sum(max a * max b) + (N - 1) 2^(2W) + 2^(64-W) < 2^64, the documented operand bound of the product routines"""
    s = sum(max(a) * max(b) for a, b in pairs)
    if f.N * s + (f.N - 1) * (1 << (2 * f.W)) + (1 << (64 - f.W)) >= 1 << 64:
        flag(what + " precondition: column bound")


def _mul_terms(f, c, a, b, k):
    return [(c, a[i], b[k - i]) for i in range(f.N) if 0 <= k - i < f.N]


def _sqr_terms(f, c, a, d, k):
    return [(c, a[i], a[i] if i == k - i else d[k - i]) for i in range(f.N) if 0 <= k - i < f.N and i <= k - i]


def _doubled(a):
    return [_u32(x << 1, "fe_sqr doubled copy") for x in a]


def fe_mul(f, a, b):
    _col_bound(f, [(a, b)], "fe_mul")
    return _mont_cols(f, 1, lambda k: _mul_terms(f, 0, a, b, k), "fe_mul")[0]


def fe_mul_limb(f, a, b0):
    if b0 >> f.W:
        flag("fe_mul_limb precondition: b0 >= 2^W")
    _col_bound(f, [(a, [b0])], "fe_mul_limb")
    return _mont_cols(f, 1, lambda k: [(0, a[k], b0)] if k < f.N else [], "fe_mul_limb")[0]


def fe_sqr(f, a):
    _col_bound(f, [(a, a)], "fe_sqr")
    d = _doubled(a)
    return _mont_cols(f, 1, lambda k: _sqr_terms(f, 0, a, d, k), "fe_sqr")[0]


def fe_mul2(f, a0, b0, a1, b1):
    _col_bound(f, [(a0, b0)], "fe_mul2")
    _col_bound(f, [(a1, b1)], "fe_mul2")
    return _mont_cols(f, 2, lambda k: _mul_terms(f, 0, a0, b0, k) + _mul_terms(f, 1, a1, b1, k), "fe_mul2")


def fe_mul3(f, a0, b0, a1, b1, a2, b2):
    for a, b in ((a0, b0), (a1, b1), (a2, b2)):
        _col_bound(f, [(a, b)], "fe_mul3")
    return _mont_cols(f, 3, lambda k: _mul_terms(f, 0, a0, b0, k) + _mul_terms(f, 1, a1, b1, k) + _mul_terms(f, 2, a2, b2, k),
                      "fe_mul3")


def fe_mma2(f, a0, b0, c0, d0, a1, b1):
    """r0 = (a0 b0 + c0 d0) / R', r1 = a1 b1 / R'"""
    _col_bound(f, [(a0, b0), (c0, d0)], "fe_mma2")
    _col_bound(f, [(a1, b1)], "fe_mma2")
    return _mont_cols(f, 2, lambda k: _mul_terms(f, 0, a0, b0, k) + _mul_terms(f, 1, a1, b1, k) + _mul_terms(f, 0, c0, d0, k),
                      "fe_mma2")


def fe_sqr2(f, a0, a1):
    _col_bound(f, [(a0, a0)], "fe_sqr2")
    _col_bound(f, [(a1, a1)], "fe_sqr2")
    d0, d1 = _doubled(a0), _doubled(a1)
    return _mont_cols(f, 2, lambda k: _sqr_terms(f, 0, a0, d0, k) + _sqr_terms(f, 1, a1, d1, k), "fe_sqr2")


# ---- fe_mul_split: data x split constant (Fr only)
R_MOD, W, N = B.R_MOD, FR.W, FR.N
MASK, M, RADIX = FR.MASK, FR.M, FR.RADIX


def limbs(v):
    return [(v >> (W * i)) & MASK for i in range(N)]


def value(l):
    return sum(x << (W * i) for i, x in enumerate(l))


def rows_of(w_mont, G, D):
    """row_j = w * 2^(W (jG + D - N)) mod r, canonical limbs (what step4_tw_kernel stores)"""
    groups = (N + G - 1) // G
    out = []
    for j in range(groups):
        e = W * (j * G + D - N)
        f = pow(2, e, R_MOD) if e >= 0 else pow(pow(2, -e, R_MOD), -1, R_MOD)
        out.append(limbs(w_mont * f % R_MOD))
    return out


def mul_split(x, rows, G, D):
    """The device routine, limb for limb.  Returns (result limbs, largest column value seen, products issued)."""
    assert M[0] == 1
    acc, peak, macs = 0, 0, 0
    q, r = [0] * D, [0] * N
    for k in range(D + N - 1):
        for i in range(N):
            b = k - i % G
            if 0 <= b < N:
                acc += x[i] * rows[i // G][b]
                macs += 1
                peak = max(peak, acc)
        for i in range(D):
            l = k - i
            if 1 <= l < N:
                acc += q[i] * M[l]
                macs += 1
                peak = max(peak, acc)
        if k < D:
            q[k] = (-acc) & MASK
            assert (acc + q[k]) >> W == (acc + MASK) >> W     # the carry does not wait for q
            acc += MASK
            peak = max(peak, acc)
        else:
            r[k - D] = acc & MASK
        acc >>= W
    r[N - 1] = acc
    return r, peak, macs


def fe_mul_split(x, rows, G, D):
    """mul_split with the violations recorded: column overflow, data limbs >= 6 * 2^W, result outside (1, <2)"""
    if max(x) >= 6 << W:
        flag("fe_mul_split precondition: data limbs")
    r, peak, _ = mul_split(x, rows, G, D)
    if peak > M64:
        flag("u64 wrap in fe_mul_split column")
    if any(v >> W for v in r) or value(r) >= 2 * R_MOD:
        flag("fe_mul_split result class")
    return [v & M32 for v in r]


# ------------------------------------------------------------------ cheap reduction, boundary
def fe_reduce_weak(f, x):
    """x (limbs < 2^32, value < 2^(W N)) -> normalised limbs, same residue, value < m + m / 2^16 (Fr) or m + m / 2^5 (Fp)"""
    N, W, MASK = f.N, f.W, f.MASK
    if value_of(f, x) >= f.RADIX:
        flag("fe_reduce_weak precondition: value >= 2^(W N)")
    RB = rbar(f)
    MAGIC = (1 << 52) // (f.M[N - 1] + 1)
    top = _u32(x[N - 1] + (x[N - 2] >> W), "fe_reduce_weak top")
    q = (_u64(top * MAGIC, "fe_reduce_weak magic") >> 52) & M32
    r, acc = [], 0
    for i in range(N):
        acc = _u64(acc + q * RB[i], "fe_reduce_weak")
        acc = _u64(acc + x[i], "fe_reduce_weak")
        r.append(acc & MASK)
        acc >>= W
    v = value_of(f, r)
    if (v - value_of(f, x)) % f.mod or acc != q:        # x + q (R' - m) = (x - q m) + q R': the dropped carry is q exactly
        flag("fe_reduce_weak result: residue")
    if v >= f.mod + (f.mod >> (16 if f is FR else 5)):
        flag(f"fe_reduce_weak result: value / m = {v / f.mod:.6f}")
    return r


def fe_unpack(f, s):
    """saturated canonical (NS x 32 bit) -> radix 2^W"""
    r = []
    for i in range(f.N):
        lo = i * f.W
        j, sh = lo // 32, lo % 32
        x = 0
        if j < f.NS:
            x = s[j] >> sh
        if j + 1 < f.NS and sh + f.W > 32:
            x |= (s[j + 1] << (32 - sh)) & M32
        r.append(x & f.MASK)
    return r


def fe_pack_raw(f, a):
    s = []
    for j in range(f.NS):
        lo, x = 32 * j, 0
        for i in range(f.N):
            l0 = i * f.W
            if l0 < lo + 32 and l0 + 32 > lo:
                x |= (a[i] << (l0 - lo)) & M32 if l0 >= lo else a[i] >> (lo - l0)
        s.append(x)
    return s


def fe_canon_pack(f, a):
    """value < 2m (limbs < 2^32) -> canonical saturated limbs"""
    N, W = f.N, f.W
    if value_of(f, a) >= 2 * f.mod:
        flag("fe_canon_pack precondition: value >= 2m")
    x = fe_norm_full(f, a)
    d, c = [], 0
    for i in range(N - 1):
        t = x[i] - f.M[i] + c
        d.append(t & f.MASK)
        c = t >> W                                                   # arithmetic shift: 0 or -1
    if x[N - 1] >> 31:
        flag("fe_canon_pack: top limb does not fit int32")
    top = x[N - 1] - f.M[N - 1] + c
    d.append(top & M32)
    s = fe_pack_raw(f, x if top < 0 else d)
    if sum(w << (32 * j) for j, w in enumerate(s)) != value_of(f, a) % f.mod:
        flag("fe_canon_pack result: not canonical")
    return s


# ------------------------------------------------------------------ inversion (csrc/field_inv.hip.h)
def fr_shl5(t):
    """poly_common.hip.h: value * 2^5 of a normalised Fr value < 2r -> limbs normalised, value < 64 r"""
    f = FR
    expect(f, t, 1, 2, False, "fr_shl5 in")
    r = [(t[0] << 5) & f.MASK]
    for i in range(1, 8):
        r.append(((t[i] << 5) & f.MASK) | (t[i - 1] >> 24))
    r.append(_u32(t[8] << 5, "fr_shl5 top") | (t[7] >> 24))
    if value_of(f, r) != value_of(f, t) << 5:
        flag("fr_shl5 result: value")
    return r


def canon_limb_max(f):
    """the largest limb fe_canon_limbs / fe_canon_pack admit: a carry < 2^(32-W) on top of it still fits 32 bits"""
    return M32 - f.SLACK


def fe_canon_limbs(f, a):
    """value < 2m, limbs < 2^32 - 2^(32-W) (the carry of fe_norm_full must fit) -> the canonical representative, limbs < 2^W"""
    N, W = f.N, f.W
    if value_of(f, a) >= 2 * f.mod:
        flag("fe_canon_limbs precondition: value >= 2m")
    if any(not 0 <= v <= canon_limb_max(f) for v in a):
        flag(f"fe_canon_limbs precondition: limb {max(a):#x} >= 2^32 - 2^(32-W)")
    x = fe_norm_full(f, a)
    d, c = [], 0
    for i in range(N - 1):
        t = _i32(_i32(x[i], "fe_canon_limbs limb as int32") - f.M[i] + c, "fe_canon_limbs borrow chain")
        d.append(t & f.MASK)
        c = t >> W                                                   # arithmetic shift: 0 or -1
    top = _i32(_i32(x[N - 1], "fe_canon_limbs top limb as int32") - f.M[N - 1] + c, "fe_canon_limbs top")
    d.append(top & M32)
    r = x if top < 0 else d
    if r != limbs_of(f, value_of(f, a) % f.mod):
        flag("fe_canon_limbs result: not canonical")
    return r


def inv_rounds(f):
    """ROUNDS = ceil((2 bits(m) - 1) / W)"""
    return (2 * f.mod.bit_length() - 1 + f.W - 1) // f.W


def _signed_value(f, l):
    return sum(x << (f.W * i) for i, x in enumerate(l))             # the top limb carries the sign


def fe_inv_int(f, y, trace=None):
    """y canonical limbs -> v >= 0 with v y = 1 (mod m) as plain integers, limbs < 2^W, value < 64 m; 0 -> 0.

    The lane runs until its own a is zero: a further round leaves b and v limb for limb as they are (the low limb of 2^W v is
    zero, so the multiple of m that clears it is zero), hence the device result does not depend on when the wave's vote lets
    the lane go.  trace, a dict, receives "rounds" (rounds run with a != 0), "v_rounds" (the last round that changed v: the
    round in which a = b = 1 turns a into 0 does not), "steps" (per round: a row negated, b row negated, exact path taken) and
    "max_u", "max_v" (the largest |u|, |v| after any round, as integers: divide by f.mod)."""
    N, W, MASK = f.N, f.W, f.MASK
    S = 64 - 2 * W
    assert N >= 3 and W <= 30 and S >= 2
    expect(f, y, 1, 1, False, "fe_inv_int in (canonical limbs)")
    a, b = list(y), list(f.M)
    u, v = [1] + [0] * (N - 1), [0] * N
    rounds, v_rounds, steps, max_u, max_v = 0, 0, [], 1, 0
    for _ in range(inv_rounds(f)):
        if not any(a):
            break
        rounds += 1
        # ---- approximations: low W bits | top W + 2 bits of max(a, b)
        a2 = a1 = a0 = b2 = b1 = b0 = 0
        found = False
        for i in range(N - 1, 1, -1):
            nz = (a[i] | b[i]) != 0
            if nz and not found:
                a2, a1, a0, b2, b1, b0 = a[i], a[i - 1], a[i - 2], b[i], b[i - 1], b[i - 2]
            found = found or nz
        above = 0
        for i in range(3, N):
            above |= a[i] | b[i]
        exact = above == 0 and (a[2] | b[2]) < 4
        xa = _u64(a2 << (W + S), "fe_inv_int xa") | _u64(a1 << S, "fe_inv_int xa") | (a0 >> (W - S))
        xb = _u64(b2 << (W + S), "fe_inv_int xb") | _u64(b1 << S, "fe_inv_int xb") | (b0 >> (W - S))
        lz = 64 - (xa | xb | 1).bit_length()
        ah = (_u64(xa << lz, "fe_inv_int lz shift") >> (64 - (W + 2)) << W) | a[0]
        bh = (_u64(xb << lz, "fe_inv_int lz shift") >> (64 - (W + 2)) << W) | b[0]
        if exact:
            ah = a[0] | (a[1] << W) | ((a[2] & 3) << (2 * W))
            bh = b[0] | (b[1] << W) | ((b[2] & 3) << (2 * W))
        # ---- W binary-GCD steps on the approximations
        f0, g0, f1, g1 = 1, 0, 0, 1
        for _i in range(W):
            odd = ah & 1
            if odd and ah < bh:
                ah, bh, f0, f1, g0, g1 = bh, ah, f1, f0, g1, g0
            if odd:
                ah = _u64(ah - bh, "fe_inv_int step difference")
                f0 = _i32(f0 - f1, "fe_inv_int f0")
                g0 = _i32(g0 - g1, "fe_inv_int g0")
            ah >>= 1
            f1 = _i32(f1 << 1, "fe_inv_int f1")
            g1 = _i32(g1 << 1, "fe_inv_int g1")
        # ---- (a, b) <- (f0 a + g0 b, f1 a + g1 b) / 2^W
        na, nb, ca, cb = [0] * N, [0] * N, 0, 0
        for i in range(N):
            ca = _i64(ca + _i64(f0 * a[i], "fe_inv_int ca") + _i64(g0 * b[i], "fe_inv_int ca"), "fe_inv_int ca")
            cb = _i64(cb + _i64(f1 * a[i], "fe_inv_int cb") + _i64(g1 * b[i], "fe_inv_int cb"), "fe_inv_int cb")
            if i > 0:
                na[i - 1], nb[i - 1] = ca & MASK, cb & MASK
            elif (ca | cb) & MASK:
                flag("fe_inv_int: the low limb of a row of (a, b) is not zero")
            ca >>= W
            cb >>= W
        na[N - 1] = _i32(ca, "fe_inv_int ca top") & M32
        nb[N - 1] = _i32(cb, "fe_inv_int cb top") & M32
        sa, sb = ca < 0, cb < 0
        ma, mb = (M32 if sa else 0), (M32 if sb else 0)
        cya, cyb = int(sa), int(sb)
        for i in range(N - 1):
            ta, tb = ((na[i] ^ ma) & MASK) + cya, ((nb[i] ^ mb) & MASK) + cyb
            a[i], b[i] = ta & MASK, tb & MASK
            cya, cyb = ta >> W, tb >> W
        a[N - 1] = _u32((na[N - 1] ^ ma) + cya, "fe_inv_int a top")
        b[N - 1] = _u32((nb[N - 1] ^ mb) + cyb, "fe_inv_int b top")
        if sa:
            f0, g0 = _i32(-f0, "fe_inv_int -f0"), _i32(-g0, "fe_inv_int -g0")
        if sb:
            f1, g1 = _i32(-f1, "fe_inv_int -f1"), _i32(-g1, "fe_inv_int -g1")
        # ---- (u, v) <- (f0 u + g0 v, f1 u + g1 v) / 2^W mod m; the digits are computed modulo 2^32 by design
        lu, lv = (f0 * u[0] + g0 * v[0]) & MASK, (f1 * u[0] + g1 * v[0]) & MASK
        qu, qv = (lu * f.NINV) & MASK, (lv * f.NINV) & MASK
        nu, nv, cu, cv = [0] * N, [0] * N, 0, 0
        for i in range(N):
            cu = _i64(cu + _i64(f0 * u[i], "fe_inv_int cu") + _i64(g0 * v[i], "fe_inv_int cu") + qu * f.M[i], "fe_inv_int cu")
            cv = _i64(cv + _i64(f1 * u[i], "fe_inv_int cv") + _i64(g1 * v[i], "fe_inv_int cv") + qv * f.M[i], "fe_inv_int cv")
            if i > 0:
                nu[i - 1], nv[i - 1] = cu & MASK, cv & MASK
            elif (cu | cv) & MASK:
                flag("fe_inv_int: the low limb of a row of (u, v) is not zero")
            cu >>= W
            cv >>= W
        nu[N - 1] = _i32(cu, "fe_inv_int u top")
        nv[N - 1] = _i32(cv, "fe_inv_int v top")
        if nv != v:
            v_rounds = rounds
        u, v = nu, nv
        steps.append((sa, sb, exact))
        max_u, max_v = max(max_u, abs(_signed_value(f, u))), max(max_v, abs(_signed_value(f, v)))
    if trace is not None:
        trace.update(rounds=rounds, v_rounds=v_rounds, steps=steps, max_u=max_u, max_v=max_v)
    # ---- |v| < 32 m: add 32 m and carry
    if abs(_signed_value(f, v)) >= 32 * f.mod:
        flag(f"fe_inv_int: |v| / m = {abs(_signed_value(f, v)) / f.mod:.3f}, not below 32")
    k32 = k_mod(f, 32)
    r = [_u32(v[i] + k32[i], "fe_inv_int v + 32 m") for i in range(N - 1)]
    top = v[N - 1] + k32[N - 1]
    if not 0 <= top <= M32:
        flag(f"fe_inv_int: top limb of v + 32 m out of u32: {top:#x}")
    r.append(top & M32)
    return expect(f, fe_norm_full(f, r), 1, 64, False, "fe_inv_int out")


def fe_inv_dev(f, x):
    """x in the device Montgomery form (any representative < 2 m of fe_canon_limbs' class) -> 1 / x in the same form, in
    fe_mul's result class; 0 -> 0"""
    return fe_mul(f, fe_inv_int(f, fe_canon_limbs(f, x)), fe_pow2(f, 3 * f.W * f.N))


# ------------------------------------------------------------------ butterflies (csrc/ntt_kernels.hip.h)
def bfly(K, a, b, what="BFLY"):
    """(x, y) <- (x + y, x - y + K r);  y limbs <= 2^30 - 2, y value < (K - 1) r"""
    if value_of(FR, b) >= (K - 1) * FR.mod:
        flag(f"{what}({K}) precondition: y value >= {K - 1} r")
    return fe_add(FR, a, b), fe_sub(FR, K, 1, a, b)


def dft8(x, w1, w2, w3):
    """In: x[1..7] = (1, <2), x[0] = (<=1+, <24).  Out: x[p] = X[bitrev3(p)], every output (B < 5, V < 40)."""
    f = FR
    x = [list(v) for v in x]
    expect(f, x[0], 1, 24, True, "dft8 in x0")
    for i in range(1, 8):
        expect(f, x[i], 1, 2, False, f"dft8 in x{i}")
    for i in range(4):
        x[i], x[i + 4] = bfly(3, x[i], x[i + 4])                     # sums (2+,.), diffs (4+,.)
        expect(f, x[i], 2, 26, True, "dft8 sums")
        expect(f, x[i + 4], 4, 27, True, "dft8 diffs")
    x[5] = fe_mul(f, x[5], w1)
    x[6] = fe_mul(f, x[6], w2)
    x[7] = fe_mul(f, x[7], w3)
    x[0], x[2] = bfly(5, x[0], x[2])                                 # x0 (4+,.) x2 (5+,.)
    x[1], x[3] = bfly(5, x[1], x[3])
    expect(f, x[0], 4, 30, True, "dft8 x0")
    expect(f, x[2], 5, 31, True, "dft8 x2")
    expect(f, x[1], 4, 8, False, "dft8 x1")
    expect(f, x[3], 5, 9, False, "dft8 x3")
    x[4], x[6] = bfly(3, x[4], x[6])                                 # x4 (5+,.) x6 (7+,.)
    x[5], x[7] = bfly(3, x[5], x[7])                                 # x5 (2,4) x7 (4,5)
    expect(f, x[4], 5, 29, True, "dft8 x4")
    expect(f, x[6], 7, 30, True, "dft8 x6")
    expect(f, x[5], 2, 4, False, "dft8 x5")
    expect(f, x[7], 4, 5, False, "dft8 x7")
    x[3] = fe_mul(f, x[3], w2)
    x[7] = fe_mul(f, x[7], w2)
    for i in (0, 1, 2, 4, 6):
        x[i] = fe_norm(f, x[i])
    x[0], x[1] = bfly(9, x[0], x[1])
    x[2], x[3] = bfly(3, x[2], x[3])
    x[4], x[5] = bfly(5, x[4], x[5])
    x[6], x[7] = bfly(3, x[6], x[7])
    for i in range(8):
        expect(f, x[i], 5, 40, False, f"dft8 out x{i}")
    return x


def dft4(a0, a1, a2, a3, w4):
    """a0 = (<=1+, <24) untwiddled, a1..a3 = (1, <2).  Outputs X0..X3."""
    f = FR
    expect(f, a0, 1, 24, True, "dft4 in a0")
    for i, a in enumerate((a1, a2, a3)):
        expect(f, a, 1, 2, False, f"dft4 in a{i + 1}")
    a0, a2 = bfly(3, a0, a2)
    expect(f, a0, 2, 26, True, "dft4 a0")
    expect(f, a2, 4, 27, True, "dft4 a2")
    a1, a3 = bfly(3, a1, a3)
    expect(f, a1, 2, 4, False, "dft4 a1")
    expect(f, a3, 4, 5, False, "dft4 a3")
    a3 = fe_mul(f, a3, w4)
    a2 = fe_norm(f, a2)
    a0, a1 = bfly(5, a0, a1)
    a2, a3 = bfly(3, a2, a3)
    out = [a0, a2, a1, a3]
    for i, a in enumerate(out):
        expect(f, a, 5, 40, False, f"dft4 out X{i}")
    return out


# ------------------------------------------------------------------ group law (csrc/ec.hip.h)
# A point is (X, Y, ZZ, ZZZ, inf).  Class: X (1+, <10), Y (1+, <5), ZZ, ZZZ (1, <2).
def expect_point(p, what):
    if p[4]:
        return p
    expect(FP, p[0], 1, 10, True, what + " X")
    expect(FP, p[1], 1, 5, True, what + " Y")
    expect(FP, p[2], 1, 2, False, what + " ZZ")
    expect(FP, p[3], 1, 2, False, what + " ZZZ")
    return p


def point_in_class(p):
    return p[4] or (in_class(FP, p[0], 1, 10, True) and in_class(FP, p[1], 1, 5, True)
                    and in_class(FP, p[2], 1, 2) and in_class(FP, p[3], 1, 2))


def xyzz_identity():
    z = fe_zero(FP)
    return (z, list(z), list(z), list(z), True)


def fp_is_zero_product(a):
    return not any(a) or list(a) == FP.M


def fp_is_zero_lazy(a):
    return fp_is_zero_product(fe_mul(FP, a, fe_one(FP)))


def xyzz_double_affine(x, y):
    f = FP
    expect(f, x, 1, 10, True, "double_affine x")
    expect(f, y, 1, 5, True, "double_affine y")
    U = expect(f, fe_add(f, y, y), 2, 10, 2, "dbl U")
    V = fe_sqr(f, U)
    Wv = fe_mul(f, U, V)
    S = fe_mul(f, x, V)
    XX = fe_sqr(f, x)
    Mv = expect(f, fe_add(f, fe_add(f, XX, XX), XX), 3, 6, False, "dbl M")
    MM = fe_sqr(f, Mv)
    for n, v in (("V", V), ("W", Wv), ("S", S), ("XX", XX), ("MM", MM)):
        expect(f, v, 1, 2, False, "dbl " + n)
    X3 = expect(f, fe_norm(f, fe_sub(f, 5, 1, MM, fe_add(f, S, S))), 1, 7, True, "dbl X3")
    D = expect(f, fe_sub(f, 8, 1, S, X3), 4, 10, False, "dbl D")
    YA = expect(f, fe_mul(f, Mv, D), 1, 2, False, "dbl YA")
    YB = expect(f, fe_mul(f, Wv, y), 1, 2, False, "dbl YB")
    Y3 = expect(f, fe_norm(f, fe_sub(f, 3, 1, YA, YB)), 1, 5, True, "dbl Y3")
    return (X3, Y3, V, Wv, False)


def xyzz_double(p):
    if p[4]:
        return p
    expect_point(p, "double in")
    r = xyzz_double_affine(p[0], p[1])
    zz = fe_mul(FP, r[2], p[2])
    zzz = fe_mul(FP, r[3], p[3])
    return expect_point((r[0], r[1], zz, zzz, False), "double out")


def xyzz_madd(acc, x2, y2):
    """acc + (x2, y2), affine and not the identity; x2 (<=1, <1), y2 (<=3, <3)"""
    f = FP
    expect(f, x2, 1, 1, False, "madd x2")
    expect(f, y2, 3, 3, False, "madd y2")
    if acc[4]:
        one = fe_one(f)
        return expect_point((list(x2), fe_norm(f, y2), one, list(one), False), "madd out")
    expect_point(acc, "madd in")
    X1, Y1, ZZ1, ZZZ1 = acc[:4]
    U2, S2 = fe_mul2(f, x2, ZZ1, y2, ZZZ1)
    expect(f, U2, 1, 2, False, "madd U2")
    expect(f, S2, 1, 2, False, "madd S2")
    P = expect(f, fe_norm(f, fe_sub(f, 11, 1, U2, X1)), 1, 13, True, "madd P")
    R = expect(f, fe_norm(f, fe_sub(f, 6, 1, S2, Y1)), 1, 8, True, "madd R")
    PP, RR = fe_sqr2(f, P, R)
    PPP, Q, ZZ3 = fe_mul3(f, P, PP, X1, PP, ZZ1, PP)
    for n, v in (("PP", PP), ("RR", RR), ("PPP", PPP), ("Q", Q), ("ZZ3", ZZ3)):
        expect(f, v, 1, 2, False, "madd " + n)
    t = expect(f, fe_sub(f, 3, 1, RR, PPP), 4, 5, False, "madd t")
    X3 = expect(f, fe_norm(f, fe_sub(f, 5, 1, t, fe_add(f, Q, Q))), 1, 10, True, "madd X3")
    D = expect(f, fe_sub(f, 11, 1, Q, X3), 4, 13, False, "madd D")
    nY1 = expect(f, fe_sub(f, 6, 1, fe_zero(f), Y1), 3, 6, False, "madd nY1")
    Y3, ZZZ3 = fe_mma2(f, R, D, nY1, PPP, ZZZ1, PPP)
    expect(f, Y3, 1, 2, False, "madd Y3")
    expect(f, ZZZ3, 1, 2, False, "madd ZZZ3")
    r = (X3, Y3, ZZ3, ZZZ3, False)
    if fp_is_zero_product(ZZ3):
        r = xyzz_double_affine(x2, fe_norm(f, y2)) if fp_is_zero_lazy(R) else xyzz_identity()
    return expect_point(r, "madd out")


def xyzz_add(a, b):
    f = FP
    if a[4]:
        return b
    if b[4]:
        return a
    expect_point(a, "add in a")
    expect_point(b, "add in b")
    U1, U2 = fe_mul2(f, a[0], b[2], b[0], a[2])
    S1, S2 = fe_mul2(f, a[1], b[3], b[1], a[3])
    P = expect(f, fe_norm(f, fe_sub(f, 3, 1, U2, U1)), 1, 5, True, "add P")
    R = expect(f, fe_norm(f, fe_sub(f, 3, 1, S2, S1)), 1, 5, True, "add R")
    PP, RR = fe_sqr2(f, P, R)
    PPP, Q = fe_mul2(f, P, PP, U1, PP)
    z12, zzz12 = fe_mul2(f, a[2], b[2], a[3], b[3])
    for n, v in (("U1", U1), ("U2", U2), ("S1", S1), ("S2", S2), ("PP", PP), ("RR", RR), ("PPP", PPP), ("Q", Q),
                 ("z12", z12), ("zzz12", zzz12)):
        expect(f, v, 1, 2, False, "add " + n)
    t = expect(f, fe_sub(f, 3, 1, RR, PPP), 4, 5, False, "add t")
    X3 = expect(f, fe_norm(f, fe_sub(f, 5, 1, t, fe_add(f, Q, Q))), 1, 10, True, "add X3")
    D = expect(f, fe_sub(f, 11, 1, Q, X3), 4, 13, False, "add D")
    nS1 = expect(f, fe_sub(f, 3, 1, fe_zero(f), S1), 3, 3, False, "add nS1")
    Y3, ZZ3 = fe_mma2(f, R, D, nS1, PPP, z12, PP)
    ZZZ3 = fe_mul(f, zzz12, PPP)
    for n, v in (("Y3", Y3), ("ZZ3", ZZ3), ("ZZZ3", ZZZ3)):
        expect(f, v, 1, 2, False, "add " + n)
    r = (X3, Y3, ZZ3, ZZZ3, False)
    if fp_is_zero_product(ZZ3):
        r = xyzz_double(a) if fp_is_zero_lazy(R) else xyzz_identity()
    return expect_point(r, "add out")


def xyzz_mul_small(p, k):
    r = xyzz_identity()
    if k == 0 or p[4]:
        return r
    for bit in range(k.bit_length() - 1, -1, -1):
        r = xyzz_double(r)
        if (k >> bit) & 1:
            r = xyzz_add(r, p)
    return r


def to_affine(p):
    """(x, y) of an XYZZ point held in the device Montgomery form as plain integers, None for the identity"""
    if p[4]:
        return None
    X, Y, ZZ, ZZZ = (value_of(FP, c) * FP.RINV % FP.mod for c in p[:4])
    return (X * pow(ZZ, -1, FP.mod) % FP.mod, Y * pow(ZZZ, -1, FP.mod) % FP.mod)


# ------------------------------------------------------------------ class generator
def most_redundant(f, v, Bl, plus=False, top=None):
    """limbs of v with 2^W pushed down from limb i+1 to limb i while the class (limbs < Bl 2^W (+ slack), or limbs <= top
    where a class is not of that shape) allows it"""
    if top is None:
        top = Bl * (1 << f.W) + (f.SLACK if plus else 0) - 1
    l = limbs_of(f, v)
    for i in range(f.N - 2, -1, -1):
        k = min(l[i + 1], (top - l[i]) >> f.W)
        l[i + 1] -= k
        l[i] += k << f.W
    # a second sweep: limb i+1 may have been refilled from limb i+2 before limb i took its share
    for i in range(f.N - 2, -1, -1):
        k = min(l[i + 1], (top - l[i]) >> f.W)
        l[i + 1] -= k
        l[i] += k << f.W
    assert value_of(f, l) == v and all(0 <= x <= top for x in l[:-1])
    return l


def all_max(f, Bl, V, plus=False):
    """every limb at its maximum, the top limb as large as value < V m allows"""
    top = Bl * (1 << f.W) + (f.SLACK if plus else 0) - 1
    l = [top] * (f.N - 1)
    room = V * f.mod - 1 - value_of(f, l)
    assert room >= 0
    l.append(min(top, room >> (f.W * (f.N - 1))))
    return l


def random_member(f, Bl, V, plus, rng):
    top = Bl * (1 << f.W) + (f.SLACK if plus else 0) - 1
    kind = rng.randrange(3)
    if kind == 0:                                                    # a value of the class, normalised
        return limbs_of(f, rng.randrange(V * f.mod))
    if kind == 1:                                                    # a value of the class, carries pushed down at random
        l = limbs_of(f, rng.randrange(V * f.mod))
        for i in range(f.N - 2, -1, -1):
            k = rng.randint(0, min(l[i + 1], (top - l[i]) >> f.W))
            l[i + 1] -= k
            l[i] += k << f.W
        return l
    l = [top - rng.randrange(1 << rng.randrange(1, f.W)) for _ in range(f.N - 1)]      # limbs near the bound
    room = V * f.mod - 1 - value_of(f, l)
    l.append(rng.randint(0, min(top, room >> (f.W * (f.N - 1)))))
    return l


def class_members(f, Bl, V, plus=False, n_random=0, seed=0):
    """Worst-case, edge and seeded random members of the class (Bl[+], <V)."""
    out = [all_max(f, Bl, V, plus), most_redundant(f, V * f.mod - 1, Bl, plus), limbs_of(f, V * f.mod - 1)]
    edges = [0, 1, f.mod - 1] + ([f.mod, 2 * f.mod - 1] if V > 1 else [])
    out += [limbs_of(f, e) for e in edges]
    if V > 1:
        out += [most_redundant(f, e, Bl, plus) for e in (f.mod, 2 * f.mod - 1)]
    rng = random.Random((seed << 8) ^ (Bl << 4) ^ V ^ (0x5EED if plus else 0) ^ f.W)
    out += [random_member(f, Bl, V, plus, rng) for _ in range(n_random)]
    for l in out:
        assert in_class(f, l, Bl, V, plus), (f, Bl, V, plus, l)
    return out
