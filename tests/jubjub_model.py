"""Big-integer model of the native JubJub calls (include/plonk_mi355x.h, pm_jubjub_*): the affine law of
``gadget_model.jubjub_add`` and plain double-and-add over the INTEGER scalar, most significant bit first -- no signed digits, no
windows, no tables.  The ladder runs in projective coordinates (the same law with the denominators carried along) so that a
multiplication is one modular inversion; ``mul_affine`` is the law applied literally, and the host test compares the two.
Plain Python integers throughout; nothing here touches the library's arithmetic."""
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gadget_model as M  # noqa: E402

R = M.R
D = M.EDWARDS_D
IDENTITY = (0, 1)
Q = 0x0E7DB4EA6533AFA906673B0101343B00A6682093CCC81082D0970E5ED6F72CB7     # the order of the prime-order subgroup
GENERATOR = (0x3FD2814C43AC65A6F1FBF02D0FD6CCE62E3EBB21FD6C54ED4DF7B7FFEC7BEACA, 0x12)

add = M.jubjub_add
on_curve = M.on_curve


def _padd(p, q):
    """the affine law on (X : Y : Z), x = X / Z, y = Y / Z"""
    (x1, y1, z1), (x2, y2, z2) = p, q
    a = z1 * z2 % R
    b = a * a % R
    c, d = x1 * x2 % R, y1 * y2 % R
    e = D * c % R * d % R
    f, g = (b - e) % R, (b + e) % R
    return (a * f % R * ((x1 + y1) * (x2 + y2) - c - d) % R, a * g % R * (d + c) % R, f * g % R)


def mul(p, s: int):
    """s * p for the integer s >= 0 by double-and-add from the top bit"""
    acc, pp = (0, 1, 1), (p[0], p[1], 1)
    for i in range(s.bit_length() - 1, -1, -1):
        acc = _padd(acc, acc)
        if (s >> i) & 1:
            acc = _padd(acc, pp)
    zi = pow(acc[2], -1, R)
    return acc[0] * zi % R, acc[1] * zi % R


def mul_affine(p, s: int):
    """the same with the affine law applied literally (slow: two inversions an addition)"""
    acc = IDENTITY
    for i in range(s.bit_length() - 1, -1, -1):
        acc = add(acc, acc)
        if (s >> i) & 1:
            acc = add(acc, p)
    return acc


# ------------------------------------------------------------------------------------------ the inputs the tests share
def edge_scalars(seed: int = 5, extra: int = 12):
    """0, 1, 2, 7, 8, 9, 15, 16, 17 (the digit boundaries), the subgroup order and its neighbours, the field's, powers of two,
    the three nibble patterns that drive the recoding's carry from end to end, then `extra` random ones"""
    rng = random.Random(seed)
    fixed = [0, 1, 2, 7, 8, 9, 15, 16, 17, Q - 1, Q, Q + 1, 8 * Q, R - 1, 1 << 252, 1 << 254,
             int("8" * 64, 16) % R, int("7" * 64, 16) % R, int("f" * 64, 16) % R]
    assert all(0 <= s < R for s in fixed)
    return fixed + [rng.randrange(R) for _ in range(extra)]


SQRT_M1 = M._sqrt(R - 1)           # i with i^2 = -1


def edge_points(seed: int = 9, extra: int = 3):
    """the generator; a point whose order is not Q; the identity; (0, -1) of order 2; (i, 0) of order 4; random points"""
    rng = random.Random(seed)
    pts = [GENERATOR, M.curve_point(0x14), IDENTITY, (0, R - 1), (SQRT_M1, 0)]
    pts += [M.curve_point(rng.randrange(R)) for _ in range(extra)]
    assert all(on_curve(p) for p in pts)
    return pts


def to_limbs(points):
    """[(x, y)] -> [n, 2, 4] Montgomery limbs"""
    return M.to_limbs([c for p in points for c in p]).reshape(-1, 2, 4)
