"""Big-integer model of the JubJub wire format and of the square root under it (include/plonk_mi355x.h, pm_fr_sqrt_* and
pm_jubjub_compress / pm_jubjub_decompress*): a point is 32 bytes, the canonical y little-endian with the least significant bit
of the canonical x in bit 255.  The root is ``gadget_model._sqrt`` -- the textbook Tonelli-Shanks loop, which is neither the
device's windowed logarithm nor a copy of the library's host form -- made a function of its input by taking the EVEN root.
Plain Python integers throughout; nothing here touches the library's arithmetic."""
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gadget_model as M  # noqa: E402
import jubjub_model as J  # noqa: E402

R = M.R
D = M.EDWARDS_D
OK, BAD_RANGE, BAD_NOT_ON_CURVE, BAD_SIGN, BAD_NOT_IN_SUBGROUP = 0, 1, 2, 3, 4
ROOT_OF_UNITY = pow(7, (R - 1) >> 32, R)       # g, of order 2^32


def sqrt_even(a: int):
    """(root, is_square) of the canonical a: the root whose integer is even, 0 for 0; (0, 0) for a non-square or a >= R"""
    if a >= R:
        return 0, 0
    x = M._sqrt(a)
    if x is None:
        return 0, 0
    return (R - x if x & 1 else x), 1


def encode(p) -> bytes:
    x, y = p
    return (y | ((x & 1) << 255)).to_bytes(32, "little")


def decode(data: bytes, check_subgroup: bool = False):
    """(point, status): the LOWEST status that applies; a refused point is (0, 0)"""
    v = int.from_bytes(data, "little")
    sign, y = v >> 255, v & ((1 << 255) - 1)
    if y >= R:
        return (0, 0), BAD_RANGE
    y2 = y * y % R
    x, square = sqrt_even((y2 - 1) * pow(1 + D * y2, -1, R) % R)
    if not square:
        return (0, 0), BAD_NOT_ON_CURVE
    if x == 0 and sign:
        return (0, 0), BAD_SIGN
    if (x & 1) != sign:
        x = R - x
    if check_subgroup and J.mul((x, y), J.Q) != J.IDENTITY:
        return (0, 0), BAD_NOT_IN_SUBGROUP
    return (x, y), OK


def y_bytes(y: int, sign: int = 0) -> bytes:
    """the 32 bytes of any y below 2^255 with the sign bit: what refusals are made of"""
    return (y | (sign << 255)).to_bytes(32, "little")


# ------------------------------------------------------------------------------------------ the inputs the tests share
LOG_SQUARES = [0, 2, 1 << 8, 1 << 16, 1 << 24, 1 << 31, (1 << 16) - 2, (1 << 24) - 2, (1 << 32) - 2]
LOG_NON_SQUARES = [1, (1 << 8) + 1, (1 << 32) - 1]


def sqrt_edge_inputs(seed: int = 11):
    """0, 1, 4, r - 1, 7, d, then c^(2^32) g^k for a random c and the k of LOG_SQUARES + LOG_NON_SQUARES.  The windowed search
    runs on a^t and t = (r - 1) / 2^32 is -1 mod 2^32, so it meets -k mod 2^32, not k: k = 2 is met as 0xfffffffe, all-ones
    windows, and k = 2^32 - 2 as 2.  The list still holds zero windows, all-ones windows and carries across window boundaries
    as MET logarithms only because it is nearly closed under negation (tests/test_fr_sqrt_tables.py checks the sign;
    tests/fr_sqrt_cases.py has the inputs that are stated as what the search meets, and that reach every table entry)."""
    rng = random.Random(seed)
    out = [0, 1, 4, R - 1, 7, D]
    for k in LOG_SQUARES + LOG_NON_SQUARES:
        c = rng.randrange(1, R)
        out.append(pow(c, 1 << 32, R) * pow(ROOT_OF_UNITY, k, R) % R)
    return out


def sqrt_inputs(n: int, seed: int = 12):
    """the edge inputs first, then random ones, n in all (at least the edge inputs)"""
    rng = random.Random(seed)
    edge = sqrt_edge_inputs()
    return edge + [rng.randrange(R) for _ in range(max(0, n - len(edge)))]


def random_points(n: int, seed: int = 13):
    rng = random.Random(seed)
    return [M.curve_point(rng.randrange(R)) for _ in range(n)]


def refusals():
    """[(bytes, status without the flag)]: every kind of refusal"""
    return [(y_bytes(R), BAD_RANGE), (y_bytes(R + 1), BAD_RANGE), (y_bytes((1 << 255) - 1), BAD_RANGE),
            (y_bytes(R, 1), BAD_RANGE), (y_bytes(2), BAD_NOT_ON_CURVE), (y_bytes(4, 1), BAD_NOT_ON_CURVE),
            (y_bytes(1, 1), BAD_SIGN), (y_bytes(R - 1, 1), BAD_SIGN)]
