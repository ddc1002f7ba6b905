"""Zero-knowledge mode (pm_plonk_prove_zk) restated in plain Python integers, without a device:
the blinded prover polynomials, the quotient of the blinded numerator over an 8n coset, the blinded quotient pieces and
the two opening witnesses.  The restatement is written here, on the oracle's round helpers, so that it can disagree with
the device code; tests/test_gpu_zk.py compares GPU proofs with it."""
import random

import pytest

from oracle import bigint_oracle as B
from oracle import plonk_rounds_oracle as PO

R = B.R_MOD
BLINDERS = 17
EXTRA_BASES = 10          # t_4 holds n + 10 coefficients: deg t' <= 4n + 9
# (first blinder, terms) of the Z_H blinders: a, b, c, d, z
WIRE_BLINDERS = ((0, 3), (3, 3), (6, 2), (8, 3))
Z_BLINDERS = (11, 3)


def _add(p, q):
    out = [0] * max(len(p), len(q))
    for i, v in enumerate(p):
        out[i] = v
    for i, v in enumerate(q):
        out[i] = (out[i] + v) % R
    return out


def zh_blind(coeffs, n, beta):
    """w(X) + (beta_0 + beta_1 X + ...) (X^n - 1)"""
    out = list(coeffs) + [0] * (n + len(beta) - len(coeffs))
    for i, b in enumerate(beta):
        out[i] = (out[i] - b) % R
        out[n + i] = (out[n + i] + b) % R
    return out


def degree(p):
    d = len(p) - 1
    while d >= 0 and p[d] % R == 0:
        d -= 1
    return d


def divide_by_zh(num, n):
    """num / (X^n - 1) -> (quotient, remainder) by long division."""
    num = list(num)
    q = [0] * max(len(num) - n, 0)
    for i in range(len(num) - 1, n - 1, -1):
        c = num[i]
        if c:
            q[i - n] = c
            num[i] = 0
            num[i - n] = (num[i - n] + c) % R
    return q, num[:n]


def numerator_8n(n, wc, zc, sel_c, pic, sig_c, ch):
    """The quotient numerator of the (blinded) polynomials on the coset 7 H_8n, interpolated: its coefficients.  Exact as
    long as its degree is below 8n (5n + 9 with blinders)."""
    log8 = (8 * n).bit_length() - 1
    m = 8 * n
    cos = lambda c: B.coset_fft(c, log8)   # noqa: E731
    w = [cos(c) for c in wc]
    z = cos(zc)
    sel = {k: cos(v) for k, v in sel_c.items()}
    pi, sig, l1 = cos(pic), [cos(s) for s in sig_c], cos([B.Domain(n).size_inv] * n)
    x = PO.powers(B.Domain(m).group_gen, PO.GEN, m)
    alpha, beta, gamma = ch["alpha"], ch["beta"], ch["gamma"]
    vals = []
    for i in range(m):
        nx = (i + 8) % m                   # one step of H further on the 8n coset
        a, b, c, d = (w[j][i] for j in range(4))
        gate = (PO.gate_value({k: sel[k][i] for k in PO.SELECTORS}, a, b, c, d, w[0][nx], w[1][nx], w[3][nx], ch)
                + pi[i]) % R
        ident, copy = z[i], z[nx]
        for j in range(4):
            ident = ident * (w[j][i] + beta * PO.K[j] * x[i] + gamma) % R
            copy = copy * (w[j][i] + beta * sig[j][i] + gamma) % R
        vals.append((gate + alpha * (ident - copy) + alpha * alpha % R * (z[i] - 1) * l1[i]) % R)
    return B.coset_ifft(vals, log8)


def zk_prove(n, sel, sigma_index, witness, pi, ch, beta):
    """Every intermediate of a zero-knowledge proof for given challenges (PO.CHALLENGES) and blinders beta[0..16]
    (canonical ints).  Arguments as PO.prove."""
    log_n = n.bit_length() - 1
    dom = B.Domain(n)
    roots = PO.powers(dom.group_gen, 1, n)
    sel = {k: list(sel.get(k, [0] * n)) for k in PO.SELECTORS}
    table = [PO.K[j] * roots[i] % R for j in range(4) for i in range(n)]
    sigmas = [[table[sigma_index[j][i]] for i in range(n)] for j in range(4)]
    out = {}
    wc = [zh_blind(B.ifft(witness[j], log_n), n, beta[f:f + t]) for j, (f, t) in enumerate(WIRE_BLINDERS)]
    num, den = PO.perm_terms(witness, sigmas, roots, ch["beta"], ch["gamma"])
    z_ev = PO.grand_product(num, den)
    zc = zh_blind(B.ifft(z_ev, log_n), n, beta[Z_BLINDERS[0]:Z_BLINDERS[0] + Z_BLINDERS[1]])
    out["wire_coeffs"], out["z_coeffs"], out["z_evals"], out["sigmas"] = wc, zc, z_ev, sigmas
    sel_c = {k: B.ifft(v, log_n) for k, v in sel.items()}
    sig_c = [B.ifft(s, log_n) for s in sigmas]
    out["sel_coeffs"], out["sigma_coeffs"] = sel_c, sig_c
    pic = B.ifft(pi, log_n)
    numer = numerator_8n(n, wc, zc, sel_c, pic, sig_c, ch)
    t, rem = divide_by_zh(numer, n)
    out["numerator"], out["remainder"] = numer, rem
    t = (t + [0] * (4 * n + EXTRA_BASES))[:4 * n + EXTRA_BASES]
    out["t_coeffs"] = t
    b14, b15, b16 = beta[14:17]
    pieces = [t[:n] + [b14],
              [(t[n] - b14) % R] + t[n + 1:2 * n] + [b15],
              [(t[2 * n] - b15) % R] + t[2 * n + 1:3 * n] + [b16],
              [(t[3 * n] - b16) % R] + t[3 * n + 1:]]
    out["t_pieces"] = pieces
    zz = ch["z"]
    zw = zz * dom.group_gen % R
    ev = {nm: B.horner(wc[j], zz) for j, nm in enumerate("abcd")}
    for j, nm in ((0, "a_next"), (1, "b_next"), (3, "d_next")):
        ev[nm] = B.horner(wc[j], zw)
    for j in range(3):
        ev[f"sigma_{j + 1}"] = B.horner(sig_c[j], zz)
    for nm in ("q_arith", "q_c", "q_l", "q_r"):
        ev[nm] = B.horner(sel_c[nm], zz)
    ev["z_next"] = B.horner(zc, zw)
    zn = pow(zz, n, R)
    ev["t"] = (B.horner(pieces[0], zz) + zn * B.horner(pieces[1], zz) + zn * zn * B.horner(pieces[2], zz)
               + pow(zn, 3, R) * B.horner(pieces[3], zz)) % R
    lc = PO.linearisation_coeffs(ev, ch, n)
    names = list(PO.SELECTORS[:6]) + list(PO.WIDGET_SELECTORS)
    r = PO.lincomb([lc[k] for k in names] + [lc["sigma_4"]], [sel_c[k] for k in names] + [sig_c[3]])
    r = _add(r, [lc["z"] * v % R for v in zc])
    ev["r"] = B.horner(r, zz)
    out["r_coeffs"], out["evals"] = r, ev
    aw, aws = ch["aw"], ch["aw_shifted"]
    agg = [0]
    for c, p in zip([1, zn, zn * zn, pow(zn, 3, R)] + [pow(aw, e, R) for e in range(1, 9)],
                    pieces + [r] + wc + sig_c[:3]):
        agg = _add(agg, [c * v % R for v in p])
    agg_s = [0]
    for c, p in zip([pow(aws, e, R) for e in range(4)], [zc, wc[0], wc[1], wc[3]]):
        agg_s = _add(agg_s, [c * v % R for v in p])
    out["agg"], out["agg_shifted"] = agg, agg_s
    out["w_z"], out["w_zw"] = PO.ruffini(agg, zz), PO.ruffini(agg_s, zw)
    return out


def random_challenges(rng):
    return {k: rng.randrange(1, R) for k in PO.CHALLENGES}


def circuit_ints(n, seed, mixed):
    import plonk_prototype_amd as pa
    from plonk_prototype_amd.field import fr_vec_from_limbs
    circuit, wit, pi = (pa.synthetic.mixed_circuit if mixed else pa.synthetic.chain_circuit)(n, seed)
    sel = {k: fr_vec_from_limbs(getattr(circuit, k)) if getattr(circuit, k) is not None else [0] * n for k in PO.SELECTORS}
    return circuit, wit, pi, (sel, circuit.sigma_index.tolist(), [fr_vec_from_limbs(wit[j]) for j in range(4)],
                              fr_vec_from_limbs(pi))


CASES = [(8, False), (16, False), (32, True)]


@pytest.mark.parametrize("n,mixed", CASES)
def test_blinded_polynomials_agree_with_the_originals_on_h(n, mixed):
    rng = random.Random(n)
    _, _, _, (sel, sigma, wit, pi) = circuit_ints(n, n, mixed)
    beta = [rng.randrange(R) for _ in range(BLINDERS)]
    ch = random_challenges(rng)
    zk = zk_prove(n, sel, sigma, wit, pi, ch, beta)
    plain = PO.prove(n, sel, sigma, wit, pi, ch)
    roots = PO.powers(B.Domain(n).group_gen, 1, n)
    for j in range(4):
        assert len(zk["wire_coeffs"][j]) == (n + 2 if j == 2 else n + 3)
        assert [B.horner(zk["wire_coeffs"][j], x) for x in roots] == wit[j]
        assert zk["wire_coeffs"][j] != plain["wire_coeffs"][j]
    assert len(zk["z_coeffs"]) == n + 3
    assert [B.horner(zk["z_coeffs"], x) for x in roots] == zk["z_evals"] == plain["z_evals"]


@pytest.mark.parametrize("n,mixed", CASES)
def test_quotient_degree_is_exactly_4n_plus_9(n, mixed):
    """The numerator of the blinded polynomials divides exactly by Z_H (every widget present at n = 32), and the quotient
    has degree exactly 4n + 9: so t_4 needs n + 10 coefficients and the commit key n + 10 points."""
    rng = random.Random(100 + n)
    _, _, _, (sel, sigma, wit, pi) = circuit_ints(n, n, mixed)
    if mixed:
        assert all(any(sel[k]) for k in PO.WIDGET_SELECTORS)
    for trial in range(2):
        beta = [rng.randrange(1, R) for _ in range(BLINDERS)]
        zk = zk_prove(n, sel, sigma, wit, pi, random_challenges(rng), beta)
        assert not any(zk["remainder"])
        assert degree(zk["numerator"]) == 5 * n + 9
        assert degree(zk["t_coeffs"]) == 4 * n + 9
        assert len(zk["t_pieces"][3]) == n + EXTRA_BASES
        assert [len(p) for p in zk["t_pieces"][:3]] == [n + 1] * 3


def test_zero_blinders_give_the_plain_quotient():
    n = 16
    rng = random.Random(7)
    _, _, _, (sel, sigma, wit, pi) = circuit_ints(n, 3, False)
    ch = random_challenges(rng)
    zk = zk_prove(n, sel, sigma, wit, pi, ch, [0] * BLINDERS)
    plain = PO.prove(n, sel, sigma, wit, pi, ch)
    assert zk["t_coeffs"][:4 * n] == plain["t_coeffs"] and not any(zk["t_coeffs"][4 * n:])
    assert zk["evals"] == plain["evals"]


@pytest.mark.parametrize("n,mixed", CASES)
def test_pieces_telescope_at_every_point(n, mixed):
    """t_1' + z^n t_2' + z^2n t_3' + z^3n t_4' = t'(z): the verifier's combination of the four commitments is unchanged."""
    rng = random.Random(200 + n)
    _, _, _, (sel, sigma, wit, pi) = circuit_ints(n, n, mixed)
    beta = [rng.randrange(R) for _ in range(BLINDERS)]
    zk = zk_prove(n, sel, sigma, wit, pi, random_challenges(rng), beta)
    p = zk["t_pieces"]
    for _ in range(4):
        z = rng.randrange(R)
        zn = pow(z, n, R)
        got = (B.horner(p[0], z) + zn * B.horner(p[1], z) + zn * zn * B.horner(p[2], z) + pow(zn, 3, R) * B.horner(p[3], z))
        assert got % R == B.horner(zk["t_coeffs"], z)


@pytest.mark.parametrize("n,mixed", [(16, False), (32, True)])
def test_blinded_openings_satisfy_the_verifier_identity(n, mixed):
    """The evaluations of the blinded polynomials satisfy the verifier's scalar equation, and the opening witnesses divide."""
    rng = random.Random(300 + n)
    _, _, _, (sel, sigma, wit, pi) = circuit_ints(n, n, mixed)
    beta = [rng.randrange(R) for _ in range(BLINDERS)]
    ch = random_challenges(rng)
    zk = zk_prove(n, sel, sigma, wit, pi, ch, beta)
    pi_z = B.horner(B.ifft(pi, n.bit_length() - 1), ch["z"])
    assert PO.check_identity(zk["evals"], ch, n, pi_z)
    assert len(zk["w_z"]) == n + EXTRA_BASES - 1
    x = rng.randrange(R)
    zz = ch["z"]
    ev = zk["evals"]
    aw = ch["aw"]
    agg_z = (ev["t"] + sum(pow(aw, e + 1, R) * ev[k] for e, k in
                           enumerate(("r", "a", "b", "c", "d", "sigma_1", "sigma_2", "sigma_3")))) % R
    assert B.horner(zk["w_z"], x) * (x - zz) % R == (B.horner(zk["agg"], x) - agg_z) % R
