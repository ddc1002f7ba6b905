"""Host-side ground for the Lagrange-form commit key: the big-integer oracle of the G1 inverse NTT that
tests/test_gpu_lagrange.py checks the kernel against, and the witness-shaped synthetic circuit."""
import numpy as np

from oracle import bigint_oracle as B


def lagrange_oracle(points, log_n: int):
    """out[i] = n^-1 sum_j w^-ij P_j over affine int points (None = identity): an O(n^2) sum of scalar multiples."""
    n = 1 << log_n
    d = B.Domain(n)
    out = []
    for i in range(n):
        acc = None
        for j, p in enumerate(points[:n]):
            acc = B.g1_add(acc, B.g1_mul(d.size_inv * pow(d.group_gen_inv, i * j, B.R_MOD), p))
        out.append(acc)
    return out


def test_oracle_lagrange_key_of_tau_powers():
    """The oracle's key of [tau^j G] is [L_i(tau) G]: shows the oracle itself is right."""
    log_n, tau = 3, 0x1D0B2C3E4F5A69788796A5B4C3D2E1F00F1E2D3C4B5A6978
    powers = [B.g1_mul(pow(tau, j, B.R_MOD), B.G1_GEN) for j in range(8)]
    lag = B.Domain(8).evaluate_all_lagrange_coefficients(tau)
    assert lagrange_oracle(powers, log_n) == [B.g1_mul(c, B.G1_GEN) for c in lag]


def test_oracle_lagrange_key_edge_points():
    # (P, .., P) -> (P, O, .., O);  (P, O, .., O) -> n^-1 P everywhere
    P = B.g1_mul(12345, B.G1_GEN)
    assert lagrange_oracle([P] * 4, 2) == [P, None, None, None]
    assert lagrange_oracle([P, None, None, None], 2) == [B.g1_mul(pow(4, -1, B.R_MOD), P)] * 4


def test_boolean_circuit_satisfied_and_bit_heavy():
    import plonk_prototype_amd as pa
    from plonk_prototype_amd.field import R_MOD, fr_vec_from_limbs

    for n in (8, 16, 64, 1024):
        c, wit, pi = pa.synthetic.boolean_circuit(n, seed=n)
        assert c.n == n and wit.shape == (4, n, 4) and not pi.any()
        w = [fr_vec_from_limbs(wit[j]) for j in range(4)]
        q = {k: fr_vec_from_limbs(getattr(c, k)) for k in ("q_m", "q_l", "q_r", "q_o", "q_4", "q_c", "q_arith")}
        for i in range(n):
            assert q["q_arith"][i] == 1
            gate = (q["q_m"][i] * w[0][i] * w[1][i] + q["q_l"][i] * w[0][i] + q["q_r"][i] * w[1][i]
                    + q["q_o"][i] * w[2][i] + q["q_4"][i] * w[3][i] + q["q_c"][i])
            assert gate % R_MOD == 0, (n, i)
        # the copy permutation is a permutation and joins equal values only
        flat = sum(w, [])
        sig = np.asarray(c.sigma_index).reshape(-1)
        assert np.array_equal(np.sort(sig), np.arange(4 * n))
        assert all(flat[sig[k]] == flat[k] for k in range(4 * n))
        assert sum(v in (0, 1) for v in flat) >= 0.9 * len(flat)
        assert any(v > 1 for v in flat)                  # the recombination rows are there
