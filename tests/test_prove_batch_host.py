"""Host-side ground for the batch prover (pm_plonk_prove_batch): the new exports are in the library and bound, and the
synthetic batches -- chain_witnesses and boolean_circuit's seeds -- are distinct witnesses of ONE circuit, checked with
Python integers.  No device compute here."""
import ctypes as C

import numpy as np
import pytest

BATCH_EXPORTS = ("pm_plonk_batch_create", "pm_plonk_batch_free", "pm_plonk_batch_bytes", "pm_plonk_prove_batch")


def test_batch_symbols_exported_and_bound():
    import plonk_prototype_amd as pa
    from plonk_prototype_amd import _lib
    lib = C.CDLL(pa.LIB_PATH)
    for name in BATCH_EXPORTS:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    bound = pa.load()
    for name in BATCH_EXPORTS:
        assert getattr(bound, name).argtypes == _lib.SIGNATURES[name][1]
    assert _lib.PLONK_MAX_BATCH == 64
    assert callable(pa.prove_batch) and callable(pa.ProverKey.batch)
    assert pa.synthetic.chain_witnesses is not None


def _fr(a):
    from plonk_prototype_amd.field import fr_vec_from_limbs
    return fr_vec_from_limbs(np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4))


def _check_satisfied(circuit, witness, pi):
    """Gate equation on every row and copy constraints on every position, in Python integers."""
    from plonk_prototype_amd.field import R_MOD
    n = circuit.n
    w = _fr(witness)                                   # position j n + i
    sel = {k: (_fr(getattr(circuit, k)) if getattr(circuit, k) is not None else [0] * n)
           for k in ("q_m", "q_l", "q_r", "q_o", "q_4", "q_c", "q_arith")}
    p = _fr(pi)
    for i in range(n):
        a, b, c, d = w[i], w[n + i], w[2 * n + i], w[3 * n + i]
        g = (sel["q_m"][i] * a * b + sel["q_l"][i] * a + sel["q_r"][i] * b + sel["q_o"][i] * c + sel["q_4"][i] * d
             + sel["q_c"][i]) * sel["q_arith"][i] + p[i]
        assert g % R_MOD == 0, f"gate {i}"
    sig = np.asarray(circuit.sigma_index).reshape(-1)
    assert all(w[q] == w[int(sig[q])] for q in range(4 * n)), "copy constraint"


def _same_circuit(c1, c2):
    from plonk_prototype_amd.prover import SELECTORS
    for k in SELECTORS:
        a, b = getattr(c1, k), getattr(c2, k)
        assert (a is None) == (b is None), k
        if a is not None:
            assert np.array_equal(a, b), k
    assert np.array_equal(np.asarray(c1.sigma_index), np.asarray(c2.sigma_index))


@pytest.mark.parametrize("n", [4, 16, 64])
def test_chain_witnesses_satisfy_chain_circuit(n):
    from plonk_prototype_amd import synthetic
    circuit, wit0, pi0 = synthetic.chain_circuit(n, 3)
    rows = [(0,), (), tuple(range(min(n, 20))), (n - 1,)]
    pairs = synthetic.chain_witnesses(n, 3, count=4, witness_seed=9, public_rows=rows)
    assert len(pairs) == 4
    for (w, pi), r in zip(pairs, rows):
        assert w.shape == (4, n, 4) and pi.shape == (n, 4)
        assert set(np.flatnonzero(pi.any(axis=1)).tolist()) <= set(r)
        _check_satisfied(circuit, w, pi)
    _check_satisfied(circuit, wit0, pi0)
    ws = [w.tobytes() for w, _ in pairs] + [wit0.tobytes()]
    assert len(set(ws)) == len(ws), "the witnesses must differ"
    # deterministic, and the selectors of chain_circuit are untouched by it
    again = synthetic.chain_witnesses(n, 3, count=4, witness_seed=9, public_rows=rows)
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(pairs, again))
    other = synthetic.chain_witnesses(n, 3, count=1, witness_seed=10)[0]
    assert not np.array_equal(other[0], pairs[0][0])
    _same_circuit(circuit, synthetic.chain_circuit(n, 3)[0])


def test_chain_witnesses_with_zero_selectors():
    from plonk_prototype_amd import synthetic
    circuit, _, _ = synthetic.chain_circuit(32, 5, zero_selectors=("q_m", "q_4"))
    for w, pi in synthetic.chain_witnesses(32, 5, count=3, witness_seed=2, zero_selectors=("q_m", "q_4")):
        _check_satisfied(circuit, w, pi)
    with pytest.raises(ValueError):
        synthetic.chain_witnesses(32, 5, count=3, public_rows=[(0,), (1,)])


@pytest.mark.parametrize("n", [8, 64, 256])
def test_boolean_circuit_seeds_share_the_circuit(n):
    from plonk_prototype_amd import synthetic
    c1, w1, p1 = synthetic.boolean_circuit(n, 1)
    seen = {w1.tobytes()}
    for s in (2, 3, 7):
        c2, w2, p2 = synthetic.boolean_circuit(n, s)
        _same_circuit(c1, c2)
        _check_satisfied(c1, w2, p2)
        seen.add(w2.tobytes())
    assert len(seen) >= 3
