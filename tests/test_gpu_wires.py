"""Composer-form circuits on the GPU: the copy permutation from wire variables against a numpy
restatement of its definition (exact, and the same on every call), keys built from wire variables against keys built from that
reference permutation (verifier key and proof bytes), the witness expansion against numpy indexing, ``variables=`` end to
end, and the refusals of the contract."""
import ctypes as C

import numpy as np
import pytest

from oracle import bigint_oracle as B
from oracle.cpu_oracle import limbs_to_ints

pytestmark = pytest.mark.gpu
R = B.R_MOD
NO_VAR = 0xFFFFFFFF
TAU = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % R
_CACHE: dict = {}


# ---------------------------------------------------------------------------------- the reference
def ref_sigma(wire_vars) -> np.ndarray:
    """The definition: the positions of a variable, ordered by rank 4 i + j, form one cycle; PM_PLONK_NO_VAR positions are fixed."""
    ids = np.asarray(wire_vars).reshape(-1).astype(np.int64)
    n = ids.size // 4
    p = np.arange(4 * n)
    rank = 4 * (p % n) + p // n
    order = np.lexsort((rank, ids))
    so = ids[order]
    nxt = np.roll(order, -1)
    starts = np.flatnonzero(np.r_[True, so[1:] != so[:-1]])
    nxt[np.r_[starts[1:] - 1, 4 * n - 1]] = order[starts]
    sigma = np.empty(4 * n, np.int64)
    sigma[order] = nxt
    sigma[ids == NO_VAR] = p[ids == NO_VAR]
    return sigma


def _sigma(ctx, wire_vars, num_vars):
    """pm_plonk_sigma_from_wires as a C caller sees it -> (status, sigma_index [4n])."""
    from plonk_prototype_amd import _lib
    wv = np.ascontiguousarray(np.asarray(wire_vars).reshape(-1), dtype=np.uint32)
    n = wv.size // 4
    out = np.full(4 * n, -1, np.int64)
    rc = ctx._lib.pm_plonk_sigma_from_wires(ctx._h, wv.ctypes.data_as(_lib.u32p), num_vars, n,
                                            out.ctypes.data_as(C.POINTER(C.c_int64)))
    return rc, out


def _chain_vars(n):
    ar = np.arange(n, dtype=np.int64)
    return np.concatenate([ar, np.maximum(ar - 1, 0), ar + 1, np.maximum(ar - 2, 0)])


def _patterns(n):
    """(name, wire_vars [4n], num_vars): every id pattern of the contract at this n."""
    import plonk_prototype_amd as pa
    rng = np.random.default_rng(n)
    total = 4 * n
    yield "distinct", rng.permutation(total), total
    yield "one id", np.full(total, 5), 6
    yield "two ids", np.arange(total) % 2, 2
    yield "chain", _chain_vars(n), n + 1
    if n >= 8:
        c, _, _ = pa.synthetic.boolean_circuit_wires(n, 1)
        yield "boolean", c.wire_vars.reshape(-1), c.num_vars
    for num_vars in (1, 2, 255, 256, 257, 65535, 65536, 65537, (1 << 24) + 1, (1 << 32) - 1):
        ids = rng.integers(0, num_vars, size=total, dtype=np.uint64)
        yield f"random below {num_vars}", ids, num_vars
        holes = ids.copy()
        holes[rng.random(total) < 0.1] = NO_VAR
        yield f"random below {num_vars} with holes", holes, num_vars
    yield "all holes", np.full(total, NO_VAR), 0


# ---------------------------------------------------------------------------------- 1. permutation parity
@pytest.mark.parametrize("n", [4, 8, 64, 1 << 10, 1 << 12, 1 << 14])
def test_sigma_from_wires_is_the_definition(ctx, n):
    for name, wv, num_vars in _patterns(n):
        want = ref_sigma(wv)
        rc, got = _sigma(ctx, wv, num_vars)
        assert rc == 0, (name, ctx._lib.pm_last_error(ctx._h))
        assert np.array_equal(got, want), f"{name}: positions {np.flatnonzero(got != want)[:8]}"
        rc2, again = _sigma(ctx, wv, num_vars)
        assert rc2 == 0 and np.array_equal(again, got), f"{name}: the second call differs"
    # what "distinct" and "one id" mean
    assert np.array_equal(_sigma(ctx, np.arange(4 * n), 4 * n)[1], np.arange(4 * n))
    one = _sigma(ctx, np.zeros(4 * n), 1)[1]
    seen, p = 0, 0
    while True:
        p, seen = int(one[p]), seen + 1
        if p == 0 or seen > 4 * n:
            break
    assert seen == 4 * n, "one variable everywhere is a single cycle through all positions"
    assert one[0] == n and one[3 * n] == 1                 # gate 0: a -> b ... d -> gate 1's a


def test_sort_only_three_passes_hundreds_of_tiles(ctx):
    import plonk_prototype_amd as pa
    n = 1 << 16
    wv = np.random.default_rng(16).integers(0, 1 << 18, size=4 * n, dtype=np.uint64)
    passes, tiles = C.c_uint32(), C.c_uint32()
    assert pa.load().pm_test_wire_sort_plan(n, 1 << 18, C.byref(passes), C.byref(tiles), None) == 0
    assert passes.value == 3 and tiles.value >= 64
    rc, got = _sigma(ctx, wv, 1 << 18)
    assert rc == 0 and np.array_equal(got, ref_sigma(wv))
    assert np.array_equal(pa.sigma_from_wires(wv.reshape(4, n), 1 << 18, ctx), got.reshape(4, n))


def test_sigma_from_wires_dev(ctx):
    n = 1 << 12
    rng = np.random.default_rng(12)
    wv = rng.integers(0, 3 * n, size=4 * n, dtype=np.uint64).astype(np.uint32)
    wv[rng.random(4 * n) < 0.05] = NO_VAR
    lib, h = ctx._lib, ctx._h
    d_w, d_s = C.c_void_p(), C.c_void_p()
    ctx._check(lib.pm_dev_alloc(h, 4 * n * 4, C.byref(d_w)))
    ctx._check(lib.pm_dev_alloc(h, 4 * n * 8, C.byref(d_s)))
    ctx._check(lib.pm_dev_upload(h, d_w, wv.ctypes.data_as(C.c_void_p), 4 * n * 4))
    got = np.zeros(4 * n, np.int64)
    try:
        assert lib.pm_plonk_sigma_from_wires_dev(h, d_w, 3 * n, n, d_s, None) == 0
        ctx._check(lib.pm_dev_download(h, got.ctypes.data_as(C.c_void_p), d_s, 4 * n * 8))
    finally:
        lib.pm_dev_free(h, d_w)
        lib.pm_dev_free(h, d_s)
    assert np.array_equal(got, ref_sigma(wv))


# ---------------------------------------------------------------------------------- 2. key parity
def _commit_key(ctx, n):
    """n + 10 powers of TAU (zero-knowledge proofs need the ten more), once per size."""
    import plonk_prototype_amd as pa
    from plonk_prototype_amd.field import fr_to_limbs
    if ("ck", n) not in _CACHE:
        _CACHE[("ck", n)] = pa.CommitKey.setup(n + 9, fr_to_limbs(TAU), ctx, precompute=True)
    return _CACHE[("ck", n)]


def _mixed_wires(n, seed):
    """mixed_circuit with its variables as wire ids: every widget position its own variable, the chain rows (the ones with
    q_arith set) sharing the chain's."""
    import plonk_prototype_amd as pa
    circuit, wit, pi = pa.synthetic.mixed_circuit(n, seed)
    w0 = int(np.flatnonzero(circuit.q_arith.any(axis=1))[0])
    g = np.arange(n - w0, dtype=np.int64)
    var = np.arange(4 * n, dtype=np.int64) + 4 * n
    for j, idx in enumerate((g, np.maximum(g - 1, 0), g + 1, np.maximum(g - 2, 0))):
        var[j * n + w0:j * n + n] = idx
    sig = circuit.sigma_index.reshape(-1)
    assert np.array_equal(var[sig], var) and np.count_nonzero(sig == np.arange(4 * n)) >= 4 * w0
    sel = {k: getattr(circuit, k) for k in pa.prover.SELECTORS}
    return pa.Circuit(wire_vars=var.astype(np.uint32).reshape(4, n), num_vars=8 * n, **sel), wit, pi


def _wire_case(name, n):
    """(circuit in wire form, three (witness, public inputs) pairs of it)"""
    import plonk_prototype_amd as pa
    S = pa.synthetic
    if name == "chain":
        circuit, _, _ = S.chain_circuit_wires(n, 21)
        return circuit, S.chain_witnesses(n, 21, count=3, witness_seed=4)
    if name == "boolean":
        circuit, _, pi = S.boolean_circuit_wires(n, 1)
        return circuit, [(S.boolean_circuit(n, s)[1], pi) for s in (1, 2, 3)]
    circuit, wit, pi = _mixed_wires(n, 5)
    return circuit, [(wit, pi)] * 3


def _same(a, b):
    return a.native_bytes == b.native_bytes and a.challenges == b.challenges and len(a.native_bytes) == 1040


@pytest.mark.parametrize("name,n", [("chain", 1 << 10), ("boolean", 1 << 12), ("mixed", 64)])
def test_key_from_wires_is_the_key_from_the_reference_permutation(ctx, oracle, name, n):
    import plonk_prototype_amd as pa
    from plonk_prototype_amd.field import fr_to_limbs
    PR = pa.prover
    wires, pairs = _wire_case(name, n)
    want = ref_sigma(wires.wire_vars)
    sel = {k: getattr(wires, k) for k in PR.SELECTORS}
    dense = pa.Circuit(sigma_index=want.reshape(4, n), **sel)
    ck = _commit_key(ctx, n)
    pk_w, pk_d = PR.preprocess(wires, ctx, ck), PR.preprocess(dense, ctx, ck)
    try:
        assert ctx._lib.pm_plonk_key_num_vars(pk_w._h) == wires.num_vars and ctx._lib.pm_plonk_key_num_vars(pk_d._h) == 0
        assert set(pk_w.verifier_key) == set(PR.VK_NAMES) and len(PR.VK_NAMES) == 15
        for nm in PR.VK_NAMES:
            assert np.array_equal(pk_w.verifier_key[nm], pk_d.verifier_key[nm]), nm
        assert np.array_equal(pk_w.sigma_index, want)              # filled from pm_plonk_sigma_from_wires on first use
        wit, pi = pairs[0]
        assert _same(PR.prove(pk_w, ck, wit, pi), PR.prove(pk_d, ck, wit, pi))
        bl = np.stack([fr_to_limbs(0x1234567 * (k + 1) + k) for k in range(17)])
        pk_w.enable_zk()
        pk_d.enable_zk()
        assert _same(PR.prove(pk_w, ck, wit, pi, zero_knowledge=True, blinders=bl),
                     PR.prove(pk_d, ck, wit, pi, zero_knowledge=True, blinders=bl))
        ws, pis = [w for w, _ in pairs], [p for _, p in pairs]
        got, exp = PR.prove_batch(pk_w, ck, ws, pis), PR.prove_batch(pk_d, ck, ws, pis)
        assert len(got) == 3 and all(_same(a, b) for a, b in zip(got, exp))
        lck = ck.lagrange(n.bit_length() - 1)
        pk_w.use_lagrange(ck, lck)
        pk_d.use_lagrange(ck, lck)
        sent = PR.prove(pk_w, ck, wit, pi)
        assert _same(sent, PR.prove(pk_d, ck, wit, pi)) and _same(sent, got[0])
        if name == "mixed":
            _pairing_verifier_accepts(oracle, pk_w, sent, n, pi)
    finally:
        pk_w.free()
        pk_d.free()


def _pairing_verifier_accepts(oracle, pk, sent, n, pub):
    """The oracle's verifier on the 1040 proof bytes (as tests/test_gpu_prover.py runs it at its smallest size)."""
    import plonk_prototype_amd.prover as PR
    from oracle import pairing_oracle as PG
    from oracle import plonk_verifier_oracle as PV

    def ints(limbs):
        return limbs_to_ints(oracle.fr_from_mont(np.ascontiguousarray(limbs).reshape(-1, 4)))

    def pt(xy):
        if not np.asarray(xy).any():
            return None
        v = limbs_to_ints(oracle.fp_from_mont(np.ascontiguousarray(xy).reshape(2, 6)))
        return (v[0], v[1])

    proof = PR.Proof.from_bytes(sent.native_bytes)
    vk = {k: pt(v) for k, v in pk.verifier_key.items()}
    comms = {k: pt(v) for k, v in proof.commitments.items()}
    ev = {k: ints(v)[0] for k, v in proof.evaluations.items()}
    ch0 = PR.derive_challenges(proof, pk.verifier_key, n, pub, t_eval=0)
    pub_z = B.horner(B.ifft(ints(pub), n.bit_length() - 1), ch0["z"])
    t_eval = PV.quotient_evaluation(n, ev, ch0, pub_z)
    ch = PR.derive_challenges(proof, pk.verifier_key, n, pub, t_eval=t_eval)
    assert PV.verify(n, vk, comms, ev, ch, pub_z, PG.g2_mul(TAU, PG.G2_GEN)) == (True, True)
    assert {k: ch[k] for k in sent.challenges} == sent.challenges


# ---------------------------------------------------------------------------------- 3. witness expansion
def _selectors(n):
    import plonk_prototype_amd as pa
    if ("sel", n) not in _CACHE:
        c, _, _ = pa.synthetic.chain_circuit(n, 9)
        _CACHE[("sel", n)] = {k: getattr(c, k) for k in pa.prover.SELECTORS}
    return _CACHE[("sel", n)]


@pytest.mark.parametrize("n,batch", [(4, 1), (4, 3), (1 << 12, 1), (1 << 12, 3)])
def test_witness_from_vars_is_numpy_indexing(ctx, n, batch):
    import plonk_prototype_amd as pa
    from plonk_prototype_amd.field import fr_to_limbs
    rng = np.random.default_rng(100 * n + batch)
    num_vars, stride = n + 3, n + 8                                # var_stride > num_vars
    wv = rng.integers(0, num_vars, size=(4, n), dtype=np.uint64).astype(np.uint32)
    wv[rng.random((4, n)) < 0.1] = NO_VAR
    wv[0, 0], wv[1, 1], wv[3, n - 1] = 0, 1, NO_VAR
    vals = rng.integers(0, 1 << 63, size=(batch, stride, 4), dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    vals[:, 0] = np.array([(R - 1) >> (64 * k) & (2**64 - 1) for k in range(4)], np.uint64)   # r - 1 as raw limbs
    vals[:, 1] = np.uint64(2**64 - 1)                              # not canonical: copied as it is
    vals[-1, 2] = fr_to_limbs(R - 1)
    pk = pa.ProverKey(pa.Circuit(wire_vars=wv, num_vars=num_vars, **_selectors(n)), ctx)
    d_vars = pa.DeviceVector.from_host(ctx, vals.reshape(-1, 4))
    out = pa.DeviceVector(ctx, batch * 4 * n)
    try:
        assert ctx._lib.pm_plonk_witness_from_vars_dev(ctx._h, pk._h, d_vars._p, stride, batch, out._p, None) == 0
        got = out.to_host().reshape(batch, 4 * n, 4)
        flat = wv.reshape(-1)
        hole = flat == NO_VAR
        want = vals[:, np.where(hole, 0, flat)]
        want[:, hole] = 0
        assert np.array_equal(got, want)
        assert not got[:, hole].any() and hole.sum() >= 1
        # the Python form: host [num_vars, 4] per assignment
        dv = pk.witness_from_variables([v[:num_vars] for v in vals] if batch > 1 else vals[0, :num_vars])
        assert dv.n == batch * 4 * n and np.array_equal(dv.to_host().reshape(batch, 4 * n, 4), want)
        dv.free()
    finally:
        out.free()
        d_vars.free()
        pk.free()


# ---------------------------------------------------------------------------------- 4. variables= end to end
def _arith_masks(circuit, w, pi):
    """The arithmetic bit of pm_plonk_check_witness's definition, row by row: q_arith (q_m a b + q_l a + q_r b + q_o c + q_4 d +
    q_c) + PI != 0.  w: 4n wire values (position j n + i) as integers."""
    from plonk_prototype_amd.field import fr_vec_from_limbs
    n = circuit.n
    q = {k: fr_vec_from_limbs(getattr(circuit, k)) for k in ("q_m", "q_l", "q_r", "q_o", "q_4", "q_c", "q_arith")}
    out = np.zeros(n, np.uint8)
    for i in range(n):
        a, b, c, d = w[i], w[n + i], w[2 * n + i], w[3 * n + i]
        arith = q["q_m"][i] * a * b + q["q_l"][i] * a + q["q_r"][i] * b + q["q_o"][i] * c + q["q_4"][i] * d + q["q_c"][i]
        out[i] = 1 if (q["q_arith"][i] * arith + pi[i]) % R else 0
    return out


def test_variables_end_to_end(ctx, oracle):
    import plonk_prototype_amd as pa
    from plonk_prototype_amd import _lib
    from plonk_prototype_amd.field import fr_from_limbs, fr_to_limbs, fr_vec_from_limbs
    PR, S = pa.prover, pa.synthetic
    n = 256
    circuit, variables, pi = S.chain_circuit_wires(n, 33)
    flat = circuit.wire_vars.reshape(-1)
    witness = variables[circuit.wire_vars]
    ck = _commit_key(ctx, n)
    pk = PR.preprocess(circuit, ctx, ck)
    try:
        proof = PR.prove(pk, ck, variables=variables, public_inputs=pi)
        assert _same(proof, PR.prove(pk, ck, witness, pi))
        d_vars = pa.DeviceVector.from_host(ctx, variables)
        assert _same(proof, PR.prove(pk, ck, variables=d_vars, public_inputs=pi))
        d_vars.free()
        pub_z = fr_from_limbs(oracle.fr_poly_evaluate(oracle.fr_ntt(pi, 8, pa.NTT_INVERSE), fr_to_limbs(proof.challenges["z"])))
        assert PR.check_identity(proof, n, pub_z)
        # three assignments of the one circuit: its selectors and wire map do not depend on the witness
        dense = S.chain_witnesses(n, 33, count=3, witness_seed=2)
        assigns, pis = [], [p for _, p in dense]
        for w, _ in dense:
            v = np.zeros((n + 1, 4), np.uint64)
            v[flat] = w.reshape(-1, 4)
            assert np.array_equal(v[circuit.wire_vars], w)
            assigns.append(v)
        got = PR.prove_batch(pk, ck, variables=assigns, public_inputs=pis)
        exp = PR.prove_batch(pk, ck, [w for w, _ in dense], pis)
        assert len(got) == 3 and all(_same(a, b) for a, b in zip(got, exp))
        # the check: enable_check takes no sigma_index on this key
        assert pk.enable_check() > 0 and pk._sigma_index is None
        rep = pk.check_witness(variables=variables, public_inputs=pi, masks=True)
        assert rep.ok and not rep.row_masks.any()
        reps = pk.check_witnesses(variables=assigns, public_inputs=pis, masks=True)
        assert len(reps) == 3 and all(r.ok and not r.row_masks.any() for r in reps)
        # one variable changed: every position of it moves together, so no copy constraint breaks; the gates that read it do
        bad = variables.copy()
        bad[100] = fr_to_limbs(fr_from_limbs(bad[100]) + 1)
        want = _arith_masks(circuit, fr_vec_from_limbs(bad[flat]), fr_vec_from_limbs(pi))
        assert 2 <= np.count_nonzero(want) <= 4
        rep = pk.check_witness(variables=bad, public_inputs=pi, masks=True)
        assert np.array_equal(rep.row_masks, want * _lib.PLONK_FAIL_ARITH)
        assert rep.counts["copy"] == 0 and rep.counts["arith"] == np.count_nonzero(want) == rep.failed_rows
        assert rep.first_row == int(np.flatnonzero(want)[0]) and rep.first_reasons == ("arith",)
        with pytest.raises(pa.UnsatisfiedWitness) as e:
            PR.prove(pk, ck, variables=bad, public_inputs=pi, check=True)
        assert e.value.report.first_row == rep.first_row
        with pytest.raises(pa.UnsatisfiedWitness) as e:
            PR.prove_batch(pk, ck, variables=[assigns[0], bad, assigns[2]], public_inputs=[pis[0], pi, pis[2]], check=True)
        assert list(e.value.reports) == [1]
        assert _same(PR.prove(pk, ck, variables=variables, public_inputs=pi, check=True), proof)
        # an index-built key of the same circuit still needs its sigma_index
        pk_d = PR.ProverKey(pa.Circuit(sigma_index=ref_sigma(flat).reshape(4, n),
                                       **{k: getattr(circuit, k) for k in PR.SELECTORS}), ctx)
        out = C.c_size_t()
        assert ctx._lib.pm_plonk_key_enable_check(ctx._h, pk_d._h, None, C.byref(out)) == _lib.PM_ERR_BAD_ARG
        assert pk_d.enable_check() > 0 and pk_d.check_witness(witness, pi).ok
        with pytest.raises(ValueError):
            pk_d.witness_from_variables(variables)
        pk_d.free()
    finally:
        pk.free()


# ---------------------------------------------------------------------------------- 5. refusals
def test_refusals_leave_the_key_and_the_context_usable(ctx):
    import plonk_prototype_amd as pa
    from plonk_prototype_amd import _lib
    PR, S = pa.prover, pa.synthetic
    lib, h = ctx._lib, ctx._h
    n = 64
    circuit, variables, pi = S.chain_circuit_wires(n, 8)
    ck = _commit_key(ctx, n)
    pk = PR.preprocess(circuit, ctx, ck)
    before = PR.prove(pk, ck, variables=variables, public_inputs=pi)
    sel = {k: getattr(circuit, k) for k in PR.SELECTORS}
    # an id equal to num_vars at two positions: the lower one is named
    for n_bad, spots in ((64, (3 * 64 + 17, 64 + 5)), (1 << 12, (3 * 4096 + 4000, 2 * 4096 + 9))):
        wv = _chain_vars(n_bad).astype(np.uint32)
        for p in spots:
            wv[p] = n_bad + 1
        rc, _ = _sigma(ctx, wv, n_bad + 1)
        assert rc == _lib.PM_ERR_BAD_ARG and f"position {min(spots)} " in lib.pm_last_error(h).decode()
    wv = circuit.wire_vars.copy()
    wv[2, 7] = wv[1, 3] = circuit.num_vars
    with pytest.raises(pa.Error) as e:
        PR.ProverKey(pa.Circuit(wire_vars=wv, num_vars=circuit.num_vars, **sel), ctx)
    assert e.value.code == _lib.PM_ERR_BAD_ARG and f"position {n + 3} " in str(e.value)
    # n = 12
    out12 = np.zeros(48, np.int64)
    assert lib.pm_plonk_sigma_from_wires(h, np.zeros(48, np.uint32).ctypes.data_as(_lib.u32p), 1, 12,
                                         out12.ctypes.data_as(C.POINTER(C.c_int64))) == _lib.PM_ERR_LENGTH
    key = C.c_void_p()
    ptrs = (_lib.u64p * len(PR.SELECTORS))()
    assert lib.pm_plonk_preprocess_wires(h, ptrs, np.zeros(48, np.uint32).ctypes.data_as(_lib.u32p), 1, 12,
                                         C.byref(key)) == _lib.PM_ERR_LENGTH and not key.value
    assert lib.pm_plonk_sigma_from_wires(h, None, 1, 16, out12.ctypes.data_as(C.POINTER(C.c_int64))) == _lib.PM_ERR_BAD_ARG
    # the expansion
    d_vars = pa.DeviceVector.from_host(ctx, np.tile(variables, (2, 1)))
    d_out = pa.DeviceVector(ctx, 65 * 4 * n)
    pk_d = PR.ProverKey(S.chain_circuit(n, 8)[0], ctx)
    expand = lambda key, stride, batch: lib.pm_plonk_witness_from_vars_dev(h, key._h, d_vars._p, stride, batch, d_out._p, None)   # noqa: E731
    assert expand(pk_d, n + 1, 1) == _lib.PM_ERR_BAD_ARG and "wire variables" in lib.pm_last_error(h).decode()
    assert expand(pk, n + 1, 0) == _lib.PM_ERR_BAD_ARG
    assert expand(pk, n + 1, 65) == _lib.PM_ERR_BAD_ARG
    assert expand(pk, n, 1) == _lib.PM_ERR_BAD_ARG and "var_stride" in lib.pm_last_error(h).decode()
    assert lib.pm_plonk_witness_from_vars_dev(h, pk._h, None, n + 1, 1, d_out._p, None) == _lib.PM_ERR_BAD_ARG
    assert expand(pk, n + 1, 2) == 0
    # both forms at once, or neither
    witness = variables[circuit.wire_vars]
    for call in (lambda: PR.prove(pk, ck, witness, pi, variables=variables),
                 lambda: PR.prove(pk, ck, public_inputs=pi),
                 lambda: PR.prove_batch(pk, ck, [witness], [pi], variables=[variables]),
                 lambda: pk.check_witness(witness, pi, variables=variables),
                 lambda: pk.check_witnesses([witness], [pi], variables=[variables]),
                 lambda: PR.prove(pk_d, ck, variables=variables, public_inputs=pi)):
        with pytest.raises(ValueError):
            call()
    after = PR.prove(pk, ck, variables=variables, public_inputs=pi)
    assert _same(after, before)
    fresh = PR.ProverKey(S.chain_circuit(n, 8)[0], ctx)
    assert _same(PR.prove(pk_d, ck, witness, pi), PR.prove(fresh, ck, witness, pi))
    fresh.free()
    for v in (d_vars, d_out):
        v.free()
    pk.free()
    pk_d.free()
