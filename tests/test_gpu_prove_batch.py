"""The batch prover (pm_plonk_prove_batch): B proofs of one circuit in one call, each byte-identical -- challenges
included -- to pm_plonk_prove of the same witness and public inputs, in both transcript modes, with and without a
Lagrange-form key; no cross-talk between the slots; the workspace's reuse, its size, and every refusal of the contract."""
import ctypes as C

import numpy as np
import pytest

from oracle import bigint_oracle as B
from oracle.cpu_oracle import ints_to_limbs

pytestmark = pytest.mark.gpu
R = B.R_MOD
TAU = 0x1F2E3D4C5B6A79880123456789ABCDEF0FEDCBA9876543210A1B2C3D4E5F6071 % R
_CK: dict = {}


def _mont(oracle, v):
    return oracle.fr_to_mont(ints_to_limbs([v % R], 4))[0]


def _ck(ctx, oracle, log_n):
    """One commit key of 2^log_n powers at a time (the 2^20 one is large)."""
    import plonk_prototype_amd as pa
    if log_n not in _CK:
        _CK.clear()
        _CK[log_n] = pa.CommitKey.setup((1 << log_n) - 1, _mont(oracle, TAU), ctx, precompute=log_n >= 10)
    return _CK[log_n]


def _pi_variants(n, pis):
    """Proof b's public inputs as prove() takes them: dense, none, and (for b % 3 == 2) a list of more than 16
    (position, value) pairs with repeats -- the staged-scatter path, where a repeated position keeps its last value."""
    out = []
    for b, pi in enumerate(pis):
        if b % 3 == 2:
            pos = np.flatnonzero(pi.any(axis=1)).astype(np.uint64)
            extra = np.arange(min(n, 8), dtype=np.uint64)
            junk = np.tile(np.arange(1, 5, dtype=np.uint64), (extra.size, 1))
            allpos = np.concatenate([extra, pos, extra, np.arange(n, dtype=np.uint64)[:20]])
            dense = np.asarray(pi, np.uint64)
            vals = np.concatenate([junk, dense[pos.astype(np.int64)], dense[extra.astype(np.int64)],
                                   dense[:20]])
            out.append((allpos, vals))
        else:
            out.append(pi)
    return out


def _singles(pk, ck, wits, pis, bind):
    import plonk_prototype_amd.prover as PR
    return [PR.prove(pk, ck, w, p, bind_public_inputs=bind) for w, p in zip(wits, pis)]


def _same(batch, singles):
    assert len(batch) == len(singles)
    for b, (x, y) in enumerate(zip(batch, singles)):
        assert x.native_bytes == y.native_bytes, f"proof {b}: bytes differ"
        assert x.challenges == y.challenges, f"proof {b}: challenges differ"


def _check_batch(pk, ck, wits, pis, binds=(True, False), ws=None):
    import plonk_prototype_amd.prover as PR
    for bind in binds:
        got = PR.prove_batch(pk, ck, list(wits), list(pis), bind_public_inputs=bind, workspace=ws)
        _same(got, _singles(pk, ck, wits, pis, bind))


@pytest.mark.parametrize("log_n", [4, 8, 12])
def test_chain_batches_equal_single_proofs(ctx, oracle, log_n):
    import plonk_prototype_amd as pa
    n = 1 << log_n
    ck = _ck(ctx, oracle, 12)
    circuit, _, _ = pa.synthetic.chain_circuit(n, 21)
    pk = pa.preprocess(circuit, ctx, ck)
    ws = pk.batch(16)
    for batch in (1, 2, 5, 16):
        rows = [(0,), (), tuple(range(0, n, max(1, n // 24))), (1, 2)] * 4
        pairs = pa.synthetic.chain_witnesses(n, 21, count=batch, witness_seed=batch, public_rows=rows[:batch])
        wits = [w for w, _ in pairs]
        pis = _pi_variants(n, [p for _, p in pairs])
        _check_batch(pk, ck, wits, pis, ws=ws)
    ws.free()
    pk.free()


@pytest.mark.parametrize("lagrange", [False, True])
def test_boolean_batch_with_and_without_lagrange_key(ctx, oracle, lagrange):
    import plonk_prototype_amd as pa
    n = 1 << 12
    ck = _ck(ctx, oracle, 12)
    made = [pa.synthetic.boolean_circuit(n, s) for s in (1, 2, 3, 4, 5)]
    pk = pa.preprocess(made[0][0], ctx, ck)
    if lagrange:
        lck = ck.lagrange(12)
        pk.use_lagrange(ck, lck)
    _check_batch(pk, ck, [m[1] for m in made], [m[2] for m in made])
    # one DeviceVector of B x 4n elements, proof-major
    flat = pa.DeviceVector.from_host(ctx, np.concatenate([m[1].reshape(4 * n, 4) for m in made]))
    got = pa.prove_batch(pk, ck, flat, [None] * 5)
    _same(got, _singles(pk, ck, [m[1] for m in made], [None] * 5, True))
    flat.free()
    pk.free()


@pytest.mark.parametrize("n", [32, 128])
def test_mixed_circuit_batches_every_widget(ctx, oracle, n):
    import plonk_prototype_amd as pa
    ck = _ck(ctx, oracle, 12)
    circuit, wit, pub = pa.synthetic.mixed_circuit(n, 7)
    pk = pa.preprocess(circuit, ctx, ck)
    _check_batch(pk, ck, [wit] * 3, [pub, pub, pub])
    pk.free()


def test_wide_mixed_circuit_batch_from_device_witnesses(ctx, oracle):
    import plonk_prototype_amd as pa
    n = 1 << 10
    ck = _ck(ctx, oracle, 12)
    circuit, d_wit, _ = pa.synthetic.wide_mixed_circuit(n, ctx, seed=3)
    pk = pa.preprocess(circuit, ctx, ck)
    got = pa.prove_batch(pk, ck, [d_wit, d_wit])          # a list of DeviceVectors: copied into the staging
    _same(got, _singles(pk, ck, [d_wit, d_wit], [None, None], True))
    d_wit.free()
    pk.free()


def test_no_cross_talk_between_slots(ctx, oracle):
    import plonk_prototype_amd as pa
    import plonk_prototype_amd.prover as PR
    n = 256
    ck = _ck(ctx, oracle, 12)
    circuit, _, _ = pa.synthetic.chain_circuit(n, 33)
    pk = pa.preprocess(circuit, ctx, ck)
    pairs = pa.synthetic.chain_witnesses(n, 33, count=5, witness_seed=4, public_rows=())
    wits = [w.copy() for w, _ in pairs]
    k = 2
    wits[k][0, 17] = pa.field.fr_to_limbs(12345)             # a at gate 17: the gate equation fails there
    got = PR.prove_batch(pk, ck, wits, None)
    single_k = PR.prove(pk, ck, wits[k], None)
    assert got[k].native_bytes == single_k.native_bytes
    assert not PR.check_identity(got[k], n)
    for b in range(5):
        if b != k:
            assert got[b].native_bytes == PR.prove(pk, ck, pairs[b][0], None).native_bytes
            assert PR.check_identity(got[b], n)
    pk.free()


def test_2_16_batch_of_16(ctx, oracle):
    import plonk_prototype_amd as pa
    n = 1 << 16
    ck = _ck(ctx, oracle, 16)
    made = [pa.synthetic.boolean_circuit(n, s) for s in range(1, 17)]
    pk = pa.preprocess(made[0][0], ctx, ck)
    _check_batch(pk, ck, [m[1] for m in made], [m[2] for m in made], binds=(True,))
    pk.free()


def test_2_20_batch_of_2(ctx, oracle):
    import plonk_prototype_amd as pa
    n = 1 << 20
    ck = _ck(ctx, oracle, 20)
    made = [pa.synthetic.boolean_circuit(n, s) for s in (1, 2)]
    pk = pa.preprocess(made[0][0], ctx, ck)
    _check_batch(pk, ck, [m[1] for m in made], [m[2] for m in made], binds=(True,))
    pk.free()
    _CK.clear()


def test_batch_member_passes_the_pairing_verifier(ctx, oracle):
    import plonk_prototype_amd as pa
    import plonk_prototype_amd.prover as PR
    from oracle import pairing_oracle as PG
    from oracle import plonk_verifier_oracle as PV
    from oracle.cpu_oracle import limbs_to_ints
    n = 1 << 12
    ck = _ck(ctx, oracle, 12)
    circuit, _, _ = pa.synthetic.chain_circuit(n, 51)
    pairs = pa.synthetic.chain_witnesses(n, 51, count=4, witness_seed=8, public_rows=[(0,), (3, 9), (), (0,)])
    pk = pa.preprocess(circuit, ctx, ck)
    proofs = PR.prove_batch(pk, ck, [w for w, _ in pairs], [p for _, p in pairs])
    b = 1
    proof, pub = PR.Proof.from_bytes(proofs[b].native_bytes), pairs[b][1]

    def pt(xy):
        if not np.asarray(xy).any():
            return None
        v = limbs_to_ints(oracle.fp_from_mont(np.ascontiguousarray(xy).reshape(2, 6)))
        return (v[0], v[1])

    def fr(v):
        return limbs_to_ints(oracle.fr_from_mont(np.ascontiguousarray(v).reshape(-1, 4)))

    vk = {k: pt(v) for k, v in pk.verifier_key.items()}
    comms = {k: pt(v) for k, v in proof.commitments.items()}
    ev = {k: fr(v)[0] for k, v in proof.evaluations.items()}
    ch0 = PR.derive_challenges(proof, pk.verifier_key, n, pub, t_eval=0)
    pub_z = B.horner(B.ifft(fr(pub), 12), ch0["z"])
    t_eval = PV.quotient_evaluation(n, ev, ch0, pub_z)
    ch = PR.derive_challenges(proof, pk.verifier_key, n, pub, t_eval=t_eval)
    assert PV.verify(n, vk, comms, ev, ch, pub_z, PG.g2_mul(TAU, PG.G2_GEN)) == (True, True)
    pk.free()


def test_one_workspace_many_calls_and_max_batch_64(ctx, oracle):
    import plonk_prototype_amd as pa
    import plonk_prototype_amd.prover as PR
    n = 1 << 12
    ck = _ck(ctx, oracle, 12)
    circuit, _, _ = pa.synthetic.chain_circuit(n, 61)
    pk = pa.preprocess(circuit, ctx, ck)
    ws = pk.batch(64)
    pairs = pa.synthetic.chain_witnesses(n, 61, count=64, witness_seed=5)
    wits, pis = [w for w, _ in pairs], [p for _, p in pairs]
    singles = _singles(pk, ck, wits, pis, True)
    for batch in (3, 64, 1, 17):                              # 64 x 4 wires: four MSM passes in round 1
        got = PR.prove_batch(pk, ck, wits[:batch], pis[:batch], workspace=ws)
        _same(got, singles[:batch])
    # the key's own workspace is untouched: single proofs still match afterwards
    _same([PR.prove(pk, ck, wits[0], pis[0])], singles[:1])
    ws.free()
    pk.free()


def _raw_prove_batch(ctx, pk, ws_h, ck, batch, d_wit, n_pi=None, pos=None, vals=None, flags=0):
    from plonk_prototype_amd import _lib
    raws = (_lib.PlonkProof * max(batch, 1))()
    return ctx._lib.pm_plonk_prove_batch(ctx._h, pk._h, ws_h, ck._bases._h, batch, d_wit._p, pos, vals, n_pi, flags, raws)


def test_refusals(ctx, oracle):
    import plonk_prototype_amd as pa
    from plonk_prototype_amd import _lib
    n = 64
    ck = _ck(ctx, oracle, 12)
    circuit, wit, _ = pa.synthetic.chain_circuit(n, 71)
    pk = pa.preprocess(circuit, ctx, ck)
    other = pa.preprocess(pa.synthetic.chain_circuit(n, 72)[0], ctx, ck)
    uncommitted = pa.ProverKey(circuit, ctx)
    ws = pk.batch(4)
    d = pa.DeviceVector.from_host(ctx, np.concatenate([wit.reshape(4 * n, 4)] * 4))

    def err(rc):
        return rc, ctx._lib.pm_last_error(ctx._h).decode()

    assert _raw_prove_batch(ctx, pk, ws._h, ck, 0, d) == _lib.PM_ERR_BAD_ARG
    rc, msg = err(_raw_prove_batch(ctx, pk, ws._h, ck, 5, d))
    assert rc == _lib.PM_ERR_BAD_ARG and "max_batch" in msg
    rc, msg = err(_raw_prove_batch(ctx, other, ws._h, ck, 1, d))
    assert rc == _lib.PM_ERR_BAD_ARG and "another key" in msg
    ws_u = pa.prover.BatchWorkspace(uncommitted, 2)
    rc, msg = err(_raw_prove_batch(ctx, uncommitted, ws_u._h, ck, 1, d))
    assert rc == _lib.PM_ERR_BAD_ARG and "committed" in msg
    rc, msg = err(_raw_prove_batch(ctx, pk, ws._h, ck, 1, d, flags=3))
    assert rc == _lib.PM_ERR_BAD_ARG and "exclude" in msg
    counts = (C.c_size_t * 2)(0, 1)
    pos_arr = np.array([n], np.uint64)
    val_arr = np.zeros((1, 4), np.uint64)
    pp = (_lib.u64p * 2)(None, pos_arr.ctypes.data_as(_lib.u64p))
    vv = (_lib.u64p * 2)(None, val_arr.ctypes.data_as(_lib.u64p))
    rc, msg = err(_raw_prove_batch(ctx, pk, ws._h, ck, 2, d, counts, pp, vv))
    assert rc == _lib.PM_ERR_LENGTH and "position" in msg
    with pytest.raises(pa.Error) as e:
        pk.batch(0)
    assert e.value.code == _lib.PM_ERR_BAD_ARG
    with pytest.raises(pa.Error) as e:
        pk.batch(65)
    assert e.value.code == _lib.PM_ERR_BAD_ARG
    # the handle still works after every refusal (none of them left it busy)
    got = pa.prove_batch(pk, ck, d, None, workspace=ws)
    assert all(p.native_bytes == got[0].native_bytes for p in got)
    for h in (ws, ws_u):
        h.free()
    d.free()
    for k in (pk, other, uncommitted):
        k.free()


def test_workspace_bytes_are_what_free_returns(ctx, oracle):
    import torch
    import plonk_prototype_amd as pa
    n = 1 << 14
    circuit, _, _ = pa.synthetic.boolean_circuit(n, 1)
    pk = pa.preprocess(circuit, ctx, _ck(ctx, oracle, 16))
    ctx.sync()
    free0 = torch.cuda.mem_get_info(0)[0]
    ws = pk.batch(16)
    nbytes = ws.device_bytes()
    assert 42 * 16 * n * 32 <= nbytes <= 42 * 16 * n * 32 + (64 << 20)
    free1 = torch.cuda.mem_get_info(0)[0]
    ws.free()
    free2 = torch.cuda.mem_get_info(0)[0]
    slack = 4 << 20
    assert free0 - free1 >= nbytes - slack and free0 - free1 <= nbytes + slack
    assert abs(free2 - free0) <= slack
    pk.free()


def test_workspace_that_does_not_fit_is_oom(ctx):
    import plonk_prototype_amd as pa
    from plonk_prototype_amd import _lib
    n = 1 << 22                       # 64 proofs x ~42 n x 32 bytes = 360 GB: more than the device holds
    circuit, d_wit, _ = pa.synthetic.wide_circuit(n, ctx, seed=2)
    d_wit.free()
    pk = pa.ProverKey(circuit, ctx)
    with pytest.raises(pa.Error) as e:
        pk.batch(64)
    assert e.value.code == _lib.PM_ERR_OOM
    assert "does not fit" in ctx._lib.pm_last_error(ctx._h).decode()
    pk.free()
    # the refused allocation leaves nothing behind: the next kernel launch on the context is clean
    out = pa.DeviceVector(ctx, 8)
    ctx.fr_powers(pa.field.fr_to_limbs(3), pa.field.fr_to_limbs(1), 8, out.ptr)
    assert pa.field.fr_vec_from_limbs(out.to_host()) == [pow(3, i, R) for i in range(8)]
    out.free()
