"""The memory AROUND a call's buffers, group C: the native JubJub, Poseidon, Merkle and Schnorr calls, whose entry prologues and
scratch handling share csrc/context.h.  The method is that of tests/test_gpu_buffer_contract.py: every buffer is a region of one
guard arena (tests/guard_arena.py), carved at exactly the size the header documents -- n x 64 bytes of points, k x 4 bytes of
status words, k x 8 bytes of indices, (4^height - 1) / 3 tree nodes, pm_poseidon_merkle_update_work_bytes(k) of scratch -- the
arena is downloaded once, bands and read-only inputs must be untouched, and the outputs equal the big-integer models of
tests/*_model.py bit for bit.  Where the header refuses an overlap, the code and an unchanged arena are asserted."""
import ctypes as C
import os
import random
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gadget_model as M  # noqa: E402
import guard_arena as G  # noqa: E402
import hades_model as HM  # noqa: E402
import jubjub_model as J  # noqa: E402
import jubjub_msm_model as MM  # noqa: E402
import merkle_update_model as MU  # noqa: E402
import poseidon_model as PM  # noqa: E402
import schnorr_model as S  # noqa: E402
import test_gpu_jubjub as TJ  # noqa: E402    (the shared scalars, points and products, computed once a session)
import test_gpu_schnorr as TS  # noqa: E402   (the rig and the corrupted batch)

pytestmark = pytest.mark.gpu
R, Q = J.R, J.Q
SIZES = (1, 63, 64, 65, 130)              # the SIZES of tests/test_gpu_jubjub.py from one lane to more than two waves
NMAX = max(SIZES)
FORMS = ("auto", "thread", "wave")
SHAPE = "5_2_per_round"                  # 5 rounds, a matrix per round: every code path of the kernels, a cheap model
FILL_WORD = int.from_bytes(bytes([G.FILL]) * 8, "little")
_CACHE = {}


def _points(raw, n):
    return G.as_u64(raw, n, 2, 4)


def _refused(pa, call):
    with pytest.raises(pa.Error) as e:
        call()
    assert e.value.code == pa._lib.PM_ERR_BAD_ARG


@pytest.fixture(scope="module")
def hades(ctx):
    import plonk_prototype_amd as pa
    h = S.Hades(SHAPE)
    dev = pa.Hades(ctx, M.to_limbs(h.flat_ark), M.to_limbs(h.flat_mds), h.rounds, h.full)
    yield types.SimpleNamespace(dev=dev, model=h, args=(h.ark, h.mds, h.rounds, h.full))
    dev.free()


@pytest.fixture(scope="module")
def bases(ctx):
    import plonk_prototype_amd as pa
    g, h = pa.JubJubBase(ctx, J.GENERATOR), pa.JubJubBase(ctx, TJ.ODD)
    yield g, h
    g.free(), h.free()


# ---------------------------------------------------------------------------------- JubJub
@pytest.mark.parametrize("n", SIZES)
def test_jubjub_fixed_mul(ctx, bases, n):
    want = J.to_limbs(TJ._products(J.GENERATOR)[:n])
    with G.GuardArena.of(ctx, sc=TJ._mont(TJ._scalars(n)), out=64 * n) as ar:
        bases[0].mul_dev(ar.addr("sc"), n, ar.addr("out"))
        assert np.array_equal(_points(ar.check()["out"], n), want), n


def _commit_case():
    """the values, blinders and commitments of tests/test_gpu_jubjub.py::test_commit"""
    if "commit" not in _CACHE:
        sc = TJ._scalars()
        v = [0, sc[20], 0] + sc[:NMAX - 3]
        bl = [sc[21], 0, 0] + list(reversed(sc))[:NMAX - 3]
        pg, ph = dict(zip(sc, TJ._products(J.GENERATOR))), dict(zip(sc, TJ._products(TJ.ODD)))
        _CACHE["commit"] = (v, bl, J.to_limbs([J.add(pg[x], ph[y]) for x, y in zip(v, bl)]))
    return _CACHE["commit"]


@pytest.mark.parametrize("n", SIZES)
def test_jubjub_commit(ctx, bases, n):
    import plonk_prototype_amd as pa
    v, bl, want = _commit_case()
    with G.GuardArena.of(ctx, v=TJ._mont(v[:n]), bl=TJ._mont(bl[:n]), out=64 * n) as ar:
        pa.jubjub_commit_dev(bases[0], bases[1], ar.addr("v"), ar.addr("bl"), n, ar.addr("out"))
        assert np.array_equal(_points(ar.check()["out"], n), want[:n]), n


@pytest.mark.parametrize("n", SIZES)
def test_jubjub_mul(ctx, n):
    """out of place with the points unchanged, and "d_out_xy == d_points_xy is allowed" """
    import plonk_prototype_amd as pa
    ps, ss, want = TJ._var_case()
    pts, sc, want = J.to_limbs(ps[:n]), TJ._mont(ss[:n]), J.to_limbs(want[:n])
    with G.GuardArena.of(ctx, pts=pts, sc=sc, out=64 * n) as ar:
        pa.jubjub_mul_dev(ctx, ar.addr("pts"), ar.addr("sc"), n, ar.addr("out"))
        assert np.array_equal(_points(ar.check()["out"], n), want), (n, "out of place")
    with G.GuardArena.of(ctx, pts=pts, sc=sc) as ar:
        pa.jubjub_mul_dev(ctx, ar.addr("pts"), ar.addr("sc"), n, ar.addr("pts"))
        assert np.array_equal(_points(ar.check(written={"pts"})["pts"], n), want), (n, "in place")


@pytest.mark.parametrize("n", SIZES)
def test_jubjub_check_reads_only(ctx, n):
    pts = J.edge_points()
    good = J.to_limbs([pts[i % len(pts)] for i in range(n)])
    bad = good.copy()
    bad[n - 1] = J.to_limbs([(pts[0][0], pts[0][1] + 1)])[0]
    assert not J.on_curve((pts[0][0], pts[0][1] + 1))
    for data, want in ((good, n), (bad, n - 1)):
        with G.GuardArena.of(ctx, pts=data) as ar:
            first = C.c_size_t(12345)
            ctx._check(ctx._lib.pm_jubjub_check_dev(ctx._h, C.c_void_p(ar.addr("pts")), n, C.byref(first), None))
            assert first.value == want
            assert ar.check() == {}


def _msm_rows(n):
    """three scalar vectors over the n edge points of jubjub_msm_model: its edge scalars, 16-bit scalars, all ones"""
    pts, sc, want0 = MM.edge_case(n)
    if ("msm", n) not in _CACHE:
        rng = random.Random(3 + n)
        small = [rng.randrange(1 << 16) for _ in range(n)]
        _CACHE["msm", n] = ([sc, small, [1] * n], J.to_limbs([want0, MM.msm(pts, small), MM.psum(pts)]))
    return (pts,) + _CACHE["msm", n]


@pytest.mark.parametrize("n", SIZES)
def test_jubjub_msm_padded_batch(ctx, n):
    """batch 3 with scalar_stride = n + 3: the scalar region ends with the last vector, the padding between two vectors holds
    0xA5 words (no scalar: above r) and must not reach the sums"""
    import plonk_prototype_amd as pa
    pts, rows, want = _msm_rows(n)
    stride, batch = n + 3, 3
    sc = np.full(((batch - 1) * stride + n, 4), FILL_WORD, np.uint64)
    for b, row in enumerate(rows):
        sc[b * stride:b * stride + n] = S.scalar_words(row, True)
    with G.GuardArena.of(ctx, pts=J.to_limbs(pts), sc=sc, out=64 * batch) as ar:
        pa.jubjub_msm_dev(ctx, ar.addr("pts"), ar.addr("sc"), n, ar.addr("out"), batch, stride)
        assert np.array_equal(_points(ar.check()["out"], batch), want), n


def test_jubjub_msm_refuses_an_output_on_an_input(ctx):
    """"d_out_xy overlapping an input": PM_ERR_BAD_ARG, on the points, on the scalars, and one byte into either"""
    import plonk_prototype_amd as pa
    n, batch = 65, 3
    pts, rows, _ = _msm_rows(n)
    sc = np.concatenate([S.scalar_words(row, True) for row in rows])
    with G.GuardArena.of(ctx, pts=J.to_limbs(pts), sc=sc) as ar:
        for out in (ar.addr("pts"), ar.addr("sc"), ar.addr("pts") + 64 * n - 16, ar.addr("sc") + 32 * batch * n - 16,
                    ar.addr("sc") - 64 * batch + 16):
            _refused(pa, lambda: pa.jubjub_msm_dev(ctx, ar.addr("pts"), ar.addr("sc"), n, out, batch, n))
        ar.check_unchanged()


# ---------------------------------------------------------------------------------- Hades, the sponge
def _states():
    if "states" not in _CACHE:
        rng = random.Random(0x4841)
        h = S.Hades(SHAPE)
        st = [[0] * 5, [R - 1] * 5] + [[rng.randrange(R) for _ in range(5)] for _ in range(NMAX - 2)]
        _CACHE["states"] = (st, [HM.hades_model(s, h.ark, h.mds, h.rounds, h.full) for s in st])
    return _CACHE["states"]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", SIZES)
def test_hades_permute_in_place(ctx, hades, n, form):
    st, want = _states()
    with G.GuardArena.of(ctx, st=HM.to_limbs([x for s in st[:n] for x in s])) as ar:
        hades.dev.permute_dev(ar.addr("st"), n, form)
        got = G.as_u64(ar.check(written={"st"})["st"], 5 * n, 4)
        assert np.array_equal(got, HM.to_limbs([x for s in want[:n] for x in s])), (n, form)


MSG_LEN, MSG_STRIDE = 6, 9               # two chunks, the second one short; three elements of padding a message


def _messages():
    if "msgs" not in _CACHE:
        rng = random.Random(0x4D53)
        h = S.Hades(SHAPE)
        msgs = [[rng.randrange(R) for _ in range(MSG_LEN)] for _ in range(NMAX)]
        msgs[0], msgs[1] = [0] * MSG_LEN, [R - 1] * MSG_LEN
        _CACHE["msgs"] = (msgs, [h.hash(m) for m in msgs])
    return _CACHE["msgs"]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", SIZES)
def test_poseidon_hash_padded_messages(ctx, hades, n, form):
    """msg_stride > msg_len: the region ends with the last message, the padding holds 0xA5; n elements of output"""
    msgs, want = _messages()
    buf = np.full(((n - 1) * MSG_STRIDE + MSG_LEN, 4), FILL_WORD, np.uint64)
    for i in range(n):
        buf[i * MSG_STRIDE:i * MSG_STRIDE + MSG_LEN] = HM.to_limbs(msgs[i])
    with G.GuardArena.of(ctx, msgs=buf, out=32 * n) as ar:
        hades.dev.hash_dev(ar.addr("msgs"), MSG_LEN, n, ar.addr("out"), msg_stride=MSG_STRIDE, form=form)
        assert np.array_equal(G.as_u64(ar.check()["out"], n, 4), HM.to_limbs(want[:n])), (n, form)


def test_poseidon_hash_refuses_an_output_on_the_messages(ctx, hades):
    """"d_out must not overlap d_msgs" """
    import plonk_prototype_amd as pa
    n = 65
    msgs, _ = _messages()
    buf = HM.to_limbs([x for m in msgs[:n] for x in m])
    with G.GuardArena.of(ctx, msgs=buf) as ar:
        for out in (ar.addr("msgs"), ar.addr("msgs") + 32 * (n * MSG_LEN - 1), ar.addr("msgs") - 32 * (n - 1)):
            _refused(pa, lambda: hades.dev.hash_dev(ar.addr("msgs"), MSG_LEN, n, out))
        ar.check_unchanged()


# ---------------------------------------------------------------------------------- the Merkle tree
def _tree(height):
    """leaves and levels of the model's tree, once a height"""
    if ("tree", height) not in _CACHE:
        rng = random.Random(0x7EE + height)
        h = S.Hades(SHAPE)
        leaves = [rng.randrange(R) for _ in range(4 ** height)]
        leaves[0], leaves[-1] = 0, R - 1
        _CACHE["tree", height] = PM.tree(leaves, h.ark, h.mds, h.rounds, h.full)
    return _CACHE["tree", height]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("height", [1, 3])
def test_poseidon_merkle(ctx, hades, height, form):
    """the tree region is EXACTLY (4^height - 1) / 3 elements: the root is its last element, the band begins behind it"""
    levels = _tree(height)
    nodes = (4 ** height - 1) // 3
    with G.GuardArena.of(ctx, leaves=HM.to_limbs(levels[0]), tree=32 * nodes) as ar:
        hades.dev.merkle_dev(ar.addr("leaves"), height, ar.addr("tree"), form=form)
        assert np.array_equal(G.as_u64(ar.check()["tree"], nodes, 4), HM.to_limbs(PM.flat_tree(levels))), (height, form)


def test_poseidon_merkle_refuses_a_tree_on_the_leaves(ctx, hades):
    """the tree "must not overlap the leaves" """
    import plonk_prototype_amd as pa
    height = 3
    levels = _tree(height)
    with G.GuardArena.of(ctx, leaves=HM.to_limbs(levels[0])) as ar:
        for tree in (ar.addr("leaves"), ar.addr("leaves") + 32 * (4 ** height - 1), ar.addr("leaves") - 32 * 20):
            _refused(pa, lambda: hades.dev.merkle_dev(ar.addr("leaves"), height, tree))
        ar.check_unchanged()


HEIGHT = 4                                # 256 leaves: room for 65 distinct indices


def _indices(k):
    """k strictly ascending leaf indices, the first and the last leaf among them"""
    top = 4 ** HEIGHT - 1
    if k == 1:
        return [top]
    return sorted([0, top] + random.Random(0x1D + k).sample(range(1, top), k - 2))


def _tree_handle(pa, ctx, hades, ar):
    """pa.MerkleTree over two regions of the arena"""
    return pa.MerkleTree(ctx, types.SimpleNamespace(ptr=ar.addr("leaves")), types.SimpleNamespace(ptr=ar.addr("tree")), HEIGHT,
                         hades=hades.dev)


@pytest.mark.parametrize("k", [1, 5, 65])
def test_poseidon_merkle_paths(ctx, hades, k):
    """k x 8 bytes of indices in, k x height x 4 elements out; leaves and tree are read only"""
    import plonk_prototype_amd as pa
    levels, idx = _tree(HEIGHT), _indices(k)
    with G.GuardArena.of(ctx, leaves=HM.to_limbs(levels[0]), tree=HM.to_limbs(PM.flat_tree(levels)), idx=np.array(idx, np.uint64),
                         out=32 * k * HEIGHT * 4) as ar:
        _tree_handle(pa, ctx, hades, ar).paths_dev(ar.addr("idx"), k, ar.addr("out"))
        want = HM.to_limbs([x for path in PM.paths(levels, idx) for four in path for x in four])
        assert np.array_equal(G.as_u64(ar.check()["out"], k * HEIGHT * 4, 4), want), k


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("k", [1, 5, 65])
def test_poseidon_merkle_verify(ctx, hades, k, form):
    """k uint32 of status, exactly: good paths, an index that is not below 4^height, a broken link at every level -- the last
    path, whose status word ends the region, is always one of the bad ones when k > 1"""
    levels, idx = _tree(HEIGHT), _indices(k)
    paths = PM.paths(levels, idx)
    root = levels[HEIGHT][0]
    if k > 1:
        idx[1] = 4 ** HEIGHT + 7                                       # PM_MERKLE_PATH_INDEX
        for j in list(range(2, min(k, 6))) + ([k - 1] if k > 6 else []):
            l = (j - 2) % HEIGHT                                       # a sibling of the path node changes: the link above l breaks
            sibling = ((idx[j] >> (2 * l)) & 3) ^ 1
            paths[j][l][sibling] = (paths[j][l][sibling] + 1) % R
    want = [MU.verify(p, i, root, *hades.args) for p, i in zip(paths, idx)]
    assert want[0] == MU.PATH_OK and (k == 1 or (want[1] == MU.PATH_INDEX and want[k - 1] >= MU.PATH_LINK))
    assert k < 6 or {MU.PATH_LINK + l for l in range(HEIGHT)} <= set(want)
    with G.GuardArena.of(ctx, paths=HM.to_limbs([x for path in paths for four in path for x in four]), idx=np.array(idx, np.uint64),
                         root=HM.to_limbs([root]), status=4 * k) as ar:
        hades.dev.verify_paths_dev(ar.addr("paths"), ar.addr("idx"), k, HEIGHT, ar.addr("root"), ar.addr("status"), form=form)
        assert ar.check()["status"].view(np.uint32).tolist() == want, (k, form)


def test_poseidon_merkle_verify_refuses_a_status_on_an_input(ctx, hades):
    """"d_status must not overlap an input" """
    import plonk_prototype_amd as pa
    k = 5
    levels, idx = _tree(HEIGHT), _indices(k)
    paths = PM.paths(levels, idx)
    with G.GuardArena.of(ctx, paths=HM.to_limbs([x for path in paths for four in path for x in four]), idx=np.array(idx, np.uint64),
                         root=HM.to_limbs([levels[HEIGHT][0]])) as ar:
        for status in (ar.addr("paths"), ar.addr("idx"), ar.addr("root"), ar.addr("root") + 16, ar.addr("idx") + 32):
            _refused(pa, lambda: hades.dev.verify_paths_dev(ar.addr("paths"), ar.addr("idx"), k, HEIGHT, ar.addr("root"), status))
        ar.check_unchanged()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("k", [1, 5, 65])
def test_poseidon_merkle_update(ctx, hades, k, form):
    """leaves and tree are regions of their own: the update writes k leaves and their ancestors and "nothing else" -- not the
    bands around them, not the indices and values; d_work is carved at pm_poseidon_merkle_update_work_bytes(k) exactly"""
    import plonk_prototype_amd as pa
    levels, idx = [list(level) for level in _tree(HEIGHT)], _indices(k)
    rng = random.Random(0x0D + k)
    values = [rng.randrange(R) for _ in range(k)]
    values[0] = R - 1
    work = ctx._lib.pm_poseidon_merkle_update_work_bytes(k)
    assert work > 0
    with G.GuardArena.of(ctx, leaves=HM.to_limbs(levels[0]), tree=HM.to_limbs(PM.flat_tree(levels)), idx=np.array(idx, np.uint64),
                         values=HM.to_limbs(values), work=work) as ar:
        hashed = _tree_handle(pa, ctx, hades, ar).update_dev(ar.addr("idx"), ar.addr("values"), k, ar.addr("work"), form)
        got = ar.check(written={"leaves", "tree"})
        assert hashed == MU.update(levels, idx, values, *hades.args) == MU.hashed_count(idx, HEIGHT)
        assert np.array_equal(G.as_u64(got["leaves"], 4 ** HEIGHT, 4), HM.to_limbs(levels[0])), (k, form)
        assert np.array_equal(G.as_u64(got["tree"], -1, 4), HM.to_limbs(PM.flat_tree(levels))), (k, form)


def test_poseidon_merkle_update_refusals_change_nothing(ctx, hades):
    """"A REFUSED CALL CHANGES NO BYTE of leaves or tree": indices that do not ascend, an index that is not below 4^height, and
    "d_values, d_indices or d_work overlapping leaves or tree" """
    import plonk_prototype_amd as pa
    k = 5
    levels, idx = _tree(HEIGHT), _indices(k)
    values = HM.to_limbs(list(range(1, k + 1)))
    work = ctx._lib.pm_poseidon_merkle_update_work_bytes(k)
    for bad in (idx[:2] + [idx[1]] + idx[3:], idx[:4] + [4 ** HEIGHT]):
        with G.GuardArena.of(ctx, leaves=HM.to_limbs(levels[0]), tree=HM.to_limbs(PM.flat_tree(levels)), idx=np.array(bad, np.uint64),
                             values=values, work=work) as ar:
            t = _tree_handle(pa, ctx, hades, ar)
            _refused(pa, lambda: t.update_dev(ar.addr("idx"), ar.addr("values"), k, ar.addr("work")))
            assert set(ar.check()) == {"work"}                         # the scratch may have been used; nothing else changed
    with G.GuardArena.of(ctx, leaves=HM.to_limbs(levels[0]), tree=HM.to_limbs(PM.flat_tree(levels)), idx=np.array(idx, np.uint64),
                         values=values, work=work) as ar:
        t = _tree_handle(pa, ctx, hades, ar)
        a = ar.addr
        for i, v, w in ((a("leaves"), a("values"), a("work")), (a("idx"), a("tree"), a("work")), (a("idx"), a("values"), a("leaves")),
                        (a("idx"), a("values"), a("tree") + 32 * 84), (a("idx"), a("leaves") + 32 * 255, a("work"))):
            _refused(pa, lambda: t.update_dev(i, v, k, w))
        ar.check_unchanged()


# ---------------------------------------------------------------------------------- Schnorr
@pytest.fixture(scope="module")
def rig(ctx):
    r = TS.Rig(ctx, SHAPE)
    yield r
    r.free()


@pytest.mark.parametrize("n", SIZES)
def test_schnorr_sign(ctx, rig, n):
    cs = rig.cs
    with G.GuardArena.of(ctx, sk=S.scalar_words(cs["sk"][:n], True), k=S.scalar_words(cs["k"][:n], True), m=rig.msgs[:n].copy(),
                         sigs=96 * n) as ar:
        rig.s.sign_dev(ar.addr("sk"), ar.addr("k"), ar.addr("m"), n, ar.addr("sigs"))
        assert np.array_equal(G.as_u64(ar.check()["sigs"], n, 3, 4), rig.sigs(True)[:n]), n


@pytest.mark.parametrize("n", SIZES)
def test_schnorr_verify_reasons(ctx, rig, n):
    """n uint32 of reasons, exactly, from two kernels that walk n in strides; every reason occurs from n = 130 on, and entry 0,
    63 and 64 -- the ends of the first wave -- are corrupted ones"""
    pks, msgs, sigs, want = TS._corrupted(rig, True)
    with G.GuardArena.of(ctx, pks=pks[:n].copy(), m=msgs[:n].copy(), sigs=sigs[:n].copy(), reasons=4 * n) as ar:
        first = rig.s.verify_dev(ar.addr("pks"), ar.addr("m"), ar.addr("sigs"), n, ar.addr("reasons"))
        assert ar.check()["reasons"].view(np.uint32).tolist() == want[:n].tolist(), n
        assert first == 0 and want[0] != 0
    # ... and with d_reasons = NULL nothing at all is written
    with G.GuardArena.of(ctx, pks=pks[:n].copy(), m=msgs[:n].copy(), sigs=sigs[:n].copy()) as ar:
        assert rig.s.verify_dev(ar.addr("pks"), ar.addr("m"), ar.addr("sigs"), n) == 0
        assert ar.check() == {}


@pytest.mark.parametrize("n", SIZES)
def test_schnorr_verify_batch_sum(ctx, rig, n):
    """n x 16 bytes of weights in, the 64 bytes of W out; the last signature's message is changed, so that W is not the identity
    (entry 0 signs with sk = 0, which holds for every message: n = 1 stays accepted)"""
    cs = rig.cs
    rng = random.Random(0xBA + n)
    z = ([1, (1 << 128) - 1, 2] + [1 + rng.randrange((1 << 128) - 1) for _ in range(n)])[:n]
    msgs = list(cs["m"][:n])
    msgs[n - 1] = (msgs[n - 1] + 1) % R
    weights = np.array([[w & (2 ** 64 - 1), w >> 64] for w in z], np.uint64)
    w_model = MM.batch_sum(rig.cs["h"], J.GENERATOR, cs["pk"][:n], msgs, cs["sig"][:n], z)
    accepted = MM.cofactored_ok(w_model)
    assert accepted == (n == 1)
    with G.GuardArena.of(ctx, pks=rig.pks[:n].copy(), m=M.to_limbs(msgs), sigs=rig.sigs(True)[:n].copy(), z=weights, sum=64) as ar:
        res, bad = rig.s.verify_batch_dev(ar.addr("pks"), ar.addr("m"), ar.addr("sigs"), ar.addr("z"), n, ar.addr("sum"))
        assert (res, bad) == (S.OK if accepted else S.EQUATION, n)
        assert np.array_equal(_points(ar.check()["sum"], 1), J.to_limbs([w_model])), n
