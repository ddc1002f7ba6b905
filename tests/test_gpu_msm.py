"""Parity of the HIP MSM (through the C ABI) with the oracle, compared in affine form:
golden vectors, the reference's edge cases (zero / unit / r-1 scalars, infinity, duplicate
and opposite bases, the n = 31/32/33 window switch), skewed scalar distributions, both
scalar forms, every window width, and the discrete-log identity at 2^20."""
import numpy as np
import pytest

from oracle import bigint_oracle as B
from oracle.cpu_oracle import SCALAR_CANONICAL, SCALAR_MONTGOMERY, ints_to_limbs, limbs_to_ints
from conftest import hex_to_fr_mont, points_to_mont

pytestmark = pytest.mark.gpu
K0 = ints_to_limbs([0x1234567], 4)[0]
DD = ints_to_limbs([0xabcdef123456789abcdef], 4)[0]


def gpu_msm_affine(ctx, pts, sc, form=SCALAR_MONTGOMERY):
    import plonk_prototype_amd as pa
    xyz = pa.msm_variable_base(pts, sc, ctx, form)
    aff, ident = pa.g1_to_affine(xyz)
    assert ident == (not aff.any())
    return aff


def test_golden_vectors(ctx, oracle, golden):
    for v in golden["msm"]:
        pts = points_to_mont(oracle, v["points"])
        sc = hex_to_fr_mont(oracle, v["scalars"])
        got = gpu_msm_affine(ctx, pts, sc)
        if v["result"] is None:
            assert not got.any()
        else:
            x, y = limbs_to_ints(oracle.fp_from_mont(got.reshape(2, 6)))
            assert (x, y) == (int(v["result"][0], 16), int(v["result"][1], 16)), v["n"]


def _edge_inputs(oracle, n, seed):
    pts = oracle.g1_bases_arith(K0, DD, max(n, 1), 8)[:n]
    sc = oracle.fr_sample(seed, n)
    if n > 8:
        sc[0] = 0
        sc[1] = oracle.fr_to_mont(ints_to_limbs([1], 4))[0]
        sc[2] = oracle.fr_to_mont(ints_to_limbs([B.R_MOD - 1], 4))[0]
        pts[4] = pts[3]
        sc[4] = sc[3]                                   # duplicate base and scalar (bucket doubling)
        y6 = limbs_to_ints(oracle.fp_from_mont(pts[6, 6:].reshape(1, 6)))[0]
        pts[5, :6] = pts[6, :6]
        pts[5, 6:] = oracle.fp_to_mont(ints_to_limbs([B.P_MOD - y6], 6))[0]
        sc[5] = sc[6]                                   # P and -P, equal scalars (bucket cancels)
        pts[7] = 0                                      # infinity among the bases
    return pts, sc


@pytest.mark.parametrize("n", [0, 1, 2, 3, 31, 32, 33, 100, 1000, 4097, 1 << 14, 1 << 16])
def test_sizes_and_edge_cases(ctx, oracle, n):
    pts, sc = _edge_inputs(oracle, n, 900 + n)
    exp = oracle.g1_msm(pts, sc, SCALAR_MONTGOMERY, 8)
    assert np.array_equal(gpu_msm_affine(ctx, pts, sc), exp)
    canon = oracle.fr_from_mont(sc) if n else sc
    assert np.array_equal(gpu_msm_affine(ctx, pts, canon, SCALAR_CANONICAL), exp)


def test_trivial_scalars(ctx, oracle):
    n = 300
    pts = oracle.g1_bases_arith(K0, DD, n, 8)
    assert not gpu_msm_affine(ctx, pts, np.zeros((n, 4), np.uint64)).any()          # all zero -> identity
    ones = oracle.fr_to_mont(ints_to_limbs([1] * n, 4))
    assert np.array_equal(gpu_msm_affine(ctx, pts, ones), oracle.g1_msm(pts, ones))  # sum of the bases
    rm1 = oracle.fr_to_mont(ints_to_limbs([B.R_MOD - 1] * n, 4))
    assert np.array_equal(gpu_msm_affine(ctx, pts, rm1), oracle.g1_msm(pts, rm1))    # -sum
    assert not gpu_msm_affine(ctx, np.zeros((n, 12), np.uint64), ones).any()         # all bases infinite


@pytest.mark.parametrize("kind", ["all_equal", "zero_one_heavy", "small16", "two_values"])
def test_skewed_distributions(ctx, oracle, kind):
    """Load balance must not depend on the digits: a real witness is full of 0, 1 and small values."""
    n = 1 << 14
    pts = oracle.g1_bases_arith(K0, DD, n, 8)
    sc = oracle.fr_sample(8, n)
    one = oracle.fr_to_mont(ints_to_limbs([1], 4))[0]
    if kind == "all_equal":
        sc = np.repeat(oracle.fr_sample(7, 1), n, axis=0)
    elif kind == "zero_one_heavy":
        sc[::2] = one
        sc[1::4] = 0
    elif kind == "small16":
        small = [v % 65536 for v in limbs_to_ints(oracle.fr_from_mont(sc))]
        sc = oracle.fr_to_mont(ints_to_limbs(small, 4))
    else:
        sc[: n // 2] = sc[0]
        sc[n // 2:] = sc[1]
    assert np.array_equal(gpu_msm_affine(ctx, pts, sc), oracle.g1_msm(pts, sc, SCALAR_MONTGOMERY, 8))


@pytest.mark.parametrize("c", [4, 5, 7, 8, 11, 13, 16, 17, 20])
def test_every_window_width(ctx, oracle, c):
    n = 3000
    pts, sc = _edge_inputs(oracle, n, 55)
    exp = oracle.g1_msm(pts, sc, SCALAR_MONTGOMERY, 8)
    ctx.set_option("msm_window_bits", c)
    try:
        assert np.array_equal(gpu_msm_affine(ctx, pts, sc), exp)
    finally:
        ctx.set_option("msm_window_bits", 0)


def test_commit_key_mirror(ctx, oracle):
    import plonk_prototype_amd as pa
    n = 2048
    pts = oracle.g1_bases_arith(K0, DD, n, 8)
    ck = pa.CommitKey(pts, ctx)
    assert ck.max_degree() == n - 1
    poly = oracle.fr_sample(3, 1500)                                   # commit uses powers_of_g[..len]
    assert np.array_equal(ck.commit(poly), oracle.g1_msm(pts[:1500], poly))
    assert np.array_equal(ck.commit(poly), ck.commit(poly))            # deterministic
    assert not ck.commit(np.zeros((0, 4), np.uint64)).any()            # zero polynomial -> identity
    with pytest.raises(pa.Error) as e:
        ck.commit(oracle.fr_sample(3, n + 1))                          # PolynomialDegreeTooLarge
    assert e.value.code == -6
    with pytest.raises(pa.Error):
        pa.msm_variable_base(pts, poly, ctx)                           # length mismatch


@pytest.mark.parametrize("c", [0, 8, 13, 16, 20, 22, 24])
def test_precomputed_window_table(ctx, oracle, c):
    """pm_g1_bases_precompute: same result from the one-bucket-set path, for every table width,
    for prefixes of the SRS (commit of a shorter polynomial) and for offset shards."""
    import plonk_prototype_amd as pa
    import torch
    n = 5000
    pts, sc = _edge_inputs(oracle, n, 77)
    bases = pa.host.Bases(ctx, pts).precompute(c)
    for m in (n, 1234, 1, 0):
        got, _ = pa.g1_to_affine(bases.msm(sc[:m]))
        assert np.array_equal(got, oracle.g1_msm(pts[:m], sc[:m], SCALAR_MONTGOMERY, 8)), (c, m)
    canon = oracle.fr_from_mont(sc)
    got, _ = pa.g1_to_affine(bases.msm(canon, SCALAR_CANONICAL))
    assert np.array_equal(got, oracle.g1_msm(pts, sc, SCALAR_MONTGOMERY, 8))
    d_sc = torch.from_numpy(sc.view(np.int64)).cuda()
    part = bases.msm_dev(d_sc.data_ptr() + 32 * 1000, 3000, offset=1000)
    assert np.array_equal(pa.g1_to_affine(part)[0], oracle.g1_msm(pts[1000:4000], sc[1000:4000], SCALAR_MONTGOMERY, 8))
    with pytest.raises(pa.Error):
        bases.precompute(c)                                           # only once
    # a second MSM of another size on the same context right away: the bucket fill's control block is shared
    got, _ = pa.g1_to_affine(pa.msm_variable_base(pts[:7], sc[:7], ctx))
    assert np.array_equal(got, oracle.g1_msm(pts[:7], sc[:7], SCALAR_MONTGOMERY, 8))
    got, _ = pa.g1_to_affine(bases.msm(sc[:4097]))
    assert np.array_equal(got, oracle.g1_msm(pts[:4097], sc[:4097], SCALAR_MONTGOMERY, 8))
    # skewed digits through the table path
    eq = np.repeat(oracle.fr_sample(7, 1), n, axis=0)
    assert np.array_equal(pa.g1_to_affine(bases.msm(eq))[0], oracle.g1_msm(pts, eq, SCALAR_MONTGOMERY, 8))


def test_batched_msm_as_pipelined_pieces(ctx, oracle):
    """Option msm_pipeline = 1 (off by default: it loses, msm.hip): a batch runs as up to four pieces on two streams
    that alternate between two workspace regions.  Same results as the one-piece path, with and without the table."""
    import plonk_prototype_amd as pa
    import torch
    n, kb = 3000, 5
    pts, sc = _edge_inputs(oracle, n, 91)
    scs = np.concatenate([sc] + [oracle.fr_sample(500 + j, n) for j in range(1, kb)])
    d = torch.from_numpy(np.ascontiguousarray(scs).view(np.int64)).cuda()
    for table in (False, True):
        bases = pa.host.Bases(ctx, pts)
        if table:
            bases.precompute(13)
        ref = bases.msm_batch_dev(d.data_ptr(), n, kb)
        ctx.set_option("msm_pipeline", 1)
        try:
            for _ in range(2):
                got = bases.msm_batch_dev(d.data_ptr(), n, kb)
                assert np.array_equal(got, ref)
            assert np.array_equal(bases.msm_batch_dev(d.data_ptr(), n, 2), ref[:2])
        finally:
            ctx.set_option("msm_pipeline", 0)
        for j in range(kb):
            exp = oracle.g1_msm(pts, scs[j * n:(j + 1) * n], SCALAR_MONTGOMERY, 8)
            assert np.array_equal(pa.g1_to_affine(ref[j])[0], exp), j
        bases.free()


@pytest.mark.parametrize("table", [False, True])
def test_batched_commits(ctx, oracle, table):
    """pm_g1_msm_batch_dev: k scalar vectors over one SRS in a single pass == k separate MSMs."""
    import plonk_prototype_amd as pa
    n, k = 3000, 5
    pts, sc0 = _edge_inputs(oracle, n, 311)
    polys = np.stack([sc0] + [oracle.fr_sample(400 + j, n) for j in range(k - 1)])
    polys[2][:] = polys[2][0]                                       # one skewed vector in the batch
    polys[3][::2] = 0
    ck = pa.CommitKey(pts, ctx, precompute=table)
    got = ck.commit_many(polys)
    for j in range(k):
        assert np.array_equal(got[j], oracle.g1_msm(pts, polys[j], SCALAR_MONTGOMERY, 8)), (table, j)
    short = ck.commit_many(polys[:, :1000])                          # prefix of the SRS, like commit()
    for j in range(k):
        assert np.array_equal(short[j], oracle.g1_msm(pts[:1000], polys[j, :1000], SCALAR_MONTGOMERY, 8))
    with pytest.raises(pa.Error):
        ck.commit_many(np.zeros((2, n + 1, 4), np.uint64))
    # a batch over the 31-bit pair limit runs in halves (15 key polynomials of 2^24 coefficients do); forced
    # here with a small limit, so that the five vectors go through in two or more passes
    nwin = 256 // 13 + 1
    ctx.set_option("msm_max_pairs", 2 * n * nwin)
    try:
        split = ck.commit_many(polys)
    finally:
        ctx.set_option("msm_max_pairs", 0)
    assert np.array_equal(split, got)


def test_plans_of_every_branch_back_to_back(ctx, oracle):
    """One context, MSMs whose plans (csrc/msm_plan.h) differ in every branch, one after the other -- workspace, pinned buffer
    and control block are reused across them: two accumulate levels and the device's finish (n = 33), the window table with
    a follow-up reduction level and the host fold (4097), many sets in a batch (5000 points, 8-bit windows, four vectors),
    two follow-up reduction levels (2^14, table, msm_lb = 1), deep accumulate levels on an unplaced grid (2^14, msm_chunk =
    1), and the first shape again.  tests/test_msm_geometry.py holds the recorded decisions of these shapes."""
    import plonk_prototype_amd as pa
    import torch
    n = 1 << 14
    pts, sc = _edge_inputs(oracle, n, 4242)

    def expect(m, vec=sc):
        return oracle.g1_msm(pts[:m], vec[:m], SCALAR_MONTGOMERY, 8)

    exp33, exp_n = expect(33), expect(n)
    bases = []

    def make(points):
        bases.append(pa.host.Bases(ctx, points))
        return bases[-1]

    try:
        t13, t16, plain = make(pts[:4097]).precompute(13), make(pts).precompute(16), make(pts[:5000])
        assert np.array_equal(gpu_msm_affine(ctx, pts[:33], sc[:33]), exp33)
        assert np.array_equal(pa.g1_to_affine(t13.msm(sc[:4097]))[0], expect(4097))
        vecs = [sc[:5000]] + [oracle.fr_sample(4300 + j, 5000) for j in range(3)]
        d = torch.from_numpy(np.ascontiguousarray(np.concatenate(vecs)).view(np.int64)).cuda()
        ctx.set_option("msm_window_bits", 8)
        got = plain.msm_batch_dev(d.data_ptr(), 5000, 4)
        ctx.set_option("msm_window_bits", 0)
        for j in range(4):
            assert np.array_equal(pa.g1_to_affine(got[j])[0], expect(5000, vecs[j])), j
        ctx.set_option("msm_lb", 1)
        assert np.array_equal(pa.g1_to_affine(t16.msm(sc))[0], exp_n)
        ctx.set_option("msm_lb", 0)
        ctx.set_option("msm_chunk", 1)
        assert np.array_equal(gpu_msm_affine(ctx, pts, sc), exp_n)
        ctx.set_option("msm_chunk", 0)
        assert np.array_equal(gpu_msm_affine(ctx, pts[:33], sc[:33]), exp33)
    finally:
        for opt in ("msm_window_bits", "msm_lb", "msm_chunk"):
            ctx.set_option(opt, 0)
        for b in bases:
            b.free()


def test_sharded_msm_fold(ctx, oracle):
    """The multi-GPU decomposition on one GPU: shard by points, fold the partials."""
    import plonk_prototype_amd as pa
    import torch
    from plonk_prototype_amd.dist import shard_range
    n = 10007
    pts = oracle.g1_bases_arith(K0, DD, n, 8)
    sc = oracle.fr_sample(21, n)
    bases = pa.host.Bases(ctx, pts)
    d_sc = torch.from_numpy(sc.view(np.int64)).cuda()
    parts = []
    for r in range(3):
        lo, hi = shard_range(n, r, 3)
        parts.append(bases.msm_dev(d_sc.data_ptr() + 32 * lo, hi - lo, offset=lo))
    total, _ = pa.g1_to_affine(pa.g1_fold(np.stack(parts)))
    assert np.array_equal(total, oracle.g1_msm(pts, sc, SCALAR_MONTGOMERY, 8))


def test_full_size_2_20(ctx, oracle):
    """BASELINE config 2: 2^20 points.  Bit-exact against the CPU restatement's Pippenger AND the
    discrete-log identity (bases k_i G => result == (sum s_i k_i) G by one scalar mul)."""
    import plonk_prototype_amd as pa
    n = 1 << 20
    pts = oracle.g1_bases_arith(K0, DD, n, 16)
    sc = oracle.fr_sample(0x5343414C, n)
    ck = pa.CommitKey(pts, ctx)
    got = ck.commit(sc)
    dl = oracle.expected_dlog(sc, SCALAR_MONTGOMERY, K0, DD)
    assert np.array_equal(got, oracle.g1_mul(oracle.g1_generator(), dl))
    assert np.array_equal(got, oracle.g1_msm(pts, sc, SCALAR_MONTGOMERY, 16))
    ck_table = pa.CommitKey(pts, ctx, precompute=True)               # resident-SRS table path
    assert np.array_equal(ck_table.commit(sc), got)
    # witness-like distribution: 90 % below 2^16, 5 % zero, 1 % one
    vals = limbs_to_ints(oracle.fr_from_mont(sc[: 1 << 16]))
    w = []
    for i, v in enumerate(vals):
        m = v % 100
        w.append(0 if m < 5 else 1 if m == 5 else v % 65536 if m < 96 else v)
    wl = oracle.fr_to_mont(ints_to_limbs(w, 4))
    wl = np.tile(wl, (16, 1))
    dl = oracle.expected_dlog(wl, SCALAR_MONTGOMERY, K0, DD)
    assert np.array_equal(ck.commit(wl), oracle.g1_mul(oracle.g1_generator(), dl))


def test_full_size_2_24_against_the_discrete_log(ctx, oracle):
    """BASELINE configs[4]'s MSM size inside pytest (VERDICT r01 missing #5): 2^24 points of a powers-of-tau key
    generated on the GPU, resident-SRS table, uniform scalars; commit(s) = [s(tau)] G with s(tau) from the
    CPU restatement's Horner -- no second MSM, no 2^24 scalar multiplications on the CPU."""
    import plonk_prototype_amd as pa
    n = 1 << 24
    tau = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % B.R_MOD
    tau_m = oracle.fr_to_mont(ints_to_limbs([tau], 4))[0]
    ck = pa.CommitKey.setup(n - 1, tau_m, ctx, precompute=True)
    sc = oracle.fr_sample(0x5343414C + 24, n)
    d_sc = pa.DeviceVector.from_host(ctx, sc)
    got, ident = pa.g1_to_affine(ck._bases.msm_dev(d_sc.ptr, n))
    s_tau = oracle.fr_from_mont(oracle.fr_poly_evaluate(sc, tau_m).reshape(1, 4))[0]
    assert not ident and np.array_equal(got, oracle.g1_mul(oracle.g1_generator(), s_tau))
    # the same scalars against the first 2^24 - 5 bases only: another polynomial, another point
    got2, _ = pa.g1_to_affine(ck._bases.msm_dev(d_sc.ptr, n - 5))
    s2 = oracle.fr_from_mont(oracle.fr_poly_evaluate(sc[:n - 5], tau_m).reshape(1, 4))[0]
    assert np.array_equal(got2, oracle.g1_mul(oracle.g1_generator(), s2))
    d_sc.free()
    ck._bases.free()


def test_2_26_points_against_the_discrete_log(ctx, oracle):
    """Four times BASELINE's largest MSM: 2^26 points (6.4 GB of SRS, a 77 GB window table, 8 x 10^8 (digit, point)
    pairs -- 31-bit pair indices and 64-bit byte offsets everywhere).  Everything stays on the device: the key from
    the fixed-base kernel, uniform scalars from torch, s(tau) from the Horner kernel (no MSM code in it); the host does one
    scalar multiplication."""
    import plonk_prototype_amd as pa
    import torch
    n = 1 << 26
    tau = 0x3C6EF372FE94F82BA54FF53A5F1D36F1510E527FADE682D19B05688C2B3E6C1F % B.R_MOD
    tau_m = oracle.fr_to_mont(ints_to_limbs([tau], 4))[0]
    ck = pa.CommitKey.setup(n - 1, tau_m, ctx, precompute=True)
    g = torch.Generator(device="cuda").manual_seed(2626)
    sc = torch.randint(-(1 << 63), (1 << 63) - 1, (n, 4), dtype=torch.int64, device="cuda", generator=g)
    sc[:, 3] &= 0x3FFFFFFFFFFFFFFF                                  # below 2^254 < r: valid Montgomery residues
    torch.cuda.synchronize()
    for m in (n, n - 12345):
        got, ident = pa.g1_to_affine(ck._bases.msm_dev(sc.data_ptr(), m))
        s_tau = oracle.fr_from_mont(ctx.fr_evaluate(sc.data_ptr(), m, tau_m).reshape(1, 4))[0]
        assert not ident and np.array_equal(got, oracle.g1_mul(oracle.g1_generator(), s_tau)), m
    del sc
    ck._bases.free()
    torch.cuda.empty_cache()
    ctx.trim()                                                      # 13 GB of MSM workspace: the context is shared by the session


@pytest.mark.parametrize("n", [1, 2, 300, 5000])
def test_srs_setup_on_the_gpu(ctx, oracle, n):
    """CommitKey.setup: powers_of_g[i] = tau^i G from the fixed-base kernel, against per-point
    double-and-add in the oracle; then a commitment under the generated key."""
    import plonk_prototype_amd as pa
    from oracle import bigint_oracle as B
    from oracle.cpu_oracle import ints_to_limbs, limbs_to_ints
    tau = 0x6B8B4567327B23C6643C98696633487374B0DC5119495CFF2AE8944A625558EC % B.R_MOD
    tau_m = oracle.fr_to_mont(ints_to_limbs([tau], 4))[0]
    ck = pa.CommitKey.setup(n - 1, tau_m, ctx, host_copy=True)
    G = oracle.g1_generator()
    step = max(1, n // 40)
    for i in list(range(0, n, step)) + [n - 1]:
        assert np.array_equal(ck.powers_of_g[i], oracle.g1_mul(G, ints_to_limbs([pow(tau, i, B.R_MOD)], 4)[0])), i
    assert all(oracle.g1_is_on_curve(ck.powers_of_g[i]) for i in range(0, n, step))
    coeffs = oracle.fr_sample(n, n)
    cv = limbs_to_ints(oracle.fr_from_mont(coeffs))
    expect = oracle.g1_mul(G, ints_to_limbs([B.horner(cv, tau)], 4)[0])
    assert np.array_equal(ck.commit(coeffs), expect)                 # commit(p) = p(tau) G


def test_fixed_base_edge_scalars(ctx, oracle):
    """Scalars 0, 1, r - 1, single-byte digits, and the identity as base."""
    import ctypes as C
    import plonk_prototype_amd as pa
    from oracle import bigint_oracle as B
    from oracle.cpu_oracle import ints_to_limbs
    ks = [0, 1, B.R_MOD - 1, 255, 256, 0xFF00FF00FF, 1 << 200, (1 << 248) + 5]
    sc = pa.DeviceVector.from_host(ctx, oracle.fr_to_mont(ints_to_limbs(ks, 4)))
    out = pa.DeviceVector(ctx, 3 * len(ks))
    P = oracle.g1_mul(oracle.g1_generator(), ints_to_limbs([0xABCDEF], 4)[0])
    u64p = C.POINTER(C.c_uint64)
    ctx._check(ctx._lib.pm_g1_fixed_base_mul_dev(ctx._h, P.ctypes.data_as(u64p), sc._p, len(ks), 0, out._p, None))
    got = out.to_host().reshape(-1, 12)
    for k, g in zip(ks, got):
        assert np.array_equal(g, oracle.g1_mul(P, ints_to_limbs([k], 4)[0])), hex(k)
    assert not got[0].any()
    # canonical-form scalars give the same points
    sc2 = pa.DeviceVector.from_host(ctx, ints_to_limbs(ks, 4))
    ctx._check(ctx._lib.pm_g1_fixed_base_mul_dev(ctx._h, P.ctypes.data_as(u64p), sc2._p, len(ks), 1, out._p, None))
    assert np.array_equal(out.to_host().reshape(-1, 12), got)
    ident = np.zeros(12, np.uint64)
    ctx._check(ctx._lib.pm_g1_fixed_base_mul_dev(ctx._h, ident.ctypes.data_as(u64p), sc._p, len(ks), 0, out._p, None))
    assert not out.to_host().any()


def test_reduction_meets_equal_and_opposite_sums(ctx, oracle):
    """The bucket reduction adds bucket sums and running sums to each other: with bases drawn from
    {G, -G, 2G, infinity} and tiny scalars, neighbouring buckets, chunks and waves hold EQUAL or OPPOSITE
    points all the time, so the P + P (doubling) and P - P (identity) branches of the two-lane group law
    (ec.hip.h, half_add) run in the running sums, in the suffix scan and in the trees.  Both paths (per-call
    bases and the window table), several chunk sizes."""
    import plonk_prototype_amd as pa
    rng = np.random.default_rng(2024)
    g = oracle.g1_generator()
    neg = g.copy()
    y = limbs_to_ints(oracle.fp_from_mont(g[6:].reshape(1, 6)))[0]
    neg[6:] = oracle.fp_to_mont(ints_to_limbs([B.P_MOD - y], 6))[0]
    two = oracle.g1_add(g, g)
    palette = np.stack([g, neg, two, np.zeros(12, np.uint64)])
    try:
        for trial in range(60):
            n = int(rng.integers(2, 200))
            pts = np.ascontiguousarray(palette[rng.integers(0, 4, n)])
            top = [4, 16, 40, 1 << 13][trial % 4]
            ks = [int(v) for v in rng.integers(0, top, n)]
            sc = oracle.fr_to_mont(ints_to_limbs(ks, 4))
            exp = oracle.g1_msm(pts, sc, SCALAR_MONTGOMERY, 4)
            ctx.set_option("msm_lb", [0, 1, 2, 8][(trial // 4) % 4])
            assert np.array_equal(gpu_msm_affine(ctx, pts, sc), exp), (trial, n, top)
            if trial % 5 == 0:
                bases = pa.host.Bases(ctx, pts).precompute([8, 13][trial % 2])
                assert np.array_equal(pa.g1_to_affine(bases.msm(sc))[0], exp), (trial, n, top, "table")
    finally:
        ctx.set_option("msm_lb", 0)
