"""What the NTT driver resolves for a transform before it launches (csrc/ntt.hip, ntt_resolve), through the pure-host hook
pm_test_ntt_launches -- no context, no GPU.  The hook's records are compared, field by field, with a model written here from
the decisions the driver's launch loop took pass by pass before it was split into "resolve, acquire, launch"; the traits
of the kernel shapes the model needs are literal tables.  Also: the headline plan by literal, and the promise of
pm_domain_prepare -- the tables named by the four plans it resolves cover those of every transform of that size."""
import ctypes as C
from collections import namedtuple

import pytest

INVERSE, COSET = 1, 2
DIRECT_TW, PRE_COSET, POST_SCALE, POST_COSET, XCD_REMAP, TW_OUT, TW_APPLIED, STEP_PRIO = 1, 2, 4, 8, 16, 32, 64, 128
SINGLE, FIRST, MIDDLE, LAST = 0, 1, 2, 3

# (S, LT, role) of every radix-4 kernel: (applies the next pass's twiddles when asked, takes wave priorities by step, form G of
# the lazy step table it reads, threads per workgroup, LDS bytes) -- 9 single-pass shapes, 13 tile shapes in three roles
R4 = {
    (2, 0, 0): (0, 0, 0, 64, 0),
    (3, 0, 0): (0, 0, 0, 64, 288),
    (4, 0, 0): (0, 0, 0, 64, 576),
    (5, 0, 0): (0, 0, 0, 64, 1152),
    (5, 5, 1): (0, 0, 0, 256, 36864),
    (5, 5, 2): (0, 0, 0, 256, 36864),
    (5, 5, 3): (0, 0, 0, 256, 36864),
    (5, 6, 1): (0, 0, 0, 512, 73728),
    (5, 6, 2): (0, 0, 0, 512, 73728),
    (5, 6, 3): (0, 0, 0, 512, 73728),
    (6, 0, 0): (0, 0, 0, 64, 2304),
    (6, 4, 1): (0, 0, 0, 256, 36864),
    (6, 4, 2): (0, 0, 0, 256, 36864),
    (6, 4, 3): (0, 0, 0, 256, 36864),
    (6, 5, 1): (0, 0, 0, 512, 73728),
    (6, 5, 2): (0, 0, 0, 512, 73728),
    (6, 5, 3): (0, 0, 0, 512, 73728),
    (7, 0, 0): (0, 0, 0, 64, 4608),
    (7, 3, 1): (0, 0, 0, 256, 36864),
    (7, 3, 2): (0, 0, 0, 256, 36864),
    (7, 3, 3): (0, 0, 0, 256, 36864),
    (7, 4, 1): (0, 0, 0, 512, 73728),
    (7, 4, 2): (0, 0, 0, 512, 73728),
    (7, 4, 3): (0, 0, 0, 512, 73728),
    (8, 0, 0): (0, 0, 0, 64, 9216),
    (8, 2, 1): (0, 0, 0, 256, 36864),
    (8, 2, 2): (0, 0, 0, 256, 36864),
    (8, 2, 3): (0, 0, 0, 256, 36864),
    (8, 3, 1): (0, 0, 0, 512, 73728),
    (8, 3, 2): (0, 0, 0, 512, 73728),
    (8, 3, 3): (0, 0, 0, 512, 73728),
    (9, 0, 0): (0, 0, 0, 128, 18432),
    (9, 1, 1): (0, 0, 0, 256, 36864),
    (9, 1, 2): (0, 0, 0, 256, 36864),
    (9, 1, 3): (0, 0, 0, 256, 36864),
    (9, 2, 1): (0, 0, 0, 512, 73728),
    (9, 2, 2): (0, 0, 0, 512, 73728),
    (9, 2, 3): (0, 0, 0, 512, 73728),
    (10, 0, 0): (0, 1, 0, 256, 36864),
    (10, 0, 1): (1, 1, 0, 256, 36864),
    (10, 0, 2): (0, 1, 0, 256, 36864),
    (10, 0, 3): (0, 1, 0, 256, 36864),
    (10, 1, 1): (1, 1, 5, 512, 73728),
    (10, 1, 2): (0, 1, 3, 512, 73728),
    (10, 1, 3): (0, 1, 3, 512, 73728),
    (10, 2, 1): (1, 1, 0, 1024, 147456),
    (10, 2, 2): (0, 1, 0, 1024, 147456),
    (10, 2, 3): (0, 1, 0, 1024, 147456),
}
# the radix-8 kernels: 8 single-pass shapes (role 0) and 13 tile shapes in the roles 1 .. 3 -- (threads, LDS bytes)
R8_SINGLE = {3: (64, 0), 4: (64, 576), 5: (64, 1152), 6: (64, 2304), 7: (64, 4608), 8: (64, 9216), 9: (64, 18432),
             10: (128, 36864)}
R8_TILE = {(5, 6): (256, 73728), (6, 5): (256, 73728), (7, 4): (256, 73728), (8, 3): (256, 73728), (9, 2): (256, 73728),
           (10, 1): (256, 73728), (8, 4): (512, 147456), (9, 3): (512, 147456), (10, 2): (512, 147456),
           (5, 5): (128, 36864), (6, 4): (128, 36864), (7, 3): (128, 36864), (8, 2): (128, 36864)}
# the fixed-shape variants: (S, LT, role) -> (log_n, log_ns, group log of the blocked layout, the flags the launch must carry,
# taken already with ntt_fixed_shape = 1, G of its lazy table); a plain transform of a whole input only
FIXED = {(10, 1, 1): (20, 0, 2, TW_OUT | STEP_PRIO | XCD_REMAP, True, 3),
         (10, 1, 3): (20, 10, 2, TW_APPLIED | STEP_PRIO | XCD_REMAP, False, 3)}

Opts = namedtuple("Opts", "tile_log max_radix radix xcd direct_tw tw_producer step_prio fixed_shape")
DEFAULTS = Opts(0, 10, 4, 1, 1, 1, 1, 2)
FIELDS = ("S", "LT", "role", "family", "variant", "threads", "lds", "blocks", "flags", "log_ns", "G", "tw_in", "tw_out")


def r8_kernel(S, LT, role):
    return R8_SINGLE.get(S) if role == SINGLE and LT == 0 else (R8_TILE.get((S, LT)) if role != SINGLE else None)


def model_plan(log_n, tile_log, max_radix, radix, min_tiles, batch):
    if log_n < 3:
        return [], []
    if log_n <= 10:
        return [log_n], [0]
    npass = min(-(-log_n // max_radix), log_n // 5, 4)
    base, extra = divmod(log_n, npass)
    Ss, LTs = [], []
    for i in range(npass):
        S = base + (1 if i < extra else 0)
        lt = tile_log - S if tile_log else (1 if S >= 10 and radix == 4 else max(10 - S, 2))
        if S < 8 and lt > 11 - S:
            lt = 11 - S
        if not tile_log and radix == 4:
            while lt > (0 if S >= 10 else 1) and ((batch << log_n) >> (S + lt)) < min_tiles and (S, lt - 1, LAST) in R4:
                lt -= 1
        lt = max(lt, 0)
        if radix != 4 and lt < 1:
            lt = 1
        if radix != 4 and tile_log == 10 and S > 8:
            lt = 11 - S
        Ss.append(S)
        LTs.append(min(lt, log_n - S))
    return Ss, LTs


def model(log_n, batch, flags, in_len, o, num_cus):
    """The decisions of the driver's launch loop, in its order: (header, [record per pass])."""
    inverse, coset = bool(flags & INVERSE), bool(flags & COSET)
    pre = PRE_COSET if coset and not inverse else 0
    direct_tw = log_n <= 26 and bool(o.direct_tw)
    Ss, LTs = model_plan(log_n, o.tile_log, o.max_radix, o.radix, num_cus, batch)
    npass = len(Ss)
    scale_folded = inverse and npass > 1 and direct_tw
    post = (POST_SCALE if inverse and not scale_folded else 0) | (POST_COSET if inverse and coset else 0)
    if npass == 0:
        return dict(npass=0, glog=0, tiny=int(log_n > 0), tiny_flags=pre | post, folded=int(scale_folded)), []
    glog = max(min([3] + LTs), 2)
    recs, log_ns, tw_applied = [], 0, False
    for i in range(npass):
        last = i == npass - 1
        S, LT = Ss[i], LTs[i]
        role = SINGLE if npass == 1 else (FIRST if i == 0 else (LAST if last else MIDDLE))
        r4 = o.radix == 4 and (S, LT, role) in R4
        if r4:
            producer, prio, lazy, threads, lds = R4[(S, LT, role)]
        else:
            assert r8_kernel(S, LT, role) is not None, ("no kernel", S, LT, role)
            (threads, lds), producer, prio, lazy = r8_kernel(S, LT, role), 0, 0, 0
        tw_in = tw_out = -1
        tw_flag = 0
        if tw_applied:
            tw_flag = TW_APPLIED
        elif i > 0 and direct_tw:
            tw_in, tw_flag = i, DIRECT_TW
        tw_applied = False
        if not last and direct_tw and o.tw_producer and r4 and producer:
            if (Ss[i + 1], LTs[i + 1], LAST if i + 1 == npass - 1 else MIDDLE) in R4:
                tw_out = i + 1
                tw_flag |= TW_OUT
                tw_applied = True
        f = (pre if i == 0 else 0) | (post if last else 0) | tw_flag | (XCD_REMAP if o.xcd else 0)
        if r4 and o.step_prio and prio:
            f |= STEP_PRIO
        variant = 1
        if r4 and o.fixed_shape and (S, LT, role) in FIXED:
            fix_n, fix_ns, fix_glog, fix_flags, by_default, fix_G = FIXED[(S, LT, role)]
            if (o.fixed_shape == 2 or by_default) and (log_n, log_ns, glog, f) == (fix_n, fix_ns, fix_glog, fix_flags) and \
                    in_len == 1 << fix_n and not coset:
                variant, lazy = 2, fix_G
        recs.append(dict(S=S, LT=LT, role=role, family=4 if r4 else 8, variant=variant, threads=threads, lds=lds,
                         blocks=(1 << log_n) >> (S + LT), flags=f, log_ns=log_ns, G=lazy, tw_in=tw_in, tw_out=tw_out))
        log_ns += S
    return dict(npass=npass, glog=glog, tiny=0, tiny_flags=0, folded=int(scale_folded)), recs


@pytest.fixture(scope="module")
def lib():
    from plonk_prototype_amd import _lib
    return _lib.load()


def launches(lib, log_n, batch, flags, in_len, o, num_cus=0):
    # the hook's convention: 0 = default for the three sizes, negative = default for the switches; here every value is explicit,
    # except tile_log, whose 0 is a value and the default at once
    opts = (C.c_long * 8)(*o)
    out = (C.c_int32 * 60)()
    rc = lib.pm_test_ntt_launches(log_n, batch, flags, in_len, opts, num_cus, out)
    assert rc == 0, (rc, log_n, batch, flags, in_len, o)
    v = list(out)
    head = dict(npass=v[0], glog=v[1], tiny=v[2], tiny_flags=v[3], folded=v[4])
    assert v[5:8] == [0, 0, 0] and not any(v[8 + 13 * v[0]:])
    return head, [dict(zip(FIELDS, v[8 + 13 * i: 21 + 13 * i])) for i in range(v[0])]


def tables(log_n, flags, head, recs):
    """The device tables a resolved plan names: what the acquisition must make present."""
    if log_n == 0:
        return set()
    d = flags & INVERSE
    names = {("domain", d)} | ({("coset", d)} if flags & COSET else set())
    for r in recs:
        names.add(("step", r["family"], d, r["S"]))
        if r["G"]:
            names.add(("lazy", d, r["S"], r["G"]))
        for j in (r["tw_in"], r["tw_out"]):
            if j >= 0:   # an inter-pass table by its key: log_ns, S, last, the blocking of the wide layout
                names.add(("pass_tw", d, j, recs[j]["log_ns"], recs[j]["S"], recs[j]["role"] == LAST, head["glog"]))
    return names


def table_count(names):
    return sum(2 if t[0] in ("domain", "coset") else 1 for t in names)


def option_sets():
    """Every value of every option, the others at their defaults, and the sizes' full product in both families."""
    sets = []
    for radix in (4, 8):
        for max_radix in range(6, 11):
            for tile_log in (0, 10, 11, 12):
                sets.append(DEFAULTS._replace(radix=radix, max_radix=max_radix, tile_log=tile_log))
        for name in ("xcd", "direct_tw", "tw_producer", "step_prio"):
            sets.append(DEFAULTS._replace(radix=radix, **{name: 0}))
        for fs in (0, 1):
            sets.append(DEFAULTS._replace(radix=radix, fixed_shape=fs))
        sets.append(DEFAULTS._replace(radix=radix, xcd=0, direct_tw=0, tw_producer=0, step_prio=0, fixed_shape=0))
        sets.append(DEFAULTS._replace(radix=radix, tw_producer=0, fixed_shape=1))
        sets.append(DEFAULTS._replace(radix=radix, step_prio=0, fixed_shape=1))
    return sets


def test_every_record_equals_the_model_and_prepare_covers_every_transform(lib):
    cases = 0
    for log_n in range(0, 32):
        n = 1 << log_n
        for o in option_sets():
            # the sizes' product runs over the whole input of one vector and one ragged batch; the switches over everything
            full = o.max_radix == 10 and o.tile_log == 0
            shapes = [(b, l) for b in (1, 4, 15) for l in (n, n // 2, 0)] if full else [(1, n), (4, n // 2), (15, 0)]
            prepared = set()
            for flags in (0, INVERSE, COSET, INVERSE | COSET):
                prepared |= tables(log_n, flags, *launches(lib, log_n, 1, flags, n, o))
            for batch, in_len in shapes:
                for flags in (0, INVERSE, COSET, INVERSE | COSET):
                    head, recs = launches(lib, log_n, batch, flags, in_len, o)
                    want_head, want = model(log_n, batch, flags, in_len, o, 256)
                    tag = (log_n, batch, flags, in_len, o)
                    assert head == want_head, tag
                    assert len(recs) == len(want), tag
                    for i, (got, exp) in enumerate(zip(recs, want)):
                        for k in FIELDS:
                            assert got[k] == exp[k], (k, i, got, exp, tag)
                    assert tables(log_n, flags, head, recs) <= prepared, (tables(log_n, flags, head, recs) - prepared, tag)
                    cases += 1
    # per size and family: 10 option sets over 9 shapes and 19 over 3, four transforms each
    assert cases == 32 * 2 * (10 * 9 + 19 * 3) * 4


def test_other_compute_unit_counts(lib):
    """num_cus sets where the tiles stop narrowing: the model follows it at the sizes where it matters."""
    for num_cus in (64, 304):
        for log_n in range(11, 24):
            for batch in (1, 4):
                for flags in (0, INVERSE | COSET):
                    head, recs = launches(lib, log_n, batch, flags, 1 << log_n, DEFAULTS, num_cus)
                    assert (head, recs) == model(log_n, batch, flags, 1 << log_n, DEFAULTS, num_cus), (num_cus, log_n, batch, flags)


def test_the_hook_defaults_are_a_fresh_contexts(lib):
    zero = Opts(0, 0, 0, -1, -1, -1, -1, -1)
    for log_n in (2, 10, 20, 24):
        for flags in (0, INVERSE | COSET):
            assert launches(lib, log_n, 1, flags, 1 << log_n, zero) == launches(lib, log_n, 1, flags, 1 << log_n, DEFAULTS)


def test_headline_by_literal(lib):
    """2^20, one vector, plain, forward and inverse, defaults: two fixed-shape <10, 1> passes that read the G = 3 lazy table;
    the first applies the second's inter-pass table, the second reads none."""
    for flags in (0, INVERSE):
        head, recs = launches(lib, 20, 1, flags, 1 << 20, DEFAULTS)
        assert head == dict(npass=2, glog=2, tiny=0, tiny_flags=0, folded=int(flags == INVERSE))
        assert [r["S"] for r in recs] == [10, 10] and [r["LT"] for r in recs] == [1, 1]
        assert [r["threads"] for r in recs] == [512, 512] and [r["lds"] for r in recs] == [73728, 73728]
        assert [r["blocks"] for r in recs] == [512, 512] and [r["log_ns"] for r in recs] == [0, 10]
        assert [r["role"] for r in recs] == [FIRST, LAST] and [r["family"] for r in recs] == [4, 4]
        assert [r["variant"] for r in recs] == [2, 2] and [r["G"] for r in recs] == [3, 3]
        # pass4_fixed_flags of each pass (csrc/ntt_kernels4.hip.h)
        assert [r["flags"] for r in recs] == [TW_OUT | STEP_PRIO | XCD_REMAP, TW_APPLIED | STEP_PRIO | XCD_REMAP]
        assert [(r["tw_in"], r["tw_out"]) for r in recs] == [(-1, 1), (-1, -1)]
        # the tables of the transform: the domain's two, one step table, one lazy table, one inter-pass table
        assert table_count(tables(20, flags, head, recs)) == 5


def test_hook_arguments(lib):
    from plonk_prototype_amd import _lib
    opts, out = (C.c_long * 8)(*DEFAULTS), (C.c_int32 * 60)()
    f = lib.pm_test_ntt_launches
    assert f(32, 1, 0, 1, opts, 0, out) == _lib.PM_ERR_DOMAIN_TOO_LARGE
    assert f(4, 1, 0, 17, opts, 0, out) == _lib.PM_ERR_LENGTH
    assert f(4, 0, 0, 16, opts, 0, out) == _lib.PM_ERR_BAD_ARG and f(4, 1, 4, 16, opts, 0, out) == _lib.PM_ERR_BAD_ARG
    assert f(4, 1, 0, 16, None, 0, out) == _lib.PM_ERR_BAD_ARG and f(4, 1, 0, 16, opts, 0, None) == _lib.PM_ERR_BAD_ARG
