"""halo_pcdl_check_batch_mixed / halo_acc_decider_batch_mixed and their _combined forms on the GPU: the scalars sum_a w_a pad(h_a)
over tables of different lengths limb for limb against Python integers under every split into parts and passes; an honest batch
of three sizes accepted by ONE MSM (the profiler shows which path ran); rejects of every kind with the single calls' statuses,
code and message; a pair of members of different sizes whose unweighted defects cancel; the edges (one size, one member, a
constant, no member, whole-call errors, no staging, company on the slots, both right sides); and the table pipeline as the one
MSM on a 2^20-point key.  The pools of honest members and the helpers around them are those of tests/test_gpu_check_combined.py."""
import ctypes as C

import numpy as np
import pytest

import orc
import test_gpu_check_combined as cc

pytestmark = pytest.mark.gpu

R_MOD = cc.R_MOD
REJECT = -2


@pytest.fixture(scope="module")
def hal():
    import halo_accumulation_amd as h
    assert h._lib.HALO_E_REJECT == REJECT
    return h


@pytest.fixture(scope="module")
def ctx(hal):
    c = hal._lib.Context(urs_n=1 << 14)
    yield c
    c.close()


@pytest.fixture(scope="module")
def big(hal):
    c = hal._lib.Context(urs_n=1 << 20)
    yield c
    c.close()


@pytest.fixture(scope="module")
def big_members(big):
    """on the 2^20-point key, built once: one Instance of lg 20 and three of lg 10"""
    from halo_accumulation_amd import acc as A
    return A.random_instance_batch(big, [0xB16], (1 << 20) - 1, 1)[0], list(A.random_instance_batch(big, [0xB17], 1023, 3))


ptr = cc.ptr


def d_of(q):
    return int(q[12])


def lg_of(q):
    return (d_of(q) + 1).bit_length() - 1


def mixed(c, blobs, acc=False, combined=True, seed=None, ds=None):
    """-> (return code, status list, message); status entries the call does not write stay 77"""
    m = len(blobs)
    keep = [np.ascontiguousarray(b, dtype=np.uint64) for b in blobs]
    ps = (C.c_void_p * max(m, 1))(*[b.ctypes.data for b in keep])
    dd = (C.c_size_t * max(m, 1))(*(ds if ds is not None else [d_of(b) for b in keep]))
    st = (C.c_int * max(m, 1))(*([77] * max(m, 1)))
    if combined:
        fn = c.lib.halo_acc_decider_batch_mixed_combined if acc else c.lib.halo_pcdl_check_batch_mixed_combined
        rc = fn(c.h, dd, ps, m, seed, st)
    else:
        fn = c.lib.halo_acc_decider_batch_mixed if acc else c.lib.halo_pcdl_check_batch_mixed
        rc = fn(c.h, dd, ps, m, st)
    return rc, [st[i] for i in range(m)], (c.lib.halo_last_error().decode() if rc else "")


def single(c, q, acc=False):
    """-> (code, message) of halo_pcdl_check / halo_acc_decider on this member alone"""
    q = np.ascontiguousarray(q, dtype=np.uint64)
    if acc:
        rc = c.lib.halo_acc_decider(c.h, ptr(q))
    else:
        rc = c.lib.halo_pcdl_check(c.h, ptr(q[0:12].copy()), d_of(q), ptr(q[13:17].copy()), ptr(q[17:21].copy()), ptr(q[21:].copy()))
    return rc, (c.lib.halo_last_error().decode() if rc else "")


def by_single_calls(c, blobs, acc=False):
    """what the contract promises: every status the single call's, the code and message the first failing member's"""
    each = [single(c, q, acc) for q in blobs]
    st = [rc for rc, _ in each]
    bad = [i for i, rc in enumerate(st) if rc]
    if not bad:
        return 0, st, ""
    return st[bad[0]], st, "instance %d: %s" % (bad[0], each[bad[0]][1])


def sequences(counts):
    """MSM launch sequences: each starts with one recode launch (the small and general pipelines', or the table pipeline's)"""
    return counts.get("k_msm_recode", 0) + counts.get("k_tmsm_recode", 0)


def ran_mixed_only(counts):
    return counts.get("k_h_accumulate_mixed", 0) > 0 and counts.get("k_h_tables_mixed", 0) > 0 and counts.get("k_h_coeffs_batch", 0) == 0


def ran_exact_only(counts):
    return counts.get("k_h_accumulate_mixed", 0) == 0 and counts.get("k_h_coeffs_batch", 0) > 0


_LG10 = {}


def honest(c, lg, k, acc=False):
    """k honest members of size lg on the 2^14-point key: lg 3 and 9 from the shared pools, lg 10 a small pool of its own"""
    if lg in (3, 9):
        return list(cc.pool(c, lg)[1 if acc else 0][:k])
    assert not acc
    if lg not in _LG10:
        from halo_accumulation_amd import acc as A
        _LG10[lg] = A.random_instance_batch(c, [0x10A + lg], (1 << lg) - 1, 3)
    return list(_LG10[lg][:k])


def interleave(*classes):
    out = []
    for k in range(max(len(cl) for cl in classes)):
        out += [cl[k] for cl in classes if k < len(cl)]
    return out


# ------------------------------------------------------------------ 1. the scalars against big integers
def mixed_case(lgs):
    """random challenges and weights per table; planted: weights 0, 1 and r - 1, a challenge r - 1 and a zero challenge"""
    A = len(lgs)
    xs, s = orc.rng_scalars(0x313ED + 131 * A + sum(lgs), sum(lg + 1 for lg in lgs))
    ws, _ = orc.rng_scalars(s, A)
    xis, o = [], 0
    for lg in lgs:
        xis.append([orc.fr_from_mont(xs[o + k]) for k in range(lg + 1)])
        o += lg + 1
    w = [orc.fr_from_mont(ws[a]) for a in range(A)]
    special = [0, 1, R_MOD - 1]
    for a in range(min(A, 3)):
        w[a] = special[(a + lgs[0]) % 3]
    xis[0][lgs[0]] = R_MOD - 1
    xis[A - 1][1] = 0
    return xis, w


def want_words(xis, lgs, w):
    """want[k] = sum over the tables with k < n_a of w_a h_a[k] mod r, as Montgomery limbs"""
    want = [0] * (1 << max(lgs))
    for x, lg, wa in zip(xis, lgs, w):
        for k, v in enumerate(cc.h_poly(x, lg)):
            want[k] = (want[k] + wa * v) % R_MOD
    return cc.mont_words(want)


def mixed_scalars(hal, c, xis, lgs, w, parts, cap):
    A, lg_max = len(lgs), max(lgs)
    x = np.zeros((A, lg_max + 1, 4), dtype=np.uint64)
    for a in range(A):
        x[a, :lgs[a] + 1] = cc.mont_words(xis[a])
        x[a, lgs[a] + 1:] = np.uint64(0xDEADBEEFDEADBEEF)  # (the rest of a record is not read)
    out = np.zeros((1 << lg_max, 4), dtype=np.uint64)
    ll = (C.c_size_t * A)(*lgs)
    hal._lib.dev_hook("check_combined_parts", parts)
    hal._lib.dev_hook("check_combined_cap", cap)
    try:
        assert c.lib.halo_dev_check_mixed_scalars(c.h, ptr(x), ll, ptr(cc.mont_words(w)), A, ptr(out)) == 0, c.lib.halo_last_error()
    finally:
        hal._lib.dev_hook("reset", 0)
    return out


LENGTH_SETS = {
    "two short tables": [1, 3],
    "below a block, a block, two blocks": [7, 8, 9],
    "unsorted with repeats": [3, 9, 9, 1, 8],
    "64 tables of lg 2..10": [2 + a % 9 for a in range(64)],
}


@pytest.mark.parametrize("name", list(LENGTH_SETS))
def test_mixed_scalars_equal_the_integer_sum(hal, ctx, name):
    lgs = LENGTH_SETS[name]
    xis, w = mixed_case(lgs)
    want = want_words(xis, lgs, w)
    for parts, cap in cc.splits(len(lgs)):
        got = mixed_scalars(hal, ctx, xis, lgs, w, parts, cap)
        assert np.array_equal(got, want), "parts %d, %d tables per pass: first difference at %d" % (parts, cap, int(np.argwhere(got != want)[0][0]))


def test_mixed_scalars_with_a_third_table_level_beside_a_short_table(hal, big):
    lgs = [17, 3]
    xis, w = mixed_case(lgs)
    w = [1, R_MOD - 1]  # (two tables take two of the three planted weights: not 0 on the short one, which would hide it)
    want = want_words(xis, lgs, w)
    assert any(int(v) for v in want[:8].ravel()) and not np.array_equal(want[:8], cc.mont_words(cc.h_poly(xis[0], 17)[:8]))
    for parts, cap in cc.splits(len(lgs)):
        assert np.array_equal(mixed_scalars(hal, big, xis, lgs, w, parts, cap), want), "parts %d, %d tables per pass" % (parts, cap)


@pytest.mark.parametrize("lg", [3, 9])
def test_tables_of_one_length_give_the_uniform_words(hal, ctx, lg):
    A = 5
    xis, w = cc.scalar_case(lg, A)
    uniform = cc.combined_scalars(hal, ctx, xis, w, lg, 0, 0)
    for parts, cap in cc.splits(A):
        assert np.array_equal(mixed_scalars(hal, ctx, xis, [lg] * A, w, parts, cap), uniform), (parts, cap)


def test_scalar_argument_errors(hal, ctx):
    x = np.zeros((2, 4, 4), dtype=np.uint64)
    out = np.zeros((8, 4), dtype=np.uint64)
    w = np.zeros((2, 4), dtype=np.uint64)
    E = hal._lib.HALO_E_ARG
    f = ctx.lib.halo_dev_check_mixed_scalars
    assert f(ctx.h, None, (C.c_size_t * 2)(3, 1), ptr(w), 2, ptr(out)) == E
    assert f(ctx.h, ptr(x), (C.c_size_t * 2)(3, 0), ptr(w), 2, ptr(out)) == E, "lg 0 has nothing to combine"
    assert f(ctx.h, ptr(x), (C.c_size_t * 2)(3, 15), ptr(w), 2, ptr(out)) == E, "above the key"
    assert f(ctx.h, ptr(x), (C.c_size_t * 2)(3, 1), ptr(w), 0, ptr(out)) == E


# ------------------------------------------------------------------ 2. an honest mixed batch: one relation, one MSM
def test_honest_mixed_batch_is_accepted_by_one_relation(hal, ctx):
    blobs = interleave(honest(ctx, 3, 3), honest(ctx, 9, 3), honest(ctx, 10, 2))
    assert [lg_of(q) for q in blobs] == [3, 9, 10, 3, 9, 10, 3, 9]
    (rc, st, _), counts = cc.profiled(ctx, lambda: mixed(ctx, blobs))
    assert rc == 0 and st == [0] * 8
    assert ran_mixed_only(counts), counts
    assert sequences(counts) == 1, "ONE MSM over the key for the members of every size: %r" % counts
    (rc, st, _), counts = cc.profiled(ctx, lambda: mixed(ctx, blobs, combined=False))
    assert rc == 0 and st == [0] * 8
    assert ran_exact_only(counts) and counts.get("k_h_tables_mixed", 0) == 0, counts
    assert mixed(ctx, blobs, seed=bytes(range(32))) == (0, [0] * 8, "")


def test_python_wrappers(hal, ctx):
    from halo_accumulation_amd import acc as A, pcdl
    blobs = interleave(honest(ctx, 3, 2), honest(ctx, 9, 2))
    accs = interleave(honest(ctx, 3, 2, acc=True), honest(ctx, 9, 2, acc=True))
    assert pcdl.check_batch_mixed(ctx, blobs) == [0] * 4
    assert pcdl.check_batch_mixed_combined(ctx, blobs, seed=bytes(range(32))) == [0] * 4
    assert A.decider_batch_mixed(ctx, accs) == [0] * 4
    assert A.decider_batch_mixed_combined(ctx, accs) == [0] * 4
    bad = list(blobs)
    bad[1] = cc.tamper(bad[1], 9, "v")
    with pytest.raises(hal._lib.HaloReject) as e:
        pcdl.check_batch_mixed_combined(ctx, bad)
    assert e.value.args[1] == [0, REJECT, 0, 0] and e.value.args[0].startswith("instance 1: ")


# ------------------------------------------------------------------ 3. rejects equal the single calls'
def test_rejects_equal_the_single_calls(hal, ctx):
    """one tampered member of every kind over the three classes, and one opened under another key, which only the MSM of
    pcdl.rs:338 rejects"""
    blobs = interleave(honest(ctx, 3, 3), honest(ctx, 9, 3), honest(ctx, 10, 3))  # lg 3, 9, 10, 3, 9, 10, 3, 9, 10
    for i, what in ((1, "U"), (2, "c"), (3, "L"), (5, "v"), (6, "C")):
        blobs[i] = cc.tamper(blobs[i], lg_of(blobs[i]), what)
    blobs[7] = cc.foreign(hal, 9, [0x7E57])[0]
    want = by_single_calls(ctx, blobs)
    assert [i for i, s in enumerate(want[1]) if s] == [1, 2, 3, 5, 6, 7] and want[0] == REJECT and want[2].startswith("instance 1: ")
    assert single(ctx, blobs[7])[1] == "U != CM.Commit(ck, h_vec)"
    assert mixed(ctx, blobs, combined=False) == want
    got, counts = cc.profiled(ctx, lambda: mixed(ctx, blobs))
    assert got == want
    assert counts.get("k_h_accumulate_mixed", 0) > 0 and counts.get("k_h_coeffs_batch", 0) > 0, "the relation, then the exact path: %r" % counts
    # the foreign member alone among honest ones: its index in THIS call is in the message
    few = [honest(ctx, 3, 1)[0], blobs[7], honest(ctx, 10, 1)[0]]
    for combined in (False, True):
        assert mixed(ctx, few, combined=combined) == (REJECT, [0, REJECT, 0], "instance 1: U != CM.Commit(ck, h_vec)")


def test_decider_rejects_equal_the_single_calls(hal, ctx):
    accs = interleave(honest(ctx, 3, 3, acc=True), honest(ctx, 9, 3, acc=True))  # lg 3, 9, 3, 9, 3, 9
    accs[2] = cc.tamper(accs[2], 3, "v")
    accs[3] = cc.tamper(accs[3], 9, "U")
    f = cc.foreign(hal, 9, [0x7E58])[0]
    accs[5] = np.concatenate([f, accs[5][len(f):]])  # (the decider checks the Instance prefix)
    want = by_single_calls(ctx, accs, acc=True)
    assert [i for i, s in enumerate(want[1]) if s] == [2, 3, 5] and want[2].startswith("instance 2: ")
    assert mixed(ctx, accs, acc=True, combined=False) == want
    assert mixed(ctx, accs, acc=True) == want
    good = interleave(honest(ctx, 3, 3, acc=True), honest(ctx, 9, 3, acc=True))
    (rc, st, _), counts = cc.profiled(ctx, lambda: mixed(ctx, good, acc=True))
    assert rc == 0 and st == [0] * 6 and ran_mixed_only(counts) and sequences(counts) == 1, counts


# ------------------------------------------------------------------ 4. defects that cancel across classes
def test_defects_that_cancel_across_classes_are_rejected(hal, ctx):
    """h[0] = 1 for every member of every size.  An instance of lg 3 opened under a key whose G_0 is G_0 + G_1 has
    U = <h, G> + G_1 under the true key, one of lg 9 opened with G_0 - G_1 has U = <h, G> - G_1: each alone fails pcdl.rs:339 and
    the two defects cancel, so the relation with all weights ONE would accept the pair.  The hashed weights must not."""
    from halo_accumulation_amd import acc as A, pcdl
    from halo_accumulation_amd._lib import point_sum
    n = 512
    gs = ctx.read_bases(0, n)
    g0, g1 = cc.to_jac(gs[0]), cc.to_jac(gs[1])
    neg_g1 = g1.copy()
    neg_g1[4:8] = cc.limbs(cc.P_MOD - cc.to_int(g1[4:8]))  # -y on the Montgomery limbs
    pair = []
    for k, (shift, lg) in enumerate(((g1, 3), (neg_g1, 9))):
        key = gs.copy()
        key[0] = cc.affine_of(point_sum(np.stack([g0, shift])))
        other = hal._lib.Context(np.ascontiguousarray(key))
        try:
            pair.append(A.random_instance(other, [0xCA9CE3 + k], (1 << lg) - 1))
        finally:
            other.close()
    # the construction: each alone is an MSM reject, and the unweighted relation holds
    Us, commits = [], []
    for q in pair:
        assert single(ctx, q) == (REJECT, "U != CM.Commit(ck, h_vec)")
        xis, U = pcdl.succinct_check(ctx, q[0:12].copy(), d_of(q), q[13:17].copy(), q[17:21].copy(), q[21:].copy())
        Us.append(U)
        commits.append(ctx.h_commit(xis))
    assert orc.point_canonical(point_sum(np.stack(commits))) == orc.point_canonical(point_sum(np.stack(Us)))
    assert orc.point_canonical(commits[0]) != orc.point_canonical(Us[0])
    want = (REJECT, [REJECT, REJECT], "instance 0: U != CM.Commit(ck, h_vec)")
    assert mixed(ctx, pair, combined=False) == want
    assert mixed(ctx, pair) == want
    assert mixed(ctx, pair, seed=bytes(range(32))) == want
    among = [honest(ctx, 9, 1)[0], pair[0], honest(ctx, 3, 1)[0], pair[1], honest(ctx, 10, 1)[0]]
    assert mixed(ctx, among) == mixed(ctx, among, combined=False) == (REJECT, [0, REJECT, 0, REJECT, 0], "instance 1: U != CM.Commit(ck, h_vec)")


# ------------------------------------------------------------------ 5. edges
def test_members_of_one_size_get_the_uniform_calls_statuses(hal, ctx):
    blobs = honest(ctx, 9, 6)
    blobs[2] = cc.tamper(blobs[2], 9, "c")
    blobs[4] = cc.foreign(hal, 9, [0x7E59])[0]
    uniform = cc.call(ctx, 511, blobs)
    assert uniform[1] == [0, 0, REJECT, 0, REJECT, 0]
    assert mixed(ctx, blobs) == uniform and mixed(ctx, blobs, combined=False) == uniform
    (rc, st, _), counts = cc.profiled(ctx, lambda: mixed(ctx, honest(ctx, 9, 6)))
    assert rc == 0 and st == [0] * 6 and ran_mixed_only(counts) and sequences(counts) == 1, counts


def test_a_class_of_one_beside_a_class_of_four(hal, ctx):
    blobs = honest(ctx, 9, 4)
    blobs.insert(2, honest(ctx, 3, 1)[0])
    (rc, st, _), counts = cc.profiled(ctx, lambda: mixed(ctx, blobs))
    assert rc == 0 and st == [0] * 5 and ran_mixed_only(counts) and sequences(counts) == 1, counts
    blobs[2] = cc.tamper(blobs[2], 3, "U")
    assert mixed(ctx, blobs) == mixed(ctx, blobs, combined=False) == by_single_calls(ctx, blobs)
    assert mixed(ctx, blobs)[1] == [0, 0, REJECT, 0, 0]


def constant_instance(hal, c):
    """An Instance of degree bound 0, written by hand (random_instance starts at d = 2): p(X) = 1 without hiding, so C = G_0, and
    the proof of no rounds is U = G_0, c = 1.  At z = 0, v = p(0) = 1 and HPoly::eval's first factor 1 + xi_0 z is 1, the value of
    the constant h: C + v H' = c U + c h(z) H' (pcdl.rs:288-310), and <h, G[0 .. 1)> = G_0 = U (:338-339)."""
    g0 = cc.to_jac(c.read_bases(0, 1)[0])
    one = np.array(cc.limbs(cc.MONT % R_MOD), dtype=np.uint64)
    q = np.zeros(int(c.lib.halo_instance_words(0)), dtype=np.uint64)
    q[0:12] = g0        # C
    q[12] = 0           # d
    q[13:17] = 0        # z
    q[17:21] = one      # v
    q[21], q[22] = 0, 0  # the proof: not hiding, lg = 0
    q[23:35] = g0       # U
    q[35:39] = one      # c
    return q


def test_a_constant_takes_the_exact_path_beside_the_relation(hal, ctx):
    const = constant_instance(hal, ctx)
    assert d_of(const) == 0 and single(ctx, const) == (0, ""), "the construction: an Instance of d = 0 the single call accepts"
    blobs = [honest(ctx, 9, 1)[0], const, honest(ctx, 3, 1)[0], honest(ctx, 9, 2)[1]]
    want = by_single_calls(ctx, blobs)
    assert want[1][0] == want[1][2] == want[1][3] == 0
    got, counts = cc.profiled(ctx, lambda: mixed(ctx, blobs))
    assert got == want
    assert counts.get("k_h_accumulate_mixed", 0) > 0, "the three members with d >= 1 are combined: %r" % counts
    if want[1][1] == 0:
        assert counts.get("k_h_coeffs_batch", 0) > 0 and sequences(counts) == 2, "the constant's own exact MSM: %r" % counts
    assert mixed(ctx, blobs, combined=False) == want
    # a constant and ONE other member: nothing to combine
    got, counts = cc.profiled(ctx, lambda: mixed(ctx, blobs[:2]))
    assert got == by_single_calls(ctx, blobs[:2]) and counts.get("k_h_accumulate_mixed", 0) == 0, counts


def test_no_member_and_one_member(hal, ctx):
    for acc in (False, True):
        for combined in (False, True):
            assert mixed(ctx, [], acc=acc, combined=combined) == (0, [], "")
            q = honest(ctx, 9, 1, acc=acc)[0]
            (rc, st, _), counts = cc.profiled(ctx, lambda: mixed(ctx, [q], acc=acc, combined=combined))
            assert rc == 0 and st == [0] and ran_exact_only(counts), counts
    fn = ctx.lib.halo_pcdl_check_batch_mixed_combined
    assert fn(ctx.h, None, None, 0, None, None) == 0
    q = np.ascontiguousarray(honest(ctx, 9, 1)[0])
    assert fn(ctx.h, (C.c_size_t * 1)(511), (C.c_void_p * 1)(q.ctypes.data), 1, None, None) == 0, "status is nullable"


def test_whole_call_errors_leave_status_untouched(hal, ctx):
    E = hal._lib.HALO_E_ARG
    a, b = honest(ctx, 3, 1)[0], honest(ctx, 9, 1)[0]
    a_acc, b_acc = honest(ctx, 3, 1, acc=True)[0], honest(ctx, 9, 1, acc=True)[0]
    for acc, (x, y) in ((False, (a, b)), (True, (a_acc, b_acc))):
        for combined in (False, True):
            names = ("halo_acc_decider_batch_mixed" if acc else "halo_pcdl_check_batch_mixed") + ("_combined" if combined else "")
            fn = getattr(ctx.lib, names)
            seed = (None,) if combined else ()
            st = (C.c_int * 2)(77, 77)
            x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
            ds, ps = (C.c_size_t * 2)(7, 511), (C.c_void_p * 2)(x.ctypes.data, y.ctypes.data)
            assert fn(ctx.h, None, ps, 2, *seed, st) == E
            assert fn(ctx.h, ds, None, 2, *seed, st) == E
            assert fn(ctx.h, ds, (C.c_void_p * 2)(x.ctypes.data, None), 2, *seed, st) == E
            assert list(st) == [77, 77]
            # d + 1 not a power of two; a blob whose d word, or whose proof's lg word, disagrees with ds[i]
            assert mixed(ctx, [x, y], acc, combined, ds=[7, 510]) == (REJECT, [77, 77], "d+1 is not a power of 2!")
            assert mixed(ctx, [x, y], acc, combined, ds=[7, 255]) == (REJECT, [77, 77], "d_i != d")
            assert mixed(ctx, [x, y], acc, combined, ds=[511, 7]) == (REJECT, [77, 77], "d_i != d")
            other = y.copy()
            other[22] = 8
            assert mixed(ctx, [x, other], acc, combined) == (REJECT, [77, 77], "d_i != d")
            assert mixed(ctx, [x, y], acc, combined) == (0, [0, 0], "")


def test_without_staging_the_exact_path_runs(hal, ctx):
    blobs = interleave(honest(ctx, 3, 3), honest(ctx, 9, 3))
    blobs[2] = cc.tamper(blobs[2], 3, "v")
    blobs[3] = cc.foreign(hal, 9, [0x7E5A])[0]
    want = mixed(ctx, blobs, combined=False)
    assert want == by_single_calls(ctx, blobs) and want[1] == [0, 0, REJECT, REJECT, 0, 0]
    hal._lib.dev_hook("batch_stage_fail", 1)
    try:
        got, counts = cc.profiled(ctx, lambda: mixed(ctx, blobs))
        ok, counts_ok = cc.profiled(ctx, lambda: mixed(ctx, blobs[:2]))
    finally:
        hal._lib.dev_hook("reset", 0)
    assert got == want and ran_exact_only(counts), counts
    assert ok == (0, [0, 0], "") and ran_exact_only(counts_ok), counts_ok


def test_beside_a_callers_msm(hal, ctx):
    import torch
    blobs = interleave(honest(ctx, 3, 3), honest(ctx, 9, 3), honest(ctx, 10, 3))
    n = 1 << 14
    sc, _ = orc.rng_scalars(0xC0FFEE, n)
    dev = torch.from_numpy(sc.view(np.int64).reshape(-1).copy()).cuda()
    expect = orc.msm_affine(ctx.read_bases(), sc).tolist()

    def beside():  # (the profiler reports once every slot is idle again: the caller's MSM is collected inside its bracket)
        ctx.msm_dev_begin(1, dev.data_ptr(), n)
        try:
            return mixed(ctx, blobs)
        finally:
            got.append(ctx.msm_dev_end(1))

    got = []
    (rc, st, _), counts = cc.profiled(ctx, beside)
    assert rc == 0 and st == [0] * 9 and ran_mixed_only(counts), counts
    assert got[0].tolist() == expect, "the caller's MSM on slot 1 kept its own result"
    assert mixed(ctx, blobs) == (0, [0] * 9, ""), "and again (the second call replays its launch graphs)"
    for slot in range(4):
        ctx.msm_dev_begin(slot, dev.data_ptr(), n)
    try:
        busy = mixed(ctx, blobs)
        busy_exact = mixed(ctx, blobs, combined=False)
    finally:
        for slot in range(4):
            assert ctx.msm_dev_end(slot).tolist() == expect
    assert busy == busy_exact and busy[0] == hal._lib.HALO_E_ARG and busy[1] == [77] * 9, "no idle slot"


def test_right_side_on_the_pool_and_on_the_device(hal, ctx):
    good = interleave(honest(ctx, 3, 33), honest(ctx, 9, 33))
    assert len(good) == 66
    bad = list(good)
    bad[41] = cc.foreign(hal, 9, [0x7E5B])[0]
    assert lg_of(good[41]) == 9
    want_bad = mixed(ctx, bad, combined=False)
    assert [i for i, s in enumerate(want_bad[1]) if s] == [41]
    for usum in (1, 2):
        hal._lib.dev_hook("check_combined_usum", usum)
        try:
            (rc, st, _), counts = cc.profiled(ctx, lambda: mixed(ctx, good))
            assert rc == 0 and st == [0] * 66 and ran_mixed_only(counts), (usum, counts)
            assert (counts.get("k_batch_to_affine", 0) > 0) == (usum == 2), (usum, counts)
            assert mixed(ctx, bad) == want_bad, usum
        finally:
            hal._lib.dev_hook("reset", 0)
    (rc, st, _), counts = cc.profiled(ctx, lambda: mixed(ctx, good))
    assert rc == 0 and st == [0] * 66 and counts.get("k_batch_to_affine", 0) > 0, "64 accepted members or more: the device's sum by default"


# ------------------------------------------------------------------ 6. the table pipeline as the one MSM
def test_the_table_pipeline_is_the_one_msm(hal, big, big_members):
    long_one, short = big_members
    blobs = [short[0], long_one, short[1], short[2]]
    mixed(big, blobs)  # (the first MSM of 2^20 points builds the key's table)
    (rc, st, _), counts = cc.profiled(big, lambda: mixed(big, blobs))
    assert rc == 0 and st == [0] * 4 and ran_mixed_only(counts), counts
    assert counts.get("k_tmsm_recode", 0) == 1 and sequences(counts) == 1, "one MSM, through the table pipeline: %r" % counts
    bad = list(blobs)
    bad[2] = cc.tamper(bad[2], 10, "U")
    want = mixed(big, bad, combined=False)
    assert want[1] == [0, 0, REJECT, 0] and want[2] == "instance 2: " + single(big, bad[2])[1]
    assert mixed(big, bad) == want
