"""halo_pcdl_check_batch_combined / halo_acc_decider_batch_combined on the GPU: the combined scalars sum_a r_a h_a(X) limb for limb
against Python integers under every split into parts and passes; honest batches accepted by ONE MSM (the profiler shows which
path ran); succinct and MSM rejects with the exact batch's statuses, code and message; a pair of members whose unweighted defects
cancel; both sides of the right-hand sum; company on the slots, the fallbacks, a multi-device context and the full-size key."""
import ctypes as C

import numpy as np
import pytest

import orc

pytestmark = pytest.mark.gpu

R_MOD = 0x40000000000000000000000000000000224698FC0994A8DD8C46EB2100000001  # the scalar field
P_MOD = 0x40000000000000000000000000000000224698FC094CF91B992D30ED00000001  # the base field
MONT = 1 << 256


@pytest.fixture(scope="module")
def hal():
    import halo_accumulation_amd as h
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


def ptr(a):
    from halo_accumulation_amd._lib import ptr as p
    return p(a)


def limbs(v):
    return [(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)]


def to_int(w):
    return sum(int(w[k]) << (64 * k) for k in range(4))


def call(c, d, blobs, acc=False, combined=True, seed=None):
    """-> (return code, status list, message); status entries the call does not write stay 77"""
    m = len(blobs)
    qs = np.ascontiguousarray(np.concatenate(blobs))
    st = (C.c_int * m)(*([77] * m))
    if combined:
        fn = c.lib.halo_acc_decider_batch_combined if acc else c.lib.halo_pcdl_check_batch_combined
        rc = fn(c.h, d, ptr(qs), m, seed, st)
    else:
        fn = c.lib.halo_acc_decider_batch if acc else c.lib.halo_pcdl_check_batch
        rc = fn(c.h, d, ptr(qs), m, st)
    return rc, [st[i] for i in range(m)], (c.lib.halo_last_error().decode() if rc else "")


def profiled(c, fn):
    """-> (fn(), the launch count of every kernel it ran)"""
    c.prof_enable(1)
    try:
        c.prof_reset()
        out = fn()
        counts = {name: cnt for name, (_, cnt) in c.prof().items() if cnt}
    finally:
        c.prof_enable(0)
    return out, counts


def ran_combined(counts):
    return counts.get("k_h_accumulate_batch", 0) > 0 and counts.get("k_h_coeffs_batch", 0) == 0


def parts_for(hal, n, A):
    """the product's rule restated: one row of parts is 4 waves per block of the h-coefficient plan; enough parts for 1024 waves"""
    waves = 4 * hal._lib.fr_plan("h_coeffs", n)["blocks"]
    return max(1, min(A, -(-1024 // waves)))


def ran_exact_only(counts):
    return counts.get("k_h_accumulate_batch", 0) == 0 and counts.get("k_h_coeffs_batch", 0) > 0


def plain_instance(c, seed, d):
    from halo_accumulation_amd import pcdl
    coeffs, s = orc.rng_scalars(seed, d + 1 - (seed % 3))
    z, _ = orc.rng_scalars(s, 1)
    Cm = pcdl.commit(c, coeffs, d)
    pi = pcdl.open(c, [seed], coeffs, Cm, d, z[0])
    v = c.poly_eval(coeffs, z[0])
    return np.concatenate([Cm, np.array([d], dtype=np.uint64), z[0], v, pi])


def tamper(q, lg, what):
    """one bit of a field of the Instance.  L: the LAST round's -- random_instance draws the degree, and below n / 2 the first
    round's L is the point at infinity, which a flipped X limb leaves where it is"""
    q = q.copy()
    off = {"U": 21 + 2 + 24 * lg, "c": 21 + 2 + 24 * lg + 12, "L": 21 + 2 + 12 * (lg - 1), "v": 17, "C": 0}[what]
    q[off] ^= 1
    return q


_POOLS = {}


def pool(c, lg):
    """65 honest Instances of degree bound 2^lg - 1 (hiding ones from random_instance_batch, every seventh from index 1 plain) and
    65 honest Accumulators (acc::prover over one of the Instances each), built once per size"""
    if lg not in _POOLS:
        from halo_accumulation_amd import acc as A
        d = (1 << lg) - 1
        qs = A.random_instance_batch(c, [0xC0B1 + lg], d, 65)
        for i in range(1, 65, 7):
            qs[i] = plain_instance(c, 400 + i, d)
        accs, codes = A.prover_batch(c, [0xACC + lg], d, [[q] for q in qs])
        assert codes == [0] * 65
        _POOLS[lg] = (qs, accs)
    return _POOLS[lg]


def foreign(hal, lg, seeds, size=1 << 14):
    """Instances opened under another key: their succinct half holds under any key, only the MSM of pcdl.rs:338 tells"""
    from halo_accumulation_amd import acc as A
    other = hal._lib.Context(urs_n=size, first_index=1 << 30)
    try:
        return [A.random_instance(other, [s], (1 << lg) - 1) for s in seeds]
    finally:
        other.close()


# ------------------------------------------------------------------ 1. the combined scalars against big integers
def h_poly(xis, lg):
    """coefficient k = the product of xis[lg - i] over the set bits i of k (pcdl.rs:496-505), integers mod r"""
    h = [1]
    for i in range(lg):
        h = h + [v * xis[lg - i] % R_MOD for v in h]
    return h


def scalar_case(lg, A):
    xs, s = orc.rng_scalars(0x5CA1A + 97 * lg + A, A * (lg + 1))
    ws, _ = orc.rng_scalars(s, A)
    xis = [[orc.fr_from_mont(xs[a * (lg + 1) + k]) for k in range(lg + 1)] for a in range(A)]
    w = [orc.fr_from_mont(ws[a]) for a in range(A)]
    special = [0, 1, R_MOD - 1]
    for a in range(min(A, 3)):
        w[a] = special[(a + lg) % 3]
    xis[0][lg] = R_MOD - 1
    if A > 1 or lg > 1:
        xis[A - 1][1] = 0
    return xis, w


def mont_words(vals):
    return np.array([limbs(v * MONT % R_MOD) for v in vals], dtype=np.uint64)


def combined_scalars(hal, c, xis, w, lg, parts, cap):
    A = len(w)
    x = np.ascontiguousarray(mont_words([v for row in xis for v in row]).reshape(A, lg + 1, 4))
    out = np.zeros((1 << lg, 4), dtype=np.uint64)
    hal._lib.dev_hook("check_combined_parts", parts)
    hal._lib.dev_hook("check_combined_cap", cap)
    try:
        assert c.lib.halo_dev_check_combined_scalars(c.h, ptr(x), ptr(mont_words(w)), A, lg, ptr(out)) == 0, c.lib.halo_last_error()
    finally:
        hal._lib.dev_hook("reset", 0)
    return out


def splits(A):
    """(parts, tables per pass): parts 1, 2, 3 and A -- one that does not divide A, one above A where A < 3 (clamped) -- under
    passes of 1, A - 1 and A tables; 0 / 0 is the product's own choice"""
    return [(0, 0)] + [(p, cap) for p in sorted({1, 2, 3, A}) for cap in sorted({1, max(A - 1, 1), A})]


@pytest.mark.parametrize("lg", [1, 3, 8, 9])
@pytest.mark.parametrize("A", [1, 2, 5, 64])
def test_combined_scalars_equal_the_integer_sum(hal, ctx, lg, A):
    xis, w = scalar_case(lg, A)
    want = [0] * (1 << lg)
    for a in range(A):
        for k, v in enumerate(h_poly(xis[a], lg)):
            want[k] = (want[k] + w[a] * v) % R_MOD
    want = mont_words(want).tolist()
    for parts, cap in splits(A):
        assert combined_scalars(hal, ctx, xis, w, lg, parts, cap).tolist() == want, "parts %d, %d tables per pass" % (parts, cap)


@pytest.mark.parametrize("lg", [16, 17])
def test_combined_scalars_with_a_third_table_equal_accumulate_passes(hal, big, lg):
    A = 3
    xis, w = scalar_case(lg, A)
    x = np.ascontiguousarray(mont_words([v for row in xis for v in row]).reshape(A, lg + 1, 4))
    want = big.h_accumulate(None, x, mont_words(w)).tolist()  # (one k_h_coeffs accumulate pass per polynomial)
    for parts, cap in splits(A):
        assert combined_scalars(hal, big, xis, w, lg, parts, cap).tolist() == want, "parts %d, %d tables per pass" % (parts, cap)


# ------------------------------------------------------------------ 2. honest batches: one MSM
@pytest.mark.parametrize("lg", [3, 8, 9, 14])
@pytest.mark.parametrize("m", [2, 5, 64, 65])
@pytest.mark.parametrize("acc", [False, True], ids=["pcdl", "decider"])
def test_honest_batches_are_accepted_by_the_combined_relation(hal, ctx, lg, m, acc):
    d = (1 << lg) - 1
    blobs = pool(ctx, lg)[1 if acc else 0][:m]  # (members 1, 8, .. of the Instances are plain, the others hiding)
    (rc, st, _), counts = profiled(ctx, lambda: call(ctx, d, blobs, acc))
    assert rc == 0 and st == [0] * m
    assert ran_combined(counts), counts
    assert counts.get("k_fr_sum_rows", 0) == (1 if parts_for(hal, 1 << lg, m) > 1 else 0), "one launch adds the parts' rows; one part needs none"


@pytest.mark.parametrize("acc", [False, True], ids=["pcdl", "decider"])
def test_one_member_takes_the_exact_path(hal, ctx, acc):
    blobs = pool(ctx, 9)[1 if acc else 0][:1]
    (rc, st, _), counts = profiled(ctx, lambda: call(ctx, 511, blobs, acc))
    assert rc == 0 and st == [0]
    assert ran_exact_only(counts), counts


def test_python_wrappers(hal, ctx):
    from halo_accumulation_amd import acc as A, pcdl
    qs, accs = pool(ctx, 9)
    assert pcdl.check_batch_combined(ctx, 511, qs[:5]) == [0] * 5
    assert A.decider_batch_combined(ctx, 511, accs[:5], seed=bytes(range(32))) == [0] * 5
    with pytest.raises(hal._lib.HaloReject) as e:
        pcdl.check_batch_combined(ctx, 511, [qs[0], tamper(qs[1], 9, "v"), qs[2]])
    assert e.value.args[1] == [0, hal._lib.HALO_E_REJECT, 0]
    with pytest.raises(ValueError):
        pcdl.check_batch_combined(ctx, 511, qs[:2], seed=b"short")


# ------------------------------------------------------------------ 3. succinct rejects stay out of the relation
@pytest.mark.parametrize("lg", [3, 9])
def test_succinct_rejects_stay_out(hal, ctx, lg):
    d = (1 << lg) - 1
    blobs = list(pool(ctx, lg)[0][:12])
    for i, what in zip((0, 4, 7, 11), ("v", "C", "L", "c")):
        blobs[i] = tamper(blobs[i], lg, what)
    want = call(ctx, d, blobs, combined=False)
    assert [i for i, s in enumerate(want[1]) if s] == [0, 4, 7, 11] and want[2].startswith("instance 0: ")
    got, counts = profiled(ctx, lambda: call(ctx, d, blobs))
    assert got == want
    assert ran_combined(counts), "the eight honest members are still accepted by one MSM: %r" % counts


# ------------------------------------------------------------------ 4. an MSM reject: the exact batch's statuses
@pytest.mark.parametrize("where", [[0], [3], [6], [2, 5]])
def test_msm_rejects_get_the_exact_statuses(hal, ctx, where):
    lg, d = 9, 511
    blobs = list(pool(ctx, lg)[0][:7])
    for i, q in zip(where, foreign(hal, lg, [900 + i for i in where])):
        blobs[i] = q
    want = call(ctx, d, blobs, combined=False)
    assert [i for i, s in enumerate(want[1]) if s] == where and want[0] == hal._lib.HALO_E_REJECT
    assert want[2] == "instance %d: U != CM.Commit(ck, h_vec)" % where[0]
    got, counts = profiled(ctx, lambda: call(ctx, d, blobs))
    assert got == want
    assert counts.get("k_h_accumulate_batch", 0) > 0 and counts.get("k_h_coeffs_batch", 0) > 0, "the combined relation, then the exact path"
    accs = list(pool(ctx, lg)[1][:7])
    for i in where:
        accs[i] = np.concatenate([blobs[i], accs[i][len(blobs[i]):]])  # (the decider checks the Instance prefix)
    assert call(ctx, d, accs, acc=True) == call(ctx, d, accs, acc=True, combined=False)


# ------------------------------------------------------------------ 5. a pair whose unweighted defects cancel
def affine_of(jac):
    x, y = orc.point_canonical(jac)
    return np.array(limbs(x * MONT % P_MOD) + limbs(y * MONT % P_MOD), dtype=np.uint64)


def to_jac(aff):
    j = np.zeros(12, dtype=np.uint64)
    orc.lib().orc_affine_to_jac(orc.ptr(np.ascontiguousarray(aff)), orc.ptr(j))
    return j


def test_cancelling_pair_is_rejected(hal, ctx):
    """h_i[0] = 1 for every member.  An instance opened under a key whose G_0 is G_0 + G_1 has U = <h, G> + G_1 under the true key,
    one opened with G_0 - G_1 has U = <h, G> - G_1: each alone fails pcdl.rs:339 and the two defects cancel, so the relation with
    all weights ONE would accept the pair.  The hashed weights must not."""
    from halo_accumulation_amd import acc as A, pcdl
    from halo_accumulation_amd._lib import point_sum
    lg, d, n = 8, 255, 256
    gs = ctx.read_bases(0, n)
    g0, g1 = to_jac(gs[0]), to_jac(gs[1])
    neg_g1 = g1.copy()
    neg_g1[4:8] = limbs(P_MOD - to_int(g1[4:8]))  # -y on the Montgomery limbs
    pair = []
    for k, shift in enumerate((g1, neg_g1)):
        key = gs.copy()
        key[0] = affine_of(point_sum(np.stack([g0, shift])))
        other = hal._lib.Context(np.ascontiguousarray(key))
        try:
            pair.append(A.random_instance(other, [0xCA9CE1 + k], d))
        finally:
            other.close()
    # the construction: each alone is an MSM reject, and the unweighted relation holds
    Us, commits = [], []
    for q in pair:
        assert call(ctx, d, [q], combined=False)[1] == [hal._lib.HALO_E_REJECT]
        xis, U = pcdl.succinct_check(ctx, q[0:12].copy(), d, q[13:17].copy(), q[17:21].copy(), q[21:].copy())
        Us.append(U)
        commits.append(ctx.h_commit(xis))
    assert orc.point_canonical(point_sum(np.stack(commits))) == orc.point_canonical(point_sum(np.stack(Us)))
    assert orc.point_canonical(commits[0]) != orc.point_canonical(Us[0])
    want = call(ctx, d, pair, combined=False)
    assert want[1] == [hal._lib.HALO_E_REJECT] * 2
    assert call(ctx, d, pair) == want
    assert call(ctx, d, pair, seed=bytes(range(32))) == want
    honest = pool(ctx, lg)[0]
    mixed = [honest[0], pair[0], honest[1], pair[1], honest[2]]
    assert call(ctx, d, mixed) == call(ctx, d, mixed, combined=False)


# ------------------------------------------------------------------ 6. the right side on the pool and on the device
@pytest.mark.parametrize("m", [2, 4, 5])
def test_right_side_on_the_pool_and_on_the_device(hal, ctx, m):
    """(No member here has U at infinity: U is read from the proof, and the succinct half accepts it only if c U + c v' H' equals
    the folded commitment C_lg -- a proof whose C_lg lies in the span of H' alone.  Without a break of the commitment's binding
    none can be built, so the two sums are held equal on finite points.)"""
    lg, d = 9, 511
    honest = list(pool(ctx, lg)[0][:m])
    bad = list(honest)
    bad[m - 1] = foreign(hal, lg, [950 + m])[0]
    want_bad = call(ctx, d, bad, combined=False)
    for usum in (1, 2):
        hal._lib.dev_hook("check_combined_usum", usum)
        try:
            (rc, st, _), counts = profiled(ctx, lambda: call(ctx, d, honest))
            assert rc == 0 and st == [0] * m and ran_combined(counts), (usum, counts)
            assert (counts.get("k_batch_to_affine", 0) > 0) == (usum == 2), (usum, counts)
            assert call(ctx, d, bad) == want_bad, usum
        finally:
            hal._lib.dev_hook("reset", 0)


# ------------------------------------------------------------------ 7. company and fallbacks
def test_without_staging_the_exact_path_runs(hal, ctx):
    lg, d = 9, 511
    blobs = list(pool(ctx, lg)[0][:6])
    blobs[2] = tamper(blobs[2], lg, "v")
    blobs[4] = foreign(hal, lg, [977])[0]
    want = call(ctx, d, blobs, combined=False)
    hal._lib.dev_hook("batch_stage_fail", 1)
    try:
        got, counts = profiled(ctx, lambda: call(ctx, d, blobs))
        ok, counts_ok = profiled(ctx, lambda: call(ctx, d, blobs[:2]))
    finally:
        hal._lib.dev_hook("reset", 0)
    assert got == want and ran_exact_only(counts), counts
    assert ok == (0, [0, 0], "") and ran_exact_only(counts_ok), counts_ok


def test_beside_a_callers_msm(hal, ctx):
    import torch
    lg, d = 9, 511
    blobs = list(pool(ctx, lg)[0][:9])
    n = 1 << 14
    sc, _ = orc.rng_scalars(0xC0FFEE, n)
    dev = torch.from_numpy(sc.view(np.int64).reshape(-1).copy()).cuda()
    expect = orc.msm_affine(ctx.read_bases(), sc).tolist()
    def beside():  # (the profiler reports once every slot is idle again: the caller's MSM is collected inside its bracket)
        ctx.msm_dev_begin(1, dev.data_ptr(), n)
        try:
            return call(ctx, d, blobs)
        finally:
            got.append(ctx.msm_dev_end(1))

    got = []
    (rc, st, _), counts = profiled(ctx, beside)
    got = got[0]
    assert rc == 0 and st == [0] * 9 and ran_combined(counts), counts
    assert got.tolist() == expect, "the caller's MSM on slot 1 kept its own result"
    assert call(ctx, d, blobs) == (0, [0] * 9, ""), "and again (the second call replays its launch graphs)"
    for slot in range(4):
        ctx.msm_dev_begin(slot, dev.data_ptr(), n)
    try:
        busy = call(ctx, d, blobs)
        busy_exact = call(ctx, d, blobs, combined=False)
    finally:
        for slot in range(4):
            assert ctx.msm_dev_end(slot).tolist() == expect
    assert busy == busy_exact and busy[0] == hal._lib.HALO_E_ARG and busy[1] == [77] * 9, "no idle slot"


def test_multi_device_context_and_a_seed(hal, ctx):
    lg, d = 9, 511
    blobs = list(pool(ctx, lg)[0][:8])
    blobs[5] = foreign(hal, lg, [988])[0]
    want = call(ctx, d, blobs, combined=False)
    seed = bytes(range(100, 132))
    assert call(ctx, d, blobs, seed=seed) == want
    assert call(ctx, d, blobs[:5], seed=seed) == (0, [0] * 5, "")
    m = hal._lib.Context(urs_n=1 << 14, devices=[0, 0])
    try:
        assert call(m, d, blobs) == want
        (rc, st, _), counts = profiled(m, lambda: call(m, d, blobs[:5]))
        assert rc == 0 and st == [0] * 5 and ran_combined(counts), counts
    finally:
        m.close()


def test_argument_errors_are_the_exact_batchs(hal, ctx):
    d = 511
    q = pool(ctx, 9)[0][0]
    st = (C.c_int * 2)(77, 77)
    for fn in (ctx.lib.halo_pcdl_check_batch_combined, ctx.lib.halo_acc_decider_batch_combined):
        assert fn(ctx.h, d, None, 2, None, st) == hal._lib.HALO_E_ARG
        assert fn(ctx.h, d, None, 0, None, None) == 0
    other = q.copy()
    other[12] = 255
    assert call(ctx, d, [q, other]) == call(ctx, d, [q, other], combined=False)
    assert call(ctx, d, [q, other])[1] == [77, 77], "rejected before any work, status untouched"
    assert call(ctx, 510, [q, q]) == call(ctx, 510, [q, q], combined=False)
    qs = np.ascontiguousarray(np.concatenate([q, q]))
    assert ctx.lib.halo_pcdl_check_batch_combined(ctx.h, d, ptr(qs), 2, None, None) == 0, "status is nullable"


# ------------------------------------------------------------------ 8. full size, once
def test_full_size(hal, big):
    from halo_accumulation_amd import acc as A
    lg = 20
    d = (1 << lg) - 1
    honest = A.random_instance_batch(big, [0xF0115], d, 3)
    (rc, st, _), counts = profiled(big, lambda: call(big, d, honest))
    assert rc == 0 and st == [0] * 3 and ran_combined(counts), counts
    assert counts.get("k_fr_sum_rows", 0) == (1 if parts_for(hal, 1 << lg, 3) > 1 else 0)
    blobs = honest[:2] + foreign(hal, lg, [0xF0E16], size=1 << 20) + honest[2:]
    want = call(big, d, blobs, combined=False)
    assert want[1] == [0, 0, hal._lib.HALO_E_REJECT, 0]
    assert call(big, d, blobs) == want
