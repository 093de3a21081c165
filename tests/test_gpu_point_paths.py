"""The kernels that take points from the caller, and the one that derives the key, on the GPU over the cases of tests/point_cases.py
(which test themselves in tests/test_point_cases_cpu.py); every reference is exact.

    k_batch_to_affine   every output of every group through halo_dev_batch_to_affine against pallas_model.jacobian_to_affine, and
                        halo_msm_points over the same inputs against orc.msm_jac; each twice
    k_batch_small_msm   every case through halo_dev_batch_small_msm, in launches of 1, 2 and 65 pairwise different sums
    k_small_msm_seg     every case through halo_dev_small_msm_seg, in lists that mix the widths
    k_urs_scalars, k_urs   a context for every (first index, stride, n) through halo_ctx_create_urs and _strided, all of read_bases
    verdicts            64 instances at n = 2^10 whose proof points are tampered into exceptional ones: device path, host path,
                        single calls and the oracle agree, status for status and message for message"""
import ctypes as C

import numpy as np
import pytest

import orc
import point_cases as pc
import table_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hal():
    import halo_accumulation_amd as h
    return h


@pytest.fixture(scope="module")
def ctx(hal):
    c = hal._lib.Context(urs_n=1 << 12)
    yield c
    c.close()


def ptr(a):
    from halo_accumulation_amd._lib import ptr as p
    return p(a)


# ---------------------------------------------------------------------------------------------------- batch-to-affine
N_GROUPS = 2 + 2 * len(pc.RAGGED_SIZES)


@pytest.mark.parametrize("gi", range(N_GROUPS))
def test_batch_to_affine_every_output(ctx, gi):
    g = pc.jac_groups()[gi]
    compared = 0
    for rep in range(2):
        bad = pc.check_affine(ctx.batch_to_affine(g.jac), g)
        assert not bad, "%s, run %d: %d wrong; first (index, class): %s" % (g.name, rep, len(bad), bad[:8])
        compared += g.m
    print("%s: %d points compared" % (g.name, compared))
    assert compared == 2 * g.m


def test_batch_to_affine_compared_every_group():
    groups = pc.jac_groups()
    assert len(groups) == N_GROUPS and sum(g.m for g in groups) == sum(pc.STEP_SIZES) + 2 * sum(pc.RAGGED_SIZES)


@pytest.mark.parametrize("gi", range(N_GROUPS))
def test_msm_points_over_the_same_inputs(ctx, gi):
    g = pc.jac_groups()[gi]
    sc, _ = orc.rng_scalars(0x6D736D + gi, g.m)
    want = orc.msm_jac(g.jac, sc).tolist()
    assert want == orc.msm_affine(g.want, sc).tolist(), "the oracle reads the same points from both forms"
    for rep in range(2):
        assert ctx.msm_points(g.jac, sc).tolist() == want, "%s, run %d" % (g.name, rep)


def test_msm_points_of_nothing(ctx):
    none = np.zeros((0, 12), dtype=np.uint64)
    want = orc.msm_jac(none, np.zeros((0, 4), dtype=np.uint64))
    assert orc.point_canonical(want) is None
    for rep in range(2):
        assert ctx.msm_points(none, np.zeros((0, 4), dtype=np.uint64)).tolist() == want.tolist()
    assert ctx.batch_to_affine(none).shape == (0, 8)


# ---------------------------------------------------------------------------------------------------- the two small MSMs
@pytest.mark.parametrize("K", pc.BATCH_K)
def test_batch_small_msm_every_case(ctx, K):
    launches = [l for k, l in pc.batch_launches() if k == K]
    assert sorted({len(l) for l in launches}) == pc.BATCH_M
    compared = 0
    for n, cases in enumerate(launches):
        got = ctx.batch_small_msm(np.concatenate([c.points() for c in cases]), np.concatenate([c.scalars() for c in cases]), K)
        bad = pc.check_sums(got, cases)
        assert not bad, "K = %d, launch %d of %d sums: %s" % (K, n, len(cases), pc.describe(bad))
        compared += len(cases)
    print("K = %d: %d launches, %d sums compared" % (K, len(launches), compared))
    assert compared == sum(len(l) for l in launches) >= sum(pc.BATCH_M)


def test_batch_small_msm_ran_every_case():
    placed = {id(c) for _, l in pc.batch_launches() for c in l}
    mine = [c for c in pc.msm_cases() if c.K in pc.BATCH_K]
    assert len(mine) >= 100 and all(id(c) in placed for c in mine)


def test_batch_small_msm_refuses_misuse(hal, ctx):
    lib, E_ARG = ctx.lib, hal._lib.HALO_E_ARG
    pts, sc, out = np.zeros((65, 8), dtype=np.uint64), np.zeros((65, 4), dtype=np.uint64), np.zeros((1, 12), dtype=np.uint64)
    for K in (0, 65):
        assert lib.halo_dev_batch_small_msm(ctx.h, ptr(pts), ptr(sc), 1, K, ptr(out)) == E_ARG
        assert lib.halo_last_error() == b"batch_small_msm: 1..64 terms per sum"
    assert lib.halo_dev_batch_small_msm(ctx.h, None, ptr(sc), 1, 2, ptr(out)) == E_ARG and b"null pointer" in lib.halo_last_error()
    assert lib.halo_dev_batch_small_msm(ctx.h, ptr(pts), ptr(sc), 1, 2, None) == E_ARG
    assert lib.halo_dev_batch_small_msm(ctx.h, ptr(pts), ptr(sc), 65536, 2, ptr(out)) == E_ARG and b"65535" in lib.halo_last_error()
    assert lib.halo_dev_batch_small_msm(ctx.h, None, None, 0, 0, None) == 0
    assert lib.halo_dev_batch_to_affine(ctx.h, None, 1, ptr(out)) == E_ARG and b"null pointer" in lib.halo_last_error()
    assert lib.halo_dev_batch_to_affine(ctx.h, ptr(pts), 1, None) == E_ARG
    assert lib.halo_dev_batch_to_affine(ctx.h, ptr(pts), (1 << 22) + 1, ptr(out)) == E_ARG and b"2^22" in lib.halo_last_error()
    assert lib.halo_dev_batch_to_affine(ctx.h, None, 0, None) == 0


@pytest.mark.parametrize("li", range(3))
def test_small_msm_seg_every_case(ctx, li):
    cases = pc.seg_lists()[li]
    lens = [c.K for c in cases]
    compared = 0
    for rep in range(2):
        got = ctx.small_msm_seg(np.concatenate([c.points() for c in cases]), np.concatenate([c.scalars() for c in cases]), lens)
        bad = pc.check_sums(got, cases)
        assert not bad, "list %d, run %d: %s" % (li, rep, pc.describe(bad))
        compared += len(cases)
    print("list %d: %d sums of %d terms, widths %s, %d idle lanes" % (li, len(cases), sum(lens), sorted({pc.seg_width(k) for k in lens}),
                                                                    -sum(pc.seg_width(k) for k in lens) % 64))
    assert compared == 2 * len(cases) and len(cases) >= 50


def test_small_msm_seg_ran_every_case():
    placed = {id(c) for l in pc.seg_lists() for c in l}
    assert all(id(c) in placed for c in pc.msm_cases()) and len(placed) >= 150


# ---------------------------------------------------------------------------------------------------- the derivation of the key
@pytest.mark.parametrize("stride", pc.URS_STRIDE)
@pytest.mark.parametrize("first", pc.URS_FIRST)
def test_urs_runs(hal, first, stride):
    triples = [t for t in pc.urs_triples() if t[0] == first and t[1] == stride]
    assert [n for _, _, n in triples] == pc.URS_N
    compared = 0
    for _, _, n in triples:
        made = [hal._lib.Context(urs_n=n, first_index=first, stride=stride)]  # (stride 1: halo_ctx_create_urs)
        if stride == 1:
            h = C.c_void_p()
            hal._lib.check(made[0].lib.halo_ctx_create_urs_strided(0, first, 1, n, C.byref(h)))
            other = hal._lib.Context.__new__(hal._lib.Context)
            other.h, other.lib, other.device, other._children = h, made[0].lib, 0, []
            made.append(other)
        try:
            for c in made:
                bad = pc.check_urs(c.read_bases(), first, stride, n)
                assert not bad, "first %d, stride %d, n = %d: %d wrong; first (position, index): %s" % (first, stride, n, len(bad), bad[:6])
                compared += n
        finally:
            for c in made:
                c.close()
    assert compared == sum(pc.URS_N) * (2 if stride == 1 else 1)


# ---------------------------------------------------------------------------------------------------- verdicts at the ABI
LG = 10
D = (1 << LG) - 1
L_AT = lambda j: 23 + 12 * j
R_AT = lambda j: 23 + 12 * LG + 12 * j


def _negated_jac(p):
    o = p.copy()
    o[4:8] = tc._words((pc.P - tc._int(p[4:8])) % pc.P)
    return o


def _tamper(q, what):
    q = q.copy()
    j = 3
    if what == "one L_j infinite":
        q[L_AT(j) + 8: L_AT(j) + 12] = 0
    elif what == "every L_j and R_j infinite":
        for i in range(LG):
            q[L_AT(i) + 8: L_AT(i) + 12] = 0
            q[R_AT(i) + 8: R_AT(i) + 12] = 0
    elif what == "R_j = L_j":
        q[R_AT(j): R_AT(j) + 12] = q[L_AT(j): L_AT(j) + 12]
    elif what == "R_j = -L_j":
        q[R_AT(j): R_AT(j) + 12] = _negated_jac(q[L_AT(j): L_AT(j) + 12])
    elif what == "L_0 = H":
        H = np.zeros(12, dtype=np.uint64)
        orc.lib().orc_urs_point(C.c_uint64(1), orc.ptr(H))
        q[L_AT(0): L_AT(0) + 12] = H
    elif what == "C infinite, Z = 0 over non-zero X, Y":
        assert q[:8].any()
        q[8:12] = 0
    else:
        raise ValueError(what)
    return q


TAMPERS = ["one L_j infinite", "every L_j and R_j infinite", "R_j = L_j", "R_j = -L_j", "L_0 = H", "C infinite, Z = 0 over non-zero X, Y"]
TAMPERED_AT = [5, 12, 23, 34, 47, 63]


@pytest.fixture(scope="module")
def small(hal):
    c = hal._lib.Context(urs_n=1 << LG)
    yield c
    c.close()


@pytest.fixture(scope="module")
def instances(small):
    from halo_accumulation_amd import acc as A
    rng = [0x706F696E7473]
    honest = A.random_instance_batch(small, rng, D, 64)
    qs = [q.copy() for q in honest]
    for at, what in zip(TAMPERED_AT, TAMPERS):
        assert qs[at][L_AT(3) + 8: L_AT(3) + 12].any(), "an honest proof's L_j is finite"
        qs[at] = _tamper(qs[at], what)
    return honest, qs


def _succinct_batch(c, qs):
    blob = np.ascontiguousarray(np.concatenate(qs))
    st = (C.c_int * len(qs))(*([77] * len(qs)))
    xis, Us = np.zeros((len(qs), LG + 1, 4), dtype=np.uint64), np.zeros((len(qs), 12), dtype=np.uint64)
    rc = c.lib.halo_pcdl_succinct_check_batch(c.h, D, ptr(blob), len(qs), ptr(xis), ptr(Us), st)
    return rc, list(st), c.lib.halo_last_error().decode() if rc else ""


def _succinct_single(c, q):
    xis, U = np.zeros((LG + 1, 4), dtype=np.uint64), np.zeros(12, dtype=np.uint64)
    q = np.ascontiguousarray(q)
    rc = c.lib.halo_pcdl_succinct_check(c.h, ptr(q[:12].copy()), D, ptr(q[13:17].copy()), ptr(q[17:21].copy()), ptr(q[21:].copy()), ptr(xis), ptr(U))
    return rc, c.lib.halo_last_error().decode() if rc else ""


def test_succinct_verdicts_over_exceptional_proof_points(hal, small, instances):
    honest, qs = instances
    dev = _succinct_batch(small, qs)
    small.set_batch_verify(False)
    try:
        host = _succinct_batch(small, qs)
    finally:
        small.set_batch_verify(True)
    assert dev == host, "device path and host path: every status and the first message"
    singles = [_succinct_single(small, q) for q in qs]
    assert dev[1] == [s[0] for s in singles]
    bad = [i for i, s in enumerate(singles) if s[0]]
    assert bad and set(bad) <= set(TAMPERED_AT) and all(singles[i][0] == 0 for i in range(64) if i not in TAMPERED_AT)
    assert dev[0] == singles[bad[0]][0] and dev[2] == "instance %d: %s" % (bad[0], singles[bad[0]][1])
    pp = orc.make_pp(small.read_bases())
    for i in range(64):
        q = qs[i]
        try:
            orc.pcdl_succinct_check(pp, q[:12].copy(), D, q[13:17].copy(), q[17:21].copy(), q[21:].copy())
            accepted = True
        except ValueError:
            accepted = False
        assert accepted == (singles[i][0] == 0), "instance %d (%s)" % (i, dict(zip(TAMPERED_AT, TAMPERS)).get(i, "honest"))
    print("statuses of the tampered instances:", {w: dev[1][i] for i, w in zip(TAMPERED_AT, TAMPERS)})
    assert _succinct_batch(small, honest)[:2] == (0, [0] * 64)


def _vbatch(c, members):
    k = len(members)
    blob = np.ascontiguousarray(np.concatenate([q for m in members for q in m[0]]))
    accs = np.ascontiguousarray(np.concatenate([m[1] for m in members]))
    counts = (C.c_size_t * k)(*[len(m[0]) for m in members])
    st = (C.c_int * k)(*([77] * k))
    rc = c.lib.halo_acc_verifier_batch(c.h, D, ptr(blob), counts, k, ptr(accs), st)
    return rc, list(st)


def _vsingle(c, member):
    qs, acc = member
    return c.lib.halo_acc_verifier(c.h, D, ptr(np.ascontiguousarray(np.concatenate(qs))), len(qs), ptr(np.ascontiguousarray(acc)))


def test_verifier_batch_over_repeated_instances_and_members(hal, small, instances):
    """the device form of halo_acc_verifier_batch: a member that verifies one instance twice (its sum adds equal points), two
    identical members (equal sums in neighbouring segments), one member with an exceptional proof point"""
    from halo_accumulation_amd import acc as A
    honest, qs = instances
    rng = [0x7477696365]
    twice = ([honest[0], honest[0]], A.prover(small, rng, D, [honest[0], honest[0]]))
    plain = ([honest[1], honest[2]], A.prover(small, rng, D, [honest[1], honest[2]]))
    broken = ([honest[1], qs[TAMPERED_AT[2]]], plain[1])
    members = [twice, plain, plain, broken, twice]
    hal._lib.dev_hook("verifier_batch_min", 1)  # (tests/conftest.py resets the hooks after the test)
    dev = _vbatch(small, members)
    singles = [_vsingle(small, m) for m in members]
    assert dev[1] == singles and singles[:3] == [0, 0, 0] and singles[4] == 0 and singles[3] != 0
    assert dev[0] == singles[3]
    small.set_batch_verify(False)
    try:
        assert _vbatch(small, members) == dev
    finally:
        small.set_batch_verify(True)
    pp = orc.make_pp(small.read_bases())
    orc.acc_verifier(pp, D, twice[0], twice[1])
    with pytest.raises(ValueError):
        orc.acc_verifier(pp, D, broken[0], broken[1])
