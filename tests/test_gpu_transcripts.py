"""The batched checks' Fiat-Shamir transcripts on the device (csrc/transcript.hip: k_transcript_points, k_transcript_head,
k_batch_small_msm with K = 3, k_transcript_chain) against the host's own (succinct_challenges on the pool), word for word through
halo_dev_transcripts: honest batches that mix hiding and plain members at the member counts around the per-member kernels' wave
boundaries; planted members (points at infinity in every position, edge scalars, invalid points and scalars, header defects, a
point that is not normalised) against the host twin, and the valid ones against the integer model (oracle/pallas_model.py) and
the oracle's pcdl_succinct_check; then every public batched call under both routes ("transcript_min" 1 and above m): code,
statuses, message and outputs identical, and the profiler showing which route ran.

A zero challenge cannot be constructed (a SHA3-256 preimage of a multiple of r).  That branch -- k_transcript_chain's
`zero = zero || fe_is_zero(xi)` after each round's challenge and never after xi_0, as succinct_challenges tests xis[i + 1] only;
status 3, the message "challenge is zero", zeroed rows in halo_dev_transcripts -- is covered by reading the code, not by a test."""
import ctypes as C

import numpy as np
import pytest

import orc
import pallas_model as pm
import transcript_cases as tc

pytestmark = pytest.mark.gpu

P, R = pm.P, pm.R_ORDER
OK, BAD_INSTANCE, BAD_PROOF, HEADER = 0, 1, 2, 4


@pytest.fixture(scope="module")
def hal():
    import halo_accumulation_amd as h
    return h


@pytest.fixture(scope="module")
def ctx(hal):
    c = hal._lib.Context(urs_n=1 << 10)
    yield c
    c.close()


def ptr(a):
    from halo_accumulation_amd._lib import ptr as p
    return p(a)


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


# ------------------------------------------------------------------ members
def plain_instance(c, seed, d, hiding=False):
    """a non-hiding Instance: halo_pcdl_open without omega over a committed polynomial of full length (hiding: with omega -- the
    hiding members at d = 1, below halo_random_instance_batch's smallest degree bound)"""
    from halo_accumulation_amd import pcdl
    coeffs, s = orc.rng_scalars(seed, d + 1)
    z, _ = orc.rng_scalars(s, 2)
    w = z[1] if hiding else None
    Cm = pcdl.commit(c, coeffs, d, w)
    pi = pcdl.open(c, [seed], coeffs, Cm, d, z[0], w)
    v = c.poly_eval(coeffs, z[0])
    return np.concatenate([Cm, np.array([d], dtype=np.uint64), z[0], v, pi])


def constant_instance(i, hiding):
    """d = 0: the layout of an Instance with well-formed fields (no open is behind it: a hiding open needs degree 1, and only the
    transcript is asked for -- the twins must agree whatever the relation would say)"""
    g = lambda k: tc.jac_words(pm.mul(pm.GENERATOR, k))
    q = g(1000 + i) + [0] + tc.fr_mont(77 + i) + tc.fr_mont(99 + i) + [1 if hiding else 0, 0] + g(2000 + i) + tc.fr_mont(5 + i)
    q += (g(3000 + i) + tc.fr_mont(7 + i)) if hiding else (tc.jac_words(None) + [0] * 4)
    return np.array(q, dtype=np.uint64)


_POOLS = {}
PLAIN_EVERY = 5  # members 1, 6, 11, .. are plain, the others hiding


def pool(c, lg, m):
    """m honest Instances of degree bound 2^lg - 1, built once per size: hiding ones from halo_random_instance_batch, every fifth
    from index 1 plain (lg = 0: all plain -- a hiding open needs degree 1)"""
    if (lg, m) not in _POOLS:
        from halo_accumulation_amd import acc as A
        d = (1 << lg) - 1
        if lg == 0:
            qs = [constant_instance(i, hiding=i % PLAIN_EVERY != 1) for i in range(m)]
        elif lg == 1:
            qs = [plain_instance(c, 700 + i, d, hiding=i % PLAIN_EVERY != 1) for i in range(m)]
        else:
            qs = A.random_instance_batch(c, [0x7A5C + lg], d, m)
            for i in range(1, m, PLAIN_EVERY):
                qs[i] = plain_instance(c, 900 + i, d)
        _POOLS[(lg, m)] = qs
    return [q.copy() for q in _POOLS[(lg, m)]]


def is_hiding(q):
    return int(q[21]) == 1


def off(lg, what, j=0):
    base = 21 + 2
    return {"C": 0, "z": 13, "v": 17, "L": base + 12 * j, "R": base + 12 * lg + 12 * j, "U": base + 24 * lg, "c": base + 24 * lg + 12,
            "Cbar": base + 24 * lg + 16, "wp": base + 24 * lg + 28}[what]


def fq_int(w):
    return pm.from_mont_limbs([int(x) for x in w], P)


def point_of(q, at):
    """the affine point (None: infinity) of 12 Jacobian words"""
    return pm.jacobian_to_affine(fq_int(q[at:at + 4]), fq_int(q[at + 4:at + 8]), fq_int(q[at + 8:at + 12]))


def put(q, at, ws):
    q[at:at + len(ws)] = np.array(ws, dtype=np.uint64)


def model_transcript(q, lg):
    """(xis as Montgomery words, C' as normalised Jacobian words) of an Instance with a valid transcript, from Python integers"""
    fr = lambda at: pm.from_mont_limbs([int(x) for x in q[at:at + 4]], R)
    Cp, z, v = point_of(q, 0), fr(off(lg, "z")), fr(off(lg, "v"))
    if is_hiding(q):
        Cbar, wp = point_of(q, off(lg, "Cbar")), fr(off(lg, "wp"))
        a = pm.rho_0(("p", Cp), ("s", z), ("s", v), ("p", Cbar))
        S = pm.mul(pm.GENERATOR, pm.generator_hash_scalar(0))
        Cp = pm.add(pm.add(Cp, pm.mul(Cbar, a)), pm.neg(pm.mul(S, wp)))
    xis = [pm.rho_0(("p", Cp), ("s", z), ("s", v))]
    for j in range(lg):
        xis.append(pm.rho_0(("s", xis[-1]), ("p", point_of(q, off(lg, "L", j))), ("p", point_of(q, off(lg, "R", j)))))
    return [tc.fr_mont(x) for x in xis], tc.jac_words(Cp)


def twins(c, d, blobs):
    qs = np.ascontiguousarray(np.concatenate(blobs))
    host = c.transcripts(d, qs, 0)
    (dev, counts) = profiled(c, lambda: c.transcripts(d, qs, 1))
    return host, dev, counts


def assert_same(host, dev, what=""):
    assert host[2].tolist() == dev[2].tolist(), "status %s" % what
    bad = [i for i in range(len(host[2])) if host[0][i].tolist() != dev[0][i].tolist() or host[1][i].tolist() != dev[1][i].tolist()]
    assert not bad, "members whose challenges or C' differ %s: %s" % (what, bad[:8])


# ------------------------------------------------------------------ 1. device against host twin
SHAPES = [(lg, m) for lg in (1, 2, 3) for m in (1, 2, 63, 64, 65, 130)] + [(10, 65), (0, 3)]


@pytest.mark.parametrize("lg,m", SHAPES)
def test_device_transcripts_equal_the_host_twin(hal, ctx, lg, m):
    """m around the wave of the per-member kernels; m (2 lg + 3) is no multiple of the point kernel's 256 lanes at any of them"""
    d = (1 << lg) - 1
    blobs = pool(ctx, lg, 130 if lg in (1, 2, 3) else m)[:m]
    if lg and m >= 2:
        assert {is_hiding(q) for q in blobs} == {True, False}
    assert (m * (2 * lg + 3)) % 256 != 0
    host, dev, counts = twins(ctx, d, blobs)
    assert_same(host, dev)
    assert dev[2].tolist() == [OK] * m and np.any(dev[0][:, 0] != 0)
    assert counts.get("k_transcript_points") == 1 and counts.get("k_transcript_head") == 1 and counts.get("k_transcript_chain") == 1, counts
    assert counts.get("k_batch_small_msm") == 1, counts
    # the first hiding and the first plain member against the integer model, and against the oracle's succinct check
    for i in sorted({0, min(1, m - 1)}):
        xis, cp = model_transcript(blobs[i], lg)
        assert dev[0][i].tolist() == xis and dev[1][i].tolist() == cp, i
    if lg:
        pp = orc.make_pp(ctx.read_bases())
        q = blobs[0]
        want, _ = orc.pcdl_succinct_check(pp, q[:12], d, q[13:17], q[17:21], q[21:])
        assert dev[0][0].tolist() == want.tolist()


# ------------------------------------------------------------------ 2. planted members
LG = 3


def planted(ctx):
    """65 members at lg = 3 -> (blobs, {index: (what, expected status, transcript valid)}, the honest batch)"""
    lg = LG
    base = pool(ctx, lg, 130)[:65]
    blobs = [q.copy() for q in base]
    inf = tc.jac_words(None)
    one = tc.fq_mont(1)
    plan = {}

    def y_plus_one(q, at):
        y = (fq_int(q[at + 4:at + 8]) + 1) % P
        put(q, at + 4, tc.fq_mont(y))

    def hiding(i):
        assert is_hiding(blobs[i]), i
        return blobs[i]

    def plain(i):
        assert not is_hiding(blobs[i]), i
        return blobs[i]

    put(hiding(0), off(lg, "L", 0), inf); plan[0] = ("L_0 = infinity", OK, True)
    put(hiding(2), off(lg, "R", lg - 1), inf); plan[2] = ("R_(lg-1) = infinity", OK, True)
    put(hiding(3), off(lg, "Cbar"), inf); plan[3] = ("C_bar = infinity", OK, True)
    put(plain(1), 0, inf); plan[1] = ("C = infinity, plain: C' is infinity", OK, True)
    put(hiding(4), off(lg, "wp"), tc.fr_mont(0)); plan[4] = ("omega' = 0", OK, True)
    put(hiding(5), off(lg, "wp"), tc.fr_mont(R - 1)); plan[5] = ("omega' = r - 1", OK, True)
    def finite(q):
        """L_1, or R_1 where L_1 is the point at infinity (random_instance draws the degree: a short polynomial's left halves vanish)"""
        for what in ("L", "R"):
            if point_of(q, off(lg, what, 1)) is not None:
                return off(lg, what, 1)
        raise AssertionError("no finite point in round 1")

    q = hiding(7)
    at = finite(q)
    x, y = point_of(q, at)
    put(q, at, tc.jac_words((x, P - y))); plan[7] = ("L_1 negated", OK, True)
    y_plus_one(hiding(8), off(lg, "U")); plan[8] = ("U off the curve", BAD_PROOF, False)
    y_plus_one(hiding(9), 0); plan[9] = ("C off the curve", BAD_INSTANCE, False)
    y_plus_one(hiding(10), 0); y_plus_one(blobs[10], off(lg, "U")); plan[10] = ("C and U off the curve: the instance first", BAD_INSTANCE, False)
    put(hiding(12), off(lg, "z"), tc.words(R)); plan[12] = ("z = r", BAD_INSTANCE, False)
    put(hiding(13), off(lg, "c"), tc.words(R)); plan[13] = ("c = r", BAD_PROOF, False)
    put(hiding(14), off(lg, "wp"), tc.words(R)); plan[14] = ("omega' = r", BAD_PROOF, False)
    blobs[15][21] = 2; plan[15] = ("flag word 2", BAD_PROOF, False)
    blobs[17][22] = lg + 1; plan[17] = ("proof length", HEADER, False)
    q = hiding(18)
    at = finite(q)
    put(q, at, tc.jac_words(point_of(q, at), z=0xABCDEF12345)); plan[18] = ("L_1 at Z = lambda", OK, None)
    q = plain(6)
    put(q, off(lg, "Cbar"), one + one + tc.fq_mont(7)); plan[6] = ("a plain member's dead C_bar slot holds anything", OK, None)
    return blobs, plan, base


def test_planted_members_agree_with_the_host_and_the_model(hal, ctx):
    lg, d = LG, (1 << LG) - 1
    blobs, plan, base = planted(ctx)
    host, dev, _ = twins(ctx, d, blobs)
    assert_same(host, dev, "(planted)")
    want = [plan[i][1] if i in plan else OK for i in range(65)]
    assert dev[2].tolist() == want, [(i, plan[i][0]) for i in plan if dev[2][i] != plan[i][1]]
    for i, (what, status, valid) in plan.items():
        if status != OK:
            assert not dev[0][i].any() and not dev[1][i].any(), what
        if valid:
            xis, cp = model_transcript(blobs[i], lg)
            assert dev[0][i].tolist() == xis and dev[1][i].tolist() == cp, what
    assert dev[1][1].tolist() == tc.jac_words(None), "C' of the plain member with C at infinity"
    # the rescaled and the dead-slot member: every output equals the honest member's
    honest = ctx.transcripts(d, np.ascontiguousarray(np.concatenate(base)), 0)
    for i in (18, 6):
        assert dev[0][i].tolist() == honest[0][i].tolist() and dev[1][i].tolist() == honest[1][i].tolist(), plan[i][0]
    # the honest members of the planted batch still match the oracle
    pp = orc.make_pp(ctx.read_bases())
    for i in (11, 20, 64):
        q = blobs[i]
        xs, _ = orc.pcdl_succinct_check(pp, q[:12], d, q[13:17], q[17:21], q[21:])
        assert dev[0][i].tolist() == xs.tolist(), i


def test_dev_transcripts_argument_errors(hal, ctx):
    E_ARG = hal._lib.HALO_E_ARG
    q = np.ascontiguousarray(np.concatenate(pool(ctx, 1, 130)[:2]))
    xis, cp, st = np.zeros((2, 2, 4), dtype=np.uint64), np.zeros((2, 12), dtype=np.uint64), (C.c_int * 2)()
    f = ctx.lib.halo_dev_transcripts
    assert f(ctx.h, 1, ptr(q), 0, 1, None, None, None) == 0
    assert f(ctx.h, 1, None, 2, 1, ptr(xis), ptr(cp), st) == E_ARG and b"null pointer" in ctx.lib.halo_last_error()
    assert f(ctx.h, 2, ptr(q), 2, 1, ptr(xis), ptr(cp), st) == E_ARG
    assert f(None, 1, ptr(q), 2, 1, ptr(xis), ptr(cp), st) == E_ARG
    hal._lib.dev_hook("batch_stage_fail", 1)  # (tests/conftest.py resets the hooks after the test)
    assert f(ctx.h, 1, ptr(q), 2, 1, ptr(xis), ptr(cp), st) == hal._lib.HALO_E_DEVICE and b"staging" in ctx.lib.halo_last_error()
    assert f(ctx.h, 1, ptr(q), 2, 0, ptr(xis), ptr(cp), st) == 0 and list(st) == [0, 0]


# ------------------------------------------------------------------ 3. the public calls under both routes
def run_succinct(c, d, blobs):
    m, lg = len(blobs), (d + 1).bit_length() - 1
    qs = np.ascontiguousarray(np.concatenate(blobs))
    xis, Us, st = np.zeros((m, lg + 1, 4), dtype=np.uint64), np.zeros((m, 12), dtype=np.uint64), (C.c_int * m)(*([77] * m))
    rc = c.lib.halo_pcdl_succinct_check_batch(c.h, d, ptr(qs), m, ptr(xis), ptr(Us), st)
    return rc, list(st), c.lib.halo_last_error().decode() if rc else "", xis.tolist(), Us.tolist()


def run_check(c, d, blobs, which):
    m = len(blobs)
    qs = np.ascontiguousarray(np.concatenate(blobs))
    st = (C.c_int * m)(*([77] * m))
    if which == "exact":
        rc = c.lib.halo_pcdl_check_batch(c.h, d, ptr(qs), m, st)
    elif which == "combined":
        rc = c.lib.halo_pcdl_check_batch_combined(c.h, d, ptr(qs), m, None, st)
    elif which == "fused":
        rc = c.lib.halo_pcdl_check_batch_fused(c.h, d, ptr(qs), m, None, st)
    else:
        rc = c.lib.halo_acc_decider_batch_fused(c.h, d, ptr(qs), m, None, st)
    return rc, list(st), c.lib.halo_last_error().decode() if rc else ""


def run_prover(c, d, members):
    k, lg = len(members), (d + 1).bit_length() - 1
    counts = (C.c_size_t * k)(*[len(qs) for qs in members])
    qs = np.ascontiguousarray(np.concatenate([q for qs in members for q in qs]))
    rng = C.c_uint64(0xBEE5)
    out = np.zeros((k, c.lib.halo_accumulator_words(lg)), dtype=np.uint64)
    st = (C.c_int * k)(*([77] * k))
    rc = c.lib.halo_acc_prover_batch(c.h, C.byref(rng), d, ptr(qs), counts, k, ptr(out), st)
    return rc, list(st), c.lib.halo_last_error().decode() if rc else "", out.tolist(), rng.value


def both_routes(hal, c, fn, m, stage_fail=False):
    """fn() with the transcripts forced onto the device, then onto the host -> the two results and launch counts"""
    out = []
    for min_members in (1, m + 1000):
        try:
            hal._lib.dev_hook("transcript_min", min_members)
            if stage_fail:
                hal._lib.dev_hook("batch_stage_fail", 1)
            out.append(profiled(c, fn))
        finally:
            hal._lib.dev_hook("reset", 0)
    return out


def accumulators(c, d, qs):
    from halo_accumulation_amd import acc as A
    accs, codes = A.prover_batch(c, [0xACC], d, [[q] for q in qs])
    assert codes == [0] * len(qs)
    return accs


def with_rejects(blobs, lg):
    """two planted rejects: a proof point and an instance point off the curve"""
    bad = [q.copy() for q in blobs]
    bad[8][off(lg, "U")] ^= 1
    bad[40][0] ^= 1
    return bad


CALLS = ["succinct", "exact", "combined", "fused", "decider_fused", "prover"]


@pytest.mark.parametrize("rejects", [False, True], ids=["valid", "rejects"])
@pytest.mark.parametrize("which", CALLS)
def test_public_calls_are_identical_under_both_routes(hal, ctx, which, rejects):
    lg, d, m = LG, (1 << LG) - 1, 65
    blobs = pool(ctx, lg, 130)[:m]
    if which == "decider_fused":
        blobs = accumulators(ctx, d, blobs)
    if rejects:
        blobs = with_rejects(blobs, lg)
    if which == "succinct":
        fn = lambda: run_succinct(ctx, d, blobs)
    elif which == "prover":
        two = pool(ctx, lg, 130)[:66]
        if rejects:
            two[40][0] ^= 1
        fn = lambda: run_prover(ctx, d, [two[:33], two[33:]])
    else:
        fn = lambda: run_check(ctx, d, blobs, which)
    (dev, dev_counts), (host, host_counts) = both_routes(hal, ctx, fn, m)
    assert dev == host
    assert dev_counts.get("k_transcript_chain", 0) >= 1 and dev_counts.get("k_transcript_points", 0) >= 1, dev_counts
    assert not [k for k in host_counts if k.startswith("k_transcript")], host_counts
    if rejects:
        assert dev[0] == hal._lib.HALO_E_REJECT
        if which == "prover":
            assert [j for j, s in enumerate(dev[1]) if s] == [1], "instance 40 is the second member's"
        else:
            assert [i for i, s in enumerate(dev[1]) if s] == [8, 40]
            assert dev[2] == "instance 8: proof holds an invalid point or scalar"
    else:
        assert dev[0] == 0 and set(dev[1]) == {0}


@pytest.mark.parametrize("which", ["succinct", "fused"])
def test_refused_staging_gives_the_host_route(hal, ctx, which):
    lg, d, m = LG, (1 << LG) - 1, 65
    blobs = with_rejects(pool(ctx, lg, 130)[:m], lg)
    fn = (lambda: run_succinct(ctx, d, blobs)) if which == "succinct" else (lambda: run_check(ctx, d, blobs, "fused"))
    (refused, refused_counts), (host, _) = both_routes(hal, ctx, fn, m, stage_fail=True)
    assert not [k for k in refused_counts if k.startswith("k_transcript")], refused_counts
    (dev, dev_counts), _ = both_routes(hal, ctx, fn, m)
    assert dev_counts.get("k_transcript_chain", 0) >= 1
    assert refused == host == dev


def test_hook_argument_errors(hal, ctx):
    lib = hal.load()
    try:
        assert lib.halo_dev_hook(b"transcript_min", 7) == 0 and lib.halo_dev_tuning(b"transcript_min") == 7
        assert lib.halo_dev_hook(b"transcript_min", -1) == hal._lib.HALO_E_ARG and b"transcript_min is 0" in lib.halo_last_error()
        assert lib.halo_dev_tuning(b"transcript_min") == 7, "a refused value leaves the hook as it was"
        assert lib.halo_dev_hook(b"reset", 0) == 0 and lib.halo_dev_tuning(b"transcript_min") == 0
    finally:
        lib.halo_dev_hook(b"reset", 0)
