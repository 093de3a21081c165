"""The scalar-side kernels of csrc/fr_vec.hip and csrc/hpoly.hip (K4 - K9) at every size where their launch plan changes (csrc/fr_plan.hpp): chain
lengths 4 .. 64 with short chains and idle lanes in the last wave, 1 .. 5 windows of the exponent, several trips through the
capped grids of k_poly_eval_partial and k_dot2_partial with full, ragged and idle last trips, and the third table of h(X).  The
cases are tests/fr_plan_cases.py's (tests/test_fr_plan_cases_cpu.py prints their coverage table); the development hooks "pow_e",
"dot_blocks" and "poly_blocks" bring every plan down to a 2^17-point context.

Every comparison is exact, against the C oracle (`orc`) -- which the CPU test holds against Python integers at these sizes -- and,
for one-hot vectors, against the identities p(z) = c z^p and <x, y> = x_p y_p, which pin one lane, one table entry per window
and one z^(64 k) entry per case where a dense sum does not.  Each test first asserts through halo_dev_fr_plan that the plan it
names is the one in force.  Whole arrays are compared byte for byte (`same`: as exact as .tolist() equality at a fraction of
its time over 2^17 elements), single elements as lists."""
import ctypes as C
import functools

import numpy as np
import pytest

import fr_plan_cases as fp
import lazy_cases as lz
import orc

pytestmark = pytest.mark.gpu
R = fp.R


@pytest.fixture(scope="module")
def hal():
    import halo_accumulation_amd as h
    return h


@pytest.fixture(scope="module")
def ctx(hal):
    c = hal._lib.Context(urs_n=fp.CTX_N)
    yield c
    c.close()


@pytest.fixture(scope="module")
def zs():
    return {k: (z, lz.fr_mont([z])[0]) for k, z in fp.Z_SCALARS.items()}


@pytest.fixture(scope="module")
def all_powers(zs):
    """z -> orc.powers(z, 2^17): every shorter run is its prefix (the oracle's loop is one product per element)"""
    return {k: orc.powers(zw, fp.CTX_N) for k, (_z, zw) in zs.items()}


def force(hal, case):
    """the hooks of a case, then: is the plan the case claims the one the launcher would run?"""
    hal._lib.dev_hook("reset", 0)
    if case.pow_e:
        hal._lib.dev_hook("pow_e", case.pow_e)
    if case.blocks_hook:
        hal._lib.dev_hook("dot_blocks" if fp.PLAN_OF[case.kernel] == "dot" else "poly_blocks", case.blocks_hook)
    got = hal._lib.fr_plan(fp.PLAN_OF[case.kernel], case.n)
    assert fp.Plan(got["E"], got["nwin"], got["blocks"], got["trips"]) == case.plan, "nothing here would test %r: the plan in force is %r" % (case, got)


def same(got, want):
    """exact equality of two uint64 arrays; a mismatch names its first element"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype == np.uint64 and got.shape == want.shape, (got.dtype, got.shape, want.dtype, want.shape)
    if got.tobytes() == want.tobytes():
        return True
    k = int(np.nonzero((got != want).reshape(len(got), -1).any(axis=1))[0][0])
    raise AssertionError("element %d: got %s, want %s" % (k, got[k].tolist(), want[k].tolist()))


@functools.lru_cache(maxsize=4)
def dense(n):
    return fp.dense_vectors(n)


@functools.lru_cache(maxsize=None)
def want_poly_dense(n):
    """(vector, z) -> the oracle's p(z) over the dense vectors of length n (shared by the chain lengths that meet the same n)"""
    out = {}
    for k, (_v, w) in dense(n).items():
        for kz, z in fp.Z_SCALARS.items():
            out[k, kz] = orc.poly_eval(w, lz.fr_mont([z])[0]).tolist()
    return out


def ids(es):
    return ["default" if e == 0 else "E%d" % e for e in es]


# ------------------------------------------------------------------ 1. k_powers
@pytest.mark.parametrize("pow_e", fp.POW_ES, ids=ids(fp.POW_ES))
def test_powers_every_element(hal, ctx, zs, all_powers, pow_e):
    cases = [c for c in fp.chain_cases("powers") if c.pow_e == pow_e]
    assert {c.plan.nwin for c in cases} >= {1, 2, 3, 4} and {c.tail for c in cases} == {"full", "in-wave"}
    for c in cases:
        force(hal, c)
        for kz, (_z, zw) in zs.items():
            assert same(ctx.powers(zw, c.n), all_powers[kz][: c.n]), (c, kz)


# ------------------------------------------------------------------ 2. k_poly_eval_partial
def check_poly_dense(ctx, zs, c):
    want = want_poly_dense(c.n)
    for k, (_v, w) in dense(c.n).items():
        for kz, (_z, zw) in zs.items():
            assert ctx.poly_eval(w, zw).tolist() == want[k, kz], (c, k, kz)


def check_poly_one_hot(ctx, zs, c, extra=()):
    for p in sorted(set(fp.one_hot_positions(c.n, 64 * c.plan.E)) | {q for q in extra if 0 <= q < c.n}):
        coeff, w = fp.one_hot(c.n, p, 2)
        for kz, (z, zw) in zs.items():
            got = ctx.poly_eval(w, zw)
            assert lz.fr_ints(got) == [coeff * pow(z, p, R) % R], (c, p, kz)
            assert got.tolist() == orc.poly_eval(w, zw).tolist(), (c, p, kz)


@pytest.mark.parametrize("pow_e", fp.POW_ES, ids=ids(fp.POW_ES))
def test_poly_eval_dense_vectors(hal, ctx, zs, pow_e):
    cases = [c for c in fp.chain_cases("poly_eval") if c.pow_e == pow_e]
    assert {c.plan.nwin for c in cases} >= {1, 2, 3, 4} and all(c.plan.trips == 1 for c in cases)
    for c in cases:
        force(hal, c)
        check_poly_dense(ctx, zs, c)


@pytest.mark.parametrize("pow_e", fp.POW_ES, ids=ids(fp.POW_ES))
def test_poly_eval_one_hot_vectors(hal, ctx, zs, pow_e):
    for c in [c for c in fp.chain_cases("poly_eval") if c.pow_e == pow_e]:
        force(hal, c)
        check_poly_one_hot(ctx, zs, c)


TRIP_PARAMS = sorted({(c.pow_e, c.blocks_hook, c.plan.trips) for c in fp.poly_trip_cases()})  # (no fourth trip at E = 64 under poly_blocks = 3)


@pytest.mark.parametrize("pow_e,poly_blocks,trips", TRIP_PARAMS, ids=["%s-blocks%d-trips%d" % (ids([e])[0], b, t) for e, b, t in TRIP_PARAMS])
def test_poly_eval_trips_through_a_capped_grid(hal, ctx, zs, pow_e, poly_blocks, trips):
    """one test per chain length, grid and trip count (a case at E = 64 has up to 2^17 coefficients): the last trip full, ending
    inside a wave, with idle waves -- all three wherever the context holds them (fr_plan_cases.TRIPS_PAST_THE_CONTEXT)"""
    cases = [c for c in fp.poly_trip_cases() if (c.pow_e, c.blocks_hook, c.plan.trips) == (pow_e, poly_blocks, trips)]
    E = cases[0].plan.E
    assert [c.tail for c in cases] == [k for k in fp.TRIP_TAILS if (E, poly_blocks, trips, k) not in fp.TRIPS_PAST_THE_CONTEXT]
    for c in cases:
        force(hal, c)
        assert (c.plan.E, c.plan.blocks, c.plan.trips) == (E, poly_blocks, trips)
        check_poly_dense(ctx, zs, c)
        T = 4 * c.plan.blocks * 64 * c.plan.E  # one-hot: also the last element of the first trip and the first of each later one
        check_poly_one_hot(ctx, zs, c, extra=[T - 1] + [t * T for t in range(1, c.plan.trips)] + [(c.plan.trips - 1) * T + 64 * c.plan.E])


# ------------------------------------------------------------------ 3. k_dot2_partial, one pair of vectors
def dot_positions(c):
    half = 256 * c.plan.blocks  # a lane takes i and i + half of every trip
    return sorted({p for p in fp.one_hot_positions(c.n, half) + [half + 32, half + 33, 2 * half - 1, 2 * half, c.n - 34, c.n - 33, c.n - 2] if 0 <= p < c.n})


def check_dot(ctx, c):
    other = fp.fr_words(fp.random_ints(c.n, 11))
    for k, (_v, w) in dense(c.n).items():
        want = orc.scalar_dot(w, other).tolist()
        assert ctx.scalar_dot(w, other).tolist() == want, (c, k, "x")
        assert ctx.scalar_dot(other, w).tolist() == want, (c, k, "y")
    assert ctx.scalar_dot(*[dense(c.n)["all r-1"][1]] * 2).tolist() == orc.scalar_dot(*[dense(c.n)["all r-1"][1]] * 2).tolist(), c
    oi = lz.fr_ints(other)
    for p in dot_positions(c):
        coeff, w = fp.one_hot(c.n, p, 3)
        for got in (ctx.scalar_dot(w, other), ctx.scalar_dot(other, w)):
            assert lz.fr_ints(got) == [coeff * oi[p] % R], (c, p)
            assert got.tolist() == orc.scalar_dot(w, other).tolist(), (c, p)


@pytest.mark.parametrize("dot_blocks", [0] + fp.BLOCK_HOOKS)
def test_scalar_dot(hal, ctx, dot_blocks):
    cases = [c for c in fp.dot_cases() if c.blocks_hook == dot_blocks]
    assert dot_blocks == 0 or ({c.plan.trips for c in cases} == {1, 2, 3, 4} and sum(c.n % (256 * dot_blocks) == 33 for c in cases) == 4)
    for c in cases:
        force(hal, c)
        check_dot(ctx, c)


# ------------------------------------------------------------------ 4. k_dot2_partial, the two pairs of an IPA round
@pytest.mark.parametrize("dot_blocks", [1, 2])
@pytest.mark.parametrize("m", [257, 1025, 256, 1024])
def test_two_sum_form(hal, ctx, m, dot_blocks):
    """<c_hi, z_lo> and <c_lo, z_hi> in one launch.  An IPA round only ever has a power of two as m (pcdl.rs:130), so the odd
    m = 257 and 1025 run through halo_dev_dot2_cross, the powers of two also through Ipa.dot_cz and a round's cross terms."""
    (c,) = [c for c in fp.dot2_cases() if c.n == m and c.blocks_hook == dot_blocks]
    force(hal, c)
    n = 2 * m
    other = fp.fr_words(fp.random_ints(n, 12))
    for k, (_v, w) in dense(n).items():
        for cs, zv in ((w, other), (other, w)):
            want_l = orc.scalar_dot(np.ascontiguousarray(cs[m:]), np.ascontiguousarray(zv[:m])).tolist()
            want_r = orc.scalar_dot(np.ascontiguousarray(cs[:m]), np.ascontiguousarray(zv[m:])).tolist()
            dl, dr = ctx.dot2_cross(cs, zv)
            assert (dl.tolist(), dr.tolist()) == (want_l, want_r), (c, k)
            if m & (m - 1) == 0:
                ipa = hal._lib.Ipa(ctx, n, cs, None, z_vec=zv)
                assert ipa.dot_cz().tolist() == orc.scalar_dot(cs, zv).tolist(), (c, k)
                rec = ipa.round_lr_partial()
                ipa.close()
                assert (rec[24:28].tolist(), rec[28:32].tolist()) == (want_l, want_r), (c, k)
    # one-hot in either half of c: exactly one of the two sums is c_p z_q, the other zero
    oi = lz.fr_ints(other)
    for p in sorted({0, 63, 64, 255, 256, m - 1, m, m + 33, m + 255, m + 256, n - 1} & set(range(n))):
        coeff, w = fp.one_hot(n, p, 4)
        dl, dr = ctx.dot2_cross(w, other)
        hit = coeff * oi[p - m if p >= m else p + m] % R
        assert (lz.fr_ints(dl), lz.fr_ints(dr)) == (([hit], [0]) if p >= m else ([0], [hit])), (c, p)


# ------------------------------------------------------------------ 5. h(X): coefficients, accumulated sums, evaluation
@functools.lru_cache(maxsize=None)
def h_data(lg_n):
    """name -> (ints, words, the oracle's coefficients)"""
    out = {}
    for k, v in fp.h_challenges(lg_n).items():
        w = lz.fr_mont(v)
        out[k] = (v, w, orc.h_coeffs(w))
    return out


@pytest.mark.parametrize("pow_e", fp.H_ES, ids=ids(fp.H_ES))
@pytest.mark.parametrize("lg_n", fp.H_LGS)
def test_h_coeffs_single_and_batch(hal, ctx, lg_n, pow_e):
    (c,) = [c for c in fp.h_cases() if c.n == 1 << lg_n and c.pow_e == pow_e]
    assert c.plan.nwin == (lg_n + 7) // 8
    force(hal, c)
    data = h_data(lg_n)
    names = list(data)
    for k, (_v, w, want) in data.items():
        assert same(ctx.h_coeffs(w), want), (c, k)
    for i in range(0, len(names), 3):  # three members with different data per launch
        grp = names[i: i + 3]
        stack = np.ascontiguousarray(np.stack([data[k][1] for k in grp]))
        out = np.full((len(grp), 1 << lg_n, 4), 0x77, dtype=np.uint64)
        assert ctx.lib.halo_dev_h_coeffs_batch(ctx.h, hal._lib.ptr(stack), len(grp), lg_n, hal._lib.ptr(out)) == 0, ctx.lib.halo_last_error()
        for j, k in enumerate(grp):
            assert same(out[j], data[k][2]), (c, k, "member %d" % j)


H_ACC_MEMBERS = [list(range(7)), [0], [0, 4, 6]]  # (tests/test_gpu_lazy_bounds.py: 7, 1 and 3 instances, the all-(r-1) one first)
H_ACC_H0 = [(R - 1, R - 1), (1, R - 1), (0, 0)]


@functools.lru_cache(maxsize=1)
def h_acc_expected():
    """lg_n = 17 over Python integers: per member sum_i alpha_i h_i(X) (without h_0) -> (challenge words, [sums])"""
    names = list(lz.fr_extreme_vectors(18))
    data = h_data(17)
    hs = [lz.fr_ints(data[k][2]) for k in names]
    sums = []
    for mem in H_ACC_MEMBERS:
        acc = [0] * (1 << 17)
        for i in mem:
            a = fp.ALPHAS[i]
            if a:
                acc = [(s + a * h) % R for s, h in zip(acc, hs[i])]
        sums.append(acc)
    return np.ascontiguousarray(np.stack([data[k][1] for k in names])), sums


def with_h0(acc, h0):
    return fp.fr_words([(acc[0] + h0[0]) % R, (acc[1] + h0[1]) % R] + acc[2:])


@pytest.mark.parametrize("pow_e", [0, 8], ids=ids([0, 8]))
def test_h_accumulate_lg_17(hal, ctx, pow_e):
    """acc.rs:85-94 at the smallest size whose high table has two entries: every h_i and alpha at an extreme, the scale folded into
    both entries of the high table; single (k_h_coeffs accumulating) and batched (k_h_tables with scales, k_h_accumulate_batch,
    also with fewer tables per pass than a member brings)"""
    (c,) = [c for c in fp.h_cases() if c.n == 1 << 17 and c.pow_e == pow_e]
    assert c.plan.nwin == 3
    force(hal, c)
    xis, sums = h_acc_expected()
    alphas = lz.fr_mont(fp.ALPHAS)
    for h0 in ((R - 1, R - 1), (0, 0)):
        assert same(ctx.h_accumulate(lz.fr_mont(h0), xis, alphas), with_h0(sums[0], h0)), (c, h0)
    want = [with_h0(s, h0) for s, h0 in zip(sums, H_ACC_H0)]
    flat = [i for mem in H_ACC_MEMBERS for i in mem]
    bx = np.ascontiguousarray(np.concatenate([xis[i] for i in flat]))
    ba = lz.fr_mont([fp.ALPHAS[i] for i in flat])
    bh = lz.fr_mont([v for h0 in H_ACC_H0 for v in h0])
    counts = (C.c_size_t * 3)(*[len(mem) for mem in H_ACC_MEMBERS])
    for max_tables in (0, 2, 3):
        out = np.full((3, 1 << 17, 4), 0x77, dtype=np.uint64)
        rc = ctx.lib.halo_dev_h_accumulate_batch(ctx.h, hal._lib.ptr(bh), hal._lib.ptr(bx), hal._lib.ptr(ba), counts, 3, 17, max_tables, hal._lib.ptr(out))
        assert rc == 0, ctx.lib.halo_last_error()
        for j in range(3):
            assert same(out[j], want[j]), (c, "member %d, %d tables per pass" % (j, max_tables))


@pytest.mark.parametrize("lg_n", fp.H_EVAL_LGS)
def test_h_eval_batch(ctx, zs, lg_n):
    vecs = {k: lz.fr_mont(v) for k, v in fp.h_challenges(lg_n).items()}
    stack = np.ascontiguousarray(np.stack(list(vecs.values())))
    for kz, (_z, zw) in zs.items():
        got = ctx.h_eval_batch(stack, zw)
        for i, (k, x) in enumerate(vecs.items()):
            assert got[i].tolist() == orc.h_eval(x, zw).tolist(), (lg_n, k, kz)


# ------------------------------------------------------------------ 6. a batched open under a forced plan
def test_open_batch_under_a_forced_plan_equals_single_opens_and_the_oracle(hal, ctx):
    """halo_pcdl_open_batch of three members at n = 4096 under pow_e = 16, dot_blocks = 2, poly_blocks = 1 (k_powers_batch,
    k_poly_eval_partial_batch and its table, k_dot2_partial_batch): word for word the three single opens under the default plan
    and the oracle's proofs"""
    import test_gpu_open_batch as ob
    lg, m, state = 12, 3, 0x0F0B
    n, d = 1 << lg, (1 << lg) - 1
    hal._lib.dev_hook("reset", 0)
    assert [hal._lib.fr_plan(k, n)["E"] for k in ("powers", "poly_eval", "poly_eval_batch")] == [4, 4, 4], "nothing here would test the default plan"
    ps, Cs, zv, ws = ob.members(ctx, lg, m, True, 0x0F0B0001)
    want, codes, _msgs, st_want = ob.loop(ctx, state, d, ps, Cs, zv, ws)
    assert codes == [0] * m
    for name, v in (("pow_e", 16), ("dot_blocks", 2), ("poly_blocks", 1)):
        hal._lib.dev_hook(name, v)
    plans = {k: hal._lib.fr_plan(k, n) for k in ("powers", "poly_eval_batch")}  # (poly_eval_batch: open_batch_eval's own plan)
    plans["dot"] = hal._lib.fr_plan("dot", n // 2)
    assert plans == {"powers": {"E": 16, "nwin": 3, "blocks": 1, "trips": 1}, "poly_eval_batch": {"E": 16, "nwin": 3, "blocks": 1, "trips": 1},
                     "dot": {"E": 2, "nwin": 0, "blocks": 2, "trips": 2}}, "nothing here would test the forced plan: %r" % plans
    rc, got, status, st_got, msg = ob.batch(ctx, state, d, ps, Cs, zv, ws)
    assert rc == 0 and status == [0] * m and st_got == st_want, msg
    pp = orc.make_pp(ctx.read_bases(0, n))
    s = state
    for i in range(m):
        assert got[i].tolist() == want[i].tolist(), "member %d against its single open" % i
        deg = int(np.nonzero(ps[i].any(axis=1))[0][-1])
        ref, s = orc.pcdl_open(pp, s, np.ascontiguousarray(ps[i][: deg + 1]), Cs[i], d, zv[i], ws[i])
        assert got[i].tolist() == ref.tolist(), "member %d against the oracle" % i
    assert s == st_got


# ------------------------------------------------------------------ 7. misuse
def test_hook_misuse_is_refused_with_its_rule(hal, ctx):
    lib = ctx.lib
    for name, bad, rule in ((b"pow_e", (0, 2, 12, 128), b"pow_e must be a power of two in [4, 64]"),
                            (b"dot_blocks", (0, 1025), b"dot_blocks must be in [1, 1024]"), (b"poly_blocks", (0, 1025), b"poly_blocks must be in [1, 1024]")):
        for v in bad:
            assert lib.halo_dev_hook(name, v) == hal._lib.HALO_E_ARG and rule in lib.halo_last_error(), (name, v)
    assert hal._lib.fr_plan("poly_eval", 5000, ctx) == {"E": 4, "nwin": 4, "blocks": 5, "trips": 1}, "a refused value changes nothing"
    out = np.zeros(8, dtype=np.uint64)
    big = np.zeros((fp.CTX_N + 2, 4), dtype=np.uint64)
    assert lib.halo_dev_dot2_cross(ctx.h, hal._lib.ptr(big), hal._lib.ptr(big), fp.CTX_N // 2 + 1, hal._lib.ptr(out)) == hal._lib.HALO_E_ARG
    assert b"exceeds context size" in lib.halo_last_error()
    assert lib.halo_dev_dot2_cross(ctx.h, None, None, 4, hal._lib.ptr(out)) == hal._lib.HALO_E_ARG and b"null pointer" in lib.halo_last_error()
    assert lib.halo_dev_dot2_cross(ctx.h, None, None, 0, hal._lib.ptr(out)) == 0 and not out.any()
