"""The open batches above the no-fold size: the small MSM pipeline with one base offset per member (halo_dev_msm_offsets), the
member-batched key folds (halo_dev_fold_points_batch: k_fold_points_batch, k_fold_points4_batch, k_fold_points4_quad_batch) and the
folded schedule of halo_pcdl_open_batch / halo_random_instance_batch / halo_instance_from_poly_batch forced by the hook
"open_batch_fold" -- every word, status and the final RNG state against the loop over the single calls, and against the oracle.
A lowered switch (halo_set_ipa_switch) brings every fold step -- one level, two levels, two steps -- down to keys of 2^7 .. 2^12
points; the full sizes 2^15 and 2^16 under the default switch run once."""
import ctypes as C

import numpy as np
import pytest

import fold_cases as fc
import orc

pytestmark = pytest.mark.gpu

R = fc.R
FOLD_KERNELS = ("k_fold_points_batch", "k_fold_points4_batch", "k_fold_points4_quad_batch")
GENERAL_SORT_KERNELS = ("k_msm_hist", "k_msm_scatter", "k_msm_coarse_hist", "k_msm_coarse_scatter", "k_msm_fine_sort")


@pytest.fixture(scope="module")
def hal():
    import halo_accumulation_amd as h
    return h


@pytest.fixture(scope="module")
def ctx(hal):
    """2^10 URS points, the switch at 2^6: opens of 2^7 .. 2^10 points fold their key"""
    c = hal._lib.Context(urs_n=1 << 10)
    c.set_ipa_switch(1 << 6)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx12(hal):
    c = hal._lib.Context(urs_n=1 << 12)
    c.set_ipa_switch(1 << 10)
    yield c
    c.close()


@pytest.fixture
def forced(hal):
    hal._lib.dev_hook("open_batch_fold", 1)
    yield
    hal._lib.dev_hook("reset", 0)


def ptr(a):
    from halo_accumulation_amd._lib import ptr as p
    return None if a is None else p(a)


# ------------------------------------------------------------------ 1. the small MSM pipeline, one base offset per member
def offset_sets(n, count, key_n):
    """all equal; all different, ascending and descending; pairwise equal (a round's L and R).  Different offsets are b * n where
    the key has room for count stretches of n points, else b * step with the largest step that keeps the last stretch inside it."""
    step = n if count * n <= key_n else (key_n - n) // max(count - 1, 1)
    asc = [b * step for b in range(count)]
    pairs = [(b // 2) * min(n, (key_n - n) // max((count - 1) // 2, 1)) for b in range(count)]
    return {"equal": [key_n - n] * count, "ascending": asc, "descending": asc[::-1], "pairwise": pairs}


@pytest.mark.parametrize("count", [1, 2, 5, 8])
@pytest.mark.parametrize("n", [64, 256])
def test_small_msm_with_member_offsets(hal, n, count):
    c = hal._lib.Context(urs_n=1 << 10)
    try:
        sc, _ = orc.rng_scalars(0x0FF5E7 + 16 * n + count, count * n)
        sc = sc.reshape(count, n, 4).copy()
        sc[:, 3] = 0
        sc[:, 5] = fc._mont(R - 1)
        sc[0, : n // 2] = 0  # (half of member 0's digits fall into no bucket)
        if count > 1:
            sc[count - 1] = fc._mont(R - 1)
        for name, offs in offset_sets(n, count, 1 << 10).items():
            assert all(0 <= o and o + n <= 1 << 10 for o in offs)
            want = np.stack([c.msm(sc[b], off=offs[b]) for b in range(count)])
            c.prof_enable(1)
            c.prof_reset()
            got = c.msm_offsets(offs, n, sc, mont=True)
            prof = c.prof()
            c.prof_enable(0)
            assert got.tolist() == want.tolist(), (name, offs)
            assert prof["k_smsm_sort"][1] == 1 and not [k for k in GENERAL_SORT_KERNELS if k in prof], (name, sorted(prof))
            assert c.msm_offsets(offs, n, sc, mont=True).tolist() == want.tolist(), (name, "without the profiler")
            c.set_small_path(0)
            try:
                assert c.msm_offsets(offs, n, sc, mont=True).tolist() == want.tolist(), (name, "the general pipeline")
            finally:
                c.set_small_path(-1)
    finally:
        c.close()


# ------------------------------------------------------------------ 2. the batched folds on their own
CHALLENGES = {1: [("xi", 1), ("xi", R - 1), ("xi", fc.RANDOM[0]), ("xi", fc.RANDOM[1])],
              2: [("pair", 1, 1), ("pair", R - 1, R - 1), ("pair", fc.RANDOM[5], fc.RANDOM[4]), ("pair", fc.RANDOM[0], R - 1)]}
FORMS = {1: (0, 1, 2), 2: (0, 1, 2, 3)}
_CASES = {}


def fold_cases(levels, m):
    """four exceptional keys (infinite, repeated, opposite and scalar-related points, rotated from case to case) with the
    challenges 1, r - 1 and random ones; the oracle's outputs and the single hook's, computed once"""
    if (levels, m) not in _CASES:
        _CASES[levels, m] = [fc.Case(levels, m, str(spec[1:]), spec, ci) for ci, spec in enumerate(CHALLENGES[levels])]
    return _CASES[levels, m]


@pytest.mark.parametrize("m", [32, 64, 129])
@pytest.mark.parametrize("levels", [1, 2])
def test_batched_folds_small(ctx, levels, m):
    cs = fold_cases(levels, m)
    before = ctx.read_bases()
    single = [ctx.fold_points(c.key, levels, c.scalars) for c in cs]
    for c, s in zip(cs, single):
        fc.assert_same(s, c.want, "the single hook, %s" % c.name)
    shared_single = [ctx.fold_points(cs[0].key, levels, c.scalars) for c in cs]  # every member's scalars over member 0's key
    for members in (1, 2, 3, 4):
        keys = np.concatenate([c.key for c in cs[:members]])
        scalars = np.concatenate([c.scalars for c in cs[:members]])
        for form in FORMS[levels]:
            what = "levels %d, m = %d, %d members, form %d" % (levels, m, members, form)
            got = ctx.fold_points_batch(keys, levels, scalars, members, shared=False, form=form)
            for b in range(members):
                assert np.array_equal(got[b], single[b]), (what, "own keys, member %d" % b)
                if m <= 64:
                    fc.assert_same(got[b], cs[b].want, what)
            got = ctx.fold_points_batch(cs[0].key, levels, scalars, members, shared=True, form=form)
            for b in range(members):
                assert np.array_equal(got[b], shared_single[b]), (what, "one key, member %d" % b)
            if m <= 64:
                fc.assert_same(got[0], cs[0].want, what)
    assert np.array_equal(ctx.read_bases(), before)


@pytest.mark.parametrize("levels,m,form", [(1, 1024, 2), (2, 1024, 2), (2, 128, 3), (2, 1024, 0), (1, 1024, 0)])
def test_batched_folds_span_blocks(hal, levels, m, form):
    """a member spans more than one block: 512 lanes of two outputs each, 512 lanes of the quad form; the context's key as the
    shared source (key_affine = NULL), and per-member keys folded in place"""
    n = 2 * levels * m
    c = hal._lib.Context(urs_n=n)
    try:
        key = c.read_bases()
        sc, _ = orc.rng_scalars(0xF01D + m + levels, 4 * 3)
        per = 1 if levels == 1 else 3
        scalars = sc[: 4 * per]
        single = [c.fold_points(None, levels, scalars[b * per: (b + 1) * per]) for b in range(4)]
        got = c.fold_points_batch(None, levels, scalars, 4, shared=True, form=form)
        for b in range(4):
            assert np.array_equal(got[b], single[b]), b
        own = np.concatenate([np.roll(key, 17 * b, axis=0) for b in range(3)])
        got = c.fold_points_batch(own, levels, scalars[: 3 * per], 3, shared=False, form=form)
        for b in range(3):
            want = c.fold_points(np.roll(key, 17 * b, axis=0), levels, scalars[b * per: (b + 1) * per])
            assert np.array_equal(got[b], want), b
        assert np.array_equal(c.read_bases(), key)
    finally:
        c.close()


# ------------------------------------------------------------------ the members of a batch, the loop, the batch
def members(c, lg, m, hiding, seed):
    """m seeded polynomials of degree bound d = 2^lg - 1, zero-padded: mixed degrees (every fourth at full degree); a plain batch
    also holds the zero polynomial (member 1) and a constant (member 2) -> (coeffs (m, d + 1, 4), Cs, zs, ws or None)"""
    from halo_accumulation_amd import pcdl
    d = (1 << lg) - 1
    ps = np.zeros((m, d + 1, 4), dtype=np.uint64)
    ws, s = orc.rng_scalars(seed, m)
    zs, s = orc.rng_scalars(s, m)
    Cs = np.zeros((m, 12), dtype=np.uint64)
    for i in range(m):
        deg = d if i % 4 == 0 else 1 + (i * 7919 + lg) % d
        if not hiding and i in (1, 2):
            deg = 0
        co, s = orc.rng_scalars(s, deg + 1)
        if not hiding and i == 1:
            co[:] = 0
        ps[i, : deg + 1] = co
        Cs[i] = pcdl.commit(c, ps[i], d, ws[i] if hiding else None)
    return ps, Cs, zs, (ws if hiding else None)


def open_loop(c, state, d, ps, Cs, zs, ws):
    lg = (d + 1).bit_length() - 1
    st = C.c_uint64(state)
    out, codes = [], []
    for i in range(len(ps)):
        pf = np.zeros(c.lib.halo_proof_words(lg), dtype=np.uint64)
        rc = c.lib.halo_pcdl_open(c.h, C.byref(st), ptr(ps[i]), d + 1, ptr(Cs[i]), d, ptr(zs[i]), ptr(None if ws is None else ws[i]), ptr(pf))
        codes.append(rc)
        out.append(pf if rc == 0 else np.zeros_like(pf))
    return np.array(out), codes, st.value


def open_batch(c, state, d, ps, Cs, zs, ws):
    m, lg = len(ps), (d + 1).bit_length() - 1
    st = C.c_uint64(state)
    out = np.zeros((m, c.lib.halo_proof_words(lg)), dtype=np.uint64)
    status = (C.c_int * m)(*([77] * m))
    rc = c.lib.halo_pcdl_open_batch(c.h, C.byref(st), d, ptr(np.ascontiguousarray(ps)), m, ptr(Cs), ptr(zs), ptr(ws), ptr(out), status)
    return rc, out, list(status), st.value


def expect_like_loop(c, state, d, ps, Cs, zs, ws, batched):
    """the batch against the loop; info(10) = `batched` members through member-batched launches"""
    want, codes, st_want = open_loop(c, state, d, ps, Cs, zs, ws)
    rc, got, status, st_got = open_batch(c, state, d, ps, Cs, zs, ws)
    assert status == codes and rc == ([x for x in codes if x] or [0])[0]
    for i in range(len(ps)):
        assert got[i].tolist() == want[i].tolist(), "member %d" % i
    assert st_got == st_want
    assert c.info(10) == batched
    return rc, got, status, st_got


def fold_steps(lg, switch_lg):
    """the levels of every fold step of an open of 2^lg points under a switch of 2^switch_lg"""
    steps, M = [], lg
    while M > switch_lg:
        k = min(2, M - switch_lg)
        steps.append(k)
        M -= k
    return steps


def fold_launches(c):
    return sum(cnt for name, (_, cnt) in c.prof().items() if name in FOLD_KERNELS)


# ------------------------------------------------------------------ 3. parity of the whole call with the loop, the schedule forced
def parity(c, lg, switch_lg, m, hiding):
    d = (1 << lg) - 1
    ps, Cs, zs, ws = members(c, lg, m, hiding, 0xF01D0000 + 64 * lg + m)
    ref = expect_like_loop(c, 0x5EED0000 + 100 * lg + m, d, ps, Cs, zs, ws, batched=m)
    if m == 5:  # the launches, seen by the profiler (which also takes the launch graphs away): one batched fold per group and step
        c.prof_enable(1)
        c.prof_reset()
        try:
            again = open_batch(c, 0x5EED0000 + 100 * lg + m, d, ps, Cs, zs, ws)
            assert again[1].tolist() == ref[1].tolist() and again[3] == ref[3]
            assert fold_launches(c) == 2 * len(fold_steps(lg, switch_lg)), (c.prof(), fold_steps(lg, switch_lg))  # groups of 4 + 1
        finally:
            c.prof_enable(0)


@pytest.mark.parametrize("hiding", [False, True])
@pytest.mark.parametrize("m", [1, 4, 5, 9])
@pytest.mark.parametrize("lg", [7, 8, 9, 10])
def test_parity_with_the_loop(ctx, forced, lg, m, hiding):
    assert fold_steps(lg, 6) == {7: [1], 8: [2], 9: [2, 1], 10: [2, 2]}[lg]
    parity(ctx, lg, 6, m, hiding)


@pytest.mark.parametrize("hiding", [False, True])
@pytest.mark.parametrize("m", [1, 4, 5, 9])
@pytest.mark.parametrize("lg", [11, 12])
def test_parity_with_the_loop_larger_key(ctx12, forced, lg, m, hiding):
    parity(ctx12, lg, 10, m, hiding)


@pytest.mark.parametrize("m", [1, 4, 5, 9])
def test_random_instance_batch(ctx, forced, m):
    lg = 8
    d = (1 << lg) - 1
    st = C.c_uint64(0x4A4D + m)
    want = np.zeros((m, ctx.lib.halo_instance_words(lg)), dtype=np.uint64)
    for i in range(m):
        assert ctx.lib.halo_random_instance(ctx.h, C.byref(st), d, ptr(want[i])) == 0
    got = np.zeros_like(want)
    st2 = C.c_uint64(0x4A4D + m)
    assert ctx.lib.halo_random_instance_batch(ctx.h, C.byref(st2), d, m, ptr(got)) == 0, ctx.lib.halo_last_error()
    assert got.tolist() == want.tolist() and st2.value == st.value  # (words 0 .. 11 of a blob: the member's C)
    assert ctx.info(10) == m


@pytest.mark.parametrize("hiding", [False, True])
@pytest.mark.parametrize("m", [1, 4, 5, 9])
@pytest.mark.parametrize("lg", [7, 8])
def test_instance_from_poly_batch(hal, ctx, forced, lg, m, hiding):
    d = (1 << lg) - 1
    ps, Cs, zs, ws = members(ctx, lg, m, hiding, 0x1F9 + 64 * lg + m)
    iw = ctx.lib.halo_instance_words(lg)
    st = C.c_uint64(0x1F9 + m)
    want = np.zeros((m, iw), dtype=np.uint64)
    for i in range(m):
        assert ctx.lib.halo_instance_from_poly(ctx.h, C.byref(st), ptr(ps[i]), d + 1, d, ptr(zs[i]), ptr(None if ws is None else ws[i]), ptr(want[i])) == 0
    for group in (0, 3):  # (m = 1 runs alone, as measured, unless the group is forced)
        hal._lib.dev_hook("open_batch_group", group)
        got = np.zeros_like(want)
        st2 = C.c_uint64(0x1F9 + m)
        status = (C.c_int * m)(*([77] * m))
        assert ctx.lib.halo_instance_from_poly_batch(ctx.h, C.byref(st2), d, ptr(np.ascontiguousarray(ps)), m, ptr(zs), ptr(ws), ptr(got), status) == 0
        assert got.tolist() == want.tolist() and st2.value == st.value and list(status) == [0] * m
        assert got[:, :12].tolist() == Cs.tolist(), "every member's C"
        assert ctx.info(10) == (0 if m == 1 and group == 0 else m)


# ------------------------------------------------------------------ 4. the oracle, its RNG state chained from member to member
def test_oracle(ctx, forced):
    lg, m = 8, 3
    d = (1 << lg) - 1
    ps, Cs, zs, ws = members(ctx, lg, m, True, 0x0AC1E)
    rc, got, status, st = open_batch(ctx, 0xFEED, d, ps, Cs, zs, ws)
    assert rc == 0 and status == [0] * m and ctx.info(10) == m
    pp = orc.make_pp(ctx.read_bases(0, d + 1))
    s = 0xFEED
    for i in range(m):
        deg = int(np.nonzero(ps[i].any(axis=1))[0][-1])
        ref, s = orc.pcdl_open(pp, s, np.ascontiguousarray(ps[i][: deg + 1]), Cs[i], d, zs[i], ws[i])
        assert got[i].tolist() == ref.tolist(), "member %d" % i
    assert st == s


# ------------------------------------------------------------------ 5. an exceptional key
def test_exceptional_key(hal, forced):
    """2^8 caller points folded two levels to 2^6: output j sums the points j, j + 64, j + 128, j + 192.  Infinities at one, at two
    and at all four of them, a repeated pair and an opposite pair among the partners, and an opposite pair at (j, j + 64)."""
    ua, uj = fc.urs(256)
    key = ua.copy()
    key[5] = 0
    key[6] = 0; key[6 + 128] = 0
    for t in range(4):
        key[7 + 64 * t] = 0
    key[10 + 128] = key[10 + 64]
    key[20 + 192] = fc.aff_of(fc.neg(uj[20 + 64]))
    key[30 + 64] = fc.aff_of(fc.neg(uj[30]))
    key[63] = key[62]
    c = hal._lib.Context(bases=key)
    try:
        c.set_ipa_switch(1 << 6)
        for hiding in (True, False):
            ps, Cs, zs, ws = members(c, 8, 5, hiding, 0xE8CE)
            expect_like_loop(c, 0xE8, 255, ps, Cs, zs, ws, batched=5)
        assert np.array_equal(c.read_bases(), key)
    finally:
        c.close()


# ------------------------------------------------------------------ 6. routes
def test_routes(hal, ctx):
    from halo_accumulation_amd import pcdl
    import torch
    lg, m = 9, 9
    d = (1 << lg) - 1
    ps, Cs, zs, ws = members(ctx, lg, m, True, 0x6E0)
    cl = ctx.clone()
    try:
        single_before = [pcdl.open(x, [9], ps[1], Cs[1], d, zs[1], ws[1]).tolist() for x in (ctx, cl)]
        hal._lib.dev_hook("open_batch_fold", 1)
        ref = expect_like_loop(ctx, 77, d, ps, Cs, zs, ws, batched=m)

        def same_as_ref(c, batched, why):
            got = open_batch(c, 77, d, ps, Cs, zs, ws)
            assert (got[0], got[1].tolist(), got[2], got[3]) == (ref[0], ref[1].tolist(), ref[2], ref[3]), why
            assert c.info(10) == batched, why

        for name, value, batched in (("open_batch_group", 1, m), ("open_batch_group", 2, m), ("open_batch_group", 3, m), ("batch_stage_fail", 1, 0),
                                     ("open_batch_fold", 2, 0)):
            hal._lib.dev_hook(name, value)
            try:
                same_as_ref(ctx, batched, (name, value))
            finally:
                hal._lib.dev_hook("reset", 0)
                hal._lib.dev_hook("open_batch_fold", 1)
        # a zero memory budget: a fresh context, no optional memory taken, the loop
        c0 = hal._lib.Context(urs_n=1 << 10)
        budget = c0.info(3)
        try:
            c0.set_ipa_switch(1 << 6)
            c0.set_memory_budget(0)
            before = c0.info(4)
            same_as_ref(c0, 0, "zero budget")
            assert c0.info(4) <= before, "no optional memory under a zero budget"
        finally:
            c0.set_memory_budget(budget)
            c0.close()
        # a failing member in the middle: the others are unaffected
        bad = ps.copy()
        bad[4] = 0
        bad[4][0] = ps[0][0]
        rc, got, status, st = expect_like_loop(ctx, 77, d, bad, Cs, zs, ws, batched=m - 1)
        assert rc == hal._lib.HALO_E_ASSERT and status == [0] * 4 + [hal._lib.HALO_E_ASSERT] + [0] * 4 and not got[4].any()
        assert got[:4].tolist() == ref[1][:4].tolist(), "the members in front of it"
        # a caller's MSM in flight on slot 3 is left alone
        n = 1 << 10
        sc, _ = orc.rng_scalars(0xC0FFEE, n)
        dev = torch.from_numpy(sc.view(np.int64).reshape(-1).copy()).cuda()
        ctx.msm_dev_begin(3, dev.data_ptr(), n)
        try:
            same_as_ref(ctx, m, "beside a caller's MSM")
        finally:
            res = ctx.msm_dev_end(3)
        assert res.tolist() == orc.msm_affine(ctx.read_bases(), sc).tolist(), "the caller's MSM on slot 3 kept its own result"
        # no lasting side effects: the context and its clone open as before
        hal._lib.dev_hook("reset", 0)
        assert [pcdl.open(x, [9], ps[1], Cs[1], d, zs[1], ws[1]).tolist() for x in (ctx, cl)] == single_before
    finally:
        hal._lib.dev_hook("reset", 0)
        cl.close()


# ------------------------------------------------------------------ 7. full size, once
def test_full_size(hal, forced):
    c = hal._lib.Context(urs_n=1 << 16)
    try:
        for lg in (15, 16):
            assert fold_steps(lg, 14) == [lg - 14]
            ps, Cs, zs, ws = members(c, lg, 5, True, 0xB16 + lg)
            expect_like_loop(c, 0xB16, (1 << lg) - 1, ps, Cs, zs, ws, batched=5)
    finally:
        c.close()
