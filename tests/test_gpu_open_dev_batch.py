"""halo_pcdl_open_dev_batch / halo_instance_from_poly_dev / halo_instance_from_poly_dev_batch: every word, status and the final RNG
state against the host forms over the same rows (halo_pcdl_open_batch, halo_instance_from_poly, halo_instance_from_poly_batch) and
against the oracle -- rows passed at full length with zero top coefficients, at degree + 1, and as null pointers of length 0; the
folded schedule and its launches; the routes without member-batched launches; members that fail alone; whole-call errors; the
source rows bit-identical after every call."""
import ctypes as C

import numpy as np
import pytest

import orc
from test_gpu_open_batch_fold import fold_launches, fold_steps, members, open_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hal():
    import halo_accumulation_amd as h
    return h


@pytest.fixture(scope="module")
def ctx(hal):
    c = hal._lib.Context(urs_n=1 << 10)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_fold(hal):
    """the switch at 2^6: opens of 2^7 .. 2^10 points fold their key"""
    c = hal._lib.Context(urs_n=1 << 10)
    c.set_ipa_switch(1 << 6)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def hooks_reset(hal):
    yield
    hal._lib.dev_hook("reset", 0)


def ptr(a):
    from halo_accumulation_amd._lib import ptr as p
    return None if a is None else p(a)


def degree(p):
    nz = np.nonzero(p.any(axis=1))[0]
    return int(nz[-1]) if len(nz) else 0


class DevRows:
    """the rows of ps (m, width, 4) in one device buffer; unchanged(): the buffer still holds what was uploaded"""

    def __init__(self, ps):
        import torch
        self.ps = np.ascontiguousarray(ps)
        self.width = self.ps.shape[1]
        self.dev = torch.from_numpy(self.ps.reshape(-1).view(np.int64).copy()).cuda()

    def ptrs(self, lens):
        """(a row of length 0 is passed as a null pointer)"""
        return [self.dev.data_ptr() + 32 * self.width * i if k else 0 for i, k in enumerate(lens)]

    def unchanged(self):
        return np.array_equal(self.dev.cpu().numpy().view(np.uint64), self.ps.reshape(-1))


def c_rows(ptrs, lens):
    m = len(ptrs)
    return (C.c_void_p * m)(*ptrs), (C.c_size_t * m)(*lens)


def open_dev_batch(c, state, d, rows, lens, Cs, zs, ws, ptrs=None):
    m, lg = len(lens), (d + 1).bit_length() - 1
    st = C.c_uint64(state)
    out = np.zeros((m, c.lib.halo_proof_words(lg)), dtype=np.uint64)
    status = (C.c_int * m)(*([77] * m))
    p, ln = c_rows(rows.ptrs(lens) if ptrs is None else ptrs, lens)
    rc = c.lib.halo_pcdl_open_dev_batch(c.h, C.byref(st), d, p, ln, m, ptr(Cs), ptr(zs), ptr(ws), ptr(out), status)
    assert rows.unchanged()
    return rc, out, list(status), st.value


def instance_batch(c, state, d, ps, zs, ws):
    m, lg = len(ps), (d + 1).bit_length() - 1
    st = C.c_uint64(state)
    out = np.zeros((m, c.lib.halo_instance_words(lg)), dtype=np.uint64)
    status = (C.c_int * m)(*([77] * m))
    rc = c.lib.halo_instance_from_poly_batch(c.h, C.byref(st), d, ptr(np.ascontiguousarray(ps)), m, ptr(zs), ptr(ws), ptr(out), status)
    return rc, out, list(status), st.value


def instance_dev_batch(c, state, d, rows, lens, zs, ws, ptrs=None):
    m, lg = len(lens), (d + 1).bit_length() - 1
    st = C.c_uint64(state)
    out = np.zeros((m, c.lib.halo_instance_words(lg)), dtype=np.uint64)
    status = (C.c_int * m)(*([77] * m))
    p, ln = c_rows(rows.ptrs(lens) if ptrs is None else ptrs, lens)
    rc = c.lib.halo_instance_from_poly_dev_batch(c.h, C.byref(st), d, p, ln, m, ptr(zs), ptr(ws), ptr(out), status)
    assert rows.unchanged()
    return rc, out, list(status), st.value


def same(got, want, why):
    assert got[0] == want[0] and got[2] == want[2] and got[3] == want[3], (why, got[0], got[2], want[2])
    for i in range(len(want[1])):
        assert got[1][i].tolist() == want[1][i].tolist(), (why, "member %d" % i)


def length_sets(ps, d, null_zero):
    """the same rows three ways: every row at d + 1 scalars (zero top coefficients wherever the degree is below d), every row at
    degree + 1 (the zero polynomial: length 0 and a null pointer where null_zero, else its one zero scalar), and the two in turn"""
    full = [d + 1] * len(ps)
    tight = [0 if null_zero and not ps[i].any() else degree(ps[i]) + 1 for i in range(len(ps))]
    return {"full": full, "tight": tight, "mixed": [full[i] if i % 2 else tight[i] for i in range(len(ps))]}


# ------------------------------------------------------------------ 1. parity with the host batch
@pytest.mark.parametrize("hiding", [False, True])
@pytest.mark.parametrize("m", [1, 4, 5, 9])
@pytest.mark.parametrize("lg", [1, 5, 8, 10])
def test_open_parity_with_the_host_batch(ctx, lg, m, hiding):
    d = (1 << lg) - 1
    ps, Cs, zs, ws = members(ctx, lg, m, hiding, 0xDE7B0000 + 64 * lg + m)
    state = 0x5EED0000 + 100 * lg + m
    want = open_batch(ctx, state, d, ps, Cs, zs, ws)
    assert want[0] == 0 and ctx.info(10) == m
    rows = DevRows(ps)
    sets = length_sets(ps, d, null_zero=True)
    if not hiding and m >= 4:
        assert sets["tight"][1] == 0 and sets["tight"][2] == 1, "the zero polynomial as a null row, a constant"
    if m >= 4 and (d > 1 or not hiding):  # (d = 1: a member that hides has degree 1, the full length)
        assert any(sets["full"][i] > sets["tight"][i] for i in range(m)), "a row with zero top coefficients"
    for name, lens in sets.items():
        same(open_dev_batch(ctx, state, d, rows, lens, Cs, zs, ws), want, name)
        assert ctx.info(10) == m, name


def test_open_equals_the_loop_over_open_dev(ctx):
    """every top coefficient non-zero: the batch is the loop over halo_pcdl_open_dev"""
    from halo_accumulation_amd import pcdl
    lg, m = 8, 5
    d = (1 << lg) - 1
    ps, Cs, zs, ws = members(ctx, lg, m, True, 0x100B)
    rows = DevRows(ps)
    lens = length_sets(ps, d, True)["tight"]
    rng = [0xAB]
    want = [pcdl.open_dev(ctx, rng, p, k, Cs[i], d, zs[i], ws[i]) for i, (p, k) in enumerate(zip(rows.ptrs(lens), lens))]
    rc, got, status, st = open_dev_batch(ctx, 0xAB, d, rows, lens, Cs, zs, ws)
    assert rc == 0 and status == [0] * m and st == rng[0]
    assert got.tolist() == np.array(want).tolist()
    rng = [0xAB]
    assert np.array(pcdl.open_dev_batch(ctx, rng, rows.ptrs(lens), lens, Cs, d, zs, ws)).tolist() == got.tolist() and rng[0] == st


def test_oracle(ctx):
    lg, m = 8, 3
    d = (1 << lg) - 1
    ps, Cs, zs, ws = members(ctx, lg, m, True, 0x0AC1E)
    rows = DevRows(ps)
    lens = length_sets(ps, d, True)["mixed"]
    rc, got, status, st = open_dev_batch(ctx, 0xFEED, d, rows, lens, Cs, zs, ws)
    assert rc == 0 and status == [0] * m and ctx.info(10) == m
    pp = orc.make_pp(ctx.read_bases(0, d + 1))
    s = 0xFEED
    for i in range(m):
        ref, s = orc.pcdl_open(pp, s, np.ascontiguousarray(ps[i][: degree(ps[i]) + 1]), Cs[i], d, zs[i], ws[i])
        assert got[i].tolist() == ref.tolist(), "member %d" % i
    assert st == s


# ------------------------------------------------------------------ 2. the Instance forms
def instance_members(lg, m, hiding, seed):
    """degrees 15 and 16 (the two sides of the host commit's shortcut) among full and seeded degrees; plain: the zero polynomial
    and a constant too -> (coeffs (m, d + 1, 4), zs, ws or None)"""
    d = (1 << lg) - 1
    degs = ([d, 15, 16, 37, d, 1, 100, 16, 15] if hiding else [d, -1, 0, 15, 16, 37, d, 1, 100])[:m]
    ws, s = orc.rng_scalars(seed, m)
    zs, s = orc.rng_scalars(s, m)
    ps = np.zeros((m, d + 1, 4), dtype=np.uint64)
    for i, deg in enumerate(degs):
        co, s = orc.rng_scalars(s, d + 1)
        ps[i, : deg + 1] = co[: deg + 1]
    return ps, zs, (ws if hiding else None)


@pytest.mark.parametrize("hiding", [False, True])
@pytest.mark.parametrize("m", [1, 5, 9])
def test_instance_forms(hal, ctx, m, hiding):
    from halo_accumulation_amd import acc, pcdl
    lg = 8
    d = (1 << lg) - 1
    ps, zs, ws = instance_members(lg, m, hiding, 0x1F9D + m)
    w_of = lambda i: None if ws is None else ws[i]
    rows = DevRows(ps)
    state = 0x1F9 + m
    for name, lens in length_sets(ps, d, null_zero=True).items():
        ptrs = rows.ptrs(lens)
        Cs = [pcdl.commit_dev(ctx, ptrs[i], lens[i], d, w_of(i)).tolist() for i in range(m)]
        # the single form against halo_instance_from_poly, member by member, the state chained
        st_host, st_dev = [state], [state]
        for i in range(m):
            want = acc.instance_from_poly(ctx, st_host, ps[i], d, zs[i], w_of(i))
            got = acc.instance_from_poly_dev(ctx, st_dev, ptrs[i], lens[i], d, zs[i], w_of(i))
            assert got.tolist() == want.tolist() and st_dev == st_host, (name, i)
            assert got[:12].tolist() == Cs[i], (name, i)
        for group in (0, 3):  # (m = 1 runs alone, the host form's rule, unless the group is forced)
            hal._lib.dev_hook("open_batch_group", group)
            want = instance_batch(ctx, state, d, ps, zs, ws)
            batched = 0 if m == 1 and group == 0 else m
            assert want[0] == 0 and want[3] == st_host[0] and ctx.info(10) == batched
            got = instance_dev_batch(ctx, state, d, rows, lens, zs, ws)
            same(got, want, (name, group))
            assert ctx.info(10) == batched, (name, group)
            assert got[1][:, :12].tolist() == Cs, "every member's C is halo_pcdl_commit_dev's"
    assert rows.unchanged()
    rng = [state]
    hal._lib.dev_hook("open_batch_group", 3)
    lens = [d + 1] * m
    assert np.array(acc.instance_from_poly_dev_batch(ctx, rng, rows.ptrs(lens), lens, d, zs, ws)).tolist() == got[1].tolist() and rng[0] == got[3]


# ------------------------------------------------------------------ 3. the folded schedule and its launches
@pytest.mark.parametrize("hiding", [False, True])
@pytest.mark.parametrize("lg", [8, 9])
def test_folded_schedule(hal, ctx_fold, lg, hiding):
    c, m = ctx_fold, 5
    d = (1 << lg) - 1
    hal._lib.dev_hook("open_batch_fold", 1)
    ps, Cs, zs, ws = members(c, lg, m, hiding, 0xF01DDE7 + lg)
    want = open_batch(c, 0x5EED + lg, d, ps, Cs, zs, ws)
    assert want[0] == 0 and c.info(10) == m
    rows = DevRows(ps)
    lens = length_sets(ps, d, True)["mixed"]
    same(open_dev_batch(c, 0x5EED + lg, d, rows, lens, Cs, zs, ws), want, "folded")
    assert c.info(10) == m
    want_inst = instance_batch(c, 0x5EED + lg, d, ps, zs, ws)
    same(instance_dev_batch(c, 0x5EED + lg, d, rows, lens, zs, ws), want_inst, "folded, instances")
    assert c.info(10) == m
    c.prof_enable(1)  # (the profiler also takes the launch graphs away)
    c.prof_reset()
    try:
        got = open_dev_batch(c, 0x5EED + lg, d, rows, lens, Cs, zs, ws)
    finally:
        c.prof_enable(0)  # (collects the launches' events)
    same(got, want, "folded, profiled")
    prof = c.prof()
    assert fold_launches(c) == 2 * len(fold_steps(lg, 6)), (prof, fold_steps(lg, 6))  # groups of 4 + 1
    assert prof["k_pad_members_batch"][1] == 2, "one padding launch per group"
    assert prof["k_poly_degree_batch"][1] == 1, "one degree launch per call"


# ------------------------------------------------------------------ 4. routes without member-batched launches
def test_routes(hal, ctx_fold):
    c, lg, m = ctx_fold, 9, 5
    d = (1 << lg) - 1
    ps, Cs, zs, ws = members(c, lg, m, True, 0x6E0DE7)
    rows = DevRows(ps)
    lens = length_sets(ps, d, True)["mixed"]
    hal._lib.dev_hook("open_batch_fold", 1)
    want = open_batch(c, 77, d, ps, Cs, zs, ws)
    want_inst = instance_batch(c, 77, d, ps, zs, ws)
    assert want[0] == 0 and want_inst[0] == 0 and c.info(10) == m

    def both(cc, batched, why):
        same(open_dev_batch(cc, 77, d, rows, lens, Cs, zs, ws), want, why)
        assert cc.info(10) == batched, why
        same(instance_dev_batch(cc, 77, d, rows, lens, zs, ws), want_inst, why)
        assert cc.info(10) == batched, why

    both(c, m, "the folded schedule")
    for name, value in (("batch_stage_fail", 1), ("open_batch_fold", 2)):
        hal._lib.dev_hook(name, value)
        try:
            both(c, 0, (name, value))
        finally:
            hal._lib.dev_hook("reset", 0)
            hal._lib.dev_hook("open_batch_fold", 1)
    # a zero memory budget: a fresh context, no optional memory taken, the loop over the single device bodies
    c0 = hal._lib.Context(urs_n=1 << 10)
    budget = c0.info(3)
    try:
        c0.set_ipa_switch(1 << 6)
        c0.set_memory_budget(0)
        before = c0.info(4)
        both(c0, 0, "zero budget")
        assert c0.info(4) <= before, "no optional memory under a zero budget"
    finally:
        c0.set_memory_budget(budget)
        c0.close()


# ------------------------------------------------------------------ 5. members that fail alone
@pytest.mark.parametrize("hiding", [False, True])
def test_a_member_longer_than_the_bound_fails_alone(hal, ctx, hiding):
    lg, m, bad = 8, 5, 2
    d = (1 << lg) - 1
    ps, Cs, zs, ws = members(ctx, lg, m, hiding, 0xBAD0 + hiding)
    wide = np.zeros((m, d + 3, 4), dtype=np.uint64)  # rows of d + 3 scalars: the bad member's d + 2 are all non-zero
    wide[:, : d + 1] = ps
    wide[bad, : d + 2] = orc.rng_scalars(0xBAD, d + 2)[0]
    rows = DevRows(wide)
    lens = [d + 1] * m
    lens[bad] = d + 2
    keep = [i for i in range(m) if i != bad]
    sub = lambda a: None if a is None else np.ascontiguousarray(a[keep])
    E = hal._lib.HALO_E_ASSERT
    want = open_batch(ctx, 0xBAD5EED, d, ps[keep], sub(Cs), sub(zs), sub(ws))
    rc, got, status, st = open_dev_batch(ctx, 0xBAD5EED, d, rows, lens, Cs, zs, ws)
    assert rc == E and status == [0, 0, E, 0, 0] and st == want[3], "the member draws nothing"
    assert ctx.lib.halo_last_error().decode() == "member 2: open: p.degree() > d"
    assert not got[bad].any() and got[keep].tolist() == want[1].tolist()
    assert ctx.info(10) == m - 1
    want = instance_batch(ctx, 0xBAD5EED, d, ps[keep], sub(zs), sub(ws))
    rc, got, status, st = instance_dev_batch(ctx, 0xBAD5EED, d, rows, lens, zs, ws)
    assert rc == E and status == [0, 0, E, 0, 0] and st == want[3]
    assert ctx.lib.halo_last_error().decode() == "member 2: commit: p.degree() > d"
    assert not got[bad].any() and got[keep].tolist() == want[1].tolist()
    # the single form: the commit's assert, nothing written
    inst = np.full(ctx.lib.halo_instance_words(lg), 7, dtype=np.uint64)
    s1 = C.c_uint64(5)
    rc = ctx.lib.halo_instance_from_poly_dev(ctx.h, C.byref(s1), C.c_void_p(rows.ptrs(lens)[bad]), d + 2, d, ptr(zs[0]), None, ptr(inst))
    assert rc == E and ctx.lib.halo_last_error().decode() == "commit: p.degree() > d" and s1.value == 5 and (inst == 7).all()


def test_a_hiding_constant_fails_alone(hal, ctx):
    lg, m = 5, 4
    d = (1 << lg) - 1
    ps, Cs, zs, ws = members(ctx, lg, m, True, 0xC0457)
    ps = ps.copy()
    ps[1, 1:] = 0  # a constant that hides
    rows = DevRows(ps)
    E = hal._lib.HALO_E_ASSERT
    want = open_batch(ctx, 9, d, ps, Cs, zs, ws)
    assert want[0] == E and want[2] == [0, E, 0, 0]
    for name, lens in length_sets(ps, d, True).items():
        same(open_dev_batch(ctx, 9, d, rows, lens, Cs, zs, ws), want, name)
        assert "member 1: open: hiding needs p.degree() >= 1" == ctx.lib.halo_last_error().decode()
    want = instance_batch(ctx, 9, d, ps, zs, ws)
    assert want[0] == E
    same(instance_dev_batch(ctx, 9, d, rows, [d + 1] * m, zs, ws), want, "instances")


# ------------------------------------------------------------------ 6. whole-call errors, and a caller's MSM beside the call
def test_whole_call_errors(hal, ctx):
    import torch
    lg, m = 8, 5
    d = (1 << lg) - 1
    ps, Cs, zs, ws = members(ctx, lg, m, True, 0xE220)
    rows = DevRows(ps)
    lens = [d + 1] * m
    good = rows.ptrs(lens)
    A = hal._lib.HALO_E_ARG

    def refused(ptrs, ln, code, message, dd=d):
        for fn in (lambda: open_dev_batch(ctx, 5, dd, rows, ln, Cs, zs, ws, ptrs=ptrs), lambda: instance_dev_batch(ctx, 5, dd, rows, ln, zs, ws, ptrs=ptrs)):
            rc, out, status, st = fn()
            assert rc == code and message in ctx.lib.halo_last_error().decode(), ctx.lib.halo_last_error()
            assert status == [77] * m and st == 5 and not out.any(), "nothing written"

    refused(good[:2] + [good[2] + 16] + good[3:], lens, A, "null or misaligned pointer")
    refused(good[:4] + [0], lens, A, "null or misaligned pointer")
    refused(good, lens, hal._lib.HALO_E_ASSERT, "d + 1 is not a power of two", dd=d - 1)
    refused(good, lens, hal._lib.HALO_E_ASSERT, "d > D", dd=(1 << 11) - 1)
    st = C.c_uint64(5)
    out = np.zeros((m, ctx.lib.halo_proof_words(lg)), dtype=np.uint64)
    assert ctx.lib.halo_pcdl_open_dev_batch(ctx.h, C.byref(st), d, None, None, m, ptr(Cs), ptr(zs), ptr(ws), ptr(out), None) == A
    assert ctx.lib.halo_pcdl_open_dev_batch(ctx.h, C.byref(st), d, None, None, 0, None, None, None, None, None) == 0 and st.value == 5
    # beside a caller's MSM on slot 3: the same results, and the caller's MSM keeps its own
    want = open_batch(ctx, 5, d, ps, Cs, zs, ws)
    want_inst = instance_batch(ctx, 5, d, ps, zs, ws)
    n = 1 << 10
    sc, _ = orc.rng_scalars(0xC0FFEE, n)
    dev = torch.from_numpy(sc.view(np.int64).reshape(-1).copy()).cuda()
    ctx.msm_dev_begin(3, dev.data_ptr(), n)
    try:
        same(open_dev_batch(ctx, 5, d, rows, lens, Cs, zs, ws), want, "beside a caller's MSM")
        assert ctx.info(10) == m
        same(instance_dev_batch(ctx, 5, d, rows, lens, zs, ws), want_inst, "beside a caller's MSM, instances")
    finally:
        res = ctx.msm_dev_end(3)
    assert res.tolist() == orc.msm_affine(ctx.read_bases(), sc).tolist(), "the caller's MSM on slot 3 kept its own result"
    # every slot busy: the host batch's error
    for slot in range(4):
        ctx.msm_dev_begin(slot, dev.data_ptr(), n)
    try:
        rc, out, status, st = open_dev_batch(ctx, 5, d, rows, lens, Cs, zs, ws)
        assert rc == A and "every slot has an MSM in flight" in ctx.lib.halo_last_error().decode() and status == [77] * m and st == 5
    finally:
        for slot in range(4):
            ctx.msm_dev_end(slot)
