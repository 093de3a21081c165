"""halo_pcdl_commit_batch / halo_pcdl_commit_dev_batch on the GPU: every point against halo_pcdl_commit / halo_pcdl_commit_dev on
that member and against the oracle -- plain, hiding and w = 0; the zero polynomial, constants, both sides of the host shortcut,
full degree, r - 1 everywhere; every group size the rotation meets, without staging, beside a caller's MSM; whole-call errors;
device-resident members of every length class in one group; the general and the table pipelines."""
import ctypes as C

import numpy as np
import pytest

import orc
from pallas_model import R_ORDER

pytestmark = pytest.mark.gpu

KEY_LG = 10
M_MAX = 37  # 4 slots x 8 members + 5: every slot comes round again and the last group is partial


@pytest.fixture(scope="module")
def hal():
    import halo_accumulation_amd as h
    return h


@pytest.fixture(scope="module")
def ctx(hal):
    c = hal._lib.Context(urs_n=1 << KEY_LG)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pp(ctx):
    return orc.make_pp(ctx.read_bases())


def ptr(a):
    from halo_accumulation_amd._lib import ptr as p
    return None if a is None else p(a)


_members = {}


def members(n):
    """M_MAX seeded polynomials zero-padded to n coefficients, the kinds in turn: the zero polynomial, a constant, degree exactly
    15 and exactly 16 (the two sides of the host shortcut, where n holds them), full degree, every coefficient r - 1, upper
    half zero, a seeded degree.  -> (coeffs (M_MAX, n, 4), ws (M_MAX, 4)); computed once per n and never written"""
    if n not in _members:
        ps = np.zeros((M_MAX, n, 4), dtype=np.uint64)
        ws, s = orc.rng_scalars(0xC0AA1700 + n, M_MAX)
        minus_one = orc.fr_to_mont(R_ORDER - 1)
        for i in range(M_MAX):
            kind = i % 8
            co, s = orc.rng_scalars(s, n)
            if kind == 0:
                deg = -1
            elif kind == 1:
                deg = 0
            elif kind == 2:
                deg = min(15, n - 1)
            elif kind == 3:
                deg = min(16, n - 1)
            elif kind == 4:
                deg = n - 1
            elif kind == 5:
                deg = n - 1
                co[:] = minus_one
            elif kind == 6:
                deg = n // 2 - 1
            else:
                deg = (i * 7919) % n
            ps[i, : deg + 1] = co[: deg + 1]
        ps.setflags(write=False)
        ws.setflags(write=False)
        _members[n] = (ps, ws)
    return _members[n]


MODES = ("plain", "hiding", "w0")


def ws_of(mode, ws, m):
    if mode == "plain":
        return None
    return np.ascontiguousarray(ws[:m]) if mode == "hiding" else np.zeros((m, 4), dtype=np.uint64)


_singles = {}


def singles(c, n, mode):
    """halo_pcdl_commit on each of the M_MAX members of size n (once per n and mode, on the module's context)"""
    if (n, mode) not in _singles:
        from halo_accumulation_amd import pcdl
        ps, ws = members(n)
        w = ws_of(mode, ws, M_MAX)
        _singles[(n, mode)] = np.array([pcdl.commit(c, ps[i], n - 1, None if w is None else w[i]) for i in range(M_MAX)])
    return _singles[(n, mode)]


_oracle = {}


def oracle(pp, n, mode):
    """orc.pcdl_commit on each of the M_MAX members of size n, from their deg + 1 coefficients (once per n and mode)"""
    if (n, mode) not in _oracle:
        ps, ws = members(n)
        w = ws_of(mode, ws, M_MAX)
        pts = []
        for i in range(M_MAX):
            deg = int(np.nonzero(ps[i].any(axis=1))[0][-1]) if ps[i].any() else 0
            pts.append(orc.pcdl_commit(pp, np.ascontiguousarray(ps[i][: deg + 1]), n - 1, None if w is None else w[i]))
        _oracle[(n, mode)] = np.array(pts)
    return _oracle[(n, mode)]


def batch(c, d, coeffs, m, ws):
    """one halo_pcdl_commit_batch -> (code, points (marked where not written), message)"""
    out = np.full((max(m, 1), 12), 0xA5, dtype=np.uint64)
    rc = c.lib.halo_pcdl_commit_batch(c.h, d, ptr(None if coeffs is None else np.ascontiguousarray(coeffs)), m, ptr(ws), ptr(out))
    return rc, out[:m], c.lib.halo_last_error().decode() if rc else ""


# ------------------------------------------------------------------ 1. parity with the single call and the oracle
@pytest.mark.parametrize("m", [1, 8, 9, M_MAX])
@pytest.mark.parametrize("n", [2, 16, 32, 64, 1024])
def test_parity(hal, ctx, pp, n, m):
    ps, ws = members(n)
    for mode in MODES:
        w = ws_of(mode, ws, m)
        rc, got, msg = batch(ctx, n - 1, ps[:m], m, w)
        assert rc == 0, msg
        assert got.tolist() == singles(ctx, n, mode)[:m].tolist(), mode
        assert got.tolist() == oracle(pp, n, mode)[:m].tolist(), mode


def test_zero_polynomial_points(hal, ctx):
    from halo_accumulation_amd import pcdl
    n = 64
    ps, ws = members(n)
    assert not ps[0].any()
    plain = pcdl.commit_batch(ctx, [ps[0]], n - 1)[0]
    assert plain[:4].tolist() == plain[4:8].tolist() and plain[:4].any() and not plain[8:].any(), "(1, 1, 0)"
    assert plain.tolist() == pcdl.commit(ctx, ps[0], n - 1).tolist()
    hid = pcdl.commit_batch(ctx, [ps[0]], n - 1, [ws[0]])[0]
    assert hid.tolist() == pcdl.commit(ctx, ps[0], n - 1, ws[0]).tolist() and hid[8:].any(), "w S"


# ------------------------------------------------------------------ 2. group rotation, fallback
@pytest.mark.parametrize("n", [32, 1024])
def test_group_sizes_and_fallback(hal, ctx, n):
    ps, ws = members(n)
    m = 13
    for mode in ("plain", "hiding"):
        w = ws_of(mode, ws, m)
        want = singles(ctx, n, mode)[:m].tolist()
        for name, value in (("commit_batch_group", 1), ("commit_batch_group", 3), ("batch_stage_fail", 1)):
            hal._lib.dev_hook(name, value)
            try:
                rc, got, msg = batch(ctx, n - 1, ps[:m], m, w)
                assert rc == 0 and got.tolist() == want, (name, value, mode, msg)
            finally:
                hal._lib.dev_hook("reset", 0)


def test_without_memory_budget(hal):
    n, m = 64, 9
    ps, ws = members(n)
    c = hal._lib.Context(urs_n=1 << KEY_LG)  # (a fresh context: no staging grown before the budget goes to zero)
    budget = c.info(3)
    try:
        want = batch(c, n - 1, ps[:m], m, np.ascontiguousarray(ws[:m]))
        assert want[0] == 0
    finally:
        c.close()
    c = hal._lib.Context(urs_n=1 << KEY_LG)
    try:
        c.set_memory_budget(0)
        before = c.info(4)
        rc, got, msg = batch(c, n - 1, ps[:m], m, np.ascontiguousarray(ws[:m]))
        assert rc == 0 and got.tolist() == want[1].tolist(), msg
        assert c.info(4) <= before, "no optional memory under a zero budget"
    finally:
        c.set_memory_budget(budget)
        c.close()


# ------------------------------------------------------------------ 3. slots
def test_beside_a_callers_msm(hal, ctx):
    import torch
    n, m = 1024, 20
    ps, ws = members(n)
    w = np.ascontiguousarray(ws[:m])
    want = singles(ctx, n, "hiding")[:m].tolist()
    sc, _ = orc.rng_scalars(0xC0FFEE, n)
    dev = torch.from_numpy(sc.view(np.int64).reshape(-1).copy()).cuda()
    own = orc.msm_affine(ctx.read_bases(), sc).tolist()
    dptrs = [dev.data_ptr()] * 3
    for busy in (0, 3):  # (slot 0 is the one the single calls use)
        for stage_fail in (0, 1):
            ctx.msm_dev_begin(busy, dev.data_ptr(), n)
            hal._lib.dev_hook("batch_stage_fail", stage_fail)
            try:
                rc, got, msg = batch(ctx, n - 1, ps[:m], m, w)
                got_dev = pcdl_dev_batch(ctx, dptrs, [n, n - 5, 3], n - 1)
            finally:
                hal._lib.dev_hook("reset", 0)
                res = ctx.msm_dev_end(busy)
            assert res.tolist() == own, "the caller's MSM on slot %d kept its own result" % busy
            assert rc == 0 and got.tolist() == want, (busy, stage_fail, msg)
            assert got_dev.tolist() == [ctx_commit_dev(ctx, dptrs[i], k, n - 1, None).tolist() for i, k in enumerate([n, n - 5, 3])], (busy, stage_fail)
    for slot in range(4):
        ctx.msm_dev_begin(slot, dev.data_ptr(), n)
    try:
        rc, got, msg = batch(ctx, n - 1, ps[:m], m, w)
        assert rc == hal._lib.HALO_E_ARG and (got == 0xA5).all(), "no idle slot: nothing written"
        ptrs = (C.c_void_p * 1)(dev.data_ptr())
        lens = (C.c_size_t * 1)(n)
        status = (C.c_int * 1)(77)
        out = np.full((1, 12), 0xA5, dtype=np.uint64)
        assert ctx.lib.halo_pcdl_commit_dev_batch(ctx.h, n - 1, ptrs, lens, 1, None, ptr(out), status) == hal._lib.HALO_E_ARG
        assert (out == 0xA5).all() and status[0] == 77
    finally:
        for slot in range(4):
            assert ctx.msm_dev_end(slot).tolist() == res.tolist()


# ------------------------------------------------------------------ 4. whole-call errors
def test_whole_call_errors(hal, ctx):
    n, m = 32, 3
    ps, ws = members(n)
    w = np.ascontiguousarray(ws[:m])
    E_ARG, E_ASSERT = hal._lib.HALO_E_ARG, hal._lib.HALO_E_ASSERT
    for dd, want in ((30, "commit: d + 1 is not a power of two"), ((1 << (KEY_LG + 1)) - 1, "commit: d > D")):
        rc, got, msg = batch(ctx, dd, ps[:m], m, w)
        assert (rc, msg) == (E_ASSERT, want) and (got == 0xA5).all()
        single = np.zeros(12, dtype=np.uint64)
        assert ctx.lib.halo_pcdl_commit(ctx.h, ptr(np.ascontiguousarray(ps[0])), 1, dd, None, ptr(single)) == rc
        assert ctx.lib.halo_last_error().decode() == want, "the single call's message"
    rc, got, _ = batch(ctx, n - 1, None, m, w)
    assert rc == E_ARG and (got == 0xA5).all()
    assert ctx.lib.halo_pcdl_commit_batch(ctx.h, n - 1, ptr(np.ascontiguousarray(ps[:m])), m, ptr(w), None) == E_ARG
    assert batch(ctx, n - 1, None, 0, None)[0] == 0
    assert ctx.lib.halo_pcdl_commit_batch(ctx.h, n - 1, None, 0, None, None) == 0, "m = 0"
    # the device form's own
    out = np.full((m, 12), 0xA5, dtype=np.uint64)
    status = (C.c_int * m)(*([77] * m))
    ptrs = (C.c_void_p * m)(0, 0, 0)
    lens = (C.c_size_t * m)(0, 0, 0)

    def dev_call(d, p, ln, o):
        rc = ctx.lib.halo_pcdl_commit_dev_batch(ctx.h, d, p, ln, m, ptr(w), o, status)
        return rc, ctx.lib.halo_last_error().decode() if rc else ""

    assert dev_call(n - 1, None, lens, ptr(out))[0] == E_ARG
    assert dev_call(n - 1, ptrs, None, ptr(out))[0] == E_ARG
    assert dev_call(n - 1, ptrs, lens, None)[0] == E_ARG
    assert dev_call(n - 1, ptrs, (C.c_size_t * m)(0, 4, 0), ptr(out))[0] == E_ARG, "a null pointer with a length"
    assert dev_call(30, ptrs, lens, ptr(out)) == (E_ASSERT, "commit: d + 1 is not a power of two")
    assert dev_call((1 << (KEY_LG + 1)) - 1, ptrs, lens, ptr(out)) == (E_ASSERT, "commit: d > D")
    assert (out == 0xA5).all() and list(status) == [77] * m
    assert ctx.lib.halo_pcdl_commit_dev_batch(ctx.h, n - 1, None, None, 0, None, None, None) == 0, "m = 0"
    assert dev_call(n - 1, ptrs, lens, ptr(out)) == (0, ""), "empty members: the point at infinity, or w S"
    assert out.tolist() == [ctx_commit_dev(ctx, 0, 0, n - 1, w[i]).tolist() for i in range(m)] and list(status) == [0] * m


def pcdl_dev_batch(c, dptrs, lens, d, ws=None):
    from halo_accumulation_amd import pcdl
    return pcdl.commit_dev_batch(c, dptrs, lens, d, ws)


def ctx_commit_dev(c, dptr, length, d, w):
    from halo_accumulation_amd import pcdl
    return pcdl.commit_dev(c, dptr, length, d, w)


# ------------------------------------------------------------------ 5. device-resident polynomials
def device_members(n, lens, seed):
    import torch
    host, dev = [], []
    s = seed
    for k in lens:
        co, s = orc.rng_scalars(s, max(k, 1))
        co = co[:k]
        host.append(co)
        dev.append(torch.from_numpy(co.view(np.int64).reshape(-1).copy()).cuda() if k else None)
    return host, dev


@pytest.mark.parametrize("hiding", [False, True])
def test_device_form(hal, ctx, pp, hiding):
    import torch
    from halo_accumulation_amd import pcdl
    n = 1 << KEY_LG
    d = n - 1
    # group of 2: slot 0 takes (n - 1, n) and then (2, n) -- a padded row that held a longer member, an in-place neighbour;
    # group of 1: slot 0 takes n - 1, then 1, then 2; the default: all ten members in two groups
    lens = [n - 1, n, 17, 16, 1, 0, n, 5, 2, n]
    m = len(lens)
    assert {0, 1, 16, 17, n - 1, n} <= set(lens)
    host, dev = device_members(n, lens, 0xDE7 + hiding)
    ws, _ = orc.rng_scalars(0xDE77, m)
    w = ws if hiding else None
    dptrs = [t.data_ptr() if t is not None else 0 for t in dev]
    want = [pcdl.commit_dev(ctx, dptrs[i], lens[i], d, None if w is None else w[i]).tolist() for i in range(m)]
    for i in range(m):
        co = host[i] if lens[i] else np.zeros((1, 4), dtype=np.uint64)
        assert want[i] == orc.pcdl_commit(pp, np.ascontiguousarray(co), d, None if w is None else w[i]).tolist(), i
    for g in (0, 1, 2, 3):
        hal._lib.dev_hook("commit_batch_group", g)
        try:
            assert pcdl.commit_dev_batch(ctx, dptrs, lens, d, w).tolist() == want, g
        finally:
            hal._lib.dev_hook("reset", 0)
    hal._lib.dev_hook("batch_stage_fail", 1)
    try:
        assert pcdl.commit_dev_batch(ctx, dptrs, lens, d, w).tolist() == want, "without staging"
    finally:
        hal._lib.dev_hook("reset", 0)
    torch.cuda.synchronize()
    for i in range(m):
        if lens[i]:
            assert dev[i].cpu().numpy().view(np.uint64).reshape(-1, 4).tolist() == host[i].tolist(), "member %d was written" % i


def test_device_form_failing_member(hal, ctx, pp):
    import torch
    from halo_accumulation_amd import pcdl
    n = 64
    d = n - 1
    lens = [n, n + 1, 7, n + 3, n - 1]
    m = len(lens)
    host, dev = device_members(n, lens, 0xFA17)
    ws, _ = orc.rng_scalars(0xFA18, m)
    ptrs = (C.c_void_p * m)(*[t.data_ptr() for t in dev])
    ln = (C.c_size_t * m)(*lens)
    out = np.full((m, 12), 0xA5, dtype=np.uint64)
    status = (C.c_int * m)(*([77] * m))
    rc = ctx.lib.halo_pcdl_commit_dev_batch(ctx.h, d, ptrs, ln, m, ptr(ws), ptr(out), status)
    E = hal._lib.HALO_E_ASSERT
    assert rc == E and ctx.lib.halo_last_error().decode() == "member 1: commit: p.degree() > d"
    assert list(status) == [0, E, 0, E, 0]
    for i in range(m):
        if lens[i] > n:
            assert not out[i].any()
            with pytest.raises(AssertionError, match="commit: p.degree\\(\\) > d"):
                pcdl.commit_dev(ctx, dev[i].data_ptr(), lens[i], d, ws[i])
        else:
            assert out[i].tolist() == pcdl.commit_dev(ctx, dev[i].data_ptr(), lens[i], d, ws[i]).tolist(), i
            assert out[i].tolist() == orc.pcdl_commit(pp, np.ascontiguousarray(host[i]), d, ws[i]).tolist(), i
    with pytest.raises(AssertionError) as e:
        pcdl.commit_dev_batch(ctx, [t.data_ptr() for t in dev], lens, d, ws)
    assert e.value.args[1] == [0, E, 0, E, 0] and e.value.args[2].tolist() == out.tolist()
    torch.cuda.synchronize()
    for i in range(m):
        assert dev[i].cpu().numpy().view(np.uint64).reshape(-1, 4).tolist() == host[i].tolist()


# ------------------------------------------------------------------ 6. the general pipeline and the table pipeline
def big_members(n, m, seed):
    ps = np.zeros((m, n, 4), dtype=np.uint64)
    s = seed
    for i in range(m):
        deg = n - 1 if i == 0 else n - 1 - (i * 7919) % (n // 2)
        co, s = orc.rng_scalars(s, deg + 1)
        ps[i, : deg + 1] = co
    ws, _ = orc.rng_scalars(s, m)
    return ps, ws


def test_general_pipeline(hal):
    """2^17 points: the smallest size at which a batched launch leaves the small pipeline (msm_plan: n <= 2^16 stays in it)"""
    from halo_accumulation_amd import pcdl
    n, m = 1 << 17, 3
    c = hal._lib.Context(urs_n=n)
    try:
        ps, ws = big_members(n, m, 0x6E17)
        want = [pcdl.commit(c, ps[i], n - 1, ws[i]).tolist() for i in range(m)]
        hal._lib.dev_hook("commit_batch_group", 2)
        try:
            rc, got, msg = batch(c, n - 1, ps, m, ws)
        finally:
            hal._lib.dev_hook("reset", 0)
        assert rc == 0 and got.tolist() == want, msg
    finally:
        c.close()


def test_table_pipeline(hal):
    from halo_accumulation_amd import pcdl
    n, m = 1 << 20, 3
    c = hal._lib.Context(urs_n=n)
    try:
        c.set_table_mode(1)  # (the 13-row table of the fixed windows)
        ps, ws = big_members(n, m, 0x7AB1E)
        want = [pcdl.commit(c, ps[i], n - 1, ws[i]).tolist() for i in range(m)]
        rc, got, msg = batch(c, n - 1, ps, m, ws)
        assert rc == 0 and got.tolist() == want, msg
        assert c.info(9) != 0, "the table pipeline ran"
        # one member takes the single call's route, which needs slots 0 and 1: with a caller's MSM there it stays in the pipeline
        import torch
        dev = torch.from_numpy(ps[1].view(np.int64).reshape(-1).copy()).cuda()
        rc, got1, msg = batch(c, n - 1, ps[:1], 1, ws[:1])
        assert rc == 0 and got1.tolist() == want[:1], msg
        c.msm_dev_begin(0, dev.data_ptr(), n)
        try:
            rc, got1, msg = batch(c, n - 1, ps[:1], 1, ws[:1])
        finally:
            res = c.msm_dev_end(0)
        assert rc == 0 and got1.tolist() == want[:1], msg
        assert res.tolist() == pcdl.commit(c, ps[1], n - 1).tolist(), "the caller's MSM on slot 0 kept its own result"
    finally:
        c.close()
