"""halo_pcdl_open_batch / halo_random_instance_batch on the GPU: every proof and instance word, every status and the final RNG
state against a loop of the single calls (and the oracle) -- hiding and plain members, the zero polynomial and constants, a
failing member, argument errors, every members-per-launch setting, without staging memory, beside a caller's MSM, at full size,
on a multi-device context -- and no lasting side effects on the context or its clone."""
import ctypes as C

import numpy as np
import pytest

import orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hal():
    import halo_accumulation_amd as h
    return h


@pytest.fixture(scope="module")
def ctx(hal):
    c = hal._lib.Context(urs_n=1 << 14)
    yield c
    c.close()


def ptr(a):
    from halo_accumulation_amd._lib import ptr as p
    return None if a is None else p(a)


def members(c, lg, m, hiding, seed):
    """m seeded polynomials of degree bound d = 2^lg - 1, zero-padded to d + 1: mixed degrees from 1 to d (every fourth at full
    degree); a plain batch also holds the zero polynomial (member 1) and a constant (member 2).  -> (coeffs (m, d + 1, 4), Cs,
    zs, ws or None)"""
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


def loop(c, state, d, ps, Cs, zs, ws):
    """halo_pcdl_open member after member from one state -> (proofs, failing members' zeroed; codes; messages; final state)"""
    lg = (d + 1).bit_length() - 1
    st = C.c_uint64(state)
    out, codes, msgs = [], [], []
    for i in range(len(ps)):
        pf = np.zeros(c.lib.halo_proof_words(lg), dtype=np.uint64)
        rc = c.lib.halo_pcdl_open(c.h, C.byref(st), ptr(ps[i]), d + 1, ptr(Cs[i]), d, ptr(zs[i]), ptr(None if ws is None else ws[i]), ptr(pf))
        codes.append(rc)
        msgs.append(c.lib.halo_last_error().decode() if rc else "")
        out.append(pf if rc == 0 else np.zeros_like(pf))
    return np.array(out), codes, msgs, st.value


def batch(c, state, d, ps, Cs, zs, ws, m=None, lg=None):
    """one halo_pcdl_open_batch -> (code, proofs, status list (77: not written), final state, message)"""
    m = len(ps) if m is None else m
    lg = (d + 1).bit_length() - 1 if lg is None else lg
    st = C.c_uint64(state)
    out = np.zeros((max(m, 1), c.lib.halo_proof_words(lg)), dtype=np.uint64)
    status = (C.c_int * max(m, 1))(*([77] * max(m, 1)))
    rc = c.lib.halo_pcdl_open_batch(c.h, C.byref(st), d, ptr(None if ps is None else np.ascontiguousarray(ps)), m, ptr(Cs), ptr(zs), ptr(ws),
                                    ptr(out), status)
    return rc, out[:m], [status[i] for i in range(m)], st.value, c.lib.halo_last_error().decode()


def same(a, b):
    return (a[0], a[1].tolist(), a[2], a[3]) == (b[0], b[1].tolist(), b[2], b[3])


def expect_like_loop(c, state, d, ps, Cs, zs, ws):
    want, codes, msgs, st_want = loop(c, state, d, ps, Cs, zs, ws)
    got = batch(c, state, d, ps, Cs, zs, ws)
    rc, proofs, status, st_got, msg = got
    assert status == codes
    bad = [i for i, x in enumerate(codes) if x]
    if bad:
        assert rc == codes[bad[0]] and msg == "member %d: %s" % (bad[0], msgs[bad[0]])
    else:
        assert rc == 0
    for i in range(len(ps)):
        assert proofs[i].tolist() == want[i].tolist(), "member %d" % i
    assert st_got == st_want
    return got


# ------------------------------------------------------------------ 1. parity with the loop
@pytest.mark.parametrize("hiding", [False, True])
@pytest.mark.parametrize("m", [1, 3, 8, 9, 33])
@pytest.mark.parametrize("lg", [1, 5, 9, 10, 14])
def test_parity_with_the_loop(hal, ctx, lg, m, hiding):
    d = (1 << lg) - 1
    ps, Cs, zs, ws = members(ctx, lg, m, hiding, 0x0B470000 + 64 * lg + m)
    expect_like_loop(ctx, 0x5EED0000 + 100 * lg + m, d, ps, Cs, zs, ws)


# ------------------------------------------------------------------ 2. the oracle, its RNG state chained from member to member
def test_oracle(hal, ctx):
    lg, m = 10, 3
    d = (1 << lg) - 1
    ps, Cs, zs, ws = members(ctx, lg, m, True, 0x0AC1E)
    rc, got, status, st, _ = batch(ctx, 0xFEED, d, ps, Cs, zs, ws)
    assert rc == 0 and status == [0] * m
    pp = orc.make_pp(ctx.read_bases(0, d + 1))
    s = 0xFEED
    for i in range(m):
        deg = int(np.nonzero(ps[i].any(axis=1))[0][-1])
        ref, s = orc.pcdl_open(pp, s, np.ascontiguousarray(ps[i][: deg + 1]), Cs[i], d, zs[i], ws[i])
        assert got[i].tolist() == ref.tolist(), "member %d" % i
    assert st == s


# ------------------------------------------------------------------ 3. a failing member
def test_failing_member(hal, ctx):
    from halo_accumulation_amd import pcdl
    lg, m = 9, 5
    d = (1 << lg) - 1
    ps, Cs, zs, ws = members(ctx, lg, m, True, 0xFA11)
    ps[2] = 0
    ps[2][0] = ps[0][0]  # a constant: hiding needs degree >= 1
    rc, got, status, st, msg = expect_like_loop(ctx, 0xFA11, d, ps, Cs, zs, ws)
    assert rc == hal._lib.HALO_E_ASSERT and msg == "member 2: open: hiding needs p.degree() >= 1"
    assert status == [0, 0, hal._lib.HALO_E_ASSERT, 0, 0] and not got[2].any()
    rng = [0xFA11]
    with pytest.raises(AssertionError) as e:
        pcdl.open_batch(ctx, rng, list(ps), Cs, d, zs, ws)
    assert e.value.args[1] == status and rng[0] == st
    good = [0, 1, 3, 4]
    want, _, _, st_good = loop(ctx, 0xFA11, d, ps[good], Cs[good], zs[good], ws[good])
    rng = [0xFA11]
    pis = pcdl.open_batch(ctx, rng, [ps[i] for i in good], Cs[good], d, zs[good], ws[good])
    assert [p.tolist() for p in pis] == want.tolist() and rng[0] == st_good


# ------------------------------------------------------------------ 4. argument errors
def test_argument_errors(hal, ctx):
    lg = 5
    d = (1 << lg) - 1
    ps, Cs, zs, ws = members(ctx, lg, 2, True, 0xA46)
    for dd, want in ((30, "open: d + 1 is not a power of two"), ((1 << 15) - 1, "open: d > D")):
        rc, _, status, st, msg = batch(ctx, 0x1234, dd, ps, Cs, zs, ws, lg=lg)
        assert (rc, msg, status, st) == (hal._lib.HALO_E_ASSERT, want, [77, 77], 0x1234)
        single = C.c_uint64(0x1234)
        pf = np.zeros(ctx.lib.halo_proof_words(lg), dtype=np.uint64)
        assert ctx.lib.halo_pcdl_open(ctx.h, C.byref(single), ptr(ps[0]), 1, ptr(Cs[0]), dd, ptr(zs[0]), ptr(ws[0]), ptr(pf)) == rc
        assert ctx.lib.halo_last_error().decode() == want
    out = np.zeros((2, ctx.lib.halo_proof_words(lg)), dtype=np.uint64)
    for k in range(4):
        args = [ps, Cs, zs]
        if k < 3:
            args[k] = None
        st = C.c_uint64(0x1234)
        status = (C.c_int * 2)(77, 77)
        rc = ctx.lib.halo_pcdl_open_batch(ctx.h, C.byref(st), d, ptr(None if args[0] is None else np.ascontiguousarray(args[0])), 2, ptr(args[1]),
                                          ptr(args[2]), ptr(ws), None if k == 3 else ptr(out), status)
        assert rc == hal._lib.HALO_E_ARG and list(status) == [77, 77] and st.value == 0x1234, k
    rc, _, status, st, _ = batch(ctx, 0x1234, d, None, None, None, None, m=0)
    assert (rc, st) == (0, 0x1234)
    assert ctx.lib.halo_pcdl_open_batch(ctx.h, None, d, ptr(ps), 2, ptr(Cs), ptr(zs), ptr(ws), ptr(out), None) == 0, "state and status nullable"
    inst = np.zeros((2, ctx.lib.halo_instance_words(lg)), dtype=np.uint64)
    for dd, want in ((1, "random_instance: bad d"), (30, "random_instance: bad d"), ((1 << 15) - 1, "random_instance: d > D")):
        st = C.c_uint64(0x1234)
        assert ctx.lib.halo_random_instance_batch(ctx.h, C.byref(st), dd, 2, ptr(inst)) == hal._lib.HALO_E_ASSERT
        assert ctx.lib.halo_last_error().decode() == want and st.value == 0x1234
    assert ctx.lib.halo_random_instance_batch(ctx.h, C.byref(st), d, 2, None) == hal._lib.HALO_E_ARG
    assert ctx.lib.halo_random_instance_batch(ctx.h, C.byref(st), d, 0, None) == 0 and st.value == 0x1234


# ------------------------------------------------------------------ 5. random_instance
def random_instances_loop(c, state, d, m):
    lg = (d + 1).bit_length() - 1
    st = C.c_uint64(state)
    out = np.zeros((m, c.lib.halo_instance_words(lg)), dtype=np.uint64)
    for i in range(m):
        assert c.lib.halo_random_instance(c.h, C.byref(st), d, ptr(out[i])) == 0
    return out, st.value


@pytest.mark.parametrize("m", [1, 7, 40])
@pytest.mark.parametrize("lg", [3, 10, 14])
def test_random_instance_batch(hal, ctx, lg, m):
    from halo_accumulation_amd import acc as A, pcdl
    d = (1 << lg) - 1
    seed = 0x4A4D0000 + 64 * lg + m
    want, st_want = random_instances_loop(ctx, seed, d, m)
    got = np.zeros_like(want)
    st = C.c_uint64(seed)
    assert ctx.lib.halo_random_instance_batch(ctx.h, C.byref(st), d, m, ptr(got)) == 0, ctx.lib.halo_last_error()
    assert got.tolist() == want.tolist() and st.value == st_want
    rng = [seed]
    assert [q.tolist() for q in A.random_instance_batch(ctx, rng, d, m)] == want.tolist() and rng[0] == st_want
    assert pcdl.check_batch(ctx, d, list(got)) == [0] * m


# ------------------------------------------------------------------ 6. members per launch, staging refused, no memory budget
def test_members_per_launch_and_staging(hal):
    lg, m = 9, 9
    d = (1 << lg) - 1
    c = hal._lib.Context(urs_n=1 << 12)
    try:
        ps, Cs, zs, ws = members(c, lg, m, True, 0x6E0)
        ref = expect_like_loop(c, 77, d, ps, Cs, zs, ws)
        inst, st_inst = random_instances_loop(c, 78, d, 6)
        for name, value in (("open_batch_group", 1), ("open_batch_group", 2), ("open_batch_group", 4), ("batch_stage_fail", 1)):
            hal._lib.dev_hook(name, value)
            try:
                assert same(batch(c, 77, d, ps, Cs, zs, ws), ref), (name, value)
                got = np.zeros_like(inst)
                st = C.c_uint64(78)
                assert c.lib.halo_random_instance_batch(c.h, C.byref(st), d, 6, ptr(got)) == 0
                assert got.tolist() == inst.tolist() and st.value == st_inst, (name, value)
            finally:
                hal._lib.dev_hook("reset", 0)
    finally:
        c.close()
    c = hal._lib.Context(urs_n=1 << 12)  # (a fresh context: no staging grown before the budget goes to zero)
    budget = c.info(3)
    try:
        c.set_memory_budget(0)
        before = c.info(4)
        assert same(batch(c, 77, d, ps, Cs, zs, ws), ref)
        assert c.info(4) <= before, "no optional memory under a zero budget"
    finally:
        c.set_memory_budget(budget)
        c.close()


# ------------------------------------------------------------------ 7. slots
def test_beside_a_callers_msm(hal, ctx):
    import torch
    lg, m = 10, 9
    d = (1 << lg) - 1
    ps, Cs, zs, ws = members(ctx, lg, m, True, 0x5107)
    want = loop(ctx, 0x51, d, ps, Cs, zs, ws)
    n = 1 << 14
    sc, _ = orc.rng_scalars(0xC0FFEE, n)
    dev = torch.from_numpy(sc.view(np.int64).reshape(-1).copy()).cuda()
    gs = ctx.read_bases()
    ctx.msm_dev_begin(3, dev.data_ptr(), n)
    try:
        rc, got, status, st, _ = batch(ctx, 0x51, d, ps, Cs, zs, ws)
    finally:
        res = ctx.msm_dev_end(3)
    assert res.tolist() == orc.msm_affine(gs, sc).tolist(), "the caller's MSM on slot 3 kept its own result"
    assert rc == 0 and got.tolist() == want[0].tolist() and st == want[3]
    for slot in range(4):
        ctx.msm_dev_begin(slot, dev.data_ptr(), n)
    try:
        rc, _, status, st, _ = batch(ctx, 0x51, d, ps, Cs, zs, ws)
        assert (rc, status, st) == (hal._lib.HALO_E_ARG, [77] * m, 0x51), "no idle slot"
    finally:
        for slot in range(4):
            assert ctx.msm_dev_end(slot).tolist() == res.tolist()


# ------------------------------------------------------------------ 8. full size, and the device path over a larger key
def test_full_size(hal):
    c = hal._lib.Context(urs_n=1 << 20)
    try:
        ps, Cs, zs, ws = members(c, 20, 3, True, 0xB16)
        expect_like_loop(c, 0xB16, (1 << 20) - 1, ps, Cs, zs, ws)
        ps, Cs, zs, ws = members(c, 14, 9, True, 0xB17)
        expect_like_loop(c, 0xB17, (1 << 14) - 1, ps, Cs, zs, ws)
    finally:
        c.close()


# ------------------------------------------------------------------ 9. no lasting side effects; a multi-device context
def test_no_lasting_side_effects(hal, ctx):
    from halo_accumulation_amd import pcdl
    lg = 12
    d = (1 << lg) - 1
    ps, Cs, zs, ws = members(ctx, lg, 5, True, 0x51DE)
    cl = ctx.clone()
    try:
        before = [pcdl.open(x, [9], ps[1], Cs[1], d, zs[1], ws[1]).tolist() for x in (ctx, cl)]
        for x in (ctx, cl):
            assert batch(x, 9, d, ps, Cs, zs, ws)[0] == 0
        assert [pcdl.open(x, [9], ps[1], Cs[1], d, zs[1], ws[1]).tolist() for x in (ctx, cl)] == before
    finally:
        cl.close()


def test_multi_device_context(hal, ctx):
    lg, m = 10, 6
    d = (1 << lg) - 1
    ps, Cs, zs, ws = members(ctx, lg, m, True, 0x3D)
    want = batch(ctx, 5, d, ps, Cs, zs, ws)
    mc = hal._lib.Context(urs_n=1 << 14, devices=[0, 0])
    try:
        assert same(expect_like_loop(mc, 5, d, ps, Cs, zs, ws), want)
    finally:
        mc.close()
