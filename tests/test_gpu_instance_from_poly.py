"""halo_instance_from_poly / halo_instance_from_poly_batch on the GPU: every blob word and the final RNG state against the three
single calls (halo_pcdl_commit, halo_poly_eval over deg + 1 coefficients, halo_pcdl_open) and against the oracle; the batch
against the loop, through every route it can take; the blobs accepted by the check batch and by an accumulation step; a failing
member."""
import ctypes as C

import numpy as np
import pytest

import orc

pytestmark = pytest.mark.gpu

KEY_LG = 10


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


def degree(p):
    nz = np.nonzero(p.any(axis=1))[0]
    return int(nz[-1]) if len(nz) else 0


def three_calls(c, st, p, d, z, w):
    """commit, evaluate, open, pack as a caller of the three single calls does -> (code of the failing call or 0, blob, message)"""
    lg = (d + 1).bit_length() - 1
    p = np.ascontiguousarray(p)
    inst = np.zeros(c.lib.halo_instance_words(lg), dtype=np.uint64)
    Cm = np.zeros(12, dtype=np.uint64)
    v = np.zeros(4, dtype=np.uint64)
    rc = c.lib.halo_pcdl_commit(c.h, ptr(p), len(p), d, ptr(w), ptr(Cm))
    if not rc:
        rc = c.lib.halo_poly_eval(c.h, ptr(p), degree(p) + 1, ptr(z), ptr(v))
    if not rc:
        rc = c.lib.halo_pcdl_open(c.h, C.byref(st), ptr(p), len(p), ptr(Cm), d, ptr(z), ptr(w), ptr(inst[21:]))
    if rc:
        return rc, np.zeros_like(inst), c.lib.halo_last_error().decode()
    inst[:12], inst[12], inst[13:17], inst[17:21] = Cm, d, z, v
    return 0, inst, ""


def members(lg, m, hiding, seed):
    """m seeded polynomials zero-padded to d + 1 = 2^lg coefficients: degrees mixed, member 0 of degree d, member 1 (if any) of
    degree 1; a plain batch also holds the zero polynomial and a constant from member 5 on -> (ps, zs, ws or None)"""
    n = 1 << lg
    ps = np.zeros((m, n, 4), dtype=np.uint64)
    ws, s = orc.rng_scalars(seed, m)
    zs, s = orc.rng_scalars(s, m)
    for i in range(m):
        deg = n - 1 if i == 0 else 1 if i == 1 else 1 + (i * 7919 + lg) % (n - 1)
        if not hiding and i in (5, 6):
            deg = 0
        co, s = orc.rng_scalars(s, deg + 1)
        if not hiding and i == 5:
            co[:] = 0
        ps[i, : deg + 1] = co
    return ps, zs, (ws if hiding else None)


def loop(c, state, d, ps, zs, ws):
    st = C.c_uint64(state)
    out, codes, msgs = [], [], []
    for i in range(len(ps)):
        rc, inst, msg = three_calls(c, st, ps[i], d, zs[i], None if ws is None else ws[i])
        out.append(inst)
        codes.append(rc)
        msgs.append(msg)
    return np.array(out), codes, msgs, st.value


def batch(c, state, d, ps, zs, ws, m=None):
    """one halo_instance_from_poly_batch -> (code, blobs, status list (77: not written), final state, message)"""
    m = len(ps) if m is None else m
    lg = (d + 1).bit_length() - 1
    st = C.c_uint64(state)
    out = np.full((max(m, 1), c.lib.halo_instance_words(lg)), 0xA5, dtype=np.uint64)
    status = (C.c_int * max(m, 1))(*([77] * max(m, 1)))
    rc = c.lib.halo_instance_from_poly_batch(c.h, C.byref(st), d, ptr(None if ps is None else np.ascontiguousarray(ps)), m, ptr(zs), ptr(ws), ptr(out),
                                             status)
    return rc, out[:m], [status[i] for i in range(m)], st.value, c.lib.halo_last_error().decode() if rc else ""


def expect_like_loop(c, state, d, ps, zs, ws):
    want, codes, msgs, st_want = loop(c, state, d, ps, zs, ws)
    rc, got, status, st_got, msg = batch(c, state, d, ps, zs, ws)
    assert status == codes
    bad = [i for i, x in enumerate(codes) if x]
    assert (rc, msg) == ((codes[bad[0]], "member %d: %s" % (bad[0], msgs[bad[0]])) if bad else (0, ""))
    for i in range(len(ps)):
        assert got[i].tolist() == want[i].tolist(), "member %d" % i
    assert st_got == st_want
    return rc, got, status, st_got, msg


# ------------------------------------------------------------------ 1. the single call
@pytest.mark.parametrize("hiding", [False, True])
@pytest.mark.parametrize("lg", [1, 2, 6, 10])
def test_single_call(hal, ctx, pp, lg, hiding):
    from halo_accumulation_amd import acc as A
    d = (1 << lg) - 1
    ps, zs, ws = members(lg, 3, hiding, 0x51E0 + 2 * lg + hiding)
    for i in range(3):
        w = ws[i] if hiding else None
        seed = 0xABCD00 + i
        st = C.c_uint64(seed)
        rc, want, msg = three_calls(ctx, st, ps[i], d, zs[i], w)
        assert rc == 0, msg
        rng = [seed]
        deg = degree(ps[i])
        for p in (ps[i], ps[i][: deg + 1]):  # (zero-padded and exact length: the same blob)
            rng = [seed]
            assert A.instance_from_poly(ctx, rng, p, d, zs[i], w).tolist() == want.tolist(), i
            assert rng[0] == st.value
        co = np.ascontiguousarray(ps[i][: deg + 1])
        Cm = orc.pcdl_commit(pp, co, d, w)
        pi, s = orc.pcdl_open(pp, seed, co, Cm, d, zs[i], w)
        ref = np.concatenate([Cm, np.array([d], dtype=np.uint64), zs[i], orc.poly_eval(co, zs[i]), pi])
        assert want.tolist() == ref.tolist() and s == st.value, "the oracle from the same seed"


def test_single_call_errors(hal, ctx):
    lg = 5
    d = (1 << lg) - 1
    ps, zs, ws = members(lg, 2, True, 0xE44)
    iw = ctx.lib.halo_instance_words(lg)
    E_ARG, E_ASSERT = hal._lib.HALO_E_ARG, hal._lib.HALO_E_ASSERT

    def call(p, length, dd, z=zs[0], w=ws[0], out=True):
        st = C.c_uint64(0x1234)
        inst = np.full(iw, 0xA5, dtype=np.uint64)
        rc = ctx.lib.halo_instance_from_poly(ctx.h, C.byref(st), ptr(p), length, dd, ptr(z), ptr(w), ptr(inst) if out else None)
        return rc, ctx.lib.halo_last_error().decode() if rc else "", st.value, inst

    p = np.ascontiguousarray(ps[0])
    for dd, length, want in ((30, d + 1, "commit: d + 1 is not a power of two"), (15, d + 1, "commit: p.degree() > d"),
                             ((1 << (KEY_LG + 1)) - 1, d + 1, "commit: d > D")):
        rc, msg, st, inst = call(p, length, dd)
        assert (rc, msg, st) == (E_ASSERT, want, 0x1234) and (inst == 0xA5).all()
        assert ctx.lib.halo_pcdl_commit(ctx.h, ptr(p), length, dd, ptr(ws[0]), ptr(np.zeros(12, dtype=np.uint64))) == rc
        assert ctx.lib.halo_last_error().decode() == want, "the first of the three calls reports the same"
    assert call(None, 4, d)[0] == E_ARG and call(p, d + 1, d, z=None)[0] == E_ARG and call(p, d + 1, d, out=False)[0] == E_ARG
    const = np.zeros((d + 1, 4), dtype=np.uint64)
    const[0] = ps[0][0]
    rc, msg, st, _ = call(const, d + 1, d)
    assert (rc, msg, st) == (E_ASSERT, "open: hiding needs p.degree() >= 1", 0x1234), "as halo_pcdl_open: no randomness consumed"
    assert call(const, d + 1, d, w=None)[0] == 0, "a constant opens without hiding"
    assert call(None, 0, d, w=None)[0] == 0, "the empty polynomial is the zero polynomial"


# ------------------------------------------------------------------ 2. the batch against the loop
@pytest.mark.parametrize("hiding", [False, True])
@pytest.mark.parametrize("m", [1, 4, 5, 17])
@pytest.mark.parametrize("lg", [1, 6, 10])
def test_batch_like_the_loop(hal, ctx, lg, m, hiding):
    from halo_accumulation_amd import acc as A, pcdl
    d = (1 << lg) - 1
    seed = 0x1F9B0000 + 64 * lg + 2 * m + hiding
    ps, zs, ws = members(lg, m, hiding, seed)
    rc, got, status, st, _ = expect_like_loop(ctx, seed, d, ps, zs, ws)
    assert rc == 0 and status == [0] * m
    rng = [seed]
    assert [q.tolist() for q in A.instance_from_poly_batch(ctx, rng, list(ps), d, zs, ws)] == got.tolist() and rng[0] == st
    assert pcdl.check_batch(ctx, d, list(got)) == [0] * m


def test_blobs_accumulate(hal, ctx):
    from halo_accumulation_amd import acc as A
    lg, m = 6, 5
    d = (1 << lg) - 1
    ps, zs, ws = members(lg, m, True, 0xACC)
    qs = A.instance_from_poly_batch(ctx, [0xACC], list(ps), d, zs, ws)
    rng = [0xACC1]
    acc = A.prover(ctx, rng, d, qs)
    A.verifier(ctx, d, qs, acc)
    A.decider(ctx, acc)


# ------------------------------------------------------------------ 3. the routes through the loop
@pytest.mark.parametrize("hiding", [False, True])
def test_loop_routes(hal, ctx, hiding):
    lg, m = 6, 9
    d = (1 << lg) - 1
    ps, zs, ws = members(lg, m, hiding, 0x10077 + hiding)
    ref = expect_like_loop(ctx, 0x77, d, ps, zs, ws)
    for name, value in (("open_batch_group", 1), ("open_batch_group", 3), ("batch_stage_fail", 1)):
        hal._lib.dev_hook(name, value)
        try:
            got = batch(ctx, 0x77, d, ps, zs, ws)
            assert (got[0], got[1].tolist(), got[2], got[3]) == (ref[0], ref[1].tolist(), ref[2], ref[3]), (name, value)
        finally:
            hal._lib.dev_hook("reset", 0)
    c = hal._lib.Context(urs_n=1 << KEY_LG)
    try:
        c.set_ipa_switch(1 << (lg - 1))  # (the no-fold size below d + 1: the single call's body, member after member)
        got = batch(c, 0x77, d, ps, zs, ws)
        assert (got[0], got[1].tolist(), got[2], got[3]) == (ref[0], ref[1].tolist(), ref[2], ref[3]), "above the no-fold size"
    finally:
        c.close()


# ------------------------------------------------------------------ 4. a failing member, whole-call errors
def test_failing_member(hal, ctx):
    from halo_accumulation_amd import acc as A
    lg, m = 6, 7
    d = (1 << lg) - 1
    ps, zs, ws = members(lg, m, True, 0xFA11)
    ps[3] = 0
    ps[3][0] = ps[0][0]  # a constant in the middle: hiding needs degree >= 1
    rc, got, status, st, msg = expect_like_loop(ctx, 0xFA11, d, ps, zs, ws)
    E = hal._lib.HALO_E_ASSERT
    assert rc == E and msg == "member 3: open: hiding needs p.degree() >= 1"
    assert status == [0, 0, 0, E, 0, 0, 0] and not got[3].any()
    good = [0, 1, 2, 4, 5, 6]
    want, _, _, st_good = loop(ctx, 0xFA11, d, ps[good], zs[good], ws[good])
    assert got[good].tolist() == want.tolist() and st == st_good, "the members behind it start from the state it left untouched"
    rng = [0xFA11]
    with pytest.raises(AssertionError) as e:
        A.instance_from_poly_batch(ctx, rng, list(ps), d, zs, ws)
    assert e.value.args[1] == status and rng[0] == st
    hal._lib.dev_hook("batch_stage_fail", 1)
    try:
        again = batch(ctx, 0xFA11, d, ps, zs, ws)
        assert (again[0], again[1].tolist(), again[2], again[3], again[4]) == (rc, got.tolist(), status, st, msg), "the loop route"
    finally:
        hal._lib.dev_hook("reset", 0)


def test_whole_call_errors(hal, ctx):
    lg, m = 5, 2
    d = (1 << lg) - 1
    ps, zs, ws = members(lg, m, True, 0xA46)
    E_ARG, E_ASSERT = hal._lib.HALO_E_ARG, hal._lib.HALO_E_ASSERT
    for dd, want in ((30, "commit: d + 1 is not a power of two"), ((1 << (KEY_LG + 1)) - 1, "commit: d > D")):
        st = C.c_uint64(0x1234)
        out = np.full((m, ctx.lib.halo_instance_words(lg)), 0xA5, dtype=np.uint64)
        status = (C.c_int * m)(77, 77)
        rc = ctx.lib.halo_instance_from_poly_batch(ctx.h, C.byref(st), dd, ptr(np.ascontiguousarray(ps)), m, ptr(zs), ptr(ws), ptr(out), status)
        assert (rc, ctx.lib.halo_last_error().decode(), list(status), st.value) == (E_ASSERT, want, [77, 77], 0x1234) and (out == 0xA5).all()
    out = np.full((m, ctx.lib.halo_instance_words(lg)), 0xA5, dtype=np.uint64)
    for k in range(3):
        args = [np.ascontiguousarray(ps), zs, out]
        args[k] = None
        st = C.c_uint64(0x1234)
        status = (C.c_int * m)(77, 77)
        rc = ctx.lib.halo_instance_from_poly_batch(ctx.h, C.byref(st), d, ptr(args[0]), m, ptr(args[1]), ptr(ws), ptr(args[2]), status)
        assert rc == E_ARG and list(status) == [77, 77] and st.value == 0x1234 and (out == 0xA5).all(), k
    rc, _, _, st, _ = batch(ctx, 0x1234, d, None, None, None, m=0)
    assert (rc, st) == (0, 0x1234)
    assert ctx.lib.halo_instance_from_poly_batch(ctx.h, None, d, ptr(np.ascontiguousarray(ps)), m, ptr(zs), ptr(ws), ptr(out), None) == 0, \
        "state and status nullable"
    import torch
    n = 1 << KEY_LG
    sc, _ = orc.rng_scalars(0xC0FFEE, n)
    dev = torch.from_numpy(sc.view(np.int64).reshape(-1).copy()).cuda()
    for slot in range(4):
        ctx.msm_dev_begin(slot, dev.data_ptr(), n)
    try:
        rc, got, status, st, _ = batch(ctx, 0x1234, d, ps, zs, ws)
        assert (rc, status, st) == (E_ARG, [77] * m, 0x1234) and (got == 0xA5).all(), "no idle slot"
    finally:
        for slot in range(4):
            ctx.msm_dev_end(slot)
