"""halo_pcdl_check_batch / halo_acc_decider_batch on the GPU: the batched h expansion (k_h_tables + k_h_coeffs_batch) bit for
bit against halo_h_coeffs and the oracle, and every member's status code for code against the single halo_pcdl_check /
halo_acc_decider -- with hiding, plain, tampered and foreign-key members, across the 64-member device path of the succinct half,
at full size, beside a caller's MSM in flight, without staging memory and on a multi-device context."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

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


@pytest.fixture(scope="module")
def big(hal):
    c = hal._lib.Context(urs_n=1 << 20)
    yield c
    c.close()


def ptr(a):
    from halo_accumulation_amd._lib import ptr as p
    return p(a)


def batch(c, d, blobs, acc=False, m=None):
    """-> (return code, status list, message); status entries the call does not write stay 77"""
    m = len(blobs) if m is None else m
    qs = np.ascontiguousarray(np.concatenate(blobs)) if len(blobs) else np.zeros(1, dtype=np.uint64)
    st = (C.c_int * max(m, 1))(*([77] * max(m, 1)))
    fn = c.lib.halo_acc_decider_batch if acc else c.lib.halo_pcdl_check_batch
    rc = fn(c.h, d, ptr(qs), m, st)
    return rc, [st[i] for i in range(m)], c.lib.halo_last_error().decode()


def single(c, d, blob, acc=False):
    """-> (code, message) of the one-member call"""
    if acc:
        rc = c.lib.halo_acc_decider(c.h, ptr(blob))
    else:
        rc = c.lib.halo_pcdl_check(c.h, ptr(blob[0:12].copy()), d, ptr(blob[13:17].copy()), ptr(blob[17:21].copy()), ptr(blob[21:].copy()))
    return rc, c.lib.halo_last_error().decode()


def expect_like_singles(c, d, blobs, acc=False):
    rc, st, msg = batch(c, d, blobs, acc)
    singles = [single(c, d, b, acc) for b in blobs]
    assert st == [s[0] for s in singles]
    bad = [i for i, s in enumerate(singles) if s[0]]
    if bad:
        assert rc == singles[bad[0]][0] and msg == "instance %d: %s" % (bad[0], singles[bad[0]][1])
    else:
        assert rc == 0
    return st


def plain_instance(c, seed, d):
    from halo_accumulation_amd import pcdl
    coeffs, s = orc.rng_scalars(seed, d + 1 - (seed % 3))
    z, _ = orc.rng_scalars(s, 1)
    Cm = pcdl.commit(c, coeffs, d)
    pi = pcdl.open(c, [seed], coeffs, Cm, d, z[0])
    v = c.poly_eval(coeffs, z[0])
    return np.concatenate([Cm, np.array([d], dtype=np.uint64), z[0], v, pi])


def tamper(q, lg, what):
    q = q.copy()
    off = {"U": 21 + 2 + 24 * lg, "c": 21 + 2 + 24 * lg + 12, "L": 21 + 2, "v": 17, "C": 0}[what]
    q[off] ^= 1
    return q


# ------------------------------------------------------------------ 1. the batched h expansion
@pytest.mark.parametrize("lg", [1, 3, 8, 9, 16, 17, 20])
@pytest.mark.parametrize("m", [1, 5, 64])
def test_h_coeffs_batch_equals_single_expansion(hal, ctx, big, lg, m):
    if lg == 20 and m == 64:
        m = 8  # (64 x 32 MiB would be 2 GiB of output for no more coverage)
    c = ctx if lg <= 14 else big
    xis, _ = orc.rng_scalars(7000 + 100 * lg + m, m * (lg + 1))
    xis = np.ascontiguousarray(xis.reshape(m, lg + 1, 4))
    out = np.zeros((m, 1 << lg, 4), dtype=np.uint64)
    assert c.lib.halo_dev_h_coeffs_batch(c.h, ptr(xis), m, lg, ptr(out)) == 0, c.lib.halo_last_error()
    for b in range(m):
        xb = np.ascontiguousarray(xis[b])
        assert out[b].tolist() == c.h_coeffs(xb).tolist(), "member %d" % b
        if lg <= 9:
            assert out[b].tolist() == orc.h_coeffs(xb).tolist(), "member %d vs the oracle" % b


# ------------------------------------------------------------------ 2. argument errors
def test_argument_errors(hal, ctx):
    from halo_accumulation_amd import acc as A
    d = 511
    q = A.random_instance(ctx, [5], d)
    st = (C.c_int * 2)(77, 77)
    assert ctx.lib.halo_pcdl_check_batch(ctx.h, d, None, 2, st) == hal._lib.HALO_E_ARG
    assert ctx.lib.halo_acc_decider_batch(ctx.h, d, None, 2, st) == hal._lib.HALO_E_ARG
    other = q.copy()
    other[12] = 255
    rc, s, msg = batch(ctx, d, [q, other])
    assert rc == hal._lib.HALO_E_REJECT and "d_i != d" in msg and s == [77, 77], "rejected before any work, status untouched"
    rc, s, msg = batch(ctx, 510, [q])
    assert rc == hal._lib.HALO_E_REJECT and s == [77]
    assert batch(ctx, d, [], m=0)[0] == 0
    assert ctx.lib.halo_pcdl_check_batch(ctx.h, d, None, 0, None) == 0
    assert ctx.lib.halo_pcdl_check_batch(ctx.h, d, ptr(q), 1, None) == 0, "status is nullable"


# ------------------------------------------------------------------ 3. parity with the single check
_POOLS = {}


def pool(hal, ctx, lg):
    """70 members: hiding instances from random_instance, every seventh plain, five tampered ones (U, c, L, v, C) and two from
    another key (their succinct half holds; only the MSM of pcdl.rs:338 tells them apart)"""
    if lg in _POOLS:
        return _POOLS[lg]
    from halo_accumulation_amd import acc as A
    d = (1 << lg) - 1
    rng = [0x5EED0000 + lg]
    qs = [plain_instance(ctx, 40 + i, d) if i % 7 == 3 else A.random_instance(ctx, rng, d) for i in range(70)]
    for i, what in zip((2, 10, 30, 50, 66), ("U", "c", "L", "v", "C")):
        qs[i] = tamper(qs[i], lg, what)
    other = hal._lib.Context(urs_n=1 << 14, first_index=1 << 30)
    try:
        for i in (6, 64):
            qs[i] = A.random_instance(other, [900 + i], d)
    finally:
        other.close()
    _POOLS[lg] = qs
    return qs


@pytest.mark.parametrize("lg", [3, 9, 12, 14])
@pytest.mark.parametrize("m", [1, 8, 9, 33, 70])
def test_check_batch_matches_single_checks(hal, ctx, lg, m):
    d = (1 << lg) - 1
    qs = pool(hal, ctx, lg)
    members = qs[:m] if m != 1 else [qs[6]]  # (m = 1: the foreign-key member alone)
    st = expect_like_singles(ctx, d, members)
    if m == 70:
        assert [i for i, s in enumerate(st) if s] == [2, 6, 10, 30, 50, 64, 66]
    if m >= 33 and lg in (3, 9):
        pp = orc.make_pp(ctx.read_bases(0, 1 << lg))
        for i in (0, 3, 4, 10):
            q = members[i]
            if st[i]:
                with pytest.raises(ValueError):
                    orc.pcdl_check(pp, q[0:12].copy(), d, q[13:17].copy(), q[17:21].copy(), q[21:].copy())
            else:
                orc.pcdl_check(pp, q[0:12].copy(), d, q[13:17].copy(), q[17:21].copy(), q[21:].copy())


def test_check_batch_on_the_host_pool_path(hal, ctx):
    """70 members with the device relations switched off: the same codes"""
    d = (1 << 9) - 1
    qs = pool(hal, ctx, 9)
    ctx.set_batch_verify(False)
    try:
        expect_like_singles(ctx, d, qs)
    finally:
        ctx.set_batch_verify(True)


# ------------------------------------------------------------------ 4. full size from the 2^20 fixture's seeds
def test_full_size_from_fixture_seeds(hal, big):
    from halo_accumulation_amd import acc as A, pcdl
    with open(os.path.join(ROOT, "tests", "golden", "open_2_20.json")) as f:
        fx = json.load(f)
    lg = fx["lg_n"]
    d = (1 << lg) - 1
    coeffs, s = orc.rng_scalars(fx["coeff_seed"], fx["deg"] + 1)
    zw, _ = orc.rng_scalars(s, 2)
    v = big.poly_eval(coeffs, zw[0])
    inst = []
    for name in ("plain", "hiding"):
        case = fx["cases"][name]
        w = zw[1] if case["hiding"] else None
        Cm = pcdl.commit(big, coeffs, d, w)
        pi = pcdl.open(big, [fx["open_seed"]], coeffs, Cm, d, zw[0], w)
        assert hashlib.sha256(pi.tobytes()).hexdigest() == case["proof_sha256"], name
        inst.append(np.concatenate([Cm, np.array([d], dtype=np.uint64), zw[0], v, pi]))
    members = [inst[0], inst[1], tamper(inst[0], lg, "v"), tamper(inst[1], lg, "U")]
    rc, st, msg = batch(big, d, members)
    assert st == [0, 0, hal._lib.HALO_E_REJECT, hal._lib.HALO_E_REJECT] and rc == hal._lib.HALO_E_REJECT and msg.startswith("instance 2: ")
    a = fx["acc"]
    qs = [A.random_instance(big, [int(a["q_seeds"][k], 16)], d) for k in range(2)]
    for k in range(2):
        assert hashlib.sha256(qs[k].tobytes()).hexdigest() == a["q_sha256"][k]
    acc = A.prover(big, [int(a["acc_seed"], 16)], d, qs)
    assert hashlib.sha256(acc.tobytes()).hexdigest() == a["acc_sha256"]
    bad = acc.copy()
    bad[17] ^= 1
    rc, st, msg = batch(big, d, [bad, acc], acc=True)
    assert st == [hal._lib.HALO_E_REJECT, 0] and msg.startswith("instance 0: ")


# ------------------------------------------------------------------ 5. the decider over acc_compare chains
def chain(ctx, lg, k):
    from halo_accumulation_amd import acc as A
    d = (1 << lg) - 1
    rng = [0xACC0000 + lg]
    accs, acc = [], None
    for _ in range(k):
        q = A.random_instance(ctx, rng, d)
        qs = [q] if acc is None else [A.instance_from_accumulator(ctx, acc, d), q]
        acc = A.prover(ctx, rng, d, qs)
        accs.append(acc)
    return accs


@pytest.mark.parametrize("lg", [9, 14])
def test_decider_batch_over_a_chain(hal, ctx, lg):
    from halo_accumulation_amd import acc as A
    d = (1 << lg) - 1
    accs = chain(ctx, lg, 10)
    assert A.decider_batch(ctx, d, accs) == [0] * 10
    assert expect_like_singles(ctx, d, accs, acc=True) == [0] * 10
    bad = list(accs)
    bad[3] = accs[3].copy(); bad[3][0] ^= 1     # C_bar
    bad[7] = accs[7].copy(); bad[7][17] ^= 1    # v
    st = expect_like_singles(ctx, d, bad, acc=True)
    assert [i for i, s in enumerate(st) if s] == [3, 7]
    with pytest.raises(hal._lib.HaloReject):
        A.decider_batch(ctx, d, bad)
    if lg == 9:
        pp = orc.make_pp(ctx.read_bases(0, 1 << lg))
        for i in (0, 9):
            orc.acc_decider(pp, accs[i])
        with pytest.raises(ValueError):
            orc.acc_decider(pp, bad[7])


# ------------------------------------------------------------------ 6. slots and launch graphs
def test_beside_a_callers_msm_and_repeated(hal, ctx):
    import torch
    d = (1 << 12) - 1
    qs = pool(hal, ctx, 12)[:20]
    want = [single(ctx, d, q)[0] for q in qs]
    n = 1 << 14
    sc, _ = orc.rng_scalars(0xC0FFEE, n)
    dev = torch.from_numpy(sc.view(np.int64).reshape(-1).copy()).cuda()
    gs = ctx.read_bases()
    ctx.msm_dev_begin(1, dev.data_ptr(), n)
    try:
        assert batch(ctx, d, qs)[1] == want
    finally:
        got = ctx.msm_dev_end(1)
    assert got.tolist() == orc.msm_affine(gs, sc).tolist(), "the caller's MSM on slot 1 kept its own result"
    first = batch(ctx, d, qs)
    assert first[1] == want and batch(ctx, d, qs) == first, "two calls in a row (the second replays its launch graphs)"
    assert ctx.msm(sc).tolist() == orc.msm_affine(gs, sc).tolist()
    for slot in range(4):
        ctx.msm_dev_begin(slot, dev.data_ptr(), n)
    try:
        assert batch(ctx, d, qs)[0] == hal._lib.HALO_E_ARG, "no idle slot"
    finally:
        for slot in range(4):
            assert ctx.msm_dev_end(slot).tolist() == got.tolist()


# ------------------------------------------------------------------ 7. without staging memory
def test_staging_fallback(hal):
    c = hal._lib.Context(urs_n=1 << 12)
    try:
        d = (1 << 10) - 1
        from halo_accumulation_amd import acc as A
        rng = [77]
        qs = [A.random_instance(c, rng, d) for _ in range(12)]
        qs[5] = tamper(qs[5], 10, "U")
        want = [single(c, d, q)[0] for q in qs]
        hal._lib.dev_hook("batch_stage_fail", 1)
        try:
            r_hook = batch(c, d, qs)
        finally:
            hal._lib.dev_hook("reset", 0)
        assert r_hook[1] == want and r_hook[0] == hal._lib.HALO_E_REJECT
        budget = c.info(3)
        c.set_memory_budget(0)
        try:
            before = c.info(4)
            r0 = batch(c, d, qs)
            assert c.info(4) <= before, "no optional memory under a zero budget"
        finally:
            c.set_memory_budget(budget)
        assert r0 == r_hook
        assert batch(c, d, qs) == r_hook, "with staging"
    finally:
        c.close()


# ------------------------------------------------------------------ 8. multi-device context
def test_multi_device_context(hal, ctx):
    d = (1 << 12) - 1
    qs = pool(hal, ctx, 12)[:20]
    want = batch(ctx, d, qs)
    m = hal._lib.Context(urs_n=1 << 14, devices=[0, 0])
    try:
        assert batch(m, d, qs) == want
    finally:
        m.close()
