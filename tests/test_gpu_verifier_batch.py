"""halo_acc_verifier_batch on the GPU: the segmented small MSM (k_small_msm_seg) against the oracle's MSM, and every member's
status code for code against the single halo_acc_verifier -- over acc_compare chains, with one member tampered at every check
position, with 0, 1, 2 and 64 instances per member, in both forms (device launch and host pool), at full size, beside a caller's
MSM in flight, without staging memory and on a multi-device context."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 0x40000000000000000000000000000000224698fc0994a8dd8c46eb2100000001

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


def lg_of(d):
    return (d + 1).bit_length() - 1


def vbatch(c, d, members):
    """members: [(instances, acc)] -> (return code, status list, message); status entries the call does not write stay 77"""
    k = len(members)
    qs = [q for m in members for q in m[0]]
    blob = np.ascontiguousarray(np.concatenate(qs)) if qs else np.zeros(1, dtype=np.uint64)
    accs = np.ascontiguousarray(np.concatenate([m[1] for m in members])) if k else np.zeros(1, dtype=np.uint64)
    counts = (C.c_size_t * max(k, 1))(*[len(m[0]) for m in members])
    st = (C.c_int * max(k, 1))(*([77] * max(k, 1)))
    rc = c.lib.halo_acc_verifier_batch(c.h, d, ptr(blob), counts, k, ptr(accs), st)
    return rc, [st[i] for i in range(k)], c.lib.halo_last_error().decode()


def vsingle(c, d, member):
    qs, acc = member
    blob = np.ascontiguousarray(np.concatenate(qs)) if qs else np.zeros(1, dtype=np.uint64)
    rc = c.lib.halo_acc_verifier(c.h, d, ptr(blob), len(qs), ptr(np.ascontiguousarray(acc)))
    return rc, c.lib.halo_last_error().decode()


def expect_like_singles(c, d, members):
    rc, st, msg = vbatch(c, d, members)
    singles = [vsingle(c, d, m) for m in members]
    assert st == [s[0] for s in singles]
    bad = [j for j, s in enumerate(singles) if s[0]]
    if bad:
        assert rc == singles[bad[0]][0] and msg == "member %d: %s" % (bad[0], singles[bad[0]][1])
    else:
        assert rc == 0
    return st, msg


# ------------------------------------------------------------------ 1. the segmented small MSM
def test_small_msm_seg_matches_the_oracle(hal, ctx):
    lens = [1, 2, 3, 4, 5, 17, 32, 33, 64, 64, 3, 1, 5, 33, 17, 2]
    total = sum(lens)
    pts = np.ascontiguousarray(ctx.read_bases(0, total))
    rng = np.random.default_rng(1234)
    ks = [int.from_bytes(rng.bytes(32), "little") % R for _ in range(total)]
    special = [0, 1, R - 1]
    for t in range(0, total, 7):
        ks[t] = special[(t // 7) % 3]
    for t in range(3, total, 11):
        pts[t] = 0  # infinity
    sc = np.zeros((total, 4), dtype=np.uint64)
    for t, k in enumerate(ks):
        for w in range(4):
            sc[t, w] = (k >> (64 * w)) & 0xFFFFFFFFFFFFFFFF
    out = np.zeros((len(lens), 12), dtype=np.uint64)
    cl = (C.c_size_t * len(lens))(*lens)
    assert ctx.lib.halo_dev_small_msm_seg(ctx.h, ptr(pts), ptr(sc), cl, len(lens), ptr(out)) == 0, ctx.lib.halo_last_error()
    at = 0
    for s, n in enumerate(lens):
        keep = [t for t in range(at, at + n) if pts[t].any()]
        if keep:
            want = orc.msm_affine(np.ascontiguousarray(pts[keep]), orc.scalars_to_mont([ks[t] for t in keep]))
        else:
            want = np.array([1, 0, 0, 0] * 2 + [0] * 4, dtype=np.uint64)
        assert orc.point_canonical(out[s]) == orc.point_canonical(want), "sum %d of %d terms" % (s, n)
        at += n
    cl = (C.c_size_t * 1)(65)
    assert ctx.lib.halo_dev_small_msm_seg(ctx.h, ptr(pts), ptr(sc), cl, 1, ptr(out)) == hal._lib.HALO_E_ARG


# ------------------------------------------------------------------ chains (acc_compare, benches/acc.rs:76-98)
_CHAINS = {}


def chain(hal, c, lg, k):
    """[(instances, acc)] of one acc_compare chain: step 0 verifies one instance, every later step the previous accumulator's
    Instance and a fresh one"""
    key = (id(c), lg)
    have = _CHAINS.get(key, [])
    if len(have) >= k:
        return have[:k]
    from halo_accumulation_amd import acc as A
    d = (1 << lg) - 1
    rng = [0xACCF0000 + lg + 17 * len(have)]
    prev = have[-1][1] if have else None
    for _ in range(k - len(have)):
        q = A.random_instance(c, rng, d)
        qs = [q] if prev is None else [A.instance_from_accumulator(c, prev, d), q]
        prev = A.prover(c, rng, d, qs)
        have.append((qs, prev))
    _CHAINS[key] = have
    return have[:k]


def tampered(member, lg, what, other=None):
    """one member broken at one check position of acc::verifier (acc.rs:223-243)"""
    qs, acc = [q.copy() for q in member[0]], member[1].copy()
    d = (1 << lg) - 1
    iw = 21 + 2 + 24 * lg + 32
    pf = 21 + 2 + 24 * lg  # U of a proof
    if what == "C_bar_offcurve":
        acc[0] ^= 1
    elif what == "h0":
        acc[iw] ^= 1
    elif what == "d_i":
        qs[-1][12] = d - 1
    elif what == "L":  # the first round's L that is not the point at infinity (any X of Z = 0 is on the curve)
        off = next(23 + 12 * i for i in range(lg) if qs[-1][23 + 12 * i + 8: 23 + 12 * i + 12].any())
        qs[-1][off] ^= 1
    elif what == "U":
        qs[0][pf] ^= 1
    elif what == "c":
        qs[-1][pf + 12] ^= 1
    elif what == "v":
        qs[0][17] ^= 1
    elif what == "hiding_C_bar":
        assert qs[-1][21] == 1
        qs[-1][pf + 16] ^= 1
    elif what == "foreign_acc":
        acc = other.copy()
    elif what == "z":
        acc[13] ^= 1
    elif what == "acc_d":
        acc[12] = d - 1
    elif what == "acc_v":
        acc[17] ^= 1
    else:
        raise ValueError(what)
    return qs, acc


KINDS = ["C_bar_offcurve", "h0", "d_i", "L", "U", "c", "v", "hiding_C_bar", "foreign_acc", "z", "acc_d", "acc_v"]


def with_tampers(members, lg, step):
    out = list(members)
    for n, what in enumerate(KINDS):
        j = 1 + n * step
        if j >= len(out):
            break
        out[j] = tampered(out[j], lg, what, other=members[j - 1][1])
    return out


# ------------------------------------------------------------------ 2. argument errors
def test_argument_errors(hal, ctx):
    d = (1 << 9) - 1
    members = chain(hal, ctx, 9, 2)
    E_ARG, E_REJECT, E_ASSERT = hal._lib.HALO_E_ARG, hal._lib.HALO_E_REJECT, hal._lib.HALO_E_ASSERT
    counts = (C.c_size_t * 2)(1, 2)
    st = (C.c_int * 2)(77, 77)
    acc = np.ascontiguousarray(np.concatenate([m[1] for m in members]))
    qs = np.ascontiguousarray(np.concatenate([q for m in members for q in m[0]]))
    lib = ctx.lib
    assert lib.halo_acc_verifier_batch(None, d, ptr(qs), counts, 2, ptr(acc), st) == E_ARG and b"null context" in lib.halo_last_error()
    assert lib.halo_acc_verifier_batch(ctx.h, d, ptr(qs), counts, 2, None, st) == E_ARG
    assert lib.halo_acc_verifier_batch(ctx.h, d, ptr(qs), None, 2, ptr(acc), st) == E_ARG
    assert lib.halo_acc_verifier_batch(ctx.h, d, None, counts, 2, ptr(acc), st) == E_ARG
    assert lib.halo_acc_verifier_batch(ctx.h, d - 1, ptr(qs), counts, 2, ptr(acc), st) == E_REJECT
    assert lib.halo_last_error() == b"d+1 is not a power of 2!"
    huge = (1 << 15) - 1
    assert lib.halo_acc_verifier_batch(ctx.h, huge, ptr(qs), counts, 2, ptr(acc), st) == E_ASSERT
    assert lib.halo_last_error() == b"commit: d > D"
    assert list(st) == [77, 77], "whole-call errors leave status untouched"
    assert lib.halo_acc_verifier_batch(ctx.h, d, None, None, 0, None, st) == 0 and list(st) == [77, 77]
    assert lib.halo_acc_verifier_batch(ctx.h, d, ptr(qs), counts, 2, ptr(acc), None) == 0, "status is nullable"
    zero = (C.c_size_t * 1)(0)
    assert lib.halo_acc_verifier_batch(ctx.h, d, None, zero, 1, ptr(np.ascontiguousarray(members[0][1])), st) == vsingle(ctx, d, ([], members[0][1]))[0]
    from halo_accumulation_amd import acc as A
    assert A.verifier_batch(ctx, d, [m[0] for m in members], [m[1] for m in members]) == [0, 0]
    with pytest.raises(hal._lib.HaloReject):
        A.verifier_batch(ctx, d, [members[1][0], members[0][0]], [members[0][1], members[1][1]])


# ------------------------------------------------------------------ 3. parity with the single verifier over chains
@pytest.mark.parametrize("lg", [3, 9, 12, 14])
@pytest.mark.parametrize("k", [1, 10, 33, 100])
def test_matches_single_verifiers(hal, ctx, lg, k):
    d = (1 << lg) - 1
    members = chain(hal, ctx, lg, k)
    assert expect_like_singles(ctx, d, members)[0] == [0] * k
    if k == 1:
        bad = [tampered(members[0], lg, "v")]
    else:
        bad = with_tampers(members, lg, 1 if k <= 33 else 8)
    st, _ = expect_like_singles(ctx, d, bad)
    broken = [j for j in range(k) if bad[j][1] is not members[j][1] or any(a is not b for a, b in zip(bad[j][0], members[j][0]))]
    assert [j for j, s in enumerate(st) if s] == broken
    if lg in (3, 9) and k >= 10:
        pp = orc.make_pp(ctx.read_bases(0, 1 << lg))
        for j in (0, 1, 2, 5, 9):
            if st[j]:
                with pytest.raises(ValueError):
                    orc.acc_verifier(pp, d, bad[j][0], bad[j][1])
            else:
                orc.acc_verifier(pp, d, bad[j][0], bad[j][1])


@pytest.mark.parametrize("lg", [9, 12])
def test_instances_per_member(hal, ctx, lg):
    """0, 1, 2 and 64 instances per member (64: the single call's own device form of the succinct half)"""
    from halo_accumulation_amd import acc as A
    d = (1 << lg) - 1
    rng = [0x64640000 + lg]
    qs64 = A.random_instance_batch(ctx, rng, d, 64)
    m0 = ([], A.prover(ctx, rng, d, []))
    m64 = (qs64, A.prover(ctx, rng, d, qs64))
    c = chain(hal, ctx, lg, 3)
    members = [m0, c[0], c[1], m64, c[2], m0]
    assert expect_like_singles(ctx, d, members)[0] == [0] * 6
    bad = list(members)
    bad[3] = tampered(m64, lg, "c")
    bad[4] = tampered(c[2], lg, "acc_v")
    bad[5] = tampered(m0, lg, "h0")
    st, _ = expect_like_singles(ctx, d, bad)
    assert [j for j, s in enumerate(st) if s] == [3, 4, 5]
    q_late = list(qs64)
    q_late[40] = tampered(([qs64[40]], m64[1]), lg, "v")[0][0]
    q_late[50] = tampered(([qs64[50]], m64[1]), lg, "L")[0][0]
    st, msg = expect_like_singles(ctx, d, [c[0], (q_late, m64[1])])
    assert st[1] == hal._lib.HALO_E_REJECT and "C_(log_n)" in msg, "instance 40's relation before instance 50's transcript"


# ------------------------------------------------------------------ 4. both forms
def test_host_form_agrees(hal, ctx):
    d = (1 << 12) - 1
    members = with_tampers(chain(hal, ctx, 12, 40), 12, 3)
    dev = vbatch(ctx, d, members)
    ctx.set_batch_verify(False)
    try:
        host = vbatch(ctx, d, members)
        st, _ = expect_like_singles(ctx, d, members)
    finally:
        ctx.set_batch_verify(True)
    assert host == dev and dev[1] == st


# ------------------------------------------------------------------ 5. full size from the 2^20 fixture's seeds
def test_full_size_from_fixture_seeds(hal, big):
    from halo_accumulation_amd import acc as A
    with open(os.path.join(ROOT, "tests", "golden", "open_2_20.json")) as f:
        fx = json.load(f)
    lg = fx["lg_n"]
    d = (1 << lg) - 1
    a = fx["acc"]
    qs = [A.random_instance(big, [int(a["q_seeds"][k], 16)], d) for k in range(2)]
    acc = A.prover(big, [int(a["acc_seed"], 16)], d, qs)
    assert hashlib.sha256(acc.tobytes()).hexdigest() == a["acc_sha256"]
    bad = acc.copy()
    bad[17] ^= 1
    rc, st, msg = vbatch(big, d, [(qs, acc), (qs, bad)])
    assert st == [0, hal._lib.HALO_E_REJECT] and rc == hal._lib.HALO_E_REJECT
    assert [vsingle(big, d, (qs, acc))[0], vsingle(big, d, (qs, bad))[0]] == st
    assert msg == "member 1: " + vsingle(big, d, (qs, bad))[1]


# ------------------------------------------------------------------ 6. slots and repetition
def test_beside_a_callers_msm_and_repeated(hal, ctx):
    import torch
    d = (1 << 12) - 1
    members = with_tampers(chain(hal, ctx, 12, 40), 12, 3)  # 79 relations: the device form
    want = [vsingle(ctx, d, m)[0] for m in members]
    n = 1 << 14
    sc, _ = orc.rng_scalars(0xC0FFEE, n)
    dev = torch.from_numpy(sc.view(np.int64).reshape(-1).copy()).cuda()
    gs = ctx.read_bases()
    ref = orc.msm_affine(gs, sc)
    ctx.msm_dev_begin(1, dev.data_ptr(), n)
    try:
        assert vbatch(ctx, d, members)[1] == want
    finally:
        got = ctx.msm_dev_end(1)
    assert got.tolist() == ref.tolist(), "the caller's MSM on slot 1 kept its own result"
    first = vbatch(ctx, d, members)
    assert first[1] == want and vbatch(ctx, d, members) == first, "two calls in a row"
    for slot in range(4):
        ctx.msm_dev_begin(slot, dev.data_ptr(), n)
    try:
        assert vbatch(ctx, d, members) == first, "no idle slot: the host form, the same codes"
    finally:
        for slot in range(4):
            assert ctx.msm_dev_end(slot).tolist() == ref.tolist()


# ------------------------------------------------------------------ 7. without staging memory
def test_staging_fallback(hal):
    c = hal._lib.Context(urs_n=1 << 12)
    try:
        d = (1 << 10) - 1
        members = with_tampers(chain(hal, c, 10, 40), 10, 3)
        want = [vsingle(c, d, m)[0] for m in members]
        hal._lib.dev_hook("batch_stage_fail", 1)
        try:
            r_hook = vbatch(c, d, members)
        finally:
            hal._lib.dev_hook("reset", 0)
        assert r_hook[1] == want and r_hook[0] == hal._lib.HALO_E_REJECT
        budget = c.info(3)
        c.set_memory_budget(0)
        try:
            before = c.info(4)
            r0 = vbatch(c, d, members)
            assert c.info(4) <= before, "no optional memory under a zero budget"
        finally:
            c.set_memory_budget(budget)
        assert r0 == r_hook
        assert vbatch(c, d, members) == r_hook, "with staging"
    finally:
        c.close()


# ------------------------------------------------------------------ 8. multi-device context
def test_multi_device_context(hal, ctx):
    d = (1 << 12) - 1
    members = with_tampers(chain(hal, ctx, 12, 40), 12, 3)
    want = vbatch(ctx, d, members)
    m = hal._lib.Context(urs_n=1 << 14, devices=[0, 0])
    try:
        assert vbatch(m, d, members) == want
    finally:
        m.close()


# ------------------------------------------------------------------ 9. the acc_cmp_f shape (benches/acc.rs:64-74)
def test_acc_cmp_f_shape(hal, ctx):
    from halo_accumulation_amd import acc as A
    d = (1 << 9) - 1
    members = chain(hal, ctx, 9, 10)
    assert A.verifier_batch(ctx, d, [m[0] for m in members], [m[1] for m in members]) == [0] * 10
    A.decider(ctx, members[-1][1])
