"""halo_acc_prover_batch on the GPU.  Everything is bit-exact.  The kernels of the accumulated polynomial (k_h_tables with
scales + k_h_accumulate_batch) against the oracle's h coefficients and big-integer arithmetic; the batch against the loop of
single halo_acc_prover calls from the same seed -- blobs, zero-filled failures, status list, return code, message and final rng
state -- over members in the acc_compare step shape, with members tampered at every position the prover can notice, with 0, 1,
2 and 64 instances per member, against the oracle's prover, over chains in lockstep, through every fallback, and at full size."""
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


def ptr(a):
    from halo_accumulation_amd._lib import ptr as p
    return p(a)


def cat(qs):
    return np.ascontiguousarray(np.concatenate(qs)) if len(qs) else np.zeros(1, dtype=np.uint64)


def aw_of(lg):
    return 21 + 2 + 24 * lg + 32 + 24


def run_loop(c, d, members, seed):
    """the loop the batch is defined by: one rng state through k single calls, continuing after a failure
    -> [(code, message, blob, state before the call)], final state"""
    lg = (d + 1).bit_length() - 1
    st = C.c_uint64(seed)
    out = []
    for qs in members:
        before = st.value
        acc = np.zeros(aw_of(lg), dtype=np.uint64)
        rc = c.lib.halo_acc_prover(c.h, C.byref(st), d, ptr(cat(qs)), len(qs), ptr(acc))
        out.append((rc, c.lib.halo_last_error().decode() if rc else "", acc, before))
    return out, st.value


def run_batch(c, d, members, seed):
    """-> return code, status list (77 where the call wrote nothing), message, blobs (k x words), final state"""
    lg = (d + 1).bit_length() - 1
    k = len(members)
    counts = (C.c_size_t * max(k, 1))(*[len(qs) for qs in members])
    status = (C.c_int * max(k, 1))(*([77] * max(k, 1)))
    blobs = np.full((max(k, 1), aw_of(lg)), 0x5A5A, dtype=np.uint64)
    st = C.c_uint64(seed)
    rc = c.lib.halo_acc_prover_batch(c.h, C.byref(st), d, ptr(cat([q for qs in members for q in qs])), counts, k, ptr(blobs), status)
    return rc, [status[j] for j in range(k)], c.lib.halo_last_error().decode() if rc else "", blobs, st.value


def expect_like_loop(c, d, members, seed):
    loop, loop_state = run_loop(c, d, members, seed)
    rc, status, msg, blobs, state = run_batch(c, d, members, seed)
    assert status == [m[0] for m in loop]
    for j, (code, _, acc, _) in enumerate(loop):
        if code:
            assert not blobs[j].any(), "member %d failed: its blob is zero-filled" % j
        else:
            assert blobs[j].tolist() == acc.tolist(), "member %d" % j
    bad = [j for j, m in enumerate(loop) if m[0]]
    if bad:
        assert rc == loop[bad[0]][0] and msg == "member %d: %s" % (bad[0], loop[bad[0]][1])
    else:
        assert rc == 0
    assert state == loop_state
    return loop, status, blobs, state


# ------------------------------------------------------------------ 1. the kernels alone
def ints(a):
    a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)
    return sum(a[:, i].astype(object) << (64 * i) for i in range(4))


@pytest.mark.parametrize("lg", [1, 3, 8, 9, 14])
def test_accumulate_kernels_match_the_oracle(hal, ctx, lg):
    counts = [0, 1, 2, 3, 64, 2]
    total, n = sum(counts), 1 << lg
    xis, s = orc.rng_scalars(0xACC0 + lg, total * (lg + 1))
    alphas, s = orc.rng_scalars(s, total)
    alphas[1] = orc.fr_to_mont(0)
    alphas[2] = orc.fr_to_mont(1)
    alphas[10] = orc.fr_to_mont(R - 1)
    h0s, s = orc.rng_scalars(s, 2 * len(counts))
    h0s[2 * 2 + 1] = 0  # a zero linear term
    h0s[2 * 5] = 0
    want = []
    t = 0
    for j, m in enumerate(counts):
        acc = np.zeros(n, dtype=object)
        acc[0] = ints(h0s[2 * j])[0]
        acc[1] = ints(h0s[2 * j + 1])[0]
        for i in range(m):
            h = ints(orc.h_coeffs(np.ascontiguousarray(xis[(t + i) * (lg + 1):(t + i + 1) * (lg + 1)])))
            acc = (acc + orc.fr_from_mont(alphas[t + i]) * h) % R  # Montgomery form is linear: a (h R) = (a h) R
        want.append([int(x) for x in acc])
        t += m
    cl = (C.c_size_t * len(counts))(*counts)
    for max_tables in (0, 5, 64):  # one pass; members spread over passes; the 64-instance member exactly one pass
        out = np.full((len(counts), n, 4), 0x77, dtype=np.uint64)
        rc = ctx.lib.halo_dev_h_accumulate_batch(ctx.h, ptr(h0s), ptr(xis), ptr(alphas), cl, len(counts), lg, max_tables, ptr(out))
        assert rc == 0, ctx.lib.halo_last_error()
        for j in range(len(counts)):
            assert [int(x) for x in ints(out[j])] == want[j], "member %d, %d tables per pass" % (j, max_tables)
    assert ctx.lib.halo_dev_h_accumulate_batch(ctx.h, ptr(h0s), ptr(xis), ptr(alphas), cl, len(counts), 15, 0, ptr(out)) == hal._lib.HALO_E_ARG


# ------------------------------------------------------------------ members in the acc_compare step shape (benches/acc.rs:76-98)
_MEMBERS = {}


def step_members(hal, c, lg, k):
    """k members [Instance of a previous accumulator, a fresh random instance]: built with random_instance_batch and single provers"""
    key = (id(c), lg)
    have = _MEMBERS.get(key, [])
    if len(have) < k:
        from halo_accumulation_amd import acc as A
        d = (1 << lg) - 1
        rng = [0xB0B0000 + lg + 31 * len(have)]
        need = k - len(have)
        fresh = A.random_instance_batch(c, rng, d, 2 * need)
        for j in range(need):
            prev = A.prover(c, rng, d, [fresh[2 * j]])
            have.append([A.instance_from_accumulator(c, prev, d), fresh[2 * j + 1]])
        _MEMBERS[key] = have
    return [list(m) for m in have[:k]]


def tampered(qs, lg, what):
    """one member broken at one position acc::prover notices (acc.rs:158-170)"""
    qs = [q.copy() for q in qs]
    d = (1 << lg) - 1
    pf = 21 + 2 + 24 * lg  # U of a proof
    if what == "d_i":
        qs[-1][12] = d - 1
    elif what == "length":
        qs[0][22] = lg + 1
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
    else:
        raise ValueError(what)
    return qs


KINDS = ["d_i", "length", "L", "U", "c", "v", "hiding_C_bar"]


def with_tampers(members, lg, first, step):
    out, broken = list(members), []
    for n, what in enumerate(KINDS):
        j = first + n * step
        if j >= len(out):
            break
        out[j] = tampered(out[j], lg, what)
        broken.append(j)
    return out, broken


# ------------------------------------------------------------------ 2. argument errors
def test_argument_errors(hal, ctx):
    lg = 9
    d = (1 << lg) - 1
    members = step_members(hal, ctx, lg, 2)
    E_ARG, E_ASSERT = hal._lib.HALO_E_ARG, hal._lib.HALO_E_ASSERT
    lib = ctx.lib
    counts = (C.c_size_t * 2)(2, 2)
    qs = cat([q for m in members for q in m])

    def call(h, dd, q, cn, k, out, st, state):
        return lib.halo_acc_prover_batch(h, C.byref(state) if state is not None else None, dd, q, cn, k, out, st)

    st = (C.c_int * 2)(77, 77)
    state = C.c_uint64(0xFEED)
    out = np.full((2, aw_of(lg)), 0x5A5A, dtype=np.uint64)
    assert call(None, d, ptr(qs), counts, 2, ptr(out), st, state) == E_ARG and b"null context" in lib.halo_last_error()
    assert call(ctx.h, d, ptr(qs), counts, 2, None, st, state) == E_ARG
    assert call(ctx.h, d, ptr(qs), None, 2, ptr(out), st, state) == E_ARG
    assert call(ctx.h, d, None, counts, 2, ptr(out), st, state) == E_ARG
    assert call(ctx.h, d - 1, ptr(qs), counts, 2, ptr(out), st, state) == E_ASSERT
    assert lib.halo_last_error() == b"prover: d + 1 is not a power of two"
    assert call(ctx.h, (1 << 15) - 1, ptr(qs), counts, 2, ptr(out), st, state) == E_ASSERT
    assert lib.halo_last_error() == b"prover: d > D"
    assert call(ctx.h, d, None, None, 0, None, st, state) == 0
    assert list(st) == [77, 77] and state.value == 0xFEED and (out == 0x5A5A).all(), "whole-call errors and k = 0 touch nothing"
    # the single call's codes and messages
    acc = np.zeros(aw_of(lg), dtype=np.uint64)
    s1 = C.c_uint64(0xFEED)
    assert lib.halo_acc_prover(ctx.h, C.byref(s1), d - 1, ptr(qs), 2, ptr(acc)) == E_ASSERT and lib.halo_last_error() == b"prover: d + 1 is not a power of two"
    assert lib.halo_acc_prover(ctx.h, C.byref(s1), (1 << 15) - 1, ptr(qs), 2, ptr(acc)) == E_ASSERT and lib.halo_last_error() == b"prover: d > D"
    # nullable status and rng state (NULL: state 0, as the single call)
    assert call(ctx.h, d, ptr(qs), counts, 2, ptr(out), None, state) == 0
    want, _ = run_loop(ctx, d, members, 0xFEED)
    assert [out[j].tolist() for j in range(2)] == [w[2].tolist() for w in want]
    out0 = np.zeros((2, aw_of(lg)), dtype=np.uint64)
    assert call(ctx.h, d, ptr(qs), counts, 2, ptr(out0), st, None) == 0
    assert lib.halo_acc_prover(ctx.h, None, d, ptr(cat(members[0])), 2, ptr(acc)) == 0 and out0[0].tolist() == acc.tolist()
    # a member without instances
    expect_like_loop(ctx, d, [members[0], [], members[1], []], 0x5EED)
    from halo_accumulation_amd import acc as A
    rng = [0x5EED]
    accs, codes = A.prover_batch(ctx, rng, d, [members[0], [], members[1], []])
    loop, final = run_loop(ctx, d, [members[0], [], members[1], []], 0x5EED)
    assert codes == [0] * 4 and rng[0] == final and [a.tolist() for a in accs] == [w[2].tolist() for w in loop]
    with pytest.raises(hal._lib.HaloReject) as e:
        A.prover_batch(ctx, rng, d, [members[0], tampered(members[1], lg, "v")])
    assert e.value.args[1] == [0, hal._lib.HALO_E_REJECT]


# ------------------------------------------------------------------ 3. parity with the loop, 4. against the oracle
@pytest.mark.parametrize("lg,k", [(lg, k) for lg in (3, 9, 12, 14) for k in (1, 10, 33)] + [(9, 100)])
def test_matches_the_loop(hal, ctx, lg, k):
    d = (1 << lg) - 1
    members = step_members(hal, ctx, lg, k)
    loop, status, blobs, final = expect_like_loop(ctx, d, members, 0x10000 + 97 * lg + k)
    assert status == [0] * k
    if lg in (3, 9) and k == 10:  # the oracle's prover from each member's start state
        pp = orc.make_pp(ctx.read_bases(0, 1 << lg))
        for j in (0, 1, k - 1):
            want, after = orc.acc_prover(pp, loop[j][3], d, members[j])
            assert blobs[j].tolist() == want.tolist()
            assert after == (loop[j + 1][3] if j + 1 < k else final)
    if k == 1:
        bad, broken = [tampered(members[0], lg, "c")], [0]
    else:
        bad, broken = with_tampers(members, lg, 0 if k == 10 else 1, 1 if k <= 10 else 4)
    loop, status, _, _ = expect_like_loop(ctx, d, bad, 0x20000 + 97 * lg + k)
    assert [j for j, s in enumerate(status) if s] == broken
    if k > 1:
        good_after = [j for j in range(broken[0] + 1, k) if not status[j]]
        assert good_after, "a broken member is followed by good ones"
        # a rejected member draws nothing: the next member starts from the same state
        for j in broken:
            if j + 1 < k:
                assert loop[j + 1][3] == loop[j][3]


# ------------------------------------------------------------------ 5. instances per member
@pytest.mark.parametrize("lg", [9, 12])
def test_instances_per_member(hal, ctx, lg):
    """0, 1, 2 and 64 instances per member in one call (64: the succinct half's own device form)"""
    from halo_accumulation_amd import acc as A
    d = (1 << lg) - 1
    rng = [0x64640000 + lg]
    qs64 = A.random_instance_batch(ctx, rng, d, 64)
    two = step_members(hal, ctx, lg, 3)
    members = [[], two[0], qs64, [qs64[5]], two[1], [], two[2]]
    _, status, _, _ = expect_like_loop(ctx, d, members, 0x646464)
    assert status == [0] * 7
    late = list(qs64)
    late[40] = tampered([qs64[40]], lg, "v")[0]
    late[50] = tampered([qs64[50]], lg, "L")[0]
    loop, status, _, _ = expect_like_loop(ctx, d, [two[0], late, [], tampered(two[1], lg, "d_i"), qs64], 0x646465)
    assert status == [0, hal._lib.HALO_E_REJECT, 0, hal._lib.HALO_E_REJECT, 0]
    assert "C_(log_n)" in loop[1][1], "instance 40's relation before instance 50's transcript"
    ctx.set_batch_verify(False)  # the succinct half on the host pool: the same
    try:
        assert expect_like_loop(ctx, d, [two[0], late, qs64], 0x646466)[1] == [0, hal._lib.HALO_E_REJECT, 0]
    finally:
        ctx.set_batch_verify(True)


# ------------------------------------------------------------------ 6. the device form really ran
def launches(c, fn):
    c.prof_enable(1)
    c.prof_reset()
    try:
        fn()
        return {name: v[1] for name, v in c.prof().items()}
    finally:
        c.prof_enable(0)


def test_device_form_ran(hal, ctx):
    lg, k = 12, 10
    d = (1 << lg) - 1
    members = step_members(hal, ctx, lg, k)
    want = run_batch(ctx, d, members, 0xD0D0)
    assert want[0] == 0
    ran = launches(ctx, lambda: run_batch(ctx, d, members, 0xD0D0))
    assert ran.get("k_h_accumulate_batch", 0) == 3, "groups of 4 members: ceil(10 / 4) launches"
    assert ran.get("k_h_tables", 0) == 3 and ran.get("k_h_coeffs", 0) == 0
    for group in (1, 2):
        hal._lib.dev_hook("open_batch_group", group)
        try:
            ran = launches(ctx, lambda: run_batch(ctx, d, members, 0xD0D0))
        finally:
            hal._lib.dev_hook("reset", 0)
        assert ran.get("k_h_accumulate_batch", 0) == (k + group - 1) // group and ran.get("k_h_coeffs", 0) == 0
    # 64 + 2 + 0 instances: 66 polynomials in passes of 32 -> three passes of the one group
    from halo_accumulation_amd import acc as A
    qs64 = A.random_instance_batch(ctx, [0x4040], d, 64)
    ran = launches(ctx, lambda: run_batch(ctx, d, [qs64, members[0], []], 0xD0D1))
    assert ran.get("k_h_accumulate_batch", 0) == 3 and ran.get("k_h_coeffs", 0) == 0


# ------------------------------------------------------------------ 7. chains in lockstep
def test_chains_in_lockstep(hal, ctx):
    from halo_accumulation_amd import acc as A
    lg, chains, steps = 10, 8, 6
    d = (1 << lg) - 1

    def run(batched):
        rng = [0xC4A1]
        prev, all_members, all_accs = [None] * chains, [], []
        for _ in range(steps):
            if batched:
                fresh = A.random_instance_batch(ctx, rng, d, chains)
            else:
                fresh = [A.random_instance(ctx, rng, d) for _ in range(chains)]
            members = [[fresh[j]] if prev[j] is None else [A.instance_from_accumulator(ctx, prev[j], d), fresh[j]] for j in range(chains)]
            if batched:
                prev, codes = A.prover_batch(ctx, rng, d, members)
                assert codes == [0] * chains
            else:
                prev = [A.prover(ctx, rng, d, m) for m in members]
            all_members += members
            all_accs += prev
        return all_members, all_accs, rng[0]

    mb, ab, sb = run(True)
    ml, al, sl = run(False)
    assert sb == sl
    assert [a.tolist() for a in ab] == [a.tolist() for a in al]
    assert [[q.tolist() for q in m] for m in mb] == [[q.tolist() for q in m] for m in ml]
    assert A.verifier_batch(ctx, d, mb, ab) == [0] * (chains * steps)
    assert A.decider_batch(ctx, d, ab[-chains:]) == [0] * chains


# ------------------------------------------------------------------ 8. fallbacks
def same(a, b):
    return a[0] == b[0] and a[1] == b[1] and a[2] == b[2] and a[3].tolist() == b[3].tolist() and a[4] == b[4]


def test_fallbacks_give_the_same_answer(hal, ctx):
    import torch
    lg, k = 10, 9
    d = (1 << lg) - 1
    members, broken = with_tampers(step_members(hal, ctx, lg, k), lg, 2, 5)
    assert broken == [2, 7]
    expect_like_loop(ctx, d, members, 0xFA11)
    want = run_batch(ctx, d, members, 0xFA11)
    assert same(run_batch(ctx, d, members, 0xFA11), want), "two calls in a row"
    hal._lib.dev_hook("batch_stage_fail", 1)
    try:
        got = []
        ran = launches(ctx, lambda: got.append(run_batch(ctx, d, members, 0xFA11)))
    finally:
        hal._lib.dev_hook("reset", 0)
    assert same(got[0], want) and ran.get("k_h_accumulate_batch", 0) == 0 and ran.get("k_h_coeffs", 0) > 0
    for group in (1, 2):
        hal._lib.dev_hook("open_batch_group", group)
        try:
            assert same(run_batch(ctx, d, members, 0xFA11), want)
        finally:
            hal._lib.dev_hook("reset", 0)
    # a caller's MSM in flight on slot 1; all four slots busy
    n = 1 << 14
    sc, _ = orc.rng_scalars(0xC0FFEE, n)
    dev = torch.from_numpy(sc.view(np.int64).reshape(-1).copy()).cuda()
    ref = orc.msm_affine(ctx.read_bases(), sc)
    ctx.msm_dev_begin(1, dev.data_ptr(), n)
    try:
        assert same(run_batch(ctx, d, members, 0xFA11), want)
    finally:
        got1 = ctx.msm_dev_end(1)
    assert got1.tolist() == ref.tolist(), "the caller's MSM on slot 1 kept its own result"
    for slot in range(4):
        ctx.msm_dev_begin(slot, dev.data_ptr(), n)
    try:
        busy = run_batch(ctx, d, members, 0xFA11)
    finally:
        for slot in range(4):
            assert ctx.msm_dev_end(slot).tolist() == ref.tolist()
    assert busy[0] == hal._lib.HALO_E_ARG and busy[1] == [77] * k and busy[4] == 0xFA11 and (busy[3] == 0x5A5A).all()
    assert same(run_batch(ctx, d, members, 0xFA11), want)


def test_zero_budget_and_multi_device(hal, ctx):
    lg, k = 10, 6
    d = (1 << lg) - 1
    members, _ = with_tampers(step_members(hal, ctx, lg, k), lg, 1, 3)
    want = run_batch(ctx, d, members, 0xB0D6)
    c = hal._lib.Context(urs_n=1 << 10)
    try:
        budget = c.info(3)
        c.set_memory_budget(0)
        try:
            before = c.info(4)
            got = []
            ran = launches(c, lambda: got.append(run_batch(c, d, members, 0xB0D6)))
            assert c.info(4) <= before, "no optional memory under a zero budget"
        finally:
            c.set_memory_budget(budget)
        assert same(got[0], want) and ran.get("k_h_accumulate_batch", 0) == 0
        assert same(run_batch(c, d, members, 0xB0D6), want), "with staging"
    finally:
        c.close()
    m = hal._lib.Context(urs_n=1 << 14, devices=[0, 0])
    try:
        assert same(run_batch(m, d, members, 0xB0D6), want)
    finally:
        m.close()


def test_above_the_device_form(hal):
    """d + 1 above the no-fold size: the members one at a time, the same answer"""
    lg = 15
    d = (1 << lg) - 1
    c = hal._lib.Context(urs_n=1 << lg)
    try:
        members, broken = with_tampers(step_members(hal, c, lg, 3), lg, 1, 1)
        ran = launches(c, lambda: expect_like_loop(c, d, members[:3], 0xAB0E))
        assert ran.get("k_h_accumulate_batch", 0) == 0
    finally:
        c.close()


# ------------------------------------------------------------------ 9. full size from the 2^20 fixture's seeds
def test_full_size_from_fixture_seeds(hal):
    from halo_accumulation_amd import acc as A
    with open(os.path.join(ROOT, "tests", "golden", "open_2_20.json")) as f:
        fx = json.load(f)
    lg = fx["lg_n"]
    d = (1 << lg) - 1
    a = fx["acc"]
    big = hal._lib.Context(urs_n=1 << lg)
    try:
        qs = [A.random_instance(big, [int(a["q_seeds"][k], 16)], d) for k in range(2)]
        members = [qs, [qs[1]]]
        loop, status, blobs, _ = expect_like_loop(big, d, members, int(a["acc_seed"], 16))
        assert status == [0, 0]
        assert hashlib.sha256(blobs[0].tobytes()).hexdigest() == a["acc_sha256"]
    finally:
        big.close()
