"""halo_pcdl_check_batch_mixed_fused / halo_acc_decider_batch_mixed_fused on the GPU: the term kernel's scalars over members of
their own sizes limb for limb against Python integers; an honest batch of three sizes accepted by ONE relation with no per-member
ladder, no per-member MSM and one MSM over the key (the profiler shows which path ran); the left side cut into chunks inside a
member's terms; every kind of reject with the exact mixed call's statuses, code and message; a pair of members of different sizes
whose unweighted defects cancel; the edges (one size, a class of one, a constant, no member, one member, whole-call errors, no
staging); and the table pipeline as the key's MSM on a 2^20-point key.  The pools of honest members are those of
tests/test_gpu_check_combined.py, the helpers around them those of tests/test_gpu_check_mixed.py."""
import ctypes as C

import numpy as np
import pytest

import fused_cases as fc
import orc
import test_gpu_check_combined as cc
import test_gpu_check_fused as cf
import test_gpu_check_mixed as mt
from test_gpu_check_mixed import big, big_members, ctx, hal  # noqa: F401  (the fixtures: a 2^14-point and a 2^20-point key)

pytestmark = pytest.mark.gpu

R_MOD = fc.R_MOD
REJECT = mt.REJECT
ptr = cc.ptr
lg_of = mt.lg_of
honest = mt.honest
interleave = mt.interleave


def fused(c, blobs, acc=False, seed=None, ds=None):
    """-> (return code, status list, message); status entries the call does not write stay 77"""
    m = len(blobs)
    keep = [np.ascontiguousarray(b, dtype=np.uint64) for b in blobs]
    ps = (C.c_void_p * max(m, 1))(*[b.ctypes.data for b in keep])
    dd = (C.c_size_t * max(m, 1))(*(ds if ds is not None else [mt.d_of(b) for b in keep]))
    st = (C.c_int * max(m, 1))(*([77] * max(m, 1)))
    fn = c.lib.halo_acc_decider_batch_mixed_fused if acc else c.lib.halo_pcdl_check_batch_mixed_fused
    rc = fn(c.h, dd, ps, m, seed, st)
    return rc, [st[i] for i in range(m)], (c.lib.halo_last_error().decode() if rc else "")


def exact(c, blobs, acc=False, ds=None):
    return mt.mixed(c, blobs, acc=acc, combined=False, ds=ds)


def ran_relation_only(counts):
    """the mixed relation ran, once, and nothing of the exact path did: no ladder per member, no h expansion per member"""
    return (counts.get("k_mixed_terms", 0) == 1 and counts.get("k_fused_terms", 0) == 0 and counts.get("k_batch_small_msm", 0) == 0
            and counts.get("k_h_coeffs_batch", 0) == 0 and counts.get("k_h_accumulate_mixed", 0) > 0 and counts.get("k_batch_to_affine", 0) == 1)


def ran_relation_then_exact(counts):
    return counts.get("k_mixed_terms", 0) == 1 and counts.get("k_h_accumulate_mixed", 0) > 0 and counts.get("k_h_coeffs_batch", 0) > 0


def ran_exact_only(counts):
    return counts.get("k_mixed_terms", 0) == 0 and counts.get("k_h_accumulate_mixed", 0) == 0 and counts.get("k_h_coeffs_batch", 0) > 0


def terms_of(blobs):
    """T: every member's 2 lg + 2 terms and H"""
    return sum(2 * lg_of(q) + 2 for q in blobs) + 1


_ACC10 = {}


def honest_accs(c, lg, k):
    """k honest accumulators of size lg on the 2^14-point key: lg 3 and 9 from the shared pools, lg 10 over the small pool of lg 10"""
    if lg in (3, 9):
        return honest(c, lg, k, acc=True)
    if lg not in _ACC10:
        from halo_accumulation_amd import acc as A
        accs, codes = A.prover_batch(c, [0xACC0 + lg], (1 << lg) - 1, [[q] for q in honest(c, lg, 3)])
        assert codes == [0] * 3
        _ACC10[lg] = list(accs)
    return list(_ACC10[lg][:k])


def accepted_alone(c, blobs, acc=False):
    """every honest pool is accepted by the single calls before it is used"""
    got = mt.by_single_calls(c, blobs, acc)
    assert got == (0, [0] * len(blobs), ""), got
    return blobs


# ------------------------------------------------------------------ 1. the term kernel against integers
TERM_SETS = {
    "one member": [1],
    "the shortest and the longest": [1, 24],
    "unsorted with repeats": [3, 9, 9, 1, 8],
    "one full wave of lg 1..24": [1 + a % 24 for a in range(64)],
    "a second block with one live lane": [1 + a % 24 for a in range(65)],
}


def term_members(lgs):
    """member a: the a-th of fused_cases.members(lg_a, 65): the special values lie among them, shuffled in"""
    pools = {lg: fc.members(lg, 65, seed=11) for lg in set(lgs)}
    return [pools[lg][a] for a, lg in enumerate(lgs)]


def mixed_terms(c, mem):
    recs = np.ascontiguousarray(np.concatenate([m.record() for m in mem]))
    terms = sum(2 * m.lg + 2 for m in mem)
    sc, h = np.full((terms, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    ll = (C.c_size_t * len(mem))(*[m.lg for m in mem])
    assert c.lib.halo_dev_check_mixed_terms(c.h, ptr(recs), ll, len(mem), ptr(sc), ptr(h)) == 0, c.lib.halo_last_error()
    return sc, h


@pytest.mark.parametrize("name", list(TERM_SETS))
def test_term_kernel_equals_python_integers(hal, ctx, name):
    lgs = TERM_SETS[name]
    mem = term_members(lgs)
    assert [m.lg for m in mem] == lgs
    if len(lgs) == 65:
        assert lgs[64] != lgs[0], "the second block's one live lane has another size than lane 0"
    if len(lgs) >= 64:
        assert any(m.r in fc.SPECIAL_W and m.s in fc.SPECIAL_W for m in mem) and any(m.c in fc.SPECIAL_C for m in mem)
        assert any(m.xis[-1] in fc.SPECIAL_XI for m in mem) and any(m.z == 0 for m in mem), "the special values are among the members"
    sc, h = mixed_terms(ctx, mem)
    bad, t = [], 0
    for a, m in enumerate(mem):
        K = 2 * m.lg + 2
        bad += [(a, m.lg) + b for b in fc.check_member(m, sc[t:t + K], None)]
        t += K
    assert t == len(sc)
    assert not bad, "%d wrong scalars; first (member, lg, what, index): %s" % (len(bad), bad[:8])
    assert [int(w) for w in h] == fc.words(sum(m.share() for m in mem) % R_MOD), "H's scalar is the integer sum of the shares"


def test_members_of_one_size_give_the_uniform_kernels_words(hal, ctx):
    mem = fc.members(9, 5, seed=5)
    sc, h = mixed_terms(ctx, mem)
    recs = np.ascontiguousarray(np.concatenate([m.record() for m in mem]))
    sc_u, h_u = np.zeros((5 * 20, 4), dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    assert ctx.lib.halo_dev_check_fused_terms(ctx.h, ptr(recs), 5, 9, ptr(sc_u), ptr(h_u)) == 0
    assert np.array_equal(sc, sc_u) and np.array_equal(h, h_u)


def test_term_kernel_argument_errors(hal, ctx):
    recs, sc, h = np.zeros(2 * 7 * 4, dtype=np.uint64), np.zeros(2 * 4 * 4, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    f = ctx.lib.halo_dev_check_mixed_terms
    E = hal._lib.HALO_E_ARG
    ok = (C.c_size_t * 2)(1, 1)
    for M in (0, 65536):
        assert f(ctx.h, ptr(recs), ok, M, ptr(sc), ptr(h)) == E, M
    for lgs in ((0, 1), (1, 0), (25, 1), (1, 25)):
        assert f(ctx.h, ptr(recs), (C.c_size_t * 2)(*lgs), 2, ptr(sc), ptr(h)) == E, lgs
    assert f(ctx.h, None, ok, 2, ptr(sc), ptr(h)) == E
    assert f(ctx.h, ptr(recs), None, 2, ptr(sc), ptr(h)) == E
    assert f(ctx.h, ptr(recs), ok, 2, None, ptr(h)) == E
    assert f(ctx.h, ptr(recs), ok, 2, ptr(sc), None) == E
    assert f(None, ptr(recs), ok, 2, ptr(sc), ptr(h)) == E


# ------------------------------------------------------------------ 2. an honest mixed batch: one relation
@pytest.mark.parametrize("acc", [False, True], ids=["pcdl", "decider"])
def test_honest_mixed_batch_is_accepted_by_one_relation(hal, ctx, acc):
    pick = honest_accs if acc else honest
    blobs = accepted_alone(ctx, interleave(pick(ctx, 3, 3), pick(ctx, 9, 3), pick(ctx, 10, 2)), acc)
    assert [lg_of(q) for q in blobs] == [3, 9, 10, 3, 9, 10, 3, 9]
    (rc, st, _), counts = cc.profiled(ctx, lambda: fused(ctx, blobs, acc))
    assert rc == 0 and st == [0] * 8
    assert ran_relation_only(counts), counts
    assert terms_of(blobs) == 129 and mt.sequences(counts) == 2, "ONE MSM over the key and one sequence of the left side's one chunk: %r" % counts
    assert fused(ctx, blobs, acc, seed=bytes(range(32))) == (0, [0] * 8, "")


def test_python_wrappers(hal, ctx):
    from halo_accumulation_amd import acc as A, pcdl
    blobs = interleave(honest(ctx, 3, 2), honest(ctx, 9, 2))
    accs = interleave(honest_accs(ctx, 3, 2), honest_accs(ctx, 9, 2))
    assert pcdl.check_batch_mixed_fused(ctx, blobs) == [0] * 4
    assert pcdl.check_batch_mixed_fused(ctx, blobs, seed=bytes(range(32))) == [0] * 4
    assert A.decider_batch_mixed_fused(ctx, accs) == [0] * 4
    bad = list(blobs)
    bad[1] = cc.tamper(bad[1], 9, "v")
    with pytest.raises(hal._lib.HaloReject) as e:
        pcdl.check_batch_mixed_fused(ctx, bad)
    assert e.value.args[1] == [0, REJECT, 0, 0] and e.value.args[0].startswith("instance 1: ")


# ------------------------------------------------------------------ 3. the left side in chunks and sequences
def test_left_side_in_chunks_that_cut_inside_a_member(hal, ctx):
    """lg 3, 9, 10, 3, 9, 10, 3, 9: T = 129 terms, member 1 (lg 9) holds terms 8 .. 27, its L terms 9 .. 17.  8 terms a chunk: 17
    chunks in three sequences, a cut at term 16; 13 a chunk: 10 chunks in two sequences, a cut at term 13"""
    blobs = accepted_alone(ctx, interleave(honest(ctx, 3, 3), honest(ctx, 9, 3), honest(ctx, 10, 2)))
    T = terms_of(blobs)
    bad = list(blobs)
    bad[4] = cc.foreign(hal, 9, [0xF0A])[0]
    want_bad = exact(ctx, bad)
    assert [i for i, s in enumerate(want_bad[1]) if s] == [4]
    for chunk in (8, 13):
        assert any(10 <= cut <= 17 for cut in range(chunk, T, chunk)), "a chunk ends inside member 1's L terms"
        chunks = -(-T // chunk)
        seqs = -(-chunks // 8)
        (rc, st, _), counts = cc.profiled(ctx, lambda: cf.chunked(hal, chunk, lambda: fused(ctx, blobs)))
        assert rc == 0 and st == [0] * 8 and ran_relation_only(counts), (chunk, counts)
        assert mt.sequences(counts) == 1 + seqs, "%d chunks in %d sequences beside the key's MSM: %r" % (chunks, seqs, counts)
        assert cf.chunked(hal, chunk, lambda: fused(ctx, bad)) == want_bad, chunk
    accs = accepted_alone(ctx, interleave(honest_accs(ctx, 3, 3), honest_accs(ctx, 9, 3)), acc=True)
    assert cf.chunked(hal, 13, lambda: fused(ctx, accs, acc=True)) == (0, [0] * 6, "")


def test_with_one_idle_slot_the_left_side_follows_the_keys_msm(hal, ctx):
    import torch
    blobs = interleave(honest(ctx, 3, 3), honest(ctx, 9, 3), honest(ctx, 10, 2))
    bad = list(blobs)
    bad[3] = cc.tamper(bad[3], 3, "c")
    want_bad = exact(ctx, bad)
    n = 1 << 14
    sc, _ = orc.rng_scalars(0xC0FFEE, n)
    dev = torch.from_numpy(sc.view(np.int64).reshape(-1).copy()).cuda()
    expect = orc.msm_affine(ctx.read_bases(), sc).tolist()
    for held in ((1,), (1, 2, 3)):  # (three idle slots; then ONE: the left side runs on it after the key's MSM)
        got = []

        def beside():  # (the profiler reports once every slot is idle again: the caller's MSMs are collected inside its bracket)
            for slot in held:
                ctx.msm_dev_begin(slot, dev.data_ptr(), n)
            try:
                return cf.chunked(hal, 8, lambda: fused(ctx, blobs)), fused(ctx, bad)
            finally:
                for slot in held:
                    got.append(ctx.msm_dev_end(slot))

        ((rc, st, _), rejected), counts = cc.profiled(ctx, beside)
        assert rc == 0 and st == [0] * 8 and counts.get("k_mixed_terms", 0) == 2, (held, counts)
        assert rejected == want_bad, held
        assert all(g.tolist() == expect for g in got), "the caller's MSMs kept their own results"
    for slot in range(4):
        ctx.msm_dev_begin(slot, dev.data_ptr(), n)
    try:
        busy = fused(ctx, blobs)
    finally:
        for slot in range(4):
            assert ctx.msm_dev_end(slot).tolist() == expect
    assert busy[0] == hal._lib.HALO_E_ARG and busy[1] == [77] * 8, "no idle slot"
    assert fused(ctx, blobs) == (0, [0] * 8, "")


# ------------------------------------------------------------------ 4. rejects equal the exact mixed call's and the single calls'
def test_rejects_equal_the_exact_mixed_call_and_the_single_calls(hal, ctx):
    """one tampered member of every kind over the three classes, and one opened under another key, which only the MSM of
    pcdl.rs:338 rejects"""
    blobs = accepted_alone(ctx, interleave(honest(ctx, 3, 3), honest(ctx, 9, 3), honest(ctx, 10, 3)))  # lg 3, 9, 10, 3, 9, 10, 3, 9, 10
    for i, what in ((1, "U"), (2, "c"), (3, "L"), (5, "v"), (6, "C")):
        blobs[i] = cc.tamper(blobs[i], lg_of(blobs[i]), what)
    blobs[7] = cc.foreign(hal, 9, [0x7E57])[0]
    want = mt.by_single_calls(ctx, blobs)
    assert [i for i, s in enumerate(want[1]) if s] == [1, 2, 3, 5, 6, 7] and want[0] == REJECT and want[2].startswith("instance 1: ")
    assert exact(ctx, blobs) == want
    got, counts = cc.profiled(ctx, lambda: fused(ctx, blobs))
    assert got == want
    assert ran_relation_then_exact(counts), "the relation, then the exact path: %r" % counts
    assert fused(ctx, blobs, seed=bytes(range(3, 35))) == want
    # the foreign member alone among honest ones: its index in THIS call is in the message
    few = [honest(ctx, 3, 1)[0], blobs[7], honest(ctx, 10, 1)[0]]
    assert fused(ctx, few) == exact(ctx, few) == (REJECT, [0, REJECT, 0], "instance 1: U != CM.Commit(ck, h_vec)")


def test_one_tampered_member_among_four_of_another_size(hal, ctx):
    for what in ("v", "U"):  # (v: the relation fails; U: off the curve, rejected with the transcripts, the four are accepted by the relation)
        blobs = honest(ctx, 9, 4)
        blobs.insert(2, cc.tamper(honest(ctx, 3, 1)[0], 3, what))
        want = mt.by_single_calls(ctx, blobs)
        assert want[1] == [0, 0, REJECT, 0, 0] and want[2].startswith("instance 2: ")
        got, counts = cc.profiled(ctx, lambda: fused(ctx, blobs))
        assert got == want == exact(ctx, blobs), what
        assert ran_relation_then_exact(counts) if what == "v" else ran_relation_only(counts), (what, counts)


def test_decider_rejects_equal_the_single_calls(hal, ctx):
    accs = accepted_alone(ctx, interleave(honest_accs(ctx, 3, 3), honest_accs(ctx, 9, 3)), acc=True)  # lg 3, 9, 3, 9, 3, 9
    accs[2] = cc.tamper(accs[2], 3, "v")
    accs[3] = cc.tamper(accs[3], 9, "U")
    f = cc.foreign(hal, 9, [0x7E58])[0]
    accs[5] = np.concatenate([f, accs[5][len(f):]])  # (the decider checks the Instance prefix)
    want = mt.by_single_calls(ctx, accs, acc=True)
    assert [i for i, s in enumerate(want[1]) if s] == [2, 3, 5] and want[2].startswith("instance 2: ")
    assert exact(ctx, accs, acc=True) == want
    assert fused(ctx, accs, acc=True) == want


# ------------------------------------------------------------------ 5. defects that cancel across classes
def test_defects_that_cancel_across_classes_are_rejected(hal, ctx):
    """The construction of tests/test_gpu_check_mixed.py: an instance of lg 3 opened under a key whose G_0 is G_0 + G_1 has
    U = <h, G> + G_1 under the true key, one of lg 9 opened with G_0 - G_1 has U = <h, G> - G_1.  Each has E = 0 and F = +-G_1, so
    the relation with every s_a ONE would accept the pair.  The hashed weights must not."""
    from halo_accumulation_amd import acc as A, pcdl
    from halo_accumulation_amd._lib import point_sum
    n = 512
    gs = ctx.read_bases(0, n)
    g0, g1 = cc.to_jac(gs[0]), cc.to_jac(gs[1])
    neg_g1 = g1.copy()
    neg_g1[4:8] = cc.limbs(cc.P_MOD - cc.to_int(g1[4:8]))  # -y on the Montgomery limbs
    pair = []
    for k, (shift, lg) in enumerate(((g1, 3), (neg_g1, 9))):
        key = gs.copy()
        key[0] = cc.affine_of(point_sum(np.stack([g0, shift])))
        other = hal._lib.Context(np.ascontiguousarray(key))
        try:
            pair.append(A.random_instance(other, [0xCA9CE5 + k], (1 << lg) - 1))
        finally:
            other.close()
    # the construction: each alone is an MSM reject, and the unweighted sum holds
    Us, commits = [], []
    for q in pair:
        assert mt.single(ctx, q) == (REJECT, "U != CM.Commit(ck, h_vec)")
        xis, U = pcdl.succinct_check(ctx, q[0:12].copy(), mt.d_of(q), q[13:17].copy(), q[17:21].copy(), q[21:].copy())
        Us.append(U)
        commits.append(ctx.h_commit(xis))
    assert orc.point_canonical(point_sum(np.stack(commits))) == orc.point_canonical(point_sum(np.stack(Us)))
    assert orc.point_canonical(commits[0]) != orc.point_canonical(Us[0])
    want = (REJECT, [REJECT, REJECT], "instance 0: U != CM.Commit(ck, h_vec)")
    assert exact(ctx, pair) == want
    got, counts = cc.profiled(ctx, lambda: fused(ctx, pair))
    assert got == want and ran_relation_then_exact(counts), counts
    assert fused(ctx, pair, seed=bytes(range(32))) == want
    among = [honest(ctx, 9, 1)[0], pair[0], honest(ctx, 3, 1)[0], pair[1], honest(ctx, 10, 1)[0]]
    want = (REJECT, [0, REJECT, 0, REJECT, 0], "instance 1: U != CM.Commit(ck, h_vec)")
    assert exact(ctx, among) == want
    assert fused(ctx, among) == want and fused(ctx, among, seed=bytes(range(32))) == want


# ------------------------------------------------------------------ 6. edges
def test_members_of_one_size_get_the_uniform_fused_calls_statuses(hal, ctx):
    blobs = accepted_alone(ctx, honest(ctx, 9, 6))
    (rc, st, _), counts = cc.profiled(ctx, lambda: fused(ctx, blobs))
    assert (rc, st) == cf.call(ctx, 511, blobs)[:2] == (0, [0] * 6) and ran_relation_only(counts), counts
    blobs[2] = cc.tamper(blobs[2], 9, "c")
    blobs[4] = cc.foreign(hal, 9, [0x7E59])[0]
    uniform = cf.call(ctx, 511, blobs)
    assert uniform[1] == [0, 0, REJECT, 0, REJECT, 0]
    got, counts = cc.profiled(ctx, lambda: fused(ctx, blobs))
    assert got == uniform and counts.get("k_mixed_terms", 0) == 1 and counts.get("k_fused_terms", 0) == 0, counts


def test_a_class_of_one_beside_a_class_of_four(hal, ctx):
    blobs = honest(ctx, 9, 4)
    blobs.insert(2, honest(ctx, 3, 1)[0])
    accepted_alone(ctx, blobs)
    (rc, st, _), counts = cc.profiled(ctx, lambda: fused(ctx, blobs))
    assert rc == 0 and st == [0] * 5 and ran_relation_only(counts) and mt.sequences(counts) == 2, counts


def test_a_constant_takes_the_exact_path_beside_the_relation(hal, ctx):
    const = mt.constant_instance(hal, ctx)
    assert mt.d_of(const) == 0 and mt.single(ctx, const) == (0, ""), "the construction: an Instance of d = 0 the single call accepts"
    blobs = accepted_alone(ctx, [honest(ctx, 9, 1)[0], const, honest(ctx, 3, 1)[0], honest(ctx, 9, 2)[1]])
    got, counts = cc.profiled(ctx, lambda: fused(ctx, blobs))
    assert got == (0, [0] * 4, "")
    assert counts.get("k_mixed_terms", 0) == 1 and counts.get("k_h_accumulate_mixed", 0) > 0, "the three members with d >= 1 take the relation: %r" % counts
    assert counts.get("k_h_coeffs_batch", 0) > 0 and mt.sequences(counts) == 3, "the key's MSM, the left side's, and the constant's own exact MSM: %r" % counts
    bad = list(blobs)
    bad[1] = cc.tamper(const, 0, "c")
    assert fused(ctx, bad) == exact(ctx, bad) == mt.by_single_calls(ctx, bad) and fused(ctx, bad)[1] == [0, REJECT, 0, 0]
    # a constant and ONE other member: no relation
    got, counts = cc.profiled(ctx, lambda: fused(ctx, blobs[:2]))
    assert got == (0, [0, 0], "") and ran_exact_only(counts), counts


def test_no_member_and_one_member(hal, ctx):
    for acc in (False, True):
        assert fused(ctx, [], acc=acc) == (0, [], "")
        q = honest(ctx, 9, 1, acc=acc)[0]
        (rc, st, _), counts = cc.profiled(ctx, lambda: fused(ctx, [q], acc=acc))
        assert rc == 0 and st == [0] and ran_exact_only(counts), counts
    # ... and so does a batch of which one member is left after the transcripts
    two = [honest(ctx, 9, 1)[0], cc.tamper(honest(ctx, 3, 1)[0], 3, "U")]
    got, counts = cc.profiled(ctx, lambda: fused(ctx, two))
    assert got == exact(ctx, two) and got[1] == [0, REJECT] and ran_exact_only(counts), counts
    fn = ctx.lib.halo_pcdl_check_batch_mixed_fused
    assert fn(ctx.h, None, None, 0, None, None) == 0
    a, b = np.ascontiguousarray(honest(ctx, 9, 1)[0]), np.ascontiguousarray(honest(ctx, 3, 1)[0])
    assert fn(ctx.h, (C.c_size_t * 1)(511), (C.c_void_p * 1)(a.ctypes.data), 1, None, None) == 0, "status is nullable"
    assert fn(ctx.h, (C.c_size_t * 2)(511, 7), (C.c_void_p * 2)(a.ctypes.data, b.ctypes.data), 2, None, None) == 0, "status is nullable"


def test_whole_call_errors_leave_status_untouched(hal, ctx):
    E = hal._lib.HALO_E_ARG
    for acc in (False, True):
        x, y = np.ascontiguousarray(honest(ctx, 3, 1, acc=acc)[0]), np.ascontiguousarray(honest(ctx, 9, 1, acc=acc)[0])
        fn = ctx.lib.halo_acc_decider_batch_mixed_fused if acc else ctx.lib.halo_pcdl_check_batch_mixed_fused
        st = (C.c_int * 2)(77, 77)
        ds, ps = (C.c_size_t * 2)(7, 511), (C.c_void_p * 2)(x.ctypes.data, y.ctypes.data)
        assert fn(ctx.h, None, ps, 2, None, st) == E
        assert fn(ctx.h, ds, None, 2, None, st) == E
        assert fn(ctx.h, ds, (C.c_void_p * 2)(x.ctypes.data, None), 2, None, st) == E
        assert list(st) == [77, 77]
        # d + 1 not a power of two; a blob whose d word, or whose proof's lg word, disagrees with ds[i]
        assert fused(ctx, [x, y], acc, ds=[7, 510]) == exact(ctx, [x, y], acc, ds=[7, 510]) == (REJECT, [77, 77], "d+1 is not a power of 2!")
        assert fused(ctx, [x, y], acc, ds=[7, 255]) == (REJECT, [77, 77], "d_i != d")
        assert fused(ctx, [x, y], acc, ds=[511, 7]) == (REJECT, [77, 77], "d_i != d")
        other = y.copy()
        other[22] = 8
        assert fused(ctx, [x, other], acc) == (REJECT, [77, 77], "d_i != d")
        assert fused(ctx, [x, y], acc) == (0, [0, 0], "")


def test_without_staging_the_exact_path_runs(hal, ctx):
    blobs = interleave(honest(ctx, 3, 3), honest(ctx, 9, 3))
    blobs[2] = cc.tamper(blobs[2], 3, "v")
    blobs[3] = cc.foreign(hal, 9, [0x7E5A])[0]
    want = exact(ctx, blobs)
    assert want == mt.by_single_calls(ctx, blobs) and want[1] == [0, 0, REJECT, REJECT, 0, 0]
    hal._lib.dev_hook("batch_stage_fail", 1)
    try:
        got, counts = cc.profiled(ctx, lambda: fused(ctx, blobs))
        ok, counts_ok = cc.profiled(ctx, lambda: fused(ctx, blobs[:2]))
    finally:
        hal._lib.dev_hook("reset", 0)
    assert got == want and ran_exact_only(counts), counts
    assert ok == (0, [0, 0], "") and ran_exact_only(counts_ok), counts_ok
    assert fused(ctx, blobs) == want


# ------------------------------------------------------------------ 7. the table pipeline as the key's MSM
def test_the_table_pipeline_is_the_keys_msm(hal, big, big_members):
    long_one, short = big_members
    blobs = accepted_alone(big, [short[0], long_one, short[1], short[2]])  # (the first MSM of 2^20 points builds the key's table)
    (rc, st, _), counts = cc.profiled(big, lambda: fused(big, blobs))
    assert rc == 0 and st == [0] * 4 and ran_relation_only(counts), counts
    assert counts.get("k_tmsm_recode", 0) == 1 and counts.get("k_mixed_terms", 0) == 1, "the key's MSM through the table pipeline: %r" % counts
    bad = list(blobs)
    bad[2] = cc.tamper(bad[2], 10, "v")
    want = exact(big, bad)
    assert want[1] == [0, 0, REJECT, 0] and want[2] == "instance 2: " + mt.single(big, bad[2])[1]
    assert fused(big, bad) == want
