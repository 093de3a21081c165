"""halo_pcdl_check_batch_fused / halo_acc_decider_batch_fused on the GPU: the term kernel's scalars limb for limb against Python
integers; honest batches accepted by ONE relation with no per-member ladder and no per-member MSM (the profiler shows which path
ran); the left side cut into chunks and sequences; every kind of reject with the exact batch's statuses, code and message; a pair
of members whose unweighted defects cancel; company on the slots, the fallbacks, a multi-device context and the full-size key.
The pools of honest members and the helpers around them are those of tests/test_gpu_check_combined.py."""
import ctypes as C

import numpy as np
import pytest

import fused_cases as fc
import orc
import test_gpu_check_combined as cc

pytestmark = pytest.mark.gpu

R_MOD = fc.R_MOD


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
def small(hal):
    c = hal._lib.Context(urs_n=1 << 9)
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


def call(c, d, blobs, acc=False, fused=True, seed=None):
    """-> (return code, status list, message); status entries the call does not write stay 77"""
    m = len(blobs)
    qs = np.ascontiguousarray(np.concatenate(blobs))
    st = (C.c_int * m)(*([77] * m))
    if fused:
        fn = c.lib.halo_acc_decider_batch_fused if acc else c.lib.halo_pcdl_check_batch_fused
        rc = fn(c.h, d, ptr(qs), m, seed, st)
    else:
        fn = c.lib.halo_acc_decider_batch if acc else c.lib.halo_pcdl_check_batch
        rc = fn(c.h, d, ptr(qs), m, st)
    return rc, [st[i] for i in range(m)], (c.lib.halo_last_error().decode() if rc else "")


def ran_fused_only(counts):
    """the relation ran and nothing of the exact batch did: no ladder per member, no h expansion per member"""
    return counts.get("k_fused_terms", 0) == 1 and counts.get("k_batch_small_msm", 0) == 0 and counts.get("k_h_coeffs_batch", 0) == 0


def ran_fused_then_exact(counts):
    return counts.get("k_fused_terms", 0) == 1 and counts.get("k_h_coeffs_batch", 0) > 0


def ran_exact_only(counts):
    return counts.get("k_fused_terms", 0) == 0 and counts.get("k_h_coeffs_batch", 0) > 0


def chunked(hal, chunk, fn):
    hal._lib.dev_hook("check_fused_chunk", chunk)
    try:
        return fn()
    finally:
        hal._lib.dev_hook("reset", 0)


# ------------------------------------------------------------------ 1. the term kernel against integers
@pytest.mark.parametrize("lg", [1, 3, 9])
@pytest.mark.parametrize("M", [1, 2, 5, 64, 65])
def test_term_kernel_equals_python_integers(hal, ctx, lg, M):
    """M = 65: a second block with one live lane.  From 64 members on every special value of tests/fused_cases.py is among them"""
    mem = fc.members(lg, M, seed=M)
    assert len(mem) == M
    recs = np.ascontiguousarray(np.concatenate([m.record() for m in mem]))
    K = 2 * lg + 2
    sc, h = np.zeros((M, K, 4), dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    assert ctx.lib.halo_dev_check_fused_terms(ctx.h, ptr(recs), M, lg, ptr(sc), ptr(h)) == 0, ctx.lib.halo_last_error()
    bad = [(a,) + b for a, m in enumerate(mem) for b in fc.check_member(m, sc[a], None)]
    assert not bad, "%d wrong scalars; first (member, what, index): %s" % (len(bad), bad[:8])
    assert [int(w) for w in h] == fc.words(sum(m.share() for m in mem) % R_MOD), "H's scalar"


def test_term_kernel_argument_errors(hal, ctx):
    recs, sc, h = np.zeros(7 * 4, dtype=np.uint64), np.zeros(4 * 4, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    for M, lg in ((0, 1), (65536, 1), (1, 0), (1, 25)):
        assert ctx.lib.halo_dev_check_fused_terms(ctx.h, ptr(recs), M, lg, ptr(sc), ptr(h)) == hal._lib.HALO_E_ARG, (M, lg)
    assert ctx.lib.halo_dev_check_fused_terms(ctx.h, None, 1, 1, ptr(sc), ptr(h)) == hal._lib.HALO_E_ARG


# ------------------------------------------------------------------ 2. honest batches: one relation
@pytest.mark.parametrize("lg", [3, 8, 9, 14])
@pytest.mark.parametrize("m", [2, 5, 64, 65])
@pytest.mark.parametrize("acc", [False, True], ids=["pcdl", "decider"])
def test_honest_batches_are_accepted_by_the_fused_relation(hal, ctx, lg, m, acc):
    d = (1 << lg) - 1
    blobs = cc.pool(ctx, lg)[1 if acc else 0][:m]  # (members 1, 8, .. of the Instances are plain, the others hiding)
    (rc, st, _), counts = cc.profiled(ctx, lambda: call(ctx, d, blobs, acc))
    assert rc == 0 and st == [0] * m
    assert ran_fused_only(counts), counts
    assert counts.get("k_batch_to_affine", 0) == 1 and counts.get("k_fr_sum_rows", 0) >= 1, counts


@pytest.mark.parametrize("acc", [False, True], ids=["pcdl", "decider"])
def test_one_member_takes_the_exact_path(hal, ctx, acc):
    blobs = cc.pool(ctx, 9)[1 if acc else 0][:1]
    (rc, st, _), counts = cc.profiled(ctx, lambda: call(ctx, 511, blobs, acc))
    assert rc == 0 and st == [0]
    assert ran_exact_only(counts), counts
    # ... and so does a batch of which one member is left after the transcripts
    two = [blobs[0], cc.tamper(cc.pool(ctx, 9)[1 if acc else 0][1], 9, "U")]
    got, counts = cc.profiled(ctx, lambda: call(ctx, 511, two, acc))
    assert got == call(ctx, 511, two, acc, fused=False) and got[1] == [0, hal._lib.HALO_E_REJECT]
    assert ran_exact_only(counts), counts


def test_degree_bound_zero_takes_the_exact_path(hal, ctx):
    """d = 0: a constant, nothing to fuse.  Two blobs of an Instance's length at lg = 0 with d and the proof length in place"""
    W = int(ctx.lib.halo_instance_words(0))
    rng = np.random.default_rng(5)
    blobs = []
    for _ in range(2):
        q = rng.integers(0, 1 << 62, size=W, dtype=np.uint64)
        q[12], q[22] = 0, 0
        blobs.append(q)
    got, counts = cc.profiled(ctx, lambda: call(ctx, 0, blobs))
    assert got == call(ctx, 0, blobs, fused=False) and got[0] != 0
    assert counts.get("k_fused_terms", 0) == 0, counts


def test_python_wrappers(hal, ctx):
    from halo_accumulation_amd import acc as A, pcdl
    qs, accs = cc.pool(ctx, 9)
    assert pcdl.check_batch_fused(ctx, 511, qs[:5]) == [0] * 5
    assert A.decider_batch_fused(ctx, 511, accs[:5], seed=bytes(range(32))) == [0] * 5
    with pytest.raises(hal._lib.HaloReject) as e:
        pcdl.check_batch_fused(ctx, 511, [qs[0], cc.tamper(qs[1], 9, "v"), qs[2]])
    assert e.value.args[1] == [0, hal._lib.HALO_E_REJECT, 0]
    with pytest.raises(ValueError):
        pcdl.check_batch_fused(ctx, 511, qs[:2], seed=b"short")
    with pytest.raises(ValueError):
        A.decider_batch_fused(ctx, 511, accs[:2], seed=b"short")


# ------------------------------------------------------------------ 3. the left side in chunks and sequences
def test_left_side_in_chunks_and_sequences(hal, small):
    """The 2^9-point key, 65 members at lg = 9: T = 65 x 20 + 1 = 1301 terms.  The key's size cuts them into 3 chunks (one launch
    sequence); 64 terms a chunk into 21 (three sequences of at most 8); 100 a chunk into 13 and a last one of H alone"""
    lg, d, m = 9, 511, 65
    blobs = list(cc.pool(small, lg)[0][:m])
    bad = list(blobs)
    bad[40] = cc.foreign(hal, lg, [0xF09])[0]
    want_bad = call(small, d, bad, fused=False)
    assert [i for i, s in enumerate(want_bad[1]) if s] == [40]
    T = m * (2 * lg + 2) + 1
    for chunk, size in ((0, 512), (64, 64), (100, 100)):
        chunks = -(-T // size)
        seqs = -(-chunks // 8)
        (rc, st, _), counts = cc.profiled(small, lambda: chunked(hal, chunk, lambda: call(small, d, blobs)))
        assert rc == 0 and st == [0] * m and ran_fused_only(counts), (chunk, counts)
        assert counts.get("k_msm_recode", 0) in (seqs, seqs + 1), "%d chunks in %d sequences (and the key's MSM): %r" % (chunks, seqs, counts)
        assert chunked(hal, chunk, lambda: call(small, d, bad)) == want_bad, chunk
    assert T % 100 == 1, "the last chunk of 100 is H alone"
    # the decider form, and a chunk size above the key's (clamped to it)
    accs = cc.pool(small, lg)[1][:m]
    assert chunked(hal, 100, lambda: call(small, d, accs, acc=True)) == (0, [0] * m, "")
    assert chunked(hal, 1 << 20, lambda: call(small, d, blobs[:9])) == (0, [0] * 9, "")


# ------------------------------------------------------------------ 4. rejects equal the exact batch
@pytest.mark.parametrize("lg", [3, 9])
def test_structure_rejects_stay_out_of_the_relation(hal, ctx, lg):
    """a flipped bit of C, U or the last round's L leaves the curve: rejected with the transcripts, and the honest rest is still
    accepted by the fused relation"""
    d = (1 << lg) - 1
    blobs = list(cc.pool(ctx, lg)[0][:12])
    for i, what in zip((0, 4, 11), ("C", "U", "L")):
        blobs[i] = cc.tamper(blobs[i], lg, what)
    want = call(ctx, d, blobs, fused=False)
    assert [i for i, s in enumerate(want[1]) if s] == [0, 4, 11] and want[2].startswith("instance 0: ")
    got, counts = cc.profiled(ctx, lambda: call(ctx, d, blobs))
    assert got == want
    assert ran_fused_only(counts), "the nine honest members are accepted by one relation: %r" % counts


@pytest.mark.parametrize("lg", [3, 9])
def test_relation_rejects_get_the_exact_statuses(hal, ctx, lg):
    """a flipped bit of v or c keeps the transcript valid and breaks pcdl.rs:307-310: the relation fails, the exact batch decides"""
    d = (1 << lg) - 1
    for where, whats in (((0, 4, 7, 9, 11), ("v", "C", "L", "U", "c")), ((5,), ("c",)), ((11,), ("v",))):
        blobs = list(cc.pool(ctx, lg)[0][:12])
        for i, what in zip(where, whats):
            blobs[i] = cc.tamper(blobs[i], lg, what)
        want = call(ctx, d, blobs, fused=False)
        assert [i for i, s in enumerate(want[1]) if s] == list(where) and want[2].startswith("instance %d: " % where[0])
        got, counts = cc.profiled(ctx, lambda: call(ctx, d, blobs))
        assert got == want, where
        assert ran_fused_then_exact(counts), counts
    accs = list(cc.pool(ctx, lg)[1][:6])
    accs[2] = cc.tamper(accs[2], lg, "v")
    assert call(ctx, d, accs, acc=True) == call(ctx, d, accs, acc=True, fused=False)


@pytest.mark.parametrize("where", [[0], [3], [6], [2, 5]])
def test_msm_rejects_get_the_exact_statuses(hal, ctx, where):
    lg, d = 9, 511
    blobs = list(cc.pool(ctx, lg)[0][:7])
    for i, q in zip(where, cc.foreign(hal, lg, [900 + i for i in where])):
        blobs[i] = q
    want = call(ctx, d, blobs, fused=False)
    assert [i for i, s in enumerate(want[1]) if s] == where and want[0] == hal._lib.HALO_E_REJECT
    assert want[2] == "instance %d: U != CM.Commit(ck, h_vec)" % where[0]
    got, counts = cc.profiled(ctx, lambda: call(ctx, d, blobs))
    assert got == want
    assert ran_fused_then_exact(counts), counts
    accs = list(cc.pool(ctx, lg)[1][:7])
    for i in where:
        accs[i] = np.concatenate([blobs[i], accs[i][len(blobs[i]):]])  # (the decider checks the Instance prefix)
    assert call(ctx, d, accs, acc=True) == call(ctx, d, accs, acc=True, fused=False)


def test_both_kinds_of_defect_in_one_batch(hal, ctx):
    lg, d = 9, 511
    blobs = list(cc.pool(ctx, lg)[0][:8])
    blobs[1] = cc.tamper(blobs[1], lg, "c")        # the succinct relation alone
    blobs[6] = cc.foreign(hal, lg, [0xB07])[0]     # the MSM alone
    want = call(ctx, d, blobs, fused=False)
    assert [i for i, s in enumerate(want[1]) if s] == [1, 6]
    assert "C_(log_n)" in want[2]
    assert call(ctx, d, blobs) == want
    assert call(ctx, d, blobs, seed=bytes(range(7, 39))) == want


def test_cancelling_pair_is_rejected(hal, ctx):
    """The pair of tests/test_gpu_check_combined.py: one instance opened under a key whose G_0 is G_0 + G_1, one under G_0 - G_1.
    Each has F = U - <h, G> = +-G_1 and E = 0, so the relation with every s_a ONE would accept the pair.  The hashed weights must
    not."""
    from halo_accumulation_amd import acc as A
    from halo_accumulation_amd._lib import point_sum
    lg, d, n = 8, 255, 256
    gs = ctx.read_bases(0, n)
    g0, g1 = cc.to_jac(gs[0]), cc.to_jac(gs[1])
    neg_g1 = g1.copy()
    neg_g1[4:8] = cc.limbs(cc.P_MOD - cc.to_int(g1[4:8]))  # -y on the Montgomery limbs
    pair = []
    for k, shift in enumerate((g1, neg_g1)):
        key = gs.copy()
        key[0] = cc.affine_of(point_sum(np.stack([g0, shift])))
        other = hal._lib.Context(np.ascontiguousarray(key))
        try:
            pair.append(A.random_instance(other, [0xCA9CE1 + k], d))
        finally:
            other.close()
    want = call(ctx, d, pair, fused=False)
    assert want[1] == [hal._lib.HALO_E_REJECT] * 2 and "U != CM.Commit" in want[2]
    got, counts = cc.profiled(ctx, lambda: call(ctx, d, pair))
    assert got == want and ran_fused_then_exact(counts), counts
    assert call(ctx, d, pair, seed=bytes(range(32))) == want
    honest = cc.pool(ctx, lg)[0]
    mixed = [honest[0], pair[0], honest[1], pair[1], honest[2]]
    assert call(ctx, d, mixed) == call(ctx, d, mixed, fused=False)
    assert call(ctx, d, mixed, seed=bytes(range(32))) == call(ctx, d, mixed, fused=False)


# ------------------------------------------------------------------ 5. company and fallbacks
def test_without_staging_the_exact_path_runs(hal, ctx):
    lg, d = 9, 511
    blobs = list(cc.pool(ctx, lg)[0][:6])
    blobs[2] = cc.tamper(blobs[2], lg, "v")
    blobs[4] = cc.foreign(hal, lg, [977])[0]
    want = call(ctx, d, blobs, fused=False)
    hal._lib.dev_hook("batch_stage_fail", 1)
    try:
        got, counts = cc.profiled(ctx, lambda: call(ctx, d, blobs))
        ok, counts_ok = cc.profiled(ctx, lambda: call(ctx, d, blobs[:2]))
    finally:
        hal._lib.dev_hook("reset", 0)
    assert got == want and ran_exact_only(counts), counts
    assert ok == (0, [0, 0], "") and ran_exact_only(counts_ok), counts_ok


def test_beside_a_callers_msms(hal, ctx):
    import torch
    lg, d = 9, 511
    blobs = list(cc.pool(ctx, lg)[0][:9])
    bad = list(blobs)
    bad[3] = cc.foreign(hal, lg, [0x51D])[0]
    want_bad = call(ctx, d, bad, fused=False)
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
                return call(ctx, d, blobs), call(ctx, d, bad)
            finally:
                for slot in held:
                    got.append(ctx.msm_dev_end(slot))

        ((rc, st, _), rejected), counts = cc.profiled(ctx, beside)
        assert rc == 0 and st == [0] * 9 and counts.get("k_fused_terms", 0) == 2, (held, counts)
        assert rejected == want_bad, held
        assert all(g.tolist() == expect for g in got), "the caller's MSMs kept their own results"
    assert call(ctx, d, blobs) == (0, [0] * 9, "")
    assert call(ctx, d, blobs) == (0, [0] * 9, ""), "and again (the second call replays its launch graphs)"
    for slot in range(4):
        ctx.msm_dev_begin(slot, dev.data_ptr(), n)
    try:
        busy = call(ctx, d, blobs)
        busy_exact = call(ctx, d, blobs, fused=False)
    finally:
        for slot in range(4):
            assert ctx.msm_dev_end(slot).tolist() == expect
    assert busy == busy_exact and busy[0] == hal._lib.HALO_E_ARG and busy[1] == [77] * 9, "no idle slot"


def test_multi_device_context_and_a_seed(hal, ctx):
    lg, d = 9, 511
    blobs = list(cc.pool(ctx, lg)[0][:8])
    blobs[5] = cc.foreign(hal, lg, [988])[0]
    want = call(ctx, d, blobs, fused=False)
    seed = bytes(range(100, 132))
    assert call(ctx, d, blobs, seed=seed) == want
    assert call(ctx, d, blobs[:5], seed=seed) == (0, [0] * 5, "")
    m = hal._lib.Context(urs_n=1 << 14, devices=[0, 0])
    try:
        assert call(m, d, blobs) == want
        (rc, st, _), counts = cc.profiled(m, lambda: call(m, d, blobs[:5]))
        assert rc == 0 and st == [0] * 5 and ran_fused_only(counts), counts
    finally:
        m.close()


def test_argument_errors_are_the_exact_batchs(hal, ctx):
    d = 511
    q = cc.pool(ctx, 9)[0][0]
    st = (C.c_int * 2)(77, 77)
    for fn in (ctx.lib.halo_pcdl_check_batch_fused, ctx.lib.halo_acc_decider_batch_fused):
        assert fn(ctx.h, d, None, 2, None, st) == hal._lib.HALO_E_ARG
        assert fn(ctx.h, d, None, 0, None, None) == 0
    assert [st[0], st[1]] == [77, 77]
    other = q.copy()
    other[12] = 255
    assert call(ctx, d, [q, other]) == call(ctx, d, [q, other], fused=False)
    assert call(ctx, d, [q, other])[1] == [77, 77], "rejected before any work, status untouched"
    assert call(ctx, 510, [q, q]) == call(ctx, 510, [q, q], fused=False)
    qs = np.ascontiguousarray(np.concatenate([q, q]))
    assert ctx.lib.halo_pcdl_check_batch_fused(ctx.h, d, ptr(qs), 2, None, None) == 0, "status is nullable"


# ------------------------------------------------------------------ 6. full size, once
def test_full_size(hal, big):
    from halo_accumulation_amd import acc as A
    lg = 20
    d = (1 << lg) - 1
    honest = A.random_instance_batch(big, [0xF0115], d, 3)
    (rc, st, _), counts = cc.profiled(big, lambda: call(big, d, honest))
    assert rc == 0 and st == [0] * 3 and ran_fused_only(counts), counts
    blobs = honest[:2] + cc.foreign(hal, lg, [0xF0E16], size=1 << 20) + honest[2:]
    want = call(big, d, blobs, fused=False)
    assert want[1] == [0, 0, hal._lib.HALO_E_REJECT, 0]
    assert call(big, d, blobs) == want
