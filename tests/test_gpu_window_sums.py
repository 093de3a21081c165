"""The MSM's window sums over keys of small multiples of one point (tests/window_cases.py): every record the launch leaves for the
host's combination is read back through halo_dev_msm_window_sums and compared, exactly, with m G for the integer m its definition
gives.  The bucket values are planted so that the additions behind the bucket kernel -- k_msm_combine, k_msm_reduce1, k_smsm_reduce,
k_smsm_final, k_msm_reduce_rc, k_rc_mid, the host's msm_combine_member -- meet equal, opposite and infinite operands at their every
level.  Each launch first asserts, through halo_dev_msm_last_plan, that it took the plan its case was built for; it runs three times
(plain, captured into a graph, replayed) with identical read-backs, and its result is the oracle's, limb for limb."""
import numpy as np
import pytest

import orc
import table_cases as tc
import window_cases as wc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hal():
    import halo_accumulation_amd as h
    return h._lib


def reset_knobs(c):
    c.set_small_path(-1)
    c.set_window_bits(0)
    c.set_reduce_span(0)
    c.set_task_len(0)
    c.set_sort_mode(-1)
    c.set_table_mode(-1)


def assert_plan(got, want):
    """the fields of halo_dev_msm_last_plan the case was built for"""
    diff = {k: (got[k], v) for k, v in want.items() if got[k] != v}
    assert not diff, "the launch took another plan (field: got, expected): %s" % diff


def run_three_times(c, key, scalars, want_plan, values, cases=None, off=0, same_words=True):
    """one scalar array through halo_msm_dev three times: plan, read-back, window sums, final point.  same_words = False: the order
    of the entries inside a multi-task bucket is the sort's atomics', and with it the Jacobian representation of a record -- the three
    read-backs are then compared as points"""
    import torch
    sc = tc.scalar_words(scalars)
    d = torch.from_numpy(sc.view(np.int64)).cuda()
    reads, results = [], []
    for _ in range(3):  # a plain launch, its capture into a graph, the replay
        results.append(c.msm_dev(d.data_ptr(), len(scalars), off=off, mont=False).tolist())
        plan = c.msm_last_plan(0)
        assert_plan(plan, want_plan)
        reads.append(c.msm_window_sums(0))
    for rd in reads if not same_words else reads[:1]:
        bad = wc.check_window_sums(rd, plan, values, cases)
        assert not bad, wc.describe(bad)
    if same_words:
        assert reads[0].tolist() == reads[1].tolist() == reads[2].tolist(), "plain launch, capture and replay left different records"
    else:
        same = [[orc.point_canonical(r) for r in rd] for rd in reads]
        assert same[0] == same[1] == same[2], "plain launch, capture and replay left different points"
    assert results[0] == results[1] == results[2]
    assert results[0] == orc.msm_affine(np.ascontiguousarray(key[off:off + len(scalars)]), tc.scalar_mont(scalars)).tolist()
    return plan


def plan_fields(plan, kmax):
    return dict(pipeline=plan["pipeline"], form=plan["form"], c=plan["c"], W=plan["W"], B=plan["B"], members=1, kmax=kmax, L=plan["L"],
                logL=plan["logL"], nseg=plan["nseg"], live_seg=plan["live_seg"])


# ---------------------------------------------------------------------------------------------------- general pipeline
@pytest.mark.parametrize("c,span", wc.GENERAL_PLANS)
def test_general_pipeline_every_site_and_class(hal, c, span):
    """k_msm_reduce1 + k_smsm_final: one window per (site, class) of the plan (window_cases.build_cases), W - 1 windows a launch"""
    plan, bg, cases = wc.build_cases(c, span)
    ks, launches = wc.pack_launches(plan, bg, cases)
    assert len(ks) <= 4096
    key = wc.multiples_key(len(ks), ks)
    ctx = hal.Context(key)
    try:
        ctx.set_small_path(0)
        ctx.set_window_bits(c)
        ctx.set_reduce_span(span)
        for launch in launches:
            run_three_times(ctx, key, launch.scalars, plan_fields(plan, 8), launch.values, launch.cases)
    finally:
        reset_knobs(ctx)
        ctx.close()


@pytest.mark.parametrize("span,L,nseg", wc.REDUCE1_SPANS)
def test_general_pipeline_at_2_15_buckets_per_window(hal, span, L, nseg):
    """k_msm_reduce1 + k_smsm_final at c = 16, the plan of every table-free MSM of 2^20 points or more: 8 buckets per lane and 64
    segments, and under reduce span 64 the reverse -- equal and opposite lane sums and segment sums at every level of both scans"""
    launch = wc.reduce1_launch(span)
    assert (launch.plan["L"], launch.plan["nseg"]) == (L, nseg)
    for kern, live in ((wc.K_REDUCE1, 64), (wc.K_FINAL, nseg)):
        off = 1
        while off < live:
            for cl in ("P+P", "P-P"):
                assert launch.counts.get((kern, "scan/%d" % off, cl), 0), (kern, off, cl)
            off <<= 1
    key = wc.multiples_key(len(launch.ks), launch.ks)
    ctx = hal.Context(key)
    try:
        ctx.set_small_path(0)
        ctx.set_window_bits(wc.REDUCE1_C)
        ctx.set_reduce_span(span)
        run_three_times(ctx, key, launch.scalars, plan_fields(launch.plan, 8), launch.values)
    finally:
        reset_knobs(ctx)
        ctx.close()


@pytest.mark.parametrize("sort_mode", [0, 1])
def test_combine_equal_opposite_and_infinite_partials(hal, sort_mode):
    """k_msm_combine under a task length of 8: buckets of 2, 8, 9, 64 and 65 equal tasks, the two-task P-P bucket, a cancellation at
    every level of the wave's tree, two infinite partials; both sorts write their own lists of multi-task buckets"""
    launch = wc.combine_launch()
    key = wc.multiples_key(len(launch.ks), launch.ks)
    ctx = hal.Context(key)
    try:
        ctx.set_small_path(0)
        ctx.set_window_bits(launch.plan["c"])
        ctx.set_task_len(wc.COMBINE_KMAX)
        ctx.set_sort_mode(sort_mode)
        run_three_times(ctx, key, launch.scalars, plan_fields(launch.plan, wc.COMBINE_KMAX), launch.values, same_words=False)
    finally:
        reset_knobs(ctx)
        ctx.close()


@pytest.mark.parametrize("c", [7, 13])
def test_horner_over_equal_opposite_and_empty_window_sums(hal, c):
    """msm_combine_member's Horner: a window sum equal to the doubled accumulator, opposite to it, the skipped doublings behind"""
    launch = wc.horner_launch(c)
    for cl in wc.EDGE:
        assert launch.counts.get((wc.K_HOST, "horner", cl), 0) >= 1
    key = wc.multiples_key(len(launch.ks), launch.ks)
    ctx = hal.Context(key)
    try:
        ctx.set_small_path(0)
        ctx.set_window_bits(c)
        run_three_times(ctx, key, launch.scalars, plan_fields(launch.plan, 8), launch.values)
    finally:
        reset_knobs(ctx)
        ctx.close()


# ---------------------------------------------------------------------------------------------------- small pipeline
@pytest.mark.parametrize("c,span", wc.SMALL_PLANS)
def test_small_pipeline_every_site_and_class(hal, c, span):
    """k_smsm_reduce (+ k_smsm_final over more than one segment) on the default path: one window per (site, class) of the plan"""
    plan, bg, cases = wc.build_cases(c, span, 1)
    ks, launches = wc.pack_launches(plan, bg, cases)
    assert len(ks) <= 1 << 14
    key = wc.multiples_key(len(ks), ks)
    ctx = hal.Context(key)
    try:
        ctx.set_window_bits(c)
        ctx.set_reduce_span(span)
        for launch in launches:
            run_three_times(ctx, key, launch.scalars, plan_fields(plan, 8), launch.values, launch.cases)
    finally:
        reset_knobs(ctx)
        ctx.close()


def test_small_pipeline_partial_loop_and_heavy_buckets(hal):
    """neighbouring quads of 1, 2 and 4 partials, the P-P pair of partials, a heavy bucket of 5 partials, two infinite partials"""
    launch = wc.partials_launch()
    for site, cl in (("partial", "P+P"), ("partial", "P-P"), ("partial", "Q+inf"), ("heavy tree/4", "P+P"), ("heavy strided", "inf+Q")):
        assert launch.counts.get((wc.K_SREDUCE, site, cl), 0) >= 1
    key = wc.multiples_key(len(launch.ks), launch.ks)
    ctx = hal.Context(key)
    try:
        ctx.set_window_bits(launch.plan["c"])
        run_three_times(ctx, key, launch.scalars, plan_fields(launch.plan, 8), launch.values, same_words=False)
    finally:
        reset_knobs(ctx)
        ctx.close()


# ---------------------------------------------------------------------------------------------------- table plans
NO_TABLE, FIXED, SLIDING = 0, 1, 22  # halo_ctx_info(ctx, 9): the plan of the launch enqueued last
SLIDE_PLAN = dict(pipeline=3, form=2, c=20, B=1 << 19, members=1, sets=1, pieces=1, kmax=16, lg_rows=9, lg_cols=10, per=16)
FIXED_PLAN = dict(SLIDE_PLAN, pipeline=2, W=13)


@pytest.fixture(scope="module")
def table_ctx(hal):
    """one context over the table key with the all-shifts table built (the sliding plan forced onto 4096 points)"""
    hal.dev_hook("table_slide_min", 4096)
    ks, _ = wc.table_key()
    key = wc.multiples_key(len(ks), ks)
    ctx = hal.Context(key)
    yield ctx, key
    reset_knobs(ctx)
    ctx.close()


def run_table(table_ctx, launch, want_plan, info9, same_words=True):
    import halo_accumulation_amd as h
    h._lib.dev_hook("table_slide_min", 4096)  # (tests/conftest.py resets the development hooks after every test)
    ctx, key = table_ctx
    run_three_times(ctx, key, launch.scalars, want_plan, [launch.values], [launch.cases] if launch.cases else None, same_words=same_words)
    assert ctx.info(9) == info9


def test_sliding_plan_rc_trees_equal_and_opposite(table_ctx):
    """k_msm_reduce_rc: equal and opposite lane sums at every level of the 32-lane column trees and the 64-lane row trees, equal and
    opposite cells inside a lane"""
    ks, launch, cells = wc.slide_structure_launch()
    rec = wc.IntRec()
    wc.model_reduce_rc(rec, cells, 9, 10, 16)
    for name, top in (("col", 16), ("row", 32)):
        off = top
        while off >= 1:
            for cl in wc.EDGE:
                assert rec.counts.get(("k_msm_reduce_rc", "%s tree/%d" % (name, off), cl), 0), (name, off, cl)
            off >>= 1
    run_table(table_ctx, launch, SLIDE_PLAN, SLIDING)


def test_sliding_plan_rc_mid_every_site_and_class(table_ctx):
    """k_rc_mid: every (site, class) of its block_weighted_sum in some block of 64 column sums or 64 row sums"""
    ks, launches = wc.slide_rc_mid_launches()
    for launch in launches:
        run_table(table_ctx, launch, SLIDE_PLAN, SLIDING)


def test_sliding_plan_host_combination_with_infinite_parts(table_ctx):
    """msm_combine_member: weighted == plain for the columns, for the rows, for both"""
    for name, launch in wc.slide_host_launches()[1]:
        run_table(table_ctx, launch, SLIDE_PLAN, SLIDING)
    for name, launch in wc.extra_host_launches()[1]:  # (cells of several points: buckets of several tasks)
        run_table(table_ctx, launch, SLIDE_PLAN, SLIDING, same_words=False)


def test_fixed_windows_on_the_same_table(table_ctx):
    """table mode 1: the fixed windows read rows 20 w of the same table and take the same row / column sums over the bucket index
    itself (k_msm_reduce_rc + k_rc_mid, the host's cols + 2^10 (rows - plain)): the same three families of cases"""
    ctx, key = table_ctx
    ctx.set_table_mode(1)
    try:
        launches = [wc.slide_structure_launch("fixed")[1]] + wc.slide_rc_mid_launches("fixed")[1] + [l for _, l in wc.slide_host_launches("fixed")[1]]
        for launch in launches:
            run_table(table_ctx, launch, FIXED_PLAN, FIXED)
        for name, launch in wc.extra_host_launches("fixed")[1]:
            run_table(table_ctx, launch, FIXED_PLAN, FIXED, same_words=False)
    finally:
        ctx.set_table_mode(-1)


# ---------------------------------------------------------------------------------------------------- small-key plan
@pytest.fixture(scope="module")
def small_ctx(hal):
    """one context over the table key tiled to 2^17 points: the c = 17 plan with its 256 x 256 row / column sums"""
    key = wc.small_key()
    ctx = hal.Context(key)
    yield ctx, key
    reset_knobs(ctx)
    ctx.close()


@pytest.mark.parametrize("members", [1, 4, 8])
def test_small_key_plan_one_member_and_batches(small_ctx, members):
    """k_msm_reduce_rc with 4, 8 and 16 buckets per lane (trees of 64, 32 and 16 lanes), k_rc_mid and the host's combination per set:
    one member, batches of 4 and 8 through the batch entry point, a member of zero scalars beside planted ones"""
    import torch
    ctx, key = small_ctx
    per, batches = wc.small_key_batches()[members]
    want = dict(pipeline=2, form=2, c=17, W=15, B=1 << 16, members=members, sets=members, pieces=1, kmax=16 if members == 1 else 64,
                lg_rows=8, lg_cols=8, per=per)
    n, head = wc.SMALL_KEY_N, wc.TABLE_N
    for batch in batches:
        assert len(batch) == members
        rec = wc.IntRec()
        for launch in batch:
            wc.model_reduce_rc(rec, {(b >> 8, b & 255): x for b, x in launch.values.items()}, 8, 8, per)
        sc = [np.concatenate([tc.scalar_words(l.scalars), np.zeros((n - head, 4), dtype=np.uint64)]) for l in batch]
        dev = [torch.from_numpy(a.view(np.int64)).cuda() for a in sc]
        reads, results = [], []
        for _ in range(3):  # a plain launch, its capture into a graph, the replay
            if members == 1:
                results.append([ctx.msm_dev(dev[0].data_ptr(), n, mont=False).tolist()])
            else:
                ctx.msm_dev_batch_begin(0, [d.data_ptr() for d in dev], n, mont=False)
                results.append(ctx.msm_dev_batch_end(0, members).tolist())
            plan = ctx.msm_last_plan(0)
            assert_plan(plan, want)
            assert ctx.info(9) == FIXED
            reads.append(ctx.msm_window_sums(0))
        assert reads[0].shape[0] == members * 16
        bad = wc.check_window_sums(reads[0], plan, [l.values for l in batch], [l.cases for l in batch])
        assert not bad, wc.describe(bad)
        assert reads[0].tolist() == reads[1].tolist() == reads[2].tolist() and results[0] == results[1] == results[2]
        for b, launch in enumerate(batch):
            assert results[0][b] == orc.msm_affine(np.ascontiguousarray(key[:head]), tc.scalar_mont(launch.scalars)).tolist(), b
        if any(not l.values for l in batch):  # the member of zero scalars: every pair of its set is the infinity
            e = [l.values for l in batch].index({})
            assert all(orc.point_canonical(r) is None for r in reads[0][16 * e:16 * e + 16])


def test_small_pipeline_heavy_bucket_of_70_partials(hal):
    """k_smsm_reduce's pre-sum with a partial in every quad and a second trip, then a cancellation at every level of its tree"""
    launch = wc.heavy_launch()
    for off in (32, 16, 8, 4, 2, 1):
        for cl in ("P+P", "P-P"):
            assert launch.counts.get((wc.K_SREDUCE, "heavy tree/%d" % off, cl), 0), (off, cl)
    for cl in ("P+P", "inf+Q", "Q+inf"):
        assert launch.counts.get((wc.K_SREDUCE, "heavy strided", cl), 0)
    key = wc.multiples_key(len(launch.ks), launch.ks)
    ctx = hal.Context(key)
    try:
        ctx.set_window_bits(launch.plan["c"])
        run_three_times(ctx, key, launch.scalars, plan_fields(launch.plan, 16), launch.values, same_words=False)
    finally:
        reset_knobs(ctx)
        ctx.close()


def test_small_pipeline_strided_loop_cancellation(hal):
    """128 partials in one bucket: every quad of the heavy pre-sum makes a second trip, and the one that holds the odd partial adds
    it to its opposite"""
    launch = wc.strided_launch()
    assert launch.counts.get((wc.K_SREDUCE, "heavy strided", "P-P")) == 2  # (counted with the odd partial first and last)
    assert launch.counts.get((wc.K_SREDUCE, "heavy strided", "P+P")) == 2 * 63
    key = wc.multiples_key(len(launch.ks), launch.ks)
    ctx = hal.Context(key)
    try:
        ctx.set_window_bits(launch.plan["c"])
        run_three_times(ctx, key, launch.scalars, plan_fields(launch.plan, 16), launch.values, same_words=False)
    finally:
        reset_knobs(ctx)
        ctx.close()


# ---------------------------------------------------------------------------------------------------- the two hooks
def test_plan_and_window_sum_hooks_misuse_is_reported(hal):
    """halo_dev_msm_last_plan / halo_dev_msm_window_sums: no launch yet, a slot that is not there, a slot in flight, a null pointer,
    too little room (the count still comes back) -- each refused with its message, nothing dereferenced"""
    import ctypes as C
    import torch
    n = 4096
    c = hal.Context(urs_n=n)
    lib = hal.load()
    try:
        for call in (lambda: c.msm_last_plan(0), lambda: c.msm_window_sums(0)):
            with pytest.raises(hal.HaloError, match="no launch"):
                call()
        for slot in (-1, 4, 99):
            with pytest.raises(hal.HaloError, match="slot out of range"):
                c.msm_last_plan(slot)
            with pytest.raises(hal.HaloError, match="slot out of range"):
                c.msm_window_sums(slot, cap=64)
        d = torch.empty(n * 4, dtype=torch.int64, device="cuda")
        c.rng_scalars_dev(0x77696E73756D, n, d.data_ptr())
        c.msm_dev_begin(1, d.data_ptr(), n)
        with pytest.raises(hal.HaloError, match="in flight"):
            c.msm_last_plan(1)
        with pytest.raises(hal.HaloError, match="in flight"):
            c.msm_window_sums(1, cap=64)
        with pytest.raises(hal.HaloError, match="no launch"):
            c.msm_last_plan(0)   # (another slot's launch is not this slot's)
        want = c.msm_dev_end(1).tolist()
        plan = c.msm_last_plan(1)
        assert plan["pipeline"] == 1 and plan["members"] == 1 and plan["W"] == wc.windows_of(plan["c"]) and plan["B"] == 1 << (plan["c"] - 1)
        sums = c.msm_window_sums(1)
        assert sums.shape == (plan["W"], 12)
        cnt = C.c_size_t(0)
        out = np.zeros((plan["W"], 12), dtype=np.uint64)
        with pytest.raises(hal.HaloError, match="room for fewer"):
            hal.check(lib.halo_dev_msm_window_sums(c.h, 1, hal.ptr(out), plan["W"] - 1, C.byref(cnt)))
        assert cnt.value == plan["W"] and not out.any()
        with pytest.raises(hal.HaloError, match="null pointer"):
            hal.check(lib.halo_dev_msm_window_sums(c.h, 1, None, plan["W"], C.byref(cnt)))
        with pytest.raises(hal.HaloError, match="null pointer"):
            hal.check(lib.halo_dev_msm_window_sums(c.h, 1, hal.ptr(out), plan["W"], None))
        with pytest.raises(hal.HaloError, match="null pointer"):
            hal.check(lib.halo_dev_msm_last_plan(c.h, 1, None))
        with pytest.raises(hal.HaloError):
            hal.check(lib.halo_dev_msm_last_plan(None, 1, (C.c_long * 16)()))
        # the records are the host's inputs: Horner over them is the result
        acc = None
        for w in range(plan["W"] - 1, -1, -1):
            for _ in range(plan["c"]):
                acc = wc.pm.add(acc, acc)
            acc = wc.pm.add(acc, orc.point_canonical(sums[w]))
        assert acc == orc.point_canonical(np.array(want, dtype=np.uint64))
        c.msm_dev(d.data_ptr(), 0)   # a launch of no points: no windows, no records
        assert c.msm_last_plan(0)["W"] == 0 and c.msm_window_sums(0).shape == (0, 12)
    finally:
        c.close()
