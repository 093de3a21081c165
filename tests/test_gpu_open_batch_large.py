"""The batched opens, Instances and provers at 2^17 and 2^18 points (the prover at 2^15, one open batch at 2^19), once
each: the default switch, contexts of 2^17, 2^18 and 2^19 URS points.  Every word, status and the final RNG state against the loop
over the single calls.  A size takes the folded schedule by default where the measurements routed it (profiles/r18_*_batch_fold.json: every row of the size won);
elsewhere the hook "open_batch_fold" forces it, and the default is the loop (halo_ctx_info(10) == 0).  The fold kernels at the
shapes these sizes bring: 4 members x 2^15 and x 2^16 outputs from the context's key, 2^14 and 2^15 outputs from per-member keys in
place."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import orc
import test_gpu_open_batch_fold as ob
import test_gpu_open_dev_batch as od
import test_gpu_prover_batch as pb

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def routed(kind, lg):
    """did the measurements route this size?  Every row of it won (the rule of DESIGN.md 4.5), and nothing holds it back"""
    with open(os.path.join(ROOT, "profiles", "r18_%s_batch_fold.json" % kind)) as f:
        doc = json.load(f)
    rows = [r for r in doc["rows"] if r["n"] == 1 << lg]
    return bool(rows) and all(r["won"] for r in rows) and (1 << lg) not in doc.get("held_back_n", [])


@pytest.fixture(scope="module")
def hal():
    import halo_accumulation_amd as h
    return h


@pytest.fixture(scope="module")
def ctx17(hal):
    c = hal._lib.Context(urs_n=1 << 17)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx18(hal):
    c = hal._lib.Context(urs_n=1 << 18)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def hooks_reset(hal):
    yield
    hal._lib.dev_hook("reset", 0)


def schedule(hal, kind, lg):
    """the folded schedule for the call that follows: by default where routed, else forced"""
    if not routed(kind, lg):
        hal._lib.dev_hook("open_batch_fold", 1)


def test_fold_steps_of_the_sizes():
    assert [ob.fold_steps(lg, 14) for lg in (15, 16, 17, 18, 19)] == [[1], [2], [2, 1], [2, 2], [2, 2, 1]]


def test_random_instance_batch_2_17(hal, ctx17):
    lg, m = 17, 5  # a group of 4 and a group of 1
    d = (1 << lg) - 1
    st = C.c_uint64(0x4A4D17)
    want = np.zeros((m, ctx17.lib.halo_instance_words(lg)), dtype=np.uint64)
    for i in range(m):
        assert ctx17.lib.halo_random_instance(ctx17.h, C.byref(st), d, ob.ptr(want[i])) == 0
    schedule(hal, "open", lg)
    got = np.zeros_like(want)
    st2 = C.c_uint64(0x4A4D17)
    assert ctx17.lib.halo_random_instance_batch(ctx17.h, C.byref(st2), d, m, ob.ptr(got)) == 0, ctx17.lib.halo_last_error()
    assert ctx17.info(10) == m
    assert got.tolist() == want.tolist() and st2.value == st.value


def test_default_route_follows_the_measurements(hal, ctx17):
    """no hook: member-batched where the size was routed, else one member at a time"""
    lg, m = 17, 2
    d = (1 << lg) - 1
    got = np.zeros((m, ctx17.lib.halo_instance_words(lg)), dtype=np.uint64)
    st = C.c_uint64(5)
    assert ctx17.lib.halo_random_instance_batch(ctx17.h, C.byref(st), d, m, ob.ptr(got)) == 0
    assert ctx17.info(10) == (m if routed("open", lg) else 0)


def test_plain_open_batch_2_17(hal, ctx17):
    """m = 3: a full polynomial, the zero polynomial and a constant"""
    lg = 17
    ps, Cs, zs, ws = ob.members(ctx17, lg, 3, False, 0xB17)
    assert not ps[1].any() and ps[2][0].any() and not ps[2][1:].any()
    schedule(hal, "open", lg)
    ob.expect_like_loop(ctx17, 0xB17, (1 << lg) - 1, ps, Cs, zs, ws, batched=3)


def test_instances_from_device_rows_2_17(hal, ctx17):
    """m = 2 from zero-padded device rows: a short polynomial at full length, a full one"""
    lg, m = 17, 2
    d = (1 << lg) - 1
    ps, _, zs, ws = ob.members(ctx17, lg, m, True, 0xD17)
    ps = ps[::-1].copy()  # (member 0 short, member 1 at full degree)
    assert od.degree(ps[0]) < d and od.degree(ps[1]) == d
    want = od.instance_batch(ctx17, 0xD17, d, ps, zs, ws)  # (the loop's words: one member at a time unless routed)
    loop = np.zeros_like(want[1])
    st = C.c_uint64(0xD17)
    for i in range(m):
        assert ctx17.lib.halo_instance_from_poly(ctx17.h, C.byref(st), ob.ptr(ps[i]), d + 1, d, ob.ptr(zs[i]), ob.ptr(ws[i]), ob.ptr(loop[i])) == 0
    assert want[0] == 0 and want[1].tolist() == loop.tolist() and want[3] == st.value
    schedule(hal, "open", lg)
    got = od.instance_dev_batch(ctx17, 0xD17, d, od.DevRows(ps), [d + 1] * m, zs, ws)
    assert ctx17.info(10) == m
    od.same(got, want, "device rows")


def test_hiding_open_batch_2_18(hal, ctx18):
    lg = 18
    ps, Cs, zs, ws = ob.members(ctx18, lg, 2, True, 0xB18)
    schedule(hal, "open", lg)
    ob.expect_like_loop(ctx18, 0xB18, (1 << lg) - 1, ps, Cs, zs, ws, batched=2)


@pytest.mark.parametrize("lg", [15, 17])
def test_prover_batch(hal, ctx17, lg):
    """k = 2 with 2 and 1 instances"""
    d = (1 << lg) - 1
    two = pb.step_members(hal, ctx17, lg, 2)
    members = [two[0], [two[1][1]]]
    schedule(hal, "prover", lg)
    _, status, _, _ = pb.expect_like_loop(ctx17, d, members, 0xACC0 + lg)
    assert status == [0, 0] and ctx17.info(10) == 2


def test_fold_kernels_at_the_new_shapes(hal, ctx17):
    """levels 2 from the context's key, 4 members x 2^15 outputs (form 0: two outputs per lane, 64 blocks a member); levels 1 from
    per-member keys in place, 2^14 outputs each (form 0: one per lane) -- against the single hook member by member"""
    sc, _ = orc.rng_scalars(0xF01D17, 4 * 3)
    single = [ctx17.fold_points(None, 2, sc[3 * b: 3 * b + 3]) for b in range(4)]
    got = ctx17.fold_points_batch(None, 2, sc, 4, shared=True, form=0)
    assert got.shape[1] == 1 << 15
    for b in range(4):
        assert np.array_equal(got[b], single[b]), b
    key = ctx17.read_bases(0, 1 << 15)
    own = np.concatenate([np.roll(key, 17 * b, axis=0) for b in range(4)])
    got = ctx17.fold_points_batch(own, 1, sc[:4], 4, shared=False, form=0)
    assert got.shape[1] == 1 << 14
    for b in range(4):
        assert np.array_equal(got[b], ctx17.fold_points(np.roll(key, 17 * b, axis=0), 1, sc[b: b + 1])), b


def test_fold_kernels_at_the_shapes_of_2_18_and_2_19(hal, ctx17, ctx18):
    """form 0 again: 4 members x 2^16 outputs from the context's key (2^18's first step: two outputs per lane, 128 blocks a member);
    levels 2 from per-member keys in place, 4 x 2^14 outputs (2^18's second step: one per lane) and 4 x 2^15 (2^19's second step: two
    per lane, each lane reading j, j + half and their partners and writing j and j + half)"""
    sc, _ = orc.rng_scalars(0xF01D18, 4 * 3)
    got = ctx18.fold_points_batch(None, 2, sc, 4, shared=True, form=0)
    assert got.shape[1] == 1 << 16
    for b in range(4):
        assert np.array_equal(got[b], ctx18.fold_points(None, 2, sc[3 * b: 3 * b + 3])), b
    for lg in (16, 17):
        key = ctx17.read_bases(0, 1 << lg)
        own = np.concatenate([np.roll(key, 17 * b, axis=0) for b in range(4)])
        got = ctx17.fold_points_batch(own, 2, sc, 4, shared=False, form=0)
        assert got.shape[1] == 1 << (lg - 2)
        for b in range(4):
            assert np.array_equal(got[b], ctx17.fold_points(np.roll(key, 17 * b, axis=0), 2, sc[3 * b: 3 * b + 3])), (lg, b)


def test_hiding_open_batch_2_19(hal):
    """the largest batched size, a group of 4: fold steps [2, 2, 1], the second over 2^17-point staged keys (the general MSM pipeline
    with one base offset per member)"""
    lg = 19
    c = hal._lib.Context(urs_n=1 << lg)
    try:
        ps, Cs, zs, ws = ob.members(c, lg, 4, True, 0xB19)
        schedule(hal, "open", lg)
        ob.expect_like_loop(c, 0xB19, (1 << lg) - 1, ps, Cs, zs, ws, batched=4)
    finally:
        c.close()


def test_memory_refusal_falls_back_to_the_loop(hal):
    """a budget below one slot's staging at 2^17 (one member: 28 MiB of vectors, 4 MiB of key): the loop's words, no error"""
    lg, m = 17, 2
    d = (1 << lg) - 1
    c = hal._lib.Context(urs_n=1 << lg)
    budget = c.info(3)
    try:
        want = np.zeros((m, c.lib.halo_instance_words(lg)), dtype=np.uint64)
        st = C.c_uint64(0x8EF)
        for i in range(m):
            assert c.lib.halo_random_instance(c.h, C.byref(st), d, ob.ptr(want[i])) == 0
        c.set_memory_budget(c.info(4) + (16 << 20))
        hal._lib.dev_hook("open_batch_fold", 1)
        got = np.zeros_like(want)
        st2 = C.c_uint64(0x8EF)
        assert c.lib.halo_random_instance_batch(c.h, C.byref(st2), d, m, ob.ptr(got)) == 0, c.lib.halo_last_error()
        assert c.info(10) == 0
        assert got.tolist() == want.tolist() and st2.value == st.value
    finally:
        c.set_memory_budget(budget)
        c.close()


def test_one_fold_launch_per_group_and_step(hal, ctx17):
    """m = 5 under the profiler: groups of 4 + 1, fold steps [2, 1]"""
    lg, m = 17, 5
    d = (1 << lg) - 1
    hal._lib.dev_hook("open_batch_fold", 1)
    want = np.zeros((m, ctx17.lib.halo_instance_words(lg)), dtype=np.uint64)
    st = C.c_uint64(0x9F0)
    assert ctx17.lib.halo_random_instance_batch(ctx17.h, C.byref(st), d, m, ob.ptr(want)) == 0
    ctx17.prof_enable(1)
    ctx17.prof_reset()
    try:
        got = np.zeros_like(want)
        st2 = C.c_uint64(0x9F0)
        assert ctx17.lib.halo_random_instance_batch(ctx17.h, C.byref(st2), d, m, ob.ptr(got)) == 0
        assert ctx17.info(10) == m and got.tolist() == want.tolist() and st2.value == st.value
        assert ob.fold_launches(ctx17) == 2 * len(ob.fold_steps(lg, 14)), ctx17.prof()
    finally:
        ctx17.prof_enable(0)
