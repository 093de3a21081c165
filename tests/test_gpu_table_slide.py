"""The sliding odd-digit plan over the all-shifts table (msm_table.hip: TblPlan::slide, k_table_all_shifts, slide_lane.hpp), forced
through the development library's "table_slide_min" hook onto keys of 4096, 2^15 and 2^17 points (the product takes it from 2^20
points on: 34 GB of table; here 134 MB .. 4.3 GB).  Every launch must give, bit for bit, what the general pipeline gives on the
same context, and what the fixed 13-row plan gives on the same table (rows 20 w through the row stride).  The `sub` stretches of
halo_msm and the forced task lengths run over a 2^20-point key in tests/test_gpu_table_tasks.py, which takes this plan by default."""
import numpy as np
import pytest

import orc
import pallas_model as pm

pytestmark = pytest.mark.gpu

R = pm.R_ORDER
SIZES = [4096, 1 << 15, 1 << 17]
ALL_ROWS = 255
NO_TABLE, FIXED, SLIDING = 0, 1, 22  # halo_ctx_info(ctx, 9): the plan of the launch enqueued last (sliding: window width + 1)


@pytest.fixture(scope="module")
def hal():
    import halo_accumulation_amd as h
    return h._lib


@pytest.fixture(autouse=True)
def slide_from_4096(hal):
    """(tests/conftest.py resets the development hooks after every test)"""
    hal.dev_hook("table_slide_min", 4096)
    yield


def _limbs(vals):
    return np.array([[(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)] for v in vals], dtype=np.uint64)


def patterns(n, seed):
    """name -> (n, 4) uint64, plain 256-bit integers (scalars_are_mont = 0)"""
    rng = np.random.default_rng(seed)
    out = {}
    u = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    u[:, 3] &= np.uint64((1 << 62) - 1)  # below 2^254
    out["uniform"] = u
    out["zero"] = np.zeros((n, 4), dtype=np.uint64)
    # twelve buckets hold n entries each: the overflow region, k_msm_combine's wave form, unstaged runs
    out["equal"] = np.tile(_limbs([0x1234567890ABCDEF0FEDCBA987654321 * ((1 << 120) + 12345) % R]), (n, 1))
    # one digit per scalar (even values: the digit sits on a row above 0)
    b = np.zeros((n, 4), dtype=np.uint64)
    b[:, 0] = rng.integers(0, 1 << 20, size=n, dtype=np.uint64)
    out["one_digit"] = b
    # [2^254, r) and [r, r + 2^40): the last window, the carry into bit 254, the canonicalisation
    t = _limbs([R - 1 - int(k) for k in rng.integers(0, 1 << 40, size=48)] + [R + int(k) for k in rng.integers(0, 1 << 40, size=14)] + [1 << 254, (1 << 254) + 1])
    out["top_2_254"] = t[rng.integers(0, 64, size=n)]
    # buckets of exactly kmax and kmax + 1 entries for every task length (these launches run at 16), all else empty: an odd value
    # is one digit on row 0, an even one a digit on a higher row
    e = np.zeros((n, 4), dtype=np.uint64)
    where, at = rng.permutation(n), 0
    for kmax, digit in ((8, 701), (16, 1001), (16, 1 << 12), (32, 3001), (64, 5001)):
        e[where[at:at + kmax], 0] = digit
        at += kmax
        e[where[at:at + kmax + 1], 0] = digit + 2
        at += kmax + 1
    out["task_len_edge"] = e
    return {k: np.ascontiguousarray(v) for k, v in out.items()}


NAMES = ["uniform", "zero", "equal", "one_digit", "top_2_254", "task_len_edge"]
STRETCH = ["uniform", "task_len_edge", "top_2_254"]


class Case:
    """One context with the scalar sets resident, the general pipeline's results computed once and the all-shifts table built."""

    def __init__(self, hal, n):
        import torch
        self.n = n
        self.c = hal.Context(urs_n=n)
        self.host = patterns(n, 21 + n % 97)
        self.dev = {k: torch.from_numpy(v.view(np.int64)).cuda() for k, v in self.host.items()}
        self.c.set_table_mode(0)
        self.want = {k: self.c.msm_dev(d.data_ptr(), n, mont=False).tolist() for k, d in self.dev.items()}
        self.off, self.m = n // 4 + 8, n // 2 + 36  # a stretch of the key (table mode 0 would release the table later on)
        self.want_stretch = {k: self.c.msm_dev(self.dev[k].data_ptr(), self.m, off=self.off, mont=False).tolist() for k in STRETCH}
        assert self.c.info(9) == NO_TABLE
        self.c.set_table_mode(-1)
        self.c.msm_dev(self.dev["uniform"].data_ptr(), n, mont=False)  # builds the table
        assert self.c.info(8) == ALL_ROWS and self.c.info(0) == ALL_ROWS * 128 * n, "no all-shifts table: nothing here would test the sliding plan"
        assert self.c.info(9) == SLIDING, "the launch did not take the sliding plan"

    def ptr(self, name):
        return self.dev[name].data_ptr()


@pytest.fixture(scope="module", params=SIZES)
def case(request, hal):
    hal.dev_hook("table_slide_min", 4096)
    k = Case(hal, request.param)
    yield k
    k.c.close()


@pytest.mark.parametrize("name", NAMES)
def test_one_member_matches_the_general_pipeline_and_the_fixed_plan(case, name):
    c = case.c
    got = c.msm_dev(case.ptr(name), case.n, mont=False)
    again = c.msm_dev(case.ptr(name), case.n, mont=False)  # graph replay
    assert got.tolist() == again.tolist() == case.want[name]
    assert c.info(9) == SLIDING
    c.set_table_mode(1)  # the fixed 13-row plan, read from rows 20 w of the same table
    try:
        fixed = c.msm_dev(case.ptr(name), case.n, mont=False)
        assert c.info(8) == ALL_ROWS, "same allocation"
        assert c.info(9) == FIXED
    finally:
        c.set_table_mode(-1)
    assert fixed.tolist() == case.want[name]


def test_the_oracle_agrees(case):
    sc, _ = orc.rng_scalars(0x736C696465, case.n)
    assert case.c.msm(sc).tolist() == orc.msm_affine(case.c.read_bases(), sc).tolist()


def test_begin_end_on_every_slot_and_batches(case):
    """asynchronous launches on two slots at once; batches of 1, 2 and 8 members (more than one member of a c = 20 key runs
    table-free: same points)"""
    c = case.c
    c.msm_dev_begin(0, case.ptr("uniform"), case.n, mont=False)
    c.msm_dev_begin(3, case.ptr("task_len_edge"), case.n, mont=False)
    assert c.msm_dev_end(0).tolist() == case.want["uniform"] and c.msm_dev_end(3).tolist() == case.want["task_len_edge"]
    for names in (["top_2_254"], ["task_len_edge", "equal"], NAMES + ["uniform", "one_digit"]):
        c.msm_dev_batch_begin(1, [case.ptr(k) for k in names], case.n, mont=False)
        got = c.msm_dev_batch_end(1, len(names))
        assert [g.tolist() for g in got] == [case.want[k] for k in names]
        assert c.info(9) == (SLIDING if len(names) == 1 else NO_TABLE)


def test_a_stretch_of_the_key(case):
    """a launch over GS[off, off + m): entry references carry the offset on every row (at 4096 points the stretch is below the
    plan's least size and runs table-free)"""
    c = case.c
    for name in STRETCH:
        assert c.msm_dev(case.ptr(name), case.m, off=case.off, mont=False).tolist() == case.want_stretch[name]
    assert c.info(8) == ALL_ROWS and c.info(9) == (SLIDING if case.m >= 4096 else NO_TABLE)


def test_a_clone_shares_the_table(case):
    c = case.c
    assert c.info(8) == ALL_ROWS
    used = c.info(4)
    b = c.clone()
    try:
        assert b.msm_dev(case.ptr("uniform"), case.n, mont=False).tolist() == case.want["uniform"]
        assert b.info(8) == ALL_ROWS and b.info(4) == used, "adopted, not built again"
    finally:
        b.close()
    assert c.msm_dev(case.ptr("equal"), case.n, mont=False).tolist() == case.want["equal"]


def test_a_budget_without_room_for_every_shift_keeps_the_13_rows(hal):
    """optional memory: refused -> the context builds the 13-row table and runs the fixed plan, never an error"""
    import torch
    n = 4096
    c = hal.Context(urs_n=n)
    orig = c.info(3)
    try:
        sc = patterns(n, 5)["uniform"]
        d = torch.from_numpy(sc.view(np.int64)).cuda()
        c.set_table_mode(0)
        want = c.msm_dev(d.data_ptr(), n, mont=False).tolist()
        c.set_table_mode(-1)
        c.set_memory_budget(c.info(4) + (16 << 20))  # 13 rows are 6.8 MB, 255 rows 134 MB
        assert c.msm_dev(d.data_ptr(), n, mont=False).tolist() == want
        assert c.info(8) == 13 and c.info(0) == 13 * 128 * n and c.info(6) == 2
        assert c.msm_dev(d.data_ptr(), n, mont=False).tolist() == want
    finally:
        c.set_memory_budget(orig)
        c.close()


def test_forced_fixed_mode_builds_no_large_table(hal):
    import torch
    n = 4096
    c = hal.Context(urs_n=n)
    try:
        sc = patterns(n, 6)["uniform"]
        d = torch.from_numpy(sc.view(np.int64)).cuda()
        c.set_table_mode(0)
        want = c.msm_dev(d.data_ptr(), n, mont=False).tolist()
        c.set_table_mode(1)
        assert c.msm_dev(d.data_ptr(), n, mont=False).tolist() == want and c.info(8) == 13
    finally:
        c.close()


def test_the_fold_table_displaces_the_all_shifts_table(hal):
    """2^20 points, default modes and default budget (room for the all-shifts table OR the fold table): the first MSM builds the 255
    rows; the key's 8th full-size open asks for the fold table, is refused beside them, and the MSM table goes down to its 13 rows
    at the next MSM enqueued with nothing in flight; a later open gets the fold table.  Same commitment and proof throughout."""
    import torch
    from halo_accumulation_amd import pcdl
    hal.dev_hook("table_slide_min", 0)
    n = 1 << 20
    d = n - 1
    c = hal.Context(urs_n=n)
    orig = c.info(3)
    try:
        c.set_memory_budget(c.info(4) + (48 << 30))  # the default of a 288 GB device, whatever this process was given
        dv = torch.empty((n + 1) * 4, dtype=torch.int64, device="cuda")
        c.rng_scalars_dev(0xF01D, n + 1, dv.data_ptr())
        z = np.ascontiguousarray(dv[4 * n:].cpu().numpy().view(np.uint64))
        C = pcdl.commit_dev(c, dv.data_ptr(), n, d)
        assert c.info(8) == ALL_ROWS and c.info(7) > 0
        first = pcdl.open_dev(c, [1], dv.data_ptr(), n, C, d, z)
        for k in range(2, 8):
            assert pcdl.open_dev(c, [1], dv.data_ptr(), n, C, d, z).tolist() == first.tolist()
        assert c.info(8) == ALL_ROWS and c.info(1) == 0, "seven opens: nothing has asked for the room"
        built = None
        for k in range(8, 200):  # (the fold table's memory arrives on a helper thread: 0.5 ms .. 2 s)
            assert pcdl.open_dev(c, [1], dv.data_ptr(), n, C, d, z).tolist() == first.tolist()
            if c.info(1):
                built = k
                break
        assert built is not None and c.info(8) == 13 and c.info(0) == 13 * 128 * n
        assert pcdl.open_dev(c, [1], dv.data_ptr(), n, C, d, z).tolist() == first.tolist()
        assert pcdl.commit_dev(c, dv.data_ptr(), n, d).tolist() == C.tolist()
    finally:
        c.set_memory_budget(orig)
        c.close()


GB = 1 << 30


def _key_2_20(hal, budget_gb=48):
    """a 2^20-point context under the default budget of a 288 GB device, scalars and an evaluation point resident"""
    import torch
    n = 1 << 20
    c = hal.Context(urs_n=n)
    orig = c.info(3)
    c.set_memory_budget(c.info(4) + budget_gb * GB)
    dv = torch.empty((n + 1) * 4, dtype=torch.int64, device="cuda")
    c.rng_scalars_dev(0xF01D, n + 1, dv.data_ptr())
    z = np.ascontiguousarray(dv[4 * n:].cpu().numpy().view(np.uint64))
    return c, orig, dv, z, n


def test_sub_stretches_take_the_sliding_plan(hal):
    """halo_msm on 2^19 host scalars over a 2^20-point key: two `sub` stretches (2^17 and 3 * 2^17 points), both through the sliding
    plan on the all-shifts table, against the general pipeline in one launch"""
    hal.dev_hook("table_slide_min", 0)
    c, orig, dv, z, n = _key_2_20(hal)
    try:
        v = patterns(1 << 19, 31)["uniform"]
        c.set_table_mode(0)
        want = c.msm(v, mont=False).tolist()
        c.set_table_mode(-1)
        c.msm_dev(dv.data_ptr(), n)
        assert c.info(8) == ALL_ROWS and c.info(9) == SLIDING
        c.prof_enable(True); c.prof_reset()
        got = c.msm(v, mont=False)
        ran = c.prof()
        c.prof_enable(False)
        assert ran["k_tmsm_fine_sort"][1] == 2 and ran.get("k_msm_task_order", (0, 0))[1] == 0, "not two stretches over the table"
        assert c.info(9) == SLIDING and got.tolist() == want
        assert c.msm(v, mont=False).tolist() == want
    finally:
        c.set_memory_budget(orig)
        c.close()


def _opens_until_fold_table(c, dv, z, n, limit=200):
    from halo_accumulation_amd import pcdl
    C = pcdl.commit_dev(c, dv.data_ptr(), n, n - 1)
    first = pcdl.open_dev(c, [1], dv.data_ptr(), n, C, n - 1, z)
    rows = []
    for k in range(2, limit):
        assert pcdl.open_dev(c, [1], dv.data_ptr(), n, C, n - 1, z).tolist() == first.tolist()
        rows.append(c.info(8))
        if c.info(1):
            return k, rows
    return None, rows


def test_a_clone_makes_the_key_keep_room_for_the_fold_table(hal):
    """The decision is per key.  (a) A context with the 255 rows is cloned: while it is still the table's only user the table goes
    down to 13 rows, and the opens that follow get the fold table, as they did before there was an all-shifts table.  (b) A key
    that already has a clone builds the 13 rows in the first place.  In neither case is a table released again later: the rows
    read 13 at every open."""
    hal.dev_hook("table_slide_min", 0)
    for clone_first in (False, True):
        c, orig, dv, z, n = _key_2_20(hal)
        b = None
        try:
            if clone_first:
                b = c.clone()
            c.msm_dev(dv.data_ptr(), n)
            assert c.info(8) == (13 if clone_first else ALL_ROWS)
            if not clone_first:
                b = c.clone()
                assert c.info(8) == 0 and c.info(0) == 0, "the only user's all-shifts table made room"
            want = c.msm_dev(dv.data_ptr(), n).tolist()
            assert c.info(8) == 13 and c.info(9) == FIXED and b.msm_dev(dv.data_ptr(), n).tolist() == want and b.info(8) == 13
            built, rows = _opens_until_fold_table(c, dv, z, n)
            assert built is not None and set(rows) == {13}, (built, rows)
            assert b.msm_dev(dv.data_ptr(), n).tolist() == want
        finally:
            if b is not None:
                b.close()
            c.set_memory_budget(orig)
            c.close()


def test_a_table_that_clones_share_or_that_would_not_make_room_stays(hal):
    """(a) The 255 rows were built while nobody wanted a fold table and a clone shares them: the fold table, asked for later, is
    refused once with its usual back-off (status 3) and the table is neither released nor rebuilt.  (b) A budget that holds the
    all-shifts table but could never hold the fold table: asking for the fold table does not throw the MSM table away."""
    from halo_accumulation_amd import pcdl
    hal.dev_hook("table_slide_min", 0)
    for shared, budget in ((True, 48), (False, 36)):
        c, orig, dv, z, n = _key_2_20(hal, budget)
        b = None
        try:
            c.set_fold_table(0)
            if shared:
                b = c.clone()
            want = c.msm_dev(dv.data_ptr(), n).tolist()
            assert c.info(8) == ALL_ROWS
            built_us = c.info(7)
            c.set_fold_table(1)
            assert c.info(8) == ALL_ROWS, "not released"
            C = pcdl.commit_dev(c, dv.data_ptr(), n, n - 1)
            first = pcdl.open_dev(c, [1], dv.data_ptr(), n, C, n - 1, z)
            for _ in range(3):
                assert pcdl.open_dev(c, [1], dv.data_ptr(), n, C, n - 1, z).tolist() == first.tolist()
                assert c.info(8) == ALL_ROWS and c.info(1) == 0 and c.info(5) == 3 and c.info(7) == built_us
            assert c.msm_dev(dv.data_ptr(), n).tolist() == want and c.info(9) == SLIDING
        finally:
            if b is not None:
                b.close()
            c.set_memory_budget(orig)
            c.close()
