"""The table pipeline's task records: k_tmsm_fine_sort lays them out itself (an overflow region, then one slot per bucket in
a rank-major order) and no k_msm_task_order runs between the sort and the bucket kernel.  Every launch shape of the table
pipeline must still give, bit for bit, what the general pipeline gives on the same context, for the scalar sets at which
a layout bug would show: all records empty, everything in the overflow region, buckets at the task-length boundary."""
import os
import subprocess
import sys

import numpy as np
import pytest

import orc
import pallas_model as pm

pytestmark = pytest.mark.gpu

R = pm.R_ORDER
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hal():
    import halo_accumulation_amd as h
    return h._lib


def _limbs(vals):
    return np.array([[(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)] for v in vals], dtype=np.uint64)


def edge_set(n, spans, rng):
    """Buckets of exactly kmax and kmax + 1 entries side by side, for every automatic task length (16, 32, 64) and the forced 8;
    all else empty.  A bucket's entries are the scalars of ONE launch, so every span [lo, hi) of indices that runs as a launch
    of its own (a stretch, a piece) gets its own full set of pairs, placed inside it."""
    e = np.zeros((n, 4), dtype=np.uint64)
    for lo, hi in spans:
        where = lo + rng.permutation(hi - lo)
        at = 0
        for kmax, digit in ((8, 700), (16, 1000), (32, 3000), (64, 5000)):
            e[where[at:at + kmax], 0] = digit
            at += kmax
            e[where[at:at + kmax + 1], 0] = digit + 1
            at += kmax + 1
    return np.ascontiguousarray(e)


def patterns(n, seed):
    """name -> (n, 4) uint64, plain 256-bit integers (scalars_are_mont = 0)"""
    rng = np.random.default_rng(seed)
    out = {}
    u = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    u[:, 3] &= np.uint64((1 << 62) - 1)  # below 2^254
    out["uniform"] = u
    out["zero"] = np.zeros((n, 4), dtype=np.uint64)
    # one bucket per window holds all n entries: the overflow region, k_msm_combine's wave form, an unstaged run
    out["equal"] = np.tile(_limbs([0x1234567890ABCDEF0FEDCBA987654321 * ((1 << 120) + 12345) % R]), (n, 1))
    # one window only: most coarse ranges are empty
    b = np.zeros((n, 4), dtype=np.uint64)
    b[:, 0] = rng.integers(0, 1 << 20, size=n, dtype=np.uint64)
    out["below_2_20"] = b
    out["task_len_edge"] = edge_set(n, [(0, n)], rng)
    # scalars >= 2^254: the c = 17 plan folds them to r - s
    t = _limbs([R - 1 - int(k) for k in rng.integers(0, 1 << 40, size=64)])
    out["top_2_254"] = t[rng.integers(0, 64, size=n)]
    return {k: np.ascontiguousarray(v) for k, v in out.items()}


NAMES = ["uniform", "zero", "equal", "below_2_20", "task_len_edge", "top_2_254"]


class Case:
    """One context with the scalar sets resident and the general pipeline's results computed once."""

    def __init__(self, hal, n, seed):
        import torch
        self.n = n
        self.c = hal.Context(urs_n=n)
        self.host = patterns(n, seed)
        self.dev = {k: torch.from_numpy(v.view(np.int64)).cuda() for k, v in self.host.items()}
        self.c.set_table_mode(0)
        self.want = {k: self.c.msm_dev(d.data_ptr(), n, mont=False).tolist() for k, d in self.dev.items()}
        self.c.set_table_mode(-1)
        self.c.msm_dev(self.dev["uniform"].data_ptr(), n, mont=False)  # builds the table
        assert self.c.info(0) > 0, "no table: nothing here would test the table pipeline"

    def ptr(self, name):
        return self.dev[name].data_ptr()


@pytest.fixture(scope="module")
def small(hal):
    k = Case(hal, 1 << 17, 11)
    yield k
    k.c.close()


@pytest.fixture(scope="module")
def large(hal):
    k = Case(hal, 1 << 20, 12)
    yield k
    k.c.close()


@pytest.mark.parametrize("name", NAMES)
def test_small_key_one_member(small, name):
    """c = 17 plan, one member (64 coarse ranges of 1024 buckets, task length 16)"""
    got = small.c.msm_dev(small.ptr(name), small.n, mont=False)
    again = small.c.msm_dev(small.ptr(name), small.n, mont=False)  # graph replay
    assert got.tolist() == again.tolist() == small.want[name]


def test_small_key_matches_the_oracle(small):
    sc, _ = orc.rng_scalars(0x7461626C65, small.n)
    got = small.c.msm(sc)
    assert got.tolist() == orc.msm_affine(small.c.read_bases(), sc).tolist()


def test_small_key_eight_members(small):
    """c = 17 plan, eight bucket sets side by side (512 coarse ranges, task length 64): one member per scalar set"""
    names = NAMES + ["uniform", "equal"]
    ptrs = [small.ptr(k) for k in names]
    for _ in range(2):
        small.c.msm_dev_batch_begin(0, ptrs, small.n, mont=False)
        got = small.c.msm_dev_batch_end(0, len(ptrs))
        assert [g.tolist() for g in got] == [small.want[k] for k in names]
    # and two members (128 ranges, task length 32), one of them with the buckets at that boundary
    two = ["task_len_edge", "equal"]
    small.c.msm_dev_batch_begin(1, [small.ptr(k) for k in two], small.n, mont=False)
    got = small.c.msm_dev_batch_end(1, 2)
    assert [g.tolist() for g in got] == [small.want[k] for k in two]


@pytest.mark.parametrize("name", NAMES[:5])
def test_large_key_full_msm(large, name):
    """c = 20 plan, one full MSM (512 coarse ranges of 1024 buckets, task length 64)"""
    got = large.c.msm_dev(large.ptr(name), large.n, mont=False)
    again = large.c.msm_dev(large.ptr(name), large.n, mont=False)
    assert got.tolist() == again.tolist() == large.want[name]


def stretch_sets(large, first):
    """2^19 host scalars whose first stretch is `first` points long: uniform, all-equal, and the task-length edges placed inside
    each of the two stretches"""
    m = 1 << 19
    return {"uniform": large.host["uniform"][:m], "equal": large.host["equal"][:m],
            "task_len_edge": edge_set(m, [(0, first), (first, m)], np.random.default_rng(14))}


def check_stretches(c, sets, full_ptr, full_n):
    """every set through halo_msm: the general pipeline in one launch, then two `sub` stretches over the table"""
    c.set_table_mode(0)
    try:
        want = {k: c.msm(v, mont=False).tolist() for k, v in sets.items()}
    finally:
        c.set_table_mode(-1)
    c.msm_dev(full_ptr, full_n, mont=False)  # the table again
    for k, v in sets.items():
        c.prof_enable(True); c.prof_reset()
        got = c.msm(v, mont=False)
        ran = c.prof()
        c.prof_enable(False)
        assert ran["k_tmsm_fine_sort"][1] == 2 and ran.get("k_msm_task_order", (0, 0))[1] == 0, "not two stretches over the table"
        assert got.tolist() == want[k], k


def test_large_key_sub_stretches(large):
    """Host scalars: halo_msm runs 2^19 points as two `sub` stretches of 2^17 and 3 * 2^17 points through the c = 20 plan
    (task lengths 16 and 64): the default split."""
    check_stretches(large.c, stretch_sets(large, 1 << 17), large.ptr("uniform"), large.n)


CHILD = """
import sys
sys.path[:0] = [%r, %r, %r]
import numpy as np, torch
import halo_accumulation_amd as h
import test_gpu_table_tasks as t
l = h.load()
assert l.halo_dev_tuning(b"host_pieces") == 2 and l.halo_dev_tuning(b"host_split0") == 1
large = t.Case(h._lib, 1 << 20, 12)
t.check_stretches(large.c, t.stretch_sets(large, 1 << 15), large.ptr("uniform"), large.n)
large.c.close()
print("stretches ok")
"""


def test_large_key_shortest_sub_stretch():
    """The shortest `sub` stretch a call can make: a sixteenth of 2^19 host scalars, 2^15 points (task length 16), beside one of
    15 sixteenths.  The library reads HALO_HOST_SPLIT once per process, so this runs in a child.  (table_eligible admits `sub`
    launches from 4096 points, but halo_msm splits only from 2^19 points on, into sixteenths: nothing shorter can be asked for.)"""
    env = dict(os.environ, HALO_HOST_SPLIT="1,15")
    code = CHILD % (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "stretches ok" in out.stdout, (out.stdout[-400:], out.stderr[-1200:])


@pytest.mark.parametrize("kmax", [8, 64])
@pytest.mark.parametrize("name", ["uniform", "equal"])
def test_forced_task_length(large, name, kmax):
    """halo_set_task_len: at 8 nearly every bucket of a uniform set has overflow tasks, and the all-equal set 1.7 million"""
    large.c.set_task_len(kmax)
    try:
        got = large.c.msm_dev(large.ptr(name), large.n, mont=False)
    finally:
        large.c.set_task_len(0)
    assert got.tolist() == large.want[name]
    assert large.c.msm_dev(large.ptr(name), large.n, mont=False).tolist() == large.want[name]


def test_kernels_of_a_table_launch(large):
    c = large.c
    c.prof_enable(True); c.prof_reset()
    c.msm_dev(large.ptr("uniform"), large.n, mont=False)
    ran = {k: v[1] for k, v in c.prof().items()}  # launches since the reset (a name stays listed once it has run)
    assert ran.get("k_tmsm_fine_sort") == 1 and ran.get("k_msm_accumulate") == 1 and ran.get("k_msm_task_order", 0) == 0, ran
    c.set_table_mode(0)
    try:
        c.prof_reset()
        c.msm_dev(large.ptr("uniform"), large.n, mont=False)
        ran = {k: v[1] for k, v in c.prof().items()}
        assert ran.get("k_msm_task_order") == 1 and ran.get("k_msm_accumulate") == 1 and ran.get("k_tmsm_fine_sort", 0) == 0, ran
    finally:
        c.prof_enable(False)
        c.set_table_mode(-1)


def test_pieces_of_a_2_21_point_msm(hal):
    """More than TBL_PIECE points: two pieces of 2^20 points, alternating over two slots in a synchronous call (the second
    piece on the partner slot's workspace) and one after the other on one slot in an asynchronous one -- at the automatic
    task length (64) and at a forced 8, which multiplies the records and makes both workspaces grow.  The edge set has its
    kmax / kmax + 1 buckets inside each piece."""
    import torch
    n = 1 << 21
    c = hal.Context(urs_n=n)
    try:
        rng = np.random.default_rng(13)
        u = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
        u[:, 3] &= np.uint64((1 << 62) - 1)
        sets = {"uniform": np.ascontiguousarray(u), "task_len_edge": edge_set(n, [(0, n // 2), (n // 2, n)], rng)}
        dev = {k: torch.from_numpy(v.view(np.int64)).cuda() for k, v in sets.items()}
        c.set_table_mode(0)
        want = {k: c.msm_dev(d.data_ptr(), n, mont=False).tolist() for k, d in dev.items()}
        c.set_table_mode(-1)
        for kmax in (0, 8):
            c.set_task_len(kmax)
            for name, d in dev.items():
                c.prof_enable(True); c.prof_reset()
                got = c.msm_dev(d.data_ptr(), n, mont=False)
                assert c.prof()["k_tmsm_fine_sort"][1] == 2 and c.prof().get("k_msm_task_order", (0, 0))[1] == 0
                c.prof_enable(False)
                c.msm_dev_begin(2, d.data_ptr(), n, mont=False)
                got2 = c.msm_dev_end(2)
                assert got.tolist() == got2.tolist() == want[name], (name, kmax)
    finally:
        c.close()
