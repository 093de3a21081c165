"""The bucket kernel and the window sums on the signed field layer (csrc/fq29s.hpp; XyzzS in csrc/curve.hpp): every pipeline at the
smallest sizes it admits must give, bit for bit, what the oracle gives -- and the table plans what the general pipeline gives on
the same context.  The scalar sets are those at which the group law leaves its common path: buckets of exactly kmax and kmax + 1
entries (a task boundary: a partial is stored, read back and added with xyzs_add), all-equal scalars (one bucket per window takes
every point), and, over the caller's bases, equal and opposite points in one bucket (the doubling and the cancellation inside
xyzs_madd).  Only equality is asserted.

Not here: a 4096-point `sub` stretch of the c = 20 plan.  table_eligible admits one, but no entry point makes a stretch shorter
than a sixteenth of 2^19 host scalars (tests/test_gpu_table_tasks.py runs that one); the c = 20 plan is run here through the two
default stretches of 2^19 host scalars."""
import numpy as np
import pytest

import orc
import pallas_model as pm

pytestmark = pytest.mark.gpu

R = pm.R_ORDER


@pytest.fixture(scope="module")
def hal():
    import halo_accumulation_amd as h
    return h._lib


def mont_words(vals):
    """Montgomery words (what the oracle and halo_msm take by default) of plain integers; few distinct values are expected"""
    memo = {}
    out = np.zeros((len(vals), 4), dtype=np.uint64)
    for i, v in enumerate(vals):
        if v not in memo:
            memo[v] = pm.to_mont_limbs(v % R, R)
        out[i] = memo[v]
    return out


def edge_scalars(n, rng):
    """plain integers: buckets of exactly kmax and kmax + 1 entries side by side for every task length (8, 16, 32, 64), the rest zero"""
    e = [0] * n
    where = rng.permutation(n)
    at = 0
    for kmax, digit in ((8, 700), (16, 1000), (32, 3000), (64, 5000)):
        for d, cnt in ((digit, kmax), (digit + 1, kmax + 1)):
            for i in where[at:at + cnt]:
                e[int(i)] = d
            at += cnt
    return e


def scalar_sets(n, seed):
    rng = np.random.default_rng(seed)
    uni, _ = orc.rng_scalars(0x7369676E6564 + seed, n)
    out = {"uniform": uni, "equal": mont_words([0x1234567890ABCDEF0FEDCBA987654321 * ((1 << 120) + 12345) % R] * n), "zero": mont_words([0] * n)}
    if n >= 256:
        out["task_len_edge"] = mont_words(edge_scalars(n, rng))
    return out


@pytest.mark.parametrize("n", [1, 2, 65])
def test_small_pipeline(hal, n):
    c = hal.Context(urs_n=n)
    try:
        gs = c.read_bases()
        for name, sc in scalar_sets(n, n).items():
            assert c.msm(sc).tolist() == orc.msm_affine(gs, sc).tolist(), name
    finally:
        c.close()


def with_equal_and_opposite(gs):
    """the caller's bases: runs of one point repeated, and a point next to its negative (y -> p - y in Montgomery words)"""
    b = np.array(gs, dtype=np.uint64).reshape(-1, 8).copy()
    n = len(b)
    for i in range(0, n - 8, 8):
        b[i + 1] = b[i]          # P, P
        b[i + 2] = b[i]
        y = sum(int(b[i + 3, 4 + k]) << (64 * k) for k in range(4))
        ny = pm.P - y
        b[i + 4, :4] = b[i + 3, :4]  # Q, -Q
        b[i + 4, 4:] = [(ny >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)]
    return b


def test_general_pipeline_2_16(hal):
    n = 1 << 16
    c = hal.Context(urs_n=n)
    try:
        c.set_table_mode(0)
        gs = c.read_bases()
        sets = scalar_sets(n, 16)
        for name, sc in sets.items():
            assert c.msm(sc).tolist() == orc.msm_affine(gs, sc).tolist(), name
        # equal and opposite points in one bucket: all-equal scalars put every base of a window into the same one
        b = with_equal_and_opposite(gs)
        for name in ("equal", "uniform", "task_len_edge"):
            assert c.msm_affine(b, sets[name]).tolist() == orc.msm_affine(b, sets[name]).tolist(), name
    finally:
        c.close()


def test_table_plan_c17_over_a_2_17_key(hal):
    import torch
    n = 1 << 17
    c = hal.Context(urs_n=n)
    try:
        gs = c.read_bases()
        sets = scalar_sets(n, 17)
        c.set_table_mode(0)
        general = {k: c.msm(v).tolist() for k, v in sets.items()}
        c.set_table_mode(-1)
        d = torch.from_numpy(sets["uniform"].view(np.int64)).cuda()
        c.msm_dev(d.data_ptr(), n)  # builds the table
        assert c.info(0) > 0, "no table: nothing here would test the table pipeline"
        for name, sc in sets.items():
            got = c.msm(sc).tolist()
            assert got == c.msm(sc).tolist() == general[name], name  # (the second call replays the launch graph)
        assert general["uniform"] == orc.msm_affine(gs, sets["uniform"]).tolist()
        assert general["task_len_edge"] == orc.msm_affine(gs, sets["task_len_edge"]).tolist()
    finally:
        c.close()


def test_table_plan_c20_through_two_stretches(hal):
    """2^19 host scalars over a 2^20 key: halo_msm runs them as two `sub` stretches (2^17 and 3 * 2^17 points) of the c = 20 plan"""
    import torch
    n, m = 1 << 20, 1 << 19
    c = hal.Context(urs_n=n)
    try:
        full, _ = orc.rng_scalars(0x7369676E656420, n)
        d = torch.from_numpy(full.view(np.int64)).cuda()
        c.msm_dev(d.data_ptr(), n)  # builds the table
        assert c.info(0) > 0, "no table: nothing here would test the table pipeline"
        sets = scalar_sets(m, 20)
        rng = np.random.default_rng(21)
        e = edge_scalars(1 << 17, rng) + edge_scalars(3 << 17, rng)  # the boundary buckets inside each stretch
        sets["task_len_edge"] = mont_words(e)
        c.set_table_mode(0)
        general = {k: c.msm(v).tolist() for k, v in sets.items()}
        c.set_table_mode(-1)
        c.msm_dev(d.data_ptr(), n)  # the table again
        for name, sc in sets.items():
            c.prof_enable(True); c.prof_reset()
            got = c.msm(sc).tolist()
            ran = c.prof()
            c.prof_enable(False)
            assert ran["k_tmsm_fine_sort"][1] == 2, "not two stretches over the table"
            assert got == general[name], name
        gs = c.read_bases()[:m]
        assert general["task_len_edge"] == orc.msm_affine(gs, sets["task_len_edge"]).tolist()
    finally:
        c.close()
