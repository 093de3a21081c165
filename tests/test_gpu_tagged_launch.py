"""The tagged two-set table launch (MsmBatch::tagged: L and R of the first rounds of an open over 2^20 points) asked for directly,
through the development library's halo_dev_msm_tagged, over short keys that the hook "table_slide_min" sends through the c = 20
plans -- with scalars and tags of the test's choice (tests/tagged_cases.py), which the opens never bring:

    key A, 4096 + 260 points   infinite, repeated and opposite points (table_cases), on the all-shifts table (rows 20 w) and on the 13-row
                               table: every scalar set under every tag pattern, stretches with off != 0, forced task lengths
    key M, 160 004 points      the device's URS on the 13-row table: chunks longer than a scatter tile, a ragged last chunk, runs far above
                               the LDS stage and runs of exactly TBL_STAGE and TBL_STAGE + 1 entries
    the table key, 4096 points planted equal, opposite and empty buckets in either set: all records of the 2-set window sums read back

Every result is the oracle's (orc.msm_affine over the values of each tag), limb for limb; every launch runs three times with identical
results (its scalars at one address: a plain launch, its capture into a graph, the replay) and first asserts, through
halo_dev_msm_last_plan, that it took the 2-set plan."""
import numpy as np
import pytest

import orc
import table_cases as tc
import tagged_cases as tg
import window_cases as wc
from test_gpu_table_build import STRETCHES

pytestmark = pytest.mark.gpu

ALL_ROWS = 255
PLAN = dict(pipeline=2, c=20, W=13, B=1 << 19, members=2, sets=2, pieces=1, form=2, lg_rows=9, lg_cols=10, per=16)
TWO_SET_KERNELS = {"k_tmsm_recode": 1, "k_tmsm_coarse_hist2": 1, "k_tmsm_coarse_scatter2": 1, "k_tmsm_scan_ranges": 1, "k_tmsm_fine_sort": 1,
                   "k_msm_accumulate": 1, "k_msm_reduce_rc": 1, "k_msm_task_order": 0, "k_tmsm_coarse_hist": 0, "k_tmsm_coarse_scatter": 0}
REFUSAL = "a tagged launch is one canonical scalar array over the context's key with the c = 20 table in place"


@pytest.fixture(scope="module")
def hal():
    import halo_accumulation_amd as h
    return h._lib


@pytest.fixture(autouse=True)
def slide_from_4096(hal):
    """short keys take the c = 20 plans (tests/conftest.py resets the development hooks after every test)"""
    hal.dev_hook("table_slide_min", 4096)
    yield


def assert_plan(c, kmax):
    got = c.msm_last_plan(0)
    diff = {k: (got[k], v) for k, v in dict(PLAN, kmax=kmax).items() if got[k] != v}
    assert not diff, "the launch took another plan (field: got, expected): %s" % diff
    return got


def run_three_times(c, tagged, kmax, off=0, reads=None):
    """one tagged array three times (plain launch, capture, replay): the 2-set plan each time, identical results -> 2 x 12 words
    as lists.  reads: a list that takes the window-sum records of each run"""
    results = []
    for _ in range(3):
        results.append(c.msm_tagged(tagged, off=off).tolist())
        assert_plan(c, kmax)
        if reads is not None:
            reads.append(c.msm_window_sums(0))
    assert results[0] == results[1] == results[2], "plain launch, capture and replay gave different results"
    return results[0]


def assert_two_set_kernels(c, tagged, kmax, off=0):
    """the same launch under the profile counters: the kernels with a 2 in their names ran once, their one-set forms and the general
    pipeline's task order did not"""
    c.prof_enable(True)
    try:
        c.prof_reset()
        got = c.msm_tagged(tagged, off=off).tolist()
        ran = {k: v[1] for k, v in c.prof().items()}
    finally:
        c.prof_enable(False)
    assert_plan(c, kmax)
    assert {k: ran.get(k, 0) for k in TWO_SET_KERNELS} == TWO_SET_KERNELS, ran
    return got


def build_table(c, n, rows):
    """the context's first table MSM builds its table; a tagged launch builds none"""
    sc, _ = orc.rng_scalars(0x746167676564, n)
    c.msm(sc)
    assert c.info(8) == rows, "not the table this test is about"


class Cases:
    """a key, its scalar sets, and the oracle's two sums of every (set, pattern, stretch) asked for: computed once"""

    def __init__(self, key, sets):
        self.key, self.n, self.sets = key, key.shape[0], sets
        self._tags, self._values, self._want = {}, {}, {}

    def tags(self, pattern, off=0, m=None):
        m = self.n - off if m is None else m
        if (pattern, m) not in self._tags:
            self._tags[(pattern, m)] = tg.tags(pattern, m)
        return self._tags[(pattern, m)]

    def values(self, name, pattern, off=0, m=None):
        m = self.n - off if m is None else m
        k = (name, pattern, off, m)
        if k not in self._values:
            self._values[k] = tg.task_len_edge(self.tags(pattern, off, m)) if name == "task_len_edge" else self.sets[name][off:off + m]
        return self._values[k]

    def case(self, name, pattern, off=0, m=None):
        """-> (tagged words, [want of set 0, want of set 1])"""
        m = self.n - off if m is None else m
        v, t = self.values(name, pattern, off, m), self.tags(pattern, off, m)
        k = (name, pattern, off, m)
        if k not in self._want:
            self._want[k] = tg.want(self.key, v, t, off)
        return tg.split(v, t)[0], self._want[k]


def _urs(hal, n):
    c = hal.Context(urs_n=n)
    try:
        return c.read_bases()
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------------- key A
@pytest.fixture(scope="module")
def a(hal):
    """key A on two contexts: the all-shifts table (a tagged launch reads rows 20 w) and the 13 rows of k_table_step"""
    hal.dev_hook("table_slide_min", 4096)
    key, classes = tc.exceptional_key(_urs(hal, tc.N_A), "all_shifts")
    k = Cases(key, tg.key_a_sets(tc.N_A, classes, 0x7461626C65))
    k.ctx = {"all-shifts table": hal.Context(bases=key), "13-row table": hal.Context(bases=key)}
    k.ctx["13-row table"].set_table_mode(1)
    build_table(k.ctx["all-shifts table"], tc.N_A, ALL_ROWS)
    build_table(k.ctx["13-row table"], tc.N_A, 13)
    yield k
    for c in k.ctx.values():
        c.set_task_len(0)
        c.close()


def test_first_tagged_launch_on_a_fresh_context_grows_the_workspace(hal, a):
    """A context of 4356 points allocates slot 0 for one bucket set (2^19 per-bucket counters, 533 256 task records); the two sets
    take 2^20 and 1 052 160 (the overflow region at the stretch's own task length, 16).  Nothing reports a slot's capacities: the
    launch not being refused (tmsm_enqueue_piece: "table plan exceeds workspace") and giving the oracle's sums is the assertion."""
    c = hal.Context(bases=a.key)
    try:
        build_table(c, tc.N_A, ALL_ROWS)
        tagged, want = a.case("uniform", "halves")
        assert c.msm_tagged(tagged).tolist() == want
        assert_plan(c, 16)
        assert assert_two_set_kernels(c, tagged, 16) == want
        assert c.msm_tagged(np.zeros((0, 4), dtype=np.uint64)).tolist() == [orc_infinity(), orc_infinity()], "n = 0 is two infinities"
    finally:
        c.close()


def orc_infinity():
    """the normalised point at infinity as the entry points store it: what the oracle's MSM of zeros gives"""
    return orc.msm_affine(np.zeros((1, 8), dtype=np.uint64), np.zeros((1, 4), dtype=np.uint64)).tolist()


@pytest.mark.parametrize("form", ["all-shifts table", "13-row table"])
def test_key_a_runs_the_two_set_kernels(a, form):
    tagged, want = a.case("uniform", "random")
    assert assert_two_set_kernels(a.ctx[form], tagged, 16) == want


@pytest.mark.parametrize("name", tg.KEY_A_SETS)
@pytest.mark.parametrize("form", ["all-shifts table", "13-row table"])
def test_key_a_every_set_under_every_tag_pattern(a, form, name):
    c = a.ctx[form]
    bad = []  # (every pattern runs: a failure under one does not hide the others)
    for pattern in tg.PATTERNS:
        tagged, want = a.case(name, pattern)
        got = run_three_times(c, tagged, 16)
        if got != want:
            bad.append((pattern, "outputs swapped" if got == want[::-1] else "wrong sums"))
        empty = {"all0": [1], "all1": [0]}.get(pattern, []) + ([0, 1] if name in tc.INFINITE_RESULT else [])
        for t in (0, 1):  # (an empty set is the point at infinity, a live one is not: the oracle's own sums say so)
            assert (orc.point_canonical(np.array(want[t], dtype=np.uint64)) is None) == (t in empty), (name, pattern, t)
    assert not bad, (name, bad)


@pytest.mark.parametrize("name", ["uniform", "equal", "paired"])
@pytest.mark.parametrize("off,m", STRETCHES)
def test_a_stretch_of_key_a(a, off, m, name):
    """off != 0: the table rows are read at base_off + i, the spread takes i of the stretch; through the run of copies and through the
    run of negations"""
    assert m % 4 == 0 and m >= 4096 and off and off + m <= tc.N_A
    bad = []
    for pattern in ("halves", "random"):
        tagged, want = a.case(name, pattern, off, m)
        if run_three_times(a.ctx["all-shifts table"], tagged, 16, off=off) != want:
            bad.append(pattern)
    assert not bad, bad


@pytest.mark.parametrize("kmax", [8, 64])
@pytest.mark.parametrize("name", ["uniform", "equal", "task_len_edge"])
@pytest.mark.parametrize("form", ["all-shifts table", "13-row table"])
def test_key_a_forced_task_length(a, form, name, kmax):
    """halo_set_task_len: at 8 the all-equal set is overflow tasks all over, and the buckets of 8 / 9 and 64 / 65 entries sit at the boundary"""
    c = a.ctx[form]
    bad = []
    c.set_task_len(kmax)
    try:
        for pattern in ("halves", "random"):
            tagged, want = a.case(name, pattern)
            if run_three_times(c, tagged, kmax) != want:
                bad.append(pattern)
    finally:
        c.set_task_len(0)
    tagged, want = a.case(name, "halves")
    assert run_three_times(c, tagged, 16) == want and not bad, bad


# ---------------------------------------------------------------------------------------------------- key M
@pytest.fixture(scope="module")
def m_key(hal):
    hal.dev_hook("table_slide_min", 4096)
    c = hal.Context(urs_n=tg.N_M)
    c.set_table_mode(1)
    k = Cases(c.read_bases(), tg.key_m_sets(tg.N_M, 0x6B65794D))
    k.c = c
    build_table(c, tg.N_M, 13)
    chunk_len = (((tg.N_M + 18) // 19) + 3) // 4 * 4  # 256 / 13 = 19 chunks a window
    assert chunk_len == 8424 > tg.TBL_TILE and tg.N_M - 18 * chunk_len < chunk_len and 13 * tg.N_M <= 16 * 131072
    yield k
    c.set_task_len(0)
    c.close()


def test_key_m_runs_the_two_set_kernels(m_key):
    tagged, want = m_key.case("uniform", "halves")
    assert assert_two_set_kernels(m_key.c, tagged, 16) == want


@pytest.mark.parametrize("pattern", ["halves", "random"])
@pytest.mark.parametrize("name", tg.KEY_M_SETS)
def test_key_m_against_the_oracle(m_key, name, pattern):
    tagged, want = m_key.case(name, pattern)
    assert run_three_times(m_key.c, tagged, 16) == want


@pytest.mark.parametrize("swapped", [False, True])
def test_key_m_runs_at_the_stage_boundary(m_key, swapped):
    """a coarse run of exactly TBL_STAGE entries in one set (staged in LDS) beside one of TBL_STAGE + 1 in the other (placed directly);
    35 or 36 entries a bucket: one task each under a task length of 64"""
    values, tags = tg.stage_edge(tg.N_M, swapped)
    tagged = tg.split(values, tags)[0]
    m_key.c.set_task_len(64)
    try:
        got = run_three_times(m_key.c, tagged, 64)
    finally:
        m_key.c.set_task_len(0)
    assert got == tg.want(m_key.key, values, tags)


# ---------------------------------------------------------------------------------------------------- planted window sums
KS, PAIRS = tg.planted_pairs()


@pytest.fixture(scope="module")
def table_ctx(hal):
    hal.dev_hook("table_slide_min", 4096)
    key = wc.multiples_key(len(KS), KS)
    c = hal.Context(key)
    build_table(c, len(KS), ALL_ROWS)
    yield c, key
    c.close()


def test_table_key_runs_the_two_set_kernels(table_ctx):
    c, key = table_ctx
    tagged = tg.split(PAIRS[0].scalars, PAIRS[0].tags)[0]
    assert assert_two_set_kernels(c, tagged, 16) == tg.want(key, PAIRS[0].scalars, PAIRS[0].tags)


@pytest.mark.parametrize("pair", PAIRS, ids=[p.name for p in PAIRS])
def test_planted_buckets_in_either_set(table_ctx, pair):
    """every record the 2-set launch leaves for the host -- per set the (S, T) pairs of 16 column blocks and 8 row blocks -- against
    m G for the m its definition gives, with one planted launch in set 0 and another in set 1; then both final points"""
    c, key = table_ctx
    tagged = tg.split(pair.scalars, pair.tags)[0]
    reads = []
    got = run_three_times(c, tagged, 16, reads=reads)
    plan = c.msm_last_plan(0)
    for rd in reads if not pair.same_words else reads[:1]:
        bad = wc.check_window_sums(rd, plan, pair.values, pair.cases)
        assert not bad, wc.describe(bad)
    if pair.same_words:
        assert reads[0].tolist() == reads[1].tolist() == reads[2].tolist(), "plain launch, capture and replay left different records"
    assert len(reads[0]) == 2 * 2 * (16 + 8)
    assert got == tg.want(key, pair.scalars, pair.tags)


# ---------------------------------------------------------------------------------------------------- misuse
def test_misuse_is_refused_with_the_drivers_message_and_the_next_call_succeeds(hal, a):
    c = hal.Context(bases=a.key)
    tagged, want = a.case("uniform", "halves")
    code = "(code %d)" % hal.HALO_E_ARG

    def refused(why, *args, **kw):
        with pytest.raises(hal.HaloError) as e:
            c.msm_tagged(*args, **kw)
        assert why in str(e.value) and code in str(e.value), str(e.value)

    try:
        refused(REFUSAL, tagged)  # no table yet: a tagged launch builds none
        build_table(c, tc.N_A, ALL_ROWS)
        assert c.msm_tagged(tagged).tolist() == want
        refused(REFUSAL, tagged[:tc.N_A - 2])  # n % 4 != 0
        assert c.msm_tagged(tagged).tolist() == want
        refused(REFUSAL, tagged[:4092])  # below the least stretch of the table plans
        refused("dev_msm_tagged: range exceeds the context's key", tagged, off=4)
        assert c.msm_tagged(tagged).tolist() == want
        c.set_window_bits(12)
        try:
            refused(REFUSAL, tagged)
        finally:
            c.set_window_bits(0)
        assert c.msm_tagged(tagged).tolist() == want
        c.set_table_mode(0)  # (releases the table)
        try:
            refused(REFUSAL, tagged)
        finally:
            c.set_table_mode(-1)
        refused(REFUSAL, tagged)  # the table is gone until the next table MSM
        build_table(c, tc.N_A, ALL_ROWS)
        assert c.msm_tagged(tagged).tolist() == want
        assert_plan(c, 16)
        assert assert_two_set_kernels(c, tagged, 16) == want
    finally:
        c.close()
