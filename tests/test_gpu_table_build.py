"""The MSM's fixed-base tables entry by entry (msm_table.hip k_table_all_shifts, k_table_step), read back through the development
library's halo_dev_table_read, over keys with infinite, repeated and opposite points planted where the build kernels have their
edges (tests/table_cases.py) and whose sizes are no powers of two: a partial block, partial stripes, padding lanes.

    key A, 4096 + 260 points   the 255-row all-shifts table: EVERY entry against the affine doubling law over Python integers; the
                               13-row table of k_table_step (c = 20, grid stride 1280): every entry against rows 20 w of the former,
                               and a stated set of columns against the oracle's scalar multiplication
    key B, 2^17 + 260 points   the 15-row table of the c = 17 plan (128 coarse ranges): a stated set of columns against the oracle
    MSMs over both keys        every launch form, against orc.msm_affine alone, limb for limb: the bucket chains meet P + P, P + (-P)
                               and infinite table entries on table rows with signed digits

The keys' base points are the device's URS (pinned by the known-answer test elsewhere); the exceptions are planted on the host."""
import numpy as np
import pytest

import orc
import table_cases as tc

pytestmark = pytest.mark.gpu

N_A, N_B = tc.N_A, (1 << 17) + 260
ALL_ROWS, BAND = 255, 51
NO_TABLE, FIXED, SLIDING = 0, 1, 22  # halo_ctx_info(ctx, 9): the plan of the launch enqueued last (sliding: window width + 1)


@pytest.fixture(scope="module")
def hal():
    import halo_accumulation_amd as h
    return h._lib


@pytest.fixture(autouse=True)
def slide_from_4096(hal):
    """key A takes the c = 20 plans (tests/conftest.py resets the development hooks after every test)"""
    hal.dev_hook("table_slide_min", 4096)
    yield


def _urs(hal, n):
    c = hal.Context(urs_n=n)
    try:
        return c.read_bases()
    finally:
        c.close()


def _read_rows(c):
    return np.stack([c.table_read(j) for j in range(c.info(8))])


class Key:
    """an exceptional key, its scalar sets resident on the device, the oracle's MSM of each (computed once, when first asked for)"""

    def __init__(self, hal, n, layout, seed):
        import torch
        self.n = n
        self.key, self.classes = tc.exceptional_key(_urs(hal, n), layout)
        self.sets = tc.scalar_sets(n, self.classes, seed)
        self.dev = {k: torch.from_numpy(tc.scalar_words(v).view(np.int64).copy()).cuda() for k, v in self.sets.items()}
        self._want = {}
        self.ctxs = []

    def context(self, hal):
        c = hal.Context(bases=self.key)
        self.ctxs.append(c)
        return c

    def ptr(self, name, off=0):
        """the scalars of `name` from index off on (device)"""
        return self.dev[name][off:].data_ptr()

    def want(self, name, off=0, m=None):
        m = self.n - off if m is None else m
        if (name, off, m) not in self._want:
            sc = tc.scalar_mont(self.sets[name][off:off + m])
            got = orc.msm_affine(np.ascontiguousarray(self.key[off:off + m]), sc)
            assert (orc.point_canonical(got) is None) == (name in tc.INFINITE_RESULT), name
            self._want[(name, off, m)] = got.tolist()
        return self._want[(name, off, m)]

    def close(self):
        for c in self.ctxs:
            c.close()


@pytest.fixture(scope="module")
def a(hal):
    """key A: a context with the all-shifts table (read once, all 255 rows), one with the 13 rows of k_table_step, one table-free"""
    hal.dev_hook("table_slide_min", 4096)
    k = Key(hal, N_A, "all_shifts", 0x7461626C65)
    k.slide = k.context(hal)
    k.slide.msm_dev(k.ptr("uniform"), N_A, mont=False)  # builds the table
    assert k.slide.info(8) == ALL_ROWS and k.slide.info(9) == SLIDING, "no all-shifts table: nothing here would test it"
    k.table = _read_rows(k.slide)
    k.fixed = k.context(hal)
    k.fixed.set_table_mode(1)
    k.fixed.msm_dev(k.ptr("uniform"), N_A, mont=False)
    assert k.fixed.info(8) == 13 and k.fixed.info(9) == FIXED, "no 13-row table: k_table_step has not run"
    k.general = k.context(hal)
    k.general.set_table_mode(0)
    k.general.set_small_path(0)
    yield k
    k.close()


@pytest.fixture(scope="module")
def b_key(hal):
    hal.dev_hook("table_slide_min", 0)
    k = Key(hal, N_B, "step", 0x6B657942)
    k.c = k.context(hal)
    k.c.msm_dev(k.ptr("uniform"), N_B, mont=False)
    assert k.c.info(8) == 15 and k.c.info(9) == FIXED, "no 15-row table: the c = 17 plan has not run"
    yield k
    k.close()


@pytest.fixture
def b(b_key, hal):
    """key B takes the c = 17 plan: the hook that key A needs is off while its launches are enqueued"""
    hal.dev_hook("table_slide_min", 0)
    return b_key


# ---------------------------------------------------------------------------------------------------- table contents
@pytest.mark.parametrize("band", range(ALL_ROWS // BAND))
def test_every_entry_of_the_all_shifts_table(a, band):
    """rows [51 band, 51 band + 51), every column: row 0 is the key word for word, every other row doubles the row before it"""
    t, lo = a.table, band * BAND
    assert t.shape == (ALL_ROWS, N_A, 8)
    counted, bad = [0], []
    if band == 0:
        bad += tc.check_row0(t[0], a.key, a.classes)
        counted[0] += N_A
        lo = 1
    hi = (band + 1) * BAND
    bad += tc.check_doubling_rows(t[lo - 1:hi - 1], t[lo:hi], first_row=lo, classes=a.classes, counted=counted)
    assert counted[0] == BAND * N_A, "entries left out"
    assert not bad, tc.describe(bad)


def test_every_entry_of_the_13_row_table(a):
    """k_table_step with c = 20 over 4356 points: stride 1280, stripe e = 3 partial, lanes 516 .. 1279 pad with infinity"""
    t13 = _read_rows(a.fixed)
    assert t13.shape == (13, N_A, 8) and tc.step_stride(N_A) == 1280
    bad = tc.check_row0(t13[0], a.key, a.classes)
    for w in range(1, 13):  # word for word: both tables hold canonical words (the all-shifts rows were checked for it)
        bad += [(w, int(i), a.classes[i]) for i in np.nonzero((t13[w] != a.table[20 * w]).any(axis=1))[0]]
    assert not bad, "against rows 20 w of the all-shifts table: " + tc.describe(bad)
    cols = tc.step_columns(N_A, a.classes)
    assert set(tc.planted(a.classes)) <= set(cols) and {0, 1279, 1280, 3840, N_A - 1} <= set(cols)
    counted = [0]
    bad = tc.check_shift_rows(a.key, t13, 20, cols, a.classes, counted)
    assert counted[0] == 13 * len(cols)
    assert not bad, "against the oracle: " + tc.describe(bad)


def test_the_15_row_table_of_the_c17_plan(b):
    """k_table_step with c = 17 over 2^17 + 260 points (stride 33024): every planted index, the first and last 8 indices of each of
    the four stripes and the last 8 of the key, 15 rows each, against the oracle"""
    t = _read_rows(b.c)
    assert t.shape == (15, N_B, 8) and tc.step_stride(N_B) == 33024
    bad = tc.check_row0(t[0], b.key, b.classes)
    assert not bad, tc.describe(bad)
    cols = tc.step_columns(N_B, b.classes)
    assert set(tc.planted(b.classes)) <= set(cols) and {0, 33023, 33024, 3 * 33024, N_B - 1} <= set(cols) and len(cols) >= 200
    # an infinite key entry is (0, 0) on every row, in every column of the key (cheap: the whole table)
    inf = np.array(tc.is_infinite(b.classes))
    assert not t[:, inf].any() and t[:, ~inf].any(axis=2).all(), "an infinity where a finite entry belongs, or the reverse"
    counted = [0]
    bad = tc.check_shift_rows(b.key, t, 17, cols, b.classes, counted)
    assert counted[0] == 15 * len(cols)
    assert not bad, tc.describe(bad)


# ---------------------------------------------------------------------------------------------------- MSMs over the keys
def _twice(c, k, name, n, off=0):
    got = c.msm_dev(k.ptr(name, off), n, off=off, mont=False)
    again = c.msm_dev(k.ptr(name, off), n, off=off, mont=False)  # graph replay
    return got.tolist(), again.tolist()


@pytest.mark.parametrize("name", tc.SCALAR_SETS)
@pytest.mark.parametrize("form", ["sliding", "fixed plan on the all-shifts table", "13-row table", "general pipeline"])
def test_msm_over_key_a_against_the_oracle(a, form, name):
    want = a.want(name)
    if form == "sliding":
        got, again = _twice(a.slide, a, name, N_A)
        assert a.slide.info(9) == SLIDING
    elif form == "fixed plan on the all-shifts table":
        a.slide.set_table_mode(1)
        try:
            got, again = _twice(a.slide, a, name, N_A)
            assert a.slide.info(8) == ALL_ROWS and a.slide.info(9) == FIXED
        finally:
            a.slide.set_table_mode(-1)
    elif form == "13-row table":
        got, again = _twice(a.fixed, a, name, N_A)
        assert a.fixed.info(8) == 13 and a.fixed.info(9) == FIXED
    else:
        c = a.general
        got, again = _twice(c, a, name, N_A)
        c.prof_enable(True); c.prof_reset()
        third = c.msm_dev(a.ptr(name), N_A, mont=False).tolist()
        ran = c.prof()
        c.prof_enable(False)
        assert c.info(9) == NO_TABLE and c.info(8) == 0 and third == want
        assert "k_msm_accumulate" in ran and "k_tmsm_recode" not in ran and "k_smsm_accumulate" not in ran, sorted(ran)
    assert got == want and again == want


# (off, m): multiples of 4, at least 4096 points -- the sliding plan takes them; the first begins in the middle of the run of copies,
# the second in the middle of the run of negations and ends at n
STRETCHES = [(tc.COPIES + 30, 4096), (tc.NEGATIONS + 30, N_A - tc.NEGATIONS - 30)]


@pytest.mark.parametrize("name", ["uniform", "equal", "paired"])
@pytest.mark.parametrize("off,m", STRETCHES)
def test_a_stretch_of_key_a_against_the_oracle(a, off, m, name):
    assert m % 4 == 0 and m >= 4096 and off + m <= N_A
    got, again = _twice(a.slide, a, name, m, off)
    assert a.slide.info(9) == SLIDING
    assert got == again == a.want(name, off, m)


@pytest.mark.parametrize("name", tc.SCALAR_SETS)
def test_msm_over_key_b_against_the_oracle(b, name):
    got, again = _twice(b.c, b, name, N_B)
    assert b.c.info(8) == 15 and b.c.info(9) == FIXED
    assert got == again == b.want(name)


@pytest.mark.parametrize("names", [("paired", "equal"), ("top_2_254", "uniform")])
def test_a_batch_of_two_over_key_b_against_the_oracle(b, names):
    for _ in range(2):  # (the second launch is a graph replay)
        b.c.msm_dev_batch_begin(1, [b.ptr(k) for k in names], N_B, mont=False)
        got = b.c.msm_dev_batch_end(1, 2)
        assert b.c.info(9) == FIXED, "the batch did not go through the table"
        assert [g.tolist() for g in got] == [b.want(k) for k in names]
