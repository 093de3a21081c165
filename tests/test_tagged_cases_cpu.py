"""halo_dev_msm_tagged and tests/tagged_cases.py without a GPU: the hook is exported by the development library and by it alone,
declared with its prototype and bound by the Python prototypes, and a null context is an argument error before any device is
touched; the generators of the tagged cases keep their promises -- split() against Python integers and the oracle, the edge values at
every residue mod 31 under both tags, the entry counts of task_len_edge and stage_edge recounted through a restatement of the recode,
the planted launches' coverage table full for either set."""
import os
import re
import subprocess

import numpy as np
import pytest

import orc
import pallas_model as pm
import table_cases as tc
import tagged_cases as tg
import window_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = pm.R_ORDER
NAME = "halo_dev_msm_tagged"


@pytest.fixture(scope="module")
def hal():
    import halo_accumulation_amd as h
    h.build()
    return h


# ---------------------------------------------------------------------------------------------------- the hook
def test_exported_by_the_development_library_alone_declared_and_bound(hal):
    dev = subprocess.check_output(["nm", "-D", "--defined-only", hal._lib.DEV_LIB_PATH], text=True)
    product = subprocess.check_output(["nm", "-D", "--defined-only", hal._lib.LIB_PATH], text=True)
    assert re.search(r" T %s$" % NAME, dev, flags=re.M)
    assert NAME not in product and not re.search(r"halo_(dev|test|bench)_", product), "the product library exports a development symbol"
    assert NAME in hal._lib.declared_dev_symbols() and NAME not in hal._lib.declared_symbols()
    header = open(os.path.join(ROOT, "include", "halo_accumulation_dev.h")).read()
    plain = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert "int halo_dev_msm_tagged(halo_ctx *ctx, size_t off, size_t n, const uint64_t *scalars , uint64_t *out_jac );" in plain
    # the header's prototype, kind by kind, is the Python one
    res, args = hal._lib._DEV_SIGS[NAME]
    assert res.__name__ == "c_int" and [a.__name__ for a in args] == ["c_void_p", "c_ulong", "c_ulong", "LP_c_ulong", "LP_c_ulong"]
    assert callable(hal._lib.Context.msm_tagged)
    assert NAME not in open(os.path.join(ROOT, "include", "halo_accumulation.h")).read()


def test_null_context_and_null_pointers_touch_nothing(hal):
    lib = hal.load()
    p = hal._lib.ptr
    out = np.full(24, 0xA5, dtype=np.uint64)
    sc = np.zeros((4, 4), dtype=np.uint64)
    for args in ((None, 0, 4, p(sc), p(out)), (None, 0, 4, None, p(out)), (None, 0, 4, p(sc), None), (None, 0, 0, None, None), (None, 1 << 40, 4, p(sc), p(out))):
        assert lib.halo_dev_msm_tagged(*args) == hal._lib.HALO_E_ARG
        assert b"null context" in lib.halo_last_error()
    assert (out == 0xA5).all()


# ---------------------------------------------------------------------------------------------------- tags and split
def test_tag_patterns():
    n = 4356
    assert tg.PATTERNS == ("all0", "all1", "alternating", "halves", "random")
    assert set(tg.tags("all0", n)) == {0} and set(tg.tags("all1", n)) == {1}
    assert tg.tags("alternating", n)[:4] == [0, 1, 0, 1]
    h = tg.tags("halves", n)
    assert h == [0] * (n // 2) + [1] * (n - n // 2)
    r = tg.tags("random", n)
    assert r == tg.tags("random", n) and 0.4 * n < sum(r) < 0.6 * n and r != tg.tags("alternating", n)
    assert all(len(tg.tags(pt, n)) == n for pt in tg.PATTERNS)


@pytest.fixture(scope="module")
def key_a():
    """key A over the first points of the URS as the oracle restates it"""
    key, classes = tc.exceptional_key(orc.urs_affine(2, tc.N_A), "all_shifts")
    return key, classes, tg.key_a_sets(tc.N_A, classes, 0x7461626C65)


def test_split_against_python_integers():
    vals = [0, 1, R - 1, 1 << 254, (1 << 254) + 1, 12345 << 200]
    tags = [0, 1, 1, 0, 1, 0]
    tagged, masked = tg.split(vals, tags)
    assert tagged.shape == (6, 4) and tagged.dtype == np.uint64
    for i, (v, t) in enumerate(zip(vals, tags)):
        word = tc._int(tagged[i])
        assert word >> 255 == t and word & (tg.TAG - 1) == v
        assert masked[t][i] == v and masked[1 - t][i] == 0
    assert tc._int(tg.split([0], [1])[0][0]) == 1 << 255, "a tagged zero"
    with pytest.raises(AssertionError):
        tg.split([R], [0])


@pytest.mark.parametrize("name", tg.KEY_A_SETS)
def test_the_two_sums_add_up_to_the_untagged_msm(key_a, name):
    """want[0] + want[1] is the oracle's MSM of the values themselves, for every set and pattern; an empty set is the infinity"""
    key, classes, sets = key_a
    L = orc.lib()
    for pattern in tg.PATTERNS:
        tags = tg.tags(pattern, tc.N_A)
        vals = tg.task_len_edge(tags) if name == "task_len_edge" else sets[name]
        assert len(vals) == tc.N_A and all(0 <= v < R for v in vals)
        w = tg.want(key, vals, tags)
        both = np.zeros(12, dtype=np.uint64)
        L.orc_point_add(orc.ptr(np.array(w[0], dtype=np.uint64)), orc.ptr(np.array(w[1], dtype=np.uint64)), orc.ptr(both))
        whole = orc.msm_affine(key, tc.scalar_mont(vals))
        assert orc.point_canonical(both) == orc.point_canonical(whole), (name, pattern)
        empty = {"all0": [1], "all1": [0]}.get(pattern, []) + ([0, 1] if name in tc.INFINITE_RESULT else [])
        for t in (0, 1):
            assert (orc.point_canonical(np.array(w[t], dtype=np.uint64)) is None) == (t in empty), (name, pattern, t)
        if pattern in tg.ASYMMETRIC and name not in tc.INFINITE_RESULT:
            assert w[0] != w[1], "swapped outputs would pass"


def test_key_a_sets_are_reduced(key_a):
    key, classes, sets = key_a
    assert set(sets) == set(tc.SCALAR_SETS) | {"edge"} and set(tg.KEY_A_SETS) == set(sets) | {"task_len_edge"}
    top = set(sets["top_2_254"])
    assert {1 << 254, (1 << 254) + 1} <= top and max(top) < R and any(v >= R - (1 << 40) for v in top)
    assert all(v >> 254 == 1 for v in top), "every member is at least 2^254"
    assert tc._int(tg.split(sets["zero"], [1] * tc.N_A)[0][7]) == 1 << 255


# ---------------------------------------------------------------------------------------------------- the recode, restated
def test_the_restated_recode_gives_back_the_scalar():
    """sum_w (+-magnitude) 2^(20 w) = s + (i mod 31) r exactly, magnitudes within [0, 2^19], for the edge values at every residue"""
    for v in tg.EDGE_VALUES + [0, 1, (1 << 19), (1 << 19) + 1, (1 << 20) - 1, 0x1234567890ABCDEF0FEDCBA987654321 * ((1 << 120) + 12345) % R]:
        for i in range(62):
            for t in (0, 1):
                st, d = tg.tagged_digits(v | t << 255, i)
                k = i % 31 if 0 < (v >> 240) <= 16384 else 0
                assert st == t and sum((-m if neg else m) << (20 * w) for w, (m, neg) in enumerate(d)) == v + k * R
                assert (sum((-m if neg else m) << (20 * w) for w, (m, neg) in enumerate(d)) - v) % R == 0
    assert tg.tagged_digits(1 << 255, 5) == (1, [(0, 0)] * 13), "a tagged zero lands nowhere"
    # the spread moves the top digit: 31 residues, 31 different top buckets
    assert len({tg.tagged_digits(1 << 240, i)[1][12] for i in range(31)}) == 31


@pytest.mark.parametrize("n", [tc.N_A, tg.N_M])
def test_every_edge_value_at_every_residue_under_both_tags(n):
    vals = tg.edge_set(n)
    assert len(tg.EDGE_VALUES) == 12 and set(vals) == set(tg.EDGE_VALUES)
    every = {(v, rho, t) for v in tg.EDGE_VALUES for rho in range(31) for t in (0, 1)}
    for pattern in ("alternating", "halves") + (("random",) if n == tg.N_M else ()):
        assert tg.edge_coverage(vals, tg.tags(pattern, n)) == every, pattern
    # (4356 points hold each (value, residue) ten or twelve times: a random pattern misses a tag now and then; the union does not)
    got = set()
    for pattern in tg.PATTERNS:
        got |= tg.edge_coverage(vals, tg.tags(pattern, n))
    assert got == every
    # the stretches of key A and both halves see whole blocks
    half = tg.edge_coverage(vals[:n // 2], [0] * (n // 2))
    assert {(v, rho) for v, rho, _ in half} == {(v, rho) for v, rho, _ in every}


@pytest.mark.parametrize("pattern", tg.PATTERNS)
def test_task_len_edge_has_the_buckets_it_claims(pattern):
    tags = tg.tags(pattern, tc.N_A)
    vals = tg.task_len_edge(tags)
    counts = tg.bucket_counts(vals, tags)
    want = {}
    for st in (0, 1):
        if st in tags:
            for kmax, digit in zip(tg.KMAXES, (700, 1000, 3000, 5000)):
                want[st * tg.B + digit - 1] = kmax
                want[st * tg.B + digit] = kmax + 1
    assert counts == want and (len(want) == 16) == (pattern in tg.ASYMMETRIC)
    assert all(tags[i] == st for st in (0, 1) for i, v in enumerate(vals) if v and tg.tagged_digits(v | tags[i] << 255, i)[0] == st)


@pytest.mark.parametrize("swapped", [False, True])
def test_stage_edge_has_the_runs_it_claims(swapped):
    vals, tags = tg.stage_edge(tg.N_M, swapped)
    assert len(vals) == tg.N_M and all(0 <= v < 1 << 19 for v in vals)
    counts = tg.bucket_counts(vals, tags)
    runs = tg.range_counts(counts)
    lo, hi = tg.STAGE_RANGES[0], tg.RANGES + tg.STAGE_RANGES[1]
    exact, over = (hi, lo) if swapped else (lo, hi)
    assert runs == {exact: tg.TBL_STAGE, over: tg.TBL_STAGE + 1}
    for rng_ in (lo, hi):  # every bucket of the range, 35 or 36 entries: one task under a task length of 64
        mine = [k for b, k in counts.items() if b >> tg.FBITS == rng_]
        assert len(mine) == 1024 and set(mine) <= {35, 36} and max(mine) <= 64
    assert 13 * tg.N_M <= 16 * 131072 and (((tg.N_M + 18) // 19) + 3) // 4 * 4 > tg.TBL_TILE


# ---------------------------------------------------------------------------------------------------- planted launches
@pytest.fixture(scope="module")
def planted():
    return tg.planted_pairs()


def test_the_pairs_hold_each_launch_once_in_either_set(planted):
    ks, pairs = planted
    assert len(ks) == wc.TABLE_N
    first, second = [id(p.launches[0]) for p in pairs], [id(p.launches[1]) for p in pairs]
    assert len(set(first)) == len(set(second)) and set(first) == set(second), "a launch that sits in one set only"
    assert all(a != b for a, b in zip(first, second)), "a launch beside itself"
    for p in pairs:
        assert len(p.scalars) == len(p.tags) == wc.TABLE_N and 1 in p.tags and all(0 <= s <= 1 << 19 for s in p.scalars)
        # the tagged array, recounted through the recode: every point sits in the bucket of its set that its launch planted
        got = [{}, {}]
        for i, (s, t) in enumerate(zip(p.scalars, p.tags)):
            st, d = tg.tagged_digits(s | t << 255, i)
            assert all(m == 0 for m, _ in d[1:]) and d[0][1] == 0
            if d[0][0] and ks[i]:
                got[st][d[0][0] - 1] = got[st].get(d[0][0] - 1, 0) + ks[i]
        assert [{b: x for b, x in g.items() if x} for g in got] == p.values, p.name


def test_the_planted_coverage_table_is_full_for_either_set(planted):
    counts = tg.planted_counts(planted[1])
    print(tg.format_counts(counts))
    sites = tg.planted_sites()
    assert len(sites) == 13 + 13 + 10 and len(set(sites)) == len(sites)
    assert set(wc.sites(wc.RC_MID_PLAN)) <= set(sites)
    assert not tg.uncovered(counts), tg.uncovered(counts)
    for s in (0, 1):  # nothing is counted at a site the table does not list
        assert {(k, site) for k, site, _ in counts[s] if "dbl" not in site} <= set(sites)
