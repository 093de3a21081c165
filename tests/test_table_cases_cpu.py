"""tests/table_cases.py checks itself: the checkers of the table-build tests (tests/test_gpu_table_build.py) accept a table built on
the CPU with pallas_model and reject every single mutation of it, naming the entry -- they cannot pass vacuously.  The generator
of the exceptional key keeps its promises, and the oracle's two MSMs agree over such a key (it is the GPU tests' only reference)."""
import numpy as np
import pytest

import orc
import pallas_model as pm
import table_cases as tc

P = pm.P
ROWS, INF_AT = 6, 5


@pytest.fixture(scope="module")
def table():
    """T[j][i] = 2^j G_i: 8 points (one of them infinity), 6 rows -> (points, (6, 8, 8) affine words)"""
    pts = [pm.mul(pm.GENERATOR, k) for k in (1, 2, 3, 0x1234567, pm.R_ORDER - 5)] + [None] + [pm.mul(pm.GENERATOR, k) for k in ((1 << 200) + 7, 11)]
    assert pts[INF_AT] is None and len(pts) == 8
    rows = [[pm.mul(g, 1 << j) for g in pts] for j in range(ROWS)]
    return rows, np.stack([np.stack([tc.aff_words(g) for g in r]) for r in rows])


def _fails(t):
    return {(r, i) for r, i, _ in tc.check_doubling_rows(t[:-1], t[1:])}


def _coord(v):
    return [(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)]


def test_the_checkers_accept_a_correct_table(table):
    rows, t = table
    counted = [0]
    assert tc.check_doubling_rows(t[:-1], t[1:], counted=counted) == [] and counted[0] == (ROWS - 1) * 8
    assert tc.check_row0(t[0], t[0]) == []
    for c in (1, 2):  # rows 0, c, 2 c of the table are a table of shifts by c
        sub = t[::c]
        counted = [0]
        assert tc.check_shift_rows(t[0], sub, c, range(8), counted=counted) == [] and counted[0] == 8 * sub.shape[0]


MUTATIONS = ["bit of x'", "y' negated", "infinite for finite", "finite for infinite", "x' + p", "y' + p", "columns swapped", "row not doubled"]


@pytest.mark.parametrize("what", MUTATIONS)
@pytest.mark.parametrize("row", [1, 3, ROWS - 1])
def test_the_doubling_check_rejects_every_single_mutation_and_names_it(table, what, row):
    rows, good = table
    t = good.copy()
    col = 2
    if what == "bit of x'":
        t[row, col, 1] ^= np.uint64(1 << 17)
    elif what == "y' negated":  # -2 P: right x', on the curve -- a check of x' alone would pass it
        t[row, col] = tc.negated(t[row, col])
        assert (t[row, col, :4] == good[row, col, :4]).all()
    elif what == "infinite for finite":
        t[row, col] = 0
    elif what == "finite for infinite":
        col = INF_AT
        t[row, col] = good[row, 0]
    elif what in ("x' + p", "y' + p"):  # the right value mod p, not canonical (p < 2^255: the sum fits the words)
        k = 0 if what[0] == "x" else 4
        t[row, col, k:k + 4] = _coord(tc._int(good[row, col, k:k + 4]) + P)
    elif what == "columns swapped":
        t[row, [col, col + 1]] = good[row, [col + 1, col]]
    else:
        t[row] = good[row - 1]
    bad = _fails(t)
    if what == "row not doubled":  # every finite column of the row; the infinite column is right as it is
        assert bad >= {(row, i) for i in range(8) if i != INF_AT} and not any(i == INF_AT for _, i in bad)
        return
    cols = {col, col + 1} if what == "columns swapped" else {col}
    assert bad >= {(row, i) for i in cols}, "the mutated entry is not named"
    # (the row above doubles a wrong entry: it may be named too -- nothing else)
    assert bad <= {(r, i) for r in (row, row + 1) for i in cols}, bad
    if what in ("x' + p", "y' + p"):
        assert bad == {(row, col)}


def test_the_other_checkers_reject_too(table):
    rows, good = table
    t = good.copy()
    t[0, 4, 7] ^= np.uint64(1)
    assert tc.check_row0(t[0], good[0], classes=list("abcdefgh")) == [(0, 4, "e")]
    sub = good[::2].copy()
    sub[1, 3] = tc.negated(sub[1, 3])
    sub[2, INF_AT] = good[0, 0]
    sub[2, 6] = 0
    assert {(r, i) for r, i, _ in tc.check_shift_rows(good[0], sub, 2, range(8))} == {(1, 3), (2, INF_AT), (2, 6)}
    assert tc.check_shift_rows(good[0], sub, 2, [0, 1, 7]) == []  # only the columns asked for


def _cheap_key(n):
    """n distinct finite points without a scalar multiplication each: G, 2 G, 3 G, ..."""
    out, acc = [], None
    for _ in range(n):
        acc = pm.add(acc, pm.GENERATOR)
        out.append(tc.aff_words(acc))
    return np.stack(out)


@pytest.fixture(scope="module")
def key_a():
    return tc.exceptional_key(_cheap_key(tc.N_A))


def test_the_exceptional_key_has_what_it_promises(key_a):
    key, cls = key_a
    n = tc.N_A
    inf = {i for i in range(n) if not key[i].any()}
    assert inf == {i for i, c in enumerate(cls) if c.startswith("inf")}
    lane = lambda i: (i % 4096) % 256
    e_of = lambda i: (i % 4096) // 256
    assert {7 + 256 * e for e in range(16)} <= inf and 4096 in inf and n - 1 in inf and any(lane(i) == 0 and i < 4096 for i in inf)
    es = {e_of(i): lane(i) for i in inf if i < 4096 and lane(i) not in (0, 7)}
    assert {0, 8, 15} <= set(es) and len({es[0], es[8], es[15]}) == 3, "infinities at e = 0, a middle e and e = 15, each on its own lane"
    src = tc.original_of(cls)
    copies = sorted(i for i, c in enumerate(cls) if c.startswith("copy of"))
    negs = sorted(i for i, c in enumerate(cls) if c.startswith("negation of"))
    for run in (copies, negs):
        assert len(run) == 64 and run[-1] - run[0] == 63 and run[0] % 64 != 0
    g = key[tc.ORIGINAL]
    assert all((key[i] == g).all() for i in copies) and all((key[i] == tc.negated(g)).all() for i in negs)
    pairs = [(i, s) for i, s in src.items() if i not in copies and i not in negs]
    assert len(pairs) == 2 and all(i == s + 256 for i, s in pairs)
    assert sorted((key[i] == key[s]).all() for i, s in pairs) == [False, True]
    assert all((key[i, :4] == key[s, :4]).all() for i, s in pairs)
    assert all(pm.is_on_curve((tc._int(key[i, :4]) * tc.RINV % P, tc._int(key[i, 4:]) * tc.RINV % P)) for i in tc.planted(cls) if i not in inf)
    # the same classes on the stripes of k_table_step
    n_b = (1 << 12) + 260
    kb, cb = tc.exceptional_key(_cheap_key(n_b), "step")
    s = tc.step_stride(n_b)
    assert s == 1280 and {7 + s * e for e in range(4)} <= {i for i in range(n_b) if not kb[i].any()}
    assert tc.original_of(cb)[1000 + s] == 1000 and any(c.endswith("lane that pads") for c in cb)
    cols = tc.step_columns(n_b, cb)
    assert set(tc.planted(cb)) <= set(cols) and {0, s - 1, s, 3 * s, n_b - 1} <= set(cols) and len(cols) < 400


def test_the_oracles_two_msms_agree_over_the_exceptional_key(key_a):
    """orc.msm_affine (the reference of the GPU tests) against the oracle's double-and-add sum, over repeated, opposite and
    infinite points"""
    key, cls = key_a
    sets = tc.scalar_sets(tc.N_A, cls, 7)
    assert set(sets) == set(tc.SCALAR_SETS)
    for name in ("uniform", "equal", "paired", "one_on_infinity"):
        sc = tc.scalar_mont(sets[name])
        got = orc.msm_affine(key, sc)
        assert got.tolist() == orc.msm_naive(key, sc).tolist(), name
        assert (orc.point_canonical(got) is None) == (name in tc.INFINITE_RESULT), name
    # what cancels: the run of negations against the run of copies, the opposite pair -- the sum without them is the same
    src = tc.original_of(cls)
    gone = {i for i, c in enumerate(cls) if c.startswith(("copy", "negation", "-G["))} | {src[i] for i, c in enumerate(cls) if c.startswith("-G[")}
    keep = [i for i in range(tc.N_A) if i not in gone]
    assert len(gone) == 130 and orc.msm_affine(np.ascontiguousarray(key[keep]), np.ascontiguousarray(sc[keep])).tolist() == orc.msm_affine(key, sc).tolist()
    assert tc.scalar_words(sets["top_2_254"]).max() >= 1 << 62 and max(sets["top_2_254"]) >= pm.R_ORDER
