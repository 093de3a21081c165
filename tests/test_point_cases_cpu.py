"""tests/point_cases.py checks itself: every level of the two small-MSM kernels' trees is the first to meet every exceptional
addition in some case (the table is printed), the oracle and the integer model agree on every cancelling, doubling and edge-scalar
sum and on the URS derivation at indices either side of 2^32 and above 2^63, the Jacobian groups hold what they promise, and the
checkers reject every single mutation of a correct result, naming it -- the GPU tests over them (tests/test_gpu_point_paths.py)
cannot pass vacuously."""
import numpy as np
import pytest

import orc
import pallas_model as pm
import point_cases as pc
import table_cases as tc


# ---------------------------------------------------------------------------------------------------- small-MSM sums
def test_every_level_of_both_trees_is_the_first_to_meet_every_event():
    cases = pc.all_sum_cases()
    table = pc.coverage(cases)
    print(pc.format_coverage(table))
    print("%d sums, %d different terms" % (len(cases), pc.unique_terms()))
    for kernel, levels in table.items():
        for off in pc.LEVELS:
            for ev in pc.EVENTS:
                assert levels[off][ev], "%s: no case makes off = %d the first level to meet %s" % (kernel, off, ev)
    assert pc.unique_terms() < 3500, "the references stay in seconds"


def test_the_listed_cases_are_there():
    names = [c.name for c in pc.msm_cases()]
    for K in (2, 3, 33, 63, 64):
        assert "all %d terms equal" % K in names
    for off in pc.LEVELS:
        for how in ("negated point, same scalar", "same point, scalar r - k"):
            assert any(n.startswith("sparse, off = %d: %s" % (off, how)) for n in names)
    for what in ("whole sum of", "first half of", "at term 0", "at term K - 1", "at alternating", "finite point with scalar 0", "terms infinite"):
        assert any(what in n for n in names), what
    for nm, k in pc.EDGE_SCALARS:
        assert 0 <= k < pc.R and "scalar %s on an ordinary point" % nm in names
    want = {0, 1, 2, 3, pc.R - 1, pc.R - 2, (pc.R - 1) // 2, (pc.R + 1) // 2, 1 << 253, 1 << 254, (1 << 254) - 1}
    want |= {x for j in range(1, 8) for x in ((1 << 32 * j) - 1, 1 << 32 * j, pc.R - (1 << 32 * j))}
    assert {k for _, k in pc.EDGE_SCALARS} == want
    whole = [c for c in pc.msm_cases() if c.name.startswith("whole sum") or "terms infinite" in c.name]
    assert whole and all(c.canon is None for c in whole)
    assert all(c.canon is not None for c in pc.msm_cases() if c.name.startswith("first half"))


def test_the_launches_and_lists_have_the_stated_shapes():
    launches = pc.batch_launches()
    assert {K for K, _ in launches} == set(pc.BATCH_K) >= {1, 2, 22, 42, 63, 64}
    for K in pc.BATCH_K:
        assert {len(l) for k, l in launches if k == K} == set(pc.BATCH_M)
    for K, launch in launches:
        assert all(c.K == K for c in launch) and len({c.canon for c in launch}) == len(launch), "pairwise different sums"
    placed = {id(c) for _, l in launches for c in l}
    assert all(id(c) in placed for c in pc.msm_cases() if c.K in pc.BATCH_K)
    lists = pc.seg_lists()
    assert {1, 2, 3, 5, 9, 17, 33, 64} <= {c.K for l in lists for c in l}, "1, 2, 3, 5, 17, 33, 64 and w / 2 + 1 for every w"
    assert all(id(c) in {id(x) for l in lists for x in l} for c in pc.msm_cases())
    for l in lists:
        assert len({pc.seg_width(c.K) for c in l}) >= 6, "the widths mix"
        assert any(a.canon is None and b.canon is not None for a, b in zip(l, l[1:])), "a sum that cancels next to a finite one"
        edge = [(a, b) for a, b in zip(l, l[1:]) if a.prods[-1] is not None and a.prods[-1] == pm.neg(b.prods[0])]
        assert edge, "the last term of one sum is the negation of the first term of the next"
    assert any(sum(pc.seg_width(c.K) for c in l) % 64 for l in lists), "one list leaves idle lanes in its last wave"


def test_the_two_references_agree_on_the_stated_subset():
    """orc_point_mul / orc_point_add against pallas_model.mul / add on every cancelling, doubling and edge-scalar case"""
    subset = [c for c in pc.all_sum_cases() if c.both]
    for c in subset:
        assert pc.model_sum(c.terms) == c.canon, c.name
    names = " | ".join(c.name for c in subset)
    for what in ("first to meet P + P", "first to meet P + (-P)", "first to meet inf + inf", "sparse, off = 1:", "terms equal", "cancel", "scalar r - 1 on", "edge scalars"):
        assert what in names, what
    print("%d of %d sums through both references" % (len(subset), len(pc.all_sum_cases())))
    assert len(subset) >= 100


def _jac_of(canon):
    return tc._jac(tc.aff_words(canon))


SUM_MUTATIONS = ["neighbours swapped", "the neighbour's first term added", "reported infinite", "reported finite"]


@pytest.mark.parametrize("what", SUM_MUTATIONS)
def test_the_sum_checker_rejects_every_single_mutation_and_names_it(what):
    groups = [l for _, l in pc.batch_launches() if len(l) > 1] + pc.seg_lists()
    tried = 0
    for cases in groups:
        good = np.stack([c.want for c in cases])
        assert pc.check_sums(good, cases) == []
        for s in range(len(cases) - 1):
            a, b = cases[s], cases[s + 1]
            got = good.copy()
            named = {s}
            if what == "neighbours swapped":
                if a.canon == b.canon:
                    continue
                got[[s, s + 1]] = good[[s + 1, s]]
                named = {s, s + 1}
            elif what == "the neighbour's first term added":
                if b.prods[0] is None:
                    continue
                got[s] = pc.orc_sum([good[s], pc.product(b.terms[0])[0]])
            elif what == "reported infinite":
                if a.canon is None:
                    continue
                got[s] = _jac_of(None)
            else:
                if a.canon is not None:
                    continue
                got[s] = _jac_of(pc.base_point(7))
            bad = pc.check_sums(got, cases)
            assert {i for i, _ in bad} == named and all(nm == cases[i].name for i, nm in bad), (what, s, bad)
            tried += 1
    print("%s: %d mutations, each rejected and named" % (what, tried))
    assert tried >= (10 if what == "reported finite" else 500)


# ---------------------------------------------------------------------------------------------------- Jacobian groups
def test_the_jacobian_groups_hold_what_they_promise():
    groups = pc.jac_groups()
    assert [g.m for g in groups] == list(pc.STEP_SIZES) + [m for m in pc.RAGGED_SIZES for _ in range(2)]
    a, b = groups[0], groups[1]
    assert tc.step_stride(a.m) == 256 and 3 * 256 < a.m < 4 * 256, "stride 256 with a partial stripe e = 3"
    assert tc.step_stride(b.m) == 512
    for g in (a, b):
        cl = " | ".join(g.classes)
        for what in pc.Z_CLASSES + pc.INF_SPELLINGS + ["copy of G[", "negation of G[", "same lane", "every point of lane 7", "lane that pads"]:
            assert what in cl, (g.name, what)
        copies = [i for i, c in enumerate(g.classes) if c.startswith("copy of G[%d]" % tc.ORIGINAL)]
        assert len({g.jac[i, 8:].tobytes() for i in copies}) > 4 and len({g.want[i].tobytes() for i in copies}) == 1, "one point under many Z"
        assert (g.want[copies[0]] == g.want[tc.ORIGINAL]).all()
        negs = [i for i, c in enumerate(g.classes) if c.startswith("negation of G[%d]" % tc.ORIGINAL)]
        assert all((g.want[i] == tc.negated(g.want[tc.ORIGINAL])).all() for i in negs)
    for g in groups:
        inf = set(g.infinite())
        assert inf == {i for i in range(g.m) if not g.want[i].any()} == {i for i, c in enumerate(g.classes) if c.startswith("inf")}
        for i in range(g.m):  # the reference, once more from the words: on the curve, and X = x Z^2, Y = y Z^3
            if i not in inf:
                x, y = pc.model_point(g.want[i])
                X, Y, Z = (tc._int(g.jac[i, k:k + 4]) * tc.RINV % pc.P for k in (0, 4, 8))
                assert pm.is_on_curve((x, y)) and (x * Z * Z - X) % pc.P == 0 and (y * Z * Z * Z - Y) % pc.P == 0
        if "planted" in g.name:
            s = tc.step_stride(g.m)
            assert {0, g.m - 1} <= inf
            if g.m > 3:
                lane = 2 if g.m <= 5 else 5
                assert {lane + e * s for e in range(4) if lane + e * s < g.m} <= inf
            spelled = [g.jac[i, :8].any() for i in inf]
            assert g.m < 3 or (any(spelled) and not all(spelled)), "Z = 0 over zero and over non-zero X, Y"
        elif "plain" in g.name:
            assert not inf


AFFINE_MUTATIONS = ["one word flipped", "finite reported infinite", "infinite reported finite", "neighbours swapped"]


@pytest.mark.parametrize("what", AFFINE_MUTATIONS)
def test_the_affine_checker_rejects_every_single_mutation_and_names_it(what):
    tried = 0
    for g in pc.jac_groups():
        assert pc.check_affine(g.want, g) == []
        inf = set(g.infinite())
        for i in range(0, g.m, max(1, g.m // 97)):
            got = g.want.copy()
            named = {i}
            if what == "one word flipped":
                got[i, (3 * i) % 8] ^= np.uint64(1 << (i % 64))
            elif what == "finite reported infinite":
                if i in inf:
                    continue
                got[i] = 0
            elif what == "infinite reported finite":
                i = min(inf, key=lambda j: abs(j - i)) if inf else None
                if i is None:
                    continue
                got[i] = tc.aff_words(pc.base_point(9))
                named = {i}
            else:
                if i + 1 >= g.m or (g.want[i] == g.want[i + 1]).all():
                    continue
                got[[i, i + 1]] = g.want[[i + 1, i]]
                named = {i, i + 1}
            bad = pc.check_affine(got, g)
            assert {j for j, _ in bad} == named and all(c == g.classes[j] for j, c in bad), (g.name, what, i, bad)
            tried += 1
    print("%s: %d mutations, each rejected and named" % (what, tried))
    assert tried >= 100


# ---------------------------------------------------------------------------------------------------- URS runs
def test_oracle_and_model_agree_on_the_derivation():
    """orc.urs_affine (the reference of the GPU test) against pallas_model.get_generator_hash (hashlib's SHA3) at the first and last
    index of every run and either side of 2^32 -- the oracle's C restatement serialises the whole 64-bit index"""
    triples = pc.urs_triples()
    assert len(triples) == 45
    seen, crossing = {}, 0
    for first, stride, n in triples:
        want = pc.urs_expected(first, stride, n)
        assert want.shape == (n, 8)
        pos = pc.urs_model_positions(first, stride, n)
        crossing += any(pc.urs_index(first, stride, i) < 1 << 32 <= pc.urs_index(first, stride, i + 1) and {i, i + 1} <= set(pos) for i in range(n - 1))
        for i in pos:
            idx = pc.urs_index(first, stride, i)
            if idx not in seen:
                seen[idx] = tc.aff_words(pm.get_generator_hash(idx))
            assert (want[i] == seen[idx]).all(), (first, stride, n, i, idx)
    assert crossing == 15, "runs that cross 2^32"
    assert sum(1 for i in seen if i >= 1 << 32) >= 20 and max(seen) >= (1 << 63) + 1024 * (1 << 33)
    assert {(1 << 32) - 1, 1 << 32} <= set(seen)
    print("%d triples, %d indices through both references, the largest %d" % (len(triples), len(seen), max(seen)))


def test_the_urs_checker_names_a_wrong_point():
    first, stride, n = (1 << 32) - 3, 1, 257
    good = pc.urs_expected(first, stride, n)
    assert pc.check_urs(good, first, stride, n) == []
    low = pc.urs_expected(2, 1, 257)  # what a derivation that dropped the index's high half would give from 2^32 on: another run
    bad = good.copy()
    bad[3:] = orc.urs_affine(0, n - 3)
    assert [i for i, _ in pc.check_urs(bad, first, stride, n)] == list(range(3, n)) and pc.check_urs(bad, first, stride, n)[0][1] == 1 << 32
    assert len(pc.check_urs(low, first, stride, n)) == n
