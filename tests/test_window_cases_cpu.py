"""tests/window_cases.py tests itself: the coverage table of the built cases is complete, the integer models of the schedules meet
the classes the point arithmetic of pallas_model meets, the checkers reject corrupted read-backs, and the planted scalars give the
digits claimed.  No GPU."""
import numpy as np
import pytest

import orc
import pallas_model as pm
import window_cases as wc
from test_slide_recode_host import recode, slide_host  # noqa: F401 -- the sliding recode compiled for the CPU (fixture)


def test_the_coverage_table_is_complete():
    """every (kernel, site, class) of the four edge classes is met by a built case, for every plan, or is exempt for a structural
    reason -- and no exemption names a level of a scan or of a tree"""
    table = wc.coverage()
    print(wc.format_coverage(table))
    assert not wc.uncovered(table)
    for kern, site, cl, cond, why in wc.UNREACHABLE:
        assert not site.startswith(("scan", "tree")) and cl in wc.EDGE and why
    for key in wc.PLAN_SET:
        plan, _, cases = wc.build_cases(key[1], key[2], key[0])
        for case in cases:  # the target is met; an equal or opposite pair is the window's only one (natural_events aside)
            assert case.counts.get(case.target, 0) >= 1, case.name()
            if case.target[2] in ("P+P", "P-P"):
                others = [k for k in case.counts if k[2] in ("P+P", "P-P") and k != case.target and k not in wc.natural_events(plan)]
                assert not others, (case.name(), others)
            assert max(abs(x) for x in case.values.values()) * plan["B"] ** 2 < wc.LIMIT


def test_the_planted_launches_meet_every_class_at_every_site():
    """the launches planted by hand -- k_msm_combine, the partial loop and the heavy pre-sum of k_smsm_reduce, k_msm_reduce_rc in its
    five shapes, the host's Horner and its row / column forms -- meet P+P, P-P, inf+Q and
    Q+inf at every site, with no exemption.  Cells marked * : the sort's atomics decide which task holds the odd entry, both
    placements are counted, and a run on the device meets one of the two (EITHER_SIDE)"""
    counts = wc.planted_counts()
    sites = wc.planted_sites(counts)
    for k, s in sites:
        star = lambda cl: "*" if (k, s) in wc.EITHER_SIDE and cl in ("inf+Q", "Q+inf") else ""
        print("%-20s %-18s %s" % (k, s, "  ".join("%s %d%s" % (cl, counts.get((k, s, cl), 0), star(cl)) for cl in wc.EDGE)))
    print("* one of the two on the device: which task holds the odd entry is the sort's atomics'")
    assert all(site in sites for site in wc.EITHER_SIDE)
    kernels = {k for k, _ in sites}
    assert kernels == {wc.K_COMBINE, wc.K_SREDUCE, "k_msm_reduce_rc", wc.K_HOST}
    for name, top in (("col", 32), ("row", 32)):  # every level of every tree shape: 64, 32 and 16 lanes
        assert all(("k_msm_reduce_rc", "%s tree/%d" % (name, 32 >> t)) in sites for t in range(6))
    assert all((wc.K_COMBINE, "tree/%d" % (32 >> t)) in sites and (wc.K_SREDUCE, "heavy tree/%d" % (32 >> t)) in sites for t in range(6))
    for site in ("cols t+=T", "cols run+=S", "cols tot+=run", "cols t+tot", "rows t+=T", "rows run+=S", "rows tot+=run", "rows t+tot", "cols - plain",
                 "rows - plain", "cw + rw", "+ s_all", "cols + rows", "horner"):
        assert (wc.K_HOST, site) in sites, site
    missing = [(k, s, cl) for k, s in sites for cl in wc.EDGE if not counts.get((k, s, cl))]
    assert not missing, missing


def test_span_one_is_the_default_plan_below_c_13():
    for c in (7, 8, 10):
        assert dict(wc.small_plan(c), span=1) == wc.small_plan(c, 1)
    assert wc.small_plan(13)["L"] == 8 and wc.small_plan(13, 1)["L"] == 1


def _small_values(rng, n):
    """integers in [-3, 3]: zeros, repeats and opposites everywhere"""
    return [int(rng.next_u64() % 7) - 3 for _ in range(n)]


def _replay(run, to_point):
    """run(recorder, convert) over integers and over points: the same classes at the same sites in the same order, the result m G"""
    ir, pr = wc.IntRec(keep=True), wc.PointRec()
    m = run(ir, lambda x: x)
    pt = run(pr, to_point)
    assert ir.events == pr.events
    assert pt == to_point(m)
    return len(ir.events)


@pytest.mark.parametrize("pipeline", [0, 1])
def test_the_models_against_pallas_model(pipeline):
    """seeded small plans (B = 64 .. 256, L = 1 .. 4, 1 .. 4 segments): every schedule replayed over real points"""
    G = wc.g_model()
    pts = {m: pm.mul(G, m) if m >= 0 else pm.neg(pm.mul(G, -m)) for m in range(-40, 41)}
    assert all(pts[m] == wc.multiple(m) for m in pts)
    to_point = lambda m: pts[m] if m in pts else (pm.mul(G, m) if m >= 0 else pm.neg(pm.mul(G, -m)))
    rng, events = pm.SplitMix64(0x6D6F64656C + pipeline), 0
    for seed in range(100):
        L = 1 << (seed % 3)
        nseg = 1 + rng.next_u64() % 4
        B = 64 * L * nseg - (0 if pipeline == 0 else int(rng.next_u64() % 3))
        live = 1
        while live < nseg:
            live <<= 1
        plan = dict(pipeline=pipeline, B=B, L=L, logL=L.bit_length() - 1, nseg=nseg, live_seg=live)
        v = _small_values(rng, B)
        if pipeline == 0:
            events += _replay(lambda rec, cv: wc.model_window(rec, plan, [cv(x) for x in v]), to_point)
        else:  # partials: up to 6 per bucket (more than 4: the heavy pre-sum)
            parts = [[x for x in _small_values(rng, rng.next_u64() % 7 if rng.next_u64() % 8 == 0 else 1)] for _ in range(B)]
            events += _replay(lambda rec, cv: wc.model_window(rec, plan, None, 0, [[cv(x) for x in p] for p in parts]), to_point)
    for seed in range(40):
        tasks = _small_values(rng, 2 + rng.next_u64() % (7 if seed % 2 else 80))
        events += _replay(lambda rec, cv: wc.model_combine(rec, [cv(x) for x in tasks]), to_point)
        sums = _small_values(rng, 6)
        events += _replay(lambda rec, cv: wc.model_horner(rec, [cv(x) for x in sums], 3), to_point)
        e = _small_values(rng, 64)
        events += _replay(lambda rec, cv: wc.model_window(rec, wc.RC_MID_PLAN, [cv(x) for x in e]), to_point)
    assert events > 100000
    if pipeline == 0:  # the row / column sums and the host's table forms, over small shapes and values; the planted task lists
        for seed in range(12):
            lg_rows, lg_cols, per = 6 + seed % 2, 6 + (seed // 2) % 2, 4 << (seed % 3)
            cells = {(int(rng.next_u64() % (1 << lg_rows)), int(rng.next_u64() % (1 << lg_cols))): x for x in _small_values(rng, 150) if x}
            _replay(lambda rec, cv: sum_points(rec, wc.model_reduce_rc(rec, {k: cv(x) for k, x in cells.items()}, lg_rows, lg_cols, per)), to_point)
            values = {(r << lg_cols) + c: x for (r, c), x in cells.items()}
            for pipe in (2, 3):
                plan = dict(pipeline=pipe, form=2, lg_rows=lg_rows, lg_cols=lg_cols)
                vals = values if pipe == 2 else {(c << lg_rows) + r: x for (r, c), x in cells.items()}
                _replay(lambda rec, cv: wc.model_host_rc(rec, plan, vals, cv), to_point)
        g, k = wc.COMBINE_G, wc.COMBINE_KMAX
        for tasks in ([k * g] * 65, [0] + [k * g] * 63, [k * g] * 127 + [-k * g], [-24 * g] + [k * g] * 63, [k * g, 0], [0, 0]):
            _replay(lambda rec, cv: wc.model_combine(rec, [cv(x) for x in tasks]), to_point)


def sum_points(rec, sums):
    """(column sums, row sums) -> one value the replay can compare: the columns' total"""
    acc = rec.zero
    for x in sums[0]:
        acc = rec.add("check", "total", acc, x)
    return acc


def _records(plan, values):
    """the read-back a correct launch leaves: Jacobian words of m G per record"""
    out = np.zeros((len(wc.expected_records(plan, values)), 12), dtype=np.uint64)
    g = wc.tc._jac(wc.g_affine())
    for r, (_, m) in enumerate(wc.expected_records(plan, values)):
        if m:
            orc.lib().orc_point_mul(orc.ptr(g), orc.ptr(orc.fr_to_mont(m % wc.R)), orc.ptr(out[r]))
    return out


CHECKER_PLANS = [
    (dict(pipeline=0, form=0), [{0: 5, 3: -2}, {1: 7}, {}, {63: 1, 2: 9}]),
    (dict(pipeline=3, form=2, lg_rows=9, lg_cols=10), [{5: 3, (700 << 9) + 300: -4, (1023 << 9) + 511: 2, 513: 6}]),
    (dict(pipeline=2, form=2, lg_rows=8, lg_cols=8), [{5: 3, 65535: 2}, {77: -1, 300: 8}]),
]


@pytest.mark.parametrize("plan,values", CHECKER_PLANS)
def test_the_checkers_fail_when_they_should(plan, values):
    good = _records(plan, values)
    assert wc.check_window_sums(good, plan, values) == []
    distinct = [r for r in range(len(good)) if good[r].any()]
    a, b = distinct[0], distinct[-1]
    assert a != b and good[a].tolist() != good[b].tolist()
    swapped = good.copy()
    swapped[[a, b]] = swapped[[b, a]]
    assert {x[0] for x in wc.check_window_sums(swapped, plan, values)} == {a, b}
    lost = good.copy()
    lost[a] = 0
    assert [x[0] for x in wc.check_window_sums(lost, plan, values)] == [a]
    other = [dict(v) for v in values]
    bucket = next(iter(other[0]))
    other[0][bucket] += 1
    bad = wc.check_window_sums(good, plan, other)
    assert bad and "wrong records" in wc.describe(bad)
    assert wc.check_window_sums(good[:-1], plan, values)[0][0] == -1  # a record short


def _check_digits(launch):
    """the scalars' digits by the recode's rule: positive, in the planted buckets, the top window empty; and they give the values"""
    plan = launch.plan
    c, W = plan["c"], plan["W"]
    got = [dict() for _ in range(W)]
    for i, s in enumerate(launch.scalars):
        dg = wc.recode_digits(s, c)
        assert dg[W - 1] == (0, 0), "top window"
        for w, (mag, neg) in enumerate(dg):
            assert not neg and mag <= plan["B"]
            if mag:
                got[w][mag - 1] = got[w].get(mag - 1, 0) + launch.ks[i]
    assert [{b: x for b, x in g.items() if x} for g in got] == [dict(v) for v in launch.values]


def test_the_planted_scalars_give_the_digits_claimed():
    for key in wc.PLAN_SET[:-1]:
        plan, bg, cases = wc.build_cases(key[1], key[2], key[0])
        ks, launches = wc.pack_launches(plan, bg, cases)
        assert len(ks) <= (4096 if key[0] == 0 else 1 << 14) and len(ks) % 8 == 0
        for launch in launches:
            launch.ks = ks
            _check_digits(launch)
    for launch in (wc.combine_launch(), wc.horner_launch(7), wc.horner_launch(13), wc.partials_launch(), wc.heavy_launch(), wc.strided_launch(),
                   wc.reduce1_launch(0), wc.reduce1_launch(64)):
        _check_digits(launch)
    # the fixed windows of the table plan: one digit in window 0
    fixed = [l for _, l in wc.extra_host_launches("fixed")[1]] + [wc.slide_structure_launch("fixed")[1]]
    for launch in fixed:
        for s in launch.scalars:
            dg = wc.recode_digits(s, 20)
            assert dg[0] == (s, 0) and not any(m for m, _ in dg[1:])
    for members, (per, batches) in wc.small_key_batches().items():  # the small-key plan: one digit in window 0 of c = 17
        for launch in [l for batch in batches for l in batch]:
            for s in launch.scalars:
                dg = wc.recode_digits(s, 17)
                assert dg[0] == (s, 0) and s <= 1 << 16 and not any(m for m, _ in dg[1:])


def test_the_sliding_scalars_are_one_digit_on_row_zero(slide_host):
    """through the sliding recode compiled for the CPU (tests/native/slide_host.cpp): scalar 2 b + 1 is the digit 2 b + 1 on row 0"""
    scalars = set()
    ks, launches = wc.slide_rc_mid_launches()
    for launch in launches + [wc.slide_structure_launch()[1]] + [l for _, l in wc.slide_host_launches()[1] + wc.extra_host_launches()[1]]:
        scalars.update(s for s in launch.scalars if s)
    scalars = sorted(scalars | {1, (1 << 20) - 1})
    rec = recode(slide_host, scalars, "window_cases")
    for s, row in zip(scalars, rec):
        assert row[0] == 1 and (int(row[1]), int(row[2]), int(row[3])) == (s, 0, 0), s
