"""The key-fold kernels of pcdl::open -- k_fold_points (one and two outputs per lane), k_fold_points4 (one and two outputs per lane,
the first result parked in LDS), k_fold_points4_quad, k_fold_tab4 over the comb table (one and two outputs per lane) and
k_foldtab_build -- through halo_dev_fold_points: one fold over a chosen key, in a chosen kernel form, at a chosen m.  The cases are
those of tests/fold_cases.py (edge challenges, exceptional keys, odd m); the reference is the oracle's fold, compared exactly."""
import numpy as np
import pytest

import fold_cases as fc

pytestmark = pytest.mark.gpu

FORMS = {1: (0, 1, 2), 2: (0, 1, 2, 3)}
FORM_NAMES = ["the launcher's choice", "one output per lane", "two outputs per lane", "quad", "table, one per lane", "table, two per lane"]


@pytest.fixture(scope="module")
def hal():
    import halo_accumulation_amd as h
    return h


@pytest.fixture(scope="module")
def ctx(hal):
    c = hal._lib.Context(urs_n=64)
    yield c
    c.close()


@pytest.mark.parametrize("levels", [1, 2])
@pytest.mark.parametrize("m", fc.SIZES)
def test_every_generic_form_matches_the_oracle(ctx, levels, m):
    """Every case of this size through every kernel form the levels have (k_fold_points; k_fold_points4 in both lane forms and the
    quad kernel -- forced at sizes the product's thresholds of 2^16 .. 2^18 never give them), out of place and in place, and
    through the launcher's own choice: every output equals the oracle's.  Odd m puts the lane without a second output at the edge
    of a block (m = 257, 513: half = 129, 257) and clamps surplus quads (m = 3, 63, 65, ...)."""
    cs = fc.cases(levels, m)
    runs = 0
    for c in cs:
        for form in FORMS[levels]:
            for in_place in (False, True):
                got = ctx.fold_points(c.key, levels, c.scalars, form=form, in_place=in_place)
                fc.assert_same(got, c.want, "levels %d, m = %d, %s, %s, in place %d" % (levels, m, c.name, FORM_NAMES[form], in_place))
                runs += 1
    print("levels %d m = %d: %d cases x %d forms x 2 = %d folds; classes %s" % (levels, m, len(cs), len(FORMS[levels]), runs, fc.class_counts(cs)))
    print("   lanes (j, j + half) with results", {k: sum(c.mixed[k] for c in cs) for k in cs[0].mixed})


@pytest.mark.parametrize("n", fc.TABLE_SIZES)
def test_table_forms_match_the_oracle_and_the_generic_forms(hal, n):
    """A context made from an exceptional key of n points (k_foldtab_build over infinities, repeated, negated and scalar-related
    points): the table kernel with one and with two outputs per lane (m = 512: the product's own switch) over scalars whose comb
    digits hold +32 and -32, an empty lambda half, an empty plain half, zero members -- equal to the oracle and to every generic
    form on the same context.  The context's key is unchanged afterwards."""
    tc = fc.TableCase(n, hal.load())
    c = hal._lib.Context(bases=tc.key)
    try:
        assert np.array_equal(c.read_bases(), tc.key)
        for (name, _), scalars, want in zip(tc.triples, tc.scalars, tc.want):
            outs = {}
            for form in (4, 5, 0, 1, 2, 3):
                outs[form] = c.fold_points(None, 2, scalars, form=form)
                fc.assert_same(outs[form], want, "n = %d, %s, %s" % (n, name, FORM_NAMES[form]))
            for form in (0, 1, 2, 3):
                assert np.array_equal(outs[form], outs[4]) and np.array_equal(outs[form], outs[5]), (n, name, form)
            # the generic kernels in place and one level over the context's key work on a copy of it
            fc.assert_same(c.fold_points(None, 2, scalars, form=3, in_place=True), want, "n = %d, %s, in place" % (n, name))
        assert c.info(5) == 2  # (the table is there: built by the first table fold)
        assert np.array_equal(c.read_bases(), tc.key), "an out-of-place fold wrote to the key"
        print("n = %d: %d triples x 7 folds; classes %s" % (n, len(tc.triples), {k: tc.classes.count(k) for k in fc.L2_CLASSES}))
    finally:
        c.close()


def test_one_level_fold_of_the_contexts_own_key(ctx):
    """key_affine = NULL, levels 1: the first n points of the context's key, folded in a copy"""
    before = ctx.read_bases()
    scalars = np.stack([fc._mont(fc.RANDOM[0])])
    _, uj = fc.urs(64)
    want = fc.expected(np.ascontiguousarray(uj), 32, 1, ("xi", fc.RANDOM[0]))
    for form in (0, 1, 2):
        fc.assert_same(ctx.fold_points(None, 1, scalars, form=form), want, "own key, form %d" % form)
    want16 = fc.expected(np.ascontiguousarray(uj[:32]), 16, 1, ("xi", fc.RANDOM[0]))
    fc.assert_same(ctx.fold_points(None, 1, scalars, form=2, n=32), want16, "own key, first 32 points")
    assert np.array_equal(ctx.read_bases(), before)


def test_impossible_combinations_are_refused(hal, ctx):
    key, _ = fc.urs(64)
    s1, s3 = np.stack([fc._mont(5)]), np.stack([fc._mont(5)] * 3)
    bad = [
        (dict(key=key[:3], levels=1, scalars=s1), "odd n"),
        (dict(key=key[:6], levels=2, scalars=s3), "n not a multiple of 4"),
        (dict(key=None, levels=1, scalars=s1, n=0), "n = 0"),
        (dict(key=None, levels=1, scalars=s1, n=128), "more than the context's key"),
        (dict(key=key, levels=3, scalars=s1), "levels 3"),
        (dict(key=key, levels=0, scalars=s1), "levels 0"),
        (dict(key=key, levels=1, scalars=s1, form=3), "quad form with levels 1"),
        (dict(key=key, levels=1, scalars=s1, form=4), "table form with levels 1"),
        (dict(key=key, levels=2, scalars=s3, form=6), "form 6"),
        (dict(key=key, levels=2, scalars=s3, form=-1), "form -1"),
        (dict(key=key, levels=2, scalars=s3, form=4), "table form with a foreign key"),
        (dict(key=key, levels=2, scalars=s3, form=5), "table form with a foreign key"),
        (dict(key=None, levels=2, scalars=s3, form=4, n=32), "table form over a part of the key"),
        (dict(key=None, levels=2, scalars=s3, form=4, in_place=True), "table form in place"),
        (dict(key=None, levels=2, scalars=s3, form=5, in_place=True), "table form in place"),
    ]
    for kw, why in bad:
        k = dict(kw)
        key_, levels, scalars = k.pop("key"), k.pop("levels"), k.pop("scalars")
        out = np.zeros((64, 8), dtype=np.uint64)
        n = key_.shape[0] if key_ is not None else k.get("n", ctx.size)
        kp = None if key_ is None else hal._lib.ptr(np.ascontiguousarray(key_))
        rc = ctx.lib.halo_dev_fold_points(ctx.h, kp, n, levels, hal._lib.ptr(scalars), k.get("form", 0), int(k.get("in_place", False)), hal._lib.ptr(out))
        assert rc == -3 and ctx.lib.halo_last_error(), why  # HALO_E_ARG, with a message
        assert not out.any(), why
    # and the same context still folds
    fc.assert_same(ctx.fold_points(None, 2, s3, form=4), ctx.fold_points(None, 2, s3, form=3), "after the refusals")
