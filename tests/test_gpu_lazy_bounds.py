"""The lazy radix-2^29 fields and the group law on them AT their value bounds, as the device compiler emits them.

The parity tests reach the device arithmetic through the C ABI, which converts canonical words: every operand is then below
2p and a Y is never stored as 8p - y, while the bucket kernels carry X, Y < 8p from one addition to the next and run products at
116/120 of the Montgomery bound.  Here the operands are raw limbs (halo_test_lazy_field_op / halo_test_lazy_point_op,
csrc/dev_lazy_ops.hpp), built by tests/lazy_cases.py: the same cases the CPU build of the same headers passes under ASan + UBSan
(tests/test_host_sanitizers.py).  Each result must satisfy the big-integer contract AND equal the host build's result limb for
limb: the algorithm is deterministic, so a difference is a code-generation fault in the pinned v_mad_u64_u32 chains.

Last, the Fr kernels (dot, powers, p(z), h(X), folds, axpy, the accumulate batch) on the data that drives their lazy sums to the
largest values: vectors of r - 1, zeros, ones, 2^254, scalars 0, 1, r - 1, 2 -- exact against the C oracle, which
tests/test_oracle_extremes.py holds against Python integers on these very vectors."""
import ctypes as C
import random

import numpy as np
import pytest

import lazy_cases as lz
import orc
import pallas_model as pm
import test_gpu_pcdl_acc as _acc

pytestmark = pytest.mark.gpu
R = pm.R_ORDER
# Every IPA strategy, as tests/test_gpu_pcdl_acc.py defines them.  The fixture asks for `ctx` by name, and pytest resolves that
# name where the fixture is USED: it sets the modes on THIS module's context (the `ctx` fixture below), not on that module's.
ipa_mode = _acc.ipa_mode


@pytest.fixture(scope="module")
def hal():
    import halo_accumulation_amd as h
    return h


@pytest.fixture(scope="module")
def ctx(hal):
    c = hal._lib.Context(urs_n=4096)
    yield c
    c.close()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """the CPU build of the same headers, or None where it cannot be built (then the contract alone decides)"""
    d = tmp_path_factory.mktemp("lazy_host")
    exe, why = lz.build_host(d)
    if exe is None:
        print("host build unavailable (%s): only the big-integer contract is checked" % why)
        return None
    return lz.HostRunner(exe, d)


def _same_limbs(name, got, want):
    if not np.array_equal(got, want):
        bad = np.nonzero((got != want).any(axis=1))[0]
        raise AssertionError("%s: device and host limbs differ in %d of %d cases, first case %d\n device %s\n host   %s"
                             % (name, len(bad), len(got), bad[0], got[bad[0]].tolist(), want[bad[0]].tolist()))


# ------------------------------------------------------------------ 1. field layer
def test_lazy_fields_at_their_value_bounds(ctx, host):
    rng = random.Random(0x4C415A59)  # (the seed of the host test: the same cases)
    rows = [(row, lz.field_cases(row, rng)) for row in lz.FIELD_TABLE]
    blocks = [(0, row[0], lz.encode_field(row, cases), None) for row, cases in rows]
    dev = lz.DeviceRunner(ctx).run(blocks)
    ref = host.run(blocks) if host else None
    total = 0
    for k, (row, cases) in enumerate(rows):
        lz.check_field(row, cases, dev[k], "device")
        if ref:
            _same_limbs(row[1], dev[k], ref[k])
        print("%-28s %6d cases" % (row[1], len(cases)))
        total += len(cases)
    print("lazy field layer on the device: %d cases over %d instantiations; %s"
          % (total, len(rows), "raw limbs equal to the host build's" if ref else "contract only: no host build on this machine"))


# ------------------------------------------------------------------ 2. group law
def test_group_law_over_non_canonical_representatives(ctx, host, kat):
    pc = lz.PointCases(kat)
    ops = list(range(16))
    blocks = pc.blocks(ops)
    dev = lz.DeviceRunner(ctx).run(blocks)
    ref = host.run(blocks) if host else None
    for k, op in enumerate(ops):
        counts = pc.check(op, dev[k], "device")
        if ref:
            _same_limbs(lz.POINT_OP_NAMES[op], dev[k], ref[k])
        print("%-28s %6d cases  %s" % (lz.POINT_OP_NAMES[op], len(pc.cases[op]), counts))
    assert lz.madd_p_multiples(pc.cases[lz.XYZZ_MADD]) == set(range(1, 10))
    print("group law on the device: %s" % ("raw limbs equal to the host build's" if ref else "contract only: no host build on this machine"))


def _wave_with(cases, kinds):
    """index of a wave (16 neighbouring quads) that holds every one of `kinds`"""
    for w in range(len(cases) // 16):
        here = {c[4] for c in cases[16 * w: 16 * w + 16]}
        if all(any(h.startswith(k) for h in here) for k in kinds):
            return w
    return None


def test_quad_forms_over_non_canonical_representatives(ctx, kat):
    """curve_quad.hpp over the same matrix, one case per 4 lanes: general additions, the doubling branch, P + (-P) and
    infinities sit in neighbouring quads of one wave (the doubling inside an addition is taken by the whole wave when any quad
    needs it), and every lane's operands carry a non-trivial representative."""
    pc = lz.PointCases(kat)
    assert _wave_with(pc.cases[lz.XYZZ_ADD], ("generic", "double", "inverse", "inf")) is not None
    assert _wave_with(pc.cases[lz.JAC_MADD], ("generic", "double", "inverse", "inf")) is not None
    assert _wave_with(pc.cases[lz.XYZZ_DBL], ("double", "inf")) is not None and _wave_with(pc.cases[lz.JAC_DBL], ("double", "inf")) is not None
    outs = lz.DeviceRunner(ctx, quad=True).run(pc.blocks(lz.QUAD_OPS))
    for op, out in zip(lz.QUAD_OPS, outs):
        counts = pc.check(op, out, "device quad")
        print("%-28s %6d cases  %s" % (lz.POINT_OP_NAMES[op] + "_quad", len(pc.cases[op]), counts))


@pytest.mark.parametrize("op,quad", [(lz.XYZZ_MADD, False), (lz.XYZZ_ADD, False), (lz.XYZZ_ADD, True)], ids=["xyzz_madd", "xyzz_add", "xyzz_add_quad"])
def test_chains_of_additions_without_normalising_stay_in_bounds(ctx, kat, op, quad):
    got = lz.run_chains(lz.DeviceRunner(ctx, quad=quad), kat, op)
    print(lz.POINT_OP_NAMES[op], "quad" if quad else "", got)
    assert got["steps"] >= 64


def test_lazy_hooks_refuse_what_they_do_not_know(hal, ctx):
    a = np.zeros((1, 40), dtype=np.uint32)
    for bad in (-1, 36, 39, 55):
        with pytest.raises(hal._lib.HaloError):
            ctx.lazy_field_op(bad, a)
    with pytest.raises(hal._lib.HaloError):
        ctx.lazy_point_op(16, a, a)
    with pytest.raises(hal._lib.HaloError):
        ctx.lazy_point_op(lz.JAC_TO_AFF, a, a, quad=True)


# ------------------------------------------------------------------ 3. Fr kernels at extreme data
@pytest.mark.parametrize("m", lz.FR_LENGTHS)
def test_scalar_dot_powers_poly_eval_at_extremes(ctx, m):
    vecs = {k: lz.fr_mont(v) for k, v in lz.fr_extreme_vectors(m).items()}
    for ka, a in vecs.items():
        for kb, b in vecs.items():
            assert ctx.scalar_dot(a, b).tolist() == orc.scalar_dot(a, b).tolist(), (ka, kb)
    for z in lz.FR_SCALARS:
        zw = lz.fr_mont([z])[0]
        assert ctx.powers(zw, m).tolist() == orc.powers(zw, m).tolist(), z
        for k, a in vecs.items():
            assert ctx.poly_eval(a, zw).tolist() == orc.poly_eval(a, zw).tolist(), (k, z)


@pytest.mark.parametrize("lg_n", [1, 2, 3, 6, 7, 8, 9, 12])
def test_h_coeffs_and_h_eval_at_extremes(hal, ctx, lg_n):
    vecs = {k: lz.fr_mont(v) for k, v in lz.fr_extreme_vectors(lg_n + 1).items()}
    want = {k: orc.h_coeffs(x) for k, x in vecs.items()}
    for k, x in vecs.items():
        assert ctx.h_coeffs(x).tolist() == want[k].tolist(), k
    stack = np.ascontiguousarray(np.stack(list(vecs.values())))
    for z in lz.FR_SCALARS:
        zw = lz.fr_mont([z])[0]
        got = ctx.h_eval_batch(stack, zw)
        for i, (k, x) in enumerate(vecs.items()):
            assert got[i].tolist() == orc.h_eval(x, zw).tolist(), (k, z)
    out = np.zeros((len(vecs), 1 << lg_n, 4), dtype=np.uint64)
    assert ctx.lib.halo_dev_h_coeffs_batch(ctx.h, hal._lib.ptr(stack), len(vecs), lg_n, hal._lib.ptr(out)) == 0, ctx.lib.halo_last_error()
    for i, k in enumerate(vecs):
        assert out[i].tolist() == want[k].tolist(), k


@pytest.mark.parametrize("lg_n", [1, 6, 10])
def test_h_accumulate_at_extremes(hal, ctx, lg_n):
    """acc.rs:85-94, h0 + sum alpha_i h_i, single and batched (also with fewer tables per pass than a member has instances):
    every h_i and every alpha at an extreme, so each coefficient's running sum takes its largest values"""
    n = 1 << lg_n
    xi_ints = list(lz.fr_extreme_vectors(lg_n + 1).values())
    xis = np.ascontiguousarray(np.stack([lz.fr_mont(v) for v in xi_ints]))
    hs = [lz.fr_ints(orc.h_coeffs(np.ascontiguousarray(x))) for x in xis]
    alpha_ints = [R - 1, 0, 1, 2, R - 1, (R - 1) // 2, (1 << 254) % R]
    assert len(alpha_ints) == len(hs) == 7

    def expect(h0, members):
        acc = [0] * n
        acc[0], acc[1] = h0
        for i in members:
            acc = [(a + alpha_ints[i] * h) % R for a, h in zip(acc, hs[i])]
        return acc

    for h0 in ((R - 1, R - 1), (0, 0)):
        got = ctx.h_accumulate(lz.fr_mont(h0), xis, lz.fr_mont(alpha_ints))
        assert lz.fr_ints(got) == expect(h0, range(7)), h0
    # the batch: members of 7, 1 and 3 instances (the all-(r-1) instance first in each)
    members = [list(range(7)), [0], [0, 4, 6]]
    h0s = [(R - 1, R - 1), (1, R - 1), (0, 0)]
    flat = [i for mem in members for i in mem]
    bx = np.ascontiguousarray(np.concatenate([xis[i] for i in flat]))
    ba = lz.fr_mont([alpha_ints[i] for i in flat])
    bh = lz.fr_mont([v for h0 in h0s for v in h0])
    counts = (C.c_size_t * len(members))(*[len(mem) for mem in members])
    for max_tables in (0, 2, 3, 7):
        out = np.full((len(members), n, 4), 0x77, dtype=np.uint64)
        rc = ctx.lib.halo_dev_h_accumulate_batch(ctx.h, hal._lib.ptr(bh), hal._lib.ptr(bx), hal._lib.ptr(ba), counts, len(members), lg_n, max_tables,
                                                 hal._lib.ptr(out))
        assert rc == 0, ctx.lib.halo_last_error()
        for j, mem in enumerate(members):
            assert lz.fr_ints(out[j]) == expect(h0s[j], mem), "member %d, %d tables per pass" % (j, max_tables)


@pytest.mark.parametrize("n", [2, 8, 64, 128, 1024])
def test_fold_of_c_and_z_at_extremes(hal, ctx, n, ipa_mode):
    """pcdl.rs:221-227 under every IPA strategy: c' = c_l + xi^-1 c_r, z' = z_l + xi z_r.  Each of xi = 1, r - 1, 2 meets the
    UNTOUCHED extreme vector in the first round, once as c and once as z; the other vector is random, so it never collapses,
    and after every round <c, z> of the folded state (halo_ipa_dot_cz) must equal the oracle's: one wrong element of either
    vector moves that sum.  Later rounds use random xi.  The two vectors with different halves stay non-zero through every
    round (a constant vector folds to zero under xi = r - 1: the right answer, but nothing for later rounds to work on); the
    last c and z are compared directly."""
    vecs = lz.fr_fold_vectors(n)
    rng = random.Random(0x464F4C44 + n)
    for name, v in vecs.items():
        for role in ("c", "z"):
            for first in (1, R - 1, 2):
                other = [rng.randrange(1, R) for _ in range(n)]
                cs, zs = (lz.fr_mont(v), lz.fr_mont(other)) if role == "c" else (lz.fr_mont(other), lz.fr_mont(v))
                tag = (name, role, first)
                ipa = hal._lib.Ipa(ctx, n, cs, None, z_vec=zs)
                assert ipa.dot_cz().tolist() == orc.scalar_dot(cs, zs).tolist(), tag
                gj = np.zeros((n, 12), dtype=np.uint64)  # (the oracle folds points too: all at infinity)
                m, xi = n // 2, first
                while m >= 1:
                    xw, xiw = lz.fr_mont([xi])[0], lz.fr_mont([pm.inv_mod(xi, R)])[0]
                    ipa.round_fold(xw, xiw)
                    orc.lib().orc_ipa_round_fold(orc.ptr(gj), orc.ptr(cs), orc.ptr(zs), orc.C.c_size_t(m), orc.ptr(xw), orc.ptr(xiw))
                    assert ipa.dot_cz().tolist() == orc.scalar_dot(np.ascontiguousarray(cs[:m]), np.ascontiguousarray(zs[:m])).tolist(), (tag, m)
                    if name in lz.SPLIT_VECTORS:
                        assert (cs[:m] if role == "c" else zs[:m]).any(), (tag, m)
                    assert (zs[:m] if role == "c" else cs[:m]).any(), (tag, m)
                    m //= 2
                    xi = rng.randrange(2, R - 1)
                _U, c0, z0 = ipa.finish_z()
                ipa.close()
                assert c0.tolist() == cs[0].tolist() and z0.tolist() == zs[0].tolist(), tag


@pytest.mark.parametrize("n", [64, 1024])
def test_axpy_at_extremes(hal, ctx, n):
    """k_axpy as the library exposes it: p' = p + alpha p_bar of the hiding open (pcdl.rs:156), p at an extreme, alpha = 0, 1,
    r - 1, 2, p_bar = q (X - z') from the seeded stream.  Read back through <p', (1, z, z^2, ..)> -- any wrong element moves
    the sum -- and compared with the same sum over Python integers; the share of C_bar against the oracle's MSM."""
    seed, deg = 0x41585059 + n, n - 1
    qw, _ = orc.rng_scalars(seed, deg)
    q = lz.fr_ints(qw)
    z, zq = random.Random(n).randrange(2, R), random.Random(n + 1).randrange(2, R)
    pbar = [(-zq * q[0]) % R] + [(q[i - 1] - zq * q[i]) % R for i in range(1, deg)] + [q[deg - 1]]
    assert len(pbar) == n and pm.poly_eval(pbar, zq) == 0
    zw, zqw = lz.fr_mont([z])[0], lz.fr_mont([zq])[0]
    zs = pm.construct_powers(z, n)
    gs = ctx.read_bases(0, n)
    for k, p in lz.fr_extreme_vectors(n).items():
        for alpha in lz.FR_SCALARS:
            ipa = hal._lib.Ipa(ctx, n, lz.fr_mont(p), zw)
            part = ipa.hiding_partial(seed, deg, zqw, 1, 0)
            ipa.apply_hiding(lz.fr_mont([alpha])[0])
            got = ipa.dot_cz()
            ipa.close()
            assert lz.fr_ints(got) == [pm.scalar_dot([(a + alpha * b) % R for a, b in zip(p, pbar)], zs)], (k, alpha)
        assert orc.point_canonical(part) == orc.point_canonical(orc.msm_affine(gs, lz.fr_mont(pbar))), k
