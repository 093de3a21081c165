"""Mirror of the reference's `acc` module (code/src/acc.rs): prover / verifier / decider."""
import ctypes as C

import numpy as np

from halo_accumulation_amd import _lib
from halo_accumulation_amd._lib import check, ptr
from halo_accumulation_amd.pcdl import _a, _check_batch, _check_batch_mixed, _pack_polys, _pack_rows, _seed32, lg_of


def _cat(qs):
    return np.ascontiguousarray(np.concatenate(qs)) if len(qs) else np.zeros(0, dtype=np.uint64)


def instance_from_accumulator(ctx, acc, d):
    """impl From<Accumulator> for Instance (acc.rs:121-131)"""
    return np.ascontiguousarray(acc[: ctx.lib.halo_instance_words(lg_of(d))]).copy()


def random_instance(ctx, rng, d):
    """benches/acc.rs:15-29"""
    st = C.c_uint64(rng[0])
    inst = np.zeros(ctx.lib.halo_instance_words(lg_of(d)), dtype=np.uint64)
    check(ctx.lib.halo_random_instance(ctx.h, C.byref(st), d, ptr(inst)))
    rng[0] = st.value
    return inst


def random_instance_batch(ctx, rng, d, m):
    """benches/acc.rs:15-29, m times in one call (halo_random_instance_batch) -> the m Instances random_instance returns in turn,
    rng[0] updated as it would update it"""
    st = C.c_uint64(rng[0])
    out = np.zeros((max(m, 1), ctx.lib.halo_instance_words(lg_of(d))), dtype=np.uint64)
    check(ctx.lib.halo_random_instance_batch(ctx.h, C.byref(st), d, m, ptr(out)))
    rng[0] = st.value
    return [out[i].copy() for i in range(m)]


def instance_from_poly(ctx, rng, p, d, z, w=None):
    """benches/acc.rs:15-29 for the caller's polynomial (halo_instance_from_poly): commit, evaluate at z, open, pack -> Instance"""
    p = _a(p).reshape(-1, 4)
    st = C.c_uint64(rng[0])
    inst = np.zeros(ctx.lib.halo_instance_words(max(lg_of(d), 0)), dtype=np.uint64)
    check(ctx.lib.halo_instance_from_poly(ctx.h, C.byref(st), ptr(p), p.shape[0], d, ptr(_a(z)), ptr(_a(w)), ptr(inst)))
    rng[0] = st.value
    return inst


def instance_from_poly_batch(ctx, rng, ps, d, zs, ws=None):
    """... of m polynomials of degree bound d at once (halo_instance_from_poly_batch) -> the Instances m instance_from_poly calls
    return in turn, rng[0] updated as they would update it.  A failing member raises as pcdl.open_batch does, with the status
    list as the exception's second argument."""
    m = len(ps)
    zs = _pack_rows(zs, m, 4, "instance_from_poly_batch", "zs")
    if zs is None:
        raise ValueError("instance_from_poly_batch: zs is required")
    ws = _pack_rows(ws, m, 4, "instance_from_poly_batch", "ws")
    coeffs = _pack_polys(ps, d, "commit")
    st = C.c_uint64(rng[0])
    out = np.zeros((max(m, 1), ctx.lib.halo_instance_words(max(lg_of(d), 0))), dtype=np.uint64)
    status = (C.c_int * max(m, 1))()
    rc = ctx.lib.halo_instance_from_poly_batch(ctx.h, C.byref(st), d, ptr(coeffs), m, ptr(zs), ptr(ws), ptr(out), status)
    if rc in (_lib.HALO_OK, _lib.HALO_E_ASSERT):
        rng[0] = st.value
    if rc == _lib.HALO_E_ASSERT:
        raise AssertionError(ctx.lib.halo_last_error().decode(), [status[i] for i in range(m)], [out[i].copy() for i in range(m)])
    check(rc)
    return [out[i].copy() for i in range(m)]


def instance_from_poly_dev(ctx, rng, dptr, length, d, z, w=None):
    """instance_from_poly for `length` coefficients resident in device memory, trailing zeros allowed (halo_instance_from_poly_dev)"""
    st = C.c_uint64(rng[0])
    inst = np.zeros(ctx.lib.halo_instance_words(max(lg_of(d), 0)), dtype=np.uint64)
    check(ctx.lib.halo_instance_from_poly_dev(ctx.h, C.byref(st), C.c_void_p(int(dptr or 0)), length, d, ptr(_a(z)), ptr(_a(w)), ptr(inst)))
    rng[0] = st.value
    return inst


def instance_from_poly_dev_batch(ctx, rng, dptrs, lens, d, zs, ws=None):
    """instance_from_poly_batch for m device-resident polynomials (halo_instance_from_poly_dev_batch): dptrs[i] = device address of
    lens[i] coefficients -> the Instances, rng[0] updated, as instance_from_poly_batch for the same rows; raises as it does"""
    m = len(dptrs)
    ptrs, ln = _lib.dev_rows(dptrs, lens, "instance_from_poly_dev_batch")
    zs = _pack_rows(zs, m, 4, "instance_from_poly_dev_batch", "zs")
    if zs is None:
        raise ValueError("instance_from_poly_dev_batch: zs is required")
    ws = _pack_rows(ws, m, 4, "instance_from_poly_dev_batch", "ws")
    st = C.c_uint64(rng[0])
    out = np.zeros((max(m, 1), ctx.lib.halo_instance_words(max(lg_of(d), 0))), dtype=np.uint64)
    status = (C.c_int * max(m, 1))()
    rc = ctx.lib.halo_instance_from_poly_dev_batch(ctx.h, C.byref(st), d, ptrs, ln, m, ptr(zs), ptr(ws), ptr(out), status)
    if rc in (_lib.HALO_OK, _lib.HALO_E_ASSERT):
        rng[0] = st.value
    if rc == _lib.HALO_E_ASSERT:
        raise AssertionError(ctx.lib.halo_last_error().decode(), [status[i] for i in range(m)], [out[i].copy() for i in range(m)])
    check(rc)
    return [out[i].copy() for i in range(m)]


def prover(ctx, rng, d, qs):
    """acc.rs:190-220"""
    st = C.c_uint64(rng[0])
    acc = np.zeros(ctx.lib.halo_accumulator_words(lg_of(d)), dtype=np.uint64)
    check(ctx.lib.halo_acc_prover(ctx.h, C.byref(st), d, ptr(_cat(qs)), len(qs), ptr(acc)))
    rng[0] = st.value
    return acc


def prover_batch(ctx, rng, d, qss):
    """acc::prover (acc.rs:190-220) of k members at once (halo_acc_prover_batch): qss[j] = member j's Instances (may be empty) ->
    (accs, status), the accumulators prover returns in turn (a failed member's is zero-filled), rng[0] updated as the loop would
    update it; raises HaloReject with the status list as verifier_batch does"""
    k = len(qss)
    counts = (C.c_size_t * max(k, 1))(*[len(qs) for qs in qss])
    qs = _cat([q for qs in qss for q in qs])
    st = C.c_uint64(rng[0])
    out = np.zeros((max(k, 1), ctx.lib.halo_accumulator_words(lg_of(d))), dtype=np.uint64)
    status = (C.c_int * max(k, 1))()
    rc = ctx.lib.halo_acc_prover_batch(ctx.h, C.byref(st), d, ptr(qs), counts, k, ptr(out), status)
    codes = [status[i] for i in range(k)]
    if rc == _lib.HALO_E_REJECT:
        rng[0] = st.value
        raise _lib.HaloReject(ctx.lib.halo_last_error().decode(), codes)
    check(rc)
    rng[0] = st.value
    return [out[i].copy() for i in range(k)], codes


def verifier(ctx, d, qs, acc):
    """acc.rs:223-243"""
    check(ctx.lib.halo_acc_verifier(ctx.h, d, ptr(_cat(qs)), len(qs), ptr(np.ascontiguousarray(acc, dtype=np.uint64))))


def verifier_batch(ctx, d, qss, accs):
    """acc::verifier (acc.rs:223-243) of k accumulators at once (benches/acc.rs:64-74's loop in one call): qss[j] = the Instances
    accs[j] is verified against (may be empty) -> status list; raises HaloReject as decider_batch does"""
    k = len(accs)
    if len(qss) != k:
        raise ValueError("verifier_batch: one list of instances per accumulator")
    counts = (C.c_size_t * max(k, 1))(*[len(qs) for qs in qss])
    qs = _cat([q for qs in qss for q in qs])
    blob = _cat(accs) if k else np.zeros(0, dtype=np.uint64)
    status = (C.c_int * max(k, 1))()
    rc = ctx.lib.halo_acc_verifier_batch(ctx.h, d, ptr(qs), counts, k, ptr(blob), status)
    st = [status[i] for i in range(k)]
    if rc == _lib.HALO_E_REJECT:
        raise _lib.HaloReject(ctx.lib.halo_last_error().decode(), st)
    check(rc)
    return st


def decider(ctx, acc):
    """acc.rs:245-255"""
    check(ctx.lib.halo_acc_decider(ctx.h, ptr(np.ascontiguousarray(acc, dtype=np.uint64))))


def decider_batch(ctx, d, accs):
    """acc::decider (acc.rs:245-255) of m accumulators of degree bound d at once (benches/acc.rs:100-106 in one call) -> status
    list; raises HaloReject as pcdl.check_batch does"""
    return _check_batch(ctx, ctx.lib.halo_acc_decider_batch, d, accs)


def decider_batch_combined(ctx, d, accs, seed=None):
    """decider_batch with ONE MSM for all accepted members (halo_acc_decider_batch_combined; seed: 32 bytes or None) -> status
    list; statuses and HaloReject as decider_batch whenever a member is bad"""
    return _check_batch(ctx, lambda h, dd, qs, m, st: ctx.lib.halo_acc_decider_batch_combined(h, dd, qs, m, _seed32(seed), st), d, accs)


def decider_batch_fused(ctx, d, accs, seed=None):
    """decider_batch as ONE relation, the succinct relations included (halo_acc_decider_batch_fused; seed: 32 bytes or None) ->
    status list; statuses and HaloReject as decider_batch whenever a member is bad"""
    return _check_batch(ctx, lambda h, dd, qs, m, st: ctx.lib.halo_acc_decider_batch_fused(h, dd, qs, m, _seed32(seed), st), d, accs)


def decider_batch_mixed(ctx, accs):
    """acc::decider of m accumulators, each of its own degree bound (read from the blob's word 12), in one call
    (halo_acc_decider_batch_mixed) -> status list; raises HaloReject as pcdl.check_batch does"""
    return _check_batch_mixed(ctx, ctx.lib.halo_acc_decider_batch_mixed, accs)


def decider_batch_mixed_combined(ctx, accs, seed=None):
    """decider_batch_mixed with ONE MSM for the accepted members of every size (halo_acc_decider_batch_mixed_combined; seed: 32 bytes
    or None) -> status list; statuses and HaloReject as decider_batch_mixed whenever a member is bad"""
    return _check_batch_mixed(ctx, lambda h, ds, ps, m, st: ctx.lib.halo_acc_decider_batch_mixed_combined(h, ds, ps, m, _seed32(seed), st), accs)


def decider_batch_mixed_fused(ctx, accs, seed=None):
    """decider_batch_mixed as ONE relation over the members of every size, the succinct relations included
    (halo_acc_decider_batch_mixed_fused; seed: 32 bytes or None) -> status list; statuses and HaloReject as decider_batch_mixed
    whenever a member is bad"""
    return _check_batch_mixed(ctx, lambda h, ds, ps, m, st: ctx.lib.halo_acc_decider_batch_mixed_fused(h, ds, ps, m, _seed32(seed), st), accs)
