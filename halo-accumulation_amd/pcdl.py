"""Mirror of the reference's `pcdl` module (code/src/pcdl.rs): commit / open / succinct_check / check.

Polynomials are coefficient arrays (len, 4); proofs are the flat EvalProof blobs described in
include/halo_accumulation.h.  `rng` is a one-element list holding a SplitMix64 state (mutated),
standing in for the reference's `rng: &mut R`.
"""
import ctypes as C

import numpy as np

from halo_accumulation_amd import _lib
from halo_accumulation_amd._lib import check, ptr


def _a(x):
    return None if x is None else np.ascontiguousarray(x, dtype=np.uint64)


def lg_of(d):
    return (d + 1).bit_length() - 1


def commit(ctx, p, d, w=None):
    """pcdl.rs:99-110"""
    p = _a(p).reshape(-1, 4)
    out = np.zeros(12, dtype=np.uint64)
    check(ctx.lib.halo_pcdl_commit(ctx.h, ptr(p), p.shape[0], d, ptr(_a(w)), ptr(out)))
    return out


def open(ctx, rng, p, Cm, d, z, w=None):
    """pcdl.rs:120-242 -> EvalProof blob"""
    p = _a(p).reshape(-1, 4)
    st = C.c_uint64(rng[0])
    proof = np.zeros(ctx.lib.halo_proof_words(max(lg_of(d), 0)), dtype=np.uint64)
    check(ctx.lib.halo_pcdl_open(ctx.h, C.byref(st), ptr(p), p.shape[0], ptr(_a(Cm)), d, ptr(_a(z)), ptr(_a(w)), ptr(proof)))
    rng[0] = st.value
    return proof


def open_batch(ctx, rng, ps, Cs, d, zs, ws=None):
    """pcdl::open of m polynomials of degree bound d at once (halo_pcdl_open_batch) -> list of EvalProof blobs: what m pcdl.open
    calls in member order return, rng[0] updated as they would update it.  A failing member raises as pcdl.open does, with the
    status list (what halo_pcdl_open returns for each member alone) as the exception's second argument."""
    m, lg = len(ps), max(lg_of(d), 0)
    coeffs = np.zeros((max(m, 1), d + 1, 4), dtype=np.uint64)
    for i, p in enumerate(ps):
        p = _a(p).reshape(-1, 4)
        nz = np.nonzero(p.any(axis=1))[0]
        k = int(nz[-1]) + 1 if len(nz) else 1
        if k > d + 1:
            raise AssertionError("open: p.degree() > d")
        coeffs[i, :k] = p[:k]
    st = C.c_uint64(rng[0])
    out = np.zeros((max(m, 1), ctx.lib.halo_proof_words(lg)), dtype=np.uint64)
    status = (C.c_int * max(m, 1))()
    rc = ctx.lib.halo_pcdl_open_batch(ctx.h, C.byref(st), d, ptr(coeffs), m, ptr(_a(Cs)), ptr(_a(zs)), ptr(_a(ws)), ptr(out), status)
    if rc in (_lib.HALO_OK, _lib.HALO_E_ASSERT):
        rng[0] = st.value
    if rc == _lib.HALO_E_ASSERT:
        raise AssertionError(ctx.lib.halo_last_error().decode(), [status[i] for i in range(m)])
    check(rc)
    return [out[i].copy() for i in range(m)]


def _pack_polys(ps, d, who):
    """m coefficient arrays -> (max(m, 1), d + 1, 4), zero-padded (the layout of halo_pcdl_open_batch)"""
    coeffs = np.zeros((max(len(ps), 1), d + 1, 4), dtype=np.uint64)
    for i, p in enumerate(ps):
        p = _a(p).reshape(-1, 4)
        nz = np.nonzero(p.any(axis=1))[0]
        k = int(nz[-1]) + 1 if len(nz) else 0
        if k > d + 1:
            raise AssertionError(who + ": p.degree() > d")
        coeffs[i, :k] = p[:k]
    return coeffs


def _pack_rows(rows, m, width, who, what):
    """m rows of `width` words (None stays None); a list of another length is the caller's mistake, found before the library runs"""
    if rows is None:
        return None
    if len(rows) != m:
        raise ValueError("%s: %d %s for %d polynomials" % (who, len(rows), what, m))
    out = np.zeros((max(m, 1), width), dtype=np.uint64)
    for i, r in enumerate(rows):
        out[i] = _a(r).reshape(width)
    return out


def commit_batch(ctx, ps, d, ws=None):
    """pcdl::commit of m polynomials of degree bound d at once (halo_pcdl_commit_batch) -> (m, 12): the points m pcdl.commit
    calls return.  ws: one w per polynomial, or None (no member hides)."""
    m = len(ps)
    ws = _pack_rows(ws, m, 4, "commit_batch", "ws")
    coeffs = _pack_polys(ps, d, "commit")
    out = np.zeros((max(m, 1), 12), dtype=np.uint64)
    check(ctx.lib.halo_pcdl_commit_batch(ctx.h, d, ptr(coeffs), m, ptr(ws), ptr(out)))
    return out[:m].copy()


def commit_dev_batch(ctx, dptrs, lens, d, ws=None):
    """pcdl::commit of m device-resident polynomials at once (halo_pcdl_commit_dev_batch): dptrs[i] = device address of lens[i]
    coefficients -> (m, 12).  A member longer than d + 1 raises as pcdl.commit_dev does, with the status list as the
    exception's second argument and the points (that member's zero-filled) as its third."""
    m = len(dptrs)
    if len(lens) != m:
        raise ValueError("commit_dev_batch: %d lengths for %d pointers" % (len(lens), m))
    ws = _pack_rows(ws, m, 4, "commit_dev_batch", "ws")
    ptrs = (C.c_void_p * max(m, 1))(*[C.c_void_p(int(p)) for p in dptrs])
    ln = (C.c_size_t * max(m, 1))(*[int(k) for k in lens])
    out = np.zeros((max(m, 1), 12), dtype=np.uint64)
    status = (C.c_int * max(m, 1))()
    rc = ctx.lib.halo_pcdl_commit_dev_batch(ctx.h, d, ptrs, ln, m, ptr(ws), ptr(out), status)
    if rc == _lib.HALO_E_ASSERT:
        raise AssertionError(ctx.lib.halo_last_error().decode(), [status[i] for i in range(m)], out[:m].copy())
    check(rc)
    return out[:m].copy()


def commit_dev(ctx, dptr, length, d, w=None):
    """pcdl::commit for `length` coefficients resident in device memory"""
    out = np.zeros(12, dtype=np.uint64)
    check(ctx.lib.halo_pcdl_commit_dev(ctx.h, C.c_void_p(dptr), length, d, ptr(_a(w)), ptr(out)))
    return out


def open_dev(ctx, rng, dptr, length, Cm, d, z, w=None):
    """pcdl::open for a polynomial resident in device memory (length = degree + 1) -> EvalProof blob"""
    st = C.c_uint64(rng[0])
    proof = np.zeros(ctx.lib.halo_proof_words(max(lg_of(d), 0)), dtype=np.uint64)
    check(ctx.lib.halo_pcdl_open_dev(ctx.h, C.byref(st), C.c_void_p(dptr), length, ptr(_a(Cm)), d, ptr(_a(z)), ptr(_a(w)), ptr(proof)))
    rng[0] = st.value
    return proof


def poly_degrees_dev(ctx, dptrs, lens):
    """DensePolynomial::degree of m device-resident rows, found on the device (halo_poly_degrees_dev) -> list of m ints"""
    return ctx.poly_degrees_dev(dptrs, lens)


def poly_eval_dev(ctx, dptr, length, z):
    """p(z) for `length` coefficients resident in device memory (halo_poly_eval_dev)"""
    return ctx.poly_eval_dev(dptr, length, z)


def open_dev_batch(ctx, rng, dptrs, lens, Cs, d, zs, ws=None):
    """pcdl::open of m device-resident polynomials at once (halo_pcdl_open_dev_batch): dptrs[i] = device address of lens[i]
    coefficients, trailing zeros allowed -> list of EvalProof blobs, rng[0] updated, as open_batch for the same rows.  A failing
    member (a constant that hides, more than d + 1 coefficients) raises as open_batch does, with the status list as the
    exception's second argument and the blobs (that member's zero-filled) as its third."""
    m, lg = len(dptrs), max(lg_of(d), 0)
    ptrs, ln = _lib.dev_rows(dptrs, lens, "open_dev_batch")
    Cs = _pack_rows(Cs, m, 12, "open_dev_batch", "Cs")
    zs = _pack_rows(zs, m, 4, "open_dev_batch", "zs")
    if Cs is None or zs is None:
        raise ValueError("open_dev_batch: Cs and zs are required")
    ws = _pack_rows(ws, m, 4, "open_dev_batch", "ws")
    st = C.c_uint64(rng[0])
    out = np.zeros((max(m, 1), ctx.lib.halo_proof_words(lg)), dtype=np.uint64)
    status = (C.c_int * max(m, 1))()
    rc = ctx.lib.halo_pcdl_open_dev_batch(ctx.h, C.byref(st), d, ptrs, ln, m, ptr(Cs), ptr(zs), ptr(ws), ptr(out), status)
    if rc in (_lib.HALO_OK, _lib.HALO_E_ASSERT):
        rng[0] = st.value
    if rc == _lib.HALO_E_ASSERT:
        raise AssertionError(ctx.lib.halo_last_error().decode(), [status[i] for i in range(m)], [out[i].copy() for i in range(m)])
    check(rc)
    return [out[i].copy() for i in range(m)]


def succinct_check(ctx, Cm, d, z, v, pi):
    """pcdl.rs:252-314 -> (xis of h, U); raises HaloReject where the reference returns Err"""
    lg = max(lg_of(d), 0)
    xis = np.zeros((lg + 1, 4), dtype=np.uint64)
    U = np.zeros(12, dtype=np.uint64)
    check(ctx.lib.halo_pcdl_succinct_check(ctx.h, ptr(_a(Cm)), d, ptr(_a(z)), ptr(_a(v)), ptr(_a(pi)), ptr(xis), ptr(U)))
    return xis, U


def succinct_check_batch(ctx, d, instances):
    """m succinct checks at once -> (xis (m, lg+1, 4), Us (m, 12), status (m,)); raises HaloReject if any instance fails
    (status then still tells which: use return_status=True semantics through the status array of the exception args)"""
    qs = np.ascontiguousarray(np.concatenate(instances)) if len(instances) else np.zeros(0, dtype=np.uint64)
    m, lg = len(instances), max(lg_of(d), 0)
    xis = np.zeros((m, lg + 1, 4), dtype=np.uint64)
    Us = np.zeros((m, 12), dtype=np.uint64)
    status = (C.c_int * max(m, 1))()
    rc = ctx.lib.halo_pcdl_succinct_check_batch(ctx.h, d, ptr(qs), m, ptr(xis), ptr(Us), status)
    st = [status[i] for i in range(m)]
    if rc == _lib.HALO_E_REJECT:
        raise _lib.HaloReject(ctx.lib.halo_last_error().decode(), st)
    check(rc)
    return xis, Us, st


def check_proof(ctx, Cm, d, z, v, pi):
    """pcdl::check (pcdl.rs:323-342)"""
    check(ctx.lib.halo_pcdl_check(ctx.h, ptr(_a(Cm)), d, ptr(_a(z)), ptr(_a(v)), ptr(_a(pi))))


def _check_batch(ctx, fn, d, blobs):
    qs = np.ascontiguousarray(np.concatenate(blobs), dtype=np.uint64) if len(blobs) else np.zeros(0, dtype=np.uint64)
    m = len(blobs)
    status = (C.c_int * max(m, 1))()
    rc = fn(ctx.h, d, ptr(qs), m, status)
    st = [status[i] for i in range(m)]
    if rc == _lib.HALO_E_REJECT:
        raise _lib.HaloReject(ctx.lib.halo_last_error().decode(), st)
    check(rc)
    return st


def check_batch(ctx, d, instances):
    """pcdl::check (pcdl.rs:323-342) of m instances of degree bound d at once -> status list (all 0); raises HaloReject if any
    instance fails, with the status list (what halo_pcdl_check returns for each alone) as its second argument"""
    return _check_batch(ctx, ctx.lib.halo_pcdl_check_batch, d, instances)


def _seed32(seed):
    if seed is None:
        return None
    seed = bytes(seed)
    if len(seed) != 32:
        raise ValueError("seed: 32 bytes or None")
    return seed


def check_batch_combined(ctx, d, instances, seed=None):
    """check_batch with ONE MSM for all accepted members (halo_pcdl_check_batch_combined: <sum r_i h_i, G> = sum r_i U_i with
    hashed weights; seed: 32 bytes of the caller's randomness or None) -> status list; statuses and HaloReject as check_batch
    whenever a member is bad"""
    return _check_batch(ctx, lambda h, dd, qs, m, st: ctx.lib.halo_pcdl_check_batch_combined(h, dd, qs, m, _seed32(seed), st), d, instances)


def check_batch_fused(ctx, d, instances, seed=None):
    """check_batch as ONE relation, the succinct relations included (halo_pcdl_check_batch_fused: one MSM over the members' own points
    beside the one over the key, two hashed weights per member; seed: 32 bytes of the caller's randomness or None) -> status list;
    statuses and HaloReject as check_batch whenever a member is bad"""
    return _check_batch(ctx, lambda h, dd, qs, m, st: ctx.lib.halo_pcdl_check_batch_fused(h, dd, qs, m, _seed32(seed), st), d, instances)


def _pack_mixed(blobs):
    """-> (the blobs as contiguous uint64 arrays -- keep them alive over the call --, ds from each blob's word 12, the pointer array)"""
    keep = [np.ascontiguousarray(b, dtype=np.uint64).reshape(-1) for b in blobs]
    for b in keep:
        if b.size < 23:
            raise ValueError("a blob is shorter than an Instance's head")
    m = len(keep)
    ds = (C.c_size_t * max(m, 1))(*[int(b[12]) for b in keep])
    ptrs = (C.c_void_p * max(m, 1))(*[b.ctypes.data for b in keep])
    return keep, ds, ptrs


def _check_batch_mixed(ctx, fn, blobs):
    keep, ds, ptrs = _pack_mixed(blobs)
    m = len(keep)
    status = (C.c_int * max(m, 1))()
    rc = fn(ctx.h, ds, ptrs, m, status)
    st = [status[i] for i in range(m)]
    if rc == _lib.HALO_E_REJECT:
        raise _lib.HaloReject(ctx.lib.halo_last_error().decode(), st)
    check(rc)
    return st


def check_batch_mixed(ctx, instances):
    """pcdl::check of m instances, each of its own degree bound (read from the blob's word 12), in one call
    (halo_pcdl_check_batch_mixed) -> status list; statuses and HaloReject as check_batch"""
    return _check_batch_mixed(ctx, ctx.lib.halo_pcdl_check_batch_mixed, instances)


def check_batch_mixed_combined(ctx, instances, seed=None):
    """check_batch_mixed with ONE MSM for the accepted members of every size (halo_pcdl_check_batch_mixed_combined: a shorter h is a
    zero-padded vector over the same key; seed: 32 bytes of the caller's randomness or None) -> status list; statuses and
    HaloReject as check_batch_mixed whenever a member is bad"""
    return _check_batch_mixed(ctx, lambda h, ds, ps, m, st: ctx.lib.halo_pcdl_check_batch_mixed_combined(h, ds, ps, m, _seed32(seed), st), instances)


def check_batch_mixed_fused(ctx, instances, seed=None):
    """check_batch_mixed as ONE relation over the members of every size, the succinct relations included
    (halo_pcdl_check_batch_mixed_fused; seed: 32 bytes of the caller's randomness or None) -> status list; statuses and HaloReject
    as check_batch_mixed whenever a member is bad"""
    return _check_batch_mixed(ctx, lambda h, ds, ps, m, st: ctx.lib.halo_pcdl_check_batch_mixed_fused(h, ds, ps, m, _seed32(seed), st), instances)


def check_partial(ctx, Cm, d, z, v, pi, stride, offset):
    """One rank's half of pcdl::check over a cyclically sharded key (halo_pcdl_check_partial): -> (U, this rank's share of
    CM.Commit(ck, h)).  The caller adds the shares in rank order and accepts iff the sum is U (sharded.ShardedOpen.check)."""
    U, part = np.zeros(12, dtype=np.uint64), np.zeros(12, dtype=np.uint64)
    check(ctx.lib.halo_pcdl_check_partial(ctx.h, ptr(_a(Cm)), d, ptr(_a(z)), ptr(_a(v)), ptr(_a(pi)), stride, offset, ptr(U), ptr(part)))
    return U, part


class HPoly:
    """pcdl.rs:44-92"""

    def __init__(self, ctx, xis):
        self.ctx, self.xis = ctx, _a(xis).reshape(-1, 4)

    def get_poly(self):
        return self.ctx.h_coeffs(self.xis)

    def eval(self, z):
        return self.ctx.h_eval_batch(self.xis[None], z)[0]
