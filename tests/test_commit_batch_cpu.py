"""halo_pcdl_commit_batch / halo_pcdl_commit_dev_batch / halo_instance_from_poly / halo_instance_from_poly_batch without a GPU:
exported, declared and bound; a null context touches nothing; the "commit_batch_group" hook; the padding kernel's resources; the
Python wrappers' own argument checks."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEADER = {
    "halo_pcdl_commit_batch": "int halo_pcdl_commit_batch(halo_ctx *ctx, size_t d, const uint64_t *coeffs, size_t m, const uint64_t *ws /*nullable*/, "
                              "uint64_t *out_jac);",
    "halo_pcdl_commit_dev_batch": "int halo_pcdl_commit_dev_batch(halo_ctx *ctx, size_t d, const void *const *d_coeffs, const size_t *lens, size_t m, "
                                  "const uint64_t *ws /*nullable*/, uint64_t *out_jac, int *status /*nullable*/);",
    "halo_instance_from_poly": "int halo_instance_from_poly(halo_ctx *ctx, uint64_t *rng_state, const uint64_t *coeffs, size_t len, size_t d, "
                               "const uint64_t z[4], const uint64_t *w /*nullable*/, uint64_t *instance_out);",
    "halo_instance_from_poly_batch": "int halo_instance_from_poly_batch(halo_ctx *ctx, uint64_t *rng_state, size_t d, const uint64_t *coeffs, size_t m, "
                                     "const uint64_t *zs, const uint64_t *ws /*nullable*/, uint64_t *instances_out, int *status /*nullable*/);",
}
FFI = {
    "halo_pcdl_commit_batch": "pub fn halo_pcdl_commit_batch(ctx: *mut HaloCtx, d: usize, coeffs: *const u64, m: usize, ws: *const u64, out_jac: *mut u64) "
                              "-> c_int;",
    "halo_pcdl_commit_dev_batch": "pub fn halo_pcdl_commit_dev_batch(ctx: *mut HaloCtx, d: usize, d_coeffs: *const *const c_void, lens: *const usize, "
                                  "m: usize, ws: *const u64, out_jac: *mut u64, status: *mut c_int) -> c_int;",
    "halo_instance_from_poly": "pub fn halo_instance_from_poly(ctx: *mut HaloCtx, rng_state: *mut u64, coeffs: *const u64, len: usize, d: usize, "
                               "z: *const u64, w: *const u64, instance_out: *mut u64) -> c_int;",
    "halo_instance_from_poly_batch": "pub fn halo_instance_from_poly_batch(ctx: *mut HaloCtx, rng_state: *mut u64, d: usize, coeffs: *const u64, m: usize, "
                                     "zs: *const u64, ws: *const u64, instances_out: *mut u64, status: *mut c_int) -> c_int;",
}


@pytest.fixture(scope="module")
def hal():
    import halo_accumulation_amd as h
    h.build()
    return h


@pytest.fixture(scope="module")
def lib(hal):
    return hal.load()


def ptr(a):
    from halo_accumulation_amd._lib import ptr as p
    return None if a is None else p(a)


def test_exported_declared_and_bound(hal):
    exported = subprocess.check_output(["nm", "-D", "--defined-only", hal._lib.LIB_PATH], text=True)
    header = " ".join(open(os.path.join(ROOT, "include", "halo_accumulation.h")).read().split())
    ffi = " ".join(open(os.path.join(ROOT, "integration", "ffi.rs")).read().split())
    for name in HEADER:
        assert re.search(r" T %s$" % name, exported, flags=re.M), name
        assert HEADER[name] in header, name
        assert FFI[name] in ffi, name
        assert name in hal._lib.declared_symbols()
    from halo_accumulation_amd import acc, pcdl
    for fn in (pcdl.commit_batch, pcdl.commit_dev_batch, acc.instance_from_poly, acc.instance_from_poly_batch):
        assert callable(fn)


def test_null_context_touches_nothing(hal, lib):
    lg, m = 3, 2
    n = 1 << lg
    iw = lib.halo_instance_words(lg)
    coeffs = np.ones((m, n, 4), dtype=np.uint64)
    zs = np.ones((m, 4), dtype=np.uint64)
    ws = np.ones((m, 4), dtype=np.uint64)
    mark = np.uint64(0xA5A5A5A5A5A5A5A5)

    def untouched(rc, out, status=None, st=None):
        assert rc == hal._lib.HALO_E_ARG and lib.halo_last_error().decode() == "null context"
        assert (out == mark).all()
        assert status is None or list(status) == [77] * m
        assert st is None or st.value == 0x1234

    out = np.full((m, 12), mark, dtype=np.uint64)
    untouched(lib.halo_pcdl_commit_batch(None, n - 1, ptr(coeffs), m, ptr(ws), ptr(out)), out)
    status = (C.c_int * m)(77, 77)
    ptrs = (C.c_void_p * m)(64, 128)
    lens = (C.c_size_t * m)(n, n)
    untouched(lib.halo_pcdl_commit_dev_batch(None, n - 1, ptrs, lens, m, ptr(ws), ptr(out), status), out, status)
    st = C.c_uint64(0x1234)
    inst = np.full(iw, mark, dtype=np.uint64)
    untouched(lib.halo_instance_from_poly(None, C.byref(st), ptr(coeffs[0]), n, n - 1, ptr(zs[0]), ptr(ws[0]), ptr(inst)), inst, None, st)
    insts = np.full((m, iw), mark, dtype=np.uint64)
    untouched(lib.halo_instance_from_poly_batch(None, C.byref(st), n - 1, ptr(coeffs), m, ptr(zs), ptr(ws), ptr(insts), status), insts, status, st)


def test_commit_batch_group_hook(hal, lib):
    try:
        for g in (0, 1, 3, 8):
            assert lib.halo_dev_hook(b"commit_batch_group", g) == 0
            assert lib.halo_dev_tuning(b"commit_batch_group") == g
        assert lib.halo_dev_hook(b"commit_batch_group", 3) == 0
        assert lib.halo_dev_hook(b"reset", 0) == 0
        assert lib.halo_dev_tuning(b"commit_batch_group") == 0, "reset clears the hook"
        assert lib.halo_dev_hook(b"commit_batch_groups", 1) == hal._lib.HALO_E_ARG
        assert "commit_batch_group" in lib.halo_last_error().decode(), "the unknown-hook message lists it"
    finally:
        lib.halo_dev_hook(b"reset", 0)


def test_padding_kernel_passes_the_resource_gate(hal):
    res = json.load(open(os.path.join(hal._lib.CSRC, "_obj", "kernel_resources.json")))
    hits = [(k, v) for k, v in _kernels(res) if "k_pad_members_batch" in k]
    assert len(hits) == 1, [k for k, _ in hits]
    k = hits[0][1]
    assert int(k["ScratchSize [bytes/lane]"]) == 0 and int(k["SGPRs Spill"]) == 0 and k["Dynamic Stack"] == "False"
    assert 0 < int(k["VGPRs"]) <= 256


def _kernels(node):
    """(name, record) of every kernel record in the resource file, whatever its nesting by translation unit"""
    for key, val in node.items():
        if isinstance(val, dict) and "ScratchSize [bytes/lane]" in val:
            yield key, val
        elif isinstance(val, dict):
            yield from _kernels(val)


class _NoLibrary:
    """stands for a context: a wrapper that reached the library would touch .lib"""

    @property
    def lib(self):
        raise AssertionError("the wrapper called the library")

    h = None


def test_wrappers_reject_ragged_inputs(hal):
    from halo_accumulation_amd import acc, pcdl
    p = np.ones((4, 4), dtype=np.uint64)
    w = np.ones(4, dtype=np.uint64)
    c = _NoLibrary()
    with pytest.raises(ValueError):
        pcdl.commit_batch(c, [p, p, p], 3, [w, w])
    with pytest.raises(AssertionError, match="p.degree\\(\\) > d"):
        pcdl.commit_batch(c, [np.ones((8, 4), dtype=np.uint64)], 3)
    with pytest.raises(ValueError):
        pcdl.commit_dev_batch(c, [64, 128], [4], 3)
    with pytest.raises(ValueError):
        pcdl.commit_dev_batch(c, [64, 128], [4, 4], 3, [w])
    with pytest.raises(ValueError):
        acc.instance_from_poly_batch(c, [1], [p, p], 3, [w])
    with pytest.raises(ValueError):
        acc.instance_from_poly_batch(c, [1], [p, p], 3, [w, w], [w, w, w])
    with pytest.raises(ValueError):
        acc.instance_from_poly_batch(c, [1], [p, p], 3, None)
    with pytest.raises(ValueError):
        pcdl.commit_batch(c, [p], 3, [np.ones(5, dtype=np.uint64)])
