"""halo_acc_verifier_batch without a GPU: exported by the product library, declared by its header with its prototype, bound by
the Python prototypes and integration/ffi.rs; a null context is an argument error that leaves status untouched; the development
library exports the segmented small MSM (halo_dev_small_msm_seg) and its header declares it."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "halo_acc_verifier_batch"


@pytest.fixture(scope="module")
def hal():
    import halo_accumulation_amd as h
    h.build()
    return h


def test_exported_declared_and_bound(hal):
    exported = subprocess.check_output(["nm", "-D", "--defined-only", hal._lib.LIB_PATH], text=True)
    assert re.search(r" T %s$" % NAME, exported, flags=re.M)
    header = " ".join(open(os.path.join(ROOT, "include", "halo_accumulation.h")).read().split())
    assert ("int halo_acc_verifier_batch(halo_ctx *ctx, size_t d, const uint64_t *instances, const size_t *counts, size_t k, "
            "const uint64_t *accs, int *status /*nullable*/);") in header
    ffi = open(os.path.join(ROOT, "integration", "ffi.rs")).read()
    assert ("pub fn halo_acc_verifier_batch(ctx: *mut HaloCtx, d: usize, instances: *const u64, counts: *const usize, k: usize, "
            "accs: *const u64, status: *mut c_int) -> c_int;") in ffi
    assert NAME in hal._lib.declared_symbols()
    from halo_accumulation_amd import acc
    assert callable(acc.verifier_batch)


def test_development_entry_point(hal):
    dev = subprocess.check_output(["nm", "-D", "--defined-only", hal._lib.DEV_LIB_PATH], text=True)
    assert re.search(r" T halo_dev_small_msm_seg$", dev, flags=re.M)
    header = " ".join(open(os.path.join(ROOT, "include", "halo_accumulation_dev.h")).read().split())
    assert ("int halo_dev_small_msm_seg(halo_ctx *ctx, const uint64_t *points, const uint64_t *scalars, const size_t *lens, "
            "size_t nsums, uint64_t *out_jac);") in header
    assert "halo_dev_small_msm_seg" in hal._lib.declared_dev_symbols()


def test_null_context(hal):
    lib = hal.load()
    st = (C.c_int * 2)(77, 77)
    counts = (C.c_size_t * 2)(1, 1)
    assert lib.halo_acc_verifier_batch(None, 511, None, counts, 2, None, st) == hal._lib.HALO_E_ARG
    assert b"null context" in lib.halo_last_error()
    assert list(st) == [77, 77]
    assert lib.halo_acc_verifier_batch(None, 511, None, None, 0, None, None) == hal._lib.HALO_E_ARG
    assert lib.halo_dev_small_msm_seg(None, None, None, None, 1, None) == hal._lib.HALO_E_ARG
