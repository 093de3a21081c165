"""halo_pcdl_check_batch / halo_acc_decider_batch without a GPU: exported by the product library, declared by its header,
bound by the Python prototypes and integration/ffi.rs; a null context is an argument error; the development library knows
the check batch's hooks and its h-expansion entry point."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("halo_pcdl_check_batch", "halo_acc_decider_batch")


@pytest.fixture(scope="module")
def hal():
    import halo_accumulation_amd as h
    h.build()
    return h


def test_exported_declared_and_bound(hal):
    exported = subprocess.check_output(["nm", "-D", "--defined-only", hal._lib.LIB_PATH], text=True)
    header = open(os.path.join(ROOT, "include", "halo_accumulation.h")).read()
    ffi = open(os.path.join(ROOT, "integration", "ffi.rs")).read()
    for name in NEW:
        assert re.search(r" T %s$" % name, exported, flags=re.M), name
        assert re.search(r"\bint %s\(halo_ctx \*ctx, size_t d, const uint64_t \*\w+, size_t m, int \*status" % name, header), name
        assert re.search(r"pub fn %s\(ctx: \*mut HaloCtx, d: usize, \w+: \*const u64, m: usize, status: \*mut c_int\) -> c_int;" % name, ffi), name
        assert name in hal._lib.declared_symbols()
    dev = subprocess.check_output(["nm", "-D", "--defined-only", hal._lib.DEV_LIB_PATH], text=True)
    assert re.search(r" T halo_dev_h_coeffs_batch$", dev, flags=re.M)
    assert "halo_dev_h_coeffs_batch" in hal._lib.declared_dev_symbols()


def test_null_context(hal):
    lib = hal.load()
    st = (C.c_int * 1)(77)
    for name in NEW:
        assert getattr(lib, name)(None, 511, None, 0, st) == hal._lib.HALO_E_ARG
        assert b"null context" in lib.halo_last_error()
    assert st[0] == 77
    assert lib.halo_dev_h_coeffs_batch(None, None, 1, 3, None) == hal._lib.HALO_E_ARG


def test_development_hooks(hal):
    lib = hal.load()
    assert lib.halo_dev_hook(b"batch_stage_fail", 1) == 0
    assert lib.halo_dev_hook(b"check_batch_group", 2) == 0
    assert lib.halo_dev_hook(b"reset", 0) == 0
