"""The two development hooks of tests/test_gpu_point_paths.py without a GPU: halo_dev_batch_to_affine and halo_dev_batch_small_msm
are exported by the development library and by it alone, declared by its header with their prototypes and bound by the Python
prototypes; a null context is an argument error with a message."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROTOTYPES = {
    "halo_dev_batch_to_affine": "int halo_dev_batch_to_affine(halo_ctx *ctx, const uint64_t *pts_jac, size_t m, uint64_t *out_affine);",
    "halo_dev_batch_small_msm": ("int halo_dev_batch_small_msm(halo_ctx *ctx, const uint64_t *points, const uint64_t *scalars, size_t m, size_t K, "
                                 "uint64_t *out_jac);"),
}


@pytest.fixture(scope="module")
def hal():
    import halo_accumulation_amd as h
    h.build()
    return h


def test_exported_declared_and_bound(hal):
    dev = subprocess.check_output(["nm", "-D", "--defined-only", hal._lib.DEV_LIB_PATH], text=True)
    product = subprocess.check_output(["nm", "-D", "--defined-only", hal._lib.LIB_PATH], text=True)
    header = " ".join(open(os.path.join(ROOT, "include", "halo_accumulation_dev.h")).read().split())
    for name, proto in PROTOTYPES.items():
        assert re.search(r" T %s$" % name, dev, flags=re.M)
        assert name not in product, "libhalo_hip.so is unchanged: the hooks live in the development library"
        assert proto in header
        assert name in hal._lib.declared_dev_symbols() and name not in hal._lib.declared_symbols()
    for method in ("batch_to_affine", "batch_small_msm", "small_msm_seg"):
        assert callable(getattr(hal._lib.Context, method))


def test_null_arguments(hal):
    lib = hal.load()
    assert lib.halo_dev_batch_to_affine(None, None, 1, None) == hal._lib.HALO_E_ARG
    assert b"null context" in lib.halo_last_error()
    assert lib.halo_dev_batch_to_affine(None, None, 0, None) == hal._lib.HALO_E_ARG
    assert lib.halo_dev_batch_small_msm(None, None, None, 1, 22, None) == hal._lib.HALO_E_ARG
    assert b"null context" in lib.halo_last_error()
    assert lib.halo_dev_batch_small_msm(None, None, None, 0, 0, None) == hal._lib.HALO_E_ARG
