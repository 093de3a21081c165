"""The open batches' folded schedule without a GPU: the two development entry points are exported, declared and bound with one
signature, a null context is an argument error that writes nothing, the hook "open_batch_fold" takes 0 / 1 / 2 only and "reset"
clears it, halo_ctx_info documents what 10 reports, and the member-batched fold kernels passed the build's resource gate."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_fold_points_batch", "k_fold_points4_batch", "k_fold_points4_quad_batch")


@pytest.fixture(scope="module")
def hal():
    import halo_accumulation_amd as h
    h.build()
    return h


def test_exported_declared_and_bound(hal):
    exported = subprocess.check_output(["nm", "-D", "--defined-only", hal._lib.DEV_LIB_PATH], text=True)
    dev_header = open(os.path.join(ROOT, "include", "halo_accumulation_dev.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", dev_header, flags=re.S)
    plain = re.sub(r"\s+", " ", plain)
    for name in ("halo_dev_fold_points_batch", "halo_dev_msm_offsets"):
        assert re.search(r" T %s$" % name, exported, flags=re.M), name
        assert name in hal._lib.declared_dev_symbols()
    assert ("int halo_dev_fold_points_batch(halo_ctx *ctx, const uint64_t *key_affine , size_t n, int levels, const uint64_t *scalars , "
            "int members , int shared , int form, uint64_t *out_affine );") in plain
    assert ("int halo_dev_msm_offsets(halo_ctx *ctx, const size_t *offs , size_t n, const uint64_t *scalars , int count , "
            "int scalars_are_mont, uint64_t *out_jac );") in plain
    # the Python prototypes carry as many arguments, of the same kinds
    sigs = hal._lib._DEV_SIGS
    assert [a.__name__ for a in sigs["halo_dev_fold_points_batch"][1]] == ["c_void_p", "LP_c_ulong", "c_ulong", "c_int", "LP_c_ulong", "c_int", "c_int",
                                                                          "c_int", "LP_c_ulong"]
    assert [a.__name__ for a in sigs["halo_dev_msm_offsets"][1]] == ["c_void_p", "LP_c_ulong", "c_ulong", "LP_c_ulong", "c_int", "c_int", "LP_c_ulong"]
    header = open(os.path.join(ROOT, "include", "halo_accumulation.h")).read()
    assert re.search(r"10 = how many members of\s+\* the last halo_pcdl_open_batch / halo_random_instance_batch / halo_instance_from_poly_batch", header)
    assert '"open_batch_fold"' in dev_header


def test_null_context_and_no_context(hal):
    lib = hal.load()
    out = np.full(96, 0xA5, dtype=np.uint64)
    one = np.zeros(12, dtype=np.uint64)
    offs = (C.c_size_t * 2)(0, 0)
    p = hal._lib.ptr
    assert lib.halo_dev_fold_points_batch(None, None, 64, 2, p(one), 2, 1, 0, p(out)) == hal._lib.HALO_E_ARG
    assert b"null context" in lib.halo_last_error()
    assert lib.halo_dev_msm_offsets(None, offs, 4, p(one), 2, 1, p(out)) == hal._lib.HALO_E_ARG
    assert b"null context" in lib.halo_last_error()
    assert (out == 0xA5).all()
    assert lib.halo_ctx_info(None, 10) == 0


def test_development_hook(hal):
    lib = hal.load()
    try:
        assert lib.halo_dev_tuning(b"open_batch_fold") == 0
        for v in (1, 2, 0, 2):
            assert lib.halo_dev_hook(b"open_batch_fold", v) == 0
            assert lib.halo_dev_tuning(b"open_batch_fold") == v
        for v in (-1, 3, 77):
            assert lib.halo_dev_hook(b"open_batch_fold", v) == hal._lib.HALO_E_ARG
            assert b"open_batch_fold is 0" in lib.halo_last_error()
            assert lib.halo_dev_tuning(b"open_batch_fold") == 2, "a refused value leaves the hook as it was"
        assert lib.halo_dev_hook(b"reset", 0) == 0
        assert lib.halo_dev_tuning(b"open_batch_fold") == 0
        assert lib.halo_dev_hook(b"no_such_hook", 1) == hal._lib.HALO_E_ARG and b"open_batch_fold" in lib.halo_last_error()
    finally:
        lib.halo_dev_hook(b"reset", 0)


def test_batched_fold_kernels_pass_the_resource_gate(hal):
    res = json.load(open(os.path.join(hal._lib.CSRC, "_obj", "kernel_resources.json")))
    for k in KERNELS:
        hits = [r for name, r in res.items() if re.search(r"\d%sE" % k, name)]
        assert len(hits) == 1, k
        assert hits[0]["ScratchSize [bytes/lane]"] == "0" and int(hits[0]["VGPRs"]) <= 256, (k, hits[0])
    # (the single kernels they share their lanes with keep their registers: the build gate has no scratch anywhere)
    assert all(r["ScratchSize [bytes/lane]"] == "0" for r in res.values())
