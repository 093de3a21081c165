"""halo_pcdl_open_batch / halo_random_instance_batch without a GPU: exported by the product library, declared by its header,
bound by the Python prototypes and integration/ffi.rs; a null context is an argument error that writes nothing; the development
library knows the open batch's hook; the member-batched kernels passed the build's resource gate."""
import ctypes as C
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_poly_eval_partial_batch", "k_sum_partials_batch", "k_powers_batch", "k_pbar_batch", "k_rng_batch", "k_axpy_batch",
           "k_nofold_expand_batch", "k_dot2_partial_batch", "k_fold_scalars_batch", "k_nofold_s_update_batch")


@pytest.fixture(scope="module")
def hal():
    import halo_accumulation_amd as h
    h.build()
    return h


def test_exported_declared_and_bound(hal):
    exported = subprocess.check_output(["nm", "-D", "--defined-only", hal._lib.LIB_PATH], text=True)
    header = open(os.path.join(ROOT, "include", "halo_accumulation.h")).read()
    ffi = open(os.path.join(ROOT, "integration", "ffi.rs")).read()
    for name in ("halo_pcdl_open_batch", "halo_random_instance_batch"):
        assert re.search(r" T %s$" % name, exported, flags=re.M), name
        assert name in hal._lib.declared_symbols()
    assert re.search(r"\bint halo_pcdl_open_batch\(halo_ctx \*ctx, uint64_t \*rng_state, size_t d, const uint64_t \*coeffs, size_t m, "
                     r"const uint64_t \*Cs,\s+const uint64_t \*zs, const uint64_t \*ws /\*nullable\*/, uint64_t \*proofs_out, "
                     r"int \*status /\*nullable\*/\);", header)
    assert re.search(r"\bint halo_random_instance_batch\(halo_ctx \*ctx, uint64_t \*rng_state, size_t d, size_t m, uint64_t \*instances_out\);",
                     header)
    assert re.search(r"pub fn halo_pcdl_open_batch\(ctx: \*mut HaloCtx, rng_state: \*mut u64, d: usize, coeffs: \*const u64, m: usize, "
                     r"cs: \*const u64, zs: \*const u64,\s+ws: \*const u64, proofs_out: \*mut u64, status: \*mut c_int\) -> c_int;", ffi)
    assert re.search(r"pub fn halo_random_instance_batch\(ctx: \*mut HaloCtx, rng_state: \*mut u64, d: usize, m: usize, "
                     r"instances_out: \*mut u64\) -> c_int;", ffi)


def test_null_context(hal):
    lib = hal.load()
    st = (C.c_int * 1)(77)
    state = C.c_uint64(1234)
    assert lib.halo_pcdl_open_batch(None, C.byref(state), 511, None, 1, None, None, None, None, st) == hal._lib.HALO_E_ARG
    assert b"null context" in lib.halo_last_error()
    assert lib.halo_random_instance_batch(None, C.byref(state), 511, 1, None) == hal._lib.HALO_E_ARG
    assert b"null context" in lib.halo_last_error()
    assert st[0] == 77 and state.value == 1234


def test_development_hook(hal):
    lib = hal.load()
    for g in (0, 1, 2, 4):
        assert lib.halo_dev_hook(b"open_batch_group", g) == 0
    assert lib.halo_dev_hook(b"batch_stage_fail", 1) == 0
    assert lib.halo_dev_hook(b"reset", 0) == 0


def test_batched_kernels_pass_the_resource_gate(hal):
    res = json.load(open(os.path.join(hal._lib.CSRC, "_obj", "kernel_resources.json")))
    for k in KERNELS:
        hits = [r for name, r in res.items() if re.search(r"\d%s" % k, name)]
        assert len(hits) == 1, k
        assert hits[0]["ScratchSize [bytes/lane]"] == "0" and int(hits[0]["VGPRs"]) <= 256, (k, hits[0])
