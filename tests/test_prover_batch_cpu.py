"""halo_acc_prover_batch without a GPU: exported by the product library, declared by its header with its prototype, bound by the
Python prototypes and integration/ffi.rs; a null context is an argument error that leaves status, the rng state and the output
untouched; the development library exports the accumulation hook (halo_dev_h_accumulate_batch) and its header declares it; the
two kernels of the accumulated polynomial pass the build's resource gate."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "halo_acc_prover_batch"


@pytest.fixture(scope="module")
def hal():
    import halo_accumulation_amd as h
    h.build()
    return h


def test_exported_declared_and_bound(hal):
    exported = subprocess.check_output(["nm", "-D", "--defined-only", hal._lib.LIB_PATH], text=True)
    assert re.search(r" T %s$" % NAME, exported, flags=re.M)
    header = " ".join(open(os.path.join(ROOT, "include", "halo_accumulation.h")).read().split())
    assert ("int halo_acc_prover_batch(halo_ctx *ctx, uint64_t *rng_state, size_t d, const uint64_t *instances, const size_t *counts, "
            "size_t k, uint64_t *accs_out, int *status /*nullable*/);") in header
    ffi = " ".join(open(os.path.join(ROOT, "integration", "ffi.rs")).read().split())
    assert ("pub fn halo_acc_prover_batch(ctx: *mut HaloCtx, rng_state: *mut u64, d: usize, instances: *const u64, counts: *const usize, "
            "k: usize, accs_out: *mut u64, status: *mut c_int) -> c_int;") in ffi
    assert NAME in hal._lib.declared_symbols()
    from halo_accumulation_amd import acc
    assert callable(acc.prover_batch)


def test_development_entry_point(hal):
    dev = subprocess.check_output(["nm", "-D", "--defined-only", hal._lib.DEV_LIB_PATH], text=True)
    assert re.search(r" T halo_dev_h_accumulate_batch$", dev, flags=re.M)
    product = subprocess.check_output(["nm", "-D", "--defined-only", hal._lib.LIB_PATH], text=True)
    assert "halo_dev_h_accumulate_batch" not in product
    header = " ".join(open(os.path.join(ROOT, "include", "halo_accumulation_dev.h")).read().split())
    assert ("int halo_dev_h_accumulate_batch(halo_ctx *ctx, const uint64_t *h0s, const uint64_t *xis, const uint64_t *alphas, "
            "const size_t *counts, size_t members, size_t lg_n, size_t max_tables, uint64_t *out);") in header
    assert "halo_dev_h_accumulate_batch" in hal._lib.declared_dev_symbols()


def test_null_context(hal):
    lib = hal.load()
    st = (C.c_int * 2)(77, 77)
    counts = (C.c_size_t * 2)(1, 1)
    state = C.c_uint64(0x1234)
    out = np.full(64, 0xABCD, dtype=np.uint64)
    assert lib.halo_acc_prover_batch(None, C.byref(state), 511, None, counts, 2, hal._lib.ptr(out), st) == hal._lib.HALO_E_ARG
    assert b"null context" in lib.halo_last_error()
    assert list(st) == [77, 77] and state.value == 0x1234 and (out == 0xABCD).all()
    assert lib.halo_acc_prover_batch(None, None, 511, None, None, 0, None, None) == hal._lib.HALO_E_ARG
    assert lib.halo_dev_h_accumulate_batch(None, None, None, None, None, 1, 3, 0, None) == hal._lib.HALO_E_ARG


def test_kernels_pass_the_resource_gate(hal):
    with open(os.path.join(ROOT, "halo-accumulation_amd", "csrc", "_obj", "kernel_resources.json")) as f:
        res = json.load(f)
    for kernel in ("k_h_accumulate_batch", "k_h_tables"):
        hits = [v for name, v in res.items() if re.search(r"\d%sE" % kernel, name)]
        assert len(hits) == 1, kernel
        assert int(hits[0]["ScratchSize [bytes/lane]"]) == 0 and hits[0]["Dynamic Stack"] == "False", kernel
        assert int(hits[0]["VGPRs"]) <= 256 and int(hits[0]["VGPRs Spill"]) == 0, kernel
