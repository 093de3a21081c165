"""halo_poly_degrees_dev / halo_poly_eval_dev / halo_instance_from_poly_dev / halo_pcdl_open_dev_batch /
halo_instance_from_poly_dev_batch without a GPU: exported by the product library, declared by its header, bound by the Python
prototypes and integration/ffi.rs; a null context is an argument error that writes nothing; the degree kernel passed the build's
resource gate; the Python wrappers' own argument checks."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("halo_poly_degrees_dev", "halo_poly_eval_dev", "halo_instance_from_poly_dev", "halo_pcdl_open_dev_batch", "halo_instance_from_poly_dev_batch")


@pytest.fixture(scope="module")
def hal():
    import halo_accumulation_amd as h
    h.build()
    return h


def ptr(a):
    from halo_accumulation_amd._lib import ptr as p
    return None if a is None else p(a)


def test_exported_declared_and_bound(hal):
    exported = subprocess.check_output(["nm", "-D", "--defined-only", hal._lib.LIB_PATH], text=True)
    header = open(os.path.join(ROOT, "include", "halo_accumulation.h")).read()
    ffi = open(os.path.join(ROOT, "integration", "ffi.rs")).read()
    for name in NAMES:
        assert re.search(r" T %s$" % name, exported, flags=re.M), name
        assert name in hal._lib.declared_symbols()
    rows_c = r"const void \*const \*d_coeffs, const size_t \*lens,\s+size_t m"
    rows_rs = r"d_coeffs: \*const \*const c_void, lens: \*const usize,\s+m: usize"
    assert re.search(r"\bint halo_poly_degrees_dev\(halo_ctx \*ctx, " + rows_c + r", size_t \*degrees_out\);", header)
    assert re.search(r"\bint halo_poly_eval_dev\(halo_ctx \*ctx, const void \*d_coeffs, size_t len, const uint64_t z\[4\], uint64_t out\[4\]\);", header)
    assert re.search(r"\bint halo_instance_from_poly_dev\(halo_ctx \*ctx, uint64_t \*rng_state, const void \*d_coeffs, size_t len, size_t d, "
                     r"const uint64_t z\[4\],\s+const uint64_t \*w /\*nullable\*/, uint64_t \*instance_out\);", header)
    assert re.search(r"\bint halo_pcdl_open_dev_batch\(halo_ctx \*ctx, uint64_t \*rng_state, size_t d, " + rows_c + r",\s+const uint64_t \*Cs, "
                     r"const uint64_t \*zs, const uint64_t \*ws /\*nullable\*/, uint64_t \*proofs_out,\s+int \*status /\*nullable\*/\);", header)
    assert re.search(r"\bint halo_instance_from_poly_dev_batch\(halo_ctx \*ctx, uint64_t \*rng_state, size_t d, " + rows_c + r", const uint64_t \*zs, "
                     r"const uint64_t \*ws /\*nullable\*/, uint64_t \*instances_out,\s+int \*status /\*nullable\*/\);", header)
    assert re.search(r"pub fn halo_poly_degrees_dev\(ctx: \*mut HaloCtx, " + rows_rs + r", degrees_out: \*mut usize\) -> c_int;", ffi)
    assert re.search(r"pub fn halo_poly_eval_dev\(ctx: \*mut HaloCtx, d_coeffs: \*const c_void, len: usize, z: \*const u64, out: \*mut u64\) -> c_int;", ffi)
    assert re.search(r"pub fn halo_instance_from_poly_dev\(ctx: \*mut HaloCtx, rng_state: \*mut u64, d_coeffs: \*const c_void, len: usize, d: usize, "
                     r"z: \*const u64,\s+w: \*const u64, instance_out: \*mut u64\) -> c_int;", ffi)
    assert re.search(r"pub fn halo_pcdl_open_dev_batch\(ctx: \*mut HaloCtx, rng_state: \*mut u64, d: usize, " + rows_rs + r",\s+cs: \*const u64, "
                     r"zs: \*const u64, ws: \*const u64, proofs_out: \*mut u64, status: \*mut c_int\) -> c_int;", ffi)
    assert re.search(r"pub fn halo_instance_from_poly_dev_batch\(ctx: \*mut HaloCtx, rng_state: \*mut u64, d: usize, " + rows_rs + r", zs: \*const u64, "
                     r"ws: \*const u64, instances_out: \*mut u64, status: \*mut c_int\) -> c_int;", ffi)
    from halo_accumulation_amd import acc, pcdl
    for fn in (pcdl.open_dev_batch, pcdl.poly_eval_dev, pcdl.poly_degrees_dev, acc.instance_from_poly_dev, acc.instance_from_poly_dev_batch):
        assert callable(fn)


def test_null_context_touches_nothing(hal):
    lib = hal.load()
    lg, m = 3, 2
    n = 1 << lg
    mark = np.uint64(0xA5A5A5A5A5A5A5A5)
    zs = np.ones((m, 4), dtype=np.uint64)
    Cs = np.ones((m, 12), dtype=np.uint64)
    ptrs = (C.c_void_p * m)(64, 128)
    lens = (C.c_size_t * m)(n, n)

    def untouched(rc, out, status=None, st=None):
        assert rc == hal._lib.HALO_E_ARG and lib.halo_last_error().decode() == "null context"
        assert (np.asarray(out) == mark).all()
        assert status is None or list(status) == [77] * m
        assert st is None or st.value == 0x1234

    degs = (C.c_size_t * m)(int(mark), int(mark))
    untouched(lib.halo_poly_degrees_dev(None, ptrs, lens, m, degs), list(degs))
    v = np.full(4, mark, dtype=np.uint64)
    untouched(lib.halo_poly_eval_dev(None, C.c_void_p(64), n, ptr(zs[0]), ptr(v)), v)
    st = C.c_uint64(0x1234)
    inst = np.full(lib.halo_instance_words(lg), mark, dtype=np.uint64)
    untouched(lib.halo_instance_from_poly_dev(None, C.byref(st), C.c_void_p(64), n, n - 1, ptr(zs[0]), ptr(zs[1]), ptr(inst)), inst, None, st)
    status = (C.c_int * m)(77, 77)
    proofs = np.full((m, lib.halo_proof_words(lg)), mark, dtype=np.uint64)
    untouched(lib.halo_pcdl_open_dev_batch(None, C.byref(st), n - 1, ptrs, lens, m, ptr(Cs), ptr(zs), ptr(zs), ptr(proofs), status), proofs, status, st)
    insts = np.full((m, lib.halo_instance_words(lg)), mark, dtype=np.uint64)
    untouched(lib.halo_instance_from_poly_dev_batch(None, C.byref(st), n - 1, ptrs, lens, m, ptr(zs), ptr(zs), ptr(insts), status), insts, status, st)


def _kernels(node):
    for key, val in node.items():
        if isinstance(val, dict) and "ScratchSize [bytes/lane]" in val:
            yield key, val
        elif isinstance(val, dict):
            yield from _kernels(val)


def test_degree_kernel_passes_the_resource_gate(hal):
    res = json.load(open(os.path.join(hal._lib.CSRC, "_obj", "kernel_resources.json")))
    hits = [(k, v) for k, v in _kernels(res) if "k_poly_degree_batch" in k]
    assert len(hits) == 1, [k for k, _ in hits]
    k = hits[0][1]
    assert int(k["ScratchSize [bytes/lane]"]) == 0 and int(k["SGPRs Spill"]) == 0 and k["Dynamic Stack"] == "False"
    assert int(k["LDS Size [bytes/block]"]) == 0
    assert 0 < int(k["VGPRs"]) <= 256


class _NoLibrary:
    """stands for a context: a wrapper that reached the library would touch .lib"""

    @property
    def lib(self):
        raise AssertionError("the wrapper called the library")

    h = None


def test_wrappers_reject_ragged_inputs(hal):
    from halo_accumulation_amd import acc, pcdl
    w = np.ones(4, dtype=np.uint64)
    P = np.ones(12, dtype=np.uint64)
    c = _NoLibrary()
    with pytest.raises(ValueError):
        pcdl.open_dev_batch(c, [1], [64, 128], [4], [P, P], 3, [w, w])
    with pytest.raises(ValueError):
        pcdl.open_dev_batch(c, [1], [64, 128], [4, 4], [P], 3, [w, w])
    with pytest.raises(ValueError):
        pcdl.open_dev_batch(c, [1], [64, 128], [4, 4], [P, P], 3, [w, w], [w])
    with pytest.raises(ValueError):
        pcdl.open_dev_batch(c, [1], [64, 128], [4, 4], None, 3, [w, w])
    with pytest.raises(ValueError):
        acc.instance_from_poly_dev_batch(c, [1], [64, 128], [4], 3, [w, w])
    with pytest.raises(ValueError):
        acc.instance_from_poly_dev_batch(c, [1], [64, 128], [4, 4], 3, None)
    with pytest.raises(ValueError):
        acc.instance_from_poly_dev_batch(c, [1], [64, 128], [4, 4], 3, [w, w], [w, w, w])
