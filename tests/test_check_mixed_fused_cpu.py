"""halo_pcdl_check_batch_mixed_fused / halo_acc_decider_batch_mixed_fused without a GPU: exported by the product library and not by
the development library, declared by the header with the mixed calls' prototype, covered by the export maps, bound by the Python
prototypes and integration/ffi.rs; the Python wrappers' packing and argument errors; a null context is an argument error; the
weights (halo_dev_check_mixed_fused_weights) are the rule of include/halo_accumulation.h restated with hashlib.sha3_256 and Python
integers, under a domain of their own; and k_mixed_terms passed the resource gate."""
import ctypes as C
import fnmatch
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import test_check_mixed_cpu as mc

ROOT = mc.ROOT
FUSED = ("halo_pcdl_check_batch_mixed_fused", "halo_acc_decider_batch_mixed_fused")
DEV = ("halo_dev_check_mixed_fused_weights", "halo_dev_check_mixed_terms")
R_MOD = mc.R_MOD
DOMAIN = b"halo-accumulation/check-batch-mixed-fused/v1"
UNIFORM_FUSED_DOMAIN = b"halo-accumulation/check-batch-fused/v1"


@pytest.fixture(scope="module")
def hal():
    import halo_accumulation_amd as h
    h.build()
    return h


ptr = mc.ptr
le64 = mc.le64


# ------------------------------------------------------------------ the names
def test_exported_declared_and_bound(hal):
    exported = subprocess.check_output(["nm", "-D", "--defined-only", hal._lib.LIB_PATH], text=True)
    dev = subprocess.check_output(["nm", "-D", "--defined-only", hal._lib.DEV_LIB_PATH], text=True)
    header = open(os.path.join(ROOT, "include", "halo_accumulation.h")).read()
    ffi = open(os.path.join(ROOT, "integration", "ffi.rs")).read()
    product_map = mc.map_globals("product.map")
    for name in FUSED:
        assert re.search(r" T %s$" % name, exported, flags=re.M), name
        assert not re.search(r"\b%s$" % name, dev, flags=re.M), name
        assert re.search(r"\bint %s\(halo_ctx \*ctx, const size_t \*ds, const uint64_t \*const \*\w+, size_t m,\s+const uint8_t seed\[32\] /\*nullable\*/,"
                         r"\s+int \*status /\*nullable\*/\);" % name, header), name
        assert re.search(r"pub fn %s\(ctx: \*mut HaloCtx, ds: \*const usize, \w+: \*const \*const u64, m: usize, seed: \*const u8, status: \*mut c_int\) -> c_int;"
                         % name, ffi), name
        assert name in hal._lib.declared_symbols() and name not in hal._lib.declared_dev_symbols()
        assert any(fnmatch.fnmatchcase(name, p) for p in product_map), "product.map exports it"
    assert "Weight rule (mixed fused)" in header and DOMAIN.decode() in header, "the header states the weight rule"
    from halo_accumulation_amd import acc, pcdl
    assert callable(pcdl.check_batch_mixed_fused) and callable(acc.decider_batch_mixed_fused)


def test_dev_symbols_are_in_the_development_library_only(hal):
    prod = subprocess.check_output(["nm", "-D", "--defined-only", hal._lib.LIB_PATH], text=True)
    dev = subprocess.check_output(["nm", "-D", "--defined-only", hal._lib.DEV_LIB_PATH], text=True)
    dev_header = open(os.path.join(ROOT, "include", "halo_accumulation_dev.h")).read()
    header = open(os.path.join(ROOT, "include", "halo_accumulation.h")).read()
    c_abi_map = mc.map_globals("c_abi.map")
    for name in DEV:
        assert re.search(r" T %s$" % name, dev, flags=re.M), name
        assert not re.search(r"\b%s$" % name, prod, flags=re.M), name
        assert name in hal._lib.declared_dev_symbols() and name not in hal._lib.declared_symbols()
        assert re.search(r"\bint %s\(" % name, dev_header) and not re.search(r"\bint %s\(" % name, header), name
        assert any(fnmatch.fnmatchcase(name, p) for p in c_abi_map)
    for hook in ("check_fused_chunk", "check_combined_parts", "check_combined_cap", "batch_stage_fail"):
        assert hook in dev_header
    assert "halo_pcdl_check_batch_mixed_fused" in dev_header, "the hook list says which hooks the new call reads"


def test_the_term_kernel_passed_the_resource_gate(hal):
    csrc = os.path.join(ROOT, "halo-accumulation_amd", "csrc")
    res = json.load(open(os.path.join(csrc, "_obj", "kernel_resources.json")))
    gate = open(os.path.join(csrc, "check_resources.py")).read()
    mine = [r for name, r in res.items() if "k_mixed_terms" in name]
    assert len(mine) == 1, "one kernel of that name"
    assert mine[0]["ScratchSize [bytes/lane]"] == "0" and mine[0]["LDS Size [bytes/block]"] == "0" and mine[0]["Dynamic Stack"] == "False", mine[0]
    assert '"k_mixed_terms"' in gate, "the gate fails if the kernel's remarks go missing"
    assert len([name for name in res if "k_fused_terms" in name]) == 1, "the uniform call keeps its own kernel"
    kernel = open(os.path.join(csrc, "mixed_terms.hip")).read()
    lane = open(os.path.join(csrc, "mixed_terms_lane.hpp")).read()
    assert '#include "mixed_terms_lane.hpp"' in kernel and kernel.count("mixed_terms_member(") == 1 and "fused_terms_lane(" not in kernel
    assert lane.count("fused_terms_lane(") == 1 and "fs_inv(" not in lane, "the lane is fused_lane.hpp's, called once"
    assert "mixed_terms.hip" in open(os.path.join(csrc, "Makefile")).read()


# ------------------------------------------------------------------ whole-call errors that need no device
def test_null_context_and_null_pointers(hal):
    lib = hal.load()
    st = (C.c_int * 2)(77, 77)
    ds = (C.c_size_t * 2)(7, 7)
    ps = (C.c_void_p * 2)(None, None)
    for name in FUSED:
        assert getattr(lib, name)(None, ds, ps, 0, None, st) == hal._lib.HALO_E_ARG
        assert b"null context" in lib.halo_last_error()
        assert getattr(lib, name)(None, None, None, 2, bytes(32), st) == hal._lib.HALO_E_ARG
    assert list(st) == [77, 77]
    out = np.zeros(4, dtype=np.uint64)
    assert lib.halo_dev_check_mixed_terms(None, None, None, 1, None, ptr(out)) == hal._lib.HALO_E_ARG


# ------------------------------------------------------------------ the Python wrappers
class FakeLib(mc.FakeLib):
    def halo_pcdl_check_batch_mixed_fused(self, h, ds, ps, m, seed, st):
        return self._take("check_fused", h, ds, ps, m, seed, st)

    def halo_acc_decider_batch_mixed_fused(self, h, ds, ps, m, seed, st):
        return self._take("decider_fused", h, ds, ps, m, seed, st)


def test_wrappers_pack_d_from_word_12_and_one_pointer_per_blob(hal):
    from halo_accumulation_amd import acc, pcdl
    blobs = [mc.fake_blob(7, 40, 1), mc.fake_blob(511, 300, 2)[::1], mc.fake_blob(0, 30, 3).astype(np.int64), list(mc.fake_blob(7, 40, 4))]
    seed = bytes(range(32))
    for fn, name, sd in ((lambda c, b: pcdl.check_batch_mixed_fused(c, b, seed=seed), "check_fused", seed),
                         (lambda c, b: pcdl.check_batch_mixed_fused(c, b), "check_fused", None),
                         (lambda c, b: acc.decider_batch_mixed_fused(c, b, seed=seed), "decider_fused", seed),
                         (lambda c, b: acc.decider_batch_mixed_fused(c, b), "decider_fused", None)):
        lib = FakeLib()
        assert fn(mc.FakeCtx(lib), blobs) == [0, 0, 0, 0]
        (got_name, ds, words, m, got_seed), = lib.calls
        assert (got_name, ds, m, got_seed) == (name, [7, 511, 0, 7], 4, sd)
        assert [int(w[0]) for w in words] == [1, 2, 3, 4] and [int(w[12]) for w in words] == [7, 511, 0, 7]
    lib = FakeLib()
    assert pcdl.check_batch_mixed_fused(mc.FakeCtx(lib), []) == [] and lib.calls[0][3] == 0


def test_wrappers_raise_as_the_mixed_combined_ones(hal):
    from halo_accumulation_amd import acc, pcdl
    blobs = [mc.fake_blob(7, 40, 1), mc.fake_blob(511, 300, 2)]
    R = hal._lib.HALO_E_REJECT
    for fn in (pcdl.check_batch_mixed_fused, acc.decider_batch_mixed_fused):
        with pytest.raises(hal._lib.HaloReject) as e:
            fn(mc.FakeCtx(FakeLib(R, (0, R))), blobs)
        assert e.value.args == ("instance 1: told so", [0, R])
        with pytest.raises(Exception) as e:
            fn(mc.FakeCtx(FakeLib(hal._lib.HALO_E_ARG)), blobs)
        assert not isinstance(e.value, hal._lib.HaloReject)
        with pytest.raises(ValueError):
            fn(mc.FakeCtx(FakeLib()), blobs, seed=b"short")
        with pytest.raises(ValueError):
            fn(mc.FakeCtx(FakeLib()), blobs, seed=bytes(33))
        with pytest.raises(ValueError):
            fn(mc.FakeCtx(FakeLib()), [np.zeros(12, dtype=np.uint64)])  # (no word 12 to read d from)


# ------------------------------------------------------------------ the weight rule
def weights_by_the_rule(blobs, ds, idx, seed, words_of):
    """-> [(r_a, s_a)]"""
    h = hashlib.sha3_256()
    h.update(DOMAIN)
    h.update(bytes(32) if seed is None else seed)
    h.update(le64(len(idx)))
    for i in idx:
        h.update(le64(i))
        h.update(le64(ds[i]))
        h.update(b"".join(le64(w) for w in blobs[i][:words_of(ds[i])]))
    D = h.digest()
    w = [int.from_bytes(hashlib.sha3_256(D + le64(k)).digest(), "little") % R_MOD for k in range(2 * len(idx))]
    return [(w[2 * a], w[2 * a + 1]) for a in range(len(idx))]


def dev_weights(hal, blobs, ds, idx, seed):
    lib = hal.load()
    keep = [np.ascontiguousarray(b, dtype=np.uint64) for b in blobs]
    ps = (C.c_void_p * len(keep))(*[b.ctypes.data for b in keep])
    dd = (C.c_size_t * len(ds))(*ds)
    ix = (C.c_size_t * len(idx))(*idx)
    out = np.zeros((2 * len(idx), 4), dtype=np.uint64)
    assert lib.halo_dev_check_mixed_fused_weights(ps, dd, ix, len(idx), seed, ptr(out)) == 0, lib.halo_last_error()
    w = mc.from_mont(out)
    return [(w[2 * a], w[2 * a + 1]) for a in range(len(idx))]


@pytest.mark.parametrize("lgs", [[2, 3], [3, 2, 2, 3, 3], [3, 9, 10, 3, 9, 10, 3], [14, 0, 3, 14, 9]])
def test_weights_equal_the_restated_rule(hal, lgs):
    blobs, ds, words_of = mc.synthetic(hal, lgs, extra=24 if 14 in lgs else 0)
    m = len(lgs)
    idx = [i for i in range(m) if i != 1 or m < 3]  # (a subset: the members taking part)
    seed = bytes(range(1, 33))
    want = weights_by_the_rule(blobs, ds, idx, seed, words_of)
    assert dev_weights(hal, blobs, ds, idx, seed) == want
    flat = [x for pair in want for x in pair]
    assert len(set(flat)) == 2 * len(idx) and all(0 < w < R_MOD for w in flat)
    null = dev_weights(hal, blobs, ds, idx, None)
    assert null == dev_weights(hal, blobs, ds, idx, bytes(32)) == weights_by_the_rule(blobs, ds, idx, None, words_of)
    assert all(a != b for a, b in zip(null, want))
    if 14 in lgs:  # words behind the Instance (an accumulator's tail) are not hashed
        tail = [b.copy() for b in blobs]
        for b, d in zip(tail, ds):
            b[words_of(d):] ^= np.uint64(1)
        assert dev_weights(hal, tail, ds, idx, seed) == want
    # the index, the order and the degree bound reach every weight
    assert not set(flat) & {x for pair in dev_weights(hal, blobs, ds, idx[::-1], seed) for x in pair}


@pytest.mark.parametrize("lg", [2, 3])
def test_the_weights_differ_from_the_uniform_fused_and_the_mixed_combined_rules(hal, lg):
    """a batch of ONE degree bound is a valid input of all three calls: the domains keep their weights apart"""
    lib = hal.load()
    A = 4
    blobs, ds, words_of = mc.synthetic(hal, [lg] * A, salt=lg)
    idx = list(range(A))
    seed = bytes(range(7, 39))
    mine = {x for pair in dev_weights(hal, blobs, ds, idx, seed) for x in pair}
    combined = mc.dev_weights(hal, blobs, ds, idx, seed)
    assert combined == mc.weights_by_the_rule(blobs, ds, idx, seed, words_of)
    flat = np.ascontiguousarray(np.stack(blobs))
    ix = (C.c_size_t * A)(*idx)
    out = np.zeros((2 * A, 4), dtype=np.uint64)
    assert lib.halo_dev_check_fused_weights(ptr(flat), flat.shape[1], ix, A, ds[0], seed, ptr(out)) == 0
    uniform = mc.from_mont(out)
    h = hashlib.sha3_256(UNIFORM_FUSED_DOMAIN + seed + le64(ds[0]) + le64(A))
    for i in idx:
        h.update(le64(i) + flat[i].tobytes())
    assert uniform == [int.from_bytes(hashlib.sha3_256(h.digest() + le64(k)).digest(), "little") % R_MOD for k in range(2 * A)]
    assert len(mine) == 2 * A and not mine & set(uniform) and not mine & set(combined)


def test_weight_argument_errors(hal):
    lib = hal.load()
    blobs, ds, _ = mc.synthetic(hal, [2, 3])
    ps = (C.c_void_p * 2)(*[b.ctypes.data for b in blobs])
    dd = (C.c_size_t * 2)(*ds)
    ix = (C.c_size_t * 2)(0, 1)
    out = np.zeros((4, 4), dtype=np.uint64)
    E = hal._lib.HALO_E_ARG
    f = lib.halo_dev_check_mixed_fused_weights
    assert f(None, dd, ix, 2, None, ptr(out)) == E
    assert f(ps, None, ix, 2, None, ptr(out)) == E
    assert f(ps, dd, None, 2, None, ptr(out)) == E
    assert f(ps, dd, ix, 2, None, None) == E
    assert f((C.c_void_p * 2)(blobs[0].ctypes.data, None), dd, ix, 2, None, ptr(out)) == E
    assert f(ps, (C.c_size_t * 2)(3, 6), ix, 2, None, ptr(out)) == E
    assert f(ps, dd, ix, 0, None, None) == 0
