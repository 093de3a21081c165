"""halo_pcdl_check_batch_fused / halo_acc_decider_batch_fused without a GPU: exported by the product library, declared by its
header, bound by the Python prototypes and integration/ffi.rs; a null context is an argument error; the development library alone
holds the dev entry points and knows the hook; the term kernel passed the resource gate; and the 2 M weights of the fused relation
(halo_dev_check_fused_weights) are the rule of include/halo_accumulation.h restated with hashlib.sha3_256 and Python integers."""
import ctypes as C
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("halo_pcdl_check_batch_fused", "halo_acc_decider_batch_fused")
DEV = ("halo_dev_check_fused_weights", "halo_dev_check_fused_terms")
R_MOD = 0x40000000000000000000000000000000224698FC0994A8DD8C46EB2100000001
DOMAIN = b"halo-accumulation/check-batch-fused/v1"


@pytest.fixture(scope="module")
def hal():
    import halo_accumulation_amd as h
    h.build()
    return h


def ptr(a):
    from halo_accumulation_amd._lib import ptr as p
    return p(a)


def test_exported_declared_and_bound(hal):
    exported = subprocess.check_output(["nm", "-D", "--defined-only", hal._lib.LIB_PATH], text=True)
    header = open(os.path.join(ROOT, "include", "halo_accumulation.h")).read()
    ffi = open(os.path.join(ROOT, "integration", "ffi.rs")).read()
    for name in NEW:
        assert re.search(r" T %s$" % name, exported, flags=re.M), name
        assert re.search(r"\bint %s\(halo_ctx \*ctx, size_t d, const uint64_t \*\w+, size_t m, const uint8_t seed\[32\] /\*nullable\*/,\s*int \*status /\*nullable\*/\);"
                         % name, header), name
        assert re.search(r"pub fn %s\(ctx: \*mut HaloCtx, d: usize, \w+: \*const u64, m: usize, seed: \*const u8, status: \*mut c_int\) -> c_int;"
                         % name, ffi), name
        assert name in hal._lib.declared_symbols()
    assert "Weight rule (fused)" in header and DOMAIN.decode() in header, "the header states the weight rule"
    from halo_accumulation_amd import acc, pcdl
    assert callable(pcdl.check_batch_fused) and callable(acc.decider_batch_fused)


def test_dev_symbols_are_in_the_development_library_only(hal):
    prod = subprocess.check_output(["nm", "-D", "--defined-only", hal._lib.LIB_PATH], text=True)
    dev = subprocess.check_output(["nm", "-D", "--defined-only", hal._lib.DEV_LIB_PATH], text=True)
    dev_header = open(os.path.join(ROOT, "include", "halo_accumulation_dev.h")).read()
    for name in DEV:
        assert re.search(r" T %s$" % name, dev, flags=re.M), name
        assert not re.search(r"\b%s$" % name, prod, flags=re.M), name
        assert name in hal._lib.declared_dev_symbols() and name not in hal._lib.declared_symbols()
        assert re.search(r"\bint %s\(" % name, dev_header), name
    for name in NEW:
        assert not re.search(r"\b%s$" % name, dev, flags=re.M), name


def test_null_context(hal):
    lib = hal.load()
    st = (C.c_int * 1)(77)
    for name in NEW:
        assert getattr(lib, name)(None, 511, None, 0, None, st) == hal._lib.HALO_E_ARG
        assert b"null context" in lib.halo_last_error()
        assert getattr(lib, name)(None, 511, None, 1, bytes(32), st) == hal._lib.HALO_E_ARG
    assert st[0] == 77
    out = np.zeros(4, dtype=np.uint64)
    assert lib.halo_dev_check_fused_terms(None, None, 1, 3, None, ptr(out)) == hal._lib.HALO_E_ARG


def test_development_hook(hal):
    lib = hal.load()
    try:
        for value in (8, 64, 100, 1 << 20, 0):
            assert lib.halo_dev_hook(b"check_fused_chunk", value) == 0, value
        for value in (1, 7, -1):
            assert lib.halo_dev_hook(b"check_fused_chunk", value) == hal._lib.HALO_E_ARG, value
            assert b"check_fused_chunk" in lib.halo_last_error()
    finally:
        assert lib.halo_dev_hook(b"reset", 0) == 0


def test_term_kernel_passed_the_resource_gate(hal):
    res = json.load(open(os.path.join(ROOT, "halo-accumulation_amd", "csrc", "_obj", "kernel_resources.json")))
    mine = [r for name, r in res.items() if "k_fused_terms" in name]
    assert len(mine) == 1 and mine[0]["ScratchSize [bytes/lane]"] == "0" and mine[0]["Dynamic Stack"] == "False"
    assert mine[0]["LDS Size [bytes/block]"] == "0"
    gate = open(os.path.join(ROOT, "halo-accumulation_amd", "csrc", "check_resources.py")).read()
    assert '"k_fused_terms"' in gate, "the gate fails if the kernel's remarks go missing"


# ------------------------------------------------------------------ the weight rule
def le64(v):
    return int(v).to_bytes(8, "little")


def weights_by_the_rule(blobs, idx, d, seed, W):
    """blobs: (m, stride) uint64; -> [(r_a, s_a)] as integers"""
    h = hashlib.sha3_256()
    h.update(DOMAIN)
    h.update(bytes(32) if seed is None else seed)
    h.update(le64(d))
    h.update(le64(len(idx)))
    for i in idx:
        h.update(le64(i))
        h.update(b"".join(le64(w) for w in blobs[i, :W]))
    D = h.digest()
    w = [int.from_bytes(hashlib.sha3_256(D + le64(k)).digest(), "little") % R_MOD for k in range(2 * len(idx))]
    return [(w[2 * a], w[2 * a + 1]) for a in range(len(idx))]


def dev_weights(hal, blobs, idx, d, seed):
    """-> [(r_a, s_a)] of halo_dev_check_fused_weights as integers (out of Montgomery form: x R mod r with R = 2^256)"""
    lib = hal.load()
    blobs = np.ascontiguousarray(blobs, dtype=np.uint64)
    ix = (C.c_size_t * len(idx))(*idx)
    out = np.zeros((2 * len(idx), 4), dtype=np.uint64)
    assert lib.halo_dev_check_fused_weights(ptr(blobs), blobs.shape[1], ix, len(idx), d, seed, ptr(out)) == 0, lib.halo_last_error()
    r_inv = pow(1 << 256, -1, R_MOD)
    w = [sum(int(out[k, j]) << (64 * j) for j in range(4)) * r_inv % R_MOD for k in range(2 * len(idx))]
    return [(w[2 * a], w[2 * a + 1]) for a in range(len(idx))]


def synthetic(hal, lg, m, extra=0, salt=0):
    """m blobs of random words at a stride of an Instance plus `extra` words (an Accumulator's tail)"""
    W = int(hal.load().halo_instance_words(lg))
    rng = np.random.default_rng(2000 * lg + m + salt)
    return rng.integers(0, 1 << 64, size=(m, W + extra), dtype=np.uint64), W


def every_weight_differs(a, b):
    return all(x[0] != y[0] and x[1] != y[1] for x, y in zip(a, b))


@pytest.mark.parametrize("lg", [1, 3, 14])
@pytest.mark.parametrize("M", [2, 3, 65])
def test_weights_equal_the_restated_rule(hal, lg, M):
    d = (1 << lg) - 1
    m = M + 3
    blobs, W = synthetic(hal, lg, m, extra=24 if M == 3 else 0)
    idx = [i for i in range(m) if i not in (1, 3, m - 1)]  # (the members taking part: three were rejected)
    assert len(idx) == M
    seed = bytes(range(1, 33))
    want = weights_by_the_rule(blobs, idx, d, seed, W)
    assert dev_weights(hal, blobs, idx, d, seed) == want
    flat = [x for pair in want for x in pair]
    assert len(set(flat)) == 2 * M and all(0 < x < R_MOD for x in flat), "r_a != s_a, and no two alike"
    # the fused rule has its own domain: not the combined call's weights
    out = np.zeros((M, 4), dtype=np.uint64)
    ix = (C.c_size_t * M)(*idx)
    assert hal.load().halo_dev_check_weights(ptr(np.ascontiguousarray(blobs)), blobs.shape[1], ix, M, d, seed, ptr(out)) == 0
    r_inv = pow(1 << 256, -1, R_MOD)
    combined = {sum(int(out[a, j]) << (64 * j) for j in range(4)) * r_inv % R_MOD for a in range(M)}
    assert not combined & set(flat)
    # a null seed is 32 zero bytes; another seed gives other weights
    null = dev_weights(hal, blobs, idx, d, None)
    assert null == dev_weights(hal, blobs, idx, d, bytes(32)) == weights_by_the_rule(blobs, idx, d, None, W)
    assert every_weight_differs(null, want)
    # words behind the Instance (an accumulator's tail) are not hashed
    if blobs.shape[1] > W:
        tail = blobs.copy()
        tail[:, W:] ^= np.uint64(1)
        assert dev_weights(hal, tail, idx, d, seed) == want


@pytest.mark.parametrize("lg", [1, 3, 14])
def test_every_blob_bit_and_the_member_order_reach_every_weight(hal, lg):
    d = (1 << lg) - 1
    M = 3
    blobs, W = synthetic(hal, lg, M, salt=7)
    idx = list(range(M))
    base = dev_weights(hal, blobs, idx, d, None)
    for member in range(M):
        for word, bit in ((0, 0), (W // 2, 17), (W - 1, 63)):
            changed = blobs.copy()
            changed[member, word] ^= np.uint64(1 << bit)
            got = dev_weights(hal, changed, idx, d, None)
            assert got == weights_by_the_rule(changed, idx, d, None, W)
            assert every_weight_differs(got, base), "member %d word %d" % (member, word)
    for perm in ([1, 0, 2], [0, 2, 1], [2, 0, 1]):  # two members swapped, and a rotation
        got = dev_weights(hal, blobs, perm, d, None)
        assert got == weights_by_the_rule(blobs, perm, d, None, W)
        assert every_weight_differs(got, base), perm
    fewer = dev_weights(hal, blobs, idx[:2], d, None)
    assert every_weight_differs(fewer, base[:2]), "the member count is hashed"


def test_weight_argument_errors(hal):
    lib = hal.load()
    blobs, W = synthetic(hal, 3, 2)
    ix = (C.c_size_t * 2)(0, 1)
    out = np.zeros((4, 4), dtype=np.uint64)
    assert lib.halo_dev_check_fused_weights(None, W, ix, 2, 7, None, ptr(out)) == hal._lib.HALO_E_ARG
    assert lib.halo_dev_check_fused_weights(ptr(blobs), W, ix, 2, 6, None, ptr(out)) == hal._lib.HALO_E_ARG
    assert lib.halo_dev_check_fused_weights(ptr(blobs), W - 1, ix, 2, 7, None, ptr(out)) == hal._lib.HALO_E_ARG
    assert lib.halo_dev_check_fused_weights(ptr(blobs), W, ix, 0, 7, None, None) == 0
