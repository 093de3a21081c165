"""halo_pcdl_check_batch_mixed / halo_acc_decider_batch_mixed and their _combined forms without a GPU: exported by the product
library, declared by its header, covered by the export maps, bound by the Python prototypes and integration/ffi.rs; the Python
wrappers' packing (d from each blob's word 12, one pointer per blob) and argument errors; a null context is an argument error; and
the weights of the mixed relation (halo_dev_check_mixed_weights) are the rule of include/halo_accumulation.h restated with
hashlib.sha3_256 and Python integers -- under a domain of their own, so they differ from the uniform call's for the same blobs."""
import ctypes as C
import fnmatch
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = ("halo_pcdl_check_batch_mixed", "halo_acc_decider_batch_mixed")
COMBINED = ("halo_pcdl_check_batch_mixed_combined", "halo_acc_decider_batch_mixed_combined")
DEV = ("halo_dev_check_mixed_weights", "halo_dev_check_mixed_scalars")
R_MOD = 0x40000000000000000000000000000000224698FC0994A8DD8C46EB2100000001
DOMAIN = b"halo-accumulation/check-batch-mixed-combined/v1"
UNIFORM_DOMAIN = b"halo-accumulation/check-batch-combined/v1"


@pytest.fixture(scope="module")
def hal():
    import halo_accumulation_amd as h
    h.build()
    return h


def ptr(a):
    from halo_accumulation_amd._lib import ptr as p
    return p(a)


def map_globals(name):
    """the global patterns of a linker export map"""
    text = open(os.path.join(ROOT, "halo-accumulation_amd", "csrc", name)).read()
    text = re.sub(r"#.*", "", text)
    body = text[text.index("global:") + len("global:"):text.index("local:")]
    return [p.strip() for p in body.split(";") if p.strip()]


# ------------------------------------------------------------------ the names
def test_exported_declared_and_bound(hal):
    exported = subprocess.check_output(["nm", "-D", "--defined-only", hal._lib.LIB_PATH], text=True)
    header = open(os.path.join(ROOT, "include", "halo_accumulation.h")).read()
    ffi = open(os.path.join(ROOT, "integration", "ffi.rs")).read()
    product_map, c_abi_map = map_globals("product.map"), map_globals("c_abi.map")
    for name in EXACT + COMBINED:
        seed_c = r"\s+const uint8_t seed\[32\] /\*nullable\*/," if name in COMBINED else ""
        seed_rs = r" seed: \*const u8," if name in COMBINED else ""
        assert re.search(r" T %s$" % name, exported, flags=re.M), name
        assert re.search(r"\bint %s\(halo_ctx \*ctx, const size_t \*ds, const uint64_t \*const \*\w+, size_t m,%s\s+int \*status /\*nullable\*/\);"
                         % (name, seed_c), header), name
        assert re.search(r"pub fn %s\(ctx: \*mut HaloCtx, ds: \*const usize, \w+: \*const \*const u64, m: usize,%s status: \*mut c_int\) -> c_int;"
                         % (name, seed_rs), ffi), name
        assert name in hal._lib.declared_symbols()
        assert any(fnmatch.fnmatchcase(name, p) for p in product_map), "product.map exports it"
    for name in DEV:
        assert any(fnmatch.fnmatchcase(name, p) for p in c_abi_map), "c_abi.map exports it from the development library"
    assert "Weight rule (mixed)" in header and DOMAIN.decode() in header, "the header states the weight rule"
    assert "no fused form for mixed sizes" in header


def test_dev_symbols_are_in_the_development_library_only(hal):
    prod = subprocess.check_output(["nm", "-D", "--defined-only", hal._lib.LIB_PATH], text=True)
    dev = subprocess.check_output(["nm", "-D", "--defined-only", hal._lib.DEV_LIB_PATH], text=True)
    dev_header = open(os.path.join(ROOT, "include", "halo_accumulation_dev.h")).read()
    for name in DEV:
        assert re.search(r" T %s$" % name, dev, flags=re.M), name
        assert not re.search(r"\b%s$" % name, prod, flags=re.M), name
        assert name in hal._lib.declared_dev_symbols() and name not in hal._lib.declared_symbols()
        assert re.search(r"\bint %s\(" % name, dev_header), name
    for name in EXACT + COMBINED:
        assert not re.search(r"\b%s$" % name, dev, flags=re.M), name


def test_both_new_kernels_passed_the_resource_gate(hal):
    import json
    res = json.load(open(os.path.join(ROOT, "halo-accumulation_amd", "csrc", "_obj", "kernel_resources.json")))
    gate = open(os.path.join(ROOT, "halo-accumulation_amd", "csrc", "check_resources.py")).read()
    for kernel in ("k_h_tables_mixed", "k_h_accumulate_mixed"):
        mine = [r for name, r in res.items() if kernel in name]
        assert len(mine) == 1 and mine[0]["ScratchSize [bytes/lane]"] == "0" and mine[0]["Dynamic Stack"] == "False", kernel
        assert '"%s"' % kernel in gate, "the gate fails if the kernel's remarks go missing"


# ------------------------------------------------------------------ whole-call errors that need no device
def test_null_context_and_null_pointers(hal):
    lib = hal.load()
    st = (C.c_int * 2)(77, 77)
    ds = (C.c_size_t * 2)(7, 7)
    ps = (C.c_void_p * 2)(None, None)
    for name in EXACT + COMBINED:
        args = (None,) if name in COMBINED else ()
        assert getattr(lib, name)(None, ds, ps, 0, *args, st) == hal._lib.HALO_E_ARG
        assert b"null context" in lib.halo_last_error()
        assert getattr(lib, name)(None, None, None, 2, *args, st) == hal._lib.HALO_E_ARG
    assert list(st) == [77, 77]
    assert lib.halo_dev_check_mixed_scalars(None, None, None, None, 1, None) == hal._lib.HALO_E_ARG


# ------------------------------------------------------------------ the Python wrappers
class FakeLib:
    """records what a wrapper passes: (ds, the words each pointer points at, m, seed)"""

    def __init__(self, rc=0, status=()):
        self.rc, self.status, self.calls = rc, status, []

    def _take(self, name, h, ds, ps, m, seed, st):
        words = [np.ctypeslib.as_array(C.cast(ps[i], C.POINTER(C.c_uint64)), shape=(23,)).copy() for i in range(m)]
        self.calls.append((name, [ds[i] for i in range(m)], words, m, seed))
        for i, s in enumerate(self.status):
            st[i] = s
        return self.rc

    def halo_pcdl_check_batch_mixed(self, h, ds, ps, m, st):
        return self._take("check", h, ds, ps, m, "none", st)

    def halo_pcdl_check_batch_mixed_combined(self, h, ds, ps, m, seed, st):
        return self._take("check_combined", h, ds, ps, m, seed, st)

    def halo_acc_decider_batch_mixed(self, h, ds, ps, m, st):
        return self._take("decider", h, ds, ps, m, "none", st)

    def halo_acc_decider_batch_mixed_combined(self, h, ds, ps, m, seed, st):
        return self._take("decider_combined", h, ds, ps, m, seed, st)

    def halo_last_error(self):
        return b"instance 1: told so"


class FakeCtx:
    def __init__(self, lib):
        self.lib, self.h = lib, None


def fake_blob(d, words, fill):
    b = np.full(words, fill, dtype=np.uint64)
    b[12] = d
    return b


def test_wrappers_pack_d_from_word_12_and_one_pointer_per_blob(hal):
    from halo_accumulation_amd import acc, pcdl
    blobs = [fake_blob(7, 40, 1), fake_blob(511, 300, 2)[::1], fake_blob(0, 30, 3).astype(np.int64), list(fake_blob(7, 40, 4))]
    seed = bytes(range(32))
    for fn, name, sd in ((pcdl.check_batch_mixed, "check", "none"), (acc.decider_batch_mixed, "decider", "none"),
                         (lambda c, b: pcdl.check_batch_mixed_combined(c, b, seed=seed), "check_combined", seed),
                         (lambda c, b: acc.decider_batch_mixed_combined(c, b), "decider_combined", None)):
        lib = FakeLib()
        assert fn(FakeCtx(lib), blobs) == [0, 0, 0, 0]
        (got_name, ds, words, m, got_seed), = lib.calls
        assert (got_name, ds, m, got_seed) == (name, [7, 511, 0, 7], 4, sd)
        assert [int(w[0]) for w in words] == [1, 2, 3, 4] and [int(w[12]) for w in words] == [7, 511, 0, 7]
    lib = FakeLib()
    assert pcdl.check_batch_mixed(FakeCtx(lib), []) == [] and lib.calls[0][3] == 0


def test_wrappers_raise_as_the_uniform_ones(hal):
    from halo_accumulation_amd import acc, pcdl
    blobs = [fake_blob(7, 40, 1), fake_blob(511, 300, 2)]
    R = hal._lib.HALO_E_REJECT
    with pytest.raises(hal._lib.HaloReject) as e:
        pcdl.check_batch_mixed_combined(FakeCtx(FakeLib(R, (0, R))), blobs)
    assert e.value.args == ("instance 1: told so", [0, R])
    with pytest.raises(Exception) as e:
        acc.decider_batch_mixed(FakeCtx(FakeLib(hal._lib.HALO_E_ARG)), blobs)
    assert not isinstance(e.value, hal._lib.HaloReject)
    with pytest.raises(ValueError):
        pcdl.check_batch_mixed_combined(FakeCtx(FakeLib()), blobs, seed=b"short")
    with pytest.raises(ValueError):
        acc.decider_batch_mixed_combined(FakeCtx(FakeLib()), blobs, seed=bytes(33))
    with pytest.raises(ValueError):
        pcdl.check_batch_mixed(FakeCtx(FakeLib()), [np.zeros(12, dtype=np.uint64)])  # (no word 12 to read d from)


# ------------------------------------------------------------------ the weight rule
def le64(v):
    return int(v).to_bytes(8, "little")


def weights_by_the_rule(blobs, ds, idx, seed, words_of):
    h = hashlib.sha3_256()
    h.update(DOMAIN)
    h.update(bytes(32) if seed is None else seed)
    h.update(le64(len(idx)))
    for i in idx:
        h.update(le64(i))
        h.update(le64(ds[i]))
        h.update(b"".join(le64(w) for w in blobs[i][:words_of(ds[i])]))
    D = h.digest()
    return [int.from_bytes(hashlib.sha3_256(D + le64(a)).digest(), "little") % R_MOD for a in range(len(idx))]


def from_mont(out):
    r_inv = pow(1 << 256, -1, R_MOD)
    return [sum(int(row[k]) << (64 * k) for k in range(4)) * r_inv % R_MOD for row in out]


def dev_weights(hal, blobs, ds, idx, seed):
    lib = hal.load()
    keep = [np.ascontiguousarray(b, dtype=np.uint64) for b in blobs]
    ps = (C.c_void_p * len(keep))(*[b.ctypes.data for b in keep])
    dd = (C.c_size_t * len(ds))(*ds)
    ix = (C.c_size_t * len(idx))(*idx)
    out = np.zeros((len(idx), 4), dtype=np.uint64)
    assert lib.halo_dev_check_mixed_weights(ps, dd, ix, len(idx), seed, ptr(out)) == 0, lib.halo_last_error()
    return from_mont(out)


def synthetic(hal, lgs, extra=0, salt=0):
    """one blob of random words per lg: an Instance plus `extra` words (an Accumulator's tail)"""
    words_of = lambda d: int(hal.load().halo_instance_words(int(d + 1).bit_length() - 1))
    rng = np.random.default_rng(4242 + salt)
    ds = [(1 << lg) - 1 for lg in lgs]
    return [rng.integers(0, 1 << 64, size=words_of(d) + extra, dtype=np.uint64) for d in ds], ds, words_of


@pytest.mark.parametrize("lgs", [[1, 3], [3, 9, 10, 3, 9, 10, 3], [14, 0, 3, 14, 9], [9] * 66])
def test_weights_equal_the_restated_rule(hal, lgs):
    blobs, ds, words_of = synthetic(hal, lgs, extra=24 if len(lgs) == 5 else 0)
    m = len(lgs)
    idx = [i for i in range(m) if i != 1 or m < 3]  # (the accepted members: one was rejected)
    seed = bytes(range(1, 33))
    want = weights_by_the_rule(blobs, ds, idx, seed, words_of)
    assert dev_weights(hal, blobs, ds, idx, seed) == want
    assert len(set(want)) == len(idx) and all(0 < w < R_MOD for w in want)
    null = dev_weights(hal, blobs, ds, idx, None)
    assert null == dev_weights(hal, blobs, ds, idx, bytes(32)) == weights_by_the_rule(blobs, ds, idx, None, words_of)
    assert all(a != b for a, b in zip(null, want))
    if len(lgs) == 5:  # words behind the Instance (an accumulator's tail) are not hashed
        tail = [b.copy() for b in blobs]
        for b, d in zip(tail, ds):
            b[words_of(d):] ^= np.uint64(1)
        assert dev_weights(hal, tail, ds, idx, seed) == want


def test_every_blob_bit_the_order_and_the_degree_bounds_reach_every_weight(hal):
    lgs = [3, 9, 3]
    blobs, ds, words_of = synthetic(hal, lgs, salt=7)
    idx = [0, 1, 2]
    base = dev_weights(hal, blobs, ds, idx, None)
    for member in idx:
        W = words_of(ds[member])
        for word, bit in ((0, 0), (W // 2, 17), (W - 1, 63)):
            changed = [b.copy() for b in blobs]
            changed[member][word] ^= np.uint64(1 << bit)
            got = dev_weights(hal, changed, ds, idx, None)
            assert got == weights_by_the_rule(changed, ds, idx, None, words_of)
            assert all(a != b for a, b in zip(got, base)), "member %d word %d" % (member, word)
    for perm in ([1, 0, 2], [0, 2, 1], [2, 0, 1]):
        got = dev_weights(hal, blobs, ds, perm, None)
        assert got == weights_by_the_rule(blobs, ds, perm, None, words_of)
        assert all(a != b for a, b in zip(got, base)), perm
    fewer = dev_weights(hal, blobs, ds, idx[:2], None)
    assert all(a != b for a, b in zip(fewer, base[:2])), "the member count is hashed"
    # LE64(d_i) is hashed: the same words read as two members of a smaller d give other weights
    longer = [np.concatenate([blobs[0], blobs[0]]), blobs[1], blobs[2]]
    as_d1 = dev_weights(hal, longer, [1, ds[1], ds[2]], idx, None)
    assert as_d1 == weights_by_the_rule(longer, [1, ds[1], ds[2]], idx, None, words_of) and all(a != b for a, b in zip(as_d1, base))


@pytest.mark.parametrize("lg", [3, 14])
def test_the_mixed_and_the_uniform_digests_differ_for_the_same_blobs(hal, lg):
    """a batch of ONE degree bound is a valid input of both calls: the domains keep their weights apart"""
    lib = hal.load()
    A = 4
    blobs, ds, words_of = synthetic(hal, [lg] * A, salt=lg)
    idx = list(range(A))
    seed = bytes(range(7, 39))
    mixed = dev_weights(hal, blobs, ds, idx, seed)
    flat = np.ascontiguousarray(np.stack(blobs))
    ix = (C.c_size_t * A)(*idx)
    out = np.zeros((A, 4), dtype=np.uint64)
    assert lib.halo_dev_check_weights(ptr(flat), flat.shape[1], ix, A, ds[0], seed, ptr(out)) == 0
    uniform = from_mont(out)
    h = hashlib.sha3_256(UNIFORM_DOMAIN + seed + le64(ds[0]) + le64(A))
    for i in idx:
        h.update(le64(i) + flat[i].tobytes())
    assert uniform == [int.from_bytes(hashlib.sha3_256(h.digest() + le64(a)).digest(), "little") % R_MOD for a in range(A)]
    assert all(a != b for a, b in zip(mixed, uniform)) and not set(mixed) & set(uniform)


def test_weight_argument_errors(hal):
    lib = hal.load()
    blobs, ds, _ = synthetic(hal, [3, 9])
    ps = (C.c_void_p * 2)(*[b.ctypes.data for b in blobs])
    dd = (C.c_size_t * 2)(*ds)
    ix = (C.c_size_t * 2)(0, 1)
    out = np.zeros((2, 4), dtype=np.uint64)
    E = hal._lib.HALO_E_ARG
    assert lib.halo_dev_check_mixed_weights(None, dd, ix, 2, None, ptr(out)) == E
    assert lib.halo_dev_check_mixed_weights(ps, None, ix, 2, None, ptr(out)) == E
    assert lib.halo_dev_check_mixed_weights(ps, dd, None, 2, None, ptr(out)) == E
    assert lib.halo_dev_check_mixed_weights(ps, dd, ix, 2, None, None) == E
    assert lib.halo_dev_check_mixed_weights((C.c_void_p * 2)(blobs[0].ctypes.data, None), dd, ix, 2, None, ptr(out)) == E
    assert lib.halo_dev_check_mixed_weights(ps, (C.c_size_t * 2)(7, 510), ix, 2, None, ptr(out)) == E
    assert lib.halo_dev_check_mixed_weights(ps, dd, ix, 0, None, None) == 0
