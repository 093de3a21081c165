"""halo_proof_decode_batch / halo_instance_decode_batch / halo_accumulator_decode_batch without a GPU (ctx = NULL: the host
pool): exported, declared and bound; every member's status, lg and words those of the single decoder, slot tails zero;
malformed members between good ones; the reading order at a short stride; whole-call errors."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import decode_batch_cases as dc
import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["halo_proof_decode_batch", "halo_instance_decode_batch", "halo_accumulator_decode_batch"]


@pytest.fixture(scope="module")
def hal():
    import halo_accumulation_amd as h
    h.build()
    return h


@pytest.fixture(scope="module")
def lib(hal):
    return hal.load()


@pytest.fixture(scope="module")
def pp(urs4096):
    return orc.make_pp(urs4096)


@pytest.fixture(scope="module")
def proofs(hal, pp):
    """{(lg, hiding): bytes}"""
    out = {}
    for lg in (3, 6):
        for hiding in (True, False):
            n = 1 << lg
            coeffs, s = orc.rng_scalars(4000 + 2 * n + hiding, n)
            zw, _ = orc.rng_scalars(s, 2)
            w = zw[1] if hiding else None
            Cm = orc.pcdl_commit(pp, coeffs, n - 1, w)
            pf, _ = orc.pcdl_open(pp, 9, coeffs, Cm, n - 1, zw[0], w)
            out[(lg, hiding)] = hal._lib.proof_encode(pf)
    return out


@pytest.fixture(scope="module")
def chain(hal, pp):
    """[(lg, instance bytes, accumulator bytes, accumulator words)] from the oracle, lg 3 .. 6"""
    out = []
    seed = 0xDEC0DE
    for lg in (3, 4, 5, 6):
        d = (1 << lg) - 1
        q, seed = orc.random_instance(pp, seed, d)
        acc, seed = orc.acc_prover(pp, seed, d, [q])
        out.append((lg, hal._lib.instance_encode(q), hal._lib.accumulator_encode(acc), acc))
    return out


def test_exported_declared_and_bound(hal):
    exported = subprocess.check_output(["nm", "-D", "--defined-only", hal._lib.LIB_PATH], text=True)
    header = " ".join(open(os.path.join(ROOT, "include", "halo_accumulation.h")).read().split())
    ffi = " ".join(open(os.path.join(ROOT, "integration", "ffi.rs")).read().split())
    for name in NAMES:
        assert re.search(r" T %s$" % name, exported, flags=re.M)
        assert ("int %s(halo_ctx *ctx /*nullable*/, const uint8_t *in, const size_t *offs, size_t m, uint64_t *out, "
                "size_t stride_words, size_t *lg_out /*nullable*/, int *status /*nullable*/);" % name) in header
        assert ("pub fn %s(ctx: *mut HaloCtx, input: *const u8, offs: *const usize, m: usize, out: *mut u64, stride_words: usize, "
                "lg_out: *mut usize, status: *mut c_int) -> c_int;" % name) in ffi
        assert name in hal._lib.declared_symbols()
    for fn in ("proof_decode_batch", "instance_decode_batch", "accumulator_decode_batch"):
        assert callable(getattr(hal._lib, fn))
    dev = subprocess.check_output(["nm", "-D", "--defined-only", hal._lib.DEV_LIB_PATH], text=True)
    assert re.search(r" T halo_dev_fq_sqrt$", dev, flags=re.M)
    dev_header = " ".join(open(os.path.join(ROOT, "include", "halo_accumulation_dev.h")).read().split())
    assert "int halo_dev_fq_sqrt(halo_ctx *ctx, const uint64_t *a, size_t m, uint64_t *root_out, uint32_t *ok_out);" in dev_header
    assert "halo_dev_fq_sqrt" in hal._lib.declared_dev_symbols()
    assert hal.load().halo_dev_fq_sqrt(None, None, 1, None, None) == hal._lib.HALO_E_ARG
    hal._lib.dev_hook("decode_batch_min", 16)
    hal._lib.dev_hook("decode_batch_min", 0)
    assert "decompress.hip" in open(os.path.join(ROOT, "halo-accumulation_amd", "csrc", "Makefile")).read()


def test_matches_the_loop_of_single_calls(hal, lib, proofs, chain):
    datas = [proofs[k] for k in sorted(proofs)]
    for stride in (lib.halo_proof_words(6), lib.halo_proof_words(6) + 37, lib.halo_proof_words(40)):
        assert dc.expect_like_singles(lib, "proof", datas, stride) == [0] * len(datas)
    insts, accs = [c[1] for c in chain], [c[2] for c in chain]
    for stride in (lib.halo_instance_words(6), lib.halo_instance_words(9) + 5):
        assert dc.expect_like_singles(lib, "instance", insts, stride) == [0] * len(insts)
    for stride in (lib.halo_accumulator_words(6), lib.halo_accumulator_words(8) + 1):
        assert dc.expect_like_singles(lib, "accumulator", accs, stride) == [0] * len(accs)
    # an accumulator is an instance followed by pi_V: as an instance it has trailing bytes, and an instance lacks pi_V
    assert dc.expect_like_singles(lib, "instance", [insts[0], accs[0]], lib.halo_instance_words(6)) == [0, hal._lib.HALO_E_REJECT]
    assert dc.expect_like_singles(lib, "accumulator", [insts[0], accs[0]], lib.halo_accumulator_words(6)) == [hal._lib.HALO_E_REJECT, 0]
    # the Python wrappers
    blobs, lgs, st = hal._lib.accumulator_decode_batch(accs)
    assert st.tolist() == [0] * 4 and lgs.tolist() == [c[0] for c in chain]
    for i, c in enumerate(chain):
        assert blobs[i, : len(c[3])].tolist() == c[3].tolist() and not blobs[i, len(c[3]):].any()
    blobs, lgs, st = hal._lib.proof_decode_batch(datas + [datas[0][:-1]], stride_words=lib.halo_proof_words(7))
    assert st.tolist() == [0] * len(datas) + [hal._lib.HALO_E_REJECT] and blobs.shape == (len(datas) + 1, lib.halo_proof_words(7))
    assert hal._lib.instance_decode_batch([])[0].shape[0] == 0


def test_accumulator_h_of_0_1_2_coefficients(hal, lib, chain):
    lg, _, _, acc = chain[1]
    iw = lib.halo_instance_words(lg)
    datas = []
    for keep in (0, 1, 2):
        a = acc.copy()
        a[iw + 4 * keep: iw + 8] = 0
        datas.append(hal._lib.accumulator_encode(a))
        assert int.from_bytes(datas[-1][-(8 + 32 * keep + 33 + 32):][:8], "little") == keep
    assert len(set(len(d) for d in datas)) == 3
    assert dc.expect_like_singles(lib, "accumulator", datas, lib.halo_accumulator_words(lg) + 3) == [0, 0, 0]


def test_malformed_members_between_good_ones(hal, lib, proofs, chain):
    REJECT = hal._lib.HALO_E_REJECT
    # proofs
    good = proofs[(3, True)]
    bad = dc.malformed_proofs(good, 3)
    assert len(bad) == 10
    datas = [good]
    for name in bad:
        datas += [bad[name], proofs[(6, False)]]
    st = dc.expect_like_singles(lib, "proof", datas, lib.halo_proof_words(6))
    assert st == [0] + [REJECT, 0] * len(bad)
    for first in ("x off the curve", "c = r", "truncated"):  # the first failure names the call's message
        assert dc.expect_like_singles(lib, "proof", [good, good, bad[first], bad["option tag 2"]], lib.halo_proof_words(3))[2:] == [REJECT, REJECT]
    # instances
    lg, inst, accb, _ = chain[2]
    bad = dc.malformed_instances(inst, lg)
    assert "d + 1 != 2^lg" in bad and len(bad) == 12
    datas = [inst]
    for name in bad:
        datas += [bad[name], chain[0][1]]
    assert dc.expect_like_singles(lib, "instance", datas, lib.halo_instance_words(lg)) == [0] + [REJECT, 0] * len(bad)
    # accumulators
    bad = dc.malformed_accumulators(accb, lg, lib.halo_instance_encoded_size(lg, 1))
    assert {"h with 3 coefficients", "h with a zero leading coefficient", "d + 1 != 2^lg", "x off the curve"} <= set(bad)
    datas = [accb]
    for name in bad:
        datas += [bad[name], chain[3][2]]
    st = dc.expect_like_singles(lib, "accumulator", datas, lib.halo_accumulator_words(6))
    assert st == [0] + [REJECT, 0] * len(bad)
    # the distinct messages of the accumulator decoder come through
    for name, text in (("h with 3 coefficients", "at most two coefficients"), ("h with a zero leading coefficient", "leading coefficient of h is zero")):
        rc, _, _, _, msg = dc.batch(lib, "accumulator", [accb, bad[name]], lib.halo_accumulator_words(lg))
        assert rc == REJECT and msg.startswith("member 1: decode: malformed Accumulator") and text in msg
    # a bad point in front of a bad h: the point is what the single call meets first
    both = bytearray(bad["h with 3 coefficients"]); both[32] |= 0xC0
    rc, _, _, _, msg = dc.batch(lib, "accumulator", [bytes(both)], lib.halo_accumulator_words(lg))
    assert (rc, msg) == (REJECT, "member 0: decode: malformed Accumulator")
    dc.expect_like_singles(lib, "accumulator", [bytes(both), accb], lib.halo_accumulator_words(lg))


def test_stride_cases(hal, lib, proofs, chain):
    ARG, REJECT = hal._lib.HALO_E_ARG, hal._lib.HALO_E_REJECT
    lg, inst, accb, _ = chain[1]
    off = bytearray(accb); off[:33] = dc.off_curve_x().to_bytes(32, "little") + b"\x00"  # C of the Instance part is no point
    for stride in (lib.halo_instance_words(lg), lib.halo_instance_words(lg) + 11, lib.halo_accumulator_words(lg) - 1):
        st = dc.expect_like_singles(lib, "accumulator", [accb, bytes(off), accb], stride)
        assert st == [ARG, REJECT, ARG], "the Instance part is read, and judged, before the room for pi_V"
        rc, _, _, _, msg = dc.batch(lib, "accumulator", [accb], stride)
        assert (rc, msg) == (ARG, "member 0: decode: output buffer too small")
    assert dc.expect_like_singles(lib, "accumulator", [accb, bytes(off)], lib.halo_accumulator_words(lg)) == [0, REJECT]
    # a member whose lg does not fit the stride
    datas = [proofs[(3, True)], proofs[(6, True)], proofs[(3, False)]]
    assert dc.expect_like_singles(lib, "proof", datas, lib.halo_proof_words(3)) == [0, REJECT, 0]
    assert dc.expect_like_singles(lib, "proof", datas, lib.halo_proof_words(5)) == [0, REJECT, 0]
    assert dc.expect_like_singles(lib, "instance", [chain[0][1], chain[3][1]], lib.halo_instance_words(3)) == [0, REJECT]
    assert dc.expect_like_singles(lib, "instance", [chain[0][1]], 20) == [REJECT]
    assert dc.expect_like_singles(lib, "proof", [proofs[(3, True)]], 0) == [REJECT]


def test_whole_call_errors(hal, lib, proofs):
    ARG = hal._lib.HALO_E_ARG
    data = proofs[(3, True)]
    stride = lib.halo_proof_words(3)
    u64p = C.POINTER(C.c_uint64)
    for name in NAMES:
        fn = getattr(lib, name)
        out = np.full(2 * stride, 0x77, dtype=np.uint64)
        st = (C.c_int * 2)(77, 77)
        lgs = (C.c_size_t * 2)(77, 77)
        offs = (C.c_size_t * 3)(0, len(data), 2 * len(data))
        down = (C.c_size_t * 3)(0, len(data), len(data) - 1)
        p = out.ctypes.data_as(u64p)
        assert fn(None, None, offs, 2, p, stride, lgs, st) == ARG and b"null pointer" in lib.halo_last_error()
        assert fn(None, data + data, None, 2, p, stride, lgs, st) == ARG
        assert fn(None, data + data, offs, 2, None, stride, lgs, st) == ARG
        assert fn(None, data + data, down, 2, p, stride, lgs, st) == ARG and b"decrease" in lib.halo_last_error()
        assert list(st) == [77, 77] and list(lgs) == [77, 77] and (out == 0x77).all(), "whole-call errors touch nothing"
        assert fn(None, None, None, 0, None, 0, None, None) == 0
        assert fn(None, data + data, offs, 0, p, stride, lgs, st) == 0
        assert list(st) == [77, 77] and (out == 0x77).all(), "m = 0 touches nothing"
    # status and lg_out are nullable; an empty member is a truncated one
    out = np.zeros(2 * stride, dtype=np.uint64)
    offs = (C.c_size_t * 3)(0, len(data), len(data))
    assert lib.halo_proof_decode_batch(None, data, offs, 2, out.ctypes.data_as(u64p), stride, None, None) == hal._lib.HALO_E_REJECT
    assert lib.halo_last_error() == b"member 1: decode: malformed EvalProof"
    assert out[:stride].tolist() == dc.single(lib, "proof", data, stride)[2].tolist() and not out[stride:].any()
