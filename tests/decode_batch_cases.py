"""Shared by tests/test_decode_batch_cpu.py and tests/test_gpu_decode_batch.py: the malformed wire blobs, built afresh from good
ones, and the comparison of halo_*_decode_batch with a loop of the single decoders (status, lg, every word, the zero tails, the
return value and the message)."""
import ctypes as C

import numpy as np

import pallas_model as pm

KINDS = ("proof", "instance", "accumulator")
INSTANCE_HEAD = 33 + 8 + 32 + 32  # C, d, z, v in front of an Instance's proof


def _fns(lib, kind):
    return getattr(lib, "halo_%s_decode" % kind), getattr(lib, "halo_%s_decode_batch" % kind), getattr(lib, "halo_%s_words" % kind)


def off_curve_x():
    """the smallest x with x^3 + 5 a non-residue"""
    x = 1
    while pow((x ** 3 + 5) % pm.P, (pm.P - 1) // 2, pm.P) == 1:
        x += 1
    return x


def malformed_proofs(good, lg):
    """name -> bytes: one good EvalProof of lg >= 1 rounds (hiding) broken in one place each"""
    bad = {}
    bad["truncated"] = good[:-1]
    bad["trailing byte"] = good + b"\x00"
    bad["absurd vector length"] = b"\xff" * 8 + good[8:]
    b = bytearray(good); b[8 + 32] |= 0xC0; bad["both flag bits"] = bytes(b)
    b = bytearray(good); b[8 + 32] = (b[8 + 32] & 0x3F) | 0x40; bad["infinity flag with x != 0"] = bytes(b)
    b = bytearray(good); b[8:8 + 32] = pm.P.to_bytes(32, "little"); bad["x = p"] = bytes(b)
    b = bytearray(good); b[8:8 + 33] = off_curve_x().to_bytes(32, "little") + b"\x00"; bad["x off the curve"] = bytes(b)
    o = 8 + 33 * lg + 8 + 33 * lg + 33
    b = bytearray(good); b[o:o + 32] = pm.R_ORDER.to_bytes(32, "little"); bad["c = r"] = bytes(b)
    b = bytearray(good); b[o + 32] = 2; bad["option tag 2"] = bytes(b)
    b = bytearray(good); b[8 + 33 * lg] = lg - 1 if lg > 1 else 2; bad["|Rs| != |Ls|"] = bytes(b)
    return bad


def malformed_instances(good, lg):
    """the proof cases inside an Instance, and its own d + 1 != 2^lg"""
    bad = {name: good[:INSTANCE_HEAD] + data for name, data in malformed_proofs(good[INSTANCE_HEAD:], lg).items()}
    b = bytearray(good); b[33:41] = ((1 << lg) - 2).to_bytes(8, "little"); bad["d + 1 != 2^lg"] = bytes(b)
    b = bytearray(good); b[32] |= 0xC0; bad["both flag bits in C"] = bytes(b)
    return bad


def malformed_accumulators(good, lg, inst_len):
    """the Instance cases inside an Accumulator (its pi_V behind them untouched), and the cases of h.  good: an accumulator
    whose h has two coefficients; inst_len: the bytes of its Instance part"""
    tail = good[inst_len:]
    assert int.from_bytes(tail[:8], "little") == 2
    bad = {}
    for name, data in malformed_instances(good[:inst_len], lg).items():
        if name in ("truncated", "trailing byte"):
            continue  # (they move the boundary: made on the whole blob below)
        bad[name] = data + tail
    bad["truncated"] = good[:-1]
    bad["trailing byte"] = good + b"\x00"
    bad["h with 3 coefficients"] = good[:inst_len] + (3).to_bytes(8, "little") + tail[8:8 + 64] + tail[8:8 + 32] + tail[8 + 64:]
    bad["h with a zero leading coefficient"] = good[:inst_len] + tail[:8 + 32] + bytes(32) + tail[8 + 64:]
    b = bytearray(good); b[inst_len + 8 + 64 + 32] |= 0xC0; bad["both flag bits in U"] = bytes(b)
    b = bytearray(good); b[-32:] = pm.R_ORDER.to_bytes(32, "little"); bad["w = r"] = bytes(b)
    return bad


def single(lib, kind, data, stride):
    """(code, lg, the stride words the single decoder leaves in a zeroed buffer, message)"""
    fn, _, _ = _fns(lib, kind)
    out = np.zeros(max(stride, 1), dtype=np.uint64)
    lg = C.c_size_t(0)
    rc = fn(data, len(data), out.ctypes.data_as(C.POINTER(C.c_uint64)), stride, C.byref(lg))
    return rc, lg.value, out[:stride], lib.halo_last_error().decode() if rc else ""


def batch(lib, kind, datas, stride, ctx=None):
    """(return code, statuses, lgs, blobs (m, stride), message) of the raw entry point; untouched entries stay 77 / 0x77.."""
    _, fn, _ = _fns(lib, kind)
    m = len(datas)
    offs = (C.c_size_t * (m + 1))()
    for i, d in enumerate(datas):
        offs[i + 1] = offs[i] + len(d)
    out = np.full((max(m, 1), max(stride, 1)), 0x7777777777777777, dtype=np.uint64)
    lgs = (C.c_size_t * max(m, 1))(*([77] * max(m, 1)))
    st = (C.c_int * max(m, 1))(*([77] * max(m, 1)))
    rc = fn(ctx.h if ctx is not None else None, b"".join(datas), offs, m, out.ctypes.data_as(C.POINTER(C.c_uint64)), stride, lgs, st)
    return rc, [st[i] for i in range(m)], [lgs[i] for i in range(m)], out[:m, :stride], lib.halo_last_error().decode() if rc else ""


def expect_like_singles(lib, kind, datas, stride, ctx=None, singles=None):
    """the batch against the loop of single calls; returns the statuses"""
    _, _, words = _fns(lib, kind)
    singles = singles if singles is not None else [single(lib, kind, d, stride) for d in datas]
    rc, st, lgs, out, msg = batch(lib, kind, datas, stride, ctx)
    assert st == [s[0] for s in singles]
    for i, (s_rc, s_lg, s_out, _) in enumerate(singles):
        if s_rc:
            assert lgs[i] == 0 and not out[i].any(), "member %d failed: its slot is zero" % i
        else:
            w = words(s_lg)
            assert lgs[i] == s_lg and np.array_equal(out[i, :w], s_out[:w]), "member %d" % i
            assert not out[i, w:].any(), "member %d: the rest of its slot is zero" % i
    bad = [i for i, s in enumerate(singles) if s[0]]
    if bad:
        assert rc == singles[bad[0]][0] and msg == "member %d: %s" % (bad[0], singles[bad[0]][3])
    else:
        assert rc == 0
    return st
