"""The device code of point decompression (csrc/decompress.hpp) compiled for the CPU under ASan + UBSan
(tests/native/decompress_host.cpp) and fed the library's own torsion tables: every record it writes is what the host decoder
writes for the same 33 bytes -- good points of both signs, infinity, and every way a point can be malformed -- and its square
root holds against Python integers over every 2-adic order.  The tables themselves are checked against their definition."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import decode_batch_cases as dc
import pallas_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = pm.P
T = (P - 1) >> 32
MASK = (1 << 64) - 1
TAB_WORDS = 4 * 256 * 8 + 256


@pytest.fixture(scope="module")
def hal():
    import halo_accumulation_amd as h
    h.build()
    return h


@pytest.fixture(scope="module")
def tables(hal):
    tab = np.zeros(TAB_WORDS, dtype=np.uint32)
    assert hal.load().halo_dev_sqrt_tables(tab.ctypes.data_as(C.POINTER(C.c_uint32)), TAB_WORDS) == 0
    assert hal.load().halo_dev_sqrt_tables(tab.ctypes.data_as(C.POINTER(C.c_uint32)), TAB_WORDS - 1) == hal._lib.HALO_E_ARG
    return tab


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    assert shutil.which("g++") and os.path.isdir("/opt/rocm/include"), "g++ and the HIP headers are part of the build image"
    out = os.path.join(str(tmp_path_factory.mktemp("decompress_host")), "decompress_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", os.path.join(ROOT, "halo-accumulation_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "decompress_host.cpp"), "-o", out]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    b = subprocess.run(cmd + san, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "sanitize" in b.stderr:  # no sanitizer runtime: the plain build still checks the results
        b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    return out


def run(exe, tmp_path, mode, tables, words_in, ow):
    ft, fi, fo = (os.path.join(str(tmp_path), n) for n in ("tables.bin", "in.bin", "out.bin"))
    tables.tofile(ft)
    np.ascontiguousarray(words_in, dtype=np.uint64).tofile(fi)
    r = subprocess.run([exe, str(mode), ft, fi, fo], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    return np.fromfile(fo, dtype=np.uint64).reshape(-1, ow)


def mont_words(v):
    v = v * pm.MONT_R % P
    return [(v >> (64 * k)) & MASK for k in range(4)]


def test_tables_are_what_the_kernel_expects(tables):
    g = pow(5, T, P)
    assert pow(g, 1 << 31, P) == P - 1, "g generates the 2^32-torsion"
    ginv = pow(g, -1, P)
    for i in range(4):
        for d in (0, 1, 2, 3, 128, 254, 255):
            e = d >> 1 if i == 0 else d << (8 * i - 1)
            want = mont_words(pow(ginv, e, P))
            got = tables[8 * (256 * i + d): 8 * (256 * i + d) + 8].view(np.uint64).tolist()
            assert got == want, (i, d)
    h = pow(g, 1 << 24, P)
    keys = [mont_words(pow(h, d, P))[0] & 0xFFFFFFFF for d in range(256)]
    assert tables[4 * 256 * 8:].tolist() == keys and len(set(keys)) == 256, "one limb tells the 256 powers apart"


def test_square_root_against_python_integers(exe, tables, tmp_path):
    rnd = np.random.default_rng(7)
    draw = lambda: int.from_bytes(rnd.bytes(40), "little") % P
    elems = [0, 1, P - 1, 5, 4]
    for k in range(33):
        found = 0
        while found < 2:
            a = pow(draw(), 1 << (32 - k), P)
            b = pow(a, T, P)
            if pow(b, 1 << k, P) == 1 and (k == 0 or pow(b, 1 << (k - 1), P) != 1):
                elems.append(a); found += 1
    elems += [draw() for _ in range(200)]
    out = run(exe, tmp_path, 1, tables, np.array([mont_words(e) for e in elems], dtype=np.uint64), 6)
    r_inv = pow(pm.MONT_R, -1, P)
    n_ok = 0
    for i, e in enumerate(elems):
        if out[i, 4]:
            r = sum(int(out[i, w]) << (64 * w) for w in range(4))
            assert r < P and (r * r_inv) ** 2 % P == e, i
            n_ok += 1
        else:
            assert out[i, 4] == 0 and pow(e, (P - 1) // 2, P) == P - 1, i
    assert not out[5 + 64: 5 + 66, 4].any(), "order 2^32: the non-residues"
    assert 60 < n_ok - 69 < 140


def test_records_match_the_host_decoder(hal, exe, tables, tmp_path):
    """every point as the one point of an lg = 0 proof through halo_proof_decode: U's 12 words, or a rejection"""
    lib = hal.load()
    rnd = np.random.default_rng(11)
    pts = []
    x = 0
    while len(pts) < 120:  # consecutive x: about half are on the curve; both signs of each
        x += 1
        pts += [x.to_bytes(32, "little") + bytes([f]) for f in (0x00, 0x80)]
    for _ in range(60):
        pts.append((int.from_bytes(rnd.bytes(40), "little") % P).to_bytes(32, "little") + bytes([int(rnd.integers(0, 2)) * 0x80]))
    pts += [bytes(32) + b"\x40", bytes(32) + b"\xc0", bytes(32) + b"\x00", bytes(32) + b"\x80", b"\x01" + bytes(31) + b"\x40",
            bytes(32) + b"\x41", (P - 1).to_bytes(32, "little") + b"\x00", (P - 1).to_bytes(32, "little") + b"\x80",
            P.to_bytes(32, "little") + b"\x00", (P + 1).to_bytes(32, "little") + b"\x80", b"\xff" * 32 + b"\x00", b"\xff" * 32 + b"\x3f",
            (P - 1).to_bytes(32, "little") + b"\x01", (P - 1).to_bytes(32, "little") + b"\x20", dc.off_curve_x().to_bytes(32, "little") + b"\x80",
            (P - 1).to_bytes(32, "little") + b"\xc0"]
    recs = np.zeros((len(pts), 6), dtype=np.uint64)
    for i, b in enumerate(pts):
        recs[i, :5] = np.frombuffer(b + bytes(7), dtype=np.uint64)
    out = run(exe, tmp_path, 0, tables, recs, 14)
    stride = lib.halo_proof_words(0)
    accepted = 0
    for i, b in enumerate(pts):
        data = (0).to_bytes(8, "little") * 2 + b + (7).to_bytes(32, "little") + b"\x00\x00"
        rc, _, words, _ = dc.single(lib, "proof", data, stride)
        assert out[i, 12] in (0, 1) and out[i, 13] == 0
        assert (rc == 0) == (out[i, 12] == 1), "point %d: %s" % (i, b.hex())
        if rc == 0:
            assert out[i, :12].tolist() == words[2:14].tolist(), "point %d: %s" % (i, b.hex())
            accepted += 1
    assert 70 < accepted < 130
