"""Cases and checkers for the lanes of the device transcripts (csrc/keccak_lane.hpp, csrc/transcript_lane.hpp), shared by
tests/test_transcript_host.py (the lanes compiled for the CPU under ASan + UBSan: tests/native/transcript_lane_host.cpp) and
tests/test_gpu_transcripts.py (raw word helpers for planted members).  The reference is hashlib.sha3_256 and the integer model
(oracle/pallas_model.py: rho_0, ser_point, ser_scalar), exactly: every result is an integer, so there is no tolerance."""
import hashlib
import os
import random
import shutil
import subprocess

import numpy as np

import pallas_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, R = pm.P, pm.R_ORDER
M64 = (1 << 64) - 1
VALID, INVALID, FOREIGN = 0, 1, 2  # transcript_lane.hpp TR_*


def words(v):
    return [(v >> (64 * i)) & M64 for i in range(4)]


def fq_mont(x):
    return pm.to_mont_limbs(x % P, P)


def fr_mont(x):
    return pm.to_mont_limbs(x % R, R)


def jac_words(pt, z=1):
    """arkworks Jacobian words of the affine point pt (None: infinity as the library writes it) scaled to Z = z"""
    if pt is None:
        return fq_mont(1) + fq_mont(1) + [0] * 4
    x, y = pt
    return fq_mont(x * z * z) + fq_mont(y * z * z * z) + fq_mont(z)


def sqrt_fq(a):
    """a square root of a in Fq, or None (Tonelli-Shanks: p - 1 = 2^32 t)"""
    a %= P
    if a == 0:
        return 0
    if pow(a, (P - 1) // 2, P) != 1:
        return None
    s, t = 32, (P - 1) >> 32
    z = 2
    while pow(z, (P - 1) // 2, P) != P - 1:  # the first non-residue
        z += 1
    c, x, b, m = pow(z, t, P), pow(a, (t + 1) // 2, P), pow(a, t, P), s
    while b != 1:
        i, b2 = 0, b
        while b2 != 1:
            b2 = b2 * b2 % P
            i += 1
        g = pow(c, 1 << (m - i - 1), P)
        x, c = x * g % P, g * g % P
        b, m = b * c % P, i
    return x


def point_with_top_word_max():
    """a curve point whose x has the largest top 64-bit word a value below p can have (2^62: x >= 2^254)"""
    x = 1 << 254
    while True:
        y = sqrt_fq(x * x * x + 5)
        if y is not None and y != 0:
            assert x < P and (x >> 192) == (P >> 192)
            return (x, y)
        x += 1


def points():
    """named affine points: P and -P of a few multiples of the generator (both sign flags), infinity, the top-word point"""
    out = {"inf": None}
    for k in (1, 2, 0x1234567, R - 5):
        pt = pm.mul(pm.GENERATOR, k)
        out["%dG" % k if k < 10 else "%xG" % k] = pt
        out["-" + ("%dG" % k if k < 10 else "%xG" % k)] = pm.neg(pt)
    top = point_with_top_word_max()
    out["top"], out["-top"] = top, pm.neg(top)
    return out


def flag_of(pt):
    return pm.ser_point(pt)[32]


def compressed(pt):
    """the 5 words point_compress_lane writes for a valid point"""
    b = pm.ser_point(pt)
    return words(int.from_bytes(b[:32], "little")) + [b[32]]


# ------------------------------------------------------------------ the permutation
def perm_cases(count=24, seed=0x6b656363):
    """(state words, message): one padded SHA3-256 block of a message of 0 .. 135 bytes (every lane count, the pad bytes meeting
    in one byte at 135)"""
    rng = random.Random(seed)
    lens = [0, 1, 7, 8, 9, 101, 102, 134, 135] + [rng.randrange(136) for _ in range(count - 9)]
    out = []
    for n in lens:
        msg = bytes(rng.randrange(256) for _ in range(n))
        block = bytearray(msg + bytes(136 - n))
        block[n] ^= 0x06
        block[135] ^= 0x80
        state = [int.from_bytes(block[8 * i:8 * i + 8], "little") for i in range(17)] + [0] * 8
        out.append((state, msg))
    return out


def check_perm(state_out, msg):
    """-> None, or what is wrong"""
    got = b"".join(int(w).to_bytes(8, "little") for w in state_out[:4])
    return None if got == hashlib.sha3_256(msg).digest() else "digest differs"


# ------------------------------------------------------------------ rho_0
class Hash:
    """form 0: rho_0(P0, s0, s1); 1: rho_0(P0, s0, s1, P1); 2: rho_0(s0, P0, P1)"""

    def __init__(self, name, form, p0, p1, s0, s1):
        self.name, self.form, self.p0, self.p1, self.s0, self.s1 = name, form, p0, p1, s0 % R, s1 % R
        items = {0: [("p", p0), ("s", s0), ("s", s1)], 1: [("p", p0), ("s", s0), ("s", s1), ("p", p1)], 2: [("s", s0), ("p", p0), ("p", p1)]}[form]
        data = b"".join(pm._ser_item(it) for it in items) + (0).to_bytes(4, "little")
        assert len(data) == (101, 134, 102)[form] and len(data) < 136
        self.digest = int.from_bytes(hashlib.sha3_256(data).digest(), "little")
        self.subs = self.digest // R  # subtractions of r that bring the digest below r
        self.want = pm.rho_0(*items)
        assert self.want == self.digest - self.subs * R and 0 <= self.subs <= 3

    def record(self):
        return [self.form] + jac_words(self.p0) + jac_words(self.p1) + fr_mont(self.s0) + fr_mont(self.s1)


def hash_cases():
    pts = points()
    g, ng = pts["1G"], pts["-1G"]
    out = []
    edge = [0, 1, R - 1]
    for form in (0, 1, 2):
        for a in edge:
            for b in edge:
                out.append(Hash("form%d s0=%s s1=%s" % (form, a, b), form, g, ng, a, b))
        for name, pt in pts.items():  # every point in each position, infinity among them
            out.append(Hash("form%d P0=%s" % (form, name), form, pt, g, 0x1111 + form, 0x2222))
            out.append(Hash("form%d P1=%s" % (form, name), form, ng, pt, 0x3333 + form, 0x4444))
        out.append(Hash("form%d both infinite" % form, form, None, None, 5, 6))
        # digests that need 0, 1, 2 and 3 subtractions of r: seeds searched until each class is hit
        seen, seed = set(), 0
        while len(seen) < 4:
            h = Hash("form%d seed %d" % (form, seed), form, g, pts["2G"], 0xABCDEF0000 + seed, 0x77 + form)
            if h.subs not in seen:
                seen.add(h.subs)
                h.name += " (%d subtractions)" % h.subs
                out.append(h)
            seed += 1
            assert seed < 10000
    return out


def check_hash(h, got):
    """got: the 14 result words of a hash record -> None, or what is wrong"""
    got = [int(w) for w in got]
    if got[:4] != fr_mont(h.want):
        return "challenge differs"
    if got[4:9] != compressed(h.p0):
        return "first point's encoding differs"
    if got[9:14] != compressed(h.p1):
        return "second point's encoding differs"
    return None


# ------------------------------------------------------------------ verdicts
def point_cases():
    """(name, 12 Jacobian words, verdict, compressed words or None)"""
    pts = points()
    out = []
    for name, pt in pts.items():
        out.append((name, jac_words(pt), VALID, compressed(pt)))
    x, y = pts["2G"]
    out.append(("(x, y + 1)", fq_mont(x) + fq_mont(y + 1) + fq_mont(1), INVALID, None))
    out.append(("(x + 1, y)", fq_mont(x + 1) + fq_mont(y) + fq_mont(1), INVALID, None))
    out.append(("x = p", words(P) + fq_mont(y) + fq_mont(1), INVALID, None))
    out.append(("x = 2^256 - 1", words((1 << 256) - 1) + fq_mont(y) + fq_mont(1), INVALID, None))
    out.append(("y = p", fq_mont(x) + words(P) + fq_mont(1), INVALID, None))
    out.append(("Z = p", fq_mont(x) + fq_mont(y) + words(P), INVALID, None))
    out.append(("Z = 0, X = p", words(P) + fq_mont(y) + [0] * 4, INVALID, None))
    out.append(("Z = 2", jac_words(pts["2G"], 2), FOREIGN, None))
    out.append(("Z = 2 off the curve", fq_mont(x) + fq_mont(y) + fq_mont(2), FOREIGN, None))
    out.append(("Z = plain 1", fq_mont(x) + fq_mont(y) + [1, 0, 0, 0], FOREIGN, None))
    out.append(("Z = 0, X, Y arbitrary", fq_mont(123) + fq_mont(456) + [0] * 4, VALID, compressed(None)))
    out.append(("Z = 0, X = Y = 0", [0] * 12, VALID, compressed(None)))
    return out


def check_point(case, got):
    name, _, verdict, comp = case
    got = [int(w) for w in got]
    if got[5] != verdict or (got[4] >> 8) != verdict:
        return "verdict %d, expected %d" % (got[5], verdict)
    want = comp if comp is not None else [0] * 5
    if got[:4] != want[:4] or (got[4] & 0xFF) != want[4]:
        return "encoding differs"
    return None


def scalar_cases():
    """(name, 4 words, scalar_ok)"""
    return [("0", words(0), 1), ("1", words(1), 1), ("r - 1", words(R - 1), 1), ("r", words(R), 0), ("r + 1", words(R + 1), 0),
            ("2^256 - 1", words((1 << 256) - 1), 0), ("2^255", words(1 << 255), 0), ("r with a smaller low word", words(R - (1 << 32)), 1)]


# ------------------------------------------------------------------ the CPU build of the lanes
def build_host(tmp_dir, csrc=None):
    """compile tests/native/transcript_lane_host.cpp with ASan + UBSan against the headers of csrc -> (exe, None) or (None, why)"""
    if shutil.which("g++") is None or not os.path.isdir("/opt/rocm/include"):
        return None, "no g++ / HIP headers"
    exe = os.path.join(str(tmp_dir), "transcript_lane_host")
    cmd = ["g++", "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
           "-I/opt/rocm/include", "-I", csrc or os.path.join(ROOT, "halo-accumulation_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "transcript_lane_host.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "sanitize" in b.stderr:
        return None, "sanitizer runtime not installed"
    assert b.returncode == 0, b.stderr[-2000:]
    return exe, None


def run_host(exe, tmp_dir, perms, hashes, pts, scs):
    """-> (25-word states, 14-word hash results, 6-word point results, ok words); any sanitizer report fails"""
    fin, fout = os.path.join(str(tmp_dir), "tr.in"), os.path.join(str(tmp_dir), "tr.out")
    with open(fin, "wb") as f:
        np.array([len(perms), len(hashes), len(pts), len(scs)], dtype=np.uint32).tofile(f)
        flat = [w for st, _ in perms for w in st] + [w for h in hashes for w in h.record()] + [w for c in pts for w in c[1]] + [w for c in scs for w in c[1]]
        np.array(flat, dtype=np.uint64).tofile(f)
    p = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and p.stdout.startswith("ok ") and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stdout + p.stderr[-3000:]
    flat = np.fromfile(fout, dtype=np.uint64)
    a, b, c = 25 * len(perms), 14 * len(hashes), 6 * len(pts)
    assert len(flat) == a + b + c + len(scs)
    return flat[:a].reshape(-1, 25), flat[a:a + b].reshape(-1, 14), flat[a + b:a + b + c].reshape(-1, 6), flat[a + b + c:]
