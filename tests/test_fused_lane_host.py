"""One lane of the fused check batch's term kernel (csrc/fused_lane.hpp fused_terms_lane -- what k_fused_terms runs once per
lane) and the field inversion under it (csrc/fr29.hpp fs_inv) compiled for the CPU under ASan + UBSan
(tests/native/fused_lane_host.cpp), every output word against Python integers.  tests/test_gpu_check_fused.py runs the same
members through the kernel."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import fused_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "halo-accumulation_amd", "csrc")
LGS = (1, 2, 9, 24)
M29 = (1 << 29) - 1


def limbs(x):
    return [(x >> (29 * i)) & M29 for i in range(8)] + [x >> 232]


def from_limbs(l):
    return sum(int(v) << (29 * i) for i, v in enumerate(l))


# the inversion's inputs as lazy values (nine limbs, below 60 r): 0, the N-forms of 1 and r - 1, multiples of r (zero again), the
# largest value the widest admitted bound holds, and random ones
def inversion_inputs():
    import random
    rng = random.Random(29)
    n_of = lambda x: x * (1 << 261) % fc.R_MOD
    xs = [0, n_of(1), n_of(fc.R_MOD - 1), 1, fc.R_MOD - 1, fc.R_MOD, 59 * fc.R_MOD, 60 * fc.R_MOD - 1, 2 * fc.R_MOD - 1]
    xs += [rng.randrange(60 * fc.R_MOD) for _ in range(12)]
    return xs


@pytest.fixture(scope="module")
def host_run(tmp_path_factory):
    if shutil.which("g++") is None or not os.path.isdir("/opt/rocm/include"):
        pytest.skip("no g++ / HIP headers")
    d = tmp_path_factory.mktemp("fused_lane_host")
    exe = os.path.join(str(d), "fused_lane_host")
    cmd = ["g++", "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
           "-I/opt/rocm/include", "-I", CSRC, os.path.join(ROOT, "tests", "native", "fused_lane_host.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "sanitize" in b.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr[-2000:]
    lanes = [m for lg in LGS for m in fc.members(lg, 40, seed=3)]
    invs = inversion_inputs()
    fin, fout = os.path.join(str(d), "cases.in"), os.path.join(str(d), "cases.out")
    with open(fin, "wb") as f:
        np.array([len(lanes), len(invs)], dtype=np.uint32).tofile(f)
        for m in lanes:
            np.array([m.lg], dtype=np.uint32).tofile(f)
            m.record().tofile(f)
        for x in invs:
            np.array(limbs(x), dtype=np.uint32).tofile(f)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr.strip(), "sanitizer or program error:\n" + r.stderr[-3000:]
    assert r.stdout.startswith("ok %d lanes %d inversions" % (len(lanes), len(invs)))
    raw = open(fout, "rb").read()
    return lanes, invs, raw


def test_the_kernel_runs_the_headers_lane():
    kernel = open(os.path.join(CSRC, "fused_check.hip")).read()
    assert '#include "fused_lane.hpp"' in kernel and kernel.count("fused_terms_lane(") == 1 and "void fused_terms_lane" not in kernel
    lane = open(os.path.join(CSRC, "fused_lane.hpp")).read()
    assert lane.count("fs_inv(") == 1, "ONE inversion per lane"
    fr = open(os.path.join(CSRC, "fr29.hpp")).read()
    body = fr[fr.index("HALO_DEV Fs<2> fs_inv("):]
    body = body[:body.index("\n}\n")]
    assert "while" not in body and "static_assert" in body and re.search(r"0x40000000u\};\s*// r - 2", body)
    words = [int(w.strip().rstrip("u"), 0) for w in re.search(r"E\[8\] = \{([^}]*)\}", body).group(1).split(",")]
    assert sum(w << (32 * i) for i, w in enumerate(words)) == fc.R_MOD - 2, "the chain's exponent is r - 2"


def test_every_lane_word_matches_python_and_is_sanitizer_clean(host_run):
    lanes, _, raw = host_run
    at, bad = 0, []
    for i, m in enumerate(lanes):
        K = 2 * m.lg + 2
        got = np.frombuffer(raw, dtype=np.uint64, count=K * 4 + 4, offset=at)
        at += (K * 4 + 4) * 8
        for what, k in fc.check_member(m, got[:K * 4].reshape(K, 4), got[K * 4:]):
            bad.append((i, m.lg, what, k))
    print("%d lanes at lg in %s" % (len(lanes), list(LGS)))
    assert not bad, "%d wrong words; first (lane, lg, what, index): %s" % (len(bad), bad[:8])
    assert len(lanes) == 40 * len(LGS)


def test_inversion_at_its_edges(host_run):
    """fs_inv(X) for a lazy X = N(x): below 2 r, and N(x^-1) exactly -- X * result = 2^522 mod r; a multiple of r gives 0"""
    lanes, invs, raw = host_run
    at = sum(((2 * m.lg + 2) * 4 + 4) * 8 for m in lanes)
    for x in invs:
        l = np.frombuffer(raw, dtype=np.uint32, count=9, offset=at)
        canon = np.frombuffer(raw, dtype=np.uint64, count=4, offset=at + 36)
        at += 36 + 32
        y = from_limbs(l)
        assert all(int(v) <= M29 for v in l[:8]) and y < 2 * fc.R_MOD, hex(x)
        want = pow(x, -1, fc.R_MOD) * pow(2, 522, fc.R_MOD) % fc.R_MOD if x % fc.R_MOD else 0
        assert y % fc.R_MOD == want and fc.from_words(canon) == want, hex(x)
    assert at == len(raw)
