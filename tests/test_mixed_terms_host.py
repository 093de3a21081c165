"""The per-member function of the mixed fused check batch's term kernel (csrc/mixed_terms_lane.hpp mixed_terms_member -- what
k_mixed_terms runs once per lane: the descriptor walk, then fused_lane.hpp's lane on the member's own record) compiled for the CPU
under ASan + UBSan (tests/native/mixed_terms_host.cpp) over dense ragged records in heap blocks of exactly the needed size, every
output word against Python integers.  tests/test_gpu_check_mixed_fused.py runs such members through the kernel."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import fused_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "halo-accumulation_amd", "csrc")
LG_SETS = ([1, 24], [24, 1, 9, 2], [(1, 2, 9, 24)[a % 4] for a in range(40)])


def members_of(lgs, seed):
    """member a of a set: the a-th of fused_cases.members at its lg (the special values lie among the first 40 of each size)"""
    pools = {lg: fc.members(lg, 40, seed=seed) for lg in set(lgs)}
    return [pools[lg][a] for a, lg in enumerate(lgs)]


@pytest.fixture(scope="module")
def host_run(tmp_path_factory):
    if shutil.which("g++") is None or not os.path.isdir("/opt/rocm/include"):
        pytest.skip("no g++ / HIP headers")
    d = tmp_path_factory.mktemp("mixed_terms_host")
    exe = os.path.join(str(d), "mixed_terms_host")
    cmd = ["g++", "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
           "-I/opt/rocm/include", "-I", CSRC, os.path.join(ROOT, "tests", "native", "mixed_terms_host.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "sanitize" in b.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr[-2000:]
    sets = [members_of(lgs, seed=5 + k) for k, lgs in enumerate(LG_SETS)]
    fin, fout = os.path.join(str(d), "cases.in"), os.path.join(str(d), "cases.out")
    with open(fin, "wb") as f:
        np.array([len(sets)], dtype=np.uint32).tofile(f)
        for mem in sets:
            np.array([len(mem)] + [m.lg for m in mem], dtype=np.uint32).tofile(f)
            for m in mem:
                m.record().tofile(f)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr.strip(), "sanitizer or program error:\n" + r.stderr[-3000:]
    assert r.stdout.startswith("ok %d sets %d members" % (len(sets), sum(len(mem) for mem in sets)))
    return sets, open(fout, "rb").read()


def test_every_word_of_every_ragged_set_matches_python_and_is_sanitizer_clean(host_run):
    sets, raw = host_run
    assert [[m.lg for m in mem] for mem in sets] == [list(lgs) for lgs in LG_SETS]
    at, bad = 0, []
    for s, mem in enumerate(sets):
        terms = sum(2 * m.lg + 2 for m in mem)
        sc = np.frombuffer(raw, dtype=np.uint64, count=terms * 4, offset=at).reshape(terms, 4)
        shares = np.frombuffer(raw, dtype=np.uint64, count=len(mem) * 4, offset=at + terms * 32).reshape(len(mem), 4)
        at += terms * 32 + len(mem) * 32
        t = 0
        for a, m in enumerate(mem):
            K = 2 * m.lg + 2
            bad += [(s, a, m.lg) + b for b in fc.check_member(m, sc[t:t + K], shares[a])]
            t += K
        assert t == terms
    assert at == len(raw)
    assert not bad, "%d wrong words; first (set, member, lg, what, index): %s" % (len(bad), bad[:8])


def test_the_kernel_runs_the_headers_member_function():
    kernel = open(os.path.join(CSRC, "mixed_terms.hip")).read()
    assert '#include "mixed_terms_lane.hpp"' in kernel and kernel.count("mixed_terms_member(") == 1 and "void mixed_terms_member" not in kernel
    lane = open(os.path.join(CSRC, "mixed_terms_lane.hpp")).read()
    assert "HALO_DEV void mixed_terms_member(" in lane and lane.count("fused_terms_lane(") == 1
