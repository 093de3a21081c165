"""Cases for the key folds of pcdl::open (key_fold.hip k_fold_points, k_fold_points4, k_fold_points4_quad; foldtab.hip k_fold_tab4,
k_foldtab_build), shared by the host build (tests/test_fold_host.py, tests/native/fold_host.cpp) and the device hook
(tests/test_gpu_fold_points.py, halo_dev_fold_points).  Not a test module.

    levels 1:  out[j] = G[j] + xi G[j+m]                                   key of 2 m points
    levels 2:  out[j] = G[j] + s1 G[j+m] + s2 G[j+2m] + s3 G[j+3m]         key of 4 m points

The reference is the oracle alone: orc_ipa_round_fold on the Jacobian key (twice, xi1 over 2 m and xi2 over m, for a pair: that is
(s1, s2, s3) = (xi2, xi1, xi1 xi2)), orc_point_mul + orc_point_add for a triple no pair gives.  The comparison is exact, on
orc.affine_canonical: no tolerance anywhere.  The expected outputs of a (key, scalars, m) are computed once and serve every form.

Challenges: the values at which the digit strings the kernels walk (host_math.hpp glv_digits: ten 3-bit codes per word; foldtab.hip:
signed base-64 comb digits) have their edges -- see check_digit_edges / table_scalars.  Keys: URS points with exceptional positions
written in, class by class (L1_CLASSES, L2_CLASSES): position j takes class (j + 3 [j >= half] + challenge index) mod #classes with
half = (m + 1) / 2, so neighbouring lanes, neighbouring quads of the quad kernel and the two outputs j, j + half of a
two-outputs-per-lane lane fall into different classes, every wave has exceptional and plain lanes, and over a sweep of challenges
every position meets every class.  From m = 16 on three lanes are planted on top: (infinity, finite), (finite, infinity) and
(infinity, infinity) as the (j, j + half) results of one lane -- the Z = 1 substitution of the shared inversion.
"""
import ctypes as C
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import orc
import pallas_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = pm.R_ORDER
LAM = 0x6819a58283e528e511db4d81cf70f5a0fed467d47c033af2aa9d2e050aa0e4f  # lambda (x, y) = (beta x, y)
assert (LAM * LAM + LAM + 1) % R == 0

SIZES = [1, 2, 3, 63, 64, 65, 255, 256, 257, 513]
FULL_SIZES = (3, 65, 257)   # the whole challenge list runs here; two challenges at the other sizes
TABLE_SIZES = [64, 256, 1024, 2048]  # context sizes n = 4 m of the table forms (m = 512: the launcher's own switch to two outputs per lane)

_rng = pm.SplitMix64(0x464F4C44)
RANDOM = [_rng.next_scalar() for _ in range(8)]

# ---------------------------------------------------------------------------------------------------- challenges
L1_CHALLENGES = [("0", 0), ("1", 1), ("2", 2), ("3", 3), ("r-1", R - 1), ("r-2", R - 2),
                 ("lambda", LAM), ("lambda^2", LAM * LAM % R), ("lambda+1", (LAM + 1) % R), ("r-lambda", R - LAM)]
L1_CHALLENGES += [("2^%d" % k, (1 << k) % R) for k in (9, 10, 19, 20, 127, 128)]
L1_CHALLENGES += [("2^128-1", (1 << 128) - 1), ("2^254 mod r", (1 << 254) % R), ("(r-1)/2", (R - 1) // 2), ("(r+1)/2", (R + 1) // 2)]
L1_CHALLENGES += [("random%d" % i, RANDOM[i]) for i in range(3)]
L1_SHORT = [("r-1", R - 1), ("random0", RANDOM[0])]  # the two challenges of the other sizes

# levels 2: (name, ("pair", xi1, xi2)) or (name, ("triple", s1, s2, s3)); a pair folds as two rounds
_X = RANDOM[3]
L2_SCALARS = [("%s | random" % nm, ("pair", v, RANDOM[4])) for nm, v in L1_CHALLENGES]
L2_SCALARS += [("random | %s" % nm, ("pair", RANDOM[5], v)) for nm, v in L1_CHALLENGES]
L2_SCALARS += [("1 | 1", ("pair", 1, 1)), ("1 | r-1", ("pair", 1, R - 1)), ("r-1 | r-1", ("pair", R - 1, R - 1)),
               ("x | x (s1 == s2)", ("pair", _X, _X)), ("x | 1/x (s3 == 1)", ("pair", _X, pow(_X, -1, R))),
               ("lambda | lambda^2 (s3 == 1)", ("pair", LAM, LAM * LAM % R)), ("2^9 | random (lengths differ)", ("pair", 1 << 9, RANDOM[6]))]
# (no two rounds give these: through the hook and the host build only)
L2_SCALARS += [("(s1, s2, 0)", ("triple", RANDOM[0], RANDOM[1], 0)), ("(0, s2, s3)", ("triple", 0, RANDOM[1], RANDOM[2])),
               ("(s1, 0, s3)", ("triple", RANDOM[0], 0, RANDOM[2])), ("(0, 0, s3)", ("triple", 0, 0, RANDOM[2])),
               ("(0, s2, 0)", ("triple", 0, RANDOM[1], 0)), ("(s1, 0, 0)", ("triple", RANDOM[0], 0, 0))]
L2_SHORT = [("r-1 | r-1", ("pair", R - 1, R - 1)), ("random | random", ("pair", RANDOM[5], RANDOM[4]))]


def triple_of(spec):
    if spec[0] == "pair":
        return (spec[2] % R, spec[1] % R, spec[1] * spec[2] % R)
    return tuple(v % R for v in spec[1:])


def glv_digits(lib, x):
    """the digit string the generic kernels walk for x (halo_test_glv_digits, host only) -> list of codes"""
    out = (C.c_uint8 * 144)()
    n = C.c_int()
    assert lib.halo_test_glv_digits(orc.ptr(orc.fr_to_mont(x)), out, C.byref(n)) == 0
    return [out[i] for i in range(n.value)]


def comb_digits(lib, x):
    """the 22 + 22 signed base-64 digits the table kernel walks for x (halo_test_fold_digits, host only)"""
    out = (C.c_int8 * 44)()
    assert lib.halo_test_fold_digits(orc.ptr(orc.fr_to_mont(x)), out) == 0
    return [int(out[i]) for i in range(44)]


def check_digit_edges(lib):
    """the challenge list reaches the edges of the ten-codes-per-word packing; -> the facts, for the log"""
    lens = {nm: len(glv_digits(lib, v)) for nm, v in L1_CHALLENGES}
    top_at_9 = [nm for nm, n in lens.items() if n >= 1 and (n - 1) % 10 == 9]
    top_at_0 = [nm for nm, n in lens.items() if n > 1 and (n - 1) % 10 == 0]
    one = [nm for nm, n in lens.items() if n == 1]
    none = [nm for nm, n in lens.items() if n == 0]
    assert top_at_9, "no string whose top digit is the last of its word"
    assert top_at_0, "no string whose top digit is the first of a later word"
    assert one, "no one-digit string"
    assert len(none) == 1, "exactly one empty string (xi = 0)"
    # three strings of very different length in the Straus form
    l9, lr = len(glv_digits(lib, 1 << 9)), len(glv_digits(lib, RANDOM[6]))
    assert lr - l9 > 100
    return {"lengths": lens, "longest": max(lens.values()), "top digit at k = 9": top_at_9, "top digit at k = 0 of a later word": top_at_0,
            "one digit": one, "empty": none, "2^9 against random": (l9, lr)}


def table_scalars(lib):
    """scalars for the table forms, with the property each is there for (asserted) -> [(name, x)]"""
    rng = pm.SplitMix64(0x544142)
    plus = minus = None
    while plus is None or minus is None:
        x = rng.next_scalar()
        d = comb_digits(lib, x)
        if 32 in d and plus is None:
            plus = x
        elif -32 in d and minus is None:
            minus = x
    small, small_lam = 5, 5 * LAM % R
    d = comb_digits(lib, small)
    assert any(d[:22]) and not any(d[22:]), "a small integer has an all-zero lambda half"
    d = comb_digits(lib, small_lam)
    assert not any(d[:22]) and any(d[22:]), "a small multiple of lambda has an all-zero plain half"
    assert 32 in comb_digits(lib, plus) and -32 in comb_digits(lib, minus)
    return [("digit +32", plus), ("digit -32", minus), ("lambda half empty", small), ("plain half empty", small_lam)]


# ---------------------------------------------------------------------------------------------------- points
_L = None


def _lib():
    global _L
    if _L is None:
        _L = orc.lib()
        orc.fr_to_mont(1)  # (the oracle's one-time self-check runs here, before any thread calls it)
    return _L


def _mont(x):
    return orc.fr_to_mont(x % R)


def jac_of(aff):
    j = np.zeros(12, dtype=np.uint64)
    _lib().orc_affine_to_jac(orc.ptr(np.ascontiguousarray(aff, dtype=np.uint64)), orc.ptr(j))
    return j


def mul(p, k):
    o = np.zeros(12, dtype=np.uint64)
    _lib().orc_point_mul(orc.ptr(np.ascontiguousarray(p)), orc.ptr(_mont(k)), orc.ptr(o))
    return o


def add(a, b):
    o = np.zeros(12, dtype=np.uint64)
    _lib().orc_point_add(orc.ptr(np.ascontiguousarray(a)), orc.ptr(np.ascontiguousarray(b)), orc.ptr(o))
    return o


def neg(p):
    """(X, -Y, Z): the Montgomery words of -Y are p - Y"""
    o = np.array(p, dtype=np.uint64)
    y = sum(int(w) << (64 * i) for i, w in enumerate(o[4:8]))
    o[4:8] = [((pm.P - y) % pm.P >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]
    return o


def is_inf(jac):
    return not jac[8:12].any()


def aff_of(jac):
    """any Jacobian point of the oracle -> 8 affine words (canonical, Montgomery form), (0, 0) = infinity"""
    c = orc.point_canonical(jac)
    if c is None:
        return np.zeros(8, dtype=np.uint64)
    return np.array([((v << 256) % pm.P >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for v in c for i in range(4)], dtype=np.uint64)


_URS = {}


def urs(n):
    """the first n URS points -> (n x 8 affine words, n x 12 Jacobian words)"""
    if "a" not in _URS or _URS["a"].shape[0] < n:
        _URS["a"] = orc.urs_affine(2, n)
        _URS["j"] = np.stack([jac_of(_URS["a"][i]) for i in range(n)])
    return _URS["a"][:n], _URS["j"][:n]


# ---------------------------------------------------------------------------------------------------- keys
L1_CLASSES = ["plain", "inf at G[j]", "inf at G[j+m]", "inf at both", "G[j] = xi G[j+m]", "G[j] = -xi G[j+m]", "G[j+m] = G[j]", "G[j+m] = -G[j]"]
L2_CLASSES = ["plain", "inf at G[j]", "inf at G[j+m]", "inf at G[j+2m]", "inf at G[j+3m]", "inf at all four", "G[j] = sum of the upper terms",
              "G[j] = -sum of the upper terms", "p1 = p2", "p1 = -p2", "p1 = p2 = p3", "p2 = lambda p1", "p1 + p2 + p3 = 0", "p1 = G[j]", "p1 = -G[j]"]
INF_OUTPUT = {"inf at both", "G[j] = -xi G[j+m]", "inf at all four", "G[j] = -sum of the upper terms"}


def class_of(j, m, ci, ncls):
    half = (m + 1) // 2
    return (j + 3 * (j >= half) + ci) % ncls


def planted_lanes(m):
    """{j: 'inf' | 'finite'} on top of the rotation: lanes 1, 2, 3 of the two-outputs-per-lane forms get (infinity, finite),
    (finite, infinity) and (infinity, infinity)"""
    if m < 16:
        return {}
    half = (m + 1) // 2
    return {1: "inf", 1 + half: "finite", 2: "finite", 2 + half: "inf", 3: "inf", 3 + half: "inf"}


def make_key(levels, m, triple, ci):
    """-> (key as (2 levels m) x 8 affine words, as x 12 Jacobian words, the class name of every position)"""
    parts = 2 * levels
    ua, uj = urs(parts * m)
    aff, g = ua.copy().reshape(parts, m, 8), uj.copy().reshape(parts, m, 12)
    names = L1_CLASSES if levels == 1 else L2_CLASSES
    planted = planted_lanes(m)
    cls = []
    for j in range(m):
        c = names[class_of(j, m, ci, len(names))]
        if j in planted:
            c = names[3 if levels == 1 else 5] if planted[j] == "inf" else "plain"
        cls.append(c)
        p = g[:, j]
        if c == "plain":
            continue
        if c.startswith("inf at all") or c == "inf at both":
            p[:] = 0
        elif c.startswith("inf at G[j+"):
            p[1 if c == "inf at G[j+m]" else int(c[11])] = 0
        elif c == "inf at G[j]":
            p[0] = 0
        elif levels == 1:
            if c == "G[j] = xi G[j+m]":
                p[0] = mul(p[1], triple[0])
            elif c == "G[j] = -xi G[j+m]":
                p[0] = mul(p[1], R - triple[0])
            elif c == "G[j+m] = G[j]":
                p[1] = p[0]
            else:
                p[1] = neg(p[0])
        elif c == "p1 = p2":
            p[2] = p[1]
        elif c == "p1 = -p2":
            p[2] = neg(p[1])
        elif c == "p1 = p2 = p3":
            p[2] = p[1]; p[3] = p[1]
        elif c == "p2 = lambda p1":
            p[2] = mul(p[1], LAM)
        elif c == "p1 + p2 + p3 = 0":
            p[3] = neg(add(p[1], p[2]))
        elif c == "p1 = G[j]":
            p[1] = p[0]
        elif c == "p1 = -G[j]":
            p[1] = neg(p[0])
        else:
            t = add(add(mul(p[1], triple[0]), mul(p[2], triple[1])), mul(p[3], triple[2]))
            p[0] = t if c == "G[j] = sum of the upper terms" else neg(t)
        for t in range(parts):
            if not np.array_equal(p[t], uj[t * m + j]):
                aff[t, j] = aff_of(p[t])
    return np.ascontiguousarray(aff.reshape(parts * m, 8)), np.ascontiguousarray(g.reshape(parts * m, 12)), cls


# ---------------------------------------------------------------------------------------------------- the oracle's fold
_POOL = None


def _pool():
    global _POOL
    if _POOL is None:
        _POOL = ThreadPoolExecutor(max_workers=min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 4))
    return _POOL


def _fold_chunk(sub, c, rounds):
    """sub = the positions [j0, j1) of every part of the key, part after part (a key of the same shape); rounds = challenges"""
    L = _lib()
    g = np.ascontiguousarray(sub)
    mm = g.shape[0] // 2
    one = _mont(1)
    for xi in rounds:
        cs, zs = np.zeros((2 * mm, 4), dtype=np.uint64), np.zeros((2 * mm, 4), dtype=np.uint64)  # (the round folds them too: zeros)
        L.orc_ipa_round_fold(orc.ptr(g), orc.ptr(cs), orc.ptr(zs), C.c_size_t(mm), orc.ptr(_mont(xi)), orc.ptr(one))
        mm //= 2
    return g[:c].copy()


def _triple_chunk(sub, c, triple):
    p = sub.reshape(4, c, 12)
    out = np.zeros((c, 12), dtype=np.uint64)
    for j in range(c):
        out[j] = add(add(add(p[0, j], mul(p[1, j], triple[0])), mul(p[2, j], triple[1])), mul(p[3, j], triple[2]))
    return out


def expected(key_jac, m, levels, spec):
    """the oracle's folded key as m x 8 affine words; spec: ("pair", xi1, xi2) / ("triple", ...) (levels 2), ("xi", xi) (levels 1)"""
    _lib()
    parts = 2 * levels
    g = key_jac.reshape(parts, m, 12)
    step = max(1, -(-m // 32))
    jobs = []
    for j0 in range(0, m, step):
        j1 = min(m, j0 + step)
        sub = np.ascontiguousarray(g[:, j0:j1]).reshape(parts * (j1 - j0), 12)
        if spec[0] == "triple":
            jobs.append(_pool().submit(_triple_chunk, sub, j1 - j0, triple_of(spec)))
        else:
            jobs.append(_pool().submit(_fold_chunk, sub, j1 - j0, [spec[1]] if levels == 1 else [spec[1], spec[2]]))
    out = np.concatenate([f.result() for f in jobs])
    return np.stack([aff_of(p) for p in out])


class Case:
    """one (key, scalars, m): the affine key, the Montgomery scalars, the oracle's outputs, the class of every position"""

    def __init__(self, levels, m, name, spec, ci):
        self.levels, self.m, self.name, self.spec = levels, m, name, spec
        self.triple = (spec[1] % R,) if levels == 1 else triple_of(spec)
        self.key, key_jac, self.classes = make_key(levels, m, self.triple, ci)
        self.scalars = np.stack([_mont(s) for s in self.triple])
        self.want = expected(key_jac, m, levels, spec)
        # what the generator promises, on the oracle's results
        inf_out = [not self.want[j].any() for j in range(m)]
        for j, c in enumerate(self.classes):
            if c in INF_OUTPUT:
                assert inf_out[j], (name, m, j, c)
        half = (m + 1) // 2
        self.mixed = {"inf, finite": 0, "finite, inf": 0, "inf, inf": 0}
        for j in range(m - half):
            a, b = inf_out[j], inf_out[j + half]
            if a or b:
                self.mixed["inf, inf" if a and b else ("inf, finite" if a else "finite, inf")] += 1
            if m >= 2 * len(L2_CLASSES):
                assert self.classes[j] != self.classes[j + half] or j in (3,), (m, j)
        if m >= 16:
            assert all(self.mixed.values()), (name, m, self.mixed)
        if m >= 2 * len(L2_CLASSES):
            names = L1_CLASSES if levels == 1 else L2_CLASSES
            assert set(self.classes) == set(names), (name, m)
            for w in range(0, m - 63, 64):  # every wave of one-output-per-lane lanes: some exceptional lanes, not all
                seen = set(self.classes[w: w + 64])
                assert "plain" in seen and len(seen) > 1


def cases(levels, m):
    full = L1_CHALLENGES if levels == 1 else L2_SCALARS
    short = L1_SHORT if levels == 1 else L2_SHORT
    todo = full if m in FULL_SIZES else short
    out = []
    for nm, v in todo:
        ci = [n for n, _ in full].index(nm) if nm in [n for n, _ in full] else 0
        out.append(Case(levels, m, nm, ("xi", v) if levels == 1 else v, ci))
    if m in FULL_SIZES and m < 2 * len(L2_CLASSES):  # a key too small for every class: the sweep of challenges rotates through them
        names = L1_CLASSES if levels == 1 else L2_CLASSES
        assert {c for case in out for c in case.classes} == set(names)
    return out


class TableCase:
    """a context's own key of n = 4 m exceptional points (scalar-related classes made for the first triple) and the triples the
    table forms run over it, with the oracle's outputs of each"""

    def __init__(self, n, lib):
        self.n, self.m = n, n // 4
        plus, minus, small, small_lam = [x for _, x in table_scalars(lib)]
        first = ("pair", RANDOM[5], RANDOM[4])
        self.triples = [("random | random", first), ("(+32, -32, small)", ("triple", plus, minus, small)),
                        ("(small lambda, small, +32)", ("triple", small_lam, small, plus)),
                        ("(-32, small lambda, small lambda)", ("triple", minus, small_lam, small_lam)),
                        ("1 | 1", ("pair", 1, 1)), ("r-1 | r-1", ("pair", R - 1, R - 1)), ("(s1, 0, s3)", ("triple", RANDOM[0], 0, RANDOM[2])),
                        ("(0, 0, s3)", ("triple", 0, 0, RANDOM[2]))]
        self.key, key_jac, self.classes = make_key(2, self.m, triple_of(first), 0)
        assert self.m < 2 * len(L2_CLASSES) or set(self.classes) == set(L2_CLASSES)  # (16 outputs, six of them planted lanes, hold fewer)
        self.scalars = [np.stack([_mont(v) for v in triple_of(spec)]) for _, spec in self.triples]
        self.want = [expected(key_jac, self.m, 2, spec) for _, spec in self.triples]
        for j, c in enumerate(self.classes):
            if c in INF_OUTPUT:
                assert not self.want[0][j].any(), (n, j, c)


def class_counts(case_list):
    n = {}
    for case in case_list:
        for c in case.classes:
            n[c] = n.get(c, 0) + 1
    return n


def assert_same(got, want, what):
    """exact equality on orc.affine_canonical (equal words are equal points: the shortcut for the usual case)"""
    got = np.asarray(got, dtype=np.uint64).reshape(-1, 8)
    assert got.shape == want.shape, what
    if np.array_equal(got, want):
        return
    for j in np.nonzero((got != want).any(axis=1))[0]:
        assert orc.affine_canonical(got[j]) == orc.affine_canonical(want[j]), "%s: output %d of %d" % (what, j, want.shape[0])


# ---------------------------------------------------------------------------------------------------- the host build
def build_host(tmp_dir):
    """compile tests/native/fold_host.cpp with ASan + UBSan -> (exe, None) or (None, reason to skip)"""
    if shutil.which("g++") is None or not os.path.isdir("/opt/rocm/include"):
        return None, "no g++ / HIP headers"
    exe = os.path.join(str(tmp_dir), "fold_host")
    cmd = ["g++", "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
           "-I/opt/rocm/include", "-I", os.path.join(ROOT, "halo-accumulation_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "fold_host.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "sanitize" in b.stderr:
        return None, "sanitizer runtime not installed"
    assert b.returncode == 0, b.stderr[-2000:]
    return exe, None


def run_host(exe, tmp_dir, case_list, tag):
    """every case through the sanitizer build -> [m x 8 words]; any sanitizer report fails.  The cases are dealt to as many
    processes as there are CPUs (at most 16): the instrumented lanes take ~2 ms per output"""
    cpus = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 4
    nproc = max(1, min(16, cpus, len(case_list)))
    shares = [list(range(k, len(case_list), nproc)) for k in range(nproc)]
    procs = []
    for k, share in enumerate(shares):
        fin, fout = os.path.join(str(tmp_dir), "fold_%s_%d.in" % (tag, k)), os.path.join(str(tmp_dir), "fold_%s_%d.out" % (tag, k))
        with open(fin, "wb") as f:
            for i in share:
                c = case_list[i]
                np.array([c.levels, c.key.shape[0], c.m, 1], dtype=np.uint32).tofile(f)
                np.ascontiguousarray(c.key, dtype=np.uint64).tofile(f)
                np.ascontiguousarray(c.scalars, dtype=np.uint64).tofile(f)
        procs.append((subprocess.Popen([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True), fin, fout, share))
    outs = [None] * len(case_list)
    for p, fin, fout, share in procs:
        so, se = p.communicate(timeout=600)
        assert p.returncode == 0 and so.startswith("ok ") and "runtime error" not in se and "Sanitizer" not in se, so + se[-3000:]
        flat = np.fromfile(fout, dtype=np.uint64)
        at = 0
        for i in share:
            m = case_list[i].m
            outs[i] = flat[at: at + 8 * m].reshape(m, 8)
            at += 8 * m
        assert at == flat.size
        os.remove(fin); os.remove(fout)
    return outs
