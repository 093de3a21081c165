"""Cases for the kernels that take points from the caller or derive the key: k_batch_to_affine (urs.hip, the normalisation of
halo_msm_points), k_batch_small_msm and k_small_msm_seg (small_sums.hip, the relations and member sums of the device-side verifiers),
k_urs_scalars and k_urs (urs.hip).  tests/test_gpu_point_paths.py runs them on the device, tests/test_small_msm_host.py through the
lanes compiled for the CPU under ASan + UBSan; the generators and checkers test themselves in tests/test_point_cases_cpu.py.  Not a
test module.  Plain Python and numpy over pallas_model and orc: importable without a GPU.

    Jacobian groups   points of the URS under a Z of every class (Montgomery one, 2, p - 1, random), one point under two Z, a point
                      and its negation, infinity spelled three ways; planted on the index map of k_batch_to_affine (point t + e
                      stride, four per lane, one shared inversion: table_cases.exceptional_key, layout "step") and at ragged sizes
    small-MSM sums    K terms (point, canonical scalar) and their plain sum; built so that every level of the two kernels' shuffle
                      trees is the first to add P + P, P + (-P), infinity + Q, Q + infinity and infinity + infinity in some case.
                      The tree shapes are restated here (events_batch, events_seg) to COUNT that coverage, never for an expected value
    URS runs          (first index, stride, n) with indices either side of 2^32 and above 2^63
The references are exact -- Python integers (pallas_model) and the oracle's C restatement (orc): no tolerance anywhere.
"""
import os
import shutil
import subprocess

import numpy as np

import orc
import pallas_model as pm
import table_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = pm.P
R = pm.R_ORDER
RINV = tc.RINV


# ---------------------------------------------------------------------------------------------------- base points
_BASE = {}


def base_words(n=2304):
    """the first n points of the URS (orc.urs_affine(2, n)): distinct finite points, n x 8 affine words"""
    if "w" not in _BASE or _BASE["w"].shape[0] < n:
        _BASE["w"] = orc.urs_affine(2, n)
    return _BASE["w"][:n]


def model_point(aff):
    """8 affine words -> a point of pallas_model (None = infinity)"""
    aff = np.asarray(aff, dtype=np.uint64)
    if not aff.any():
        return None
    return (tc._int(aff[:4]) * RINV % P, tc._int(aff[4:8]) * RINV % P)


def base_point(i):
    if "m" not in _BASE:
        _BASE["m"] = {}
    if i not in _BASE["m"]:
        _BASE["m"][i] = model_point(base_words()[i])
    return _BASE["m"][i]


# ---------------------------------------------------------------------------------------------------- Jacobian groups
Z_CLASSES = ["Montgomery one", "2", "p - 1", "random"]
INF_SPELLINGS = ["Z = 0, X = Y = 0", "Z = 0, random X, Y", "Z = 0, X, Y of a finite point"]
STEP_SIZES = {1000: (300, 600), 2020: (1000, 1500)}  # m: the originals of the same-lane pairs (exceptional_key); strides 256 and 512
RAGGED_SIZES = [1, 2, 3, 5, 255, 257, 1023, 1025, 2049]


def _coord_words(v):
    return pm.to_mont_limbs(v, P)


class JacGroup:
    """m Jacobian points (m x 12 arkworks words), their affine forms by pallas_model.jacobian_to_affine on the de-Montgomerised
    integers (m x 8 words, (0, 0) = infinity), the class of every index"""

    def __init__(self, name, affine, classes, seed):
        affine = np.asarray(affine, dtype=np.uint64).reshape(-1, 8)
        self.name, self.m = name, affine.shape[0]
        rng = pm.SplitMix64(seed)
        rnd = lambda: (rng.next_u64() | rng.next_u64() << 64 | rng.next_u64() << 128 | rng.next_u64() << 192) % (P - 1) + 1
        self.jac = np.zeros((self.m, 12), dtype=np.uint64)
        self.classes = []
        infs = 0
        for i in range(self.m):
            pt = model_point(affine[i])
            if pt is None:
                how = INF_SPELLINGS[infs % 3]
                infs += 1
                X, Y = (0, 0) if how == INF_SPELLINGS[0] else ((rnd(), rnd()) if how == INF_SPELLINGS[1] else base_point(2000 + infs))
                Z = 0
                self.classes.append("%s; %s" % (classes[i], how))
            else:
                zc = Z_CLASSES[(i + i // 256) % 4]  # (a point and the one a stride further on take different classes)
                Z = {"Montgomery one": 1, "2": 2, "p - 1": P - 1}.get(zc) or rnd()
                X, Y = pt[0] * Z * Z % P, pt[1] * Z * Z * Z % P
                self.classes.append("%s; Z %s" % (classes[i], zc))
            self.jac[i] = _coord_words(X) + _coord_words(Y) + _coord_words(Z)
        # the reference: the words as the device gets them, out of Montgomery form, through the integer model
        self.want = np.zeros((self.m, 8), dtype=np.uint64)
        for i in range(self.m):
            X, Y, Z = (tc._int(self.jac[i, k:k + 4]) * RINV % P for k in (0, 4, 8))
            self.want[i] = tc.aff_words(pm.jacobian_to_affine(X, Y, Z))

    def infinite(self):
        return [i for i in range(self.m) if not self.jac[i, 8:].any()]


def ragged_affine(m):
    """m points of the URS with an infinity at index 0, at m - 1 and on every live point of one lane -> (affine words, classes)"""
    key = np.array(base_words()[:m], dtype=np.uint64)
    classes = ["plain"] * m
    stride = tc.step_stride(m)

    def plant(i, name):
        if classes[i] == "plain":
            classes[i] = name
        key[i] = 0

    plant(0, "inf at index 0")
    plant(m - 1, "inf at m - 1")
    lane = 2 if m <= 5 else 5
    for e in range(tc.STEP_E):
        if lane + e * stride < m and m > 3:
            plant(lane + e * stride, "inf, every live point of lane %d (e = %d)" % (lane, e))
    return key, classes


_GROUPS = []


def jac_groups():
    """every group: the two planted sizes of the step layout, then each ragged size plain and planted"""
    if not _GROUPS:
        for m, pairs in STEP_SIZES.items():
            key, classes = tc.exceptional_key(base_words()[:m], "step", pairs=pairs)
            _GROUPS.append(JacGroup("step layout, m = %d, stride %d" % (m, tc.step_stride(m)), key, classes, 0x6A6163 + m))
        for m in RAGGED_SIZES:
            _GROUPS.append(JacGroup("ragged m = %d, plain" % m, base_words()[:m], ["plain"] * m, 0x726167 + m))
            key, classes = ragged_affine(m)
            _GROUPS.append(JacGroup("ragged m = %d, planted" % m, key, classes, 0x706C61 + m))
    return _GROUPS


def check_affine(got, group):
    """every output of a group against its reference, word for word (the device writes canonical words) -> failing (index, class)"""
    got = np.asarray(got, dtype=np.uint64).reshape(-1, 8)
    assert got.shape == group.want.shape, (group.name, got.shape)
    return [(int(i), group.classes[i]) for i in np.nonzero((got != group.want).any(axis=1))[0]]


# ---------------------------------------------------------------------------------------------------- small-MSM sums
EVENTS = ["P + P", "P + (-P)", "inf + Q", "Q + inf", "inf + inf"]
LEVELS = [32, 16, 8, 4, 2, 1]          # the shuffle distances, in the order the kernels take them
BATCH_K = [1, 2, 3, 22, 33, 42, 63, 64]  # (22 and 42: the relations of lg n = 10 and 20; 3 and 33 for the all-equal sums)
BATCH_M = [1, 2, 65]                   # sums per launch
EDGE_SCALARS = ([("0", 0), ("1", 1), ("2", 2), ("3", 3), ("r - 1", R - 1), ("r - 2", R - 2), ("(r - 1) / 2", (R - 1) // 2),
                 ("(r + 1) / 2", (R + 1) // 2), ("2^253", 1 << 253), ("2^254", 1 << 254), ("2^254 - 1", (1 << 254) - 1)]
                + [x for j in range(1, 8) for x in (("2^%d - 1" % (32 * j), (1 << 32 * j) - 1), ("2^%d" % (32 * j), 1 << 32 * j),
                                                    ("r - 2^%d" % (32 * j), R - (1 << 32 * j)))])
assert all(0 <= k < R for _, k in EDGE_SCALARS) and len(EDGE_SCALARS) == 32

_PROD = {}   # (point, scalar) -> (12 Jacobian words of the oracle's product, its canonical form)
_MODEL = {}  # (point, scalar) -> pallas_model's product


def _orc_jac(pt):
    return tc._jac(tc.aff_words(pt))


def product(term):
    """orc_point_mul of one term, computed once -> (Jacobian words, canonical point or None)"""
    if term not in _PROD:
        pt, k = term
        o = np.zeros(12, dtype=np.uint64)
        orc.lib().orc_point_mul(orc.ptr(_orc_jac(pt)), orc.ptr(orc.fr_to_mont(k)), orc.ptr(o))
        _PROD[term] = (o, orc.point_canonical(o))
    return _PROD[term]


def unique_terms():
    return len(_PROD)


def orc_sum(jacs):
    acc = _orc_jac(None)
    for j in jacs:
        o = np.zeros(12, dtype=np.uint64)
        orc.lib().orc_point_add(orc.ptr(acc), orc.ptr(np.ascontiguousarray(j)), orc.ptr(o))
        acc = o
    return acc


def model_sum(terms):
    """the same plain sum through pallas_model.mul / add alone"""
    acc = None
    for t in terms:
        if t not in _MODEL:
            _MODEL[t] = pm.mul(t[0], t[1])
        acc = pm.add(acc, _MODEL[t])
    return acc


class Case:
    """K terms (point of pallas_model or None, canonical scalar) and their plain sum: orc_point_mul per term, orc_point_add over
    them.  both: also summed by pallas_model (every cancelling, doubling and edge-scalar case)."""

    def __init__(self, name, terms, both=False):
        assert 1 <= len(terms) <= 64 and all(0 <= k < R for _, k in terms), name
        self.name, self.terms, self.K, self.both = name, [(pt, int(k)) for pt, k in terms], len(terms), both
        prods = [product(t) for t in self.terms]
        self.want = orc_sum([p[0] for p in prods])
        self.canon = orc.point_canonical(self.want)
        self.prods = [p[1] for p in prods]

    def points(self):
        return np.stack([tc.aff_words(pt) for pt, _ in self.terms])

    def scalars(self):
        return tc.scalar_words([k for _, k in self.terms])


def _event(a, b):
    if a is None or b is None:
        return "inf + inf" if a is None and b is None else ("inf + Q" if a is None else "Q + inf")
    if a[0] == b[0]:
        return "P + P" if a[1] == b[1] else "P + (-P)"
    return None


def events_batch(prods):
    """k_batch_small_msm: lane l < off takes lane l + off, off = 32 .. 1 -> ({event: the first level that meets it}, lane 0's value)"""
    v = list(prods) + [None] * (64 - len(prods))
    first = {}
    for off in LEVELS:
        for l in range(off):
            ev = _event(v[l], v[l + off])
            if ev:
                first.setdefault(ev, off)
            v[l] = pm.add(v[l], v[l + off])
    return first, v[0]


def seg_width(L):
    w = 1
    while w < L:
        w *= 2
    return w


def events_seg(prods):
    """k_small_msm_seg: a sum of L terms owns w = 2^ceil(lg L) lanes, lane i takes lane i ^ off for every off < w, both partners add"""
    w = seg_width(len(prods))
    v = list(prods) + [None] * (w - len(prods))
    first = {}
    for off in LEVELS:
        if off >= w:
            continue
        for i in range(w):
            ev = _event(v[i], v[i ^ off])
            if ev:
                first.setdefault(ev, off)
        v = [pm.add(v[i], v[i ^ off]) for i in range(w)]
    return first, v[0]


def coverage(cases):
    """{kernel: {level: {event: the names of the cases that meet the event at this level first}}}"""
    table = {k: {off: {ev: [] for ev in EVENTS} for off in LEVELS} for k in ("k_batch_small_msm", "k_small_msm_seg")}
    for c in cases:
        for kernel, fn in (("k_batch_small_msm", events_batch), ("k_small_msm_seg", events_seg)):
            if kernel == "k_batch_small_msm" and c.K not in BATCH_K:
                continue
            first, top = fn(c.prods)
            assert top == c.canon, (c.name, kernel)  # (the restated tree adds the same terms: a check of the restatement only)
            for ev, off in first.items():
                table[kernel][off][ev].append(c.name)
    return table


def format_coverage(table):
    lines = []
    for kernel, levels in table.items():
        lines.append("%-18s %s" % (kernel, "".join("%12s" % ev for ev in EVENTS)))
        for off in LEVELS:
            lines.append("%-18s %s" % ("  off = %d" % off, "".join("%12d" % len(levels[off][ev]) for ev in EVENTS)))
    return "\n".join(lines)


class _Builder:
    """the small-MSM cases, made once"""

    def __init__(self):
        self.rng = pm.SplitMix64(0x736D616C6C)
        self.next_point = 64
        self.pool = [(base_point(i), self.scalar()) for i in range(64)]                  # 64 ordinary terms
        self.dull = [(base_point(2100 + i), 0) if i % 2 == 0 else (None, self.scalar()) for i in range(64)]  # 64 terms worth infinity
        self.cases = []
        self.fill = 0

    def scalar(self):
        return self.rng.next_scalar() or 1

    def point(self):
        self.next_point += 1
        assert self.next_point < 2000
        return base_point(self.next_point)

    def add(self, name, terms, both=False):
        c = Case(name, terms, both)
        self.cases.append(c)
        return c

    def random_terms(self, K):
        return [(self.point(), self.scalar()) for _ in range(K)]

    # -- a level of the tree made the first to meet an event, over 64 ordinary terms: before the step at distance off, lane a
    #    (a < 2 off) holds the sum of the lanes congruent to a mod 2 off, in both kernels
    @staticmethod
    def _class_sum(terms, a, mod, skip=None):
        acc = None
        for j in range(a % mod, 64, mod):
            if j != skip:
                acc = pm.add(acc, product(terms[j])[1])
        return acc

    def _force(self, terms, a, mod, target):
        """the term of lane a is replaced so that the lanes congruent to a mod `mod` sum to `target`"""
        pt = pm.add(target, pm.neg(self._class_sum(terms, a, mod, skip=a)))
        assert pt is not None
        terms[a] = (pt, 1)

    def forced(self, off, event):
        l = (3 * off) // 4 % off
        t = list(self.pool)
        if event == "P + P":
            self._force(t, l + off, 2 * off, self._class_sum(t, l, 2 * off))
        elif event == "P + (-P)":
            self._force(t, l + off, 2 * off, pm.neg(self._class_sum(t, l, 2 * off)))
        else:
            for side, wanted in ((l, event in ("inf + Q", "inf + inf")), (l + off, event in ("Q + inf", "inf + inf"))):
                if not wanted:
                    continue
                if off == 32:
                    t[side] = (None, self.scalar()) if side == l else (self.point(), 0)
                else:  # the lane's two halves cancel one level earlier
                    self._force(t, side + 2 * off, 4 * off, pm.neg(self._class_sum(t, side, 4 * off)))
        return self.add("64 ordinary terms, off = %d first to meet %s (lane %d)" % (off, event, l), t, both=True)

    def spelled(self, off, how):
        """62 terms worth infinity, two that meet at distance off, and (off > 1) one survivor in another residue class"""
        l = (3 * off) // 4 % off
        t = list(self.dull)
        g, k = self.point(), self.scalar()
        t[l] = (g, k)
        t[l + off] = {"same point, same scalar": (g, k), "negated point, same scalar": (pm.neg(g), k), "same point, scalar r - k": (g, R - k)}[how]
        if off > 1:
            t[(l + 1) % (2 * off)] = (self.point(), self.scalar())
        return self.add("sparse, off = %d: %s (lanes %d, %d)" % (off, how, l, l + off), t, both=True)

    def filler(self, K):
        """an ordinary sum of K terms unlike every other: the pool's first K terms, one of them replaced"""
        self.fill += 1
        t = list(self.pool[:K])
        t[self.fill % K] = (base_point(2000 - self.fill), self.scalar())
        return Case("filler %d, K = %d" % (self.fill, K), t)

    def build(self):
        for off in LEVELS:
            for ev in EVENTS:
                self.forced(off, ev)
            for how in ("same point, same scalar", "negated point, same scalar", "same point, scalar r - k"):
                self.spelled(off, how)
        for K in (2, 3, 33, 63, 64):
            self.add("all %d terms equal" % K, [(base_point(40), self.pool[40][1])] * K, both=True)
        for K in (2, 22, 42, 64):  # pairs (P, k), (-P, k) and (P, k), (P, r - k): in neighbouring lanes, and lanes apart
            t, free = [None] * K, list(range(K))
            for i in range(K // 2):
                g, k = self.point(), self.scalar()
                a = free.pop(0)
                b = free.pop(0 if i % 2 == 0 else len(free) // 2)
                t[a], t[b] = (g, k), ((pm.neg(g), k) if i % 4 < 2 else (g, R - k))
            c = self.add("whole sum of %d terms cancels" % K, t, both=True)
            assert c.canon is None
        for K in (22, 42, 64):
            h = K // 2
            t = [x for i in range(h // 2) for x in [(base_point(950 + i), 11 + i), (base_point(950 + i), R - 11 - i)]]
            t = t[:h] if len(t) >= h else t + [(None, 5)]
            c = self.add("first half of %d terms cancels, the other survives" % K, t + self.random_terms(K - len(t)), both=True)
            assert c.canon is not None
        for K in (22, 63):
            for where, idx in (("term 0", [0]), ("term K - 1", [K - 1]), ("alternating", list(range(0, K, 2)))):
                t = self.random_terms(K)
                for i in idx:
                    t[i] = (None, self.scalar())
                self.add("infinite point with a non-zero scalar at %s, K = %d" % (where, K), t)
        for K in (2, 22, 42):
            t = self.random_terms(K)
            t[K // 3] = (t[K // 3][0], 0)
            self.add("finite point with scalar 0, K = %d" % K, t)
        for K in (1, 22, 64):
            c = self.add("all %d terms infinite" % K, [(None, self.scalar()) for _ in range(K)], both=True)
            assert c.canon is None
        for name, k in EDGE_SCALARS:  # the ladder alone: one term
            self.add("scalar %s on an ordinary point" % name, [(self.point(), k)], both=True)
        for K in (33, 42):            # and every edge scalar in one sum, each on a lane of its own
            t = [(self.point(), k) for _, k in EDGE_SCALARS] + self.random_terms(K - 32)
            self.add("the 32 edge scalars in a sum of %d" % K, t, both=True)
        for K in (1, 2, 3, 5, 9, 17, 22, 33, 42, 63, 64):
            for rep in range(2):
                self.add("ordinary, K = %d (%d)" % (K, rep), self.random_terms(K))
        return self


_B = []


def _builder():
    if not _B:
        _B.append(_Builder().build())
    return _B[0]


def msm_cases():
    return _builder().cases


def batch_launches():
    """[(K, [cases])]: every case with K in BATCH_K, in launches of 1, 2 and 65 sums whose results are pairwise different (a
    result written to a neighbour's slot shows); ordinary fillers complete a launch"""
    if "launches" not in _BASE:
        b, out = _builder(), []
        for K in BATCH_K:
            pending = [c for c in b.cases if c.K == K]
            sizes = 0
            while pending or sizes < len(BATCH_M):
                size = BATCH_M[sizes % len(BATCH_M)]
                sizes += 1
                launch, seen, rest = [], set(), []
                for c in pending:
                    if len(launch) < size and c.canon not in seen:
                        launch.append(c)
                        seen.add(c.canon)
                    else:
                        rest.append(c)
                while len(launch) < size:
                    f = b.filler(K)
                    if f.canon not in seen:
                        launch.append(f)
                        seen.add(f.canon)
                assert len({c.canon for c in launch}) == size
                out.append((K, launch))
                pending = rest
        _BASE["launches"] = out
    return _BASE["launches"]


def seg_lists():
    """[[cases]]: three lists for k_small_msm_seg that mix the widths.  Each begins with a sum that cancels completely next to a
    finite one, with two sums where the last term of the first is the negation of the first term of the second and with a sum
    of w / 2 + 1 terms for every width w; the cases follow, dealt in turn.  The last list leaves idle lanes in its last wave."""
    if "seg" not in _BASE:
        b = _builder()
        heads = []
        for n, (lc, lf, la, lb) in enumerate(((2, 3, 5, 9), (22, 17, 33, 64), (64, 1, 17, 2))):
            cancel = [x for i in range(lc // 2) for x in [(base_point(1900 + 40 * n + i), 3 + i), (pm.neg(base_point(1900 + 40 * n + i)), 3 + i)]]
            g, k = b.point(), b.scalar()
            heads.append([Case("list %d: %d terms that cancel" % (n, lc), cancel, both=True), Case("list %d: a finite sum of %d beside it" % (n, lf), b.random_terms(lf)),
                          Case("list %d: %d terms, the last one P" % (n, la), b.random_terms(la - 1) + [(g, k)]),
                          Case("list %d: %d terms, the first one -P" % (n, lb), [(pm.neg(g), k)] + b.random_terms(lb - 1))])
            assert heads[-1][0].canon is None and heads[-1][1].canon is not None
            # every width in every list: w / 2 + 1 terms for w = 2 .. 64, and one term
            heads[-1] += [Case("list %d: ordinary, %d terms" % (n, L), b.random_terms(L)) for L in (3, 33, 1, 9, 2, 17, 5)]
        order = sorted(range(len(b.cases)), key=lambda i: (i * 0x9E3779B1) % 1000003)  # a fixed shuffle: the widths mix
        lists = [heads[n] + [b.cases[i] for i in order[n::3]] for n in range(3)]
        while sum(seg_width(c.K) for c in lists[2]) % 64 == 0:
            lists[2].append(Case("one more term: idle lanes in the last wave", b.random_terms(1)))
        _BASE["seg"] = lists
    return _BASE["seg"]


def all_sum_cases():
    """every Case of the launches and the lists, once"""
    seen, out = set(), []
    for c in [c for _, launch in batch_launches() for c in launch] + [c for l in seg_lists() for c in l]:
        if id(c) not in seen:
            seen.add(id(c))
            out.append(c)
    return out


def check_sums(got_jac, cases):
    """sum s of a launch against its case, on orc.point_canonical -> failing (index, name)"""
    got_jac = np.asarray(got_jac, dtype=np.uint64).reshape(-1, 12)
    assert got_jac.shape[0] == len(cases)
    return [(s, c.name) for s, c in enumerate(cases) if orc.point_canonical(got_jac[s]) != c.canon]


def describe(bad, limit=8):
    return "%d wrong; first (index, case): %s" % (len(bad), bad[:limit])


# ---------------------------------------------------------------------------------------------------- URS runs
URS_FIRST = [2, (1 << 32) - 3, (1 << 63) + 5]
URS_STRIDE = [1, 3, 1 << 33]
URS_N = [1, 3, 255, 257, 1025]


def urs_triples():
    out = [(f, s, n) for f in URS_FIRST for s in URS_STRIDE for n in URS_N]
    assert all(f + (n - 1) * s < 1 << 64 for f, s, n in out)
    return out


def urs_index(first, stride, i):
    return first + i * stride


def urs_expected(first, stride, n):
    """orc.urs_affine over the run's indices (index by index where the stride is not 1), n x 8 affine words"""
    key = ("urs", first, stride)
    if key not in _BASE or _BASE[key].shape[0] < n:
        top = max(URS_N + [n])
        _BASE[key] = orc.urs_affine(first, top) if stride == 1 else np.concatenate([orc.urs_affine(first + i * stride, 1) for i in range(top)])
    return _BASE[key][:n]


def urs_model_positions(first, stride, n):
    """the positions of a run also held against pallas_model.get_generator_hash (hashlib's SHA3): the first, the last, the indices
    either side of 2^32"""
    pos = {0, n - 1}
    for i in range(n - 1):
        if urs_index(first, stride, i) < 1 << 32 <= urs_index(first, stride, i + 1):
            pos.update((i, i + 1))
    return sorted(pos)


def check_urs(got, first, stride, n):
    """a derived key against orc.urs_affine, word for word -> failing (position, index)"""
    got, want = np.asarray(got, dtype=np.uint64).reshape(-1, 8), urs_expected(first, stride, n)
    assert got.shape == want.shape
    return [(int(i), urs_index(first, stride, int(i))) for i in np.nonzero((got != want).any(axis=1))[0]]


# ---------------------------------------------------------------------------------------------------- the host build
HOST_TBL_E = 4  # msm_kernels.hpp TBL_E, which a host program cannot include: tests/test_small_msm_host.py holds the two together


def build_host(tmp_dir, csrc=None):
    """compile tests/native/small_msm_host.cpp with ASan + UBSan against the headers of csrc -> (exe, None) or (None, reason to skip)"""
    if shutil.which("g++") is None or not os.path.isdir("/opt/rocm/include"):
        return None, "no g++ / HIP headers"
    exe = os.path.join(str(tmp_dir), "small_msm_host")
    cmd = ["g++", "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
           "-I/opt/rocm/include", "-I", csrc or os.path.join(ROOT, "halo-accumulation_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "small_msm_host.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "sanitize" in b.stderr:
        return None, "sanitizer runtime not installed"
    assert b.returncode == 0, b.stderr[-2000:]
    return exe, None


def run_host(exe, tmp_dir, cases, groups):
    """every case and group through the sanitizer build -> ([(sum in k_batch_small_msm's order, sum in k_small_msm_seg's order)],
    [m x 8 affine words]); any sanitizer report fails.  Dealt to as many processes as there are CPUs (at most 16); a process runs
    the ladder once for each different term of its cases."""
    cpus = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 4
    nproc = max(1, min(16, cpus))
    procs = []
    for k in range(nproc):
        mine, grp = list(range(k, len(cases), nproc)), list(range(k, len(groups), nproc))
        index, rows = {}, []
        for i in mine:
            for t in cases[i].terms:
                if t not in index:
                    index[t] = len(rows)
                    rows.append(np.concatenate([tc.aff_words(t[0]), tc.scalar_words([t[1]])[0]]))
        fin, fout = os.path.join(str(tmp_dir), "smsm_%d.in" % k), os.path.join(str(tmp_dir), "smsm_%d.out" % k)
        with open(fin, "wb") as f:
            np.array([len(rows), len(mine), len(grp)], dtype=np.uint32).tofile(f)
            if rows:
                np.ascontiguousarray(np.stack(rows), dtype=np.uint64).tofile(f)
            for i in mine:
                np.array([cases[i].K] + [index[t] for t in cases[i].terms], dtype=np.uint32).tofile(f)
            for g in grp:
                np.array([groups[g].m], dtype=np.uint32).tofile(f)
                np.ascontiguousarray(groups[g].jac, dtype=np.uint64).tofile(f)
        procs.append((subprocess.Popen([exe, fin, fout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True), fin, fout, mine, grp))
    sums, affs = [None] * len(cases), [None] * len(groups)
    for p, fin, fout, mine, grp in procs:
        so, se = p.communicate(timeout=900)
        assert p.returncode == 0 and so.startswith("ok ") and "runtime error" not in se and "Sanitizer" not in se, so + se[-3000:]
        flat = np.fromfile(fout, dtype=np.uint64)
        at = 0
        for i in mine:
            sums[i] = (flat[at:at + 12], flat[at + 12:at + 24])
            at += 24
        for g in grp:
            affs[g] = flat[at:at + 8 * groups[g].m].reshape(-1, 8)
            at += 8 * groups[g].m
        assert at == flat.size
        os.remove(fin)
        os.remove(fout)
    return sums, affs
