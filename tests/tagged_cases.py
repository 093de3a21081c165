"""Cases for the tagged two-set table launch (MsmBatch::tagged, msm_table.hip: ONE canonical scalar array whose bit 255 names the
bucket set of point i, run over the c = 20 table with 2 x 2^19 buckets), asked for directly through halo_dev_msm_tagged
(tests/test_gpu_tagged_launch.py); the generators check themselves in tests/test_tagged_cases_cpu.py.  Not a test module.  Plain
Python and numpy over pallas_model, orc, table_cases and window_cases: importable without a GPU.

The reference is the oracle alone: want[t] = orc.msm_affine(key[off : off + n], the values whose tag is t, zero elsewhere) -- exact,
no tolerance anywhere.  What the launch is asked:
    tag patterns      all 0, all 1 (one whole set empty: 512 empty coarse ranges, window sums of infinities only), alternating, the
                      open's own first half 0 / second half 1, random
    scalar sets       table_cases.scalar_sets reduced below r, the edges of k_tmsm_recode's top-window spread s + (i mod 31) r at every
                      residue under both tags (edge_set), buckets of exactly kmax and kmax + 1 entries in each set (task_len_edge), a
                      coarse run of exactly TBL_STAGE entries in one set beside one of TBL_STAGE + 1 in the other (stage_edge)
    planted launches  the "fixed" row / column launches of window_cases, one in each set (planted_pairs), with the additions they
                      meet counted per set (planted_counts)
tagged_digits restates the recode (strip the tag, spread, signed 20-bit digits) ONLY to recount what the generators claim."""
import numpy as np

import orc
import pallas_model as pm
import table_cases as tc
import window_cases as wc

R = pm.R_ORDER
TAG = 1 << 255
C, W, B = 20, 13, 1 << 19           # the c = 20 plan: window bits, windows, buckets per set
FBITS, RANGES = 10, 512             # a coarse range is 1024 buckets: 512 ranges per set
SPREAD = 31                         # k_tmsm_recode: k = i mod 31 copies of r on a scalar with a non-empty top window
TBL_STAGE, TBL_TILE = 35840, 8192   # msm_kernels.hpp / msm_table.hip
KMAXES = (8, 16, 32, 64)
N_M = 160004                        # key M: chunk_len = 8424 > TBL_TILE, a shorter last chunk, 13 n <= 16 * 131072 (task length 16)
PATTERNS = ("all0", "all1", "alternating", "halves", "random")
ASYMMETRIC = PATTERNS[2:]           # both sets live


# ---------------------------------------------------------------------------------------------------- tags
def tags(pattern, n, seed=0x746167):
    """n tags (0 / 1) of a named pattern"""
    if pattern == "all0":
        return [0] * n
    if pattern == "all1":
        return [1] * n
    if pattern == "alternating":
        return [i & 1 for i in range(n)]
    if pattern == "halves":  # L's scalars sit on the first half of the points, R's on the second
        return [int(i >= n // 2) for i in range(n)]
    assert pattern == "random"
    rng = pm.SplitMix64(seed)
    return [int(rng.next_u64() >> 63) for _ in range(n)]


def split(values, tg):
    """canonical values below r and their tags -> (the tagged array, n x 4 words with bit 255 = tag; [the values of set 0 with zeros
    elsewhere, those of set 1])"""
    assert len(values) == len(tg) and all(0 <= v < R for v in values) and set(tg) <= {0, 1}
    tagged = tc.scalar_words([v | (TAG if t else 0) for v, t in zip(values, tg)])
    return tagged, [[v if t == s else 0 for v, t in zip(values, tg)] for s in (0, 1)]


def want(key, values, tg, off=0):
    """the oracle's two sums over key[off : off + n] -> [12 Jacobian words as a list] x 2"""
    pts = np.ascontiguousarray(np.asarray(key, dtype=np.uint64).reshape(-1, 8)[off:off + len(values)])
    return [orc.msm_affine(pts, tc.scalar_mont(m)).tolist() for m in split(values, tg)[1]]


# ---------------------------------------------------------------------------------------------------- the recode, restated
def tagged_digits(word, i):
    """k_tmsm_recode's tagged branch for the 256-bit word at index i of its launch -> (set, [(magnitude, negative)] x 13): the tag
    is stripped, a value with a non-empty top window of at most 16384 takes (i mod 31) r on top, then window_cases.recode_digits"""
    st, s = word >> 255, word & (TAG - 1)
    top = s >> 240
    if 0 < top <= 16384:
        s += (i % SPREAD) * R
    d = wc.recode_digits(s, C)
    assert len(d) == W and all(m <= B for m, _ in d)
    return st, d


def bucket_counts(values, tg):
    """{bucket of the whole launch (set * B + magnitude - 1): entries} over all 13 windows"""
    out = {}
    for i, (v, t) in enumerate(zip(values, tg)):
        st, d = tagged_digits(v | (TAG if t else 0), i)
        for m, _ in d:
            if m:
                out[st * B + m - 1] = out.get(st * B + m - 1, 0) + 1
    return out


def range_counts(counts):
    """entries per coarse range of the launch (1024 ranges: bucket >> 10)"""
    out = {}
    for b, k in counts.items():
        out[b >> FBITS] = out.get(b >> FBITS, 0) + k
    return out


# ---------------------------------------------------------------------------------------------------- scalar sets
EDGE_VALUES = []
for _v in ((1 << 240) - 1, 1 << 240, (1 << 240) + 1, (16384 << 240) - 1, 16384 << 240, (16384 << 240) + 12345, R - 1, (1 << 254) - 1, 1 << 254,
           (1 << 254) + 1, (1 << 20) - 1, 1 << 19, (1 << 19) + 1, (1 << 239) + (1 << 19)):
    if _v not in EDGE_VALUES:  # (16384 << 240 is 2^254: the list of test_msm_table_top_window_edges names two values twice)
        EDGE_VALUES.append(_v)
assert all(v < R for v in EDGE_VALUES)
EDGE_BLOCK = 2 * SPREAD  # 62 consecutive indices: every residue mod 31 at an even and at an odd index


def edge_set(n):
    """the edges of the spread rule: value j of EDGE_VALUES at the indices i with (i / 62) mod 12 = j -- blocks of 62 indices, so
    every value meets every residue of i mod 31 under both tags of the alternating pattern, and whole blocks in either half"""
    return [EDGE_VALUES[(i // EDGE_BLOCK) % len(EDGE_VALUES)] for i in range(n)]


def edge_coverage(values, tg):
    """{(value, residue of i mod 31, tag)} that occur"""
    return {(v, i % SPREAD, t) for i, (v, t) in enumerate(zip(values, tg))}


def task_len_edge(tg, seed=14):
    """buckets of exactly kmax and kmax + 1 entries side by side for kmax = 8, 16, 32, 64, all else zero -- in EACH set that has
    the room: a bucket's entries are the points of one tag, so a set gets its own pairs on indices of its own (digits 700 / 701,
    1000 / 1001, 3000 / 3001, 5000 / 5001 on row 0, as tests/test_gpu_table_tasks.py edge_set)"""
    n = len(tg)
    e = [0] * n
    rng = np.random.default_rng(seed)
    need = sum(2 * k + 1 for k in KMAXES)
    for st in (0, 1):
        where = [i for i in range(n) if tg[i] == st]
        if len(where) < need:
            assert not where, "a set with points but no room for its pairs"
            continue
        where = [where[j] for j in rng.permutation(len(where))]
        at = 0
        for kmax, digit in zip(KMAXES, (700, 1000, 3000, 5000)):
            for i in where[at:at + kmax]:
                e[i] = digit
            at += kmax
            for i in where[at:at + kmax + 1]:
                e[i] = digit + 1
            at += kmax + 1
    return e


STAGE_RANGES = (5, 9)  # the coarse range of set 0 and the one of set 1


def stage_edge(n, swapped=False):
    """-> (values, tags): coarse range 5 of set 0 holds exactly TBL_STAGE entries (the largest staged run) and range 9 of set 1
    TBL_STAGE + 1 (the smallest unstaged one); swapped: the other way round.  Single digits on row 0, dealt round over the range's
    1024 buckets: 35 entries a bucket (36 in one), at most a task of length 64 each.  Set 0 on the even indices, set 1 on the odd."""
    v, tg = [0] * n, [i & 1 for i in range(n)]
    for st in (0, 1):
        count = TBL_STAGE + (1 if (st == 1) != swapped else 0)
        assert 2 * count <= n
        for j in range(count):
            v[2 * j + st] = (STAGE_RANGES[st] << FBITS) + j % (1 << FBITS) + 1  # the digit bucket + 1
    return v, tg


def key_a_sets(n, classes, seed):
    """name -> n canonical values: table_cases.scalar_sets with the unreduced members of top_2_254 replaced by reduced ones (R - 1 - k,
    2^254, 2^254 + 1 stay), and the edge set.  (task_len_edge depends on the tags: task_len_edge(tags))"""
    out = dict(tc.scalar_sets(n, classes, seed))
    low = sorted({v for v in out["top_2_254"] if v < R})
    assert {1 << 254, (1 << 254) + 1} <= set(low) and len(low) >= 40
    out["top_2_254"] = [v if v < R else low[i % len(low)] for i, v in enumerate(out["top_2_254"])]
    out["edge"] = edge_set(n)
    assert all(0 <= v < R for vs in out.values() for v in vs)
    return out


KEY_A_SETS = tc.SCALAR_SETS + ["edge", "task_len_edge"]


def key_m_sets(n, seed):
    """the sets of the larger key: uniform, all-equal (runs far above TBL_STAGE in either set: the unstaged fine sort), zero, edge"""
    rng = pm.SplitMix64(seed)
    u64 = lambda: rng.next_u64()
    out = {"uniform": [(u64() | u64() << 64 | u64() << 128 | (u64() & ((1 << 62) - 1)) << 192) for _ in range(n)],
           "equal": [0x1234567890ABCDEF0FEDCBA987654321 * ((1 << 120) + 12345) % R] * n, "zero": [0] * n, "edge": edge_set(n)}
    return out


KEY_M_SETS = ["uniform", "equal", "zero", "edge", "task_len_edge"]


# ---------------------------------------------------------------------------------------------------- planted window sums
FIXED = wc.PLAN_OF_LAYOUT["fixed"]
RUN_EQUAL = {1: (1, 3), 0: (1, 2)}  # {block: (S, T)} in units of g: the running sum of block 1 meets the equal S of block 0


class Pair:
    """two planted launches of window_cases over wc.table_key() in ONE tagged array: `first` in set 0, `second` in set 1.  An index
    both want goes to the first; the second takes another point of the key with the same multiple of G instead (the key repeats
    its background 22 times and holds 1400 points +g G and 500 points -g G), so every bucket of either set holds what its launch
    planted: values = [set 0, set 1] for check_window_sums, cases likewise."""

    def __init__(self, name, ks, first, second, same_words=True):
        self.name, self.same_words = name, same_words
        n = len(ks)
        self.scalars, self.tags = list(first.scalars), [0] * n
        free = {}
        for j in range(n - 1, -1, -1):
            if not first.scalars[j] and not second.scalars[j]:
                free.setdefault(ks[j], []).append(j)
        for i, s in enumerate(second.scalars):
            if s:
                j = i if not first.scalars[i] else free[ks[i]].pop()
                assert not self.scalars[j]
                self.scalars[j], self.tags[j] = s, 1
        self.values = [first.values, second.values]
        self.cases = [first.cases, second.cases] if first.cases or second.cases else None
        self.launches = (first, second)
        got = [{}, {}]
        for i, (s, t) in enumerate(zip(self.scalars, self.tags)):
            if s and ks[i]:
                got[t][s - 1] = got[t].get(s - 1, 0) + ks[i]
        assert [{b: x for b, x in g.items() if x} for g in got] == self.values, name


def planted_pairs():
    """-> (key multiples, [Pair]): the four families of "fixed" launches, each launch once in set 0 and once in set 1, beside a
    different launch.  The launches of k_rc_mid fill the key's background between them, so each of them sits beside the structure
    launch of k_msm_reduce_rc (which takes the +-g points only) and the structure launch beside each of them; the host's launches
    go round in a ring, each beside its neighbour."""
    ks, rc_mid = wc.slide_rc_mid_launches("fixed")
    _, structure, cells = wc.slide_structure_launch("fixed")
    structure.cells = cells
    pairs = []
    for k, l in enumerate(rc_mid):
        pairs.append(Pair("rc_mid %d | structure" % k, ks, l, structure))
        pairs.append(Pair("structure | rc_mid %d" % k, ks, structure, l))
    host = wc.slide_host_launches("fixed")[1]
    for k, (name, l) in enumerate(host):
        other = host[(k + 1) % len(host)]
        pairs.append(Pair("%s | %s" % (name, other[0]), ks, l, other[1]))
    extra = wc.extra_host_launches("fixed")[1]
    # (window_cases meets run+=S P+P under its other shapes only: two blocks of equal plain sums, over the columns and over the rows)
    cells = wc._pairs(RUN_EQUAL)
    extra += [("cols: run+=S P+P", wc.cells_launch("fixed", cells)), ("rows: run+=S P+P", wc.cells_launch("fixed", {(c, r): m for (r, c), m in cells.items()}))]
    for k, (name, l) in enumerate(extra):  # (cells of several points: buckets of several tasks, placed by the sort's atomics)
        other = extra[(k + 1) % len(extra)]
        pairs.append(Pair("%s | %s" % (name, other[0]), ks, l, other[1], same_words=False))
    return ks, pairs


RC_SITES = ([("k_msm_reduce_rc", "%s step" % nm) for nm in ("col", "row")] + [("k_msm_reduce_rc", "col tree/%d" % (16 >> t)) for t in range(5)] +
            [("k_msm_reduce_rc", "row tree/%d" % (32 >> t)) for t in range(6)])
HOST_SITES = [(wc.K_HOST, "%s %s" % (nm, s)) for nm in ("cols", "rows") for s in ("t+=T", "run+=S", "tot+=run", "t+tot")] + [(wc.K_HOST, "rows - plain"),
                                                                                                                      (wc.K_HOST, "cols + rows")]


def planted_sites():
    """every (kernel, site) behind the bucket kernel of a tagged launch: the lanes' steps and trees of k_msm_reduce_rc (512 x 1024, 16
    buckets a lane), one block of k_rc_mid, the host's row / column combination of the fixed windows"""
    return RC_SITES + wc.sites(wc.RC_MID_PLAN) + HOST_SITES


def planted_counts(pairs=None):
    """[{(kernel, site, class): count} for set 0, for set 1]: what the launches of planted_pairs meet in each set, by the models of
    window_cases (the structure launch through model_reduce_rc, a k_rc_mid block through the counts its case was built with, every
    launch through model_host_rc)"""
    pairs = planted_pairs()[1] if pairs is None else pairs
    recs = [wc.IntRec(), wc.IntRec()]
    for pair in pairs:
        for rec, l in zip(recs, pair.launches):
            if getattr(l, "cells", None):
                wc.model_reduce_rc(rec, l.cells, FIXED["lg_rows"], FIXED["lg_cols"], 16)
            for _, case in l.cases or []:
                rec.merge(wc.IntRec.of(case.counts))
            assert abs(wc.model_host_rc(rec, FIXED, l.values)) < wc.LIMIT
    return [dict(r.counts) for r in recs]


def uncovered(counts):
    """the (set, kernel, site, class) cells of the coverage table that are empty"""
    return [(s, k, site, cl) for s in (0, 1) for k, site in planted_sites() for cl in wc.EDGE if not counts[s].get((k, site, cl))]


def format_counts(counts):
    lines = []
    for k, site in planted_sites():
        lines.append("%-18s %-14s %s" % (k, site, "   ".join("%s %s" % (cl, "/".join(str(counts[s].get((k, site, cl), 0)) for s in (0, 1))) for cl in wc.EDGE)))
    return "\n".join(["(kernel, site): class set 0 / set 1"] + lines)
