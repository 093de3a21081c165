"""Cases for the builds of the MSM's fixed-base tables (msm_table.hip k_table_all_shifts, k_table_step), read back entry by entry
through halo_dev_table_read (tests/test_gpu_table_build.py); the checkers test themselves in tests/test_table_cases_cpu.py.  Not a
test module.  Plain Python and numpy over pallas_model and orc: importable without a GPU.

The key: an ordinary key with exceptional points written in where the build kernels' structure has its edges (exceptional_key).
    k_table_all_shifts   a block owns 4096 points, point i = 4096 block + 256 e + tid, e < 16: a lane multiplies up the Z's of its 16
                         points, lane 0 inverts the block's product once per row, every lane unwinds -- an infinite point enters
                         the product as Z = 1 in BOTH passes, or the other 4095 points of the block get a wrong 1 / Z
    k_table_step         point i = t + e stride, e < 4, stride = 256 ceil(ceil(n / 4) / 256): a lane t brings its four points back
                         to affine with one inversion, a point past the end is a padding infinity
The references: big-integer arithmetic on the affine doubling relation (check_doubling_rows: no inversion, no device value, every
entry) and the oracle's orc_point_mul (check_shift_rows, on a stated set of columns).  Both are exact: no tolerance anywhere.
"""
import re

import numpy as np

import orc
import pallas_model as pm

P = pm.P
R = pm.R_ORDER
RINV = pow(pm.MONT_R, -1, P)
ALLS_LANES, ALLS_E = 256, 16      # k_table_all_shifts: lanes per block, points per lane
STEP_E = 4                        # k_table_step: points per lane (TBL_E)
N_A = 4096 + 260                  # key A: a full block, then a partial one (e = 0 full, e = 1 with four live lanes)
RUN = 64                          # length of the runs of copies: one wave's worth of indices
ORIGINAL, COPIES, NEGATIONS = 89, 90, 170   # G[89]; G[90 .. 154) = G[89]; G[170 .. 234) = -G[89]: neither run aligned to 64


def step_stride(n):
    """the grid stride of k_table_step over n points"""
    return 256 * (((n + STEP_E - 1) // STEP_E + 255) // 256)


# ---------------------------------------------------------------------------------------------------- words
def _int(words):
    return sum(int(w) << (64 * i) for i, w in enumerate(words))


def _words(v):
    return [(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]


def aff_words(pt):
    """a point of pallas_model (None = infinity) -> 8 affine words, Montgomery form, (0, 0) = infinity"""
    if pt is None:
        return np.zeros(8, dtype=np.uint64)
    return np.array(pm.to_mont_limbs(pt[0], P) + pm.to_mont_limbs(pt[1], P), dtype=np.uint64)


def negated(aff):
    """(x, -y) on affine words: the Montgomery words of -y are p - y"""
    o = np.array(aff, dtype=np.uint64)
    if o.any():
        o[4:8] = _words((P - _int(o[4:8])) % P)
    return o


def raw_coordinates(rows):
    """rows: (..., 8) uint64 -> flat list of (X, Y) Python integers, the words as they are (still in Montgomery form)"""
    b = np.ascontiguousarray(rows, dtype="<u8").tobytes()
    f = int.from_bytes
    return [(f(b[k:k + 32], "little"), f(b[k + 32:k + 64], "little")) for k in range(0, len(b), 64)]


# ---------------------------------------------------------------------------------------------------- the key
def exceptional_key(base_affine, layout="all_shifts", pairs=(1000, 1500)):
    """n x 8 affine words of an ordinary key (distinct finite points) -> (key, classes): the same key with exceptional points
    planted, classes[i] = the name of what sits at index i ("plain" everywhere else).  layout "all_shifts": the positions of
    k_table_all_shifts (i = 4096 block + 256 e + tid); "step": the same classes on the stripes of k_table_step (i = t + e stride).
    pairs: the two originals whose copy and negation sit one stride further on, in the same lane (a key below 1500 + stride points
    names smaller ones)."""
    key = np.array(base_affine, dtype=np.uint64).reshape(-1, 8)
    n = key.shape[0]
    assert key.any(axis=1).all() and len({r.tobytes() for r in key}) == n, "the base key is distinct finite points"
    if layout == "all_shifts":
        stride, E = ALLS_LANES, ALLS_E
    else:
        assert layout == "step"
        stride, E = step_stride(n), STEP_E
    span = stride * E
    assert n > span // E * (E - 1) + 64 and n % 4 == 0
    classes = ["plain"] * n

    def plant(i, name, words=None):
        assert 0 <= i < n and classes[i] == "plain", (i, name, classes[i])
        classes[i] = name
        key[i] = 0 if words is None else words

    at = lambda e, lane: stride * e + lane  # (block 0)
    plant(at(0, 3), "inf at e = 0")
    plant(at(E - 1, 20), "inf at e = %d, the last of its lane" % (E - 1))
    plant(at(E // 2, 41), "inf at e = %d" % (E // 2))
    for e in range(E):
        if at(e, 7) < n:
            plant(at(e, 7), "inf, every point of lane 7 (e = %d)" % e)
    e0 = max(1, E // 3)
    plant(at(e0, 0), "inf on lane 0 (e = %d)" % e0)
    plant(n - 1, "inf at n - 1, the last live lane")
    if layout == "all_shifts":
        # lane 0 of the partial block: an infinity, a live point, fourteen points past the end
        assert n > span and n - span < span
        plant(span, "inf at the first point of the partial block")
    else:
        # the partial stripe e = 3: its first point, and a lane whose e = 3 is past the end with an infinity among its live points
        last = stride * (E - 1)
        assert last < n < span
        plant(last, "inf at the first point of the partial stripe")
        plant(n - last + 10, "inf at e = 0 of a lane that pads")
    # a run of 64 copies of one point and a run of 64 copies of its negation
    for k in range(RUN):
        plant(COPIES + k, "copy of G[%d]" % ORIGINAL, key[ORIGINAL])
        plant(NEGATIONS + k, "negation of G[%d]" % ORIGINAL, negated(key[ORIGINAL]))
    assert COPIES % 64 and NEGATIONS % 64
    classes[ORIGINAL] = "original of the runs"
    # two pairs that share a lane
    for a, sign in ((pairs[0], 1), (pairs[1], -1)):
        plant(a + stride, "%sG[%d], same lane" % ("-" if sign < 0 else "", a), key[a] if sign > 0 else negated(key[a]))
        assert classes[a] == "plain"
        classes[a] = "original of a pair"
    for w in range(0, n, 64):  # every wave of 64 indices keeps plain points
        assert "plain" in classes[w:w + 64], w
    return np.ascontiguousarray(key), classes


def planted(classes):
    """the indices that are not plain"""
    return [i for i, c in enumerate(classes) if c != "plain"]


def original_of(classes):
    """{index of a copy or a negation: index of its original}"""
    out = {}
    for i, c in enumerate(classes):
        m = re.search(r"G\[(\d+)\]", c)
        if m:
            out[i] = int(m.group(1))
    return out


def is_infinite(classes):
    return [c.startswith("inf") for c in classes]


# ---------------------------------------------------------------------------------------------------- checkers
def _cls(classes, i):
    return classes[i] if classes is not None else "?"


def check_row0(table_row0, key, classes=None):
    """row 0 of a table is the key, word for word -> failing (0, index, class)"""
    a, b = np.asarray(table_row0, dtype=np.uint64).reshape(-1, 8), np.asarray(key, dtype=np.uint64).reshape(-1, 8)
    assert a.shape == b.shape
    return [(0, int(i), _cls(classes, i)) for i in np.nonzero((a != b).any(axis=1))[0]]


def check_doubling_rows(prev_rows, next_rows, first_row=1, classes=None, counted=None):
    """next_rows[k][i] = 2 prev_rows[k][i] for every k and i, by the affine doubling law over Python integers (no inversion).  Both
    are (rows, n, 8) affine words; next_rows[0] is row `first_row` of the table.  An infinite entry doubles to exactly (0, 0); a
    finite (x, y) -> (x', y') must have both coordinates canonical, y'^2 = x'^3 + 5, (x' + 2 x)(2 y)^2 = 9 x^4 and
    (y' + y) 2 y = 3 x^2 (x - x').  y != 0 on this curve (no point of order 2), so the last two fix x' and y': with row 0 equal
    to the key every row is exact by induction.  -> every failing (row, index, class); counted[0] += the entries checked."""
    prev_rows, next_rows = np.asarray(prev_rows, dtype=np.uint64), np.asarray(next_rows, dtype=np.uint64)
    assert prev_rows.shape == next_rows.shape and prev_rows.ndim == 3 and prev_rows.shape[2] == 8
    rows, n = prev_rows.shape[:2]
    plain = lambda row: [(X, Y, X * RINV % P, Y * RINV % P) for X, Y in raw_coordinates(row)]  # out of Montgomery form
    bad, nx = [], None
    for k in range(rows):
        # (consecutive rows of one table: the row just checked is the next one's `prev`)
        pv = nx if k and np.array_equal(prev_rows[k], next_rows[k - 1]) else plain(prev_rows[k])
        nx = plain(next_rows[k])
        for i in range(n):
            X, Y, x, y = pv[i]
            X2, Y2, x2, y2 = nx[i]
            if X == 0 and Y == 0:
                ok = X2 == 0 and Y2 == 0
            elif (X2 == 0 and Y2 == 0) or X2 >= P or Y2 >= P:
                ok = False
            else:
                xx = x * x
                ok = ((y2 * y2 - x2 * x2 * x2 - 5) % P == 0 and ((x2 + 2 * x) * 4 * y * y - 9 * xx * xx) % P == 0
                      and ((y2 + y) * 2 * y - 3 * xx * (x - x2)) % P == 0)
            if not ok:
                bad.append((first_row + k, i, _cls(classes, i)))
        if counted is not None:
            counted[0] += n
    return bad


def _jac(aff):
    j = np.zeros(12, dtype=np.uint64)
    orc.lib().orc_affine_to_jac(orc.ptr(np.ascontiguousarray(aff, dtype=np.uint64)), orc.ptr(j))
    return j


def check_shift_rows(key, rows, c, columns, classes=None, counted=None):
    """rows[w][i] = 2^(c w) key[i] for every row w of `rows` ((W, n, 8) affine words, row 0 included) and every i of `columns`: the
    oracle's orc_point_mul by the scalar 2^(c w), compared on orc.affine_canonical -> every failing (row, index, class)"""
    key, rows = np.asarray(key, dtype=np.uint64).reshape(-1, 8), np.asarray(rows, dtype=np.uint64)
    assert rows.ndim == 3 and rows.shape[1:] == key.shape
    L = orc.lib()
    scal = [orc.fr_to_mont(pow(2, c * w, R)) for w in range(rows.shape[0])]
    bad = []
    for i in columns:
        g = _jac(key[i])
        for w in range(rows.shape[0]):
            o = np.zeros(12, dtype=np.uint64)
            L.orc_point_mul(orc.ptr(g), orc.ptr(scal[w]), orc.ptr(o))
            if orc.affine_canonical(rows[w, i]) != orc.point_canonical(o):
                bad.append((w, int(i), _cls(classes, i)))
            if counted is not None:
                counted[0] += 1
    return bad


def step_columns(n, classes):
    """the columns check_shift_rows takes for a k_table_step table: every planted index, the first and last 8 indices of each of
    the four stripes [stride e, stride (e + 1)), the last 8 of the key"""
    s = step_stride(n)
    cols = set(planted(classes))
    for e in range(STEP_E):
        lo, hi = s * e, min(s * (e + 1), n)
        cols.update(range(lo, lo + 8))
        cols.update(range(hi - 8, hi))
    cols.update(range(n - 8, n))
    return sorted(cols)


def describe(bad, limit=12):
    """a failure message: how many, which classes, the first few"""
    by = {}
    for _, _, c in bad:
        by[c] = by.get(c, 0) + 1
    return "%d wrong entries; by class %s; first (row, index, class): %s" % (len(bad), by, bad[:limit])


# ---------------------------------------------------------------------------------------------------- scalars
def scalar_words(vals):
    """Python integers below 2^256 -> (n, 4) uint64, plain (scalars_are_mont = 0)"""
    b = b"".join(int(v).to_bytes(32, "little") for v in vals)
    return np.frombuffer(b, dtype="<u8").reshape(-1, 4).astype(np.uint64)


def scalar_mont(vals):
    """the same scalars mod r in Montgomery form: what orc.msm_affine takes"""
    return scalar_words([(int(v) % R) * pm.MONT_R % R for v in vals])


def scalar_sets(n, classes, seed):
    """name -> n Python integers (below 2^256; `top_2_254` has values in [r, r + 2^40): the launches take them unreduced)"""
    rng = pm.SplitMix64(seed)
    u64 = lambda: rng.next_u64()
    out = {}
    out["uniform"] = [(u64() | u64() << 64 | u64() << 128 | (u64() & ((1 << 62) - 1)) << 192) for _ in range(n)]
    # every copy of the repeated point meets its twins in one bucket: P + P at the head of a chain, then -P runs that cancel
    out["equal"] = [0x1234567890ABCDEF0FEDCBA987654321 * ((1 << 120) + 12345) % R] * n
    p = list(out["uniform"])
    for i, src in original_of(classes).items():
        p[i] = p[src]
    out["paired"] = p
    out["zero"] = [0] * n
    edge = [R - 1 - (u64() & ((1 << 40) - 1)) for _ in range(48)] + [R + (u64() & ((1 << 40) - 1)) for _ in range(14)] + [1 << 254, (1 << 254) + 1]
    out["top_2_254"] = [edge[u64() % 64] for _ in range(n)]
    one = [0] * n
    one[[i for i, c in enumerate(classes) if c.startswith("inf at e = 0")][0]] = out["uniform"][0] | 1
    out["one_on_infinity"] = one
    return out


SCALAR_SETS = ["uniform", "equal", "paired", "zero", "top_2_254", "one_on_infinity"]
INFINITE_RESULT = {"zero", "one_on_infinity"}
