"""Cases for the MSM's window sums: the kernels behind the bucket kernel (msm_buckets.hip k_msm_combine, k_msm_reduce1 with
wave_weighted_sum, k_msm_reduce_rc; smsm.hip k_smsm_reduce, k_smsm_final and k_rc_mid with block_weighted_sum) and the host's
msm_combine_member, read back record by record through halo_dev_msm_window_sums (tests/test_gpu_window_sums.py); the models and
checkers test themselves in tests/test_window_cases_cpu.py.  Not a test module.  Plain Python and numpy over pallas_model and orc:
importable without a GPU.

The key: small signed multiples k_i G of ONE point of the URS (multiples_key; k_i = 0 is the infinity (0, 0)).  Every bucket value,
partial, running sum and window sum is then an integer multiple of G, all of them far below 2^64 in magnitude while G has prime
order r ~ 2^254: two points are equal, opposite or infinite exactly when the integers are equal, opposite or zero.  Scalars with an
empty top window (general_scalars) keep k_msm_recode's top-window spread out of it; a scalar sum_w d_w 2^(c w), 1 <= d_w <= B,
puts its point into bucket d_w - 1 of every window w: one scalar array plants W - 1 independent windows.  A scalar d < 2^19 is one
digit on row 0 of the table plans (slide_scalar, fixed_scalar).

The schedules are restated here over integers (model_combine, model_reduce1 with model_wave_weighted_sum, model_smsm_reduce and
model_final with model_block_weighted_sum, model_reduce_rc, model_horner; one block of k_rc_mid is the plan "rc_mid") ONLY to
classify the additions a case meets -- P+P, P-P, inf+Q, Q+inf, inf+inf, dbl(inf), generic -- and to count them (coverage); the
case builder (build_cases) uses them to find bucket values that put a chosen class at a chosen site of a window, alone under that
window sum.  Never for an expected value: check_window_sums compares every record with m G for the m the DEFINITION of the record
gives (sum_b (b + 1) v_b, plain sums and (S, T) pairs where the form stores them), exactly, with no tolerance anywhere.

Built by the case builder, one window (or one block of k_rc_mid) per (site, class): every site of k_msm_reduce1 and k_smsm_final in
the general pipeline, of k_smsm_reduce and k_smsm_final in the small one over single-task buckets, of k_rc_mid.  Planted by hand,
with the model counting what they meet: k_msm_combine (combine_launch), the partial loop and the heavy-bucket pre-sum of
k_smsm_reduce (partials_launch, heavy_launch, strided_launch), k_msm_reduce_rc in its five shapes (structure_cells; small_key_batches for the 256 x
256 shape of the small-key plan, one member and batches), the host's Horner (horner_launch), its row / column forms
(slide_host_launches, extra_host_launches) and k_msm_reduce1 + k_smsm_final at 2^15 buckets per window (reduce1_launch);
planted_counts is the coverage table of the others.  Where a bucket has several tasks the entries are
all equal, or one odd entry is sized so that the class falls on a known level whichever task receives it: the sorts place the
entries of a bucket with atomics."""
import numpy as np

import orc
import pallas_model as pm
import table_cases as tc

R = pm.R_ORDER
CLASSES = ("P+P", "P-P", "inf+Q", "Q+inf", "inf+inf", "dbl(inf)", "generic")
EDGE = CLASSES[:4]           # the classes the coverage table must hold at every site
K_COMBINE, K_REDUCE1, K_FINAL, K_HOST = "k_msm_combine", "k_msm_reduce1", "k_smsm_final", "msm_combine_member"
K_SREDUCE, K_RCMID = "k_smsm_reduce", "k_rc_mid"
UNIT_KERNELS = (K_REDUCE1, K_SREDUCE, K_RCMID)   # their 64 lanes or quads are the units of a case; k_smsm_final's are the segments
SMSM_HEAVY = 4
LIMIT = 1 << 63              # every multiple that occurs stays below this in magnitude


# ---------------------------------------------------------------------------------------------------- multiples of G
_G = {}


def g_affine():
    """G: the first point of the URS, 8 affine words"""
    if "aff" not in _G:
        _G["aff"] = orc.urs_affine(2, 1)[0].copy()
        _G["jac"] = tc._jac(_G["aff"])
        _G["canon"] = {0: None}
    return _G["aff"]


def multiple(m):
    """m G as canonical coordinates (None = infinity), by the oracle's orc_point_mul (the scalar is m mod r); computed once per m"""
    g_affine()
    m = int(m)
    assert abs(m) < LIMIT, m
    if m not in _G["canon"]:
        o = np.zeros(12, dtype=np.uint64)
        orc.lib().orc_point_mul(orc.ptr(_G["jac"]), orc.ptr(orc.fr_to_mont(m % R)), orc.ptr(o))
        _G["canon"][m] = orc.point_canonical(o)
    return _G["canon"][m]


def g_model():
    """G as a point of pallas_model"""
    return multiple(1)


def multiples_key(n, ks):
    """key[i] = ks[i] G for i < len(ks), infinity behind: n x 8 affine words"""
    assert len(ks) <= n
    key, words = np.zeros((n, 8), dtype=np.uint64), {}
    for i, k in enumerate(ks):
        if k not in words:
            words[k] = tc.aff_words(multiple(k))
        key[i] = words[k]
    return key


# ---------------------------------------------------------------------------------------------------- scalars
def windows_of(c):
    return (256 + c - 1) // c


def general_scalars(c, digits):
    """digits[i] = {window: d} with 1 <= d <= 2^(c-1) and window <= W - 2 -> the Python integers sum_w d 2^(c w): point i lands in
    bucket d - 1 of each named window, positive, without a carry (k_msm_recode: a raw digit <= B stays as it is), and the top window
    stays empty (no spread)"""
    W, B = windows_of(c), 1 << (c - 1)
    out = []
    for dg in digits:
        s = 0
        for w, d in dg.items():
            assert 0 <= w <= W - 2 and 1 <= d <= B, (w, d)
            s |= d << (c * w)
        assert s < 1 << (c * (W - 1))
        out.append(s)
    return out


def recode_digits(s, c):
    """k_msm_recode + next_digit for a scalar whose top window is empty (no spread: k = 0): per window (magnitude, negative)"""
    W, B = windows_of(c), 1 << (c - 1)
    out, carry = [], 0
    for w in range(W):
        v = ((s >> (c * w)) & ((1 << c) - 1)) + carry
        if v > B:
            out.append(((1 << c) - v, 1))
            carry = 1
        else:
            out.append((v, 0))
            carry = 0
    return out


def slide_scalar(bucket):
    """sliding plan: the odd scalar 2 bucket + 1 < 2^20 is one digit on table row 0, in bucket `bucket` < 2^19"""
    assert 0 <= bucket < 1 << 19
    return 2 * bucket + 1


def slide_index(bucket, lg_rows=9, lg_cols=10):
    """where the sliding plan stores bucket (range, fine) = (bucket & (rows - 1), bucket >> lg_rows): row-major index"""
    return ((bucket & ((1 << lg_rows) - 1)) << lg_cols) + (bucket >> lg_rows)


def fixed_scalar(bucket):
    """fixed windows: the scalar bucket + 1 <= 2^19 is the digit of window 0 (table row 0), in bucket `bucket`"""
    assert 0 <= bucket < 1 << 19
    return bucket + 1


# ---------------------------------------------------------------------------------------------------- recorders
def classify(a, b):
    if a == 0:
        return "inf+inf" if b == 0 else "inf+Q"
    if b == 0:
        return "Q+inf"
    if a == b:
        return "P+P"
    if a == -b:
        return "P-P"
    return "generic"


class IntRec:
    """The group law over integers (multiples of G).  counts[(kernel, site, class)]; hits[(kernel, site)] = the events there at
    the units 0, 1 and 63 (where the case builder aims) with their operands and their place; keep = True: every event in order
    (events).  cache: a dict shared between runs, in which the models keep what a segment of unchanged values gave."""
    zero = 0

    def __init__(self, keep=False, cache=None):
        self.counts, self.hits, self.events, self.cache = {}, {}, ([] if keep else None), cache

    def _note(self, kern, site, cl, a, b, where):
        key = (kern, site, cl)
        self.counts[key] = self.counts.get(key, 0) + 1
        if type(where) is tuple and where[-1] in (0, 1, 63):
            self.hits.setdefault((kern, site), []).append((cl, a, b, where))
        if self.events is not None:
            self.events.append(key)

    @classmethod
    def of(cls, counts):
        r = cls()
        r.counts = dict(counts)
        return r

    def merge(self, other):
        for k, n in other.counts.items():
            self.counts[k] = self.counts.get(k, 0) + n
        for k, h in other.hits.items():
            self.hits.setdefault(k, []).extend(h)

    def add(self, kern, site, a, b, where=None):
        self._note(kern, site, classify(a, b), a, b, where)
        return a + b

    def dbl(self, kern, site, a, where=None):
        self._note(kern, site, "dbl(inf)" if a == 0 else "generic", a, a, where)
        return 2 * a

    def is_inf(self, a):
        return a == 0

    def neg(self, a):
        return -a

    def edge_events(self, classes=("P+P", "P-P")):
        return {k: v for k, v in self.counts.items() if k[2] in classes}


class PointRec:
    """The same interface over points of pallas_model: the class is what the affine arithmetic meets (pm.add's own cases)"""
    zero = None

    def __init__(self):
        self.events = []

    def add(self, kern, site, a, b, where=None):
        if a is None:
            cl = "inf+inf" if b is None else "inf+Q"
        elif b is None:
            cl = "Q+inf"
        elif a[0] == b[0]:
            cl = "P+P" if a[1] == b[1] else "P-P"
        else:
            cl = "generic"
        self.events.append((kern, site, cl))
        return pm.add(a, b)

    def dbl(self, kern, site, a, where=None):
        self.events.append((kern, site, "dbl(inf)" if a is None else "generic"))
        return pm.add(a, a)

    def is_inf(self, a):
        return a is None

    def neg(self, a):
        return pm.neg(a)


# ---------------------------------------------------------------------------------------------------- plans
def general_plan(c, span=0):
    """the general pipeline's plan as msm_enqueue_launches computes it (msm_general.hip), restated to build cases for it: the GPU
    tests assert every field against halo_dev_msm_last_plan before they look at a result"""
    B, W = 1 << (c - 1), windows_of(c)
    if B <= 64:
        L, nseg = 1, 1
    else:
        L = 8 if B >= 16384 else 4 if B >= 4096 else 2 if B >= 1024 else 1
        nseg = B // (64 * L)
        if span > 0:
            L = span
            while 64 * L > B:
                L >>= 1
            while B // (64 * L) > 64:
                L <<= 1
            nseg = B // (64 * L)
    logL = L.bit_length() - 1
    live = 1
    while live < nseg:
        live <<= 1
    return dict(pipeline=0, form=0, c=c, W=W, B=B, L=L, logL=logL, nseg=nseg, live_seg=live, span=span)


def small_plan(c, span=0):
    """the small pipeline's plan as smsm_enqueue computes it (smsm.hip; its wave cap at the default of 1024)"""
    B, W = 1 << (c - 1), windows_of(c)
    L = 1
    while 64 * L * 16 < B:
        L <<= 1
    while L < 64 and W * ((B + 64 * L - 1) // (64 * L)) * 4 > 1024 and 64 * L < B:
        L <<= 1
    if span > 0:
        L = span
        while 64 * L * 64 < B:
            L <<= 1
    nseg = (B + 64 * L - 1) // (64 * L)
    live = 1
    while live < nseg:
        live <<= 1
    return dict(pipeline=1, form=1, c=c, W=W, B=B, L=L, logL=L.bit_length() - 1, nseg=nseg, live_seg=live, span=span)


# one block of k_rc_mid: 64 entries E_Q with S = T = E_Q, no doublings -- the builder's plan for a block of columns or rows
RC_MID_PLAN = dict(pipeline="rc_mid", form=2, c=0, W=2, B=64, L=1, logL=0, nseg=1, live_seg=1, span=0)


def make_plan(pipeline, c, span=0):
    return general_plan(c, span) if pipeline == 0 else small_plan(c, span) if pipeline == 1 else RC_MID_PLAN


# the small pipeline at the same window sizes, with the default span and with span 1.  At c = 7, 8 and 10 the default IS one bucket per
# quad (small_plan(c) == small_plan(c, 1) but for the name of the span: asserted in the CPU module); 13: L = 8 by default, 64 segments at span 1
SMALL_PLANS = [(7, 0), (8, 0), (10, 0), (13, 0), (13, 1)]
# (c, reduce span): B = 64 is the `p.B <= 64` branch; 13 with span 1 runs all six levels of k_smsm_final; 11 with span 8 is L = 8
GENERAL_PLANS = [(7, 0), (8, 0), (10, 2), (13, 1), (11, 8)]


# ---------------------------------------------------------------------------------------------------- models
def model_wave_weighted_sum(rec, kern, S, T, k, where=None):
    """wave_weighted_sum (msm_buckets.hip), live = 64: lane 0's (S, T) afterwards"""
    S, T = list(S), list(T)
    off = 1
    while off < 64:
        o = [S[(l + off) & 63] for l in range(64)]
        for l in range(64 - off):
            S[l] = rec.add(kern, "scan/%d" % off, S[l], o[l], (where, l))
        off <<= 1
    V = [S[l] if l >= 1 else rec.zero for l in range(64)]
    for i in range(k):
        V = [rec.dbl(kern, "dbl/%d" % i, V[l], (where, l)) for l in range(64)]
    T = [rec.add(kern, "T+=V", T[l], V[l], (where, l)) for l in range(64)]
    off = 32
    while off >= 1:
        o = [T[(l + off) & 63] for l in range(64)]
        for l in range(off):
            T[l] = rec.add(kern, "tree/%d" % off, T[l], o[l], (where, l))
        off >>= 1
    return S[0], T[0]


def _cached(rec, key, compute):
    """compute(sub-recorder) -> result, once per key when the recorder carries a cache (IntRec.cache): the events are merged"""
    cache = getattr(rec, "cache", None)
    if cache is None:
        return compute(rec)
    if key not in cache:
        sub = IntRec()
        cache[key] = (compute(sub), sub)
    out, sub = cache[key]
    rec.merge(sub)
    return out


def model_reduce1(rec, v, B, L, logL, nseg, window=0):
    """k_msm_reduce1 over one window's bucket values v (B integers) -> the segments' (S, T)"""
    def segment(rec, s):
        run, tot = [], []
        for lane in range(64):
            first = s * 64 * L + lane * L
            r = t = rec.zero
            for step in range(L):
                idx = first + L - 1 - step
                b = v[idx] if idx < B else rec.zero
                r = rec.add(K_REDUCE1, "run+=b/%d" % step, r, b, ((window, s), lane))
                t = rec.add(K_REDUCE1, "tot+=run/%d" % step, t, r, ((window, s), lane))
            run.append(r)
            tot.append(t)
        return model_wave_weighted_sum(rec, K_REDUCE1, run, tot, logL, (window, s))
    return [_cached(rec, (K_REDUCE1, window, s, L, tuple(v[s * 64 * L:(s + 1) * 64 * L])), lambda r, s=s: segment(r, s)) for s in range(nseg)]


def small_tasks(entries, kmax, wave_task=512):
    """the small pipeline's balanced split (smsm.hip bucket_tasks, k_smsm_sort): task sizes of a bucket"""
    if entries == 0:
        return []
    nt = (entries + kmax - 1) // kmax if entries <= 4 * kmax else (entries + wave_task - 1) // wave_task
    return [entries // nt + (1 if j < entries % nt else 0) for j in range(nt)]


def model_smsm_reduce(rec, parts, B, L, logL, nseg, window=0):
    """k_smsm_reduce over one window: parts[b] = the partials of bucket b in task order (an empty bucket: none) -> the segments'
    (S, T).  Buckets of more than SMSM_HEAVY partials are summed by all 64 quads first (at most 64 per block: more are not
    modelled); the partial loop walks to the largest count among the 16 quads of a wave, adding infinity where a bucket has fewer."""
    def segment(rec, s):
        lo = s * 64 * L
        mine = {}
        heavy = [b for b in range(lo, min(lo + 64 * L, B)) if len(parts[b]) > SMSM_HEAVY]
        assert len(heavy) <= 64
        for b in heavy:
            nt, acc = len(parts[b]), [rec.zero] * 64
            for Q in range(64):
                for j in range(Q, (nt + 63) & ~63, 64):
                    acc[Q] = rec.add(K_SREDUCE, "heavy strided", acc[Q], parts[b][j] if j < nt else rec.zero, ((window, s), Q))
            off = 32
            while off >= 1:
                o = [acc[Q + off] if Q + off < 64 else rec.zero for Q in range(64)]
                for Q in range(off):
                    acc[Q] = rec.add(K_SREDUCE, "heavy tree/%d" % off, acc[Q], o[Q], ((window, s), Q))
                off >>= 1
            mine[b] = [acc[0]]
        run, tot = [rec.zero] * 64, [rec.zero] * 64
        for step in range(L):
            ps = []
            for Q in range(64):
                idx = lo + Q * L + L - 1 - step
                ps.append(mine.get(idx, parts[idx]) if idx < B else [])
            for Q in range(64):
                ntmax = max(len(ps[q]) for q in range(Q & ~15, (Q & ~15) + 16))
                b = ps[Q][0] if ps[Q] else rec.zero
                for k in range(1, ntmax):
                    b = rec.add(K_SREDUCE, "partial", b, ps[Q][k] if k < len(ps[Q]) else rec.zero, ((window, s), Q))
                run[Q] = rec.add(K_SREDUCE, "run+=b/%d" % step, run[Q], b, ((window, s), Q))
                tot[Q] = rec.add(K_SREDUCE, "tot+=run/%d" % step, tot[Q], run[Q], ((window, s), Q))
        return model_block_weighted_sum(rec, K_SREDUCE, run, tot, logL, 64, (window, s))
    return [_cached(rec, (K_SREDUCE, window, s, L, tuple(tuple(x) for x in parts[s * 64 * L:(s + 1) * 64 * L])), lambda r, s=s: segment(r, s))
            for s in range(nseg)]


def model_block_weighted_sum(rec, kern, S, T, k, live, where=None):
    """block_weighted_sum (smsm.hip) over 64 quads: quad 0's (S, T) afterwards.  The additions of the quads below `live` are
    recorded (the quads behind hold infinity and add infinity); in the tree those of the quads that keep the sum (Q < off)."""
    S, T = list(S), list(T)
    off = 1
    while off < live:
        o = [S[Q + off] if Q + off < live else rec.zero for Q in range(64)]
        for Q in range(live):
            S[Q] = rec.add(kern, "scan/%d" % off, S[Q], o[Q], (where, Q))
        off <<= 1
    V = [S[Q] if Q >= 1 else rec.zero for Q in range(64)]
    for i in range(k):
        V = [rec.dbl(kern, "dbl/%d" % i, V[Q], (where, Q)) if Q < live else V[Q] for Q in range(64)]
    for Q in range(live):
        T[Q] = rec.add(kern, "T+=V", T[Q], V[Q], (where, Q))
    off = live >> 1
    while off >= 1:
        o = [T[Q + off] if Q + off < live else rec.zero for Q in range(64)]
        for Q in range(off):
            T[Q] = rec.add(kern, "tree/%d" % off, T[Q], o[Q], (where, Q))
        off >>= 1
    return S[0], T[0]


def model_final(rec, segs, nseg, k, live, window=0):
    """k_smsm_final: the segments' (S, T) -> the window sum"""
    S = [segs[Q][0] if Q < nseg else rec.zero for Q in range(64)]
    T = [segs[Q][1] if Q < nseg else rec.zero for Q in range(64)]
    return model_block_weighted_sum(rec, K_FINAL, S, T, k, live, window)[1]


def model_window(rec, plan, v, window=0, parts=None):
    """one window behind the combine: bucket values (small pipeline: or every bucket's partials) -> window sum.  General pipeline:
    k_msm_reduce1 + k_smsm_final; small: k_smsm_reduce, and k_smsm_final over more than one segment; "rc_mid": one block of k_rc_mid,
    whose T comes back."""
    if plan["pipeline"] == "rc_mid":
        return model_block_weighted_sum(rec, K_RCMID, v, v, 0, 64, window)[1]
    if plan["pipeline"] == 0:
        segs = model_reduce1(rec, v, plan["B"], plan["L"], plan["logL"], plan["nseg"], window)
    else:
        parts = parts if parts is not None else [[x] if x else [] for x in v]
        segs = model_smsm_reduce(rec, parts, plan["B"], plan["L"], plan["logL"], plan["nseg"], window)
        if plan["nseg"] == 1:
            return segs[0][1]
    return model_final(rec, segs, plan["nseg"], plan["logL"] + 6, plan["live_seg"], window)


def model_horner(rec, sums, c):
    """msm_combine_member's Horner over the window sums [w], top window first, with its guarded doublings"""
    acc = rec.zero
    for w in range(len(sums) - 1, -1, -1):
        if not rec.is_inf(acc):
            for k in range(c):
                acc = rec.dbl(K_HOST, "horner dbl", acc, w)
        acc = rec.add(K_HOST, "horner", acc, sums[w], w)
    return acc


def model_combine(rec, tasks, where=None):
    """k_msm_combine over one multi-task bucket's partials, in task order -> the bucket value"""
    nt = len(tasks)
    assert nt >= 2
    if nt <= 8:
        acc = tasks[0]
        for j in range(1, nt):
            acc = rec.add(K_COMBINE, "serial", acc, tasks[j], (where, j))
        return acc
    acc = [rec.zero] * 64
    for lane in range(64):
        for j in range(lane, nt, 64):
            acc[lane] = rec.add(K_COMBINE, "strided", acc[lane], tasks[j], (where, lane))
    off = 32
    while off >= 1:
        o = [acc[(l + off) & 63] for l in range(64)]
        for l in range(off):
            acc[l] = rec.add(K_COMBINE, "tree/%d" % off, acc[l], o[l], (where, l))
        off >>= 1
    return acc[0]


def general_tasks(entries, kmax):
    """the general and the table pipelines cut a bucket into tasks of kmax entries, the last one takes the rest: task sizes"""
    nt = (entries + kmax - 1) // kmax
    return [kmax] * (nt - 1) + [entries - (nt - 1) * kmax]


# ---------------------------------------------------------------------------------------------------- sites
def unit_kernel(plan):
    return {0: K_REDUCE1, 1: K_SREDUCE, "rc_mid": K_RCMID}[plan["pipeline"]]


def sites(plan):
    """every (kernel, site) the window sums have under this plan behind the combine, single-task buckets, the doublings left out (a
    doubling has no side branch but infinity)"""
    out, uk = [], unit_kernel(plan)
    if uk != K_RCMID:
        for t in range(plan["L"]):
            out += [(uk, "run+=b/%d" % t), (uk, "tot+=run/%d" % t)]
    out += [(uk, "scan/%d" % (1 << k)) for k in range(6)] + [(uk, "T+=V")] + [(uk, "tree/%d" % (32 >> k)) for k in range(6)]
    if uk == K_RCMID or (uk == K_SREDUCE and plan["nseg"] == 1):
        return out  # (one segment of the small pipeline: k_smsm_reduce writes the window sum itself)
    live, off = plan["live_seg"], 1
    while off < live:
        out.append((K_FINAL, "scan/%d" % off))
        off <<= 1
    out.append((K_FINAL, "T+=V"))
    off = live >> 1
    while off >= 1:
        out.append((K_FINAL, "tree/%d" % off))
        off >>= 1
    return out


# Structural impossibilities only: (kernel, site or site prefix, class, condition on the plan or None, reason)
_FIRST = "the left operand of a lane's (quad's) first step is always infinity"
_ONE = "one segment: quad 0 adds V = infinity, the other quads hold nothing"
UNREACHABLE = [(k, site, cl, None, _FIRST if site.startswith("run") else "tot is infinity before the first step")
               for k in (K_REDUCE1, K_SREDUCE) for site in ("run+=b/0", "tot+=run/0") for cl in ("P+P", "P-P", "Q+inf")]
UNREACHABLE += [(K_FINAL, "T+=V", cl, lambda p: p["live_seg"] == 1, _ONE) for cl in ("P+P", "P-P", "inf+Q")]


def unreachable(plan, kern, site, cl):
    for k, s, c, cond, why in UNREACHABLE:
        if k == kern and s == site and c == cl and (cond is None or cond(plan)):
            return why
    return None


def natural_events(plan):
    """P+P / P-P events every window of the plan meets whatever its values, left out when a case's target must be the window's only
    one.  L = 1: a lane's T is its bucket and V the sum of the buckets from its own upwards, so the top non-empty lane of every
    segment adds V = T."""
    return {(unit_kernel(plan), "T+=V", "P+P")} if plan["L"] == 1 else set()


def targets(plan):
    return [(k, s, cl) for k, s in sites(plan) for cl in EDGE if unreachable(plan, k, s, cl) is None]


# ---------------------------------------------------------------------------------------------------- case builder
class WindowCase:
    """One window: the bucket values (dict bucket -> integer, every other bucket empty), which of them the background's points
    give (bg: bucket -> index of the background point) and which need a point of their own (own: bucket -> value), the target
    and the model's count of every class at every site of this window."""

    def __init__(self, plan, target, values, bg, own, counts, seed):
        self.plan, self.target, self.values, self.bg, self.own, self.counts, self.seed = plan, target, values, bg, own, counts, seed

    def dense(self):
        v = [0] * self.plan["B"]
        for b, x in self.values.items():
            v[b] = x
        return v

    def window_sum(self):
        return sum((b + 1) * x for b, x in self.values.items())

    def name(self):
        return "%s %s %s (seed %d)" % (self.target + (self.seed,))


def background_values(n_bg, seed):
    """distinct non-zero integers of magnitude below 2^15, both signs, no two opposite"""
    rng, out, seen = pm.SplitMix64(seed), [], set()
    while len(out) < n_bg:
        x = rng.next_u64()
        m = 1 + (x >> 8) % 32767
        if m in seen:
            continue
        seen.add(m)
        out.append(-m if x & 1 else m)
    return out


def _scatter(B, n_bg, seed):
    """a seeded injection of the background points into the window's buckets: bucket -> background index"""
    rng, slots = pm.SplitMix64(seed), list(range(B))
    for i in range(min(n_bg, B)):
        j = i + rng.next_u64() % (B - i)
        slots[i], slots[j] = slots[j], slots[i]
    return {slots[i]: i for i in range(min(n_bg, B))}


def _recipe(plan, kern, site, cl, s0):
    """-> (empty buckets, the bucket to solve for (or a pair: with a second free bucket) or None, extra own values {bucket: value}, (where, unit) of the target event).
    Units: the 64 lanes of segment s0 (k_msm_reduce1: L buckets each) or the segments (k_smsm_final: 64 L buckets each)."""
    L, B = plan["L"], plan["B"]
    if kern == K_RCMID:
        size, base, n_units, k, where = 1, 0, 64, 0, 0
    elif kern in UNIT_KERNELS:
        size, base, n_units, k, where = L, s0 * 64 * L, 64, plan["logL"], (0, s0)
    else:
        size, base, n_units, k, where = 64 * L, 0, plan["live_seg"], plan["logL"] + 6, 0
    unit = lambda u: range(base + u * size, base + (u + 1) * size)
    units = lambda a, b: [x for u in range(a, min(b, n_units)) for x in unit(u)]
    kind, _, arg = site.partition("/")
    arg = int(arg) if arg else 0
    pp = cl in ("P+P", "P-P")
    if kind in ("run+=b", "tot+=run"):
        lane, j = 0, L - 1 - arg  # lane 0 of the segment, its bucket of step `arg`
        bucket = base + j
        if kind == "tot+=run" and arg == 1 and cl == "P+P":
            return {bucket}, None, {}, (where, lane)  # tot = run_0 and run_1 = run_0 + b: equal exactly when this bucket is empty
        if pp:
            return set(), bucket, {}, (where, lane)
        if cl == "inf+Q":
            return set(range(bucket + 1, base + L)), None, {}, (where, lane)
        if kind == "run+=b":
            return {bucket}, None, {}, (where, lane)
        return None  # tot+=run Q+inf: run cancels to infinity with tot finite -- the P-P of run+=b at this step (build_cases)
    if kind == "scan":
        if pp:
            return set(), unit(arg)[0], {}, (where, 0)
        if cl == "inf+Q":
            return set(units(0, arg)), None, {}, (where, 0)
        return set(units(arg, 2 * arg)), None, {}, (where, 0)
    if kind == "tree":
        if pp:
            return set(), unit(0)[0], {}, (where, 0)
        if cl == "inf+Q":
            return set(unit(0)) | set(units(2 * arg, n_units)), None, {}, (where, 0)
        return set(units(arg, n_units)), None, {}, (where, 0)
    assert kind == "T+=V"
    if cl == "Q+inf":
        return set(), None, {}, (where, 0)   # unit 0 adds V = infinity in every case
    if cl == "P+P" and kern in UNIT_KERNELS and k == 0:
        return set(), None, {unit(63)[0]: 30011}, (where, 63)  # (natural_events: the top lane's T and V are both its bucket)
    if pp:
        # unit 1: T_1 = sum (i + 1) b_i, V_1 = 2^k (S_1 + the units above).  k >= 1: the bucket of weight 2^k - 1 in unit 1 moves the
        # two sides by 2^k - 1 and 2^k; k = 0: a bucket of unit 2 moves only V
        # (P-P: the sides move together by 2^(k+1) - 1; the unit's last bucket, 2^k + 2^k, is the second free value that makes it divide)
        return set(), ((unit(1)[(1 << k) - 2], unit(1)[(1 << k) - 1] if cl == "P-P" else None) if k >= 1 else unit(2)[0]), {}, (where, 1)
    if n_units > 2:
        return set(unit(1)), None, {}, (where, 1)   # inf+Q: unit 1 empty, the units above it not
    # two units: T_1 = 0 with S_1 finite needs values that cancel under the weights: 2 a in the unit's first bucket, -a in its second
    return set(unit(1)), None, {unit(1)[0]: 2 * 7919, unit(1)[1]: -7919}, (where, 1)


def build_case(plan, target, bg_values, seed, tries=40, cache=None):
    """bucket values that put `target` = (kernel, site, class) into one window of `plan`: the background's points scattered by the
    seed, some buckets emptied, at most one value solved for.  The model confirms: the target event occurs where it was aimed,
    and, for P+P / P-P, it is the window's only event of those two classes."""
    kern, site, cl = target
    B = plan["B"]
    if (site.partition("/")[0], cl) == ("tot+=run", "Q+inf"):
        inner = build_case(plan, (kern, "run+=b/" + site.partition("/")[2], "P-P"), bg_values, seed, tries, cache)
        assert inner.counts.get(target, 0) >= 1
        return WindowCase(plan, target, inner.values, inner.bg, inner.own, inner.counts, inner.seed)
    for t in range(tries):
        sd = seed % 3 + 7919 * t  # (three backgrounds per plan, and more where a try fails: the segment cache pays)
        s0 = sd % plan["nseg"]
        empty, solve, extra, (where, unit) = _recipe(plan, kern, site, cl, s0)
        solve, helper = solve if isinstance(solve, tuple) else (solve, None)
        place = _scatter(B, len(bg_values), sd)
        bg = {b: i for b, i in place.items() if b not in empty and b not in (solve, helper) and b not in extra}
        values = {b: bg_values[i] for b, i in bg.items()}
        own = dict(extra)
        values.update(extra)

        def run(x=None, y=0):
            v = [0] * B
            for b, val in values.items():
                v[b] = val
            if x is not None:
                v[solve] = x
                if helper is not None:
                    v[helper] = y
            rec = IntRec(cache=cache)
            model_window(rec, plan, v)
            return rec

        if solve is not None:
            # the target's operands are linear in the free values: f = right - left (P+P) or right + left (P-P) must vanish
            def f(x, y=0):
                h = [h for h in run(x, y).hits.get((kern, site), []) if h[3] == (where, unit)]
                return None if len(h) != 1 else (h[0][2] - h[0][1] if cl == "P+P" else h[0][2] + h[0][1])
            f0, f1 = f(0), f(1)
            if f0 is None or f1 is None or f1 == f0:
                continue
            fx, y = f1 - f0, 0
            if helper is not None:  # a second free value brings f0 + fy y to a multiple of fx
                fy = f(0, 1) - f0
                y = next((y for y in range(1, abs(fx) + 1) if (f0 + fy * y) % fx == 0), None)
                if y is None:
                    continue
                f0 += fy * y
                own[helper] = values[helper] = y
            if f0 % fx or f0 == 0:
                continue
            own[solve] = values[solve] = -f0 // fx
        rec = run()
        hit = [h for h in rec.hits.get((kern, site), []) if h[3] == (where, unit)]
        if len(hit) != 1 or hit[0][0] != cl:
            continue
        edges = {k: n for k, n in rec.edge_events().items() if k == target or k not in natural_events(plan)}
        if cl in ("P+P", "P-P") and (len(edges) != 1 or target not in edges or (edges[target] != 1 and target not in natural_events(plan))):
            continue
        if max(abs(x) for x in values.values()) * B * B >= LIMIT:
            continue
        return WindowCase(plan, target, values, bg, own, rec.counts, sd)
    raise AssertionError("no case for %s under plan %s" % (target, plan))


_CASES = {}


def plan_background(plan):
    """the background points of a plan's key: one per bucket -- up to 3584 where a lane holds one bucket (a key of 4096 points keeps
    room for the solved values); with more buckets per lane every bucket gets one: an empty bucket behind a full one makes tot = run at
    the lane's second step, a P+P in every such lane"""
    return background_values(plan["B"] if plan["L"] > 1 else min(plan["B"], 3584), 0x77696E73 + plan["c"])


def build_cases(c, span=0, pipeline=0):
    """every target of the plan, one window each, built once per process -> (plan, background values, cases)"""
    key = (pipeline, c, span)
    if key not in _CASES:
        plan = make_plan(pipeline, c, span)
        bg, cache = plan_background(plan), {}
        cases = [build_case(plan, t, bg, 1000 * c + 17 * i, cache=cache) for i, t in enumerate(targets(plan))]
        _CASES[key] = (plan, bg, cases)
    return _CASES[key]


PLAN_SET = [(0, c, span) for c, span in GENERAL_PLANS] + [(1, c, span) for c, span in SMALL_PLANS] + [("rc_mid", 0, 0)]


def coverage(plan_set=PLAN_SET):
    """{(pipeline, c, span): {(kernel, site, class): number of cases that meet it}} over the built cases of every plan"""
    table = {}
    for pipeline, c, span in plan_set:
        _, _, cases = build_cases(c, span, pipeline)
        t = {}
        for case in cases:
            for key in case.counts:
                t[key] = t.get(key, 0) + 1
        table[(pipeline, c, span)] = t
    return table


def uncovered(table):
    """-> the (plan, kernel, site, class) of the four edge classes that no case meets and UNREACHABLE does not exempt"""
    out = []
    for key, t in table.items():
        plan = make_plan(*key)
        for k, s in sites(plan):
            for cl in EDGE:
                if t.get((k, s, cl), 0) == 0 and unreachable(plan, k, s, cl) is None:
                    out.append((key, k, s, cl))
    return out


def format_coverage(table):
    lines = []
    for key, t in table.items():
        plan = make_plan(*key)
        lines.append("pipeline %s c=%d span=%d: B=%d L=%d nseg=%d" % (key + (plan["B"], plan["L"], plan["nseg"])))
        for k, s in sites(plan):
            cells = []
            for cl in EDGE:
                why = unreachable(plan, k, s, cl)
                cells.append("%s %s" % (cl, "n/a" if why else "%d" % t.get((k, s, cl), 0)))
            lines.append("  %-14s %-12s %s" % (k, s, "  ".join(cells)))
    return "\n".join(lines)


# ---------------------------------------------------------------------------------------------------- launches
class Launch:
    """One scalar array over a plan's key: window w of the launch is cases[w] (W - 1 of them at most; the top window is empty).
    key_ks: the key's multiples (background first, then the cases' own points); scalars: Python integers, one per key point."""

    def __init__(self, plan, cases, key_ks, own_index):
        self.plan, self.cases = plan, cases
        digits = [dict() for _ in key_ks]
        for w, case in enumerate(cases):
            for b, i in case.bg.items():
                digits[i][w] = b + 1
            for b in case.own:
                digits[own_index[(id(case), b)]][w] = b + 1
        self.scalars = general_scalars(plan["c"], digits)
        self.values = [case.values for case in cases] + [{}] * (plan["W"] - len(cases))


def pack_launches(plan, bg_values, cases, n_multiple=8):
    """-> (key multiples, launches): the background's points, then one point per own value of every case; the cases W - 1 to a
    launch.  The key is padded with infinities to a multiple of 8 points (the two-level sort wants one)."""
    ks, own_index = list(bg_values), {}
    for case in cases:
        for b, x in case.own.items():
            own_index[(id(case), b)] = len(ks)
            ks.append(x)
    while len(ks) % n_multiple:
        ks.append(0)
    per = plan["W"] - 1
    launches = [Launch(plan, cases[i:i + per], ks, own_index) for i in range(0, len(cases), per)]
    return ks, launches


class PlantedLaunch:
    """A launch planted by hand: the key's multiples, one scalar per key point, the bucket values of every window (values[w]) and
    the model's counts over what it planted (counts)"""

    def __init__(self, plan, ks, digits, values, counts, cases=None):
        self.plan, self.ks, self.values, self.counts, self.cases = plan, ks, values, counts, cases
        self.scalars = general_scalars(plan["c"], digits)


COMBINE_G, COMBINE_KMAX = 3, 8
# (tasks, entries) of the equal-entry buckets under a task length of 8: full tasks of 8 g, the last one takes the rest -- 2 tasks are
# the serial loop's P+P, 8 its longest run, 9 the wave form with live lanes 0 .. 8, 64 every lane once, 65 lane 0's second trip
COMBINE_BUCKETS = [(2, 16), (8, 59), (9, 67), (64, 507), (65, 520), (10, 80)]
COMBINE_EQUAL = 1023         # points g G of the combine key: the 128-task bucket takes them all


def combine_launch(c=11, span=0):
    """k_msm_combine under a task length of 8: window t < 5 holds one bucket of COMBINE_BUCKETS[t] equal entries g G (its tasks do
    not depend on the order the sort leaves the entries in), window 5 the two-task bucket of 15 entries g G and one of -15 g G (tasks
    +8 g and -8 g whichever gets the large entry: P-P, the bucket is infinity); every other bucket of these windows holds one
    background point.  Windows 6 .. 11: a bucket of 64 tasks, 511 entries g G and one of -(7 + 8 (2^(t+1) - 1)) g G, t = 0 .. 5: the
    task that gets it is worth -(2^(t+1) - 1) 8 g, so that whichever lane holds it the wave's tree meets P-P at its level 32 >> t (and
    infinity on one side or the other at the next).  Window 12: a bucket of 16 entries that are all the infinity point (two infinite
    partials).  Window 13: a bucket of 128 tasks, 1023 entries g G and one of -15 g G: every lane makes two trips, and the lane that
    holds the odd task (-8 g) adds it to 8 g in the strided loop, first or second -- P-P there.  65 tasks of 8 entries: lane 0's second
    trip adds 8 g to 8 g; 10 tasks of 8: the tree's last level adds two equal halves.  Windows 14 .. 16: buckets of 64, 8 and 128
    tasks with one entry of -7 g G among entries g G -- the task that holds it is the infinity: the tree's first level, the serial
    loop and the strided loop add it on the left (inf+Q) or on the right (Q+inf).  Which task holds an odd entry is the sort's
    atomics': the counts are those of the odd task first and of the odd task last together.  B = 1024: the two-level sort (sort mode 1) takes it as well."""
    plan = general_plan(c, span)
    B, g, kmax = plan["B"], COMBINE_G, COMBINE_KMAX
    bgv = plan_background(plan)
    wave_big = [-(7 + 8 * ((2 << t) - 1)) * g for t in range(6)]
    ks = list(bgv) + [g] * COMBINE_EQUAL + [-15 * g] + wave_big + [0] * 16 + [-7 * g]
    zero_pt = len(ks) - 1
    eq0, big = len(bgv), len(bgv) + COMBINE_EQUAL
    while len(ks) % 8:
        ks.append(0)
    digits = [dict() for _ in ks]
    values, rec = [], IntRec()
    spots = [5, 300, B - 1, 64, 777, 512, 222] + [100 + 37 * t for t in range(6)] + [901, 333, 444, 555, 666]
    NB = len(COMBINE_BUCKETS)
    for w, bucket in enumerate(spots):
        place = _scatter(B, len(bgv), 0xC0B1 + w)
        v = {}
        for b, i in place.items():
            if b != bucket:
                digits[i][w] = b + 1
                v[b] = bgv[i]
        if w < len(COMBINE_BUCKETS):
            nt, entries = COMBINE_BUCKETS[w]
            sizes = general_tasks(entries, kmax)
            assert len(sizes) == nt
            for i in range(entries):
                digits[eq0 + i][w] = bucket + 1
            v[bucket] = model_combine(rec, [g * n for n in sizes], (w, bucket))
            assert v[bucket] == entries * g
        elif w == NB:
            for i in range(2 * kmax - 1):
                digits[eq0 + i][w] = bucket + 1
            digits[big][w] = bucket + 1
            assert model_combine(rec, [kmax * g, -kmax * g], (w, bucket)) == 0 == model_combine(IntRec(), [-kmax * g, kmax * g])
        elif w < NB + 7:
            t = w - NB - 1
            for i in range(64 * kmax - 1):
                digits[eq0 + i][w] = bucket + 1
            digits[big + 1 + t][w] = bucket + 1
            odd = (kmax - 1) * g + wave_big[t]
            v[bucket] = model_combine(rec, [odd] + [kmax * g] * 63, (w, bucket))  # (counted with the odd task on lane 0 and on lane 63)
            model_combine(rec, [kmax * g] * 63 + [odd], (w, bucket))
            for lane in (1, 31, 32, 63):  # wherever it lands: the same level meets the P-P
                other = IntRec()
                model_combine(other, [kmax * g] * lane + [odd] + [kmax * g] * (63 - lane))
                assert [k for k in other.counts if k[2] == "P-P"] == [(K_COMBINE, "tree/%d" % (32 >> t), "P-P")]
        elif w == NB + 7:
            for i in range(2 * kmax):
                digits[big + 7 + i][w] = bucket + 1
            assert model_combine(rec, [0, 0], (w, bucket)) == 0
        elif w > NB + 8:
            nt = {NB + 9: 64, NB + 10: 8, NB + 11: 128}[w]
            for i in range(nt * kmax - 1):
                digits[eq0 + i][w] = bucket + 1
            digits[zero_pt][w] = bucket + 1
            v[bucket] = model_combine(rec, [0] + [kmax * g] * (nt - 1), (w, bucket))
            assert v[bucket] == model_combine(rec, [kmax * g] * (nt - 1) + [0], (w, bucket)) == (nt - 1) * kmax * g
        else:
            for i in range(128 * kmax - 1):
                digits[eq0 + i][w] = bucket + 1
            digits[big][w] = bucket + 1
            v[bucket] = model_combine(rec, [-kmax * g] + [kmax * g] * 127, (w, bucket))  # (counted with the odd task first)
            for at in (5, 64, 127):  # wherever it lands: its lane's strided loop meets the P-P
                other = IntRec()
                model_combine(other, [kmax * g] * at + [-kmax * g] + [kmax * g] * (127 - at))
                assert [k for k in other.counts if k[2] == "P-P"] == [(K_COMBINE, "strided", "P-P")]
        values.append({b: x for b, x in v.items() if x})
    values += [{}] * (plan["W"] - len(values))
    return PlantedLaunch(plan, ks, digits, values, rec.counts)


def horner_launch(c):
    """the host's Horner with its guarded doublings: from the top planted window down the window sums are a, 2^c a (P+P with the
    doubled accumulator), -2^(2c+1) a (P-P: the accumulator is infinity and the doublings are skipped), nothing (inf+inf), b
    (inf+Q), nothing (Q+inf), then one background point per bucket in the windows below.  One own point per sum, in bucket 0."""
    plan = general_plan(c)
    B, W, a, b = plan["B"], plan["W"], 3, 5
    sums = [a, a << c, -(a << (2 * c + 1)), 0, b, 0]
    bgv = plan_background(plan)
    ks = list(bgv) + [x for x in sums if x]
    while len(ks) % 8:
        ks.append(0)
    digits, values, at = [dict() for _ in ks], [{} for _ in range(W)], len(bgv)
    for t, x in enumerate(sums):
        w = W - 2 - t
        if x:
            digits[at][w] = 1
            values[w] = {0: x}
            at += 1
    for w in range(W - 2 - len(sums), -1, -1):
        for bkt, i in _scatter(B, len(bgv), 0x4052 + w).items():
            digits[i][w] = bkt + 1
            values[w][bkt] = bgv[i]
    rec = IntRec()
    total = model_horner(rec, [sum((bk + 1) * x for bk, x in v.items()) for v in values], c)
    assert abs(total) < 1 << 300
    return PlantedLaunch(plan, ks, digits, values, rec.counts)


def partials_launch(c=10):
    """k_smsm_reduce's partial loop and heavy-bucket pre-sum, planted by hand under the default task length of 8 (n <= 2^14): equal
    entries g G, so that the tasks' values do not depend on the order the sort leaves.  Window 0: the neighbouring buckets 19, 20, 21
    of 8, 16 and 32 entries -- 1, 2 and 4 partials in neighbouring quads of one wave, which walks to 4 and adds infinity to the short
    ones.  Window 1: the two-task P-P bucket (15 entries g G, one of -15 g G) beside a bucket of 4 partials.  Window 2: a heavy bucket
    of 2050 entries, 5 wave tasks of 410.  Window 3: 16 entries that are all the infinity point (two infinite partials) beside a
    bucket of two.  Window 4: a two-task bucket whose odd entry makes one task the infinity.  Every other bucket of these windows holds
    one background point."""
    plan = small_plan(c)
    B, g, kmax = plan["B"], COMBINE_G, 8
    bgv = plan_background(plan)
    ks = list(bgv) + [g] * 2050 + [-15 * g] + [0] * 16 + [-7 * g]
    eq0, big, inf0 = len(bgv), len(bgv) + 2050, len(bgv) + 2051
    while len(ks) % 8:
        ks.append(0)
    digits, values, rec = [dict() for _ in ks], [], IntRec()
    planted = [{19: 8, 20: 16, 21: 32}, {40: "P-P", 41: 32}, {100: 2050}, {200: "inf", 201: 16}, {300: "zero", 301: 16}]
    for w, spec in enumerate(planted):
        parts = [[] for _ in range(B)]
        for b, i in _scatter(B, len(bgv), 0x5A11 + w).items():
            if b not in spec:
                digits[i][w] = b + 1
                parts[b] = [bgv[i]]
        at = eq0  # (a point has one digit per window: every bucket takes its own points)
        for b, what in spec.items():
            if what == "P-P":
                for i in range(2 * kmax - 1):
                    digits[at + i][w] = b + 1
                at += 2 * kmax - 1
                digits[big][w] = b + 1
                parts[b] = [kmax * g, -kmax * g]
            elif what == "inf":
                for i in range(2 * kmax):
                    digits[inf0 + i][w] = b + 1
                parts[b] = [0, 0]
            elif what == "zero":  # 15 entries g G and one of -7 g G: the task that holds it is the infinity, first (inf+Q) or second (Q+inf)
                for i in range(2 * kmax - 1):
                    digits[at + i][w] = b + 1
                at += 2 * kmax - 1
                digits[inf0 + 16][w] = b + 1
                parts[b] = [kmax * g, 0]
                model_window(rec, plan, None, w, [p if k != b else [0, kmax * g] for k, p in enumerate(parts)])  # (counted both ways)
            else:
                for i in range(what):
                    digits[at + i][w] = b + 1
                at += what
                parts[b] = [g * n for n in small_tasks(what, kmax)]
        got = model_window(rec, plan, None, w, parts)
        values.append({b: sum(x) for b, x in enumerate(parts) if sum(x)})
        assert got == sum((b + 1) * x for b, x in values[-1].items())
    values += [{}] * (plan["W"] - len(values))
    return PlantedLaunch(plan, ks, digits, values, rec.counts)


# ---------------------------------------------------------------------------------------------------- table plans
TABLE_N = 4096               # the key of the table tests: the least the c = 20 plans take (development hook "table_slide_min")
RC_BLOCKS = 22               # clean blocks of k_rc_mid per launch: 15 of columns, 7 of rows (the last of each kind takes the other's points)
T_PLUS, T_MINUS = 1400, 500  # points +g G and -g G for the patterns planted by hand


def model_reduce_rc(rec, cells, lg_rows, lg_cols, per):
    """k_msm_reduce_rc over one set: cells {(row, col): integer} -> (column sums, row sums); the `per` steps of a lane and the levels
    of its tree, columns and rows"""
    rows, cols = 1 << lg_rows, 1 << lg_cols
    out = []
    for name, n_lines, width, cell in (("col", cols, rows // per, lambda line, k: (k, line)), ("row", rows, cols // per, lambda line, k: (line, k))):
        sums = []
        for line in range(n_lines):
            if not any(cell(line, k) in cells for k in range(width * per)):
                sums.append(rec.zero)  # (an empty line adds infinities only)
                continue
            acc = [rec.zero] * width
            for sub in range(width):
                for i in range(per):
                    acc[sub] = rec.add("k_msm_reduce_rc", "%s step" % name, acc[sub], cells.get(cell(line, sub + width * i), rec.zero), (line, sub))
            off = width >> 1
            while off >= 1:
                for sub in range(off):
                    acc[sub] = rec.add("k_msm_reduce_rc", "%s tree/%d" % (name, off), acc[sub], acc[sub + off], (line, sub))
                off >>= 1
            sums.append(acc[0])
        out.append(sums)
    return out


class TableLaunch:
    """scalars over the table key (one digit on row 0 each, or zero) and the bucket values they give: {bucket: integer}"""

    def __init__(self, ks, buckets, scalar_of, cases=None):
        self.scalars = [0] * len(ks)
        self.values = {}
        for i, b in buckets.items():
            self.scalars[i] = scalar_of(b)
            self.values[b] = self.values.get(b, 0) + ks[i]
        self.values = {b: x for b, x in self.values.items() if x}
        self.cases = cases


SHAPES = {"slide": (9, 10), "fixed": (9, 10), "small": (8, 8)}   # lg_rows, lg_cols of the row / column sums


def _cell(row, col, layout="slide"):
    """the bucket stored at (row, col): sliding plan (512 x 1024) (range, fine) = (bucket & 511, bucket >> 9); the fixed windows on
    the same table (table mode 1) and the small-key plan (256 x 256) keep the bucket index, row-major"""
    lg_rows, lg_cols = SHAPES[layout]
    assert 0 <= row < 1 << lg_rows and 0 <= col < 1 << lg_cols
    return (col << lg_rows) + row if layout == "slide" else (row << lg_cols) + col


def _scalar_of(layout):
    return slide_scalar if layout == "slide" else fixed_scalar


def table_key():
    """-> (multiples, layout): [0, 64 RC_BLOCKS) the background of the k_rc_mid cases (point 64 q + i = value i of 64), then the cases'
    own points, T_PLUS points g G, T_MINUS points -g G, infinities up to TABLE_N"""
    _, bgv, cases = build_cases(0, 0, "rc_mid")
    ks, own = [], {}
    for q in range(RC_BLOCKS):
        ks += bgv
    for case in cases:
        for e, x in case.own.items():
            own[(id(case), e)] = len(ks)
            ks.append(x)
    plus = len(ks)
    ks += [COMBINE_G] * T_PLUS
    minus = len(ks)
    ks += [-COMBINE_G] * T_MINUS
    assert len(ks) <= TABLE_N
    ks += [0] * (TABLE_N - len(ks))
    return ks, dict(own=own, plus=plus, minus=minus, cases=cases)


def slide_rc_mid_launches(layout="slide"):
    """k_rc_mid: one block of 64 column sums or 64 row sums per case of the "rc_mid" plan.  All blocks but the last of the columns and
    the last of the rows take a case (512 x 1024: 15 + 7 a launch; 256 x 256: 3 + 3); entry e of a column block sits in row
    rows - 64 + e, entry e of a row block in column cols - 64 + e -- the last blocks collect the others' points and are checked by
    definition like every pair.  launch.cases[k] = (name of the block, its case)."""
    ks, lay = table_key()
    rows, cols = 1 << SHAPES[layout][0], 1 << SHAPES[layout][1]
    ncb, nrb = cols // 64 - 1, rows // 64 - 1
    launches = []
    for at in range(0, len(lay["cases"]), ncb + nrb):
        buckets, names = {}, []
        for blk, case in enumerate(lay["cases"][at:at + ncb + nrb]):
            for e in case.values:
                i = lay["own"][(id(case), e)] if e in case.own else 64 * blk + case.bg[e]
                buckets[i] = _cell(rows - 64 + e, 64 * blk + e, layout) if blk < ncb else _cell(64 * (blk - ncb) + e, cols - 64 + e, layout)
            names.append(("column block %d" % blk if blk < ncb else "row block %d" % (blk - ncb), case))
        launches.append(TableLaunch(ks, buckets, _scalar_of(layout), names))
    return ks, launches


def _pattern(plus, minus, signs):
    """indices of the +g / -g points for a list of signs"""
    return [plus.pop() if sg > 0 else minus.pop() for sg in signs]


def structure_cells(wc, wr):
    """k_msm_reduce_rc, planted by hand over cells +-g for column trees of wc lanes (a lane takes the rows sub + wc i) and row trees
    of wr lanes (the columns sub + wr i): {(row, col): sign}.
    columns from 3 on, rows 0 .. wc - 1 (one cell per lane): all equal (P+P at every level); the sign of bit off of the lane (P-P at
    level off), off = wc / 2 .. 1; only the lanes with bit off set (inf+Q at level off), only those with it clear (Q+inf); then two
    equal cells in one lane (rows 5 and 5 + wc: P+P in the lane's steps) and two opposite ones with a third behind (P-P, inf+Q).
    rows from 100 on, the same over the columns 64 .. 64 + wr - 1 (all equal) and 64 + wr .. 64 + 2 wr - 1 (the others)."""
    cells, col, row = {}, 3, 100
    levels = lambda w: [w >> (t + 1) for t in range(w.bit_length() - 1)]
    for r in range(wc):
        cells[(r, col)] = 1
    col += 1
    for off in levels(wc):
        for r in range(wc):
            cells[(r, col)] = -1 if r & off else 1
            if r & off:
                cells[(r, col + 1)] = 1
            else:
                cells[(r, col + 2)] = 1
        col += 3
    cells.update({(5, col): 1, (5 + wc, col): 1, (6, col + 1): 1, (6 + wc, col + 1): -1, (6 + 2 * wc, col + 1): 1})
    for k in range(wr):
        cells[(row, 64 + k)] = 1
    row += 1
    for off in levels(wr):
        for k in range(wr):
            cells[(row, 64 + wr + k)] = -1 if k & off else 1
            if k & off:
                cells[(row + 1, 64 + wr + k)] = 1
            else:
                cells[(row + 2, 64 + wr + k)] = 1
        row += 3
    cells.update({(row, 72): 1, (row, 72 + wr): 1, (row + 1, 72): 1, (row + 1, 72 + wr): -1, (row + 1, 72 + 2 * wr): 1})
    return cells


def slide_structure_launch(layout="slide", per=16):
    """structure_cells for the layout's shape with `per` buckets per lane -> (key multiples, launch, {(row, col): value})"""
    ks, lay = table_key()
    plus = list(range(lay["plus"], lay["plus"] + T_PLUS))
    minus = list(range(lay["minus"], lay["minus"] + T_MINUS))
    lg_rows, lg_cols = SHAPES[layout]
    cells = structure_cells((1 << lg_rows) // per, (1 << lg_cols) // per)
    buckets = {}
    for (r, c), sg in cells.items():
        buckets[_pattern(plus, minus, [sg])[0]] = _cell(r, c, layout)
    return ks, TableLaunch(ks, buckets, _scalar_of(layout)), {rc: sg * COMBINE_G for rc, sg in cells.items()}


def slide_host_launches(layout="slide"):
    """msm_combine_member's row / column forms: every point in column 0, every point in row 0, one point in cell (0, 0).  Sliding
    plan: the columns' weighted sum equals their plain sum (cw = weighted - plain is the infinity and its doublings are skipped), the
    rows' (rw likewise), both.  Fixed windows: `cols` is all there is with `rows` - plain infinite; `rows` - plain finite beside a
    single column; both."""
    ks, lay = table_key()
    col0 = {i: _cell(i, 0, layout) for i in range(64)}
    row0 = {i: _cell(0, i, layout) for i in range(64)}
    sc = _scalar_of(layout)
    return ks, [("column 0 only", TableLaunch(ks, col0, sc)), ("row 0 only", TableLaunch(ks, row0, sc)), ("cell (0, 0) only", TableLaunch(ks, {5: _cell(0, 0, layout)}, sc))]


def cells_launch(layout, cells):
    """{(row, col): m} -> a launch whose cell (row, col) holds m g G: |m| of the key's points +g G or -g G in that bucket"""
    ks, lay = table_key()
    plus = list(range(lay["plus"], lay["plus"] + T_PLUS))
    minus = list(range(lay["minus"], lay["minus"] + T_MINUS))
    buckets = {}
    for (r, c), m in cells.items():
        for i in _pattern(plus, minus, [1 if m > 0 else -1] * abs(m)):
            buckets[i] = _cell(r, c, layout)
    return TableLaunch(ks, buckets, _scalar_of(layout))


def _pairs(blocks, row=0):
    """{block q: (S, T)} in units of g -> cells of one row: a = 2 S - T in the block's first column, b = T - S in its second"""
    cells = {}
    for q, (S, T) in blocks.items():
        for col, m in ((64 * q, 2 * S - T), (64 * q + 1, T - S)):
            if m:
                cells[(row, col)] = m
    return cells


# weighted() over the blocks' pairs, from the top block down: t += T, run += S, tot += run (q >= 1), then t + 64 tot
WEIGHTED_CASES = [
    ("t+=T P+P, run+=S P-P, then weighted - plain with plain infinite", {1: (1, 5), 0: (-1, 5)}),
    ("t+=T P-P, run+=S Q+inf, t + tot with t infinite", {1: (2, 3), 0: (0, -3)}),
    ("t + tot P+P", {1: (1, 64)}),
    ("t + tot P-P", {1: (1, -64)}),
    ("tot+=run P+P: an empty block under a full one", {2: (1, 1)}),
    ("tot+=run P-P", {2: (1, 1), 1: (-2, -2)}),
    ("tot+=run Q+inf", {2: (1, 1), 1: (-1, -1)}),
    ("weighted - plain with weighted infinite", {0: (1, 0)}),
    ("weighted - plain P+P: weighted = -plain", {0: (1, -1)}),
]
SLIDE_CROSS = [("cw + rw P+P", {(0, 1): 1, (1, 0): 512}), ("cw + rw P-P", {(0, 1): -1, (1, 0): 512}), ("+ s_all Q+inf", {(0, 1): 1, (1, 0): -1}),
               ("+ s_all P+P", {(0, 0): 1, (1, 0): 1}), ("+ s_all P-P", {(0, 0): -3, (1, 0): 1})]
FIXED_CROSS = [("cols + rows P+P", {(1, 1023): 1}), ("cols + rows P-P", {(1, 0): 1, (0, 40): -25}), ("cols + rows inf+Q", {(1, 0): 1, (0, 0): -1})]


def extra_host_launches(layout="slide"):
    """msm_combine_member's row / column forms site by site: WEIGHTED_CASES over the columns' blocks (cells of row 0) and, transposed,
    over the rows' blocks; the last additions of the layout's form (SLIDE_CROSS / FIXED_CROSS) -> (key multiples, [(name, launch)])"""
    out = []
    for name, blocks in WEIGHTED_CASES:
        cells = _pairs(blocks)
        out.append(("cols: " + name, cells_launch(layout, cells)))
        out.append(("rows: " + name, cells_launch(layout, {(c, r): m for (r, c), m in cells.items()})))
    for name, cells in SLIDE_CROSS if layout == "slide" else FIXED_CROSS:
        out.append((name, cells_launch(layout, cells)))
    return table_key()[0], out


SMALL_KEY_N = 1 << 17        # the small-key plan (c = 17, 256 x 256) takes keys of 2^17 .. 2^20 points, whole or at least half


def small_key():
    """the table key tiled to 2^17 points: the launches' scalars are zero behind the first 4096"""
    ks, _ = table_key()
    return np.ascontiguousarray(np.tile(multiples_key(len(ks), ks), (SMALL_KEY_N // len(ks), 1)))


def small_key_batches():
    """the small-key plan's launches: {members: (per, [TableLaunch per member])} -- one member (per 4, trees of 64 lanes): the planted
    cells, then the first launch of k_rc_mid cases; 4 members (per 8, 32 lanes): the cells, two launches of cases and a member whose
    scalars are all zero between them; 8 members (per 16, 16 lanes): the cells, the other launches of cases, a member of zeros"""
    ks, mids = slide_rc_mid_launches("small")
    empty = TableLaunch(ks, {}, fixed_scalar)
    st = {per: slide_structure_launch("small", per)[1] for per in (4, 8, 16)}
    assert len(mids) >= 9
    return {1: (4, [[st[4]], [mids[0]]]), 4: (8, [[st[8], mids[1], empty, mids[2]]]), 8: (16, [[st[16]] + mids[3:6] + [empty] + mids[6:9]])}


HEAVY_TASKS, HEAVY_WAVE = 70, 512


def heavy_launch(c=10):
    """k_smsm_reduce's heavy-bucket pre-sum over real partials in every quad.  A key of more than 2^14 points runs tasks of 16, a
    bucket of more than 64 entries is cut into wave tasks of 512.  Window 0: a bucket of 70 x 512 entries g G -- 70 equal partials,
    every quad takes one in the strided loop and quads 0 .. 5 a second (P+P), the others add infinity (Q+inf), the tree adds equal sums.
    Windows 1 .. 6: a bucket of 64 partials, 32767 entries g G and one sized so that its task is worth -(2^(t+1) - 1) 512 g: whichever
    quad holds it, the tree meets P-P at level 32 >> t and infinity on one side at the next.  Window 7: 64 partials, one of them
    the infinity (its odd entry is -511 g G): the tree's first level adds it on the left or on the right.
    Not possible: a block with more than 64 heavy buckets -- each needs more than 4 x 512 entries, 65 of them 133,185 points, and the
    small pipeline takes 2^16 at most.  The strided loop's P-P is strided_launch's."""
    plan = small_plan(c)
    B, g = plan["B"], COMBINE_G
    bgv = plan_background(plan)
    n_eq = HEAVY_TASKS * HEAVY_WAVE
    odd = [-(HEAVY_WAVE - 1 + HEAVY_WAVE * ((2 << t) - 1)) * g for t in range(6)]
    odd.append(-(HEAVY_WAVE - 1) * g)
    ks = list(bgv) + [g] * n_eq + odd
    eq0, odd0 = len(bgv), len(bgv) + n_eq
    while len(ks) % 8:
        ks.append(0)
    assert 1 << 14 < len(ks) <= 1 << 16
    digits, values, rec = [dict() for _ in ks], [], IntRec()
    for w in range(8):
        bucket = 100 if w == 0 else 50 + w
        parts = [[] for _ in range(B)]
        for b, i in _scatter(B, len(bgv), 0x4EA7 + w).items():
            if b != bucket:
                digits[i][w] = b + 1
                parts[b] = [bgv[i]]
        if w == 0:
            for i in range(n_eq):
                digits[eq0 + i][w] = bucket + 1
            parts[bucket] = [g * n for n in small_tasks(n_eq, 16)]
            assert len(parts[bucket]) == HEAVY_TASKS
        else:
            for i in range(64 * HEAVY_WAVE - 1):
                digits[eq0 + i][w] = bucket + 1
            digits[odd0 + w - 1][w] = bucket + 1
            task = (HEAVY_WAVE - 1) * g + odd[w - 1]
            assert small_tasks(64 * HEAVY_WAVE, 16) == [HEAVY_WAVE] * 64 and task == (-((2 << (w - 1)) - 1) * HEAVY_WAVE * g if w < 7 else 0)
            parts[bucket] = [task] + [HEAVY_WAVE * g] * 63  # (counted with the odd task in quad 0 ...)
            other = IntRec()                                # (... and in the last quad: the same level meets the P-P)
            model_window(other, plan, None, w, [p if b != bucket else p[1:] + p[:1] for b, p in enumerate(parts)])
            assert [k for k in other.counts if k[2] == "P-P" and k[1].startswith("heavy")] == ([(K_SREDUCE, "heavy tree/%d" % (32 >> (w - 1)), "P-P")] if w < 7 else [])
            for k, n in other.counts.items():
                if k[1].startswith("heavy"):
                    rec.counts[k] = rec.counts.get(k, 0) + n
        got = model_window(rec, plan, None, w, parts)
        values.append({b: sum(x) for b, x in enumerate(parts) if sum(x)})
        assert got == sum((b + 1) * x for b, x in values[-1].items())
    values += [{}] * (plan["W"] - len(values))
    return PlantedLaunch(plan, ks, digits, values, rec.counts)


STRIDED_TASKS, STRIDED_LEN, STRIDED_BG = 128, 509, 376


def strided_launch(c=10):
    """P-P in the strided loop of k_smsm_reduce's heavy pre-sum: every quad must make its second trip, so that whichever quad holds
    the odd partial adds it to a real one.  A bucket of more than 127 x 512 entries is 128 wave tasks, split evenly (bucket_tasks,
    k_smsm_sort): 128 x 509 = 65,152 entries -- 65,151 of g G and one of -1017 g G -- are 128 partials of 509 g but for the one that
    holds the odd entry, -509 g.  Its quad meets 509 g + (-509 g) or the reverse on its second trip; the other 63 add equal partials
    (P+P); the tree's first level then has the infinity on one side.  With 376 background points the key has 2^16 - 8 points, the
    most the small pipeline takes being 2^16."""
    plan = small_plan(c)
    B, g = plan["B"], COMBINE_G
    bgv = plan_background(plan)[:STRIDED_BG]
    n_eq = STRIDED_TASKS * STRIDED_LEN - 1
    ks = list(bgv) + [g] * n_eq + [-(2 * STRIDED_LEN - 1) * g]
    assert len(ks) % 8 == 0 and 1 << 14 < len(ks) <= 1 << 16
    digits, rec, bucket = [dict() for _ in ks], IntRec(), 77
    parts = [[] for _ in range(B)]
    for b, i in _scatter(B, len(bgv), 0x57D1).items():
        if b != bucket:
            digits[i][0] = b + 1
            parts[b] = [bgv[i]]
    for i in range(n_eq + 1):
        digits[len(bgv) + i][0] = bucket + 1
    assert small_tasks(n_eq + 1, 16) == [STRIDED_LEN] * STRIDED_TASKS
    odd = (STRIDED_LEN - 1) * g - (2 * STRIDED_LEN - 1) * g
    assert odd == -STRIDED_LEN * g
    for at in (0, 5, 64, 127):  # wherever the odd partial lands: its quad's second trip meets the P-P, and nothing else does
        other = IntRec()
        tasks = [STRIDED_LEN * g] * at + [odd] + [STRIDED_LEN * g] * (STRIDED_TASKS - 1 - at)
        model_window(other, plan, None, 0, [p if b != bucket else tasks for b, p in enumerate(parts)])
        assert [k for k in other.counts if k[2] == "P-P"] == [(K_SREDUCE, "heavy strided", "P-P")] and other.counts[(K_SREDUCE, "heavy strided", "P-P")] == 1
        if at in (0, 127):  # (counted with it first and with it last)
            rec.merge(other)
    parts[bucket] = [odd] + [STRIDED_LEN * g] * (STRIDED_TASKS - 1)
    values = [{b: sum(x) for b, x in enumerate(parts) if sum(x)}] + [{}] * (plan["W"] - 1)
    assert values[0][bucket] == (STRIDED_TASKS - 2) * STRIDED_LEN * g
    return PlantedLaunch(plan, ks, digits, values, rec.counts)


REDUCE1_C = 16               # the general pipeline's plan for every table-free MSM of >= 2^20 points: 2^15 buckets per window
REDUCE1_SPANS = [(0, 8, 64), (64, 64, 8)]   # (reduce span, L, nseg) of its k_msm_reduce1 + k_smsm_final


def reduce1_launch(span):
    """k_msm_reduce1 + k_smsm_final at 2^15 buckets per window, planted by hand over 64 points +g G and 64 points -g G, one point in
    the first bucket of a lane (bucket L l of segment 0) or of a segment (64 L s).  Window 0: the 64 lanes all equal, windows 1 .. 6:
    with the sign of bit 32 >> t of the lane -- equal and opposite lane sums at every level of the wave's scan and tree; then the
    segments all equal and, one window per level of k_smsm_final, with the sign of bit nseg >> t of the segment.  Point l (64
    + l for the minus sign) serves lane or segment l of every window: the key has 128 points."""
    plan = general_plan(REDUCE1_C, span)
    L, nseg, g = plan["L"], plan["nseg"], COMBINE_G
    ks = [g] * 64 + [-g] * 64
    digits, values = [dict() for _ in ks], []
    levels = nseg.bit_length() - 1
    for w in range(7 + 1 + levels):
        step, units, t = (L, 64, w) if w < 7 else (64 * L, nseg, w - 7)
        v = {}
        for k in range(units):
            neg = t > 0 and bool(k & (units >> t))
            digits[64 + k if neg else k][w] = step * k + 1
            v[step * k] = -g if neg else g
        values.append(v)
    assert len(values) <= plan["W"] - 1
    rec = IntRec()
    for w, v in enumerate(values):
        model_window(rec, plan, [v.get(b, 0) for b in range(plan["B"])], w)
    values += [{}] * (plan["W"] - len(values))
    return PlantedLaunch(plan, ks, digits, values, rec.counts)


# ---------------------------------------------------------------------------------------------------- the host's table forms
def model_host_rc(rec, plan, values, cv=lambda m: m):
    """msm_combine_member over the (S, T) pairs of one set (one piece): weighted() over the columns' and the rows' blocks, the
    `- plain` subtractions and the last additions of the sliding form (cw + rw + s_all) or of the fixed one (cols + 2^lg_cols (rows -
    plain)), with their guarded doublings -> the member's point as an integer"""
    recs = [cv(m) for _, m in expected_records(dict(plan, pieces=1), [values])]
    cblocks, rblocks = (1 << plan["lg_cols"]) // 64, (1 << plan["lg_rows"]) // 64
    pair = lambda q: (recs[2 * q], recs[2 * q + 1])

    def weighted(first, count, name):
        t = run = tot = rec.zero
        for q in range(count - 1, -1, -1):
            S, T = pair(first + q)
            t = rec.add(K_HOST, "%s t+=T" % name, t, T, q)
            run = rec.add(K_HOST, "%s run+=S" % name, run, S, q)
            if q >= 1:
                tot = rec.add(K_HOST, "%s tot+=run" % name, tot, run, q)
        for k in range(6):
            if not rec.is_inf(tot):
                tot = rec.dbl(K_HOST, "%s dbl" % name, tot)
        return rec.add(K_HOST, "%s t+tot" % name, t, tot), run

    wc_, s_cols = weighted(0, cblocks, "cols")
    wr_, s_rows = weighted(cblocks, rblocks, "rows")
    if plan["pipeline"] == 3:
        cw = rec.add(K_HOST, "cols - plain", wc_, rec.neg(s_cols))
        rw = rec.add(K_HOST, "rows - plain", wr_, rec.neg(s_rows))
        for k in range(plan["lg_rows"] + 1):
            if not rec.is_inf(cw):
                cw = rec.dbl(K_HOST, "cw dbl", cw)
        if not rec.is_inf(rw):
            rw = rec.dbl(K_HOST, "rw dbl", rw)
        return rec.add(K_HOST, "+ s_all", rec.add(K_HOST, "cw + rw", cw, rw), s_rows)
    rows = rec.add(K_HOST, "rows - plain", wr_, rec.neg(s_rows))
    for k in range(plan["lg_cols"]):
        if not rec.is_inf(rows):
            rows = rec.dbl(K_HOST, "rows dbl", rows)
    return rec.add(K_HOST, "cols + rows", wc_, rows)


PLAN_OF_LAYOUT = {"slide": dict(pipeline=3, form=2, lg_rows=9, lg_cols=10), "fixed": dict(pipeline=2, form=2, lg_rows=9, lg_cols=10),
                  "small": dict(pipeline=2, form=2, lg_rows=8, lg_cols=8)}


def planted_counts():
    """what the launches planted by hand meet, by the models: {(kernel, site, class): count}, over every launch of the GPU module --
    k_msm_combine (combine_launch), the partial loop and the heavy pre-sum of k_smsm_reduce (partials_launch, heavy_launch, strided_launch),
    k_msm_reduce_rc in its five shapes, the host's Horner and its row / column forms over every table launch.  Where the sort's atomics decide which task holds an odd entry the launch is counted with it first and with
    it last: the device meets one of the two."""
    rec = IntRec()
    for launch in (combine_launch(), partials_launch(), heavy_launch(), strided_launch(), horner_launch(7), horner_launch(13)):
        rec.merge(IntRec.of(launch.counts))
    tables = []
    for layout in ("slide", "fixed"):
        _, st, cells = slide_structure_launch(layout)
        model_reduce_rc(rec, cells, 9, 10, 16)
        tables += [(layout, l) for l in [st] + slide_rc_mid_launches(layout)[1] + [l for _, l in slide_host_launches(layout)[1] + extra_host_launches(layout)[1]]]
    for members, (per, batches) in small_key_batches().items():
        for batch in batches:
            for l in batch:
                model_reduce_rc(rec, {(b >> 8, b & 255): x for b, x in l.values.items()}, 8, 8, per)
                tables.append(("small", l))
    for layout, l in tables:
        assert abs(model_host_rc(rec, PLAN_OF_LAYOUT[layout], l.values)) < LIMIT
    return {k: n for k, n in rec.counts.items() if k[0] in (K_COMBINE, K_HOST, "k_msm_reduce_rc") or k[1].startswith(("partial", "heavy"))}


def planted_sites(counts):
    return sorted({(k, s) for k, s, _ in counts if "dbl" not in s})


# Sites where the sort's atomics decide which task holds an odd entry: the level of the event is fixed by construction, its side is
# not.  planted_counts counts both placements there, a run on the device meets ONE of inf+Q and Q+inf from those buckets.
EITHER_SIDE = ([(K_COMBINE, s) for s in ["serial", "strided"] + ["tree/%d" % (32 >> t) for t in range(6)]] +
               [(K_SREDUCE, s) for s in ["partial"] + ["heavy tree/%d" % (32 >> t) for t in range(6)]])


# ---------------------------------------------------------------------------------------------------- checkers
def expected_records(plan, values):
    """the records halo_dev_msm_window_sums gives for this plan, by their DEFINITION: [(name, integer m)], the record is m G.
    plan: the fields of halo_dev_msm_last_plan.  values: general and small pipeline -- one {bucket: integer} per record, member
    after member, window after window; table plans -- one {bucket: integer} per set, the bucket as the digit names it (sliding:
    (d - 1) / 2; fixed windows: d - 1)."""
    out = []
    if plan["form"] in (0, 1) and plan["pipeline"] in (0, 1):
        for r, v in enumerate(values):
            out.append(("window %d" % r, sum((b + 1) * x for b, x in v.items())))
        return out
    assert plan.get("pieces", 1) == 1
    lg_rows, lg_cols = plan["lg_rows"], plan["lg_cols"]
    rows, cols = 1 << lg_rows, 1 << lg_cols
    for s, v in enumerate(values):
        C, Rw = [0] * cols, [0] * rows
        for b, x in v.items():
            g = slide_index(b, lg_rows, lg_cols) if plan["pipeline"] == 3 else b
            C[g & (cols - 1)] += x
            Rw[g >> lg_cols] += x
        for name, E in (("column", C), ("row", Rw)):
            for q in range(len(E) // 64):
                blk = E[64 * q:64 * q + 64]
                out.append(("set %d %s block %d S" % (s, name, q), sum(blk)))
                out.append(("set %d %s block %d T" % (s, name, q), sum((Q + 1) * e for Q, e in enumerate(blk))))
    return out


def _case_of(cases, r, name):
    """what the record was built for: the window's case, or the case of the block of k_rc_mid a pair belongs to (TableLaunch.cases of
    every set: lists of (block name, case))"""
    if cases is None:
        return None
    if cases and isinstance(cases[0], list):
        words = name.split()  # "set s column block q S"
        for blk, case in cases[int(words[1])] or []:
            if blk == " ".join(words[2:5]):
                return case.name()
        return None
    return cases[r].name() if r < len(cases) else None


def check_window_sums(readback, plan, values, cases=None):
    """every read-back record (count x 12 Jacobian words), made canonical, against m G -> the failing (index, name, m, what the
    case at that window was built for)"""
    readback = np.asarray(readback, dtype=np.uint64).reshape(-1, 12)
    want = expected_records(plan, values)
    if len(want) != len(readback):
        return [(-1, "%d records read back, the plan's layout has %d" % (len(readback), len(want)), 0, None)]
    bad = []
    for r, (name, m) in enumerate(want):
        if orc.point_canonical(readback[r]) != multiple(m):
            bad.append((r, name, m, _case_of(cases, r, name)))
    return bad


def describe(bad, limit=8):
    """a failure message: how many, the first few with their window or pair, the multiple expected and the targeted site and class"""
    return "%d wrong records; first (index, record, expected multiple of G, case): %s" % (len(bad), bad[:limit])
