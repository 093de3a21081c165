"""The cases of the Fr kernels' launch plans (csrc/fr_plan.hpp), shared by tests/test_fr_plan_cases_cpu.py and
tests/test_gpu_fr_plans.py: one seeded builder, no case skipped or sampled.

The kernels of csrc/fr_vec.hip and csrc/hpoly.hip K4 - K9 are exact, so only their indexing can be wrong, and the indexing follows a plan that depends
on the size: the chain length E (elements per lane), the number of 4-bit windows of the exponent (nwin), the grid and -- where
the grid is capped -- the trips of a lane through its loop.  A case names a kernel, a size, the hooks it runs under and the plan
it claims; `model_plan` is this file's own restatement of fr_plan.hpp, which the CPU test holds against halo_dev_fr_plan for
every case and the GPU test asserts again before it launches ("nothing here would test ...").

Tail kinds of a case (what the last wave / trip looks like), as the coverage table names them:
    full      every chain of the last wave is whole
    in-wave   the data end inside the last wave's first 64 elements (idle lanes) or inside a chain (short chains)
    idle      whole waves (or whole blocks) of the grid have nothing to do in the last trip
"""
import random
from collections import Counter, namedtuple

import numpy as np

import lazy_cases as lz
import pallas_model as pm

R = pm.R_ORDER
SEED = 0x4652504C  # "FRPL"
CTX_LG = 17        # the GPU tests' context: 2^17 points, buffers of 2^17 x 32 bytes at most
CTX_N = 1 << CTX_LG

POW_ES = [0, 8, 16, 32, 64]      # 0: the default plan (no hook)
BIG_EDGE_ES = [0, 8, 16]         # the window-count edges from 65536 on
H_ES = [0, 8, 16, 64]
H_LGS = [8, 9, 12, 13, 16, 17]   # 17: the smallest size at which the high table has a second entry
H_EVAL_LGS = [13, 17, 20, 24]
BLOCK_HOOKS = [1, 2, 3]          # poly_blocks / dot_blocks of the trip cases
TRIP_ES = POW_ES                 # chain lengths of k_poly_eval_partial's trip cases
TRIP_COUNTS = [2, 3, 4]
TRIP_TAILS = ["full", "in-wave", "idle"]
# (E, poly_blocks, trips, tail) of the trip cases that need more than the context's 2^17 coefficients -- all at E = 64 under
# poly_blocks = 3, a trip of 49152 coefficients: three full trips (147456) and every fourth trip (from 151552); poly_trip_cases
# asserts that it leaves out these and no others
TRIPS_PAST_THE_CONTEXT = {(64, 3, 3, "full")} | {(64, 3, 4, tail) for tail in TRIP_TAILS}
WINDOW_EDGES = [16, 17, 256, 257, 4096, 4097, 65536, 65537, (1 << 17) - 1, 1 << 17]
ONE_HOT_POSITIONS = [0, 15, 16, 63, 64, 255, 256, 4095, 4096, 65535, 65536]  # + W - 1, W, len - 1

_rng = random.Random(SEED)
Z_SCALARS = {"0": 0, "1": 1, "r-1": R - 1, "2": 2, "random a": _rng.randrange(3, R - 1), "random b": _rng.randrange(3, R - 1)}
ALPHAS = [R - 1, 0, 1, 2, R - 1, (R - 1) // 2, (1 << 254) % R]  # (tests/test_gpu_lazy_bounds.py: one per extreme vector)

# the plan's defaults, restated (csrc/fr_plan.hpp)
BEST_E = {"powers": 8, "poly_eval": 16, "h_coeffs": 4}
GRID_CAP, DOT_CAP = 1024, 512

Plan = namedtuple("Plan", "E nwin blocks trips")
Case = namedtuple("Case", "kernel n pow_e blocks_hook plan tail")  # pow_e / blocks_hook 0: not set; "dot2": the two-sum form of "dot"
PLAN_OF = {"powers": "powers", "poly_eval": "poly_eval", "dot": "dot", "dot2": "dot", "h_coeffs": "h_coeffs"}  # -> halo_dev_fr_plan's name


def ceil_div(a, b):
    return -(-a // b)


def bits_for(n):
    return max(1, (n - 1).bit_length())


def chain_len(kernel, n, pow_e=0, env_e=0):
    if pow_e or env_e:
        return pow_e or env_e
    e = BEST_E[kernel]
    while e > 4 and n // (64 * e) < 1024:
        e >>= 1
    return e


def model_plan(kernel, n, pow_e=0, blocks_hook=0, env_e=0, env_dot=0):
    """fr_plan.hpp in Python integers: hook, then environment, then default"""
    if kernel in ("dot", "dot2"):
        cap = blocks_hook or env_dot or DOT_CAP
        blocks = max(1, min(ceil_div(ceil_div(n, 2), 256), cap))
        return Plan(2, 0, blocks, max(1, ceil_div(n, 512 * blocks)))
    E = chain_len(kernel, n, pow_e, env_e)
    waves = ceil_div(n, 64 * E)
    blocks = ceil_div(waves, 4)
    if kernel == "powers":
        return Plan(E, ceil_div(bits_for(n), 4), blocks, 1)
    if kernel == "h_coeffs":
        return Plan(E, 0 if n < 2 else ceil_div(bits_for(n), 8), blocks, 1)
    assert kernel == "poly_eval"
    blocks = max(1, min(blocks, blocks_hook or GRID_CAP))
    return Plan(E, ceil_div(bits_for(n), 4), blocks, max(1, ceil_div(waves, 4 * blocks)))


def tail_kind(kernel, n, plan):
    """how the last trip of the grid ends (module docstring)"""
    if kernel in ("dot", "dot2"):
        per_trip = 512 * plan.blocks
        last = n - (plan.trips - 1) * per_trip
        if last == per_trip:
            return "full"
        return "idle" if ceil_div(min(last, per_trip // 2), 64) < 4 * plan.blocks else "in-wave"
    W = 64 * plan.E
    waves = ceil_div(n, W)
    if kernel == "poly_eval" and plan.trips > 1:
        last_waves = waves - (plan.trips - 1) * 4 * plan.blocks
        if last_waves < 4 * plan.blocks:
            return "idle" if n % W == 0 else "in-wave"
    return "full" if n % W == 0 else "in-wave"


def lengths_for(E):
    W = 64 * E
    return sorted({1, 2, 63, 64, 65, W - 1, W, W + 1, 4 * W - 1, 4 * W, 4 * W + 1, 4 * W + 65, 7 * W + 17})


def edges_for(pow_e):
    return [n for n in WINDOW_EDGES if n < 65536 or pow_e in BIG_EDGE_ES]


def one_hot_positions(n, W):
    return sorted({p for p in ONE_HOT_POSITIONS + [W - 1, W, n - 1] if p < n})


def _case(kernel, n, pow_e=0, blocks_hook=0):
    plan = model_plan(kernel, n, pow_e, blocks_hook)
    return Case(kernel, n, pow_e, blocks_hook, plan, tail_kind(kernel, n, plan))


def chain_cases(kernel):
    """powers / poly_eval under every chain length: the lengths around a wave's W = 64 E elements and the window-count edges"""
    out = []
    for pow_e in POW_ES:
        E = chain_len(kernel, 1, pow_e)
        for n in sorted(set(lengths_for(E)) | set(edges_for(pow_e))):
            assert n <= CTX_N
            out.append(_case(kernel, n, pow_e))
    return out


def poly_trip_cases():
    """k_poly_eval_partial's grid-stride loop under poly_blocks = 1, 2, 3 and every chain length: 2, 3 and 4 trips, the last one
    (a) full, (b) ending inside a wave, (c) with whole waves idle.  T = 4 poly_blocks W elements per trip.  Every case that the
    context holds: TRIPS_PAST_THE_CONTEXT names the others."""
    out, left_out = [], set()
    for pow_e in TRIP_ES:
        E = chain_len("poly_eval", 1, pow_e)
        W = 64 * E
        for pb in BLOCK_HOOKS:
            T = 4 * pb * W
            for trips in TRIP_COUNTS:
                for n, tail in zip((trips * T, (trips - 1) * T + W + 37, (trips - 1) * T + W), TRIP_TAILS):
                    if n > CTX_N:
                        left_out.add((E, pb, trips, tail))
                        continue
                    c = _case("poly_eval", n, pow_e, pb)
                    assert c.plan.trips == trips and c.tail == tail and c.plan.blocks == pb and c.plan.E == E, c
                    out.append(c)
    assert left_out == TRIPS_PAST_THE_CONTEXT, left_out
    return out


def dot_cases():
    """k_dot2_partial: the default plan over the lengths of the default chain, then dot_blocks = 1, 2, 3 -- a trip takes T = 512
    dot_blocks elements, a lane the elements i and i + T / 2 of it.  Odd tails: the zeroed second slot in the last trip (.. + T / 2
    + 33: the lanes from 33 on) and in a middle lane's ONLY trip (m = T / 2 + 33)."""
    out = [_case("dot", n) for n in sorted(set(lengths_for(4)) | {16, 17, 257, 4096, 4097})]
    for db in BLOCK_HOOKS:
        T = 512 * db
        out.append(_case("dot", T // 2 + 33, 0, db))
        for trips in (2, 3, 4):
            for n in (trips * T, (trips - 1) * T + 64 + 37, (trips - 1) * T + 128, (trips - 1) * T + T // 2 + 33, (trips - 1) * T + 1):
                c = _case("dot", n, 0, db)
                assert c.plan.trips == trips and c.plan.blocks == db, c
                out.append(c)
    return out


def dot2_cases():
    """the two-sum form: m = 257 and 1025 (vectors of 2 m) under dot_blocks 1 and 2, and the powers of two an IPA round reaches"""
    return [_case("dot2", m, 0, db) for m in (257, 1025, 256, 1024) for db in (1, 2)]


def h_cases():
    return [_case("h_coeffs", 1 << lg, pow_e) for lg in H_LGS for pow_e in H_ES]


def all_cases():
    return chain_cases("powers") + chain_cases("poly_eval") + poly_trip_cases() + dot_cases() + dot2_cases() + h_cases()


def coverage(cases):
    """(kernel, E, nwin, trips (4 = 4 or more), tail) -> number of cases"""
    return Counter((c.kernel, c.plan.E, c.plan.nwin, min(c.plan.trips, 4), c.tail) for c in cases)


def coverage_table(cases):
    rows = ["%-10s %3s %5s %6s  %-8s %s" % ("kernel", "E", "nwin", "trips", "tail", "cases")]
    for (k, E, nwin, trips, tail), cnt in sorted(coverage(cases).items()):
        rows.append("%-10s %3d %5d %6s  %-8s %d" % (k, E, nwin, "%d%s" % (trips, "+" if trips == 4 else ""), tail, cnt))
    return "\n".join(rows)


def promised_cells():
    """what the lists above promise, as predicates over the coverage cells: (description, function of a cell)"""
    want = []
    for k in ("powers", "poly_eval"):
        for E in (4, 8, 16, 32, 64):
            for tail in ("full", "in-wave"):
                want.append(("%s E=%d tail %s" % (k, E, tail), lambda c, k=k, E=E, tail=tail: c[0] == k and c[1] == E and c[4] == tail))
            for nwin in (1, 2, 3, 4) + ((5,) if E <= 16 else ()):
                want.append(("%s E=%d nwin=%d" % (k, E, nwin), lambda c, k=k, E=E, nwin=nwin: c[0] == k and c[1] == E and c[2] == nwin))
    for E in (4, 8, 16, 32, 64):  # (a cell holds the cases of every poly_blocks: at E = 64 a fourth trip is there under 1 and 2)
        for trips in TRIP_COUNTS:
            for tail in TRIP_TAILS:
                want.append(("poly_eval E=%d trips=%d tail %s" % (E, trips, tail),
                             lambda c, E=E, trips=trips, tail=tail: c[0] == "poly_eval" and c[1] == E and c[3] == trips and c[4] == tail))
    for trips in (1, 2, 3, 4):
        for tail in ("full", "in-wave", "idle"):
            want.append(("dot trips=%d tail %s" % (trips, tail), lambda c, trips=trips, tail=tail: c[0] == "dot" and c[3] == trips and c[4] == tail))
    for E in (4, 8, 16, 64):
        for nwin in (1, 2, 3):
            want.append(("h_coeffs E=%d tables=%d" % (E, nwin), lambda c, E=E, nwin=nwin: c[0] == "h_coeffs" and c[1] == E and c[2] == nwin))
    return want


# ------------------------------------------------------------------------------------------------ data
def fr_words(xs):
    """ints -> (n, 4) uint64 arkworks words, as lazy_cases.fr_mont (which is held against this in the CPU test), at 2^17 elements"""
    n = len(xs)
    if n > 4 and xs == xs[:2] * (n // 2) + xs[: n % 2]:  # the constant and alternating vectors
        return np.ascontiguousarray(np.resize(lz.fr_mont(xs[:2]), (n, 4)))
    buf = b"".join([(x * pm.MONT_R % R).to_bytes(32, "little") for x in xs])
    return np.frombuffer(buf, dtype="<u8").reshape(-1, 4).astype(np.uint64)


def dense_vectors(n):
    """name -> (ints, words): the vectors of lazy_cases.fr_extreme_vectors"""
    return {k: (v, fr_words(v)) for k, v in lz.fr_extreme_vectors(n).items()}


def one_hot(n, p, seed):
    """a single random non-zero coefficient at position p -> (c, words)"""
    c = random.Random(SEED ^ (seed * 0x9E3779B1 + 131 * n + p)).randrange(1, R)
    w = np.zeros((n, 4), dtype=np.uint64)
    w[p] = lz.fr_mont([c])[0]
    return c, w


def random_ints(n, seed):
    rng = random.Random(SEED + 7919 * seed + n)
    return [rng.randrange(R) for _ in range(n)]


def h_challenges(lg_n):
    """name -> ints of length lg_n + 1: the extreme vectors, plus two random ones"""
    vecs = dict(lz.fr_extreme_vectors(lg_n + 1))
    vecs["random a"] = random_ints(lg_n + 1, 1)
    vecs["random b"] = random_ints(lg_n + 1, 2)
    return vecs
