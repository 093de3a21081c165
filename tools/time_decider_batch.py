"""The acc_cmp_s shape (benches/acc.rs:100-106: k x acc::decider) timed two ways: the serial halo_acc_decider loop and ONE
halo_acc_decider_batch, alternating in the same process after a warm-up of each shape.  For every n one acc_compare chain of
1000 accumulators (random_instance + prover, benches/acc.rs:76-98) on a 2^14-point URS context; k in {10, 100, 1000} of its
accumulators.  Also a sweep of the batch's members per MSM launch (the development hook check_batch_group) at k = 100, and with
--big a 2^20-point leg (a chain of 10 on a 2^20-point context).  Statuses of both ways must be equal and all 0.  Prints one
JSON line; every time is the median of --reps alternating runs, in ms.

--combined: the three-way leg instead -- loop / exact batch (halo_acc_decider_batch) / combined batch
(halo_acc_decider_batch_combined: ONE MSM for all members), alternating in one process, over k independent accumulators
(random_instance_batch + prover_batch: a decider's work does not depend on what its accumulator accumulated).  n in --sizes with k
in {10, 100, 1000}; with --big n = 2^20 on its own context with k in {10, 100}.  Every row keeps median, least and greatest of
--reps runs of each way, and says whether the combined call's range lies below the exact batch's.  Also the sweep of the combined
call's right side (the development hook check_combined_usum: 1 the host pool, 2 the device) over the member count.

--fused: the four-way leg -- loop / exact batch / combined batch / fused batch (halo_acc_decider_batch_fused: the succinct
relations in the one relation too), alternating in one process over the same k independent accumulators.  n in {2^9, 2^12, 2^14}
(--sizes changes them) with k in {10, 100, 1000}; with --big n = 2^20 on its own context with k in {10, 100}.  The baseline is
the combined call of the same run.  Every row keeps median, least and greatest of --reps runs (5 unless given) of each way and
says whether the ranges of the fused and the combined call lie apart, and which way."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import halo_accumulation_amd as h  # noqa: E402
from halo_accumulation_amd import acc as A  # noqa: E402
from halo_accumulation_amd._lib import ptr  # noqa: E402

# acc_cmp_s_{n}_{k}, ms (report/report.md:2129-2158; the 8196 row is n = 8192 in the code)
PUBLISHED_MS = {
    10: [94.834, 151.25, 258.92, 453.55, 838.05, 1522.7],
    100: [940.91, 1504.2, 2557.9, 4494.5, 8372.3, 15253.0],
    1000: [9438.1, 15087.0, 25621.0, 44970.0, 82643.0, 152630.0],
}
SIZES = [512, 1024, 2048, 4096, 8192, 16384]


def build_chain(ctx, n, k, seed):
    d = n - 1
    rng = [seed]
    accs, acc = [], None
    for _ in range(k):
        q = A.random_instance(ctx, rng, d)
        qs = [q] if acc is None else [A.instance_from_accumulator(ctx, acc, d), q]
        acc = A.prover(ctx, rng, d, qs)
        accs.append(acc)
    return accs


def serial(ctx, ptrs):
    t = time.perf_counter()
    st = [ctx.lib.halo_acc_decider(ctx.h, p) for p in ptrs]
    return (time.perf_counter() - t) * 1e3, st


def batched(ctx, d, blob, k):
    st = (C.c_int * k)()
    t = time.perf_counter()
    rc = ctx.lib.halo_acc_decider_batch(ctx.h, d, ptr(blob), k, st)
    ms = (time.perf_counter() - t) * 1e3
    assert rc == 0, ctx.lib.halo_last_error()
    return ms, list(st)


def time_shape(ctx, d, accs, k, reps):
    ptrs = [ptr(a) for a in accs[:k]]
    blob = np.ascontiguousarray(np.concatenate(accs[:k]))
    s_ms, b_ms = [], []
    s_st = b_st = None
    serial(ctx, ptrs)  # warm-up of each shape
    batched(ctx, d, blob, k)
    for _ in range(reps):
        ms, s_st = serial(ctx, ptrs)
        s_ms.append(ms)
        ms, b_st = batched(ctx, d, blob, k)
        b_ms.append(ms)
    assert s_st == b_st == [0] * k, "statuses differ or a member was rejected"
    return statistics.median(s_ms), statistics.median(b_ms)


def combined(ctx, d, blob, k):
    st = (C.c_int * k)()
    t = time.perf_counter()
    rc = ctx.lib.halo_acc_decider_batch_combined(ctx.h, d, ptr(blob), k, None, st)
    ms = (time.perf_counter() - t) * 1e3
    assert rc == 0, ctx.lib.halo_last_error()
    return ms, list(st)


def fused(ctx, d, blob, k):
    st = (C.c_int * k)()
    t = time.perf_counter()
    rc = ctx.lib.halo_acc_decider_batch_fused(ctx.h, d, ptr(blob), k, None, st)
    ms = (time.perf_counter() - t) * 1e3
    assert rc == 0, ctx.lib.halo_last_error()
    return ms, list(st)


def stats(ms):
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def independent_accs(ctx, n, k, seed):
    d = n - 1
    rng = [seed]
    qs = A.random_instance_batch(ctx, rng, d, k)
    accs, codes = A.prover_batch(ctx, rng, d, [[q] for q in qs])
    assert codes == [0] * k
    return accs


def time_three(ctx, d, accs, k, reps):
    """-> {"loop": stats, "batch": stats, "combined": stats} of `reps` alternating runs after a warm-up of each"""
    ptrs = [ptr(a) for a in accs[:k]]
    blob = np.ascontiguousarray(np.concatenate(accs[:k]))
    ways = {"loop": lambda: serial(ctx, ptrs), "batch": lambda: batched(ctx, d, blob, k), "combined": lambda: combined(ctx, d, blob, k)}
    ms = {w: [] for w in ways}
    for fn in ways.values():
        fn()
    for _ in range(reps):
        for w, fn in ways.items():
            t, st = fn()
            assert st == [0] * k, "a member was rejected"
            ms[w].append(t)
    row = {w: stats(v) for w, v in ms.items()}
    row["combined_faster_than_batch"] = max(ms["combined"]) < min(ms["batch"])  # the ranges apart
    row["batch_faster_than_combined"] = max(ms["batch"]) < min(ms["combined"])
    row["batch_over_combined"] = round(statistics.median(ms["batch"]) / statistics.median(ms["combined"]), 2)
    return row


def time_four(ctx, d, accs, k, reps):
    """-> {"loop" | "batch" | "combined" | "fused": stats} of `reps` alternating runs after a warm-up of each, and how the fused
    call's range lies against the combined call's"""
    ptrs = [ptr(a) for a in accs[:k]]
    blob = np.ascontiguousarray(np.concatenate(accs[:k]))
    ways = {"loop": lambda: serial(ctx, ptrs), "batch": lambda: batched(ctx, d, blob, k), "combined": lambda: combined(ctx, d, blob, k),
            "fused": lambda: fused(ctx, d, blob, k)}
    ms = {w: [] for w in ways}
    for fn in ways.values():
        fn()
    for _ in range(reps):
        for w, fn in ways.items():
            t, st = fn()
            assert st == [0] * k, "a member was rejected"
            ms[w].append(t)
    row = {w: stats(v) for w, v in ms.items()}
    row["fused_runs"] = [round(v, 3) for v in ms["fused"]]
    row["combined_runs"] = [round(v, 3) for v in ms["combined"]]
    row["every_fused_run_beats_every_combined_run"] = max(ms["fused"]) < min(ms["combined"])  # won: the ranges apart
    row["every_combined_run_beats_every_fused_run"] = max(ms["combined"]) < min(ms["fused"])
    row["combined_over_fused"] = round(statistics.median(ms["combined"]) / statistics.median(ms["fused"]), 2)
    return row


def main_fused(a):
    rows = []
    sizes = [int(x) for x in a.sizes.split(",")] if a.sizes_given else [1 << 9, 1 << 12, 1 << 14]
    reps = a.reps if a.reps_given else 5
    ctx = h._lib.Context(urs_n=1 << 14)
    try:
        for n in sizes:
            accs = independent_accs(ctx, n, a.chain, 0x48414C4F00000500 + n)
            for k in (10, 100, 1000):
                if k <= len(accs):
                    rows.append({"n": n, "k": k, **time_four(ctx, n - 1, accs, k, reps)})
                    print(rows[-1], file=sys.stderr, flush=True)
    finally:
        ctx.close()
    if a.big:
        n = 1 << 20
        c = h._lib.Context(urs_n=n)
        try:
            accs = independent_accs(c, n, 100, 0x48414C4F00000600)
            for k in (10, 100):
                rows.append({"n": n, "k": k, **time_four(c, n - 1, accs, k, reps)})
                print(rows[-1], file=sys.stderr, flush=True)
        finally:
            c.close()
    print(json.dumps({"tool": "tools/time_decider_batch.py --fused", "workload": "k x acc::decider over k independent accumulators, 1 GPU: "
                      "the halo_acc_decider loop, halo_acc_decider_batch, halo_acc_decider_batch_combined and halo_acc_decider_batch_fused, "
                      "alternating; contexts of 2^14 points (n = 2^20: its own); baseline = the combined call of the same run",
                      "reps": reps, "unit": "ms", "rows": rows, "statuses": "all 0 in every run of every way"}))


def usum_sweep(ctx, d, accs, reps):
    """the combined call with its right side forced to the pool (1) and to the device (2), alternating, by member count"""
    out = []
    for k in (2, 4, 8, 16, 32, 64, 128, 256, 512, 1000):
        if k > len(accs):
            continue
        blob = np.ascontiguousarray(np.concatenate(accs[:k]))
        ms = {1: [], 2: []}
        for warm in (True, False):
            for _ in range(1 if warm else reps):
                for side in (1, 2):
                    h._lib.dev_hook("check_combined_usum", side)
                    try:
                        t, st = combined(ctx, d, blob, k)
                    finally:
                        h._lib.dev_hook("reset", 0)
                    assert st == [0] * k
                    if not warm:
                        ms[side].append(t)
        out.append({"k": k, "pool_ms": stats(ms[1]), "device_ms": stats(ms[2]), "pool_runs": [round(v, 3) for v in ms[1]],
                    "device_runs": [round(v, 3) for v in ms[2]],
                    "every_device_run_beats_every_pool_run": max(ms[2]) < min(ms[1]),
                    "every_pool_run_beats_every_device_run": max(ms[1]) < min(ms[2])})
    return out


def main_combined(a):
    rows, sweep = [], []
    sizes = [int(x) for x in a.sizes.split(",")]
    ctx = h._lib.Context(urs_n=1 << 14)
    try:
        for n in sizes:
            accs = independent_accs(ctx, n, a.chain, 0x48414C4F00000300 + n)
            for k in (10, 100, 1000):
                if k <= len(accs):
                    rows.append({"n": n, "k": k, **time_three(ctx, n - 1, accs, k, a.reps)})
                    print(rows[-1], file=sys.stderr, flush=True)
            if a.sweep and n == sizes[0]:
                sweep = usum_sweep(ctx, n - 1, accs, a.reps)
    finally:
        ctx.close()
    if a.big:
        n = 1 << 20
        c = h._lib.Context(urs_n=n)
        try:
            accs = independent_accs(c, n, 100, 0x48414C4F00000400)
            for k in (10, 100):
                rows.append({"n": n, "k": k, **time_three(c, n - 1, accs, k, a.reps)})
                print(rows[-1], file=sys.stderr, flush=True)
        finally:
            c.close()
    print(json.dumps({"tool": "tools/time_decider_batch.py --combined", "workload": "k x acc::decider over k independent accumulators, 1 GPU: "
                      "the halo_acc_decider loop, halo_acc_decider_batch and halo_acc_decider_batch_combined, alternating; contexts of 2^14 "
                      "points (n = 2^20: its own)", "reps": a.reps, "unit": "ms", "rows": rows, "right_side_sweep_n": sizes[0] if sweep else None,
                      "right_side_sweep": sweep, "statuses": "all 0 in every run of every way"}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--combined", action="store_true", help="loop / exact batch / combined batch, three ways alternating (see the module text)")
    ap.add_argument("--fused", action="store_true", help="loop / exact batch / combined batch / fused batch, four ways alternating (see the module text)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--chain", type=int, default=1000)
    ap.add_argument("--sizes", default=",".join(map(str, SIZES)))
    ap.add_argument("--sweep", type=int, default=1, help="members-per-launch sweep at k = 100 (0: off)")
    ap.add_argument("--big", action="store_true", help="add the 2^20-point leg (chain of 10)")
    a = ap.parse_args()
    a.sizes_given = any(x == "--sizes" or x.startswith("--sizes=") for x in sys.argv[1:])
    a.reps_given = any(x == "--reps" or x.startswith("--reps=") for x in sys.argv[1:])
    if a.fused:
        return main_fused(a)
    if a.combined:
        return main_combined(a)
    ctx = h._lib.Context(urs_n=1 << 14)
    rows, sweep = [], []
    t_chain = {}
    for n in [int(x) for x in a.sizes.split(",")]:
        d = n - 1
        t = time.perf_counter()
        accs = build_chain(ctx, n, a.chain, 0x48414C4F00000100 + n)
        t_chain[n] = round(time.perf_counter() - t, 2)
        for k in (10, 100, 1000):
            if k > len(accs):
                continue
            s, b = time_shape(ctx, d, accs, k, a.reps)
            row = {"n": n, "k": k, "serial_ms": round(s, 3), "batch_ms": round(b, 3), "speedup": round(s / b, 2),
                   "serial_ms_per_decider": round(s / k, 4), "batch_ms_per_decider": round(b / k, 4)}
            if n in SIZES and k in PUBLISHED_MS:
                row["published, unstated CPU, 1 thread (BASELINE.md acc_cmp_s_%d_%d), ms" % (n, k)] = PUBLISHED_MS[k][SIZES.index(n)]
            rows.append(row)
        if a.sweep and len(accs) >= 100:
            for g in (1, 2, 4, 8):
                h._lib.dev_hook("check_batch_group", g)
                try:
                    s, b = time_shape(ctx, d, accs, 100, a.reps)
                finally:
                    h._lib.dev_hook("reset", 0)
                sweep.append({"n": n, "k": 100, "members_per_launch": g, "batch_ms": round(b, 3), "serial_ms": round(s, 3)})
    big = []
    if a.big:
        n = 1 << 20
        c = h._lib.Context(urs_n=n)
        try:
            accs = build_chain(c, n, 10, 0x48414C4F00000200)
            for g in (0, 1, 2):
                if g:
                    h._lib.dev_hook("check_batch_group", g)
                try:
                    s, b = time_shape(c, n - 1, accs, 10, a.reps)
                finally:
                    h._lib.dev_hook("reset", 0)
                big.append({"n": n, "k": 10, "members_per_launch": g or "default", "serial_ms": round(s, 3), "batch_ms": round(b, 3),
                            "speedup": round(s / b, 2)})
        finally:
            c.close()
    ctx.close()
    print(json.dumps({"tool": "tools/time_decider_batch.py", "workload": "acc_cmp_s (benches/acc.rs:100-106): k x acc::decider over one "
                      "acc_compare chain, 1 GPU, context of 2^14 points", "reps": a.reps, "statistic": "median",
                      "rows": rows, "members_per_launch_sweep": sweep, "full_size": big, "chain_build_s": t_chain,
                      "statuses": "serial == batch == all 0 for every row"}))


if __name__ == "__main__":
    main()
