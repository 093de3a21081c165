"""The acc_cmp_s shape (benches/acc.rs:100-106: k x acc::decider) timed two ways: the serial halo_acc_decider loop and ONE
halo_acc_decider_batch, alternating in the same process after a warm-up of each shape.  For every n one acc_compare chain of
1000 accumulators (random_instance + prover, benches/acc.rs:76-98) on a 2^14-point URS context; k in {10, 100, 1000} of its
accumulators.  Also a sweep of the batch's members per MSM launch (the development hook check_batch_group) at k = 100, and with
--big a 2^20-point leg (a chain of 10 on a 2^20-point context).  Statuses of both ways must be equal and all 0.  Prints one
JSON line; every time is the median of --reps alternating runs, in ms."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--chain", type=int, default=1000)
    ap.add_argument("--sizes", default=",".join(map(str, SIZES)))
    ap.add_argument("--sweep", type=int, default=1, help="members-per-launch sweep at k = 100 (0: off)")
    ap.add_argument("--big", action="store_true", help="add the 2^20-point leg (chain of 10)")
    a = ap.parse_args()
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
