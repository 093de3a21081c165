"""acc::prover of k members timed two ways: the serial halo_acc_prover loop and ONE halo_acc_prover_batch, alternating in the same
process after a warm-up of each shape (halo_acc_prover is the code the batch is measured against: the loop is the baseline, never
another run's numbers).  A 2^14-point URS context; n in {512 .. 16384}; k in {10, 100, 1000}; members in the acc_compare step
shape (the previous accumulator's Instance and a fresh random instance).  A second leg: k chains in lockstep for 8 steps
(random_instance_batch + prover_batch against the two loops -- the ASDL step of many chains).  A sweep of the members per launch
(the development hook open_batch_group) at k = 100.  With --big a k = 4 leg at n = 2^20 on a 2^20-point context with the fold table
fixed off, where the members run one at a time.  Blobs, statuses and final RNG states of both ways must be equal for every row
before a time is reported.  Prints one JSON line; every time is the median of --reps alternating runs, in ms, with min and max."""
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

SIZES = [512, 1024, 2048, 4096, 8192, 16384]


def lg_of(d):
    return (d + 1).bit_length() - 1


def step_members(ctx, d, k, seed):
    """k members [Instance of a previous accumulator, a fresh instance] as one flat array (k x 2 x instance words)"""
    rng = [seed]
    fresh = A.random_instance_batch(ctx, rng, d, 2 * k)
    prev = [A.prover(ctx, rng, d, [fresh[2 * j]]) for j in range(k)]
    return np.ascontiguousarray(np.stack([np.stack([A.instance_from_accumulator(ctx, prev[j], d), fresh[2 * j + 1]]) for j in range(k)]))


def serial(ctx, d, qs, k, state):
    out = np.zeros((k, ctx.lib.halo_accumulator_words(lg_of(d))), dtype=np.uint64)
    calls = [(ptr(qs[j]), ptr(out[j])) for j in range(k)]
    st = C.c_uint64(state)
    t = time.perf_counter()
    for q, o in calls:
        assert ctx.lib.halo_acc_prover(ctx.h, C.byref(st), d, q, 2, o) == 0
    return (time.perf_counter() - t) * 1e3, out, st.value


def batched(ctx, d, qs, k, state):
    out = np.zeros((k, ctx.lib.halo_accumulator_words(lg_of(d))), dtype=np.uint64)
    counts = (C.c_size_t * k)(*([2] * k))
    status = (C.c_int * k)()
    st = C.c_uint64(state)
    t = time.perf_counter()
    rc = ctx.lib.halo_acc_prover_batch(ctx.h, C.byref(st), d, ptr(qs), counts, k, ptr(out), status)
    ms = (time.perf_counter() - t) * 1e3
    assert rc == 0 and not any(status), ctx.lib.halo_last_error()
    return ms, out, st.value


def chains(ctx, d, k, steps, state, batch):
    """k chains advanced in lockstep: per step k fresh instances, then k provers over [previous accumulator, fresh]"""
    rng = [state]
    prev = None
    t = time.perf_counter()
    for _ in range(steps):
        fresh = A.random_instance_batch(ctx, rng, d, k) if batch else [A.random_instance(ctx, rng, d) for _ in range(k)]
        members = [[fresh[j]] if prev is None else [A.instance_from_accumulator(ctx, prev[j], d), fresh[j]] for j in range(k)]
        if batch:
            prev, codes = A.prover_batch(ctx, rng, d, members)
            assert not any(codes)
        else:
            prev = [A.prover(ctx, rng, d, m) for m in members]
    return (time.perf_counter() - t) * 1e3, np.stack(prev), rng[0]


def alternate(one, two, reps):
    """a warm-up of each, then `reps` alternating runs; both ways must give the same outputs and final state"""
    a, b = one(), two()
    assert a[1].tolist() == b[1].tolist() and a[2] == b[2], "the two ways differ"
    s_ms, b_ms = [], []
    for _ in range(reps):
        s_ms.append(one()[0])
        b_ms.append(two()[0])
    return s_ms, b_ms


def row(n, k, s_ms, b_ms, extra=None):
    s, b = statistics.median(s_ms), statistics.median(b_ms)
    r = {"n": n, "k": k, "serial_ms": round(s, 3), "batch_ms": round(b, 3), "speedup": round(s / b, 2),
         "serial_min_max": [round(min(s_ms), 3), round(max(s_ms), 3)], "batch_min_max": [round(min(b_ms), 3), round(max(b_ms), 3)],
         "ranges_overlap": min(s_ms) <= max(b_ms), "serial_ms_per_member": round(s / k, 4), "batch_ms_per_member": round(b / k, 4)}
    r.update(extra or {})
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", default=",".join(map(str, SIZES)))
    ap.add_argument("--ks", default="10,100,1000")
    ap.add_argument("--chains", default="10,100", help="chains of the lockstep leg (empty: off)")
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--sweep", type=int, default=1, help="members-per-launch sweep at k = 100 (0: off)")
    ap.add_argument("--big", action="store_true", help="add the 2^20-point leg (k = 4)")
    a = ap.parse_args()
    ks = [int(x) for x in a.ks.split(",")]
    cks = [int(x) for x in a.chains.split(",") if x]
    ctx = h._lib.Context(urs_n=1 << 14)
    rows, chain_rows, sweep = [], [], []
    for n in [int(x) for x in a.sizes.split(",")]:
        d = n - 1
        qs = step_members(ctx, d, max(ks), 0x48414C4F00000500 + n)
        for k in ks:
            s, b = alternate(lambda: serial(ctx, d, qs, k, 7 + k), lambda: batched(ctx, d, qs, k, 7 + k), a.reps)
            rows.append(row(n, k, s, b))
        for k in cks:
            s, b = alternate(lambda: chains(ctx, d, k, a.steps, 13 + k, False), lambda: chains(ctx, d, k, a.steps, 13 + k, True), a.reps)
            chain_rows.append(row(n, k, s, b, {"steps": a.steps}))
        if a.sweep and 100 in ks:
            for g in (1, 2, 4):
                h._lib.dev_hook("open_batch_group", g)
                try:
                    s, b = alternate(lambda: serial(ctx, d, qs, 100, 5), lambda: batched(ctx, d, qs, 100, 5), a.reps)
                finally:
                    h._lib.dev_hook("reset", 0)
                sweep.append(row(n, 100, s, b, {"members_per_launch": g}))
        print(json.dumps({"progress_n": n}), file=sys.stderr, flush=True)
    ctx.close()
    big = []
    if a.big:
        n = 1 << 20
        c = h._lib.Context(urs_n=n)
        try:
            c.set_fold_table(0)
            qs = step_members(c, n - 1, 4, 0x48414C4F00000600)
            s, b = alternate(lambda: serial(c, n - 1, qs, 4, 3), lambda: batched(c, n - 1, qs, 4, 3), a.reps)
            big.append(row(n, 4, s, b))
        finally:
            c.close()
    print(json.dumps({"tool": "tools/time_prover_batch.py", "workload": "k x acc::prover over [previous accumulator, fresh instance] "
                      "(benches/acc.rs:76-98 step shape) and k chains in lockstep (random_instance + prover per step), 1 GPU, context of "
                      "2^14 points", "reps": a.reps, "statistic": "median", "prover": rows, "chains_lockstep": chain_rows,
                      "members_per_launch_sweep": sweep, "full_size": big,
                      "equal": "accumulators, statuses and final RNG states: loop == batch for every row"}))


if __name__ == "__main__":
    main()
