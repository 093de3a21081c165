"""acc::prover of k members timed two ways: the serial halo_acc_prover loop and ONE halo_acc_prover_batch, alternating in the same
process after a warm-up of each shape (halo_acc_prover is the code the batch is measured against: the loop is the baseline, never
another run's numbers).  A 2^14-point URS context; n in {512 .. 16384}; k in {10, 100, 1000}; members in the acc_compare step
shape (the previous accumulator's Instance and a fresh random instance).  A second leg: k chains in lockstep for 8 steps
(random_instance_batch + prover_batch against the two loops -- the ASDL step of many chains).  A sweep of the members per launch
(the development hook open_batch_group) at k = 100.  With --big a k = 4 leg at n = 2^20 on a 2^20-point context with the fold table
fixed off, where the members run one at a time.  Blobs, statuses and final RNG states of both ways must be equal for every row
before a time is reported.  Prints one JSON line; every time is the median of --reps alternating runs, in ms, with min and max.
With --fold (alone) the sizes above the no-fold size, n = 2^15 .. 2^19 (--lgs) on a context of max(2^16, n) points, k in {8, 64}
(8 only from 2^18 on): the same batched call under the development hook open_batch_fold = 2 (the loop over halo_acc_prover) and = 1 (the
opens on the folded schedule), alternating; medians of at least 5 runs with the least and the greatest, "won" where every run of the
folded schedule was faster than every run of the loop.  --held-back names sizes (log2) that the library keeps on the loop by default
although they may win: the line lists them under "held_back_n", which the tests read beside the rows.  --out writes the JSON line to a
file as well."""
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


def fold_leg(reps, lgs, ks, long_ks, held_back):
    """above the no-fold size: the same batched call under open_batch_fold = 2 (the loop over halo_acc_prover) and = 1 (the opens'
    folded schedule), alternating in one process; k from `ks`, from 2^18 on only those in `long_ks`"""
    reps = max(reps, 5)
    rows = []

    def hooked(ctx, value, call, want_batched):
        def run():
            h._lib.dev_hook("open_batch_fold", value)
            try:
                r = call()
                assert ctx.info(10) == want_batched, (value, ctx.info(10))
                return r
            finally:
                h._lib.dev_hook("reset", 0)
        return run

    for lg in lgs:
        n, d = 1 << lg, (1 << lg) - 1
        ctx = h._lib.Context(urs_n=max(n, 1 << 16))
        try:
            here = [k for k in ks if lg < 18 or k in long_ks]
            qs = step_members(ctx, d, max(here), 0x48414C4F00000700 + n)
            for k in here:
                call = lambda: batched(ctx, d, qs, k, 7 + k)  # noqa: E731
                loop, fold = hooked(ctx, 2, call, 0), hooked(ctx, 1, call, k)
                s, b = alternate(loop, fold, reps)
                r = row(n, k, s, b)
                rows.append({"n": n, "k": k, "loop_ms": r["serial_ms"], "fold_ms": r["batch_ms"], "loop_min_max_ms": r["serial_min_max"],
                             "fold_min_max_ms": r["batch_min_max"], "speedup": r["speedup"], "won": max(b) < min(s)})
                print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
        finally:
            ctx.close()
    return {"tool": "tools/time_prover_batch.py --fold", "workload": "k x acc::prover over [previous accumulator, fresh instance] above the "
            "no-fold size, 1 GPU, context of max(2^16, n) points, default switch 2^14", "reps": reps,
            "statistic": "median of alternating runs, ms; loop = open_batch_fold 2, fold = open_batch_fold 1, same process",
            "rows": rows, "held_back_n": [1 << lg for lg in held_back],
            "held_back_reason": "sizes named with --held-back: the library keeps them on the loop by default whatever their rows say "
            "(pcdl_batch.hip open_fold_route); the hook open_batch_fold = 1 reaches the folded schedule",
            "equal": "accumulators, statuses and final RNG states: loop == folded schedule for every row"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fold", action="store_true", help="only the folded schedule against the loop at n = 2^15 .. 2^19, k = 8 and 64")
    ap.add_argument("--lgs", default="15,16,17,18,19", help="with --fold: log2 of the sizes")
    ap.add_argument("--held-back", default="15", help="with --fold: log2 of the sizes the library holds back from its default route (empty: none)")
    ap.add_argument("--fold-ks", default="8,64", help="with --fold: the members per call (from 2^18 on: 8 only)")
    ap.add_argument("--out", default=None, help="with --fold: also write the JSON line to this file")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", default=",".join(map(str, SIZES)))
    ap.add_argument("--ks", default="10,100,1000")
    ap.add_argument("--chains", default="10,100", help="chains of the lockstep leg (empty: off)")
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--sweep", type=int, default=1, help="members-per-launch sweep at k = 100 (0: off)")
    ap.add_argument("--big", action="store_true", help="add the 2^20-point leg (k = 4)")
    a = ap.parse_args()
    if a.fold:
        line = json.dumps(fold_leg(a.reps, [int(x) for x in a.lgs.split(",")], [int(x) for x in a.fold_ks.split(",")], [8],
                                   [int(x) for x in a.held_back.split(",") if x]))
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        print(line)
        return
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
