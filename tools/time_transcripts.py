"""The batched checks' Fiat-Shamir transcripts on the host pool against the device route (csrc/transcript.hip), timed through the
two calls they feed: halo_pcdl_succinct_check_batch over k Instances and halo_acc_decider_batch_fused over k accumulators
(random_instance_batch + prover_batch, independent members), at n in {512, 16384} on a 2^14-point context and k in
{10, 64, 100, 1000}.  Each call runs with the development hook "transcript_min" forcing the host (a value above k: the code of the
commit before the device route) and forcing the device (1), alternating in one process after a warm-up of each, --reps runs
(5) each; every row keeps median, least and greatest and all runs, says whether the device route ran at all (the profiler, in an
untimed call: halo_pcdl_succinct_check_batch below 64 members never batches, so both ways are the pool there) and whether every
device run beats every host run.  The default threshold follows from the rows: the smallest timed k from which every device run
beats every host run at both sizes and in both calls, at every larger timed k too; none: never.  Prints one JSON line."""
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

KS = (10, 64, 100, 1000)


def stats(ms):
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def succinct(ctx, d, blob, k, lg):
    xis, Us, st = np.zeros((k, lg + 1, 4), dtype=np.uint64), np.zeros((k, 12), dtype=np.uint64), (C.c_int * k)()
    t = time.perf_counter()
    rc = ctx.lib.halo_pcdl_succinct_check_batch(ctx.h, d, ptr(blob), k, ptr(xis), ptr(Us), st)
    ms = (time.perf_counter() - t) * 1e3
    assert rc == 0 and list(st) == [0] * k, ctx.lib.halo_last_error()
    return ms, xis


def decider_fused(ctx, d, blob, k, lg):
    st = (C.c_int * k)()
    t = time.perf_counter()
    rc = ctx.lib.halo_acc_decider_batch_fused(ctx.h, d, ptr(blob), k, None, st)
    ms = (time.perf_counter() - t) * 1e3
    assert rc == 0 and list(st) == [0] * k, ctx.lib.halo_last_error()
    return ms, None


def forced(min_members, fn):
    h._lib.dev_hook("transcript_min", min_members)
    try:
        return fn()
    finally:
        h._lib.dev_hook("reset", 0)


def time_row(ctx, call, d, blob, k, lg, reps):
    ways = {"host": k + 1000, "device": 1}
    ms = {w: [] for w in ways}
    outs = {}
    for w, v in ways.items():  # warm-up of each
        _, outs[w] = forced(v, lambda: call(ctx, d, blob, k, lg))
    if outs["host"] is not None:
        assert (outs["host"] == outs["device"]).all(), "the routes' challenges differ"
    for _ in range(reps):
        for w, v in ways.items():
            t, _ = forced(v, lambda: call(ctx, d, blob, k, lg))
            ms[w].append(t)
    ctx.prof_enable(1)
    try:
        ctx.prof_reset()
        forced(1, lambda: call(ctx, d, blob, k, lg))
        ran = any(name == "k_transcript_chain" and cnt for name, (_, cnt) in ctx.prof().items())
    finally:
        ctx.prof_enable(0)
    return {"host_ms": stats(ms["host"]), "device_ms": stats(ms["device"]), "host_runs": [round(v, 3) for v in ms["host"]],
            "device_runs": [round(v, 3) for v in ms["device"]], "device_route_ran": ran,
            "every_device_run_beats_every_host_run": ran and max(ms["device"]) < min(ms["host"]),
            "every_host_run_beats_every_device_run": ran and max(ms["host"]) < min(ms["device"]),
            "host_over_device": round(statistics.median(ms["host"]) / statistics.median(ms["device"]), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="512,16384")
    ap.add_argument("--members", type=int, default=1000)
    a = ap.parse_args()
    ks = [k for k in KS if k <= a.members]
    rows = []
    ctx = h._lib.Context(urs_n=1 << 14)
    try:
        for n in [int(x) for x in a.sizes.split(",")]:
            d, lg = n - 1, n.bit_length() - 1
            rng = [0x48414C4F00000700 + n]
            qs = A.random_instance_batch(ctx, rng, d, a.members)
            accs, codes = A.prover_batch(ctx, rng, d, [[q] for q in qs])
            assert codes == [0] * a.members
            for name, call, blobs in (("halo_pcdl_succinct_check_batch", succinct, qs), ("halo_acc_decider_batch_fused", decider_fused, accs)):
                for k in ks:
                    blob = np.ascontiguousarray(np.concatenate(blobs[:k]))
                    rows.append({"call": name, "n": n, "k": k, **time_row(ctx, call, d, blob, k, lg, a.reps)})
                    print(rows[-1], file=sys.stderr, flush=True)
    finally:
        ctx.close()
    won = None
    for k in reversed(ks):  # the smallest k from which every row wins, at every larger timed k too
        if all(r["every_device_run_beats_every_host_run"] for r in rows if r["k"] == k):
            won = k
        else:
            break
    print(json.dumps({"tool": "tools/time_transcripts.py", "workload": "the succinct check's transcripts of k members on the host pool (hook transcript_min "
                      "above k) and on the device (hook 1), alternating, through halo_pcdl_succinct_check_batch (k hiding Instances) and "
                      "halo_acc_decider_batch_fused (k independent accumulators); 1 GPU, context of 2^14 points", "reps": a.reps, "unit": "ms",
                      "rows": rows, "transcript_min_by_the_rule": won if won is not None else "never",
                      "rule": "the smallest timed k from which every device run beats every host run in every row, at every larger timed k too",
                      "statuses": "all 0 in every run of every way; the challenges of the two routes equal"}))


if __name__ == "__main__":
    main()
