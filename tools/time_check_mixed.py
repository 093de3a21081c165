"""Members of SEVERAL degree bounds checked four ways, alternating in one process after a warm-up of each:

  mixed        ONE halo_pcdl_check_batch_mixed_combined over all the members (one MSM of the largest size for all of them);
  combined     the best a caller could do before it: the members sorted by d, one halo_pcdl_check_batch_combined per size;
  fused        the same with one halo_pcdl_check_batch_fused per size;
  mixed_fused  ONE halo_pcdl_check_batch_mixed_fused over all the members (the succinct relations in the same relation).

Workloads: a key of 2^14 points with the members spread evenly over lg 9 .. 14, and (--big) a key of 2^20 points with the same
members plus 1 .. 4 of lg 20; totals of 12, 60, 120 and 600 members.  The members are honest Instances (random_instance_batch: a
check's work does not depend on what was opened); every way must accept all of them.  Every row keeps median, least and
greatest of --reps runs (5 unless given) of each way, in ms, and says whether the mixed call's range lies below the two per-size
ways' ("won"), or which ranges overlap or lie below it ("not won"); and the same for the mixed fused call against each of the three
other ways ("mixed_fused_won": every one of its runs below every run of that way).  Prints one JSON line; --out writes the same to a
file."""
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

LGS = [9, 10, 11, 12, 13, 14]
TOTALS = [12, 60, 120, 600]


def members_of(ctx, total, seed, extra_lg20=0):
    """-> the members in an order that mixes the sizes: total / 6 of each lg 9 .. 14, then the lg 20 ones spread among them"""
    per = total // len(LGS)
    classes = [list(A.random_instance_batch(ctx, [seed + lg], (1 << lg) - 1, per)) for lg in LGS]
    out = [classes[c][k] for k in range(per) for c in range(len(LGS))]
    if extra_lg20:
        big = list(A.random_instance_batch(ctx, [seed + 20], (1 << 20) - 1, extra_lg20))
        step = max(1, len(out) // extra_lg20)
        for j, q in enumerate(big):
            out.insert(j * step + j, q)
    return [np.ascontiguousarray(q, dtype=np.uint64) for q in out]


class Shapes:
    """the four ways' arguments, built once per workload (packing is not what is timed)"""

    def __init__(self, ctx, members):
        self.ctx, self.m = ctx, len(members)
        self.keep = members
        self.ds = (C.c_size_t * self.m)(*[int(q[12]) for q in members])
        self.ptrs = (C.c_void_p * self.m)(*[q.ctypes.data for q in members])
        self.classes = []  # (d, the class's blobs in one array, its count): what a caller who sorts by d holds
        for d in sorted({int(q[12]) for q in members}):
            mine = [q for q in members if int(q[12]) == d]
            self.classes.append((d, np.ascontiguousarray(np.concatenate(mine)), len(mine)))

    def one_call(self, fn):
        st = (C.c_int * self.m)()
        t = time.perf_counter()
        rc = fn(self.ctx.h, self.ds, self.ptrs, self.m, None, st)
        ms = (time.perf_counter() - t) * 1e3
        assert rc == 0 and not any(st), self.ctx.lib.halo_last_error()
        return ms

    def mixed(self):
        return self.one_call(self.ctx.lib.halo_pcdl_check_batch_mixed_combined)

    def mixed_fused(self):
        return self.one_call(self.ctx.lib.halo_pcdl_check_batch_mixed_fused)

    def per_class(self, fn):
        t = time.perf_counter()
        for d, blob, k in self.classes:
            st = (C.c_int * k)()
            rc = fn(self.ctx.h, d, ptr(blob), k, None, st)
            assert rc == 0 and not any(st), self.ctx.lib.halo_last_error()
        return (time.perf_counter() - t) * 1e3

    def combined(self):
        return self.per_class(self.ctx.lib.halo_pcdl_check_batch_combined)

    def fused(self):
        return self.per_class(self.ctx.lib.halo_pcdl_check_batch_fused)


def row_of(shape, reps):
    ways = (("mixed", shape.mixed), ("combined", shape.combined), ("fused", shape.fused), ("mixed_fused", shape.mixed_fused))
    for _, fn in ways:  # warm-up of each shape
        fn()
    runs = {name: [] for name, _ in ways}
    for _ in range(reps):
        for name, fn in ways:
            runs[name].append(fn())
    row = {name: {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)} for name, v in runs.items()}
    lost = [name for name in ("combined", "fused") if row[name]["min"] <= row["mixed"]["max"]]
    row["won"] = not lost
    row["not_below"] = lost  # the ways whose range overlaps the mixed call's, or lies below it
    row["speedup_vs_combined"] = round(row["combined"]["median"] / row["mixed"]["median"], 2)
    row["speedup_vs_fused"] = round(row["fused"]["median"] / row["mixed"]["median"], 2)
    # the mixed fused call against each other way: won = every one of its runs below every run of that way
    others = ("fused", "mixed", "combined")
    row["mixed_fused_won"] = {name: row["mixed_fused"]["max"] < row[name]["min"] for name in others}
    row["mixed_fused_speedup"] = {name: round(row[name]["median"] / row["mixed_fused"]["median"], 2) for name in others}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--totals", type=int, nargs="*", default=TOTALS)
    ap.add_argument("--big", action="store_true", help="also the 2^20-point key, with 1 .. 4 members of lg 20")
    ap.add_argument("--big-totals", type=int, nargs="*", default=TOTALS)
    ap.add_argument("--out")
    args = ap.parse_args()
    res = {"tool": "time_check_mixed", "reps": args.reps, "lgs": LGS, "rows": []}
    ctx = h._lib.Context(urs_n=1 << 14)
    try:
        for total in args.totals:
            row = row_of(Shapes(ctx, members_of(ctx, total, 0x3100 + total)), args.reps)
            row.update(key_lg=14, total=total, lg20=0)
            res["rows"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    finally:
        ctx.close()
    if args.big:
        ctx = h._lib.Context(urs_n=1 << 20)
        try:
            for j, total in enumerate(args.big_totals):
                extra = 1 + j % 4
                row = row_of(Shapes(ctx, members_of(ctx, total, 0x3200 + total, extra)), args.reps)
                row.update(key_lg=20, total=total + extra, lg20=extra)
                res["rows"].append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
        finally:
            ctx.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
