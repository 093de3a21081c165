"""The acc_cmp_f shape (benches/acc.rs:64-74, acc_compare_fast_helper: k x acc::verifier + 1 x acc::decider) timed two ways: the
serial halo_acc_verifier loop + one halo_acc_decider, and ONE halo_acc_verifier_batch + one halo_acc_decider, alternating in the
same process after a warm-up of each shape.  For every n one acc_compare chain of 1000 steps (random_instance + prover,
benches/acc.rs:76-98) on a 2^14-point URS context; k in {10, 100, 1000} of its steps.  Also a sweep of the batch's host/device
threshold (the development hook verifier_batch_min; host = halo_set_batch_verify(0)) over k, and with --big a 2^20-point leg (a
chain of 10).  Statuses of both ways must be equal and all 0.  Prints one JSON line (and writes it with --out); every time is the
median of --reps alternating runs, in ms."""
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

# acc_cmp_f_{n}_{k}, ms (report/report.md:2135-2164; the 8196 row is n = 8192 in the code)
PUBLISHED_MS = {
    10: [67.098, 77.597, 99.973, 139.35, 186.34, 299.49],
    100: [607.28, 662.03, 798.48, 1014.2, 1161.1, 1648.4],
    1000: [6018.3, 6511.4, 7775.2, 9785.1, 10899.0, 15176.0],
}
SIZES = [512, 1024, 2048, 4096, 8192, 16384]


def build_chain(ctx, n, k, seed):
    """[(instances, acc)] of acc_compare: step 0 verifies one instance, every later step the previous accumulator's and a fresh one"""
    d = n - 1
    rng = [seed]
    out, acc = [], None
    for _ in range(k):
        q = A.random_instance(ctx, rng, d)
        qs = [q] if acc is None else [A.instance_from_accumulator(ctx, acc, d), q]
        acc = A.prover(ctx, rng, d, qs)
        out.append((qs, acc))
    return out


class Shape:
    def __init__(self, members, d):
        self.d, self.k = d, len(members)
        self.blobs = [np.ascontiguousarray(np.concatenate(qs)) for qs, _ in members]
        self.accs = [np.ascontiguousarray(a) for _, a in members]
        self.counts_py = [len(qs) for qs, _ in members]
        self.qs = np.ascontiguousarray(np.concatenate(self.blobs))
        self.acc_blob = np.ascontiguousarray(np.concatenate(self.accs))
        self.counts = (C.c_size_t * self.k)(*self.counts_py)
        self.last = self.accs[-1]


def serial(ctx, s):
    t = time.perf_counter()
    st = [ctx.lib.halo_acc_verifier(ctx.h, s.d, ptr(b), m, ptr(a)) for b, m, a in zip(s.blobs, s.counts_py, s.accs)]
    rc = ctx.lib.halo_acc_decider(ctx.h, ptr(s.last))
    ms = (time.perf_counter() - t) * 1e3
    assert rc == 0, ctx.lib.halo_last_error()
    return ms, st


def batched(ctx, s):
    st = (C.c_int * s.k)()
    t = time.perf_counter()
    rc = ctx.lib.halo_acc_verifier_batch(ctx.h, s.d, ptr(s.qs), s.counts, s.k, ptr(s.acc_blob), st)
    rc2 = ctx.lib.halo_acc_decider(ctx.h, ptr(s.last))
    ms = (time.perf_counter() - t) * 1e3
    assert rc == 0 and rc2 == 0, ctx.lib.halo_last_error()
    return ms, list(st)


def time_shape(ctx, s, reps):
    a_ms, b_ms = [], []
    serial(ctx, s)  # warm-up of each shape
    batched(ctx, s)
    for _ in range(reps):
        ms, a_st = serial(ctx, s)
        a_ms.append(ms)
        ms, b_st = batched(ctx, s)
        b_ms.append(ms)
        assert a_st == b_st == [0] * s.k, "statuses differ or a member was rejected"
    return statistics.median(a_ms), statistics.median(b_ms)


def time_forms(ctx, s, reps):
    """the batch with its sums forced onto the device (verifier_batch_min 1) and onto the host pool, alternating"""
    dev_ms, host_ms = [], []
    for r in range(reps + 1):
        h._lib.dev_hook("verifier_batch_min", 1)
        try:
            ms, st = batched(ctx, s)
        finally:
            h._lib.dev_hook("reset", 0)
        if r:
            dev_ms.append(ms)
        ctx.set_batch_verify(False)
        try:
            ms, st2 = batched(ctx, s)
        finally:
            ctx.set_batch_verify(True)
        if r:
            host_ms.append(ms)
        assert st == st2 == [0] * s.k
    return statistics.median(dev_ms), statistics.median(host_ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--chain", type=int, default=1000)
    ap.add_argument("--sizes", default=",".join(map(str, SIZES)))
    ap.add_argument("--sweep", default="512,16384", help="sizes of the host/device threshold sweep ('' : off)")
    ap.add_argument("--big", action="store_true", help="add the 2^20-point leg (chain of 10)")
    ap.add_argument("--out", default="", help="also write the JSON line to this file")
    a = ap.parse_args()
    ctx = h._lib.Context(urs_n=1 << 14)
    rows, sweep, t_chain = [], [], {}
    sweep_sizes = [int(x) for x in a.sweep.split(",") if x]
    for n in [int(x) for x in a.sizes.split(",")]:
        t = time.perf_counter()
        members = build_chain(ctx, n, a.chain, 0x48414C4F00000300 + n)
        t_chain[n] = round(time.perf_counter() - t, 2)
        for k in (10, 100, 1000):
            if k > len(members):
                continue
            s, b = time_shape(ctx, Shape(members[:k], n - 1), a.reps)
            row = {"n": n, "k": k, "loop_ms": round(s, 3), "batch_ms": round(b, 3), "speedup": round(s / b, 2),
                   "loop_ms_per_verifier": round(s / k, 4), "batch_ms_per_verifier": round(b / k, 4)}
            if n in SIZES and k in PUBLISHED_MS:
                row["published, unstated CPU, 1 thread (BASELINE.md acc_cmp_f_%d_%d), ms" % (n, k)] = PUBLISHED_MS[k][SIZES.index(n)]
            rows.append(row)
        print("n = %d: chain %.1f s, rows %s" % (n, t_chain[n], [(r["k"], r["loop_ms"], r["batch_ms"]) for r in rows if r["n"] == n]),
              file=sys.stderr, flush=True)
        if n in sweep_sizes:
            for k in (4, 8, 16, 32, 64, 128, 256):
                if k > len(members):
                    continue
                sh = Shape(members[:k], n - 1)
                dv, ho = time_forms(ctx, sh, a.reps)
                sweep.append({"n": n, "k": k, "relations": sum(sh.counts_py), "device_ms": round(dv, 3), "host_pool_ms": round(ho, 3)})
    big = []
    if a.big:
        n = 1 << 20
        c = h._lib.Context(urs_n=n)
        try:
            members = build_chain(c, n, 10, 0x48414C4F00000400)
            sh = Shape(members, n - 1)
            s, b = time_shape(c, sh, a.reps)
            dv, ho = time_forms(c, sh, a.reps)
            big.append({"n": n, "k": 10, "loop_ms": round(s, 3), "batch_ms": round(b, 3), "speedup": round(s / b, 2),
                        "batch_device_form_ms": round(dv, 3), "batch_host_form_ms": round(ho, 3)})
        finally:
            c.close()
    ctx.close()
    line = json.dumps({"tool": "tools/time_verifier_batch.py", "workload": "acc_cmp_f (benches/acc.rs:64-74): k x acc::verifier + 1 x "
                       "acc::decider over one acc_compare chain, 1 GPU, context of 2^14 points", "reps": a.reps, "statistic": "median",
                       "rows": rows, "threshold_sweep": sweep, "full_size": big, "chain_build_s": t_chain,
                       "statuses": "loop == batch == all 0 for every row"})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
