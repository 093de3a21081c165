"""Decoding k accumulators from wire bytes, timed three ways that alternate in one process after a warm-up of each: the loop of
single halo_accumulator_decode calls (the only way before the batch existed), ONE halo_accumulator_decode_batch with ctx = NULL
(the host pool), and ONE halo_accumulator_decode_batch with its points decompressed on the device (k_point_decompress; forced
with the development hook decode_batch_min = 1).  For every n, k accumulators over one fresh instance each (random_instance_batch
+ prover_batch on a 2^14-point URS context); k in {10, 100, 1000}.  All three must give the same words and statuses all 0.
Also: a sweep of the pool / device threshold over the number of points in the batch (decode_batch_min; batches of n = 512
accumulators, 22 points each), and for the k = 1000 rows the kernel's own duration (halo_prof_enable) beside the time of
copies of the same bytes (pageable host memory, as the call's own staging).  Prints one JSON line (and writes it with --out);
every time is the median of --reps alternating runs, in ms."""
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
POOL_ONLY = 1 << 40  # a threshold no batch reaches


class Batch:
    def __init__(self, lib, datas, lg):
        self.m, self.lg = len(datas), lg
        self.datas = datas
        self.joined = b"".join(datas)
        self.offs = (C.c_size_t * (self.m + 1))()
        for i, d in enumerate(datas):
            self.offs[i + 1] = self.offs[i] + len(d)
        self.stride = lib.halo_accumulator_words(lg)
        self.points = self.m * (2 * lg + 4)  # C_bar, Ls, Rs, U, the hiding C_bar of the proof, U of pi_V
        self.out = np.zeros((self.m, self.stride), dtype=np.uint64)
        self.st = (C.c_int * self.m)()


def loop(lib, b):
    out = np.zeros((b.m, b.stride), dtype=np.uint64)
    lg = C.c_size_t()
    u64p = C.POINTER(C.c_uint64)
    rows = [out[i].ctypes.data_as(u64p) for i in range(b.m)]
    t = time.perf_counter()
    st = [lib.halo_accumulator_decode(d, len(d), rows[i], b.stride, C.byref(lg)) for i, d in enumerate(b.datas)]
    ms = (time.perf_counter() - t) * 1e3
    assert st == [0] * b.m, lib.halo_last_error()
    return ms, out


def batched(lib, b, ctx, min_points):
    """one call; min_points: the forced threshold (1: the device whenever a context is given; POOL_ONLY: never; 0: the default)"""
    h._lib.dev_hook("decode_batch_min", min_points)
    try:
        t = time.perf_counter()
        rc = lib.halo_accumulator_decode_batch(ctx.h if ctx is not None else None, b.joined, b.offs, b.m, ptr(b.out), b.stride, None, b.st)
        ms = (time.perf_counter() - t) * 1e3
    finally:
        h._lib.dev_hook("decode_batch_min", 0)
    assert rc == 0 and list(b.st) == [0] * b.m, lib.halo_last_error()
    return ms, b.out


def time_three(lib, ctx, b, reps):
    want = loop(lib, b)[1]
    for ctx_, mn in ((None, 0), (ctx, 1)):  # warm-up of each form, and the results against the loop
        assert np.array_equal(batched(lib, b, ctx_, mn)[1], want)
    l_ms, p_ms, d_ms = [], [], []
    for _ in range(reps):
        l_ms.append(loop(lib, b)[0])
        p_ms.append(batched(lib, b, None, 0)[0])
        d_ms.append(batched(lib, b, ctx, 1)[0])
    return statistics.median(l_ms), statistics.median(p_ms), statistics.median(d_ms)


def kernel_and_copies(lib, ctx, b, reps):
    """the kernel's event-timed duration in a device run, and copies of the same bytes (48 in, 112 out per point) on their own"""
    import torch
    ctx.prof_enable(1)
    try:
        ctx.prof_reset()
        for _ in range(reps):
            batched(lib, b, ctx, 1)
        ms, launches = ctx.prof().get("k_point_decompress", (0.0, 0))
    finally:
        ctx.prof_enable(0)
    src = torch.zeros(b.points * 48, dtype=torch.uint8)
    dst = torch.zeros(b.points * 112, dtype=torch.uint8, device="cuda")
    copies = []
    for r in range(reps + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        src.cuda()
        dst.cpu()
        torch.cuda.synchronize()
        if r:
            copies.append((time.perf_counter() - t) * 1e3)
    return ms / max(launches, 1), launches // max(reps, 1), statistics.median(copies)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--members", type=int, default=1000)
    ap.add_argument("--sizes", default=",".join(map(str, SIZES)))
    ap.add_argument("--sweep", default="16,32,64,128,256,512,1024,2048,4096", help="points of the threshold sweep ('': off)")
    ap.add_argument("--out", default="", help="also write the JSON line to this file")
    a = ap.parse_args()
    ctx = h._lib.Context(urs_n=1 << 14)
    lib = ctx.lib
    rows, sweep, t_make = [], [], {}
    small = None
    for n in [int(x) for x in a.sizes.split(",")]:
        lg, d = n.bit_length() - 1, n - 1
        t = time.perf_counter()
        rng = [0x48414C4F00000500 + n]
        qs = A.random_instance_batch(ctx, rng, d, a.members)
        accs, _ = A.prover_batch(ctx, rng, d, [[q] for q in qs])
        datas = [h._lib.accumulator_encode(x) for x in accs]
        t_make[n] = round(time.perf_counter() - t, 2)
        if small is None:
            small = (lg, datas)
        for k in (10, 100, 1000):
            if k > len(datas):
                continue
            b = Batch(lib, datas[:k], lg)
            l, p, dv = time_three(lib, ctx, b, a.reps)
            row = {"n": n, "k": k, "points": b.points, "bytes": len(b.joined), "loop_ms": round(l, 3), "batch_pool_ms": round(p, 3),
                   "batch_device_ms": round(dv, 3), "loop_us_per_point": round(l * 1e3 / b.points, 2),
                   "speedup_pool": round(l / p, 2), "speedup_device": round(l / dv, 2)}
            if k == 1000:
                k_ms, launches, c_ms = kernel_and_copies(lib, ctx, b, a.reps)
                row.update({"kernel_ms": round(k_ms, 3), "launches": launches, "copies_of_the_same_bytes_ms": round(c_ms, 3)})
            rows.append(row)
        print("n = %d: made in %.1f s, rows %s" % (n, t_make[n], [(r["k"], r["loop_ms"], r["batch_pool_ms"], r["batch_device_ms"]) for r in rows if r["n"] == n]),
              file=sys.stderr, flush=True)
    if a.sweep and small is not None:
        lg, datas = small
        per = 2 * lg + 4
        for pts in [int(x) for x in a.sweep.split(",")]:
            m = max(1, min(len(datas), (pts + per - 1) // per))
            b = Batch(lib, datas[:m], lg)
            p_ms, d_ms = [], []
            for r in range(a.reps + 1):
                ms_p = batched(lib, b, ctx, POOL_ONLY)[0]
                ms_d = batched(lib, b, ctx, 1)[0]
                if r:
                    p_ms.append(ms_p)
                    d_ms.append(ms_d)
            sweep.append({"points": b.points, "members": m, "pool_ms": round(statistics.median(p_ms), 3), "device_ms": round(statistics.median(d_ms), 3)})
    ctx.close()
    line = json.dumps({"tool": "tools/time_decode_batch.py", "workload": "k accumulators from wire bytes: loop of halo_accumulator_decode, "
                       "halo_accumulator_decode_batch on the host pool (ctx = NULL) and with the points decompressed on the device, 1 GPU",
                       "reps": a.reps, "statistic": "median", "rows": rows, "threshold_sweep": sweep, "make_s": t_make,
                       "results": "loop == pool == device, statuses all 0, for every row"})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
