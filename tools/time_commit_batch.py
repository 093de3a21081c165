"""pcdl::commit of m polynomials and Instances from m polynomials, each timed against the loop of single calls on the same
context, alternating in the same process after a warm-up of each: halo_pcdl_commit_batch against m x halo_pcdl_commit (host
polynomials, hiding), halo_pcdl_commit_dev_batch against m x halo_pcdl_commit_dev (device-resident: full length, passed in
place, and three quarters of it, padded by k_pad_members_batch), halo_instance_from_poly_batch against m x (halo_pcdl_commit,
halo_poly_eval, halo_pcdl_open) and against m x halo_instance_from_poly.  n in {2^10, 2^14, 2^17, 2^20} at full degree on a
context of n points (the fold table fixed off at 2^20, so that no table build lands inside a timed run), m in {1, 8, 64} below
2^20 and m = 8 there (--ms, --big-ms: other batch sizes, for the thresholds).  "forced" is the batched pipeline whatever the
routing says (the development hooks commit_batch_group / open_batch_group at the default group size), so that the threshold
between the loop and the pipeline can be read off one run.
The points, blobs and final RNG states of every way must be equal: a difference ends the script.  Prints one JSON line and
writes it to --out; every time is the median of --reps alternating runs, in ms, with the least and greatest run beside it
("min_max_ms")."""
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
from halo_accumulation_amd._lib import ptr  # noqa: E402

SIZES = [1 << 10, 1 << 14, 1 << 17, 1 << 20]


def scalars(g, shape):
    """canonical field elements (< 2^253 < r) as 4 words each"""
    a = g.integers(0, 2 ** 63, size=tuple(shape) + (4,), dtype=np.uint64)
    a[..., 3] &= np.uint64((1 << 61) - 1)
    return a


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t) * 1e3, out


def commit_loop(ctx, d, ps, ws, m):
    out = np.zeros((m, 12), dtype=np.uint64)
    calls = [(ptr(ps[i]), ptr(ws[i]), ptr(out[i])) for i in range(m)]

    def run():
        for p, w, o in calls:
            assert ctx.lib.halo_pcdl_commit(ctx.h, p, d + 1, d, w, o) == 0, ctx.lib.halo_last_error()
    ms, _ = timed(run)
    return ms, out, 0


def commit_batch(ctx, d, ps, ws, m):
    out = np.zeros((m, 12), dtype=np.uint64)
    p, w, o = ptr(ps), ptr(ws), ptr(out)
    ms, rc = timed(lambda: ctx.lib.halo_pcdl_commit_batch(ctx.h, d, p, m, w, o))
    assert rc == 0, ctx.lib.halo_last_error()
    return ms, out, 0


def commit_dev_loop(ctx, d, dptrs, length, ws, m):
    out = np.zeros((m, 12), dtype=np.uint64)
    calls = [(C.c_void_p(dptrs[i]), ptr(ws[i]), ptr(out[i])) for i in range(m)]

    def run():
        for p, w, o in calls:
            assert ctx.lib.halo_pcdl_commit_dev(ctx.h, p, length, d, w, o) == 0, ctx.lib.halo_last_error()
    ms, _ = timed(run)
    return ms, out, 0


def commit_dev_batch(ctx, d, dptrs, length, ws, m):
    out = np.zeros((m, 12), dtype=np.uint64)
    ptrs = (C.c_void_p * m)(*dptrs[:m])
    lens = (C.c_size_t * m)(*([length] * m))
    status = (C.c_int * m)()
    w, o = ptr(ws), ptr(out)
    ms, rc = timed(lambda: ctx.lib.halo_pcdl_commit_dev_batch(ctx.h, d, ptrs, lens, m, w, o, status))
    assert rc == 0, ctx.lib.halo_last_error()
    return ms, out, 0


def instance_three_calls(ctx, d, ps, zs, ws, m, state):
    iw = ctx.lib.halo_instance_words((d + 1).bit_length() - 1)
    out = np.zeros((m, iw), dtype=np.uint64)
    vs = np.zeros((m, 4), dtype=np.uint64)
    calls = [(ptr(ps[i]), ptr(zs[i]), ptr(ws[i]), ptr(out[i]), ptr(vs[i]), ptr(out[i][21:])) for i in range(m)]
    st = C.c_uint64(state)

    def run():
        for p, z, w, o, v, pf in calls:
            assert ctx.lib.halo_pcdl_commit(ctx.h, p, d + 1, d, w, o) == 0, ctx.lib.halo_last_error()
            assert ctx.lib.halo_poly_eval(ctx.h, p, d + 1, z, v) == 0, ctx.lib.halo_last_error()
            assert ctx.lib.halo_pcdl_open(ctx.h, C.byref(st), p, d + 1, o, d, z, w, pf) == 0, ctx.lib.halo_last_error()
    ms, _ = timed(run)
    out[:, 12], out[:, 13:17], out[:, 17:21] = d, zs[:m], vs  # (packing the head is the caller's, outside the timed part)
    return ms, out, st.value


def instance_singles(ctx, d, ps, zs, ws, m, state):
    iw = ctx.lib.halo_instance_words((d + 1).bit_length() - 1)
    out = np.zeros((m, iw), dtype=np.uint64)
    calls = [(ptr(ps[i]), ptr(zs[i]), ptr(ws[i]), ptr(out[i])) for i in range(m)]
    st = C.c_uint64(state)

    def run():
        for p, z, w, o in calls:
            assert ctx.lib.halo_instance_from_poly(ctx.h, C.byref(st), p, d + 1, d, z, w, o) == 0, ctx.lib.halo_last_error()
    ms, _ = timed(run)
    return ms, out, st.value


def instance_batch(ctx, d, ps, zs, ws, m, state):
    iw = ctx.lib.halo_instance_words((d + 1).bit_length() - 1)
    out = np.zeros((m, iw), dtype=np.uint64)
    status = (C.c_int * m)()
    st = C.c_uint64(state)
    p, z, w, o = ptr(ps), ptr(zs), ptr(ws), ptr(out)
    ms, rc = timed(lambda: ctx.lib.halo_instance_from_poly_batch(ctx.h, C.byref(st), d, p, m, z, w, o, status))
    assert rc == 0, ctx.lib.halo_last_error()
    return ms, out, st.value


def alternate(ways, reps):
    """a warm-up of each way, then `reps` rounds through all of them in turn; all ways must give the same outputs and state"""
    first = [w() for w in ways]
    for r in first[1:]:
        assert r[1].tolist() == first[0][1].tolist() and r[2] == first[0][2], "the ways differ"
    ms = [[] for _ in ways]
    for _ in range(reps):
        for k, w in enumerate(ways):
            ms[k].append(w()[0])
    return [Timing(statistics.median(x), min(x), max(x)) for x in ms]


class Timing(float):
    """the median of a way's runs, with their least and greatest beside it"""

    def __new__(cls, median, lo, hi):
        t = super().__new__(cls, median)
        t.range = [round(lo, 3), round(hi, 3)]
        return t


def spread(**ways):
    """{"way": [min, max]} of the runs behind each median of a row"""
    return {k: v.range for k, v in ways.items()}


def forced(fn, group, hook="commit_batch_group"):
    def run():
        h._lib.dev_hook(hook, group)
        try:
            return fn()
        finally:
            h._lib.dev_hook("reset", 0)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default=",".join(map(str, SIZES)))
    ap.add_argument("--ms", default="1,8,64")
    ap.add_argument("--big-ms", default="8", help="the batch sizes at n >= 2^20")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_commit_batch.json"))
    a = ap.parse_args()
    import torch
    rows = {"commit_host": [], "commit_dev_in_place": [], "commit_dev_padded": [], "instance": []}
    for n in [int(x) for x in a.sizes.split(",")]:
        d = n - 1
        ms_list = [int(x) for x in (a.big_ms if n >= 1 << 20 else a.ms).split(",")]
        top = max(ms_list)
        group = 1 if n >= 1 << 20 else 8
        ctx = h._lib.Context(urs_n=n)
        try:
            if n >= 1 << 20:
                ctx.set_fold_table(0)
            g = np.random.default_rng(0x48414C4F00000500 + n)
            ps, zs, ws = scalars(g, (top, n)), scalars(g, (top,)), scalars(g, (top,))
            dev = [torch.from_numpy(ps[i].view(np.int64).reshape(-1)).cuda() for i in range(top)]
            dptrs = [t.data_ptr() for t in dev]
            torch.cuda.synchronize()
            short = n - n // 4
            for m in ms_list:
                p, z, w = np.ascontiguousarray(ps[:m]), np.ascontiguousarray(zs[:m]), np.ascontiguousarray(ws[:m])
                lo, ba, fo = alternate([lambda: commit_loop(ctx, d, p, w, m), lambda: commit_batch(ctx, d, p, w, m),
                                        forced(lambda: commit_batch(ctx, d, p, w, m), group)], a.reps)
                rows["commit_host"].append({"n": n, "m": m, "loop_ms": round(lo, 3), "batch_ms": round(ba, 3), "forced_ms": round(fo, 3),
                                            "speedup": round(lo / ba, 2), "min_max_ms": spread(loop=lo, batch=ba, forced=fo)})
                for name, length in (("commit_dev_in_place", n), ("commit_dev_padded", short)):
                    lo, ba, fo = alternate([lambda: commit_dev_loop(ctx, d, dptrs, length, w, m), lambda: commit_dev_batch(ctx, d, dptrs, length, w, m),
                                            forced(lambda: commit_dev_batch(ctx, d, dptrs, length, w, m), group)], a.reps)
                    rows[name].append({"n": n, "m": m, "len": length, "loop_ms": round(lo, 3), "batch_ms": round(ba, 3), "forced_ms": round(fo, 3),
                                       "speedup": round(lo / ba, 2), "min_max_ms": spread(loop=lo, batch=ba, forced=fo)})
                lo, si, ba, fo = alternate([lambda: instance_three_calls(ctx, d, p, z, w, m, 7 + m), lambda: instance_singles(ctx, d, p, z, w, m, 7 + m),
                                            lambda: instance_batch(ctx, d, p, z, w, m, 7 + m),
                                            forced(lambda: instance_batch(ctx, d, p, z, w, m, 7 + m), 4, "open_batch_group")], a.reps)
                rows["instance"].append({"n": n, "m": m, "three_calls_loop_ms": round(lo, 3), "single_call_loop_ms": round(si, 3),
                                         "batch_ms": round(ba, 3), "forced_ms": round(fo, 3), "speedup": round(lo / ba, 2),
                                         "min_max_ms": spread(three_calls_loop=lo, single_call_loop=si, batch=ba, forced=fo)})
                print(json.dumps({"progress": [n, m]}), file=sys.stderr, flush=True)
            del dev
        finally:
            ctx.close()
    result = {"tool": "tools/time_commit_batch.py", "workload": "m x pcdl::commit (hiding, full degree; host and device-resident) and m x Instance "
              "from the caller's polynomial (commit, evaluate, hiding open), 1 GPU, a context of n points per size", "reps": a.reps,
              "statistic": "median of alternating runs, ms", "equal": "points, blobs and final RNG states: every way equal for every row", **rows}
    line = json.dumps(result)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
