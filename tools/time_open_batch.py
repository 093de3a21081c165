"""pcdl::open of k polynomials timed two ways: the serial halo_pcdl_open loop and ONE halo_pcdl_open_batch, with hiding (as
random_instance and acc::prover open), alternating in the same process after a warm-up of each shape; and k x
halo_random_instance against one halo_random_instance_batch.  A 2^14-point URS context; n in {512 .. 16384} at full degree,
k in {10, 100, 1000}; a sweep of the members per launch (the development hook open_batch_group) at k = 100; with --big a k = 4
leg at n = 2^20 on a 2^20-point context with the fold table fixed off (halo_set_fold_table 0), so that no table build lands
inside a timed run.  The proofs, instances and final RNG states of both ways must be equal.  Prints one JSON line; every time
is the median of --reps alternating runs, in ms.
With --fold (alone: the other legs are skipped) the sizes ABOVE the no-fold size, n = 2^15 and 2^16 on a 2^16-point context and
n = 2^17, 2^18 and 2^19 on a context of n points (--lgs picks among them), m in {8, 64} (--ms; at 2^19 the least of them only) hiding members, for the open batch, halo_random_instance_batch and halo_instance_from_poly_batch: the same batched call
with the development hook open_batch_fold = 2 (the loop over the single calls' bodies) and = 1 (the folded schedule with
member-batched key folds), alternating in one process; medians of --reps (at least 5) runs with the least and the greatest, and
"won" where every run of the folded schedule was faster than every run of the loop.
With --dev (alone) polynomials that live in device memory: n in {2^10, 2^14, 2^16} on a 2^16-point context, m in {8, 64} hiding
members at full degree, three ways alternating in one process -- the loop over halo_pcdl_open_dev, ONE halo_pcdl_open_dev_batch, and
halo_pcdl_open_batch behind the download a device-side caller needs in front of it (timed separately) -- medians of --reps (at least
5) runs with the least and the greatest; and ONE Instance from a device row (halo_instance_from_poly_dev_batch, m = 1) alone, the
host form's rule, against a forced group of one.  --out writes the JSON line to a file as well."""
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
from halo_accumulation_amd import pcdl  # noqa: E402
from halo_accumulation_amd._lib import ptr  # noqa: E402

SIZES = [512, 1024, 2048, 4096, 8192, 16384]


def scalars(g, shape):
    """canonical field elements (< 2^253 < r) as 4 words each"""
    a = g.integers(0, 2 ** 63, size=tuple(shape) + (4,), dtype=np.uint64)
    a[..., 3] &= np.uint64((1 << 61) - 1)
    return a


def inputs(ctx, n, k, seed):
    g = np.random.default_rng(seed)
    ps, zs, ws = scalars(g, (k, n)), scalars(g, (k,)), scalars(g, (k,))
    Cs = np.stack([pcdl.commit(ctx, ps[i], n - 1, ws[i]) for i in range(k)])
    return ps, Cs, zs, ws


def serial(ctx, d, args, k, state):
    ps, Cs, zs, ws = args
    out = np.zeros((k, ctx.lib.halo_proof_words((d + 1).bit_length() - 1)), dtype=np.uint64)
    calls = [(ptr(ps[i]), ptr(Cs[i]), ptr(zs[i]), ptr(ws[i]), ptr(out[i])) for i in range(k)]
    st = C.c_uint64(state)
    t = time.perf_counter()
    for p, c, z, w, o in calls:
        assert ctx.lib.halo_pcdl_open(ctx.h, C.byref(st), p, d + 1, c, d, z, w, o) == 0
    return (time.perf_counter() - t) * 1e3, out, st.value


def batched(ctx, d, args, k, state):
    ps, Cs, zs, ws = (np.ascontiguousarray(a[:k]) for a in args)
    out = np.zeros((k, ctx.lib.halo_proof_words((d + 1).bit_length() - 1)), dtype=np.uint64)
    status = (C.c_int * k)()
    st = C.c_uint64(state)
    t = time.perf_counter()
    rc = ctx.lib.halo_pcdl_open_batch(ctx.h, C.byref(st), d, ptr(ps), k, ptr(Cs), ptr(zs), ptr(ws), ptr(out), status)
    ms = (time.perf_counter() - t) * 1e3
    assert rc == 0, ctx.lib.halo_last_error()
    return ms, out, st.value


def ri_serial(ctx, d, k, state):
    out = np.zeros((k, ctx.lib.halo_instance_words((d + 1).bit_length() - 1)), dtype=np.uint64)
    rows = [ptr(out[i]) for i in range(k)]
    st = C.c_uint64(state)
    t = time.perf_counter()
    for o in rows:
        assert ctx.lib.halo_random_instance(ctx.h, C.byref(st), d, o) == 0
    return (time.perf_counter() - t) * 1e3, out, st.value


def ri_batched(ctx, d, k, state):
    out = np.zeros((k, ctx.lib.halo_instance_words((d + 1).bit_length() - 1)), dtype=np.uint64)
    st = C.c_uint64(state)
    t = time.perf_counter()
    rc = ctx.lib.halo_random_instance_batch(ctx.h, C.byref(st), d, k, ptr(out))
    ms = (time.perf_counter() - t) * 1e3
    assert rc == 0, ctx.lib.halo_last_error()
    return ms, out, st.value


def ifp_batched(ctx, d, args, k, state):
    ps, _, zs, ws = (np.ascontiguousarray(a[:k]) for a in args)
    out = np.zeros((k, ctx.lib.halo_instance_words((d + 1).bit_length() - 1)), dtype=np.uint64)
    status = (C.c_int * k)()
    st = C.c_uint64(state)
    t = time.perf_counter()
    rc = ctx.lib.halo_instance_from_poly_batch(ctx.h, C.byref(st), d, ptr(ps), k, ptr(zs), ptr(ws), ptr(out), status)
    ms = (time.perf_counter() - t) * 1e3
    assert rc == 0, ctx.lib.halo_last_error()
    return ms, out, st.value


def fold_leg(reps, lgs, ms):
    """the folded schedule against the loop above the no-fold size (see the module's text)"""
    reps = max(reps, 5)
    rows = []
    ctx = None

    def hooked(value, call, want_batched):
        def run():
            h._lib.dev_hook("open_batch_fold", value)
            try:
                r = call()
                assert ctx.info(10) == want_batched, (value, ctx.info(10))
                return r
            finally:
                h._lib.dev_hook("reset", 0)
        return run

    try:
        for lg in lgs:
            n, d = 1 << lg, (1 << lg) - 1
            if ctx is None or ctx.size != max(n, 1 << 16):
                if ctx is not None:
                    ctx.close()
                ctx = h._lib.Context(urs_n=max(n, 1 << 16))
            args = inputs(ctx, n, max(ms) if lg < 19 else min(ms), 0x48414C4F00000500 + n)
            for m in (ms if lg < 19 else [min(ms)]):
                shapes = {"open_batch": lambda: batched(ctx, d, args, m, 7 + m), "random_instance_batch": lambda: ri_batched(ctx, d, m, 11 + m),
                          "instance_from_poly_batch": lambda: ifp_batched(ctx, d, args, m, 13 + m)}
                for name, call in shapes.items():
                    loop, fold = hooked(2, call, 0), hooked(1, call, m)
                    a, b = loop(), fold()
                    assert a[1].tolist() == b[1].tolist() and a[2] == b[2], "the two ways differ"
                    l_ms, f_ms = [], []
                    for _ in range(reps):
                        l_ms.append(loop()[0])
                        f_ms.append(fold()[0])
                    rows.append({"shape": name, "n": n, "m": m, "loop_ms": round(statistics.median(l_ms), 3), "fold_ms": round(statistics.median(f_ms), 3),
                                 "loop_min_max_ms": [round(min(l_ms), 3), round(max(l_ms), 3)], "fold_min_max_ms": [round(min(f_ms), 3), round(max(f_ms), 3)],
                                 "speedup": round(statistics.median(l_ms) / statistics.median(f_ms), 2), "won": max(f_ms) < min(l_ms)})
                    print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    finally:
        if ctx is not None:
            ctx.close()
    return {"tool": "tools/time_open_batch.py --fold", "workload": "m hiding opens / random instances / Instances from the caller's polynomials "
            "(full degree) above the no-fold size, 1 GPU, context of max(2^16, n) points, default switch 2^14", "reps": reps,
            "statistic": "median of alternating runs, ms; loop = open_batch_fold 2, fold = open_batch_fold 1, same process",
            "rows": rows, "equal": "proofs, instances and final RNG states: loop == folded schedule for every row"}


def dev_leg(reps):
    """device-resident polynomials: the loop of single device opens, the device batch, the host batch behind a download"""
    import torch
    reps = max(reps, 5)
    ctx = h._lib.Context(urs_n=1 << 16)
    rows, alone = [], []

    def stats(ms):
        return round(statistics.median(ms), 3), [round(min(ms), 3), round(max(ms), 3)]

    try:
        for lg in (10, 14, 16):
            n, d = 1 << lg, (1 << lg) - 1
            words = ctx.lib.halo_proof_words(lg)
            ps, Cs, zs, ws = inputs(ctx, n, 64, 0x48414C4F00000600 + n)
            dev = torch.from_numpy(ps.reshape(-1).view(np.int64)).cuda()
            torch.cuda.synchronize()
            for m in (8, 64):
                ptrs = (C.c_void_p * m)(*[dev.data_ptr() + 32 * n * i for i in range(m)])
                lens = (C.c_size_t * m)(*([n] * m))

                def loop():
                    out = np.zeros((m, words), dtype=np.uint64)
                    st = C.c_uint64(7 + m)
                    calls = [(C.c_void_p(ptrs[i]), ptr(Cs[i]), ptr(zs[i]), ptr(ws[i]), ptr(out[i])) for i in range(m)]
                    t = time.perf_counter()
                    for p, c, z, w, o in calls:
                        assert ctx.lib.halo_pcdl_open_dev(ctx.h, C.byref(st), p, n, c, d, z, w, o) == 0
                    return (time.perf_counter() - t) * 1e3, out, st.value

                def dev_batch():
                    out = np.zeros((m, words), dtype=np.uint64)
                    status = (C.c_int * m)()
                    st = C.c_uint64(7 + m)
                    t = time.perf_counter()
                    rc = ctx.lib.halo_pcdl_open_dev_batch(ctx.h, C.byref(st), d, ptrs, lens, m, ptr(Cs), ptr(zs), ptr(ws), ptr(out), status)
                    ms = (time.perf_counter() - t) * 1e3
                    assert rc == 0 and ctx.info(10) == m, ctx.lib.halo_last_error()
                    return ms, out, st.value

                def host_batch():
                    t = time.perf_counter()
                    down = dev[: 4 * n * m].cpu().numpy().view(np.uint64).reshape(m, n, 4)  # (synchronous: a pageable destination)
                    dl = (time.perf_counter() - t) * 1e3
                    ms, out, state = batched(ctx, d, (down, Cs, zs, ws), m, 7 + m)
                    return ms + dl, out, state, dl

                a, b, c3 = loop(), dev_batch(), host_batch()
                assert a[1].tolist() == b[1].tolist() == c3[1].tolist() and a[2] == b[2] == c3[2], "the three ways differ"
                l_ms, d_ms, h_ms, dl_ms = [], [], [], []
                for _ in range(reps):
                    l_ms.append(loop()[0])
                    d_ms.append(dev_batch()[0])
                    r = host_batch()
                    h_ms.append(r[0])
                    dl_ms.append(r[3])
                (l, lr), (dv, dr), (hb, hr), (dl, _) = stats(l_ms), stats(d_ms), stats(h_ms), stats(dl_ms)
                rows.append({"n": n, "m": m, "loop_dev_ms": l, "dev_batch_ms": dv, "host_batch_with_download_ms": hb, "download_ms": dl,
                             "loop_dev_min_max_ms": lr, "dev_batch_min_max_ms": dr, "host_batch_min_max_ms": hr,
                             "dev_batch_over_loop": round(l / dv, 2), "host_batch_over_loop": round(l / hb, 2),
                             "dev_batch_slower_than_host_batch_beyond_ranges": min(d_ms) > max(h_ms)})
                print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
            # ONE Instance from a device row: alone through the single body (the host form's rule), against a group of one
            iw = ctx.lib.halo_instance_words(lg)
            one_p, one_l = (C.c_void_p * 1)(dev.data_ptr()), (C.c_size_t * 1)(n)

            def instance(group, want_batched):
                def run():
                    h._lib.dev_hook("open_batch_group", group)
                    try:
                        out = np.zeros((1, iw), dtype=np.uint64)
                        st = C.c_uint64(3)
                        t = time.perf_counter()
                        rc = ctx.lib.halo_instance_from_poly_dev_batch(ctx.h, C.byref(st), d, one_p, one_l, 1, ptr(zs[:1]), ptr(ws[:1]), ptr(out), None)
                        ms = (time.perf_counter() - t) * 1e3
                        assert rc == 0 and ctx.info(10) == want_batched, ctx.lib.halo_last_error()
                        return ms, out, st.value
                    finally:
                        h._lib.dev_hook("reset", 0)
                return run

            single, grouped = instance(0, 0), instance(1, 1)
            a, b = single(), grouped()
            assert a[1].tolist() == b[1].tolist() and a[2] == b[2]
            s_ms, g_ms = [], []
            for _ in range(reps):
                s_ms.append(single()[0])
                g_ms.append(grouped()[0])
            alone.append({"n": n, "alone_ms": stats(s_ms)[0], "group_of_one_ms": stats(g_ms)[0], "alone_min_max_ms": stats(s_ms)[1],
                          "group_of_one_min_max_ms": stats(g_ms)[1]})
            print(json.dumps(alone[-1]), file=sys.stderr, flush=True)
    finally:
        ctx.close()
    return {"tool": "tools/time_open_batch.py --dev", "workload": "m hiding opens of full-degree polynomials resident in device memory, 1 GPU, "
            "context of 2^16 points", "reps": reps, "statistic": "median of alternating runs, ms, least and greatest beside it; host batch = "
            "download of the m rows + halo_pcdl_open_batch", "rows": rows, "one_instance_from_a_device_row": alone,
            "equal": "proofs and final RNG states: loop == device batch == host batch for every row"}


def alternate(one, two, reps):
    """a warm-up of each, then `reps` alternating runs; both ways must give the same outputs and final state"""
    a, b = one(), two()
    assert a[1].tolist() == b[1].tolist() and a[2] == b[2], "the two ways differ"
    s_ms, b_ms = [], []
    for _ in range(reps):
        s_ms.append(one()[0])
        b_ms.append(two()[0])
    return statistics.median(s_ms), statistics.median(b_ms)


def row(n, k, s, b, what):
    return {"n": n, "k": k, "serial_ms": round(s, 3), "batch_ms": round(b, 3), "speedup": round(s / b, 2),
            "serial_ms_per_" + what: round(s / k, 4), "batch_ms_per_" + what: round(b / k, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", default=",".join(map(str, SIZES)))
    ap.add_argument("--ks", default="10,100,1000")
    ap.add_argument("--sweep", type=int, default=1, help="members-per-launch sweep at k = 100 (0: off)")
    ap.add_argument("--big", action="store_true", help="add the 2^20-point leg (k = 4)")
    ap.add_argument("--fold", action="store_true", help="only the folded schedule against the loop at n = 2^15 .. 2^19")
    ap.add_argument("--lgs", default="15,16,17,18,19", help="with --fold: log2 of the sizes")
    ap.add_argument("--ms", default="8,64", help="with --fold: the members per call")
    ap.add_argument("--dev", action="store_true", help="only the device-resident legs at n = 2^10, 2^14, 2^16")
    ap.add_argument("--out", default=None, help="with --fold or --dev: also write the JSON line to this file")
    a = ap.parse_args()
    if a.fold or a.dev:
        line = json.dumps(fold_leg(a.reps, [int(x) for x in a.lgs.split(",")], [int(x) for x in a.ms.split(",")]) if a.fold else dev_leg(a.reps))
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        print(line)
        return
    ks = [int(x) for x in a.ks.split(",")]
    ctx = h._lib.Context(urs_n=1 << 14)
    rows, ri_rows, sweep = [], [], []
    for n in [int(x) for x in a.sizes.split(",")]:
        d = n - 1
        args = inputs(ctx, n, max(ks), 0x48414C4F00000300 + n)
        for k in ks:
            s, b = alternate(lambda: serial(ctx, d, args, k, 7 + k), lambda: batched(ctx, d, args, k, 7 + k), a.reps)
            rows.append(row(n, k, s, b, "open"))
            s, b = alternate(lambda: ri_serial(ctx, d, k, 11 + k), lambda: ri_batched(ctx, d, k, 11 + k), a.reps)
            ri_rows.append(row(n, k, s, b, "instance"))
        if a.sweep and 100 in ks:
            for g in (1, 2, 4):
                h._lib.dev_hook("open_batch_group", g)
                try:
                    s, b = alternate(lambda: serial(ctx, d, args, 100, 5), lambda: batched(ctx, d, args, 100, 5), a.reps)
                finally:
                    h._lib.dev_hook("reset", 0)
                sweep.append({"n": n, "k": 100, "members_per_launch": g, "serial_ms": round(s, 3), "batch_ms": round(b, 3)})
        print(json.dumps({"progress_n": n}), file=sys.stderr, flush=True)
    ctx.close()
    big = []
    if a.big:
        n = 1 << 20
        c = h._lib.Context(urs_n=n)
        try:
            c.set_fold_table(0)
            args = inputs(c, n, 4, 0x48414C4F00000400)
            s, b = alternate(lambda: serial(c, n - 1, args, 4, 3), lambda: batched(c, n - 1, args, 4, 3), a.reps)
            big.append(row(n, 4, s, b, "open"))
        finally:
            c.close()
    print(json.dumps({"tool": "tools/time_open_batch.py", "workload": "k x pcdl::open with hiding (full-degree polynomials) and k x "
                      "random_instance (benches/acc.rs:15-29), 1 GPU, context of 2^14 points", "reps": a.reps, "statistic": "median",
                      "open": rows, "random_instance": ri_rows, "members_per_launch_sweep": sweep, "full_size": big,
                      "equal": "proofs, instances and final RNG states: loop == batch for every row"}))


if __name__ == "__main__":
    main()
