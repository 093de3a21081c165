"""halo_msm_sharded, halo_msm_dev_sharded and halo_msm_end_sharded on the GPU: world 1 is exactly halo_msm / halo_msm_dev (with
no callback and with the native RCCL all-gather); gloo worlds of 2, 3 and 4 ranks sharing this box's GPU (index shards, window
shards, batches) give on every rank the limbs of the whole-key MSM and of the oracle; a rank that fails locally leaves nobody
waiting, and the group works again afterwards."""
import os
import socket
import sys

import numpy as np
import pytest

import orc
import pallas_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x48414C4F00000005

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hal():
    import halo_accumulation_amd as h
    return h._lib


@pytest.fixture(scope="module")
def ctx1m(hal):
    c = hal.Context(urs_n=1 << 20)
    yield c
    c.close()


def _limbs(vals):
    return np.array([[(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)] for v in vals], dtype=np.uint64)


def _edge_scalars(n, seed=SEED):
    """n Montgomery scalars of the seeded stream, the first ones replaced by 0, 1 and r - 1"""
    sc, _ = orc.rng_scalars(seed, n)
    edge = orc.scalars_to_mont([0, 1, pm.R_ORDER - 1])
    k = min(n, 3)
    sc[:k] = edge[:k]
    return np.ascontiguousarray(sc)


def _dev(sc):
    import torch
    return torch.from_numpy(np.ascontiguousarray(sc).view(np.int64)).cuda()


# ------------------------------------------------------------------ world 1
@pytest.mark.parametrize("n", [1, 1 << 10, (1 << 16) + 1, 1 << 20])
def test_world_one_without_callback_is_halo_msm(hal, ctx1m, n):
    sc = _edge_scalars(n)
    want = ctx1m.msm(sc)
    assert ctx1m.msm_sharded(sc, 1, 0, None).tolist() == want.tolist()
    d = _dev(sc)
    want_dev = ctx1m.msm_dev(d.data_ptr(), n)
    assert want_dev.tolist() == want.tolist()
    assert ctx1m.msm_dev_sharded(d.data_ptr(), n, 1, 0, None).tolist() == want_dev.tolist()
    if n <= (1 << 16) + 1:  # plain integers (scalars_are_mont = 0)
        plain = _limbs([orc.fr_from_mont(x) for x in sc])
        assert ctx1m.msm_sharded(plain, 1, 0, None, mont=False).tolist() == want.tolist()
        assert ctx1m.msm_dev_sharded(_dev(plain).data_ptr(), n, 1, 0, None, mont=False).tolist() == want.tolist()
    if n <= 1 << 10:
        assert want.tolist() == orc.msm_affine(ctx1m.read_bases(0, n), sc).tolist()
    # the asynchronous end, after a device and a host begin
    ctx1m.msm_dev_begin(0, d.data_ptr(), n)
    assert ctx1m.msm_end_sharded(0, 1, 1, 0, None)[0].tolist() == want.tolist()
    ctx1m.msm_begin(1, sc)
    assert ctx1m.msm_end_sharded(1, 1, 1, 0, None)[0].tolist() == want.tolist()
    # n = 0 is the point at infinity; off shifts the bases as in halo_msm
    assert orc.point_canonical(ctx1m.msm_sharded(np.zeros((0, 4), dtype=np.uint64), 1, 0, None)) is None
    if n < 1 << 20:
        assert ctx1m.msm_sharded(sc, 1, 0, None, off=5).tolist() == ctx1m.msm(sc, off=5).tolist()


def test_world_one_local_failures_are_halo_msm_errors(hal, ctx1m):
    sc = _edge_scalars(16)
    with pytest.raises(hal.HaloError, match="range"):
        ctx1m.msm_sharded(sc, 1, 0, None, off=(1 << 20) - 8)
    with pytest.raises(hal.HaloError, match="nothing in flight"):
        ctx1m.msm_end_sharded(2, 1, 1, 0, None)
    d = _dev(sc)
    ctx1m.msm_dev_begin(2, d.data_ptr(), 16)
    with pytest.raises(hal.HaloError, match="different size"):
        ctx1m.msm_end_sharded(2, 2, 1, 0, None)
    assert ctx1m.msm_end_sharded(2, 1, 1, 0, None)[0].tolist() == ctx1m.msm(sc).tolist()


def test_world_one_native_rccl_allgather(hal, ctx1m):
    """libhalo_rccl.so's halo_allgather_rccl carries the collective as a C function pointer: one collective per call and one per
    batched end, and the point is halo_msm's"""
    from halo_accumulation_amd import rccl
    if not rccl.available():
        pytest.skip("libhalo_rccl.so not built (no librccl in this image)")
    n = 1 << 20
    sc = _edge_scalars(n)
    want = ctx1m.msm(sc)
    d = _dev(sc)
    sc2 = np.ascontiguousarray(sc[::-1])
    d2 = _dev(sc2)
    zero = _dev(np.zeros((n, 4), dtype=np.uint64))
    g = rccl.RcclGather(rccl.unique_id(), 0, 1, device=0)
    try:
        before = g.calls
        assert ctx1m.msm_sharded(sc, 1, 0, g).tolist() == want.tolist()
        assert g.calls == before + 1
        assert ctx1m.msm_dev_sharded(d.data_ptr(), n, 1, 0, g).tolist() == want.tolist()
        assert g.calls == before + 2
        ctx1m.msm_dev_batch_begin(0, [d.data_ptr(), zero.data_ptr(), d2.data_ptr()], n)
        got = ctx1m.msm_end_sharded(0, 3, 1, 0, g)
        assert g.calls == before + 3
        assert got[0].tolist() == want.tolist() and orc.point_canonical(got[1]) is None
        assert got[2].tolist() == ctx1m.msm_dev(d2.data_ptr(), n).tolist()
        # a local failure still goes through the one collective
        with pytest.raises(hal.HaloError, match="range"):
            ctx1m.msm_sharded(sc, 1, 0, g, off=1)
        assert g.calls == before + 4
    finally:
        g.close()


# ------------------------------------------------------------------ gloo worlds on the one GPU
def _rank_worker(case, rank, world, port, n, q):
    import datetime
    for p in (ROOT, os.path.join(ROOT, "oracle")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=240))
    try:
        _rank_case(case, rank, world, n, q)
        dist.barrier()
    except BaseException as e:  # the parent stops waiting at once (and ends the peers) instead of running into its time limit
        q.put((rank, "error: %r" % (e,)))
        raise
    finally:
        dist.destroy_process_group()


def _rank_case(case, rank, world, n, q):
    import halo_accumulation_amd as h
    from halo_accumulation_amd.sharded import make_allgather, shard_range
    ag, calls = make_allgather(), [0]

    def allgather(arr):
        calls[0] += 1
        return ag(arr)

    def counted(fn):
        before = calls[0]
        try:
            return fn().tolist(), calls[0] - before
        except h.HaloError as e:
            return str(e), calls[0] - before
    res = {}
    if case == "index":
        lo, hi = shard_range(n, rank, world)
        ctx = h._lib.Context(urs_n=max(hi - lo, 1), first_index=2 + lo)  # (a rank with no points still holds one)
        sc = np.ascontiguousarray(orc.rng_scalars(SEED, n)[0][lo:hi])
        d = _dev(sc)
        res["host"] = counted(lambda: ctx.msm_sharded(sc, world, rank, allgather))
        res["dev"] = counted(lambda: ctx.msm_dev_sharded(d.data_ptr(), hi - lo, world, rank, allgather))
    elif case == "window":
        ctx = h._lib.Context(urs_n=n)
        sc, _ = orc.rng_scalars(SEED, n)
        d, d2, zero = _dev(sc), _dev(np.ascontiguousarray(sc[::-1])), _dev(np.zeros((n, 4), dtype=np.uint64))
        ctx.msm_dev_begin(0, d.data_ptr(), n, part=rank, parts=world)
        res["part"] = counted(lambda: ctx.msm_end_sharded(0, 1, world, rank, allgather))
        members = [d.data_ptr(), zero.data_ptr(), d2.data_ptr()]
        ctx.msm_dev_batch_begin(0, members, n, part=rank, parts=world)
        res["batch"] = counted(lambda: ctx.msm_end_sharded(0, 3, world, rank, allgather))
        # two slots in flight, ended in issue order: two collectives
        ctx.msm_dev_batch_begin(0, members, n, part=rank, parts=world)
        ctx.msm_dev_begin(1, d2.data_ptr(), n, part=rank, parts=world)
        before = calls[0]
        first = ctx.msm_end_sharded(0, 3, world, rank, allgather)
        second = ctx.msm_end_sharded(1, 1, world, rank, allgather)
        res["two"] = ((first.tolist(), second.tolist()), calls[0] - before)
    elif case == "fail":
        lo, hi = shard_range(n, rank, world)
        ctx = h._lib.Context(urs_n=hi - lo, first_index=2 + lo)
        sc = np.ascontiguousarray(orc.rng_scalars(SEED, n)[0][lo:hi])
        d = _dev(sc)
        h._lib.dev_hook("shard_fail_rank", 1)
        h._lib.dev_hook("shard_fail_at", -3)
        res["hook"] = counted(lambda: ctx.msm_sharded(sc, world, rank, allgather))
        res["hook_end"] = counted(lambda: (ctx.msm_dev_begin(0, d.data_ptr(), hi - lo), ctx.msm_end_sharded(0, 1, world, rank, allgather))[1])
        h._lib.dev_hook("reset", 0)
        # rank 1 asks for a range past its key
        res["range"] = counted(lambda: ctx.msm_sharded(sc, world, rank, allgather, off=1 if rank == 1 else 0))
        # rank 1 ends a slot it never started; rank 0's MSM on that slot is collected all the same
        if rank == 0:
            ctx.msm_dev_begin(3, d.data_ptr(), hi - lo)
        res["idle"] = counted(lambda: ctx.msm_end_sharded(3, 1, world, rank, allgather))
        res["clean"] = counted(lambda: ctx.msm_sharded(sc, world, rank, allgather))
        res["clean_dev"] = counted(lambda: ctx.msm_dev_sharded(d.data_ptr(), hi - lo, world, rank, allgather))
    q.put((rank, res))


def _run(case, world, n):
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_worker, args=(case, r, world, port, n, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    try:
        while len(res) < world:
            rank, r = q.get(timeout=300)
            assert not isinstance(r, str), "rank %d: %s" % (rank, r)
            res[rank] = r
    finally:
        import time
        deadline = time.monotonic() + 60
        for p in procs:
            p.join(timeout=max(1.0, deadline - time.monotonic()))
            if p.is_alive():
                p.kill()
                p.join(timeout=10)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    return res


@pytest.mark.parametrize("world, n", [(2, 1 << 20), (4, 1 << 20), (3, (1 << 17) + 3), (4, 3), (2, 1 << 21)])
def test_index_shards_gloo_on_one_gpu(hal, world, n):
    """shard_range blocks over halo_ctx_create_urs(2 + lo, hi - lo): 2^17 + 3 over 3 ranks gives uneven blocks on different
    pipelines, 3 over 4 a rank with n = 0, 2^21 over 2 a million host scalars per rank (the stretch path)"""
    res = _run("index", world, n)
    sc, _ = orc.rng_scalars(SEED, n)
    whole = hal.Context(urs_n=n)
    try:
        want = whole.msm(sc).tolist()
        if n <= 1 << 20:
            assert want == orc.msm_affine(whole.read_bases(), sc).tolist()
    finally:
        whole.close()
    for rank in range(world):
        for form in ("host", "dev"):
            got, ncalls = res[rank][form]
            assert got == want and ncalls == 1, (rank, form, got if isinstance(got, str) else "", ncalls)


def test_window_shards_and_batches_gloo_on_one_gpu(hal):
    """every rank holds the whole key: halo_msm_dev_begin_part(part = rank, parts = 2) + halo_msm_end_sharded is halo_msm_dev;
    a batch of 3 (one member all zero) is one collective and member-wise the unbatched results; two slots are two collectives"""
    n, world = 1 << 18, 2
    res = _run("window", world, n)
    sc, _ = orc.rng_scalars(SEED, n)
    whole = hal.Context(urs_n=n)
    try:
        d, d2 = _dev(sc), _dev(np.ascontiguousarray(sc[::-1]))
        w1, w2 = whole.msm_dev(d.data_ptr(), n).tolist(), whole.msm_dev(d2.data_ptr(), n).tolist()
    finally:
        whole.close()
    for rank in range(world):
        r = res[rank]
        assert r["part"] == ([w1], 1), rank
        got, ncalls = r["batch"]
        assert ncalls == 1 and got[0] == w1 and got[2] == w2 and orc.point_canonical(np.array(got[1], dtype=np.uint64)) is None
        (first, second), ncalls = r["two"]
        assert ncalls == 2 and first == got and second == [w2]


def test_a_failing_rank_gloo_on_one_gpu(hal):
    """rank 1 fails locally -- the development hook (shard_fail_at = -3), a range past its key, an idle slot: both ranks return
    the same code after exactly one collective, rank 1 with its own message, rank 0 naming rank 1; then a clean call works"""
    n, world = 1 << 16, 2
    res = _run("fail", world, n)
    sc, _ = orc.rng_scalars(SEED, n)
    whole = hal.Context(urs_n=n)
    try:
        want = whole.msm(sc).tolist()
    finally:
        whole.close()
    for case, own in (("hook", "injected"), ("hook_end", "injected"), ("range", "range"), ("idle", "nothing in flight")):
        for rank in range(world):
            msg, ncalls = res[rank][case]
            assert isinstance(msg, str) and ncalls == 1, (case, rank, msg, ncalls)
            code = "code %d" % (-4 if case.startswith("hook") else -3)
            assert code in msg, (case, rank, msg)
            if rank == 1:
                assert own in msg, (case, msg)
            else:
                assert "rank 1 failed locally" in msg, (case, msg)
    for rank in range(world):
        assert res[rank]["clean"] == (want, 1) and res[rank]["clean_dev"] == (want, 1), rank
