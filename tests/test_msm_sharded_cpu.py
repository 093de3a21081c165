"""The sharded MSM's C entry points without a device: halo_msm_sharded, halo_msm_dev_sharded and halo_msm_end_sharded are in
the header, the library, the ctypes binding and the Rust shim; misuse that every rank commits alike returns HALO_E_ARG before
any collective; a rank that fails on its own (here: every rank, whose context could not be created) still enters the ONE
collective, and every rank returns the same code after it."""
import ctypes as C
import os
import re
import socket
import sys

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("halo_msm_sharded", "halo_msm_dev_sharded", "halo_msm_end_sharded")


@pytest.fixture(scope="module")
def hal():
    import halo_accumulation_amd as h
    h.build()
    return h


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _counting_callback(hal, world):
    """a ctypes all-gather that counts its calls and hands back `world` copies of the record (no peers needed)"""
    calls = [0]

    def ag(arr):
        calls[0] += 1
        return np.tile(np.asarray(arr, dtype=np.uint64), (world, 1))
    cb = hal._lib.make_allgather_callback(ag, world)
    return cb, C.cast(cb, C.c_void_p), calls


def test_entry_points_in_header_library_binding_and_shim(hal):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "halo_accumulation.h")).read(), flags=re.S)
    lib = C.CDLL(hal._lib.LIB_PATH)
    ffi = open(os.path.join(ROOT, "integration", "ffi.rs")).read()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name + " is not declared in the header"
        assert hasattr(lib, name), name + " is not exported"
        assert name in hal._lib.declared_symbols(), name + " is not declared by _lib"
        assert re.search(r"pub fn %s\(" % name, ffi), name + " is not bound in ffi.rs"
    # and the development hook that drives their failure path is documented with its value
    assert "at = -3" in open(os.path.join(ROOT, "include", "halo_accumulation_dev.h")).read()


def test_misuse_returns_before_any_collective(hal):
    lib = hal.load()
    E = hal._lib.HALO_E_ARG
    cb, cbp, calls = _counting_callback(hal, 2)
    out = np.zeros(12 * 9, dtype=np.uint64)
    o = hal._lib.ptr(out)
    sc = np.zeros((4, 4), dtype=np.uint64)
    for world, rank, fn in ((0, 0, cbp), (2, 2, cbp), (65, 0, cbp), (2, 0, None), (3, 5, cbp)):
        assert lib.halo_msm_sharded(None, world, rank, 0, 4, hal._lib.ptr(sc), 1, fn, None, o) == E, (world, rank)
        assert lib.halo_msm_dev_sharded(None, world, rank, 0, 4, C.c_void_p(sc.ctypes.data), 1, fn, None, o) == E, (world, rank)
        assert lib.halo_msm_end_sharded(None, 0, 1, world, rank, fn, None, o) == E, (world, rank)
    for batch in (0, 9):
        assert lib.halo_msm_end_sharded(None, 0, batch, 2, 0, cbp, None, o) == E, batch
        assert "batch" in lib.halo_last_error().decode()
    # a null output is the same on every rank as well
    assert lib.halo_msm_sharded(None, 2, 0, 0, 0, None, 1, cbp, None, None) == E
    assert lib.halo_msm_end_sharded(None, 0, 1, 2, 0, cbp, None, None) == E
    assert calls[0] == 0, "an argument every rank passes alike reached the collective"


def test_null_context_on_one_rank_world_one(hal):
    """world 1 without a callback: exactly halo_msm, so a null context is halo_msm's error; with a callback: one collective"""
    lib = hal.load()
    out = np.zeros(12, dtype=np.uint64)
    assert lib.halo_msm_sharded(None, 1, 0, 0, 0, None, 1, None, None, hal._lib.ptr(out)) == hal._lib.HALO_E_ARG
    assert "null context" in lib.halo_last_error().decode()
    cb, cbp, calls = _counting_callback(hal, 1)
    assert lib.halo_msm_dev_sharded(None, 1, 0, 0, 0, None, 1, cbp, None, hal._lib.ptr(out)) == hal._lib.HALO_E_ARG
    assert calls[0] == 1 and "null context" in lib.halo_last_error().decode()


def test_python_callback_exception_reaches_the_caller(hal):
    class Boom(RuntimeError):
        pass

    def broken(arr):
        raise Boom("fabric down")
    ctx = hal._lib.Context.__new__(hal._lib.Context)  # a context that could not be created: its handle is null
    ctx.h, ctx.lib, ctx.device, ctx._children = None, hal.load(), 0, []
    with pytest.raises(Boom, match="fabric down"):
        ctx.msm_sharded(np.zeros((0, 4), dtype=np.uint64), 2, 1, broken)
    with pytest.raises(Boom):
        ctx.msm_dev_sharded(0, 0, 2, 0, broken)
    with pytest.raises(Boom):
        ctx.msm_end_sharded(0, 3, 2, 0, broken)
    # the library's own side of it: a failed collective is HALO_E_ARG with the "abort the process group" message
    cb = hal._lib.make_allgather_callback(broken, 2)
    out = np.zeros(12, dtype=np.uint64)
    rc = hal.load().halo_msm_sharded(None, 2, 0, 0, 0, None, 1, C.cast(cb, C.c_void_p), None, hal._lib.ptr(out))
    assert rc == hal._lib.HALO_E_ARG and "abort the process group" in hal.load().halo_last_error().decode()
    assert isinstance(cb.error, Boom)


def _null_ctx_worker(rank, world, port, q):
    for p in (ROOT, os.path.join(ROOT, "oracle")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import halo_accumulation_amd as h
    from halo_accumulation_amd.sharded import make_allgather
    lib = h.load()
    ag, calls = make_allgather(), [0]

    def allgather(arr):
        calls[0] += 1
        return ag(arr)
    cb = h._lib.make_allgather_callback(allgather, world)
    cbp = C.cast(cb, C.c_void_p)
    out = np.zeros(12 * 3, dtype=np.uint64)
    sc = np.zeros((8, 4), dtype=np.uint64)
    log = []
    for call in (lambda: lib.halo_msm_sharded(None, world, rank, 0, 8, h._lib.ptr(sc), 1, cbp, None, h._lib.ptr(out)),
                 lambda: lib.halo_msm_dev_sharded(None, world, rank, 0, 0, None, 0, cbp, None, h._lib.ptr(out)),
                 lambda: lib.halo_msm_end_sharded(None, 1, 3, world, rank, cbp, None, h._lib.ptr(out))):
        before = calls[0]
        rc = call()
        log.append((rc, calls[0] - before, lib.halo_last_error().decode()))
    # the group is still in step afterwards
    log.append(allgather(np.array([rank + 1], dtype=np.uint64)).reshape(-1).tolist())
    q.put((rank, log))
    dist.barrier()
    dist.destroy_process_group()


def test_null_contexts_enter_one_collective_gloo_world_three(hal):
    world = 3
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_null_ctx_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = dict(q.get(timeout=120) for _ in range(world))
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    for rank in range(world):
        log = res[rank]
        for rc, ncalls, msg in log[:3]:
            assert rc == hal._lib.HALO_E_ARG and ncalls == 1, (rank, rc, ncalls, msg)
            assert "null context" in msg, msg  # every rank failed the same way and keeps its own wording
        assert log[3] == [1, 2, 3]
