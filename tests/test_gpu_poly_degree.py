"""halo_poly_degrees_dev (fr_vec.hip k_poly_degree_batch) against a numpy restatement of host_poly_degree: every length around the
kernel's wave, pass and chunk sizes; all-zero rows, a lone scalar 0, the last non-zero scalar non-zero in one word only (the lower
16-byte lane, the upper one) and at every boundary a block meets, r - 1 everywhere; one row, mixed rows, rows sharing a pointer,
more rows than the grid's y limit; the sources unchanged.  halo_poly_eval_dev against halo_poly_eval."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import orc
from pallas_model import R_ORDER

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANES, CHUNK, WAVE = 256, 1024, 64  # lanes of a block (16 bytes each: LANES / 2 scalars a pass), scalars per block, lanes per wave
LENGTHS = sorted({0, 1, 2} | {k + e for k in (WAVE // 2, LANES // 2, LANES, CHUNK) for e in (-1, 0, 1)} | {3 * CHUNK + 1})


def test_the_test_restates_the_kernels_constants():
    text = open(os.path.join(ROOT, "halo-accumulation_amd", "csrc", "internal.hpp")).read()
    assert re.search(r"constexpr uint32_t DEG_LANES = %d;" % LANES, text)
    assert re.search(r"constexpr uint32_t DEG_CHUNK = %d;" % CHUNK, text)
    kernel = open(os.path.join(ROOT, "halo-accumulation_amd", "csrc", "fr_vec.hip")).read()
    assert "threadIdx.x & ~63u" in kernel and "dim3(DEG_LANES)" in kernel
    assert (2 * CHUNK) % LANES == 0 and LANES % WAVE == 0


@pytest.fixture(scope="module")
def hal():
    import halo_accumulation_amd as h
    return h


@pytest.fixture(scope="module")
def ctx(hal):
    c = hal._lib.Context(urs_n=1 << 11)
    yield c
    c.close()


def ref_degree(row):
    """host_poly_degree: the index of the last scalar with a non-zero word, 0 for none"""
    nz = np.nonzero(row.reshape(-1, 4).any(axis=1))[0]
    return int(nz[-1]) if len(nz) else 0


def rows_of(length):
    """the contents of one length: (name, (length, 4) array)"""
    if length == 0:
        return [("empty", np.zeros((0, 4), dtype=np.uint64))]
    rnd, _ = orc.rng_scalars(0xDE6 + length, length)
    out = [("zero", np.zeros((length, 4), dtype=np.uint64))]
    first = np.zeros((length, 4), dtype=np.uint64)
    first[0] = rnd[0]
    out.append(("scalar 0 only", first))
    tops = {length - 1} | {p for p in (WAVE // 2 - 1, WAVE // 2, LANES // 2 - 1, LANES // 2, CHUNK - 1, CHUNK, 2 * CHUNK - 1, 2 * CHUNK) if p < length}
    for top in sorted(tops):
        for word in (0, 2, 3):  # (word 2 or 3 alone: only the upper 16-byte lane of the scalar is non-zero)
            a = rnd.copy()
            a[top:] = 0
            a[top, word] = 1 + top
            out.append(("top %d word %d" % (top, word), a))
    out.append(("r - 1", np.tile(orc.fr_to_mont(R_ORDER - 1), (length, 1))))
    return out


class Rows:
    """every row of LENGTHS x rows_of in one device buffer, uploaded once; a zero-length row has a null pointer"""

    def __init__(self):
        import torch
        self.names, self.host, self.off = [], [], []
        at = 0
        for length in LENGTHS:
            for name, a in rows_of(length):
                self.names.append("len %d, %s" % (length, name))
                self.host.append(a)
                self.off.append(at)
                at += length
        self.flat = np.concatenate(self.host).reshape(-1)
        self.dev = torch.from_numpy(self.flat.view(np.int64).copy()).cuda()
        self.want = [ref_degree(a) for a in self.host]

    def ptr(self, i):
        return self.dev.data_ptr() + 32 * self.off[i] if len(self.host[i]) else 0

    def length(self, i):
        return len(self.host[i])

    def unchanged(self):
        return np.array_equal(self.dev.cpu().numpy().view(np.uint64), self.flat)


@pytest.fixture(scope="module")
def rows():
    return Rows()


def test_every_length_and_content_in_one_call(ctx, rows):
    idx = range(len(rows.names))
    ctx.prof_enable(1)
    ctx.prof_reset()
    try:
        got = ctx.poly_degrees_dev([rows.ptr(i) for i in idx], [rows.length(i) for i in idx])
    finally:
        ctx.prof_enable(0)  # (collects the launches' events)
    assert ctx.prof()["k_poly_degree_batch"][1] == 1, "one launch for all rows"
    for i in idx:
        assert got[i] == rows.want[i], rows.names[i]
    assert rows.unchanged()


def test_one_row_at_a_time(ctx, rows):
    for i in range(len(rows.names)):
        assert ctx.poly_degrees_dev([rows.ptr(i)], [rows.length(i)]) == [rows.want[i]], rows.names[i]
    assert rows.unchanged()


@pytest.mark.parametrize("m", [9, 70])
def test_mixed_rows(ctx, rows, m):
    total = len(rows.names)
    idx = [(k * 37 + 5) % total for k in range(m)]  # (37 and the number of rows are coprime or not: repeats are rows sharing a pointer)
    assert len({rows.length(i) for i in idx}) > 4
    got = ctx.poly_degrees_dev([rows.ptr(i) for i in idx], [rows.length(i) for i in idx])
    assert got == [rows.want[i] for i in idx]
    assert rows.unchanged()


def test_rows_sharing_a_pointer(ctx, rows):
    i = rows.names.index("len %d, top %d word 2" % (3 * CHUNK + 1, CHUNK))
    p, a = rows.ptr(i), rows.host[i]
    lens = [3 * CHUNK + 1, CHUNK + 1, CHUNK, 1, LANES // 2 + 1, 0]
    assert ctx.poly_degrees_dev([p] * len(lens), lens) == [ref_degree(a[:k]) for k in lens]
    assert ref_degree(a[: CHUNK + 1]) == CHUNK and ref_degree(a[:CHUNK]) == CHUNK - 1
    assert rows.unchanged()


def test_more_rows_than_the_grids_y_limit(ctx, rows):
    m = 70000
    a = rows.names.index("len 2, top 1 word 3")  # degree 1 at length 2, degree 0 at length 1 (scalar 0 is non-zero)
    b = rows.names.index("len 2, scalar 0 only")  # degree 0 either way
    assert rows.host[a][0].any() and rows.want[a] == 1 and rows.want[b] == 0
    ptrs = [rows.ptr(a) if k % 3 else rows.ptr(b) for k in range(m)]
    lens = [1 + (k % 2) for k in range(m)]
    want = [1 if (k % 3 and k % 2) else 0 for k in range(m)]
    ctx.prof_enable(1)
    ctx.prof_reset()
    try:
        got = ctx.poly_degrees_dev(ptrs, lens)
    finally:
        ctx.prof_enable(0)
    assert ctx.prof()["k_poly_degree_batch"][1] == 2, "65535 rows, then the rest"
    assert got == want
    assert want[65534:65540] == got[65534:65540] and 1 in want[65535:]
    assert rows.unchanged()


def test_argument_errors_write_nothing(hal, ctx, rows):
    i = rows.names.index("len 2, r - 1")
    mark = 0xA5A5
    for ptrs, lens in (([rows.ptr(i) + 16], [1]), ([0], [1]), ([rows.ptr(i), rows.ptr(i) + 8], [2, 1])):
        m = len(ptrs)
        out = (C.c_size_t * m)(*([mark] * m))
        rc = ctx.lib.halo_poly_degrees_dev(ctx.h, (C.c_void_p * m)(*ptrs), (C.c_size_t * m)(*lens), m, out)
        assert rc == hal._lib.HALO_E_ARG and "null or misaligned" in ctx.lib.halo_last_error().decode()
        assert list(out) == [mark] * m
    out = (C.c_size_t * 1)(mark)
    assert ctx.lib.halo_poly_degrees_dev(ctx.h, None, None, 1, out) == hal._lib.HALO_E_ARG and out[0] == mark
    assert ctx.lib.halo_poly_degrees_dev(ctx.h, None, None, 0, None) == 0
    assert ctx.poly_degrees_dev([], []) == []


@pytest.mark.parametrize("length", [0, 1, 255, 256, 1025])
def test_poly_eval_dev(hal, ctx, length):
    import torch
    co, s = orc.rng_scalars(0xE7A1 + length, max(length, 1))
    z, _ = orc.rng_scalars(s, 1)
    co = co[:length]
    dev = torch.from_numpy(co.reshape(-1).view(np.int64).copy()).cuda() if length else None
    got = ctx.poly_eval_dev(dev.data_ptr() if length else 0, length, z[0])
    assert got.tolist() == ctx.poly_eval(co, z[0]).tolist()
    if length:
        assert got.tolist() == np.asarray(orc.poly_eval(co, z[0])).reshape(4).tolist()
        assert np.array_equal(dev.cpu().numpy().view(np.uint64), co.reshape(-1))
        v = np.full(4, 7, dtype=np.uint64)
        rc = ctx.lib.halo_poly_eval_dev(ctx.h, C.c_void_p(dev.data_ptr() + 8), 1, hal._lib.ptr(z[0]), hal._lib.ptr(v))
        assert rc == hal._lib.HALO_E_ARG and v.tolist() == [7] * 4
    else:
        assert not got.any()
