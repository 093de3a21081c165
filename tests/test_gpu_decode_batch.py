"""halo_*_decode_batch on the GPU: the device square root (halo_dev_fq_sqrt) against Python integers over every 2-adic order;
the batch with its points decompressed on the device (k_point_decompress), forced and by default, word for word the loop of
single host decoders, malformed members included; every fallback (no staging, no idle slot, no budget) and a multi-device
context with the same output; bytes -> decode -> verifier / decider end to end."""
import ctypes as C

import numpy as np
import pytest

import decode_batch_cases as dc
import orc
import pallas_model as pm

pytestmark = pytest.mark.gpu

LG = 9
D = (1 << LG) - 1
K = 256
MASK = (1 << 64) - 1


@pytest.fixture(scope="module")
def hal():
    import halo_accumulation_amd as h
    return h


@pytest.fixture(scope="module")
def ctx(hal):
    c = hal._lib.Context(urs_n=1 << 14)
    yield c
    c.close()


@pytest.fixture(scope="module")
def material(hal, ctx):
    """K instances and the K accumulators over one instance each, produced on the GPU at n = 512, as words and as bytes"""
    from halo_accumulation_amd import acc as A
    rng = [0xDEC0DE0000 + LG]
    qs = A.random_instance_batch(ctx, rng, D, K)
    accs, codes = A.prover_batch(ctx, rng, D, [[q] for q in qs])
    assert codes == [0] * K
    return {"qs": qs, "accs": accs, "q_bytes": [hal._lib.instance_encode(q) for q in qs], "a_bytes": [hal._lib.accumulator_encode(a) for a in accs]}


def seeded(material, lib):
    """the good members with the malformed set spread among them: (instance datas, accumulator datas)"""
    qd, ad = list(material["q_bytes"]), list(material["a_bytes"])
    for n, (name, data) in enumerate(sorted(dc.malformed_instances(qd[3], LG).items())):
        qd[5 + 9 * n] = data
    inst_len = lib.halo_instance_encoded_size(LG, 1)
    for n, (name, data) in enumerate(sorted(dc.malformed_accumulators(ad[2], LG, inst_len).items())):
        ad[4 + 11 * n] = data
    return qd, ad


def decompress_launches(ctx):
    return ctx.prof().get("k_point_decompress", (0.0, 0))[1]


# ------------------------------------------------------------------ 1. the square root
def test_fq_sqrt_against_python_integers(hal, ctx):
    P = pm.P
    t = (P - 1) >> 32
    assert t & 1 and (t << 32) + 1 == P
    rnd = np.random.default_rng(20240601)
    draw = lambda: int.from_bytes(rnd.bytes(40), "little") % P
    elems, orders = [0, 1, P - 1], [None] * 3
    for k in range(33):
        found = 0
        while found < 4:
            c = draw()
            a = pow(c, 1 << (32 - k), P)
            b = pow(a, t, P)
            exact = pow(b, 1 << k, P) == 1 and (k == 0 or pow(b, 1 << (k - 1), P) != 1)
            if exact:
                elems.append(a); orders.append(k); found += 1
    elems += [draw() for _ in range(4096)]
    orders += [None] * 4096
    m = len(elems)
    a = np.zeros((m, 4), dtype=np.uint64)
    for i, e in enumerate(elems):
        v = e * pm.MONT_R % P
        a[i] = [(v >> (64 * w)) & MASK for w in range(4)]
    root = np.zeros((m, 4), dtype=np.uint64)
    ok = np.zeros(m, dtype=np.uint32)
    rc = ctx.lib.halo_dev_fq_sqrt(ctx.h, hal._lib.ptr(a), m, hal._lib.ptr(root), ok.ctypes.data_as(C.POINTER(C.c_uint32)))
    assert rc == 0, ctx.lib.halo_last_error()
    r_inv = pow(pm.MONT_R, -1, P)
    n_ok = 0
    for i, e in enumerate(elems):
        assert ok[i] in (0, 1)
        if ok[i]:
            r = sum(int(root[i, w]) << (64 * w) for w in range(4))
            assert r < P and (r * r_inv) ** 2 % P == e, "element %d (order 2^%s)" % (i, orders[i])
            n_ok += 1
        else:
            assert pow(e, (P - 1) // 2, P) == P - 1, "element %d (order 2^%s) is a square and was refused" % (i, orders[i])
        if orders[i] is not None:
            assert ok[i] == (0 if orders[i] == 32 else 1)
    assert ok[0] == 1 and ok[1] == 1 and ok[2] == 1, "0, 1 and p - 1 = -1 (p = 1 mod 4) are squares"
    assert 1800 < n_ok - 131 < 2300, "about half of the random elements are squares"


# ------------------------------------------------------------------ 2. the device form, forced and by default
@pytest.mark.parametrize("forced", [1, 0])
def test_device_form_matches_the_single_host_decoders(hal, ctx, material, forced):
    lib = ctx.lib
    qd, ad = seeded(material, lib)
    hal._lib.dev_hook("decode_batch_min", forced)
    ctx.prof_enable(1)
    try:
        for kind, datas, stride in (("instance", qd, lib.halo_instance_words(LG)), ("accumulator", ad, lib.halo_accumulator_words(LG) + 7),
                                    ("proof", [d[dc.INSTANCE_HEAD:] for d in qd], lib.halo_proof_words(LG))):
            ctx.prof_reset()
            st = dc.expect_like_singles(lib, kind, datas, stride, ctx)
            assert decompress_launches(ctx) == 1, "the points of the whole batch in one launch"
            assert 10 <= sum(1 for s in st if s) <= 20 and st[0] == 0
        # small batches: on the device when forced, on the pool by default -- the same words
        ctx.prof_reset()
        dc.expect_like_singles(lib, "accumulator", ad[:5], lib.halo_accumulator_words(LG), ctx)
        assert decompress_launches(ctx) == (1 if forced else 0)
        # a short stride: the accumulator's HALO_E_ARG and a bad point in front of it
        stride = lib.halo_accumulator_words(LG) - 1
        st = dc.expect_like_singles(lib, "accumulator", ad, stride, ctx)
        assert hal._lib.HALO_E_ARG in st and hal._lib.HALO_E_REJECT in st and 0 not in st
    finally:
        ctx.prof_enable(0)
        hal._lib.dev_hook("reset", 0)


def test_batches_larger_than_the_staging_run_in_chunks(hal, ctx, material):
    lib = ctx.lib
    _, ad = seeded(material, lib)
    stride = lib.halo_accumulator_words(LG)
    singles = [dc.single(lib, "accumulator", d, stride) for d in ad]
    reps = 13  # 13 x 256 members x 22 points: above the 2^16 points of one launch
    ctx.prof_enable(1)
    try:
        ctx.prof_reset()
        dc.expect_like_singles(lib, "accumulator", ad * reps, stride, ctx, singles=singles * reps)
        assert decompress_launches(ctx) == 2
    finally:
        ctx.prof_enable(0)


# ------------------------------------------------------------------ 3. the fallbacks
def test_every_fallback_gives_the_same_output(hal, ctx, material):
    import torch
    lib = ctx.lib
    _, ad = seeded(material, lib)
    stride = lib.halo_accumulator_words(LG)
    singles = [dc.single(lib, "accumulator", d, stride) for d in ad]
    run = lambda c: dc.expect_like_singles(lib, "accumulator", ad, stride, c, singles=singles)
    ctx.prof_enable(1)
    try:
        ctx.prof_reset()
        want = run(ctx)
        assert decompress_launches(ctx) == 1
        # the staging refused
        hal._lib.dev_hook("batch_stage_fail", 1)
        try:
            ctx.prof_reset()
            assert run(ctx) == want and decompress_launches(ctx) == 0
        finally:
            hal._lib.dev_hook("reset", 0)
        # a caller's MSM in flight on one slot: left alone; on every slot: the host pool
        n = 1 << 14
        sc, _ = orc.rng_scalars(0xC0FFEE, n)
        dev = torch.from_numpy(sc.view(np.int64).reshape(-1).copy()).cuda()
        ref = orc.msm_affine(ctx.read_bases(), sc)
        ctx.msm_dev_begin(0, dev.data_ptr(), n)
        try:
            ctx.prof_reset()
            assert run(ctx) == want
        finally:
            assert ctx.msm_dev_end(0).tolist() == ref.tolist(), "the caller's MSM on slot 0 kept its own result"
        for slot in range(4):
            ctx.msm_dev_begin(slot, dev.data_ptr(), n)
        try:
            assert run(ctx) == want
        finally:
            for slot in range(4):
                assert ctx.msm_dev_end(slot).tolist() == ref.tolist()
        assert run(None) == want, "no context: the host pool"
    finally:
        ctx.prof_enable(0)
    # no optional memory at all: a fresh context under a zero budget
    c = hal._lib.Context(urs_n=1 << 12)
    try:
        budget = c.info(3)
        c.set_memory_budget(0)
        try:
            before = c.info(4)
            c.prof_enable(1)
            assert run(c) == want and decompress_launches(c) == 0
            assert c.info(4) <= before, "no optional memory under a zero budget"
        finally:
            c.set_memory_budget(budget)
        c.prof_reset()
        assert run(c) == want and decompress_launches(c) == 1, "with the budget back: the device form"
    finally:
        c.close()
    # a multi-device context with one device repeated
    m = hal._lib.Context(urs_n=1 << 14, devices=[0, 0])
    try:
        assert run(m) == want
    finally:
        m.close()


# ------------------------------------------------------------------ 4. end to end
def test_bytes_to_verifier_and_decider(hal, ctx, material):
    from halo_accumulation_amd import acc as A
    E_REJECT = hal._lib.HALO_E_REJECT
    qb, ab = list(material["q_bytes"]), list(material["a_bytes"])
    aw, iw = ctx.lib.halo_accumulator_words(LG), ctx.lib.halo_instance_words(LG)
    accs, lgs, st = hal._lib.accumulator_decode_batch(ab, ctx, stride_words=aw)
    qs, qlgs, qst = hal._lib.instance_decode_batch(qb, ctx, stride_words=iw)
    assert st.tolist() == [0] * K and qst.tolist() == [0] * K and lgs.tolist() == [LG] * K and qlgs.tolist() == [LG] * K
    assert accs.shape == (K, aw) and qs.shape == (K, iw)
    for j in (0, 1, K - 1):
        assert accs[j].tolist() == material["accs"][j].tolist() and qs[j].tolist() == material["qs"][j].tolist()
    assert A.verifier_batch(ctx, D, [[qs[j]] for j in range(K)], [accs[j] for j in range(K)]) == [0] * K
    assert A.decider_batch(ctx, D, [accs[j] for j in range(K)]) == [0] * K
    # one flipped sign flag: -C_bar is a point too, the member decodes, and exactly that member fails downstream
    j = 97
    b = bytearray(ab[j]); b[32] ^= 0x80; ab[j] = bytes(b)
    accs2, _, st2 = hal._lib.accumulator_decode_batch(ab, ctx, stride_words=aw)
    assert st2.tolist() == [0] * K
    assert [i for i in range(K) if accs2[i].tolist() != accs[i].tolist()] == [j]
    want = [E_REJECT if i == j else 0 for i in range(K)]
    with pytest.raises(hal._lib.HaloReject) as e:
        A.verifier_batch(ctx, D, [[qs[i]] for i in range(K)], [accs2[i] for i in range(K)])
    assert e.value.args[1] == want
    with pytest.raises(hal._lib.HaloReject) as e:
        A.decider_batch(ctx, D, [accs2[i] for i in range(K)])
    assert e.value.args[1] == want
    # ... and in an instance: the U of member 11's proof
    i = 11
    o = dc.INSTANCE_HEAD + 8 + 33 * LG + 8 + 33 * LG
    b = bytearray(qb[i]); b[o + 32] ^= 0x80; qb[i] = bytes(b)
    qs2, _, qst2 = hal._lib.instance_decode_batch(qb, ctx, stride_words=iw)
    assert qst2.tolist() == [0] * K
    with pytest.raises(hal._lib.HaloReject) as e:
        A.verifier_batch(ctx, D, [[qs2[t]] for t in range(K)], [accs[t] for t in range(K)])
    assert e.value.args[1] == [E_REJECT if t == i else 0 for t in range(K)]
