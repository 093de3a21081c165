"""halo_acc_prover_batch above the no-fold size: the members' opens on the folded schedule of the open batches (member-batched key
folds, the batched MSMs over each member's staged key), their coefficients h(X) accumulated on the device.  A lowered switch
(halo_set_ipa_switch) brings every fold step -- one level, two levels, two steps -- down to keys of 2^7 .. 2^10 points, the hook
"open_batch_fold" forces the schedule.  Every accumulator word, every status, the message and the final RNG state against the loop
of halo_acc_prover from the same state, halo_ctx_info(10) against the members that reach their opens, and the oracle's prover."""
import numpy as np
import pytest

import orc
import test_gpu_open_batch_fold as ob
import test_gpu_prover_batch as pb

pytestmark = pytest.mark.gpu

SWITCH_LG = 6


@pytest.fixture(scope="module")
def hal():
    import halo_accumulation_amd as h
    return h


@pytest.fixture(scope="module")
def ctx(hal):
    """2^10 URS points, the switch at 2^6: provers of 2^7 .. 2^10 points fold their key"""
    c = hal._lib.Context(urs_n=1 << 10)
    c.set_ipa_switch(1 << SWITCH_LG)
    yield c
    c.close()


@pytest.fixture
def forced(hal):
    hal._lib.dev_hook("open_batch_fold", 1)
    yield
    hal._lib.dev_hook("reset", 0)


def member_list(hal, c, lg, k):
    """k members over the step-shaped pairs of test_gpu_prover_batch: 2, 0, 1 and 3 instances, a member whose instance is rejected
    (its v tampered) and one with d_i != d, in turn; one member alone has 2"""
    base = pb.step_members(hal, c, lg, max(k, 2))
    out = []
    for j in range(k):
        q, other = base[j], base[(j + 1) % len(base)]
        kind = j % 6
        out.append([q, [], [q[1]], q + [other[1]], pb.tampered(q, lg, "v"), pb.tampered(q, lg, "d_i")][kind])
    return out


@pytest.mark.parametrize("k", [1, 4, 5, 9])
@pytest.mark.parametrize("lg", [7, 8, 9, 10])
def test_parity_with_the_loop(hal, ctx, forced, lg, k):
    assert ob.fold_steps(lg, SWITCH_LG) == {7: [1], 8: [2], 9: [2, 1], 10: [2, 2]}[lg]
    d = (1 << lg) - 1
    members = member_list(hal, ctx, lg, k)
    _, status, _, _ = pb.expect_like_loop(ctx, d, members, 0xF01D0000 + 64 * lg + k)
    E = hal._lib.HALO_E_REJECT
    assert status == [E if j % 6 in (4, 5) else 0 for j in range(k)]
    assert ctx.info(10) == status.count(0), "the members that reach their opens ran through member-batched launches"


def test_the_loop_when_not_forced(hal, ctx):
    """the hook at 2: one member at a time, the same answer, nothing batched"""
    lg, k = 9, 5
    members = member_list(hal, ctx, lg, k)
    hal._lib.dev_hook("open_batch_fold", 1)
    try:
        want = pb.run_batch(ctx, (1 << lg) - 1, members, 0x100B)
        assert ctx.info(10) == 4
        hal._lib.dev_hook("open_batch_fold", 2)
        got = pb.run_batch(ctx, (1 << lg) - 1, members, 0x100B)
        assert pb.same(got, want) and ctx.info(10) == 0
    finally:
        hal._lib.dev_hook("reset", 0)


def test_device_form_ran(hal, ctx, forced):
    """five members that reach their opens: groups of 4 + 1, one accumulate launch and one batched fold per step each"""
    lg = 10
    d = (1 << lg) - 1
    members = pb.step_members(hal, ctx, lg, 5)
    want = pb.run_batch(ctx, d, members, 0xD0D0)
    assert want[0] == 0 and ctx.info(10) == 5
    got = []
    ran = pb.launches(ctx, lambda: got.append(pb.run_batch(ctx, d, members, 0xD0D0)))
    assert pb.same(got[0], want)
    assert ran.get("k_h_accumulate_batch", 0) == 2 and ran.get("k_h_coeffs", 0) == 0
    assert sum(ran.get(name, 0) for name in ob.FOLD_KERNELS) == 2 * len(ob.fold_steps(lg, SWITCH_LG)), ran


def test_oracle(hal, ctx, forced):
    """the oracle's prover from each member's start state, the RNG state chained from member to member"""
    lg, k = 8, 3
    d = (1 << lg) - 1
    members = member_list(hal, ctx, lg, 4)[:1] + member_list(hal, ctx, lg, 4)[2:]  # 2, 1 and 3 instances
    rc, status, _, blobs, final = pb.run_batch(ctx, d, members, 0x0AC1E)
    assert rc == 0 and status == [0] * k and ctx.info(10) == k
    pp = orc.make_pp(ctx.read_bases(0, d + 1))
    s = 0x0AC1E
    for j in range(k):
        want, s = orc.acc_prover(pp, s, d, members[j])
        assert blobs[j].tolist() == np.asarray(want).tolist(), "member %d" % j
    assert final == s
