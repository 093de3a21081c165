"""The lanes of the verifier's small MSMs (csrc/small_msm_lane.hpp: small_msm_ladder -- what k_batch_small_msm and k_small_msm_seg
run once per lane), the additions of their shuffle trees (curve.hpp xyzz_add, in the two kernels' orders) and the shared inversion
of k_batch_to_affine (curve.hpp jac_batch_to_aff, on the kernel's index map) compiled for the CPU under ASan + UBSan
(tests/native/small_msm_host.cpp), over every case of tests/point_cases.py, against the oracle and the integer model, exactly.  The
GPU file tests/test_gpu_point_paths.py runs the same cases through the kernels; the cross-lane moves exist on the device only."""
import os
import re

import pytest

import orc
import point_cases as pc


@pytest.fixture(scope="module")
def host_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("small_msm_host")
    exe, why = pc.build_host(d)
    if exe is None:
        pytest.skip(why)
    cases, groups = pc.all_sum_cases(), pc.jac_groups()
    sums, affs = pc.run_host(exe, d, cases, groups)
    return cases, groups, sums, affs


def test_the_host_program_restates_the_kernels_constants():
    csrc = os.path.join(pc.ROOT, "halo-accumulation_amd", "csrc")
    assert re.search(r"constexpr int TBL_E = %d;" % pc.HOST_TBL_E, open(os.path.join(csrc, "msm_kernels.hpp")).read())
    assert re.search(r"constexpr int TBL_E = %d;" % pc.HOST_TBL_E, open(os.path.join(pc.ROOT, "tests", "native", "small_msm_host.cpp")).read())
    sums = open(os.path.join(csrc, "small_sums.hip")).read()
    assert '#include "small_msm_lane.hpp"' in sums and "JacN small_msm_ladder(" not in sums, "the kernels run the header's ladder"
    assert sums.count("small_msm_ladder(p, k, live)") == 2


def test_ladders_and_trees_match_the_oracle_and_are_sanitizer_clean(host_run):
    """the ladder of every term, the terms of every sum added in the order of k_batch_small_msm and in the order of
    k_small_msm_seg: both equal to the oracle's plain sum; ASan and UBSan silent"""
    cases, _, sums, _ = host_run
    bad = []
    for c, (batch_order, seg_order) in zip(cases, sums):
        for order, got in (("k_batch_small_msm", batch_order), ("k_small_msm_seg", seg_order)):
            if orc.point_canonical(got) != c.canon:
                bad.append((order, c.name))
    print("%d sums in two orders, %d different terms" % (len(cases), pc.unique_terms()))
    assert not bad, "%d wrong sums; first (order, case): %s" % (len(bad), bad[:8])
    assert len(cases) >= 700


def test_batch_to_affine_lanes_match_the_integer_model_and_are_sanitizer_clean(host_run):
    """jac_batch_to_aff<TBL_E> over every group, lane by lane as k_batch_to_affine forms them: every output word for word"""
    _, groups, _, affs = host_run
    compared = 0
    for g, got in zip(groups, affs):
        bad = pc.check_affine(got, g)
        assert not bad, "%s: %d wrong; first (index, class): %s" % (g.name, len(bad), bad[:8])
        compared += g.m
    print("%d groups, %d points" % (len(groups), compared))
    assert compared == sum(pc.STEP_SIZES) + 2 * sum(pc.RAGGED_SIZES)
