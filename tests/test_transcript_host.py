"""The lanes of the device transcripts (csrc/keccak_lane.hpp: keccak_f1600 -- what k_urs_scalars and every rho_0 run;
csrc/transcript_lane.hpp: point_compress_lane, scalar_ok_lane, rho0_C_z_v, rho0_C_z_v_Cbar, rho0_xi_L_R -- what the k_transcript_*
kernels run once per lane) compiled for the CPU under ASan + UBSan (tests/native/transcript_lane_host.cpp), over the cases of
tests/transcript_cases.py, against hashlib.sha3_256 and the integer model (oracle/pallas_model.py), exactly.  The GPU file
tests/test_gpu_transcripts.py runs the kernels against the host's own transcript."""
import os
import re

import pytest

import pallas_model as pm
import transcript_cases as tc


@pytest.fixture(scope="module")
def host_run(tmp_path_factory):
    d = tmp_path_factory.mktemp("transcript_lane_host")
    exe, why = tc.build_host(d)
    if exe is None:
        pytest.skip(why)
    perms, hashes, pts, scs = tc.perm_cases(), tc.hash_cases(), tc.point_cases(), tc.scalar_cases()
    return (perms, hashes, pts, scs), tc.run_host(exe, d, perms, hashes, pts, scs)


def test_the_kernels_run_the_headers_lanes():
    csrc = os.path.join(tc.ROOT, "halo-accumulation_amd", "csrc")
    urs = open(os.path.join(csrc, "urs.hip")).read()
    assert '#include "keccak_lane.hpp"' in urs and "keccak_f1600(a);" in urs
    assert "rol64" not in urs and "PIL[" not in urs and "ROT[" not in urs and "0x8000000080008008" not in urs, "urs.hip carries no permutation of its own"
    lane = open(os.path.join(csrc, "keccak_lane.hpp")).read()
    assert "constexpr int ROT[24]" in lane and "constexpr int PIL[24]" in lane and "(q == r) ? RC[q] : rc" in lane
    tr = open(os.path.join(csrc, "transcript.hip")).read()
    assert '#include "transcript_lane.hpp"' in tr and "keccak_f1600" not in tr and not re.search(r"HALO_DEV \w+ rho0_", tr)
    for call in ("point_compress_lane(", "rho0_C_z_v_Cbar(", "rho0_C_z_v(", "rho0_xi_L_R(", "scalar_ok_lane("):
        assert call in tr, call
    assert "transcript.hip" in open(os.path.join(csrc, "Makefile")).read()
    gate = open(os.path.join(csrc, "check_resources.py")).read()
    for k in ("k_transcript_points", "k_transcript_head", "k_transcript_chain"):
        assert '"%s"' % k in gate, "the scratch gate must have seen " + k


def test_the_cases_cover_what_they_claim():
    hashes = tc.hash_cases()
    for form in (0, 1, 2):
        mine = [h for h in hashes if h.form == form]
        assert {h.subs for h in mine} == {0, 1, 2, 3}, "digests needing 0, 1, 2 and 3 subtractions of r"
        assert {(h.s0, h.s1) for h in mine} >= {(a, b) for a in (0, 1, tc.R - 1) for b in (0, 1, tc.R - 1)}
        assert any(h.p0 is None and h.p1 is not None for h in mine) and any(h.p1 is None and h.p0 is not None for h in mine)
        assert {tc.flag_of(h.p0) for h in mine} == {0, 0x40, 0x80} and {tc.flag_of(h.p1) for h in mine} == {0, 0x40, 0x80}
    pts = tc.points()
    assert tc.flag_of(pts["1G"]) != tc.flag_of(pts["-1G"])
    top = pts["top"]
    assert pm.is_on_curve(top) and top[0] >> 192 == tc.P >> 192 and top[0] < tc.P
    verdicts = {c[2] for c in tc.point_cases()}
    assert verdicts == {tc.VALID, tc.INVALID, tc.FOREIGN}


def test_the_checkers_reject_a_flipped_flag_and_a_wrong_digest_bit():
    h = tc.hash_cases()[0]
    good = tc.fr_mont(h.want) + tc.compressed(h.p0) + tc.compressed(h.p1)
    assert tc.check_hash(h, good) is None
    for bit in (0, 63, 64 * 3 + 61):
        bad = list(good)
        bad[bit // 64] ^= 1 << (bit % 64)
        assert tc.check_hash(h, bad) == "challenge differs"
    bad = list(good)
    bad[8] ^= 0x80
    assert tc.check_hash(h, bad) is not None
    case = tc.point_cases()[1]
    ok = case[3] + [case[2]]
    assert tc.check_point(case, ok) is None
    flipped = list(ok)
    flipped[4] ^= 0x80
    assert tc.check_point(case, flipped) == "encoding differs"
    wrong = list(ok)
    wrong[5] = tc.INVALID
    assert tc.check_point(case, wrong) is not None
    st, msg = tc.perm_cases()[3]
    import hashlib
    dig = int.from_bytes(hashlib.sha3_256(msg).digest(), "little")
    assert tc.check_perm(tc.words(dig), msg) is None and tc.check_perm(tc.words(dig ^ (1 << 200)), msg) is not None


def test_permutation_matches_sha3_and_is_sanitizer_clean(host_run):
    (perms, _, _, _), (states, _, _, _) = host_run
    bad = [len(msg) for (st, msg), out in zip(perms, states) if tc.check_perm(out, msg)]
    assert not bad, "message lengths with a wrong digest: %s" % bad
    assert len(perms) >= 24


def test_rho0_forms_match_the_model_and_are_sanitizer_clean(host_run):
    """every challenge as Montgomery words and both points' encodings, word for word"""
    (_, hashes, _, _), (_, res, _, _) = host_run
    bad = [(h.name, why) for h, got in zip(hashes, res) for why in [tc.check_hash(h, got)] if why]
    print("%d hashes" % len(hashes))
    assert not bad, "%d wrong; first: %s" % (len(bad), bad[:6])


def test_point_verdicts_and_scalar_bounds(host_run):
    (_, _, pts, scs), (_, _, pres, sres) = host_run
    bad = [(c[0], why) for c, got in zip(pts, pres) for why in [tc.check_point(c, got)] if why]
    assert not bad, bad[:6]
    bad = [c[0] for c, got in zip(scs, sres) if int(got) != c[2]]
    assert not bad, bad


def test_transcript_min_hook_without_a_gpu():
    """values >= 1 set the threshold, 0 the measured default, a negative value is refused and leaves the hook as it was"""
    import halo_accumulation_amd as hal
    lib = hal.load()
    try:
        assert lib.halo_dev_tuning(b"transcript_min") == 0
        for v in (1, 64, 0, 1000):
            assert lib.halo_dev_hook(b"transcript_min", v) == 0 and lib.halo_dev_tuning(b"transcript_min") == v
        for v in (-1, -64):
            assert lib.halo_dev_hook(b"transcript_min", v) == hal._lib.HALO_E_ARG and b"transcript_min is 0" in lib.halo_last_error()
            assert lib.halo_dev_tuning(b"transcript_min") == 1000
        assert lib.halo_dev_hook(b"reset", 0) == 0 and lib.halo_dev_tuning(b"transcript_min") == 0
        assert lib.halo_dev_hook(b"no_such_hook", 1) == hal._lib.HALO_E_ARG and b"transcript_min" in lib.halo_last_error()
        assert lib.halo_dev_transcripts(None, 1, None, 1, 1, None, None, None) == hal._lib.HALO_E_ARG and b"null context" in lib.halo_last_error()
    finally:
        lib.halo_dev_hook(b"reset", 0)
