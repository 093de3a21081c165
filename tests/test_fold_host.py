"""The lanes of the key-fold kernels (csrc/fold_lane.hpp: fold_one, fold_one4 -- what k_fold_points and k_fold_points4 run once or
twice per lane) compiled for the CPU under ASan + UBSan (tests/native/fold_host.cpp), over the edge challenges and exceptional keys
of tests/fold_cases.py, against the oracle's fold, exactly.  The GPU file tests/test_gpu_fold_points.py runs the same cases through
every kernel form; the quad and table kernels (DPP, threadIdx) exist on the device only."""
import pytest

import fold_cases as fc


@pytest.fixture(scope="module")
def fold_host(tmp_path_factory):
    d = tmp_path_factory.mktemp("fold_host")
    exe, why = fc.build_host(d)
    if exe is None:
        pytest.skip(why)
    return exe, d


def test_challenge_list_reaches_the_edges_of_the_digit_packing():
    """The kernels walk digit strings packed ten to a word and start the top word at k = (n - 1) % 10: the list holds a string
    whose top digit is the last of its word, one whose top digit is the first of a later word, a one-digit string and the empty
    one; the comb digits of the table scalars hold +32, -32, an empty lambda half and an empty plain half."""
    import halo_accumulation_amd as h
    lib = h.load()
    facts = fc.check_digit_edges(lib)
    for k, v in facts.items():
        print("%-36s %s" % (k, v))
    for nm, x in fc.table_scalars(lib):
        print("table scalar %-20s %x" % (nm, x))


@pytest.mark.parametrize("levels", [1, 2])
@pytest.mark.parametrize("m", fc.SIZES)
def test_fold_lanes_match_the_oracle_and_are_sanitizer_clean(fold_host, levels, m):
    """fold_one / fold_one4 for every j of every case at this size: the whole challenge list at m = 3, 65, 257 (levels 2: every
    challenge as xi1 and as xi2 against a random partner, s1 == s2, s3 == 1, lengths that differ by a hundred digits, triples with
    zero members), two challenges at the other sizes; keys with infinities, scalar-related, equal and opposite points and the
    Straus collisions in every class of fold_cases.  Equal to the oracle's fold on every output; ASan and UBSan silent."""
    exe, d = fold_host
    cs = fc.cases(levels, m)
    outs = fc.run_host(exe, d, cs, "%d_%d" % (levels, m))
    for c, out in zip(cs, outs):
        fc.assert_same(out, c.want, "levels %d, m = %d, %s" % (levels, m, c.name))
    print("levels %d m = %d: %d cases, %d outputs, classes %s" % (levels, m, len(cs), len(cs) * m, fc.class_counts(cs)))
