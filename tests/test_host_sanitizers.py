"""The host arithmetic of the product (csrc/host_math.hpp) under ASan + UBSan on the CPU build (GPU sanitizers are not
available on the pool): fixed-base table == double-and-add, GLV digits bounded, no UB / out-of-bounds anywhere.  The same for
the DEVICE arithmetic -- the lazy radix-2^29 fields and the group law on them -- compiled for the CPU and driven to the value
bounds its types declare (tests/lazy_cases.py, tests/native/lazy_field_host.cpp)."""
import os
import shutil
import subprocess

import pytest

import lazy_cases as lz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_math_is_sanitizer_clean(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "host_math_sanitize")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "halo-accumulation_amd", "csrc"), os.path.join(ROOT, "tests", "native", "host_math_sanitize.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "sanitize" in b.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr[-2000:]


def test_host_worker_is_thread_sanitizer_clean(tmp_path):
    """csrc/internal.hpp HostWorker (hand-over of host jobs between the caller and the helper thread, bounded spin while IPA
    states are alive, shutdown) under TSan.  Host-only: the HIP headers are included for their types, nothing is launched."""
    if shutil.which("g++") is None or not os.path.isdir("/opt/rocm/include"):
        pytest.skip("no g++ / HIP headers")
    exe = str(tmp_path / "host_worker_tsan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=thread", "-pthread", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           "-I", os.path.join(ROOT, "halo-accumulation_amd", "csrc"), os.path.join(ROOT, "tests", "native", "host_worker_tsan.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and ("sanitize" in b.stderr or "tsan" in b.stderr):
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok ") and "ThreadSanitizer" not in r.stderr, r.stdout + r.stderr[-2000:]


@pytest.fixture(scope="module")
def lazy_host(tmp_path_factory):
    d = tmp_path_factory.mktemp("lazy_host")
    exe, why = lz.build_host(d)
    if exe is None:
        pytest.skip(why)
    return lz.HostRunner(exe, d)


def test_lazy_fields_at_their_value_bounds_are_sanitizer_clean(lazy_host):
    """Every primitive of fq29.hpp / fr29.hpp in the largest-bound instantiation the kernels use (lz.FIELD_TABLE names the call
    site of each row), on 0, 1, p +- 1, k p + {-2..2} for every k up to the bound, K p - 1, q 2^254 and q 2^254 - 1, saturated low
    limbs and random values: congruent to the big-integer result, below the declared bound, limbs normalised, predicates true
    exactly on multiples of the modulus, products equal to the Montgomery quotient; ASan and UBSan silent."""
    import random
    rng = random.Random(0x4C415A59)
    rows = [(row, lz.field_cases(row, rng)) for row in lz.FIELD_TABLE]
    outs = lazy_host.run([(0, row[0], lz.encode_field(row, cases), None) for row, cases in rows])
    total = 0
    for (row, cases), out in zip(rows, outs):
        lz.check_field(row, cases, out, "host")
        print("%-28s %6d cases   (%s)" % (row[1], len(cases), row[7]))
        total += len(cases)
    print("lazy field layer: %d cases over %d instantiations" % (total, len(rows)))
    assert total >= 21598  # the sweep this test was planned from


def test_negation_bound_is_counted_where_a_negated_operand_is_used():
    """fq_neg<K>(0) is K p itself, so the contract of a negation is '<= K p' (fq29.hpp).  That is sound only because of who
    consumes it: a fused product, whose other factor is strictly below its bound (so K is what the static_assert must count --
    and it does: the rows of lz.NEG_FED_SLOT feed K p itself into that slot), or the sign flip of an affine y, a stored
    coordinate that only ever enters a product of bound 2 x 2.  A new use of fq_neg has to be added here with its reason."""
    assert lz.NEG_CONTRACT == "<="
    # (file, enclosing function, K, argument) -> who consumes the negated value
    reviewed = {
        ("curve.hpp", "xyzz_madd", 8, "acc.y"): "fused", ("curve.hpp", "jac_madd", 8, "p.y"): "fused", ("curve.hpp", "xyzz_add", 2, "S1"): "fused",
        ("curve.hpp", "aff_cneg", 2, "p.y"): "sign of y", ("curve.hpp", "aff_store", 2, "a.y"): "sign of y",
        ("fold_lane.hpp", "fold_one", 2, "hi.y"): "sign of y", ("fold_lane.hpp", "fold_one4", 2, "p.y"): "sign of y",
        ("key_fold.hip", "fold_points4_quad_lane", 2, "p.y"): "sign of y",
    }
    sites = lz.neg_call_sites()
    assert set(sites) == set(reviewed) and len(sites) == len(reviewed), sorted(set(sites) ^ set(reviewed))
    src = open(os.path.join(ROOT, "halo-accumulation_amd", "csrc", "fq29.hpp")).read()
    assert 'static_assert(Ka * Kb + Kc * Kd <= 120' in src and "<= Kc*p" in src
    for op, slot in lz.NEG_FED_SLOT.items():
        row = [r for r in lz.FIELD_TABLE if r[0] == op][0]
        ka, kb, kc, kd = row[3]
        assert slot == 2 and ka * kb + kc * kd <= 120


def test_group_law_over_non_canonical_representatives_is_sanitizer_clean(lazy_host, kat):
    """curve.hpp over operands the C ABI cannot produce: X + i p and Y + j p over the whole Fq<8> range, ZZ / ZZZ as v and v + p,
    Z = 1 and Z != 1; the generic sum, P + P and P + (-P) through every pair of representatives, infinity on either side and on
    both -- against pallas_model's affine arithmetic on the key table's points, exactly."""
    pc = lz.PointCases(kat)
    ops = list(range(16))
    outs = lazy_host.run(pc.blocks(ops))
    for op, out in zip(ops, outs):
        counts = pc.check(op, out, "host")
        print("%-28s %6d cases  %s" % (lz.POINT_OP_NAMES[op], len(pc.cases[op]), counts))
    # P = U2 - X1 + 8p of xyzz_madd took every multiple 1p .. 9p in the P = +-Q cases (limb 0 < 10: the full reduction decides);
    # the generic sums leave through the limb-0 shortcut
    assert lz.madd_p_multiples(pc.cases[lz.XYZZ_MADD]) == set(range(1, 10))
    assert lz.madd_p_multiples(pc.cases[lz.JAC_MADD], jac=True) == set(range(1, 10))


@pytest.mark.parametrize("op", [lz.XYZZ_MADD, lz.XYZZ_ADD], ids=["xyzz_madd", "xyzz_add"])
def test_chains_of_additions_without_normalising_stay_in_bounds(lazy_host, kat, op):
    got = lz.run_chains(lazy_host, kat, op)
    print(lz.POINT_OP_NAMES[op], got)
    assert got["steps"] >= 64
