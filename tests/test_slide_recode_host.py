"""The sliding odd-digit recode of the all-shifts table plan (csrc/slide_lane.hpp: slide_canon + slide_recode, what k_tmsm_recode
runs per scalar) compiled for the CPU under ASan + UBSan (tests/native/slide_host.cpp).  Every scalar's digits are checked with
Python integers: odd, |d| < 2^20, at most 13 of them, no window past bit 255, and sum d 2^j = s mod r exactly."""
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 0x40000000000000000000000000000000224698fc0994a8dd8c46eb2100000001
SLOTS, WMAX = 13, 21


@pytest.fixture(scope="module")
def slide_host(tmp_path_factory):
    d = tmp_path_factory.mktemp("slide_host")
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = os.path.join(str(d), "slide_host")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    # is the sanitizer runtime there at all?  Asked of a program that cannot fail to compile for any other reason, so that an
    # error in slide_host.cpp or slide_lane.hpp is never taken for a missing runtime
    probe = os.path.join(str(d), "probe.cpp")
    with open(probe, "w") as f:
        f.write("int main() { return 0; }\n")
    p = subprocess.run(["g++", "-std=c++17"] + san + [probe, "-o", os.path.join(str(d), "probe")], capture_output=True, text=True, timeout=120)
    if p.returncode != 0 or subprocess.run([os.path.join(str(d), "probe")]).returncode != 0:
        pytest.skip("sanitizer runtime not installed")
    cmd = ["g++", "-std=c++17", "-O2", "-g"] + san + ["-I", os.path.join(ROOT, "halo-accumulation_amd", "csrc"),
                                                    os.path.join(ROOT, "tests", "native", "slide_host.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    return exe, str(d)


def recode(slide_host, scalars, tag):
    """-> per scalar a list of (d, j, w): the digits with their rows and the widths the rule gave their windows"""
    exe, d = slide_host
    fin, fout = os.path.join(d, tag + ".in"), os.path.join(d, tag + ".out")
    with open(fin, "wb") as f:
        f.write(b"".join(int(s).to_bytes(32, "little") for s in scalars))
    p = subprocess.run([exe, str(WMAX), fin, fout], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.startswith("ok %d" % len(scalars)) and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, \
        p.stdout + p.stderr[-3000:]
    rec = np.fromfile(fout, dtype=np.uint32).reshape(len(scalars), 1 + 3 * SLOTS)
    os.remove(fin); os.remove(fout)
    return rec


def check(scalars, rec):
    """the conditions every digit string must keep; returns the digit counts"""
    counts = rec[:, 0].astype(np.int64)
    assert counts.max() <= SLOTS, "more than %d digits: %d" % (SLOTS, counts.max())
    mag, neg, row = rec[:, 1::3].astype(np.int64), rec[:, 2::3].astype(np.int64), rec[:, 3::3].astype(np.int64)
    live = np.arange(SLOTS)[None, :] < counts[:, None]
    assert (mag[live] & 1).all(), "an even digit"
    assert (mag[live] < (1 << 20)).all(), "a digit of 2^20 or more"
    assert not mag[~live].any() and not neg[~live].any() and not row[~live].any(), "an unused slot is not zero"
    assert (row[live] < 255).all()
    for s, c, m, g, j in zip(scalars, counts, mag, neg, row):
        total, prev_end = 0, 0
        for k in range(c):
            d, at = int(m[k]), int(j[k])
            assert at >= prev_end, "windows overlap: %x" % s
            # the digit fits a window of at most WMAX bits that ends at or below bit 255 (|d| < 2^(w-1), or the unsigned last window)
            w = d.bit_length() if (g[k] == 0 and 255 - at <= WMAX) else d.bit_length() + 1
            assert w <= WMAX and at + w <= 255, "window past bit 255 or wider than %d: %x" % (WMAX, s)
            prev_end = at + d.bit_length()
            total += (-d if g[k] else d) << at
        assert total == s % R, "sum of the digits: %x" % s
    return counts


def edge_scalars():
    out = [0, 1, 2, R - 1, R - 2]
    for k in (20, 21, 22, 233, 234, 253, 254):
        out += [1 << k, (1 << k) + 1, (1 << k) - 1]
    out += [1 << 254, (1 << 254) + 1, R, R + 1, (1 << 255) - 1, 1 << 255, (1 << 255) + 1, 3 * R - 1, 3 * R, 3 * R + 1, (1 << 256) - 2, (1 << 256) - 1]  # non-canonical
    rnd = random.Random(7)
    out += [rnd.randrange(1 << 254, 1 << 256) for _ in range(2000)]
    out += [(1 << 254) - 1, (1 << 256) - 1]  # all ones, as a canonical and as a non-canonical input
    alt = sum(1 << k for k in range(1, 254, 2))
    out += [alt, alt >> 1]  # (1010...)_2, (0101...)_2
    for at in (0, 100, 214):  # a run of forty zero bits at bit `at` of a random scalar below r
        for _ in range(50):
            s = rnd.randrange(R) & ~(((1 << 40) - 1) << at)
            out.append(s)
    out += [(1 << 200) + 1, (1 << 254) | 1]
    # every window boundary the rule can produce near the top: a set bit at each position with ones below it
    out += [((1 << k) - 1) for k in range(1, 255)] + [((1 << k) | 1) for k in range(1, 255)]
    return out


def test_edge_scalars_keep_every_condition(slide_host):
    sc = edge_scalars()
    rec = recode(slide_host, sc, "edges")
    counts = check(sc, rec)
    assert counts[0] == 0 and counts[1] == 1
    print("edge scalars: %d, digit counts %d .. %d" % (len(sc), counts.min(), counts.max()))


def test_uniform_scalars_mean_digits_and_range_loads(slide_host):
    """10^5 uniform scalars below r.  Mean digits <= 12.05 (simulated: 12.007).  Range loads under the plan's mapping (coarse range
    = bucket & 511, bucket = (|d| - 1) / 2): the largest range holds 1.0695 x the mean of this set (seed 20) -- what uniform low bits give
    for 2345 entries per range (sigma 2.1 %, the largest of 512 ranges near + 3.3 sigma); bound = the observed maximum + 10 % = 1.176,
    inside the 1.25 the fine sort's LDS stage allows."""
    rnd = random.Random(20)
    sc = [rnd.randrange(R) for _ in range(100000)]
    rec = recode(slide_host, sc, "uniform")
    counts = check(sc, rec)
    mean = counts.mean()
    hist = np.bincount(counts, minlength=SLOTS + 1)
    print("digits per scalar: mean %.4f, histogram %s" % (mean, {k: int(v) for k, v in enumerate(hist) if v}))
    assert mean <= 12.05
    mag = rec[:, 1::3].astype(np.int64)
    live = np.arange(SLOTS)[None, :] < counts[:, None]
    ranges = ((mag[live] - 1) >> 1) & 511
    load = np.bincount(ranges, minlength=512)
    ratio = load.max() / load.mean()
    print("range loads: max / mean = %.4f, min / mean = %.4f" % (ratio, load.min() / load.mean()))
    assert ratio <= 1.176
    assert ratio <= 1.25
