"""The sizes of the batched opens in one place each: OPEN_MAX_N in internal.hpp, the sizes the header comments of the six entry
points name, the default route in pcdl_batch.hip, and the rows of profiles/r18_*_batch_fold.json that DESIGN.md quotes -- they must
agree, and the routing must follow from the rows by the rule of DESIGN.md 4.5 (a size is routed only if every row of it won).
The fold_steps model of the GPU tests against OpenGroups::fold_levels_at at the sizes 2^17 .. 2^19."""
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "halo-accumulation_amd", "csrc")


def read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def profile(kind):
    return json.loads(read(ROOT, "profiles", "r18_%s_batch_fold.json" % kind))


def routed_sizes(kind):
    doc = profile(kind)
    sizes = sorted({r["n"] for r in doc["rows"]})
    return [n for n in sizes if all(r["won"] for r in doc["rows"] if r["n"] == n) and n not in doc.get("held_back_n", [])]


def fold_steps(lg, switch_lg):
    """tests/test_gpu_open_batch_fold.py's model (restated: that module needs a GPU to import its fixtures' library)"""
    steps, M = [], lg
    while M > switch_lg:
        k = min(2, M - switch_lg)
        steps.append(k)
        M -= k
    return steps


def fold_levels_at(M, nofold):
    """OpenGroups::fold_levels_at, read off the source below"""
    if M <= nofold:
        return 0
    return 2 if M // nofold >= 4 else 1


def test_max_n_and_the_header_agree():
    internal = read(CSRC, "internal.hpp")
    m = re.search(r"constexpr size_t OPEN_MAX_LG = (\d+), OPEN_MAX_N = \(size_t\)1 << OPEN_MAX_LG;", internal)
    assert m, "OPEN_MAX_N is 2^OPEN_MAX_LG"
    lg = int(m.group(1))
    assert lg == 19
    header = read(ROOT, "include", "halo_accumulation.h")
    for name in ("halo_pcdl_open_batch", "halo_random_instance_batch", "halo_instance_from_poly_batch", "halo_pcdl_open_dev_batch",
                 "halo_instance_from_poly_dev_batch", "halo_acc_prover_batch"):
        end = header.index("int %s(" % name)
        comment = header[header.rindex("/*", 0, end):end]
        sizes = [int(x) for x in re.findall(r"2\^(\d+)", comment)]
        assert max([s for s in sizes if s < 20], default=0) == lg, (name, sizes)  # (2^20: the table sizes some of them mention)
    assert "2^%d" % lg in read(ROOT, "INTEGRATION.md")
    assert "512 MiB" in header and "512 MiB" in read(ROOT, "INTEGRATION.md"), "the staging per slot at the largest size"


def test_the_default_route_follows_the_rows():
    src = read(CSRC, "pcdl_batch.hip")
    m = re.search(r"return n >= \(\(size_t\)1 << \(prover \? (\d+) : (\d+)\)\);", src)
    assert m, "open_fold_route's default"
    prover_from, open_from = int(m.group(1)), int(m.group(2))
    top = 19  # (OPEN_MAX_N: the callers' gate)
    assert routed_sizes("open") == [1 << lg for lg in range(open_from, top + 1)]
    assert routed_sizes("prover") == [1 << lg for lg in range(prover_from, top + 1)]
    for kind in ("open", "prover"):
        doc = profile(kind)
        assert doc["reps"] >= 5
        assert {r["n"] for r in doc["rows"]} == {1 << lg for lg in (15, 16, 17, 18, 19)}
        for r in doc["rows"]:
            assert r["won"] == (r["fold_min_max_ms"][1] < r["loop_min_max_ms"][0]), r
    assert profile("prover")["held_back_n"] == [1 << 15] and "held_back_n" in read(ROOT, "tools", "time_prover_batch.py"), "written by the tool"


def quoted(text, pattern):
    m = re.search(pattern, text)
    assert m, pattern
    return [float(x) for x in m.groups()]


def test_design_quotes_the_rows():
    design = read(ROOT, "DESIGN.md")
    assert "r18_open_batch_fold.json" in design and "r18_prover_batch_fold.json" in design
    assert "not wired" not in design
    rows = {(r["shape"], r["n"], r["m"]): r for r in profile("open")["rows"]}
    shapes = ("open_batch", "random_instance_batch", "instance_from_poly_batch")

    def shown(v):  # three significant figures, as the tables print them
        return float("%.3g" % v)

    for lg in (17, 18):
        got = quoted(design, r"\| 2\^%d, 64 \| ([\d.]+) / ([\d.]+) \| ([\d.]+) / ([\d.]+) \| ([\d.]+) / ([\d.]+) \|" % lg)
        want = [shown(rows[s, 1 << lg, 64][k]) for s in shapes for k in ("loop_ms", "fold_ms")]
        assert got == want, (lg, got, want)
    got = quoted(design, r"\| 2\^19, 8 \| ([\d.]+) / ([\d.]+) \| ([\d.]+) / ([\d.]+) \| ([\d.]+) / ([\d.]+) \|")
    assert got == [shown(rows[s, 1 << 19, 8][k]) for s in shapes for k in ("loop_ms", "fold_ms")], got
    ratios = [r["speedup"] for r in rows.values() if r["n"] <= 1 << 16]
    lo, hi = quoted(design, r"2\^15, 2\^16:\n([\d.]+)–([\d.]+)×")
    assert lo <= min(ratios) and max(ratios) <= hi
    prover = {(r["n"], r["k"]): r for r in profile("prover")["rows"]}
    for lg in (15, 16, 17):
        got = quoted(design, r"2\^%d ([\d.]+) / ([\d.]+)[;,]" % lg)
        assert got == [shown(prover[1 << lg, 64]["loop_ms"]), shown(prover[1 << lg, 64]["fold_ms"])], lg
    for lg in (18, 19):
        got = quoted(design, r"k = 8: .*2\^%d ([\d.]+) / ([\d.]+)[;,]" % lg)
        assert got == [shown(prover[1 << lg, 8]["loop_ms"]), shown(prover[1 << lg, 8]["fold_ms"])], lg
    assert re.search(r"2\^15 … 2\^19 take it by default", design) and "Default 2^16 … 2^19" in design and "held back" in design
    commit = json.loads(read(ROOT, "profiles", "r18_commit_batch_2_17.json"))
    got = quoted(design, r"\| 2\^17, 64 \| ([\d.]+) / ([\d.]+) \| ([\d.]+) / ([\d.]+) \| ([\d.]+) / ([\d.]+) \|\n\| 2\^20")
    h, dv, ins = commit["commit_host"][0], commit["commit_dev_in_place"][0], commit["instance"][0]
    want = [h["loop_ms"], h["batch_ms"], dv["loop_ms"], dv["batch_ms"], ins["three_calls_loop_ms"], ins["batch_ms"]]
    assert all(abs(g - w) <= 0.05 for g, w in zip(got, want)), (got, want)


def test_fold_steps_model_matches_fold_levels_at():
    src = read(CSRC, "pcdl_batch.hip")
    assert "if (M <= nofold) return 0;" in src and "return M / nofold >= 4 ? 2 : 1;" in src, "fold_levels_at as restated here"
    for lg, want in ((15, [1]), (16, [2]), (17, [2, 1]), (18, [2, 2]), (19, [2, 2, 1])):
        assert fold_steps(lg, 14) == want
        steps, M = [], 1 << lg
        while fold_levels_at(M, 1 << 14):
            steps.append(fold_levels_at(M, 1 << 14))
            M >>= steps[-1]
        assert steps == want and M == 1 << 14
