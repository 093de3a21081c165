"""tests/fr_plan_cases.py without a GPU: the coverage table of the cases (no promised cell empty), the cases' plan model against
halo_dev_fr_plan (host only: the development library loads without a device), the three plan hooks -- defaults, precedence over
the environment, every refused value, the clamp of HALO_DOT_BLOCKS -- the documented switch points of the plan, and the C oracle
against pallas_model's Python integers at the sizes the GPU tests newly lean on (above 4096 elements, lg_n = 17)."""
import os
import subprocess
import sys

import pytest

import fr_plan_cases as fp
import lazy_cases as lz
import orc
import pallas_model as pm

R = pm.R_ORDER
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hal():
    import halo_accumulation_amd as h
    h.build()
    return h


# ------------------------------------------------------------------ 1. the cases
def test_coverage_table_has_no_empty_promised_cell():
    cases = fp.all_cases()
    print("\n" + fp.coverage_table(cases))
    print("%d cases" % len(cases))
    cells = list(fp.coverage(cases))
    empty = [what for what, pred in fp.promised_cells() if not any(pred(c) for c in cells)]
    assert not empty, empty
    assert len(set(cases)) == len(cases), "no case twice"
    assert all(1 <= c.n <= fp.CTX_N for c in cases)
    # the one-hot positions: each list holds the first and the last element, and the first element of a second wave where there is one
    for c in cases:
        if c.kernel in ("powers", "poly_eval"):
            pos = fp.one_hot_positions(c.n, 64 * c.plan.E)
            assert pos[0] == 0 and pos[-1] == c.n - 1 and (c.n <= 64 * c.plan.E or 64 * c.plan.E in pos)
    # every trip case of the dot product with an odd tail has the zeroed slot where its docstring says
    odd = [c for c in fp.dot_cases() if c.blocks_hook and c.n % (256 * c.blocks_hook) == 33]
    assert len(odd) == 4 * len(fp.BLOCK_HOOKS) and {c.plan.trips for c in odd} == {1, 2, 3, 4}


def test_fr_words_equals_fr_mont():
    for n in (1, 2, 5, 64, 257):
        for k, v in lz.fr_extreme_vectors(n).items():
            assert fp.fr_words(v).tolist() == lz.fr_mont(v).tolist(), (n, k)
    c, w = fp.one_hot(300, 299, 3)
    assert lz.fr_ints(w) == [0] * 299 + [c] and 0 < c < R


# ------------------------------------------------------------------ 2. the plan: model, hooks, switch points
def plan(hal, which, n):
    p = hal._lib.fr_plan(fp.PLAN_OF[which], n)
    return fp.Plan(p["E"], p["nwin"], p["blocks"], p["trips"])


def set_hooks(hal, kernel, pow_e, blocks_hook):
    hal._lib.dev_hook("reset", 0)
    if pow_e:
        hal._lib.dev_hook("pow_e", pow_e)
    if blocks_hook:
        hal._lib.dev_hook("dot_blocks" if fp.PLAN_OF[kernel] == "dot" else "poly_blocks", blocks_hook)


def test_the_model_of_the_cases_is_the_plan_of_the_library(hal):
    for c in fp.all_cases():
        set_hooks(hal, c.kernel, c.pow_e, c.blocks_hook)
        assert plan(hal, c.kernel, c.n) == c.plan, c
    hal._lib.dev_hook("reset", 0)
    for kernel in ("powers", "poly_eval", "dot", "h_coeffs"):
        for lg in range(0, 25):
            for n in {max(1, (1 << lg) - 1), 1 << lg, (1 << lg) + 1}:
                if kernel != "h_coeffs" or n == 1 << lg:
                    assert plan(hal, kernel, n) == fp.model_plan(kernel, n), (kernel, n)


def test_documented_switch_points(hal):
    """A tuning change must update these knowingly (csrc/fr_plan.hpp; DESIGN.md: the chain lengths measured at 2^20)."""
    hal._lib.dev_hook("reset", 0)
    for kernel in ("powers", "poly_eval", "h_coeffs"):
        for n in (1, 4096, 1 << 17, 1 << 18):
            assert plan(hal, kernel, n).E == 4, (kernel, n)
    assert plan(hal, "powers", (1 << 19) - 1).E == 4 and plan(hal, "poly_eval", (1 << 19) - 1).E == 4
    assert plan(hal, "powers", 1 << 19).E == 8 and plan(hal, "poly_eval", 1 << 19).E == 8
    assert plan(hal, "powers", 1 << 20).E == 8 and plan(hal, "poly_eval", (1 << 20) - 1).E == 8
    assert plan(hal, "poly_eval", 1 << 20) == fp.Plan(16, 5, 256, 1)
    assert plan(hal, "powers", 1 << 20) == fp.Plan(8, 5, 512, 1)
    assert plan(hal, "h_coeffs", 1 << 20) == fp.Plan(4, 3, 1024, 1) and plan(hal, "h_coeffs", 1 << 24).E == 4
    assert [plan(hal, "powers", n).nwin for n in (1, 16, 17, 256, 257, 4096, 4097, 65536, 65537, 1 << 20, (1 << 20) + 1)] == [1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6]
    assert [plan(hal, "h_coeffs", 1 << lg).nwin for lg in (0, 1, 8, 9, 16, 17, 24)] == [0, 1, 1, 2, 2, 3, 3]
    # the grid caps: a second trip of p(z) from 2^18 E coefficients on, of the dot product from 2^18 elements on
    assert plan(hal, "poly_eval", 1 << 24) == fp.Plan(16, 6, 1024, 4) and plan(hal, "poly_eval", (1 << 22) + 1).trips == 2
    assert plan(hal, "dot", 1 << 18) == fp.Plan(2, 0, 512, 1) and plan(hal, "dot", (1 << 18) + 1).trips == 2
    assert plan(hal, "dot", 1 << 20) == fp.Plan(2, 0, 512, 4) and plan(hal, "dot", 1) == fp.Plan(2, 0, 1, 1)


def test_hooks_defaults_refusals_and_reset(hal):
    lib = hal.load()
    lib.halo_dev_hook(b"reset", 0)
    base = {k: plan(hal, k, 5000) for k in ("powers", "poly_eval", "dot", "h_coeffs")}
    assert base == {"powers": fp.Plan(4, 4, 5, 1), "poly_eval": fp.Plan(4, 4, 5, 1), "dot": fp.Plan(2, 0, 10, 1), "h_coeffs": fp.Plan(4, 2, 5, 1)}
    for e in (4, 8, 16, 32, 64):
        assert lib.halo_dev_hook(b"pow_e", e) == 0
        assert [plan(hal, k, 5000).E for k in ("powers", "poly_eval", "h_coeffs")] == [e] * 3 and plan(hal, "dot", 5000) == base["dot"]
    for name, bad, rule in ((b"pow_e", (0, 1, 2, 3, 5, 12, 48, 65, 128, -4), b"pow_e must be a power of two in [4, 64]"),
                            (b"dot_blocks", (0, -1, 1025, 1 << 20), b"dot_blocks must be in [1, 1024]"),
                            (b"poly_blocks", (0, -1, 1025, 1 << 20), b"poly_blocks must be in [1, 1024]")):
        for v in bad:
            assert lib.halo_dev_hook(name, v) == hal._lib.HALO_E_ARG, (name, v)
            assert rule in lib.halo_last_error(), (name, v)
    assert plan(hal, "powers", 5000).E == 64, "a refused value leaves the hook as it was"
    for v in (1, 3, 1024):
        assert lib.halo_dev_hook(b"dot_blocks", v) == 0 and lib.halo_dev_hook(b"poly_blocks", v) == 0
    assert plan(hal, "dot", 1 << 20) == fp.Plan(2, 0, 1024, 2) and plan(hal, "poly_eval", 1 << 24).blocks == 1024
    assert lib.halo_dev_hook(b"dot_blocks", 3) == 0 and lib.halo_dev_hook(b"poly_blocks", 2) == 0 and lib.halo_dev_hook(b"pow_e", 8) == 0
    assert plan(hal, "dot", 5000) == fp.Plan(2, 0, 3, 4) and plan(hal, "poly_eval", 5000) == fp.Plan(8, 4, 2, 2)
    assert lib.halo_dev_hook(b"reset", 0) == 0
    assert {k: plan(hal, k, 5000) for k in base} == base
    # misuse of the query itself
    out = (hal._lib.C.c_long * 4)()
    assert lib.halo_dev_fr_plan(None, 5, 100, out) == hal._lib.HALO_E_ARG and b"which is 0 powers" in lib.halo_last_error()
    assert lib.halo_dev_fr_plan(None, 0, 100, None) == hal._lib.HALO_E_ARG
    assert lib.halo_dev_dot2_cross(None, None, None, 1, None) == hal._lib.HALO_E_ARG and b"null context" in lib.halo_last_error()


def test_the_batched_open_has_its_own_grid_limit(hal):
    """open_batch_table / open_batch_eval: the single open's plan up to the 256 partial records of a member, the hook below that"""
    fr_plan = hal._lib.fr_plan
    hal._lib.dev_hook("reset", 0)
    for n in (1, 4096, 65536, 1 << 20):
        assert fr_plan("poly_eval_batch", n) == fr_plan("poly_eval", n), n
    assert fr_plan("poly_eval", 1 << 22) == {"E": 16, "nwin": 6, "blocks": 1024, "trips": 1}
    assert fr_plan("poly_eval_batch", 1 << 22) == {"E": 16, "nwin": 6, "blocks": 256, "trips": 4}
    hal._lib.dev_hook("poly_blocks", 300)
    assert fr_plan("poly_eval", 1 << 22)["blocks"] == 300 and fr_plan("poly_eval_batch", 1 << 22)["blocks"] == 256
    hal._lib.dev_hook("poly_blocks", 5)
    hal._lib.dev_hook("pow_e", 8)
    assert fr_plan("poly_eval_batch", 5000) == fr_plan("poly_eval", 5000) == {"E": 8, "nwin": 4, "blocks": 3, "trips": 1}
    assert fr_plan("poly_eval_batch", 1 << 16) == {"E": 8, "nwin": 4, "blocks": 5, "trips": 7}
    hal._lib.dev_hook("reset", 0)


CHILD = ("import sys; sys.path.insert(0, %r); import halo_accumulation_amd as h; from halo_accumulation_amd._lib import fr_plan, dev_hook\n"
         "l = h.load()\n"
         "def show(tag): print(tag, l.halo_dev_tuning(b'pow_e'), l.halo_dev_tuning(b'dot_blocks'), "
         "fr_plan('powers', 5000)['E'], fr_plan('h_coeffs', 4096)['E'], fr_plan('dot', 1 << 20)['blocks'], fr_plan('poly_eval', 1 << 24)['blocks'])\n"
         "show('env')\n"
         "dev_hook('pow_e', 16); dev_hook('dot_blocks', 3); dev_hook('poly_blocks', 5); show('hook')\n"
         "dev_hook('reset', 0); show('reset')\n" % ROOT)


def run_child(env):
    e = {k: v for k, v in os.environ.items() if not k.startswith("HALO_")}
    e.update(env)
    out = subprocess.run([sys.executable, "-c", CHILD], env=e, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-500:]
    return {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in out.stdout.splitlines()}, out.stderr


def test_hook_before_environment_before_default(hal):
    got, err = run_child({})
    assert got == {"env": [0, 0, 4, 4, 512, 1024], "hook": [0, 0, 16, 16, 3, 5], "reset": [0, 0, 4, 4, 512, 1024]} and "HALO_" not in err
    got, err = run_child({"HALO_POW_E": "8", "HALO_DOT_BLOCKS": "7"})
    assert got == {"env": [8, 7, 8, 8, 7, 1024], "hook": [8, 7, 16, 16, 3, 5], "reset": [8, 7, 8, 8, 7, 1024]} and "HALO_" not in err


def test_dot_blocks_from_the_environment_is_clamped_with_a_note(hal):
    got, err = run_child({"HALO_DOT_BLOCKS": "2000"})
    assert got["env"] == [0, 1024, 4, 4, 1024, 1024] and got["hook"][4] == 3
    assert "HALO_DOT_BLOCKS=2000 clamped to 1024: the block cap must be in [1, 1024]" in err
    got, err = run_child({"HALO_DOT_BLOCKS": "-5"})
    assert got["env"][1] == 1 and got["env"][4] == 1 and "HALO_DOT_BLOCKS=-5 clamped to 1" in err


# ------------------------------------------------------------------ 3. the oracle above 4096 elements
CPU_EDGES = [n for n in fp.WINDOW_EDGES if n <= 65537]


@pytest.fixture(scope="module")
def zs():
    return {k: (z, lz.fr_mont([z])[0]) for k, z in fp.Z_SCALARS.items()}


def test_oracle_powers_up_to_65537(zs):
    top = max(CPU_EDGES)
    for k, (z, zw) in zs.items():
        whole = orc.powers(zw, top)
        assert lz.fr_ints(whole) == pm.construct_powers(z, top), k
        for n in CPU_EDGES:
            assert orc.powers(zw, n).tolist() == whole[:n].tolist(), (k, n)


@pytest.mark.parametrize("n", CPU_EDGES)
def test_oracle_poly_eval_and_dot_at_window_edges(zs, n):
    vecs = fp.dense_vectors(n)
    other = fp.random_ints(n, 5)
    ow = fp.fr_words(other)
    for k, (v, w) in vecs.items():
        assert lz.fr_ints(orc.scalar_dot(w, ow)) == [pm.scalar_dot(v, other)], k
        for kz, (z, zw) in zs.items():
            assert lz.fr_ints(orc.poly_eval(w, zw)) == [pm.poly_eval(v, z)], (k, kz)


@pytest.mark.parametrize("n", CPU_EDGES)
def test_oracle_one_hot(zs, n):
    """p(z) = c z^p and <x, y> = x_p y_p: the identities the GPU tests use beside the oracle"""
    other = fp.random_ints(n, 6)
    ow = fp.fr_words(other)
    for p in fp.one_hot_positions(n, 256):
        c, w = fp.one_hot(n, p, 1)
        assert lz.fr_ints(orc.scalar_dot(w, ow)) == [c * other[p] % R], p
        assert lz.fr_ints(orc.scalar_dot(ow, w)) == [c * other[p] % R], p
        for kz, (z, zw) in zs.items():
            assert lz.fr_ints(orc.poly_eval(w, zw)) == [c * pow(z, p, R) % R], (p, kz)


@pytest.mark.parametrize("which", ["random a", "all r-1"])
def test_oracle_h_coeffs_lg_17(which):
    xis = fp.h_challenges(17)[which]
    xw = lz.fr_mont(xis)
    assert lz.fr_ints(orc.h_coeffs(xw)) == pm.h_coeffs(xis)
    for z in (0, 1, R - 1, 2, fp.Z_SCALARS["random a"]):
        assert lz.fr_ints(orc.h_eval(xw, lz.fr_mont([z])[0])) == [pm.h_eval(xis, z)], z
