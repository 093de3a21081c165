"""The C restatement (oracle/halo_cpu.c, `orc`) is what the GPU tests trust bit for bit.  tests/test_gpu_lazy_bounds.py leans
on it at extreme scalar data -- vectors of r - 1, of zeros, evaluation points 0, 1, r - 1 -- where nothing had compared it with
anything: here it is held against pallas_model's Python integers on those very vectors (lazy_cases.fr_extreme_vectors)."""
import random

import numpy as np
import pytest

import lazy_cases as lz
import orc
import pallas_model as pm


@pytest.mark.parametrize("m", lz.FR_LENGTHS)
def test_scalar_dot_powers_poly_eval(m):
    vecs = lz.fr_extreme_vectors(m)
    words = {k: lz.fr_mont(v) for k, v in vecs.items()}
    for ka, a in vecs.items():
        for kb, b in vecs.items():
            assert lz.fr_ints(orc.scalar_dot(words[ka], words[kb])) == [pm.scalar_dot(a, b)], (ka, kb)
    for z in lz.FR_SCALARS + [vecs["random, extremes planted"][m // 2]]:
        zw = lz.fr_mont([z])[0]
        assert lz.fr_ints(orc.powers(zw, m)) == pm.construct_powers(z, m), z
        for k, a in vecs.items():
            assert lz.fr_ints(orc.poly_eval(words[k], zw)) == [pm.poly_eval(a, z)], (k, z)


@pytest.mark.parametrize("lg_n", [1, 2, 3, 6, 7, 8, 9, 10, 12])  # (every size a GPU test leans on: lazy_cases users)
def test_h_coeffs_h_eval(lg_n):
    for k, xis in lz.fr_extreme_vectors(lg_n + 1).items():
        xw = lz.fr_mont(xis)
        assert lz.fr_ints(orc.h_coeffs(xw)) == pm.h_coeffs(xis), k
        for z in lz.FR_SCALARS:
            assert lz.fr_ints(orc.h_eval(xw, lz.fr_mont([z])[0])) == [pm.h_eval(xis, z)], (k, z)


@pytest.mark.parametrize("n", [2, 8, 64, 128, 1024])
def test_fold_of_c_and_z(n):
    """pcdl.rs:221-227 on the scalar vectors: c' = c_l + xi^-1 c_r, z' = z_l + xi z_r (the points are all at infinity here)"""
    vecs = lz.fr_fold_vectors(n)
    m = n // 2
    for xi in [1, pm.R_ORDER - 1, 2, random.Random(n).randrange(3, pm.R_ORDER - 1)]:
        xi_inv = pm.inv_mod(xi, pm.R_ORDER)
        for kc, c in vecs.items():
            kz = "all r-1" if kc != "all r-1" else "random, extremes planted"
            z = vecs[kz]
            gj, cs, zs = np.zeros((n, 12), dtype=np.uint64), lz.fr_mont(c), lz.fr_mont(z)
            orc.lib().orc_ipa_round_fold(orc.ptr(gj), orc.ptr(cs), orc.ptr(zs), orc.C.c_size_t(m), orc.ptr(lz.fr_mont([xi])[0]),
                                         orc.ptr(lz.fr_mont([xi_inv])[0]))
            assert lz.fr_ints(cs[:m]) == [(c[j] + xi_inv * c[m + j]) % pm.R_ORDER for j in range(m)], (kc, xi)
            assert lz.fr_ints(zs[:m]) == [(z[j] + xi * z[m + j]) % pm.R_ORDER for j in range(m)], (kz, xi)
