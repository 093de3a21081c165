"""Cases and big-integer checks for the lazy radix-2^29 fields (csrc/fq29.hpp, fr29.hpp) and the group law on them
(csrc/curve.hpp, curve_quad.hpp), shared by the host build (tests/test_host_sanitizers.py, tests/native/lazy_field_host.cpp)
and the device hooks (tests/test_gpu_lazy_bounds.py, csrc/dev_lazy_ops.hpp).  Not a test module.

A value of type Fq<K> is any integer below K*p with limbs 0..7 below 2^29; the product only stays correct while that holds, and
its own call sites run at up to 116/120 of the Montgomery bound.  The operands built here sit AT those bounds; every vector
comes from a seed, none is committed.

Contract checked for every case (reference: Python integers / pallas_model):
  * the result is congruent to the exact result mod p (Fq) or r (Fr);
  * its value is below the declared bound of the result type (fq_neg: at most -- see NEG_CONTRACT);
  * limbs 0..7 are below 2^29;
  * predicates are true exactly on multiples of the modulus.
A Montgomery product is also compared with the one value the algorithm can give: (S + M p) / 2^261 with M = -S / p mod 2^261
(nine limb-serial steps with m_i = -t_i mod 2^29 determine M uniquely), so a wrong carry that stays congruent still shows.
"""
import os
import random
import re
import subprocess

import numpy as np

import pallas_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, R = pm.P, pm.R_ORDER
M29 = (1 << 29) - 1
RP = 1 << 261  # the lazy fields' Montgomery radix
SLOT, FIELD_IN, POINT_WORDS = 10, 40, 40

# fq_neg<K>(0) is exactly K*p: the result of a negation is "<= K*p", every other Fq<K> is "< K*p" (fq29.hpp says so).  The only
# consumers of a negated operand are the fused products (the other factor is strictly below its bound, so the sum of products
# stays strictly below (KaKb + KcKd) p^2 and the static_assert needs no slack for it) and the sign flip of an affine y.
NEG_CONTRACT = "<="


def limbs_of(v):
    assert 0 <= v < (1 << (232 + 32))
    return [(v >> (29 * i)) & M29 for i in range(8)] + [v >> 232]


def value_of(limbs):
    return sum(int(l) << (29 * i) for i, l in enumerate(limbs[:9]))


def words8_of(v):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def value_of_words8(w):
    return sum(int(x) << (32 * i) for i, x in enumerate(w[:8]))


def mont_exact(s, m):
    """what nine 29-bit Montgomery steps give for the column sum s: (s + M m) / 2^261, M = -s / m mod 2^261"""
    big_m = (-s * pow(m, -1, RP)) % RP
    return (s + big_m * m) >> 261


# ------------------------------------------------------------------------------------------------ field table
# operand kinds: an int K = limbs of a value below K * modulus; "W" = any 256-bit pattern as 8 x 32-bit words
# result kinds: ("limbs", K), ("flag",), ("words",)
# fn(ops, m) -> the exact integer the result must be congruent to (or the truth value of a predicate)
def _mul(o, m): return o[0] * o[1] * pow(RP, -1, m)
def _sqr(o, m): return o[0] * o[0] * pow(RP, -1, m)
def _mam(o, m): return (o[0] * o[1] + o[2] * o[3]) * pow(RP, -1, m)
def _add(o, m): return o[0] + o[1]
def _sub(o, m): return o[0] - o[1]
def _ss2(o, m): return o[0] - o[1] - 2 * o[2]
def _id(o, m): return o[0]
def _neg(o, m): return -o[0]
def _muls(k): return lambda o, m: k * o[0]
def _zero(o, m): return o[0] % m == 0
def _eq(o, m): return (o[0] - o[1]) % m == 0
def _inv(o, m): return RP * RP * pow(o[0], -1, m)
def _from_words(o, m): return o[0] * 32            # x 2^266 / 2^261
def _to_words(o, m): return o[0] * pow(32, -1, m)  # x 2^256 / 2^261


FIELD_TABLE = [
    # op, name, field, operands, result, reference, exact product?, call site of this instantiation
    (0, "fq_mul<10,10>", "q", [10, 10], ("limbs", 2), _mul, True, "curve_quad.hpp jac_madd_quad r3 = {H, r0} * {H, r0}: 100 of 120"),
    (1, "fq_mul<10,8>", "q", [10, 8], ("limbs", 2), _mul, True, "curve_quad.hpp jac_madd_quad r4 = {H, X1} * I"),
    (2, "fq_mul<8,8>", "q", [8, 8], ("limbs", 2), _mul, True, "curve.hpp xyzz_dbl Y * V; curve_quad.hpp xyzz_dbl_quad r2"),
    (3, "fq_mul<6,10>", "q", [6, 10], ("limbs", 2), _mul, True, "curve.hpp xyzz_dbl M * (S - X3)"),
    (4, "fq_mul<60,1>", "q", [60, 1], ("limbs", 2), _mul, True, "fq29.hpp fq_to_words: widened operand times 2^256"),
    (5, "fq_sqr<10>", "q", [10], ("limbs", 2), _sqr, True, "curve.hpp xyzz_madd PP = P^2, jac_madd H^2 and r0^2: 100 of 120"),
    (6, "fq_sqr<8>", "q", [8], ("limbs", 2), _sqr, True, "curve.hpp xyzz_dbl Y^2, X^2 of a bucket accumulator"),
    (7, "fq_mul_add_mul<10,10,8,2>", "q", [10, 10, 8, 2], ("limbs", 2), _mam, True, "curve.hpp xyzz_madd y3 = R (Q - X3) + (8p - Y1) PPP: 116 of 120"),
    (8, "fq_mul_add_mul<10,4,8,2>", "q", [10, 4, 8, 2], ("limbs", 2), _mam, True, "curve.hpp jac_madd r0 (V - X3) + (8p - Y1) J"),
    (9, "fq_mul_add_mul<4,10,2,2>", "q", [4, 10, 2, 2], ("limbs", 2), _mam, True, "curve.hpp xyzz_add y3 = R (Q - X3) + (2p - S1) PPP"),
    (10, "fq_add<2,2>", "q", [2, 2], ("limbs", 4), _add, False, "dev.hip k_test_field29 (the product has no other fq_add)"),
    (11, "fq_sub<8>(2,8)", "q", [2, 8], ("limbs", 10), _sub, False, "curve.hpp xyzz_madd P = U2 - X1, R = S2 - Y1; jac_madd H, r0"),
    (12, "fq_sub<16>(2,16)", "q", [2, 16], ("limbs", 18), _sub, False, "curve.hpp jac_dbl X3 = F - 2D"),
    (13, "fq_sub<2>(8,2)", "q", [8, 2], ("limbs", 10), _sub, False, "curve.hpp jac_dbl D - X3"),
    (14, "fq_sub<2>(2,2)", "q", [2, 2], ("limbs", 4), _sub, False, "curve.hpp xyzz_add P = U2 - U1; fq_eq_modp"),
    (15, "fq_sub_sub2<2,2,2>", "q", [2, 2, 2], ("limbs", 8), _ss2, False, "curve.hpp xyzz_madd / xyzz_add X3 = R^2 - PPP - 2Q"),
    (16, "fq_sub_sub2<8,2,2>", "q", [8, 2, 2], ("limbs", 14), _ss2, False, "curve.hpp jac_madd X3 = 4 r0^2 - J - 2V"),
    (17, "fq_muls<8>(2)", "q", [2], ("limbs", 16), _muls(8), False, "curve.hpp jac_dbl 8C"),
    (18, "fq_muls<2>(8)", "q", [8], ("limbs", 16), _muls(2), False, "curve.hpp jac_dbl 2D"),
    (19, "fq_muls<4>(2)", "q", [2], ("limbs", 8), _muls(4), False, "curve.hpp xyzz_dbl V = 4Y^2, jac_madd I = 4H^2"),
    (20, "fq_muls<3>(2)", "q", [2], ("limbs", 6), _muls(3), False, "curve.hpp xyzz_dbl M = 3X^2, jac_dbl E"),
    (21, "fq_neg<8>(8)", "q", [8], ("neg", 8), _neg, False, "curve.hpp xyzz_madd / jac_madd 8p - Y1"),
    (22, "fq_neg<2>(2)", "q", [2], ("neg", 2), _neg, False, "curve.hpp xyzz_add 2p - S1, aff_cneg, aff_store; key_fold.hip signed digits"),
    (23, "fq_tighten<18>", "q", [18], ("limbs", 2), _id, False, "curve.hpp jac_dbl X3 = tighten(F - 2D + 16p)"),
    (24, "fq_tighten<16>", "q", [16], ("limbs", 2), _id, False, "curve.hpp jac_dbl tighten(8C)"),
    (25, "fq_tighten<14>", "q", [14], ("limbs", 2), _id, False, "curve.hpp jac_madd X3"),
    (26, "fq_tighten<60>", "q", [60], ("limbs", 2), _id, False, "fq29.hpp: the largest bound the static_assert admits"),
    (27, "fq_canonical<2>", "q", [2], ("limbs", 1), _id, False, "fq29.hpp fq_to_words; foldtab.hip canonical table coordinates"),
    (28, "fq_canonical<60>", "q", [60], ("limbs", 1), _id, False, "fq29.hpp: the largest bound the static_assert admits"),
    (29, "fq_is_zero_modp<10>", "q", [10], ("flag",), _zero, False, "curve.hpp xyzz_madd / jac_madd P = +-Q tests"),
    (30, "fq_is_zero_modp<4>", "q", [4], ("flag",), _zero, False, "curve.hpp xyzz_add, curve_quad.hpp xyzz_add_quad"),
    (31, "fq_eq_modp<2,2>", "q", [2, 2], ("flag",), _eq, False, "dev.hip aff_same"),
    (32, "fq_inv<4>", "q", [4], ("limbs", 2), _inv, False, "curve.hpp jac_to_aff 1/Z; key_fold.hip 1/(Za Zb)"),
    (33, "fq_from_words", "q", ["W"], ("limbs", 2), _from_words, False, "curve.hpp aff_from_words / jac_from_words (any 256-bit pattern is < 4p)"),
    (34, "fq_to_words<8>", "q", [8], ("words",), _to_words, False, "curve.hpp jac_store_words X, Y"),
    (35, "fq_to_words<60>", "q", [60], ("words",), _to_words, False, "fq29.hpp: the largest bound the static_assert admits"),
    (40, "fs_mul<4,4>", "s", [4, 4], ("limbs", 2), _mul, True, "fr_vec.hip folds of c and z, k_axpy; hpoly.hip h(X) tables: loaded element times loaded element"),
    (41, "fs_mul<10,10>", "s", [10, 10], ("limbs", 2), _mul, True, "fr29.hpp: 100 of 120, the headroom the Fq side uses"),
    (42, "fs_mul_add_mul<4,4,4,4>", "s", [4, 4, 4, 4], ("limbs", 2), _mam, True, "fr_vec.hip dot products and p(z): two loaded pairs per reduction"),
    (43, "fs_add<4,2>", "s", [4, 2], ("limbs", 6), _add, False, "fr_vec.hip k_fold_scalars / k_axpy: loaded element + product"),
    (44, "fs_add<2,4>", "s", [2, 4], ("limbs", 6), _add, False, "fr_vec.hip p(z): h + (t0 + t1)"),
    (45, "fs_tighten<6>", "s", [6], ("limbs", 2), _id, False, "fr_vec.hip p(z) h = tighten(h + t0 + t1)"),
    (46, "fs_tighten<60>", "s", [60], ("limbs", 2), _id, False, "fr29.hpp: the largest bound the static_assert admits"),
    (47, "fs_from_fe", "s", ["W"], ("limbs_exact", 4), _id, False, "fr29.hpp fs_load: repacking only, any 256-bit pattern is < 4r"),
    (48, "fs_to_fe<6>", "s", [6], ("words",), _id, False, "fr_vec.hip fs_store(fs_add(loaded, product))"),
    (49, "fs_to_fe<60>", "s", [60], ("words",), _id, False, "fr29.hpp: the largest bound the static_assert admits"),
    (50, "fs_to_fe<2>", "s", [2], ("words",), _id, False, "fr_vec.hip block sums of accumulators"),
    (51, "fs_to_fe<1>", "s", [1], ("words",), _id, False, "fr29.hpp fs_below_2r<1> specialisation"),
    (52, "fs_below_2r<6>", "s", [6], ("limbs", 2), _id, False, "fr29.hpp fs_to_fe"),
    (53, "fs_below_2r<2>", "s", [2], ("limbs", 2), _id, False, "fr29.hpp specialisation: a product's result is returned as it is"),
    (54, "fs_below_2r<1>", "s", [1], ("limbs", 2), _id, False, "fr29.hpp specialisation"),
]
# fused products whose third operand is a negation (fq_neg<Kc>): that slot also takes the value Kc * p itself
NEG_FED_SLOT = {7: 2, 8: 2, 9: 2}


def edge_values(k_bound, m, allow_equal=False):
    """the values the issue lists for an operand below k_bound * m (sorted, unique)"""
    top = k_bound * m
    vals = {0, 1, m - 1, m + 1, top - 1}
    for k in range(k_bound + 1):
        for d in range(-2, 3):
            vals.add(k * m + d)
    q = 0
    while (q << 254) < top + (1 << 254):
        vals.add(q << 254)
        vals.add((q << 254) - 1)
        # limbs 0..7 all 2^29 - 1 under top limbs around this multiple of 2^254
        for j in (0, 1, 1 << 21, (1 << 22) - 1):
            vals.add((((q << 22) + j) << 232) | ((1 << 232) - 1))
        q += 1
    lim = top + 1 if allow_equal else top
    return sorted(v for v in vals if 0 <= v < lim)


def word_patterns(m):
    full = (1 << 256) - 1
    vals = {0, 1, m - 1, m, m + 1, 2 * m, 3 * m, 3 * m + 5, full, full - 1, 1 << 255, (1 << 255) - 1, 1 << 254, (1 << 254) - 1,
            0xFFFFFFFF, 1 << 32, (1 << 232) - 1}
    return sorted(v for v in vals if 0 <= v <= full)


def field_cases(row, rng, n_random=300):
    """-> list of operand tuples (ints)"""
    op, _name, field, kinds, _res, _fn, _exact, _site = row
    m = P if field == "q" else R
    edges, tops = [], []
    for slot, k in enumerate(kinds):
        if k == "W":
            edges.append(word_patterns(m)); tops.append(1 << 256)
        else:
            edges.append(edge_values(k, m, allow_equal=NEG_FED_SLOT.get(op) == slot)); tops.append(k * m)
    cases = []
    if len(kinds) == 1:
        cases += [(v,) for v in edges[0]]
    else:
        # every edge of every slot against: an edge, the largest value and a random value of the other slots
        for slot in range(len(kinds)):
            for v in edges[slot]:
                for mode in range(3):
                    c = []
                    for s2 in range(len(kinds)):
                        if s2 == slot: c.append(v)
                        elif mode == 0: c.append(rng.choice(edges[s2]))
                        elif mode == 1: c.append(edges[s2][-1])
                        else: c.append(rng.randrange(tops[s2]))
                    cases.append(tuple(c))
        if len(kinds) == 2:  # and the cross product of the multiples of the modulus and of 2^254 and their neighbours
            short = [[v for v in e if min(v % m, m - v % m) <= 1 or (v & ((1 << 254) - 1)) in (0, (1 << 254) - 1)] for e in edges]
            cases += [(a, b) for a in short[0][::max(1, len(short[0]) // 40)] for b in short[1][::max(1, len(short[1]) // 40)]]
    for _ in range(n_random):
        cases.append(tuple(rng.randrange(t) for t in tops))
    if op == 32:  # fq_inv: a != 0 mod p
        cases = [c for c in cases if c[0] % m]
    return cases


def encode_field(row, cases):
    kinds = row[3]
    a = np.zeros((len(cases), FIELD_IN), dtype=np.uint32)
    for i, c in enumerate(cases):
        for s, v in enumerate(c):
            a[i, SLOT * s: SLOT * s + (8 if kinds[s] == "W" else 9)] = words8_of(v) if kinds[s] == "W" else limbs_of(v)
    return a


def check_field(row, cases, out, who):
    op, name, field, kinds, res, fn, exact, _site = row
    m = P if field == "q" else R
    assert out.shape == (len(cases), SLOT), (name, out.shape)
    for i, c in enumerate(cases):
        o = [int(x) for x in out[i]]
        where = "%s %s case %d operands %s -> %s" % (who, name, i, [hex(v) for v in c], [hex(x) for x in o])
        want = fn(c, m)
        if res[0] == "flag":
            assert o[0] == (1 if want else 0) and not any(o[1:]), where
            continue
        if res[0] == "words":
            assert o[8] == 0 and o[9] == 0 and value_of_words8(o) == want % m, where  # the canonical representative, exactly
            continue
        v = value_of(o)
        assert all(x <= M29 for x in o[:8]) and o[9] == 0, "limbs not normalised: " + where
        assert (v - want) % m == 0, "not congruent: " + where
        if res[0] == "neg":
            assert v <= res[1] * m and (v < res[1] * m or c[0] == 0), "above the bound: " + where
        else:
            assert v < res[1] * m, "not below %d * modulus: %s" % (res[1], where)
        if res[0] == "limbs_exact":
            assert v == want, where
        if exact:
            s = c[0] * c[0] if len(c) == 1 else c[0] * c[1] + (c[2] * c[3] if len(c) == 4 else 0)
            assert v == mont_exact(s, m), "not the Montgomery quotient: " + where


# ------------------------------------------------------------------------------------------------ running the blocks
def build_host(tmp_dir):
    """compile tests/native/lazy_field_host.cpp with ASan + UBSan -> (exe, None) or (None, reason to skip)"""
    import shutil
    if shutil.which("g++") is None or not os.path.isdir("/opt/rocm/include"):
        return None, "no g++ / HIP headers"
    exe = os.path.join(str(tmp_dir), "lazy_field_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
           "-I/opt/rocm/include", "-I", os.path.join(ROOT, "halo-accumulation_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "lazy_field_host.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "sanitize" in b.stderr:
        return None, "sanitizer runtime not installed"
    assert b.returncode == 0, b.stderr[-2000:]
    return exe, None


class HostRunner:
    """blocks through the sanitizer build: one process per call of run(), any sanitizer report fails"""
    name = "host"

    def __init__(self, exe, tmp_dir):
        self.exe, self.dir, self.calls = exe, str(tmp_dir), 0

    def run(self, blocks):
        """blocks: [(kind, op, a, b or None)] -> [out]"""
        self.calls += 1
        fin, fout = os.path.join(self.dir, "cases_%d.bin" % self.calls), os.path.join(self.dir, "results_%d.bin" % self.calls)
        with open(fin, "wb") as f:
            for kind, op, a, b in blocks:
                np.array([kind, op, a.shape[0]], dtype=np.uint32).tofile(f)
                np.ascontiguousarray(a, dtype=np.uint32).tofile(f)
                if kind == 1:
                    np.ascontiguousarray(b if b is not None else np.zeros_like(a), dtype=np.uint32).tofile(f)
        r = subprocess.run([self.exe, fin, fout], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.startswith("ok ") and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, \
            r.stdout + r.stderr[-3000:]
        flat = np.fromfile(fout, dtype=np.uint32)
        outs, at = [], 0
        for kind, _op, a, _b in blocks:
            w = SLOT if kind == 0 else POINT_WORDS
            outs.append(flat[at: at + a.shape[0] * w].reshape(a.shape[0], w))
            at += a.shape[0] * w
        assert at == flat.size
        os.remove(fin); os.remove(fout)
        return outs


class DeviceRunner:
    """the same blocks through halo_test_lazy_field_op / halo_test_lazy_point_op (quad: the forms of curve_quad.hpp)"""

    def __init__(self, ctx, quad=False):
        self.ctx, self.quad, self.name = ctx, quad, "device quad" if quad else "device"

    def run(self, blocks):
        outs = []
        for kind, op, a, b in blocks:
            if kind == 0:
                outs.append(self.ctx.lazy_field_op(op, a))
            else:
                outs.append(self.ctx.lazy_point_op(op, a, b if b is not None else np.zeros_like(a), quad=self.quad))
        return outs


# ------------------------------------------------------------------------------------------------ group law
(XYZZ_ADD, XYZZ_MADD, XYZZ_DBL, JAC_MADD, JAC_DBL, JAC_TO_AFF, XYZZ_TO_JAC, JAC_TO_XYZZ, JAC_BATCH_TO_AFF, AFF_FROM_WORDS, JAC_FROM_WORDS,
 JAC_STORE_WORDS, XYZZ_STORE_JAC_WORDS, AFF_STORE, AFF_LOAD_SIGNED, AFF_CNEG) = range(16)
POINT_OP_NAMES = ["xyzz_add", "xyzz_madd", "xyzz_dbl", "jac_madd", "jac_dbl", "jac_to_aff", "xyzz_to_jac", "jac_to_xyzz", "jac_batch_to_aff<2>",
                  "aff_from_words/aff_to_words", "jac_from_words", "jac_store_words", "xyzz_store_jac_words", "aff_store", "aff_load_signed", "aff_cneg"]
QUAD_OPS = [XYZZ_ADD, XYZZ_DBL, JAC_MADD, JAC_DBL]
RP_INV = pow(RP, -1, P)


def nat(x):
    return x * RP % P


def fixture_points(kat):
    """affine points of the committed key table (tests/golden/urs_kat.json): S, H, the head of GS and its last entry"""
    pts = [tuple(int(h, 16) for h in kat[k]) for k in ("S", "H")] + [tuple(int(h, 16) for h in g) for g in kat["GS_head"]]
    pts.append(tuple(int(h, 16) for h in kat["GS_16383"]))
    assert all(pm.is_on_curve(p) for p in pts) and len(set(pts)) == len(pts) >= 6
    return pts


def _put(row, at, v):
    row[at: at + 9] = limbs_of(v)


def xyzz_words(pt, i=0, j=0, z=1, dzz=0, dzzz=0, garbage=None):
    """XYZZ representative of an affine point: X = x z^2 + i p, Y = y z^3 + j p, ZZ = z^2 (+ p), ZZZ = z^3 (+ p) in native form;
    None = infinity: ZZ all zero and the other coordinates whatever `garbage` holds"""
    w = np.zeros(POINT_WORDS, dtype=np.uint32)
    if pt is None:
        if garbage:
            _put(w, 0, garbage[0] % (8 * P)); _put(w, 10, garbage[1] % (8 * P)); _put(w, 30, garbage[2] % (2 * P))
        return w
    z2, z3 = z * z % P, z * z * z % P
    zz, zzz = nat(z2) + dzz * P, nat(z3) + dzzz * P
    if zz >= 2 * P: zz -= P
    if zzz >= 2 * P: zzz -= P
    _put(w, 0, nat(pt[0] * z2) + i * P); _put(w, 10, nat(pt[1] * z3) + j * P); _put(w, 20, zz); _put(w, 30, zzz)
    return w


def jac_words(pt, i=0, j=0, z=1, dz=0, garbage=None):
    """Jacobian representative: X = x z^2 + i p, Y = y z^3 + j p (< 8p), Z = z + dz p (< 4p); None = infinity (Z all zero)"""
    w = np.zeros(POINT_WORDS, dtype=np.uint32)
    if pt is None:
        if garbage:
            _put(w, 0, garbage[0] % (8 * P)); _put(w, 10, garbage[1] % (8 * P))
        return w
    _put(w, 0, nat(pt[0] * z * z) + i * P); _put(w, 10, nat(pt[1] * z * z * z) + j * P); _put(w, 20, nat(z) + dz * P)
    return w


def aff_words(pt, i=0, j=0):
    """affine representative x + i p, y + j p where that is < 2p (else the canonical one); None = (0, 0)"""
    w = np.zeros(POINT_WORDS, dtype=np.uint32)
    if pt is None:
        return w
    x, y = nat(pt[0]) + i * P, nat(pt[1]) + j * P
    _put(w, 0, x if x < 2 * P else x - P); _put(w, 10, y if y < 2 * P else y - P)
    return w


def _norm_ok(o, n):
    return all(int(o[10 * c + k]) <= M29 for c in range(n) for k in range(8)) and all(int(o[10 * c + 9]) == 0 for c in range(n))


def decode_xyzz(o, where):
    x, y, zz, zzz = (value_of(o[10 * c: 10 * c + 9]) for c in range(4))
    if not any(int(v) for v in o[20:29]):
        return None
    assert _norm_ok(o, 4), "limbs not normalised: " + where
    assert x < 8 * P and y < 8 * P and zz < 2 * P and zzz < 2 * P, "XYZZ bounds (X, Y < 8p; ZZ, ZZZ < 2p) broken: " + where
    assert zz % P and zzz % P and pow(zz * RP_INV, 3, P) == pow(zzz * RP_INV, 2, P), "ZZ^3 != ZZZ^2: " + where
    return (x * pow(zz, -1, P) % P, y * pow(zzz, -1, P) % P)


def decode_jac(o, where):
    x, y, z = (value_of(o[10 * c: 10 * c + 9]) for c in range(3))
    assert not any(int(v) for v in o[30:40]), where
    if not any(int(v) for v in o[20:29]):
        return None
    assert _norm_ok(o, 3), "limbs not normalised: " + where
    assert x < 8 * P and y < 8 * P and z < 4 * P, "Jacobian bounds (X, Y < 8p; Z < 4p) broken: " + where
    assert z % P, where
    return pm.jacobian_to_affine(x * RP_INV % P, y * RP_INV % P, z * RP_INV % P)


def decode_aff(o, where):
    x, y = value_of(o[0:9]), value_of(o[10:19])
    if not any(int(v) for v in o[0:9]) and not any(int(v) for v in o[10:19]):
        return None
    assert _norm_ok(o, 2), "limbs not normalised: " + where
    assert x < 2 * P and y < 2 * P, "affine bounds (x, y < 2p) broken: " + where
    return (x * RP_INV % P, y * RP_INV % P)


def decode_jac_words(o, where):
    """12 x 64-bit arkworks words (x R, y R, z R with R = 2^256, canonical) as 24 x 32-bit words"""
    x, y, z = (value_of_words8(o[8 * c: 8 * c + 8]) for c in range(3))
    assert x < P and y < P and z < P and not any(int(v) for v in o[24:40]), "not canonical: " + where
    if z == 0:
        assert x == pm.MONT_R % P and y == pm.MONT_R % P, "infinity is (1, 1, 0): " + where
        return None
    ri = pow(pm.MONT_R, -1, P)
    return pm.jacobian_to_affine(x * ri % P, y * ri % P, z * ri % P)


def mont_words(v, n=8):
    return words8_of(v * pm.MONT_R % P)[:n]


class PointCases:
    """the representative matrix: per operation a list of (a words, b words, expected, kind of the result, what it is)"""

    def __init__(self, kat, seed=0x4C415A59):
        self.rng = random.Random(seed)
        self.pts = fixture_points(kat)
        self.zs = [1] + [self.rng.randrange(2, P) for _ in range(3)]
        self.cases = {op: [] for op in range(16)}
        self._build()
        for op in self.cases:  # neighbouring cases (the quads of one wave on the device) are of different kinds
            self.rng.shuffle(self.cases[op])

    def _garbage(self):
        return tuple(self.rng.randrange(1, 8 * P) for _ in range(3)) if self.rng.random() < 0.7 else None

    def _xyzz(self, pt, i=None, j=None, zsel=None):
        r = self.rng
        i = r.randrange(8) if i is None else i
        j = r.randrange(8) if j is None else j
        z = self.zs[r.randrange(4) if zsel is None else zsel]
        return xyzz_words(pt, i, j, z, r.randrange(2), r.randrange(2), self._garbage())

    def _jac(self, pt, i=None, j=None, zsel=None):
        r = self.rng
        i = r.randrange(8) if i is None else i
        j = r.randrange(8) if j is None else j
        z = self.zs[r.randrange(4) if zsel is None else zsel]
        dz = r.randrange(4)
        if nat(z) + dz * P >= 4 * P: dz = 0
        return jac_words(pt, i, j, z, dz, self._garbage())

    def _aff(self, pt, i=None, j=None):
        r = self.rng
        return aff_words(pt, r.randrange(2) if i is None else i, r.randrange(2) if j is None else j)

    def _z_with_u2_above_p(self, pt, jac):
        """z such that the kernel's U2 = (x + p) * ZZ1 is >= p: ZZ1 = z^2 + p as given (XYZZ) or the square of Z = z + 3p (Jacobian)"""
        for _ in range(100000):
            z = self.rng.randrange(2, P)
            zz = mont_exact((nat(z) + 3 * P) ** 2, P) if jac else nat(z * z % P) + P
            if zz < 2 * P and mont_exact((nat(pt[0]) + P) * zz, P) >= P:
                return z
        raise AssertionError("no z found")

    def _pairs(self):
        """(a, b, what): the generic sum, P + P, P + (-P), infinity on either side and on both"""
        pts, out = self.pts, []
        for k in range(len(pts)):
            out.append((pts[k], pts[(k + 1) % len(pts)], "generic"))
            out.append((pts[k], pm.neg(pts[(k + 3) % len(pts)]), "generic"))
        for p in pts[:4]:
            out += [(p, p, "double"), (p, pm.neg(p), "inverse"), (None, p, "inf+P"), (p, None, "P+inf")]
        out.append((None, None, "inf+inf"))
        return out

    def _build(self):
        c, r = self.cases, self.rng
        for pa, pb, what in self._pairs():
            want = pm.add(pa, pb)
            special = what in ("double", "inverse")
            # the full 8 x 8 grid of (x + i p, y + j p) of the accumulator; for P + P and P + (-P) against every representative of
            # the other operand as well (-y as k p - y for k = 1..8 is the same set as (p - y) + j p, j = 0..7)
            for i in range(8):
                for j in range(8):
                    grid_b = [(ib, jb) for ib in range(2) for jb in range(2)] if special else [(None, None)]
                    for ib, jb in grid_b:
                        for zsel in ((0, 1) if special else (None,)):
                            c[XYZZ_MADD].append((self._xyzz(pa, i, j, zsel), self._aff(pb, ib, jb), want, "xyzz", what))
                            c[JAC_MADD].append((self._jac(pa, i, j, zsel), self._aff(pb, ib, jb), want, "jac", what))
                    grid_b = [(ib, jb) for ib in range(8) for jb in range(8)] if special else [(None, None), (7 - i, 7 - j)]
                    for ib, jb in grid_b:
                        c[XYZZ_ADD].append((self._xyzz(pa, i, j), self._xyzz(pb, ib, jb), want, "xyzz", what))
        # U2 = x2 ZZ1 comes out of its product below p in ~97 % of all cases, so P = U2 - X1 + 8p reaches 9p only when it is made
        # to: search a z whose product lands in [p, 2p) (the exact Montgomery quotient says which), then sweep X1 + i p again
        for p in self.pts[:2]:
            for pb, what in ((p, "double"), (pm.neg(p), "inverse")):
                want = pm.add(p, pb)
                zx = self._z_with_u2_above_p(p, jac=False)
                zj = self._z_with_u2_above_p(p, jac=True)
                for i in range(8):
                    for j in range(8):
                        c[XYZZ_MADD].append((xyzz_words(p, i, j, zx, 1, r.randrange(2)), aff_words(pb, 1, r.randrange(2)), want, "xyzz", what))
                        c[JAC_MADD].append((jac_words(p, i, j, zj, 3), aff_words(pb, 1, r.randrange(2)), want, "jac", what))
        zero = np.zeros(POINT_WORDS, dtype=np.uint32)
        for p in self.pts + [None]:
            d = pm.add(p, p)
            for i in range(8):
                for j in range(8):
                    c[XYZZ_DBL].append((self._xyzz(p, i, j), zero, d, "xyzz", "double" if p else "inf"))
                    c[JAC_DBL].append((self._jac(p, i, j), zero, d, "jac", "double" if p else "inf"))
                    c[JAC_TO_AFF].append((self._jac(p, i, j), zero, p, "aff", "convert"))
                    c[XYZZ_TO_JAC].append((self._xyzz(p, i, j), zero, p, "jac", "convert"))
                    c[JAC_TO_XYZZ].append((self._jac(p, i, j), zero, p, "xyzz", "convert"))
                    c[JAC_STORE_WORDS].append((self._jac(p, i, j), zero, p, "jac_words", "convert"))
                    c[XYZZ_STORE_JAC_WORDS].append((self._xyzz(p, i, j), zero, p, "jac_words", "convert"))
                    q = r.choice(self.pts + [None])
                    c[JAC_BATCH_TO_AFF].append((self._jac(p, i, j), self._jac(q), (p, q), "aff2", "convert"))
            # the word forms
            w = np.zeros(POINT_WORDS, dtype=np.uint32)
            if p is not None:
                w[0:8], w[8:16] = mont_words(p[0]), mont_words(p[1])
            c[AFF_FROM_WORDS].append((w, zero, p, "aff+words", "convert"))
            for z in self.zs:
                w = np.zeros(POINT_WORDS, dtype=np.uint32)
                if p is None:
                    w[0:8], w[8:16] = mont_words(r.randrange(P)), mont_words(r.randrange(P))
                else:
                    w[0:8], w[8:16], w[16:24] = mont_words(p[0] * z * z), mont_words(p[1] * z * z * z), mont_words(z)
                c[JAC_FROM_WORDS].append((w, zero, p, "jac", "convert"))
            for i in range(2):
                for j in range(2):
                    a = self._aff(p, i, j)
                    c[AFF_STORE].append((a, zero, p, "line", "convert"))
                    for flag in (0, 1):
                        f = zero.copy(); f[0] = flag
                        c[AFF_CNEG].append((a, f, pm.neg(p) if flag else p, "cneg", "convert"))
                        line = a.copy()  # x | y | a third coordinate that is recognisably not y
                        other = nat(r.randrange(P)) + r.randrange(2) * P
                        _put(line, 20, other % (2 * P))
                        c[AFF_LOAD_SIGNED].append((line, f, None, "signed", "convert"))

    def blocks(self, ops):
        return [(1, op, np.stack([x[0] for x in self.cases[op]]), np.stack([x[1] for x in self.cases[op]])) for op in ops]

    def check(self, op, out, who):
        """-> {kind of case: count}"""
        counts = {}
        for n, (a, b, want, kind, what) in enumerate(self.cases[op]):
            o = out[n]
            where = "%s %s case %d (%s)\n a   %s\n b   %s\n out %s" % (who, POINT_OP_NAMES[op], n, what, a.tolist(), b.tolist(), o.tolist())
            counts[what] = counts.get(what, 0) + 1
            if kind == "xyzz":
                assert decode_xyzz(o, where) == want, "wrong point: " + where
            elif kind == "jac":
                assert decode_jac(o, where) == want, "wrong point: " + where
            elif kind == "aff":
                assert decode_aff(o, where) == want and not any(int(v) for v in o[20:40]), "wrong point: " + where
            elif kind == "aff2":
                assert decode_aff(o[0:20], where) == want[0] and decode_aff(o[20:40], where) == want[1], "wrong point: " + where
            elif kind == "jac_words":
                assert decode_jac_words(o, where) == want, "wrong point: " + where
            elif kind == "aff+words":
                assert decode_aff(o, where) == want and o[20:36].tolist() == a[0:16].tolist() and not any(int(v) for v in o[36:40]), where
            elif kind == "line":
                # the 128-byte table line: x | 0 | y | 0 | -y | 0 0 0; -y = 2p - y limb for limb, (0, 0) for infinity
                assert o[0:20].tolist() == a[0:20].tolist() and not any(int(v) for v in o[29:40]), where
                y, ny = value_of(a[10:19]), value_of(o[20:29])
                assert ny == (2 * P - y if want is not None else 0) and all(int(v) <= M29 for v in o[20:28]), where
            elif kind == "cneg":
                y, ny = value_of(a[10:19]), value_of(o[10:19])
                assert o[0:10].tolist() == a[0:10].tolist() and all(int(v) <= M29 for v in o[10:18]), where
                assert ny == (2 * P - y if (int(b[0]) and want is not None) else y), where
                assert decode_aff(o, where) == want, "wrong point: " + where
            elif kind == "signed":
                src = a[20:30] if int(b[0]) else a[10:20]
                assert o[0:10].tolist() == a[0:10].tolist() and o[10:20].tolist() == src.tolist() and not any(int(v) for v in o[20:40]), where
            else:
                raise AssertionError(kind)
        return counts


def run_chains(runner, kat, op, steps=64, chains=24, seed=0x43484149):
    """`chains` accumulators, `steps` additions each with nothing normalised in between: xyzz_madd (affine addends) or xyzz_add
    (XYZZ addends, Z != 1).  After every step every accumulator is decoded -- X, Y < 8p and ZZ, ZZZ < 2p by value -- and compared
    with the affine running sum.  The walk meets P + P (step 9: the addend is the running sum), P + (-P) (step 19: its negative),
    a restart from infinity (step 20) and an infinite addend (step 29)."""
    assert op in (XYZZ_MADD, XYZZ_ADD)
    rng = random.Random(seed + op)
    pts = fixture_points(kat)
    zs = [rng.randrange(2, P) for _ in range(4)]
    ref = [pts[k % len(pts)] for k in range(chains)]
    acc = np.stack([xyzz_words(ref[k], rng.randrange(8), rng.randrange(8), zs[k % 4] if k % 3 else 1, k & 1, (k >> 1) & 1) for k in range(chains)])
    doubles = cancels = 0
    for s in range(steps):
        addend = []
        for k in range(chains):
            q = pts[(k * 7 + s * (k + 1)) % len(pts)]
            if rng.random() < 0.5: q = pm.neg(q)
            if s % 32 == 9: q = ref[k]
            if s % 32 == 19: q = pm.neg(ref[k])
            if s % 32 == 29: q = None
            addend.append(q)
        if op == XYZZ_MADD:
            b = np.stack([aff_words(q, rng.randrange(2), rng.randrange(2)) for q in addend])
        else:
            b = np.stack([xyzz_words(q, rng.randrange(8), rng.randrange(8), zs[rng.randrange(4)], rng.randrange(2), rng.randrange(2),
                                     (rng.randrange(1, P), rng.randrange(1, P), rng.randrange(1, P))) for q in addend])
        out = runner.run([(1, op, acc, b)])[0]
        for k in range(chains):
            if ref[k] is not None and addend[k] == ref[k]: doubles += 1
            if ref[k] is not None and addend[k] == pm.neg(ref[k]): cancels += 1
            ref[k] = pm.add(ref[k], addend[k])
            where = "%s %s chain %d step %d\n acc %s\n b   %s\n out %s" % (runner.name, POINT_OP_NAMES[op], k, s, acc[k].tolist(), b[k].tolist(), out[k].tolist())
            assert decode_xyzz(out[k], where) == ref[k], "wrong running sum: " + where
        acc = np.ascontiguousarray(out)
    assert doubles >= chains and cancels >= chains
    return dict(chains=chains, steps=steps, doublings=doubles, cancellations=cancels)


def madd_p_multiples(cases, jac=False):
    """for the P + P and P + (-P) cases of xyzz_madd (jac_madd): the multiple k of p that P = U2 - X1 + 8p takes (U2 from the exact
    products: x2 ZZ1, or x2 Z1^2)"""
    ks = set()
    for a, b, _want, _kind, what in cases:
        if what in ("double", "inverse"):
            zz = mont_exact(value_of(a[20:29]) ** 2, P) if jac else value_of(a[20:29])
            u2 = mont_exact(value_of(b[0:9]) * zz, P)
            pd = u2 - value_of(a[0:9]) + 8 * P
            assert pd % P == 0
            ks.add(pd // P)
    return ks


def neg_call_sites():
    """every fq_neg<K>(arg) in the kernels' sources as (file, enclosing function, K, arg): no matter how the line is written"""
    out = []
    d = os.path.join(ROOT, "halo-accumulation_amd", "csrc")
    for f in sorted(os.listdir(d)):
        if f.endswith((".hpp", ".hip")) and f != "dev_lazy_ops.hpp":
            func = None
            for line in open(os.path.join(d, f)):
                code = re.sub(r"__launch_bounds__\([\d, ]+\)", "", line.split("//")[0])
                m = re.match(r"(?:HALO_DEV|__global__|static|template)\b.*?\b(\w+)\(", code)
                if m and not code.startswith("template"):
                    func = m.group(1)
                for k, arg in re.findall(r"\bfq_neg<\s*(\d+)\s*>\(\s*([\w.]+)\s*\)", code):
                    out.append((f, func, int(k), arg))
    return out


# ------------------------------------------------------------------------------------------------ Fr kernels at extreme data
# The lazy sums of the Fr kernels (fs_tighten(fs_add(acc, fs_mul ...))) reach their largest values on these, not on random data
FR_EXTREMES = [R - 1, 0, 1, (R - 1) // 2, (1 << 254) % R]
FR_SCALARS = [0, 1, R - 1, 2]  # z, xi, alpha (0 where the entry point allows it)
FR_LENGTHS = [1, 2, 63, 64, 65, 1000, 4096]
WAVE_EDGES = [63, 64, 65, 127, 128, 255, 256, 257, 1023, 1024]  # last / first lane of a wave, of a block of 256, of 1024


def fr_extreme_vectors(n, seed=0x46524558):
    """name -> n scalars: the constant vectors, the alternating one and a random one with the extremes at both ends and at
    the wave and block boundaries"""
    rng = random.Random(seed + n)
    planted = [rng.randrange(R) for _ in range(n)]
    for k, idx in enumerate([0, n - 1] + [i for i in WAVE_EDGES if i < n]):
        planted[idx] = FR_EXTREMES[k % len(FR_EXTREMES)]
    return {
        "all r-1": [R - 1] * n, "all 0": [0] * n, "all 1": [1] * n, "alternating 0, r-1": [(R - 1) * (i & 1) for i in range(n)],
        "all (r-1)/2": [(R - 1) // 2] * n, "all 2^254 mod r": [(1 << 254) % R] * n, "random, extremes planted": planted,
    }


def fr_fold_vectors(n):
    """fr_extreme_vectors plus two whose halves differ, for the folds v_l + k v_r: a constant vector folds to zero under
    k = r - 1 (and every later round then folds zeros), these stay non-zero under k = 1, r - 1, 2 and 1/2"""
    assert n >= 2 and n % 2 == 0
    h = n // 2
    vecs = fr_extreme_vectors(n)
    vecs["r-1 | (r-1)/2"] = [R - 1] * h + [(R - 1) // 2] * h
    vecs["2^254 mod r | r-1"] = [(1 << 254) % R] * h + [R - 1] * h
    return vecs


SPLIT_VECTORS = ("r-1 | (r-1)/2", "2^254 mod r | r-1")


def fr_mont(xs):
    """ints -> (n, 4) uint64 arkworks words (x 2^256 mod r)"""
    out = np.zeros((len(xs), 4), dtype=np.uint64)
    for i, x in enumerate(xs):
        v = x * pm.MONT_R % R
        out[i] = [(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)]
    return out


_MONT_R_INV = pow(pm.MONT_R, -1, R)


def fr_ints(a):
    a = np.asarray(a, dtype=np.uint64).reshape(-1, 4)
    return [sum(int(w) << (64 * k) for k, w in enumerate(row)) * _MONT_R_INV % R for row in a]
