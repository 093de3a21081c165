// The lazy fields (fq29.hpp, fr29.hpp) and the group law (curve.hpp) one operation at a time over RAW native operands: the
// caller chooses the limbs, so an operand can sit anywhere below its declared bound K*p -- at k*p, at k*p +- 1, at a power of
// two, with a Y stored as 8p - y -- where the C ABI hooks only ever produce what fq_from_words gives (< 2p).
//
// Not part of the product: included by dev.hip (libhalo_hip_dev.so, halo_test_lazy_field_op / halo_test_lazy_point_op) and by
// tests/native/lazy_field_host.cpp, which compiles the same headers for the CPU under ASan + UBSan.  One table, two
// compilers: the device result of a case must equal the host result limb for limb.
//
// The instantiations are the largest-bound ones the product uses; tests/lazy_cases.py holds the same table (operation number,
// operand bounds, result bound) with the call site of each row, and builds the operands.
//
// Memory forms.  A field element is 10 words (9 limbs + pad, as fq_store_native writes them), a field case is 4 operand
// slots in and one slot out (a predicate writes 0 / 1 into limb 0; 8 x 32-bit word forms use words 0..7 of a slot).  A point
// case is two operands of 40 words in and 40 words out: XYZZ as xyzz_load reads it, Jacobian as x | y | z, affine as
// aff_load reads it (x at word 0, y at word 10).
#pragma once
#include "curve.hpp"
#include "fr29.hpp"

namespace halo {

constexpr int LAZY_SLOT = 10;        // words per field operand
constexpr int LAZY_FIELD_IN = 40;    // four operand slots
constexpr int LAZY_POINT_WORDS = 40; // words per point operand and per point result

template <int K>
HALO_DEV Fq<K> lz_q(const uint32_t *in, int slot) {
    Fq<K> r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.v[i] = in[LAZY_SLOT * slot + i];
    return r;
}
template <int K>
HALO_DEV Fs<K> lz_s(const uint32_t *in, int slot) {
    Fs<K> r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.v[i] = in[LAZY_SLOT * slot + i];
    return r;
}
HALO_DEV Fe lz_fe(const uint32_t *in, int slot) {
    Fe r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = in[LAZY_SLOT * slot + i];
    return r;
}
template <class T>
HALO_DEV void lz_put(uint32_t *o, const T &a) {
#pragma unroll
    for (int i = 0; i < 9; i++) o[i] = a.v[i];
    o[9] = 0;
}
HALO_DEV void lz_put_fe(uint32_t *o, const Fe &a) {
#pragma unroll
    for (int i = 0; i < 8; i++) o[i] = a.v[i];
    o[8] = 0; o[9] = 0;
}
HALO_DEV void lz_put_flag(uint32_t *o, bool f) {
#pragma unroll
    for (int i = 0; i < 10; i++) o[i] = 0;
    o[0] = f ? 1u : 0u;
}

// returns false for an unknown operation number (nothing is written)
HALO_DEV bool lazy_field_op(int op, const uint32_t *in, uint32_t *out) {
    switch (op) {
        // ---- Fq products
        case 0: lz_put(out, fq_mul(lz_q<10>(in, 0), lz_q<10>(in, 1))); break;
        case 1: lz_put(out, fq_mul(lz_q<10>(in, 0), lz_q<8>(in, 1))); break;
        case 2: lz_put(out, fq_mul(lz_q<8>(in, 0), lz_q<8>(in, 1))); break;
        case 3: lz_put(out, fq_mul(lz_q<6>(in, 0), lz_q<10>(in, 1))); break;
        case 4: lz_put(out, fq_mul(lz_q<60>(in, 0), lz_q<1>(in, 1))); break;
        case 5: lz_put(out, fq_sqr(lz_q<10>(in, 0))); break;
        case 6: lz_put(out, fq_sqr(lz_q<8>(in, 0))); break;
        case 7: lz_put(out, fq_mul_add_mul(lz_q<10>(in, 0), lz_q<10>(in, 1), lz_q<8>(in, 2), lz_q<2>(in, 3))); break;
        case 8: lz_put(out, fq_mul_add_mul(lz_q<10>(in, 0), lz_q<4>(in, 1), lz_q<8>(in, 2), lz_q<2>(in, 3))); break;
        case 9: lz_put(out, fq_mul_add_mul(lz_q<4>(in, 0), lz_q<10>(in, 1), lz_q<2>(in, 2), lz_q<2>(in, 3))); break;
        // ---- Fq linear operations
        case 10: lz_put(out, fq_add(lz_q<2>(in, 0), lz_q<2>(in, 1))); break;
        case 11: lz_put(out, fq_sub<8>(lz_q<2>(in, 0), lz_q<8>(in, 1))); break;
        case 12: lz_put(out, fq_sub<16>(lz_q<2>(in, 0), lz_q<16>(in, 1))); break;
        case 13: lz_put(out, fq_sub<2>(lz_q<8>(in, 0), lz_q<2>(in, 1))); break;
        case 14: lz_put(out, fq_sub<2>(lz_q<2>(in, 0), lz_q<2>(in, 1))); break;
        case 15: lz_put(out, fq_sub_sub2(lz_q<2>(in, 0), lz_q<2>(in, 1), lz_q<2>(in, 2))); break;
        case 16: lz_put(out, fq_sub_sub2(lz_q<8>(in, 0), lz_q<2>(in, 1), lz_q<2>(in, 2))); break;
        case 17: lz_put(out, fq_muls<8>(lz_q<2>(in, 0))); break;
        case 18: lz_put(out, fq_muls<2>(lz_q<8>(in, 0))); break;
        case 19: lz_put(out, fq_muls<4>(lz_q<2>(in, 0))); break;
        case 20: lz_put(out, fq_muls<3>(lz_q<2>(in, 0))); break;
        case 21: lz_put(out, fq_neg<8>(lz_q<8>(in, 0))); break;
        case 22: lz_put(out, fq_neg<2>(lz_q<2>(in, 0))); break;
        // ---- Fq reductions and predicates
        case 23: lz_put(out, fq_tighten(lz_q<18>(in, 0))); break;
        case 24: lz_put(out, fq_tighten(lz_q<16>(in, 0))); break;
        case 25: lz_put(out, fq_tighten(lz_q<14>(in, 0))); break;
        case 26: lz_put(out, fq_tighten(lz_q<60>(in, 0))); break;
        case 27: lz_put(out, fq_canonical(lz_q<2>(in, 0))); break;
        case 28: lz_put(out, fq_canonical(lz_q<60>(in, 0))); break;
        case 29: lz_put_flag(out, fq_is_zero_modp(lz_q<10>(in, 0))); break;
        case 30: lz_put_flag(out, fq_is_zero_modp(lz_q<4>(in, 0))); break;
        case 31: lz_put_flag(out, fq_eq_modp(lz_q<2>(in, 0), lz_q<2>(in, 1))); break;
        case 32: lz_put(out, fq_inv(lz_q<4>(in, 0))); break;
        case 33: lz_put(out, fq_from_words(lz_fe(in, 0))); break;
        case 34: lz_put_fe(out, fq_to_words(lz_q<8>(in, 0))); break;
        case 35: lz_put_fe(out, fq_to_words(lz_q<60>(in, 0))); break;
        // ---- Fr
        case 40: lz_put(out, fs_mul(lz_s<4>(in, 0), lz_s<4>(in, 1))); break;
        case 41: lz_put(out, fs_mul(lz_s<10>(in, 0), lz_s<10>(in, 1))); break;
        case 42: lz_put(out, fs_mul_add_mul(lz_s<4>(in, 0), lz_s<4>(in, 1), lz_s<4>(in, 2), lz_s<4>(in, 3))); break;
        case 43: lz_put(out, fs_add(lz_s<4>(in, 0), lz_s<2>(in, 1))); break;
        case 44: lz_put(out, fs_add(lz_s<2>(in, 0), lz_s<4>(in, 1))); break;
        case 45: lz_put(out, fs_tighten(lz_s<6>(in, 0))); break;
        case 46: lz_put(out, fs_tighten(lz_s<60>(in, 0))); break;
        case 47: lz_put(out, fs_from_fe(lz_fe(in, 0))); break;
        case 48: lz_put_fe(out, fs_to_fe(lz_s<6>(in, 0))); break;
        case 49: lz_put_fe(out, fs_to_fe(lz_s<60>(in, 0))); break;
        case 50: lz_put_fe(out, fs_to_fe(lz_s<2>(in, 0))); break;
        case 51: lz_put_fe(out, fs_to_fe(lz_s<1>(in, 0))); break;
        case 52: lz_put(out, fs_below_2r(lz_s<6>(in, 0))); break;
        case 53: lz_put(out, fs_below_2r(lz_s<2>(in, 0))); break;
        case 54: lz_put(out, fs_below_2r(lz_s<1>(in, 0))); break;
        default: return false;
    }
    return true;
}

// ------------------------------------------------------------------------------ points
HALO_DEV JacN lz_jac(const uint32_t *o) {
    JacN p;
    p.x = lz_q<8>(o, 0); p.y = lz_q<8>(o, 1); p.z = lz_q<4>(o, 2);
    return p;
}
HALO_DEV void lz_put_zero(uint32_t *o, int from) {
    for (int i = from; i < LAZY_POINT_WORDS; i++) o[i] = 0;
}
HALO_DEV void lz_put_jac(uint32_t *o, const JacN &p) {
    lz_put(o, p.x); lz_put(o + 10, p.y); lz_put(o + 20, p.z); lz_put_zero(o, 30);
}
HALO_DEV void lz_put_aff(uint32_t *o, const AffN &a) {
    lz_put(o, a.x); lz_put(o + 10, a.y);
}
enum LazyPointOp {
    LZP_XYZZ_ADD = 0, LZP_XYZZ_MADD = 1, LZP_XYZZ_DBL = 2, LZP_JAC_MADD = 3, LZP_JAC_DBL = 4, LZP_JAC_TO_AFF = 5,
    LZP_XYZZ_TO_JAC = 6, LZP_JAC_TO_XYZZ = 7, LZP_JAC_BATCH_TO_AFF = 8, LZP_AFF_FROM_WORDS = 9, LZP_JAC_FROM_WORDS = 10,
    LZP_JAC_STORE_WORDS = 11, LZP_XYZZ_STORE_JAC_WORDS = 12, LZP_AFF_STORE = 13, LZP_AFF_LOAD_SIGNED = 14, LZP_AFF_CNEG = 15,
    LZP_COUNT = 16
};

// a, b, out: 16-byte aligned (aff_load and aff_store move 16 bytes at a time)
HALO_DEV bool lazy_point_op(int op, const uint32_t *a, const uint32_t *b, uint32_t *out) {
    switch (op) {
        case LZP_XYZZ_ADD: { XyzzN x = xyzz_load(a); xyzz_add(x, xyzz_load(b)); xyzz_store(out, x); break; }
        case LZP_XYZZ_MADD: { XyzzN x = xyzz_load(a); xyzz_madd(x, aff_load(b)); xyzz_store(out, x); break; }
        case LZP_XYZZ_DBL: xyzz_store(out, xyzz_dbl(xyzz_load(a))); break;
        case LZP_JAC_MADD: lz_put_jac(out, jac_madd(lz_jac(a), aff_load(b))); break;
        case LZP_JAC_DBL: lz_put_jac(out, jac_dbl(lz_jac(a))); break;
        case LZP_JAC_TO_AFF: lz_put_aff(out, jac_to_aff(lz_jac(a))); lz_put_zero(out, 20); break;
        case LZP_XYZZ_TO_JAC: lz_put_jac(out, xyzz_to_jac(xyzz_load(a))); break;
        case LZP_JAC_TO_XYZZ: xyzz_store(out, jac_to_xyzz(lz_jac(a))); break;
        case LZP_JAC_BATCH_TO_AFF: {  // two points, one inversion: a -> words 0..19, b -> words 20..39
            JacN p[2];
            AffN r[2];
            p[0] = lz_jac(a); p[1] = lz_jac(b);
            jac_batch_to_aff(p, r);
            lz_put_aff(out, r[0]); lz_put_aff(out + 20, r[1]);
            break;
        }
        // the 64-bit word forms are read and written in place: operands and results are 16-byte aligned, little-endian words
        case LZP_AFF_FROM_WORDS: {  // a: 8 x 64-bit arkworks words -> native (words 0..19), and back to words (20..35)
            AffN p = aff_from_words(reinterpret_cast<const uint64_t *>(a));
            lz_put_aff(out, p);
            aff_to_words(reinterpret_cast<uint64_t *>(out + 20), p);
            lz_put_zero(out, 36);
            break;
        }
        case LZP_JAC_FROM_WORDS: lz_put_jac(out, jac_from_words(reinterpret_cast<const uint64_t *>(a))); break;  // a: 12 words
        case LZP_JAC_STORE_WORDS: jac_store_words(reinterpret_cast<uint64_t *>(out), lz_jac(a)); lz_put_zero(out, 24); break;
        case LZP_XYZZ_STORE_JAC_WORDS: xyzz_store_jac_words(reinterpret_cast<uint64_t *>(out), xyzz_load(a)); lz_put_zero(out, 24); break;
        case LZP_AFF_STORE: aff_store(out, aff_load(a)); lz_put_zero(out, 32); break;  // the 128-byte table line: x | y | -y
        case LZP_AFF_LOAD_SIGNED: lz_put_aff(out, aff_load_signed(a, b[0] != 0)); lz_put_zero(out, 20); break;  // a: such a line
        case LZP_AFF_CNEG: lz_put_aff(out, aff_cneg(aff_load(a), b[0] != 0)); lz_put_zero(out, 20); break;
        default: return false;
    }
    return true;
}

}  // namespace halo
