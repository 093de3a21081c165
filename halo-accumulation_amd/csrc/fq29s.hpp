// Signed companion of fq29.hpp: the same nine 29-bit limbs and the same Montgomery product (R' = 2^261), with limbs and
// 64-bit columns read as two's-complement numbers.
//
// Why.  In fq29.hpp every subtraction adds a multiple of p limb by limb (to stay non-negative) and runs a carry pass (to bring
// the limbs back under 2^29), because the products take unsigned limbs.  With v_mad_i64_i32 a product takes the limb-wise
// difference as it stands, so a subtraction is nine v_sub and nothing else.  The group law has five of them per addition.
//
// Two forms of a value v (fr29.hpp has the names Fs and fs_ for the scalar field) with |v| < K*p:
//   Fqs<K>  signed normalised: limbs 0..7 in [0, 2^29), limb 8 signed and small (|limb 8| <= K 2^22 + 1).  What a product
//          returns, what stays in registers from one addition to the next.  A stored Fq<K> (non-negative) is an Fqs<K> as it is.
//   Fqd<K>  raw difference of two Fqs: limbs 0..7 in (-2^29, 2^29), limb 8 signed and small.  Only ever a product's operand or
//          the argument of a zero test.
// Columns.  Nine partial products of limbs below 2^29 in magnitude are below 9 * 2^58; the five reduction terms m * p_j add at
// most 5 * 2^58, the 2^29 - 1 start and the carries less than 2^34: a column of a product stays below 2^62 in magnitude, a
// column of the two-product fusion (18 + 5 terms) below 2^63.  Both fit int64; compiled for the CPU, the sanitizer's signed
// overflow check tests exactly this (tests/native/signed_field_host.cpp).
// Montgomery step on a signed column t (which started at 2^29 - 1, see fq_mul): m = ~t mod 2^29 is still the non-negative
// multiplier with t + 1 - 2^29 + m = 0 (mod 2^29), and the carry t >> 29 is an arithmetic shift.  The result is
// (a b + M p) / 2^261 with 0 <= M < 2^261: it lies in (-(Ka Kb / 128) p, (Ka Kb / 128 + 1) p), so with Ka Kb <= 120 it is an
// Fqs<2>; a square is never negative and comes out as an Fq<2>.
#pragma once
#include "fq29.hpp"

namespace halo {

template <int K>
struct Fqs {
    int32_t v[9];
};
template <int K>
struct Fqd {
    int32_t v[9];
};

template <int K>
HALO_DEV Fqs<K> fqs_zero() {
    Fqs<K> r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.v[i] = 0;
    return r;
}
// a stored (non-negative) value is a signed normalised one as it stands
template <int Kn, int K>
HALO_DEV Fqs<Kn> fqs_from_fq(const Fq<K> &a) {
    static_assert(K <= Kn, "cannot narrow a value bound");
    static_assert(Kn <= 60, "the top limb must stay below 2^28");
    Fqs<Kn> r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.v[i] = (int32_t)a.v[i];
    return r;
}
template <int Kn, int K>
HALO_DEV Fqs<Kn> fqs_widen(const Fqs<K> &a) {
    static_assert(K <= Kn, "cannot narrow a value bound");
    Fqs<Kn> r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.v[i] = a.v[i];
    return r;
}
// an Fqs is also a raw difference (of itself and zero)
template <int K>
HALO_DEV Fqd<K> fqd_from_fs(const Fqs<K> &a) {
    Fqd<K> r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.v[i] = a.v[i];
    return r;
}
// exact limb test: only where "zero" means all-zero limbs (infinity flags)
template <int K>
HALO_DEV bool fqs_limbs_zero(const Fqs<K> &a) {
    int32_t o = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) o |= a.v[i];
    return o == 0;
}

// ------------------------------------------------------------------ linear operations: nine instructions, no offset, no carry
template <int Ka, int Kb>
HALO_DEV Fqd<Ka + Kb> fqs_sub(const Fqs<Ka> &a, const Fqs<Kb> &b) {
    static_assert(Ka + Kb <= 60, "the top limb must stay below 2^28");
    Fqd<Ka + Kb> r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.v[i] = a.v[i] - b.v[i];
    return r;
}
template <int Ka>
HALO_DEV Fqd<Ka> fqs_neg(const Fqs<Ka> &a) {
    Fqd<Ka> r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.v[i] = -a.v[i];
    return r;
}
// signed carry pass over limb sums |t[i]| < 2^31 - 2^3: limbs 0..7 back into [0, 2^29), the top limb keeps the sign
HALO_DEV void carry_pass_signed(int32_t (&t)[9], int32_t (&out)[9]) {
#pragma unroll
    for (int i = 0; i < 8; i++) {
        int32_t c = t[i] >> 29;  // arithmetic shift: floor
        out[i] = t[i] & (int32_t)M29;
        HALO_PIN_VGPR(out[i]);  // see fqs_reduce
        t[i + 1] += c;
    }
    out[8] = t[8];
}
// a - b - 2c with one carry pass (x3 = R^2 - PPP - 2Q: limbs down to -3 * 2^29, and the value is used three ways)
template <int Ka, int Kb, int Kc>
HALO_DEV Fqs<Ka + Kb + 2 * Kc> fqs_sub_sub2(const Fqs<Ka> &a, const Fqs<Kb> &b, const Fqs<Kc> &c) {
    static_assert(Ka + Kb + 2 * Kc <= 60, "the top limb must stay below 2^28");
    int32_t t[9];
#pragma unroll
    for (int i = 0; i < 9; i++) t[i] = a.v[i] - b.v[i] - 2 * c.v[i];
    Fqs<Ka + Kb + 2 * Kc> r;
    carry_pass_signed(t, r.v);
    return r;
}
// 2a, carried (the doubled limbs would be below 2^30 only: too large for a column of the two-product fusion)
template <int Ka>
HALO_DEV Fqs<2 * Ka> fqs_muls2(const Fqs<Ka> &a) {
    static_assert(2 * Ka <= 60, "the top limb must stay below 2^28");
    int32_t t[9];
#pragma unroll
    for (int i = 0; i < 9; i++) t[i] = 2 * a.v[i];
    Fqs<2 * Ka> r;
    carry_pass_signed(t, r.v);
    return r;
}

// ------------------------------------------------------------------ products
// A column.  On the device it is accumulated in uint64_t: the same bits, but sums the compiler may not take for overflow-free
// and therefore does not split into shorter chains (it did with int64_t: 30 more 64-bit additions per mixed addition).  On the
// CPU it is int64_t, so that the sanitizer sees every sum and checks the 2^63 bound above.
#if defined(__HIP_DEVICE_COMPILE__)
typedef uint64_t fqs_col;
#else
typedef int64_t fqs_col;
#endif
HALO_DEV fqs_col fqs_mad(int32_t a, int32_t b, fqs_col acc) { return (fqs_col)((int64_t)a * (int64_t)b) + acc; }
HALO_DEV fqs_col fqs_sar29(fqs_col t) { return (fqs_col)((int64_t)t >> 29); }  // arithmetic shift: floor
// nine Montgomery steps and the final carry over signed columns c[0..17] whose low nine started at 2^29 - 1
HALO_DEV void fqs_reduce(fqs_col (&c)[18], int32_t (&r)[9]) {
    int32_t p8 = (int32_t)P29::L[8];
    HALO_PIN_VGPR(p8);  // keep m * 2^22 on a multiply-add instead of a 64-bit shift + add (fq_mul)
    fqs_col carry = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        fqs_col t = c[i] + carry;
        int32_t m = (int32_t)((~(uint32_t)t) & M29);
        HALO_PIN_VGPR(m);  // the signed multiply-add here too (same issue cost: profiles/r22_microbench_signed.txt); see below
        c[i + 1] = fqs_mad(m, (int32_t)P29::L[1], c[i + 1]);
        c[i + 2] = fqs_mad(m, (int32_t)P29::L[2], c[i + 2]);
        c[i + 3] = fqs_mad(m, (int32_t)P29::L[3], c[i + 3]);
        c[i + 4] = fqs_mad(m, (int32_t)P29::L[4], c[i + 4]);
        c[i + 8] = fqs_mad(m, p8, c[i + 8]);
        carry = fqs_sar29(t);
    }
    c[9] += carry;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        r[i] = (int32_t)((uint32_t)c[9 + i] & M29);
        // A masked limb is provably non-negative; the compiler then zero-extends it, and the product of a zero-extended and a
        // sign-extended factor is no v_mad_i64_i32 any more but two v_mad_u64_u32 and a move.  Behind the pin nothing is known
        // about the sign, so every partial product of a later product is the one signed multiply-add.
        HALO_PIN_VGPR(r[i]);
        c[10 + i] += fqs_sar29(c[9 + i]);
    }
    r[8] = (int32_t)c[17];
}
// Columns c[0..17] of a product, the low nine started at 2^29 - 1.  Every sum of a low column is pinned, not the first only as
// in fq_mul: with the first alone the compiler kept k29 in place but regrouped the rest of the column behind it, five 64-bit
// additions per product.  The partial products go row by row (all of a[0], then all of a[1], ...), so that two pinned sums of one
// column are never neighbours: a pin right in front of the instruction that reads it costs a wait state (s_nop) each time.
HALO_DEV void fqs_columns_start(fqs_col (&c)[18]) {
    fqs_col k29 = M29;
    HALO_PIN_VGPR(k29);  // a register pair: the free addend of each low column's first multiply-add (fq_mul)
#pragma unroll
    for (int k = 0; k < 18; k++) c[k] = k < 9 ? k29 : 0;
}
HALO_DEV void fqs_term(fqs_col (&c)[18], int k, int32_t x, int32_t y) {
    c[k] = fqs_mad(x, y, c[k]);
    if (k < 9) HALO_PIN_VGPR(c[k]);
}
HALO_DEV void fqs_columns(const int32_t (&a)[9], const int32_t (&b)[9], fqs_col (&c)[18]) {
    fqs_columns_start(c);
#pragma unroll
    for (int i = 0; i < 9; i++) {
#pragma unroll
        for (int j = 0; j < 9; j++) fqs_term(c, i + j, a[i], b[j]);
    }
}
// the operand of a product: Fqs or Fqd
template <int K> HALO_DEV const int32_t (&fqs_limbs(const Fqs<K> &a))[9] { return a.v; }
template <int K> HALO_DEV const int32_t (&fqs_limbs(const Fqd<K> &a))[9] { return a.v; }
template <class T> struct fqs_bound;
template <int K> struct fqs_bound<Fqs<K>> { static constexpr int value = K; };
template <int K> struct fqs_bound<Fqd<K>> { static constexpr int value = K; };

template <class A, class B>
HALO_DEV Fqs<2> fqs_mul(const A &a, const B &b) {
    static_assert(fqs_bound<A>::value * fqs_bound<B>::value <= 120, "Montgomery product bound: Ka*Kb/128 + 1 must stay < 2");
    fqs_col c[18];
    fqs_columns(fqs_limbs(a), fqs_limbs(b), c);
    Fqs<2> r;
    fqs_reduce(c, r.v);
    return r;
}
// squaring: 45 partial products; the doubled limb is below 2^30 in magnitude.  a^2 >= 0, so the result is in [0, 2p): an Fq<2>.
template <class A>
HALO_DEV Fq<2> fqs_sqr(const A &a0) {
    static_assert(fqs_bound<A>::value * fqs_bound<A>::value <= 120, "Montgomery square bound");
    const int32_t (&a)[9] = fqs_limbs(a0);
    int32_t d[9];
#pragma unroll
    for (int i = 0; i < 9; i++) {
        d[i] = a[i] * 2;
        HALO_PIN_VGPR(d[i]);  // or the compiler factors the 2 out of a column again, at the price of a 64-bit shift and an add
    }
    fqs_col c[18];
    fqs_columns_start(c);
#pragma unroll
    for (int i = 0; i < 9; i++) {
        fqs_term(c, 2 * i, a[i], a[i]);
#pragma unroll
        for (int j = i + 1; j < 9; j++) fqs_term(c, i + j, d[i], a[j]);
    }
    int32_t r[9];
    fqs_reduce(c, r);
    Fq<2> o;
#pragma unroll
    for (int i = 0; i < 9; i++) o.v[i] = (uint32_t)r[i];
    return o;
}
// a*b + c*d with ONE Montgomery reduction (fq_mul_add_mul); a difference of products takes the negated operand as it is
template <class A, class B, class C, class D>
HALO_DEV Fqs<2> fqs_mul_add_mul(const A &a0, const B &b0, const C &c0, const D &d0) {
    static_assert(fqs_bound<A>::value * fqs_bound<B>::value + fqs_bound<C>::value * fqs_bound<D>::value <= 120,
                  "fused product bound: (KaKb + KcKd)/128 + 1 must stay < 2");
    const int32_t (&a)[9] = fqs_limbs(a0), (&b)[9] = fqs_limbs(b0), (&c2)[9] = fqs_limbs(c0), (&d)[9] = fqs_limbs(d0);
    fqs_col c[18];
    fqs_columns_start(c);
#pragma unroll
    for (int i = 0; i < 9; i++) {
#pragma unroll
        for (int j = 0; j < 9; j++) {
            fqs_term(c, i + j, a[i], b[j]);
            fqs_term(c, i + j, c2[i], d[j]);
        }
    }
    Fqs<2> r;
    fqs_reduce(c, r.v);
    return r;
}

// ------------------------------------------------------------------ conversions back to the stored form
// |v| < K p -> the representative in [0, 2p).  With q = floor(v / 2^254) (the sign of limb 8 included) subtract q p if
// q < 0 and (q - 1) p otherwise: what is left is r - q d or 2^254 + r - (q - 1) d, with r < 2^254 and p = 2^254 + d, d < 2^126.
template <int K>
HALO_DEV Fq<2> fqs_tighten(const Fqs<K> &a) {
    static_assert(K <= 60, "tighten: bound too large");
    int32_t q = a.v[8] >> 22;
    int32_t s = q - 1 - (q >> 31);
    int64_t w[9];
#pragma unroll
    for (int i = 0; i < 9; i++) w[i] = (int64_t)a.v[i] - (int64_t)s * (int64_t)P29::L[i];
    Fq<2> r;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        r.v[i] = (uint32_t)w[i] & M29;
        w[i + 1] += w[i] >> 29;
    }
    r.v[8] = (uint32_t)w[8];
    return r;
}
// a raw difference plus K p, carried once: the non-negative value below 2K p
template <int K>
HALO_DEV Fq<2 * K> fqd_lift(const Fqd<K> &a) {
    static_assert(2 * K <= 60, "lift: bound too large");
    int32_t t[9];
#pragma unroll
    for (int i = 0; i < 9; i++) t[i] = a.v[i] + (int32_t)KP<K>::value.v[i];
    Fq<2 * K> r;
    carry_pass(t, r.v);
    return r;
}
// a == 0 (mod p) for a raw difference, |a| < K p.  a = k p with |k| < K has limb 0 = k (mod 2^29), of either sign: only then
// is the value lifted and reduced.
template <int K>
HALO_DEV bool fqd_is_zero_modp(const Fqd<K> &a) {
    if ((((uint32_t)a.v[0] + (uint32_t)K) & M29) >= (uint32_t)(2 * K + 1)) return false;
    return fq_limbs_zero(fq_canonical(fqd_lift(a)));
}

}  // namespace halo
