// One lane's share of the succinct check's Fiat-Shamir transcript (pcdl.rs:272-296) as transcript.hip's kernels run it: the
// compressed encoding of a blob's point with its validity verdict, and the three rho_0 messages of pcdl::succinct_check, each
// one padded block of the 136-byte rate -- one permutation (keccak_lane.hpp) over a fixed layout.  Bit for bit what
// host::Transcript and host::Point::on_curve (host_math.hpp) compute.  tests/native/transcript_lane_host.cpp compiles the same
// text for the CPU (HALO_DEV = inline) and runs it under ASan + UBSan.  No LDS, no scratch; needs field.hpp only.
//
// Blob words are 8-byte aligned, not 16 (an Instance has an odd number of words): everything here moves 64-bit words.
#pragma once
#include "decompress.hpp"  // (fe_less, fe_below_p: the y-sign rule and the coordinate bound of the wire format)
#include "keccak_lane.hpp"

namespace halo {

constexpr uint32_t TR_VALID = 0, TR_INVALID = 1, TR_FOREIGN = 2;  // verdicts of point_compress_lane
constexpr uint32_t TR_POINT_WORDS = 5;                            // a compressed point: 4 canonical x words, then flag | verdict << 8

HALO_DEV Fe fe_load64(const uint64_t *p) {
    Fe r;
#pragma unroll
    for (int k = 0; k < 4; k++) { r.v[2 * k] = (uint32_t)p[k]; r.v[2 * k + 1] = (uint32_t)(p[k] >> 32); }
    return r;
}
HALO_DEV uint64_t fe_word64(const Fe &a, int k) { return (uint64_t)a.v[2 * k] | ((uint64_t)a.v[2 * k + 1] << 32); }
HALO_DEV void fe_store64(uint64_t *p, const Fe &a) {
#pragma unroll
    for (int k = 0; k < 4; k++) p[k] = fe_word64(a, k);
}

// the four words are below r (pcdl_internal.hpp scalar_ok)
HALO_DEV bool scalar_ok_lane(const Fe &s) {
    uint64_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) br = (((uint64_t)s.v[i] - FrCfg::P[i] - br) >> 32) & 1;
    return br != 0;
}

// The 33 bytes ark-serialize writes for the normalised point (x, y) in Montgomery form, or for infinity: out[0..4) the
// canonical x (0 for infinity), out[4] the flag byte -- 0x80 iff y > -y as canonical integers, 0x40 for infinity.
HALO_DEV void point_compress_xy(const Fe &x, const Fe &y, bool inf, uint64_t out[TR_POINT_WORDS]) {
    const Fe xc = fe_from_mont<FqCfg>(x), yc = fe_from_mont<FqCfg>(y), nyc = fe_from_mont<FqCfg>(fe_neg<FqCfg>(y));
    const bool y_larger = fe_less(nyc, yc);
#pragma unroll
    for (int k = 0; k < 4; k++) out[k] = inf ? 0 : fe_word64(xc, k);
    out[4] = inf ? 0x40u : (y_larger ? 0x80u : 0u);
}

// jac: the arkworks Jacobian words of a blob's point.  What host::Point::load(jac) answers:
//   a coordinate >= p, or a finite point off the curve  -> TR_INVALID   (on_curve() false)
//   Z = 0                                               -> infinity, TR_VALID   (is_inf(); X, Y arbitrary below p)
//   Z neither 0 nor Montgomery 1                        -> TR_FOREIGN: not normalised, the host's transcript decides
//   (x, y, 1) with y^2 = x^3 + 5                        -> TR_VALID
// out: point_compress_xy's words for a valid point (zeros otherwise), the verdict in bits 8.. of out[4].
HALO_DEV uint32_t point_compress_lane(const uint64_t *jac, uint64_t out[TR_POINT_WORDS]) {
    const Fe X = fe_load64(jac), Y = fe_load64(jac + 4), Z = fe_load64(jac + 8);
    const bool below = fe_below_p(X) && fe_below_p(Y) && fe_below_p(Z);
    const bool inf = fe_is_zero(Z), unit = fe_eq(Z, fe_one<FqCfg>());
    const Fe one = fe_one<FqCfg>(), five = fe_add<FqCfg>(fe_dbl<FqCfg>(fe_dbl<FqCfg>(one)), one);
    // (a coordinate >= p never reaches the products' result: `below` decides first)
    const bool on = fe_eq(fe_sqr<FqCfg>(Y), fe_add<FqCfg>(fe_mul<FqCfg>(fe_sqr<FqCfg>(X), X), five));
    const uint32_t verdict = !below ? TR_INVALID : inf ? TR_VALID : !unit ? TR_FOREIGN : on ? TR_VALID : TR_INVALID;
    point_compress_xy(X, Y, inf, out);
    if (verdict != TR_VALID) {
#pragma unroll
        for (int k = 0; k < 5; k++) out[k] = 0;
    }
    out[4] |= (uint64_t)verdict << 8;
    return verdict;
}

// ---- the padded block: OR whole 64-bit lanes at compile-time byte offsets (the 33-byte points make them unaligned)
template <int OFF>
HALO_DEV void tr_put_word(uint64_t (&a)[25], uint64_t w) {
    constexpr int lane = OFF / 8, sh = (OFF % 8) * 8;
    if constexpr (sh == 0) a[lane] |= w;
    else { a[lane] |= w << sh; a[lane + 1] |= w >> (64 - sh); }
}
template <int OFF>
HALO_DEV void tr_put_byte(uint64_t (&a)[25], uint64_t b) { a[OFF / 8] |= (b & 0xFFu) << ((OFF % 8) * 8); }
template <int OFF>
HALO_DEV void tr_put_scalar(uint64_t (&a)[25], const Fe &s_mont) {  // 32 bytes: the canonical integer, little-endian
    const Fe c = fe_from_mont<FrCfg>(s_mont);
    tr_put_word<OFF>(a, fe_word64(c, 0)); tr_put_word<OFF + 8>(a, fe_word64(c, 1));
    tr_put_word<OFF + 16>(a, fe_word64(c, 2)); tr_put_word<OFF + 24>(a, fe_word64(c, 3));
}
template <int OFF>
HALO_DEV void tr_put_point(uint64_t (&a)[25], const uint64_t *p) {  // 33 bytes: point_compress_xy's words
    tr_put_word<OFF>(a, p[0]); tr_put_word<OFF + 8>(a, p[1]); tr_put_word<OFF + 16>(a, p[2]); tr_put_word<OFF + 24>(a, p[3]);
    tr_put_byte<OFF + 32>(a, p[4]);
}
// LEN message bytes are in: the LE32 tag 0 (four zero bytes), 0x06, 0x80 in byte 135; permute; the digest mod r, Montgomery
template <int LEN>
HALO_DEV Fe tr_finish_rho0(uint64_t (&a)[25]) {
    static_assert(LEN + 4 < 136, "one block of the rate");
    tr_put_byte<LEN + 4>(a, 0x06);
    tr_put_byte<135>(a, 0x80);
    keccak_f1600(a);
    return fe_to_mont<FrCfg>(keccak_digest_mod_r(a));
}
HALO_DEV void tr_clear(uint64_t (&a)[25]) {
#pragma unroll
    for (int k = 0; k < 25; k++) a[k] = 0;
}

// rho_0(C, z, v): 33 + 32 + 32 bytes, 101 with the tag.  Points compressed (5 words), scalars Montgomery; result Montgomery.
HALO_DEV Fe rho0_C_z_v(const uint64_t *C, const Fe &z, const Fe &v) {
    uint64_t a[25];
    tr_clear(a);
    tr_put_point<0>(a, C); tr_put_scalar<33>(a, z); tr_put_scalar<65>(a, v);
    return tr_finish_rho0<97>(a);
}
// rho_0(C, z, v, C_bar): 134 bytes with the tag
HALO_DEV Fe rho0_C_z_v_Cbar(const uint64_t *C, const Fe &z, const Fe &v, const uint64_t *Cbar) {
    uint64_t a[25];
    tr_clear(a);
    tr_put_point<0>(a, C); tr_put_scalar<33>(a, z); tr_put_scalar<65>(a, v); tr_put_point<97>(a, Cbar);
    return tr_finish_rho0<130>(a);
}
// rho_0(xi, L, R): 32 + 33 + 33 bytes, 102 with the tag
HALO_DEV Fe rho0_xi_L_R(const Fe &xi, const uint64_t *L, const uint64_t *R) {
    uint64_t a[25];
    tr_clear(a);
    tr_put_scalar<0>(a, xi); tr_put_point<32>(a, L); tr_put_point<65>(a, R);
    return tr_finish_rho0<98>(a);
}

}  // namespace halo
