// Device code of the wire format's point decompression (decompress.hip has the kernels and the story): the square root in Fq
// and one point's record.  A header so that tests/native/decompress_host.cpp can compile the same text for the CPU
// (HALO_DEV = inline), as tests/native/lazy_field_host.cpp does for the lazy fields.
#pragma once
#include "field.hpp"

namespace halo {

constexpr uint32_t DECOMP_REC_IN = 6, DECOMP_REC_OUT = 14;  // words of a point's record in and out (internal.hpp DECOMP_*_WORDS)
constexpr uint32_t SQRT_TABLE_WORDS = 4 * 256 * 8 + 256;     // S[4][256] (8 words each), then KEY[256]

// (t - 1) / 2 = 2^221 + E, E below 2^93: t = (p - 1) >> 32 is limbs 1..7 of p
constexpr uint32_t E0 = ((FqCfg::P[1] - 1u) >> 1) | (FqCfg::P[2] << 31), E1 = (FqCfg::P[2] >> 1) | (FqCfg::P[3] << 31), E2 = FqCfg::P[3] >> 1;
static_assert((FqCfg::P[1] & 1u) == 1u && FqCfg::P[4] == 0 && FqCfg::P[5] == 0 && FqCfg::P[6] == 0 && FqCfg::P[7] == 0x40000000u && (E2 >> 29) == 0, "t = 2^222 + 94 bits");

HALO_DEV Fe fq_pow_half_t(const Fe &a) {  // a^((t-1)/2)
    Fe acc = a;                           // bit 221
#pragma unroll 1
    for (int i = 0; i < 125; i++) acc = fe_sqr<FqCfg>(acc);  // bits 220..96 are zero
#pragma unroll 1
    for (int w = 2; w >= 0; w--) {
        const uint32_t e = w == 2 ? E2 : (w == 1 ? E1 : E0);
#pragma unroll 1
        for (int bit = 31; bit >= 0; bit--) {
            acc = fe_sqr<FqCfg>(acc);
            if ((e >> bit) & 1u) acc = fe_mul<FqCfg>(acc, a);
        }
    }
    return acc;
}

constexpr uint32_t TAB_S_WORDS = 4 * 256 * 8;  // S[4][256], then KEY[256]

// r with r^2 == a if a is a square (*ok), some field element otherwise
HALO_DEV Fe fq_sqrt(const Fe &a, const uint4 *s_tab, bool *ok) {
    const Fe w = fq_pow_half_t(a);
    Fe r = fe_mul<FqCfg>(a, w), b = fe_mul<FqCfg>(r, w);
    const uint4 *key = s_tab + TAB_S_WORDS / 4;
#pragma unroll 1
    for (int i = 0; i < 4; i++) {
        Fe c = b;
#pragma unroll 1
        for (int j = 8 * i; j < 24; j++) c = fe_sqr<FqCfg>(c);
        uint32_t d = 0;  // (every lane reads the same address: a broadcast)
#pragma unroll 2
        for (uint32_t j = 0; j < 64; j++) {
            const uint4 k = key[j];
            d = k.x == c.v[0] ? 4 * j : d;
            d = k.y == c.v[0] ? 4 * j + 1 : d;
            d = k.z == c.v[0] ? 4 * j + 2 : d;
            d = k.w == c.v[0] ? 4 * j + 3 : d;
        }
        const uint4 lo = s_tab[(256 * i + d) * 2], hi = s_tab[(256 * i + d) * 2 + 1];  // d < 256: inside S[i]
        Fe s;
        s.v[0] = lo.x; s.v[1] = lo.y; s.v[2] = lo.z; s.v[3] = lo.w;
        s.v[4] = hi.x; s.v[5] = hi.y; s.v[6] = hi.z; s.v[7] = hi.w;
        r = fe_mul<FqCfg>(r, s);
        b = fe_mul<FqCfg>(b, fe_sqr<FqCfg>(s));
    }
    *ok = fe_eq(fe_sqr<FqCfg>(r), a);
    return r;
}

HALO_DEV bool fe_less(const Fe &a, const Fe &b) {  // a < b as integers
    uint64_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) br = (((uint64_t)a.v[i] - b.v[i] - br) >> 32) & 1;
    return br != 0;
}
HALO_DEV bool fe_below_p(const Fe &a) {
    uint64_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) br = (((uint64_t)a.v[i] - FqCfg::P[i] - br) >> 32) & 1;
    return br != 0;
}
HALO_DEV Fe fe_select(bool c, const Fe &a, const Fe &b) {
    Fe r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = c ? a.v[i] : b.v[i];
    return r;
}

// rec: the 33 wire bytes of a point, zero-padded to DECOMP_REC_IN words.  o: DECOMP_REC_OUT words -- the Jacobian blob words
// (x, y, 1), or (1, 1, 0) for the point at infinity, then ok (1 / 0) and a pad word.  What Reader::point of wire.hip
// accepts and writes, bit for bit.
HALO_DEV void decompress_one(const uint64_t *rec, const uint4 *s_tab, uint64_t *o) {
    Fe xc = fe_load(rec);
    const uint4 top = *reinterpret_cast<const uint4 *>(rec + 4);
    const uint32_t flags = top.x & 0xC0u, stray = top.x & 0x3Fu;
    const bool inf = flags == 0x40u, want_larger = flags == 0x80u;
    // flags 11 are invalid; infinity is all zeros beside its flag; a finite x is canonical (below 2^256: no stray bit, and below p)
    bool ok = flags != 0xC0u && stray == 0 && (inf ? fe_is_zero(xc) : fe_below_p(xc));
    xc = fe_select(ok && !inf, xc, fe_zero());
    const Fe one = fe_one<FqCfg>(), four = fe_dbl<FqCfg>(fe_dbl<FqCfg>(one));
    const Fe x = fe_to_mont<FqCfg>(xc);
    const Fe a = fe_add<FqCfg>(fe_mul<FqCfg>(fe_sqr<FqCfg>(x), x), fe_add<FqCfg>(four, one));  // x^3 + 5
    bool square;
    Fe y = fq_sqrt(a, s_tab, &square);
    const Fe ny = fe_neg<FqCfg>(y);
    const Fe yc = fe_from_mont<FqCfg>(y), nyc = fe_from_mont<FqCfg>(ny);
    const bool y_larger = fe_less(nyc, yc);  // y > -y
    y = fe_select(y_larger != want_larger, ny, y);
    ok = ok && (inf || (square && !(want_larger && fe_is_zero(y))));
    fe_store(o, fe_select(inf, one, x));
    fe_store(o + 4, fe_select(inf, one, y));
    fe_store(o + 8, fe_select(inf, fe_zero(), one));
    *reinterpret_cast<uint4 *>(o + 12) = make_uint4(ok ? 1u : 0u, 0u, 0u, 0u);
}

}  // namespace halo
