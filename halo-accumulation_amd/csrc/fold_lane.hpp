// One lane's share of the key folds of pcdl::open (pcdl.rs:216-219): G[j] + xi G[j+m] and its two-round form, with the digit
// strings they walk.  key_fold.hip's k_fold_points and k_fold_points4 call them once or twice per lane; tests/native/fold_host.cpp
// compiles the same text for the CPU (HALO_DEV = inline, field.hpp) and runs it under ASan + UBSan.  Needs curve.hpp only.
#pragma once
#include "curve.hpp"

namespace halo {

// ------------------------------------------------------------------ K3: G'[j] = G[j] + xi * G[j+m]
// xi is one scalar for the whole launch, expanded on the host as xi = sum_i d_i 2^i with digits from the six
// Eisenstein units {+-1, +-lambda, +-lambda^2} (host_math.hpp glv_digits): a ~127-step double-and-add with
// ~71 additions, each of a "free" point d_i * P = (beta^e x, +-y) -- two multiplications per input point.
// Every branch below depends only on kernel arguments, so the 64 lanes of a wave never diverge.
struct GlvArg {
    uint32_t dig[14];  // ten 3-bit digit codes per word, least significant digit first (host_math.hpp glv_digits)
    int ndigits;
};
HALO_DEV Fq<2> fq_const(const uint32_t (&c)[9]) {
    Fq<2> r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.v[i] = c[i];
    return r;
}
HALO_DEV Fq<2> pick3(int e, const Fq<2> &a, const Fq<2> &b, const Fq<2> &c) {
    Fq<2> r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.v[i] = e == 0 ? a.v[i] : (e == 1 ? b.v[i] : c.v[i]);
    return r;
}
// G[j] + xi * G[j + m] as a Jacobian point
HALO_DEV JacN fold_one(const uint32_t *__restrict__ G, uint32_t j, uint32_t m, const GlvArg &a) {
    AffN hi = aff_load(G + AFF_STRIDE * (size_t)(j + m));
    AffN lo = aff_load(G + AFF_STRIDE * (size_t)j);
    if (aff_is_inf(hi)) return jac_from_aff(lo);  // G[j] + xi * infinity = G[j]
    constexpr uint32_t BETA[9] = {0x1342a796, 0x3fdac51, 0x54dab11, 0x5b221a6, 0xccd27ac, 0x15cc87a4, 0x1b1533b6, 0x169e85e1, 0x3b0093};
    constexpr uint32_t BETA2[9] = {0xcbd58eb, 0x1a2f8f16, 0xd140efa, 0x7bdfb9, 0x1333ecad, 0xa33785b, 0x4eacc49, 0x9617a1e, 0x4ff6c};
    Fq<2> x0 = hi.x, x1 = fq_mul(hi.x, fq_const(BETA)), x2 = fq_mul(hi.x, fq_const(BETA2));
    Fq<2> yp = hi.y, yn = fq_neg<2>(hi.y);
    JacN acc = jac_inf();
    int top = a.ndigits - 1;
#pragma unroll 1
    for (int word = top / 10; word >= 0; word--) {
        uint32_t w = 0;
#pragma unroll
        for (int q = 0; q < 14; q++) w = (q == word) ? a.dig[q] : w;
#pragma unroll 1
        for (int k = (word == top / 10) ? (top % 10) : 9; k >= 0; k--) {
            acc = jac_dbl(acc);
            uint32_t code = (w >> (3 * k)) & 7u;
            if (code) {  // wave-uniform: +-w^e * hi = (beta^e x, +-y)
                AffN t;
                t.x = pick3((int)((code - 1) % 3), x0, x1, x2);
                t.y = code > 3 ? yn : yp;
                acc = jac_madd(acc, t);
            }
        }
    }
    return jac_madd(acc, lo);
}

// ------------------------------------------------------------------ K3': two halving rounds of G in one pass
// After two rounds without touching G the folded key is G''[j] = G[j] + s1 G[j+m] + s2 G[j+2m] + s3 G[j+3m] with
// (s1, s2, s3) = (xi_2, xi_1, xi_1 xi_2), m = a quarter of the key (pcdl.rs:218 applied twice).  The three scalar
// multiplications share ONE doubling chain (Straus): ~128 doublings + 3 x ~71 additions per output instead of
// 2 x (128 + 71) for each of the 1.5 outputs the two separate folds produce -- ~38 % fewer field products for the
// same two rounds.  The rounds in between take L and R from MSMs over the unfolded key (the "no-fold" form below).
struct GlvArg3 {
    uint32_t dig[3][14];  // as GlvArg, one digit string per scalar
    int ndigits;          // longest of the three
};
HALO_DEV JacN fold_one4(const uint32_t *G, uint32_t j, uint32_t m, const GlvArg3 &a) {
    constexpr uint32_t BETA[9] = {0x1342a796, 0x3fdac51, 0x54dab11, 0x5b221a6, 0xccd27ac, 0x15cc87a4, 0x1b1533b6, 0x169e85e1, 0x3b0093};
    constexpr uint32_t BETA2[9] = {0xcbd58eb, 0x1a2f8f16, 0xd140efa, 0x7bdfb9, 0x1333ecad, 0xa33785b, 0x4eacc49, 0x9617a1e, 0x4ff6c};
    AffN p1 = aff_load(G + AFF_STRIDE * (size_t)(j + m)), p2 = aff_load(G + AFF_STRIDE * (size_t)(j + 2 * m)),
         p3 = aff_load(G + AFF_STRIDE * (size_t)(j + 3 * m));
    bool live1 = !aff_is_inf(p1), live2 = !aff_is_inf(p2), live3 = !aff_is_inf(p3);
    // acc += unit(code) * p: code is wave-uniform; lambda^e * (x, y) = (beta^e x, y)
    auto step = [&](JacN &acc, const AffN &p, bool live, uint32_t code) {
        if (!code) return;
        int e = (int)((code - 1) % 3);
        AffN q;
        q.x = p.x;
        if (e) q.x = fq_mul(p.x, fq_const(e == 1 ? BETA : BETA2));
        q.y = code > 3 ? fq_neg<2>(p.y) : p.y;
        if (live) acc = jac_madd(acc, q);
    };
    JacN acc = jac_inf();
    int top = a.ndigits - 1;
#pragma unroll 1
    for (int word = top / 10; word >= 0; word--) {
        uint32_t w1 = 0, w2 = 0, w3 = 0;
#pragma unroll
        for (int q = 0; q < 14; q++) {
            w1 = (q == word) ? a.dig[0][q] : w1;
            w2 = (q == word) ? a.dig[1][q] : w2;
            w3 = (q == word) ? a.dig[2][q] : w3;
        }
#pragma unroll 1
        for (int k = (word == top / 10) ? (top % 10) : 9; k >= 0; k--) {
            acc = jac_dbl(acc);
            step(acc, p1, live1, (w1 >> (3 * k)) & 7u);
            step(acc, p2, live2, (w2 >> (3 * k)) & 7u);
            step(acc, p3, live3, (w3 >> (3 * k)) & 7u);
        }
    }
    return jac_madd(acc, aff_load(G + AFF_STRIDE * (size_t)j));
}

}  // namespace halo
