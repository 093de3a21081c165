// Exercises the host-side arithmetic of the library (csrc/host_math.hpp: fields, group law, fixed-base table, GLV digit
// expansion, SHA3-based key scalars, the stream skip, h(z), the batched inversion) under AddressSanitizer + UBSan; built and run by tests/test_host_sanitizers.py.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>
#include "host_math.hpp"
using namespace halo::host;
int main() {
    std::mt19937_64 g(1);
    Point G = Point::generator();
    Point acc = Point::infinity();
    for (int i = 0; i < 200; ++i) {
        Fr k = urs_scalar(i);
        Point p = G.mul(k);
        acc = acc + p;
        GlvDigits d = glv_digits(k);
        if (d.n > 132) { printf("bad digits\n"); return 1; }
        FixedBaseTable t(p);
        Fr s = urs_scalar(1000 + i);
        Point a = t.mul(s), b = p.mul(s);
        uint64_t wa[12], wb[12];
        a.store_normalized(wa); b.store_normalized(wb);
        if (memcmp(wa, wb, 96)) { printf("table mismatch\n"); return 1; }
    }
    // inv() (62 division steps at a time, host_math.hpp modinv) against the Fermat power, both fields: random values, small
    // integers and their negatives, powers of two, raw limb patterns (any value below the modulus is some element)
    {
        long bad = 0;
        Fr x = urs_scalar(7);
        Fq q = Point::generator().mul(urs_scalar(8)).to_affine().x;
        for (int i = 0; i < 3000; ++i) {
            x = x * x + Fr::from_u64(i + 3); q = q * q + Fq::from_u64(5);
            bad += !(x.inv() == x.inv_fermat()) + !(q.inv() == q.inv_fermat());
            bad += !(x * x.inv() == Fr::one()) + !(q * q.inv() == Fq::one());
        }
        for (u64 k = 1; k < 200; ++k) {
            Fr a = Fr::from_u64(k); Fq b = Fq::from_u64(k);
            bad += !(a.inv() == a.inv_fermat()) + !((-a).inv() == (-a).inv_fermat()) + !(b.inv() == b.inv_fermat()) + !((-b).inv() == (-b).inv_fermat());
            Fr r1{{k, 0, 0, 0}}, r2{{0, 0, 0, k}}, r3{{~(u64)0, ~(u64)0, ~(u64)0, k}};
            bad += !(r1.inv() == r1.inv_fermat()) + !(r2.inv() == r2.inv_fermat()) + !(r3.inv() == r3.inv_fermat());
            Fq s1{{k, k, k, k & 0xfff}};
            bad += !(s1.inv() == s1.inv_fermat());
        }
        Fr p2 = Fr::one();
        for (int s = 0; s < 260; ++s) { p2 = p2 + p2; bad += !(p2.inv() == p2.inv_fermat()) + !((-p2).inv() == (-p2).inv_fermat()); }
        if (!Fr::zero().inv().is_zero() || bad) { printf("inverse mismatch: %ld\n", bad); return 1; }
    }
    // Rng::skip_scalars(k), then scalar(), is the (k + 1)-th scalar of the stream
    for (u64 k : {0, 1, 5, 1000}) {
        Rng a{0x48414C4F00000001ULL}, b{0x48414C4F00000001ULL};
        a.skip_scalars(k);
        Fr want;
        for (u64 i = 0; i <= k; ++i) want = b.scalar();
        if (!(a.scalar() == want) || a.state != b.state) { printf("skip_scalars mismatch at k = %llu\n", (unsigned long long)k); return 1; }
    }
    // h_eval against the product written out, factor by factor with z^(2^k) from the generic power: the head factor
    // 1 + xi_lg z, then 1 + xi_(lg-k) z^(2^k) for 0 < k < lg (pcdl.rs:79-91; the head stands alone at lg = 0 and lg = 1, where the
    // bounds 1 .. lg - 1 of the loop are empty), at a random z and at z = 0
    for (size_t lg : {0, 1, 2, 5, 20}) {
        std::vector<Fr> xis(lg + 1);
        for (size_t i = 0; i <= lg; ++i) xis[i] = urs_scalar(5000 + 100 * lg + i);
        for (const Fr &z : {urs_scalar(7000 + lg), Fr::zero()}) {
            Fr want = Fr::one() + xis[lg] * z;
            for (size_t k = 1; k < lg; ++k) {
                const uint64_t e[4] = {(u64)1 << k, 0, 0, 0};
                want = want * (Fr::one() + xis[lg - k] * z.pow(e));  // z^(2^k) by the generic power
            }
            if (!(h_eval(xis.data(), lg, z) == want)) { printf("h_eval mismatch at lg = %zu\n", lg); return 1; }
            if (z.is_zero() && !(want == Fr::one())) { printf("h(0) != 1 at lg = %zu\n", lg); return 1; }
        }
    }
    // batch_inverse times its inputs is one
    for (size_t len : {0, 1, 2, 20}) {
        std::vector<Fr> in(len), out(len + 1, Fr::from_u64(77));
        for (size_t i = 0; i < len; ++i) in[i] = urs_scalar(9000 + i);
        batch_inverse(in.data(), len, out.data());
        for (size_t i = 0; i < len; ++i)
            if (!(in[i] * out[i] == Fr::one())) { printf("batch_inverse mismatch at %zu of %zu\n", i, len); return 1; }
        if (!(out[len] == Fr::from_u64(77))) { printf("batch_inverse wrote past its output\n"); return 1; }
    }
    uint64_t w[12]; acc.store_normalized(w);
    printf("ok %016llx\n", (unsigned long long)w[0]);
    return 0;
}
