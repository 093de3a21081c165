// The signed radix-2^29 field layer and the group law built on it (csrc/fq29s.hpp, the XyzzS part of csrc/curve.hpp), compiled for
// the CPU: HALO_DEV becomes `inline`, the register pins vanish and a column is an int64_t, so that -fsanitize=undefined reports a
// column that leaves 63 bits as signed overflow.  Built with -fsanitize=address,undefined by tests/test_signed_field_host.py, which
// writes the cases and checks every result with Python integers.  No HIP call is made: the HIP headers are included for their types.
//
//   signed_field_host <cases> <results>
//
// <cases>: blocks, each a header of three 32-bit words (operation, number of cases n, parameter) and its operands:
//   0 product        n x (a, b)         -> n x 9 limbs     operands are raw signed limbs (9 words each)
//   1 square         n x a              -> n x 9 limbs
//   2 fused a b+c d  n x (a, b, c, d)   -> n x 9 limbs
//   3 a - b - 2c     n x (a, b, c)      -> n x 9 limbs     (signed normalised operands)
//   4 tighten        n x a              -> n x 9 limbs
//   5 zero test      n x a              -> n x 1 word      parameter: K (4 or 10, the two the group law uses)
//   6 2a, carried    n x a              -> n x 9 limbs
//   7 chain          n affine points (20 words each: x, pad, y, pad) added one by one to infinity with xyzs_madd -> 40 words
//   8 two chains     the first `parameter` points and the rest are summed as in 7, then the sums added with xyzs_add -> 40 words
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define HALO_DEV inline
#define HALO_PIN_VGPR(x) ((void)(x))
#include <hip/hip_runtime.h>
static inline int __shfl(int v, int, int) { return v; }  // the cross-lane moves of curve.hpp are not exercised here

#include "curve.hpp"

using namespace halo;

template <class T>
static T limbs(const uint32_t *w) {
    T r;
    for (int i = 0; i < 9; i++) r.v[i] = (int32_t)w[i];
    return r;
}
template <class T>
static void put(std::vector<uint32_t> &o, const T &a) {
    for (int i = 0; i < 9; i++) o.push_back((uint32_t)a.v[i]);
}
static AffN aff(const uint32_t *w) {
    AffN r;
    for (int i = 0; i < 9; i++) { r.x.v[i] = w[i]; r.y.v[i] = w[10 + i]; }
    return r;
}
static XyzzS chain(const uint32_t *w, uint32_t n) {
    XyzzS acc = xyzs_inf();
    for (uint32_t i = 0; i < n; i++) xyzs_madd(acc, aff(w + 20 * (size_t)i));
    return acc;
}
static void put_point(std::vector<uint32_t> &o, const XyzzS &p) {
    uint32_t w[XYZZ_WORDS];
    xyzs_store(w, p);
    o.insert(o.end(), w, w + XYZZ_WORDS);
}

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s <cases> <results>\n", argv[0]); return 2; }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open files\n"); return 2; }
    static const size_t per_case[9] = {18, 9, 36, 27, 9, 9, 9, 20, 20};
    size_t blocks = 0, cases = 0;
    uint32_t head[3];
    while (fread(head, 4, 3, in) == 3) {
        const uint32_t op = head[0], n = head[1], par = head[2];
        if (op > 8 || n > (1u << 20)) { fprintf(stderr, "bad block header\n"); return 2; }
        std::vector<uint32_t> a((size_t)n * per_case[op] + 1), o;
        if (fread(a.data(), 4, (size_t)n * per_case[op], in) != (size_t)n * per_case[op]) { fprintf(stderr, "short block\n"); return 2; }
        if (op == 7) put_point(o, chain(a.data(), n));
        else if (op == 8) {
            if (par > n) { fprintf(stderr, "bad split\n"); return 2; }
            XyzzS s = chain(a.data(), par), t = chain(a.data() + 20 * (size_t)par, n - par);
            xyzs_add(s, t);
            put_point(o, s);
        } else {
            for (size_t i = 0; i < n; i++) {
                const uint32_t *w = a.data() + i * per_case[op];
                if (op == 0) put(o, fqs_mul(limbs<Fqd<10>>(w), limbs<Fqd<10>>(w + 9)));
                else if (op == 1) put(o, fqs_sqr(limbs<Fqd<10>>(w)));
                else if (op == 2) put(o, fqs_mul_add_mul(limbs<Fqd<10>>(w), limbs<Fqd<10>>(w + 9), limbs<Fqd<8>>(w + 18), limbs<Fqs<2>>(w + 27)));
                else if (op == 3) put(o, fqs_sub_sub2(limbs<Fqs<2>>(w), limbs<Fqs<2>>(w + 9), limbs<Fqs<2>>(w + 18)));
                else if (op == 4) put(o, fqs_tighten(limbs<Fqs<10>>(w)));
                else if (op == 5) {
                    if (par == 4) o.push_back(fqd_is_zero_modp(limbs<Fqd<4>>(w)) ? 1u : 0u);
                    else if (par == 10) o.push_back(fqd_is_zero_modp(limbs<Fqd<10>>(w)) ? 1u : 0u);
                    else { fprintf(stderr, "zero test: K = %u is not built\n", par); return 2; }
                } else put(o, fqs_muls2(limbs<Fqs<2>>(w)));
            }
        }
        if (fwrite(o.data(), 4, o.size(), out) != o.size()) { fprintf(stderr, "write failed\n"); return 2; }
        blocks++;
        cases += n;
    }
    fclose(in);
    if (fclose(out)) { fprintf(stderr, "write failed\n"); return 2; }
    printf("ok %zu blocks %zu cases\n", blocks, cases);
    return 0;
}
