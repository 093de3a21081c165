// One lane's share of the key folds (csrc/fold_lane.hpp: fold_one, fold_one4 -- what k_fold_points and k_fold_points4 run once or
// twice per lane) compiled for the CPU as tests/native/lazy_field_host.cpp compiles the layer below: HALO_DEV becomes `inline`,
// the register pins vanish, everything else is the text the device compiler sees.  Built with -fsanitize=address,undefined by
// tests/test_fold_host.py, which writes the cases (tests/fold_cases.py) and compares the results with the oracle.  The digit
// strings come from host::glv_digits in this binary and are packed exactly as ipa_fold_points / ipa_fold_points4 pack them.
//
//   fold_host <cases> <results>
//
// <cases>: blocks of four 32-bit words (levels 1 | 2, n points, m outputs, k scalar sets; n = 2 m levels) followed by the key
// (n x 8 64-bit arkworks affine words, (0, 0) = infinity) and k sets of scalars (levels 1: xi; levels 2: s1 | s2 | s3; 4
// Montgomery words each).  The key goes to native limbs the way k_aff_to_native does it (aff_from_words, aff_store), every
// output comes back the way the kernels and k_native_to_aff do it (jac_to_aff, aff_to_words).
// <results>: per block and set m x 8 words.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#define HALO_DEV inline
#define HALO_PIN_VGPR(x) ((void)(x))
#include <hip/hip_runtime.h>
static inline int __shfl(int v, int, int) { return v; }  // the cross-lane moves of curve.hpp are not exercised here

#include "fold_lane.hpp"
#include "host_math.hpp"

template <class T>
static T *aligned(size_t n) {
    void *p = nullptr;
    if (posix_memalign(&p, 16, (n ? n : 1) * sizeof(T))) { fprintf(stderr, "out of memory\n"); exit(2); }
    memset(p, 0, (n ? n : 1) * sizeof(T));
    return static_cast<T *>(p);
}

// ipa_fold_points / ipa_fold_points4: ten 3-bit codes per word, least significant digit first
static int pack_digits(const uint64_t *scalar, uint32_t (&dig)[14]) {
    halo::host::GlvDigits dg = halo::host::glv_digits(halo::host::Fr::load(scalar));
    for (int i = 0; i < 14; ++i) dig[i] = 0;
    for (int i = 0; i < dg.n; ++i) dig[i / 10] |= (uint32_t)dg.d[i] << (3 * (i % 10));
    return dg.n;
}

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s <cases> <results>\n", argv[0]); return 2; }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open files\n"); return 2; }
    size_t blocks = 0, folds = 0;
    uint32_t head[4];
    while (fread(head, 4, 4, in) == 4) {
        const uint32_t levels = head[0], n = head[1], m = head[2], sets = head[3];
        if ((levels != 1 && levels != 2) || n != 2 * levels * m || n > (1u << 20) || sets > (1u << 16)) { fprintf(stderr, "bad block header\n"); return 2; }
        uint64_t *key = aligned<uint64_t>((size_t)n * 8), *sc = aligned<uint64_t>((size_t)sets * 12), *res = aligned<uint64_t>((size_t)m * 8);
        const size_t sc_words = (size_t)sets * (levels == 1 ? 4 : 12);
        if (fread(key, 8, (size_t)n * 8, in) != (size_t)n * 8 || fread(sc, 8, sc_words, in) != sc_words) { fprintf(stderr, "short block\n"); return 2; }
        uint32_t *G = aligned<uint32_t>((size_t)n * halo::AFF_STRIDE);  // exactly n points: a read past the key is ASan's to find
        for (uint32_t i = 0; i < n; i++) halo::aff_store(G + (size_t)halo::AFF_STRIDE * i, halo::aff_from_words(key + 8 * (size_t)i));
        for (uint32_t s = 0; s < sets; s++) {
            if (levels == 1) {
                halo::GlvArg a;
                a.ndigits = pack_digits(sc + 4 * (size_t)s, a.dig);
                for (uint32_t j = 0; j < m; j++) halo::aff_to_words(res + 8 * (size_t)j, halo::jac_to_aff(halo::fold_one(G, j, m, a)));
            } else {
                halo::GlvArg3 a;
                a.ndigits = 0;
                for (int t = 0; t < 3; t++) {
                    int nd = pack_digits(sc + 12 * (size_t)s + 4 * t, a.dig[t]);
                    if (nd > a.ndigits) a.ndigits = nd;
                }
                for (uint32_t j = 0; j < m; j++) halo::aff_to_words(res + 8 * (size_t)j, halo::jac_to_aff(halo::fold_one4(G, j, m, a)));
            }
            if (fwrite(res, 8, (size_t)m * 8, out) != (size_t)m * 8) { fprintf(stderr, "write failed\n"); return 2; }
            folds += m;
        }
        free(key); free(sc); free(res); free(G);
        blocks++;
    }
    fclose(in);
    if (fclose(out)) { fprintf(stderr, "write failed\n"); return 2; }
    printf("ok %zu blocks %zu folds\n", blocks, folds);
    return 0;
}
