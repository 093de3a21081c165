// One lane's share of the verifier's small MSMs (csrc/small_msm_lane.hpp: small_msm_ladder -- what k_batch_small_msm and
// k_small_msm_seg run once per lane) and the shared inversion of k_batch_to_affine (curve.hpp jac_batch_to_aff) compiled for the
// CPU as tests/native/fold_host.cpp compiles the folds: HALO_DEV becomes `inline`, the register pins vanish, everything else is
// the text the device compiler sees.  Built with -fsanitize=address,undefined by tests/test_small_msm_host.py, which writes the
// cases (tests/point_cases.py) and compares the results with the oracle.
//
//   small_msm_host <cases> <results>
//
// <cases>: three 32-bit words (terms, sums, groups); the terms, 12 64-bit words each (arkworks affine point, (0, 0) = infinity,
// then the canonical scalar); per sum a 32-bit K in 1..64 and K term numbers; per group a 32-bit m and m x 12 Jacobian words.
// The ladder runs once per term.  A sum's terms are added with xyzz_add twice: in the order of k_batch_small_msm (64 lanes, lane
// l < off takes lane l + off, off = 32 .. 1; the lanes past K hold the infinity of a dead lane) and in the order of
// k_small_msm_seg (w = 2^ceil(lg K) lanes, every lane takes lane ^ off for off < w).  A group goes through the index map of
// k_batch_to_affine: lane t holds the points t + e stride, e < TBL_E, a point past the end is an infinity, one inversion per lane.
// <results>: per sum 2 x 12 Jacobian words (xyzz_store_jac_words of lane 0), per group m x 8 affine words (aff_store into a
// native table of exactly m entries, then aff_load and aff_to_words as k_native_to_aff).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define HALO_DEV inline
#define HALO_PIN_VGPR(x) ((void)(x))
#include <hip/hip_runtime.h>
static inline int __shfl(int v, int, int) { return v; }  // the cross-lane moves of curve.hpp are not exercised here

#include "small_msm_lane.hpp"

constexpr int TBL_E = 4;  // msm_kernels.hpp (device-only text around it): tests/test_small_msm_host.py holds the two together

template <class T>
static T *aligned(size_t n) {
    void *p = nullptr;
    if (posix_memalign(&p, 16, (n ? n : 1) * sizeof(T))) { fprintf(stderr, "out of memory\n"); exit(2); }
    memset(p, 0, (n ? n : 1) * sizeof(T));
    return static_cast<T *>(p);
}

static bool read_words(FILE *in, void *dst, size_t size, size_t count) { return fread(dst, size, count, in) == count; }

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s <cases> <results>\n", argv[0]); return 2; }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open files\n"); return 2; }
    uint32_t head[3];
    if (!read_words(in, head, 4, 3) || head[0] > (1u << 20) || head[1] > (1u << 20) || head[2] > (1u << 10)) { fprintf(stderr, "bad header\n"); return 2; }
    const uint32_t nterms = head[0], nsums = head[1], ngroups = head[2];
    uint64_t *terms = aligned<uint64_t>((size_t)nterms * 12);
    if (!read_words(in, terms, 8, (size_t)nterms * 12)) { fprintf(stderr, "short terms\n"); return 2; }
    std::vector<halo::XyzzN> prod(nterms);
    for (uint32_t t = 0; t < nterms; t++) {
        halo::AffN p = halo::aff_from_words(terms + 12 * (size_t)t);
        halo::Fe k = halo::fe_load(terms + 12 * (size_t)t + 8);
        prod[t] = halo::jac_to_xyzz(halo::small_msm_ladder(p, k, true));
    }
    const halo::XyzzN dead = halo::jac_to_xyzz(halo::small_msm_ladder(halo::aff_inf(), halo::fe_zero(), false));
    uint64_t res[24];
    for (uint32_t s = 0; s < nsums; s++) {
        uint32_t K, idx[64];
        if (!read_words(in, &K, 4, 1) || K < 1 || K > 64 || !read_words(in, idx, 4, K)) { fprintf(stderr, "bad sum\n"); return 2; }
        for (uint32_t i = 0; i < K; i++)
            if (idx[i] >= nterms) { fprintf(stderr, "bad term number\n"); return 2; }
        // k_batch_small_msm
        halo::XyzzN x[64];
        for (uint32_t l = 0; l < 64; l++) x[l] = l < K ? prod[idx[l]] : dead;
        for (int off = 32; off >= 1; off >>= 1)
            for (int l = 0; l < off; l++) halo::xyzz_add(x[l], x[l + off]);
        halo::xyzz_store_jac_words(res, x[0]);
        // k_small_msm_seg
        uint32_t lgw = 0;
        while ((1u << lgw) < K) ++lgw;
        const uint32_t w = 1u << lgw;
        halo::XyzzN y[64], z[64];
        for (uint32_t l = 0; l < w; l++) y[l] = l < K ? prod[idx[l]] : dead;
        for (int off = 32; off >= 1; off >>= 1) {
            if (!((uint32_t)off < (1u << lgw))) continue;
            for (uint32_t l = 0; l < w; l++) { z[l] = y[l]; halo::xyzz_add(z[l], y[l ^ (uint32_t)off]); }
            for (uint32_t l = 0; l < w; l++) y[l] = z[l];
        }
        halo::xyzz_store_jac_words(res + 12, y[0]);
        if (fwrite(res, 8, 24, out) != 24) { fprintf(stderr, "write failed\n"); return 2; }
    }
    size_t points = 0;
    for (uint32_t g = 0; g < ngroups; g++) {
        uint32_t n;
        if (!read_words(in, &n, 4, 1) || n < 1 || n > (1u << 20)) { fprintf(stderr, "bad group\n"); return 2; }
        uint64_t *jac = aligned<uint64_t>((size_t)n * 12), *aff = aligned<uint64_t>((size_t)n * 8);
        if (!read_words(in, jac, 8, (size_t)n * 12)) { fprintf(stderr, "short group\n"); return 2; }
        uint32_t *native = aligned<uint32_t>((size_t)n * halo::AFF_STRIDE);  // exactly n entries: a store past the end is ASan's to find
        const uint32_t stride = 256u * (((n + TBL_E - 1) / TBL_E + 255u) / 256u);  // batch_to_affine's grid, 256 lanes per block
        for (uint32_t t = 0; t < stride; t++) {
            if (t >= n) continue;
            halo::JacN p[TBL_E];
            for (int e = 0; e < TBL_E; e++) {
                uint32_t i = t + (uint32_t)e * stride;
                p[e] = i < n ? halo::jac_from_words(jac + 12 * (size_t)i) : halo::jac_inf();
            }
            halo::AffN a[TBL_E];
            halo::jac_batch_to_aff(p, a);
            for (int e = 0; e < TBL_E; e++) {
                uint32_t i = t + (uint32_t)e * stride;
                if (i < n) halo::aff_store(native + halo::AFF_STRIDE * (size_t)i, a[e]);
            }
        }
        for (uint32_t i = 0; i < n; i++) halo::aff_to_words(aff + 8 * (size_t)i, halo::aff_load(native + halo::AFF_STRIDE * (size_t)i));
        if (fwrite(aff, 8, (size_t)n * 8, out) != (size_t)n * 8) { fprintf(stderr, "write failed\n"); return 2; }
        points += n;
        free(jac); free(aff); free(native);
    }
    free(terms);
    fclose(in);
    if (fclose(out)) { fprintf(stderr, "write failed\n"); return 2; }
    printf("ok %u terms %u sums %zu points\n", nterms, nsums, points);
    return 0;
}
