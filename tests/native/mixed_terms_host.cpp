// The per-member function of the mixed fused check batch's term kernel (csrc/mixed_terms_lane.hpp: mixed_terms_member -- what
// k_mixed_terms runs once per lane) compiled for the CPU as tests/native/fused_lane_host.cpp compiles the lane under it: HALO_DEV
// becomes `inline`, the register pins vanish, everything else is the text the device compiler sees.  Built with
// -fsanitize=address,undefined by tests/test_mixed_terms_host.py, which writes the cases and checks every output word against
// Python integers.
//
//   mixed_terms_host <cases> <results>
//
// <cases>: one 32-bit word (sets); per set a 32-bit member count M, M 32-bit lgs in 1..24, and the members' records one behind the
// other, (lg + 6) x 4 64-bit words each (xi_0 .. xi_lg | z | v | c | r | s, Montgomery).
// <results>: per set the members' scalars one behind the other, (2 lg + 2) x 4 words each, then M x 4 words of shares.  The
// descriptors come from the product's own mixed_terms_describe.  Records, descriptors, scalars and shares are heap blocks of
// exactly the needed size, so a lane that follows a wrong offset -- into a neighbour's words or past the end -- is ASan's to find
// or leaves a wrong word for the test.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#define HALO_DEV inline
#define HALO_PIN_VGPR(x) ((void)(x))
#include <hip/hip_runtime.h>
static inline int __shfl(int v, int, int) { return v; }  // the cross-lane moves of fr29.hpp are not exercised here

#include "mixed_terms_lane.hpp"

template <class T>
static T *exactly(size_t n) {
    T *p = static_cast<T *>(malloc(n * sizeof(T)));
    if (!p) { fprintf(stderr, "out of memory\n"); exit(2); }
    memset(p, 0xa5, n * sizeof(T));
    return p;
}

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s <cases> <results>\n", argv[0]); return 2; }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open files\n"); return 2; }
    uint32_t sets;
    if (fread(&sets, 4, 1, in) != 1 || sets > 1024) { fprintf(stderr, "bad header\n"); return 2; }
    size_t members = 0;
    for (uint32_t s = 0; s < sets; s++) {
        uint32_t M;
        if (fread(&M, 4, 1, in) != 1 || M < 1 || M > 65535) { fprintf(stderr, "bad set\n"); return 2; }
        uint32_t *lgs = exactly<uint32_t>(M), *desc = exactly<uint32_t>((size_t)M * halo::MIXED_DESC_WORDS);
        if (fread(lgs, 4, M, in) != M) { fprintf(stderr, "short set\n"); return 2; }
        for (uint32_t a = 0; a < M; a++)
            if (lgs[a] < 1 || lgs[a] > (uint32_t)halo::FUSED_MAX_LG) { fprintf(stderr, "bad lg\n"); return 2; }
        size_t rw = 0, terms = 0;
        halo::mixed_terms_describe(lgs, M, desc, &rw, &terms);
        uint64_t *recs = exactly<uint64_t>(rw), *sc = exactly<uint64_t>(terms * 4), *shares = exactly<uint64_t>((size_t)M * 4);
        if (fread(recs, 8, rw, in) != rw) { fprintf(stderr, "short records\n"); return 2; }
        for (uint32_t k = 0; k < M; k++) {
            const uint32_t a = M - 1 - k;  // (no member leans on one in front of it having run)
            halo::mixed_terms_member(recs, desc, a, sc, shares);
        }
        if (fwrite(sc, 8, terms * 4, out) != terms * 4 || fwrite(shares, 8, (size_t)M * 4, out) != (size_t)M * 4) { fprintf(stderr, "write failed\n"); return 2; }
        free(lgs); free(desc); free(recs); free(sc); free(shares);
        members += M;
    }
    fclose(in);
    if (fclose(out)) { fprintf(stderr, "write failed\n"); return 2; }
    printf("ok %u sets %zu members\n", sets, members);
    return 0;
}
