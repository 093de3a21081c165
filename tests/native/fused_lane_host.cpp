// One lane of the fused check batch's term kernel (csrc/fused_lane.hpp: fused_terms_lane -- what k_fused_terms runs once per lane)
// and the field inversion under it (csrc/fr29.hpp: fs_inv) compiled for the CPU as tests/native/small_msm_host.cpp compiles the
// ladders: HALO_DEV becomes `inline`, the register pins vanish, everything else is the text the device compiler sees.  Built with
// -fsanitize=address,undefined by tests/test_fused_lane_host.py, which writes the cases and checks every output word against
// Python integers.
//
//   fused_lane_host <cases> <results>
//
// <cases>: two 32-bit words (lanes, inversions); per lane a 32-bit lg in 1..24 and its record of (lg + 6) x 4 64-bit words
// (xi_0 .. xi_lg | z | v | c | r | s, Montgomery); per inversion nine 32-bit limbs of 29 bits, a value below 60 r (the widest
// bound fs_inv admits).
// <results>: per lane (2 lg + 2) x 4 words of scalars and 4 words of H's share -- each buffer allocated at exactly its size, so a
// store or a load past it is ASan's to find; per inversion the nine limbs of fs_inv's result and its 4 canonical words.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#define HALO_DEV inline
#define HALO_PIN_VGPR(x) ((void)(x))
#include <hip/hip_runtime.h>
static inline int __shfl(int v, int, int) { return v; }  // the cross-lane moves of fr29.hpp are not exercised here

#include "fused_lane.hpp"

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
    uint32_t head[2];
    if (fread(head, 4, 2, in) != 2 || head[0] > (1u << 20) || head[1] > (1u << 20)) { fprintf(stderr, "bad header\n"); return 2; }
    for (uint32_t i = 0; i < head[0]; i++) {
        uint32_t lg;
        if (fread(&lg, 4, 1, in) != 1 || lg < 1 || lg > (uint32_t)halo::FUSED_MAX_LG) { fprintf(stderr, "bad lane\n"); return 2; }
        const size_t rw = halo::fused_rec_words((int)lg), sw = halo::fused_term_count((int)lg) * 4;
        uint64_t *rec = exactly<uint64_t>(rw), *sc = exactly<uint64_t>(sw), *share = exactly<uint64_t>(4);
        if (fread(rec, 8, rw, in) != rw) { fprintf(stderr, "short record\n"); return 2; }
        halo::fused_terms_lane(rec, (int)lg, sc, share);
        if (fwrite(sc, 8, sw, out) != sw || fwrite(share, 8, 4, out) != 4) { fprintf(stderr, "write failed\n"); return 2; }
        free(rec); free(sc); free(share);
    }
    for (uint32_t i = 0; i < head[1]; i++) {
        halo::Fs<60> x;
        if (fread(x.v, 4, 9, in) != 9) { fprintf(stderr, "short inversion\n"); return 2; }
        const halo::Fs<2> y = halo::fs_inv(x);
        alignas(16) uint64_t canon[4];
        halo::fs_store(canon, y);
        if (fwrite(y.v, 4, 9, out) != 9 || fwrite(canon, 8, 4, out) != 4) { fprintf(stderr, "write failed\n"); return 2; }
    }
    fclose(in);
    if (fclose(out)) { fprintf(stderr, "write failed\n"); return 2; }
    printf("ok %u lanes %u inversions\n", head[0], head[1]);
    return 0;
}
