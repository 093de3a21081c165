// The device code of the wire format's point decompression (csrc/decompress.hpp: the square root in Fq and one point's
// record), compiled for the CPU: HALO_DEV becomes `inline` and the register pins vanish, everything else is the text the
// device compiler sees.  Built with -fsanitize=address,undefined by tests/test_decompress_host.py, which gives it the
// library's tables and compares its records with the host decoder's and its roots with Python integers.  No HIP call is
// made: the HIP headers are included for their types (uint4, make_uint4).
//
//   decompress_host <mode> <tables> <in> <out>
//
// <tables>: SQRT_TABLE_WORDS 32-bit words.  mode 0: <in> = records of 6 64-bit words (a point's 33 wire bytes, zero-padded),
// <out> = records of 14 words.  mode 1: <in> = field elements (4 Montgomery words), <out> = root (4 words), ok, 0 per element.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#define HALO_DEV inline
#define HALO_PIN_VGPR(x) ((void)(x))
#include <hip/hip_runtime.h>

#include "decompress.hpp"

static void *aligned(size_t bytes) {
    void *p = nullptr;
    if (posix_memalign(&p, 16, bytes ? bytes : 16)) { fprintf(stderr, "out of memory\n"); exit(2); }
    memset(p, 0, bytes ? bytes : 16);
    return p;
}

int main(int argc, char **argv) {
    if (argc != 5) { fprintf(stderr, "usage: %s <mode> <tables> <in> <out>\n", argv[0]); return 2; }
    const int mode = atoi(argv[1]);
    FILE *ft = fopen(argv[2], "rb"), *in = fopen(argv[3], "rb"), *out = fopen(argv[4], "wb");
    if (!ft || !in || !out || mode < 0 || mode > 1) { fprintf(stderr, "cannot open files\n"); return 2; }
    uint4 *tab = static_cast<uint4 *>(aligned(halo::SQRT_TABLE_WORDS * 4));
    if (fread(tab, 4, halo::SQRT_TABLE_WORDS, ft) != halo::SQRT_TABLE_WORDS) { fprintf(stderr, "short table file\n"); return 2; }
    const size_t iw = mode == 0 ? halo::DECOMP_REC_IN : 4, ow = mode == 0 ? halo::DECOMP_REC_OUT : 6;
    uint64_t *rec = static_cast<uint64_t *>(aligned(iw * 8)), *res = static_cast<uint64_t *>(aligned(ow * 8));
    size_t n = 0;
    while (fread(rec, 8, iw, in) == iw) {
        if (mode == 0) {
            halo::decompress_one(rec, tab, res);
        } else {
            bool ok;
            halo::fe_store(res, halo::fq_sqrt(halo::fe_load(rec), tab, &ok));
            res[4] = ok ? 1 : 0;
            res[5] = 0;
        }
        if (fwrite(res, 8, ow, out) != ow) { fprintf(stderr, "write failed\n"); return 2; }
        ++n;
    }
    fclose(out);
    fclose(in);
    fclose(ft);
    free(rec);
    free(res);
    free(tab);
    printf("%zu records\n", n);
    return 0;
}
