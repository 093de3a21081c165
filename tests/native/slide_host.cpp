// The lane function of the sliding odd-digit recode (csrc/slide_lane.hpp: slide_canon, slide_recode -- what k_tmsm_recode runs per
// scalar under the all-shifts table plan) compiled for the CPU, for ASan + UBSan.  tests/test_slide_recode_host.py feeds it scalars
// (8 little-endian 32-bit words each) and checks the digits it writes back: per scalar 1 + 3 * SLIDE_SLOTS words -- the digit
// count, then (magnitude, sign, row) per slot, zero for an unused slot.
#include <cstdio>
#include <cstdlib>
#include <vector>

#define HALO_DEV inline
#include "slide_lane.hpp"

int main(int argc, char **argv) {
    if (argc != 4) { fprintf(stderr, "usage: slide_host <wmax> <in> <out>\n"); return 2; }
    const int wmax = atoi(argv[1]);
    FILE *fi = fopen(argv[2], "rb"), *fo = fopen(argv[3], "wb");
    if (!fi || !fo || wmax < 2 || wmax > 21) { fprintf(stderr, "slide_host: bad arguments\n"); return 2; }
    constexpr int REC = 1 + 3 * halo::SLIDE_SLOTS;
    uint8_t wtab[256] = {0};
    for (int R = 1; R < 256; R++) wtab[R] = (uint8_t)halo::slide_width(R, wmax);
    uint32_t in[8];
    size_t count = 0;
    while (fread(in, 4, 8, fi) == 8) {
        uint32_t w[9];
        for (int k = 0; k < 8; k++) w[k] = in[k];
        w[8] = 0;
        halo::slide_canon(w);
        std::vector<uint32_t> rec(REC, 0u);
        int overflow = 0;
        int n = halo::slide_recode(w, wmax, wtab, [&](int k, uint32_t mag, uint32_t neg, uint32_t row) {
            if (k >= halo::SLIDE_SLOTS) { overflow = 1; return; }
            rec[1 + 3 * k] = mag; rec[2 + 3 * k] = neg; rec[3 + 3 * k] = row;
        });
        rec[0] = (uint32_t)n;
        (void)overflow;  // (the count says it: the test asserts n <= SLIDE_SLOTS)
        if (fwrite(rec.data(), 4, REC, fo) != (size_t)REC) return 3;
        count++;
    }
    fclose(fi);
    if (fclose(fo)) return 3;
    printf("ok %zu\n", count);
    return 0;
}
