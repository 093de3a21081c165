// The lanes of the device transcripts (csrc/keccak_lane.hpp: keccak_f1600; csrc/transcript_lane.hpp: point_compress_lane,
// scalar_ok_lane and the three rho_0 forms -- what k_urs_scalars and the k_transcript_* kernels run once per lane) compiled for the
// CPU as tests/native/small_msm_host.cpp compiles the ladder: HALO_DEV becomes `inline`, everything else is the text the device
// compiler sees.  Built with -fsanitize=address,undefined by tests/test_transcript_host.py, which writes the cases
// (tests/transcript_cases.py) and compares the results with hashlib and the integer model.
//
//   transcript_lane_host <cases> <results>
//
// <cases>: four 32-bit words (permutations, hashes, points, scalars), then 64-bit words:
//   per permutation  25 state words                                            -> 25 words (keccak_f1600)
//   per hash         form, P0 (12 Jacobian words), P1 (12), s0 (4 Montgomery words), s1 (4)
//                      form 0: rho_0(P0, s0, s1)   1: rho_0(P0, s0, s1, P1)   2: rho_0(s0, P0, P1)
//                                                                              -> 4 Montgomery words, then the two points' 5 compressed words
//   per point        12 Jacobian words                                         -> 5 compressed words (verdict in bits 8.. of the last), the verdict
//   per scalar       4 words                                                   -> 1 word (scalar_ok_lane)
// Every buffer is exactly as long as its record and 8-byte aligned only, as an Instance blob's fields are.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define HALO_DEV inline
#define HALO_PIN_VGPR(x) ((void)(x))
#include <hip/hip_runtime.h>

#include "transcript_lane.hpp"

// n words at an address that is 8 mod 16: a 16-byte access would be UBSan's to find, a word past the end ASan's
struct Odd {
    uint64_t *base, *p;
    explicit Odd(size_t n) {
        void *q = nullptr;
        if (posix_memalign(&q, 16, (n + 1) * 8)) { fprintf(stderr, "out of memory\n"); exit(2); }
        base = static_cast<uint64_t *>(q);
        p = base + 1;
    }
    ~Odd() { free(base); }
};

static bool rd(FILE *in, uint64_t *dst, size_t n) { return fread(dst, 8, n, in) == n; }
static bool wr(FILE *out, const uint64_t *src, size_t n) { return fwrite(src, 8, n, out) == n; }

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s <cases> <results>\n", argv[0]); return 2; }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open files\n"); return 2; }
    uint32_t head[4];
    if (fread(head, 4, 4, in) != 4 || head[0] > (1u << 20) || head[1] > (1u << 20) || head[2] > (1u << 20) || head[3] > (1u << 20)) {
        fprintf(stderr, "bad header\n");
        return 2;
    }
    for (uint32_t i = 0; i < head[0]; i++) {
        uint64_t a[25];
        if (!rd(in, a, 25)) { fprintf(stderr, "short permutation\n"); return 2; }
        halo::keccak_f1600(a);
        if (!wr(out, a, 25)) { fprintf(stderr, "write failed\n"); return 2; }
    }
    for (uint32_t i = 0; i < head[1]; i++) {
        Odd rec(33), res(14);
        if (!rd(in, rec.p, 33) || rec.p[0] > 2) { fprintf(stderr, "bad hash record\n"); return 2; }
        uint64_t *c0 = res.p + 4, *c1 = res.p + 9;
        halo::point_compress_lane(rec.p + 1, c0);
        halo::point_compress_lane(rec.p + 13, c1);
        const halo::Fe s0 = halo::fe_load64(rec.p + 25), s1 = halo::fe_load64(rec.p + 29);
        const halo::Fe r = rec.p[0] == 0 ? halo::rho0_C_z_v(c0, s0, s1) : rec.p[0] == 1 ? halo::rho0_C_z_v_Cbar(c0, s0, s1, c1) : halo::rho0_xi_L_R(s0, c0, c1);
        halo::fe_store64(res.p, r);
        if (!wr(out, res.p, 14)) { fprintf(stderr, "write failed\n"); return 2; }
    }
    for (uint32_t i = 0; i < head[2]; i++) {
        Odd rec(12), res(6);
        if (!rd(in, rec.p, 12)) { fprintf(stderr, "short point\n"); return 2; }
        res.p[5] = halo::point_compress_lane(rec.p, res.p);
        if (!wr(out, res.p, 6)) { fprintf(stderr, "write failed\n"); return 2; }
    }
    for (uint32_t i = 0; i < head[3]; i++) {
        Odd rec(4);
        if (!rd(in, rec.p, 4)) { fprintf(stderr, "short scalar\n"); return 2; }
        const uint64_t ok = halo::scalar_ok_lane(halo::fe_load64(rec.p)) ? 1 : 0;
        if (!wr(out, &ok, 1)) { fprintf(stderr, "write failed\n"); return 2; }
    }
    fclose(in);
    if (fclose(out)) { fprintf(stderr, "write failed\n"); return 2; }
    printf("ok %u permutations %u hashes %u points %u scalars\n", head[0], head[1], head[2], head[3]);
    return 0;
}
