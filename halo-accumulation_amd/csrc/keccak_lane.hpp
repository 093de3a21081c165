// Keccak-f[1600] for one lane, the 25 lanes of the state in registers: what a one-block SHA3-256 (rate 136 bytes) is made of.
// k_urs_scalars (urs.hip: the generators' scalars) and the transcript lanes (transcript_lane.hpp: rho_0) call it;
// tests/native/transcript_lane_host.cpp compiles the same text for the CPU (HALO_DEV = inline) and runs it under ASan + UBSan.
// No LDS, no scratch: the rotation and lane tables are compile-time, the round constant is selected, not indexed.
#pragma once
#include "field.hpp"

namespace halo {

HALO_DEV uint64_t rol64(uint64_t x, int n) { return (x << n) | (x >> (64 - n)); }

HALO_DEV void keccak_f1600(uint64_t (&a)[25]) {
    constexpr uint64_t RC[24] = {0x0000000000000001ULL, 0x0000000000008082ULL, 0x800000000000808aULL, 0x8000000080008000ULL, 0x000000000000808bULL,
                                 0x0000000080000001ULL, 0x8000000080008081ULL, 0x8000000000008009ULL, 0x000000000000008aULL, 0x0000000000000088ULL,
                                 0x0000000080008009ULL, 0x000000008000000aULL, 0x000000008000808bULL, 0x800000000000008bULL, 0x8000000000008089ULL,
                                 0x8000000000008003ULL, 0x8000000000008002ULL, 0x8000000000000080ULL, 0x000000000000800aULL, 0x800000008000000aULL,
                                 0x8000000080008081ULL, 0x8000000000008080ULL, 0x0000000080000001ULL, 0x8000000080008008ULL};
    constexpr int ROT[24] = {1, 3, 6, 10, 15, 21, 28, 36, 45, 55, 2, 14, 27, 41, 56, 8, 25, 43, 62, 18, 39, 61, 20, 44};
    constexpr int PIL[24] = {10, 7, 11, 17, 18, 3, 5, 16, 8, 21, 24, 4, 15, 23, 19, 13, 12, 2, 20, 14, 22, 9, 6, 1};
#pragma unroll 1
    for (int r = 0; r < 24; r++) {
        uint64_t c[5], t, bc;
#pragma unroll
        for (int x = 0; x < 5; x++) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
#pragma unroll
        for (int x = 0; x < 5; x++) {
            t = c[(x + 4) % 5] ^ rol64(c[(x + 1) % 5], 1);
#pragma unroll
            for (int y = 0; y < 25; y += 5) a[y + x] ^= t;
        }
        t = a[1];
#pragma unroll
        for (int k = 0; k < 24; k++) {
            bc = a[PIL[k]];
            a[PIL[k]] = rol64(t, ROT[k]);
            t = bc;
        }
#pragma unroll
        for (int y = 0; y < 25; y += 5) {
            uint64_t b0 = a[y], b1 = a[y + 1], b2 = a[y + 2], b3 = a[y + 3], b4 = a[y + 4];
            a[y] = b0 ^ (~b1 & b2); a[y + 1] = b1 ^ (~b2 & b3); a[y + 2] = b2 ^ (~b3 & b4); a[y + 3] = b3 ^ (~b4 & b0); a[y + 4] = b4 ^ (~b0 & b1);
        }
        uint64_t rc = 0;
#pragma unroll
        for (int q = 0; q < 24; q++) rc = (q == r) ? RC[q] : rc;  // (no runtime-indexed constant array: that would live in scratch)
        a[0] ^= rc;
    }
}

// the first 32 bytes of the state read as a little-endian integer mod r (ark-ff from_le_bytes_mod_order), canonical words
HALO_DEV Fe keccak_digest_mod_r(const uint64_t (&a)[25]) {
    Fe v;
#pragma unroll
    for (int k = 0; k < 4; k++) { v.v[2 * k] = (uint32_t)a[k]; v.v[2 * k + 1] = (uint32_t)(a[k] >> 32); }
    // 2^256 < 4 r: at most three subtractions bring the digest below r
#pragma unroll 1
    for (int q = 0; q < 3; q++) fe_cond_sub<FrCfg>(v);
    return v;
}

}  // namespace halo
