// One lane's share of the sliding odd-digit recode of the all-shifts table plan (msm_table.hip k_tmsm_recode, TblPlan::slide):
// a canonical scalar s < r is written as s = sum_k d_k 2^(j_k) with every d_k odd, |d_k| < 2^(wmax - 1), at most SLIDE_SLOTS
// digits and j_k + w_k <= 255.  A window starts only at a set bit, so runs of zero bits cost nothing: 12.0 digits on average for
// uniform scalars at wmax = 21, against the 13 fixed 20-bit windows of the 13-row plan.  The table holds 2^j G_i for EVERY j, so
// digit k sends row j_k of point i to bucket (|d_k| - 1) / 2.
// tests/native/slide_host.cpp compiles the same text for the CPU (HALO_DEV = inline) and runs it under ASan + UBSan.  Needs no
// other header of the library.
#pragma once
#include <cstdint>

#ifndef HALO_DEV
#define HALO_DEV __device__ __forceinline__
#endif

namespace halo {

constexpr int SLIDE_SLOTS = 13;  // digit slots per scalar (the rows of the digit array: as many as the 13-row plan has windows)
constexpr int SLIDE_BITS = 255;  // no window reaches past this bit: r < 2^255, and the table has rows 0 .. 254

// the scalar field's modulus, 32-bit words (fr29.hpp / field.hpp FrCfg::P, repeated so that the header stands alone)
HALO_DEV uint32_t slide_r_word(int k) {
    constexpr uint32_t R[8] = {0x00000001u, 0x8c46eb21u, 0x0994a8ddu, 0x224698fcu, 0x00000000u, 0x00000000u, 0x00000000u, 0x40000000u};
    return R[k];
}
// w[0..8) -= r while w >= r (an input below 2^256 is below 4 r: three rounds at most); w[8] = 0
HALO_DEV void slide_canon(uint32_t *w) {
    for (int round = 0; round < 3; round++) {
        bool ge = true;
        for (int k = 7; k >= 0; k--) {
            uint32_t p = slide_r_word(k);
            if (w[k] != p) { ge = w[k] > p; break; }
        }
        if (!ge) break;
        uint64_t borrow = 0;
        for (int k = 0; k < 8; k++) {
            uint64_t d = (uint64_t)w[k] - slide_r_word(k) - borrow;
            w[k] = (uint32_t)d;
            borrow = (d >> 32) & 1u;
        }
    }
    w[8] = 0;
}
HALO_DEV int slide_ctz(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __ffs((int)x) - 1;
#else
    return __builtin_ctz(x);
#endif
}
// Width of the window that starts with R = 255 - j bits left (1 <= R <= 255): R <= wmax takes them all (the last window: unsigned,
// nothing above it could take a carry); otherwise the R bits and a possible carry are planned as q = ceil((R + 1) / (wmax + 1))
// windows of equal width min(wmax, ceil((R + 1) / q) - 1): the windows shrink a little near the top instead of leaving a short
// fourteenth one.  (Two divisions: the kernel looks the width up in a table of 256 bytes that its block fills with this function.)
HALO_DEV int slide_width(int R, int wmax) {
    if (R <= wmax) return R;
    int q = (R + 1 + wmax) / (wmax + 1);
    int width = (R + q) / q - 1;  // ceil((R + 1) / q) - 1
    return width > wmax ? wmax : width;
}
// The recode of the canonical scalar in w[0..9) (w[8] = 0; the words are used up).  wtab[R] = slide_width(R, wmax) for R = 1 .. 255.
// emit(k, mag, neg, row) is called once per digit, k = 0, 1, ...: digit (neg ? -mag : mag) at bit `row`.  Returns the number of digits.
//   * trailing zero bits are skipped;
//   * the digit is the signed residue of the value mod 2^width: a window whose top bit is set gives d - 2^width and carries
//     2^(j + width) into the words (never the last window).  The low bit of a window is set, so d is odd, and
//     |d| < 2^(width - 1) <= 2^(wmax - 1).
template <class Emit>
HALO_DEV int slide_recode(uint32_t *w, int wmax, const uint8_t *wtab, Emit &&emit) {
    int j = 0, cnt = 0;
    for (;;) {
        while (j < SLIDE_BITS) {  // the next set bit at or above j
            uint32_t x = w[j >> 5] >> (j & 31);
            if (x) { j += slide_ctz(x); break; }
            j = (j | 31) + 1;
        }
        if (j >= SLIDE_BITS) break;
        const int R = SLIDE_BITS - j;
        const bool last = R <= wmax;
        const int width = wtab[R];
        const int word = j >> 5, sh = j & 31;
        uint64_t two = (uint64_t)w[word] | ((uint64_t)w[word + 1] << 32);
        uint32_t raw = (uint32_t)(two >> sh) & ((1u << width) - 1u);
        uint32_t neg = (!last && ((raw >> (width - 1)) & 1u)) ? 1u : 0u;
        uint32_t mag = neg ? (1u << width) - raw : raw;
        if (neg) {  // + 2^(j + width): j + width <= 254 here, the carry stays inside the nine words
            int at = j + width;
            uint32_t add = 1u << (at & 31);
            for (int k = at >> 5; k < 9 && add; k++) {
                uint32_t old = w[k];
                w[k] = old + add;
                add = w[k] < old ? 1u : 0u;
            }
        }
        emit(cnt, mag, neg, (uint32_t)j);
        cnt++;
        j += width;
    }
    return cnt;
}

}  // namespace halo
