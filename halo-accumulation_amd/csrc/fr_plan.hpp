// The launch plan of the scalar-side kernels of fr_vec.hip and hpoly.hip (K4 - K9): chain length, window count, grid and trips per lane as
// functions of the size.  Host code only.  The launchers there take their numbers from the plan_* functions below and
// halo_dev_fr_plan (dev.hip) reports the same functions' results: a test that asserts a plan asserts what the launcher runs.
//
// Every plan gives the same field elements (the sums are exact); the development hooks "pow_e", "dot_blocks" and
// "poly_blocks" (tuning.hpp DevHooks) come first, then the environment (HALO_POW_E, HALO_DOT_BLOCKS), then the measured default.
#pragma once
#include <cstddef>

#include "internal.hpp"

namespace halo {

// elements per lane: a longer chain spreads the seed (nwin - 1 products) over more elements, a shorter one puts more
// waves on the chip; measured at n = 2^20 (tools/fr_kernels.py with HALO_POW_E = 2 .. 32): k_powers 8, k_poly_eval_partial
// 16, k_h_coeffs 4 (its "seed" is one product per four elements whatever the length)
constexpr int POWERS_E = 8;      // elements per lane of k_powers
constexpr int POLY_EVAL_E = 16;  // coefficients per lane of k_poly_eval_partial
constexpr int H_COEFFS_E = 4;    // coefficients per lane of k_h_coeffs / k_h_accumulate_batch

static inline int pow_chain_len(size_t n, int best) {
    // development overrides: a power of two in [4, 64] (validated where they are set) -- k_h_coeffs relies on a chain length
    // that is a power of two (its mid * high factor is wave-uniform and changes every fourth step): another value would give
    // wrong coefficients
    const int forced = dev_hooks().pow_e > 0 ? dev_hooks().pow_e : tuning().pow_e;
    if (forced > 0) return forced;
    int e = best;
    while (e > 4 && n / (64 * (size_t)e) < 1024) e >>= 1;  // small inputs: at least a wave per SIMD
    return e;
}
static inline int bits_for(size_t n) {
    int b = 0;
    while (((size_t)1 << b) < n) b++;
    return b < 1 ? 1 : b;
}
static inline int window_count(size_t n) { return (bits_for(n) + 3) / 4; }  // 4-bit windows of the exponents below n
static inline unsigned wave_blocks(size_t n, int E) {  // blocks of 4 waves, a wave per 64 * E elements
    size_t waves = (n + 64 * (size_t)E - 1) / (64 * (size_t)E);
    return (unsigned)((waves + 3) / 4);
}
// two elements per lane and trip, at most 512 blocks (two waves per SIMD): the lanes of a large dot product run several trips
static inline unsigned dot_blocks(size_t m) {
    const int forced = dev_hooks().dot_blocks > 0 ? dev_hooks().dot_blocks : tuning().dot_blocks;  // (both in [1, FR_GRID_CAP])
    size_t nb = ((m + 1) / 2 + 255) / 256, cap = forced > 0 ? (size_t)forced : 512;
    if (nb > cap) nb = cap;
    if (nb == 0) nb = 1;
    return (unsigned)nb;
}
// the grid of k_poly_eval_partial: a wave per 64 * E coefficients up to the cap, then the waves stride over the rest
static inline unsigned poly_blocks(size_t len, int E, size_t limit) {
    size_t nb = wave_blocks(len, E), cap = dev_hooks().poly_blocks > 0 ? (size_t)dev_hooks().poly_blocks : FR_GRID_CAP;
    if (cap > limit) cap = limit;
    if (nb > cap) nb = cap;
    if (nb == 0) nb = 1;
    return (unsigned)nb;
}

// trips: the most passes any lane makes through its kernel's outer loop (1: no lane comes back for more)
struct FrPlan { int E, nwin; unsigned blocks; size_t trips; };

static inline FrPlan plan_powers(size_t n) {
    FrPlan p;
    p.E = pow_chain_len(n, POWERS_E);
    p.nwin = window_count(n);
    p.blocks = wave_blocks(n, p.E);
    p.trips = 1;
    return p;
}
// limit: the partial records the caller has room for
static inline FrPlan plan_poly_eval(size_t len, size_t limit = FR_GRID_CAP) {
    FrPlan p;
    p.E = pow_chain_len(len, POLY_EVAL_E);
    p.nwin = window_count(len);
    p.blocks = poly_blocks(len, p.E, limit);
    const size_t waves = (len + 64 * (size_t)p.E - 1) / (64 * (size_t)p.E), per_trip = 4 * (size_t)p.blocks;
    p.trips = waves ? (waves + per_trip - 1) / per_trip : 1;
    return p;
}
// the batched open's p(z) (open_batch_table, open_batch_eval): a member has room for OPEN_PART_WORDS / 4 partial records
static inline FrPlan plan_poly_eval_batch(size_t len) { return plan_poly_eval(len, OPEN_PART_WORDS / 4); }
static inline FrPlan plan_dot(size_t m) {
    FrPlan p;
    p.E = 2;  // two elements per lane and trip
    p.nwin = 0;
    p.blocks = dot_blocks(m);
    const size_t per_trip = 2 * 256 * (size_t)p.blocks;
    p.trips = m ? (m + per_trip - 1) / per_trip : 1;
    return p;
}
// n = 2^lg_n coefficients; nwin: the 256-entry tables (low, mid, high) that hold more than one entry
static inline FrPlan plan_h_coeffs(size_t n) {
    FrPlan p;
    p.E = pow_chain_len(n, H_COEFFS_E);
    const int lg = bits_for(n);
    p.nwin = n < 2 ? 0 : (lg + 7) / 8;
    p.blocks = wave_blocks(n, p.E);
    p.trips = 1;
    return p;
}

enum { FR_PLAN_POWERS = 0, FR_PLAN_POLY_EVAL = 1, FR_PLAN_DOT = 2, FR_PLAN_H_COEFFS = 3, FR_PLAN_POLY_EVAL_BATCH = 4 };
static inline bool fr_plan(int which, size_t n, FrPlan *out) {
    switch (which) {
        case FR_PLAN_POWERS: *out = plan_powers(n); return true;
        case FR_PLAN_POLY_EVAL: *out = plan_poly_eval(n); return true;
        case FR_PLAN_DOT: *out = plan_dot(n); return true;
        case FR_PLAN_H_COEFFS: *out = plan_h_coeffs(n); return true;
        case FR_PLAN_POLY_EVAL_BATCH: *out = plan_poly_eval_batch(n); return true;
        default: return false;
    }
}

}  // namespace halo
