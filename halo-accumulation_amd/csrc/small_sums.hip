// The verifier's small sums: independent sums of at most 64 scalar multiples each.  One lane per term runs the ladder of
// small_msm_lane.hpp, then a shuffle tree folds the lanes of a sum.
#include <algorithm>

#include "internal.hpp"
#include "small_msm_lane.hpp"

namespace halo {

// ------------------------------------------------------------------ batched verifier relation
// m independent sums of K <= 64 scalar multiples each (the 2 lg n + 2 terms of one pcdl::succinct_check, pcdl.rs:288-310):
// one wave per sum, one lane per term.  Every lane runs the ladder, then the wave folds its lanes with a shuffle tree.
// points: m x K x 8 words (arkworks affine, (0, 0) = infinity); scalars: m x K x 4 words, CANONICAL (not Montgomery).
__global__ __launch_bounds__(64) void k_batch_small_msm(const uint64_t *__restrict__ points, const uint64_t *__restrict__ scalars, uint32_t K,
                                                        uint64_t *__restrict__ out) {
    uint32_t inst = blockIdx.x, lane = threadIdx.x;
    bool live = lane < K;
    size_t t = (size_t)inst * K + (live ? lane : 0);
    AffN p = live ? aff_from_words(points + 8 * t) : aff_inf();
    Fe k = fe_load(scalars + 4 * t);
    JacN acc = small_msm_ladder(p, k, live);
    XyzzN x = jac_to_xyzz(acc);
#pragma unroll 1
    for (int off = 32; off >= 1; off >>= 1) {
        XyzzN o = xyzz_shfl(x, (int)((lane + off) & 63));
        if ((int)lane < off) xyzz_add(x, o);
    }
    if (lane == 0) xyzz_store_jac_words(out + 12 * (size_t)inst, x);
}
int batch_small_msm(halo_ctx *ctx, const uint64_t *d_points, const uint64_t *d_scalars, size_t m, size_t K, uint64_t *d_out) {
    if (m == 0) return HALO_OK;
    if (K == 0 || K > 64) { set_error("batch_small_msm: 1..64 terms per sum"); return HALO_E_ARG; }
    HALO_LAUNCH(ctx, "k_batch_small_msm", k_batch_small_msm, dim3((unsigned)m), dim3(64), 0, d_points, d_scalars, (uint32_t)K, d_out);
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}

// Sums of 1..64 terms of different lengths, several to a wave (the relations and the member sums of halo_acc_verifier_batch).
// A sum of L terms owns a segment of w = 2^ceil(lg L) lanes that starts at a lane divisible by w, so every xor partner of the
// shuffle tree below w lies inside it; one lane per term runs the ladder, the segment folds itself in lg w xor steps (every
// lane ends with the segment's sum) and its first lane writes the Jacobian words.  desc: 64 words per wave, one per lane,
// (sum index + 1) << 3 | lg w, 0 for an idle lane (small_msm_seg_plan); sum_off: nsums + 1 term offsets.
// points / scalars: the terms sum after sum, 8 words arkworks affine ((0, 0) = infinity) / 4 words canonical.
__global__ __launch_bounds__(64) void k_small_msm_seg(const uint64_t *__restrict__ points, const uint64_t *__restrict__ scalars,
                                                      const uint32_t *__restrict__ sum_off, const uint32_t *__restrict__ desc,
                                                      uint64_t *__restrict__ out) {
    const uint32_t lane = threadIdx.x, e = desc[64 * (size_t)blockIdx.x + lane];
    const uint32_t lgw = e & 7u, pos = lane & ((1u << lgw) - 1u);
    uint32_t s = 0, t = 0;
    bool live = false;
    if (e) {
        s = (e >> 3) - 1u;
        t = sum_off[s] + pos;
        live = t < sum_off[s + 1];
    }
    AffN p = live ? aff_from_words(points + 8 * (size_t)t) : aff_inf();
    Fe k = live ? fe_load(scalars + 4 * (size_t)t) : fe_zero();
    JacN acc = small_msm_ladder(p, k, live);
    XyzzN x = jac_to_xyzz(acc);
#pragma unroll 1
    for (int off = 32; off >= 1; off >>= 1) {
        XyzzN o = xyzz_shfl(x, (int)(lane ^ (uint32_t)off));  // (every lane takes part: the partner's registers are read)
        if ((uint32_t)off < (1u << lgw)) xyzz_add(x, o);
    }
    if (e && pos == 0) xyzz_store_jac_words(out + 12 * (size_t)s, x);
}
size_t small_msm_seg_plan(const uint32_t *sum_off, size_t nsums, std::vector<uint32_t> &desc) {
    std::vector<std::pair<uint32_t, uint32_t>> by_width(nsums);  // (lg w, sum), widest first, in sum order within a width
    for (size_t s = 0; s < nsums; ++s) {
        uint32_t len = sum_off[s + 1] - sum_off[s], lgw = 0;
        while ((1u << lgw) < len) ++lgw;
        by_width[s] = {lgw, (uint32_t)s};
    }
    std::stable_sort(by_width.begin(), by_width.end(), [](const auto &a, const auto &b) { return a.first > b.first; });
    // powers of two in falling order: every segment starts at a multiple of its width and only the last wave has idle lanes
    size_t lanes = 0;
    for (auto &e : by_width) lanes += (size_t)1 << e.first;
    desc.assign((lanes + 63) / 64 * 64, 0u);
    size_t at = 0;
    for (auto &e : by_width) {
        const uint32_t code = (e.second + 1u) << 3 | e.first;
        for (size_t l = 0; l < ((size_t)1 << e.first); ++l) desc[at + l] = code;
        at += (size_t)1 << e.first;
    }
    return desc.size() / 64;
}
int small_msm_seg(halo_ctx *ctx, const uint64_t *d_points, const uint64_t *d_scalars, const uint32_t *d_sum_off, const uint32_t *d_desc, size_t waves,
                  uint64_t *d_out) {
    if (waves == 0) return HALO_OK;
    HALO_LAUNCH(ctx, "k_small_msm_seg", k_small_msm_seg, dim3((unsigned)waves), dim3(64), 0, d_points, d_scalars, d_sum_off, d_desc, d_out);
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}

}  // namespace halo
