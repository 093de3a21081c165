// The term scalars of the mixed fused check batch (halo_pcdl_check_batch_mixed_fused): one lane per member runs
// mixed_terms_lane.hpp -- fused_lane.hpp's lane on the member's own record, at the member's own lg.  fused_check.hip's fused_terms
// launches it when it is given descriptors, and sums H's shares behind it as it does for the uniform kernel.
#include "mixed_terms_lane.hpp"
#include "internal.hpp"

namespace halo {

// recs / scalars: the M members' dense records and dense scalars, desc: their descriptors (mixed_terms_lane.hpp); shares: M x 4
// words.  One lane per member, blocks of one wave, no LDS; every lane touches its own words only.  The lanes of a wave run
// fused_terms_lane at different lg: the one inversion is common to them, the three short loops run to the largest lg of the wave
// with the shorter lanes masked off (~6 products per step of lg).  The members are launched in the caller's order, unsorted.
__global__ __launch_bounds__(64) void k_mixed_terms(const uint64_t *__restrict__ recs, const uint32_t *__restrict__ desc, uint32_t M, uint64_t *scalars,
                                                    uint64_t *shares) {
    const uint32_t a = blockIdx.x * 64 + threadIdx.x;
    if (a >= M) return;
    mixed_terms_member(recs, desc, a, scalars, shares);
}

// On ctx->stream; 1 <= M <= 65535 and every lg in 1 .. FUSED_MAX_LG are the caller's (fused_terms) to check
int mixed_terms_launch(halo_ctx *ctx, const uint64_t *d_recs, const uint32_t *d_desc, size_t M, uint64_t *d_scalars, uint64_t *d_shares) {
    HALO_LAUNCH(ctx, "k_mixed_terms", k_mixed_terms, dim3((unsigned)((M + 63) / 64)), dim3(64), 0, d_recs, d_desc, (uint32_t)M, d_scalars, d_shares);
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}

}  // namespace halo
