// The term scalars of the fused check batch (halo_pcdl_check_batch_fused): one lane per member runs fused_lane.hpp, then the
// members' shares of H's scalar are summed on the device (k_fr_sum_rows).  The host does no field arithmetic per member beyond the
// transcripts and the weights; pcdl_batch.hip check_members_fused feeds the scalars to the left side's MSMs where they lie.  The
// mixed fused check batch (members of their own sizes) has a kernel of its own, mixed_terms.hip, behind the same launcher.
#include "fused_lane.hpp"
#include "internal.hpp"

namespace halo {

// recs: M records of fused_rec_words(lg); scalars: member a's 2 lg + 2 canonical scalars at a x (2 lg + 2) x 4 words; shares: M x 4
// words, member a's share of H's scalar.  One lane per member, blocks of one wave, no LDS; every lane touches its own words only.
// The lane is a latency chain of ~330 + 6 lg dependent products, so a batch of up to 64 members is one wave's time, and a larger
// one spreads its waves over the CUs.
__global__ __launch_bounds__(64) void k_fused_terms(const uint64_t *__restrict__ recs, uint32_t M, int lg, uint64_t *scalars, uint64_t *shares) {
    const uint32_t a = blockIdx.x * 64 + threadIdx.x;
    if (a >= M) return;
    fused_terms_lane(recs + (size_t)a * fused_rec_words(lg), lg, scalars + (size_t)a * fused_term_count(lg) * 4, shares + 4 * (size_t)a);
}

// On ctx->stream: the M members' scalars to d_scalars, H's scalar (the sum of the shares, canonical) to d_h; d_shares: M x 4 words
// of working room.  1 <= M <= 65535 (fr_sum_rows' row limit).  d_desc null: every member of size lg, 1 <= lg <= FUSED_MAX_LG, records
// and scalars at constant strides (k_fused_terms).  d_desc given: the members' own sizes and offsets, records and scalars dense
// (mixed_terms.hip's k_mixed_terms; every lg in 1 .. FUSED_MAX_LG is the caller's to check, `lg` is not read).
int fused_terms(halo_ctx *ctx, const uint64_t *d_recs, size_t M, size_t lg, const uint32_t *d_desc, uint64_t *d_scalars, uint64_t *d_shares, uint64_t *d_h) {
    if (!d_desc && (lg < 1 || lg > (size_t)FUSED_MAX_LG)) { set_error("fused_terms: lg n must be in 1..24"); return HALO_E_ARG; }
    if (M < 1 || M > 65535) { set_error("fused_terms: 1..65535 members"); return HALO_E_ARG; }
    if (d_desc) {
        int rc_m = mixed_terms_launch(ctx, d_recs, d_desc, M, d_scalars, d_shares);
        if (rc_m) return rc_m;
    } else {
        HALO_LAUNCH(ctx, "k_fused_terms", k_fused_terms, dim3((unsigned)((M + 63) / 64)), dim3(64), 0, d_recs, (uint32_t)M, (int)lg, d_scalars, d_shares);
        HALO_HIP(hipGetLastError());
    }
    int rc = fr_sum_rows(ctx, d_shares, 4, M, 1);  // row a = share a, one element wide: row 0 becomes the sum
    if (rc) return rc;
    HALO_HIP(hipMemcpyAsync(d_h, d_shares, 32, hipMemcpyDeviceToDevice, ctx->stream));
    return HALO_OK;
}

}  // namespace halo
