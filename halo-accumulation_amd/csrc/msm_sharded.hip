// point_dot_affine (group.rs:24-26) sharded over one process per GPU, in one call (include/halo_accumulation.h, "sharded MSM").
//
// Each rank runs ITS share of the MSM through the ordinary entry points (halo_msm, halo_msm_dev, the begin / end halves: the
// one checked request path of msm_entry.hip, a multi-device context fanning out as it always does), then the P partial points are
// exchanged in ONE call of the caller's all-gather -- 12 words per member plus the status word of the sharded open / check
// (internal.hpp StatusGather) -- and every rank adds them in rank order on the host, halo_point_sum's rule.  That is at most
// 64 additions of 96-byte records: no kernel, no extra copy.
//
// Failure safety as in halo_pcdl_open_sharded: what every rank passes alike (world, rank, the callback, batch, out_jac) is
// checked before the collective and returns HALO_E_ARG at once; whatever can fail on one rank only -- a null context, a range
// past this rank's key, null scalars, an idle slot or a batch mismatch, a device failure -- rides into the collective as that
// rank's status and every rank returns the first non-zero one in rank order.
#include "internal.hpp"

using namespace halo;

namespace {

int sharded_args(const char *who, uint64_t world, uint64_t rank, halo_allgather_fn allgather, size_t batch, const uint64_t *out) {
    if (!out) { set_error(std::string(who) + ": null output"); return HALO_E_ARG; }
    if (world == 0 || world > 64 || rank >= world) { set_error(std::string(who) + ": world in 1..64, rank below it"); return HALO_E_ARG; }
    if (world > 1 && !allgather) { set_error(std::string(who) + ": more than one rank needs an all-gather"); return HALO_E_ARG; }
    if (batch < 1 || batch > (size_t)MSM_MAX_BATCH) { set_error(std::string(who) + ": batch must be in [1, 8]"); return HALO_E_ARG; }
    return HALO_OK;
}

// The one collective: this rank's `batch` partial points (mine, normalised; ignored if lrc != 0) and its status.  out = batch x 12
// limbs, member b the sum of the P ranks' member b in rank order -- the same limbs on every rank.
int gather_sum(const char *who, uint64_t world, uint64_t rank, halo_allgather_fn allgather, void *user, int lrc, const uint64_t *mine,
               size_t batch, uint64_t *out) {
    if (!lrc) lrc = shard_test_failure(rank, SHARD_AT_MSM);
    StatusGather sg{(size_t)world, rank, allgather, user, who, {}, {}};
    std::vector<uint64_t> recv;
    int rc = sg.run(mine, 12 * batch, lrc, recv);
    if (rc) return rc;
    for (size_t b = 0; b < batch; ++b) {
        host::Point acc = host::Point::infinity();
        for (uint64_t r = 0; r < world; ++r) acc = acc + host::Point::load(&recv[(r * batch + b) * 12]);
        acc.store_normalized(out + 12 * b);
    }
    return HALO_OK;
}

}  // namespace

extern "C" {

int halo_msm_sharded(halo_ctx *ctx, uint64_t world, uint64_t rank, size_t off, size_t n, const uint64_t *scalars, int mont,
                     halo_allgather_fn allgather, void *user, uint64_t out[12]) {
    int rc = sharded_args("msm_sharded", world, rank, allgather, 1, out);
    if (rc) return rc;
    uint64_t mine[12] = {};
    const int lrc = halo_msm(ctx, off, n, scalars, mont, mine);
    return gather_sum("msm_sharded", world, rank, allgather, user, lrc, mine, 1, out);
}

int halo_msm_dev_sharded(halo_ctx *ctx, uint64_t world, uint64_t rank, size_t off, size_t n, const void *d_scalars, int mont,
                         halo_allgather_fn allgather, void *user, uint64_t out[12]) {
    int rc = sharded_args("msm_dev_sharded", world, rank, allgather, 1, out);
    if (rc) return rc;
    uint64_t mine[12] = {};
    const int lrc = halo_msm_dev(ctx, off, n, d_scalars, mont, mine);
    return gather_sum("msm_dev_sharded", world, rank, allgather, user, lrc, mine, 1, out);
}

int halo_msm_end_sharded(halo_ctx *ctx, int slot, size_t batch, uint64_t world, uint64_t rank, halo_allgather_fn allgather, void *user,
                         uint64_t *out) {
    int rc = sharded_args("msm_end_sharded", world, rank, allgather, batch, out);
    if (rc) return rc;
    uint64_t mine[12 * MSM_MAX_BATCH] = {};
    const int lrc = msm_end_slot(ctx, slot, batch, mine);
    return gather_sum("msm_end_sharded", world, rank, allgather, user, lrc, mine, batch, out);
}

}  // extern "C"
