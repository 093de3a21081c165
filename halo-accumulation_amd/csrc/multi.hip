// Multi-device contexts ("halo_ctx_create(device_ids[], n_dev, ...) uploads (and shards) bases once";
// 8e: an MSM is a sum over independent index terms).  One process drives several GPUs:
//
//   * the handle the caller gets is a full context on devices[0] over the whole key -- every entry point of the
//     library works on it unchanged (IPA state, pcdl / acc level, h(X), ...);
//   * it owns one SHARD context per device over that device's index block of the key (block k = [k N / P, (k+1) N / P),
//     multiples of 4; each shard derives or receives only its block and builds its own fixed-base table on first use);
//   * an MSM over GS[off, off + n) -- halo_msm, halo_msm_dev, the begin/end halves and the library's own synchronous
//     MSMs over the key (commit, check, h_commit) -- is cut along the block boundaries, every shard enqueues its stretch
//     on its own device and stream, the shards' window sums are combined by their helper threads in parallel and the
//     P partial points are added on the host in block order (halo_point_sum's rule): bit-identical to the one-device
//     result, which is a normalised point.  Device-resident scalars are read in place by the shard on the same device
//     and copied peer-to-peer (xGMI) for the others; host scalars go straight to each device over its own PCIe link.
//
// There is no collective here: one process owns all partials.  Ranks of a torch.distributed job each hold a plain
// context and all-gather 96 bytes instead (halo-accumulation_amd/sharded.py).
#include <algorithm>

#include "curve.hpp"
#include "internal.hpp"

namespace halo {

static size_t block_lo(size_t N, int P, int k) {
    if (k >= P) return N;
    size_t lo = (size_t)((unsigned __int128)N * (unsigned)k / (unsigned)P);
    return lo / 4 * 4;  // (vector loads of digits want multiples of 4)
}

void multi_destroy(halo_ctx *ctx) {
    for (halo_ctx *s : ctx->shards) halo_ctx_destroy(s);
    ctx->shards.clear();
    ctx->shard_lo.clear();
}

// shards over the blocks of the parent's key: derived on their own device (URS rule) or copied from the host array
int multi_attach_shards(halo_ctx *ctx, const int *devices, int n_dev, const uint64_t *bases_affine, uint64_t first_index) {
    size_t N = ctx->n;
    ctx->shard_lo.resize((size_t)n_dev + 1);
    for (int k = 0; k <= n_dev; ++k) ctx->shard_lo[k] = block_lo(N, n_dev, k);
    for (int k = 0; k < n_dev; ++k) {
        size_t lo = ctx->shard_lo[k], len = ctx->shard_lo[k + 1] - lo;
        halo_ctx *s = nullptr;
        int rc = bases_affine ? halo_ctx_create(devices[k], bases_affine + 8 * lo, len, &s) : halo_ctx_create_urs(devices[k], first_index + lo, len, &s);
        if (rc) { multi_destroy(ctx); return rc; }
        s->parent = ctx;
        ctx->shards.push_back(s);
        if (devices[k] != ctx->device) {  // direct peer copies of device-resident scalars (xGMI); without it HIP stages through the host
            (void)hipSetDevice(devices[k]);
            (void)hipDeviceEnablePeerAccess(ctx->device, 0);
            (void)hipSetDevice(ctx->device);
            (void)hipDeviceEnablePeerAccess(devices[k], 0);
            (void)hipGetLastError();  // "already enabled" is fine
        }
    }
    (void)hipSetDevice(ctx->device);
    return HALO_OK;
}

bool multi_takes(const halo_ctx *ctx, const uint32_t *d_bases, size_t n) {
    return !ctx->shards.empty() && d_bases >= ctx->d_bases && d_bases + AFF_STRIDE * n <= ctx->d_bases + AFF_STRIDE * ctx->n;
}

static int device_of(const void *p, int fallback) {
    hipPointerAttribute_t a;
    if (p && hipPointerGetAttributes(&a, p) == hipSuccess) return a.device;
    (void)hipGetLastError();
    return fallback;
}

// fn(k, a, b) for every shard k whose block meets GS[off, off + n), [a, b) being the common stretch (indices into the key), in
// block order; stops at the first failure
template <class F>
static int for_blocks(const halo_ctx *ctx, size_t off, size_t n, F fn) {
    for (int k = 0; k + 1 < (int)ctx->shard_lo.size(); ++k) {
        size_t a = std::max(off, ctx->shard_lo[k]), b = std::min(off + n, ctx->shard_lo[k + 1]);
        if (a >= b) continue;
        int rc = fn(k, a, b);
        if (rc) return rc;
    }
    return HALO_OK;
}

// The same fn(k, a, b) on every such shard's helper thread (on the shard's device), all at once; waits for them in block order
// and returns the first failure with its message
template <class F>
static int on_shards(halo_ctx *ctx, size_t off, size_t n, F fn) {
    const int P = (int)ctx->shards.size();
    std::vector<int> rcs((size_t)P, HALO_OK);
    std::vector<std::string> errs((size_t)P);
    (void)for_blocks(ctx, off, n, [&](int k, size_t a, size_t b) {
        halo_ctx *s = ctx->shards[k];
        s->worker.submit([s, k, a, b, &fn, &rcs, &errs] {
            (void)hipSetDevice(s->device);
            rcs[k] = fn(k, a, b);
            if (rcs[k]) errs[k] = halo_last_error();
        });
        return HALO_OK;
    });
    int rc = HALO_OK;
    (void)for_blocks(ctx, off, n, [&](int k, size_t, size_t) {
        ctx->shards[k]->worker.wait();
        if (rcs[k] && !rc) { rc = rcs[k]; set_error(errs[k]); }
        return HALO_OK;
    });
    (void)hipSetDevice(ctx->device);
    return rc;
}

// Enqueue the stretches of `members.count` MSMs over GS[off, off + n) on the shards' slot `slot`: every shard runs ITS stretch of
// all members as one batched launch sequence (which is what makes a 2^17-point block a full launch: msm_table.hip, small-key table
// plan).  host: the one member's scalars are in host memory -- every device has its own PCIe link, so each shard's helper
// thread copies its stretch (msm_host_begin); else the shard on the scalars' device reads them in place and the others copy
// theirs peer-to-peer (xGMI) into member m's place in their slot's staging buffer, in front of their launches.  batch: begun by
// halo_msm_dev_batch_begin, which alone collects it.
int multi_batch_begin(halo_ctx *ctx, int slot, size_t off, size_t n, const MsmBatch &members, bool mont, bool host, bool batch) {
    halo_ctx::Fan &fan = ctx->fan[slot];
    if (fan.active) { set_error("msm: slot already has an MSM in flight"); return HALO_E_ARG; }
    int rc;
    if (host) {
        rc = on_shards(ctx, off, n, [&](int k, size_t a, size_t b) {
            halo_ctx *s = ctx->shards[k];
            return msm_host_begin(s, slot, a - ctx->shard_lo[k], b - a, members.scalars[0] + 4 * (a - off), mont);
        });
    } else {
        int src_dev[MSM_MAX_BATCH];
        for (int m = 0; m < members.count; ++m) src_dev[m] = device_of(members.scalars[m], ctx->device);
        // (a failure stops the loop; whatever the shards before it have enqueued is drained below)
        rc = for_blocks(ctx, off, n, [&](int k, size_t a, size_t b) {
            halo_ctx *s = ctx->shards[k];
            hipError_t e = hipSetDevice(s->device);
            MsmBatch mine = members;
            for (int m = 0; m < members.count && e == hipSuccess; ++m) {
                mine.scalars[m] = members.scalars[m] + 4 * (a - off);
                mine.base_off[m] = 0;
                if (src_dev[m] == s->device && !dev_hooks().force_peer_copy) continue;  // (development library's hook: the copy path on a one-GPU box)
                uint64_t *dst = slot_scalars(s, slot, members.count, m);
                if (!dst) return HALO_E_DEVICE;
                e = hipMemcpyPeerAsync(dst, s->device, mine.scalars[m], src_dev[m], (b - a) * 32, s->streams[slot]);
                mine.scalars[m] = dst;
            }
            // (same device: the shard reads the caller's buffer in place; as for halo_msm_dev on a plain context the caller has
            // synchronised whatever wrote it)
            if (e != hipSuccess) return hip_fail(e, "multi-device MSM: peer copy of the scalars");
            return msm_enqueue_batch(s, slot, s->d_bases + 32 * (a - ctx->shard_lo[k]), mine, mont, b - a);
        });
        (void)hipSetDevice(ctx->device);
    }
    fan.active = true;  // (also after a failure: multi_batch_end drains whatever was enqueued)
    fan.batch = batch;
    fan.count = members.count;
    fan.off = off;
    fan.n = n;
    if (rc) { host::Point dummy[MSM_MAX_BATCH]; std::string keep = halo_last_error(); (void)multi_batch_end(ctx, slot, dummy, members.count); set_error(keep); }
    return rc;
}

// Wait for the shards, combine their window sums (each on its own helper thread), add the per-member partials in block order.
// A wrong count is reported and leaves the MSMs in flight.
int multi_batch_end(halo_ctx *ctx, int slot, host::Point *out, int count) {
    if (slot < 0 || slot >= HALO_SLOTS || !ctx->fan[slot].active) { set_error("msm: nothing in flight on this slot"); return HALO_E_ARG; }
    halo_ctx::Fan &fan = ctx->fan[slot];
    if (fan.count != count) { set_error("msm: this slot holds a batch of a different size"); return HALO_E_ARG; }
    std::vector<host::Point> part(ctx->shards.size() * MSM_MAX_BATCH, host::Point::infinity());
    int rc = on_shards(ctx, fan.off, fan.n, [&](int k, size_t, size_t) {
        halo_ctx *s = ctx->shards[k];
        if (!s->wss[slot].in_flight) return (int)HALO_OK;  // (its begin failed or never came: it adds nothing)
        return msm_finish_batch(s, slot, &part[(size_t)k * MSM_MAX_BATCH], count);
    });
    for (int m = 0; m < count; ++m) out[m] = host::Point::infinity();
    for (size_t k = 0; k < ctx->shards.size(); ++k)
        for (int m = 0; m < count; ++m) out[m] = out[m] + part[k * MSM_MAX_BATCH + m];  // block order 0 .. P-1
    fan.active = false;
    return rc;
}

int multi_run(halo_ctx *ctx, size_t off, size_t n, const uint64_t *dev_scalars, bool mont, host::Point *out) {
    // the library's own synchronous MSMs have just written their scalars on the parent's stream
    HALO_HIP(hipStreamSynchronize(ctx->stream));
    int rc = multi_batch_begin(ctx, 0, off, n, msm_one(dev_scalars), mont, false, false);
    if (rc) return rc;
    return multi_batch_end(ctx, 0, out, 1);
}

// The synchronous host-scalar form (halo_msm, pcdl::commit with host coefficients): every shard's helper thread runs its block of
// GS[off, off + n) through msm_host_run on its own device -- its scalars over its own PCIe link, in stretches where that pays
// (msm_entry.hip: a shard's block of 2^21 points of an n = 2^24 MSM copies under its own kernels) -- and the partial points are added in
// block order.  Same point as multi_batch_begin + multi_batch_end give.
int multi_host_run(halo_ctx *ctx, size_t off, size_t n, const uint64_t *scalars, bool mont, host::Point *out) {
    std::vector<host::Point> part(ctx->shards.size(), host::Point::infinity());
    int rc = on_shards(ctx, off, n, [&](int k, size_t a, size_t b) {
        return msm_host_run(ctx->shards[k], a - ctx->shard_lo[k], b - a, scalars + 4 * (a - off), b - a, mont ? 1 : 0, &part[k]);
    });
    if (rc) return rc;
    host::Point acc = host::Point::infinity();
    for (const host::Point &p : part) acc = acc + p;  // block order
    *out = acc;
    return HALO_OK;
}

}  // namespace halo
