// The halo_msm* entry points (group.rs level): the one checked request path every MSM call passes, the scalar staging per slot,
// and the host-scalar path that copies in stretches under its own kernels.  The launch sequences are msm_driver.hip's.
#include "internal.hpp"

namespace halo {
// Every MSM request of the entry points below passes here before any device work: the slot (a synchronous call names slot 0,
// where it runs) and whether it is busy -- fan: the request fans out over the shards of a multi-device context, which keep
// their own books per slot --, 1..8 members without null scalar pointers, and GS[off, off + n) inside the key, written so that
// it cannot wrap around.  Fills `out` with the members.  halo_ctx_read_bases checks its range only (out null).
int msm_request(const halo_ctx *ctx, int slot, bool fan, size_t off, size_t n, const void *const *scalars, size_t count, MsmBatch *out) {
    if (off > ctx->n || n > ctx->n - off) { set_error("msm: bad range or null pointer"); return HALO_E_ARG; }
    if (!out) return HALO_OK;
    if (slot < 0 || slot >= HALO_SLOTS) { set_error("msm: slot out of range"); return HALO_E_ARG; }
    if (fan ? ctx->fan[slot].active : ctx->wss[slot].in_flight) { set_error("msm: slot already has an MSM in flight"); return HALO_E_ARG; }
    if (count < 1 || count > (size_t)MSM_MAX_BATCH || !scalars) { set_error("msm: batch must be in [1, 8]"); return HALO_E_ARG; }
    *out = MsmBatch();
    out->count = (int)count;
    for (size_t b = 0; b < count; ++b) {
        if (n && !scalars[b]) { set_error("msm: bad range or null pointer"); return HALO_E_ARG; }
        out->scalars[b] = static_cast<const uint64_t *>(scalars[b]);
    }
    return HALO_OK;
}
// Slot `slot`'s scalar staging buffer with room for `members` arrays of max(n, 64) scalars; returns member m's.  Host-scalar MSMs copy
// into it, the shards of a multi-device context peer-copy device scalars from other GPUs into it.  Allocated on first use and only
// grown, so its address stays put from call to call: launch graphs are keyed on scalar pointers (MsmWorkspace::GraphKey), and
// halo_msm / halo_msm_begin replay theirs through this buffer.  Every (re)allocation moves alloc_epoch; the slot's stream is
// drained before an old buffer goes.
uint64_t *slot_scalars(halo_ctx *ctx, int slot, int members, int m) {
    const size_t per = ctx_capacity(ctx), need = (size_t)members * per * 32;
    if (ctx->slot_scalars_bytes[slot] < need) {
        alloc_epoch_bump(ctx);
        if (ctx->d_slot_scalars[slot]) (void)hipStreamSynchronize(ctx->streams[slot]);
        (void)hipFree(ctx->d_slot_scalars[slot]);
        ctx->slot_scalars_bytes[slot] = 0;
        hipError_t e = hipMalloc(&ctx->d_slot_scalars[slot], need);
        if (e != hipSuccess) { ctx->d_slot_scalars[slot] = nullptr; hip_fail(e, "hipMalloc"); return nullptr; }
        ctx->slot_scalars_bytes[slot] = need;
    }
    return ctx->d_slot_scalars[slot] + (size_t)m * per * 4;
}
// scalars in host memory (a checked request: msm_request): copied on the slot's own stream right in front of the launch sequence (no
// host round trip in between), into the slot's staging buffer so that launches on different slots overlap with each other's copies
int msm_host_begin(halo_ctx *ctx, int slot, size_t off, size_t n, const uint64_t *scalars, bool mont) {
    uint64_t *d = slot_scalars(ctx, slot, 1, 0);
    if (!d) return HALO_E_DEVICE;
    if (n) HALO_HIP(hipMemcpyAsync(d, scalars, n * 32, hipMemcpyHostToDevice, ctx->streams[slot]));
    return msm_enqueue(ctx, slot, ctx->d_bases + 32 * off, d, mont, n);
}
// The one begin path of the asynchronous forms: device-resident scalars, or host scalars (host: one member), on the context
// itself or fanned out over the shards of a multi-device context -- window shards (parts != 1) stay on devices[0].  batch:
// halo_msm_dev_batch_begin, which alone collects a fanned batch.
static int msm_begin(halo_ctx *ctx, int slot, size_t off, size_t n, const void *const *scalars, size_t count, int mont, int part, int parts,
                     bool host, bool batch) {
    HALO_CTX(ctx);
    const bool fan = !ctx->shards.empty() && parts == 1;
    MsmBatch members;
    int rc = msm_request(ctx, slot, fan, off, n, scalars, count, &members);
    if (rc) return rc;
    members.part = part;
    members.parts = parts;
    if (fan) return multi_batch_begin(ctx, slot, off, n, members, mont != 0, host, batch);
    if (host) return msm_host_begin(ctx, slot, off, n, members.scalars[0], mont != 0);
    return msm_enqueue_batch(ctx, slot, ctx->d_bases + 32 * off, members, mont != 0, n);
}
// The one end path: `count` results of what `slot` holds (a fanned batch only for the batch call, which is an error for the other)
static int msm_end(halo_ctx *ctx, int slot, size_t count, bool batch, uint64_t *out) {
    HALO_CTX(ctx);
    if (!out || count < 1 || count > (size_t)MSM_MAX_BATCH) { set_error("msm: null output or bad batch"); return HALO_E_ARG; }
    const bool fanned = !ctx->shards.empty() && slot >= 0 && slot < HALO_SLOTS && ctx->fan[slot].active;
    if (fanned && ctx->fan[slot].batch && !batch) { set_error("msm: this slot holds a batch (halo_msm_dev_batch_end collects it)"); return HALO_E_ARG; }
    host::Point r[MSM_MAX_BATCH];
    int rc = fanned && ctx->fan[slot].batch == batch ? multi_batch_end(ctx, slot, r, (int)count) : msm_finish_batch(ctx, slot, r, (int)count);
    if (rc) return rc;
    for (size_t b = 0; b < count; ++b) r[b].store_normalized(out + 12 * b);
    return HALO_OK;
}
// halo_msm_end_sharded's local half: whichever begin started `slot` -- a fanned single MSM is collected as halo_msm_dev_end
// collects it, everything else (one context's slot, a fanned batch) as halo_msm_dev_batch_end; `count` must match either way
int msm_end_slot(halo_ctx *ctx, int slot, size_t count, uint64_t *out) {
    const bool fanned_one = ctx && !ctx->shards.empty() && slot >= 0 && slot < HALO_SLOTS && ctx->fan[slot].active && !ctx->fan[slot].batch;
    return msm_end(ctx, slot, count, !fanned_one, out);
}

// halo_msm, the call the reference's shim makes (integration/ffi.rs point_dot_affine: a Vec of scalars in pageable memory, one
// synchronous call).  One copy in front of one launch sequence leaves the GPU idle for the whole copy (32 MiB at PCIe speed:
// 0.65 of 1.95 ms at n = 2^20).  An MSM is a sum over index stretches, so a large one over the key's c = 20 table runs as P
// stretches on P slots: stretch k's scalars are copied on slot k's stream directly in front of its launch sequence, the copies
// queue up behind one another on the copy engine and every stretch's kernels start as soon as ITS scalars are there -- under
// the copies of the stretches behind it.  The stretches' points are added on the host in index order.  Same result, bit for
// bit (points written by the library are normalised).  Not taken: multi-device contexts (each shard copies its own block over
// its own link already), contexts without the c = 20 table (the first MSM of a context builds it), any slot busy.
// The stretches of an n-point MSM, in sixteenths: the caller's HALO_HOST_SPLIT at every size, else what was measured best on one
// box (profiles/r05_host_msm_stretches_sweep.txt): 4 + 12 below 2^21 points (2^20: 1.63 ms against 1.92 for one copy + one launch
// sequence; a short first stretch lets the kernels start early, and more stretches only serialise behind one another's bucket
// kernels), 2 + 4 + 4 + 6 from 2^21 points on, where every stretch is a full-size pipeline pass of its own (2^22: 5.2 against 7.7 ms,
// 2^24: 19.9 against 29.0).
struct HostSplit { int pieces; int sixteenths[HALO_SLOTS]; };
static HostSplit host_split_for(size_t n) {
    const Tuning &t = tuning();
    if (t.host_split_set) return HostSplit{t.host_pieces, {t.host_split[0], t.host_split[1], t.host_split[2], t.host_split[3]}};
    if (n >= ((size_t)1 << 21)) return HostSplit{4, {2, 4, 4, 6}};
    return HostSplit{2, {4, 12, 0, 0}};
}
static int host_pieces_wanted(const halo_ctx *ctx, size_t n) {
    const int P = host_split_for(n).pieces;
    if (P < 2 || !ctx->shards.empty() || !ctx->d_table || ctx->tbl.c != 20 || ctx->table_mode == 0 || ctx->window_bits != 0) return 1;
    if (n < ((size_t)1 << 19) || n % 64 != 0) return 1;
    for (int k = 0; k < P; ++k)
        if (ctx->wss[k].in_flight || ctx->wss[k].lent_from >= 0) return 1;
    return P;
}
// `valid` <= n: the host array holds that many scalars, the MSM's remaining scalars are zero (a polynomial shorter than d + 1)
static int msm_host_pieces(halo_ctx *ctx, int P, size_t off, size_t n, const uint64_t *scalars, size_t valid, int mont, host::Point *out) {
    // stretch k takes host_split[k] sixteenths of the points (n is a multiple of 64: every length a multiple of 4), the last one the rest
    size_t lens[HALO_SLOTS], offs[HALO_SLOTS];
    const HostSplit split = host_split_for(n);
    {
        size_t at = 0;
        for (int k = 0; k < P; ++k) {
            lens[k] = k == P - 1 ? n - at : n / 16 * (size_t)split.sixteenths[k];
            offs[k] = at;
            at += lens[k];
        }
    }
    uint64_t *stage[HALO_SLOTS];
    for (int k = 0; k < P; ++k)  // (every stretch's buffer is there before the first stretch goes out)
        if (!(stage[k] = slot_scalars(ctx, k, 1, 0))) return HALO_E_DEVICE;
    int rc = HALO_OK, started = 0;
    for (int k = 0; k < P && !rc; ++k) {
        const size_t len = lens[k];
        const size_t have = valid > offs[k] ? (valid - offs[k] < len ? valid - offs[k] : len) : 0;  // scalars of this stretch the caller has
        hipError_t e = hipSuccess;
        if (have < len) e = hipMemsetAsync(stage[k] + 4 * have, 0, (len - have) * 32, ctx->streams[k]);
        if (e == hipSuccess && have) e = hipMemcpyAsync(stage[k], scalars + 4 * offs[k], have * 32, hipMemcpyHostToDevice, ctx->streams[k]);
        if (e != hipSuccess) { rc = hip_fail(e, "hipMemcpyAsync"); break; }
        MsmBatch one = msm_one(stage[k]);
        one.sub = true;
        rc = msm_enqueue_batch(ctx, k, ctx->d_bases + 32 * (off + offs[k]), one, mont != 0, len);
        if (!rc) started = k + 1;
    }
    host::Point acc = host::Point::infinity();
    for (int k = 0; k < started; ++k) {  // (every stretch that went out is collected, whatever happened to the others)
        host::Point r;
        int rk = msm_finish(ctx, k, &r);
        if (rk && !rc) rc = rk;
        acc = acc + r;
    }
    *out = acc;
    return rc;
}
// One synchronous MSM over GS[off, off + n) with `valid` <= n scalars in pageable host memory (the rest zero): in stretches where
// that pays (above), else one copy in front of one launch sequence on slot 0.  halo_msm and pcdl::commit / pedersen::commit with host
// coefficients (pcdl_acc.hip) both end here.
int msm_host_run(halo_ctx *ctx, size_t off, size_t n, const uint64_t *scalars, size_t valid, int mont, host::Point *out) {
    if (valid > n) { set_error("msm: bad range or null pointer"); return HALO_E_ARG; }
    const bool fan = !ctx->shards.empty() && valid == n;
    const void *p = scalars;
    MsmBatch one;
    int rc = msm_request(ctx, 0, fan, off, n, &p, 1, &one);
    if (rc) return rc;
    if (fan) return multi_host_run(ctx, off, n, scalars, mont != 0, out);
    const int P = host_pieces_wanted(ctx, n);
    if (P > 1) return msm_host_pieces(ctx, P, off, n, scalars, valid, mont, out);
    uint64_t *d = slot_scalars(ctx, 0, 1, 0);
    if (!d) return HALO_E_DEVICE;
    if (valid < n) HALO_HIP(hipMemsetAsync(d + 4 * valid, 0, (n - valid) * 32, ctx->streams[0]));
    if (valid) HALO_HIP(hipMemcpyAsync(d, scalars, valid * 32, hipMemcpyHostToDevice, ctx->streams[0]));
    // (a multi-device context with a short polynomial: the padded scalars are device-resident now, for its shards to read)
    if (!ctx->shards.empty()) HALO_HIP(hipStreamSynchronize(ctx->streams[0]));
    return msm_run(ctx, ctx->d_bases + 32 * off, d, mont != 0, n, out);
}
// An MSM over m <= ctx_capacity points of the caller's (pt_words words each): through d_tmp_a into native 128-byte entries in
// d_tmp_b (16 words of room per element) by to_native, batch_to_affine or aff_words_to_native; the scalars follow in d_tmp_a
static int msm_caller_points(halo_ctx *ctx, const uint64_t *pts, size_t pt_words, int (*to_native)(halo_ctx *, const uint64_t *, size_t, uint32_t *),
                             const uint64_t *scalars, size_t m, bool mont, host::Point *out) {
    int rc = upload_words(ctx, ctx->d_tmp_a, pts, m * pt_words);
    if (!rc) rc = to_native(ctx, ctx->d_tmp_a, m, reinterpret_cast<uint32_t *>(ctx->d_tmp_b));
    if (rc) return rc;
    HALO_HIP(hipStreamSynchronize(ctx->stream));
    rc = upload_words(ctx, ctx->d_tmp_a, scalars, m * 4);
    if (rc) return rc;
    return msm_run(ctx, reinterpret_cast<const uint32_t *>(ctx->d_tmp_b), ctx->d_tmp_a, mont, m, out);
}
}  // namespace halo

using namespace halo;

extern "C" {
int halo_msm_dev(halo_ctx *ctx, size_t off, size_t n, const void *d_scalars, int mont, uint64_t out[12]) {
    HALO_CTX(ctx);
    if (!out) { set_error("msm: null output"); return HALO_E_ARG; }
    MsmBatch one;
    int rc = msm_request(ctx, 0, !ctx->shards.empty() && n >= MULTI_RUN_MIN, off, n, &d_scalars, 1, &one);
    if (rc) return rc;
    host::Point r;
    rc = msm_run(ctx, ctx->d_bases + 32 * off, one.scalars[0], mont != 0, n, &r);
    if (rc) return rc;
    r.store_normalized(out);
    return HALO_OK;
}

int halo_msm_dev_begin(halo_ctx *ctx, int slot, size_t off, size_t n, const void *d_scalars, int mont) {
    return msm_begin(ctx, slot, off, n, &d_scalars, 1, mont, 0, 1, false, false);
}
int halo_msm_dev_begin_part(halo_ctx *ctx, int slot, size_t off, size_t n, const void *d_scalars, int mont, int part, int parts) {
    return msm_begin(ctx, slot, off, n, &d_scalars, 1, mont, part, parts, false, false);
}
int halo_msm_dev_end(halo_ctx *ctx, int slot, uint64_t out[12]) { return msm_end(ctx, slot, 1, false, out); }

int halo_msm_dev_batch_begin(halo_ctx *ctx, int slot, size_t off, size_t n, const void *const *d_scalars, size_t batch, int mont, int part,
                             int parts) {
    return msm_begin(ctx, slot, off, n, d_scalars, batch, mont, part, parts, false, true);
}
int halo_msm_dev_batch_end(halo_ctx *ctx, int slot, size_t batch, uint64_t *out) { return msm_end(ctx, slot, batch, true, out); }

int halo_msm_begin(halo_ctx *ctx, int slot, size_t off, size_t n, const uint64_t *scalars, int mont) {
    const void *p = scalars;
    return msm_begin(ctx, slot, off, n, &p, 1, mont, 0, 1, true, false);
}
int halo_msm_end(halo_ctx *ctx, int slot, uint64_t out[12]) { return halo_msm_dev_end(ctx, slot, out); }

int halo_msm(halo_ctx *ctx, size_t off, size_t n, const uint64_t *scalars, int mont, uint64_t out[12]) {
    if (!out) { set_error("msm: null output"); return HALO_E_ARG; }
    HALO_CTX(ctx);
    host::Point r;
    int rc = msm_host_run(ctx, off, n, scalars, n, mont, &r);
    if (rc) return rc;
    r.store_normalized(out);
    return HALO_OK;
}

int halo_msm_points(halo_ctx *ctx, const uint64_t *pts_jac, const uint64_t *scalars, size_t m, uint64_t out[12]) {
    HALO_CTX(ctx);
    if (m > ctx_capacity(ctx)) { set_error("msm_points: m exceeds the context's workspace"); return HALO_E_ARG; }
    if (!out || (m && (!pts_jac || !scalars))) { set_error("msm_points: null pointer"); return HALO_E_ARG; }
    host::Point r;
    int rc = msm_caller_points(ctx, pts_jac, 12, batch_to_affine, scalars, m, true, &r);
    if (rc) return rc;
    r.store_normalized(out);
    return HALO_OK;
}

int halo_msm_affine(halo_ctx *ctx, const uint64_t *bases_affine, const uint64_t *scalars, size_t m, int mont, uint64_t out[12]) {
    HALO_CTX(ctx);
    if (!out || (m && (!bases_affine || !scalars))) { set_error("msm_affine: null pointer"); return HALO_E_ARG; }
    // more generators than the context's workspace holds: consecutive chunks, partial sums added on the host
    const size_t cap = ctx_capacity(ctx);
    host::Point acc = host::Point::infinity();
    for (size_t lo = 0; lo < m || lo == 0; lo += cap) {
        size_t len = m - lo < cap ? m - lo : cap;
        host::Point r;
        int rc = msm_caller_points(ctx, bases_affine + 8 * lo, 8, aff_words_to_native, scalars + 4 * lo, len, mont != 0, &r);
        if (rc) return rc;
        acc = acc + r;
        if (m == 0) break;
    }
    acc.store_normalized(out);
    return HALO_OK;
}
}  // extern "C"
