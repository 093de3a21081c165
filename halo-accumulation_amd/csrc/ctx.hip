// Contexts of libhalo_hip.so (include/halo_accumulation.h): error reporting, create / clone / destroy, the getters, the word
// copies between host and device that the host-pointer entry points share, and the public points S and H with their window tables.
#include "internal.hpp"

namespace halo {
static thread_local std::string g_err;
void set_error(const std::string &msg) { g_err = msg; }
int hip_fail(hipError_t e, const char *what) {
    g_err = std::string("HIP error: ") + hipGetErrorString(e) + " in " + what;
    return HALO_E_DEVICE;
}

static int ctx_alloc_common(halo_ctx *ctx, int device, size_t n) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
        set_error("no HIP device available: this library has no CPU fallback");
        return HALO_E_DEVICE;
    }
    if (device < 0 || device >= count) { set_error("device index out of range"); return HALO_E_ARG; }
    HALO_HIP(hipSetDevice(device));
    ctx->device = device;
    ctx->n = n;
    alloc_epoch_bump(ctx);
    for (int k = 0; k < HALO_SLOTS; ++k) HALO_HIP(hipStreamCreateWithFlags(&ctx->streams[k], hipStreamNonBlocking));
    ctx->stream = ctx->streams[0];
    if (!ctx->share) {  // (a clone arrives with the key it shares: halo_ctx_clone)
        HALO_HIP(hipMalloc(&ctx->d_bases, (n ? n : 1) * 128));
        ctx->share = std::make_shared<KeyShare>();
        ctx->share->d_bases = ctx->d_bases;
    }
    const size_t tn = ctx_capacity(ctx);
    ctx->tmp_words = tn * 12;
    HALO_HIP(hipMalloc(&ctx->d_tmp_a, tn * 12 * 8));
    HALO_HIP(hipMalloc(&ctx->d_tmp_b, tn * 16 * 8));
    HALO_HIP(hipMalloc(&ctx->d_tmp_c, 16384 * 8));
    HALO_HIP(hipHostMalloc(&ctx->h_pinned, 4096));
    HALO_HIP(hipHostMalloc(&ctx->h_wintab, 8192));
    if (tuning().graphs >= 0) ctx->use_graphs = tuning().graphs != 0;  // HALO_GRAPHS=0: never replay launch graphs
    if (tuning().fold_async > -2) ctx->fold_async = tuning().fold_async;  // -1 automatic, 0 every fold in line, 1 beside the rounds wherever possible (halo_set_fold_async)
    return msm_workspace_alloc(ctx, n, 0);
}

int upload_words(halo_ctx *ctx, uint64_t *dst, const uint64_t *src, size_t words) {
    if (words == 0) return HALO_OK;
    HALO_HIP(hipMemcpyAsync(dst, src, words * 8, hipMemcpyHostToDevice, ctx->stream));
    HALO_HIP(hipStreamSynchronize(ctx->stream));
    return HALO_OK;
}
int download_words(halo_ctx *ctx, uint64_t *dst, const uint64_t *src, size_t words) {
    if (words == 0) return HALO_OK;
    HALO_HIP(hipMemcpyAsync(dst, src, words * 8, hipMemcpyDeviceToHost, ctx->stream));
    HALO_HIP(hipStreamSynchronize(ctx->stream));
    return HALO_OK;
}

// The one body of the single-device constructors: a context for n points on `device` whose key fill(ctx) writes to d_bases
// (the temporaries are there for it to stage in).  Whatever fails, what was built so far is destroyed.
template <class Fill>
static int ctx_new(int device, size_t n, Fill fill, halo_ctx **out) {
    halo_ctx *ctx = new (std::nothrow) halo_ctx();
    if (!ctx) { set_error("out of host memory"); return HALO_E_ARG; }
    int rc = ctx_alloc_common(ctx, device, n);
    if (rc == HALO_OK) rc = fill(ctx);
    if (rc != HALO_OK) { halo_ctx_destroy(ctx); return rc; }
    *out = ctx;
    return HALO_OK;
}

// ... and of the two multi-device ones: create(device) builds the whole key's context on devices[0] into *out, the other
// devices' shards attach to it (multi.hip: from the caller's bases, or generated from first_index on)
template <class Create>
static int ctx_new_multi(const int *devices, int n_dev, Create create, const uint64_t *bases_affine, uint64_t first_index, halo_ctx **out) {
    int count = 0;
    if (!devices || n_dev < 1 || n_dev > 64) { set_error("ctx_create_multi: 1..64 device ids"); return HALO_E_ARG; }
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) { set_error("no HIP device available: this library has no CPU fallback"); return HALO_E_DEVICE; }
    for (int k = 0; k < n_dev; ++k)
        if (devices[k] < 0 || devices[k] >= count) { set_error("ctx_create_multi: device index out of range"); return HALO_E_ARG; }
    int rc = create(devices[0]);
    if (rc || n_dev == 1) return rc;
    rc = multi_attach_shards(*out, devices, n_dev, bases_affine, first_index);
    if (rc) { halo_ctx_destroy(*out); *out = nullptr; }
    return rc;
}

static host::FixedBaseTable public_table(int which) {  // 0: S, 1: H
    uint64_t SH[2][12];
    halo_public_points(SH[0], SH[1]);
    return host::FixedBaseTable(host::Point::load(SH[which]));
}
const host::FixedBaseTable &public_h_table() { static const host::FixedBaseTable tbl = public_table(1); return tbl; }
const host::FixedBaseTable &public_s_table() { static const host::FixedBaseTable tbl = public_table(0); return tbl; }
}  // namespace halo

using namespace halo;

extern "C" {
const char *halo_last_error(void) { return g_err.c_str(); }

int halo_device_count(void) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) return 0;
    return count;
}

int halo_ctx_create(int device, const uint64_t *bases_affine, size_t n, halo_ctx **out) {
    if (!out || (n && !bases_affine)) { set_error("ctx_create: null argument"); return HALO_E_ARG; }
    return ctx_new(device, n, [&](halo_ctx *ctx) {
        int rc = upload_words(ctx, ctx->d_tmp_a, bases_affine, n * 8);
        if (rc == HALO_OK) rc = aff_words_to_native(ctx, ctx->d_tmp_a, n, ctx->d_bases);
        if (rc == HALO_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = HALO_E_DEVICE;
        return rc;
    }, out);
}

int halo_ctx_create_urs(int device, uint64_t first_index, size_t n, halo_ctx **out) {
    if (!out) { set_error("ctx_create_urs: null argument"); return HALO_E_ARG; }
    return ctx_new(device, n, [&](halo_ctx *ctx) { return urs_generate(ctx, first_index, 1, n, ctx->d_bases); }, out);
}

int halo_ctx_create_urs_strided(int device, uint64_t first_index, uint64_t stride, size_t n, halo_ctx **out) {
    if (!out || stride == 0) { set_error("ctx_create_urs_strided: bad argument"); return HALO_E_ARG; }
    return ctx_new(device, n, [&](halo_ctx *ctx) { return urs_generate(ctx, first_index, stride, n, ctx->d_bases); }, out);
}

int halo_ctx_create_multi(const int *devices, int n_dev, const uint64_t *bases_affine, size_t n, halo_ctx **out) {
    return ctx_new_multi(devices, n_dev, [&](int device) { return halo_ctx_create(device, bases_affine, n, out); }, bases_affine, 0, out);
}
int halo_ctx_create_urs_multi(const int *devices, int n_dev, uint64_t first_index, size_t n, halo_ctx **out) {
    return ctx_new_multi(devices, n_dev, [&](int device) { return halo_ctx_create_urs(device, first_index, n, out); }, nullptr, first_index, out);
}
int halo_ctx_devices(const halo_ctx *ctx) { return ctx ? (ctx->shards.empty() ? 1 : (int)ctx->shards.size()) : 0; }

// A second context over the SAME resident key (one per host thread: contexts are independent, calls on one context must not
// overlap).  It shares the key and -- as they come into being, whoever builds them -- the fixed-base MSM table and the fold
// table, and owns its streams, workspaces, scratch and IPA buffers (~2.3 GB at 2^20 points against 37 GB for a context of its
// own with both tables).  Tuning knobs are copied from `ctx` at this moment and independent afterwards.
int halo_ctx_clone(halo_ctx *src, halo_ctx **out) {
    if (!src || !out) { set_error("ctx_clone: null argument"); return HALO_E_ARG; }
    if (!src->shards.empty() || src->parent) { set_error("ctx_clone: multi-device contexts and their shards are not cloned"); return HALO_E_ARG; }
    // A key with clones is a service that opens: while `src` is still the table's only user, an all-shifts MSM table that leaves the
    // fold table no room goes down to its 13 rows (internal.hpp table_demote; declined while src has launches in flight)
    if (fold_table_wanted(src) && !table_budget_room(src, foldtab_need_bytes(src->n)) && table_should_demote(src)) {
        HALO_CTX(src);
        (void)table_demote_now(src);
    }
    halo_ctx *ctx = new (std::nothrow) halo_ctx();
    if (!ctx) { set_error("out of host memory"); return HALO_E_ARG; }
    ctx->share = src->share;
    { std::lock_guard<std::mutex> lk(ctx->share->mu); ctx->share->users++; }
    ctx->d_bases = ctx->share->d_bases;
    int rc = ctx_alloc_common(ctx, src->device, src->n);
    if (rc != HALO_OK) { halo_ctx_destroy(ctx); return rc; }
    ctx->window_bits = src->window_bits; ctx->reduce_span = src->reduce_span; ctx->sort_two_level = src->sort_two_level;
    ctx->task_len = src->task_len; ctx->table_mode = src->table_mode; ctx->small_path = src->small_path; ctx->use_graphs = src->use_graphs;
    ctx->nofold_size = src->nofold_size; ctx->batch_verify = src->batch_verify; ctx->fold_table_mode = src->fold_table_mode;
    ctx->fold_levels = src->fold_levels; ctx->fold_async = src->fold_async;
    *out = ctx;
    return HALO_OK;
}

void halo_ctx_destroy(halo_ctx *ctx) {
    if (!ctx) return;
    multi_destroy(ctx);
    (void)hipSetDevice(ctx->device);
    for (auto st : ctx->streams) if (st) (void)hipStreamSynchronize(st);
    ctx->prof.collect();
    ctx->worker.stop();
    for (auto e : ctx->prof.pool) (void)hipEventDestroy(e);
    msm_workspace_free(ctx);
    foldtab_release(ctx);
    ipa_bufs_release(ctx);
    if (ctx->d_check_stage) {  // (optional memory of the check batch: off the budget's books before the key's remainder goes)
        (void)hipFree(ctx->d_check_stage);
        if (ctx->share) table_budget_release(ctx, ctx->check_stage_bytes);
        ctx->d_check_stage = nullptr;
    }
    if (ctx->share) {  // the key itself: freed by its last user (the tables went above, the same way)
        bool last;
        { std::lock_guard<std::mutex> lk(ctx->share->mu); last = --ctx->share->users == 0; }
        if (last) {  // (tables a user had given up while others still held them went nowhere: they go now)
            (void)hipFree(ctx->share->d_table);
            (void)hipFree(ctx->share->d_foldtab);
            ctx->share->d_table = ctx->share->d_foldtab = nullptr;
            table_budget_release(ctx, ctx->share->budget_held);
            (void)hipFree(ctx->share->d_bases);
        }
    } else {
        (void)hipFree(ctx->d_bases);
    }
    (void)hipFree(ctx->d_tmp_a);
    (void)hipFree(ctx->d_tmp_b);
    (void)hipFree(ctx->d_tmp_c);
    (void)hipFree(ctx->d_poly);
    (void)hipFree(ctx->d_poly2);
    (void)hipFree(ctx->d_verify);
    (void)hipFree(ctx->d_degree_rows);
    for (auto p : ctx->d_slot_scalars) (void)hipFree(p);
    if (ctx->h_pinned) (void)hipHostFree(ctx->h_pinned);
    if (ctx->h_wintab) (void)hipHostFree(ctx->h_wintab);
    if (ctx->h_open_pinned) (void)hipHostFree(ctx->h_open_pinned);
    for (auto &pair : ctx->ev_piece) for (auto e : pair) if (e) (void)hipEventDestroy(e);
    for (auto st : ctx->streams) if (st) (void)hipStreamDestroy(st);
    delete ctx;
}

size_t halo_ctx_size(const halo_ctx *ctx) { return ctx ? ctx->n : 0; }
void *halo_ctx_bases_dev(halo_ctx *ctx) { return ctx ? ctx->d_bases : nullptr; }
void *halo_ctx_stream(halo_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }

int halo_ctx_read_bases(halo_ctx *ctx, size_t off, size_t n, uint64_t *out) {
    HALO_CTX(ctx);
    if (!out) { set_error("read_bases: range"); return HALO_E_ARG; }
    int rc = msm_request(ctx, 0, false, off, n, nullptr, 0, nullptr);
    if (rc) return rc;
    rc = aff_native_to_words(ctx, ctx->d_bases + 32 * off, n, ctx->d_tmp_a);
    if (rc) return rc;
    return download_words(ctx, out, ctx->d_tmp_a, n * 8);
}

int halo_public_points(uint64_t S_out[12], uint64_t H_out[12]) {
    host::Point g = host::Point::generator();
    g.mul(host::urs_scalar(0)).store_normalized(S_out);
    g.mul(host::urs_scalar(1)).store_normalized(H_out);
    return HALO_OK;
}
}  // extern "C"
