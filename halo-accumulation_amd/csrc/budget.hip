// The budget for optional device memory (the MSM fixed-base table, the fold table, the batch staging), per device and
// process-wide, with the setters that decide what a context may spend it on and halo_ctx_info, which reports both; and the
// other thing a caller asks a context about: the profiler behind HALO_LAUNCH (internal.hpp) with its halo_prof_* hooks.
#include "internal.hpp"

namespace halo {
namespace {
struct DeviceBudget { size_t budget = 0, used = 0; bool known = false; };
std::mutex g_budget_mu;
DeviceBudget g_budget[64];
// HALO_MEMORY_BUDGET=<bytes>[K|M|G] in the environment (read by tuning()) replaces the default (for hosts that cannot call the setter: the Rust shim)
DeviceBudget &budget_of(int device) {  // (g_budget_mu held; the device is current)
    DeviceBudget &b = g_budget[device & 63];
    if (!b.known) {
        b.known = true;
        size_t free_b = 0, total = 0;
        if (tuning().memory_budget_set) b.budget = tuning().memory_budget;
        else if (hipMemGetInfo(&free_b, &total) == hipSuccess) b.budget = total / 6;  // 48 GB of an MI355X's 288
        else (void)hipGetLastError();
    }
    return b;
}
}  // namespace
bool table_budget_reserve(halo_ctx *ctx, size_t bytes) {
    std::lock_guard<std::mutex> lk(g_budget_mu);
    DeviceBudget &b = budget_of(ctx->device);
    size_t free_b = 0, total = 0;
    if (hipMemGetInfo(&free_b, &total) != hipSuccess) { (void)hipGetLastError(); return false; }
    if (b.used + bytes > b.budget || free_b / 2 < bytes) {
        if (debug_trace()) fprintf(stderr, "[halo] optional table of %zu bytes refused on device %d: %zu of %zu budget bytes in use, %zu free\n", bytes, ctx->device, b.used, b.budget, free_b);
        return false;
    }
    b.used += bytes;
    ctx->share->budget_held += bytes;  // (on the books of the key: a clone may outlive the context that built a table)
    return true;
}
bool table_budget_room(halo_ctx *ctx, size_t bytes, size_t freed) {
    std::lock_guard<std::mutex> lk(g_budget_mu);
    DeviceBudget &b = budget_of(ctx->device);
    return b.used - (freed < b.used ? freed : b.used) + bytes <= b.budget;
}
void table_budget_release(halo_ctx *ctx, size_t bytes) {
    std::lock_guard<std::mutex> lk(g_budget_mu);
    DeviceBudget &b = g_budget[ctx->device & 63];
    if (bytes > ctx->share->budget_held) bytes = ctx->share->budget_held;
    ctx->share->budget_held -= bytes;
    b.used = b.used >= bytes ? b.used - bytes : 0;
}

// ------------------------------------------------------------------ measurement hooks
int Profiler::find(const char *name) {
    for (size_t i = 0; i < entries.size(); ++i)
        if (std::strcmp(entries[i].name, name) == 0) return (int)i;
    ProfEntry e;
    e.name = name;
    entries.push_back(e);
    return (int)entries.size() - 1;
}
void Profiler::begin(const char *name, hipStream_t s) {
    Pending p;
    p.idx = find(name);
    auto get = [&]() {
        hipEvent_t e;
        if (!pool.empty()) { e = pool.back(); pool.pop_back(); }
        else (void)hipEventCreate(&e);
        return e;
    };
    p.a = get();
    p.b = get();
    (void)hipEventRecord(p.a, s);
    pending.push_back(p);
}
void Profiler::end(hipStream_t s) { (void)hipEventRecord(pending.back().b, s); }
void Profiler::collect() {
    for (auto &p : pending) {
        float ms = 0;
        if (hipEventSynchronize(p.b) == hipSuccess && hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
            entries[p.idx].total_ms += ms;
            entries[p.idx].launches += 1;
        }
        pool.push_back(p.a);
        pool.push_back(p.b);
    }
    pending.clear();
}

// (a multi-device context: the shards profile too, and count/get show the sums over parent and shards per kernel name)
static int prof_enable_one(halo_ctx *ctx, int on, bool reset) {
    HALO_HIP(hipSetDevice(ctx->device));
    for (int k = 0; k < HALO_SLOTS; ++k) HALO_HIP(hipStreamSynchronize(ctx->streams[k]));
    ctx->prof.collect();
    if (reset) {
        for (auto &e : ctx->prof.entries) { e.total_ms = 0; e.launches = 0; }
    } else {
        ctx->prof.on = on != 0;
        ctx->prof.dominant_only = on == 2;
    }
    return HALO_OK;
}
static int prof_enable_all(halo_ctx *ctx, int on, bool reset) {
    HALO_CTX(ctx);
    for (halo_ctx *s : ctx->shards) { int rc = prof_enable_one(s, on, reset); if (rc) return rc; }
    return prof_enable_one(ctx, on, reset);
}
static void prof_merge(halo_ctx *ctx) {
    ctx->prof_merged = ctx->prof.entries;
    for (halo_ctx *s : ctx->shards)
        for (const ProfEntry &e : s->prof.entries) {
            bool found = false;
            for (ProfEntry &m : ctx->prof_merged)
                if (std::strcmp(m.name, e.name) == 0) { m.total_ms += e.total_ms; m.launches += e.launches; found = true; break; }
            if (!found) ctx->prof_merged.push_back(e);
        }
}
}  // namespace halo

using namespace halo;

extern "C" {
int halo_set_table_mode(halo_ctx *ctx, int mode) {
    if (!ctx || mode < -1 || mode > 1) { set_error("table mode must be -1 (automatic), 0 (never) or 1 (automatic, fixed-window plan only)"); return HALO_E_ARG; }
    if (mode == 0 && ctx->d_table) {  // "no table memory": a table already built is released, not just left unused
        HALO_CTX(ctx);
        int rc = table_release(ctx);
        if (rc) return rc;
    }
    ctx->table_mode = mode;
    ctx->table_retry_at = 0;
    ctx->table_status = 0;
    for (halo_ctx *sh : ctx->shards) (void)halo_set_table_mode(sh, mode);  // a multi-device context: its shards run the MSMs
    return HALO_OK;
}
int halo_set_fold_table(halo_ctx *ctx, int mode) {
    if (!ctx || mode < -1 || mode > 1) { set_error("fold table mode must be -1 (automatic), 0 (never) or 1 (at the first full-size open)"); return HALO_E_ARG; }
    if (mode == 0) {  // releases the table, and whatever the helper thread of the automatic mode has obtained
        HALO_CTX(ctx);
        for (int k = 0; k < HALO_SLOTS; ++k) HALO_HIP(hipStreamSynchronize(ctx->streams[k]));
        foldtab_release(ctx);
        ctx->table_demote = false;
        std::lock_guard<std::mutex> lk(ctx->share->mu);
        ctx->share->table_fixed_only = false;
    }
    if (mode == 1 && !ctx->d_foldtab && !table_budget_room(ctx, foldtab_need_bytes(ctx->n)) && table_should_demote(ctx)) {
        // the caller asks for the fold table and the budget has room for it only without this context's all-shifts MSM table: that one goes
        HALO_CTX(ctx);
        (void)table_demote_now(ctx);
    }
    ctx->fold_table_mode = mode;
    ctx->foldtab_retry_at = 0;  // (a table that could not be had before is considered again)
    ctx->foldtab_status = 0;
    return HALO_OK;
}

int halo_set_memory_budget(halo_ctx *ctx, size_t bytes) {
    HALO_CTX(ctx);
    {
        std::lock_guard<std::mutex> lk(g_budget_mu);
        DeviceBudget &b = budget_of(ctx->device);
        b.budget = bytes;
    }
    // a table that was refused is considered again at the next opportunity
    ctx->foldtab_retry_at = 0; ctx->table_retry_at = 0;
    ctx->table_demote = false;
    { std::lock_guard<std::mutex> lk(ctx->share->mu); ctx->share->table_fixed_only = false; }
    for (halo_ctx *sh : ctx->shards) (void)halo_set_memory_budget(sh, bytes);  // (a shard on another device: that device's budget)
    return HALO_OK;
}
/* what: 0 = bytes of the MSM fixed-base table, 1 = bytes of the fold table, 2 = microseconds its build took, 3 = the budget for optional
 * table memory on this context's device, 4 = bytes of it in use (all contexts of the process), 5 / 6 = status of the fold table / the
 * MSM table: 0 nothing yet, 1 memory requested, 2 built, 3 over the budget, 4 allocation failed (tried again later), 5 off,
 * 7 = microseconds the MSM table's build took, 8 = its rows (13 / 15: fixed windows, 255: every shift, the sliding-window plan),
 * 9 = plan of the launch enqueued last: 0 no table pipeline, 1 its fixed windows, w + 1 sliding windows of at most w bits,
 * 10 = members of the last open-type batch call that went through member-batched launches (0: one at a time) */
size_t halo_ctx_info(const halo_ctx *ctx, int what) {
    if (!ctx) return 0;
    if (what == 0) return ctx->d_table ? (size_t)ctx->tbl.rows * ctx->n * 128 : 0;
    if (what == 7) return (size_t)(ctx->share ? ctx->share->table_build_ms * 1e3 : 0);
    if (what == 8) return ctx->d_table ? (size_t)ctx->tbl.rows : 0;
    if (what == 9) return (size_t)(ctx->last_table_plan + 1);
    if (what == 10) return ctx->open_batch_members;
    if (what == 1) return ctx->foldtab_bytes;
    if (what == 2) return (size_t)(ctx->foldtab_build_ms * 1e3);
    if (what == 3 || what == 4) {
        std::lock_guard<std::mutex> lk(g_budget_mu);
        DeviceBudget &b = g_budget[ctx->device & 63];
        if (!b.known) {  // (the default is a fraction of THIS device's memory: asked once, the caller's current device is put back)
            int prev = -1;
            (void)hipGetDevice(&prev);
            (void)hipSetDevice(ctx->device);
            (void)budget_of(ctx->device);
            if (prev >= 0) (void)hipSetDevice(prev);
        }
        return what == 3 ? b.budget : b.used;
    }
    if (what == 5) return ctx->fold_table_mode == 0 ? 5 : ctx->d_foldtab ? 2 : (size_t)ctx->foldtab_status;
    if (what == 6) return ctx->table_mode == 0 ? 5 : ctx->d_table ? 2 : (size_t)ctx->table_status;
    return 0;
}

int halo_prof_enable(halo_ctx *ctx, int on) { return prof_enable_all(ctx, on, false); }
int halo_prof_reset(halo_ctx *ctx) { return prof_enable_all(ctx, 0, true); }
int halo_prof_count(halo_ctx *ctx) {
    if (!ctx) return 0;
    prof_merge(ctx);
    return (int)ctx->prof_merged.size();
}
int halo_prof_get(halo_ctx *ctx, int i, const char **name, double *total_ms, long *launches) {
    if (!ctx || i < 0 || i >= (int)ctx->prof_merged.size()) { set_error("prof_get: index (call halo_prof_count first)"); return HALO_E_ARG; }
    if (name) *name = ctx->prof_merged[i].name;
    if (total_ms) *total_ms = ctx->prof_merged[i].total_ms;
    if (launches) *launches = ctx->prof_merged[i].launches;
    return HALO_OK;
}
}  // extern "C"
