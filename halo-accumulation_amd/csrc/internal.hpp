// Internal declarations shared by the translation units of libhalo_hip.so.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/halo_accumulation.h"
#include "host_math.hpp"
#include "kernel_args.hpp"
#include "tuning.hpp"

namespace halo {

void set_error(const std::string &msg);
int hip_fail(hipError_t e, const char *what);

#define HALO_HIP(expr)                                   \
    do {                                                 \
        hipError_t _e = (expr);                          \
        if (_e != hipSuccess) return hip_fail(_e, #expr); \
    } while (0)

struct ProfEntry {
    const char *name;
    double total_ms = 0;
    long launches = 0;
};

struct Profiler {
    bool on = false;
    bool dominant_only = false;  // bracket only k_msm_accumulate / k_fold_points (2 events per MSM)
    std::vector<ProfEntry> entries;
    struct Pending { int idx; hipEvent_t a, b; };
    std::vector<Pending> pending;
    std::vector<hipEvent_t> pool;
    int find(const char *name);
    void begin(const char *name, hipStream_t s);
    void end(hipStream_t s);
    void collect();  // needs the stream to be idle
};

// k_msm_accumulate, k_smsm_accumulate, k_fold_points, k_fold_points4
inline bool prof_is_dominant(const char *name) {
    return name[2] == 'm' ? name[6] == 'a' : name[2] == 's' ? name[7] == 'a' : (name[2] == 'f' && name[7] == 'p');
}
// Launch wrapper: brackets the launch with events when profiling is on.
#define HALO_LAUNCH(ctx, name, kernel, grid, block, shmem, ...)                              \
    do {                                                                                     \
        bool _p = (ctx)->prof.on && (!(ctx)->prof.dominant_only || halo::prof_is_dominant(name)); \
        if (_p) (ctx)->prof.begin(name, (ctx)->stream);                                      \
        if (halo::debug_trace()) fprintf(stderr, "[halo] launch %s ctx=%p stream=%p\n", name, (void *)(ctx), (void *)(ctx)->stream); \
        hipLaunchKernelGGL(kernel, grid, block, shmem, (ctx)->stream, __VA_ARGS__);          \
        if (_p) (ctx)->prof.end((ctx)->stream);                                              \
    } while (0)

struct MsmPlan {
    int c;        // window bits
    int W;        // windows = ceil(256 / c)
    uint32_t B;   // buckets per window = 2^(c-1)
    int batch;    // MSMs sharing the launch sequence (their windows are laid side by side: W * batch in all)
    int w0, w1;   // windows [w0, w1) of 0..W are computed (a window-sharded partial); the result carries 2^(c*w0)
    // the fixed-base table pipeline (pipeline >= 2): window sums by rows and columns of the bucket index (msm_buckets.hip
    // k_msm_reduce_rc); h_winsum holds (2^lg_cols + 2^lg_rows) / 64 pairs (S, T) per piece and set
    int table_pieces = 1;    // a large table MSM runs as this many consecutive pieces
    int table_sets = 1;      // bucket sets side by side in a batched table launch (members, rounded up to a power of two)
    int table_rc_lg_rows = 0, table_rc_lg_cols = 0;
    // the sliding odd-digit plan over the all-shifts table (TblPlan::slide): bucket index = range * 2^lg_cols + fine holds the
    // digits of magnitude 2 (fine * 2^lg_rows + range) + 1 -- other constants in msm_combine_member, same (S, T) pairs
    int table_slide = 0;  // (its window width)
    // > 0: the launch's last kernel(s) write their sums straight into the slot's pinned buffer and each adds one to the slot's
    // pinned counter when its last block is through (MsmWorkspace::h_done; one per piece); msm_wait polls the counter.  0: a copy
    // and a stream wait.
    int publishers = 0;
    // What the launch sequence chose for its window sums, noted where it computes them.  Nothing in the product reads these: the
    // development library reports them (halo_dev_msm_last_plan), so that a test can assert the plan its case was built for.
    int pipeline = 0;          // 0 general, 1 small (smsm.hip), 2 table with fixed windows, 3 table sliding
    int winsum_form = 0;       // 0 k_msm_reduce1 + k_smsm_final, 1 k_smsm_reduce (+ k_smsm_final beyond one segment), 2 k_msm_reduce_rc + k_rc_mid
    uint32_t kmax = 0;         // longest chain of the bucket kernel: a bucket of more entries is several tasks
    uint32_t red_L = 0, red_nseg = 0;  // forms 0, 1: buckets per lane / quad, segments per window
    int red_logL = 0, red_live_seg = 0;
    int table_rc_per = 0;      // form 2: buckets per lane of k_msm_reduce_rc
};
constexpr int MSM_MAX_BATCH = 8;
constexpr size_t REDUCE_WAVES = 1024;  // most waves of k_msm_reduce1 / k_smsm_reduce: one per SIMD (msm_general.hip, smsm.hip)
// fixed-base table plan of a context (msm_table.hip: table_plan)
struct TblPlan {
    int c, W, fbits;                 // window bits, windows, fine-bucket bits of a coarse range
    uint32_t B, ranges, spread;      // buckets (2^(c-1)), coarse ranges, modulus of the top-window spread (0: none)
    int fold_top;                    // scalars >= 2^254 are recoded as r - s with flipped signs (c = 17: the top window is full)
    // The table of a c = 20 key may hold EVERY shift, rows 0 .. 254 (`rows` = 255: T[j][i] = 2^j G_i) instead of the W rows 2^(c w) G_i.
    // slide > 0 (21): the launch recodes its scalars into sliding windows of at most `slide` bits that start at set bits only (odd
    // digits, slide_lane.hpp), a digit names its own row, coarse range = bucket & (ranges - 1), fine key = bucket >> log2(ranges).
    // slide = 0 on such a table: the fixed windows, window w on row row_step * w (row_step = c).
    // Only slide = 21 is built: B = 2^19, the 19-bit bucket field of a digit word (TBL_ROW_SHIFT) and the 512 x 1024 shape of the
    // window sums are those of 21-bit windows; a width of 20 (2^18 buckets) would have to derive all three from it.
    // rbits = log2(ranges).
    int rows, row_step, slide, rbits;
};
TblPlan table_plan(size_t key_n);
// the members of a batched launch: same n, one scalar array and one base offset (in points) each
struct MsmBatch {
    int count = 1;
    const uint64_t *scalars[MSM_MAX_BATCH] = {};
    uint32_t base_off[MSM_MAX_BATCH] = {};
    int part = 0, parts = 1;  // window shard: this launch computes windows [part*W/parts, (part+1)*W/parts)
    int c_hint = 0;           // window bits the caller knows to be better for THIS launch's scalars (0: the size-based table); halo_set_window_bits wins
    // TWO sums from ONE scalar array (count = 1, canonical form, c = 20 table plan only: msm_tagged_ready): bit 255 of scalar i --
    // free, r < 2^255 -- says which of two bucket sets point i goes to.  One recode / sort / bucket kernel / window-sum pass for
    // both; results as for a batch of two (msm_wait(.., 2), msm_combine_member 0 / 1).  The IPA's L and R over the full key.
    bool tagged = false;
    // A stretch of a LARGER sum over the context's key (halo_msm with host scalars: the stretches run on different slots, each
    // behind the copy of its own scalars): takes the c = 20 table plan although n is below its usual 2^20 points.
    bool sub = false;
};
struct MemberOffsets { uint32_t v[MSM_MAX_BATCH]; };  // ... as a kernel argument (the sort kernels of msm_general.hip and smsm.hip)
inline int msm_outputs(const MsmBatch &m) { return m.tagged ? 2 : m.count; }
inline MsmBatch msm_one(const uint64_t *scalars) { MsmBatch one; one.scalars[0] = scalars; return one; }
MsmPlan msm_plan(size_t n, int forced_c);
uint32_t msm_spread(const MsmPlan &p, uint32_t *top_bit);  // top-window spread of the recode (0: none)

struct MsmWorkspace {
    size_t cap_n = 0;
    uint64_t *d_canon = nullptr;     // u16 signed digits, layout [w][i]
    uint32_t *d_hist = nullptr;      // per (window, chunk) bucket histograms / prefixes
    uint32_t *d_counts = nullptr;    // W*B
    uint32_t *d_starts = nullptr;    // W*B exclusive scan within 4096-entry blocks
    uint32_t *d_blockoff = nullptr;  // per 4096-entry block offset
    uint32_t *d_sorted = nullptr;    // n*W entries: point index | sign << 31
    uint32_t *d_presort = nullptr;   // the same entries grouped by bucket range only (two-level sort of large MSMs)
    uint32_t *d_buckets = nullptr;   // one native XYZZ partial (40 words) per task
    uint32_t *d_ntask = nullptr, *d_toff = nullptr, *d_tblockoff = nullptr, *d_biglist = nullptr, *d_meta = nullptr;
    uint32_t *d_task_g = nullptr, *d_order = nullptr;  // per task: bucket | length bin << 24; task records (4 words) by decreasing length
    uint16_t *d_fine16 = nullptr;    // table pipeline: low bucket bits beside d_presort (allocated on first use)
    uint32_t *d_seg = nullptr;       // W*64 x 2 native XYZZ (S, T per 512-bucket segment)
    uint64_t *d_winsum = nullptr;    // W x 12 (Jacobian)
    uint64_t *h_winsum = nullptr;    // pinned
    uint32_t *h_done = nullptr;      // pinned: blocks that have published their sums, ever (see MsmPlan::publishers)
    uint32_t done_expect = 0;        // ... and what it reads once the launches enqueued so far are done
    size_t cap_counts = 0, cap_sorted = 0, cap_tasks = 0, cap_hist = 0, cap_windows = 0;
    MsmPlan plan{};          // plan of the MSM in flight on this slot
    bool in_flight = false;
    bool launched = false;   // a launch has been enqueued on this workspace: `plan` is that launch's (halo_dev_msm_last_plan)
    int lent_from = -1;      // this slot's workspace and stream run the odd pieces of the large MSM in flight on slot `lent_from`
    int borrowed = -1;       // ... and that slot remembers which one it borrowed (msm_wait gives it back)
    // hipGraph of the launch sequence, replayed while the same (bases, scalars, n, form, window) repeats
    struct GraphKey {
        const void *bases = nullptr;
        MsmBatch members;
        size_t n = 0;
        int mont = 0, c = 0, span = 0;
        bool operator==(const GraphKey &o) const {
            if (!(bases == o.bases && n == o.n && mont == o.mont && c == o.c && span == o.span && members.count == o.members.count &&
                  members.part == o.members.part && members.parts == o.members.parts && members.c_hint == o.members.c_hint && members.tagged == o.members.tagged && members.sub == o.members.sub))
                return false;
            for (int b = 0; b < members.count; ++b)
                if (members.scalars[b] != o.members.scalars[b] || members.base_off[b] != o.members.base_off[b]) return false;
            return true;
        }
    };
    // Launch graphs of this slot, by key: an open's rounds come back with the same few keys open after open (the tagged launch of
    // rounds 0-1, the batches over the 2^18-, 2^16- and 2^14-point keys, the check's MSM), so the slot keeps several -- with ONE
    // graph a slot re-captured and re-instantiated four of them per open and launched the other four rounds kernel by kernel.
    static constexpr int GRAPHS = 8, SEEN = 8;
    struct CachedGraph { GraphKey key; hipGraphExec_t exec = nullptr; MsmPlan plan{}; uint64_t used = 0; };
    CachedGraph graphs[GRAPHS];
    GraphKey seen[SEEN];       // keys that have arrived once (plain launches): the second arrival is captured
    int seen_at = 0;
    uint64_t graph_epoch = 0;  // the context's alloc_epoch the graphs were instantiated under (all go when it moves)
    uint64_t graph_clock = 0;  // least recently used goes first
};

}  // namespace halo

constexpr int HALO_SLOTS = 4;

namespace halo {
// One helper thread per context for pure host arithmetic that would otherwise serialise on the caller's thread
// (the window combine of the second MSM of an IPA round while the caller combines the first); a shard of a multi-device
// context also runs its own HIP calls on it (multi.hip: copies, launches and the stream wait of its stretch of an MSM, on
// its own device).  While an IPA state of the context is alive (`hot` counts them) a round arrives every few hundred
// microseconds and a condition-variable wake-up would cost a good part of what the overlap saves, so after a job
// the thread polls for the next one -- but only for SPIN_US: an idle state (a caller thinking between rounds, a long
// sharded open waiting on a collective) does not hold a core; the thread falls back to the condition variable.
class HostWorker {
   public:
    ~HostWorker() { stop(); }
    void submit(std::function<void()> fn) {
        start();
        job_ = std::move(fn);
        done_.store(false, std::memory_order_relaxed);
        { std::lock_guard<std::mutex> lk(mu_); pending_.store(true, std::memory_order_release); }
        cv_.notify_one();
    }
    // A job of pure host arithmetic ends within tens of microseconds: poll for it.  A job that sits in hipStreamSynchronize
    // for the length of an MSM (multi.hip: a shard's stretch) would make the caller burn a core per shard for milliseconds:
    // after SPIN_US of polling the caller sleeps on a condition variable instead.
    void wait() {
        if (!thread_.joinable()) return;
        auto t0 = std::chrono::steady_clock::now();
        while (!done_.load(std::memory_order_acquire)) {
            if (std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count() < SPIN_US) {
                std::this_thread::yield();
                continue;
            }
            std::unique_lock<std::mutex> lk(mu_);
            done_cv_.wait(lk, [this] { return done_.load(std::memory_order_acquire); });
        }
    }
    // one call per IPA state created (+1) / destroyed (-1)
    void add_hot(int delta) {
        int now = hot_.fetch_add(delta, std::memory_order_relaxed) + delta;
        if (delta > 0 && now > 0) start();
    }
    void stop() {
        if (!thread_.joinable()) return;
        { std::lock_guard<std::mutex> lk(mu_); quit_.store(true); }
        cv_.notify_one();
        thread_.join();
    }

   private:
    static constexpr long SPIN_US = 600;
    void start() {
        if (thread_.joinable()) return;
        done_.store(true);
        thread_ = std::thread([this] { loop(); });
    }
    void loop() {
        auto last = std::chrono::steady_clock::now();
        for (;;) {
            if (!pending_.load(std::memory_order_acquire)) {
                if (quit_.load()) return;
                if (hot_.load(std::memory_order_relaxed) > 0 &&
                    std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - last).count() < SPIN_US) {
                    std::this_thread::yield();
                    continue;
                }
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [this] { return pending_.load() || quit_.load(); });
                continue;
            }
            pending_.store(false, std::memory_order_relaxed);
            job_();
            { std::lock_guard<std::mutex> lk(mu_); done_.store(true, std::memory_order_release); }  // (under the lock: a waiter about to sleep cannot miss it)
            done_cv_.notify_all();
            last = std::chrono::steady_clock::now();
        }
    }
    std::thread thread_;
    std::mutex mu_;
    std::condition_variable cv_, done_cv_;
    std::function<void()> job_;
    std::atomic<bool> pending_{false}, done_{true}, quit_{false};
    std::atomic<int> hot_{0};
};
// ---- fr_vec.hip: a row of k_poly_degree_batch's table in device memory -- len Montgomery scalars at src (32-byte aligned, only
// read); top: 0 on the way in, index + 1 of the row's last non-zero scalar (0: none) on the way out
struct DegreeRow {
    const uint64_t *src;
    uint64_t len;
    uint32_t top, pad;
};
constexpr uint32_t DEG_LANES = 256;   // lanes of a block: DEG_LANES / 2 scalars a pass
constexpr uint32_t DEG_CHUNK = 1024;  // scalars of a row per block
}  // namespace halo

// Device buffers of one pcdl::open (pcdl.rs:183-186 state + the no-fold vectors), owned by the context and reused
// from open to open: the open path performs no device allocation after the first call.
struct IpaBuffers {
    uint32_t *d_G = nullptr;                                       // cap_n x 32 words (native affine, 128-B stride)
    uint64_t *d_c = nullptr, *d_z = nullptr;                       // cap_n x 4
    uint64_t *d_s = nullptr, *d_s2 = nullptr, *d_FL = nullptr, *d_FR = nullptr;  // cap_M x 4
    uint64_t *d_pbar = nullptr;                                    // cap_n x 4, hiding branch of a sharded open (lazy)
    size_t cap_n = 0, cap_M = 0;
    bool in_use = false;
};

namespace halo {
// What the contexts over ONE resident key have in common (halo_ctx_clone): the key, its fixed-base MSM table and its fold
// table -- immutable once built -- and the optional-memory bytes they hold on the device's books.  Every context owns a
// reference (a context that was never cloned is the only user of its own); the last one to go frees the memory.  `mu` guards
// the fields; a table is built by ONE context at a time (`*_busy`), the others run table-free meanwhile and adopt it at their
// next opportunity.
struct KeyShare {
    std::mutex mu;
    int users = 1;
    uint32_t *d_bases = nullptr;
    uint32_t *d_table = nullptr;
    TblPlan tbl{};
    double table_build_ms = 0;  // build of d_table (kernels, without the allocation)
    uint32_t *d_foldtab = nullptr;
    size_t foldtab_bytes = 0;
    double foldtab_build_ms = 0;
    bool table_busy = false, foldtab_busy = false;
    bool table_fixed_only = false;  // the key's all-shifts MSM table made room for the fold table: table_build keeps to the fixed windows (until halo_set_fold_table(ctx, 0) or a new budget)
    long full_opens = 0;     // full-size opens over this key by any of its contexts while no fold table existed (the automatic mode builds from tuning().fold_table_after on)
    size_t budget_held = 0;  // bytes of optional memory reserved for this key (budget.hip table_budget_*)
};
}  // namespace halo

struct halo_ctx {
    int device = 0;
    std::shared_ptr<halo::KeyShare> share;  // d_bases / d_table / d_foldtab below are this context's view of it
    hipStream_t stream = nullptr;      // stream the launch macro uses (= streams[slot in use])
    hipStream_t streams[HALO_SLOTS] = {};
    size_t n = 0;
    uint32_t *d_bases = nullptr;  // n x 32 words (AFF_STRIDE): native affine x | y | -y, one 128-byte line per point (curve.hpp AffN)
    uint32_t *sink_done = nullptr;             // while a launch is being enqueued: the counter its last kernel publishes to (null: copy + stream wait)
    int sink_publishers = 0;                   // ... and how many blocks will
    halo::MsmWorkspace wss[HALO_SLOTS];        // slots (workspace + stream) so that independent MSMs can overlap
    halo::Profiler prof;
    std::vector<halo::ProfEntry> prof_merged;  // what halo_prof_count / _get show: this context's entries plus its shards'
    int window_bits = 0;
    int reduce_span = 0;                   // buckets per lane in k_msm_reduce1 (0 = automatic)
    int sort_two_level = -1;               // two-level sort: -1 automatic (n >= 2^17), 0 never, 1 whenever the shape allows
    int task_len = 0;                      // longest chain per lane in k_msm_accumulate (0 = automatic)
    int table_mode = -1;                   // fixed-base tables for MSMs over the context's own bases: -1 automatic (n >= 2^20), 0 never, 1 as -1 with the fixed-window plan forced (no all-shifts table is built; one that exists is read through its row stride)
    uint32_t *d_table = nullptr;           // tbl.rows x n native affine points: T[w][i] = 2^(c w) G_i, or every shift T[j][i] = 2^j G_i (built on first use)
    halo::TblPlan tbl{};                   // the plan d_table was built for
    int small_path = -1;                   // smsm.hip pipeline: -1 automatic (n <= 2^16, one MSM per launch), 0 never
    bool use_graphs = true;                // replay cached hipGraphs for repeated MSM shapes
    size_t nofold_size = (size_t)1 << 14;  // key size at which the IPA stops folding G (0/1 = never)
    bool batch_verify = true;              // succinct checks of >= 64 instances in two device launches (else a host thread pool)
    int fold_table_mode = -1;              // comb table for the first fold of an open (foldtab.hip): -1 after tuning().fold_table_after (8) full-size opens over the key -- memory requested on a helper thread, built at the first later open that finds it; 1 at the next open; 0 never
    uint32_t *d_foldtab = nullptr;         // E[w][d][i - n/4] = d 64^w G_i, 64-byte affine entries
    size_t foldtab_bytes = 0;
    double foldtab_build_ms = 0;
    int foldtab_opens = 0;                 // full-size opens seen while the table did not exist
    // A table that could not be had (budget, allocation) is tried again later, with a doubling back-off, instead of never:
    // memory comes back when other contexts go.  status: 0 nothing yet, 1 memory requested, 2 built, 3 over the
    // memory budget, 4 allocation or build failed, 5 off (halo_ctx_info 5 / 6)
    int foldtab_retry_at = 0, foldtab_backoff = 8, foldtab_status = 0;
    long table_calls = 0, table_retry_at = 0, table_backoff = 64;
    int table_status = 0;
    // The all-shifts MSM table (34 GB at 2^20 points) and the fold table (35 + 5 GB) do not both fit the default budget, and the
    // fold table saves an opening workload more.  The decision is per KEY (msm_table.hip table_should_demote): a fold table that the
    // budget refused beside an all-shifts table which only this context uses, and that would fit without it, asks for the MSM table
    // to be taken down to its 13 rows (table_demote: done at the next MSM enqueued with every slot idle, or at once by
    // halo_set_fold_table(ctx, 1) and by halo_ctx_clone, whose callers open); KeyShare::table_fixed_only then keeps table_build from
    // asking for the large table again.  A table that clones share is never taken from them: the fold table is refused with its
    // usual back-off and line on stderr -- and a key with clones builds the large table only if the budget holds both.
    bool table_demote = false;
    bool table_said = false, foldtab_said = false;  // the one line on stderr has been printed
    // (the optional-memory bytes are on the books of the key: share->budget_held)
    // automatic mode: the table's 40 GB are requested on a helper thread at the first full-size open (hipMalloc of that size
    // takes 0.5 ms .. 2 s depending on what the driver has at hand) and the table is built at the first later open that
    // finds them there.  state: 0 nothing, 1 running, 2 ready, 3 failed
    std::thread foldtab_alloc_thread;
    std::atomic<int> foldtab_alloc_state{0};
    uint32_t *foldtab_pending = nullptr, *foldtab_pending_tmp = nullptr;
    int fold_levels = 2;                   // halving rounds folded into G at a time (1: every round; 2: every other round, k_fold_points4)
    int fold_async = -1;                   // folds of keys of <= 2^18 points beside the next two rounds: -1 in opens of <= 2^18 points (measured), 0 never, 1 always (halo_set_fold_async)
    // scratch for host-pointer entry points
    uint64_t *d_tmp_a = nullptr, *d_tmp_b = nullptr, *d_tmp_c = nullptr;
    size_t tmp_words = 0;
    uint64_t *h_pinned = nullptr;  // small pinned staging (4 KiB)
    uint64_t *h_wintab = nullptr;  // pinned staging of a window table of powers (fr_vec.hip upload_window_table), 8 KiB
    uint64_t *d_slot_scalars[HALO_SLOTS] = {};  // scalar staging per slot (msm_entry.hip slot_scalars): host scalars, a shard's peer copies
    size_t slot_scalars_bytes[HALO_SLOTS] = {};
    uint64_t *d_verify = nullptr;  // staging of the batched verifier (points, scalars, challenges, results), grown on demand
    size_t verify_words = 0;
    halo::DegreeRow *d_degree_rows = nullptr;  // the table of halo_poly_degrees_dev and of the device-row batches (fr_vec.hip poly_degrees_dev), grown on demand
    size_t degree_bytes = 0;
    // staging of halo_pcdl_check_batch / halo_acc_decider_batch (pcdl_batch.hip): h coefficients and tables of the members in flight.
    // Optional memory (on the budget of halo_set_memory_budget; released at destroy), only grown, so its address stays put
    uint64_t *d_check_stage = nullptr;
    size_t check_stage_bytes = 0;
    // (the same staging holds the member state of halo_pcdl_open_batch / halo_random_instance_batch; these are their per-slot
    // constants and results in pinned memory, allocated at the first batched open)
    uint64_t *h_open_pinned = nullptr;
    // lazily allocated n x 4 polynomial buffers for pcdl::open / acc::prover
    uint64_t *d_poly = nullptr, *d_poly2 = nullptr;
    halo::HostWorker worker;      // host arithmetic overlapped with the caller's (see HostWorker; multi.hip also runs a shard's HIP calls on it)
    IpaBuffers ipa_bufs;          // reused by every halo_ipa of this context (one at a time; a second one allocates its own)
    uint64_t alloc_epoch = 0;     // bumped whenever this context allocates or frees device memory (see msm_driver.hip, launch graphs)
    size_t open_batch_members = 0;  // members of the last open-type batch call that ran through member-batched launches (0: one at a time; halo_ctx_info 10)
    int last_table_plan = -1;     // the launch enqueued last: -1 no table pipeline, 0 its fixed windows, else the sliding plan's window width (halo_ctx_info 9)
    int may_borrow = 0;           // > 0 inside a synchronous MSM call: a large MSM may run its odd pieces on the neighbouring slot (msm_driver.hip)
    hipEvent_t ev_piece[HALO_SLOTS][2] = {};  // fork / join of those pieces (created on first use)
    // multi-device contexts (multi.hip): one shard context per device over its index block of the key; MSMs over the key fan out
    std::vector<halo_ctx *> shards;
    std::vector<size_t> shard_lo;  // shards.size() + 1 block boundaries
    halo_ctx *parent = nullptr;    // set on a shard
    // the MSM(s) in flight over the shards on each slot: `count` members over GS[off, off + n); batch: begun by
    // halo_msm_dev_batch_begin, which alone collects it
    struct Fan { bool active = false, batch = false; int count = 0; size_t off = 0, n = 0; };
    Fan fan[HALO_SLOTS];
};

// Elements that the context's temporaries (d_tmp_a / _b) and each slot's scalar staging hold: the key's size, at least 64
inline size_t ctx_capacity(const halo_ctx *ctx) { return ctx->n < 64 ? 64 : ctx->n; }

struct halo_ipa {
    halo_ctx *ctx = nullptr;
    size_t n = 0, m = 0;  // m = current length (n, n/2, ...)
    IpaBuffers buf;  // the context's own set (borrowed: returned by halo_ipa_destroy) or a private one (freed there); d_G is folded in
                     // place, d_c / d_z hold the m live elements, d_s .. d_FR are the no-fold vectors (M x 4), d_pbar this shard of p_bar
    const uint32_t *G_src = nullptr;  // where the current key is read from: the context's own table of bases until the first real
                                      // fold (no copy, and its MSMs may use the context's fixed-base table), d_G afterwards
    halo::host::FixedBaseTable hp_table;  // window table of the H' this open uses (pcdl.rs:181)
    bool hp_from_scalar = false;          // H' = hp_scalar * H: terms k * H' come from the process-wide table of H as (k * hp_scalar) * H
    halo::host::Fr hp_scalar;
    hipEvent_t ev = nullptr;  // orders slot 1's stream after the folds queued on stream 0
    // no-fold mode (fr_vec.hip): G stays at M points, s holds the challenge products
    bool nofold = false;
    bool deferred = false;                   // the no-fold phase ends in a two-level fold once s_len reaches 4
    std::vector<halo::host::Fr> s_host;      // host copy of s while deferred (<= 4 entries)
    size_t M = 0, s_len = 0;
    bool pbar_valid = false;     // halo_ipa_hiding_partial has filled buf.d_pbar for this state
    // The LAST round of a no-fold phase already holds U (ipa_state.hip halo_ipa_finish): with two coefficients c0, c1 left, its MSMs are
    // L' = c1 A and R' = c0 B over the even / odd points of the key, and U = G_final[0] = A + xi B.  Kept here: L', R' before
    // their H' terms, c0, c1 (copied to the host with the round's results) and the round's challenge.
    bool last_valid = false, last_folded = false;
    halo::host::Point last_L, last_R;
    halo::host::Fr last_c0, last_c1, last_xi, last_xi_inv;
    // A two-level fold of a key of at most 2^18 points is a latency chain on one wave per SIMD (1.6 and 1.1 ms in a 2^20 open):
    // it runs on the context's fourth stream BESIDE the next two rounds, which keep reading the unfolded key (ipa_state.hip
    // ipa_round_fold_impl).  fold_pending: launched, not yet switched to; fold_dst / fold_m: its output; tail_host: the products
    // of the challenges hashed since (they are the first entries of d_s and the scalars of the fold after this one);
    // g_off: points of d_G already taken by earlier keys (the folds no longer run in place).
    bool fold_pending = false;
    uint32_t *fold_dst = nullptr;
    size_t fold_m = 0, g_off = 0;
    std::vector<halo::host::Fr> tail_host;
    hipEvent_t ev_fold = nullptr;
    bool counted_hot = false;    // this state is counted in ctx->worker's hot count (undone by halo_ipa_destroy)
    bool borrowed = false;       // buf is ctx->ipa_bufs (returned, not freed, by halo_ipa_destroy)
};

namespace halo {

// ---- msm_driver.hip (the fixed-base table: msm_table.hip)
// scope of a synchronous MSM call (nothing else of the caller's can be in flight on the context's other slots meanwhile)
struct BorrowScope {
    halo_ctx *c;
    explicit BorrowScope(halo_ctx *ctx) : c(ctx) { c->may_borrow++; }
    ~BorrowScope() { c->may_borrow--; }
};
// the launch macro uses ctx->stream: a slot's own stream for the launches of a scope
struct StreamGuard {
    halo_ctx *ctx;
    hipStream_t saved;
    StreamGuard(halo_ctx *c, hipStream_t s) : ctx(c), saved(c->stream) { c->stream = s; }
    ~StreamGuard() { ctx->stream = saved; }
};
// The slots a batched call may use: no MSM of the caller's in flight, not lent to a neighbour's large MSM, no fan-out over the
// shards.  out[0 .. count), in slot order.
inline int idle_slots(const halo_ctx *ctx, int out[HALO_SLOTS]) {
    int S = 0;
    for (int k = 0; k < HALO_SLOTS; ++k)
        if (!ctx->wss[k].in_flight && ctx->wss[k].lent_from < 0 && !ctx->fan[k].active) out[S++] = k;
    return S;
}
// The outcomes of a batched call in member order: status[i] (nullable) = code_of(i), on_fail(i) for every failing member (its
// output zeroed, or nothing).  Returns the first failing member's code with the message "<noun> <i>: <err_of(i)>", else 0.
template <class CodeOf, class ErrOf, class OnFail>
int report_members(const char *noun, size_t m, CodeOf code_of, ErrOf err_of, int *status, OnFail on_fail) {
    size_t first = m;
    for (size_t i = 0; i < m; ++i) {
        const int rc = code_of(i);
        if (status) status[i] = rc;
        if (!rc) continue;
        on_fail(i);
        if (first == m) first = i;
    }
    if (first == m) return HALO_OK;
    set_error(std::string(noun) + " " + std::to_string(first) + ": " + err_of(first));
    return code_of(first);
}
// a context's count of its own device (de)allocations
inline void alloc_epoch_bump(halo_ctx *ctx) { ctx->alloc_epoch++; }
int msm_workspace_alloc(halo_ctx *ctx, size_t n, int slot);
void msm_workspace_free(halo_ctx *ctx);
int table_release(halo_ctx *ctx);  // gives up the context's fixed-base table (every slot idle): freed unless a clone still uses it
void table_detach(halo_ctx *ctx);   // the same without the idle check (context teardown)
// asynchronous halves of msm_run on workspace/stream `slot`
int msm_enqueue(halo_ctx *ctx, int slot, const uint32_t *d_bases, const uint64_t *d_scalars, bool scalars_mont, size_t n);
int msm_finish(halo_ctx *ctx, int slot, host::Point *out);
// the two halves of msm_finish: wait for the slot's launches (HIP), then combine the window sums (pure host arithmetic,
// may run on another thread); batch as msm_finish_batch
int msm_wait(halo_ctx *ctx, int slot, int count);
void msm_combine(halo_ctx *ctx, int slot, host::Point *out, int count);
void msm_combine_member(halo_ctx *ctx, int slot, int b, host::Point *out);
// the same for `members.count` MSMs of n points each issued as ONE launch sequence; out[count]
int msm_enqueue_batch(halo_ctx *ctx, int slot, const uint32_t *d_bases, const MsmBatch &members, bool scalars_mont, size_t n);
bool msm_tagged_ready(const halo_ctx *ctx, const uint32_t *d_bases, size_t n);  // can a `tagged` launch (MsmBatch) over these points run now?
int msm_finish_batch(halo_ctx *ctx, int slot, host::Point *out, int count);
// sum scalars[i] * bases[i]; bases affine (device), scalars device; result host Jacobian (un-normalised)
// bases: native affine table (20 words per point)
int msm_run(halo_ctx *ctx, const uint32_t *d_bases, const uint64_t *d_scalars, bool scalars_mont, size_t n, host::Point *out);
// fn(0) .. fn(m - 1) on a bounded pool of host threads (at most 16; the caller's thread takes part)
inline void pool_run(size_t m, const std::function<void(size_t)> &fn) {
    unsigned hw = std::thread::hardware_concurrency();
    size_t nthreads = hw ? hw : 4;
    if (nthreads > 16) nthreads = 16;
    if (nthreads > m) nthreads = m;
    std::atomic<size_t> next{0};
    auto worker = [&]() { for (size_t i; (i = next.fetch_add(1)) < m;) fn(i); };
    std::vector<std::thread> th;
    for (size_t t = 1; t < nthreads; ++t) th.emplace_back(worker);
    worker();
    for (auto &t : th) t.join();
}
// ---- urs.hip (key generation and the affine layouts)
int urs_generate(halo_ctx *ctx, uint64_t first_index, uint64_t stride, size_t n, uint32_t *d_out_native);
int batch_to_affine(halo_ctx *ctx, const uint64_t *d_jac_words, size_t n, uint32_t *d_out_native);
int aff_words_to_native(halo_ctx *ctx, const uint64_t *d_in, size_t n, uint32_t *d_out);
int aff_native_to_words(halo_ctx *ctx, const uint32_t *d_in, size_t n, uint64_t *d_out);

// ---- budget.hip: the budget for OPTIONAL device memory (the MSM fixed-base table, the fold table and its temporary), per device and
// process-wide: reserve() succeeds if what all contexts of this process hold on ctx's device plus `bytes` stays within the
// device's budget (halo_set_memory_budget; default 1/6 of the device's memory) and at least 2 x bytes are free right now
bool table_budget_reserve(halo_ctx *ctx, size_t bytes);
bool table_budget_room(halo_ctx *ctx, size_t bytes, size_t freed = 0);  // would `bytes` more stay within the budget once `freed` bytes have gone back?  (reserves nothing)
size_t foldtab_need_bytes(size_t n);                 // foldtab.hip: the fold table of an n-point key and its build's temporary
bool table_should_demote(halo_ctx *ctx);             // msm_table.hip: this context alone holds an all-shifts table, and the key's fold table fits the budget only without it
bool fold_table_wanted(const halo_ctx *ctx);         // msm_table.hip: the key may still ask for a fold table (mode 1, or the automatic mode at its sizes)
int table_demote_now(halo_ctx *ctx);                 // msm_table.hip: that table goes (every slot idle, no other user); the next table MSM builds the fixed windows
void table_budget_release(halo_ctx *ctx, size_t bytes);

// ---- foldtab.hip: the first two-level fold of an open from a comb table over the context's key
void foldtab_cancel_alloc(halo_ctx *ctx);  // joins the helper thread and frees what it obtained
int fold_points4_tab(halo_ctx *ctx, const uint32_t *d_src, uint32_t *d_dst, size_t m, const host::Fr s[3], int form = 0);  // 1 = done, 0 = not applicable
void foldtab_release(halo_ctx *ctx);
void fold_digits_host(const host::Fr &s, int8_t out[44]);

// ---- multi.hip: MSMs over the key of a multi-device context, cut along the shards' blocks
int multi_attach_shards(halo_ctx *ctx, const int *devices, int n_dev, const uint64_t *bases_affine, uint64_t first_index);
void multi_destroy(halo_ctx *ctx);
bool multi_takes(const halo_ctx *ctx, const uint32_t *d_bases, size_t n);  // a stretch of the parent's own key?
constexpr size_t MULTI_RUN_MIN = (size_t)1 << 16;  // synchronous MSMs over the key fan out from this many points (msm_run)
// members over GS[off, off + n) on every shard's slot `slot` (host: one member in host memory); collected by count
int multi_batch_begin(halo_ctx *ctx, int slot, size_t off, size_t n, const MsmBatch &members, bool mont, bool host, bool batch);
int multi_batch_end(halo_ctx *ctx, int slot, host::Point *out, int count);
int multi_run(halo_ctx *ctx, size_t off, size_t n, const uint64_t *dev_scalars, bool mont, host::Point *out);
int multi_host_run(halo_ctx *ctx, size_t off, size_t n, const uint64_t *scalars, bool mont, host::Point *out);  // synchronous, host scalars, per shard msm_host_run
// ---- msm_entry.hip: the checked request path, host-scalar MSMs and the scalar staging buffers
// (out null: the range check alone, halo_ctx_read_bases)
int msm_request(const halo_ctx *ctx, int slot, bool fan, size_t off, size_t n, const void *const *scalars, size_t count, MsmBatch *out);
uint64_t *slot_scalars(halo_ctx *ctx, int slot, int members, int m);  // member m's array in slot `slot`'s buffer (null: allocation failed)
int msm_host_begin(halo_ctx *ctx, int slot, size_t off, size_t n, const uint64_t *scalars, bool mont);
int msm_host_run(halo_ctx *ctx, size_t off, size_t n, const uint64_t *scalars, size_t valid, int mont, host::Point *out);  // synchronous, zero-padded beyond `valid`
int msm_end_slot(halo_ctx *ctx, int slot, size_t count, uint64_t *out);  // `count` results of whatever begin started `slot` (halo_msm_end_sharded)

// ---- smsm.hip: the 4-launch pipeline for MSMs of up to 2^16 points (digits already in ws.d_canon)
// (winsum may be pinned host memory; done: the counter to publish to, or null)
int quad_final_enqueue(halo_ctx *ctx, MsmWorkspace &ws, uint32_t Wt, uint32_t nseg, int k, uint64_t *winsum, uint32_t *done = nullptr);
int rc_mid_enqueue(halo_ctx *ctx, const uint32_t *entries, uint32_t blocks, uint64_t *winsum, uint32_t *done = nullptr, uint32_t *ticket = nullptr);
// (offs: one base offset per member, in points; a block of k_smsm_sort sorts one window, so one member)
int smsm_enqueue(halo_ctx *ctx, MsmWorkspace &ws, const uint32_t *d_bases, const MemberOffsets &offs, size_t n, MsmPlan &p, uint32_t Wt,
                 uint32_t kmax);
int smsm_prepare();

// ---- key_fold.hip
// (form: 0 in the product -- the sizes pick the kernel form; halo_dev_fold_points forces one, include/halo_accumulation_dev.h)
int ipa_fold_points(halo_ctx *ctx, uint32_t *d_G, size_t m, const host::Fr &xi_mont, int form = 0);
int ipa_fold_points4(halo_ctx *ctx, const uint32_t *d_src, uint32_t *d_dst, size_t m, const host::Fr s[3], int form = 0);
// ---- fr_vec.hip
int ipa_fold_scalars(halo_ctx *ctx, uint64_t *d_c, uint64_t *d_z, size_t m, const host::Fr &xi, const host::Fr &xi_inv);
// out[0] = <xs0, ys0>, out[1] = <xs1, ys1> (either pair may be null to skip)
int fr_dot2(halo_ctx *ctx, const uint64_t *xs0, const uint64_t *ys0, const uint64_t *xs1, const uint64_t *ys1, size_t m,
            host::Fr out[2]);
int fr_dot2_launch(halo_ctx *ctx, const uint64_t *xs0, const uint64_t *ys0, const uint64_t *xs1, const uint64_t *ys1, size_t m);  // on ctx->stream
int fr_dot2_collect(halo_ctx *ctx, hipStream_t stream, size_t m, host::Fr out[2]);
int fr_powers(halo_ctx *ctx, const host::Fr &z, size_t n, uint64_t *d_out);
// d_v[i] *= a
int fr_scale(halo_ctx *ctx, uint64_t *d_v, size_t n, const host::Fr &a);
int fr_poly_eval(halo_ctx *ctx, const uint64_t *d_coeffs, size_t len, const host::Fr &z, host::Fr *out);
// SplitMix64 stream -> n Montgomery scalars (element i = draws 4i+1..4i+4 after state0)
int rng_scalars_dev(halo_ctx *ctx, uint64_t state0, size_t n, uint64_t *d_out);
int pbar_dev(halo_ctx *ctx, const uint64_t *d_q, size_t deg, const host::Fr &z, uint64_t *d_out);
int axpy_dev(halo_ctx *ctx, uint64_t *d_y, const uint64_t *d_x, size_t n, const host::Fr &a);
int pbar_stream_dev(halo_ctx *ctx, uint64_t state0, size_t deg, const host::Fr &z, uint64_t stride, uint64_t offset, size_t n_local,
                    uint64_t *d_out);
int bench_fr_kernel(halo_ctx *ctx, int which, size_t n, int reps);
int nofold_expand(halo_ctx *ctx, const uint64_t *d_c, const uint64_t *d_s, size_t m, size_t M, uint64_t *d_L, uint64_t *d_R);
int nofold_expand_tagged(halo_ctx *ctx, const uint64_t *d_c, const uint64_t *d_s, size_t m, size_t M, uint64_t *d_F);  // one array for a tagged launch
int nofold_s_update(halo_ctx *ctx, const uint64_t *d_s_in, size_t len, const host::Fr &xi, uint64_t *d_s_out);
// ---- hpoly.hip
// d_out[k] (+)= scale * prod_{bit i of k} xis[lg_n - i]
int h_coeffs_dev(halo_ctx *ctx, const host::Fr *xis, size_t lg_n, const host::Fr &scale, bool accumulate, uint64_t *d_out);
// m of them at once, scale one: tables (d_tabs, m x 3072 words) built on the device from d_xis (m x (lg_n + 1) x 4), member b's
// coefficients at d_out + b * out_stride (bit-identical to h_coeffs_dev per member)
int h_coeffs_batch_dev(halo_ctx *ctx, const uint64_t *d_xis, size_t m, size_t lg_n, uint64_t *d_tabs, uint64_t *d_out, size_t out_stride);
constexpr size_t H_TABLES_WORDS = 3 * 256 * 4;
// h(X) = h_0 + sum_i scale_i h_i(X) of several members at once (k_h_tables with scales + k_h_accumulate_batch; acc.rs:85-94):
// member b's polynomials are xis[i] (lg_n + 1 challenges each) with scales[i], i < count
struct HAccMember {
    const host::Fr *h0 = nullptr;  // two coefficients
    std::vector<const host::Fr *> xis;
    const host::Fr *scales = nullptr;
    size_t count = 0;
};
constexpr size_t HACC_REC_WORDS = 10;  // a member's record: first table | count << 32, mode, h_0
// words of the pinned / device staging of one call with G members and room for `cap` tables per pass
constexpr size_t hacc_pin_words(size_t G, size_t lg_n, size_t cap) { return G * HACC_REC_WORDS + cap * (lg_n + 2) * 4; }
inline size_t hacc_stage_words(size_t G, size_t lg_n, size_t cap) { return hacc_pin_words(G, lg_n, cap) + cap * H_TABLES_WORDS; }
int h_accumulate_group(halo_ctx *ctx, const HAccMember *mem, size_t G, size_t lg_n, size_t cap, uint64_t *h_stage, uint64_t *d_stage, uint64_t *d_out,
                       size_t out_stride);
// s = sum_a r_a h_a(X) over A polynomials in P parts, `cap` tables per pass (hpoly.hip; halo_pcdl_check_batch_combined): the
// device staging's layout is the A records | the part records (rounded up to 32 bytes) | cap tables | P rows of n elements,
// and row 0 (hcomb_rows) holds s when the launches on ctx->stream are through
inline size_t hcomb_part_words(size_t A, size_t P, size_t cap) {
    if (cap > A) cap = A;
    return (((A + cap - 1) / cap) * P * HACC_REC_WORDS + 3) & ~(size_t)3;
}
inline size_t hcomb_rows_offset(size_t A, size_t lg_n, size_t P, size_t cap) {
    return A * (lg_n + 2) * 4 + hcomb_part_words(A, P, cap) + (cap > A ? A : cap) * H_TABLES_WORDS;
}
inline size_t hcomb_stage_words(size_t A, size_t lg_n, size_t P, size_t cap) { return hcomb_rows_offset(A, lg_n, P, cap) + P * (((size_t)1 << lg_n) * 4); }
int h_combine_rows(halo_ctx *ctx, const uint64_t *h_recs, size_t A, size_t lg_n, size_t P, size_t cap, uint64_t *d_stage);
// ... over polynomials of their own lengths 2^lgs[a] <= 2^lg_max, zero-padded to the row (halo_pcdl_check_batch_mixed_combined): the
// records at the fixed stride of lg_max + 2 elements in the caller's order, sorted by decreasing length inside; the staging holds
// the A lgs (32 bits each, rounded up to 32 bytes) behind the records, else the layout above
inline size_t hmix_lg_words(size_t A) { return ((A + 1) / 2 + 3) & ~(size_t)3; }
inline size_t hmix_rows_offset(size_t A, size_t lg_max, size_t P, size_t cap) { return hcomb_rows_offset(A, lg_max, P, cap) + hmix_lg_words(A); }
inline size_t hmix_stage_words(size_t A, size_t lg_max, size_t P, size_t cap) { return hcomb_stage_words(A, lg_max, P, cap) + hmix_lg_words(A); }
int h_combine_rows_mixed(halo_ctx *ctx, const uint64_t *h_recs, const uint32_t *lgs, size_t A, size_t lg_max, size_t P, size_t cap, uint64_t *d_stage);
// fr_vec.hip: rows[0] = the sum of P rows of n elements at `stride` words (k_fr_sum_rows; P = 1 launches nothing), on ctx->stream
int fr_sum_rows(halo_ctx *ctx, uint64_t *d_rows, size_t stride, size_t P, size_t n);
int h_eval_batch(halo_ctx *ctx, const uint64_t *d_xis, size_t m, size_t lg_n, const host::Fr &z, uint64_t *d_out);
// m polynomials h_i at their own points z_i
int h_eval_each(halo_ctx *ctx, const uint64_t *d_xis, const uint64_t *d_zs, size_t m, size_t lg_n, uint64_t *d_out);
// ---- fused_check.hip: the term scalars of the fused check batch (k_fused_terms + the sum of H's shares), on ctx->stream; the record
// and scalar layouts are fused_lane.hpp's (lg + 6 Montgomery elements in, 2 lg + 2 canonical scalars out per member)
// d_desc (nullable): the members' own sizes and offsets, mixed_terms_lane.hpp's descriptors -- the mixed fused check batch, whose
// records and scalars lie dense (mixed_terms.hip: k_mixed_terms in k_fused_terms' place; mixed_terms_launch is the launch alone)
int fused_terms(halo_ctx *ctx, const uint64_t *d_recs, size_t M, size_t lg, const uint32_t *d_desc, uint64_t *d_scalars, uint64_t *d_shares, uint64_t *d_h);
int mixed_terms_launch(halo_ctx *ctx, const uint64_t *d_recs, const uint32_t *d_desc, size_t M, uint64_t *d_scalars, uint64_t *d_shares);
// ---- small_sums.hip: m sums of K scalar multiples (canonical scalars, affine points) -> m Jacobian points
int batch_small_msm(halo_ctx *ctx, const uint64_t *d_points, const uint64_t *d_scalars, size_t m, size_t K, uint64_t *d_out);
// sums of 1..64 terms each, several to a wave (k_small_msm_seg): sum s holds terms sum_off[s] .. sum_off[s + 1] (same term
// format as above).  plan: the lane descriptor (64 words per wave) -> the number of waves; the launch writes nsums Jacobian points
size_t small_msm_seg_plan(const uint32_t *sum_off, size_t nsums, std::vector<uint32_t> &desc);
int small_msm_seg(halo_ctx *ctx, const uint64_t *d_points, const uint64_t *d_scalars, const uint32_t *d_sum_off, const uint32_t *d_desc, size_t waves,
                  uint64_t *d_out);

// ---- fr_vec.hip: the member-batched kernels of halo_pcdl_open_batch (pcdl_batch.hip).  G <= OPEN_MAX_GROUP members per launch,
// blockIdx.y = member.  Member b's vectors sit at b * ms words from the base pointers; its window table, constants, partial sums
// and results at b * OPEN_*_WORDS in the group's own regions.
constexpr int OPEN_MAX_GROUP = 4;
constexpr size_t OPEN_TAB_WORDS = 1024, OPEN_CONST_WORDS = 32, OPEN_PART_WORDS = 1024, OPEN_OUT_WORDS = 32;
// The largest batched open.  What is sized from it: a member's window table (16 (1 + nwin) + E entries of 4 words, nwin = 5 windows
// of 4 bits and a chain of E <= 64 here; open_batch_table refuses a table of more than OPEN_TAB_WORDS / 4 entries), its partial
// records (the grids of open_batch_eval and open_batch_dots are capped to what OPEN_PART_WORDS holds and their lanes stride), the
// prover batch's pinned records (pcdl_batch.hip HACC_PIN_WORDS) and the 32-bit element counts and base offsets of the kernels.
constexpr size_t OPEN_MAX_LG = 19, OPEN_MAX_N = (size_t)1 << OPEN_MAX_LG;
static_assert((16 * (1 + (OPEN_MAX_LG + 3) / 4) + 64) * 4 <= OPEN_TAB_WORDS, "a member's window table at OPEN_MAX_N");
static_assert((uint64_t)OPEN_MAX_GROUP * (OPEN_MAX_N / 2) < ((uint64_t)1 << 31), "base offsets of the staged keys: 31-bit point indices");
// One member's constants in device memory (uploaded once per step of a group, never kernel arguments): N-form multipliers
// (kernel_args.hpp FsArg: 9 x 29-bit limbs) and Montgomery limbs (FeArg: 8 x 32 bits)
struct OpenConst {
    FsArg xi_n, xi_inv_n, alpha_n, z64_n;
    FeArg xi_m, z_m;
    uint64_t s_q;  // rng state before q of p_bar (deg scalars)
    uint64_t s_p;  // rng state before p of random_instance (deg + 1 scalars)
    uint32_t deg;  // the member's degree
    uint32_t len;  // axpy: coefficients of p' = p + alpha p_bar (deg + 1)
    uint32_t pad[6];
};
// (the host fills an array of these and the kernels index records of OPEN_CONST_WORDS: the two strides must agree)
static_assert(sizeof(OpenConst) == OPEN_CONST_WORDS * 8, "OpenConst record");
// host: member's window table of z (powers and p(z) over n coefficients) into h_tab (OPEN_TAB_WORDS), z and z^64 into k
int open_batch_table(const host::Fr &z, size_t n, uint64_t *h_tab, OpenConst *k);
void open_const_xi(OpenConst *k, const host::Fr &xi, const host::Fr &xi_inv);
void open_const_alpha(OpenConst *k, const host::Fr &alpha);
// on ctx->stream; outs: the group's result records (OPEN_OUT_WORDS each): v at +0, dot_l / dot_r at +4 / +8
int open_batch_eval(halo_ctx *ctx, int G, const uint64_t *d_coeffs, size_t ms, size_t n, const uint64_t *d_tabs, uint64_t *d_parts, uint64_t *d_outs);
int open_batch_powers(halo_ctx *ctx, int G, const uint64_t *d_tabs, const uint64_t *d_consts, size_t n, uint64_t *d_z, size_t ms);
int open_batch_pbar(halo_ctx *ctx, int G, const uint64_t *d_consts, size_t n, uint64_t *d_out, size_t ms);
int open_batch_rng(halo_ctx *ctx, int G, const uint64_t *d_consts, size_t n, uint64_t *d_out, size_t ms);
int open_batch_axpy(halo_ctx *ctx, int G, uint64_t *d_y, const uint64_t *d_x, size_t ms, size_t n, const uint64_t *d_consts);
int open_batch_expand(halo_ctx *ctx, int G, const uint64_t *d_c, const uint64_t *d_s, size_t ms, size_t m, size_t M, uint64_t *d_L, uint64_t *d_R);
int open_batch_dots(halo_ctx *ctx, int G, const uint64_t *d_c, const uint64_t *d_z, size_t ms, size_t m, uint64_t *d_parts, uint64_t *d_outs);
// s_out[2t + u] = s_in[t] xi^u (t < s_len), then c' = c_l + xi^-1 c_r, z' = z_l + xi z_r over m
int open_batch_fold(halo_ctx *ctx, int G, uint64_t *d_c, uint64_t *d_z, const uint64_t *d_s_in, uint64_t *d_s_out, size_t ms, size_t m,
                    size_t s_len, const uint64_t *d_consts);
// ---- key_fold.hip: the member-batched key folds (blockIdx.y = member).  Member b reads d_src + b * src_stride points (0: one key for
// all) and writes d_dst + b * dst_stride (may be its source); its digits are record b of d_digs, FOLD_DIG_WORDS 32-bit words of
// device memory that fold_digits fills on the host from the fold's scalars: xi (levels 1) or s1 | s2 | s3 (levels 2).
// form: 0 = the single launchers' rule over all G x m outputs; 1 / 2 = one / two outputs per lane; 3 = one per quad (4 only)
constexpr size_t FOLD_DIG_WORDS = 64;
void fold_digits(const host::Fr *s, int levels, uint32_t *rec);
int ipa_fold_points_batch(halo_ctx *ctx, int G, const uint32_t *d_src, size_t src_stride, uint32_t *d_dst, size_t dst_stride, size_t m,
                          const uint32_t *d_digs, int form = 0);
int ipa_fold_points4_batch(halo_ctx *ctx, int G, const uint32_t *d_src, size_t src_stride, uint32_t *d_dst, size_t dst_stride, size_t m,
                           const uint32_t *d_digs, int form = 0);
// ---- fr_vec.hip: the member-batched padding of halo_pcdl_commit_dev_batch (pcdl_batch.hip).  Entry k of the table: src[k], len[k]
// Montgomery scalars in device memory (32-byte aligned), copied to d_out + row[k] * ms words and zero-padded to n scalars.  The
// table travels as a kernel argument; count <= MSM_MAX_BATCH entries, one launch on ctx->stream.
struct PadMembers {
    const uint64_t *src[MSM_MAX_BATCH];
    uint32_t len[MSM_MAX_BATCH];
    uint32_t row[MSM_MAX_BATCH];
};
int pad_members_batch(halo_ctx *ctx, const PadMembers &t, int count, size_t n, uint64_t *d_out, size_t ms);
// ---- fr_vec.hip: degrees_out[i] = the index of row i's last non-zero scalar, 0 for none (host_poly_degree, found on the device:
// k_poly_degree_batch); rows as dev_rows_ok accepts them
int poly_degrees_dev(halo_ctx *ctx, const void *const *d_coeffs, const size_t *lens, size_t m, size_t *degrees_out);
// the pointer conventions of every entry point over device rows: lens[i] = 0 with a null pointer is the zero polynomial; a null
// pointer with a length, a misaligned pointer or a null table is HALO_E_ARG ("<who>: null or misaligned pointer")
inline int dev_rows_ok(const char *who, const void *const *d_coeffs, const size_t *lens, size_t m) {
    bool ok = m == 0 || (d_coeffs && lens);
    for (size_t i = 0; i < m && ok; ++i) ok = !((lens[i] && !d_coeffs[i]) || ((uintptr_t)d_coeffs[i] & 31));
    if (!ok) set_error(std::string(who) + ": null or misaligned pointer");
    return ok ? HALO_OK : HALO_E_ARG;
}

// ---- decompress.hip: point decompression of the wire format on the device (wire.hip halo_*_decode_batch)
constexpr size_t DECOMP_IN_WORDS = 6;    // a point's 33 wire bytes, zero-padded to 48
constexpr size_t DECOMP_OUT_WORDS = 14;  // 12 Jacobian blob words, ok, pad
constexpr size_t SQRT_TAB_WORDS = 4 * 256 * 8 + 256;  // 32-bit words of the square root's torsion tables
const uint32_t *sqrt_tables_host();  // built on first use (null: the lookup limbs collide -- never for this field)
int point_decompress_dev(halo_ctx *ctx, const uint64_t *d_in, size_t n, const uint32_t *d_tab, uint64_t *d_out);  // on ctx->stream
int fq_sqrt_dev(halo_ctx *ctx, const uint64_t *d_a, size_t n, const uint32_t *d_tab, uint64_t *d_root, uint32_t *d_ok);
// ---- pcdl_batch.hip: the context's staging for batched calls (optional memory), grown to `want` x per_bytes if the budget
// allows; returns how many units of per_bytes it holds (0: none)
size_t check_stage(halo_ctx *ctx, size_t want, size_t per_bytes);

// ---- ctx.hip
// process-wide window table of the public point H (consts.rs:45-65), built on first use
const host::FixedBaseTable &public_h_table();
const host::FixedBaseTable &public_s_table();  // (k S and k H from the process-wide window tables: ~14 us against ~80 for a generic double-and-add)
// synchronous copies of 64-bit words on ctx->stream
int upload_words(halo_ctx *ctx, uint64_t *dst, const uint64_t *src, size_t words);
int download_words(halo_ctx *ctx, uint64_t *dst, const uint64_t *src, size_t words);
// ---- ipa_state.hip
// halo_ipa_begin over coefficients in device memory (padded to n); the z vector: d_z_vec if given, else z_base^j (times *z_scale if given)
int ipa_begin_dev(halo_ctx *ctx, size_t n, const uint64_t *d_coeffs_padded, const host::Fr &z_base, halo_ipa **out, const host::Fr *z_scale = nullptr,
                  const uint64_t *d_z_vec = nullptr);
// H' = xi0 * H for this state (pcdl.rs:181): lets the rounds use the process-wide window table of H
void ipa_set_hprime_scalar(halo_ipa *st, const host::Fr &xi0);
void ipa_bufs_release(halo_ctx *ctx);  // frees the context's own IPA buffers (no state may be borrowing them)


// ---- pcdl_acc.hip, msm_sharded.hip: the collectives of the sharded entry points (include/halo_accumulation.h, "sharded open /
// check"): the caller's all-gather with ONE status word behind every rank's record
// The development library's hooks "shard_fail_rank" / "shard_fail_at" (DevHooks; never the environment): the rank with that
// offset fails locally (HALO_E_DEVICE) before collective number `at` of a sharded open (0 = the share of p(z), 1.. = the rounds,
// then the tail), or, with at = SHARD_AT_CHECK, in a sharded check, or, with at = SHARD_AT_MSM, before the collective of a
// sharded MSM -- what tests/test_sharded_gloo.py, tests/test_gpu_pcdl_acc.py and tests/test_gpu_msm_sharded.py use to drive
// the failure path
constexpr long SHARD_AT_CHECK = -2, SHARD_AT_MSM = -3;
inline int shard_test_failure(uint64_t offset, long step) {
    const DevHooks &h = dev_hooks();
    if (h.shard_fail_rank < 0 || (uint64_t)h.shard_fail_rank != offset) return HALO_OK;
    if ((long)h.shard_fail_at != step) return HALO_OK;
    set_error("sharded call: local failure injected by the development library's shard_fail hook");
    return HALO_E_DEVICE;
}
struct StatusGather {
    size_t P;
    uint64_t offset;
    halo_allgather_fn fn;
    void *user;
    const char *who;
    std::vector<uint64_t> sbuf, rbuf;
    // all-gather of `words` record words + this rank's status; recv = P x words.  Returns the first non-zero status in rank
    // order (the same value on every rank), HALO_E_ARG if the collective itself failed, else 0.
    int run(const uint64_t *rec, size_t words, int local_rc, std::vector<uint64_t> &recv) {
        recv.assign(P * words, 0);
        if (!fn) {  // one rank, no callback: nothing to agree on
            if (local_rc) return local_rc;
            std::memcpy(recv.data(), rec, words * 8);
            return HALO_OK;
        }
        sbuf.assign(words + 1, 0);
        if (!local_rc) std::memcpy(sbuf.data(), rec, words * 8);
        sbuf[words] = (uint64_t)(int64_t)local_rc;
        rbuf.assign(P * (words + 1), 0);
        std::string own = local_rc ? halo_last_error() : "";
        if (fn(user, sbuf.data(), words + 1, rbuf.data())) {
            set_error(std::string(who) + ": the caller's all-gather failed (abort the process group: the ranks are no longer in step)");
            return HALO_E_ARG;
        }
        for (size_t r = 0; r < P; ++r) {
            int st = (int)(int64_t)rbuf[r * (words + 1) + words];
            if (!st) continue;
            if (r == offset || local_rc == st) set_error(own);  // (a rejection every rank found by itself keeps its own wording)
            else set_error(std::string(who) + ": rank " + std::to_string(r) + " failed locally (code " + std::to_string(st) + "); every rank returns its code");
            return st;
        }
        for (size_t r = 0; r < P; ++r) std::memcpy(&recv[r * words], &rbuf[r * (words + 1)], words * 8);
        return HALO_OK;
    }
};

}  // namespace halo

// guard used by every entry point that touches the device
#define HALO_CTX(ctx)                                                 \
    do {                                                              \
        if (!(ctx)) { halo::set_error("null context"); return HALO_E_ARG; } \
        hipError_t _e = hipSetDevice((ctx)->device);                  \
        if (_e != hipSuccess) return halo::hip_fail(_e, "hipSetDevice"); \
    } while (0)
