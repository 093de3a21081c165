// The IPA state behind halo_ipa_* (pcdl.rs:183-231): its device buffers, the begin forms, one round's L / R and dot products,
// the folds with their schedules (in place, no-fold, deferred two-level, beside the rounds) and finish.  The stream ordering
// between the context's four streams lives here and nowhere else.
#include "pcdl_internal.hpp"  // (is_pow2)

namespace halo {
// From a key of ctx->nofold_size points on the IPA stops folding G and runs its MSMs over the fixed key (fr_vec.hip): s starts at (1)
static int ipa_enter_nofold(halo_ipa *st) {
    halo_ctx *ctx = st->ctx;
    st->nofold = true;
    st->M = st->m;
    st->s_len = 1;
    uint64_t *one = ctx->h_pinned + 200;
    host::Fr::one().store(one);
    HALO_HIP(hipMemcpyAsync(st->buf.d_s, one, 32, hipMemcpyHostToDevice, ctx->stream));  // the pinned word always holds 1: no wait needed
    return HALO_OK;
}

static void ipa_bufs_free(IpaBuffers &b) {
    (void)hipFree(b.d_G); (void)hipFree(b.d_c); (void)hipFree(b.d_z);
    (void)hipFree(b.d_s); (void)hipFree(b.d_s2); (void)hipFree(b.d_FL); (void)hipFree(b.d_FR);
    (void)hipFree(b.d_pbar);
    b = IpaBuffers();
}
// n x (128 + 32 + 32) bytes of state and four cap_M-element vectors for the no-fold rounds
static int ipa_bufs_alloc(halo_ctx *ctx, IpaBuffers &b, size_t n, size_t M) {
    alloc_epoch_bump(ctx);
    b.cap_n = n;
    b.cap_M = M;
    bool ok = hipMalloc(&b.d_G, n * 128) == hipSuccess && hipMalloc(&b.d_c, n * 32) == hipSuccess && hipMalloc(&b.d_z, n * 32) == hipSuccess &&
              hipMalloc(&b.d_s, M * 32) == hipSuccess && hipMalloc(&b.d_s2, M * 32) == hipSuccess && hipMalloc(&b.d_FL, M * 32) == hipSuccess &&
              hipMalloc(&b.d_FR, M * 32) == hipSuccess;
    if (debug_trace()) fprintf(stderr, "[halo] ipa buffers ctx=%p n=%zu M=%zu G=[%p,+%zu) c=%p z=%p\n", (void *)ctx, n, M, (void *)b.d_G, n * 128, (void *)b.d_c, (void *)b.d_z);
    if (!ok) { ipa_bufs_free(b); set_error("ipa_begin: device allocation failed"); return HALO_E_DEVICE; }
    return HALO_OK;
}
void ipa_bufs_release(halo_ctx *ctx) {
    if (ctx->ipa_bufs.d_G) alloc_epoch_bump(ctx);
    ipa_bufs_free(ctx->ipa_bufs);
}

// z vector: d_z_vec if given, else z_base^j (times *z_scale if given)
int ipa_begin_dev(halo_ctx *ctx, size_t n, const uint64_t *d_coeffs_padded, const host::Fr &z_base, halo_ipa **out, const host::Fr *z_scale,
                  const uint64_t *d_z_vec) {
    halo_ipa *st = new (std::nothrow) halo_ipa();
    if (!st) { set_error("out of host memory"); return HALO_E_ARG; }
    st->ctx = ctx;
    st->n = st->m = n;
    int rc = HALO_OK;
    if (hipEventCreateWithFlags(&st->ev, hipEventDisableTiming) != hipSuccess) { delete st; set_error("ipa_begin: event"); return HALO_E_DEVICE; }
    if (hipEventCreateWithFlags(&st->ev_fold, hipEventDisableTiming) != hipSuccess) { (void)hipEventDestroy(st->ev); delete st; set_error("ipa_begin: event"); return HALO_E_DEVICE; }
    do {
        // The context's own buffers (sized for the whole key on first use) serve one state at a time: the opens of a
        // prover loop allocate nothing.  A second concurrent state of the same context gets private buffers.
        // the no-fold vectors span the key the MSMs run over: the whole key when folds are deferred (two levels at a time)
        bool defer = ctx->fold_levels >= 2 && n > ctx->nofold_size;
        size_t M = defer ? n : (n < ctx->nofold_size ? n : ctx->nofold_size);
        IpaBuffers &cb = ctx->ipa_bufs;
        if (!cb.in_use) {
            size_t want_n = ctx->n > n ? ctx->n : n, want_M = (ctx->fold_levels >= 2 || want_n < ctx->nofold_size) ? want_n : ctx->nofold_size;
            if (want_M < M) want_M = M;
            if (cb.cap_n < n || cb.cap_M < M) {
                for (int k = 0; k < HALO_SLOTS; ++k) (void)hipStreamSynchronize(ctx->streams[k]);
                ipa_bufs_release(ctx);
                rc = ipa_bufs_alloc(ctx, cb, want_n, want_M);
                if (rc) break;
            }
            cb.in_use = true;
            st->borrowed = true;
            st->buf = cb;  // (with the d_pbar an earlier hiding open left there)
        } else {
            rc = ipa_bufs_alloc(ctx, st->buf, n, M);  // (d_pbar stays null until a hiding branch asks for it)
            if (rc) break;
        }
        // The key is only copied when it is going to be folded in place round by round; the no-fold forms read the
        // context's own bases until the first real fold writes d_G (and may then use the context's fixed-base table).
        bool read_only_key = defer || n <= ctx->nofold_size;
        st->G_src = read_only_key ? ctx->d_bases : st->buf.d_G;
        if ((!read_only_key && hipMemcpyAsync(st->buf.d_G, ctx->d_bases, n * 128, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess) ||
            hipMemcpyAsync(st->buf.d_c, d_coeffs_padded, n * 32, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess) {
            set_error("ipa_begin: copy failed"); rc = HALO_E_DEVICE; break;
        }
        if (d_z_vec) {
            if (hipMemcpyAsync(st->buf.d_z, d_z_vec, n * 32, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess) {
                set_error("ipa_begin: copy failed"); rc = HALO_E_DEVICE; break;
            }
        } else {
            rc = fr_powers(ctx, z_base, n, st->buf.d_z);
            if (!rc && z_scale) rc = fr_scale(ctx, st->buf.d_z, n, *z_scale);
        }
        if (rc) break;
        if (n <= ctx->nofold_size || defer) rc = ipa_enter_nofold(st);
        st->deferred = defer;
        st->s_host.assign(1, host::Fr::one());
    } while (0);
    if (rc) { halo_ipa_destroy(st); return rc; }
    ctx->worker.add_hot(1);
    st->counted_hot = true;
    *out = st;
    return HALO_OK;
}

// the asserts of pcdl::open that every begin form shares
static int ipa_begin_checks(const halo_ctx *ctx, size_t n, size_t len) {
    if (!is_pow2(n)) { set_error("ipa_begin: n is not a power of two"); return HALO_E_ASSERT; }  // pcdl.rs:130
    if (n > ctx->n) { set_error("ipa_begin: n exceeds the commitment key (d <= D)"); return HALO_E_ASSERT; }  // pcdl.rs:132
    if (len > n) { set_error("ipa_begin: more coefficients than n (p.degree() <= d)"); return HALO_E_ASSERT; }  // pcdl.rs:131
    return HALO_OK;
}
// d_tmp_a = the caller's len coefficients, zero-padded to n
static int ipa_stage_coeffs(halo_ctx *ctx, size_t n, const uint64_t *coeffs, size_t len) {
    HALO_HIP(hipMemsetAsync(ctx->d_tmp_a, 0, n * 32, ctx->stream));
    return upload_words(ctx, ctx->d_tmp_a, coeffs, len * 4);
}

static host::Fr fr_pow_u64(const host::Fr &z, uint64_t e) {
    uint64_t ex[4] = {e, 0, 0, 0};
    return z.pow(ex);
}

void ipa_set_hprime_scalar(halo_ipa *st, const host::Fr &xi0) {
    st->hp_from_scalar = true;
    st->hp_scalar = xi0;
    (void)public_h_table();
}

// HALO_IPA_TIMING=1: where the host side of a round goes (printed when the state is destroyed; development aid)
namespace {
struct RoundTiming { double enqueue = 0, dots = 0, hterm = 0, wait = 0, combine = 0, fold = 0; long rounds = 0; };
thread_local RoundTiming g_rt;
const bool g_rt_on = tuning().ipa_timing;
inline double now_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
}
// <c_r, G_l>, <c_l, G_r> and the two dot products of one round, without the H' terms
// with_hterm: dot * H' is added to L (0) / R (1), each on the thread that combines it, and the sums come back normalised
static int ipa_round_lr_points(halo_ipa *st, host::Fr dots[2], host::Point *Lp_out, host::Point *Rp_out, bool with_hterm = false) {
    halo_ctx *ctx = st->ctx;
    if (st->m < 2) { set_error("ipa_round_lr: no rounds left"); return HALO_E_ARG; }
    size_t m = st->m / 2;
    int rc;
    bool batched = false;
    host::Point Lp, Rp;
    double t0 = g_rt_on ? now_us() : 0;
    // <c_r, G_l> on slot 0 and <c_l, G_r> on slot 1 run concurrently; the other streams first wait
    // for everything queued on stream 0 (the previous round's folds)
    // (a batched round -- see below -- does not use stream 1, and every API call here is GPU idle time in the late rounds:
    // leaving out its two waits and the second event record shortened an open by 0.3 ms)
    // Over the full key with its c = 20 table in place L and R are ONE launch sequence too, of another kind: their non-zero scalars
    // sit on disjoint points, so one array with a set bit per element feeds two bucket sets (MsmBatch::tagged) -- one recode, one
    // sort, one bucket kernel of 13 n additions instead of two of 13 n / 2, one window-sum pass of 2048 waves instead of two of 1024.
    const bool tagged = st->nofold && st->M >= ((size_t)1 << 20) && msm_tagged_ready(ctx, st->G_src, st->M);
    const bool will_batch = (st->nofold && st->M < ((size_t)1 << 20)) || tagged;
    HALO_HIP(hipEventRecord(st->ev, ctx->streams[0]));
    if (!will_batch) HALO_HIP(hipStreamWaitEvent(ctx->streams[1], st->ev, 0));
    HALO_HIP(hipStreamWaitEvent(ctx->streams[2], st->ev, 0));
    // dot_l = <c_r, z_l>, dot_r = <c_l, z_r>   (pcdl.rs:203,207) on a third stream.  In the rounds with large MSMs they are
    // issued BEFORE the MSMs' launches: queued behind them the two small kernels waited for the bucket kernel's waves to
    // drain, and the H' terms, which need only the dot products, were computed after the MSMs instead of under them.  In
    // the late rounds (an MSM of a few 10^4 additions: the GPU is mostly idle) the MSM's launches go first instead: the
    // three API calls of the dot products would only delay its start.
    const bool dots_first = (st->nofold ? st->M : m) > ((size_t)1 << 16);
    auto launch_dots = [&]() -> int {
        StreamGuard on_third(ctx, ctx->streams[2]);
        return fr_dot2_launch(ctx, st->buf.d_c + 4 * m, st->buf.d_z, st->buf.d_c, st->buf.d_z + 4 * m, m);
    };
    if (dots_first) { int rcl = launch_dots(); if (rcl) return rcl; }
    // the last round of a no-fold phase: its two coefficients travel to the host with the round's results (halo_ipa_finish
    // gets U from this round's own MSMs; pinned words 208..215, read after the wait for stream 0 below)
    const bool last_round = st->nofold && st->M > 1 && st->m == 2;
    st->last_valid = false;
    if (last_round) HALO_HIP(hipMemcpyAsync(ctx->h_pinned + 208, st->buf.d_c, 64, hipMemcpyDeviceToHost, ctx->streams[0]));
    if (st->nofold) {
        rc = tagged ? nofold_expand_tagged(ctx, st->buf.d_c, st->buf.d_s, st->m, st->M, st->buf.d_FL) : nofold_expand(ctx, st->buf.d_c, st->buf.d_s, st->m, st->M, st->buf.d_FL, st->buf.d_FR);
        if (rc) return rc;
        if (!will_batch) {
            HALO_HIP(hipEventRecord(st->ev, ctx->streams[0]));
            HALO_HIP(hipStreamWaitEvent(ctx->streams[1], st->ev, 0));
        }
        // Below the fixed-base table's size both MSMs go out as ONE batched launch (same points, two scalar arrays): two
        // launch sequences on two streams did not overlap -- the second one's 1024-thread sort blocks cannot start on a CU
        // that still holds waves of the first one's bucket kernel -- so a round took two MSM latencies instead of one.
        batched = will_batch;
        if (tagged) {
            MsmBatch both;
            both.count = 1;
            both.scalars[0] = st->buf.d_FL;
            both.tagged = true;
            rc = msm_enqueue_batch(ctx, 0, st->G_src, both, false, st->M);
            if (rc) return rc;
        } else if (batched) {
            MsmBatch both;
            both.count = 2;
            both.scalars[0] = st->buf.d_FL;
            both.scalars[1] = st->buf.d_FR;
            // half of each scalar array is zero: over a 2^16-point key 23 windows of 11 bits beat the table's 20 of 13 (measured,
            // medians of 13 opens on one box: 15.40 / 15.42 -> 15.23 / 15.37 ms; 10, 12 and 14 bits are worse, other key sizes keep the table)
            if (st->M == ((size_t)1 << 16)) both.c_hint = 11;
            rc = msm_enqueue_batch(ctx, 0, st->G_src, both, true, st->M);
            if (rc) return rc;
        } else {
            rc = msm_enqueue(ctx, 0, st->G_src, st->buf.d_FL, true, st->M);
            if (rc) return rc;
            rc = msm_enqueue(ctx, 1, st->G_src, st->buf.d_FR, true, st->M);
        }
    } else {
        rc = msm_enqueue(ctx, 0, st->buf.d_G, st->buf.d_c + 4 * m, true, m);
        if (rc) return rc;
        rc = msm_enqueue(ctx, 1, st->buf.d_G + 32 * m, st->buf.d_c, true, m);
    }
    if (rc) { host::Point dummy; (void)msm_finish(ctx, 0, &dummy); return rc; }
    if (!dots_first) { int rcl = launch_dots(); if (rcl) { host::Point dummy; (void)msm_finish(ctx, 0, &dummy); return rcl; } }
    double t1 = g_rt_on ? now_us() : 0;
    int rcd = fr_dot2_collect(ctx, ctx->streams[2], m, dots);
    // Window combine (~250 doublings), the H' term and the normalisation of L start on the helper thread as soon as L's
    // launches are done, while this thread still waits for R's and then does R's: pure host arithmetic on both sides.
    // the H' terms only need the dot products: computed now, while the MSMs are still running
    double t2 = g_rt_on ? now_us() : 0;
    host::Point hterm[2] = {host::Point::infinity(), host::Point::infinity()};
    if (with_hterm && !rcd)
        for (int k = 0; k < 2; ++k) hterm[k] = st->hp_from_scalar ? public_h_table().mul(dots[k] * st->hp_scalar) : st->hp_table.mul(dots[k]);
    auto finish_one = [ctx, st, last_round, with_hterm, &hterm, batched](int which, host::Point *out) {
        host::Point p;
        if (batched) msm_combine_member(ctx, 0, which, &p);
        else msm_combine(ctx, which, &p, 1);
        if (last_round) (which == 0 ? st->last_L : st->last_R) = p;  // before the H' term
        if (with_hterm) p = (p + hterm[which]).normalized();
        *out = p;
    };
    double t3 = g_rt_on ? now_us() : 0;
    rc = msm_wait(ctx, 0, batched ? 2 : 1);
    double t4 = g_rt_on ? now_us() : 0;
    bool l_started = !rc && !rcd;
    if (l_started) ctx->worker.submit([&finish_one, &Lp] { finish_one(0, &Lp); });
    int rc2 = batched ? HALO_OK : msm_wait(ctx, 1, 1);
    if (!rc && !rc2 && !rcd) finish_one(1, &Rp);
    if (l_started) ctx->worker.wait();
    if (g_rt_on) {
        double t5 = now_us();
        g_rt.enqueue += t1 - t0; g_rt.dots += t2 - t1; g_rt.hterm += t3 - t2; g_rt.wait += t4 - t3; g_rt.combine += t5 - t4; g_rt.rounds++;
    }
    if (rc || rc2 || rcd) return rc ? rc : (rc2 ? rc2 : rcd);
    if (last_round) {
        st->last_c0 = host::Fr::load(ctx->h_pinned + 208);
        st->last_c1 = host::Fr::load(ctx->h_pinned + 212);
        st->last_valid = true;
        st->last_folded = false;
    }
    *Lp_out = Lp;
    *Rp_out = Rp;
    return HALO_OK;
}

static int ipa_round_fold_impl(halo_ipa *st, const uint64_t xi[4], const uint64_t xi_inv[4]) {
    if (!st) { set_error("null ipa state"); return HALO_E_ARG; }
    halo_ctx *ctx = st->ctx;
    HALO_CTX(ctx);
    if (st->m < 2) { set_error("ipa_round_fold: no rounds left"); return HALO_E_ARG; }
    size_t m = st->m / 2;
    host::Fr x = host::Fr::load(xi), xinv = host::Fr::load(xi_inv);
    int rc;
    if (st->last_valid && st->m == 2) {  // the fold after the last round: halo_ipa_finish needs its challenge, see there
        st->last_xi = x;
        st->last_xi_inv = xinv;
        st->last_folded = true;
    } else {
        st->last_valid = false;
    }
    if (st->nofold) {
        rc = nofold_s_update(ctx, st->buf.d_s, st->s_len, x, st->buf.d_s2);
        if (!rc) { std::swap(st->buf.d_s, st->buf.d_s2); st->s_len *= 2; }
        if (!rc && st->deferred) {  // host copy of the (short) challenge products: s'[2t + u] = s[t] xi^u
            std::vector<host::Fr> &cur = st->fold_pending ? st->tail_host : st->s_host;  // (a fold under way has taken s_host)
            std::vector<host::Fr> s2(2 * cur.size());
            for (size_t t = 0; t < cur.size(); ++t) { s2[2 * t] = cur[t]; s2[2 * t + 1] = cur[t] * x; }
            cur.swap(s2);
        }
    } else {
        rc = ipa_fold_points(ctx, st->buf.d_G, m, x);
    }
    if (!rc) rc = ipa_fold_scalars(ctx, st->buf.d_c, st->buf.d_z, m, x, xinv);
    if (rc) return rc;
    st->m = m;
    if (st->nofold && st->deferred && st->fold_pending && st->tail_host.size() == 4) {
        // Two rounds have run beside the fold launched two rounds ago: switch to its output.  The challenge products since
        // then are s[0..4) (the newest challenge is the lowest index bit and s[0] = 1): nothing to upload, s just gets shorter.
        HALO_HIP(hipStreamWaitEvent(ctx->streams[0], st->ev_fold, 0));
        st->G_src = st->fold_dst;
        st->M = st->fold_m;
        st->s_len = 4;
        st->s_host.swap(st->tail_host);
        st->tail_host.clear();
        st->fold_pending = false;
        st->deferred = st->M > ctx->nofold_size;
        if (!st->deferred) return HALO_OK;  // (the key stays as it is for the remaining rounds; s goes on from its 4 entries)
    }
    if (st->nofold && st->deferred && !st->fold_pending && st->s_len == 4) {
        // two rounds are due: G[j] <- G[j] + s1 G[j+m] + s2 G[j+2m] + s3 G[j+3m] with one shared doubling chain
        const size_t Mcur = 4 * m;
        // Measured (tools/open_loop.py, medians of 11, one box): opens of 2^18 points 9.33 -> 8.99 ms with the folds beside the
        // rounds; at 2^19 12.35 -> 12.61 and at 2^20 15.68 -> 16.43 (only the last fold beside: 15.89): there the rounds over the
        // larger key lose more than the hidden fold returns -- a fold's waves sit on every CU (one per SIMD, 232-252 registers,
        // the lane form 27 KB of LDS) and the rounds' 1024-thread sort blocks (140 KB of LDS) cannot start beside them.
        // Hence the automatic mode: opens of at most 2^18 points.
        const bool want_async = ctx->fold_async > 0 || (ctx->fold_async < 0 && st->n <= ((size_t)1 << 18));
        if (want_async && Mcur <= ((size_t)1 << 18) && m >= 64 && st->g_off + m <= (st->borrowed ? ctx->ipa_bufs.cap_n : st->n)) {
            // ... BESIDE the next two rounds (see halo_ipa::fold_pending): on the fourth stream, behind whatever wrote the
            // key it reads (stream 0: an earlier in-line fold; stream 3 itself: the previous fold of this kind)
            uint32_t *dst = st->buf.d_G + 32 * st->g_off;  // (32 words = one 128-byte point, curve.hpp AFF_STRIDE)
            HALO_HIP(hipEventRecord(st->ev, ctx->streams[0]));
            HALO_HIP(hipStreamWaitEvent(ctx->streams[3], st->ev, 0));
            {
                StreamGuard on_fourth(ctx, ctx->streams[3]);
                rc = ipa_fold_points4(ctx, st->G_src, dst, m, &st->s_host[1]);
            }
            if (rc) return rc;
            HALO_HIP(hipEventRecord(st->ev_fold, ctx->streams[3]));
            st->fold_pending = true;
            st->fold_dst = dst;
            st->fold_m = m;
            st->g_off += m;
            st->tail_host.assign(1, host::Fr::one());
            return HALO_OK;
        }
        rc = ipa_fold_points4(ctx, st->G_src, st->buf.d_G, m, &st->s_host[1]);
        if (rc) return rc;
        st->G_src = st->buf.d_G;
        st->g_off = m;  // (in place from here on would overwrite this key: later folds go behind it)
        st->deferred = m > ctx->nofold_size;  // below the switch size the key stays as it is for the remaining rounds
        st->s_host.assign(1, host::Fr::one());
        if (m > 1) return ipa_enter_nofold(st);
        st->nofold = false;  // the last two rounds: G[0] is U
        st->M = 1;
        st->s_len = 1;
        return HALO_OK;
    }
    if (!st->nofold && m <= ctx->nofold_size && m > 1) rc = ipa_enter_nofold(st);
    return rc;
}
}  // namespace halo

using namespace halo;

extern "C" {
int halo_ipa_begin(halo_ctx *ctx, size_t n, const uint64_t *coeffs, size_t len, const uint64_t z[4], halo_ipa **out) {
    HALO_CTX(ctx);
    if (!out || !z || (len && !coeffs)) { set_error("ipa_begin: null pointer"); return HALO_E_ARG; }
    int rc = ipa_begin_checks(ctx, n, len);
    if (!rc) rc = ipa_stage_coeffs(ctx, n, coeffs, len);
    if (rc) return rc;
    return ipa_begin_dev(ctx, n, ctx->d_tmp_a, host::Fr::load(z), out);
}

int halo_ipa_begin_strided(halo_ctx *ctx, size_t n_local, const uint64_t *coeffs_local, size_t len, const uint64_t z[4], uint64_t stride,
                           uint64_t offset, halo_ipa **out) {
    HALO_CTX(ctx);
    if (!out || !z || (len && !coeffs_local) || stride == 0) { set_error("ipa_begin_strided: bad argument"); return HALO_E_ARG; }
    int rc = ipa_begin_checks(ctx, n_local, len);
    if (!rc) rc = ipa_stage_coeffs(ctx, n_local, coeffs_local, len);
    if (rc) return rc;
    host::Fr zz = host::Fr::load(z);
    host::Fr base = fr_pow_u64(zz, stride), scale = fr_pow_u64(zz, offset);  // z^(offset + j * stride)
    return ipa_begin_dev(ctx, n_local, ctx->d_tmp_a, base, out, &scale);
}

int halo_ipa_begin_vectors(halo_ctx *ctx, size_t n, const uint64_t *c_vec, const uint64_t *z_vec, halo_ipa **out) {
    HALO_CTX(ctx);
    if (!out || (n && (!c_vec || !z_vec))) { set_error("ipa_begin_vectors: null pointer"); return HALO_E_ARG; }
    int rc = ipa_begin_checks(ctx, n, n);
    if (!rc) rc = upload_words(ctx, ctx->d_tmp_a, c_vec, n * 4);
    if (!rc) rc = upload_words(ctx, ctx->d_tmp_b, z_vec, n * 4);
    if (rc) return rc;
    return ipa_begin_dev(ctx, n, ctx->d_tmp_a, host::Fr::one(), out, nullptr, ctx->d_tmp_b);
}

int halo_ipa_dot_cz(halo_ipa *st, uint64_t out[4]) {
    if (!st || !out) { set_error("null ipa state"); return HALO_E_ARG; }
    halo_ctx *ctx = st->ctx;
    HALO_CTX(ctx);
    host::Fr r[2];
    int rc = fr_dot2(ctx, st->buf.d_c, st->buf.d_z, nullptr, nullptr, st->m, r);
    if (rc) return rc;
    r[0].store(out);
    return HALO_OK;
}

int halo_ipa_round_lr_partial(halo_ipa *st, uint64_t L[12], uint64_t R[12], uint64_t dots_out[8]) {
    if (!st || !L || !R || !dots_out) { set_error("null ipa state"); return HALO_E_ARG; }
    halo_ctx *ctx = st->ctx;
    HALO_CTX(ctx);
    host::Fr dots[2];
    host::Point Lp, Rp;
    int rc = ipa_round_lr_points(st, dots, &Lp, &Rp);
    if (rc) return rc;
    Lp.store_normalized(L);
    Rp.store_normalized(R);
    dots[0].store(dots_out);
    dots[1].store(dots_out + 4);
    return HALO_OK;
}

int halo_ipa_round_lr(halo_ipa *st, const uint64_t H_prime[12], uint64_t L[12], uint64_t R[12]) {
    if (!st) { set_error("null ipa state"); return HALO_E_ARG; }
    halo_ctx *ctx = st->ctx;
    HALO_CTX(ctx);
    host::Fr dots[2];
    host::Point Lp, Rp, Hp = host::Point::load(H_prime);
    if (!st->hp_from_scalar && !st->hp_table.matches(Hp)) st->hp_table = host::FixedBaseTable(Hp);  // H' is fixed for a whole open
    int rc = ipa_round_lr_points(st, dots, &Lp, &Rp, true);  // L, R come back with their H' terms, normalised
    if (rc) return rc;
    Lp.store(L);
    Rp.store(R);
    return HALO_OK;
}

int halo_ipa_round_fold(halo_ipa *st, const uint64_t xi[4], const uint64_t xi_inv[4]) {
    double t0 = g_rt_on ? now_us() : 0;
    int rc = ipa_round_fold_impl(st, xi, xi_inv);
    if (g_rt_on) g_rt.fold += now_us() - t0;
    return rc;
}

int halo_ipa_finish(halo_ipa *st, uint64_t U[12], uint64_t c[4]) {
    if (!st) { set_error("null ipa state"); return HALO_E_ARG; }
    halo_ctx *ctx = st->ctx;
    HALO_CTX(ctx);
    if (st->m != 1) { set_error("ipa_finish: rounds remaining"); return HALO_E_ARG; }
    if (st->fold_pending) {  // (cannot happen with >= 2 rounds behind every fold launched beside them; kept for safety)
        HALO_HIP(hipStreamWaitEvent(ctx->streams[0], st->ev_fold, 0));
        st->fold_pending = false;
    }
    int rc;
    if (st->nofold && st->M > 1 && st->last_valid && st->last_folded && !st->last_c0.is_zero() && !st->last_c1.is_zero()) {
        // U = G_final[0] = sum_b s''[b] K[b] with s''[2t + u] = s[t] xi^u (the last fold): U = A + xi B, A / B = the sums of
        // s[t] K[2t] / s[t] K[2t + 1].  The last round had two coefficients left, so its MSMs were exactly L' = c1 A and
        // R' = c0 B (k_nofold_expand with m = 2: FL[2t] = c[1] s[t], FR[2t + 1] = c[0] s[t]): U = L' / c1 + (xi / c0) R' -- two
        // scalar multiples on the host (~80 us, side by side on two threads) instead of one more MSM over the key (0.45 ms at
        // 2^14 points), and c = c0 + xi^-1 c1 (pcdl.rs:222) without another copy.  A zero coefficient takes the MSM below.
        host::Fr inv01 = (st->last_c0 * st->last_c1).inv();  // one inversion for both
        host::Fr a = inv01 * st->last_c0, b = inv01 * st->last_c1 * st->last_xi;  // 1 / c1, xi / c0
        host::Point Lp = st->last_L, Rp = st->last_R, Ua, Ub;
        ctx->worker.submit([&Ua, &Lp, &a] { Ua = Lp.mul(a); });
        Ub = Rp.mul(b);
        ctx->worker.wait();
        (Ua + Ub).store_normalized(U);
        (st->last_c0 + st->last_xi_inv * st->last_c1).store(c);
        if (ctx->prof.on) {
            for (int k = 0; k < 4; ++k) HALO_HIP(hipStreamSynchronize(ctx->streams[k]));
            ctx->prof.collect();
        }
        return HALO_OK;
    }
    if (st->nofold && st->M > 1) {
        // U = G_final[0] = sum_t s[t] * G0[t]
        host::Point Up;
        rc = msm_run(ctx, st->G_src, st->buf.d_s, true, st->M, &Up);
        if (!rc) rc = download_words(ctx, c, st->buf.d_c, 4);
        if (rc) return rc;
        if (ctx->prof.on) ctx->prof.collect();
        Up.store_normalized(U);
        return HALO_OK;
    }
    uint64_t g[8];
    rc = aff_native_to_words(ctx, st->G_src, 1, ctx->d_tmp_a);
    if (!rc) rc = download_words(ctx, g, ctx->d_tmp_a, 8);
    if (!rc) rc = download_words(ctx, c, st->buf.d_c, 4);
    if (rc) return rc;
    if (ctx->prof.on) ctx->prof.collect();
    host::Point::load_affine(g).store_normalized(U);
    return HALO_OK;
}

// hiding branch, sharded (pcdl.rs:140-150): this shard's slice of p_bar = q (X - z) from the rng stream and
// its share <p_bar_loc, G_loc> of C_bar (without the w_bar S term)
int halo_ipa_hiding_partial(halo_ipa *st, uint64_t rng_state, size_t deg, const uint64_t z[4], uint64_t stride, uint64_t offset,
                            uint64_t Cbar_part[12]) {
    if (!st || !z || !Cbar_part || stride == 0) { set_error("ipa_hiding_partial: bad argument"); return HALO_E_ARG; }
    halo_ctx *ctx = st->ctx;
    HALO_CTX(ctx);
    if (st->m != st->n) { set_error("ipa_hiding_partial: rounds already started"); return HALO_E_ARG; }
    if (deg == 0) { set_error("open: hiding needs p.degree() >= 1"); return HALO_E_ASSERT; }
    if (!st->buf.d_pbar) {
        alloc_epoch_bump(ctx);
        size_t cap = st->borrowed ? ctx->ipa_bufs.cap_n : st->n;
        if (hipMalloc(&st->buf.d_pbar, cap * 32) != hipSuccess) { set_error("ipa_hiding_partial: allocation failed"); return HALO_E_DEVICE; }
    }
    int rc = pbar_stream_dev(ctx, rng_state, deg, host::Fr::load(z), stride, offset, st->n, st->buf.d_pbar);
    if (rc) return rc;
    st->pbar_valid = true;
    host::Point part;
    rc = msm_run(ctx, st->G_src, st->buf.d_pbar, true, st->n, &part);
    if (rc) return rc;
    part.store_normalized(Cbar_part);
    return HALO_OK;
}
// p' = p + alpha p_bar on this shard (pcdl.rs:156)
int halo_ipa_apply_hiding(halo_ipa *st, const uint64_t alpha[4]) {
    if (!st || !alpha || !st->buf.d_pbar || !st->pbar_valid) { set_error("ipa_apply_hiding: no p_bar on this state"); return HALO_E_ARG; }
    halo_ctx *ctx = st->ctx;
    HALO_CTX(ctx);
    if (st->m != st->n) { set_error("ipa_apply_hiding: rounds already started"); return HALO_E_ARG; }
    return axpy_dev(ctx, st->buf.d_c, st->buf.d_pbar, st->n, host::Fr::load(alpha));
}

int halo_ipa_finish_z(halo_ipa *st, uint64_t U[12], uint64_t c[4], uint64_t z0[4]) {
    int rc = halo_ipa_finish(st, U, c);
    if (rc) return rc;
    if (!z0) { set_error("ipa_finish_z: null pointer"); return HALO_E_ARG; }
    return download_words(st->ctx, z0, st->buf.d_z, 4);
}

void halo_ipa_destroy(halo_ipa *st) {
    if (!st) return;
    if (g_rt_on && g_rt.rounds) {
        fprintf(stderr, "[halo] ipa host time over %ld rounds (us): enqueue %.0f  dot launch + wait %.0f  H' terms %.0f  wait for the MSMs %.0f  combine %.0f  fold calls %.0f\n",
                g_rt.rounds, g_rt.enqueue, g_rt.dots, g_rt.hterm, g_rt.wait, g_rt.combine, g_rt.fold);
        g_rt = RoundTiming();
    }
    halo_ctx *ctx = st->ctx;
    if (ctx) {
        (void)hipSetDevice(ctx->device);
        for (int k = 0; k < 4; ++k) (void)hipStreamSynchronize(ctx->streams[k]);  // folds, the second MSM, the dot products, a fold beside the rounds
    }
    if (ctx && st->counted_hot) ctx->worker.add_hot(-1);
    if (st->borrowed && ctx) {
        ctx->ipa_bufs.d_pbar = st->buf.d_pbar;  // lazily allocated by the hiding branch of a sharded open: kept with the rest
        ctx->ipa_bufs.in_use = false;
    } else if (st->buf.d_G) {
        if (ctx) alloc_epoch_bump(ctx);
        ipa_bufs_free(st->buf);
    }
    if (st->ev) (void)hipEventDestroy(st->ev);
    if (st->ev_fold) (void)hipEventDestroy(st->ev_fold);
    delete st;
}
size_t halo_ipa_len(const halo_ipa *st) { return st ? st->m : 0; }
}  // extern "C"
