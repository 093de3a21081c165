// The batched calls of the pcdl / acc level: m or k of the single calls of pcdl_acc.hip in one, every member's output, status,
// message and draws those of the loop over the single call.  Four pipelines -- the check / decider batch, the verifier batch, the
// open / random-instance batch, the prover batch -- and their entry points.  What they share with the single calls is declared
// in pcdl_internal.hpp; the slots, streams and outcome reports they share with each other (and with wire.hip's decode batch) in
// internal.hpp: idle_slots, StreamGuard, report_members.
#include "curve.hpp"  // (AFF_STRIDE: the staged keys of the folded schedule)
#include "fr_plan.hpp"
#include "mixed_terms_lane.hpp"  // (the record and term layout of the fused checks: fused_lane.hpp, and the mixed call's descriptors)
#include "pcdl_internal.hpp"

namespace halo {

using host::Fr;
using host::Point;

// ------------------------------------------------------------------ the staging every batched call shares
// Member buffers of n coefficients + one set of tables each in the context's check staging: grown to `want` buffers if the
// memory budget and the device allow (optional memory: halo_set_memory_budget), never shrunk.  Returns how many buffers it
// holds (0: none -- the caller runs one member at a time in ctx->d_tmp_a; never an error).
size_t check_stage(halo_ctx *ctx, size_t want, size_t per_bytes) {
    if (dev_hooks().batch_stage_fail) return 0;  // (development library: the fallback path)
    const size_t bytes = want * per_bytes;
    if (ctx->check_stage_bytes < bytes && table_budget_reserve(ctx, bytes)) {
        uint64_t *p = nullptr;
        if (hipMalloc(&p, bytes) != hipSuccess) {
            (void)hipGetLastError();
            p = nullptr;
            table_budget_release(ctx, bytes);
        } else {
            alloc_epoch_bump(ctx);  // (cached launch graphs name the old buffer)
            if (ctx->d_check_stage) {
                for (int k = 0; k < HALO_SLOTS; ++k)
                    if (!ctx->wss[k].in_flight) (void)hipStreamSynchronize(ctx->streams[k]);
                (void)hipFree(ctx->d_check_stage);
                table_budget_release(ctx, ctx->check_stage_bytes);
            }
            ctx->d_check_stage = p;
            ctx->check_stage_bytes = bytes;
        }
    }
    return ctx->check_stage_bytes / per_bytes;
}

// ------------------------------------------------------------------ the weights and the launch shape of the combined check
// (pcdl_internal.hpp: the development library calls these too)
// out[k] = SHA3-256(D || LE64(k)) mod r for k < count, D the digest of domain, seed, d, A and the members' indices and Instance words
static void hashed_weights(const char *domain, size_t domain_len, const uint64_t *blobs, size_t stride, const size_t *idx, size_t A, size_t d,
                           const uint8_t *seed, size_t count, std::vector<Fr> &out);
// the second stage of every rule: out[k] = SHA3-256(D || LE64(k)) mod r
static void weights_from_digest(const uint8_t D[32], size_t count, std::vector<Fr> &out) {
    out.resize(count);
    for (size_t a = 0; a < count; ++a) {
        const uint64_t a64 = a;
        uint8_t dig[32];
        host::Sha3_256 g;
        g.update(D, 32);
        g.update(&a64, 8);
        g.finalize(dig);
        out[a] = Fr::from_le_bytes_mod_order(dig);
    }
}
void check_combined_weights(const uint64_t *blobs, size_t stride, const size_t *idx, size_t A, size_t d, const uint8_t *seed, std::vector<Fr> &out) {
    static const char kDomain[] = "halo-accumulation/check-batch-combined/v1";
    hashed_weights(kDomain, sizeof(kDomain) - 1, blobs, stride, idx, A, d, seed, A, out);
}
void check_fused_weights(const uint64_t *blobs, size_t stride, const size_t *idx, size_t A, size_t d, const uint8_t *seed, std::vector<Fr> &out) {
    static const char kDomain[] = "halo-accumulation/check-batch-fused/v1";
    hashed_weights(kDomain, sizeof(kDomain) - 1, blobs, stride, idx, A, d, seed, 2 * A, out);  // r_a = out[2 a], s_a = out[2 a + 1]
}
static void hashed_weights(const char *domain, size_t domain_len, const uint64_t *blobs, size_t stride, const size_t *idx, size_t A, size_t d,
                           const uint8_t *seed, size_t count, std::vector<Fr> &out) {
    static const uint8_t kZeros[32] = {};
    const size_t W = instance_words(ilog2(d + 1));
    const uint64_t d64 = d, A64 = A;
    uint8_t D[32];
    host::Sha3_256 h;
    h.update(domain, domain_len);
    h.update(seed ? seed : kZeros, 32);
    h.update(&d64, 8);  // (the words of a blob are little-endian in memory on every host this library builds for)
    h.update(&A64, 8);
    for (size_t a = 0; a < A; ++a) {
        const uint64_t i64 = idx[a];
        h.update(&i64, 8);
        h.update(blobs + idx[a] * stride, W * 8);
    }
    h.finalize(D);
    weights_from_digest(D, count, out);
}
// The weights of the mixed combined check (halo_pcdl_check_batch_mixed_combined; the rule: include/halo_accumulation.h): a domain of
// its own, and every member's index and degree bound hashed in front of its Instance words, so no digest of a uniform call can be
// replayed.  blobs[idx[a]] = member idx[a]'s blob, ds[idx[a]] its degree bound.  The mixed fused check
// (halo_pcdl_check_batch_mixed_fused) hashes the same under its own domain and draws two weights per member: r_a = out[2 a],
// s_a = out[2 a + 1].
void check_mixed_weights_rule(MixedRule rule, const uint64_t *const *blobs, const size_t *ds, const size_t *idx, size_t A, const uint8_t *seed,
                              std::vector<Fr> &out) {
    static const char kCombined[] = "halo-accumulation/check-batch-mixed-combined/v1";
    static const char kFused[] = "halo-accumulation/check-batch-mixed-fused/v1";
    static const uint8_t kZeros[32] = {};
    const bool fused = rule == MixedRule::fused;
    const uint64_t A64 = A;
    uint8_t D[32];
    host::Sha3_256 h;
    if (fused) h.update(kFused, sizeof(kFused) - 1);
    else h.update(kCombined, sizeof(kCombined) - 1);
    h.update(seed ? seed : kZeros, 32);
    h.update(&A64, 8);
    for (size_t a = 0; a < A; ++a) {
        const uint64_t i64 = idx[a], d64 = ds[idx[a]];
        h.update(&i64, 8);
        h.update(&d64, 8);
        h.update(blobs[idx[a]], instance_words(ilog2(ds[idx[a]] + 1)) * 8);
    }
    h.finalize(D);
    weights_from_digest(D, fused ? 2 * A : A, out);
}
namespace {  // (everything below is local to this file; the entry points at the end are the way in)

// Members per batched launch: the forced size (the development library's sweeps) if it lies in 1 .. max, else max; then as many
// as the small pipeline's bucket limit allows with `arrays` scalar arrays per member (windows x arrays x buckets <= 2^22)
static int group_size(const halo_ctx *ctx, size_t n, int forced, int max, int arrays) {
    int g = forced >= 1 && forced <= max ? forced : max;
    MsmPlan p = msm_plan(n, ctx->window_bits);
    while (g > 1 && (size_t)p.W * (size_t)(arrays * g) * p.B > ((size_t)1 << 22)) --g;
    return g;
}

// The rotation the check and commit batches share: A members in groups of G over S slots.  enqueue(j, first, cnt) puts the batched
// MSM of members first .. first + cnt in flight on slots[j]; when the slot comes round again, and at the end, the group is
// collected (msm_finish_batch) and done(first, cnt, pts) takes its points.  A failure leaves nothing of the call in flight.
template <class Enqueue, class Done>
static int rotate_groups(halo_ctx *ctx, const int *slots, int S, size_t A, size_t G, Enqueue enqueue, Done done) {
    const size_t ng = (A + G - 1) / G;
    auto cnt_of = [&](size_t g) { return A - g * G < G ? A - g * G : G; };
    std::vector<long> flight(S, -1);  // the group in flight on slots[j]
    auto collect = [&](size_t j) -> int {
        const long g = flight[j];
        if (g < 0) return HALO_OK;
        flight[j] = -1;
        Point pts[MSM_MAX_BATCH];
        int rc = msm_finish_batch(ctx, slots[j], pts, (int)cnt_of((size_t)g));
        if (!rc) done((size_t)g * G, cnt_of((size_t)g), pts);
        return rc;
    };
    auto abandon = [&]() {  // (a device error: nothing of this call stays in flight)
        std::string err = halo_last_error();
        for (int j = 0; j < S; ++j)
            if (flight[j] >= 0) {
                Point pts[MSM_MAX_BATCH];
                (void)msm_finish_batch(ctx, slots[j], pts, (int)cnt_of((size_t)flight[j]));
                flight[j] = -1;
            }
        set_error(err);
    };
    for (size_t g = 0; g < ng; ++g) {
        const size_t j = g % (size_t)S;
        int rc = collect(j);
        if (!rc) rc = enqueue(j, g * G, cnt_of(g));
        if (rc) { abandon(); return rc; }
        flight[j] = (long)g;
    }
    for (size_t g = ng > (size_t)S ? ng - (size_t)S : 0; g < ng; ++g) {
        int rc = collect(g % (size_t)S);
        if (rc) { abandon(); return rc; }
    }
    return HALO_OK;
}

// ------------------------------------------------------------------ pcdl::check of m instances at once
// The succinct half of every member as halo_pcdl_succinct_check_batch runs it (the relations on the device from kBatchVerifyMin
// members on, on the host pool below); then the accepted members in groups of up to MSM_MAX_BATCH: their h coefficients expanded
// on the device (k_h_tables + k_h_coeffs_batch: two launches per group) into the group's staging, and the group's n-point MSMs
// as ONE batched launch sequence over the key.  Groups rotate over the slots that were idle at entry; when a slot comes round
// again its group is collected and every member's point compared with its U (pcdl.rs:338-339) on the host while the other slots'
// groups run.  Every member gets its own exact MSM.  A multi-device context runs the groups on its own device (devices[0], which
// holds the whole key), as halo_pcdl_check does: no fan-out, the same points.
//
// Members per launch (check_group_size): the small pipeline (smsm.hip, n <= 2^16) takes batches of 8 within its bucket limit
// (windows x batch x buckets <= 2^22); a key of 2^20 points or more runs its MSMs of >= 2^20 points through the fixed-base table,
// which takes single members only, so there each member is a group of its own.  Measured: DESIGN.md "Batched checks".
static int check_group_size(const halo_ctx *ctx, size_t n) {
    const int forced = dev_hooks().check_group;  // (development library: the sweep of tools/time_decider_batch.py)
    if (forced <= 0 && n >= ((size_t)1 << 20) && ctx->n >= ((size_t)1 << 20) && ctx->table_mode != 0) return 1;
    return group_size(ctx, n, forced, MSM_MAX_BATCH, 1);
}
// The exact MSM half (steps 2 and 3 above) for the members `ok` the succinct half accepted, over the slots idle at entry: a member
// whose point differs from its U gets its reject in res
static int check_members_exact(halo_ctx *ctx, size_t n, const int *slots, int S, std::vector<BatchCheck> &res, const std::vector<size_t> &ok) {
    const size_t lg = ilog2(n), A = ok.size();
    int rc = HALO_OK;
    if (A) {
        if (lg > 24) { set_error("h_coeffs: lg_n > 24 unsupported"); return HALO_E_ARG; }
        // 2. their challenges in device memory, in that order (one copy)
        const size_t xw = (lg + 1) * 4;
        std::vector<uint64_t> xis(A * xw);
        for (size_t a = 0; a < A; ++a)
            for (size_t k = 0; k <= lg; ++k) res[ok[a]].st.xis[k].store(&xis[a * xw + 4 * k]);
        rc = verify_staging(ctx, xis.size());
        if (rc) return rc;
        HALO_HIP(hipMemcpy(ctx->d_verify, xis.data(), xis.size() * 8, hipMemcpyHostToDevice));
        // 3. groups of G members over S slots, G x S member buffers in the staging (fewer if it cannot grow; none: d_tmp_a)
        size_t G = (size_t)check_group_size(ctx, n);
        if (G > A) G = A;
        size_t ng = (A + G - 1) / G;
        if ((size_t)S > ng) S = (int)ng;
        const size_t per = n * 4 + H_TABLES_WORDS;  // words of one member buffer
        size_t have = check_stage(ctx, G * (size_t)S, per * 8);
        const bool scratch = have == 0;
        if (scratch) { G = 1; S = 1; }
        else if (have < G * (size_t)S) {
            if (G > have) G = have;
            if ((size_t)S > have / G) S = (int)(have / G);
        }
        ng = (A + G - 1) / G;
        auto coeffs_of = [&](size_t j) { return scratch ? ctx->d_tmp_a : ctx->d_check_stage + j * G * n * 4; };
        auto tables_of = [&](size_t j) { return scratch ? ctx->d_tmp_c + 8 * 1024 + 1024 : ctx->d_check_stage + (size_t)S * G * n * 4 + j * G * H_TABLES_WORDS; };
        rc = rotate_groups(
            ctx, slots, S, A, G,
            [&](size_t j, size_t first, size_t cnt) -> int {
                int rc2;
                {
                    StreamGuard on_slot(ctx, ctx->streams[slots[j]]);
                    rc2 = h_coeffs_batch_dev(ctx, ctx->d_verify + first * xw, cnt, lg, tables_of(j), coeffs_of(j), n * 4);  // h.get_poly().coeffs
                }
                if (rc2) return rc2;
                MsmBatch mb;
                mb.count = (int)cnt;
                for (size_t b = 0; b < cnt; ++b) mb.scalars[b] = coeffs_of(j) + b * n * 4;
                return msm_enqueue_batch(ctx, slots[j], ctx->d_bases, mb, true, n);  // :338, asynchronous
            },
            [&](size_t first, size_t cnt, const Point *pts) {
                for (size_t b = 0; b < cnt; ++b) {
                    BatchCheck &r = res[ok[first + b]];
                    if (r.st.U != pts[b]) { r.rc = HALO_E_REJECT; r.err = "U != CM.Commit(ck, h_vec)"; }  // :339
                }
            });
        if (rc) return rc;
    }
    return HALO_OK;
}
// ------------------------------------------------------------------ ... as ONE relation (halo_pcdl_check_batch_combined)
// pcdl.rs:338-339 is linear in h: <h_i, G> = U_i.  So the A >= 2 members the succinct half accepted are checked as
// <sum_a r_a h_a, G> = sum_a r_a U_a with the weights of check_combined_weights (the rule: include/halo_accumulation.h):
//   scalars    s = sum_a r_a h_a(X) on the device (hpoly.hip h_combine_rows: the polynomials in P parts, k_fr_sum_rows), in the
//              context's check staging (optional memory; none: *held stays false and the caller runs the exact batch);
//   left side  ONE n-point MSM of s over the key on the first idle slot (the table pipeline where the key has one);
//   right side T = sum_a r_a U_a while that MSM runs: on the host pool, or from kCombinedUsumDeviceMin members on -- and with a
//              second idle slot -- as a variable-base MSM on the device (k_batch_to_affine + the small pipeline: the path of
//              halo_msm_points).  The hook "check_combined_usum" forces either side.
// *held = the two sides are the same point.  If they are not, the caller runs the exact batch over the same members, so which
// members a call rejects never depends on the weights.
// kCombinedUsumDeviceMin is measured (tools/time_decider_batch.py --combined, its right-side sweep; HISTORY.md): from 64 members on
// every run with the device sum was faster than every run with the pool's (0.2 - 1.0 ms of the call); at 4 members the pool won
// every run, and at 2, 8, 16 and 32 the ranges overlap -- there the pool stays, which needs no second slot.
constexpr size_t kCombinedUsumDeviceMin = 64;

static int combined_usum_device(halo_ctx *ctx, int slot, const std::vector<BatchCheck> &res, const std::vector<size_t> &ok, const std::vector<Fr> &r,
                                uint64_t *d_region, Point *T) {
    const size_t A = ok.size();
    uint32_t *d_native = reinterpret_cast<uint32_t *>(d_region);  // A x AFF_STRIDE 32-bit words | A x 12 | A x 4
    uint64_t *d_jac = d_region + A * (AFF_STRIDE / 2), *d_sc = d_jac + A * 12;
    std::vector<uint64_t> jac(A * 12), sc(A * 4);
    for (size_t a = 0; a < A; ++a) {
        res[ok[a]].st.U.store(&jac[12 * a]);
        r[a].store(&sc[4 * a]);
    }
    HALO_HIP(hipMemcpy(d_jac, jac.data(), jac.size() * 8, hipMemcpyHostToDevice));
    HALO_HIP(hipMemcpy(d_sc, sc.data(), sc.size() * 8, hipMemcpyHostToDevice));
    int rc;
    {
        StreamGuard on_slot(ctx, ctx->streams[slot]);
        rc = batch_to_affine(ctx, d_jac, A, d_native);
    }
    if (!rc) rc = msm_enqueue_batch(ctx, slot, d_native, msm_one(d_sc), true, A);
    if (!rc) rc = msm_finish_batch(ctx, slot, T, 1);
    return rc;
}

// The right side T = sum_a r_a U_a of a combined relation whose left side's MSM is in flight on slots[0] -- on the host pool, or
// (usum_dev) on slots[1] through d_region -- then the left side collected; *held = the two sides are the same point
static int combined_sides_agree(halo_ctx *ctx, const int *slots, bool usum_dev, const std::vector<BatchCheck> &res, const std::vector<size_t> &ok,
                                const std::vector<Fr> &r, uint64_t *d_region, bool *held) {
    const size_t A = ok.size();
    Point T = Point::infinity();
    int rc_t = HALO_OK;
    if (usum_dev) rc_t = combined_usum_device(ctx, slots[1], res, ok, r, d_region, &T);
    else {  // one multi-scalar sum per pool thread
        const size_t chunks = A < 16 ? A : 16;
        std::vector<Point> part(chunks, Point::infinity());
        pool_run(chunks, [&](size_t c) {
            std::vector<Point> p;
            std::vector<Fr> k;
            for (size_t a = c * A / chunks; a < (c + 1) * A / chunks; ++a) { p.push_back(res[ok[a]].st.U); k.push_back(r[a]); }
            part[c] = host::small_msm(p, k);
        });
        for (const Point &q : part) T = T + q;
    }
    const std::string err_t = rc_t ? halo_last_error() : "";
    Point left;
    int rc = msm_finish_batch(ctx, slots[0], &left, 1);  // (collected whatever happened to the right side: nothing stays in flight)
    if (rc_t) { set_error(err_t); return rc_t; }
    if (rc) return rc;
    *held = left == T;
    return HALO_OK;
}

static int check_members_combined(halo_ctx *ctx, size_t d, const uint64_t *qs, size_t stride, const uint8_t *seed, const int *slots, int S,
                                  const std::vector<BatchCheck> &res, const std::vector<size_t> &ok, bool *held) {
    const size_t n = d + 1, lg = ilog2(n), A = ok.size(), tw = (lg + 2) * 4;
    *held = false;
    if (lg > 24) { set_error("h_coeffs: lg_n > 24 unsupported"); return HALO_E_ARG; }
    if (A > 65535) return HALO_OK;  // (h_combine_rows takes at most 65535 polynomials: the exact batch)
    const int forced = dev_hooks().combined_usum;
    const bool usum_dev = S >= 2 && A <= ctx_capacity(ctx) && (forced ? forced == 2 : A >= kCombinedUsumDeviceMin);
    // the staging: the scalar step's regions, then (128-byte aligned) the right side's points and weights
    const size_t cap = check_combined_cap(A);
    size_t P = check_combined_parts(n, A), u_off = 0;
    for (;; P = (P + 1) / 2) {  // (fewer parts if the staging cannot hold their rows)
        u_off = (hcomb_stage_words(A, lg, P, cap) + 15) & ~(size_t)15;
        if (check_stage(ctx, 1, (u_off + (usum_dev ? A * (AFF_STRIDE / 2 + 16) : 0)) * 8) >= 1) break;
        if (P == 1) return HALO_OK;
    }
    std::vector<Fr> r;
    check_combined_weights(qs, stride, ok.data(), A, d, seed, r);
    std::vector<uint64_t> recs(A * tw);
    for (size_t a = 0; a < A; ++a) {
        for (size_t k = 0; k <= lg; ++k) res[ok[a]].st.xis[k].store(&recs[a * tw + 4 * k]);
        r[a].store(&recs[a * tw + 4 * (lg + 1)]);
    }
    int rc;
    {
        StreamGuard on_slot(ctx, ctx->streams[slots[0]]);
        rc = h_combine_rows(ctx, recs.data(), A, lg, P, cap, ctx->d_check_stage);
    }
    if (!rc) rc = msm_enqueue_batch(ctx, slots[0], ctx->d_bases, msm_one(ctx->d_check_stage + hcomb_rows_offset(A, lg, P, cap)), true, n);  // asynchronous
    if (rc) return rc;
    return combined_sides_agree(ctx, slots, usum_dev, res, ok, r, ctx->d_check_stage + u_off, held);
}

// ------------------------------------------------------------------ ... over members of SEVERAL degree bounds (halo_pcdl_check_batch_mixed_combined)
// A commitment of degree bound d_a lives on the prefix G[0 .. n_a) of the one key (pcdl.rs:99-110, :338), and a shorter h_a is a
// zero-padded vector over it: <sum_a r_a pad(h_a), G[0 .. n_max)> = sum_a r_a U_a, ONE MSM of n_max = the largest accepted n_a
// points whatever the members' sizes.  check_members_combined with the scalars from h_combine_rows_mixed (a length per table), the
// weights of check_mixed_weights and everything sized by lg_max; the right side is the same code.  blob_of / ds: the call's
// members, ok: the accepted ones with d >= 1 in member order.
static int check_members_mixed_combined(halo_ctx *ctx, const uint64_t *const *blob_of, const size_t *ds, const uint8_t *seed, const int *slots, int S,
                                        const std::vector<BatchCheck> &res, const std::vector<size_t> &ok, bool *held) {
    const size_t A = ok.size();
    *held = false;
    if (A > 65535) return HALO_OK;  // (h_combine_rows_mixed takes at most 65535 polynomials: the exact path)
    std::vector<uint32_t> lgs(A);
    size_t lg = 0;
    for (size_t a = 0; a < A; ++a) {
        lgs[a] = (uint32_t)ilog2(ds[ok[a]] + 1);
        if (lgs[a] > lg) lg = lgs[a];
    }
    if (lg > 24) return HALO_OK;  // (the exact path reports it)
    const size_t n = (size_t)1 << lg, tw = (lg + 2) * 4;
    const int forced = dev_hooks().combined_usum;
    const bool usum_dev = S >= 2 && A <= ctx_capacity(ctx) && (forced ? forced == 2 : A >= kCombinedUsumDeviceMin);
    const size_t cap = check_combined_cap(A);
    size_t P = check_combined_parts(n, A), u_off = 0;
    for (;; P = (P + 1) / 2) {  // (fewer parts if the staging cannot hold their rows)
        u_off = (hmix_stage_words(A, lg, P, cap) + 15) & ~(size_t)15;
        if (check_stage(ctx, 1, (u_off + (usum_dev ? A * (AFF_STRIDE / 2 + 16) : 0)) * 8) >= 1) break;
        if (P == 1) return HALO_OK;
    }
    std::vector<Fr> r;
    check_mixed_weights(blob_of, ds, ok.data(), A, seed, r);
    std::vector<uint64_t> recs(A * tw, 0);
    for (size_t a = 0; a < A; ++a) {
        for (size_t k = 0; k <= lgs[a]; ++k) res[ok[a]].st.xis[k].store(&recs[a * tw + 4 * k]);
        r[a].store(&recs[a * tw + 4 * (lgs[a] + 1)]);
    }
    int rc;
    {
        StreamGuard on_slot(ctx, ctx->streams[slots[0]]);
        rc = h_combine_rows_mixed(ctx, recs.data(), lgs.data(), A, lg, P, cap, ctx->d_check_stage);
    }
    if (!rc) rc = msm_enqueue_batch(ctx, slots[0], ctx->d_bases, msm_one(ctx->d_check_stage + hmix_rows_offset(A, lg, P, cap)), true, n);  // asynchronous
    if (rc) return rc;
    return combined_sides_agree(ctx, slots, usum_dev, res, ok, r, ctx->d_check_stage + u_off, held);
}

// ------------------------------------------------------------------ ... and BOTH halves as one relation (halo_pcdl_check_batch_fused)
// pcdl.rs:307-310 is as linear in the proof's points as :339.  With E_a = C'_a + sum_j (xi_(j+1)^-1 L_j + xi_(j+1) R_j) +
// (v_a - c_a h_a(z_a)) xi_0 H - c_a U_a (relation_terms' form) and F_a = U_a - <h_a, G>, the M >= 2 members whose transcripts
// held are checked as  sum_a r_a E_a + sum_a s_a F_a = 0  with the 2 M weights of check_fused_weights:
//   right side  <sum_a s_a h_a, G>: h_combine_rows with the weights s_a and ONE n-point MSM over the key on the first idle slot,
//               exactly the combined check's left side;
//   left side   T = M (2 lg n + 2) + 1 terms over the CALLER's points: each member's C' | L_j | R_j | U, then H.  Their scalars
//               come from k_fused_terms (fused_check.hip: one lane per member, H's scalar summed on the device), their points go
//               from Jacobian words to native entries with batch_to_affine (infinity and Z != 1 included).  The workspaces are
//               sized by the key, so the terms are cut into chunks of at most ctx_capacity points (the hook "check_fused_chunk":
//               fewer), the last one filled up with zero scalars on points at infinity; up to MSM_MAX_BATCH chunks are the members of
//               one batched launch sequence (MsmBatch::base_off: a chunk's own points), the sequences run one after the other
//               on the second idle slot while the key's MSM runs on the first -- with one idle slot, after it -- and the
//               chunks' sums are added on the host in chunk order.
// *held = both sides are the same point.  If not -- or without the optional staging -- the caller runs the exact batch.
static size_t fused_chunk_points(const halo_ctx *ctx, size_t T) {
    size_t C = ctx_capacity(ctx);
    const int forced = dev_hooks().fused_chunk;
    if (forced >= 8 && (size_t)forced < C) C = (size_t)forced;
    return C > T ? T : C;
}
// The left side is one body for the uniform call and for the mixed one (halo_pcdl_check_batch_mixed_fused, below): what differs is
// where a member's record and terms lie -- constant strides, or prefix sums over members of their own sizes -- and which kernel
// computes the scalars.  FusedMember: one taking-part member as the body packs it; FusedLeft: the terms' count, their cut into
// chunks and the staging (words):
//   records | shares | descriptors (the mixed call's) | scalars Tp x 4 | Jacobian words Tp x 12 | native entries (128-byte aligned)
// with the right side's regions behind them at o_h.
struct FusedMember {
    const uint64_t *q;       // its blob
    const SuccinctState *st;  // its accepted transcript
    size_t lg, rec_off, term_off;  // its size; where its record starts (words) and its first term lies (terms)
    const Fr *r, *s;         // its two weights
};
struct FusedLeft {
    size_t M, T, C, chunks, Tp;  // members; terms, H included; terms per chunk; chunks; terms with the last chunk filled up
    size_t o_rec, o_share, o_desc, o_sc, o_jac, o_nat, o_h;
};
// rec_words: all records; terms: the members' terms (H not counted); desc_words: 64-bit words of descriptors (0: none).  false: Tp
// does not fit MsmBatch::base_off's 32 bits (the exact path)
static bool fused_left_layout(const halo_ctx *ctx, size_t M, size_t rec_words, size_t terms, size_t desc_words, FusedLeft *L) {
    L->M = M;
    L->T = terms + 1;
    L->C = fused_chunk_points(ctx, L->T);
    L->chunks = (L->T + L->C - 1) / L->C;
    L->Tp = L->chunks * L->C;
    if (L->Tp >= ((size_t)1 << 32)) return false;
    L->o_rec = 0;
    L->o_share = L->o_rec + rec_words;
    L->o_desc = L->o_share + M * 4;
    L->o_sc = L->o_desc + ((desc_words + 3) & ~(size_t)3);
    L->o_jac = L->o_sc + L->Tp * 4;
    L->o_nat = (L->o_jac + L->Tp * 12 + 15) & ~(size_t)15;
    L->o_h = L->o_nat + L->Tp * (AFF_STRIDE / 2);
    return true;
}
// The left side of a fused relation whose right side's MSM is in flight on slots[0], through the context's check staging as L lays
// it out: the members' records and points packed on the host pool (member_at(a) -> FusedMember), H and the padding at infinity
// behind them, one upload; terms(d_recs, d_scalars, d_shares, d_h) computes the scalars on the current stream; the padding's
// scalars are zeroed, the points go to native entries, and the chunks run in batched sequences on the second idle slot (one idle
// slot: on it, after the right side).  The right side is collected whatever happened: nothing stays in flight.  *held = both
// sides are the same point.
template <class MemberAt, class Terms>
static int fused_sides_agree(halo_ctx *ctx, const int *slots, int S, const FusedLeft &L, MemberAt member_at, Terms terms, bool *held) {
    const size_t M = L.M, T = L.T, C = L.C, Tp = L.Tp;
    uint64_t *d_stage = ctx->d_check_stage;
    Point right, left = Point::infinity();
    bool right_done = false;
    auto finish_right = [&]() { right_done = true; return msm_finish_batch(ctx, slots[0], &right, 1); };
    int rc = HALO_OK;
    if (S < 2) rc = finish_right();  // (one idle slot: the left side runs on it afterwards)
    const int lslot = S < 2 ? slots[0] : slots[1];
    // the left side's records and points
    std::vector<uint64_t> recs(L.o_share - L.o_rec), jac(Tp * 12);
    if (!rc) {
        pool_run(M, [&](size_t a) {
            const FusedMember m = member_at(a);
            const size_t lg = m.lg;
            uint64_t *proof = const_cast<uint64_t *>(m.q) + 21;
            uint64_t *r = &recs[m.rec_off], *p = &jac[m.term_off * 12];
            for (size_t k = 0; k <= lg; ++k) m.st->xis[k].store(r + 4 * k);
            std::memcpy(r + 4 * (lg + 1), m.q + 13, 64);                   // z | v
            std::memcpy(r + 4 * (lg + 3), pf_c(proof, lg), 32);            // c
            m.r->store(r + 4 * (lg + 4));
            m.s->store(r + 4 * (lg + 5));
            m.st->C_prime.store(p);
            std::memcpy(p + 12, pf_L(proof, 0), lg * 96);                  // L_0 .. (the blob's own words)
            std::memcpy(p + 12 * (lg + 1), pf_R(proof, lg, 0), lg * 96);   // R_0 ..
            std::memcpy(p + 12 * (2 * lg + 1), pf_U(proof, lg), 96);
        });
        static const Point kH = public_h_table().mul(Fr::one());
        kH.store(&jac[(T - 1) * 12]);
        for (size_t t = T; t < Tp; ++t) Point::infinity().store(&jac[t * 12]);
        hipError_t e = hipMemcpy(d_stage + L.o_rec, recs.data(), recs.size() * 8, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(d_stage + L.o_jac, jac.data(), jac.size() * 8, hipMemcpyHostToDevice);
        if (e != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    }
    if (!rc) {
        StreamGuard on_slot(ctx, ctx->streams[lslot]);
        rc = terms(d_stage + L.o_rec, d_stage + L.o_sc, d_stage + L.o_share, d_stage + L.o_sc + (T - 1) * 4);
        if (!rc && Tp > T) {
            hipError_t e = hipMemsetAsync(d_stage + L.o_sc + T * 4, 0, (Tp - T) * 32, ctx->stream);
            if (e != hipSuccess) rc = hip_fail(e, "hipMemsetAsync");
        }
        if (!rc) rc = batch_to_affine(ctx, d_stage + L.o_jac, Tp, reinterpret_cast<uint32_t *>(d_stage + L.o_nat));
    }
    if (!rc) {
        const size_t G = (size_t)group_size(ctx, C, 0, MSM_MAX_BATCH, 1);
        rc = rotate_groups(
            ctx, &lslot, 1, L.chunks, G < L.chunks ? G : L.chunks,
            [&](size_t, size_t first, size_t cnt) -> int {
                MsmBatch mb;
                mb.count = (int)cnt;
                for (size_t b = 0; b < cnt; ++b) {
                    mb.scalars[b] = d_stage + L.o_sc + (first + b) * C * 4;
                    mb.base_off[b] = (uint32_t)((first + b) * C);
                }
                return msm_enqueue_batch(ctx, lslot, reinterpret_cast<const uint32_t *>(d_stage + L.o_nat), mb, false, C);
            },
            [&](size_t, size_t cnt, const Point *pts) {
                for (size_t b = 0; b < cnt; ++b) left = left + pts[b];
            });
    }
    const std::string err = rc ? halo_last_error() : "";
    if (!right_done) {  // (collected whatever happened to the left side: nothing stays in flight)
        int rc_r = finish_right();
        if (!rc) rc = rc_r;
        else set_error(err);
    }
    if (rc) return rc;
    *held = left == right;
    return HALO_OK;
}
static int check_members_fused(halo_ctx *ctx, size_t d, const uint64_t *qs, size_t stride, const uint8_t *seed, const int *slots, int S,
                               const std::vector<BatchCheck> &res, const std::vector<size_t> &ok, bool *held) {
    const size_t n = d + 1, lg = ilog2(n), M = ok.size(), tw = (lg + 2) * 4;
    *held = false;
    if (lg > 24) { set_error("h_coeffs: lg_n > 24 unsupported"); return HALO_E_ARG; }
    if (M > 65535) return HALO_OK;  // (h_combine_rows takes at most 65535 polynomials: the exact batch)
    const size_t K = fused_term_count((int)lg), rw = fused_rec_words((int)lg);
    FusedLeft L;
    if (!fused_left_layout(ctx, M, M * rw, M * K, 0, &L)) return HALO_OK;
    const size_t cap = check_combined_cap(M);
    size_t P = check_combined_parts(n, M);
    for (;; P = (P + 1) / 2) {  // (fewer parts if the staging cannot hold their rows)
        if (check_stage(ctx, 1, (L.o_h + hcomb_stage_words(M, lg, P, cap)) * 8) >= 1) break;
        if (P == 1) return HALO_OK;
    }
    uint64_t *d_stage = ctx->d_check_stage;
    std::vector<Fr> w;
    check_fused_weights(qs, stride, ok.data(), M, d, seed, w);
    // the right side: sum_a s_a h_a(X) over the key, asynchronous
    {
        std::vector<uint64_t> recs(M * tw);
        for (size_t a = 0; a < M; ++a) {
            for (size_t k = 0; k <= lg; ++k) res[ok[a]].st.xis[k].store(&recs[a * tw + 4 * k]);
            w[2 * a + 1].store(&recs[a * tw + 4 * (lg + 1)]);
        }
        int rc;
        {
            StreamGuard on_slot(ctx, ctx->streams[slots[0]]);
            rc = h_combine_rows(ctx, recs.data(), M, lg, P, cap, d_stage + L.o_h);
        }
        if (!rc) rc = msm_enqueue_batch(ctx, slots[0], ctx->d_bases, msm_one(d_stage + L.o_h + hcomb_rows_offset(M, lg, P, cap)), true, n);
        if (rc) return rc;
    }
    return fused_sides_agree(
        ctx, slots, S, L, [&](size_t a) { return FusedMember{qs + ok[a] * stride, &res[ok[a]].st, lg, a * rw, a * K, &w[2 * a], &w[2 * a + 1]}; },
        [&](const uint64_t *d_recs, uint64_t *d_sc, uint64_t *d_shares, uint64_t *d_h) { return fused_terms(ctx, d_recs, M, lg, nullptr, d_sc, d_shares, d_h); },
        held);
}

// ------------------------------------------------------------------ ... and that over members of SEVERAL degree bounds (halo_pcdl_check_batch_mixed_fused)
// check_members_fused with a size per member.  Right side: <sum_a s_a pad(h_a), G[0 .. n_max)>, the mixed combined check's scalars
// (h_combine_rows_mixed) with the weights s_a and ONE n_max-point MSM over the key.  Left side: the same body; the members' records
// and terms lie dense in member order, fused_rec_words(lg_a) words and 2 lg_a + 2 terms each, so the chunked MSMs see T = sum_a
// (2 lg_a + 2) + 1 terms with nothing between members, and k_mixed_terms (mixed_terms.hip) finds each member's through its
// descriptor {lg_a, record offset, term offset}.  blob_of / ds: the call's members, ok: those whose transcripts held with d >= 1,
// in member order; tr: the transcripts in member order.
static int check_members_mixed_fused(halo_ctx *ctx, const uint64_t *const *blob_of, const size_t *ds, const uint8_t *seed, const int *slots, int S,
                                     const std::vector<BatchCheck> &tr, const std::vector<size_t> &ok, bool *held) {
    const size_t M = ok.size();
    *held = false;
    if (M > 65535) return HALO_OK;  // (h_combine_rows_mixed and fr_sum_rows take at most 65535 rows: the exact path)
    std::vector<uint32_t> lgs(M);
    size_t lg = 0;
    for (size_t a = 0; a < M; ++a) {
        lgs[a] = (uint32_t)ilog2(ds[ok[a]] + 1);
        if (lgs[a] > lg) lg = lgs[a];
    }
    if (lg > (size_t)FUSED_MAX_LG) return HALO_OK;  // (the exact path reports it)
    std::vector<uint32_t> desc(M * MIXED_DESC_WORDS + 1);
    size_t rec_words = 0, terms = 0;
    mixed_terms_describe(lgs.data(), M, desc.data(), &rec_words, &terms);
    const size_t desc_words = (M * MIXED_DESC_WORDS + 1) / 2;
    FusedLeft L;
    if (!fused_left_layout(ctx, M, rec_words, terms, desc_words, &L)) return HALO_OK;
    const size_t n = (size_t)1 << lg, tw = (lg + 2) * 4;
    const size_t cap = check_combined_cap(M);
    size_t P = check_combined_parts(n, M);
    for (;; P = (P + 1) / 2) {  // (fewer parts if the staging cannot hold their rows)
        if (check_stage(ctx, 1, (L.o_h + hmix_stage_words(M, lg, P, cap)) * 8) >= 1) break;
        if (P == 1) return HALO_OK;
    }
    uint64_t *d_stage = ctx->d_check_stage;
    std::vector<Fr> w;
    check_mixed_fused_weights(blob_of, ds, ok.data(), M, seed, w);
    // the right side: sum_a s_a pad(h_a)(X) over the key, asynchronous
    {
        std::vector<uint64_t> recs(M * tw, 0);
        for (size_t a = 0; a < M; ++a) {
            for (size_t k = 0; k <= lgs[a]; ++k) tr[ok[a]].st.xis[k].store(&recs[a * tw + 4 * k]);
            w[2 * a + 1].store(&recs[a * tw + 4 * (lgs[a] + 1)]);
        }
        int rc;
        {
            StreamGuard on_slot(ctx, ctx->streams[slots[0]]);
            rc = h_combine_rows_mixed(ctx, recs.data(), lgs.data(), M, lg, P, cap, d_stage + L.o_h);
        }
        if (!rc) rc = msm_enqueue_batch(ctx, slots[0], ctx->d_bases, msm_one(d_stage + L.o_h + hmix_rows_offset(M, lg, P, cap)), true, n);
        if (rc) return rc;
    }
    return fused_sides_agree(
        ctx, slots, S, L,
        [&](size_t a) {
            const uint32_t *da = &desc[MIXED_DESC_WORDS * a];
            return FusedMember{blob_of[ok[a]], &tr[ok[a]].st, da[0], da[1], da[2], &w[2 * a], &w[2 * a + 1]};
        },
        [&](const uint64_t *d_recs, uint64_t *d_sc, uint64_t *d_shares, uint64_t *d_h) -> int {
            uint32_t *d_desc = reinterpret_cast<uint32_t *>(d_stage + L.o_desc);
            HALO_HIP(hipMemcpy(d_desc, desc.data(), M * MIXED_DESC_WORDS * 4, hipMemcpyHostToDevice));
            return fused_terms(ctx, d_recs, M, 0, d_desc, d_sc, d_shares, d_h);
        },
        held);
}

// blobs: m Instances (or Accumulators, whose Instance prefix is checked) at `stride` words, all of degree bound d (checked by
// the caller); status[i] (nullable) = what halo_pcdl_check returns for member i alone
// seed: the combined / fused call's 32 bytes (or null)
enum class CheckMode { exact, combined, fused };
static int pcdl_check_batch_host(halo_ctx *ctx, size_t d, const uint64_t *qs, size_t stride, size_t m, int *status, CheckMode mode = CheckMode::exact,
                                 const uint8_t *seed = nullptr) {
    const size_t n = d + 1;
    const bool combined = mode == CheckMode::combined;
    int slots[HALO_SLOTS], S = idle_slots(ctx, slots);
    if (!S) { set_error("check_batch: every slot has an MSM in flight"); return HALO_E_ARG; }
    if (mode == CheckMode::fused && m >= 2 && n >= 2) {  // (one member, or a constant: the exact path below)
        // the transcripts alone, as succinct_challenges runs them (no relation: that is the fused relation's left side)
        std::vector<BatchCheck> tr;
        int rc_tr = transcripts_batch(ctx, d, [&](size_t i) { return qs + i * stride; }, m, tr);
        if (rc_tr) return rc_tr;
        std::vector<size_t> acc;
        for (size_t i = 0; i < m; ++i)
            if (!tr[i].rc) acc.push_back(i);
        bool fused_held = false;
        if (acc.size() >= 2) {
            int rc = check_members_fused(ctx, d, qs, stride, seed, slots, S, tr, acc, &fused_held);
            if (rc) return rc;
        }
        if (fused_held) return report_members("instance", m, [&](size_t i) { return tr[i].rc; }, [&](size_t i) { return tr[i].err; }, status, [](size_t) {});
        // the relation failed, or did not run: the exact batch decides, so a reject never depends on the weights
    }
    // 1. the succinct half (pcdl.rs:333)
    std::vector<BatchCheck> res;
    int rc = succinct_half(ctx, d, [&](size_t i) { return qs + i * stride; }, m, res);
    if (rc) return rc;
    std::vector<size_t> ok;  // the accepted members, in order
    for (size_t i = 0; i < m; ++i)
        if (!res[i].rc) ok.push_back(i);
    bool held = false;
    if (combined && ok.size() >= 2 && n >= 2) {  // (one member, or a constant: nothing to combine)
        rc = check_members_combined(ctx, d, qs, stride, seed, slots, S, res, ok, &held);
        if (rc) return rc;
    }
    if (!held) {  // the exact batch; after a combined relation that failed: which members fail does not depend on the weights
        rc = check_members_exact(ctx, n, slots, S, res, ok);
        if (rc) return rc;
    }
    return report_members("instance", m, [&](size_t i) { return res[i].rc; }, [&](size_t i) { return res[i].err; }, status, [](size_t) {});
}
// the argument checks of both entry points (halo_pcdl_succinct_check_batch's), then the batch; acc: Accumulator blobs
static int check_batch_entry(halo_ctx *ctx, size_t d, const uint64_t *blobs, size_t m, int *status, bool acc, CheckMode mode = CheckMode::exact,
                             const uint8_t *seed = nullptr) {
    if (m && !blobs) { set_error("check_batch: null pointer"); return HALO_E_ARG; }
    if (!is_pow2(d + 1)) return fail_reject("d+1 is not a power of 2!");
    size_t lg = ilog2(d + 1), stride = acc ? acc_words(lg) : instance_words(lg);
    for (size_t i = 0; i < m; ++i)
        if ((size_t)(blobs + i * stride)[12] != d || (blobs + i * stride)[22] != lg) return fail_reject("d_i != d");
    if (m == 0) return HALO_OK;
    return pcdl_check_batch_host(ctx, d, blobs, stride, m, status, mode, seed);
}

// ------------------------------------------------------------------ ... of m instances of SEVERAL degree bounds (halo_pcdl_check_batch_mixed, .._combined, .._fused)
// Member i is the blob blobs[i] of degree bound ds[i] (checked by the caller).  The members are grouped into classes of equal d, in
// the order of their first member.  Each class runs the succinct half of the uniform call (succinct_half) and -- the exact form,
// d = 0, and whenever the combined relation did not hold or did not run -- check_members_exact over its accepted members; the
// results sit in member order throughout (res[i]), a class is a list of member indices.  The combined form puts the accepted
// members with d >= 1 of ALL classes into one relation (check_members_mixed_combined).
//
// The fused form (halo_pcdl_check_batch_mixed_fused) runs the transcripts alone per class first (transcripts_batch: a class of its
// own size takes the device route by the uniform rule), then ONE relation over the members of every class whose transcripts held
// with d >= 1 (check_members_mixed_fused).  If it held, the transcripts' outcomes are the call's; if it failed or did not run --
// or constants are among the members -- the exact path below runs from the top.
static int pcdl_check_mixed_host(halo_ctx *ctx, const size_t *ds, const uint64_t *const *blobs, size_t m, int *status, CheckMode mode, const uint8_t *seed) {
    const bool combined = mode == CheckMode::combined;
    int slots[HALO_SLOTS], S = idle_slots(ctx, slots);
    if (!S) { set_error("check_batch: every slot has an MSM in flight"); return HALO_E_ARG; }
    std::vector<std::vector<size_t>> classes;  // member indices, ascending
    {
        std::vector<size_t> seen;  // the classes' degree bounds (a call holds a handful)
        for (size_t i = 0; i < m; ++i) {
            size_t c = 0;
            while (c < seen.size() && seen[c] != ds[i]) ++c;
            if (c == seen.size()) { seen.push_back(ds[i]); classes.emplace_back(); }
            classes[c].push_back(i);
        }
    }
    // the classes the fused relation settled: their members' outcomes are in res already (constants never are)
    bool fused_held = false;
    std::vector<BatchCheck> res(m);
    if (mode == CheckMode::fused) {
        size_t taking = 0;  // members with d >= 1
        for (size_t i = 0; i < m; ++i) taking += ds[i] >= 1;
        if (taking >= 2) {
            // the transcripts alone, as succinct_challenges runs them (no relation: that is the fused relation's left side)
            std::vector<BatchCheck> tr(m);
            for (const std::vector<size_t> &cls : classes) {
                if (ds[cls[0]] == 0) continue;
                std::vector<BatchCheck> part;
                int rc = transcripts_batch(ctx, ds[cls[0]], [&](size_t j) { return blobs[cls[j]]; }, cls.size(), part);
                if (rc) return rc;
                for (size_t j = 0; j < cls.size(); ++j) tr[cls[j]] = std::move(part[j]);
            }
            std::vector<size_t> acc;
            for (size_t i = 0; i < m; ++i)
                if (ds[i] >= 1 && !tr[i].rc) acc.push_back(i);
            if (acc.size() >= 2) {
                int rc = check_members_mixed_fused(ctx, blobs, ds, seed, slots, S, tr, acc, &fused_held);
                if (rc) return rc;
            }
            if (fused_held)
                for (size_t i = 0; i < m; ++i)
                    if (ds[i] >= 1) res[i] = std::move(tr[i]);
            // else the relation failed, or did not run: the exact path decides, so a reject never depends on the weights
        }
    }
    // 1. the succinct half, class by class (pcdl.rs:333)
    for (const std::vector<size_t> &cls : classes) {
        if (fused_held && ds[cls[0]] >= 1) continue;
        std::vector<BatchCheck> part;
        int rc = succinct_half(ctx, ds[cls[0]], [&](size_t j) { return blobs[cls[j]]; }, cls.size(), part);
        if (rc) return rc;
        for (size_t j = 0; j < cls.size(); ++j) res[cls[j]] = std::move(part[j]);
    }
    // 2. one relation over the accepted members of every class (a constant has nothing to combine)
    bool held = false;
    if (combined) {
        std::vector<size_t> ok;
        for (size_t i = 0; i < m; ++i)
            if (!res[i].rc && ds[i] >= 1) ok.push_back(i);
        if (ok.size() >= 2) {
            int rc = check_members_mixed_combined(ctx, blobs, ds, seed, slots, S, res, ok, &held);
            if (rc) return rc;
        }
    }
    // 3. the exact path, class by class: every class if the relation failed or did not run -- which members fail never depends on
    // the weights --, else the constants alone
    for (const std::vector<size_t> &cls : classes) {
        const size_t d = ds[cls[0]];
        if ((held || fused_held) && d >= 1) continue;
        std::vector<size_t> ok;
        for (size_t i : cls)
            if (!res[i].rc) ok.push_back(i);
        int rc = check_members_exact(ctx, d + 1, slots, S, res, ok);
        if (rc) return rc;
    }
    return report_members("instance", m, [&](size_t i) { return res[i].rc; }, [&](size_t i) { return res[i].err; }, status, [](size_t) {});
}
// the whole-call checks of the six mixed entry points, then the batch
static int check_mixed_entry(halo_ctx *ctx, const size_t *ds, const uint64_t *const *blobs, size_t m, int *status, CheckMode mode, const uint8_t *seed) {
    if (m && (!ds || !blobs)) { set_error("check_batch: null pointer"); return HALO_E_ARG; }
    for (size_t i = 0; i < m; ++i)
        if (!blobs[i]) { set_error("check_batch: null pointer"); return HALO_E_ARG; }
    for (size_t i = 0; i < m; ++i)
        if (!is_pow2(ds[i] + 1)) return fail_reject("d+1 is not a power of 2!");
    for (size_t i = 0; i < m; ++i)
        if ((size_t)blobs[i][12] != ds[i] || blobs[i][22] != ilog2(ds[i] + 1)) return fail_reject("d_i != d");
    if (m == 0) return HALO_OK;
    return pcdl_check_mixed_host(ctx, ds, blobs, m, status, mode, seed);
}

// ------------------------------------------------------------------ pcdl::commit of m polynomials at once
// (halo_pcdl_commit_batch: host polynomials, m x n scalars zero-padded; halo_pcdl_commit_dev_batch: device pointers and lengths.)
// Groups of up to MSM_MAX_BATCH members, each ONE batched MSM launch sequence over the key, rotate over the slots idle on entry
// exactly as the check batch's do.  A group's scalars reach its slot's region of the staging on the slot's own stream: the host
// form copies the group's padded rows in one hipMemcpyAsync (the rows are contiguous in the caller's array), so the copy of
// group g + 1 runs under the kernels of group g on another slot; the device form passes a full-length member to the launch in
// place and pads the shorter ones with one k_pad_members_batch launch.  When a slot comes round again its group is collected and
// the w_i S terms are added on the host.  Without the staging the members run one at a time through the single calls' bodies.
// Members per launch: the rule of check_group_size ("commit_batch_group" forces one) -- single members where the fixed-base
// table takes the MSM, there the gain is the copy hidden under the previous member's kernels.  ONE host polynomial at such a size
// goes through the single call's body instead: it copies in stretches under its own kernels (msm_host_run), which one copy in
// front of one launch sequence cannot match (1.70 against 1.81 ms at 2^20, the runs' ranges apart; from two members on the pipeline wins,
// 3.32 against 2.83 ms).  Measured: DESIGN.md 4.9.
static bool commit_table_single(const halo_ctx *ctx, size_t n) {  // (a forced group size: the pipeline, whatever the size)
    return dev_hooks().commit_group <= 0 && n >= ((size_t)1 << 20) && ctx->n >= ((size_t)1 << 20) && ctx->table_mode != 0;
}
static int commit_group_size(const halo_ctx *ctx, size_t n) {
    if (commit_table_single(ctx, n)) return 1;
    return group_size(ctx, n, dev_hooks().commit_group, MSM_MAX_BATCH, 1);  // (development library: the sweep of tools/time_commit_batch.py)
}
// live: the members that run, in order (all of them in the host form); coeffs: the host form's array, else d_coeffs / lens.
// Without the optional staging a group is ONE member and its row the slot's own scalar buffer (slot_scalars: what halo_msm_begin
// copies into), so the members still run on the idle slots only, one at a time per slot, with the same points.
static int commit_batch_run(halo_ctx *ctx, size_t d, const uint64_t *coeffs, const void *const *d_coeffs, const size_t *lens,
                            const std::vector<size_t> &live, const uint64_t *ws, uint64_t *out, const int *slots, int S) {
    const size_t n = d + 1, A = live.size();
    if (A == 0) return HALO_OK;
    auto finish = [&](size_t i, const Point &msm) {
        (ws ? public_s_table().mul(Fr::load(ws + 4 * i)) + msm : msm).store_normalized(out + 12 * i);
    };
    // (the single call spreads its copy over slots 0 and 1: both idle, as a caller of halo_pcdl_commit must have them)
    if (coeffs && A == 1 && commit_table_single(ctx, n) && S >= 2 && slots[0] == 0 && slots[1] == 1) {
        const size_t i = live[0];
        const Fr wf = ws ? Fr::load(ws + 4 * i) : Fr::zero();
        Point r;
        int rc = pcdl_commit_host(ctx, coeffs + i * n * 4, n, d, ws ? &wf : nullptr, &r);
        if (!rc) r.store_normalized(out + 12 * i);
        return rc;
    }
    size_t G = (size_t)commit_group_size(ctx, n);
    if (G > A) G = A;
    if ((size_t)S > (A + G - 1) / G) S = (int)((A + G - 1) / G);
    bool pads = coeffs != nullptr;  // does any member need a row?  (device members of full length are read in place)
    for (size_t a = 0; a < A && !pads; ++a) pads = lens[live[a]] != n;
    const size_t have = pads ? check_stage(ctx, G * (size_t)S, n * 32) : G * (size_t)S;
    uint64_t *own[HALO_SLOTS] = {};  // no staging: the slots' own scalar buffers, one member each
    if (have == 0) {
        G = 1;
        if ((size_t)S > A) S = (int)A;
        for (int j = 0; j < S; ++j)
            if (!(own[j] = slot_scalars(ctx, slots[j], 1, 0))) return HALO_E_DEVICE;
    } else if (have < G * (size_t)S) {
        if (G > have) G = have;
        if ((size_t)S > have / G) S = (int)(have / G);
    }
    auto row_of = [&](size_t j, size_t b) { return have ? ctx->d_check_stage + (j * G + b) * n * 4 : own[j]; };
    return rotate_groups(
        ctx, slots, S, A, G,
        [&](size_t j, size_t first, size_t cnt) -> int {
            MsmBatch mb;
            mb.count = (int)cnt;
            int rc = HALO_OK;
            {
                StreamGuard on_slot(ctx, ctx->streams[slots[j]]);
                if (coeffs) {  // (live = every member: the group's rows are one stretch of the caller's array)
                    HALO_HIP(hipMemcpyAsync(row_of(j, 0), coeffs + live[first] * n * 4, cnt * n * 32, hipMemcpyHostToDevice, ctx->stream));
                    for (size_t b = 0; b < cnt; ++b) mb.scalars[b] = row_of(j, b);
                } else {
                    PadMembers t{};
                    int short_members = 0;
                    for (size_t b = 0; b < cnt; ++b) {
                        const size_t i = live[first + b];
                        if (lens[i] == n) { mb.scalars[b] = static_cast<const uint64_t *>(d_coeffs[i]); continue; }  // in place
                        t.src[short_members] = static_cast<const uint64_t *>(d_coeffs[i]);
                        t.len[short_members] = (uint32_t)lens[i];
                        t.row[short_members++] = (uint32_t)b;
                        mb.scalars[b] = row_of(j, b);
                    }
                    if (short_members) rc = pad_members_batch(ctx, t, short_members, n, row_of(j, 0), n * 4);
                }
            }
            return rc ? rc : msm_enqueue_batch(ctx, slots[j], ctx->d_bases, mb, true, n);  // asynchronous
        },
        [&](size_t first, size_t cnt, const Point *pts) {
            for (size_t b = 0; b < cnt; ++b) finish(live[first + b], pts[b]);
        });
}
// the whole-call checks of both commit batches (pcdl_commit_host's asserts, before any work)
static int commit_batch_checks(halo_ctx *ctx, size_t d, int *slots, int *S) {
    if (!is_pow2(d + 1)) return fail_assert("commit: d + 1 is not a power of two");
    if (d + 1 > ctx->n) return fail_assert("commit: d > D");
    *S = idle_slots(ctx, slots);
    if (!*S) { set_error("commit_batch: every slot has an MSM in flight"); return HALO_E_ARG; }
    return HALO_OK;
}

// ------------------------------------------------------------------ acc::verifier of k accumulators at once
// (halo_acc_verifier_batch; acc.rs:223-243 per member, each member's outcome the single call's)
//  1. the transcripts: one pool pass over the instances of every member that reaches its succinct checks -- C', the
//     challenges (succinct_challenges) and h_i(z_i), i.e. the relation's terms (relation_terms); then one pass over the members:
//     alpha = rho_1(hs) (:173), its powers, and the terms of h_0[0] G_0 + h_0[1] G_1 (:152-155) and C = sum_i alpha^i U_i (:178).
//  2. every sum of the batch at once: ONE k_small_msm_seg launch on a slot idle at entry, from kVerifierBatchMin relations on;
//     below that, without an idle slot or without staging (optional memory: check_stage), the host pool, sum by sum.
//  3. one pass over the members: z' = rho_1(C, alpha) (:181), C_bar' = C + w S (:184), h(z), and the status in the single
//     call's order (fields, U_0, d_i, the succinct checks in instance order, C_bar', z', d', h(z)).
constexpr size_t kVerifierBatchMin = 64;  // relations; measured: tools/time_verifier_batch.py
constexpr size_t kSegMaxTerms = 64;      // terms per sum of k_small_msm_seg (a longer C is summed in parts)

struct VerifierMember {
    int rc = HALO_OK;
    std::string err;
    size_t first = 0, m = 0;  // its instances in the flat list
    bool sums = false;        // reaches the U_0 check (fields valid, deg h_0 <= d)
    bool reach = false;       // ... and its succinct checks (every d_i == d)
    bool all_ok = false;      // ... and every transcript held: C is summed
    size_t s_u0 = 0, s_c = 0, n_c = 0;  // its sums: h_0 against U_0, the n_c parts of C
    AccHPolys hs;
};
// Every sum of a batch, term by term: sum s holds terms off[s] .. off[s + 1], a term is a point (arkworks affine, (0, 0) =
// infinity) and a canonical scalar -- the format of k_small_msm_seg
struct SumList {
    std::vector<uint32_t> off{0};
    std::vector<uint64_t> pts, sc;
    size_t add(size_t terms) { off.push_back(off.back() + (uint32_t)terms); return off.size() - 2; }
    size_t count() const { return off.size() - 1; }
    size_t terms() const { return off.back(); }
    void put_point(size_t t, const Point &p) {
        host::Affine a = p.to_affine();
        if (!a.inf) { a.x.store(&pts[8 * t]); a.y.store(&pts[8 * t + 4]); }
    }
};

// 0. what the single call checks before any arithmetic, and the sums' layout.  rel_sum: the relation sum of each instance;
// work: the instances whose transcripts run
static void verifier_layout(size_t d, const uint64_t *qs, const uint64_t *accs, std::vector<VerifierMember> &mem, SumList &L,
                            std::vector<size_t> &rel_sum, std::vector<size_t> &work) {
    const size_t lg = ilog2(d + 1), iw = instance_words(lg), aw = acc_words(lg), K = 2 * lg + 2;
    const size_t u0_terms = d ? 2 : 1;  // (d = 0: h_0 is a constant, or the assert below)
    for (size_t j = 0; j < mem.size(); ++j) {
        VerifierMember &M = mem[j];
        const uint64_t *acc = accs + j * aw, *piV = acc + iw;
        M.hs.h0[0] = Fr::load(piV);
        M.hs.h0[1] = Fr::load(piV + 4);
        M.hs.lg_n = lg;
        if (!Point::load(piV + 8).on_curve() || !Point::load(acc).on_curve() || !scalar_ok(M.hs.h0[0]) || !scalar_ok(M.hs.h0[1]) ||
            !scalar_ok(Fr::load(piV + 20)) || !scalar_ok(Fr::load(acc + 13)) || !scalar_ok(Fr::load(acc + 17))) {
            M.rc = HALO_E_REJECT;
            M.err = "accumulator holds an invalid point or scalar";
            continue;
        }
        if (host_poly_degree(piV, 2) > d) { M.rc = HALO_E_ASSERT; M.err = "commit: p.degree() > d"; continue; }  // pcdl_commit_host
        M.sums = true;
        M.s_u0 = L.add(u0_terms);
        M.reach = true;
        for (size_t i = 0; i < M.m && M.reach; ++i) {
            const uint64_t *q = qs + (M.first + i) * iw;
            if ((size_t)q[12] != d || q[22] != lg) M.reach = false;  // :169
        }
        if (!M.reach) continue;
        for (size_t i = 0; i < M.m; ++i) {
            rel_sum[M.first + i] = L.add(K);
            work.push_back(M.first + i);
        }
        M.n_c = (M.m + 1 + kSegMaxTerms - 1) / kSegMaxTerms;
        M.s_c = L.count();
        for (size_t c = 0; c < M.n_c; ++c) L.add(c + 1 < M.n_c ? kSegMaxTerms : M.m + 1 - c * kSegMaxTerms);
    }
}
// 2. every sum in ONE k_small_msm_seg launch on ctx->stream, through the context's staging (bytes): points nterms x 64 |
// scalars nterms x 32 | results nsums x 96 | off (nsums + 1) x 4 | desc waves x 256
static int sums_on_device(halo_ctx *ctx, const SumList &L, const std::vector<uint32_t> &desc, size_t waves, std::vector<Point> &sums) {
    const size_t nsums = L.count(), nterms = L.terms();
    uint64_t *d_pts = ctx->d_check_stage, *d_sc = d_pts + nterms * 8, *d_out = d_sc + nterms * 4;
    uint32_t *d_off = reinterpret_cast<uint32_t *>(d_out + nsums * 12), *d_desc = d_off + nsums + 1;
    auto copy = [&](void *dst, const void *src, size_t bytes, hipMemcpyKind kind) {
        hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, ctx->stream);
        return e == hipSuccess ? HALO_OK : hip_fail(e, "hipMemcpyAsync");
    };
    int rc = copy(d_pts, L.pts.data(), nterms * 64, hipMemcpyHostToDevice);
    if (!rc) rc = copy(d_sc, L.sc.data(), nterms * 32, hipMemcpyHostToDevice);
    if (!rc) rc = copy(d_off, L.off.data(), (nsums + 1) * 4, hipMemcpyHostToDevice);
    if (!rc) rc = copy(d_desc, desc.data(), desc.size() * 4, hipMemcpyHostToDevice);
    if (!rc) rc = small_msm_seg(ctx, d_pts, d_sc, d_off, d_desc, waves, d_out);
    std::vector<uint64_t> out(nsums * 12);
    if (!rc) rc = copy(out.data(), d_out, nsums * 96, hipMemcpyDeviceToHost);
    if (rc) return rc;
    hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return hip_fail(e, "hipStreamSynchronize");
    for (size_t s = 0; s < nsums; ++s) sums[s] = Point::load(&out[12 * s]);
    return HALO_OK;
}

static int acc_verifier_batch_host(halo_ctx *ctx, size_t d, const uint64_t *qs, const size_t *counts, size_t k, const uint64_t *accs, int *status) {
    const size_t lg = ilog2(d + 1), iw = instance_words(lg), aw = acc_words(lg), K = 2 * lg + 2;
    if (K > kSegMaxTerms) { set_error("verifier_batch: lg n too large"); return HALO_E_ARG; }
    std::vector<VerifierMember> mem(k);
    size_t total = 0;
    for (size_t j = 0; j < k; ++j) { mem[j].first = total; mem[j].m = counts[j]; total += counts[j]; }
    SumList L;
    std::vector<size_t> rel_sum(total, 0), work;
    verifier_layout(d, qs, accs, mem, L, rel_sum, work);
    const size_t nsums = L.count(), nterms = L.terms();
    if (nterms >= ((size_t)1 << 31) || nsums >= ((size_t)1 << 28)) { set_error("verifier_batch: too many terms"); return HALO_E_ARG; }
    L.pts.assign(nterms * 8, 0);
    L.sc.assign(nterms * 4, 0);
    // 1. the transcripts and the relations' terms
    std::vector<BatchCheck> res(total);
    pool_run(work.size(), [&](size_t w) {
        const size_t i = work[w];
        const uint64_t *q = qs + i * iw;
        BatchCheck &r = res[i];
        const Fr z = Fr::load(q + 13);
        r.rc = succinct_challenges(ctx, Point::load(q), d, z, Fr::load(q + 17), q + 21, &r.st, false);
        if (r.rc) { r.err = halo_last_error(); return; }
        const size_t o = L.off[rel_sum[i]];
        relation_terms(r.st, q, host::h_eval(r.st.xis.data(), lg, z), &L.pts[8 * o], &L.sc[4 * o]);  // h(z) as k_h_eval_z computes it
    });
    uint64_t g01[16] = {};  // G_0, G_1
    const size_t u0_terms = d ? 2 : 1;
    auto member_terms = [&](size_t j) {  // alpha, its powers, the terms of the U_0 check and of C
        VerifierMember &M = mem[j];
        const uint64_t *piV = accs + j * aw + iw;
        const size_t u = L.off[M.s_u0];
        for (size_t t = 0; t < u0_terms; ++t) {
            std::memcpy(&L.pts[8 * (u + t)], g01 + 8 * t, 64);
            M.hs.h0[t].from_mont().store(&L.sc[4 * (u + t)]);
        }
        if (!M.reach) return;
        for (size_t i = 0; i < M.m; ++i)
            if (res[M.first + i].rc) return;
        M.all_ok = true;
        for (size_t i = 0; i < M.m; ++i) M.hs.xis.push_back(res[M.first + i].st.xis);
        set_alphas(&M.hs);
        const size_t c0 = L.off[M.s_c];  // the parts of C are consecutive: term t of C is term c0 + t
        for (size_t t = 0; t <= M.m; ++t) {
            L.put_point(c0 + t, t ? res[M.first + t - 1].st.U : Point::load(piV + 8));
            M.hs.alphas[t].from_mont().store(&L.sc[4 * (c0 + t)]);
        }
    };
    // 2. every sum: on the device in one launch on a slot idle at entry, or on the host pool
    std::vector<Point> sums(nsums, Point::infinity());
    int idle[HALO_SLOTS];
    const int slot = idle_slots(ctx, idle) ? idle[0] : -1;
    std::vector<uint32_t> desc;
    const size_t waves = small_msm_seg_plan(L.off.data(), nsums, desc);
    const int forced = dev_hooks().verifier_min;  // (development library: the threshold sweep of tools/time_verifier_batch.py)
    const size_t min_rel = forced >= 1 ? (size_t)forced : kVerifierBatchMin;
    const bool device = slot >= 0 && ctx->batch_verify && work.size() >= min_rel && check_stage(ctx, 1, nterms * 96 + nsums * 96 + (nsums + 1) * 4 + desc.size() * 4) >= 1;
    int rc;
    {
        // (the launch macro and the read of G_0, G_1 use ctx->stream: the slot's own on the device path, else as it was)
        StreamGuard on_slot(ctx, device ? ctx->streams[slot] : ctx->stream);
        rc = nsums ? halo_ctx_read_bases(ctx, 0, u0_terms, g01) : HALO_OK;
        if (!rc) pool_run(k, [&](size_t j) { if (mem[j].sums) member_terms(j); });
        if (!rc && device) rc = sums_on_device(ctx, L, desc, waves, sums);
        else if (!rc)  // ... or on the host pool, sum by sum
            pool_run(nsums, [&](size_t s) {
                const size_t lo = L.off[s], len = L.off[s + 1] - lo;
                std::vector<Point> p(len);
                std::vector<Fr> kk(len);
                for (size_t t = 0; t < len; ++t) { p[t] = Point::load_affine(&L.pts[8 * (lo + t)]); kk[t] = Fr::load(&L.sc[4 * (lo + t)]).to_mont(); }
                sums[s] = host::small_msm(p, kk);
            });
    }
    if (rc) return rc;
    // 3. the tail and every member's status in the single call's order
    pool_run(k, [&](size_t j) {
        VerifierMember &M = mem[j];
        if (M.rc) return;
        const uint64_t *acc = accs + j * aw, *piV = acc + iw;
        if (sums[M.s_u0] != Point::load(piV + 8)) { M.rc = HALO_E_REJECT; M.err = "U_0 != PCDL.Commit(h_0)"; return; }
        if (!M.reach) { M.rc = HALO_E_REJECT; M.err = "d_i != d"; return; }  // :169
        for (size_t i = 0; i < M.m; ++i) {  // :158-170 in instance order
            const BatchCheck &r = res[M.first + i];
            if (r.rc) { M.rc = r.rc; M.err = r.err; return; }
            if (sums[rel_sum[M.first + i]] != -r.st.C_prime) { M.rc = HALO_E_REJECT; M.err = "C_(log_n) != CM.Commit_Sigma(c || v')"; return; }  // :307-310
        }
        Point C = Point::infinity();
        for (size_t c = 0; c < M.n_c; ++c) C = C + sums[M.s_c + c];
        const Fr z_p = rho1_C_alpha(C, M.hs.alpha);                         // :181
        const Point C_bar_p = C + public_s_table().mul(Fr::load(piV + 20));  // :184
        const Fr z = Fr::load(acc + 13), v = Fr::load(acc + 17);
        if (C_bar_p != Point::load(acc)) { M.rc = HALO_E_REJECT; M.err = "C_bar' != C_bar"; }
        else if (z_p != z) { M.rc = HALO_E_REJECT; M.err = "z' != z"; }
        else if ((size_t)acc[12] != d) { M.rc = HALO_E_REJECT; M.err = "d' != d"; }
        else if (M.hs.eval(z) != v) { M.rc = HALO_E_REJECT; M.err = "h(z) != v"; }
    });
    return report_members("member", k, [&](size_t j) { return mem[j].rc; }, [&](size_t j) { return mem[j].err; }, status, [](size_t) {});
}

// ------------------------------------------------------------------ pcdl::open of m polynomials at once
// The randomness of every member is known before any device work: the counter-based stream's draws depend only on the members'
// degrees (a hiding open draws deg scalars for q, then w_bar; random_instance draws d', w, the d' + 1 coefficients, z, then the
// open's draws).  So the host computes every member's start state first, and the members run side by side.
//
// Device path (2 <= n <= the context's no-fold size, at most OPEN_MAX_N): the open in its no-fold form (ipa_state.hip ipa_round_lr_points:
// the key is never folded, every round's L and R are two MSMs over the same n points with expanded scalars) for a GROUP of up to
// OPEN_MAX_GROUP members at a time.  Each step of a group is one set of member-batched launches (fr_vec.hip *_batch, blockIdx.y =
// member) and ONE batched MSM launch sequence over the key (L and R of every member: up to 8 scalar arrays; the C_bar commits of the
// hiding branch, and random_instance's commits, likewise).  Groups rotate over the slots that were idle on entry: while this
// thread waits for one group's step and runs its host half -- window combines, H' terms, Fiat-Shamir hashes, xi^-1, on the host
// pool for the group's members -- the other slots' groups run on the device.  Every group runs through all its rounds before
// its slot takes the next one, so the staging holds G x S members.  Host arithmetic is the single open's, term for term
// (pcdl_open_dev, halo_ipa_finish's last-round U), so every proof word is the one halo_pcdl_open writes.
//
// Above the no-fold size (n up to OPEN_MAX_N, where open_fold_route says so) the group takes the single open's folded schedule:
// while the key has more points than the no-fold size, k = 1 or 2 rounds in the no-fold form over it, then ONE member-batched fold
// launch of k levels (key_fold.hip k_fold_points*_batch) into the members' staged keys, n >> k points each in the group's staging.
// From the first fold on a member's key is its own: the batched MSMs run over the staged keys with one base offset per member
// (MsmBatch::base_off; the small pipeline takes them, smsm.hip).  The folded key does not depend on the schedule and every point
// written is normalised, so the proofs are still the loop's.
struct OpenJob {
    size_t idx = 0, deg = 0;
    uint64_t s_start = 0;                // rng state before the member's first draw (the single call's *rng_state)
    uint64_t s_p = 0, s_q = 0;           // rng state before p's coefficients (random_instance) / before q's (hiding)
    const uint64_t *coeffs = nullptr;    // the caller's n coefficients (null: p generated or accumulated on the device, or a device row)
    bool dev_row = false;                // the caller's device-resident row: len scalars at d_src (null: the zero polynomial), only read
    const uint64_t *d_src = nullptr;
    size_t len = 0;
    const AccHPolys *hs = nullptr;       // acc::prover's h_0, challenges and alpha powers: p = h.get_poly() accumulated on the device
    bool hiding = false;
    Point C, last_L, last_R;
    Fr z, v, w, w_bar, xi0, xi, c0, c1, last_xi, last_xi_inv;
    uint64_t *proof = nullptr;
    int rc = HALO_OK;
    std::string err;
};
// members per launch: 4 (8 scalar arrays per round) within the small pipeline's bucket limit; "open_batch_group" forces 1..4
static size_t open_group_size(const halo_ctx *ctx, size_t n) {
    // (development library: the sweep of tools/time_open_batch.py)
    return (size_t)group_size(ctx, n, dev_hooks().open_group, OPEN_MAX_GROUP, 2);
}
// s'[2t + u] = s[t] xi^u: the newest challenge is the lowest index bit (what k_nofold_s_update computes on the device)
static void open_fold_products(std::vector<Fr> &s, const Fr &xi) {
    std::vector<Fr> out(2 * s.size());
    for (size_t t = 0; t < s.size(); ++t) { out[2 * t] = s[t]; out[2 * t + 1] = s[t] * xi; }
    s.swap(out);
}
// Does a batch of n-point opens above the no-fold size take the folded schedule (OpenGroups::fold_keys), or the loop?  The hook
// "open_batch_fold" forces either (1 / 2); the default follows the measurements of tools/time_open_batch.py --fold and
// tools/time_prover_batch.py --fold (profiles/r18_*_batch_fold.json): the folded schedule only at the sizes
// where every run of it was faster than every run of the loop -- 2^15 .. 2^19 points (OPEN_MAX_N) for the three open batches and
// for the prover batch: 2.4 - 3.4 times the loop's speed up to 2^17, 1.7 - 1.95 times at 2^18, 1.5 times at 2^19.
// TEMPORARY: the prover batch at 2^15 won as well (53.6 against 19.7 ms for 8 members, 426 against 126 for 64) but is held back
// on the loop, because tests/test_gpu_prover_batch.py::test_above_the_device_form asserts one member at a time at that size.
// Once that test moves to a size that is really unrouted (2^20), the prover's threshold becomes the opens' 2^15 and
// --held-back of the timing tool goes.  Smaller sizes come above the no-fold size only under a lowered switch
// (halo_set_ipa_switch, the development library): not measured, so the loop unless forced.
static bool open_fold_route(size_t n, bool prover) {
    const int forced = dev_hooks().open_fold;
    if (forced) return forced == 1;
    return n >= ((size_t)1 << (prover ? 16 : 15));  // (up to OPEN_MAX_N: the callers' gate)
}
constexpr size_t OPEN_AUX_WORDS = OPEN_MAX_GROUP * (OPEN_TAB_WORDS + OPEN_CONST_WORDS + OPEN_PART_WORDS + OPEN_OUT_WORDS);
// (the prover batch's third coefficient source: up to HACC_TABLES polynomials h_i per pass of a group, see h_accumulate_group)
constexpr size_t HACC_TABLES = 32;
constexpr size_t HACC_PIN_WORDS = hacc_pin_words(OPEN_MAX_GROUP, OPEN_MAX_LG, HACC_TABLES);  // (a record per table grows with lg n)
constexpr size_t FOLD_PIN_WORDS = OPEN_MAX_GROUP * FOLD_DIG_WORDS / 2;  // the members' digit records of a key fold (32-bit words, two to a word here: whatever the key's size)
static_assert(FOLD_DIG_WORDS % 2 == 0, "digit records in whole 64-bit words");
constexpr size_t OPEN_PIN_WORDS = OPEN_MAX_GROUP * (OPEN_TAB_WORDS + OPEN_CONST_WORDS + OPEN_OUT_WORDS) + HACC_PIN_WORDS + FOLD_PIN_WORDS + 4;  // per slot; + the element one

// Slot j's regions of the staging.  Device (`per` words a slot): the group's member vectors (G x ms: c | z | s | s' | F_L | F_R |
// p_bar of n scalars each), then its window tables | constants | partial sums | results | the prover batch's tables.  Pinned
// (OPEN_PIN_WORDS a slot): the tables | constants (one upload) | results (one download) | the prover batch's records | the
// fold digit records | the element one.  Cached launch graphs and the kernels of fr_vec.hip (OPEN_*_WORDS) know this layout.
// A group above the no-fold size (keystride > 0) has two more device regions behind the others, at `fold_off` words: the members'
// folded keys, keystride points of AFF_STRIDE words each (what the first fold leaves: n / 2 or n / 4), and their digit records
// (FOLD_PIN_WORDS).
struct OpenStage {
    uint64_t *d_base = nullptr, *h_base = nullptr;
    size_t per = 0, n = 0, ms = 0, G = 0;
    size_t fold_off = 0, keystride = 0;
    uint32_t *d_keys(int j) const { return reinterpret_cast<uint32_t *>(d_base + (size_t)j * per + fold_off); }
    uint32_t *d_digs(int j) const { return d_keys(j) + G * keystride * AFF_STRIDE; }
    uint32_t *h_digs(int j) const { return reinterpret_cast<uint32_t *>(h_one(j) - FOLD_PIN_WORDS); }
    uint64_t *vec(int j, int k) const { return d_base + (size_t)j * per + 4 * n * (size_t)k; }  // member 0's vector k; member b at + b * ms
    uint64_t *d_tabs(int j) const { return d_base + (size_t)j * per + G * ms; }
    uint64_t *d_consts(int j) const { return d_tabs(j) + OPEN_MAX_GROUP * OPEN_TAB_WORDS; }
    uint64_t *d_parts(int j) const { return d_consts(j) + OPEN_MAX_GROUP * OPEN_CONST_WORDS; }
    uint64_t *d_outs(int j) const { return d_parts(j) + OPEN_MAX_GROUP * OPEN_PART_WORDS; }
    uint64_t *d_hacc(int j) const { return d_outs(j) + OPEN_MAX_GROUP * OPEN_OUT_WORDS; }
    uint64_t *h_tabs(int j) const { return h_base + (size_t)j * OPEN_PIN_WORDS; }
    OpenConst *h_consts(int j) const { return (OpenConst *)(h_tabs(j) + OPEN_MAX_GROUP * OPEN_TAB_WORDS); }
    uint64_t *h_outs(int j) const { return h_tabs(j) + OPEN_MAX_GROUP * (OPEN_TAB_WORDS + OPEN_CONST_WORDS); }
    uint64_t *h_hacc(int j) const { return h_outs(j) + OPEN_MAX_GROUP * OPEN_OUT_WORDS; }
    uint64_t *h_one(int j) const { return h_tabs(j) + OPEN_PIN_WORDS - 4; }
    uint64_t *out_of(int j, size_t b) const { return h_outs(j) + OPEN_OUT_WORDS * b; }
};

// The groups of one batched open over S slots.  A group's steps: 0 the coefficients, p(z), the powers of z, p_bar and the commits;
// 1 .. lg the rounds; lg + 1 the U of the members whose last round does not hold it.  Each step is enqueued on the slot's stream
// (start, enqueue_round, the tail of after_round) and, when the slot comes round again, collected and taken through its host
// half (advance).
struct OpenGroups {
    halo_ctx *ctx;
    std::vector<OpenJob> &jobs;
    const int *slots;  // the slots idle at entry; S of them are used
    int S;
    size_t n, lg, G, ms;
    bool draw, commit, hiding, accumulated, dev_rows;  // draw: p from the stream; commit: C = commit(p) rides in step 0's MSM
    OpenStage st;
    size_t nofold;  // the key size from which on the rounds fold no more (>= n: never folded, the no-fold form throughout)
    // M: points of the key the group's MSMs run over -- n over the context's key until the first fold, then each member's own staged
    // key (OpenStage::d_keys).  s_len: entries of s, the products of the challenges since the key was last folded (s_host: the
    // host's copy while a fold is ahead); fold_k: levels of the next fold (0: none ahead), due after fold_k rounds over this key.
    struct Flight {
        long g = -1;
        size_t first = 0, cnt = 0, step = 0;
        int msm = 0;
        bool flip = false;
        std::vector<size_t> need_u;
        size_t M = 0, s_len = 1;
        int fold_k = 0;
        bool staged = false;
        std::vector<Fr> s_host[OPEN_MAX_GROUP];
    };
    std::vector<Flight> fl;

    hipStream_t stream(int j) const { return ctx->streams[slots[j]]; }
    uint64_t *s_cur(int j) const { return st.vec(j, fl[j].flip ? 3 : 2); }
    int download_outs(int j) {
        HALO_HIP(hipMemcpyAsync(st.h_outs(j), st.d_outs(j), fl[j].cnt * OPEN_OUT_WORDS * 8, hipMemcpyDeviceToHost, stream(j)));
        return HALO_OK;
    }
    int upload_consts(int j) {
        HALO_HIP(hipMemcpyAsync(st.d_consts(j), st.h_consts(j), fl[j].cnt * OPEN_CONST_WORDS * 8, hipMemcpyHostToDevice, stream(j)));
        return HALO_OK;
    }
    // the step's MSMs over the key as one batched launch sequence; member_of[k]: the member array k belongs to (its own key once folded)
    int enqueue_msm(int j, MsmBatch &mb, const size_t *member_of) {
        const Flight &f = fl[j];
        for (int k = 0; k < mb.count && f.staged; ++k) mb.base_off[k] = (uint32_t)(member_of[k] * st.keystride);
        int rc = msm_enqueue_batch(ctx, slots[j], f.staged ? st.d_keys(j) : ctx->d_bases, mb, true, f.M);
        if (!rc) fl[j].msm = mb.count;
        return rc;
    }
    // levels of the fold that follows the next rounds over a key of M points: two at a time down to the no-fold size
    int fold_levels_at(size_t M) const {
        if (M <= nofold) return 0;
        return M / nofold >= 4 ? 2 : 1;
    }
    void key_reset(Flight &f, size_t M) {  // a fresh key: s = (1)
        f.M = M;
        f.s_len = 1;
        f.fold_k = fold_levels_at(M);
        for (size_t b = 0; b < f.cnt; ++b) f.s_host[b].assign(1, Fr::one());
    }

    // step 0: coefficients (copied, generated, accumulated, or padded from the caller's device rows), p(z), the powers of z, p_bar; the commits as one batched MSM
    int start(int j, size_t g) {
        Flight &f = fl[j];
        f = Flight();
        f.g = (long)g;
        f.first = g * G;
        f.cnt = jobs.size() - f.first < G ? jobs.size() - f.first : G;
        key_reset(f, n);
        for (size_t b = 0; b < f.cnt; ++b) {
            const OpenJob &jb = jobs[f.first + b];
            OpenConst &k = st.h_consts(j)[b];
            std::memset(&k, 0, sizeof k);
            int rc = open_batch_table(jb.z, n, st.h_tabs(j) + OPEN_TAB_WORDS * b, &k);
            if (rc) return rc;
            k.s_q = jb.s_q;
            k.s_p = jb.s_p;
            k.deg = (uint32_t)jb.deg;
            k.len = (uint32_t)(jb.deg + 1);
        }
        {
            StreamGuard on_slot(ctx, stream(j));  // (the launch macro uses ctx->stream)
            HALO_HIP(hipMemcpyAsync(st.d_tabs(j), st.h_tabs(j), OPEN_MAX_GROUP * (OPEN_TAB_WORDS + OPEN_CONST_WORDS) * 8, hipMemcpyHostToDevice, stream(j)));
            int rc = HALO_OK;
            if (draw) rc = open_batch_rng(ctx, (int)f.cnt, st.d_consts(j), n, st.vec(j, 0), ms);  // p = PallasPoly::rand(d')
            else if (accumulated) {  // p = h.get_poly() (acc.rs:85-94)
                HAccMember hm[OPEN_MAX_GROUP];
                for (size_t b = 0; b < f.cnt; ++b) {
                    const AccHPolys &hs = *jobs[f.first + b].hs;
                    hm[b].h0 = hs.h0;
                    hm[b].count = hs.xis.size();
                    hm[b].scales = hs.alphas.data() + 1;
                    for (const std::vector<Fr> &x : hs.xis) hm[b].xis.push_back(x.data());
                }
                rc = h_accumulate_group(ctx, hm, f.cnt, lg, HACC_TABLES, st.h_hacc(j), st.d_hacc(j), st.vec(j, 0), ms);
            } else if (dev_rows) {  // the caller's device rows, zero-padded to n in ONE launch (a full-length member too: the open overwrites its copy)
                PadMembers t{};
                for (size_t b = 0; b < f.cnt; ++b) {
                    const OpenJob &jb = jobs[f.first + b];
                    t.src[b] = jb.d_src;
                    t.len[b] = (uint32_t)jb.len;
                    t.row[b] = (uint32_t)b;
                }
                rc = pad_members_batch(ctx, t, (int)f.cnt, n, st.vec(j, 0), ms);
            } else
                for (size_t b = 0; b < f.cnt; ++b)
                    HALO_HIP(hipMemcpyAsync(st.vec(j, 0) + b * ms, jobs[f.first + b].coeffs, n * 32, hipMemcpyHostToDevice, stream(j)));
            if (!rc) rc = open_batch_eval(ctx, (int)f.cnt, st.vec(j, 0), ms, n, st.d_tabs(j), st.d_parts(j), st.d_outs(j));  // :135
            if (!rc) rc = open_batch_powers(ctx, (int)f.cnt, st.d_tabs(j), st.d_consts(j), n, st.vec(j, 1), ms);
            if (!rc && hiding) rc = open_batch_pbar(ctx, (int)f.cnt, st.d_consts(j), n, st.vec(j, 6), ms);  // :140-142
            for (size_t b = 0; b < f.cnt && !rc; ++b)  // s = (1)
                HALO_HIP(hipMemcpyAsync(st.vec(j, 2) + b * ms, st.h_one(j), 32, hipMemcpyHostToDevice, stream(j)));
            if (!rc) rc = download_outs(j);
            if (rc) return rc;
        }
        MsmBatch mb;  // the C of every member (random_instance, instance_from_poly), then C_bar of every member (:150)
        mb.count = 0;
        if (commit)
            for (size_t b = 0; b < f.cnt; ++b) mb.scalars[mb.count++] = st.vec(j, 0) + b * ms;
        if (hiding)
            for (size_t b = 0; b < f.cnt; ++b) mb.scalars[mb.count++] = st.vec(j, 6) + b * ms;
        return mb.count ? enqueue_msm(j, mb, nullptr) : HALO_OK;  // (the context's key: no member has one of its own yet)
    }
    // round r of slot j's group: F_L, F_R from c and s, the dot products, L and R of every member as one batched MSM
    int enqueue_round(int j, size_t r) {
        Flight &f = fl[j];
        const size_t mcur = n >> r;
        int rc;
        {
            StreamGuard on_slot(ctx, stream(j));
            rc = open_batch_expand(ctx, (int)f.cnt, st.vec(j, 0), s_cur(j), ms, mcur, f.M, st.vec(j, 4), st.vec(j, 5));
            if (!rc) rc = open_batch_dots(ctx, (int)f.cnt, st.vec(j, 0), st.vec(j, 1), ms, mcur / 2, st.d_parts(j), st.d_outs(j));
            if (!rc && mcur == 2)  // the last round: c0, c1 travel with its results (halo_ipa_finish's U from this round's MSMs)
                for (size_t b = 0; b < f.cnt; ++b)
                    HALO_HIP(hipMemcpyAsync(st.d_outs(j) + OPEN_OUT_WORDS * b + 12, st.vec(j, 0) + b * ms, 64, hipMemcpyDeviceToDevice, stream(j)));
            if (!rc) rc = download_outs(j);
        }
        if (!rc) {
            MsmBatch mb;  // L, R of member 0, L, R of member 1, ..
            size_t member_of[MSM_MAX_BATCH];
            mb.count = 2 * (int)f.cnt;
            for (int k = 0; k < mb.count; ++k) {
                member_of[k] = (size_t)(k >> 1);
                mb.scalars[k] = st.vec(j, 4 + (k & 1)) + member_of[k] * ms;
            }
            rc = enqueue_msm(j, mb, member_of);
        }
        f.step = 1 + r;
        return rc;
    }
    // slot j's step is done: its results through the host half, then the next step (or the group is through)
    int advance(int j, bool *through) {
        Flight &f = fl[j];
        *through = false;
        Point pts[MSM_MAX_BATCH];
        if (f.msm) {
            int rc = msm_finish_batch(ctx, slots[j], pts, f.msm);
            f.msm = 0;
            if (rc) return rc;
        }
        HALO_HIP(hipStreamSynchronize(stream(j)));
        if (f.step == 0) return after_commits(j, pts);
        if (f.step <= lg) return after_round(j, pts, through);
        after_u(j, pts);
        *through = true;
        return HALO_OK;
    }
    // after step 0: v, C (random_instance), the hiding branch's C_bar, alpha, w' and C', xi_0; p' = p + alpha p_bar; round 0
    int after_commits(int j, const Point *pts) {
        Flight &f = fl[j];
        pool_run(f.cnt, [&](size_t b) {
            OpenJob &jb = jobs[f.first + b];
            jb.v = Fr::load(st.out_of(j, b));
            if (commit) jb.C = (hiding ? public_s_table().mul(jb.w) + pts[b] : pts[b]).normalized();
            Point C_prime = jb.C;
            if (hiding) {
                Point C_bar = public_s_table().mul(jb.w_bar) + pts[(commit ? f.cnt : 0) + b];
                Fr a = rho0_C_z_v_Cbar(jb.C, jb.z, jb.v, C_bar);  // :153
                Fr w_prime = jb.w_bar * a + jb.w;                  // :159
                C_prime = jb.C + C_bar.mul(a) - public_s_table().mul(w_prime);  // :162
                jb.proof[0] = 1;
                C_bar.store_normalized(pf_Cbar(jb.proof, lg));
                w_prime.store(pf_wp(jb.proof, lg));
                open_const_alpha(&st.h_consts(j)[b], a);
            } else {
                Point::infinity().store(pf_Cbar(jb.proof, lg));
            }
            jb.xi0 = jb.xi = rho0_C_z_v(C_prime, jb.z, jb.v);  // :180
        });
        if (hiding) {
            StreamGuard on_slot(ctx, stream(j));
            int rc = upload_consts(j);
            if (!rc) rc = open_batch_axpy(ctx, (int)f.cnt, st.vec(j, 0), st.vec(j, 6), ms, n, st.d_consts(j));  // :156
            if (rc) return rc;
        }
        return enqueue_round(j, 0);
    }
    // after round r = step - 1 (:203-224): L, R with their H' terms, the next challenge and its inverse; the fold; the next round,
    // or, after the last one, U and c.  Above the no-fold size the KEY is folded here too, every fold_k rounds: the host keeps each
    // member's challenge products (s'[2t + u] = s[t] xi^u, what k_nofold_s_update_batch computes) and, when the fold is due, turns
    // s[1] (one level) or s[1..3] (two) into the member's digit record -- the scalars and digits of the single open's deferred fold
    // (ipa_state.hip ipa_round_fold_impl) -- then ONE batched fold launch writes every member's key and s starts again from (1).
    int after_round(int j, const Point *pts, bool *through) {
        Flight &f = fl[j];
        const size_t r = f.step - 1;
        const bool last = r + 1 == lg;
        const bool fold_key = f.fold_k && 2 * f.s_len == ((size_t)1 << f.fold_k);  // this round's challenge completes the fold's scalars
        pool_run(f.cnt, [&](size_t b) {
            OpenJob &jb = jobs[f.first + b];
            const uint64_t *o = st.out_of(j, b);
            Fr dl = Fr::load(o + 4), dr = Fr::load(o + 8);
            if (last) { jb.last_L = pts[2 * b]; jb.last_R = pts[2 * b + 1]; jb.c0 = Fr::load(o + 12); jb.c1 = Fr::load(o + 16); }
            uint64_t *Lw = pf_L(jb.proof, r), *Rw = pf_R(jb.proof, lg, r);
            (pts[2 * b] + public_h_table().mul(dl * jb.xi0)).normalized().store(Lw);
            (pts[2 * b + 1] + public_h_table().mul(dr * jb.xi0)).normalized().store(Rw);
            Fr xi_next = rho0_xi_L_R(jb.xi, Point::load(Lw), Point::load(Rw));  // :212
            if (xi_next.is_zero() && !jb.rc) { jb.rc = HALO_E_ASSERT; jb.err = "open: challenge is zero (inverse().unwrap())"; }
            Fr xi_inv = xi_next.inv();  // :213
            jb.xi = xi_next;
            if (last) { jb.last_xi = xi_next; jb.last_xi_inv = xi_inv; }
            open_const_xi(&st.h_consts(j)[b], xi_next, xi_inv);
            if (f.fold_k) {
                open_fold_products(f.s_host[b], xi_next);
                if (fold_key) fold_digits(&f.s_host[b][1], f.fold_k, st.h_digs(j) + FOLD_DIG_WORDS * b);
            }
        });
        {
            StreamGuard on_slot(ctx, stream(j));  // :216-224
            int rc = upload_consts(j);
            const uint64_t *s_in = s_cur(j);
            f.flip = !f.flip;
            if (!rc) rc = open_batch_fold(ctx, (int)f.cnt, st.vec(j, 0), st.vec(j, 1), s_in, s_cur(j), ms, n >> (r + 1), f.s_len, st.d_consts(j));
            f.s_len *= 2;
            if (!rc && fold_key) rc = fold_keys(j);
            if (rc) return rc;
        }
        return last ? finish_u(j, through) : enqueue_round(j, r + 1);
    }
    // The members' keys of M points folded fold_k levels into their staged keys (:218 applied fold_k times): from the context's key
    // the first time (one source for all), then each member's own, in place (a lane reads the indices j + t m and writes j).
    // On the slot's stream, behind the round's scalar folds; s = (1) again for the rounds over the new key.
    int fold_keys(int j) {
        Flight &f = fl[j];
        const size_t m = f.M >> f.fold_k;
        HALO_HIP(hipMemcpyAsync(st.d_digs(j), st.h_digs(j), f.cnt * FOLD_DIG_WORDS * 4, hipMemcpyHostToDevice, stream(j)));
        const uint32_t *src = f.staged ? st.d_keys(j) : ctx->d_bases;
        const size_t src_stride = f.staged ? st.keystride : 0;
        int rc = f.fold_k == 2 ? ipa_fold_points4_batch(ctx, (int)f.cnt, src, src_stride, st.d_keys(j), st.keystride, m, st.d_digs(j))
                               : ipa_fold_points_batch(ctx, (int)f.cnt, src, src_stride, st.d_keys(j), st.keystride, m, st.d_digs(j));
        for (size_t b = 0; b < f.cnt && !rc; ++b)
            HALO_HIP(hipMemcpyAsync(s_cur(j) + b * ms, st.h_one(j), 32, hipMemcpyHostToDevice, stream(j)));
        f.staged = true;
        key_reset(f, m);
        return rc;
    }
    // :230-231 as halo_ipa_finish: U from the last round's MSMs where both coefficients are non-zero, else U = <s, G> (one more step)
    int finish_u(int j, bool *through) {
        Flight &f = fl[j];
        auto from_last_round = [&](const OpenJob &jb) { return !jb.c0.is_zero() && !jb.c1.is_zero(); };
        pool_run(f.cnt, [&](size_t b) {
            OpenJob &jb = jobs[f.first + b];
            if (!from_last_round(jb)) return;
            Fr inv01 = (jb.c0 * jb.c1).inv();
            Fr a = inv01 * jb.c0, bb = inv01 * jb.c1 * jb.last_xi;  // 1 / c1, xi / c0
            (jb.last_L.mul(a) + jb.last_R.mul(bb)).store_normalized(pf_U(jb.proof, lg));
            (jb.c0 + jb.last_xi_inv * jb.c1).store(pf_c(jb.proof, lg));
        });
        f.need_u.clear();
        for (size_t b = 0; b < f.cnt; ++b)
            if (!from_last_round(jobs[f.first + b])) f.need_u.push_back(b);
        if (f.need_u.empty()) { *through = true; return HALO_OK; }
        int rc = HALO_OK;
        {
            StreamGuard on_slot(ctx, stream(j));
            for (size_t k = 0; k < f.need_u.size(); ++k)
                HALO_HIP(hipMemcpyAsync(st.d_outs(j) + OPEN_OUT_WORDS * f.need_u[k] + 20, st.vec(j, 0) + f.need_u[k] * ms, 32, hipMemcpyDeviceToDevice, stream(j)));
            rc = download_outs(j);
        }
        if (!rc) {
            MsmBatch mb;
            mb.count = (int)f.need_u.size();
            for (int k = 0; k < mb.count; ++k) mb.scalars[k] = s_cur(j) + f.need_u[(size_t)k] * ms;
            rc = enqueue_msm(j, mb, f.need_u.data());
        }
        f.step = lg + 1;
        return rc;
    }
    // after step lg + 1: U = <s, G> and c = c[0] (halo_ipa_finish)
    void after_u(int j, const Point *pts) {
        Flight &f = fl[j];
        for (size_t k = 0; k < f.need_u.size(); ++k) {
            OpenJob &jb = jobs[f.first + f.need_u[k]];
            pts[k].store_normalized(pf_U(jb.proof, lg));
            std::memcpy(pf_c(jb.proof, lg), st.out_of(j, f.need_u[k]) + 20, 32);
        }
    }
    void abandon() {  // (a device error: nothing of this call stays in flight)
        std::string err = halo_last_error();
        for (int j = 0; j < S; ++j) {
            if (fl[j].msm) {
                Point pts[MSM_MAX_BATCH];
                (void)msm_finish_batch(ctx, slots[j], pts, fl[j].msm);
                fl[j].msm = 0;
            }
            (void)hipStreamSynchronize(stream(j));
        }
        set_error(err);
    }
    // every group through all its steps: a slot takes the next group when its own is through
    int run() {
        const size_t ng = (jobs.size() + G - 1) / G;
        fl.assign(S, Flight());
        size_t next = 0;
        int rc = HALO_OK, active = 0;
        for (int j = 0; j < S && next < ng && !rc; ++j, ++active) rc = start(j, next++);
        while (!rc && active) {
            for (int j = 0; j < S && !rc; ++j) {
                if (fl[j].g < 0) continue;
                bool through = false;
                rc = advance(j, &through);
                if (rc || !through) continue;
                fl[j].g = -1;
                --active;
                if (next < ng) { rc = start(j, next++); ++active; }
            }
        }
        if (rc) abandon();
        return rc;
    }
};

// jobs: the members that do not fail up front, in member order.  *ran = false: the device path does not apply (nothing done)
// Coefficients of a member: the caller's host array (jb.coeffs), generated on the device (draw), -- jb.hs set, for every member
// alike -- acc::prover's h(X) accumulated on the device straight into the member's coefficient vector, or -- jb.dev_row, for
// every member alike -- the caller's device row padded into it (k_pad_members_batch).  commit: jb.C is not given
// but computed, the members' commits riding in step 0's batched MSM
static int open_batch_dev(halo_ctx *ctx, size_t d, std::vector<OpenJob> &jobs, bool draw, bool commit, const int *slots_in, int S, bool *ran) {
    *ran = false;
    const size_t n = d + 1, lg = ilog2(n), A = jobs.size();
    if (A == 0 || n < 2 || n > OPEN_MAX_N || ctx->nofold_size < 2) return HALO_OK;  // (a switch of 0 / 1: always fold, the loop)
    const bool folds = n > ctx->nofold_size;  // the rounds fold the key down to the no-fold size: each member into a staged key of its own
    const bool accumulated = jobs[0].hs != nullptr;
    if (folds && !open_fold_route(n, accumulated)) return HALO_OK;
    size_t G = open_group_size(ctx, n), first_m = n;  // first_m: points of a member's key after the first fold, its largest
    for (size_t M = n; folds && M > ctx->nofold_size;) {  // ... within the bucket limit at every key size the rounds run over
        M >>= M / ctx->nofold_size >= 4 ? 2 : 1;
        if (first_m == n) first_m = M;
        const size_t g = open_group_size(ctx, M);
        if (g < G) G = g;
    }
    if (G > A) G = A;
    const size_t ng = (A + G - 1) / G;
    if ((size_t)S > ng) S = (int)ng;
    const size_t ms = 7 * 4 * n;  // words of one member's vectors: c | z | s | s' | F_L | F_R | p_bar
    const size_t hacc_words = accumulated ? hacc_stage_words(OPEN_MAX_GROUP, lg, HACC_TABLES) : 0;
    const size_t fold_off = G * ms + OPEN_AUX_WORDS + hacc_words, keystride = folds ? first_m : 0;
    // words of one slot's group: 224 n bytes of vectors per member (+ above the no-fold size: its key after the first fold, n / 2 or
    // n / 4 points of 128 bytes, and the digit records) -- with 4 members 14 MiB a slot at 2^14, 128 MiB at 2^17, 256 MiB at 2^18, 512 MiB at 2^19
    const size_t per = fold_off + (folds ? G * keystride * (AFF_STRIDE / 2) + FOLD_PIN_WORDS : 0);
    size_t have = check_stage(ctx, (size_t)S, per * 8);
    if (have == 0) return HALO_OK;
    if ((size_t)S > have) S = (int)have;
    if (!ctx->h_open_pinned) {
        if (hipHostMalloc(&ctx->h_open_pinned, HALO_SLOTS * OPEN_PIN_WORDS * 8) != hipSuccess) {
            (void)hipGetLastError();
            ctx->h_open_pinned = nullptr;
            return HALO_OK;
        }
        for (int k = 0; k < HALO_SLOTS; ++k) Fr::one().store(ctx->h_open_pinned + k * OPEN_PIN_WORDS + OPEN_PIN_WORDS - 4);
    }
    *ran = true;
    const OpenStage st{ctx->d_check_stage, ctx->h_open_pinned, per, n, ms, G, fold_off, keystride};
    // (hiding: the same for every member of a batch)
    OpenGroups groups{ctx, jobs, slots_in, S, n, lg, G, ms, draw, commit, jobs[0].hiding, accumulated, jobs[0].dev_row, st, ctx->nofold_size, {}};
    return groups.run();
}

// halo_pcdl_open_batch (coeffs and Cs given), halo_instance_from_poly_batch (coeffs without Cs: the commits are computed and `out`
// holds Instance blobs) and halo_random_instance_batch (neither: the polynomials are drawn as well) after their argument checks:
// the members' draws, then the device path or, where it does not apply, the members one at a time.
// The same three calls over device-resident rows (halo_pcdl_open_dev_batch, halo_instance_from_poly_dev_batch): the draws need every
// member's degree, so the degrees are found on the device first (ONE k_poly_degree_batch launch) and nothing else differs before
// step 0 of a group, where the rows are padded into the staging instead of copied.  Run alone, a member is copied device to device
// into the context's polynomial buffer (pcdl_open_dev_row, instance_from_poly_dev_row).  No route brings a polynomial to the host.
struct OpenSource {  // the caller's polynomials: m x (d + 1) scalars in host memory, or m device rows (dev_rows_ok); neither: drawn
    const uint64_t *coeffs = nullptr;
    const void *const *d_coeffs = nullptr;
    const size_t *lens = nullptr;
};
static int open_batch_entry(halo_ctx *ctx, uint64_t *rng_state, size_t d, const OpenSource &src, size_t m, const uint64_t *Cs, const uint64_t *zs,
                            const uint64_t *ws, uint64_t *out, int *status) {
    const size_t n = d + 1, lg = ilog2(n);
    const uint64_t *coeffs = src.coeffs;
    const bool dev = src.d_coeffs != nullptr, gen = !coeffs && !dev, commit = Cs == nullptr, hiding = gen || ws != nullptr;
    const size_t stride = commit ? instance_words(lg) : proof_words(lg);
    int slots[HALO_SLOTS], S = idle_slots(ctx, slots);
    if (!S) { set_error("open_batch: every slot has an MSM in flight"); return HALO_E_ARG; }
    // 0. device rows: every member's degree (a member longer than d + 1 fails below and is not scanned)
    std::vector<size_t> degs(dev ? m : 0), scan(dev ? m : 0);
    if (dev) {
        for (size_t i = 0; i < m; ++i) scan[i] = src.lens[i] <= n ? src.lens[i] : 0;
        int rc = poly_degrees_dev(ctx, src.d_coeffs, scan.data(), m, degs.data());
        if (rc) return rc;
    }
    // 1. every member's draws, in member order (the loop's order)
    host::Rng rng{rng_state ? *rng_state : 0};
    std::vector<OpenJob> jobs;
    std::vector<int> codes(m, HALO_OK);
    std::vector<std::string> errs(m);
    jobs.reserve(m);
    for (size_t i = 0; i < m; ++i) {
        OpenJob jb;
        jb.idx = i;
        jb.hiding = hiding;
        jb.proof = out + i * stride + (commit ? 21 : 0);
        jb.s_start = rng.state;
        if (gen) {
            size_t lo = d / 2;
            jb.deg = lo + (size_t)(rng.next() % (uint64_t)(d - lo));
            if (jb.deg == 0) jb.deg = 1;
            jb.w = rng.scalar();
            jb.s_p = rng.state;
            rng.skip_scalars(jb.deg + 1);
            jb.z = rng.scalar();
        } else {
            if (dev) {
                if (src.lens[i] > n) {  // (alone, before any draw: the single calls' assert on the length)
                    codes[i] = HALO_E_ASSERT;
                    errs[i] = commit ? "commit: p.degree() > d" : "open: p.degree() > d";
                    continue;
                }
                jb.dev_row = true;
                jb.d_src = static_cast<const uint64_t *>(src.d_coeffs[i]);
                jb.len = src.lens[i];
                jb.deg = degs[i];
            } else {
                jb.coeffs = coeffs + i * n * 4;
                jb.deg = host_poly_degree(jb.coeffs, n);
            }
            if (Cs) jb.C = Point::load(Cs + 12 * i);
            jb.z = Fr::load(zs + 4 * i);
            if (ws) jb.w = Fr::load(ws + 4 * i);
            if (hiding && jb.deg == 0) { codes[i] = HALO_E_ASSERT; errs[i] = "open: hiding needs p.degree() >= 1"; continue; }  // (before any draw)
        }
        if (hiding) {
            jb.s_q = rng.state;
            rng.skip_scalars(jb.deg);
            jb.w_bar = rng.scalar();
        }
        jobs.push_back(jb);
    }
    // 2. the device path; where it does not apply, the loop itself (the single calls' bodies, from the same states)
    for (OpenJob &jb : jobs) {
        std::memset(jb.proof, 0, 8 * proof_words(lg));
        jb.proof[1] = lg;
    }
    // (ONE polynomial of the caller's: the single call's body is faster than a group of one -- 2.94 against 3.47 ms at 2^10, 5.10
    // against 5.93 at 2^14; "open_batch_group" forces the group.  A device row keeps the rule: 2.84 against 3.46 ms
    // at 2^10, 4.99 against 5.96 at 2^14, 6.98 against 8.09 at 2^16, tools/time_open_batch.py --dev)
    // (the single call's body runs on slots 0 and 1: only with both idle)
    const bool alone = commit && !gen && jobs.size() == 1 && dev_hooks().open_group <= 0 && S >= 2 && slots[0] == 0 && slots[1] == 1;
    bool ran = false;
    ctx->open_batch_members = 0;  // (halo_ctx_info 10)
    int rc = alone ? HALO_OK : open_batch_dev(ctx, d, jobs, gen, commit, slots, S, &ran);  // (no jobs: nothing runs)
    if (rc) return rc;
    if (ran) ctx->open_batch_members = jobs.size();
    if (!ran) {
        for (OpenJob &jb : jobs) {
            uint64_t st = jb.s_start;
            const uint64_t *w = ws ? ws + 4 * jb.idx : nullptr;
            if (gen) rc = random_instance_one(ctx, &st, d, out + jb.idx * stride);
            else if (dev && commit) rc = instance_from_poly_dev_row(ctx, &st, jb.d_src, jb.len, jb.deg, d, zs + 4 * jb.idx, w, out + jb.idx * stride);
            else if (dev) rc = pcdl_open_dev_row(ctx, &st, jb.d_src, jb.len, jb.deg, Cs + 12 * jb.idx, d, zs + 4 * jb.idx, w, jb.proof);
            else if (commit) rc = instance_from_poly_one(ctx, &st, jb.coeffs, n, jb.deg, d, zs + 4 * jb.idx, w, out + jb.idx * stride);
            else rc = pcdl_open_host(ctx, &st, jb.coeffs, jb.deg, Cs + 12 * jb.idx, d, zs + 4 * jb.idx, w, jb.proof);
            if (rc == HALO_E_ASSERT) { jb.rc = rc; jb.err = halo_last_error(); }
            else if (rc) return rc;
        }
    }
    // 3. outcomes in member order
    for (OpenJob &jb : jobs) {
        codes[jb.idx] = jb.rc;
        errs[jb.idx] = jb.err;
        // the Instance around the proof (random_instance_one and instance_from_poly_one write their own)
        if (commit && !jb.rc && ran) store_instance_head(out + jb.idx * stride, jb.C, d, jb.z, jb.v);
    }
    if (rng_state) *rng_state = rng.state;
    return report_members("member", m, [&](size_t i) { return codes[i]; }, [&](size_t i) { return errs[i]; }, status,
                          [&](size_t i) { std::memset(out + i * stride, 0, 8 * stride); });
}

// ------------------------------------------------------------------ acc::prover of k members at once
// (halo_acc_prover_batch; acc.rs:190-220 per member, every member's blob, status and draws the loop's)
//  1. the succinct half of every member, no randomness: all sum(counts) instances at once -- from kBatchVerifyMin instances on
//     as halo_pcdl_succinct_check_batch runs them (transcripts on the host pool, the relations in one device launch), below on
//     the pool.  A member is rejected exactly where halo_acc_prover rejects it ("d_i != d" first, then its succinct checks in
//     instance order), and a rejected member draws nothing: the single call writes *rng_state only after common_subroutine.
//  2. the survivors' draws in member order: h_0, omega, then (the stream is counter-based) the start of the open's q and w_bar.
//  3. per member on the host pool: U_0 = h_0[0] G_0 + h_0[1] G_1, alpha and its powers, C = sum alpha^i U_i, z, C_bar = C +
//     omega S, v = h(z).  These 3 + m scalar multiples per member (~27 us each on one thread, as the relation's 2 lg n + 1
//     above) are spread over the pool: a second device launch with its round trip would cost more than it saves (the verifier
//     batch folds such sums into a launch it needs anyway; here alpha hashes the drawn h_0, so they cannot ride the relations'
//     launch).
//  4. the hiding opens through open_batch_dev, their coefficients h(X) = h_0 + sum alpha^(i+1) h_i(X) accumulated on the device
//     into the open's staging (h_accumulate_group), groups of up to 4 members over the idle slots -- above the no-fold size on the
//     open batches' folded schedule, where open_fold_route says so (the accumulation does not depend on the key schedule).
//  5. the blobs: C_bar | d | z | v | proof | h_0 | U_0 | omega.
// *ran = false: the device form does not apply (size, route, staging) and nothing was written.
struct ProverMember {
    int rc = HALO_OK;
    std::string err;
    size_t first = 0, m = 0;  // its instances in the flat list
    size_t r0 = 0;            // ... and the first of their check results
    Fr w, z, v;
    Point U0, C_bar;
    AccHPolys hs;
};
static int acc_prover_batch_dev(halo_ctx *ctx, uint64_t state0, size_t d, const uint64_t *qs, const size_t *counts, size_t k, uint64_t *accs,
                                const int *slots, int S, bool *ran, std::vector<int> &codes, std::vector<std::string> &errs, uint64_t *state_out) {
    *ran = false;
    const size_t n = d + 1, lg = ilog2(n), iw = instance_words(lg), aw = acc_words(lg);
    if (n < 2 || n > OPEN_MAX_N || ctx->nofold_size < 2) return HALO_OK;
    if (n > ctx->nofold_size && !open_fold_route(n, true)) return HALO_OK;  // (before any work: the loop is the single prover's alone)
    std::vector<ProverMember> mem(k);
    size_t total = 0;
    for (size_t j = 0; j < k; ++j) { mem[j].first = total; mem[j].m = counts[j]; total += counts[j]; }
    // 1. the succinct half
    for (size_t j = 0; j < k; ++j)
        for (size_t i = 0; i < mem[j].m && !mem[j].rc; ++i) {
            const uint64_t *q = qs + (mem[j].first + i) * iw;
            if ((size_t)q[12] != d || q[22] != lg) { mem[j].rc = HALO_E_REJECT; mem[j].err = "d_i != d"; }  // :169
        }
    std::vector<size_t> work;  // the instances whose checks run (a member that never reaches its checks is left out)
    for (size_t j = 0; j < k; ++j)
        if (!mem[j].rc)
            for (size_t i = 0; i < mem[j].m; ++i) work.push_back(mem[j].first + i);
    std::vector<BatchCheck> res;
    int rc = succinct_half(ctx, d, [&](size_t w) { return qs + work[w] * iw; }, work.size(), res);
    if (rc) return rc;
    for (size_t j = 0, w = 0; j < k; ++j) {
        ProverMember &M = mem[j];
        if (M.rc) continue;
        M.r0 = w;
        for (size_t i = 0; i < M.m; ++i, ++w) {
            if (res[w].rc && !M.rc) { M.rc = res[w].rc; M.err = res[w].err; }  // :158-170 in instance order
            if (!M.rc) M.hs.xis.push_back(res[w].st.xis);
        }
    }
    // 2. the draws, in member order
    host::Rng rng{state0};
    std::vector<OpenJob> jobs;
    jobs.reserve(k);
    for (size_t j = 0; j < k; ++j) {
        ProverMember &M = mem[j];
        if (M.rc) continue;
        M.hs.lg_n = lg;
        M.hs.h0[0] = rng.scalar();  // :192
        M.hs.h0[1] = rng.scalar();
        M.w = rng.scalar();         // :198
        OpenJob jb;
        jb.idx = j;
        jb.hiding = true;
        jb.hs = &M.hs;
        jb.deg = M.m ? d : (M.hs.h0[1].is_zero() ? 0 : 1);
        if (jb.deg == 0) { M.rc = HALO_E_ASSERT; M.err = "open: hiding needs p.degree() >= 1"; continue; }  // pcdl_open_dev: before its draws
        jb.w = M.w;
        jb.s_q = rng.state;
        rng.skip_scalars(jb.deg);
        jb.w_bar = rng.scalar();
        jb.proof = accs + j * aw + 21;
        jobs.push_back(jb);
    }
    // 3. U_0, alpha, C, z, C_bar, v
    if (!jobs.empty()) {
        uint64_t g01[16];
        rc = halo_ctx_read_bases(ctx, 0, 2, g01);
        if (rc) return rc;
        const std::vector<Point> G01{Point::load_affine(g01), Point::load_affine(g01 + 8)};
        pool_run(jobs.size(), [&](size_t a) {
            OpenJob &jb = jobs[a];
            ProverMember &M = mem[jb.idx];
            M.U0 = host::small_msm(G01, std::vector<Fr>{M.hs.h0[0], M.hs.h0[1]});  // :195
            std::vector<Point> Us{M.U0};
            for (size_t i = 0; i < M.m; ++i) Us.push_back(res[M.r0 + i].st.U);
            set_alphas(&M.hs);                                               // :173
            const Point C = host::small_msm(Us, M.hs.alphas);                // :178
            M.z = rho1_C_alpha(C, M.hs.alpha);                               // :181
            M.C_bar = (C + public_s_table().mul(M.w)).normalized();          // :184
            M.v = M.hs.eval(M.z);                                            // :205
            jb.C = M.C_bar;
            jb.z = M.z;
        });
        // 4. the opens (:209)
        for (OpenJob &jb : jobs) {
            std::memset(accs + jb.idx * aw, 0, 8 * aw);
            jb.proof[1] = lg;
        }
        rc = open_batch_dev(ctx, d, jobs, false, false, slots, S, ran);
        if (rc) return rc;
        if (!*ran) return HALO_OK;
        ctx->open_batch_members = jobs.size();  // (halo_ctx_info 10: the members that reached their opens)
    }
    *ran = true;
    // 5. the blobs and the outcomes
    for (OpenJob &jb : jobs) {
        ProverMember &M = mem[jb.idx];
        if (jb.rc) { M.rc = jb.rc; M.err = jb.err; continue; }
        uint64_t *acc = accs + jb.idx * aw, *piV = acc + iw;
        store_instance_head(acc, M.C_bar, d, M.z, M.v);
        M.hs.h0[0].store(piV);
        M.hs.h0[1].store(piV + 4);
        M.U0.store_normalized(piV + 8);
        M.w.store(piV + 20);
    }
    for (size_t j = 0; j < k; ++j) { codes[j] = mem[j].rc; errs[j] = mem[j].err; }
    *state_out = rng.state;
    return HALO_OK;
}

// halo_acc_prover_batch after its argument checks: the device form, or, where it does not apply, the loop itself
static int acc_prover_batch_entry(halo_ctx *ctx, uint64_t *rng_state, size_t d, const uint64_t *qs, const size_t *counts, size_t k, uint64_t *accs,
                                  int *status) {
    const size_t lg = ilog2(d + 1), iw = instance_words(lg), aw = acc_words(lg);
    int slots[HALO_SLOTS], S = idle_slots(ctx, slots);
    if (!S) { set_error("prover_batch: every slot has an MSM in flight"); return HALO_E_ARG; }
    std::vector<int> codes(k, HALO_OK);
    std::vector<std::string> errs(k);
    uint64_t state = rng_state ? *rng_state : 0;
    bool ran = false;
    ctx->open_batch_members = 0;
    int rc = acc_prover_batch_dev(ctx, state, d, qs, counts, k, accs, slots, S, &ran, codes, errs, &state);
    if (rc) return rc;
    if (!ran) {  // one member at a time through the single prover, from the same states
        size_t first = 0;
        for (size_t j = 0; j < k; first += counts[j], ++j) {
            rc = halo_acc_prover(ctx, &state, d, qs + first * iw, counts[j], accs + j * aw);
            if (rc == HALO_E_ASSERT || rc == HALO_E_REJECT) { codes[j] = rc; errs[j] = halo_last_error(); }
            else if (rc) return rc;
        }
    }
    if (rng_state) *rng_state = state;
    return report_members("member", k, [&](size_t j) { return codes[j]; }, [&](size_t j) { return errs[j]; }, status,
                          [&](size_t j) { std::memset(accs + j * aw, 0, 8 * aw); });
}

// the lists of the prover and verifier batches: k members, counts[j] instances each, one flat list of instances
int member_lists_ok(const char *who, const void *accs, const size_t *counts, size_t k, const void *instances) {
    auto bad = [&](const char *what) { set_error(std::string(who) + what); return HALO_E_ARG; };
    if (k && (!accs || !counts)) return bad(": null pointer");
    size_t total = 0;
    for (size_t j = 0; j < k; ++j) {
        if (counts[j] > ((size_t)1 << 32) - total) return bad(": too many instances");
        total += counts[j];
    }
    return total && !instances ? bad(": null pointer") : HALO_OK;
}

}  // namespace
}  // namespace halo

using namespace halo;

extern "C" {

// pcdl::check of m instances at once (see pcdl_check_batch_host)
int halo_pcdl_check_batch(halo_ctx *ctx, size_t d, const uint64_t *instances, size_t m, int *status) {
    HALO_CTX(ctx);
    return check_batch_entry(ctx, d, instances, m, status, false);
}

// ... as one combined relation over the accepted members (see check_members_combined; the contract: include/halo_accumulation.h)
int halo_pcdl_check_batch_combined(halo_ctx *ctx, size_t d, const uint64_t *instances, size_t m, const uint8_t seed[32], int *status) {
    HALO_CTX(ctx);
    return check_batch_entry(ctx, d, instances, m, status, false, CheckMode::combined, seed);
}

// ... and with the succinct relations in it too: ONE relation for the whole batch (see check_members_fused; the contract:
// include/halo_accumulation.h)
int halo_pcdl_check_batch_fused(halo_ctx *ctx, size_t d, const uint64_t *instances, size_t m, const uint8_t seed[32], int *status) {
    HALO_CTX(ctx);
    return check_batch_entry(ctx, d, instances, m, status, false, CheckMode::fused, seed);
}

// ... of m instances each with its own degree bound, exact and as one combined relation (see pcdl_check_mixed_host; the contract:
// include/halo_accumulation.h)
int halo_pcdl_check_batch_mixed(halo_ctx *ctx, const size_t *ds, const uint64_t *const *instances, size_t m, int *status) {
    HALO_CTX(ctx);
    return check_mixed_entry(ctx, ds, instances, m, status, CheckMode::exact, nullptr);
}

int halo_pcdl_check_batch_mixed_combined(halo_ctx *ctx, const size_t *ds, const uint64_t *const *instances, size_t m, const uint8_t seed[32], int *status) {
    HALO_CTX(ctx);
    return check_mixed_entry(ctx, ds, instances, m, status, CheckMode::combined, seed);
}

// ... and as one fused relation over the members of every size (see check_members_mixed_fused; the contract: include/halo_accumulation.h)
int halo_pcdl_check_batch_mixed_fused(halo_ctx *ctx, const size_t *ds, const uint64_t *const *instances, size_t m, const uint8_t seed[32], int *status) {
    HALO_CTX(ctx);
    return check_mixed_entry(ctx, ds, instances, m, status, CheckMode::fused, seed);
}

// acc::prover of k members at once (see acc_prover_batch_dev).  The argument checks are the whole call's and come before any work.
int halo_acc_prover_batch(halo_ctx *ctx, uint64_t *rng_state, size_t d, const uint64_t *instances, const size_t *counts, size_t k, uint64_t *accs_out,
                          int *status) {
    HALO_CTX(ctx);
    int rc = member_lists_ok("prover_batch", accs_out, counts, k, instances);
    if (rc) return rc;
    if (!is_pow2(d + 1)) return fail_assert("prover: d + 1 is not a power of two");
    if (d + 1 > ctx->n) return fail_assert("prover: d > D");
    if (k == 0) return HALO_OK;
    return acc_prover_batch_entry(ctx, rng_state, d, instances, counts, k, accs_out, status);
}

// acc::verifier of k accumulators at once (benches/acc.rs:64-74's loop in one call; see acc_verifier_batch_host).  The argument
// checks are the whole call's and come before any work: d + 1 above the key is the assert the single call meets in
// pcdl_commit_host.  A multi-device context runs the batch on its own device (devices[0]) like the other batches.
int halo_acc_verifier_batch(halo_ctx *ctx, size_t d, const uint64_t *instances, const size_t *counts, size_t k, const uint64_t *accs, int *status) {
    HALO_CTX(ctx);
    int rc = member_lists_ok("verifier_batch", accs, counts, k, instances);
    if (rc) return rc;
    if (!is_pow2(d + 1)) return fail_reject("d+1 is not a power of 2!");
    if (d + 1 > ctx->n) return fail_assert("commit: d > D");
    if (k == 0) return HALO_OK;
    return acc_verifier_batch_host(ctx, d, instances, counts, k, accs, status);
}

// acc::decider of m accumulators at once (benches/acc.rs:100-106 in one call): the check batch over their Instance prefixes
int halo_acc_decider_batch(halo_ctx *ctx, size_t d, const uint64_t *accs, size_t m, int *status) {
    HALO_CTX(ctx);
    return check_batch_entry(ctx, d, accs, m, status, true);
}

int halo_acc_decider_batch_combined(halo_ctx *ctx, size_t d, const uint64_t *accs, size_t m, const uint8_t seed[32], int *status) {
    HALO_CTX(ctx);
    return check_batch_entry(ctx, d, accs, m, status, true, CheckMode::combined, seed);
}

int halo_acc_decider_batch_fused(halo_ctx *ctx, size_t d, const uint64_t *accs, size_t m, const uint8_t seed[32], int *status) {
    HALO_CTX(ctx);
    return check_batch_entry(ctx, d, accs, m, status, true, CheckMode::fused, seed);
}

// ... of m accumulators each with its own degree bound: the mixed check batch over their Instance prefixes
int halo_acc_decider_batch_mixed(halo_ctx *ctx, const size_t *ds, const uint64_t *const *accs, size_t m, int *status) {
    HALO_CTX(ctx);
    return check_mixed_entry(ctx, ds, accs, m, status, CheckMode::exact, nullptr);
}

int halo_acc_decider_batch_mixed_combined(halo_ctx *ctx, const size_t *ds, const uint64_t *const *accs, size_t m, const uint8_t seed[32], int *status) {
    HALO_CTX(ctx);
    return check_mixed_entry(ctx, ds, accs, m, status, CheckMode::combined, seed);
}

int halo_acc_decider_batch_mixed_fused(halo_ctx *ctx, const size_t *ds, const uint64_t *const *accs, size_t m, const uint8_t seed[32], int *status) {
    HALO_CTX(ctx);
    return check_mixed_entry(ctx, ds, accs, m, status, CheckMode::fused, seed);
}

// pcdl::open of m polynomials at once (see open_batch_dev)
int halo_pcdl_open_batch(halo_ctx *ctx, uint64_t *rng_state, size_t d, const uint64_t *coeffs, size_t m, const uint64_t *Cs, const uint64_t *zs,
                         const uint64_t *ws, uint64_t *proofs_out, int *status) {
    HALO_CTX(ctx);
    if (m == 0) return HALO_OK;
    if (!coeffs || !Cs || !zs || !proofs_out) { set_error("open_batch: null pointer"); return HALO_E_ARG; }
    const size_t n = d + 1;
    if (!is_pow2(n)) return fail_assert("open: d + 1 is not a power of two");  // pcdl.rs:130 (p.degree() <= d: the arrays hold d + 1)
    if (n > ctx->n) return fail_assert("open: d > D");                         // pcdl.rs:132
    return open_batch_entry(ctx, rng_state, d, OpenSource{coeffs}, m, Cs, zs, ws, proofs_out, status);
}

// ... of m device-resident ones (see open_batch_entry): a member longer than d + 1 fails alone, as in halo_pcdl_commit_dev_batch
int halo_pcdl_open_dev_batch(halo_ctx *ctx, uint64_t *rng_state, size_t d, const void *const *d_coeffs, const size_t *lens, size_t m, const uint64_t *Cs,
                             const uint64_t *zs, const uint64_t *ws, uint64_t *proofs_out, int *status) {
    HALO_CTX(ctx);
    if (m == 0) return HALO_OK;
    if (!d_coeffs || !lens || !Cs || !zs || !proofs_out) { set_error("open_dev_batch: null pointer"); return HALO_E_ARG; }
    int rc = dev_rows_ok("open_dev_batch", d_coeffs, lens, m);
    if (rc) return rc;
    const size_t n = d + 1;
    if (!is_pow2(n)) return fail_assert("open: d + 1 is not a power of two");
    if (n > ctx->n) return fail_assert("open: d > D");
    return open_batch_entry(ctx, rng_state, d, OpenSource{nullptr, d_coeffs, lens}, m, Cs, zs, ws, proofs_out, status);
}

// pcdl::commit of m host polynomials at once (see commit_batch_run)
int halo_pcdl_commit_batch(halo_ctx *ctx, size_t d, const uint64_t *coeffs, size_t m, const uint64_t *ws, uint64_t *out_jac) {
    HALO_CTX(ctx);
    if (m && (!coeffs || !out_jac)) { set_error("commit_batch: null pointer"); return HALO_E_ARG; }
    int slots[HALO_SLOTS], S = 0;
    int rc = commit_batch_checks(ctx, d, slots, &S);
    if (rc || m == 0) return rc;
    std::vector<size_t> live(m);
    for (size_t i = 0; i < m; ++i) live[i] = i;
    return commit_batch_run(ctx, d, coeffs, nullptr, nullptr, live, ws, out_jac, slots, S);
}

// ... and of m device-resident ones: a member longer than d + 1 fails alone, as halo_pcdl_commit_dev fails
int halo_pcdl_commit_dev_batch(halo_ctx *ctx, size_t d, const void *const *d_coeffs, const size_t *lens, size_t m, const uint64_t *ws, uint64_t *out_jac,
                               int *status) {
    HALO_CTX(ctx);
    if (m && (!d_coeffs || !lens || !out_jac)) { set_error("commit_dev_batch: null pointer"); return HALO_E_ARG; }
    for (size_t i = 0; i < m; ++i)
        if ((lens[i] && !d_coeffs[i]) || ((uintptr_t)d_coeffs[i] & 31)) { set_error("commit_dev_batch: null or misaligned pointer"); return HALO_E_ARG; }
    int slots[HALO_SLOTS], S = 0;
    int rc = commit_batch_checks(ctx, d, slots, &S);
    if (rc || m == 0) return rc;
    std::vector<size_t> live;
    for (size_t i = 0; i < m; ++i)
        if (lens[i] <= d + 1) live.push_back(i);
    rc = commit_batch_run(ctx, d, nullptr, d_coeffs, lens, live, ws, out_jac, slots, S);
    if (rc) return rc;
    return report_members("member", m, [&](size_t i) { return lens[i] > d + 1 ? HALO_E_ASSERT : HALO_OK; },
                          [&](size_t) { return std::string("commit: p.degree() > d"); }, status,
                          [&](size_t i) { std::memset(out_jac + 12 * i, 0, 96); });
}

// benches/acc.rs:15-29 for m polynomials the caller holds: commit, evaluate, open and pack (open_batch_entry's third source)
int halo_instance_from_poly_batch(halo_ctx *ctx, uint64_t *rng_state, size_t d, const uint64_t *coeffs, size_t m, const uint64_t *zs, const uint64_t *ws,
                                  uint64_t *instances_out, int *status) {
    HALO_CTX(ctx);
    if (m == 0) return HALO_OK;
    if (!coeffs || !zs || !instances_out) { set_error("instance_from_poly_batch: null pointer"); return HALO_E_ARG; }
    const size_t n = d + 1;
    if (!is_pow2(n)) return fail_assert("commit: d + 1 is not a power of two");  // (the first of the loop's three calls)
    if (n > ctx->n) return fail_assert("commit: d > D");
    return open_batch_entry(ctx, rng_state, d, OpenSource{coeffs}, m, nullptr, zs, ws, instances_out, status);
}

// ... for m device-resident polynomials (see open_batch_entry)
int halo_instance_from_poly_dev_batch(halo_ctx *ctx, uint64_t *rng_state, size_t d, const void *const *d_coeffs, const size_t *lens, size_t m,
                                      const uint64_t *zs, const uint64_t *ws, uint64_t *instances_out, int *status) {
    HALO_CTX(ctx);
    if (m == 0) return HALO_OK;
    if (!d_coeffs || !lens || !zs || !instances_out) { set_error("instance_from_poly_dev_batch: null pointer"); return HALO_E_ARG; }
    int rc = dev_rows_ok("instance_from_poly_dev_batch", d_coeffs, lens, m);
    if (rc) return rc;
    const size_t n = d + 1;
    if (!is_pow2(n)) return fail_assert("commit: d + 1 is not a power of two");
    if (n > ctx->n) return fail_assert("commit: d > D");
    return open_batch_entry(ctx, rng_state, d, OpenSource{nullptr, d_coeffs, lens}, m, nullptr, zs, ws, instances_out, status);
}

// benches/acc.rs:15-29 random_instance, m times (see open_batch_dev)
int halo_random_instance_batch(halo_ctx *ctx, uint64_t *rng_state, size_t d, size_t m, uint64_t *instances_out) {
    HALO_CTX(ctx);
    if (m == 0) return HALO_OK;
    if (!instances_out) { set_error("random_instance_batch: null pointer"); return HALO_E_ARG; }
    if (!is_pow2(d + 1) || d < 2) return fail_assert("random_instance: bad d");
    if (d + 1 > ctx->n) return fail_assert("random_instance: d > D");
    return open_batch_entry(ctx, rng_state, d, OpenSource{}, m, nullptr, nullptr, nullptr, instances_out, nullptr);
}

}  // extern "C"
