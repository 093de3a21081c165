// Host side above the kernels: the reference's `pedersen`, `pcdl` and `acc` modules with the
// same names, argument meaning and error behaviour (pedersen.rs:6-20, pcdl.rs:99-342,
// acc.rs:135-255), every linear-time step running in HIP.  The reference is Rust and there is
// no Rust toolchain in this image, so this layer is C++ behind a C ABI; INTEGRATION.md shows
// the Rust shim that would sit on the group.rs-level entry points instead.
//
// What stays on the host, exactly as in the reference: Fiat-Shamir hashing (rho_0!/rho_1!),
// challenge inversion, the O(lg n) succinct check and the struct packing.
#include <atomic>
#include <functional>
#include <memory>
#include <thread>

#include "internal.hpp"

namespace halo {

using host::Fr;
using host::Point;
using host::Transcript;

// ---- flat layouts (include/halo_accumulation.h, "pcdl / acc level")
static size_t proof_words(size_t lg) { return 2 + 24 * lg + 32; }
static size_t instance_words(size_t lg) { return 21 + proof_words(lg); }
static size_t acc_words(size_t lg) { return instance_words(lg) + 24; }
static uint64_t *pf_L(uint64_t *pf, size_t i) { return pf + 2 + 12 * i; }
static uint64_t *pf_R(uint64_t *pf, size_t lg, size_t i) { return pf + 2 + 12 * lg + 12 * i; }
static uint64_t *pf_U(uint64_t *pf, size_t lg) { return pf + 2 + 24 * lg; }
static uint64_t *pf_c(uint64_t *pf, size_t lg) { return pf + 2 + 24 * lg + 12; }
static uint64_t *pf_Cbar(uint64_t *pf, size_t lg) { return pf + 2 + 24 * lg + 16; }
static uint64_t *pf_wp(uint64_t *pf, size_t lg) { return pf + 2 + 24 * lg + 28; }

static bool is_pow2(size_t n) { return n && !(n & (n - 1)); }
static size_t ilog2(size_t n) { size_t l = 0; while (n > 1) { n >>= 1; ++l; } return l; }
static int fail_assert(const char *m) { set_error(m); return HALO_E_ASSERT; }
static int fail_reject(const char *m) { set_error(m); return HALO_E_REJECT; }

struct PublicPoints { Point S, H; };
static const PublicPoints &public_points() {  // main.rs:35-45 / consts.rs:26-65
    static PublicPoints pp = [] {
        Point g = Point::generator();
        return PublicPoints{g.mul(host::urs_scalar(0)).normalized(), g.mul(host::urs_scalar(1)).normalized()};
    }();
    return pp;
}

static Fr rho0_C_z_v(const Point &C, const Fr &z, const Fr &v) {
    Transcript t; t.point(C); t.scalar(z); t.scalar(v); return t.finish(0);
}
static Fr rho0_C_z_v_Cbar(const Point &C, const Fr &z, const Fr &v, const Point &Cb) {
    Transcript t; t.point(C); t.scalar(z); t.scalar(v); t.point(Cb); return t.finish(0);
}
static Fr rho0_xi_L_R(const Fr &xi, const Point &L, const Point &R) {
    Transcript t; t.scalar(xi); t.point(L); t.point(R); return t.finish(0);
}

static int ensure_poly_buffers(halo_ctx *ctx) {
    size_t n = ctx->n < 64 ? 64 : ctx->n;
    if (!ctx->d_poly || !ctx->d_poly2) alloc_epoch_bump(ctx);
    if (!ctx->d_poly) HALO_HIP(hipMalloc(&ctx->d_poly, n * 32));
    if (!ctx->d_poly2) HALO_HIP(hipMalloc(&ctx->d_poly2, n * 32));
    return HALO_OK;
}

// DensePolynomial::degree: the index of the last non-zero coefficient (0 for the zero polynomial).  Scanned from the END: a
// dense polynomial answers at its first look (the forward scan this replaces read all 32 MiB of a 2^20-coefficient polynomial
// on the host, ~1 ms of every halo_pcdl_open / halo_pcdl_commit with host coefficients).
static size_t host_poly_degree(const uint64_t *coeffs, size_t len) {
    for (size_t i = len; i-- > 0;)
        if (coeffs[4 * i] | coeffs[4 * i + 1] | coeffs[4 * i + 2] | coeffs[4 * i + 3]) return i;
    return 0;
}

// pedersen::commit over GS[0..n) for device-resident, zero-padded scalars (pedersen.rs:6-20)
static int pedersen_commit_dev(halo_ctx *ctx, const Fr *w, const uint64_t *d_ms, size_t n, Point *out) {
    Point acc;
    int rc = msm_run(ctx, ctx->d_bases, d_ms, true, n, &acc);
    if (rc) return rc;
    if (w) acc = public_s_table().mul(*w) + acc;
    *out = acc;
    return HALO_OK;
}

// pcdl::commit for a short host polynomial (acc.rs:153,195: two coefficients): same point, no launch
static int commit_short_host(halo_ctx *ctx, const uint64_t *coeffs, size_t len, const Fr *w, Point *out) {
    std::vector<uint64_t> bases(8 * len);
    int rc = halo_ctx_read_bases(ctx, 0, len, bases.data());
    if (rc) return rc;
    std::vector<Point> pts(len);
    std::vector<Fr> ks(len);
    for (size_t i = 0; i < len; ++i) { pts[i] = Point::load_affine(&bases[8 * i]); ks[i] = Fr::load(coeffs + 4 * i); }
    Point acc = host::small_msm(pts, ks);
    if (w) acc = public_s_table().mul(*w) + acc;
    *out = acc;
    return HALO_OK;
}

// pcdl.rs:99-110
static int pcdl_commit_host(halo_ctx *ctx, const uint64_t *coeffs, size_t len, size_t d, const Fr *w, Point *out) {
    size_t n = d + 1;
    if (!is_pow2(n)) return fail_assert("commit: d + 1 is not a power of two");
    size_t deg = host_poly_degree(coeffs, len);
    if (deg > d) return fail_assert("commit: p.degree() > d");
    if (d + 1 > ctx->n) return fail_assert("commit: d > D");
    size_t used = deg + 1 < len ? deg + 1 : len;
    if (used <= 16) return commit_short_host(ctx, coeffs, used, w, out);
    // pedersen::commit over GS[0..n) (pedersen.rs:6-20) with the coefficients still in host memory: halo_msm's path (abi.hip
    // msm_host_run: the copy in stretches under the kernels where that pays), zero-padded beyond the polynomial
    Point acc;
    int rc = msm_host_run(ctx, 0, n, coeffs, used, 1, &acc);
    if (rc) return rc;
    if (w) acc = public_s_table().mul(*w) + acc;
    *out = acc;
    return HALO_OK;
}

// pcdl.rs:120-242 on a device-resident polynomial (d_poly: n coefficients, zero padded, clobbered)
static int pcdl_open_dev(halo_ctx *ctx, host::Rng *rng, size_t deg, const Point &C, size_t d, const Fr &z, const Fr *w,
                         uint64_t *proof) {
    size_t n = d + 1, lg_n = ilog2(n);
    std::memset(proof, 0, 8 * proof_words(lg_n));
    proof[1] = lg_n;
    Fr v;
    int rc = fr_poly_eval(ctx, ctx->d_poly, deg + 1, z, &v);  // :135
    if (rc) return rc;
    Point C_prime = C;
    if (w) {
        if (deg == 0) return fail_assert("open: hiding needs p.degree() >= 1");  // usize underflow at :141
        // :140-142  q uniform of degree deg-1, p_bar = q (X - z)
        rc = rng_scalars_dev(ctx, rng->state, deg, ctx->d_tmp_a);
        if (rc) return rc;
        rng->state += 4 * (uint64_t)deg * 0x9E3779B97F4A7C15ULL;
        HALO_HIP(hipMemsetAsync(ctx->d_poly2, 0, n * 32, ctx->stream));
        rc = pbar_dev(ctx, ctx->d_tmp_a, deg, z, ctx->d_poly2);
        if (rc) return rc;
        Fr w_bar = rng->scalar();  // :147
        Point C_bar;
        rc = pedersen_commit_dev(ctx, &w_bar, ctx->d_poly2, n, &C_bar);  // :150
        if (rc) return rc;
        Fr a = rho0_C_z_v_Cbar(C, z, v, C_bar);                            // :153
        rc = axpy_dev(ctx, ctx->d_poly, ctx->d_poly2, deg + 1, a);         // :156
        if (rc) return rc;
        Fr w_prime = w_bar * a + *w;                                       // :159
        C_prime = C + C_bar.mul(a) - public_s_table().mul(w_prime);                    // :162
        proof[0] = 1;
        C_bar.store_normalized(pf_Cbar(proof, lg_n));
        w_prime.store(pf_wp(proof, lg_n));
    } else {
        Point::infinity().store(pf_Cbar(proof, lg_n));
    }
    Fr xi = rho0_C_z_v(C_prime, z, v);  // :180
    Point Hp = public_h_table().mul(xi).normalized();  // :181
    uint64_t Hp_w[12];
    Hp.store(Hp_w);
    halo_ipa *st = nullptr;
    rc = ipa_begin_dev(ctx, n, ctx->d_poly, z, &st);  // :183-186
    if (rc) return rc;
    std::unique_ptr<halo_ipa, void (*)(halo_ipa *)> guard(st, halo_ipa_destroy);
    ipa_set_hprime_scalar(st, xi);  // H' = xi_0 H: the rounds take k H' = (k xi_0) H from the process-wide table of H
    for (size_t round = 0; round < lg_n; ++round) {
        uint64_t *Lw = pf_L(proof, round), *Rw = pf_R(proof, lg_n, round);
        rc = halo_ipa_round_lr(st, Hp_w, Lw, Rw);  // :203-208
        if (rc) return rc;
        Fr xi_next = rho0_xi_L_R(xi, Point::load(Lw), Point::load(Rw));  // :212
        if (xi_next.is_zero()) return fail_assert("open: challenge is zero (inverse().unwrap())");
        Fr xi_inv = xi_next.inv();  // :213
        xi = xi_next;
        uint64_t xw[4], xiw[4];
        xi.store(xw);
        xi_inv.store(xiw);
        rc = halo_ipa_round_fold(st, xw, xiw);  // :216-224
        if (rc) return rc;
    }
    return halo_ipa_finish(st, pf_U(proof, lg_n), pf_c(proof, lg_n));  // :230-231
}

static bool scalar_ok(const Fr &s) { return !Fr::geq(s.l, host::FrP::M); }
// every point of the blob on the curve, every scalar canonical, flag word 0 or 1
static bool proof_wellformed(uint64_t *proof, size_t lg_n) {
    if (proof[0] > 1) return false;
    for (size_t i = 0; i < lg_n; ++i)
        if (!Point::load(pf_L(proof, i)).on_curve() || !Point::load(pf_R(proof, lg_n, i)).on_curve()) return false;
    if (!Point::load(pf_U(proof, lg_n)).on_curve() || !scalar_ok(Fr::load(pf_c(proof, lg_n)))) return false;
    if (proof[0] && (!Point::load(pf_Cbar(proof, lg_n)).on_curve() || !scalar_ok(Fr::load(pf_wp(proof, lg_n))))) return false;
    return true;
}

// pcdl.rs:252-314 in two halves.  challenges(): everything the transcript decides -- C', xi_0 .. xi_lg (pcdl.rs:272-296);
// this is all pcdl::check's linear-time half (h.get_poly + the MSM, pcdl.rs:338) needs, so that half is launched
// before relation() runs on the host.  relation(): the 2 lg n + O(1) scalar multiplications as one interleaved
// host MSM and the final comparison (pcdl.rs:288-310).
struct SuccinctState {
    size_t lg_n = 0;
    Point C_prime, Hp, U;
    std::vector<Fr> xis;
};
// key_n: the size of the key the check is against (ctx->n; a rank's cyclic shard stands for stride * ctx->n points)
static int succinct_challenges(halo_ctx *ctx, const Point &C, size_t d, const Fr &z, const Fr &v, const uint64_t *proof_c, SuccinctState *st,
                               bool need_hp = true, size_t key_n = 0) {
    uint64_t *proof = const_cast<uint64_t *>(proof_c);
    size_t n = d + 1;
    if (!is_pow2(n)) return fail_reject("d+1 is not a power of 2!");
    if (d + 1 > (key_n ? key_n : ctx->n)) return fail_reject("d was larger than D!");
    size_t lg_n = ilog2(n);
    if (proof[1] != lg_n) return fail_reject("proof length does not match d");
    // Everything below reads exactly proof_words(lg_n) words.  The blob is verifier input: the reference's typed
    // `PallasPoint`/`PallasScalar` values are on the curve / below the modulus by construction, here that is checked.
    if (!C.on_curve() || !scalar_ok(z) || !scalar_ok(v)) return fail_reject("instance holds an invalid point or scalar");
    if (!proof_wellformed(proof, lg_n)) return fail_reject("proof holds an invalid point or scalar");
    st->lg_n = lg_n;
    st->C_prime = C;
    if (proof[0]) {
        Point C_bar = Point::load(pf_Cbar(proof, lg_n));
        Fr wp = Fr::load(pf_wp(proof, lg_n));
        Fr a = rho0_C_z_v_Cbar(C, z, v, C_bar);
        st->C_prime = C + C_bar.mul(a) - public_s_table().mul(wp);
    }
    st->xis.assign(lg_n + 1, Fr::zero());
    st->xis[0] = rho0_C_z_v(st->C_prime, z, v);
    if (need_hp) st->Hp = public_h_table().mul(st->xis[0]);  // the batched relation multiplies H by (v - v') xi_0 instead
    for (size_t i = 0; i < lg_n; ++i) {
        st->xis[i + 1] = rho0_xi_L_R(st->xis[i], Point::load(pf_L(proof, i)), Point::load(pf_R(proof, lg_n, i)));
        if (st->xis[i + 1].is_zero()) return fail_reject("challenge is zero");
    }
    st->U = Point::load(pf_U(proof, lg_n));
    return HALO_OK;
}
static int succinct_relation(const SuccinctState &st, const Fr &z, const Fr &v, const uint64_t *proof_c) {
    uint64_t *proof = const_cast<uint64_t *>(proof_c);
    size_t lg_n = st.lg_n;
    const std::vector<Fr> &xis = st.xis;
    std::vector<Point> pts;
    std::vector<Fr> ks;
    pts.reserve(2 * lg_n + 1);
    ks.reserve(2 * lg_n + 1);
    for (size_t i = 0; i < lg_n; ++i) {
        pts.push_back(Point::load(pf_L(proof, i))); ks.push_back(xis[i + 1]);  // scalar replaced by its inverse below
        pts.push_back(Point::load(pf_R(proof, lg_n, i))); ks.push_back(xis[i + 1]);
    }
    // one inversion for all challenges (Montgomery's trick)
    {
        std::vector<Fr> pref(lg_n + 1, Fr::one());
        for (size_t i = 0; i < lg_n; ++i) pref[i + 1] = pref[i] * xis[i + 1];
        Fr inv = lg_n ? pref[lg_n].inv() : Fr::one();
        for (size_t i = lg_n; i-- > 0;) {
            ks[2 * i] = inv * pref[i];  // xi_{i+1}^-1
            inv = inv * xis[i + 1];
        }
    }
    pts.push_back(st.Hp); ks.push_back(v);
    // :288-298.  2 lg n + 1 scalar multiples (~1.1 ms on one thread at lg n = 20): four interleaved-window sums on the host
    // pool, added in order (the verifier's two instances run side by side: eight threads for ~0.35 ms)
    Point C_i = st.C_prime;
    {
        const size_t ways = pts.size() >= 16 ? 4 : 1, per = (pts.size() + ways - 1) / ways;
        std::vector<Point> part(ways, Point::infinity());
        pool_run(ways, [&](size_t k) {
            size_t lo = k * per, hi = lo + per < pts.size() ? lo + per : pts.size();
            if (lo >= hi) return;
            part[k] = host::small_msm(std::vector<Point>(pts.begin() + lo, pts.begin() + hi), std::vector<Fr>(ks.begin() + lo, ks.begin() + hi));
        });
        for (size_t k = 0; k < ways; ++k) C_i = C_i + part[k];
    }
    // :301-304  v' = c * h(z)
    Fr c = Fr::load(pf_c(proof, lg_n));
    Fr hz = Fr::one() + xis[lg_n] * z, zi = z;
    for (size_t i = 1; i < lg_n; ++i) { zi = zi.sqr(); hz = hz * (Fr::one() + xis[lg_n - i] * zi); }
    Fr v_prime = c * hz;
    std::vector<Point> p2{st.U, st.Hp};
    std::vector<Fr> k2{c, v_prime};
    if (C_i != host::small_msm(p2, k2)) return fail_reject("C_(log_n) != CM.Commit_Sigma(c || v')");  // :307-310
    return HALO_OK;
}
static int succinct_check_host(halo_ctx *ctx, const Point &C, size_t d, const Fr &z, const Fr &v, const uint64_t *proof_c,
                               std::vector<Fr> *xis_out, Point *U_out) {
    SuccinctState st;
    int rc = succinct_challenges(ctx, C, d, z, v, proof_c, &st);
    if (!rc) rc = succinct_relation(st, z, v, proof_c);
    if (rc) return rc;
    *xis_out = std::move(st.xis);
    *U_out = st.U;
    return HALO_OK;
}

// ------------------------------------------------------------------ batched succinct checks (acc.rs:158-170)
// m instances at once: the transcripts (hashes, C') are computed by a bounded pool of host threads, then ONE launch evaluates
// the m polynomials h_i at their own z_i (k_h_eval_z) and ONE launch computes the m relations (k_batch_small_msm):
//     C'_i + sum_j (xi_j^-1 L_j + xi_j R_j) + (v_i - c_i h_i(z_i)) xi_0 H - c_i U_i  ==  0        (pcdl.rs:288-310)
// as 2 lg n + 2 scalar multiples per instance, compared with -C'_i on the host.  Per-instance outcome equals the host path's.
constexpr size_t kBatchVerifyMin = 64;  // below this the host pool is faster than a 256-step device ladder (~2 ms)
static int verify_staging(halo_ctx *ctx, size_t words) {
    if (words <= ctx->verify_words) return HALO_OK;
    alloc_epoch_bump(ctx);
    (void)hipFree(ctx->d_verify);
    ctx->d_verify = nullptr;
    ctx->verify_words = 0;
    HALO_HIP(hipMalloc(&ctx->d_verify, words * 8));
    ctx->verify_words = words;
    return HALO_OK;
}
struct BatchCheck { int rc = HALO_OK; std::string err; SuccinctState st; };
// The 2 lg n + 2 terms of one instance's relation (q: its blob, hz = h(z) of its challenges, st: its accepted transcript) whose
// sum is -C' exactly when pcdl.rs:288-310 accepts: points arkworks affine ((0, 0) = infinity), scalars canonical
static void relation_terms(const SuccinctState &st, const uint64_t *q, const Fr &hz, uint64_t *pts, uint64_t *sc) {
    const size_t lg = st.lg_n;
    uint64_t *proof = const_cast<uint64_t *>(q + 21);
    auto put_point = [&](size_t slot, const Point &p) {
        host::Affine a = p.to_affine();
        if (!a.inf) { a.x.store(pts + 8 * slot); a.y.store(pts + 8 * slot + 4); }
    };
    // challenge inverses with one inversion (Montgomery's trick)
    std::vector<Fr> pref(lg + 1, Fr::one()), inv(lg + 1);
    for (size_t j = 0; j < lg; ++j) pref[j + 1] = pref[j] * st.xis[j + 1];
    Fr run = lg ? pref[lg].inv() : Fr::one();
    for (size_t j = lg; j-- > 0;) { inv[j + 1] = run * pref[j]; run = run * st.xis[j + 1]; }
    for (size_t j = 0; j < lg; ++j) {
        put_point(j, Point::load(pf_L(proof, j)));
        inv[j + 1].from_mont().store(sc + 4 * j);
        put_point(lg + j, Point::load(pf_R(proof, lg, j)));
        st.xis[j + 1].from_mont().store(sc + 4 * (lg + j));
    }
    Fr c = Fr::load(pf_c(proof, lg)), v = Fr::load(q + 17);
    put_point(2 * lg, public_points().H);
    ((v - c * hz) * st.xis[0]).from_mont().store(sc + 4 * (2 * lg));      // (v - v') xi_0 on H: the two H' terms of :288 and :307
    put_point(2 * lg + 1, st.U);
    (-c).from_mont().store(sc + 4 * (2 * lg + 1));
}
// instances: m blobs at stride `stride` words (0: instance_words(lg(d+1)); an Accumulator's Instance prefix at acc_words);
// res[i].rc / .err / .st filled; returns a device / argument error only
static int succinct_check_batch(halo_ctx *ctx, size_t d, const uint64_t *qs, size_t m, std::vector<BatchCheck> &res, size_t stride = 0) {
    size_t lg = ilog2(d + 1), iw = stride ? stride : instance_words(lg), K = 2 * lg + 2;
    res.assign(m, BatchCheck());
    if (K > 64) { set_error("batched succinct check: lg n too large"); return HALO_E_ARG; }
    pool_run(m, [&](size_t i) {
        const uint64_t *q = qs + i * iw;
        res[i].rc = succinct_challenges(ctx, Point::load(q), (size_t)q[12], Fr::load(q + 13), Fr::load(q + 17), q + 21, &res[i].st, false);
        if (res[i].rc) res[i].err = halo_last_error();
    });
    // staging layout (words): xis m (lg+1) 4 | zs m 4 | hz m 4 | points m K 8 | scalars m K 4 | out m 12
    size_t o_xis = 0, o_zs = o_xis + m * (lg + 1) * 4, o_hz = o_zs + m * 4, o_pts = o_hz + m * 4, o_sc = o_pts + m * K * 8, o_out = o_sc + m * K * 4,
           total = o_out + m * 12;
    int rc = verify_staging(ctx, total);
    if (rc) return rc;
    std::vector<uint64_t> host(total, 0);
    for (size_t i = 0; i < m; ++i) {
        if (res[i].rc) continue;  // a rejected transcript: its (zero) rows are computed and ignored
        for (size_t k = 0; k <= lg; ++k) res[i].st.xis[k].store(&host[o_xis + (i * (lg + 1) + k) * 4]);
        std::memcpy(&host[o_zs + 4 * i], qs + i * iw + 13, 32);
    }
    HALO_HIP(hipMemcpyAsync(ctx->d_verify, host.data(), (o_hz) * 8, hipMemcpyHostToDevice, ctx->stream));
    rc = h_eval_each(ctx, ctx->d_verify + o_xis, ctx->d_verify + o_zs, m, lg, ctx->d_verify + o_hz);
    if (rc) return rc;
    HALO_HIP(hipMemcpyAsync(&host[o_hz], ctx->d_verify + o_hz, m * 32, hipMemcpyDeviceToHost, ctx->stream));
    HALO_HIP(hipStreamSynchronize(ctx->stream));
    pool_run(m, [&](size_t i) {
        if (res[i].rc) return;
        relation_terms(res[i].st, qs + i * iw, Fr::load(&host[o_hz + 4 * i]), &host[o_pts + i * K * 8], &host[o_sc + i * K * 4]);
    });
    HALO_HIP(hipMemcpyAsync(ctx->d_verify + o_pts, &host[o_pts], (o_out - o_pts) * 8, hipMemcpyHostToDevice, ctx->stream));
    rc = batch_small_msm(ctx, ctx->d_verify + o_pts, ctx->d_verify + o_sc, m, K, ctx->d_verify + o_out);
    if (rc) return rc;
    HALO_HIP(hipMemcpyAsync(&host[o_out], ctx->d_verify + o_out, m * 96, hipMemcpyDeviceToHost, ctx->stream));
    HALO_HIP(hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < m; ++i) {
        if (res[i].rc) continue;
        if (Point::load(&host[o_out + 12 * i]) != -res[i].st.C_prime) {
            res[i].rc = HALO_E_REJECT;
            res[i].err = "C_(log_n) != CM.Commit_Sigma(c || v')";  // :307-310
        }
    }
    return HALO_OK;
}

// pcdl.rs:323-342.  The device half (h coefficients + the n-point MSM, :338) runs while the host evaluates the
// succinct relation; errors are reported in the reference's order (succinct check first).
static int pcdl_check_host(halo_ctx *ctx, const Point &C, size_t d, const Fr &z, const Fr &v, const uint64_t *proof) {
    SuccinctState st;
    int rc = succinct_challenges(ctx, C, d, z, v, proof, &st, false);  // (H' = xi_0 H: only the relation needs it -- below, under the MSM)
    if (rc) return rc;
    size_t lg_n = st.lg_n, n = d + 1;
    rc = h_coeffs_dev(ctx, st.xis.data(), lg_n, Fr::one(), false, ctx->d_tmp_a);  // h.get_poly().coeffs
    if (rc) return rc;
    {
        BorrowScope scope(ctx);  // (nothing else of the caller's is in flight during a check: a large MSM may use slot 1 as well)
        rc = msm_enqueue(ctx, 0, ctx->d_bases, ctx->d_tmp_a, true, n);  // :338, asynchronous
    }
    if (rc) return rc;
    st.Hp = public_h_table().mul(st.xis[0]);
    int rc_rel = succinct_relation(st, z, v, proof);
    std::string rel_err = rc_rel ? halo_last_error() : "";
    Point comm;
    rc = msm_finish(ctx, 0, &comm);
    if (rc_rel) { set_error(rel_err); return rc_rel; }
    if (rc) return rc;
    if (st.U != comm) return fail_reject("U != CM.Commit(ck, h_vec)");  // :339
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
    int g = forced >= 1 && forced <= MSM_MAX_BATCH ? forced : MSM_MAX_BATCH;
    if (forced <= 0 && n >= ((size_t)1 << 20) && ctx->n >= ((size_t)1 << 20) && ctx->table_mode != 0) g = 1;
    MsmPlan p = msm_plan(n, ctx->window_bits);
    while (g > 1 && (size_t)p.W * (size_t)g * p.B > ((size_t)1 << 22)) --g;
    return g;
}
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
// blobs: m Instances (or Accumulators, whose Instance prefix is checked) at `stride` words, all of degree bound d (checked by
// the caller); status[i] (nullable) = what halo_pcdl_check returns for member i alone
static int pcdl_check_batch_host(halo_ctx *ctx, size_t d, const uint64_t *qs, size_t stride, size_t m, int *status) {
    const size_t n = d + 1, lg = ilog2(n);
    int slots[HALO_SLOTS], S = 0;
    for (int k = 0; k < HALO_SLOTS; ++k)
        if (!ctx->wss[k].in_flight && ctx->wss[k].lent_from < 0 && !ctx->fan[k].active) slots[S++] = k;
    if (!S) { set_error("check_batch: every slot has an MSM in flight"); return HALO_E_ARG; }
    // 1. the succinct half (pcdl.rs:333)
    std::vector<BatchCheck> res;
    if (m >= kBatchVerifyMin && ctx->batch_verify) {
        int rc = succinct_check_batch(ctx, d, qs, m, res, stride);
        if (rc) return rc;
    } else {
        res.assign(m, BatchCheck());
        pool_run(m, [&](size_t i) {
            const uint64_t *q = qs + i * stride;
            res[i].rc = succinct_challenges(ctx, Point::load(q), d, Fr::load(q + 13), Fr::load(q + 17), q + 21, &res[i].st);
            if (!res[i].rc) res[i].rc = succinct_relation(res[i].st, Fr::load(q + 13), Fr::load(q + 17), q + 21);
            if (res[i].rc) res[i].err = halo_last_error();
        });
    }
    std::vector<size_t> ok;  // the accepted members, in order
    for (size_t i = 0; i < m; ++i)
        if (!res[i].rc) ok.push_back(i);
    const size_t A = ok.size();
    if (A) {
        if (lg > 24) { set_error("h_coeffs: lg_n > 24 unsupported"); return HALO_E_ARG; }
        // 2. their challenges in device memory, in that order (one copy)
        const size_t xw = (lg + 1) * 4;
        std::vector<uint64_t> xis(A * xw);
        for (size_t a = 0; a < A; ++a)
            for (size_t k = 0; k <= lg; ++k) res[ok[a]].st.xis[k].store(&xis[a * xw + 4 * k]);
        int rc = verify_staging(ctx, xis.size());
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
        std::vector<long> flight(S, -1);  // the group in flight on slots[j]
        auto collect = [&](size_t j) -> int {
            long g = flight[j];
            if (g < 0) return HALO_OK;
            flight[j] = -1;
            size_t first = (size_t)g * G, cnt = A - first < G ? A - first : G;
            Point pts[MSM_MAX_BATCH];
            int rc2 = msm_finish_batch(ctx, slots[j], pts, (int)cnt);
            if (rc2) return rc2;
            for (size_t b = 0; b < cnt; ++b) {
                BatchCheck &r = res[ok[first + b]];
                if (r.st.U != pts[b]) { r.rc = HALO_E_REJECT; r.err = "U != CM.Commit(ck, h_vec)"; }  // :339
            }
            return HALO_OK;
        };
        auto abandon = [&]() {  // (a device error: nothing of this call stays in flight)
            std::string err = halo_last_error();
            for (int j = 0; j < S; ++j)
                if (flight[j] >= 0) {
                    Point pts[MSM_MAX_BATCH];
                    size_t first = (size_t)flight[j] * G;
                    (void)msm_finish_batch(ctx, slots[j], pts, (int)(A - first < G ? A - first : G));
                    flight[j] = -1;
                }
            set_error(err);
        };
        for (size_t g = 0; g < ng; ++g) {
            const size_t j = g % (size_t)S, first = g * G, cnt = A - first < G ? A - first : G;
            rc = collect(j);
            if (!rc) {
                hipStream_t saved = ctx->stream;  // (the launch macro uses ctx->stream: the slot's own)
                ctx->stream = ctx->streams[slots[j]];
                rc = h_coeffs_batch_dev(ctx, ctx->d_verify + first * xw, cnt, lg, tables_of(j), coeffs_of(j), n * 4);  // h.get_poly().coeffs
                ctx->stream = saved;
            }
            if (!rc) {
                MsmBatch mb;
                mb.count = (int)cnt;
                for (size_t b = 0; b < cnt; ++b) mb.scalars[b] = coeffs_of(j) + b * n * 4;
                rc = msm_enqueue_batch(ctx, slots[j], ctx->d_bases, mb, true, n);  // :338, asynchronous
            }
            if (rc) { abandon(); return rc; }
            flight[j] = (long)g;
        }
        for (size_t g = ng > (size_t)S ? ng - (size_t)S : 0; g < ng; ++g) {
            rc = collect(g % (size_t)S);
            if (rc) { abandon(); return rc; }
        }
    }
    int first = -1;
    for (size_t i = 0; i < m; ++i) {
        if (status) status[i] = res[i].rc;
        if (res[i].rc && first < 0) first = (int)i;
    }
    if (first >= 0) { set_error("instance " + std::to_string(first) + ": " + res[first].err); return res[first].rc; }
    return HALO_OK;
}
// the argument checks of both entry points (halo_pcdl_succinct_check_batch's), then the batch; acc: Accumulator blobs
static int check_batch_entry(halo_ctx *ctx, size_t d, const uint64_t *blobs, size_t m, int *status, bool acc) {
    if (m && !blobs) { set_error("check_batch: null pointer"); return HALO_E_ARG; }
    if (!is_pow2(d + 1)) return fail_reject("d+1 is not a power of 2!");
    size_t lg = ilog2(d + 1), stride = acc ? acc_words(lg) : instance_words(lg);
    for (size_t i = 0; i < m; ++i)
        if ((size_t)(blobs + i * stride)[12] != d || (blobs + i * stride)[22] != lg) return fail_reject("d_i != d");
    if (m == 0) return HALO_OK;
    return pcdl_check_batch_host(ctx, d, blobs, stride, m, status);
}

// One rank's half of pcdl::check when the key is sharded cyclically (point i on rank i mod P): the succinct check (host
// arithmetic, the same on every rank) and this rank's share of CM.Commit(ck, h) (:338).  The coefficient of X^(r + j P) is
//     prod_{i < p, bit i of r} xi_(lg n - i)  *  prod_{bit i' of j} xi_(lg n - p - i')            (P = 2^p, pcdl.rs:56-77)
// i.e. a constant of the rank times the j-th coefficient of the h polynomial of the first lg n - p challenges: the shard's
// scalars are h_coeffs_dev over lg n - p variables scaled by that constant.  The caller adds the P shares and compares
// with U (:339).
static int pcdl_check_partial_host(halo_ctx *ctx, const Point &C, size_t d, const Fr &z, const Fr &v, const uint64_t *proof, uint64_t stride,
                                   uint64_t offset, Point *U_out, Point *part_out) {
    if (stride == 0 || !is_pow2(stride) || offset >= stride) { set_error("check_partial: stride must be a power of two, offset below it"); return HALO_E_ARG; }
    if (ctx->n == 0 || !is_pow2(ctx->n)) { set_error("check_partial: the shard's key must hold a power of two of points"); return HALO_E_ARG; }
    SuccinctState st;
    int rc = succinct_challenges(ctx, C, d, z, v, proof, &st, true, ctx->n * stride);
    if (rc) return rc;
    size_t lg_n = st.lg_n, n = d + 1, p = ilog2((size_t)stride);
    if (n < stride) { set_error("check_partial: fewer coefficients than ranks"); return HALO_E_ARG; }
    size_t n_local = n / stride;  // <= ctx->n
    Fr scale = Fr::one();
    for (size_t i = 0; i < p; ++i)
        if ((offset >> i) & 1) scale = scale * st.xis[lg_n - i];
    rc = h_coeffs_dev(ctx, st.xis.data(), lg_n - p, scale, false, ctx->d_tmp_a);
    if (rc) return rc;
    rc = msm_enqueue(ctx, 0, ctx->d_bases, ctx->d_tmp_a, true, n_local);  // asynchronous: the relation runs on the host meanwhile
    if (rc) return rc;
    int rc_rel = succinct_relation(st, z, v, proof);
    std::string rel_err = rc_rel ? halo_last_error() : "";
    Point part;
    rc = msm_finish(ctx, 0, &part);
    if (rc_rel) { set_error(rel_err); return rc_rel; }
    if (rc) return rc;
    *U_out = st.U;
    *part_out = part;
    return HALO_OK;
}

// ------------------------------------------------------------------ acc.rs
struct AccHPolys {  // acc.rs:61-66
    Fr h0[2];
    std::vector<std::vector<Fr>> xis;
    Fr alpha;
    std::vector<Fr> alphas;  // alpha^0 .. alpha^m
    size_t lg_n = 0;

    Fr eval(const Fr &z) const {  // acc.rs:97-106
        Fr v = h0[0] + h0[1] * z;
        for (size_t i = 0; i < xis.size(); ++i) {
            const std::vector<Fr> &x = xis[i];
            Fr hz = Fr::one() + x[lg_n] * z, zi = z;
            for (size_t k = 1; k < lg_n; ++k) { zi = zi.sqr(); hz = hz * (Fr::one() + x[lg_n - k] * zi); }
            v = v + hz * alphas[i + 1];
        }
        return v;
    }
};

// :173  alpha = rho_1(hs): h_0 Some(poly), hs Vec<HPoly>, alpha None, alphas empty; then alpha^0 .. alpha^m
static void set_alphas(AccHPolys *hs) {
    const Fr *h0 = hs->h0;
    const size_t lg = hs->lg_n, m = hs->xis.size();
    Transcript t;
    size_t h0len = h0[1].is_zero() ? (h0[0].is_zero() ? 0 : 1) : 2;
    t.byte(1); t.u64le(h0len);
    for (size_t k = 0; k < h0len; ++k) t.scalar(h0[k]);
    t.u64le(m);
    for (size_t i = 0; i < m; ++i) { t.u64le(lg + 1); for (size_t k = 0; k <= lg; ++k) t.scalar(hs->xis[i][k]); }
    t.byte(0); t.u64le(0);
    hs->alpha = t.finish(1);
    hs->alphas.assign(m + 1, Fr::one());
    for (size_t i = 1; i <= m; ++i) hs->alphas[i] = hs->alphas[i - 1] * hs->alpha;
}
// :181  z = rho_1(C, alpha)
static Fr rho1_C_alpha(const Point &C, const Fr &alpha) {
    Transcript t; t.point(C); t.scalar(alpha); return t.finish(1);
}

// acc.rs:135-188
static int common_subroutine(halo_ctx *ctx, size_t d, const uint64_t *qs, size_t m, const Fr h0[2], const Point &U0, const Fr &w,
                             Point *C_bar_out, Fr *z_out, AccHPolys *hs) {
    if (!is_pow2(d + 1)) return fail_reject("d+1 is not a power of 2!");
    size_t lg = ilog2(d + 1), iw = instance_words(lg);
    hs->h0[0] = h0[0];
    hs->h0[1] = h0[1];
    hs->lg_n = lg;
    std::vector<Point> Us{U0};
    uint64_t h0w[8];
    h0[0].store(h0w);
    h0[1].store(h0w + 4);
    Point chk;
    int rc = pcdl_commit_host(ctx, h0w, 2, d, nullptr, &chk);  // :152-155
    if (rc) return rc;
    if (U0 != chk) return fail_reject("U_0 != PCDL.Commit(h_0)");
    // :158-170  the m succinct checks are independent host work (hashing + a 2 lg n + 1 point MSM
    // each): one thread per instance; errors are reported in instance order like the serial loop
    struct CheckResult { int rc = HALO_OK; std::string err; std::vector<Fr> xis; Point U; };
    std::vector<CheckResult> res(m);
    // The instances are laid out with the stride of degree d.  An instance that claims another degree (or whose
    // proof claims another length) would be read past its end: it is rejected here, before anything is parsed --
    // the reference fails on it too (acc.rs:169, after its typed, bounds-safe succinct check).
    for (size_t i = 0; i < m; ++i) {
        const uint64_t *q = qs + i * iw;
        if ((size_t)q[12] != d || q[22] != lg) return fail_reject("d_i != d");  // :169
    }
    auto run_one = [&](size_t i) {
        const uint64_t *q = qs + i * iw;
        res[i].rc = succinct_check_host(ctx, Point::load(q), (size_t)q[12], Fr::load(q + 13), Fr::load(q + 17), q + 21, &res[i].xis,
                                        &res[i].U);  // :164
        if (res[i].rc) res[i].err = halo_last_error();
    };
    if (m >= kBatchVerifyMin && ctx->batch_verify) {  // the relations of all instances in two launches
        std::vector<BatchCheck> bres;
        rc = succinct_check_batch(ctx, d, qs, m, bres);
        if (rc) return rc;
        for (size_t i = 0; i < m; ++i) {
            res[i].rc = bres[i].rc;
            res[i].err = std::move(bres[i].err);
            res[i].xis = std::move(bres[i].st.xis);
            res[i].U = bres[i].st.U;
        }
    } else if (m <= 1) {
        for (size_t i = 0; i < m; ++i) run_one(i);
    } else {  // a bounded pool: at most 16 host threads pull instances off a shared counter
        pool_run(m, run_one);
    }
    for (size_t i = 0; i < m; ++i) {
        if (res[i].rc) { set_error(res[i].err); return res[i].rc; }
        hs->xis.push_back(std::move(res[i].xis));
        Us.push_back(res[i].U);
    }
    set_alphas(hs);  // :173
    Point C = host::small_msm(Us, hs->alphas);  // :178  (m + 1 points)
    *z_out = rho1_C_alpha(C, hs->alpha);         // :181
    *C_bar_out = C + public_s_table().mul(w);   // :184
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

static int acc_verifier_batch_host(halo_ctx *ctx, size_t d, const uint64_t *qs, const size_t *counts, size_t k, const uint64_t *accs, int *status) {
    const size_t lg = ilog2(d + 1), iw = instance_words(lg), aw = acc_words(lg), K = 2 * lg + 2;
    if (K > kSegMaxTerms) { set_error("verifier_batch: lg n too large"); return HALO_E_ARG; }
    std::vector<VerifierMember> mem(k);
    size_t total = 0;
    for (size_t j = 0; j < k; ++j) { mem[j].first = total; mem[j].m = counts[j]; total += counts[j]; }
    // 0. what the single call checks before any arithmetic, and the sums' layout (sum_off: term offsets)
    std::vector<uint32_t> sum_off{0};
    auto add_sum = [&](size_t terms) { sum_off.push_back(sum_off.back() + (uint32_t)terms); return sum_off.size() - 2; };
    std::vector<size_t> rel_sum(total, 0), work;  // relation sum of each instance; the instances whose transcripts run
    const size_t u0_terms = d ? 2 : 1;            // (d = 0: h_0 is a constant, or the assert below)
    for (size_t j = 0; j < k; ++j) {
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
        M.s_u0 = add_sum(u0_terms);
        M.reach = true;
        for (size_t i = 0; i < M.m && M.reach; ++i) {
            const uint64_t *q = qs + (M.first + i) * iw;
            if ((size_t)q[12] != d || q[22] != lg) M.reach = false;  // :169
        }
        if (!M.reach) continue;
        for (size_t i = 0; i < M.m; ++i) {
            rel_sum[M.first + i] = add_sum(K);
            work.push_back(M.first + i);
        }
        M.n_c = (M.m + 1 + kSegMaxTerms - 1) / kSegMaxTerms;
        M.s_c = sum_off.size() - 1;
        for (size_t c = 0; c < M.n_c; ++c) add_sum(c + 1 < M.n_c ? kSegMaxTerms : M.m + 1 - c * kSegMaxTerms);
    }
    const size_t nsums = sum_off.size() - 1, nterms = sum_off.back();
    if (nterms >= ((size_t)1 << 31) || nsums >= ((size_t)1 << 28)) { set_error("verifier_batch: too many terms"); return HALO_E_ARG; }
    std::vector<uint64_t> pts(nterms * 8, 0), sc(nterms * 4, 0);
    // 1. the transcripts and the relations' terms
    std::vector<BatchCheck> res(total);
    pool_run(work.size(), [&](size_t w) {
        const size_t i = work[w];
        const uint64_t *q = qs + i * iw;
        BatchCheck &r = res[i];
        const Fr z = Fr::load(q + 13);
        r.rc = succinct_challenges(ctx, Point::load(q), d, z, Fr::load(q + 17), q + 21, &r.st, false);
        if (r.rc) { r.err = halo_last_error(); return; }
        const std::vector<Fr> &x = r.st.xis;  // h(z) as k_h_eval_z computes it (pcdl.rs:301-304)
        Fr hz = Fr::one() + x[lg] * z, zi = z;
        for (size_t t = 1; t < lg; ++t) { zi = zi.sqr(); hz = hz * (Fr::one() + x[lg - t] * zi); }
        const size_t o = sum_off[rel_sum[i]];
        relation_terms(r.st, q, hz, &pts[8 * o], &sc[4 * o]);
    });
    uint64_t g01[16] = {};  // G_0, G_1
    auto put_affine = [&](size_t t, const Point &p) {
        host::Affine a = p.to_affine();
        if (!a.inf) { a.x.store(&pts[8 * t]); a.y.store(&pts[8 * t + 4]); }
    };
    auto member_terms = [&](size_t j) {  // alpha, its powers, the terms of the U_0 check and of C
        VerifierMember &M = mem[j];
        const uint64_t *piV = accs + j * aw + iw;
        const size_t u = sum_off[M.s_u0];
        for (size_t t = 0; t < u0_terms; ++t) {
            std::memcpy(&pts[8 * (u + t)], g01 + 8 * t, 64);
            M.hs.h0[t].from_mont().store(&sc[4 * (u + t)]);
        }
        if (!M.reach) return;
        for (size_t i = 0; i < M.m; ++i)
            if (res[M.first + i].rc) return;
        M.all_ok = true;
        for (size_t i = 0; i < M.m; ++i) M.hs.xis.push_back(res[M.first + i].st.xis);
        set_alphas(&M.hs);
        const size_t c0 = sum_off[M.s_c];  // the parts of C are consecutive: term t of C is term c0 + t
        for (size_t t = 0; t <= M.m; ++t) {
            put_affine(c0 + t, t ? res[M.first + t - 1].st.U : Point::load(piV + 8));
            M.hs.alphas[t].from_mont().store(&sc[4 * (c0 + t)]);
        }
    };
    // 2. every sum: on the device in one launch, or on the host pool
    std::vector<Point> sums(nsums, Point::infinity());
    int slot = -1;
    for (int s = 0; s < HALO_SLOTS && slot < 0; ++s)
        if (!ctx->wss[s].in_flight && ctx->wss[s].lent_from < 0 && !ctx->fan[s].active) slot = s;
    std::vector<uint32_t> desc;
    const size_t waves = small_msm_seg_plan(sum_off.data(), nsums, desc);
    // staging (bytes): points nterms x 64 | scalars nterms x 32 | results nsums x 96 | sum_off (nsums + 1) x 4 | desc waves x 256
    const size_t bytes = nterms * 96 + nsums * 96 + (nsums + 1) * 4 + desc.size() * 4;
    const int forced = dev_hooks().verifier_min;  // (development library: the threshold sweep of tools/time_verifier_batch.py)
    const size_t min_rel = forced >= 1 ? (size_t)forced : kVerifierBatchMin;
    const bool device = slot >= 0 && ctx->batch_verify && work.size() >= min_rel && check_stage(ctx, 1, bytes) >= 1;
    hipStream_t saved = ctx->stream;
    if (device) ctx->stream = ctx->streams[slot];  // (the launch macro and the reads below use ctx->stream: the slot's own)
    int rc = nsums ? halo_ctx_read_bases(ctx, 0, u0_terms, g01) : HALO_OK;
    if (!rc) pool_run(k, [&](size_t j) { if (mem[j].sums) member_terms(j); });
    if (!rc && device) {
        uint64_t *d_pts = ctx->d_check_stage, *d_sc = d_pts + nterms * 8, *d_out = d_sc + nterms * 4;
        uint32_t *d_off = reinterpret_cast<uint32_t *>(d_out + nsums * 12), *d_desc = d_off + nsums + 1;
        hipError_t e = hipMemcpyAsync(d_pts, pts.data(), nterms * 64, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_sc, sc.data(), nterms * 32, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_off, sum_off.data(), (nsums + 1) * 4, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_desc, desc.data(), desc.size() * 4, hipMemcpyHostToDevice, ctx->stream);
        rc = e == hipSuccess ? small_msm_seg(ctx, d_pts, d_sc, d_off, d_desc, waves, d_out) : hip_fail(e, "hipMemcpyAsync");
        std::vector<uint64_t> out(nsums * 12);
        if (!rc && (e = hipMemcpyAsync(out.data(), d_out, nsums * 96, hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess) rc = hip_fail(e, "hipMemcpyAsync");
        if (!rc && (e = hipStreamSynchronize(ctx->stream)) != hipSuccess) rc = hip_fail(e, "hipStreamSynchronize");
        if (!rc)
            for (size_t s = 0; s < nsums; ++s) sums[s] = Point::load(&out[12 * s]);
    } else if (!rc) {
        pool_run(nsums, [&](size_t s) {
            const size_t lo = sum_off[s], len = sum_off[s + 1] - lo;
            std::vector<Point> p(len);
            std::vector<Fr> kk(len);
            for (size_t t = 0; t < len; ++t) { p[t] = Point::load_affine(&pts[8 * (lo + t)]); kk[t] = Fr::load(&sc[4 * (lo + t)]).to_mont(); }
            sums[s] = host::small_msm(p, kk);
        });
    }
    ctx->stream = saved;
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
    int first = -1;
    for (size_t j = 0; j < k; ++j) {
        if (status) status[j] = mem[j].rc;
        if (mem[j].rc && first < 0) first = (int)j;
    }
    if (first >= 0) { set_error("member " + std::to_string(first) + ": " + mem[first].err); return mem[first].rc; }
    return HALO_OK;
}

}  // namespace halo

using namespace halo;

// the body of halo_pcdl_open after its argument checks (deg = host_poly_degree(coeffs) <= d)
static int pcdl_open_host(halo_ctx *ctx, uint64_t *rng_state, const uint64_t *coeffs, size_t deg, const uint64_t C[12], size_t d, const uint64_t z[4],
                          const uint64_t *w, uint64_t *proof_out) {
    int rc = ensure_poly_buffers(ctx);
    if (rc) return rc;
    HALO_HIP(hipMemsetAsync(ctx->d_poly, 0, (d + 1) * 32, ctx->stream));
    rc = upload_words(ctx, ctx->d_poly, coeffs, (deg + 1) * 4);
    if (rc) return rc;
    host::Rng rng{rng_state ? *rng_state : 0};
    Fr wf = w ? Fr::load(w) : Fr::zero();
    rc = pcdl_open_dev(ctx, &rng, deg, Point::load(C), d, Fr::load(z), w ? &wf : nullptr, proof_out);
    if (rng_state) *rng_state = rng.state;
    return rc;
}

// the body of halo_random_instance after its argument checks
static int random_instance_one(halo_ctx *ctx, uint64_t *rng_state, size_t d, uint64_t *inst) {
    size_t lg = ilog2(d + 1), n = d + 1;
    host::Rng rng{rng_state ? *rng_state : 0};
    size_t lo = d / 2, d_prime = lo + (size_t)(rng.next() % (uint64_t)(d - lo));
    if (d_prime == 0) d_prime = 1;
    Fr w = rng.scalar();
    int rc = ensure_poly_buffers(ctx);
    if (rc) return rc;
    // p = PallasPoly::rand(d_prime): d_prime + 1 scalars of the stream, generated on the device
    HALO_HIP(hipMemsetAsync(ctx->d_poly, 0, n * 32, ctx->stream));
    rc = rng_scalars_dev(ctx, rng.state, d_prime + 1, ctx->d_poly);
    if (rc) return rc;
    rng.state += 4 * (uint64_t)(d_prime + 1) * 0x9E3779B97F4A7C15ULL;
    Point C;
    rc = pedersen_commit_dev(ctx, &w, ctx->d_poly, n, &C);
    if (rc) return rc;
    C = C.normalized();
    Fr z = rng.scalar(), v;
    rc = fr_poly_eval(ctx, ctx->d_poly, d_prime + 1, z, &v);
    if (rc) return rc;
    std::memset(inst, 0, 8 * instance_words(lg));
    C.store(inst);
    inst[12] = d;
    z.store(inst + 13);
    v.store(inst + 17);
    // the leading coefficient is non-zero with overwhelming probability: degree = d_prime
    rc = pcdl_open_dev(ctx, &rng, d_prime, C, d, z, &w, inst + 21);
    if (rng_state) *rng_state = rng.state;
    return rc;
}

// ------------------------------------------------------------------ pcdl::open of m polynomials at once
// The randomness of every member is known before any device work: the counter-based stream's draws depend only on the members'
// degrees (a hiding open draws deg scalars for q, then w_bar; random_instance draws d', w, the d' + 1 coefficients, z, then the
// open's draws).  So the host computes every member's start state first, and the members run side by side.
//
// Device path (2 <= n <= the context's no-fold size, at most OPEN_MAX_N): the open in its no-fold form (abi.hip ipa_round_lr_points:
// the key is never folded, every round's L and R are two MSMs over the same n points with expanded scalars) for a GROUP of up to
// OPEN_MAX_GROUP members at a time.  Each step of a group is one set of member-batched launches (ipa.hip *_batch, blockIdx.y =
// member) and ONE batched MSM launch sequence over the key (L and R of every member: up to 8 scalar arrays; the C_bar commits of the
// hiding branch, and random_instance's commits, likewise).  Groups rotate over the slots that were idle on entry: while this
// thread waits for one group's step and runs its host half -- window combines, H' terms, Fiat-Shamir hashes, xi^-1, on the host
// pool for the group's members -- the other slots' groups run on the device.  Every group runs through all its rounds before
// its slot takes the next one, so the staging holds G x S members.  Host arithmetic is the single open's, term for term
// (pcdl_open_dev, halo_ipa_finish's last-round U), so every proof word is the one halo_pcdl_open writes.
struct OpenJob {
    size_t idx = 0, deg = 0;
    uint64_t s_start = 0;                // rng state before the member's first draw (the single call's *rng_state)
    uint64_t s_p = 0, s_q = 0;           // rng state before p's coefficients (random_instance) / before q's (hiding)
    const uint64_t *coeffs = nullptr;    // the caller's n coefficients (null: p generated or accumulated on the device)
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
    const int forced = dev_hooks().open_group;  // (development library: the sweep of tools/time_open_batch.py)
    int g = forced >= 1 && forced <= OPEN_MAX_GROUP ? forced : OPEN_MAX_GROUP;
    MsmPlan p = msm_plan(n, ctx->window_bits);
    while (g > 1 && (size_t)p.W * (size_t)(2 * g) * p.B > ((size_t)1 << 22)) --g;
    return (size_t)g;
}
constexpr size_t OPEN_AUX_WORDS = OPEN_MAX_GROUP * (OPEN_TAB_WORDS + OPEN_CONST_WORDS + OPEN_PART_WORDS + OPEN_OUT_WORDS);
// (the prover batch's third coefficient source: up to HACC_TABLES polynomials h_i per pass of a group, see h_accumulate_group)
constexpr size_t HACC_TABLES = 32;
constexpr size_t HACC_PIN_WORDS = OPEN_MAX_GROUP * HACC_REC_WORDS + HACC_TABLES * (16 + 2) * 4;  // lg n <= 16 (OPEN_MAX_N)
constexpr size_t OPEN_PIN_WORDS = OPEN_MAX_GROUP * (OPEN_TAB_WORDS + OPEN_CONST_WORDS + OPEN_OUT_WORDS) + HACC_PIN_WORDS + 4;  // per slot; + the element one

// jobs: the members that do not fail up front, in member order.  *ran = false: the device path does not apply (nothing done)
// Coefficients of a member: the caller's host array (jb.coeffs), generated on the device (gen), or -- jb.hs set, for every member
// alike -- acc::prover's h(X) accumulated on the device straight into the member's coefficient vector
static int open_batch_dev(halo_ctx *ctx, size_t d, std::vector<OpenJob> &jobs, bool gen, const int *slots_in, int S, bool *ran) {
    *ran = false;
    const size_t n = d + 1, lg = ilog2(n), A = jobs.size();
    if (A == 0 || n < 2 || n > ctx->nofold_size || n > OPEN_MAX_N) return HALO_OK;
    size_t G = open_group_size(ctx, n);
    if (G > A) G = A;
    size_t ng = (A + G - 1) / G;
    if ((size_t)S > ng) S = (int)ng;
    const size_t ms = 7 * 4 * n;  // words of one member's vectors: c | z | s | s' | F_L | F_R | p_bar
    const bool accumulated = jobs[0].hs != nullptr;
    const size_t hacc_words = accumulated ? hacc_stage_words(OPEN_MAX_GROUP, lg, HACC_TABLES) : 0;
    const size_t per = G * ms + OPEN_AUX_WORDS + hacc_words;  // words of one slot's group
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
    const bool hiding = jobs[0].hiding;  // (the same for every member of a batch)
    const bool u_from_last_round = tuning().u_from_last_round;
    struct Flight { long g = -1; size_t first = 0, cnt = 0, step = 0; int msm = 0; bool flip = false; std::vector<size_t> need_u; };
    std::vector<Flight> fl(S);
    // slot j's regions: the group's member vectors, then its window tables | constants | partial sums | results; in pinned memory
    // the tables | constants (one upload) | results (one download) | the element one
    auto dev = [&](int j) { return ctx->d_check_stage + (size_t)j * per; };
    auto vec = [&](int j, int k) { return dev(j) + 4 * n * (size_t)k; };  // member 0's vector k; member b at + b * ms
    auto aux = [&](int j) { return dev(j) + G * ms; };
    auto d_tabs = [&](int j) { return aux(j); };
    auto d_consts = [&](int j) { return aux(j) + OPEN_MAX_GROUP * OPEN_TAB_WORDS; };
    auto d_parts = [&](int j) { return d_consts(j) + OPEN_MAX_GROUP * OPEN_CONST_WORDS; };
    auto d_outs = [&](int j) { return d_parts(j) + OPEN_MAX_GROUP * OPEN_PART_WORDS; };
    auto h_tabs = [&](int j) { return ctx->h_open_pinned + (size_t)j * OPEN_PIN_WORDS; };
    auto h_consts = [&](int j) { return (OpenConst *)(h_tabs(j) + OPEN_MAX_GROUP * OPEN_TAB_WORDS); };
    auto h_outs = [&](int j) { return h_tabs(j) + OPEN_MAX_GROUP * (OPEN_TAB_WORDS + OPEN_CONST_WORDS); };
    auto h_one = [&](int j) { return h_tabs(j) + OPEN_PIN_WORDS - 4; };
    auto d_hacc = [&](int j) { return d_outs(j) + OPEN_MAX_GROUP * OPEN_OUT_WORDS; };
    auto h_hacc = [&](int j) { return h_outs(j) + OPEN_MAX_GROUP * OPEN_OUT_WORDS; };
    auto out_of = [&](int j, size_t b) { return h_outs(j) + OPEN_OUT_WORDS * b; };
    auto s_cur = [&](int j) { return vec(j, fl[j].flip ? 3 : 2); };
    // the launches of one step of slot j's group on the slot's stream (the launch macro uses ctx->stream)
    auto on_slot = [&](int j, const std::function<int(hipStream_t)> &body) -> int {
        hipStream_t saved = ctx->stream;
        ctx->stream = ctx->streams[slots_in[j]];
        int rc = body(ctx->stream);
        ctx->stream = saved;
        return rc;
    };
    auto msm_out = [&](int j, int count, const std::function<const uint64_t *(int)> &scalars) -> int {
        MsmBatch mb;
        mb.count = count;
        for (int k = 0; k < count; ++k) mb.scalars[k] = scalars(k);
        int rc = msm_enqueue_batch(ctx, slots_in[j], ctx->d_bases, mb, true, n);
        if (!rc) fl[j].msm = count;
        return rc;
    };
    auto download_outs = [&](int j, hipStream_t st) -> int {
        HALO_HIP(hipMemcpyAsync(h_outs(j), d_outs(j), fl[j].cnt * OPEN_OUT_WORDS * 8, hipMemcpyDeviceToHost, st));
        return HALO_OK;
    };
    auto upload_consts = [&](int j, hipStream_t st) -> int {
        HALO_HIP(hipMemcpyAsync(d_consts(j), h_consts(j), fl[j].cnt * OPEN_CONST_WORDS * 8, hipMemcpyHostToDevice, st));
        return HALO_OK;
    };
    // round r of slot j's group: F_L, F_R from c and s, the dot products, L and R of every member as one batched MSM
    auto enqueue_round = [&](int j, size_t r) -> int {
        Flight &f = fl[j];
        const size_t mcur = n >> r;
        int rc = on_slot(j, [&](hipStream_t st) -> int {
            int rc2 = open_batch_expand(ctx, (int)f.cnt, vec(j, 0), s_cur(j), ms, mcur, n, vec(j, 4), vec(j, 5));
            if (!rc2) rc2 = open_batch_dots(ctx, (int)f.cnt, vec(j, 0), vec(j, 1), ms, mcur / 2, d_parts(j), d_outs(j));
            if (rc2) return rc2;
            if (mcur == 2)  // the last round: c0, c1 travel with its results (halo_ipa_finish's U from this round's MSMs)
                for (size_t b = 0; b < f.cnt; ++b)
                    HALO_HIP(hipMemcpyAsync(d_outs(j) + OPEN_OUT_WORDS * b + 12, vec(j, 0) + b * ms, 64, hipMemcpyDeviceToDevice, st));
            return download_outs(j, st);
        });
        if (!rc) rc = msm_out(j, 2 * (int)f.cnt, [&](int k) { return vec(j, 4 + (k & 1)) + (size_t)(k >> 1) * ms; });
        f.step = 1 + r;
        return rc;
    };
    // step 0: coefficients (copied, or generated), p(z), the powers of z, p_bar; the commits as one batched MSM
    auto start = [&](int j, size_t g) -> int {
        Flight &f = fl[j];
        f.g = (long)g;
        f.first = g * G;
        f.cnt = A - f.first < G ? A - f.first : G;
        f.step = 0;
        f.msm = 0;
        f.flip = false;
        for (size_t b = 0; b < f.cnt; ++b) {
            const OpenJob &jb = jobs[f.first + b];
            OpenConst &k = h_consts(j)[b];
            std::memset(&k, 0, sizeof k);
            int rc = open_batch_table(jb.z, n, h_tabs(j) + OPEN_TAB_WORDS * b, &k);
            if (rc) return rc;
            k.s_q = jb.s_q;
            k.s_p = jb.s_p;
            k.deg = (uint32_t)jb.deg;
            k.len = (uint32_t)(jb.deg + 1);
        }
        int rc = on_slot(j, [&](hipStream_t st) -> int {
            HALO_HIP(hipMemcpyAsync(d_tabs(j), h_tabs(j), OPEN_MAX_GROUP * (OPEN_TAB_WORDS + OPEN_CONST_WORDS) * 8, hipMemcpyHostToDevice, st));
            int rc2 = HALO_OK;
            if (gen) rc2 = open_batch_rng(ctx, (int)f.cnt, d_consts(j), n, vec(j, 0), ms);  // p = PallasPoly::rand(d')
            else if (accumulated) {  // p = h.get_poly() (acc.rs:85-94)
                HAccMember hm[OPEN_MAX_GROUP];
                for (size_t b = 0; b < f.cnt; ++b) {
                    const AccHPolys &hs = *jobs[f.first + b].hs;
                    hm[b].h0 = hs.h0;
                    hm[b].count = hs.xis.size();
                    hm[b].scales = hs.alphas.data() + 1;
                    for (const std::vector<Fr> &x : hs.xis) hm[b].xis.push_back(x.data());
                }
                rc2 = h_accumulate_group(ctx, hm, f.cnt, lg, HACC_TABLES, h_hacc(j), d_hacc(j), vec(j, 0), ms);
            } else
                for (size_t b = 0; b < f.cnt; ++b)
                    HALO_HIP(hipMemcpyAsync(vec(j, 0) + b * ms, jobs[f.first + b].coeffs, n * 32, hipMemcpyHostToDevice, st));
            if (!rc2) rc2 = open_batch_eval(ctx, (int)f.cnt, vec(j, 0), ms, n, d_tabs(j), d_parts(j), d_outs(j));  // :135
            if (!rc2) rc2 = open_batch_powers(ctx, (int)f.cnt, d_tabs(j), d_consts(j), n, vec(j, 1), ms);
            if (!rc2 && hiding) rc2 = open_batch_pbar(ctx, (int)f.cnt, d_consts(j), n, vec(j, 6), ms);  // :140-142
            for (size_t b = 0; b < f.cnt && !rc2; ++b)  // s = (1)
                HALO_HIP(hipMemcpyAsync(vec(j, 2) + b * ms, h_one(j), 32, hipMemcpyHostToDevice, st));
            if (!rc2) rc2 = download_outs(j, st);
            return rc2;
        });
        const int commits = (gen ? (int)f.cnt : 0) + (hiding ? (int)f.cnt : 0);  // random_instance's C, then C_bar (:150)
        if (!rc && commits)
            rc = msm_out(j, commits, [&](int k) { return (gen && (size_t)k < f.cnt) ? vec(j, 0) + (size_t)k * ms : vec(j, 6) + (k % f.cnt) * ms; });
        return rc;
    };
    // slot j's step is done: its results through the host half, then the next step (or the group is through)
    auto advance = [&](int j, bool *through) -> int {
        Flight &f = fl[j];
        *through = false;
        Point pts[MSM_MAX_BATCH];
        if (f.msm) {
            int rc = msm_finish_batch(ctx, slots_in[j], pts, f.msm);
            f.msm = 0;
            if (rc) return rc;
        }
        HALO_HIP(hipStreamSynchronize(ctx->streams[slots_in[j]]));
        if (f.step == 0) {
            pool_run(f.cnt, [&](size_t b) {
                OpenJob &jb = jobs[f.first + b];
                jb.v = Fr::load(out_of(j, b));
                if (gen) jb.C = (public_s_table().mul(jb.w) + pts[b]).normalized();
                Point C_prime = jb.C;
                if (hiding) {
                    Point C_bar = public_s_table().mul(jb.w_bar) + pts[(gen ? f.cnt : 0) + b];
                    Fr a = rho0_C_z_v_Cbar(jb.C, jb.z, jb.v, C_bar);  // :153
                    Fr w_prime = jb.w_bar * a + jb.w;                  // :159
                    C_prime = jb.C + C_bar.mul(a) - public_s_table().mul(w_prime);  // :162
                    jb.proof[0] = 1;
                    C_bar.store_normalized(pf_Cbar(jb.proof, lg));
                    w_prime.store(pf_wp(jb.proof, lg));
                    open_const_alpha(&h_consts(j)[b], a);
                } else {
                    Point::infinity().store(pf_Cbar(jb.proof, lg));
                }
                jb.xi0 = jb.xi = rho0_C_z_v(C_prime, jb.z, jb.v);  // :180
            });
            int rc = HALO_OK;
            if (hiding)
                rc = on_slot(j, [&](hipStream_t st) -> int {
                    int rc2 = upload_consts(j, st);
                    return rc2 ? rc2 : open_batch_axpy(ctx, (int)f.cnt, vec(j, 0), vec(j, 6), ms, n, d_consts(j));  // :156
                });
            return rc ? rc : enqueue_round(j, 0);
        }
        if (f.step <= lg) {  // round r = step - 1 (:203-224)
            const size_t r = f.step - 1;
            const bool last = r + 1 == lg;
            pool_run(f.cnt, [&](size_t b) {
                OpenJob &jb = jobs[f.first + b];
                const uint64_t *o = out_of(j, b);
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
                open_const_xi(&h_consts(j)[b], xi_next, xi_inv);
            });
            int rc = on_slot(j, [&](hipStream_t st) -> int {  // :216-224
                int rc2 = upload_consts(j, st);
                const uint64_t *s_in = s_cur(j);
                f.flip = !f.flip;
                return rc2 ? rc2 : open_batch_fold(ctx, (int)f.cnt, vec(j, 0), vec(j, 1), s_in, s_cur(j), ms, n >> (r + 1), (size_t)1 << r, d_consts(j));
            });
            if (rc) return rc;
            if (!last) return enqueue_round(j, r + 1);
            // :230-231 as halo_ipa_finish: U from the last round's MSMs where both coefficients are non-zero, else U = <s, G>
            f.need_u.clear();
            pool_run(f.cnt, [&](size_t b) {
                OpenJob &jb = jobs[f.first + b];
                if (!(u_from_last_round && !jb.c0.is_zero() && !jb.c1.is_zero())) return;
                Fr inv01 = (jb.c0 * jb.c1).inv();
                Fr a = inv01 * jb.c0, bb = inv01 * jb.c1 * jb.last_xi;  // 1 / c1, xi / c0
                (jb.last_L.mul(a) + jb.last_R.mul(bb)).store_normalized(pf_U(jb.proof, lg));
                (jb.c0 + jb.last_xi_inv * jb.c1).store(pf_c(jb.proof, lg));
            });
            for (size_t b = 0; b < f.cnt; ++b) {
                const OpenJob &jb = jobs[f.first + b];
                if (!(u_from_last_round && !jb.c0.is_zero() && !jb.c1.is_zero())) f.need_u.push_back(b);
            }
            if (f.need_u.empty()) { *through = true; return HALO_OK; }
            rc = on_slot(j, [&](hipStream_t st) -> int {
                for (size_t k = 0; k < f.need_u.size(); ++k)
                    HALO_HIP(hipMemcpyAsync(d_outs(j) + OPEN_OUT_WORDS * f.need_u[k] + 20, vec(j, 0) + f.need_u[k] * ms, 32, hipMemcpyDeviceToDevice, st));
                return download_outs(j, st);
            });
            if (!rc) rc = msm_out(j, (int)f.need_u.size(), [&](int k) { return s_cur(j) + f.need_u[(size_t)k] * ms; });
            f.step = lg + 1;
            return rc;
        }
        for (size_t k = 0; k < f.need_u.size(); ++k) {  // U = <s, G> and c = c[0] (halo_ipa_finish)
            OpenJob &jb = jobs[f.first + f.need_u[k]];
            pts[k].store_normalized(pf_U(jb.proof, lg));
            std::memcpy(pf_c(jb.proof, lg), out_of(j, f.need_u[k]) + 20, 32);
        }
        *through = true;
        return HALO_OK;
    };
    auto abandon = [&]() {  // (a device error: nothing of this call stays in flight)
        std::string err = halo_last_error();
        for (int j = 0; j < S; ++j) {
            if (fl[j].msm) {
                Point pts[MSM_MAX_BATCH];
                (void)msm_finish_batch(ctx, slots_in[j], pts, fl[j].msm);
                fl[j].msm = 0;
            }
            (void)hipStreamSynchronize(ctx->streams[slots_in[j]]);
        }
        set_error(err);
    };
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
    if (rc) { abandon(); return rc; }
    return HALO_OK;
}

// halo_pcdl_open_batch (coeffs != null) and halo_random_instance_batch (coeffs == null: `out` holds Instance blobs) after their
// argument checks: the members' draws, then the device path or, where it does not apply, the members one at a time
static int open_batch_entry(halo_ctx *ctx, uint64_t *rng_state, size_t d, const uint64_t *coeffs, size_t m, const uint64_t *Cs, const uint64_t *zs,
                            const uint64_t *ws, uint64_t *out, int *status) {
    const size_t n = d + 1, lg = ilog2(n);
    const bool gen = coeffs == nullptr, hiding = gen || ws != nullptr;
    const size_t stride = gen ? instance_words(lg) : proof_words(lg);
    constexpr uint64_t GAMMA = 0x9E3779B97F4A7C15ULL;
    int slots[HALO_SLOTS], S = 0;
    for (int k = 0; k < HALO_SLOTS; ++k)
        if (!ctx->wss[k].in_flight && ctx->wss[k].lent_from < 0 && !ctx->fan[k].active) slots[S++] = k;
    if (!S) { set_error("open_batch: every slot has an MSM in flight"); return HALO_E_ARG; }
    // 1. every member's draws, in member order (the loop's order)
    host::Rng rng{rng_state ? *rng_state : 0};
    std::vector<OpenJob> jobs;
    std::vector<int> pre(m, HALO_OK);  // members that fail before any draw (a hiding open of a constant polynomial)
    jobs.reserve(m);
    for (size_t i = 0; i < m; ++i) {
        OpenJob jb;
        jb.idx = i;
        jb.hiding = hiding;
        jb.proof = out + i * stride + (gen ? 21 : 0);
        jb.s_start = rng.state;
        if (gen) {
            size_t lo = d / 2;
            jb.deg = lo + (size_t)(rng.next() % (uint64_t)(d - lo));
            if (jb.deg == 0) jb.deg = 1;
            jb.w = rng.scalar();
            jb.s_p = rng.state;
            rng.state += 4 * (uint64_t)(jb.deg + 1) * GAMMA;
            jb.z = rng.scalar();
        } else {
            jb.coeffs = coeffs + i * n * 4;
            jb.deg = host_poly_degree(jb.coeffs, n);
            jb.C = Point::load(Cs + 12 * i);
            jb.z = Fr::load(zs + 4 * i);
            if (ws) jb.w = Fr::load(ws + 4 * i);
            if (hiding && jb.deg == 0) { pre[i] = HALO_E_ASSERT; continue; }  // pcdl_open_dev: before any draw
        }
        if (hiding) {
            jb.s_q = rng.state;
            rng.state += 4 * (uint64_t)jb.deg * GAMMA;
            jb.w_bar = rng.scalar();
        }
        jobs.push_back(jb);
    }
    // 2. the device path; where it does not apply, the loop itself (the single calls' bodies, from the same states)
    bool ran = false;
    int rc = HALO_OK;
    if (!jobs.empty()) {
        for (OpenJob &jb : jobs) {
            std::memset(jb.proof, 0, 8 * proof_words(lg));
            jb.proof[1] = lg;
        }
        rc = open_batch_dev(ctx, d, jobs, gen, slots, S, &ran);
        if (rc) return rc;
    }
    if (!ran) {
        for (OpenJob &jb : jobs) {
            uint64_t st = jb.s_start;
            if (gen) rc = random_instance_one(ctx, &st, d, out + jb.idx * stride);
            else rc = pcdl_open_host(ctx, &st, jb.coeffs, jb.deg, Cs + 12 * jb.idx, d, zs + 4 * jb.idx, ws ? ws + 4 * jb.idx : nullptr, jb.proof);
            if (rc == HALO_E_ASSERT) { jb.rc = rc; jb.err = halo_last_error(); }
            else if (rc) return rc;
        }
    }
    // 3. outcomes in member order
    std::vector<int> codes(pre);
    std::vector<std::string> errs(m);
    for (size_t i = 0; i < m; ++i)
        if (pre[i]) errs[i] = "open: hiding needs p.degree() >= 1";
    for (OpenJob &jb : jobs) {
        codes[jb.idx] = jb.rc;
        errs[jb.idx] = jb.err;
        if (gen && !jb.rc && ran) {  // the Instance around the proof (random_instance_one writes its own)
            uint64_t *inst = out + jb.idx * stride;
            jb.C.store(inst);
            inst[12] = d;
            jb.z.store(inst + 13);
            jb.v.store(inst + 17);
        }
    }
    int first = -1;
    for (size_t i = 0; i < m; ++i) {
        if (codes[i]) {
            std::memset(out + i * stride, 0, 8 * stride);
            if (first < 0) first = (int)i;
        }
        if (status) status[i] = codes[i];
    }
    if (rng_state) *rng_state = rng.state;
    if (first >= 0) { set_error("member " + std::to_string(first) + ": " + errs[first]); return codes[first]; }
    return HALO_OK;
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
//     into the open's staging (h_accumulate_group), groups of up to 4 members over the idle slots.
//  5. the blobs: C_bar | d | z | v | proof | h_0 | U_0 | omega.
// *ran = false: the device form does not apply (size, staging) and nothing was written.
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
    constexpr uint64_t GAMMA = 0x9E3779B97F4A7C15ULL;
    if (n < 2 || n > ctx->nofold_size || n > OPEN_MAX_N) return HALO_OK;
    std::vector<ProverMember> mem(k);
    size_t total = 0;
    for (size_t j = 0; j < k; ++j) { mem[j].first = total; mem[j].m = counts[j]; total += counts[j]; }
    // 1. the succinct half
    bool all_reach = true;
    for (size_t j = 0; j < k; ++j)
        for (size_t i = 0; i < mem[j].m && !mem[j].rc; ++i) {
            const uint64_t *q = qs + (mem[j].first + i) * iw;
            if ((size_t)q[12] != d || q[22] != lg) { mem[j].rc = HALO_E_REJECT; mem[j].err = "d_i != d"; all_reach = false; }  // :169
        }
    std::vector<size_t> work;  // the instances whose checks run, and where their results go
    for (size_t j = 0; j < k; ++j)
        if (!mem[j].rc)
            for (size_t i = 0; i < mem[j].m; ++i) work.push_back(mem[j].first + i);
    std::vector<BatchCheck> res;
    if (work.size() >= kBatchVerifyMin && ctx->batch_verify) {
        std::vector<uint64_t> packed;  // (members that never reach their checks are left out: the rest, contiguous)
        if (!all_reach) {
            packed.resize(work.size() * iw);
            for (size_t w = 0; w < work.size(); ++w) std::memcpy(&packed[w * iw], qs + work[w] * iw, iw * 8);
        }
        int rc = succinct_check_batch(ctx, d, all_reach ? qs : packed.data(), work.size(), res);
        if (rc) return rc;
    } else {
        res.assign(work.size(), BatchCheck());
        pool_run(work.size(), [&](size_t w) {
            const uint64_t *q = qs + work[w] * iw;
            res[w].rc = succinct_challenges(ctx, Point::load(q), d, Fr::load(q + 13), Fr::load(q + 17), q + 21, &res[w].st);
            if (!res[w].rc) res[w].rc = succinct_relation(res[w].st, Fr::load(q + 13), Fr::load(q + 17), q + 21);
            if (res[w].rc) res[w].err = halo_last_error();
        });
    }
    {
        size_t w = 0;
        for (size_t j = 0; j < k; ++j) {
            ProverMember &M = mem[j];
            if (M.rc) continue;
            M.r0 = w;
            for (size_t i = 0; i < M.m; ++i, ++w) {
                if (res[w].rc && !M.rc) { M.rc = res[w].rc; M.err = res[w].err; }  // :158-170 in instance order
                if (!M.rc) M.hs.xis.push_back(res[w].st.xis);
            }
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
        rng.state += 4 * (uint64_t)jb.deg * GAMMA;
        jb.w_bar = rng.scalar();
        jb.proof = accs + j * aw + 21;
        jobs.push_back(jb);
    }
    // 3. U_0, alpha, C, z, C_bar, v
    if (!jobs.empty()) {
        uint64_t g01[16];
        int rc = halo_ctx_read_bases(ctx, 0, 2, g01);
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
        rc = open_batch_dev(ctx, d, jobs, false, slots, S, ran);
        if (rc) return rc;
        if (!*ran) return HALO_OK;
    }
    *ran = true;
    // 5. the blobs and the outcomes
    for (OpenJob &jb : jobs) {
        ProverMember &M = mem[jb.idx];
        if (jb.rc) { M.rc = jb.rc; M.err = jb.err; continue; }
        uint64_t *acc = accs + jb.idx * aw, *piV = acc + iw;
        M.C_bar.store(acc);
        acc[12] = d;
        M.z.store(acc + 13);
        M.v.store(acc + 17);
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
    int slots[HALO_SLOTS], S = 0;
    for (int s = 0; s < HALO_SLOTS; ++s)
        if (!ctx->wss[s].in_flight && ctx->wss[s].lent_from < 0 && !ctx->fan[s].active) slots[S++] = s;
    if (!S) { set_error("prover_batch: every slot has an MSM in flight"); return HALO_E_ARG; }
    std::vector<int> codes(k, HALO_OK);
    std::vector<std::string> errs(k);
    uint64_t state = rng_state ? *rng_state : 0;
    bool ran = false;
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
    int first_bad = -1;
    for (size_t j = 0; j < k; ++j) {
        if (codes[j]) {
            std::memset(accs + j * aw, 0, 8 * aw);
            if (first_bad < 0) first_bad = (int)j;
        }
        if (status) status[j] = codes[j];
    }
    if (rng_state) *rng_state = state;
    if (first_bad >= 0) { set_error("member " + std::to_string(first_bad) + ": " + errs[first_bad]); return codes[first_bad]; }
    return HALO_OK;
}

#define HALO_CTX2(ctx)                                                   \
    do {                                                                 \
        if (!(ctx)) { halo::set_error("null context"); return HALO_E_ARG; } \
        hipError_t _e = hipSetDevice((ctx)->device);                     \
        if (_e != hipSuccess) return halo::hip_fail(_e, "hipSetDevice"); \
    } while (0)

extern "C" {

size_t halo_proof_words(size_t lg_n) { return proof_words(lg_n); }
size_t halo_instance_words(size_t lg_n) { return instance_words(lg_n); }
size_t halo_accumulator_words(size_t lg_n) { return acc_words(lg_n); }

int halo_pedersen_commit(halo_ctx *ctx, const uint64_t *w, size_t n_bases, const uint64_t *ms, size_t n_ms, uint64_t out[12]) {
    HALO_CTX2(ctx);
    if (n_bases != n_ms) return fail_assert("Length did not match for pedersen commitment");  // pedersen.rs:7-12
    if (n_bases > ctx->n) return fail_assert("pedersen commit: more bases than the key holds");
    if (!out || (n_ms && !ms)) { set_error("pedersen commit: null pointer"); return HALO_E_ARG; }
    // pedersen.rs:14-17 with the scalars in host memory: the host-scalar MSM path of halo_msm (abi.hip msm_host_run)
    Point r;
    int rc = msm_host_run(ctx, 0, n_ms, ms, n_ms, 1, &r);
    if (rc) return rc;
    if (w) r = public_s_table().mul(Fr::load(w)) + r;
    r.store_normalized(out);
    return HALO_OK;
}

int halo_pedersen_commit_affine(halo_ctx *ctx, const uint64_t *w, const uint64_t *bases_affine, size_t n_bases, const uint64_t *ms,
                                size_t n_ms, uint64_t out[12]) {
    HALO_CTX2(ctx);
    if (n_bases != n_ms) return fail_assert("Length did not match for pedersen commitment");  // pedersen.rs:7-12
    uint64_t acc_w[12];
    int rc = halo_msm_affine(ctx, bases_affine, ms, n_ms, 1, acc_w);  // pedersen.rs:14 over the caller's generators
    if (rc) return rc;
    Point acc = Point::load(acc_w);
    if (w) acc = public_s_table().mul(Fr::load(w)) + acc;  // pedersen.rs:15-17
    acc.store_normalized(out);
    return HALO_OK;
}

int halo_pcdl_commit(halo_ctx *ctx, const uint64_t *coeffs, size_t len, size_t d, const uint64_t *w, uint64_t out[12]) {
    HALO_CTX2(ctx);
    Fr wf = w ? Fr::load(w) : Fr::zero();
    Point r;
    int rc = pcdl_commit_host(ctx, coeffs, len, d, w ? &wf : nullptr, &r);
    if (rc) return rc;
    r.store_normalized(out);
    return HALO_OK;
}

int halo_pcdl_open(halo_ctx *ctx, uint64_t *rng_state, const uint64_t *coeffs, size_t len, const uint64_t C[12], size_t d,
                   const uint64_t z[4], const uint64_t *w, uint64_t *proof_out) {
    HALO_CTX2(ctx);
    size_t n = d + 1;
    if (!is_pow2(n)) return fail_assert("open: d + 1 is not a power of two");  // pcdl.rs:130
    size_t deg = host_poly_degree(coeffs, len);
    if (deg > d) return fail_assert("open: p.degree() > d");                   // pcdl.rs:131
    if (n > ctx->n) return fail_assert("open: d > D");                         // pcdl.rs:132
    return pcdl_open_host(ctx, rng_state, coeffs, deg, C, d, z, w, proof_out);
}

// pcdl::open for a polynomial that already lives in device memory (the coefficients are copied, not clobbered)
int halo_pcdl_open_dev(halo_ctx *ctx, uint64_t *rng_state, const void *d_coeffs, size_t len, const uint64_t C[12], size_t d,
                       const uint64_t z[4], const uint64_t *w, uint64_t *proof_out) {
    HALO_CTX2(ctx);
    size_t n = d + 1;
    if (!is_pow2(n)) return fail_assert("open: d + 1 is not a power of two");  // pcdl.rs:130
    if (len == 0 || !d_coeffs || !C || !z || !proof_out) { set_error("open_dev: null pointer or empty polynomial"); return HALO_E_ARG; }
    if (len - 1 > d) return fail_assert("open: p.degree() > d");                // pcdl.rs:131
    if (n > ctx->n) return fail_assert("open: d > D");                          // pcdl.rs:132
    int rc = ensure_poly_buffers(ctx);
    if (rc) return rc;
    HALO_HIP(hipMemcpyAsync(ctx->d_poly, d_coeffs, len * 32, hipMemcpyDeviceToDevice, ctx->stream));
    if (len < n) HALO_HIP(hipMemsetAsync(ctx->d_poly + 4 * len, 0, (n - len) * 32, ctx->stream));
    host::Rng rng{rng_state ? *rng_state : 0};
    Fr wf = w ? Fr::load(w) : Fr::zero();
    rc = pcdl_open_dev(ctx, &rng, len - 1, Point::load(C), d, Fr::load(z), w ? &wf : nullptr, proof_out);
    if (rng_state) *rng_state = rng.state;
    return rc;
}
// pcdl::commit for device-resident coefficients (len <= d + 1)
int halo_pcdl_commit_dev(halo_ctx *ctx, const void *d_coeffs, size_t len, size_t d, const uint64_t *w, uint64_t out[12]) {
    HALO_CTX2(ctx);
    size_t n = d + 1;
    if (!is_pow2(n)) return fail_assert("commit: d + 1 is not a power of two");
    if (!out || (len && !d_coeffs)) { set_error("commit_dev: null pointer"); return HALO_E_ARG; }
    if (len > n) return fail_assert("commit: p.degree() > d");
    if (n > ctx->n) return fail_assert("commit: d > D");
    int rc = ensure_poly_buffers(ctx);
    if (rc) return rc;
    if (len) HALO_HIP(hipMemcpyAsync(ctx->d_poly2, d_coeffs, len * 32, hipMemcpyDeviceToDevice, ctx->stream));
    if (len < n) HALO_HIP(hipMemsetAsync(ctx->d_poly2 + 4 * len, 0, (n - len) * 32, ctx->stream));
    Fr wf = w ? Fr::load(w) : Fr::zero();
    Point r;
    rc = pedersen_commit_dev(ctx, w ? &wf : nullptr, ctx->d_poly2, n, &r);
    if (rc) return rc;
    r.store_normalized(out);
    return HALO_OK;
}

int halo_pcdl_succinct_check(halo_ctx *ctx, const uint64_t C[12], size_t d, const uint64_t z[4], const uint64_t v[4],
                             const uint64_t *proof, uint64_t *xis_out, uint64_t U_out[12]) {
    HALO_CTX2(ctx);
    std::vector<Fr> xis;
    Point U;
    int rc = succinct_check_host(ctx, Point::load(C), d, Fr::load(z), Fr::load(v), proof, &xis, &U);
    if (rc) return rc;
    for (size_t i = 0; i < xis.size(); ++i) xis[i].store(xis_out + 4 * i);
    U.store_normalized(U_out);
    return HALO_OK;
}

// m succinct checks at once (instances at stride halo_instance_words(lg(d+1)), all of degree bound d): on the device from
// 64 instances on, on a pool of host threads below.  status[i] = 0 or HALO_E_REJECT; returns HALO_E_REJECT (message names the
// first rejected instance) if any was rejected.  xis_out: m x (lg+1) x 4, U_out: m x 12 (both nullable).
int halo_pcdl_succinct_check_batch(halo_ctx *ctx, size_t d, const uint64_t *instances, size_t m, uint64_t *xis_out, uint64_t *U_out,
                                   int *status) {
    HALO_CTX2(ctx);
    if (m && !instances) { set_error("succinct_check_batch: null pointer"); return HALO_E_ARG; }
    if (!is_pow2(d + 1)) return fail_reject("d+1 is not a power of 2!");
    size_t lg = ilog2(d + 1), iw = instance_words(lg);
    for (size_t i = 0; i < m; ++i)
        if ((size_t)(instances + i * iw)[12] != d || (instances + i * iw)[22] != lg) return fail_reject("d_i != d");
    std::vector<BatchCheck> res;
    if (m >= kBatchVerifyMin && ctx->batch_verify) {
        int rc = succinct_check_batch(ctx, d, instances, m, res);
        if (rc) return rc;
    } else {
        res.assign(m, BatchCheck());
        pool_run(m, [&](size_t i) {
            const uint64_t *q = instances + i * iw;
            res[i].rc = succinct_challenges(ctx, Point::load(q), d, Fr::load(q + 13), Fr::load(q + 17), q + 21, &res[i].st);
            if (!res[i].rc) res[i].rc = succinct_relation(res[i].st, Fr::load(q + 13), Fr::load(q + 17), q + 21);
            if (res[i].rc) res[i].err = halo_last_error();
        });
    }
    int first = -1;
    for (size_t i = 0; i < m; ++i) {
        if (status) status[i] = res[i].rc;
        if (res[i].rc) { if (first < 0) first = (int)i; continue; }
        if (xis_out) for (size_t k = 0; k <= lg; ++k) res[i].st.xis[k].store(xis_out + ((lg + 1) * i + k) * 4);
        if (U_out) res[i].st.U.store_normalized(U_out + 12 * i);
    }
    if (first >= 0) { set_error("instance " + std::to_string(first) + ": " + res[first].err); return res[first].rc; }
    return HALO_OK;
}

int halo_pcdl_check(halo_ctx *ctx, const uint64_t C[12], size_t d, const uint64_t z[4], const uint64_t v[4], const uint64_t *proof) {
    HALO_CTX2(ctx);
    return pcdl_check_host(ctx, Point::load(C), d, Fr::load(z), Fr::load(v), proof);
}

// pcdl::check of m instances at once (see pcdl_check_batch_host)
int halo_pcdl_check_batch(halo_ctx *ctx, size_t d, const uint64_t *instances, size_t m, int *status) {
    HALO_CTX2(ctx);
    return check_batch_entry(ctx, d, instances, m, status, false);
}

int halo_pcdl_check_partial(halo_ctx *ctx, const uint64_t C[12], size_t d, const uint64_t z[4], const uint64_t v[4], const uint64_t *proof,
                            uint64_t stride, uint64_t offset, uint64_t U_out[12], uint64_t part_out[12]) {
    HALO_CTX2(ctx);
    if (!C || !z || !v || !proof || !U_out || !part_out) { set_error("check_partial: null pointer"); return HALO_E_ARG; }
    Point U, part;
    int rc = pcdl_check_partial_host(ctx, Point::load(C), d, Fr::load(z), Fr::load(v), proof, stride, offset, &U, &part);
    if (rc) return rc;
    U.store_normalized(U_out);
    part.store_normalized(part_out);
    return HALO_OK;
}

// ------------------------------------------------------------------ sharded open / check in one call each
// The round loop of sharded.ShardedOpen (Python) in the library: G, c and the z-powers are placed cyclically (element i on
// rank i mod P; the context is that rank's halo_ctx_create_urs_strided shard) and every collective of the open is one call
// of the caller's all-gather: P x words in rank order.  What a rank exchanges: its share of p(z) (4 words; with the hiding
// branch 16: the share of C_bar as well), per round L | R | dot_l | dot_r (32 words), at the end its last element of G, c
// and z (20 words) -- and ONE STATUS WORD behind every record.  Every rank computes the same challenges and returns the
// same proof: the bytes of halo_pcdl_open.
//
// Failure safety.  The number and order of collectives of a call depend only on the arguments every rank passes alike
// (P, d, hiding or not).  Whatever fails on ONE rank between two collectives -- a device allocation, a launch, a copy, a
// per-rank argument such as too many local coefficients -- does not make that rank return: it enters the next collective
// with its error code in the status word (its record zeroed), every rank reads the P status words of that collective and
// all of them return the first non-zero one in rank order, at the same collective.  No rank is left waiting in an
// all-gather its peers never enter.  (A collective that itself fails -- the callback returns non-zero -- is the caller's
// fabric failing: the call returns HALO_E_ARG on the ranks that see it and the caller must abort its process group.)
// (StatusGather and the development hook shard_test_failure live in internal.hpp: halo_msm_sharded shares them.)

int halo_pcdl_open_sharded(halo_ctx *ctx, uint64_t stride, uint64_t offset, uint64_t *rng_state, const uint64_t *coeffs_local, size_t len_local,
                           size_t deg, const uint64_t C_w[12], size_t d, const uint64_t z_w[4], const uint64_t *w_w, halo_allgather_fn allgather,
                           void *user, uint64_t *proof, uint64_t v_out[4]) {
    HALO_CTX2(ctx);
    // (arguments every rank passes alike: a mistake here is the same mistake everywhere, returned before any collective)
    if (!C_w || !z_w || !proof || !v_out || (w_w && !rng_state)) { set_error("open_sharded: null pointer"); return HALO_E_ARG; }
    const size_t P = (size_t)stride;
    if (P == 0 || !is_pow2(P) || offset >= stride || (P > 1 && !allgather)) { set_error("open_sharded: stride must be a power of two, offset below it, and an all-gather given"); return HALO_E_ARG; }
    if (P > 64) { set_error("open_sharded: at most 64 ranks"); return HALO_E_ARG; }
    size_t n = d + 1;
    if (!is_pow2(n)) return fail_assert("open: d+1 is not a power of 2");  // pcdl.rs:130-132
    if (n < P) return fail_assert("open: d > D");
    const size_t nl = n / P, lg_n = ilog2(n), lg_l = ilog2(nl);
    std::memset(proof, 0, 8 * proof_words(lg_n));
    proof[1] = lg_n;
    StatusGather sg{P, offset, allgather, user, "open_sharded", {}, {}};
    long step = 0;
    // lrc: this rank's own failure since the last collective; it rides into the next one (see above)
    int lrc = HALO_OK, rc;
    if (len_local && !coeffs_local) { set_error("open_sharded: null pointer"); lrc = HALO_E_ARG; }
    else if (nl > ctx->n) lrc = fail_assert("open: d > D");                    // (per-rank: the shard contexts may differ)
    else if (len_local > nl) lrc = fail_assert("open: p.degree() > d");
    halo_ipa *st = nullptr;
    if (!lrc) lrc = halo_ipa_begin_strided(ctx, nl, coeffs_local, len_local, z_w, stride, offset, &st);
    std::unique_ptr<halo_ipa, void (*)(halo_ipa *)> guard(st, halo_ipa_destroy);
    std::vector<uint64_t> recv;
    uint64_t send[32] = {};
    if (!lrc) lrc = halo_ipa_dot_cz(st, send);  // this shard's share of p(z)   (:135)
    uint64_t Cm[12];
    std::memcpy(Cm, C_w, sizeof Cm);
    if (!lrc) lrc = shard_test_failure(offset, step);
    if (w_w) {  // :137-164
        if (!lrc) lrc = halo_ipa_hiding_partial(st, *rng_state, deg, z_w, stride, offset, send + 4);
        rc = sg.run(send, 16, lrc, recv);
        if (rc) return rc;
        std::vector<uint64_t> v_parts(4 * P), cb_parts(12 * P);
        for (size_t r = 0; r < P; ++r) { std::memcpy(&v_parts[4 * r], &recv[16 * r], 32); std::memcpy(&cb_parts[12 * r], &recv[16 * r + 4], 96); }
        uint64_t alpha[4], Cprime[12];
        // (host arithmetic on gathered data: the same outcome on every rank)
        rc = halo_open_hiding_combine(C_w, z_w, v_parts.data(), cb_parts.data(), P, w_w, rng_state, deg, pf_Cbar(proof, lg_n), alpha, pf_wp(proof, lg_n), Cprime);
        if (rc) return rc;
        lrc = halo_ipa_apply_hiding(st, alpha);  // p' = p + alpha p_bar   (:156)
        std::memcpy(Cm, Cprime, sizeof Cm);
        proof[0] = 1;
        recv.swap(v_parts);
    } else {
        Point::infinity().store(pf_Cbar(proof, lg_n));
        rc = sg.run(send, 4, lrc, recv);
        if (rc) return rc;
    }
    uint64_t xi[4], Hp[12];
    rc = halo_open_start(Cm, z_w, recv.data(), P, v_out, xi, Hp);  // v, xi_0, H'   (:135, :180-181)
    if (rc) return rc;
    for (size_t round = 0; round < lg_l; ++round) {
        ++step;
        if (!lrc) lrc = shard_test_failure(offset, step);
        if (!lrc) lrc = halo_ipa_round_lr_partial(st, send, send + 12, send + 24);
        rc = sg.run(send, 32, lrc, recv);
        if (rc) return rc;
        uint64_t xn[4], xinv[4];
        rc = halo_open_combine(recv.data(), P, Hp, xi, pf_L(proof, round), pf_R(proof, lg_n, round), xn, xinv);  // :203-213
        if (rc) return rc;
        std::memcpy(xi, xn, sizeof xi);
        lrc = halo_ipa_round_fold(st, xn, xinv);  // :216-224
    }
    uint64_t last[20] = {};
    ++step;
    if (!lrc) lrc = shard_test_failure(offset, step);
    if (!lrc) lrc = halo_ipa_finish_z(st, last, last + 12, last + 16);
    if (P == 1) {
        if (lrc) return lrc;
        std::memcpy(pf_U(proof, lg_n), last, 96);
        std::memcpy(pf_c(proof, lg_n), last + 12, 32);
        return HALO_OK;
    }
    rc = sg.run(last, 20, lrc, recv);  // the P remaining elements, in index order
    if (rc) return rc;
    size_t lgP = ilog2(P);
    std::vector<uint64_t> Ls(12 * lgP), Rs(12 * lgP);
    rc = halo_open_tail(recv.data(), P, Hp, xi, Ls.data(), Rs.data(), pf_U(proof, lg_n), pf_c(proof, lg_n));  // the last lg P rounds
    if (rc) return rc;
    for (size_t k = 0; k < lgP; ++k) {
        std::memcpy(pf_L(proof, lg_l + k), &Ls[12 * k], 96);
        std::memcpy(pf_R(proof, lg_n, lg_l + k), &Rs[12 * k], 96);
    }
    return HALO_OK;
}

// pcdl::check over the same shards: halo_pcdl_check_partial, one all-gather of 12 words + the status word, the shares added
// in rank order, U compared (pcdl.rs:338-339).  HALO_E_REJECT on every rank alike; a rank whose own half failed (device error)
// still enters the collective and every rank returns its code (see halo_pcdl_open_sharded).
int halo_pcdl_check_sharded(halo_ctx *ctx, uint64_t stride, uint64_t offset, const uint64_t C[12], size_t d, const uint64_t z[4], const uint64_t v[4],
                            const uint64_t *proof, halo_allgather_fn allgather, void *user) {
    HALO_CTX2(ctx);
    if (!C || !z || !v || !proof || (stride > 1 && !allgather)) { set_error("check_sharded: null pointer"); return HALO_E_ARG; }
    if (stride == 0 || stride > 64 || offset >= stride) { set_error("check_sharded: stride in 1..64, offset below it"); return HALO_E_ARG; }
    Point U, part;
    // The succinct check is host arithmetic on the same proof on every rank: its HALO_E_REJECT is the same everywhere, but it
    // goes through the status word like any other outcome, so that the collective count stays fixed (one).
    int lrc = shard_test_failure(offset, SHARD_AT_CHECK);
    if (!lrc) lrc = pcdl_check_partial_host(ctx, Point::load(C), d, Fr::load(z), Fr::load(v), proof, stride, offset, &U, &part);
    uint64_t send[12] = {};
    if (!lrc) part.store_normalized(send);
    StatusGather sg{(size_t)stride, offset, allgather, user, "check_sharded", {}, {}};
    std::vector<uint64_t> recv;
    int rc = sg.run(send, 12, lrc, recv);
    if (rc) return rc;
    Point comm = Point::infinity();
    for (uint64_t r = 0; r < stride; ++r) comm = comm + Point::load(&recv[12 * r]);
    if (U != comm) return fail_reject("U != CM.Commit(ck, h_vec)");  // :339
    return HALO_OK;
}

// acc.rs:190-220
int halo_acc_prover(halo_ctx *ctx, uint64_t *rng_state, size_t d, const uint64_t *qs, size_t m, uint64_t *acc) {
    HALO_CTX2(ctx);
    if (!is_pow2(d + 1)) return fail_assert("prover: d + 1 is not a power of two");
    if (d + 1 > ctx->n) return fail_assert("prover: d > D");
    size_t lg = ilog2(d + 1), n = d + 1;
    host::Rng rng{rng_state ? *rng_state : 0};
    Fr h0[2] = {rng.scalar(), rng.scalar()};  // :192
    uint64_t h0w[8];
    h0[0].store(h0w);
    h0[1].store(h0w + 4);
    Point U0;
    int rc = pcdl_commit_host(ctx, h0w, 2, d, nullptr, &U0);  // :195
    if (rc) return rc;
    Fr w = rng.scalar();  // :198
    Point C_bar;
    Fr z;
    AccHPolys hs;
    rc = common_subroutine(ctx, d, qs, m, h0, U0, w, &C_bar, &z, &hs);  // :202
    if (rc) return rc;
    Fr v = hs.eval(z);  // :205
    // h.get_poly(): h_0 + sum alpha^(i+1) h_i(X), expanded on the device (acc.rs:85-94)
    rc = ensure_poly_buffers(ctx);
    if (rc) return rc;
    HALO_HIP(hipMemsetAsync(ctx->d_poly, 0, n * 32, ctx->stream));
    rc = upload_words(ctx, ctx->d_poly, h0w, (n < 2 ? n : 2) * 4);
    if (rc) return rc;
    for (size_t i = 0; i < m; ++i) {
        rc = h_coeffs_dev(ctx, hs.xis[i].data(), lg, hs.alphas[i + 1], true, ctx->d_poly);
        if (rc) return rc;
    }
    std::memset(acc, 0, 8 * acc_words(lg));
    C_bar = C_bar.normalized();
    C_bar.store(acc);
    acc[12] = d;
    z.store(acc + 13);
    v.store(acc + 17);
    size_t deg = m ? d : (h0[1].is_zero() ? 0 : 1);
    rc = pcdl_open_dev(ctx, &rng, deg, C_bar, d, z, &w, acc + 21);  // :209
    uint64_t *piV = acc + instance_words(lg);
    std::memcpy(piV, h0w, 64);
    U0.store_normalized(piV + 8);
    w.store(piV + 20);
    if (rng_state) *rng_state = rng.state;
    return rc;
}

// acc::prover of k members at once (see acc_prover_batch_dev).  The argument checks are the whole call's and come before any work.
int halo_acc_prover_batch(halo_ctx *ctx, uint64_t *rng_state, size_t d, const uint64_t *instances, const size_t *counts, size_t k, uint64_t *accs_out,
                          int *status) {
    HALO_CTX2(ctx);
    if (k && (!accs_out || !counts)) { set_error("prover_batch: null pointer"); return HALO_E_ARG; }
    size_t total = 0;
    for (size_t j = 0; j < k; ++j) {
        if (counts[j] > ((size_t)1 << 32) - total) { set_error("prover_batch: too many instances"); return HALO_E_ARG; }
        total += counts[j];
    }
    if (total && !instances) { set_error("prover_batch: null pointer"); return HALO_E_ARG; }
    if (!is_pow2(d + 1)) return fail_assert("prover: d + 1 is not a power of two");
    if (d + 1 > ctx->n) return fail_assert("prover: d > D");
    if (k == 0) return HALO_OK;
    return acc_prover_batch_entry(ctx, rng_state, d, instances, counts, k, accs_out, status);
}

// acc.rs:223-243
int halo_acc_verifier(halo_ctx *ctx, size_t d, const uint64_t *qs, size_t m, const uint64_t *acc) {
    HALO_CTX2(ctx);
    if (!is_pow2(d + 1)) return fail_reject("d+1 is not a power of 2!");
    size_t lg = ilog2(d + 1);
    const uint64_t *piV = acc + instance_words(lg);
    Fr h0[2] = {Fr::load(piV), Fr::load(piV + 4)};
    if (!Point::load(piV + 8).on_curve() || !Point::load(acc).on_curve() || !scalar_ok(h0[0]) || !scalar_ok(h0[1]) ||
        !scalar_ok(Fr::load(piV + 20)) || !scalar_ok(Fr::load(acc + 13)) || !scalar_ok(Fr::load(acc + 17)))
        return fail_reject("accumulator holds an invalid point or scalar");
    Point C_bar_p;
    Fr z_p;
    AccHPolys hs;
    int rc = common_subroutine(ctx, d, qs, m, h0, Point::load(piV + 8), Fr::load(piV + 20), &C_bar_p, &z_p, &hs);
    if (rc) return rc;
    Fr z = Fr::load(acc + 13), v = Fr::load(acc + 17);
    if (C_bar_p != Point::load(acc)) return fail_reject("C_bar' != C_bar");
    if (z_p != z) return fail_reject("z' != z");
    if ((size_t)acc[12] != d) return fail_reject("d' != d");
    if (hs.eval(z) != v) return fail_reject("h(z) != v");
    return HALO_OK;
}

// acc::verifier of k accumulators at once (benches/acc.rs:64-74's loop in one call; see acc_verifier_batch_host).  The argument
// checks are the whole call's and come before any work: d + 1 above the key is the assert the single call meets in
// pcdl_commit_host.  A multi-device context runs the batch on its own device (devices[0]) like the other batches.
int halo_acc_verifier_batch(halo_ctx *ctx, size_t d, const uint64_t *instances, const size_t *counts, size_t k, const uint64_t *accs, int *status) {
    HALO_CTX2(ctx);
    if (k && (!accs || !counts)) { set_error("verifier_batch: null pointer"); return HALO_E_ARG; }
    size_t total = 0;
    for (size_t j = 0; j < k; ++j) {
        if (counts[j] > ((size_t)1 << 32) - total) { set_error("verifier_batch: too many instances"); return HALO_E_ARG; }
        total += counts[j];
    }
    if (total && !instances) { set_error("verifier_batch: null pointer"); return HALO_E_ARG; }
    if (!is_pow2(d + 1)) return fail_reject("d+1 is not a power of 2!");
    if (d + 1 > ctx->n) return fail_assert("commit: d > D");
    if (k == 0) return HALO_OK;
    return acc_verifier_batch_host(ctx, d, instances, counts, k, accs, status);
}

// acc.rs:245-255
int halo_acc_decider(halo_ctx *ctx, const uint64_t *acc) {
    HALO_CTX2(ctx);
    return pcdl_check_host(ctx, Point::load(acc), (size_t)acc[12], Fr::load(acc + 13), Fr::load(acc + 17), acc + 21);
}

// acc::decider of m accumulators at once (benches/acc.rs:100-106 in one call): the check batch over their Instance prefixes
int halo_acc_decider_batch(halo_ctx *ctx, size_t d, const uint64_t *accs, size_t m, int *status) {
    HALO_CTX2(ctx);
    return check_batch_entry(ctx, d, accs, m, status, true);
}

// benches/acc.rs:15-29 random_instance (workload generator for BASELINE config 4)
int halo_random_instance(halo_ctx *ctx, uint64_t *rng_state, size_t d, uint64_t *inst) {
    HALO_CTX2(ctx);
    if (!is_pow2(d + 1) || d < 2) return fail_assert("random_instance: bad d");
    if (d + 1 > ctx->n) return fail_assert("random_instance: d > D");
    return random_instance_one(ctx, rng_state, d, inst);
}

// pcdl::open of m polynomials at once (see open_batch_dev)
int halo_pcdl_open_batch(halo_ctx *ctx, uint64_t *rng_state, size_t d, const uint64_t *coeffs, size_t m, const uint64_t *Cs, const uint64_t *zs,
                         const uint64_t *ws, uint64_t *proofs_out, int *status) {
    HALO_CTX2(ctx);
    if (m == 0) return HALO_OK;
    if (!coeffs || !Cs || !zs || !proofs_out) { set_error("open_batch: null pointer"); return HALO_E_ARG; }
    const size_t n = d + 1;
    if (!is_pow2(n)) return fail_assert("open: d + 1 is not a power of two");  // pcdl.rs:130 (p.degree() <= d: the arrays hold d + 1)
    if (n > ctx->n) return fail_assert("open: d > D");                         // pcdl.rs:132
    return open_batch_entry(ctx, rng_state, d, coeffs, m, Cs, zs, ws, proofs_out, status);
}

// benches/acc.rs:15-29 random_instance, m times (see open_batch_dev)
int halo_random_instance_batch(halo_ctx *ctx, uint64_t *rng_state, size_t d, size_t m, uint64_t *instances_out) {
    HALO_CTX2(ctx);
    if (m == 0) return HALO_OK;
    if (!instances_out) { set_error("random_instance_batch: null pointer"); return HALO_E_ARG; }
    if (!is_pow2(d + 1) || d < 2) return fail_assert("random_instance: bad d");
    if (d + 1 > ctx->n) return fail_assert("random_instance: d > D");
    return open_batch_entry(ctx, rng_state, d, nullptr, m, nullptr, nullptr, nullptr, instances_out, nullptr);
}

}  // extern "C"
