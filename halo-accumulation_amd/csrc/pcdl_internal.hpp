// Shared by the pcdl / acc level of the library: pcdl_acc.hip (the single calls, the sharded open and check), pcdl_batch.hip (the
// batched calls) and, for the blob layout alone, wire.hip; for the transcript's hashes open_host.hip, for is_pow2 ipa_state.hip.
#pragma once
#include "fr_plan.hpp"  // (plan_h_coeffs: the parts of the combined checks' scalar step)
#include "internal.hpp"

namespace halo {

// ---- flat layouts (include/halo_accumulation.h, "pcdl / acc level")
inline size_t proof_words(size_t lg) { return 2 + 24 * lg + 32; }
inline size_t instance_words(size_t lg) { return 21 + proof_words(lg); }
inline size_t acc_words(size_t lg) { return instance_words(lg) + 24; }
inline uint64_t *pf_L(uint64_t *pf, size_t i) { return pf + 2 + 12 * i; }
inline uint64_t *pf_R(uint64_t *pf, size_t lg, size_t i) { return pf + 2 + 12 * lg + 12 * i; }
inline uint64_t *pf_U(uint64_t *pf, size_t lg) { return pf + 2 + 24 * lg; }
inline uint64_t *pf_c(uint64_t *pf, size_t lg) { return pf + 2 + 24 * lg + 12; }
inline uint64_t *pf_Cbar(uint64_t *pf, size_t lg) { return pf + 2 + 24 * lg + 16; }
inline uint64_t *pf_wp(uint64_t *pf, size_t lg) { return pf + 2 + 24 * lg + 28; }

// an Instance's fields in front of its proof: C | d | z | v
inline void store_instance_head(uint64_t *inst, const host::Point &C, size_t d, const host::Fr &z, const host::Fr &v) {
    C.store(inst);
    inst[12] = d;
    z.store(inst + 13);
    v.store(inst + 17);
}

inline bool is_pow2(size_t n) { return n && !(n & (n - 1)); }
inline size_t ilog2(size_t n) { size_t l = 0; while (n > 1) { n >>= 1; ++l; } return l; }
inline int fail_assert(const char *m) { set_error(m); return HALO_E_ASSERT; }
inline int fail_reject(const char *m) { set_error(m); return HALO_E_REJECT; }
inline bool scalar_ok(const host::Fr &s) { return !host::Fr::geq(s.l, host::FrP::M); }

// DensePolynomial::degree: the index of the last non-zero coefficient (0 for the zero polynomial).  Scanned from the END: a
// dense polynomial answers at its first look (the forward scan this replaces read all 32 MiB of a 2^20-coefficient polynomial
// on the host, ~1 ms of every halo_pcdl_open / halo_pcdl_commit with host coefficients).
inline size_t host_poly_degree(const uint64_t *coeffs, size_t len) {
    for (size_t i = len; i-- > 0;)
        if (coeffs[4 * i] | coeffs[4 * i + 1] | coeffs[4 * i + 2] | coeffs[4 * i + 3]) return i;
    return 0;
}

// ---- the transcript's hashes (rho_0!, rho_1!)
inline host::Fr rho0_C_z_v(const host::Point &C, const host::Fr &z, const host::Fr &v) {
    host::Transcript t; t.point(C); t.scalar(z); t.scalar(v); return t.finish(0);
}
inline host::Fr rho0_C_z_v_Cbar(const host::Point &C, const host::Fr &z, const host::Fr &v, const host::Point &Cb) {
    host::Transcript t; t.point(C); t.scalar(z); t.scalar(v); t.point(Cb); return t.finish(0);
}
inline host::Fr rho0_xi_L_R(const host::Fr &xi, const host::Point &L, const host::Point &R) {
    host::Transcript t; t.scalar(xi); t.point(L); t.point(R); return t.finish(0);
}
// acc.rs:181  z = rho_1(C, alpha)
inline host::Fr rho1_C_alpha(const host::Point &C, const host::Fr &alpha) {
    host::Transcript t; t.point(C); t.scalar(alpha); return t.finish(1);
}

// ---- pcdl_acc.hip: pcdl::succinct_check in two halves (see succinct_challenges there)
struct SuccinctState {
    size_t lg_n = 0;
    host::Point C_prime, Hp, U;
    std::vector<host::Fr> xis;
};
// one instance's outcome as its single call reports it: code, message, accepted transcript
struct BatchCheck { int rc = HALO_OK; std::string err; SuccinctState st; };
// key_n: the size of the key the check is against (ctx->n; a rank's cyclic shard stands for stride * ctx->n points)
int succinct_challenges(halo_ctx *ctx, const host::Point &C, size_t d, const host::Fr &z, const host::Fr &v, const uint64_t *proof, SuccinctState *st,
                        bool need_hp = true, size_t key_n = 0);
int succinct_relation(const SuccinctState &st, const host::Fr &z, const host::Fr &v, const uint64_t *proof);
// The 2 lg n + 2 terms of one instance's relation (q: its blob, hz = h(z) of its challenges, st: its accepted transcript) whose
// sum is -C' exactly when pcdl.rs:288-310 accepts: points arkworks affine ((0, 0) = infinity), scalars canonical
void relation_terms(const SuccinctState &st, const uint64_t *q, const host::Fr &hz, uint64_t *pts, uint64_t *sc);
// The succinct half of m Instance blobs of degree bound d (checked by the caller), blob_at(i) = instance i's words: res[i] = what
// halo_pcdl_succinct_check reports for it alone.  succinct_check_batch: the relations in two device launches.  succinct_half: the
// one rule of every batched call -- that from kBatchVerifyMin instances on if ctx->batch_verify, else the host pool.  Both
// return a device / argument error only.
using BlobAt = std::function<const uint64_t *(size_t)>;
constexpr size_t kBatchVerifyMin = 64;  // below this the host pool is faster than a 256-step device ladder (~2 ms)
int succinct_check_batch(halo_ctx *ctx, size_t d, const BlobAt &blob_at, size_t m, std::vector<BatchCheck> &res);
int succinct_half(halo_ctx *ctx, size_t d, const BlobAt &blob_at, size_t m, std::vector<BatchCheck> &res);
int verify_staging(halo_ctx *ctx, size_t words);  // ctx->d_verify holds at least `words`

// ---- transcript.hip: the transcripts alone (no relation) of m Instance blobs of degree bound d: res[i].rc / err / st.{lg_n, C_prime,
// xis, U} as succinct_challenges leaves them (C_prime normalised on the device route: the same point).  transcripts_batch: the rule
// of every batched call -- the device from transcript_min members on (the hook "transcript_min", else kTranscriptMin) if
// ctx->batch_verify and the optional staging is granted, else the host pool.  transcripts_batch_dev: the device route whatever m
// is; kTranscriptNoStage if the staging is refused (nothing ran), else a device / argument error only.  need_relation_inputs: fill
// st.U as well (the development library's twin needs the challenges and C' only).
// measured (tools/time_transcripts.py, profiles/r20_transcripts.json): at k = 1000 every device run beats every host
// run at 2^9 and 2^14 points in both timed calls; at k = 64 and 100 the host pool wins (the K = 3 ladder launch costs ~2 ms flat)
constexpr size_t kTranscriptMin = 1000;
constexpr int kTranscriptNoStage = 1;
int transcripts_batch(halo_ctx *ctx, size_t d, const BlobAt &blob_at, size_t m, std::vector<BatchCheck> &res);
int transcripts_batch_dev(halo_ctx *ctx, size_t d, const BlobAt &blob_at, size_t m, std::vector<BatchCheck> &res, bool need_relation_inputs);

// ---- pcdl_batch.hip: the combined check batch (halo_pcdl_check_batch_combined; the development library runs its steps alone)
// The weights r_a of the A accepted members idx[0 .. A) of the blobs at `stride` words, degree bound d, seed = 32 bytes or null
// (32 zero bytes): the rule of include/halo_accumulation.h, Montgomery form
void check_combined_weights(const uint64_t *blobs, size_t stride, const size_t *idx, size_t A, size_t d, const uint8_t *seed, std::vector<host::Fr> &out);
// parts and tables per pass of the scalar step for A polynomials of n coefficients (the hooks "check_combined_parts" / "_cap" first;
// the mixed call: n = the longest polynomial's).  Inline: the development library's twins of the scalar step use the same rule.
// P: one row of parts is plan_h_coeffs(n).blocks x 4 waves; enough parts for a wave per SIMD (1024) where the members allow
inline size_t check_combined_parts(size_t n, size_t A) {
    const int forced = dev_hooks().combined_parts;
    size_t P;
    if (forced >= 1) P = (size_t)forced;
    else {
        const size_t waves = (size_t)plan_h_coeffs(n).blocks * 4;
        P = (1024 + waves - 1) / waves;
    }
    return P > A ? A : (P < 1 ? 1 : P);
}
// tables per pass: 256 x 24 KiB = 6 MiB of staging, and a pass of 256 tables is long enough to hide the next launch
inline size_t check_combined_cap(size_t A) {
    const int forced = dev_hooks().combined_cap;
    const size_t cap = forced >= 1 ? (size_t)forced : 256;
    return cap > A ? A : cap;
}
// ---- pcdl_batch.hip: the mixed combined check batch (halo_pcdl_check_batch_mixed_combined): the weights r_a of the accepted members
// idx[0 .. A) of a call whose member i is the blob blobs[i] of degree bound ds[i], under the rule's own domain, Montgomery form
// ... and of the mixed fused check batch (halo_pcdl_check_batch_mixed_fused): the 2 A weights r_0, s_0, r_1, s_1, .. under that rule's
// domain.  The two rules hash the same things, so they are one function behind two names (one name in the development library's
// reach, product.map).
enum class MixedRule { combined, fused };
void check_mixed_weights_rule(MixedRule rule, const uint64_t *const *blobs, const size_t *ds, const size_t *idx, size_t A, const uint8_t *seed,
                              std::vector<host::Fr> &out);
inline void check_mixed_weights(const uint64_t *const *blobs, const size_t *ds, const size_t *idx, size_t A, const uint8_t *seed, std::vector<host::Fr> &out) {
    check_mixed_weights_rule(MixedRule::combined, blobs, ds, idx, A, seed, out);
}
inline void check_mixed_fused_weights(const uint64_t *const *blobs, const size_t *ds, const size_t *idx, size_t A, const uint8_t *seed,
                                      std::vector<host::Fr> &out) {
    check_mixed_weights_rule(MixedRule::fused, blobs, ds, idx, A, seed, out);
}
// ---- pcdl_batch.hip: the fused check batch (halo_pcdl_check_batch_fused): the 2 A weights r_0, s_0, r_1, s_1, .. of the accepted
// members, arguments as check_combined_weights, under the rule's own domain string (include/halo_accumulation.h), Montgomery form
void check_fused_weights(const uint64_t *blobs, size_t stride, const size_t *idx, size_t A, size_t d, const uint8_t *seed, std::vector<host::Fr> &out);

// ---- pcdl_acc.hip: acc.rs
struct AccHPolys {  // acc.rs:61-66
    host::Fr h0[2];
    std::vector<std::vector<host::Fr>> xis;
    host::Fr alpha;
    std::vector<host::Fr> alphas;  // alpha^0 .. alpha^m
    size_t lg_n = 0;

    host::Fr eval(const host::Fr &z) const {  // acc.rs:97-106
        host::Fr v = h0[0] + h0[1] * z;
        for (size_t i = 0; i < xis.size(); ++i) v = v + host::h_eval(xis[i].data(), lg_n, z) * alphas[i + 1];
        return v;
    }
};
// acc.rs:173  alpha = rho_1(hs): h_0 Some(poly), hs Vec<HPoly>, alpha None, alphas empty; then alpha^0 .. alpha^m
void set_alphas(AccHPolys *hs);

// ---- pcdl_acc.hip: the bodies of halo_pcdl_open (deg = host_poly_degree(coeffs) <= d) and halo_random_instance after their argument checks
int pcdl_open_host(halo_ctx *ctx, uint64_t *rng_state, const uint64_t *coeffs, size_t deg, const uint64_t C[12], size_t d, const uint64_t z[4],
                   const uint64_t *w, uint64_t *proof_out);
int random_instance_one(halo_ctx *ctx, uint64_t *rng_state, size_t d, uint64_t *inst);
// ... of halo_pcdl_commit (its own checks inside) and of halo_instance_from_poly (len coefficients of degree deg <= d)
int pcdl_commit_host(halo_ctx *ctx, const uint64_t *coeffs, size_t len, size_t d, const host::Fr *w, host::Point *out);
int instance_from_poly_one(halo_ctx *ctx, uint64_t *rng_state, const uint64_t *coeffs, size_t len, size_t deg, size_t d, const uint64_t z[4],
                           const uint64_t *w, uint64_t *inst);
// ... of halo_pcdl_open_dev, and instance_from_poly_one's counterpart, for a device-resident row: len <= d + 1 scalars of degree deg
// (poly_degrees_dev), copied device to device into the context's polynomial buffer and never modified
int pcdl_open_dev_row(halo_ctx *ctx, uint64_t *rng_state, const void *d_coeffs, size_t len, size_t deg, const uint64_t C[12], size_t d,
                      const uint64_t z[4], const uint64_t *w, uint64_t *proof_out);
int instance_from_poly_dev_row(halo_ctx *ctx, uint64_t *rng_state, const void *d_coeffs, size_t len, size_t deg, size_t d, const uint64_t z[4],
                               const uint64_t *w, uint64_t *inst);

}  // namespace halo
