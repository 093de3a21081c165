// The small vector calls of the group.rs level over host arrays (dot product, powers, evaluation), the halo_h_* calls on
// h(X) and the scalar stream: each stages its input in the context's temporaries and runs the kernels of fr_vec.hip / hpoly.hip.
#include "internal.hpp"

namespace halo {
static std::vector<host::Fr> load_frs(const uint64_t *p, size_t count) {
    std::vector<host::Fr> v(count);
    for (size_t i = 0; i < count; ++i) v[i] = host::Fr::load(p + 4 * i);
    return v;
}
}  // namespace halo

using namespace halo;

extern "C" {
int halo_scalar_dot(halo_ctx *ctx, const uint64_t *xs, const uint64_t *ys, size_t m, uint64_t out[4]) {
    HALO_CTX(ctx);
    if (m > ctx_capacity(ctx)) { set_error("scalar_dot: m exceeds context size"); return HALO_E_ARG; }
    int rc = upload_words(ctx, ctx->d_tmp_a, xs, m * 4);
    if (!rc) rc = upload_words(ctx, ctx->d_tmp_b, ys, m * 4);
    if (rc) return rc;
    host::Fr r[2];
    rc = fr_dot2(ctx, ctx->d_tmp_a, ctx->d_tmp_b, nullptr, nullptr, m, r);
    if (rc) return rc;
    r[0].store(out);
    return HALO_OK;
}

int halo_powers(halo_ctx *ctx, const uint64_t z[4], size_t n, uint64_t *out) {
    HALO_CTX(ctx);
    if (n > ctx_capacity(ctx)) { set_error("powers: n exceeds context size"); return HALO_E_ARG; }
    int rc = fr_powers(ctx, host::Fr::load(z), n, ctx->d_tmp_a);
    if (rc) return rc;
    return download_words(ctx, out, ctx->d_tmp_a, n * 4);
}

int halo_poly_eval(halo_ctx *ctx, const uint64_t *coeffs, size_t len, const uint64_t z[4], uint64_t out[4]) {
    HALO_CTX(ctx);
    if (len > ctx_capacity(ctx)) { set_error("poly_eval: len exceeds context size"); return HALO_E_ARG; }
    int rc = upload_words(ctx, ctx->d_tmp_a, coeffs, len * 4);
    if (rc) return rc;
    host::Fr r;
    rc = fr_poly_eval(ctx, ctx->d_tmp_a, len, host::Fr::load(z), &r);
    if (rc) return rc;
    r.store(out);
    return HALO_OK;
}

// ... over coefficients in device memory, read in place (no staging: len is not bound by the context's size)
int halo_poly_eval_dev(halo_ctx *ctx, const void *d_coeffs, size_t len, const uint64_t z[4], uint64_t out[4]) {
    HALO_CTX(ctx);
    if (!z || !out) { set_error("poly_eval_dev: null pointer"); return HALO_E_ARG; }
    int rc = dev_rows_ok("poly_eval_dev", &d_coeffs, &len, 1);
    if (rc) return rc;
    if (len >= ((size_t)1 << 32)) { set_error("poly_eval_dev: len exceeds 2^32 - 1"); return HALO_E_ARG; }
    host::Fr r;
    rc = fr_poly_eval(ctx, static_cast<const uint64_t *>(d_coeffs), len, host::Fr::load(z), &r);
    if (rc) return rc;
    r.store(out);
    return HALO_OK;
}

// DensePolynomial::degree of m device-resident rows (fr_vec.hip k_poly_degree_batch)
int halo_poly_degrees_dev(halo_ctx *ctx, const void *const *d_coeffs, const size_t *lens, size_t m, size_t *degrees_out) {
    HALO_CTX(ctx);
    if (m && !degrees_out) { set_error("poly_degrees_dev: null pointer"); return HALO_E_ARG; }
    int rc = dev_rows_ok("poly_degrees_dev", d_coeffs, lens, m);
    if (rc) return rc;
    std::vector<size_t> degs(m);  // (nothing is written unless the whole call succeeds)
    rc = poly_degrees_dev(ctx, d_coeffs, lens, m, degs.data());
    if (rc) return rc;
    for (size_t i = 0; i < m; ++i) degrees_out[i] = degs[i];
    return HALO_OK;
}

// ------------------------------------------------------------------ h(X)
int halo_h_coeffs(halo_ctx *ctx, const uint64_t *xis, size_t lg_n, uint64_t *out) {
    HALO_CTX(ctx);
    size_t n = (size_t)1 << lg_n;
    if (n > ctx_capacity(ctx)) { set_error("h_coeffs: 2^lg_n exceeds context size"); return HALO_E_ARG; }
    std::vector<host::Fr> x = load_frs(xis, lg_n + 1);
    int rc = h_coeffs_dev(ctx, x.data(), lg_n, host::Fr::one(), false, ctx->d_tmp_a);
    if (rc) return rc;
    return download_words(ctx, out, ctx->d_tmp_a, n * 4);
}

int halo_h_commit(halo_ctx *ctx, const uint64_t *xis, size_t lg_n, uint64_t out[12]) {
    HALO_CTX(ctx);
    size_t n = (size_t)1 << lg_n;
    if (n > ctx->n) { set_error("h_commit: 2^lg_n exceeds the commitment key"); return HALO_E_ARG; }
    std::vector<host::Fr> x = load_frs(xis, lg_n + 1);
    int rc = h_coeffs_dev(ctx, x.data(), lg_n, host::Fr::one(), false, ctx->d_tmp_a);
    if (rc) return rc;
    host::Point r;
    rc = msm_run(ctx, ctx->d_bases, ctx->d_tmp_a, true, n, &r);
    if (rc) return rc;
    r.store_normalized(out);
    return HALO_OK;
}

int halo_h_eval_batch(halo_ctx *ctx, const uint64_t *xis, size_t m, size_t lg_n, const uint64_t z[4], uint64_t *out) {
    HALO_CTX(ctx);
    if (m * (lg_n + 1) * 4 > ctx->tmp_words) { set_error("h_eval_batch: batch too large for context"); return HALO_E_ARG; }
    int rc = upload_words(ctx, ctx->d_tmp_a, xis, m * (lg_n + 1) * 4);
    if (rc) return rc;
    rc = h_eval_batch(ctx, ctx->d_tmp_a, m, lg_n, host::Fr::load(z), ctx->d_tmp_b);
    if (rc) return rc;
    return download_words(ctx, out, ctx->d_tmp_b, m * 4);
}

int halo_h_accumulate(halo_ctx *ctx, const uint64_t *h0, const uint64_t *xis, const uint64_t *alphas, size_t m, size_t lg_n,
                      uint64_t *out) {
    HALO_CTX(ctx);
    size_t n = (size_t)1 << lg_n;
    if (n > ctx_capacity(ctx)) { set_error("h_accumulate: 2^lg_n exceeds context size"); return HALO_E_ARG; }
    HALO_HIP(hipMemsetAsync(ctx->d_tmp_a, 0, n * 32, ctx->stream));
    if (h0) {
        int rc = upload_words(ctx, ctx->d_tmp_a, h0, (n < 2 ? n : 2) * 4);
        if (rc) return rc;
    }
    for (size_t i = 0; i < m; ++i) {
        std::vector<host::Fr> x = load_frs(xis + 4 * i * (lg_n + 1), lg_n + 1);
        int rc = h_coeffs_dev(ctx, x.data(), lg_n, host::Fr::load(alphas + 4 * i), true, ctx->d_tmp_a);
        if (rc) return rc;
    }
    return download_words(ctx, out, ctx->d_tmp_a, n * 4);
}

int halo_rng_scalars_dev(halo_ctx *ctx, uint64_t *rng_state, size_t n, void *d_out) {
    HALO_CTX(ctx);
    if (!rng_state || (n && !d_out)) { set_error("rng_scalars: null pointer"); return HALO_E_ARG; }
    int rc = rng_scalars_dev(ctx, *rng_state, n, static_cast<uint64_t *>(d_out));
    if (rc) return rc;
    HALO_HIP(hipStreamSynchronize(ctx->stream));
    *rng_state = host::Rng{*rng_state}.skip_scalars(n).state;  // n scalars = 4n draws of the SplitMix64 stream
    return HALO_OK;
}
}  // extern "C"
