// libhalo_hip_dev.so: what developers and the test-suite need and a production host does not (include/halo_accumulation_dev.h).
//
//   * the primitive test hooks (one field / group operation per lane, compared with the oracle by tests/test_gpu_parity.py),
//   * halo_bench_fr_kernel (back-to-back launches of one bandwidth-side kernel for the profiler),
//   * the per-context experiment knobs (window bits, task length, sort / fold / IPA strategy),
//   * halo_dev_hook: the fault injectors and forced test paths of csrc/tuning.hpp DevHooks.
//
// It links AGAINST libhalo_hip.so (one copy of the library's state in the process) and holds nothing the product path calls:
// `nm -D libhalo_hip.so` shows no halo_test_* / halo_bench_* / halo_dev_* symbol, and the product library reads no fault
// injector from the environment (tests/test_abi_cpu.py checks both).  What this file calls in the product is the reach that
// product.map exports, name by name: a call to another internal fails this library's link until the map lists it.
#include <cstring>

#include "../../include/halo_accumulation_dev.h"
#include "curve_quad.hpp"
#include "dev_lazy_ops.hpp"
#include "fr_plan.hpp"
#include "internal.hpp"
#include "mixed_terms_lane.hpp"  // (the descriptors of halo_dev_check_mixed_terms)
#include "pcdl_internal.hpp"

namespace halo {

// ------------------------------------------------------------------------------ test hooks
template <class F>
__global__ __launch_bounds__(256) void k_test_field(int op, const uint64_t *a, const uint64_t *b, uint32_t n, uint64_t *out) {
    uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    Fe x = fe_load(a + 4 * (size_t)i);
    Fe y = b ? fe_load(b + 4 * (size_t)i) : fe_zero();
    Fe r;
    switch (op) {
        case 0: r = fe_mul<F>(x, y); break;
        case 1: r = fe_add<F>(x, y); break;
        case 2: r = fe_sub<F>(x, y); break;
        case 3: r = fe_is_zero(x) ? fe_zero() : fe_inv<F>(x); break;
        case 4: r = fe_from_mont<F>(x); break;
        default: r = fe_to_mont<F>(x); break;
    }
    fe_store(out + 4 * (size_t)i, r);
}
// the same operations through the native radix-2^29 field (Fq only): in/out in arkworks words
__global__ __launch_bounds__(256) void k_test_field29(int op, const uint64_t *a, const uint64_t *b, uint32_t n, uint64_t *out) {
    uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    Fq<2> x = fq_from_words(fe_load(a + 4 * (size_t)i));
    Fq<2> y = b ? fq_from_words(fe_load(b + 4 * (size_t)i)) : fq_zero<2>();
    Fe r;
    switch (op) {
        case 0: r = fq_to_words(fq_mul(x, y)); break;
        case 1: r = fq_to_words(fq_add(x, y)); break;
        case 2: r = fq_to_words(fq_sub<2>(x, y)); break;
        case 3: r = fq_is_zero_modp(x) ? fe_zero() : fq_to_words(fq_inv(x)); break;
        case 6: r = fq_to_words(fq_sqr(x)); break;
        case 7: r = fq_to_words(fq_muls<4>(fq_muls<3>(fq_add(x, y)))); break;  // 12 (x + y), lazy chain
        case 8: r = fq_to_words(fq_tighten(fq_sub_sub2(fq_muls<4>(x), y, x))); break;  // 2x - y
        default: r = fq_to_words(x); break;                                            // round trip
    }
    fe_store(out + 4 * (size_t)i, r);
}
HALO_DEV bool aff_same(const AffN &a, const AffN &b) {
    if (aff_is_inf(a) || aff_is_inf(b)) return aff_is_inf(a) && aff_is_inf(b);
    return fq_eq_modp(a.x, b.x) && fq_eq_modp(a.y, b.y);
}
__global__ __launch_bounds__(256) void k_test_point(int op, const uint64_t *a, const uint64_t *b, uint32_t n, uint64_t *out) {
    uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    JacN p = jac_from_words(a + 12 * (size_t)i);
    uint64_t *o = out + 12 * (size_t)i;
    if (op == 0) {
        XyzzN x = jac_to_xyzz(p);
        xyzz_add(x, jac_to_xyzz(jac_from_words(b + 12 * (size_t)i)));
        xyzz_store_jac_words(o, x);
    } else if (op == 1) {
        AffN q = aff_from_words(b + 8 * (size_t)i);
        XyzzN x = jac_to_xyzz(p);
        xyzz_madd(x, q);
        JacN r2 = jac_madd(p, q);  // both mixed-add forms must agree; disagreement poisons the output
        JacN x1; x1.x = fq_widen<8>(fq_mul(x.x, fq_sqr(x.zz))); x1.y = fq_widen<8>(fq_mul(x.y, fq_sqr(x.zzz))); x1.z = fq_widen<4>(x.zzz);
        if (xyzz_is_inf(x)) x1 = jac_inf();
        if (aff_same(jac_to_aff(x1), jac_to_aff(r2))) jac_store_words(o, r2);
        else { AffN bad; bad.x = fq_widen<2>(fq_one()); bad.y = bad.x; jac_store_words(o, jac_from_aff(bad)); }
    } else if (op == 2) {
        JacN r1 = jac_dbl(p);
        XyzzN x = xyzz_dbl(jac_to_xyzz(p));
        JacN x1; x1.x = fq_widen<8>(fq_mul(x.x, fq_sqr(x.zz))); x1.y = fq_widen<8>(fq_mul(x.y, fq_sqr(x.zzz))); x1.z = fq_widen<4>(x.zzz);
        if (xyzz_is_inf(x)) x1 = jac_inf();
        if (aff_same(jac_to_aff(r1), jac_to_aff(x1))) jac_store_words(o, r1);
        else { AffN bad; bad.x = fq_widen<2>(fq_one()); bad.y = bad.x; jac_store_words(o, jac_from_aff(bad)); }
    } else {
        // p * scalar (Montgomery Fr), MSB-first double-and-add on the affine form of p
        Fe k = fe_from_mont<FrCfg>(fe_load(b + 4 * (size_t)i));
        AffN pa = jac_to_aff(p);
        JacN acc = jac_inf();
#pragma unroll 1
        for (int limb = 7; limb >= 0; limb--) {
            uint32_t word = 0;
#pragma unroll
            for (int q = 0; q < 8; q++) word = (q == limb) ? k.v[q] : word;
#pragma unroll 1
            for (int bit = 31; bit >= 0; bit--) {
                acc = jac_dbl(acc);
                if ((word >> bit) & 1u) acc = jac_madd(acc, pa);
            }
        }
        jac_store_words(o, acc);
    }
}

// the quad-parallel forms of curve_quad.hpp, one point per 4 lanes: op 4 = a + b (XYZZ add), op 5 = 2a, op 6 = a + b where
// every fourth pair is replaced by (a, a) so that general additions and doublings share a wave
__global__ __launch_bounds__(256) void k_test_point_quad(int op, const uint64_t *a, const uint64_t *b, uint32_t n, uint64_t *out) {
    uint32_t t = blockIdx.x * 256 + threadIdx.x;
    uint32_t i = t >> 2;
    int ql = (int)(t & 3);
    bool live = i < n;
    if (!live) i = n - 1;  // keep every lane of the wave busy: the quad forms need whole quads
    XyzzN x = jac_to_xyzz(jac_from_words(a + 12 * (size_t)i));
    XyzzN y = jac_to_xyzz(jac_from_words((op == 5 || (op == 6 && (i & 3) == 3) ? a : b) + 12 * (size_t)i));
    if (op == 5) x = xyzz_dbl_quad(x, ql);
    else xyzz_add_quad(x, y, ql);
    if (live && ql == 0) xyzz_store_jac_words(out + 12 * (size_t)i, x);
}

// ---- raw-limb hooks (dev_lazy_ops.hpp): the caller chooses the representative of every operand, one case per lane
// (*unknown is set where the table of dev_lazy_ops.hpp does not know the operation: the switch there is the only list)
__global__ __launch_bounds__(256) void k_lazy_field(int op, const uint32_t *in, uint32_t n, uint32_t *out, uint32_t *unknown) {
    uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (!lazy_field_op(op, in + (size_t)LAZY_FIELD_IN * i, out + (size_t)LAZY_SLOT * i)) *unknown = 1u;
}
__global__ __launch_bounds__(256) void k_lazy_point(int op, const uint32_t *a, const uint32_t *b, uint32_t n, uint32_t *out, uint32_t *unknown) {
    uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (!lazy_point_op(op, a + (size_t)LAZY_POINT_WORDS * i, b + (size_t)LAZY_POINT_WORDS * i, out + (size_t)LAZY_POINT_WORDS * i)) *unknown = 1u;
}
// the quad-parallel forms of curve_quad.hpp over the same operands, one case per 4 lanes (neighbouring cases share a wave):
// xyzz_add_quad, xyzz_dbl_quad, jac_madd_quad (beta^e = 1; an affine infinity is a dead addition) and jac_dbl_quad.  Every
// lane of a quad holds the result; lane (case mod 4) stores it, so a broadcast that reached only lane 0 would show.
__global__ __launch_bounds__(256) void k_lazy_point_quad(int op, const uint32_t *a, const uint32_t *b, uint32_t n, uint32_t *out) {
    uint32_t t = blockIdx.x * 256 + threadIdx.x;
    uint32_t i = t >> 2;
    int ql = (int)(t & 3);
    bool live = i < n;
    if (!live) i = n - 1;  // whole quads, whole waves: the DPP moves read every lane
    const uint32_t *pa = a + (size_t)LAZY_POINT_WORDS * i, *pb = b + (size_t)LAZY_POINT_WORDS * i;
    uint32_t *o = out + (size_t)LAZY_POINT_WORDS * i;
    bool store = live && ql == (int)(i & 3);
    if (op == LZP_XYZZ_ADD || op == LZP_XYZZ_DBL) {
        XyzzN x = xyzz_load(pa);
        if (op == LZP_XYZZ_ADD) xyzz_add_quad(x, xyzz_load(pb), ql);
        else x = xyzz_dbl_quad(x, ql);
        if (store) xyzz_store(o, x);
    } else {
        JacN p = lz_jac(pa);
        if (op == LZP_JAC_MADD) {
            AffN q = aff_load(pb);
            p = jac_madd_quad(p, q.x, q.y, fq_widen<2>(fq_one()), !aff_is_inf(q), ql);
        } else {
            p = jac_dbl_quad(p, ql);
        }
        if (store) lz_put_jac(o, p);
    }
}

static int test_field_op(halo_ctx *ctx, int field, int op, const uint64_t *d_a, const uint64_t *d_b, size_t n, uint64_t *d_out) {
    dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (field == 2) HALO_LAUNCH(ctx, "k_test_field29", k_test_field29, grid, block, 0, op, d_a, d_b, (uint32_t)n, d_out);
    else if (field == 0) HALO_LAUNCH(ctx, "k_test_field", k_test_field<FqCfg>, grid, block, 0, op, d_a, d_b, (uint32_t)n, d_out);
    else HALO_LAUNCH(ctx, "k_test_field", k_test_field<FrCfg>, grid, block, 0, op, d_a, d_b, (uint32_t)n, d_out);
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}
static int test_point_op(halo_ctx *ctx, int op, const uint64_t *d_a, const uint64_t *d_b, size_t n, uint64_t *d_out) {
    dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (op >= 4) {
        HALO_LAUNCH(ctx, "k_test_point_quad", k_test_point_quad, dim3((unsigned)((4 * n + 255) / 256)), block, 0, op, d_a, d_b, (uint32_t)n, d_out);
        HALO_HIP(hipGetLastError());
        return HALO_OK;
    }
    HALO_LAUNCH(ctx, "k_test_point", k_test_point, grid, block, 0, op, d_a, d_b, (uint32_t)n, d_out);
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}

}  // namespace halo

using namespace halo;

extern "C" {

// what tuning() read from the environment (csrc/tuning.hip), by field name: lets a CPU test pin the parsing
long halo_dev_tuning(const char *name) {
    if (!name) return -1;
    const Tuning &t = tuning();
    if (!std::strcmp(name, "host_split_set")) return t.host_split_set ? 1 : 0;
    if (!std::strcmp(name, "host_pieces")) return t.host_pieces;
    if (!std::strncmp(name, "host_split", 10) && name[10] >= '0' && name[10] <= '3' && !name[11]) return t.host_split[name[10] - '0'];
    if (!std::strcmp(name, "fold_table_after")) return t.fold_table_after;
    if (!std::strcmp(name, "pow_e")) return t.pow_e;
    if (!std::strcmp(name, "dot_blocks")) return t.dot_blocks;
    if (!std::strcmp(name, "spin_us")) return t.spin_us;
    if (!std::strcmp(name, "graphs")) return t.graphs;
    if (!std::strcmp(name, "memory_budget")) return t.memory_budget_set ? (long)(t.memory_budget >> 20) : -1;  // MiB
    if (!std::strcmp(name, "trace")) return t.trace ? 1 : 0;
    if (!std::strcmp(name, "commit_batch_group")) return dev_hooks().commit_group;  // (the hook as it stands: a CPU test sees "reset" clear it)
    if (!std::strcmp(name, "open_batch_fold")) return dev_hooks().open_fold;
    if (!std::strcmp(name, "transcript_min")) return dev_hooks().transcript_min;
    return -1;
}

int halo_dev_hook(const char *name, long value) {
    if (!name) { set_error("dev_hook: null name"); return HALO_E_ARG; }
    DevHooks &h = dev_hooks();
    if (!std::strcmp(name, "table_fail")) h.table_fail = (int)value;
    else if (!std::strcmp(name, "force_peer_copy")) h.force_peer_copy = (int)value;
    else if (!std::strcmp(name, "shard_fail_rank")) h.shard_fail_rank = (int)value;
    else if (!std::strcmp(name, "shard_fail_at")) h.shard_fail_at = (int)value;  // >= 0: a sharded open's collective, -2: check, -3: MSM
    else if (!std::strcmp(name, "batch_stage_fail")) h.batch_stage_fail = (int)value;
    else if (!std::strcmp(name, "check_batch_group")) h.check_group = (int)value;
    else if (!std::strcmp(name, "open_batch_group")) h.open_group = (int)value;
    else if (!std::strcmp(name, "commit_batch_group")) h.commit_group = (int)value;
    else if (!std::strcmp(name, "open_batch_fold")) {
        if (value < 0 || value > 2) { set_error("dev_hook: open_batch_fold is 0 (the measured default), 1 (the folded schedule wherever it applies) or 2 (never: the loop)"); return HALO_E_ARG; }
        h.open_fold = (int)value;
    }
    else if (!std::strcmp(name, "check_combined_parts")) h.combined_parts = value > 0 ? (int)value : 0;
    else if (!std::strcmp(name, "check_combined_cap")) h.combined_cap = value > 0 ? (int)value : 0;
    else if (!std::strcmp(name, "check_combined_usum")) {
        if (value < 0 || value > 2) { set_error("dev_hook: check_combined_usum is 0 (by the member count), 1 (the host pool) or 2 (the device)"); return HALO_E_ARG; }
        h.combined_usum = (int)value;
    }
    else if (!std::strcmp(name, "check_fused_chunk")) {
        if (value != 0 && value < 8) { set_error("dev_hook: check_fused_chunk is 0 (the context's capacity) or at least 8 terms"); return HALO_E_ARG; }
        h.fused_chunk = value > (1 << 30) ? (1 << 30) : (int)value;
    }
    else if (!std::strcmp(name, "verifier_batch_min")) h.verifier_min = (int)value;
    else if (!std::strcmp(name, "transcript_min")) {
        if (value < 0) { set_error("dev_hook: transcript_min is 0 (the measured default) or the member count, at least 1, from which transcripts run on the device"); return HALO_E_ARG; }
        h.transcript_min = value;
    }
    else if (!std::strcmp(name, "decode_batch_min")) h.decode_min = value;
    else if (!std::strcmp(name, "table_slide_min")) h.slide_min = value > 0 && value < 4096 ? 4096 : value;
    else if (!std::strcmp(name, "pow_e")) {
        // (the rule of HALO_POW_E: k_h_coeffs' mid * high factor is wave-uniform only over a power-of-two chain)
        if (value < 4 || value > 64 || (value & (value - 1)) != 0) { set_error("dev_hook: pow_e must be a power of two in [4, 64]"); return HALO_E_ARG; }
        h.pow_e = (int)value;
    } else if (!std::strcmp(name, "dot_blocks")) {
        if (value < 1 || value > (long)FR_GRID_CAP) { set_error("dev_hook: dot_blocks must be in [1, " + std::to_string(FR_GRID_CAP) + "]"); return HALO_E_ARG; }
        h.dot_blocks = (int)value;
    } else if (!std::strcmp(name, "poly_blocks")) {
        if (value < 1 || value > (long)FR_GRID_CAP) { set_error("dev_hook: poly_blocks must be in [1, " + std::to_string(FR_GRID_CAP) + "]"); return HALO_E_ARG; }
        h.poly_blocks = (int)value;
    }
    else if (!std::strcmp(name, "reset")) h = DevHooks();
    else { set_error("dev_hook: unknown hook (table_fail, force_peer_copy, shard_fail_rank, shard_fail_at, batch_stage_fail, check_batch_group, open_batch_group, open_batch_fold, commit_batch_group, check_combined_parts, check_combined_cap, check_combined_usum, check_fused_chunk, verifier_batch_min, transcript_min, decode_batch_min, table_slide_min, pow_e, dot_blocks, poly_blocks, reset)"); return HALO_E_ARG; }
    return HALO_OK;
}

// host only: the launch plan of one Fr kernel family at size n as its launcher computes it NOW (hooks, environment, defaults):
// the plan_* functions of fr_plan.hpp, which are the ones the launchers of fr_vec.hip and hpoly.hip call.  which = 1 is the single open's p(z)
// (fr_poly_eval: up to FR_GRID_CAP blocks), 4 the batched open's (open_batch_table / open_batch_eval: a member's OPEN_PART_WORDS / 4)
int halo_dev_fr_plan(halo_ctx *ctx, int which, size_t n, long out[4]) {
    (void)ctx;  // (no plan depends on the context today)
    if (!out) { set_error("dev_fr_plan: null pointer"); return HALO_E_ARG; }
    FrPlan p;
    if (!fr_plan(which, n, &p)) { set_error("dev_fr_plan: which is 0 powers, 1 poly_eval, 2 dot, 3 h_coeffs, 4 poly_eval of the batched open"); return HALO_E_ARG; }
    out[0] = p.E; out[1] = p.nwin; out[2] = (long)p.blocks; out[3] = (long)p.trips;
    return HALO_OK;
}

// the two dot products of an IPA round (k_dot2_partial with both pairs, fr_dot2) on their own, over vectors of any half length m:
// out = <c_hi, z_lo> | <c_lo, z_hi> for c, z of 2 m elements (tests/test_gpu_fr_plans.py: the rounds themselves only reach powers of two)
int halo_dev_dot2_cross(halo_ctx *ctx, const uint64_t *c, const uint64_t *z, size_t m, uint64_t out[8]) {
    HALO_CTX(ctx);
    if (!out || (m && (!c || !z))) { set_error("dev_dot2_cross: null pointer"); return HALO_E_ARG; }
    if (2 * m > ctx_capacity(ctx)) { set_error("dev_dot2_cross: 2 m exceeds context size"); return HALO_E_ARG; }
    if (m == 0) { std::memset(out, 0, 64); return HALO_OK; }
    int rc = upload_words(ctx, ctx->d_tmp_a, c, m * 8);
    if (!rc) rc = upload_words(ctx, ctx->d_tmp_b, z, m * 8);
    if (rc) return rc;
    host::Fr r[2];
    rc = fr_dot2(ctx, ctx->d_tmp_a + 4 * m, ctx->d_tmp_b, ctx->d_tmp_a, ctx->d_tmp_b + 4 * m, m, r);
    if (rc) return rc;
    r[0].store(out);
    r[1].store(out + 4);
    return HALO_OK;
}

// the check batch's h expansion on its own (tests/test_gpu_check_batch.py holds it against halo_h_coeffs): temporary device
// buffers of this call only
int halo_dev_h_coeffs_batch(halo_ctx *ctx, const uint64_t *xis, size_t m, size_t lg_n, uint64_t *out) {
    HALO_CTX(ctx);
    if (m == 0) return HALO_OK;
    if (!xis || !out) { set_error("h_coeffs_batch: null pointer"); return HALO_E_ARG; }
    if (lg_n > 24 || ((size_t)1 << lg_n) > ctx_capacity(ctx)) { set_error("h_coeffs_batch: 2^lg_n exceeds context size"); return HALO_E_ARG; }
    if (m > 65535) { set_error("h_coeffs_batch: at most 65535 members"); return HALO_E_ARG; }
    const size_t n = (size_t)1 << lg_n, xw = (lg_n + 1) * 4;
    uint64_t *d = nullptr;
    alloc_epoch_bump(ctx);
    HALO_HIP(hipMalloc(&d, (m * (xw + H_TABLES_WORDS + n * 4)) * 8));
    uint64_t *d_xis = d, *d_tabs = d + m * xw, *d_out = d_tabs + m * H_TABLES_WORDS;
    hipError_t e = hipMemcpy(d_xis, xis, m * xw * 8, hipMemcpyHostToDevice);
    int rc = e == hipSuccess ? h_coeffs_batch_dev(ctx, d_xis, m, lg_n, d_tabs, d_out, n * 4) : hip_fail(e, "hipMemcpy");
    if (!rc && (e = hipStreamSynchronize(ctx->stream)) != hipSuccess) rc = hip_fail(e, "hipStreamSynchronize");
    if (!rc && (e = hipMemcpy(out, d_out, m * n * 32, hipMemcpyDeviceToHost)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    (void)hipFree(d);
    return rc;
}

// the prover batch's accumulated polynomials on their own (tests/test_gpu_prover_batch.py holds them against the oracle's
// h_coeffs): temporary device and pinned buffers of this call only
int halo_dev_h_accumulate_batch(halo_ctx *ctx, const uint64_t *h0s, const uint64_t *xis, const uint64_t *alphas, const size_t *counts, size_t members,
                                size_t lg_n, size_t max_tables, uint64_t *out) {
    HALO_CTX(ctx);
    if (members == 0) return HALO_OK;
    if (!h0s || !counts || !out) { set_error("h_accumulate_batch: null pointer"); return HALO_E_ARG; }
    if (lg_n < 1 || lg_n > 24 || ((size_t)1 << lg_n) > ctx_capacity(ctx)) { set_error("h_accumulate_batch: 2^lg_n exceeds context size"); return HALO_E_ARG; }
    if (members > 65535) { set_error("h_accumulate_batch: at most 65535 members"); return HALO_E_ARG; }
    const size_t n = (size_t)1 << lg_n, xw = (lg_n + 1) * 4;
    size_t total = 0;
    for (size_t j = 0; j < members; ++j) {
        if (counts[j] > 65535 - total) { set_error("h_accumulate_batch: at most 65535 polynomials"); return HALO_E_ARG; }
        total += counts[j];
    }
    if (total && (!xis || !alphas)) { set_error("h_accumulate_batch: null pointer"); return HALO_E_ARG; }
    std::vector<host::Fr> h0(2 * members), x(total * (lg_n + 1)), a(total);
    for (size_t i = 0; i < h0.size(); ++i) h0[i] = host::Fr::load(h0s + 4 * i);
    for (size_t i = 0; i < x.size(); ++i) x[i] = host::Fr::load(xis + 4 * i);
    for (size_t i = 0; i < total; ++i) a[i] = host::Fr::load(alphas + 4 * i);
    std::vector<HAccMember> mem(members);
    for (size_t j = 0, t = 0; j < members; t += counts[j], ++j) {
        mem[j].h0 = &h0[2 * j];
        mem[j].count = counts[j];
        mem[j].scales = a.data() + t;
        for (size_t i = 0; i < counts[j]; ++i) mem[j].xis.push_back(x.data() + (t + i) * (xw / 4));
    }
    const size_t cap = max_tables ? max_tables : (total ? total : 1);
    uint64_t *d = nullptr, *h = nullptr;
    alloc_epoch_bump(ctx);
    HALO_HIP(hipMalloc(&d, (hacc_stage_words(members, lg_n, cap) + members * n * 4) * 8));
    hipError_t e = hipHostMalloc(&h, hacc_pin_words(members, lg_n, cap) * 8);
    if (e != hipSuccess) { (void)hipFree(d); return hip_fail(e, "hipHostMalloc"); }
    uint64_t *d_out = d + hacc_stage_words(members, lg_n, cap);
    int rc = h_accumulate_group(ctx, mem.data(), members, lg_n, cap, h, d, d_out, n * 4);
    if (!rc && (e = hipStreamSynchronize(ctx->stream)) != hipSuccess) rc = hip_fail(e, "hipStreamSynchronize");
    if (!rc && (e = hipMemcpy(out, d_out, members * n * 32, hipMemcpyDeviceToHost)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    if (rc) (void)hipStreamSynchronize(ctx->stream);
    (void)hipHostFree(h);
    (void)hipFree(d);
    return rc;
}

// host only: the weights of the combined check batch as the product computes them (tests/test_check_combined_cpu.py restates the rule)
int halo_dev_check_weights(const uint64_t *blobs, size_t stride_words, const size_t *idx, size_t A, size_t d, const uint8_t seed[32], uint64_t *out) {
    if (A == 0) return HALO_OK;
    if (!blobs || !idx || !out) { set_error("check_weights: null pointer"); return HALO_E_ARG; }
    if (!is_pow2(d + 1) || stride_words < instance_words(ilog2(d + 1))) { set_error("check_weights: d + 1 is a power of two, the stride at least an Instance"); return HALO_E_ARG; }
    std::vector<host::Fr> r;
    check_combined_weights(blobs, stride_words, idx, A, d, seed, r);
    for (size_t a = 0; a < A; ++a) r[a].store(out + 4 * a);
    return HALO_OK;
}

// the combined check's scalar step on its own (tests/test_gpu_check_combined.py holds it against Python integers): temporary
// device buffers of this call only
int halo_dev_check_combined_scalars(halo_ctx *ctx, const uint64_t *xis, const uint64_t *weights, size_t A, size_t lg_n, uint64_t *out) {
    HALO_CTX(ctx);
    if (!xis || !weights || !out) { set_error("check_combined_scalars: null pointer"); return HALO_E_ARG; }
    if (A < 1 || A > 65535) { set_error("check_combined_scalars: 1..65535 polynomials"); return HALO_E_ARG; }
    if (lg_n < 1 || lg_n > 24 || ((size_t)1 << lg_n) > ctx_capacity(ctx)) { set_error("check_combined_scalars: 2^lg_n exceeds context size"); return HALO_E_ARG; }
    const size_t n = (size_t)1 << lg_n, xw = (lg_n + 1) * 4, tw = xw + 4;
    const size_t P = check_combined_parts(n, A), cap = check_combined_cap(A);
    std::vector<uint64_t> recs(A * tw);
    for (size_t a = 0; a < A; ++a) {
        std::memcpy(&recs[a * tw], xis + a * xw, xw * 8);
        std::memcpy(&recs[a * tw + xw], weights + 4 * a, 32);
    }
    uint64_t *d = nullptr;
    alloc_epoch_bump(ctx);
    HALO_HIP(hipMalloc(&d, hcomb_stage_words(A, lg_n, P, cap) * 8));
    int rc = h_combine_rows(ctx, recs.data(), A, lg_n, P, cap, d);
    hipError_t e = hipStreamSynchronize(ctx->stream);  // (also on failure: nothing of this call may be in flight when its buffer goes)
    if (!rc && e != hipSuccess) rc = hip_fail(e, "hipStreamSynchronize");
    if (!rc && (e = hipMemcpy(out, d + hcomb_rows_offset(A, lg_n, P, cap), n * 32, hipMemcpyDeviceToHost)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    (void)hipFree(d);
    return rc;
}

// host only: the weights of the mixed combined check batch as the product computes them (tests/test_check_mixed_cpu.py restates the rule)
int halo_dev_check_mixed_weights(const uint64_t *const *blobs, const size_t *ds, const size_t *idx, size_t A, const uint8_t seed[32], uint64_t *out) {
    if (A == 0) return HALO_OK;
    if (!blobs || !ds || !idx || !out) { set_error("check_mixed_weights: null pointer"); return HALO_E_ARG; }
    for (size_t a = 0; a < A; ++a) {
        if (!blobs[idx[a]]) { set_error("check_mixed_weights: null pointer"); return HALO_E_ARG; }
        if (!is_pow2(ds[idx[a]] + 1)) { set_error("check_mixed_weights: every d + 1 is a power of two"); return HALO_E_ARG; }
    }
    std::vector<host::Fr> r;
    check_mixed_weights(blobs, ds, idx, A, seed, r);
    for (size_t a = 0; a < A; ++a) r[a].store(out + 4 * a);
    return HALO_OK;
}

// the mixed combined check's scalar step on its own (tests/test_gpu_check_mixed.py holds it against Python integers): the tables in
// the caller's order -- the launcher sorts --, temporary device buffers of this call only
int halo_dev_check_mixed_scalars(halo_ctx *ctx, const uint64_t *xis, const size_t *lgs, const uint64_t *weights, size_t A, uint64_t *out) {
    HALO_CTX(ctx);
    if (!xis || !lgs || !weights || !out) { set_error("check_mixed_scalars: null pointer"); return HALO_E_ARG; }
    if (A < 1 || A > 65535) { set_error("check_mixed_scalars: 1..65535 polynomials"); return HALO_E_ARG; }
    size_t lg_max = 0;
    for (size_t a = 0; a < A; ++a) {
        if (lgs[a] < 1 || lgs[a] > 24 || ((size_t)1 << lgs[a]) > ctx_capacity(ctx)) { set_error("check_mixed_scalars: 2^lg_n exceeds context size"); return HALO_E_ARG; }
        if (lgs[a] > lg_max) lg_max = lgs[a];
    }
    const size_t n = (size_t)1 << lg_max, xw = (lg_max + 1) * 4, tw = xw + 4;
    const size_t P = check_combined_parts(n, A), cap = check_combined_cap(A);
    std::vector<uint64_t> recs(A * tw, 0);
    std::vector<uint32_t> lg32(A);
    for (size_t a = 0; a < A; ++a) {
        lg32[a] = (uint32_t)lgs[a];
        std::memcpy(&recs[a * tw], xis + a * xw, (lgs[a] + 1) * 32);
        std::memcpy(&recs[a * tw + (lgs[a] + 1) * 4], weights + 4 * a, 32);
    }
    uint64_t *d = nullptr;
    alloc_epoch_bump(ctx);
    HALO_HIP(hipMalloc(&d, hmix_stage_words(A, lg_max, P, cap) * 8));
    int rc = h_combine_rows_mixed(ctx, recs.data(), lg32.data(), A, lg_max, P, cap, d);
    hipError_t e = hipStreamSynchronize(ctx->stream);  // (also on failure: nothing of this call may be in flight when its buffer goes)
    if (!rc && e != hipSuccess) rc = hip_fail(e, "hipStreamSynchronize");
    if (!rc && (e = hipMemcpy(out, d + hmix_rows_offset(A, lg_max, P, cap), n * 32, hipMemcpyDeviceToHost)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    (void)hipFree(d);
    return rc;
}

// host only: the 2 A weights r_0, s_0, r_1, s_1, .. of the fused check batch as the product computes them (tests/test_check_fused_cpu.py
// restates the rule)
int halo_dev_check_fused_weights(const uint64_t *blobs, size_t stride_words, const size_t *idx, size_t A, size_t d, const uint8_t seed[32], uint64_t *out) {
    if (A == 0) return HALO_OK;
    if (!blobs || !idx || !out) { set_error("check_fused_weights: null pointer"); return HALO_E_ARG; }
    if (!is_pow2(d + 1) || stride_words < instance_words(ilog2(d + 1))) { set_error("check_fused_weights: d + 1 is a power of two, the stride at least an Instance"); return HALO_E_ARG; }
    std::vector<host::Fr> w;
    check_fused_weights(blobs, stride_words, idx, A, d, seed, w);
    for (size_t k = 0; k < 2 * A; ++k) w[k].store(out + 4 * k);
    return HALO_OK;
}

// the fused check's term kernel on its own (tests/test_gpu_check_fused.py holds it against Python integers): M records of
// lg_n + 6 Montgomery elements (xi_0 .. xi_lg | z | v | c | r | s) -> M x (2 lg_n + 2) canonical scalars and H's scalar; temporary
// device buffers of this call only
int halo_dev_check_fused_terms(halo_ctx *ctx, const uint64_t *recs, size_t M, size_t lg_n, uint64_t *scalars_out, uint64_t h_out[4]) {
    HALO_CTX(ctx);
    if (!recs || !scalars_out || !h_out) { set_error("check_fused_terms: null pointer"); return HALO_E_ARG; }
    if (M < 1 || M > 65535) { set_error("check_fused_terms: 1..65535 members"); return HALO_E_ARG; }
    if (lg_n < 1 || lg_n > 24) { set_error("check_fused_terms: lg n must be in 1..24"); return HALO_E_ARG; }
    const size_t rw = (lg_n + 6) * 4, K = 2 * lg_n + 2;
    uint64_t *d = nullptr;
    alloc_epoch_bump(ctx);
    HALO_HIP(hipMalloc(&d, (M * (rw + 4 + K * 4) + 4) * 8));
    uint64_t *d_recs = d, *d_shares = d + M * rw, *d_sc = d_shares + M * 4, *d_h = d_sc + M * K * 4;
    hipError_t e = hipMemcpy(d_recs, recs, M * rw * 8, hipMemcpyHostToDevice);
    int rc = e == hipSuccess ? fused_terms(ctx, d_recs, M, lg_n, nullptr, d_sc, d_shares, d_h) : hip_fail(e, "hipMemcpy");
    e = hipStreamSynchronize(ctx->stream);  // (also on failure: nothing of this call may be in flight when its buffer goes)
    if (!rc && e != hipSuccess) rc = hip_fail(e, "hipStreamSynchronize");
    if (!rc && (e = hipMemcpy(scalars_out, d_sc, M * K * 32, hipMemcpyDeviceToHost)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    if (!rc && (e = hipMemcpy(h_out, d_h, 32, hipMemcpyDeviceToHost)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    (void)hipFree(d);
    return rc;
}

// host only: the 2 A weights of the mixed fused check batch as the product computes them (tests/test_check_mixed_fused_cpu.py restates
// the rule)
int halo_dev_check_mixed_fused_weights(const uint64_t *const *blobs, const size_t *ds, const size_t *idx, size_t A, const uint8_t seed[32], uint64_t *out) {
    if (A == 0) return HALO_OK;
    if (!blobs || !ds || !idx || !out) { set_error("check_mixed_fused_weights: null pointer"); return HALO_E_ARG; }
    for (size_t a = 0; a < A; ++a) {
        if (!blobs[idx[a]]) { set_error("check_mixed_fused_weights: null pointer"); return HALO_E_ARG; }
        if (!is_pow2(ds[idx[a]] + 1)) { set_error("check_mixed_fused_weights: every d + 1 is a power of two"); return HALO_E_ARG; }
    }
    std::vector<host::Fr> w;
    check_mixed_fused_weights(blobs, ds, idx, A, seed, w);
    for (size_t k = 0; k < 2 * A; ++k) w[k].store(out + 4 * k);
    return HALO_OK;
}

// the mixed fused check's term kernel on its own (tests/test_gpu_check_mixed_fused.py holds it against Python integers): M dense
// records of lgs[a] + 6 Montgomery elements -> the members' dense scalars and H's scalar; temporary device buffers of this call only
int halo_dev_check_mixed_terms(halo_ctx *ctx, const uint64_t *recs, const size_t *lgs, size_t M, uint64_t *scalars_out, uint64_t h_out[4]) {
    HALO_CTX(ctx);
    if (!recs || !lgs || !scalars_out || !h_out) { set_error("check_mixed_terms: null pointer"); return HALO_E_ARG; }
    if (M < 1 || M > 65535) { set_error("check_mixed_terms: 1..65535 members"); return HALO_E_ARG; }
    std::vector<uint32_t> lg32(M), desc(M * MIXED_DESC_WORDS);
    for (size_t a = 0; a < M; ++a) {
        if (lgs[a] < 1 || lgs[a] > (size_t)FUSED_MAX_LG) { set_error("check_mixed_terms: lg n must be in 1..24"); return HALO_E_ARG; }
        lg32[a] = (uint32_t)lgs[a];
    }
    size_t rw = 0, terms = 0;
    mixed_terms_describe(lg32.data(), M, desc.data(), &rw, &terms);
    const size_t dw = ((desc.size() + 1) / 2 + 3) & ~(size_t)3;  // the descriptors in 64-bit words, the regions behind them 32-byte aligned
    uint64_t *d = nullptr;
    alloc_epoch_bump(ctx);
    HALO_HIP(hipMalloc(&d, (rw + M * 4 + dw + terms * 4 + 4) * 8));
    uint64_t *d_recs = d, *d_shares = d + rw, *d_desc = d_shares + M * 4, *d_sc = d_desc + dw, *d_h = d_sc + terms * 4;
    hipError_t e = hipMemcpy(d_recs, recs, rw * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_desc, desc.data(), desc.size() * 4, hipMemcpyHostToDevice);
    int rc = e == hipSuccess ? fused_terms(ctx, d_recs, M, 0, reinterpret_cast<const uint32_t *>(d_desc), d_sc, d_shares, d_h) : hip_fail(e, "hipMemcpy");
    e = hipStreamSynchronize(ctx->stream);  // (also on failure: nothing of this call may be in flight when its buffer goes)
    if (!rc && e != hipSuccess) rc = hip_fail(e, "hipStreamSynchronize");
    if (!rc && (e = hipMemcpy(scalars_out, d_sc, terms * 32, hipMemcpyDeviceToHost)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    if (!rc && (e = hipMemcpy(h_out, d_h, 32, hipMemcpyDeviceToHost)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    (void)hipFree(d);
    return rc;
}

// the verifier batch's segmented sums on their own (tests/test_gpu_verifier_batch.py holds them against the oracle): one
// k_small_msm_seg launch over nsums sums of lens[s] in 1..64 terms, temporary device buffers of this call only
int halo_dev_small_msm_seg(halo_ctx *ctx, const uint64_t *points, const uint64_t *scalars, const size_t *lens, size_t nsums, uint64_t *out_jac) {
    HALO_CTX(ctx);
    if (nsums == 0) return HALO_OK;
    if (!points || !scalars || !lens || !out_jac) { set_error("small_msm_seg: null pointer"); return HALO_E_ARG; }
    if (nsums >= ((size_t)1 << 20)) { set_error("small_msm_seg: too many sums"); return HALO_E_ARG; }
    std::vector<uint32_t> off{0};
    for (size_t s = 0; s < nsums; ++s) {
        if (lens[s] < 1 || lens[s] > 64) { set_error("small_msm_seg: 1..64 terms per sum"); return HALO_E_ARG; }
        off.push_back(off.back() + (uint32_t)lens[s]);
    }
    const size_t nterms = off.back();
    std::vector<uint32_t> desc;
    const size_t waves = small_msm_seg_plan(off.data(), nsums, desc);
    uint64_t *d = nullptr;
    alloc_epoch_bump(ctx);
    HALO_HIP(hipMalloc(&d, nterms * 96 + nsums * 96 + off.size() * 4 + desc.size() * 4));
    uint64_t *d_pts = d, *d_sc = d_pts + nterms * 8, *d_out = d_sc + nterms * 4;
    uint32_t *d_off = reinterpret_cast<uint32_t *>(d_out + nsums * 12), *d_desc = d_off + off.size();
    hipError_t e = hipMemcpy(d_pts, points, nterms * 64, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_sc, scalars, nterms * 32, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_off, off.data(), off.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_desc, desc.data(), desc.size() * 4, hipMemcpyHostToDevice);
    int rc = e == hipSuccess ? small_msm_seg(ctx, d_pts, d_sc, d_off, d_desc, waves, d_out) : hip_fail(e, "hipMemcpy");
    if (!rc && (e = hipStreamSynchronize(ctx->stream)) != hipSuccess) rc = hip_fail(e, "hipStreamSynchronize");
    if (!rc && (e = hipMemcpy(out_jac, d_out, nsums * 96, hipMemcpyDeviceToHost)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    (void)hipFree(d);
    return rc;
}

// the relation kernel of the device-side succinct checks on its own (tests/test_gpu_point_paths.py holds it against the oracle):
// one k_batch_small_msm launch through the product's batch_small_msm, m sums of K terms each, temporary device buffers of this
// call only
int halo_dev_batch_small_msm(halo_ctx *ctx, const uint64_t *points, const uint64_t *scalars, size_t m, size_t K, uint64_t *out_jac) {
    HALO_CTX(ctx);
    if (m == 0) return HALO_OK;
    if (!points || !scalars || !out_jac) { set_error("batch_small_msm: null pointer"); return HALO_E_ARG; }
    if (m > 65535) { set_error("batch_small_msm: at most 65535 sums"); return HALO_E_ARG; }
    if (K == 0 || K > 64) return batch_small_msm(ctx, nullptr, nullptr, m, K, nullptr);  // (the product's refusal, before any launch)
    const size_t nterms = m * K;
    uint64_t *d = nullptr;
    alloc_epoch_bump(ctx);
    HALO_HIP(hipMalloc(&d, nterms * 96 + m * 96));
    uint64_t *d_pts = d, *d_sc = d_pts + nterms * 8, *d_out = d_sc + nterms * 4;
    hipError_t e = hipMemcpy(d_pts, points, nterms * 64, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_sc, scalars, nterms * 32, hipMemcpyHostToDevice);
    int rc = e == hipSuccess ? batch_small_msm(ctx, d_pts, d_sc, m, K, d_out) : hip_fail(e, "hipMemcpy");
    if (!rc && (e = hipStreamSynchronize(ctx->stream)) != hipSuccess) rc = hip_fail(e, "hipStreamSynchronize");
    if (!rc && (e = hipMemcpy(out_jac, d_out, m * 96, hipMemcpyDeviceToHost)) != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    (void)hipFree(d);
    return rc;
}

// the succinct check's transcripts of m Instances on their own, on the host pool (succinct_challenges) or through the product's
// transcripts_batch_dev whatever the threshold (tests/test_gpu_transcripts.py holds the two against each other word for word)
int halo_dev_transcripts(halo_ctx *ctx, size_t d, const uint64_t *instances, size_t m, int on_device, uint64_t *xis_out, uint64_t *cprime_out,
                         int *status_out) {
    HALO_CTX(ctx);
    if (m == 0) return HALO_OK;
    if (!instances || !xis_out || !cprime_out || !status_out) { set_error("dev_transcripts: null pointer"); return HALO_E_ARG; }
    if (!is_pow2(d + 1)) { set_error("dev_transcripts: d + 1 is not a power of two"); return HALO_E_ARG; }
    const size_t lg = ilog2(d + 1), iw = instance_words(lg);
    const BlobAt blob_at = [&](size_t i) { return instances + i * iw; };
    std::vector<BatchCheck> res;
    if (on_device) {
        int rc = transcripts_batch_dev(ctx, d, blob_at, m, res, false);
        if (rc == kTranscriptNoStage) { set_error("dev_transcripts: the staging was refused"); return HALO_E_DEVICE; }
        if (rc) return rc;
    } else {
        res.assign(m, BatchCheck());
        pool_run(m, [&](size_t i) {
            const uint64_t *q = blob_at(i);
            res[i].rc = succinct_challenges(ctx, host::Point::load(q), (size_t)q[12], host::Fr::load(q + 13), host::Fr::load(q + 17), q + 21, &res[i].st, false);
            if (res[i].rc) res[i].err = halo_last_error();
        });
    }
    for (size_t i = 0; i < m; ++i) {
        uint64_t *xs = xis_out + i * (lg + 1) * 4, *cp = cprime_out + i * 12;
        std::memset(xs, 0, (lg + 1) * 32);
        std::memset(cp, 0, 96);
        const std::string &e = res[i].err;
        status_out[i] = !res[i].rc ? 0 : !e.compare(0, 8, "instance") ? 1 : !e.compare(0, 11, "proof holds") ? 2 : !e.compare(0, 9, "challenge") ? 3 : 4;
        if (res[i].rc) continue;
        for (size_t k = 0; k <= lg; ++k) res[i].st.xis[k].store(xs + 4 * k);
        res[i].st.C_prime.store_normalized(cp);
    }
    return HALO_OK;
}

// halo_msm_points' normalisation on its own (tests/test_gpu_point_paths.py holds every output against Python integers): upload,
// the product's batch_to_affine (k_batch_to_affine), k_native_to_aff, download; temporary device buffers of this call only
int halo_dev_batch_to_affine(halo_ctx *ctx, const uint64_t *pts_jac, size_t m, uint64_t *out_affine) {
    HALO_CTX(ctx);
    if (m == 0) return HALO_OK;
    if (!pts_jac || !out_affine) { set_error("dev_batch_to_affine: null pointer"); return HALO_E_ARG; }
    if (m > ((size_t)1 << 22)) { set_error("dev_batch_to_affine: at most 2^22 points"); return HALO_E_ARG; }
    uint64_t *d = nullptr;
    alloc_epoch_bump(ctx);
    HALO_HIP(hipMalloc(&d, m * (96 + 64) + m * (size_t)AFF_STRIDE * 4));
    uint64_t *d_jac = d, *d_out = d_jac + m * 12;
    uint32_t *d_native = reinterpret_cast<uint32_t *>(d_out + m * 8);  // (every part a multiple of 32 bytes)
    hipError_t e = hipMemcpyAsync(d_jac, pts_jac, m * 96, hipMemcpyHostToDevice, ctx->stream);
    int rc = e == hipSuccess ? batch_to_affine(ctx, d_jac, m, d_native) : hip_fail(e, "hipMemcpyAsync");
    if (!rc) rc = aff_native_to_words(ctx, d_native, m, d_out);
    if (!rc && (e = hipMemcpyAsync(out_affine, d_out, m * 64, hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess) rc = hip_fail(e, "hipMemcpyAsync");
    e = hipStreamSynchronize(ctx->stream);  // (also on failure: nothing of this call may be in flight when its buffers go)
    if (!rc && e != hipSuccess) rc = hip_fail(e, "hipStreamSynchronize");
    (void)hipFree(d);
    return rc;
}

// the decode batch's square root in Fq (k_fq_sqrt, the routine of k_point_decompress) on its own (tests/test_gpu_decode_batch.py
// holds it against Python integers): temporary device buffers of this call only
int halo_dev_fq_sqrt(halo_ctx *ctx, const uint64_t *a, size_t m, uint64_t *root_out, uint32_t *ok_out) {
    HALO_CTX(ctx);
    if (m == 0) return HALO_OK;
    if (!a || !root_out || !ok_out) { set_error("fq_sqrt: null pointer"); return HALO_E_ARG; }
    if (m > ((size_t)1 << 22)) { set_error("fq_sqrt: at most 2^22 elements"); return HALO_E_ARG; }
    const uint32_t *tab = sqrt_tables_host();
    if (!tab) { set_error("fq_sqrt: the torsion tables could not be built"); return HALO_E_DEVICE; }
    uint64_t *d = nullptr;
    alloc_epoch_bump(ctx);
    HALO_HIP(hipMalloc(&d, m * 64 + SQRT_TAB_WORDS * 4 + m * 4));
    uint64_t *d_a = d, *d_root = d + 4 * m;
    uint32_t *d_tab = reinterpret_cast<uint32_t *>(d_root + 4 * m), *d_ok = d_tab + SQRT_TAB_WORDS;  // (the tables 16-byte aligned)
    hipError_t e = hipMemcpyAsync(d_a, a, m * 32, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_tab, tab, SQRT_TAB_WORDS * 4, hipMemcpyHostToDevice, ctx->stream);
    int rc = e == hipSuccess ? fq_sqrt_dev(ctx, d_a, m, d_tab, d_root, d_ok) : hip_fail(e, "hipMemcpyAsync");
    if (!rc && (e = hipMemcpyAsync(root_out, d_root, m * 32, hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess) rc = hip_fail(e, "hipMemcpyAsync");
    if (!rc && (e = hipMemcpyAsync(ok_out, d_ok, m * 4, hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess) rc = hip_fail(e, "hipMemcpyAsync");
    e = hipStreamSynchronize(ctx->stream);  // (also on failure: nothing of this call may be in flight when its buffers go)
    if (!rc && e != hipSuccess) rc = hip_fail(e, "hipStreamSynchronize");
    (void)hipFree(d);
    return rc;
}

// host only: the torsion tables of that square root as the kernels get them (tests/test_decompress_host.py)
int halo_dev_sqrt_tables(uint32_t *out, size_t cap_words) {
    const uint32_t *tab = sqrt_tables_host();
    if (!out || cap_words < SQRT_TAB_WORDS || !tab) { set_error("sqrt_tables: null pointer, fewer than 8448 words, or no tables"); return HALO_E_ARG; }
    std::memcpy(out, tab, SQRT_TAB_WORDS * 4);
    return HALO_OK;
}

int halo_bench_fr_kernel(halo_ctx *ctx, int which, size_t n, int reps) {
    HALO_CTX(ctx);
    return bench_fr_kernel(ctx, which, n, reps);
}

int halo_test_glv_digits(const uint64_t xi[4], uint8_t out[144], int *n_out) {
    if (!xi || !out || !n_out) { set_error("glv_digits: null pointer"); return HALO_E_ARG; }
    host::GlvDigits dg = host::glv_digits(host::Fr::load(xi));
    for (int i = 0; i < 144; ++i) out[i] = i < dg.n ? dg.d[i] : 0;
    *n_out = dg.n;
    return HALO_OK;
}

int halo_test_fold_digits(const uint64_t s[4], int8_t out[44]) {
    if (!s || !out) { set_error("fold_digits: null pointer"); return HALO_E_ARG; }
    fold_digits_host(host::Fr::load(s), out);
    return HALO_OK;
}

int halo_set_graphs(halo_ctx *ctx, int on) {
    if (!ctx) { set_error("null context"); return HALO_E_ARG; }
    ctx->use_graphs = on != 0;
    for (halo_ctx *sh : ctx->shards) (void)halo_set_graphs(sh, on);  // a multi-device context: its shards run the MSMs
    return HALO_OK;
}

int halo_set_ipa_switch(halo_ctx *ctx, size_t size) {
    if (!ctx) { set_error("null context"); return HALO_E_ARG; }
    ctx->nofold_size = size;
    return HALO_OK;
}

int halo_set_window_bits(halo_ctx *ctx, int c) {
    if (!ctx || (c != 0 && (c < 4 || c > 16))) { set_error("window bits must be 0 or in [4, 16]"); return HALO_E_ARG; }
    ctx->window_bits = c;
    for (halo_ctx *sh : ctx->shards) (void)halo_set_window_bits(sh, c);  // a multi-device context: its shards run the MSMs
    return HALO_OK;
}

int halo_set_reduce_span(halo_ctx *ctx, int span) {
    if (!ctx || span < 0 || span > 512 || (span & (span - 1))) { set_error("reduce span must be 0 or a power of two <= 512"); return HALO_E_ARG; }
    ctx->reduce_span = span;
    for (halo_ctx *sh : ctx->shards) (void)halo_set_reduce_span(sh, span);  // a multi-device context: its shards run the MSMs
    return HALO_OK;
}

int halo_set_sort_mode(halo_ctx *ctx, int mode) {
    if (!ctx || mode < -1 || mode > 1) { set_error("sort mode must be -1 (automatic), 0 (one level) or 1 (two levels)"); return HALO_E_ARG; }
    ctx->sort_two_level = mode;
    for (halo_ctx *sh : ctx->shards) (void)halo_set_sort_mode(sh, mode);  // a multi-device context: its shards run the MSMs
    return HALO_OK;
}

int halo_set_small_path(halo_ctx *ctx, int mode) {
    if (!ctx || mode < -1 || mode > 0) { set_error("small path mode must be -1 (automatic) or 0 (never)"); return HALO_E_ARG; }
    ctx->small_path = mode;
    for (halo_ctx *sh : ctx->shards) (void)halo_set_small_path(sh, mode);  // a multi-device context: its shards run the MSMs
    return HALO_OK;
}

int halo_set_batch_verify(halo_ctx *ctx, int on) {
    if (!ctx) { set_error("null context"); return HALO_E_ARG; }
    ctx->batch_verify = on != 0;
    return HALO_OK;
}

int halo_set_fold_levels(halo_ctx *ctx, int levels) {
    if (!ctx || (levels != 1 && levels != 2)) { set_error("fold levels must be 1 or 2"); return HALO_E_ARG; }
    ctx->fold_levels = levels;
    return HALO_OK;
}

int halo_set_fold_async(halo_ctx *ctx, int mode) {
    if (!ctx || mode < -1 || mode > 1) { set_error("fold async mode must be -1 (automatic), 0 (never) or 1 (wherever possible)"); return HALO_E_ARG; }
    ctx->fold_async = mode;
    return HALO_OK;
}

int halo_set_task_len(halo_ctx *ctx, int len) {
    if (!ctx || !(len == 0 || len == 8 || len == 16 || len == 32 || len == 64)) { set_error("task length must be 0, 8, 16, 32 or 64"); return HALO_E_ARG; }
    ctx->task_len = len;
    for (halo_ctx *sh : ctx->shards) (void)halo_set_task_len(sh, len);  // a multi-device context: its shards run the MSMs
    return HALO_OK;
}

int halo_test_field_op(halo_ctx *ctx, int field, int op, const uint64_t *a, const uint64_t *b, size_t n, uint64_t *out) {
    HALO_CTX(ctx);
    if (n > ctx_capacity(ctx)) { set_error("test_field_op: n exceeds context size"); return HALO_E_ARG; }
    int rc = upload_words(ctx, ctx->d_tmp_a, a, n * 4);
    if (!rc && b) rc = upload_words(ctx, ctx->d_tmp_b, b, n * 4);
    if (rc) return rc;
    rc = test_field_op(ctx, field, op, ctx->d_tmp_a, b ? ctx->d_tmp_b : nullptr, n, ctx->d_tmp_a + 4 * n);
    if (rc) return rc;
    return download_words(ctx, out, ctx->d_tmp_a + 4 * n, n * 4);
}

int halo_test_point_op(halo_ctx *ctx, int op, const uint64_t *a_jac, const uint64_t *b, size_t n, uint64_t *out_jac) {
    HALO_CTX(ctx);
    if (n > ctx_capacity(ctx) / 2) { set_error("test_point_op: n exceeds half the context size"); return HALO_E_ARG; }
    size_t bw = (op == 0 || op == 4 || op == 6) ? 12 : (op == 1 ? 8 : 4);
    int rc = upload_words(ctx, ctx->d_tmp_a, a_jac, n * 12);
    if (!rc && b && op != 2 && op != 5) rc = upload_words(ctx, ctx->d_tmp_b, b, n * bw);
    if (rc) return rc;
    // output goes to the upper half of d_tmp_a? keep it simple: a dedicated allocation
    uint64_t *d_out = nullptr;
    HALO_HIP(hipMalloc(&d_out, n * 96));
    rc = test_point_op(ctx, op, ctx->d_tmp_a, ctx->d_tmp_b, n, d_out);
    if (!rc) rc = download_words(ctx, out_jac, d_out, n * 12);
    (void)hipFree(d_out);
    if (rc) return rc;
    for (size_t i = 0; i < n; ++i) host::Point::load(out_jac + 12 * i).store_normalized(out_jac + 12 * i);
    return HALO_OK;
}

// n cases of one operation of dev_lazy_ops.hpp over caller-chosen limbs: temporary device buffers of this call only, every
// copy and the launch in order on the context's stream.  kind 0: field (no second operand), 1: point, 2: point, quad forms.
static int lazy_run(halo_ctx *ctx, int kind, int op, const uint32_t *a, const uint32_t *b, size_t n, uint32_t *out) {
    const size_t in_words = n * (kind == 0 ? (size_t)LAZY_FIELD_IN : (size_t)LAZY_POINT_WORDS);
    const size_t out_words = n * (kind == 0 ? (size_t)LAZY_SLOT : (size_t)LAZY_POINT_WORDS);
    const size_t b_words = b ? in_words : 0;
    uint32_t *d = nullptr, unknown = 0;
    alloc_epoch_bump(ctx);
    HALO_HIP(hipMalloc(&d, (in_words + b_words + out_words + 4) * 4));
    uint32_t *d_a = d, *d_b = d_a + in_words, *d_out = d_b + b_words, *d_unknown = d_out + out_words;  // (every part a multiple of 16 bytes)
    hipError_t e = hipMemcpyAsync(d_a, a, in_words * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess && b) e = hipMemcpyAsync(d_b, b, b_words * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_unknown, 0, 16, ctx->stream);
    int rc = e == hipSuccess ? HALO_OK : hip_fail(e, "hipMemcpyAsync");
    if (!rc) {
        dim3 block(256), grid((unsigned)((n + 255) / 256)), qgrid((unsigned)((4 * n + 255) / 256));
        if (kind == 0) HALO_LAUNCH(ctx, "k_lazy_field", k_lazy_field, grid, block, 0, op, d_a, (uint32_t)n, d_out, d_unknown);
        else if (kind == 1) HALO_LAUNCH(ctx, "k_lazy_point", k_lazy_point, grid, block, 0, op, d_a, d_b, (uint32_t)n, d_out, d_unknown);
        else HALO_LAUNCH(ctx, "k_lazy_point_quad", k_lazy_point_quad, qgrid, block, 0, op, d_a, d_b, (uint32_t)n, d_out);
        if ((e = hipGetLastError()) != hipSuccess) rc = hip_fail(e, "launch");
    }
    if (!rc && (e = hipMemcpyAsync(out, d_out, out_words * 4, hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess) rc = hip_fail(e, "hipMemcpyAsync");
    if (!rc && (e = hipMemcpyAsync(&unknown, d_unknown, 4, hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess) rc = hip_fail(e, "hipMemcpyAsync");
    e = hipStreamSynchronize(ctx->stream);  // (also on failure: nothing of this call may be in flight when its buffers go)
    if (!rc && e != hipSuccess) rc = hip_fail(e, "hipStreamSynchronize");
    (void)hipFree(d);
    if (!rc && unknown) { set_error("test_lazy_op: unknown operation"); rc = HALO_E_ARG; }
    return rc;
}

// One point fold through the product's launcher over a key of the caller's choice, in a kernel form of the caller's choice
// (include/halo_accumulation_dev.h).  Device buffers of this call only; every copy and launch in order on the context's stream.
int halo_dev_fold_points(halo_ctx *ctx, const uint64_t *key_affine, size_t n, int levels, const uint64_t *scalars, int form, int in_place,
                         uint64_t *out_affine) {
    HALO_CTX(ctx);
    if (levels != 1 && levels != 2) { set_error("dev_fold_points: levels must be 1 or 2"); return HALO_E_ARG; }
    const size_t parts = 2 * (size_t)levels;
    if (n == 0 || n % parts || n > ((size_t)1 << 24)) { set_error("dev_fold_points: n must be a positive multiple of 2 (levels 1) or 4 (levels 2), at most 2^24"); return HALO_E_ARG; }
    if (!scalars || !out_affine) { set_error("dev_fold_points: null pointer"); return HALO_E_ARG; }
    if (!key_affine && n > ctx->n) { set_error("dev_fold_points: n exceeds the context's key"); return HALO_E_ARG; }
    if (form < 0 || form > 5 || (levels == 1 && form > 2)) { set_error("dev_fold_points: form is 0, 1 or 2 for levels 1; 0 .. 5 for levels 2"); return HALO_E_ARG; }
    const size_t m = n / parts;
    const bool table = form >= 4;
    if (table && (key_affine || n != ctx->n || n < 64)) { set_error("dev_fold_points: the table forms fold the context's own key (key_affine = NULL, n = its size >= 64)"); return HALO_E_ARG; }
    if (table && in_place) { set_error("dev_fold_points: the table kernel never runs in place"); return HALO_E_ARG; }
    // the source: the uploaded key, or the context's own -- itself where nothing is written to it, else a copy
    const bool own_src = !key_affine && levels == 2 && !in_place;
    const size_t src_words = own_src ? 0 : n * (size_t)AFF_STRIDE, dst_words = (levels == 2 && !in_place) ? m * (size_t)AFF_STRIDE : 0;
    const size_t in_words = key_affine ? n * 8 : 0, out_words = m * 8;
    uint32_t *d = nullptr;
    alloc_epoch_bump(ctx);
    HALO_HIP(hipMalloc(&d, (src_words + dst_words) * 4 + (in_words + out_words) * 8));
    uint32_t *d_src = d, *d_dst = d + src_words;  // (every part a multiple of 128 bytes or of 64)
    uint64_t *d_in = reinterpret_cast<uint64_t *>(d_dst + dst_words), *d_out = d_in + in_words;
    int rc = HALO_OK;
    hipError_t e = hipSuccess;
    if (key_affine) {
        e = hipMemcpyAsync(d_in, key_affine, in_words * 8, hipMemcpyHostToDevice, ctx->stream);
        rc = e == hipSuccess ? aff_words_to_native(ctx, d_in, n, d_src) : hip_fail(e, "hipMemcpyAsync");
    } else if (!own_src) {
        e = hipMemcpyAsync(d_src, ctx->d_bases, src_words * 4, hipMemcpyDeviceToDevice, ctx->stream);
        if (e != hipSuccess) rc = hip_fail(e, "hipMemcpyAsync");
    }
    const uint32_t *src = own_src ? ctx->d_bases : d_src;
    uint32_t *dst = dst_words ? d_dst : d_src;
    if (!rc && levels == 1) rc = ipa_fold_points(ctx, d_src, m, host::Fr::load(scalars), form);
    if (!rc && levels == 2) {
        const host::Fr s[3] = {host::Fr::load(scalars), host::Fr::load(scalars + 4), host::Fr::load(scalars + 8)};
        const int mode = ctx->fold_table_mode;
        if (table) {  // as halo_set_fold_table(ctx, 1): built at this fold if it is not there yet
            ctx->fold_table_mode = 1;
            ctx->foldtab_retry_at = 0;
        }
        rc = ipa_fold_points4(ctx, src, dst, m, s, form);
        if (table) {
            ctx->fold_table_mode = mode;
            if (mode == 0) {  // a context that was told to hold no table holds none afterwards
                (void)hipStreamSynchronize(ctx->stream);
                foldtab_release(ctx);
            }
        }
    }
    if (!rc) rc = aff_native_to_words(ctx, dst, m, d_out);
    if (!rc && (e = hipMemcpyAsync(out_affine, d_out, out_words * 8, hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess) rc = hip_fail(e, "hipMemcpyAsync");
    e = hipStreamSynchronize(ctx->stream);  // (also on failure: nothing of this call may be in flight when its buffers go)
    if (!rc && e != hipSuccess) rc = hip_fail(e, "hipStreamSynchronize");
    (void)hipFree(d);
    return rc;
}

// The member-batched key folds through the product's launchers (include/halo_accumulation_dev.h).  Device buffers of this call only;
// every copy and launch in order on the context's stream.  A shared source (the context's key, or one uploaded key) is folded into
// a destination of members x m points; per-member sources are folded in place, member b's key at b * n points, as the open batch
// folds a staged key a second time.
int halo_dev_fold_points_batch(halo_ctx *ctx, const uint64_t *key_affine, size_t n, int levels, const uint64_t *scalars, int members, int shared, int form,
                               uint64_t *out_affine) {
    HALO_CTX(ctx);
    if (levels != 1 && levels != 2) { set_error("dev_fold_points_batch: levels must be 1 or 2"); return HALO_E_ARG; }
    const size_t parts = 2 * (size_t)levels;
    if (n == 0 || n % parts || n > ((size_t)1 << 24)) { set_error("dev_fold_points_batch: n must be a positive multiple of 2 (levels 1) or 4 (levels 2), at most 2^24"); return HALO_E_ARG; }
    if (!scalars || !out_affine) { set_error("dev_fold_points_batch: null pointer"); return HALO_E_ARG; }
    if (members < 1 || members > OPEN_MAX_GROUP) { set_error("dev_fold_points_batch: 1 .. 4 members"); return HALO_E_ARG; }
    if (!key_affine && !shared) { set_error("dev_fold_points_batch: the context's key (key_affine = NULL) is a shared source"); return HALO_E_ARG; }
    if (!key_affine && n > ctx->n) { set_error("dev_fold_points_batch: n exceeds the context's key"); return HALO_E_ARG; }
    if (form < 0 || form > 3 || (levels == 1 && form > 2)) { set_error("dev_fold_points_batch: form is 0, 1 or 2 for levels 1; 0 .. 3 for levels 2"); return HALO_E_ARG; }
    const size_t m = n / parts, G = (size_t)members, keys = shared ? 1 : G;
    const size_t src_words = key_affine ? keys * n * (size_t)AFF_STRIDE : 0, dst_words = shared ? G * m * (size_t)AFF_STRIDE : 0;
    const size_t in_words = key_affine ? keys * n * 8 : 0, out_words = G * m * 8;
    uint32_t *d = nullptr;
    alloc_epoch_bump(ctx);
    HALO_HIP(hipMalloc(&d, (src_words + dst_words + G * FOLD_DIG_WORDS) * 4 + (in_words + out_words) * 8));
    uint32_t *d_src = d, *d_dst = d + src_words, *d_digs = d_dst + dst_words;  // (every part a multiple of 128 bytes or of 64)
    uint64_t *d_in = reinterpret_cast<uint64_t *>(d_digs + G * FOLD_DIG_WORDS), *d_out = d_in + in_words;
    std::vector<uint32_t> digs(G * FOLD_DIG_WORDS);
    const size_t per = levels == 1 ? 1 : 3;  // scalars per member
    for (size_t b = 0; b < G; ++b) {
        host::Fr sc[3];
        for (size_t t = 0; t < per; ++t) sc[t] = host::Fr::load(scalars + 4 * (b * per + t));
        fold_digits(sc, levels, &digs[b * FOLD_DIG_WORDS]);
    }
    int rc = HALO_OK;
    hipError_t e = hipMemcpyAsync(d_digs, digs.data(), digs.size() * 4, hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) rc = hip_fail(e, "hipMemcpyAsync");
    if (!rc && key_affine) {
        e = hipMemcpyAsync(d_in, key_affine, in_words * 8, hipMemcpyHostToDevice, ctx->stream);
        rc = e == hipSuccess ? aff_words_to_native(ctx, d_in, keys * n, d_src) : hip_fail(e, "hipMemcpyAsync");
    }
    const uint32_t *src = key_affine ? d_src : ctx->d_bases;
    uint32_t *dst = shared ? d_dst : d_src;
    const size_t src_stride = shared ? 0 : n, dst_stride = shared ? m : n;
    if (!rc) rc = levels == 1 ? ipa_fold_points_batch(ctx, members, src, src_stride, dst, dst_stride, m, d_digs, form)
                              : ipa_fold_points4_batch(ctx, members, src, src_stride, dst, dst_stride, m, d_digs, form);
    for (size_t b = 0; b < G && !rc; ++b) rc = aff_native_to_words(ctx, dst + b * dst_stride * AFF_STRIDE, m, d_out + b * m * 8);
    if (!rc && (e = hipMemcpyAsync(out_affine, d_out, out_words * 8, hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess) rc = hip_fail(e, "hipMemcpyAsync");
    e = hipStreamSynchronize(ctx->stream);  // (also on failure: nothing of this call may be in flight when its buffers go)
    if (!rc && e != hipSuccess) rc = hip_fail(e, "hipStreamSynchronize");
    (void)hipFree(d);
    return rc;
}

// One batched MSM launch sequence over the context's key with one base offset per member, on slot 0 (include/halo_accumulation_dev.h)
int halo_dev_msm_offsets(halo_ctx *ctx, const size_t *offs, size_t n, const uint64_t *scalars, int count, int scalars_are_mont, uint64_t *out_jac) {
    HALO_CTX(ctx);
    if (count < 1 || count > MSM_MAX_BATCH) { set_error("dev_msm_offsets: 1 .. 8 members"); return HALO_E_ARG; }
    if (!offs || !out_jac || (n && !scalars)) { set_error("dev_msm_offsets: null pointer"); return HALO_E_ARG; }
    for (int b = 0; b < count; ++b)
        if (offs[b] > ctx->n || n > ctx->n - offs[b]) { set_error("dev_msm_offsets: range exceeds the context's key"); return HALO_E_ARG; }
    if (ctx->wss[0].in_flight || ctx->wss[0].lent_from >= 0 || ctx->fan[0].active) { set_error("dev_msm_offsets: slot 0 has an MSM in flight"); return HALO_E_ARG; }
    uint64_t *d_sc = nullptr;
    const size_t words = (size_t)count * n * 4;
    if (words) {
        alloc_epoch_bump(ctx);
        HALO_HIP(hipMalloc(&d_sc, words * 8));
    }
    int rc = HALO_OK;
    hipError_t e = words ? hipMemcpy(d_sc, scalars, words * 8, hipMemcpyHostToDevice) : hipSuccess;
    if (e != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    MsmBatch mb;
    mb.count = count;
    for (int b = 0; b < count; ++b) { mb.scalars[b] = d_sc + (size_t)b * n * 4; mb.base_off[b] = (uint32_t)offs[b]; }
    host::Point pts[MSM_MAX_BATCH];
    if (!rc) rc = msm_enqueue_batch(ctx, 0, ctx->d_bases, mb, scalars_are_mont != 0, n);
    if (!rc) rc = msm_finish_batch(ctx, 0, pts, count);
    (void)hipStreamSynchronize(ctx->streams[0]);  // (also on failure: nothing of this call may be in flight when its buffer goes)
    if (d_sc) (void)hipFree(d_sc);
    for (int b = 0; b < count && !rc; ++b) pts[b].store_normalized(out_jac + 12 * b);
    return rc;
}

// One tagged launch (MsmBatch::tagged) over a stretch of the context's key, on slot 0 (include/halo_accumulation_dev.h): the two
// outputs are finished as ipa_state.hip finishes L and R of a batched round (msm_wait for two, msm_combine_member 0 and 1).  The
// scalars go to a device buffer of this call only, with no word to alloc_epoch: a launch graph is keyed on the scalar pointer and
// replays only while that very address holds this call's scalars again, so the second and third call of a test capture and replay
// whenever the allocator hands the same block back (and run as plain launches, with the same results, when it does not).
int halo_dev_msm_tagged(halo_ctx *ctx, size_t off, size_t n, const uint64_t *scalars, uint64_t *out_jac) {
    HALO_CTX(ctx);
    if (!out_jac || (n && !scalars)) { set_error("dev_msm_tagged: null pointer"); return HALO_E_ARG; }
    if (off > ctx->n || n > ctx->n - off) { set_error("dev_msm_tagged: range exceeds the context's key"); return HALO_E_ARG; }
    if (ctx->wss[0].in_flight || ctx->wss[0].lent_from >= 0 || ctx->fan[0].active) { set_error("dev_msm_tagged: slot 0 has an MSM in flight"); return HALO_E_ARG; }
    host::Point pts[2] = {host::Point::infinity(), host::Point::infinity()};
    if (n == 0) {  // (nothing to launch: msm_tagged_ready takes no empty stretch)
        for (int b = 0; b < 2; ++b) pts[b].store_normalized(out_jac + 12 * b);
        return HALO_OK;
    }
    uint64_t *d_sc = nullptr;
    HALO_HIP(hipMalloc(&d_sc, n * 32));
    int rc = HALO_OK;
    hipError_t e = hipMemcpy(d_sc, scalars, n * 32, hipMemcpyHostToDevice);
    if (e != hipSuccess) rc = hip_fail(e, "hipMemcpy");
    MsmBatch both;
    both.count = 1;
    both.scalars[0] = d_sc;
    both.tagged = true;
    if (!rc) rc = msm_enqueue_batch(ctx, 0, ctx->d_bases + (size_t)AFF_STRIDE * off, both, /*mont*/ false, n);
    if (!rc) rc = msm_wait(ctx, 0, 2);
    for (int b = 0; b < 2 && !rc; ++b) msm_combine_member(ctx, 0, b, &pts[b]);
    (void)hipStreamSynchronize(ctx->streams[0]);  // (also on failure: nothing of this call may be in flight when its buffer goes)
    (void)hipFree(d_sc);
    for (int b = 0; b < 2 && !rc; ++b) pts[b].store_normalized(out_jac + 12 * b);
    return rc;
}

// Entries [off, off + count) of row `row` of the context's MSM table as arkworks affine words (include/halo_accumulation_dev.h): the
// conversion is halo_ctx_read_bases' (k_native_to_aff), the device buffer is this call's only.  Nothing may be in flight: a launch
// enqueued with every slot idle may release or rebuild the table (table_demote), and its slot's stream is not the one waited for here.
int halo_dev_table_read(halo_ctx *ctx, size_t row, size_t off, size_t count, uint64_t *out_affine) {
    HALO_CTX(ctx);
    if (!ctx->d_table) { set_error("dev_table_read: the context has no MSM table (built by its first table MSM)"); return HALO_E_ARG; }
    if (row >= (size_t)ctx->tbl.rows) { set_error("dev_table_read: row exceeds the table's rows (halo_ctx_info 8)"); return HALO_E_ARG; }
    if (off > ctx->n || count > ctx->n - off) { set_error("dev_table_read: range exceeds the context's key"); return HALO_E_ARG; }
    for (int k = 0; k < HALO_SLOTS; ++k)
        if (ctx->wss[k].in_flight || ctx->wss[k].lent_from >= 0 || ctx->fan[k].active) { set_error("dev_table_read: an MSM is in flight on this context"); return HALO_E_ARG; }
    if (count == 0) return HALO_OK;
    if (!out_affine) { set_error("dev_table_read: null pointer"); return HALO_E_ARG; }
    uint64_t *d_out = nullptr;
    alloc_epoch_bump(ctx);
    HALO_HIP(hipMalloc(&d_out, count * 64));
    int rc = aff_native_to_words(ctx, ctx->d_table + (size_t)AFF_STRIDE * (row * ctx->n + off), count, d_out);
    hipError_t e = hipSuccess;
    if (!rc && (e = hipMemcpyAsync(out_affine, d_out, count * 64, hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess) rc = hip_fail(e, "hipMemcpyAsync");
    e = hipStreamSynchronize(ctx->stream);  // (also on failure: nothing of this call may be in flight when its buffer goes)
    if (!rc && e != hipSuccess) rc = hip_fail(e, "hipStreamSynchronize");
    (void)hipFree(d_out);
    return rc;
}

// The two read-only views of a slot's last MSM launch (include/halo_accumulation_dev.h): host only, nothing is enqueued or waited for.
static int msm_slot_idle(halo_ctx *ctx, int slot, const char *who) {
    if (slot < 0 || slot >= HALO_SLOTS) { set_error(std::string(who) + ": slot out of range"); return HALO_E_ARG; }
    if (ctx->wss[slot].in_flight || ctx->wss[slot].lent_from >= 0 || ctx->fan[slot].active) { set_error(std::string(who) + ": the slot has an MSM in flight"); return HALO_E_ARG; }
    if (!ctx->wss[slot].launched) { set_error(std::string(who) + ": no launch on this slot yet"); return HALO_E_ARG; }
    return HALO_OK;
}
// records the plan's launch left in h_winsum: what msm_combine_member walks over
static size_t msm_winsum_records(const MsmPlan &p) {
    if (p.W == 0) return 0;
    if (p.pipeline >= 2)
        return (size_t)p.table_pieces * p.table_sets * 2 * (size_t)(((1 << p.table_rc_lg_cols) + (1 << p.table_rc_lg_rows)) / 64);
    return (size_t)(p.w1 - p.w0) * p.batch;
}
int halo_dev_msm_last_plan(halo_ctx *ctx, int slot, long out[16]) {
    HALO_CTX(ctx);
    if (!out) { set_error("dev_msm_last_plan: null pointer"); return HALO_E_ARG; }
    int rc = msm_slot_idle(ctx, slot, "dev_msm_last_plan");
    if (rc) return rc;
    const MsmPlan &p = ctx->wss[slot].plan;
    const long v[16] = {p.pipeline, p.c, p.W, (long)p.B, p.batch, p.table_sets, p.table_pieces, (long)p.kmax, p.winsum_form, (long)p.red_L, p.red_logL,
                        (long)p.red_nseg, p.red_live_seg,
                        p.pipeline >= 2 ? (long)p.table_rc_lg_rows | (long)p.table_rc_lg_cols << 8 | (long)p.table_rc_per << 16 : 0, 0, 0};
    for (int k = 0; k < 16; ++k) out[k] = v[k];
    return HALO_OK;
}
int halo_dev_msm_window_sums(halo_ctx *ctx, int slot, uint64_t *out_jac, size_t cap_points, size_t *count) {
    HALO_CTX(ctx);
    if (!count) { set_error("dev_msm_window_sums: null pointer"); return HALO_E_ARG; }
    *count = 0;
    int rc = msm_slot_idle(ctx, slot, "dev_msm_window_sums");
    if (rc) return rc;
    const MsmWorkspace &ws = ctx->wss[slot];
    const size_t records = msm_winsum_records(ws.plan);
    *count = records;
    if (records > cap_points) { set_error("dev_msm_window_sums: room for fewer points than the launch left (see *count)"); return HALO_E_ARG; }
    if (!out_jac) { set_error("dev_msm_window_sums: null pointer"); return HALO_E_ARG; }
    if (records > ws.cap_windows) { set_error("dev_msm_window_sums: the plan names more records than the slot's buffer holds"); return HALO_E_ARG; }
    for (size_t k = 0; k < 12 * records; ++k) out_jac[k] = ws.h_winsum[k];
    return HALO_OK;
}

int halo_test_lazy_field_op(halo_ctx *ctx, int op, const uint32_t *in, size_t n, uint32_t *out) {
    HALO_CTX(ctx);
    if (n == 0) return HALO_OK;
    if (!in || !out) { set_error("test_lazy_field_op: null pointer"); return HALO_E_ARG; }
    if (n > ((size_t)1 << 22)) { set_error("test_lazy_field_op: at most 2^22 cases"); return HALO_E_ARG; }
    return lazy_run(ctx, 0, op, in, nullptr, n, out);
}

int halo_test_lazy_point_op(halo_ctx *ctx, int op, int quad, const uint32_t *a, const uint32_t *b, size_t n, uint32_t *out) {
    HALO_CTX(ctx);
    if (n == 0) return HALO_OK;
    if (!a || !b || !out) { set_error("test_lazy_point_op: null pointer"); return HALO_E_ARG; }
    if (n > ((size_t)1 << 20)) { set_error("test_lazy_point_op: at most 2^20 cases"); return HALO_E_ARG; }
    if (op < 0 || op >= LZP_COUNT) { set_error("test_lazy_point_op: unknown operation"); return HALO_E_ARG; }
    if (quad && !(op == LZP_XYZZ_ADD || op == LZP_XYZZ_DBL || op == LZP_JAC_MADD || op == LZP_JAC_DBL)) {
        set_error("test_lazy_point_op: the quad forms are xyzz_add, xyzz_dbl, jac_madd and jac_dbl");
        return HALO_E_ARG;
    }
    return lazy_run(ctx, quad ? 2 : 1, op, a, b, n, out);
}

}  // extern "C"
