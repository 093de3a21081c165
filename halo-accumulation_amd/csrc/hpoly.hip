// h(X) of pcdl.rs:56-91 and pcdl.rs:496-505: its coefficients from three 256-entry tables (K7), the sum of several scaled
// polynomials per member (K7b, acc.rs:85-94) and HPoly::eval, one polynomial per lane (K8).  The launch plan of the coefficient
// kernels is fr_plan.hpp's plan_h_coeffs.
#include <algorithm>

#include "fr29.hpp"
#include "fr_plan.hpp"
#include "internal.hpp"

namespace halo {

// ------------------------------------------------------------------ K7: h coefficients from three 256-entry tables
constexpr size_t H_TAB_WORDS = H_TABLES_WORDS;  // one polynomial's low | mid | high tables
// tab = low (A-form) | mid | high (N-form), 256 x 4 words each; coefficient k = low[k & 255] * mid[(k >> 8) & 255] * high[k >> 16].
// Lane l of a wave takes k = base + l + 64 j: (k >> 8) is the same for the whole wave and changes every fourth step,
// so mid * high is one product per four elements and low * (mid high) the only product per element.
HALO_DEV void h_coeffs_wave(const uint64_t *__restrict__ tab, uint32_t n, int E, int accumulate, uint64_t *__restrict__ out) {
    uint32_t wave = (blockIdx.x * 256 + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    uint32_t k = wave * (64u * (uint32_t)E) + lane;
    if (k >= n) return;
    Fs<4> hm = fs_zero<4>();
#pragma unroll 1
    for (int j = 0; j < E && k < n; j++, k += 64) {
        if ((j & 3) == 0) {
            uint32_t kk = __builtin_amdgcn_readfirstlane(k);  // wave-uniform: (k >> 8) does not depend on the lane
            hm = fs_widen<4>(fs_mul(fs_load(tab + 4 * (size_t)(256 + ((kk >> 8) & 255u))), fs_load(tab + 4 * (size_t)(512 + ((kk >> 16) & 255u)))));
        }
        Fs<2> v = fs_mul(fs_load(tab + 4 * (size_t)(k & 255u)), hm);
        if (accumulate) fs_store(out + 4 * (size_t)k, fs_add(v, fs_load(out + 4 * (size_t)k)));
        else fs_store(out + 4 * (size_t)k, v);
    }
}
__global__ __launch_bounds__(256) void k_h_coeffs(const uint64_t *__restrict__ tab, uint32_t n, int E, int accumulate, uint64_t *__restrict__ out) {
    h_coeffs_wave(tab, n, E, accumulate, out);
}
// The same for a batch of polynomials: blockIdx.y = member, its own table (3 x 256 x 4 words) and its own n x 4 output words
__global__ __launch_bounds__(256) void k_h_coeffs_batch(const uint64_t *__restrict__ tabs, uint32_t n, int E, uint64_t *__restrict__ outs, uint64_t out_stride) {
    h_coeffs_wave(tabs + (size_t)blockIdx.y * H_TAB_WORDS, n, E, 0, outs + (size_t)blockIdx.y * out_stride);
}
// The three tables of k_h_coeffs built on the device, one block per polynomial (challenges: lg_n + 1 Montgomery elements per
// polynomial, contiguous).  Thread k of level L (bits 8L .. 8L + 7 of the coefficient index) multiplies the challenges of the set
// bits of k, xis[lg_n - (8L + b)] -- the same field element the host's doubling construction in h_coeffs_dev reaches, and both
// are canonical Montgomery limbs, so the tables are bit-identical.  Entries past a level's 2^bits stay one as on the host; the
// mid and high levels are N-form multipliers (32 x, five doublings), the low one A-form.
// scaled = 1: a record is lg_n + 2 elements, the last one the polynomial's scale (alpha^(i+1) of acc.rs:85-94), folded into the
// high table exactly as h_coeffs_dev(xis, lg_n, scale, ..) folds it on the host.
// h_tables_block: one block's work for the record x; the two kernels differ only in where a record stands and where its lg comes from.
HALO_DEV void h_tables_block(const uint64_t *__restrict__ x, int lg_n, int scaled, uint64_t *__restrict__ tab) {
    const uint32_t k = threadIdx.x;
#pragma unroll 1
    for (int level = 0; level < 3; level++) {
        int bits = lg_n - 8 * level;
        bits = bits < 0 ? 0 : (bits > 8 ? 8 : bits);
        Fe t = fe_one<FrCfg>();
        if ((k >> bits) == 0) {
            if (level == 2 && scaled) t = fe_load(x + 4 * (size_t)(lg_n + 1));
#pragma unroll 1
            for (int b = 0; b < bits; b++)
                if ((k >> b) & 1u) t = fe_mul<FrCfg>(t, fe_load(x + 4 * (size_t)(lg_n - (8 * level + b))));
        }
        if (level > 0) {
#pragma unroll
            for (int d = 0; d < 5; d++) t = fe_dbl<FrCfg>(t);
        }
        fe_store(tab + 4 * (size_t)(256 * level + k), t);
    }
}
__global__ __launch_bounds__(256) void k_h_tables(const uint64_t *__restrict__ xis, int lg_n, int scaled, uint64_t *__restrict__ tabs) {
    h_tables_block(xis + (size_t)blockIdx.x * 4 * (size_t)(lg_n + 1 + scaled), lg_n, scaled, tabs + (size_t)blockIdx.x * H_TAB_WORDS);
}
// The same with a length per polynomial (halo_pcdl_check_batch_mixed_combined): records at the fixed stride of lg_max + 1 + scaled
// elements, record t's own lg in lgs[t]; its lgs[t] + 1 challenges (and the scale behind them) stand at the record's start as in a
// record of k_h_tables for that lg, the rest of the record is not read.  A table depends on its own record alone, so it is word
// for word what k_h_tables builds for lgs[t].
__global__ __launch_bounds__(256) void k_h_tables_mixed(const uint64_t *__restrict__ xis, const uint32_t *__restrict__ lgs, int lg_max, int scaled,
                                                        uint64_t *__restrict__ tabs) {
    h_tables_block(xis + (size_t)blockIdx.x * 4 * (size_t)(lg_max + 1 + scaled), (int)lgs[blockIdx.x], scaled, tabs + (size_t)blockIdx.x * H_TAB_WORDS);
}

// ------------------------------------------------------------------ K7b: h(X) = h_0 + sum_i alpha^(i+1) h_i(X) of several members
// (acc.rs:85-94, halo_acc_prover_batch).  blockIdx.y = member; its record (HACC_REC_WORDS words) names its tables of this launch:
//     word 0 = first table | count << 32, word 1 = mode, words 2..9 = h_0 (two Montgomery elements)
// mode 0: nothing to do in this launch; 1: out = h_0 + the sum (count 0: h_0 and zeros); 2: out += the sum (a member with more
// tables than one launch holds).  Everything read from the record is the same for every lane of the grid row.
// Lane l of a wave takes the coefficients base + l + 64 j as h_coeffs_wave does.  Four steps share (k >> 8), so for every table
// mid * high is ONE wave-uniform product per four coefficients and low * (mid high) the only product per coefficient and table.
// The four running sums stay in the lazy 29-bit form: a product is < 2 r, sum + product < 4 r is brought back below 2 r at once
// (fs_tighten: ~30 VALU against ~230 of the product), so the bound never depends on the count -- a member of 64 instances works
// like one of 2 -- and fs_add's static_assert holds it.  Every coefficient is stored ONCE, canonical (fs_store): field sums are
// exact, so the words equal m accumulate passes of k_h_coeffs in any order.  The tables are read through L2: 24 KiB per
// instance, the same lines for every wave of a member.
HALO_DEV void h_acc_step(Fs<2> &acc, const uint64_t *__restrict__ tab, uint32_t k, const Fs<4> &hm) {
    acc = fs_tighten(fs_add(acc, fs_mul(fs_load(tab + 4 * (size_t)(k & 255u)), hm)));
}
HALO_DEV void h_acc_store(uint64_t *__restrict__ out, const uint64_t *__restrict__ rec, uint32_t mode, uint32_t k, uint32_t n, const Fs<2> &acc) {
    if (k >= n) return;
    Fs<4> extra = fs_zero<4>();
    if (mode == 2) extra = fs_load(out + 4 * (size_t)k);
    else if (k < 2) extra = fs_load(rec + 2 + 4 * (size_t)k);
    fs_store(out + 4 * (size_t)k, fs_add(acc, extra));
}
__global__ __launch_bounds__(256) void k_h_accumulate_batch(const uint64_t *__restrict__ tabs, const uint64_t *__restrict__ recs, uint32_t n, int E,
                                                            uint64_t *__restrict__ outs, uint64_t out_stride) {
    const uint64_t *rec = recs + HACC_REC_WORDS * (size_t)blockIdx.y;
    const uint32_t first = (uint32_t)rec[0], count = (uint32_t)(rec[0] >> 32), mode = (uint32_t)rec[1];
    if (mode == 0) return;
    uint64_t *out = outs + (size_t)blockIdx.y * out_stride;
    const uint32_t wave = (blockIdx.x * 256 + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    uint32_t k = wave * (64u * (uint32_t)E) + lane;
#pragma unroll 1
    for (int j = 0; j < E && k < n; j += 4, k += 256) {  // (E is a multiple of four: pow_chain_len)
        const uint32_t kk = __builtin_amdgcn_readfirstlane(k);  // wave-uniform: (k >> 8) does not depend on the lane
        Fs<2> a0 = fs_zero<2>(), a1 = fs_zero<2>(), a2 = fs_zero<2>(), a3 = fs_zero<2>();
#pragma unroll 1
        for (uint32_t t = 0; t < count; t++) {
            const uint64_t *tab = tabs + (size_t)(first + t) * H_TAB_WORDS;
            const Fs<4> hm = fs_widen<4>(fs_mul(fs_load(tab + 4 * (size_t)(256 + ((kk >> 8) & 255u))), fs_load(tab + 4 * (size_t)(512 + ((kk >> 16) & 255u)))));
            // (a step past n multiplies a valid table entry and is never stored: no divergence around the products)
            h_acc_step(a0, tab, k, hm);
            h_acc_step(a1, tab, k + 64, hm);
            h_acc_step(a2, tab, k + 128, hm);
            h_acc_step(a3, tab, k + 192, hm);
        }
        h_acc_store(out, rec, mode, k, n, a0);
        h_acc_store(out, rec, mode, k + 64, n, a1);
        h_acc_store(out, rec, mode, k + 128, n, a2);
        h_acc_store(out, rec, mode, k + 192, n, a3);
    }
}

// The same sum over tables of DIFFERENT lengths (halo_pcdl_check_batch_mixed_combined): s = sum_t pad(h_t), a shorter polynomial
// zero-padded to the row's n coefficients.  lgs[t] = table t's lg; blockIdx.y = part, its record as above.  The tables of a
// launch stand in order of DECREASING length, so within a part too.  The four steps of a lane cover one 256-aligned block
// [kk, kk + 256) of coefficients:
//   - a table with n_t <= kk adds nothing to the block, and neither does any table behind it: the table loop ends there.  kk is
//     wave-uniform, so the exit is;
//   - a table with n_t >= 256 that reaches the block covers all of it (n_t is a power of two, kk a multiple of 256);
//   - a table shorter than 256 reaches block 0 only, and there a step adds its product only where k < n_t.  The product is
//     computed for every lane (entries of the low table past 2^lg are one, mid[0] and high[0] valid): only the add is selected,
//     no divergence around the multiplies.  For the longer tables the selection is always true.
// Every coefficient below n is stored once, canonical; a block no table of the part reaches stores zeros (mode 1) or stays (mode 2).
HALO_DEV void h_acc_step_below(Fs<2> &acc, const uint64_t *__restrict__ tab, uint32_t k, uint32_t n_t, const Fs<4> &hm) {
    const Fs<2> sum = fs_tighten(fs_add(acc, fs_mul(fs_load(tab + 4 * (size_t)(k & 255u)), hm)));
    const bool take = k < n_t;
#pragma unroll
    for (int i = 0; i < 9; i++) acc.v[i] = take ? sum.v[i] : acc.v[i];  // (same bound on both sides: limbs copied within Fs<2>)
}
__global__ __launch_bounds__(256) void k_h_accumulate_mixed(const uint64_t *__restrict__ tabs, const uint32_t *__restrict__ lgs,
                                                            const uint64_t *__restrict__ recs, uint32_t n, int E, uint64_t *__restrict__ outs,
                                                            uint64_t out_stride) {
    const uint64_t *rec = recs + HACC_REC_WORDS * (size_t)blockIdx.y;
    const uint32_t first = (uint32_t)rec[0], count = (uint32_t)(rec[0] >> 32), mode = (uint32_t)rec[1];
    if (mode == 0) return;
    uint64_t *out = outs + (size_t)blockIdx.y * out_stride;
    const uint32_t wave = (blockIdx.x * 256 + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    uint32_t k = wave * (64u * (uint32_t)E) + lane;
#pragma unroll 1
    for (int j = 0; j < E && k < n; j += 4, k += 256) {  // (E is a multiple of four: pow_chain_len)
        const uint32_t kk = __builtin_amdgcn_readfirstlane(k);  // wave-uniform: the block's start is kk & ~255
        Fs<2> a0 = fs_zero<2>(), a1 = fs_zero<2>(), a2 = fs_zero<2>(), a3 = fs_zero<2>();
#pragma unroll 1
        for (uint32_t t = 0; t < count; t++) {
            const uint32_t n_t = 1u << __builtin_amdgcn_readfirstlane(lgs[first + t]);
            if (n_t <= (kk & ~255u)) break;  // (decreasing lengths: no later table reaches this block)
            const uint64_t *tab = tabs + (size_t)(first + t) * H_TAB_WORDS;
            const Fs<4> hm = fs_widen<4>(fs_mul(fs_load(tab + 4 * (size_t)(256 + ((kk >> 8) & 255u))), fs_load(tab + 4 * (size_t)(512 + ((kk >> 16) & 255u)))));
            h_acc_step_below(a0, tab, k, n_t, hm);
            h_acc_step_below(a1, tab, k + 64, n_t, hm);
            h_acc_step_below(a2, tab, k + 128, n_t, hm);
            h_acc_step_below(a3, tab, k + 192, n_t, hm);
        }
        h_acc_store(out, rec, mode, k, n, a0);
        h_acc_store(out, rec, mode, k + 64, n, a1);
        h_acc_store(out, rec, mode, k + 128, n, a2);
        h_acc_store(out, rec, mode, k + 192, n, a3);
    }
}

// ------------------------------------------------------------------ K8: HPoly::eval, one polynomial per lane
// polynomial i (lg_n + 1 challenges at xis) at the point z
HALO_DEV void h_eval_lane(const uint64_t *__restrict__ xis, uint32_t i, int lg_n, const Fe &z, uint64_t *__restrict__ out) {
    const uint64_t *x = xis + 4 * (size_t)i * (size_t)(lg_n + 1);
    Fe one = fe_one<FrCfg>();
    Fe v = fe_add<FrCfg>(one, fe_mul<FrCfg>(fe_load(x + 4 * (size_t)lg_n), z));
    Fe zi = z;
#pragma unroll 1
    for (int k = 1; k < lg_n; k++) {
        zi = fe_sqr<FrCfg>(zi);
        v = fe_mul<FrCfg>(v, fe_add<FrCfg>(one, fe_mul<FrCfg>(fe_load(x + 4 * (size_t)(lg_n - k)), zi)));
    }
    fe_store(out + 4 * (size_t)i, v);
}
__global__ __launch_bounds__(256) void k_h_eval(const uint64_t *__restrict__ xis, uint32_t m, int lg_n, FeArg zarg,
                                                uint64_t *__restrict__ out) {
    uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    h_eval_lane(xis, i, lg_n, from_arg(zarg), out);
}
// HPoly::eval for m polynomials, each at its own point (the m succinct checks of acc.rs:158-170 have their own z_i)
__global__ __launch_bounds__(256) void k_h_eval_z(const uint64_t *__restrict__ xis, const uint64_t *__restrict__ zs, uint32_t m, int lg_n,
                                                  uint64_t *__restrict__ out) {
    uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    h_eval_lane(xis, i, lg_n, fe_load(zs + 4 * (size_t)i), out);
}

// ================================================================== host launchers
int h_coeffs_dev(halo_ctx *ctx, const host::Fr *xis, size_t lg_n, const host::Fr &scale, bool accumulate, uint64_t *d_out) {
    if (lg_n > 24) { set_error("h_coeffs: lg_n > 24 unsupported"); return HALO_E_ARG; }
    // coefficient k = prod over set bits i of k of xis[lg_n - i]  (pcdl.rs:496-505)
    std::vector<uint64_t> tab(3 * 256 * 4);
    for (int level = 0; level < 3; ++level) {
        std::vector<host::Fr> t(256, host::Fr::one());
        if (level == 2) t[0] = scale;
        size_t len = 1;
        for (int b = 0; b < 8; ++b) {
            size_t bit = (size_t)level * 8 + b;
            if (bit >= lg_n) break;
            const host::Fr &x = xis[lg_n - bit];
            for (size_t k = 0; k < len; ++k) t[len + k] = t[k] * x;
            len *= 2;
        }
        if (level == 2 && len == 1) t[0] = scale;
        // low table in A-form (what the kernel multiplies INTO), mid and high as N-form multipliers (fr29.hpp): 32 x
        const host::Fr k32 = host::Fr::from_u64(32);
        for (size_t k = 0; k < 256; ++k) (level == 0 ? t[k] : t[k] * k32).store(&tab[((size_t)level * 256 + k) * 4]);
    }
    uint64_t *d_tab = ctx->d_tmp_c + 8 * 1024 + 1024;  // (the window table of fr_powers / fr_poly_eval sits below)
    HALO_HIP(hipMemcpyAsync(d_tab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    HALO_HIP(hipStreamSynchronize(ctx->stream));  // `tab` is pageable and dies at return
    size_t n = (size_t)1 << lg_n;
    const FrPlan p = plan_h_coeffs(n);
    HALO_LAUNCH(ctx, "k_h_coeffs", k_h_coeffs, dim3(p.blocks), dim3(256), 0, d_tab, (uint32_t)n, p.E, accumulate ? 1 : 0, d_out);
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}

// m polynomials at once (scale one, no accumulation): member b's coefficients go to d_out + b * out_stride words, bit-identical
// to h_coeffs_dev(xis_b, lg_n, 1, false).  Two launches on ctx->stream whatever m is: the tables (d_tabs: m x H_TAB_WORDS) from
// the challenges already in device memory (d_xis: m x (lg_n + 1) x 4 words), then the coefficients.
int h_coeffs_batch_dev(halo_ctx *ctx, const uint64_t *d_xis, size_t m, size_t lg_n, uint64_t *d_tabs, uint64_t *d_out, size_t out_stride) {
    if (lg_n > 24) { set_error("h_coeffs: lg_n > 24 unsupported"); return HALO_E_ARG; }
    if (m == 0) return HALO_OK;
    if (m > 65535) { set_error("h_coeffs_batch: at most 65535 members per launch"); return HALO_E_ARG; }
    size_t n = (size_t)1 << lg_n;
    const FrPlan p = plan_h_coeffs(n);
    HALO_LAUNCH(ctx, "k_h_tables", k_h_tables, dim3((unsigned)m), dim3(256), 0, d_xis, (int)lg_n, 0, d_tabs);
    HALO_LAUNCH(ctx, "k_h_coeffs_batch", k_h_coeffs_batch, dim3(p.blocks, (unsigned)m), dim3(256), 0, d_tabs, (uint32_t)n, p.E, d_out,
                (uint64_t)out_stride);
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}

// h(X) = h_0 + sum_i scale_i h_i(X) of G members at once (acc.rs:85-94 for each), member b's n coefficients stored once at
// d_out + b * out_stride.  Staging, the same layout in pinned (h_stage) and device memory (d_stage): G records of
// HACC_REC_WORDS, then one record of lg_n + 2 elements per table (the challenges, then the scale); the device staging holds
// cap x H_TAB_WORDS of tables behind that (hacc_stage_words).  Per pass ONE copy from pinned memory, k_h_tables over the
// pass's polynomials and k_h_accumulate_batch over the members: one pass unless the members bring more than `cap` polynomials,
// then the later passes add to what is there (mode 2) after the stream has drained the pinned records.  On ctx->stream.
int h_accumulate_group(halo_ctx *ctx, const HAccMember *mem, size_t G, size_t lg_n, size_t cap, uint64_t *h_stage, uint64_t *d_stage, uint64_t *d_out,
                       size_t out_stride) {
    if (lg_n > 24) { set_error("h_coeffs: lg_n > 24 unsupported"); return HALO_E_ARG; }
    if (G == 0) return HALO_OK;
    if (G > 65535 || cap == 0) { set_error("h_accumulate: 1..65535 members, at least one table"); return HALO_E_ARG; }
    const size_t n = (size_t)1 << lg_n, head = G * HACC_REC_WORDS, tw = (lg_n + 2) * 4;
    const FrPlan p = plan_h_coeffs(n);
    uint64_t *d_tabs = d_stage + head + cap * tw;
    std::vector<size_t> done(G, 0);
    for (bool first_pass = true;; first_pass = false) {
        size_t T = 0;
        bool more = false;
        for (size_t b = 0; b < G; ++b) {
            const HAccMember &m = mem[b];
            size_t take = m.count - done[b];
            if (take > cap - T) take = cap - T;
            uint64_t *rec = h_stage + b * HACC_REC_WORDS;
            rec[0] = (uint64_t)T | ((uint64_t)take << 32);
            rec[1] = first_pass ? 1 : (take ? 2 : 0);
            m.h0[0].store(rec + 2);
            m.h0[1].store(rec + 6);
            for (size_t t = 0; t < take; ++t) {
                uint64_t *x = h_stage + head + (T + t) * tw;
                const host::Fr *xi = m.xis[done[b] + t];
                for (size_t q = 0; q <= lg_n; ++q) xi[q].store(x + 4 * q);
                m.scales[done[b] + t].store(x + 4 * (lg_n + 1));
            }
            T += take;
            done[b] += take;
            if (done[b] < m.count) more = true;
        }
        HALO_HIP(hipMemcpyAsync(d_stage, h_stage, (head + T * tw) * 8, hipMemcpyHostToDevice, ctx->stream));
        if (T) HALO_LAUNCH(ctx, "k_h_tables", k_h_tables, dim3((unsigned)T), dim3(256), 0, d_stage + head, (int)lg_n, 1, d_tabs);
        HALO_LAUNCH(ctx, "k_h_accumulate_batch", k_h_accumulate_batch, dim3(p.blocks, (unsigned)G), dim3(256), 0, d_tabs, d_stage, (uint32_t)n, p.E,
                    d_out, (uint64_t)out_stride);
        HALO_HIP(hipGetLastError());
        if (!more) return HALO_OK;
        HALO_HIP(hipStreamSynchronize(ctx->stream));  // (the next pass rewrites the pinned records)
    }
}

// s = sum_a r_a h_a(X) over A polynomials (halo_pcdl_check_batch_combined), n canonical elements in row 0 of d_stage's rows.
// One member row of k_h_accumulate_batch would be plan_h_coeffs(n).blocks x 1 blocks walking all A tables in turn: a handful of
// waves at n = 512.  So the polynomials are cut into P PARTS, blockIdx.y = part, each with its own first / count record (h_0 = 0)
// and its own n-element partial row; k_fr_sum_rows then adds the rows into row 0 (P = 1: nothing to add).  The tables are built
// `cap` at a time (k_h_tables, scaled: r_a folded into the high table); a later pass adds to the rows (mode 2).  Field sums are
// exact and every stored element canonical, so the words of s depend neither on P nor on cap.
// h_recs: A records of lg_n + 2 Montgomery elements (the challenges, then r_a) in host memory.  d_stage (hcomb_stage_words):
// the A records | passes x P part records | cap tables | P rows.  The uploads are complete when the call returns (hipMemcpy),
// the launches are on ctx->stream.
int h_combine_rows(halo_ctx *ctx, const uint64_t *h_recs, size_t A, size_t lg_n, size_t P, size_t cap, uint64_t *d_stage) {
    if (lg_n > 24) { set_error("h_coeffs: lg_n > 24 unsupported"); return HALO_E_ARG; }
    if (A == 0 || A > 65535 || P == 0 || P > A || cap == 0) { set_error("h_combine: 1..65535 polynomials, 1..A parts, at least one table"); return HALO_E_ARG; }
    if (cap > A) cap = A;
    const size_t n = (size_t)1 << lg_n, tw = (lg_n + 2) * 4, passes = (A + cap - 1) / cap;
    const FrPlan p = plan_h_coeffs(n);
    uint64_t *d_recs = d_stage, *d_parts = d_recs + A * tw, *d_tabs = d_parts + hcomb_part_words(A, P, cap), *d_rows = d_tabs + cap * H_TAB_WORDS;
    std::vector<uint64_t> parts(passes * P * HACC_REC_WORDS, 0);  // (h_0 = 0 in every record)
    for (size_t pass = 0; pass < passes; ++pass) {
        const size_t T = A - pass * cap < cap ? A - pass * cap : cap;
        for (size_t q = 0; q < P; ++q) {  // part q: tables [q T / P, (q + 1) T / P) of this pass
            const size_t lo = q * T / P, hi = (q + 1) * T / P;
            uint64_t *rec = &parts[(pass * P + q) * HACC_REC_WORDS];
            rec[0] = (uint64_t)lo | ((uint64_t)(hi - lo) << 32);
            rec[1] = pass == 0 ? 1 : (hi > lo ? 2 : 0);
        }
    }
    HALO_HIP(hipMemcpy(d_recs, h_recs, A * tw * 8, hipMemcpyHostToDevice));
    HALO_HIP(hipMemcpy(d_parts, parts.data(), parts.size() * 8, hipMemcpyHostToDevice));
    for (size_t pass = 0; pass < passes; ++pass) {
        const size_t T = A - pass * cap < cap ? A - pass * cap : cap;
        HALO_LAUNCH(ctx, "k_h_tables", k_h_tables, dim3((unsigned)T), dim3(256), 0, d_recs + pass * cap * tw, (int)lg_n, 1, d_tabs);
        HALO_LAUNCH(ctx, "k_h_accumulate_batch", k_h_accumulate_batch, dim3(p.blocks, (unsigned)P), dim3(256), 0, d_tabs, d_parts + pass * P * HACC_REC_WORDS,
                    (uint32_t)n, p.E, d_rows, (uint64_t)(n * 4));
    }
    HALO_HIP(hipGetLastError());
    return fr_sum_rows(ctx, d_rows, n * 4, P, n);
}

// s = sum_a r_a pad(h_a)(X) over A polynomials of their own lengths (halo_pcdl_check_batch_mixed_combined): n = 2^lg_max canonical
// elements in row 0, a polynomial of 2^lgs[a] < n coefficients zero-padded.  h_combine_rows with three differences:
//   - h_recs: A records at the fixed stride of lg_max + 2 elements in the CALLER's order, record a = its lgs[a] + 1 challenges,
//     then r_a.  They are sorted here by decreasing length (stable) and staged in that order with their lgs, which is what
//     k_h_accumulate_mixed's early loop end needs; a pass takes the next `cap` tables of the sorted order;
//   - the parts of a pass are cut by summed table LENGTH, not by table count -- in sorted order equal counts would put all the
//     long tables into the first parts: table j of the pass, with the lengths before it summing to s_j of L, goes to part
//     s_j P / L (monotone in j, so a part is a stretch of tables; a part may be empty and then writes zeros in the first pass);
//   - the launches are k_h_tables_mixed and k_h_accumulate_mixed.
// Field sums are exact and every stored element canonical, so the words of s depend neither on P, on cap nor on the cuts.
// d_stage (hmix_stage_words): the A records | their lgs | passes x P part records | cap tables | P rows.
int h_combine_rows_mixed(halo_ctx *ctx, const uint64_t *h_recs, const uint32_t *lgs, size_t A, size_t lg_max, size_t P, size_t cap, uint64_t *d_stage) {
    if (lg_max > 24) { set_error("h_coeffs: lg_n > 24 unsupported"); return HALO_E_ARG; }
    if (A == 0 || A > 65535 || P == 0 || P > A || cap == 0) { set_error("h_combine: 1..65535 polynomials, 1..A parts, at least one table"); return HALO_E_ARG; }
    for (size_t a = 0; a < A; ++a)
        if (lgs[a] > lg_max) { set_error("h_combine: a polynomial longer than the row"); return HALO_E_ARG; }
    if (cap > A) cap = A;
    const size_t n = (size_t)1 << lg_max, tw = (lg_max + 2) * 4, passes = (A + cap - 1) / cap;
    const FrPlan p = plan_h_coeffs(n);
    uint64_t *d_recs = d_stage, *d_lgs64 = d_recs + A * tw, *d_parts = d_lgs64 + hmix_lg_words(A), *d_tabs = d_parts + hcomb_part_words(A, P, cap),
             *d_rows = d_tabs + cap * H_TAB_WORDS;
    const uint32_t *d_lgs = reinterpret_cast<const uint32_t *>(d_lgs64);
    std::vector<size_t> order(A);
    for (size_t a = 0; a < A; ++a) order[a] = a;
    std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return lgs[x] > lgs[y]; });
    std::vector<uint64_t> recs(A * tw);
    std::vector<uint32_t> slg(A);
    for (size_t j = 0; j < A; ++j) {
        std::memcpy(&recs[j * tw], h_recs + order[j] * tw, tw * 8);
        slg[j] = lgs[order[j]];
    }
    std::vector<uint64_t> parts(passes * P * HACC_REC_WORDS, 0);  // (h_0 = 0 in every record)
    for (size_t pass = 0; pass < passes; ++pass) {
        const size_t lo = pass * cap, T = A - lo < cap ? A - lo : cap;
        uint64_t L = 0;
        for (size_t j = 0; j < T; ++j) L += (uint64_t)1 << slg[lo + j];
        std::vector<size_t> cnt(P, 0), start(P, 0);
        uint64_t s = 0;
        for (size_t j = 0; j < T; ++j) {
            const size_t q = (size_t)(s * P / L);  // (s < L, so q < P)
            if (cnt[q]++ == 0) start[q] = j;
            s += (uint64_t)1 << slg[lo + j];
        }
        for (size_t q = 0; q < P; ++q) {
            uint64_t *rec = &parts[(pass * P + q) * HACC_REC_WORDS];
            rec[0] = (uint64_t)start[q] | ((uint64_t)cnt[q] << 32);
            rec[1] = pass == 0 ? 1 : (cnt[q] ? 2 : 0);
        }
    }
    HALO_HIP(hipMemcpy(d_recs, recs.data(), A * tw * 8, hipMemcpyHostToDevice));
    HALO_HIP(hipMemcpy(d_lgs64, slg.data(), A * 4, hipMemcpyHostToDevice));
    HALO_HIP(hipMemcpy(d_parts, parts.data(), parts.size() * 8, hipMemcpyHostToDevice));
    for (size_t pass = 0; pass < passes; ++pass) {
        const size_t T = A - pass * cap < cap ? A - pass * cap : cap;
        HALO_LAUNCH(ctx, "k_h_tables_mixed", k_h_tables_mixed, dim3((unsigned)T), dim3(256), 0, d_recs + pass * cap * tw, d_lgs + pass * cap, (int)lg_max, 1,
                    d_tabs);
        HALO_LAUNCH(ctx, "k_h_accumulate_mixed", k_h_accumulate_mixed, dim3(p.blocks, (unsigned)P), dim3(256), 0, d_tabs, d_lgs + pass * cap,
                    d_parts + pass * P * HACC_REC_WORDS, (uint32_t)n, p.E, d_rows, (uint64_t)(n * 4));
    }
    HALO_HIP(hipGetLastError());
    return fr_sum_rows(ctx, d_rows, n * 4, P, n);
}

int h_eval_batch(halo_ctx *ctx, const uint64_t *d_xis, size_t m, size_t lg_n, const host::Fr &z, uint64_t *d_out) {
    if (m == 0) return HALO_OK;
    HALO_LAUNCH(ctx, "k_h_eval", k_h_eval, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, d_xis, (uint32_t)m, (int)lg_n, to_arg(z), d_out);
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}

int h_eval_each(halo_ctx *ctx, const uint64_t *d_xis, const uint64_t *d_zs, size_t m, size_t lg_n, uint64_t *d_out) {
    if (m == 0) return HALO_OK;
    HALO_LAUNCH(ctx, "k_h_eval_z", k_h_eval_z, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, d_xis, d_zs, (uint32_t)m, (int)lg_n, d_out);
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}

}  // namespace halo
