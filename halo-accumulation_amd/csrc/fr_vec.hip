// K4-K6, K9: the Fr vector kernels behind pcdl::open's halving loop (pcdl.rs:195-227), construct_powers (group.rs:29-37),
// scalar_dot (group.rs:13-15) and p(z) (pcdl.rs:135), with the input generator and the bookkeeping of the no-fold rounds.
//
// Fr work is one 32-byte element per lane, loaded as two dwordx4 from contiguous arrays
// (coalesced 2 KiB per wave-instruction pair); these kernels are the HBM-bound part of the path.
//
// Member-batched forms (halo_pcdl_open_batch): every kernel of one open has a `_batch` twin with blockIdx.y = member, and the two
// share ONE device function.  The twin differs only in where its operands come from: member b's vectors at b * ms words from the
// base pointers, its window table / partial sums / results at b * OPEN_TAB_WORDS / OPEN_PART_WORDS / OPEN_OUT_WORDS, its field
// constants in record b of `consts` (OpenConst, device memory) where the single kernel has by-value arguments.  Everything a
// block reads of its member is the same for all of its lanes: control flow stays wave-uniform over the member index.
#include "curve.hpp"  // (fe_shfl)
#include "fr29.hpp"
#include "fr_plan.hpp"
#include "internal.hpp"

namespace halo {

HALO_DEV const OpenConst &open_const(const uint64_t *consts) { return *(const OpenConst *)(consts + OPEN_CONST_WORDS * (size_t)blockIdx.y); }

// ------------------------------------------------------------------ K4: c' = c_l + xi^-1 c_r ; z' = z_l + xi z_r
// 192 bytes moved and two products per element: HBM-bound with the 29-bit product (fr29.hpp)
HALO_DEV void fold_scalars_body(uint64_t *__restrict__ c, uint64_t *__restrict__ z, uint32_t m, const FsArg &xi, const FsArg &xi_inv) {
    uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    Fe cl = fe_load(c + 4 * (size_t)j), cr = fe_load(c + 4 * (size_t)(j + m));
    Fe zl = fe_load(z + 4 * (size_t)j), zr = fe_load(z + 4 * (size_t)(j + m));
    fs_store(c + 4 * (size_t)j, fs_add(fs_from_fe(cl), fs_mul(fs_from_fe(cr), from_nform(xi_inv))));
    fs_store(z + 4 * (size_t)j, fs_add(fs_from_fe(zl), fs_mul(fs_from_fe(zr), from_nform(xi))));
}
__global__ __launch_bounds__(256) void k_fold_scalars(uint64_t *__restrict__ c, uint64_t *__restrict__ z, uint32_t m, FsArg xi,
                                                      FsArg xi_inv) {
    fold_scalars_body(c, z, m, xi, xi_inv);
}
__global__ __launch_bounds__(256) void k_fold_scalars_batch(uint64_t *__restrict__ c, uint64_t *__restrict__ z, uint64_t ms, uint32_t m,
                                                            const uint64_t *__restrict__ consts) {
    const OpenConst &k = open_const(consts);
    fold_scalars_body(c + ms * blockIdx.y, z + ms * blockIdx.y, m, k.xi_n, k.xi_inv_n);
}

// ------------------------------------------------------------------ block-wide Fr sum
HALO_DEV Fe block_sum_fr(Fe v, Fe *lds /* >= 4 entries */) {
    int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll 1
    for (int off = 32; off >= 1; off >>= 1) {
        Fe o = fe_shfl(v, (lane + off) & 63);
        if (lane < off) v = fe_add<FrCfg>(v, o);
    }
    if (lane == 0) lds[wave] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < (int)(blockDim.x >> 6); w++) v = fe_add<FrCfg>(v, lds[w]);
    }
    return v;  // valid in thread 0
}

// ------------------------------------------------------------------ K5: two dot products per launch
// A lane takes two elements of each pair of vectors per trip -- x_i y_i + x_j y_j share one reduction -- and the next
// trip's operands are requested before the current products run.  The products of two A-form values carry 1/32
// (fr29.hpp): the partial sums stay in that skewed form and k_sum_partials multiplies the total by 32 once.
// The grid is kept small (two waves per SIMD): with one trip per lane the block-wide sum cost as many instructions as the
// products themselves.
struct DotOps { Fe x, y, x2, y2; };
HALO_DEV DotOps dot_load(const uint64_t *__restrict__ xs, const uint64_t *__restrict__ ys, uint32_t i, uint32_t i2, uint32_t m) {
    DotOps o;
    uint32_t j = i2 < m ? i2 : i;  // (past the end: the slot re-reads element i and is zeroed)
    o.x = fe_load(xs + 4 * (size_t)i); o.y = fe_load(ys + 4 * (size_t)i);
    o.x2 = fe_load(xs + 4 * (size_t)j); o.y2 = fe_load(ys + 4 * (size_t)j);
    if (i2 >= m) o.x2 = fe_zero();
    return o;
}
HALO_DEV Fs<2> dot_step(const Fs<2> &acc, const DotOps &o) {
    return fs_tighten(fs_add(acc, fs_mul_add_mul(fs_from_fe(o.x), fs_from_fe(o.y), fs_from_fe(o.x2), fs_from_fe(o.y2))));
}
template <bool HAS1>
HALO_DEV void dot2_partial_body(const uint64_t *__restrict__ xs0, const uint64_t *__restrict__ ys0, const uint64_t *__restrict__ xs1,
                                const uint64_t *__restrict__ ys1, uint32_t m, uint64_t *__restrict__ partial, Fe *lds /* 8 */) {
    Fs<2> a0 = fs_zero<2>(), a1 = fs_zero<2>();
    const uint32_t stride = gridDim.x * 256;
    uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < m) {
        DotOps n0 = dot_load(xs0, ys0, i, i + stride, m), n1 = n0;
        if (HAS1) n1 = dot_load(xs1, ys1, i, i + stride, m);
        for (; i < m; i += 2 * stride) {
            DotOps c0 = n0, c1 = n1;
            uint32_t nx = i + 2 * stride;
            if (nx < m) {
                n0 = dot_load(xs0, ys0, nx, nx + stride, m);
                if (HAS1) n1 = dot_load(xs1, ys1, nx, nx + stride, m);
            }
            a0 = dot_step(a0, c0);
            if (HAS1) a1 = dot_step(a1, c1);
        }
    }
    Fe s0 = block_sum_fr(fs_to_fe(a0), lds), s1 = fe_zero();
    if (HAS1) {
        __syncthreads();
        s1 = block_sum_fr(fs_to_fe(a1), lds + 4);
    }
    if (threadIdx.x == 0) {
        fe_store(partial + 8 * (size_t)blockIdx.x, s0);
        fe_store(partial + 8 * (size_t)blockIdx.x + 4, s1);
    }
}
template <bool HAS1>
__global__ __launch_bounds__(256) void k_dot2_partial(const uint64_t *__restrict__ xs0, const uint64_t *__restrict__ ys0,
                                                      const uint64_t *__restrict__ xs1, const uint64_t *__restrict__ ys1, uint32_t m,
                                                      uint64_t *__restrict__ partial) {
    __shared__ Fe lds[8];
    dot2_partial_body<HAS1>(xs0, ys0, xs1, ys1, m, partial, lds);
}
// <c_r, z_l> and <c_l, z_r> of each member (k_dot2_partial<true>)
__global__ __launch_bounds__(256) void k_dot2_partial_batch(const uint64_t *__restrict__ c, const uint64_t *__restrict__ z, uint64_t ms, uint32_t m,
                                                            uint64_t *__restrict__ parts) {
    __shared__ Fe lds[8];
    const size_t o = ms * blockIdx.y;
    dot2_partial_body<true>(c + o + 4 * (size_t)m, z + o, c + o, z + o + 4 * (size_t)m, m, parts + OPEN_PART_WORDS * (size_t)blockIdx.y, lds);
}
// sums `count` partial records of `width` Fr each into out[width]; times32: the records are sums of A(x) A(y) products
// (1/32 of the A-form value): the total is multiplied by 32 (fr29.hpp C266)
HALO_DEV void sum_partials_body(const uint64_t *__restrict__ partial, uint32_t count, uint32_t width, int times32, uint64_t *__restrict__ out,
                                Fe *lds /* 4 */) {
    for (uint32_t k = 0; k < width; k++) {
        Fe a = fe_zero();
        for (uint32_t i = threadIdx.x; i < count; i += 256) a = fe_add<FrCfg>(a, fe_load(partial + 4 * ((size_t)i * width + k)));
        Fe s = block_sum_fr(a, lds);
        if (threadIdx.x == 0) {
            if (times32) s = fs_to_fe(fs_mul(fs_from_fe(s), fs_c266()));
            fe_store(out + 4 * (size_t)k, s);
        }
        __syncthreads();
    }
}
__global__ __launch_bounds__(256) void k_sum_partials(const uint64_t *__restrict__ partial, uint32_t count, uint32_t width, int times32,
                                                      uint64_t *__restrict__ out) {
    __shared__ Fe lds[4];
    sum_partials_body(partial, count, width, times32, out, lds);
}
// one block per member: k_sum_partials into the member's result record
__global__ __launch_bounds__(256) void k_sum_partials_batch(const uint64_t *__restrict__ parts, uint32_t count, uint32_t width, int times32,
                                                            uint64_t *__restrict__ outs) {
    __shared__ Fe lds[4];
    sum_partials_body(parts + OPEN_PART_WORDS * (size_t)blockIdx.y, count, width, times32, outs + OPEN_OUT_WORDS * (size_t)blockIdx.y, lds);
}

// ---- powers of one scalar: the window table the host prepares (upload_window_table)
//   tab[d]               = A(z^d),          d < 16           (window 0 in A-form: seeds of k_powers)
//   tab[16 + 16 k + d]   = N(z^(d 16^k)),   d < 16, k < nwin
// z^e is a product of one entry per window: nwin - 1 products for any lane, whatever its exponent (a square-and-multiply
// over a table of z^(2^k) ran up to 17 divergent products per lane: that, not bandwidth, was what k_powers and
// k_poly_eval_partial spent their time on).
constexpr int POW_WIN = 8;  // most windows: exponents below 2^32
// every table entry is requested before the first product runs (the entries' addresses depend on e only): one memory
// latency per seed, not one per window
HALO_DEV Fs<4> window_power(const uint64_t *__restrict__ tab, uint32_t e, int nwin, bool a_form) {
    Fe w[POW_WIN];
#pragma unroll
    for (int k = 0; k < POW_WIN; k++) {
        uint32_t idx = k == 0 ? (a_form ? 0u : 16u) + (e & 15u) : 16u + 16u * (uint32_t)k + ((e >> (4 * k)) & 15u);
        w[k] = fe_load(tab + 4 * (size_t)(k < nwin ? idx : 0u));
    }
    Fs<4> acc = fs_from_fe(w[0]);
#pragma unroll
    for (int k = 1; k < POW_WIN; k++)
        if (k < nwin) acc = fs_widen<4>(fs_mul(acc, fs_from_fe(w[k])));  // (nwin is a kernel argument: wave-uniform)
    return acc;
}
// (elements per lane of these kernels, window count and grids: fr_plan.hpp)

// ------------------------------------------------------------------ K6: out[i] = z^i
// One product per 32 bytes written: VALU-bound (fr29.hpp: 5.3 TB/s if nothing else ran).  Lane l of a wave writes the
// elements base + l + 64 k: every store instruction of the wave covers 2 KiB of consecutive addresses.
HALO_DEV void powers_body(const uint64_t *__restrict__ tab, int nwin, int E, uint32_t n, const Fs<1> &step, uint64_t *__restrict__ out) {
    uint32_t wave = (blockIdx.x * 256 + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    uint32_t e = wave * (64u * (uint32_t)E) + lane;
    if (e >= n) return;
    Fs<2> cur = fs_tighten(window_power(tab, e, nwin, true));
#pragma unroll 1
    for (int k = 0; k < E && e < n; k++, e += 64) {
        fs_store(out + 4 * (size_t)e, cur);  // (a product's result is below 2 r: one conditional subtraction)
        cur = fs_mul(cur, step);
    }
}
__global__ __launch_bounds__(256) void k_powers(const uint64_t *__restrict__ tab, int nwin, int E, uint32_t n, FsArg z64, uint64_t *__restrict__ out) {
    powers_body(tab, nwin, E, n, from_nform(z64), out);
}
// z_b^i, i < n
__global__ __launch_bounds__(256) void k_powers_batch(const uint64_t *__restrict__ tabs, const uint64_t *__restrict__ consts, int nwin, int E,
                                                      uint32_t n, uint64_t *__restrict__ out, uint64_t ms) {
    powers_body(tabs + OPEN_TAB_WORDS * (size_t)blockIdx.y, nwin, E, n, from_nform(open_const(consts).z64_n), out + ms * blockIdx.y);
}

// ------------------------------------------------------------------ K9: p(z)
// Lane l of a wave takes the coefficients base + l + 64 k, k < E (coalesced loads), and multiplies each by N(z^(64 k)) -- a
// table entry that is the same for every lane of every wave -- two products per reduction (fs_mul_add_mul); then one
// product with N(z^(base + l)).  The E products of a lane are INDEPENDENT: the Horner chain in z^64 this replaces (VERDICT
// r3 weak #7: 1.34 TB/s, half of the kernel's own VALU bound) was E dependent products on a grid of one wave per SIMD, i.e.
// one product in flight per SIMD; here the next pair's operands are in flight and its products issue while the current
// reduction runs.
HALO_DEV void poly_eval_partial_body(const uint64_t *__restrict__ coeffs, uint32_t len, const uint64_t *__restrict__ tab, int nwin, int E,
                                     const uint64_t *__restrict__ zpow, uint64_t *__restrict__ partial, Fe *lds /* 4 */) {
    Fs<2> acc = fs_zero<2>();
    uint32_t lane = threadIdx.x & 63u, nwaves = gridDim.x * 4;
    for (uint32_t wave = (blockIdx.x * 256 + threadIdx.x) >> 6; (size_t)wave * (64u * (uint32_t)E) < len; wave += nwaves) {
        uint32_t base = wave * (64u * (uint32_t)E) + lane;
        if (base >= len) continue;
        Fs<2> h = fs_zero<2>();
        // four coefficients per trip, written out (the unroller does not duplicate the products' inline asm): two fused
        // pairs whose operands are all requested before the first product runs; E is a multiple of 4 (pow_chain_len)
#pragma unroll 1
        for (int k = 0; k < E; k += 4) {
            Fe c[4], pw[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                uint32_t i = base + 64u * (uint32_t)(k + q);
                c[q] = fe_load(coeffs + 4 * (size_t)(i < len ? i : base));
                pw[q] = fe_load(zpow + 4 * (size_t)(k + q));
                if (i >= len) c[q] = fe_zero();
            }
            Fs<2> t0 = fs_mul_add_mul(fs_from_fe(c[0]), fs_from_fe(pw[0]), fs_from_fe(c[1]), fs_from_fe(pw[1]));
            Fs<2> t1 = fs_mul_add_mul(fs_from_fe(c[2]), fs_from_fe(pw[2]), fs_from_fe(c[3]), fs_from_fe(pw[3]));
            h = fs_tighten(fs_add(h, fs_add(t0, t1)));
        }
        acc = fs_tighten(fs_add(acc, fs_mul(h, window_power(tab, base, nwin, false))));
    }
    Fe s = block_sum_fr(fs_to_fe(acc), lds);
    if (threadIdx.x == 0) fe_store(partial + 4 * (size_t)blockIdx.x, s);
}
__global__ __launch_bounds__(256) void k_poly_eval_partial(const uint64_t *__restrict__ coeffs, uint32_t len, const uint64_t *__restrict__ tab,
                                                           int nwin, int E, const uint64_t *__restrict__ zpow, uint64_t *__restrict__ partial) {
    __shared__ Fe lds[4];
    poly_eval_partial_body(coeffs, len, tab, nwin, E, zpow, partial, lds);
}
// v_b = p_b(z_b): k_poly_eval_partial over each member's coefficients with its own table (zpow behind the window entries)
__global__ __launch_bounds__(256) void k_poly_eval_partial_batch(const uint64_t *__restrict__ coeffs, uint64_t ms, uint32_t len,
                                                                 const uint64_t *__restrict__ tabs, int nwin, int E, uint64_t *__restrict__ parts) {
    __shared__ Fe lds[4];
    const uint64_t *tab = tabs + OPEN_TAB_WORDS * (size_t)blockIdx.y;
    poly_eval_partial_body(coeffs + ms * blockIdx.y, len, tab, nwin, E, tab + 4 * (size_t)(16 * (1 + nwin)), parts + OPEN_PART_WORDS * (size_t)blockIdx.y, lds);
}

// ------------------------------------------------------------------ input generator / polynomial helpers
// SplitMix64 is counter based: draw k of a stream with state s0 is mix(s0 + k*gamma), so the
// scalars of `PallasPoly::rand` (pcdl.rs:141) can be produced in parallel, bit-identical to a
// sequential host stream.  Element i uses draws 4i+1 .. 4i+4, reduced mod r, to Montgomery form.
HALO_DEV uint64_t splitmix_at(uint64_t s0, uint64_t k) {
    uint64_t z = s0 + k * 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
// element `idx` of the scalar stream that starts after state s0, in Montgomery form
HALO_DEV Fe rng_scalar_at(uint64_t s0, uint64_t idx) {
    Fe v;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        uint64_t w = splitmix_at(s0, 4 * idx + k + 1);
        v.v[2 * k] = (uint32_t)w;
        v.v[2 * k + 1] = (uint32_t)(w >> 32);
    }
    // 2^256 < 4r: at most three subtractions
#pragma unroll 1
    for (int r = 0; r < 3; r++) {
        uint32_t d[8];
        uint64_t br = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            uint64_t t = (uint64_t)v.v[k] - FrCfg::P[k] - br;
            d[k] = (uint32_t)t;
            br = (t >> 32) & 1;
        }
        if (!br) {
#pragma unroll
            for (int k = 0; k < 8; k++) v.v[k] = d[k];
        }
    }
    return fe_to_mont<FrCfg>(v);
}
__global__ __launch_bounds__(256) void k_rng_scalars(uint64_t s0, uint32_t n, uint64_t *__restrict__ out) {
    uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    fe_store(out + 4 * (size_t)i, rng_scalar_at(s0, i));
}
// p_b = deg + 1 scalars of the stream after s_p, zero-padded to n (random_instance's PallasPoly::rand)
__global__ __launch_bounds__(256) void k_rng_batch(const uint64_t *__restrict__ consts, uint32_t n, uint64_t *__restrict__ out, uint64_t ms) {
    uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const OpenConst &k = open_const(consts);
    fe_store(out + ms * blockIdx.y + 4 * (size_t)i, i <= k.deg ? rng_scalar_at(k.s_p, i) : fe_zero());
}
// A cyclic shard of p_bar = q (X - z) straight from the stream (q is never materialised):
// out[j] = p_bar[offset + j*stride] = q[i-1] - z q[i], q[k] = stream element k for k < deg, else 0
HALO_DEV void pbar_stream_body(uint64_t s0, uint32_t deg, const FeArg &z, uint32_t stride, uint32_t offset, uint32_t n_local,
                               uint64_t *__restrict__ out) {
    uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n_local) return;
    uint64_t i = (uint64_t)offset + (uint64_t)j * stride;
    Fe r = fe_zero();
    if (i <= deg) {
        Fe lo = (i >= 1) ? rng_scalar_at(s0, i - 1) : fe_zero();
        Fe hi = (i < deg) ? rng_scalar_at(s0, i) : fe_zero();
        r = fe_sub<FrCfg>(lo, fe_mul<FrCfg>(from_arg(z), hi));
    }
    fe_store(out + 4 * (size_t)j, r);
}
__global__ __launch_bounds__(256) void k_pbar_stream(uint64_t s0, uint32_t deg, FeArg zarg, uint32_t stride, uint32_t offset,
                                                     uint32_t n_local, uint64_t *__restrict__ out) {
    pbar_stream_body(s0, deg, zarg, stride, offset, n_local, out);
}
// p_bar_b = q_b (X - z_b) over all n coefficients (zero past deg), q_b = deg scalars of the stream after s_q: the whole of the
// member's p_bar as one shard (stride 1, offset 0)
__global__ __launch_bounds__(256) void k_pbar_batch(const uint64_t *__restrict__ consts, uint32_t n, uint64_t *__restrict__ out, uint64_t ms) {
    const OpenConst &k = open_const(consts);
    pbar_stream_body(k.s_q, k.deg, k.z_m, 1, 0, n, out + ms * blockIdx.y);
}
// p_bar = q * (X - z): p_bar[i] = q[i-1] - z q[i], i in [0, deg]; q has deg coefficients (pcdl.rs:140-142)
__global__ __launch_bounds__(256) void k_pbar(const uint64_t *__restrict__ q, uint32_t deg, FeArg zarg, uint64_t *__restrict__ out) {
    uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i > deg) return;
    Fe z = from_arg(zarg);
    Fe lo = (i >= 1) ? fe_load(q + 4 * (size_t)(i - 1)) : fe_zero();
    Fe hi = (i < deg) ? fe_load(q + 4 * (size_t)i) : fe_zero();
    fe_store(out + 4 * (size_t)i, fe_sub<FrCfg>(lo, fe_mul<FrCfg>(z, hi)));
}
// y[i] += a * x[i]   (p' = p + alpha p_bar, pcdl.rs:156): 96 bytes moved per product, HBM-bound
HALO_DEV void axpy_body(uint64_t *__restrict__ y, const uint64_t *__restrict__ x, uint32_t n, const FsArg &a) {
    uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    Fe yv = fe_load(y + 4 * (size_t)i), xv = fe_load(x + 4 * (size_t)i);
    fs_store(y + 4 * (size_t)i, fs_add(fs_from_fe(yv), fs_mul(fs_from_fe(xv), from_nform(a))));
}
__global__ __launch_bounds__(256) void k_axpy(uint64_t *__restrict__ y, const uint64_t *__restrict__ x, uint32_t n, FsArg aarg) {
    axpy_body(y, x, n, aarg);
}
// y_b[i] += alpha_b x_b[i], i < len_b
__global__ __launch_bounds__(256) void k_axpy_batch(uint64_t *__restrict__ y, const uint64_t *__restrict__ x, uint64_t ms, const uint64_t *__restrict__ consts) {
    const OpenConst &k = open_const(consts);
    axpy_body(y + ms * blockIdx.y, x + ms * blockIdx.y, k.len, k.alpha_n);
}
// v[i] *= a   (z-powers of a cyclic shard: z^(r + jP) = z^r * (z^P)^j)
__global__ __launch_bounds__(256) void k_scale(uint64_t *__restrict__ v, uint32_t n, FeArg aarg) {
    uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    fe_store(v + 4 * (size_t)i, fe_mul<FrCfg>(fe_load(v + 4 * (size_t)i), from_arg(aarg)));
}

// ------------------------------------------------------------------ "no-fold" late rounds
// Once the key has been folded down to M points (G0), folding it further is latency-bound
// (one uniform scalar multiplication is a ~1 ms serial chain whatever m is).  Instead G0 stays
// fixed and the folded key is kept implicitly:  G_k[j] = sum_t s[t] * G0[j + t*m]  with
// s = products of the challenges since the switch.  Then
//   L = <c_r, G_l> = sum_{b: (b mod m) <  m/2} (c[(b mod m) + m/2] * s[b div m]) * G0[b]
//   R = <c_l, G_r> = sum_{b: (b mod m) >= m/2} (c[(b mod m) - m/2] * s[b div m]) * G0[b]
// are two MSMs over the fixed G0 (half of each scalar vector is zero and is skipped at recode).
HALO_DEV void nofold_expand_body(const uint64_t *__restrict__ c, const uint64_t *__restrict__ sv, uint32_t m, int log2m, uint32_t M,
                                 uint64_t *__restrict__ outL, uint64_t *__restrict__ outR) {
    uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b >= M) return;
    uint32_t u = b & (m - 1), t = b >> log2m, h = m >> 1;
    Fe sc = fe_load(sv + 4 * (size_t)t);
    if (u < h) {
        fe_store(outL + 4 * (size_t)b, fe_mul<FrCfg>(fe_load(c + 4 * (size_t)(u + h)), sc));
        fe_store(outR + 4 * (size_t)b, fe_zero());
    } else {
        fe_store(outR + 4 * (size_t)b, fe_mul<FrCfg>(fe_load(c + 4 * (size_t)(u - h)), sc));
        fe_store(outL + 4 * (size_t)b, fe_zero());
    }
}
__global__ __launch_bounds__(256) void k_nofold_expand(const uint64_t *__restrict__ c, const uint64_t *__restrict__ sv, uint32_t m,
                                                       int log2m, uint32_t M, uint64_t *__restrict__ outL, uint64_t *__restrict__ outR) {
    nofold_expand_body(c, sv, m, log2m, M, outL, outR);
}
// each member from its own c and s
__global__ __launch_bounds__(256) void k_nofold_expand_batch(const uint64_t *__restrict__ c, const uint64_t *__restrict__ sv, uint64_t ms, uint32_t m,
                                                             int log2m, uint32_t M, uint64_t *__restrict__ outL, uint64_t *__restrict__ outR) {
    const size_t o = ms * blockIdx.y;
    nofold_expand_body(c + o, sv + o, m, log2m, M, outL + o, outR + o);
}
// The same two vectors as ONE array for a tagged launch (msm_table.hip, MsmBatch::tagged): L's and R's non-zero scalars sit on
// disjoint points, so F[b] = c[(b mod m) +- m/2] * s[b div m] in canonical form with bit 255 (free: r < 2^255) set on R's half
// says everything -- half the bytes written, and one launch sequence computes both sums.
__global__ __launch_bounds__(256) void k_nofold_expand_tagged(const uint64_t *__restrict__ c, const uint64_t *__restrict__ sv, uint32_t m,
                                                              int log2m, uint32_t M, uint64_t *__restrict__ out) {
    uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b >= M) return;
    uint32_t u = b & (m - 1), t = b >> log2m, h = m >> 1;
    Fe v = fe_mul<FrCfg>(fe_load(c + 4 * (size_t)(u < h ? u + h : u - h)), fe_load(sv + 4 * (size_t)t));
    v = fe_from_mont<FrCfg>(v);
    if (u >= h) v.v[7] |= 0x80000000u;
    fe_store(out + 4 * (size_t)b, v);
}
// s'[2t + u] = s[t] * xi^u : the stride of the implicit key halves (pcdl.rs:218 applied to the representation)
HALO_DEV void nofold_s_update_body(const uint64_t *__restrict__ s_in, uint32_t len, const FeArg &xi, uint64_t *__restrict__ s_out) {
    uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * len) return;
    Fe v = fe_load(s_in + 4 * (size_t)(i >> 1));
    if (i & 1) v = fe_mul<FrCfg>(v, from_arg(xi));
    fe_store(s_out + 4 * (size_t)i, v);
}
__global__ __launch_bounds__(256) void k_nofold_s_update(const uint64_t *__restrict__ s_in, uint32_t len, FeArg xi,
                                                         uint64_t *__restrict__ s_out) {
    nofold_s_update_body(s_in, len, xi, s_out);
}
// with each member's xi
__global__ __launch_bounds__(256) void k_nofold_s_update_batch(const uint64_t *__restrict__ s_in, uint64_t *__restrict__ s_out, uint64_t ms, uint32_t len,
                                                               const uint64_t *__restrict__ consts) {
    nofold_s_update_body(s_in + ms * blockIdx.y, len, open_const(consts).xi_m, s_out + ms * blockIdx.y);
}

// The short members of one commit group zero-padded to n scalars in ONE launch (halo_pcdl_commit_dev_batch): blockIdx.y = entry
// of the table that arrives with the launch -- source, length and row of the group's staging -- and a lane moves 16 bytes, half
// a scalar: the source's below 2 len, zero from there to 2 n.  The sources are only read.
__global__ __launch_bounds__(256) void k_pad_members_batch(PadMembers t, uint32_t n, uint64_t *__restrict__ out, uint64_t ms) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * n) return;
    const uint4 *src = reinterpret_cast<const uint4 *>(t.src[blockIdx.y]);
    uint4 v = make_uint4(0, 0, 0, 0);
    if (i < 2 * t.len[blockIdx.y]) v = src[i];
    reinterpret_cast<uint4 *>(out + ms * t.row[blockIdx.y])[i] = v;
}

// DensePolynomial::degree of m device-resident rows in ONE launch (halo_poly_degrees_dev; host_poly_degree on the host): blockIdx.y =
// row of the table in device memory, blockIdx.x = the row's chunk of DEG_CHUNK scalars, a lane reads 16 bytes (half a scalar) per
// pass of DEG_LANES lanes.  A wave keeps the highest scalar of its lanes with a non-zero half (the ballot's top bit; the passes
// ascend) and publishes index + 1 with one atomicMax into the row's `top`, which arrives zeroed: 0 stays "no non-zero scalar".
// The rows are only read; no shared memory, no scratch.
__global__ __launch_bounds__(256) void k_poly_degree_batch(DegreeRow *rows) {
    DegreeRow *r = rows + blockIdx.y;
    const uint64_t len = r->len, lo = (uint64_t)blockIdx.x * DEG_CHUNK;
    if (lo >= len) return;
    const uint64_t end = 2 * (lo + DEG_CHUNK < len ? lo + DEG_CHUNK : len);  // in halves
    const uint4 *src = reinterpret_cast<const uint4 *>(r->src);
    const uint32_t wave0 = threadIdx.x & ~63u;
    uint32_t top = 0;
    for (uint64_t base = 2 * lo; base < end; base += DEG_LANES) {  // (uniform over the block: every lane reaches the ballot)
        const uint64_t i = base + threadIdx.x;
        bool nz = false;
        if (i < end) {
            const uint4 v = src[i];
            nz = (v.x | v.y | v.z | v.w) != 0;
        }
        const uint64_t mask = __ballot(nz);
        if (mask) top = (uint32_t)((base + wave0 + (63 - __clzll((long long)mask))) >> 1) + 1;
    }
    if ((threadIdx.x & 63) == 0 && top) atomicMax(&r->top, top);
}

// ------------------------------------------------------------------ the partial rows of the combined check's scalars
// rows[0][k] = sum_p rows[p][k] over P rows of n elements at `stride` words (halo_pcdl_check_batch_combined: the parts of
// sum_a r_a h_a(X), hpoly.hip h_combine_rows).  One element per lane; the running sum stays in the lazy 29-bit form, brought back
// below 2 r after every addition as h_acc_step does (a canonical element is < r, the sum < 6 r before fs_tighten), so the bound
// does not depend on P; ONE canonical store per element.  Field sums are exact: the words do not depend on P.
__global__ __launch_bounds__(256) void k_fr_sum_rows(uint64_t *__restrict__ rows, uint64_t stride, uint32_t P, uint32_t n) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    Fs<2> acc = fs_tighten(fs_load(rows + 4 * (size_t)k));
#pragma unroll 1
    for (uint32_t p = 1; p < P; p++) acc = fs_tighten(fs_add(acc, fs_load(rows + (size_t)p * stride + 4 * (size_t)k)));
    fs_store(rows + 4 * (size_t)k, acc);
}

// ================================================================== host launchers
int ipa_fold_scalars(halo_ctx *ctx, uint64_t *d_c, uint64_t *d_z, size_t m, const host::Fr &xi, const host::Fr &xi_inv) {
    if (m == 0) return HALO_OK;
    HALO_LAUNCH(ctx, "k_fold_scalars", k_fold_scalars, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, d_c, d_z, (uint32_t)m, to_nform(xi),
                to_nform(xi_inv));
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}

// the two halves of fr_dot2: launch (kernels + the copy of the two sums to pinned memory, on ctx->stream) and collect (wait)
int fr_dot2_launch(halo_ctx *ctx, const uint64_t *xs0, const uint64_t *ys0, const uint64_t *xs1, const uint64_t *ys1, size_t m) {
    if (m == 0) return HALO_OK;
    if (!xs0) { set_error("dot2: the first pair of vectors is required"); return HALO_E_ARG; }
    unsigned nb = plan_dot(m).blocks;  // (<= FR_GRID_CAP)
    uint64_t *partial = ctx->d_tmp_c;  // >= 1024 * 8 words
    if (xs1) HALO_LAUNCH(ctx, "k_dot2_partial", k_dot2_partial<true>, dim3(nb), dim3(256), 0, xs0, ys0, xs1, ys1, (uint32_t)m, partial);
    else HALO_LAUNCH(ctx, "k_dot2_partial", k_dot2_partial<false>, dim3(nb), dim3(256), 0, xs0, ys0, xs1, ys1, (uint32_t)m, partial);
    HALO_LAUNCH(ctx, "k_sum_partials", k_sum_partials, dim3(1), dim3(256), 0, partial, nb, 2u, 1, partial + 8 * 1024);
    HALO_HIP(hipGetLastError());
    HALO_HIP(hipMemcpyAsync(ctx->h_pinned, partial + 8 * 1024, 64, hipMemcpyDeviceToHost, ctx->stream));
    return HALO_OK;
}
int fr_dot2_collect(halo_ctx *ctx, hipStream_t stream, size_t m, host::Fr out[2]) {
    out[0] = out[1] = host::Fr::zero();
    if (m == 0) return HALO_OK;
    HALO_HIP(hipStreamSynchronize(stream));
    out[0] = host::Fr::load(ctx->h_pinned);
    out[1] = host::Fr::load(ctx->h_pinned + 4);
    return HALO_OK;
}
int fr_dot2(halo_ctx *ctx, const uint64_t *xs0, const uint64_t *ys0, const uint64_t *xs1, const uint64_t *ys1, size_t m,
            host::Fr out[2]) {
    out[0] = out[1] = host::Fr::zero();
    int rc = fr_dot2_launch(ctx, xs0, ys0, xs1, ys1, m);
    if (rc) return rc;
    return fr_dot2_collect(ctx, ctx->stream, m, out);
}

// Window table of z (see window_power): 16 A-form entries, then nwin x 16 N-form entries, staged through pinned memory.
// ~32 nwin host products (a few microseconds).
// zpows > 0: N(z^(64 k)), k < zpows, behind the window table (k_poly_eval_partial's per-element multipliers)
// fills h (16 (1 + nwin) + zpows entries of 4 words); -1 if that is more than 256 entries
static long fill_window_table(const host::Fr &z, int nwin, uint64_t *h, host::Fr *z64, int zpows) {
    const host::Fr k32 = host::Fr::from_u64(32);
    host::Fr base = z;  // z^(16^k)
    for (int k = 0; k < nwin; ++k) {
        host::Fr cur = host::Fr::one();
        for (int d = 0; d < 16; ++d) {
            if (k == 0) cur.store(h + 4 * d);
            (cur * k32).store(h + 4 * (16 + 16 * k + d));
            cur = cur * base;
        }
        base = cur;  // z^(16^(k+1))
    }
    host::Fr t = z;
    for (int i = 0; i < 6; ++i) t = t.sqr();
    *z64 = t;
    size_t entries = (size_t)16 * (1 + nwin);
    if (entries + (size_t)zpows > 256) return -1;  // (h_wintab: 256 entries)
    host::Fr cur = host::Fr::one();
    for (int k = 0; k < zpows; ++k) {
        (cur * k32).store(h + 4 * (entries + (size_t)k));
        cur = cur * t;
    }
    return (long)(entries + (size_t)zpows);
}
static int upload_window_table(halo_ctx *ctx, const host::Fr &z, int nwin, uint64_t *d_tab, host::Fr *z64, int zpows = 0) {
    uint64_t *h = ctx->h_wintab;  // pinned, 1024 words: nwin <= 15
    long entries = fill_window_table(z, nwin, h, z64, zpows);
    if (entries < 0) { set_error("window table: too many entries"); return HALO_E_ARG; }
    HALO_HIP(hipMemcpyAsync(d_tab, h, (size_t)entries * 32, hipMemcpyHostToDevice, ctx->stream));
    HALO_HIP(hipStreamSynchronize(ctx->stream));  // the staging memory is reused by the next call
    return HALO_OK;
}
int fr_powers(halo_ctx *ctx, const host::Fr &z, size_t n, uint64_t *d_out) {
    if (n == 0) return HALO_OK;
    uint64_t *d_tab = ctx->d_tmp_c + 8 * 1024 + 64;
    const FrPlan p = plan_powers(n);
    host::Fr z64;
    int rc = upload_window_table(ctx, z, p.nwin, d_tab, &z64);
    if (rc) return rc;
    HALO_LAUNCH(ctx, "k_powers", k_powers, dim3(p.blocks), dim3(256), 0, d_tab, p.nwin, p.E, (uint32_t)n, to_nform(z64), d_out);
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}

int fr_poly_eval(halo_ctx *ctx, const uint64_t *d_coeffs, size_t len, const host::Fr &z, host::Fr *out) {
    *out = host::Fr::zero();
    if (len == 0) return HALO_OK;
    uint64_t *d_tab = ctx->d_tmp_c + 8 * 1024 + 64;
    const FrPlan p = plan_poly_eval(len);
    const int nwin = p.nwin, E = p.E;
    host::Fr z64;
    int rc = upload_window_table(ctx, z, nwin, d_tab, &z64, E);
    if (rc) return rc;
    const unsigned nb = p.blocks;  // (<= FR_GRID_CAP: the waves stride over what the grid does not cover)
    uint64_t *partial = ctx->d_tmp_c;
    HALO_LAUNCH(ctx, "k_poly_eval_partial", k_poly_eval_partial, dim3(nb), dim3(256), 0, d_coeffs, (uint32_t)len, d_tab, nwin, E,
                d_tab + 4 * (size_t)(16 * (1 + nwin)), partial);
    HALO_LAUNCH(ctx, "k_sum_partials", k_sum_partials, dim3(1), dim3(256), 0, partial, nb, 1u, 0, partial + 8 * 1024);
    HALO_HIP(hipGetLastError());
    HALO_HIP(hipMemcpyAsync(ctx->h_pinned, partial + 8 * 1024, 32, hipMemcpyDeviceToHost, ctx->stream));
    HALO_HIP(hipStreamSynchronize(ctx->stream));
    *out = host::Fr::load(ctx->h_pinned);
    return HALO_OK;
}

int rng_scalars_dev(halo_ctx *ctx, uint64_t state0, size_t n, uint64_t *d_out) {
    if (n == 0) return HALO_OK;
    HALO_LAUNCH(ctx, "k_rng_scalars", k_rng_scalars, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, state0, (uint32_t)n, d_out);
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}
int pbar_dev(halo_ctx *ctx, const uint64_t *d_q, size_t deg, const host::Fr &z, uint64_t *d_out) {
    HALO_LAUNCH(ctx, "k_pbar", k_pbar, dim3((unsigned)((deg + 1 + 255) / 256)), dim3(256), 0, d_q, (uint32_t)deg, to_arg(z), d_out);
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}
int axpy_dev(halo_ctx *ctx, uint64_t *d_y, const uint64_t *d_x, size_t n, const host::Fr &a) {
    if (n == 0) return HALO_OK;
    HALO_LAUNCH(ctx, "k_axpy", k_axpy, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, d_y, d_x, (uint32_t)n, to_nform(a));
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}

// the least k with 2^k >= m
static int ceil_log2(size_t m) {
    int k = 0;
    while (((size_t)1 << k) < m) k++;
    return k;
}
int nofold_expand(halo_ctx *ctx, const uint64_t *d_c, const uint64_t *d_s, size_t m, size_t M, uint64_t *d_L, uint64_t *d_R) {
    HALO_LAUNCH(ctx, "k_nofold_expand", k_nofold_expand, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, d_c, d_s, (uint32_t)m, ceil_log2(m),
                (uint32_t)M, d_L, d_R);
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}
int nofold_expand_tagged(halo_ctx *ctx, const uint64_t *d_c, const uint64_t *d_s, size_t m, size_t M, uint64_t *d_F) {
    HALO_LAUNCH(ctx, "k_nofold_expand_tagged", k_nofold_expand_tagged, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, d_c, d_s, (uint32_t)m, ceil_log2(m),
                (uint32_t)M, d_F);
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}
int nofold_s_update(halo_ctx *ctx, const uint64_t *d_s_in, size_t len, const host::Fr &xi, uint64_t *d_s_out) {
    HALO_LAUNCH(ctx, "k_nofold_s_update", k_nofold_s_update, dim3((unsigned)((2 * len + 255) / 256)), dim3(256), 0, d_s_in, (uint32_t)len,
                to_arg(xi), d_s_out);
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}

int fr_scale(halo_ctx *ctx, uint64_t *d_v, size_t n, const host::Fr &a) {
    if (n == 0) return HALO_OK;
    HALO_LAUNCH(ctx, "k_scale", k_scale, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, d_v, (uint32_t)n, to_arg(a));
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}

int pbar_stream_dev(halo_ctx *ctx, uint64_t state0, size_t deg, const host::Fr &z, uint64_t stride, uint64_t offset, size_t n_local,
                    uint64_t *d_out) {
    if (n_local == 0) return HALO_OK;
    HALO_LAUNCH(ctx, "k_pbar_stream", k_pbar_stream, dim3((unsigned)((n_local + 255) / 256)), dim3(256), 0, state0, (uint32_t)deg, to_arg(z),
                (uint32_t)stride, (uint32_t)offset, (uint32_t)n_local, d_out);
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}


// ---- member-batched launchers (halo_pcdl_open_batch)
// One window table per member serves both of its uses: powers of z over n (window part) and p(z) over n coefficients (the
// zpow entries behind it); fr_powers / fr_poly_eval build the same entries.
int open_batch_table(const host::Fr &z, size_t n, uint64_t *h_tab, OpenConst *k) {
    const FrPlan p = plan_poly_eval_batch(n);  // (open_batch_eval's: the table carries its E multipliers)
    const int nwin = p.nwin;
    host::Fr z64;
    if (fill_window_table(z, nwin, h_tab, &z64, p.E) < 0) { set_error("window table: too many entries"); return HALO_E_ARG; }
    k->z64_n = to_nform(z64);
    k->z_m = to_arg(z);
    return HALO_OK;
}
void open_const_xi(OpenConst *k, const host::Fr &xi, const host::Fr &xi_inv) {
    k->xi_n = to_nform(xi);
    k->xi_inv_n = to_nform(xi_inv);
    k->xi_m = to_arg(xi);
}
void open_const_alpha(OpenConst *k, const host::Fr &alpha) {
    k->alpha_n = to_nform(alpha);
}
int open_batch_eval(halo_ctx *ctx, int G, const uint64_t *d_coeffs, size_t ms, size_t n, const uint64_t *d_tabs, uint64_t *d_parts, uint64_t *d_outs) {
    // at most OPEN_PART_WORDS / 4 partial records per member: the waves of a longer polynomial stride over the rest (the sums are
    // exact: any grid gives the same field element)
    const FrPlan p = plan_poly_eval_batch(n);
    const int nwin = p.nwin, E = p.E;
    const unsigned nb = p.blocks;
    if (n > OPEN_MAX_N || (size_t)nb * 4 > OPEN_PART_WORDS) { set_error("open_batch_eval: bad shape"); return HALO_E_ARG; }
    HALO_LAUNCH(ctx, "k_poly_eval_partial_batch", k_poly_eval_partial_batch, dim3(nb, (unsigned)G), dim3(256), 0, d_coeffs, (uint64_t)ms, (uint32_t)n,
                d_tabs, nwin, E, d_parts);
    HALO_LAUNCH(ctx, "k_sum_partials_batch", k_sum_partials_batch, dim3(1, (unsigned)G), dim3(256), 0, d_parts, nb, 1u, 0, d_outs);
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}
int open_batch_powers(halo_ctx *ctx, int G, const uint64_t *d_tabs, const uint64_t *d_consts, size_t n, uint64_t *d_z, size_t ms) {
    const FrPlan p = plan_powers(n);
    HALO_LAUNCH(ctx, "k_powers_batch", k_powers_batch, dim3(p.blocks, (unsigned)G), dim3(256), 0, d_tabs, d_consts, p.nwin, p.E, (uint32_t)n, d_z,
                (uint64_t)ms);
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}
int open_batch_pbar(halo_ctx *ctx, int G, const uint64_t *d_consts, size_t n, uint64_t *d_out, size_t ms) {
    HALO_LAUNCH(ctx, "k_pbar_batch", k_pbar_batch, dim3((unsigned)((n + 255) / 256), (unsigned)G), dim3(256), 0, d_consts, (uint32_t)n, d_out, (uint64_t)ms);
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}
int open_batch_rng(halo_ctx *ctx, int G, const uint64_t *d_consts, size_t n, uint64_t *d_out, size_t ms) {
    HALO_LAUNCH(ctx, "k_rng_batch", k_rng_batch, dim3((unsigned)((n + 255) / 256), (unsigned)G), dim3(256), 0, d_consts, (uint32_t)n, d_out, (uint64_t)ms);
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}
int open_batch_axpy(halo_ctx *ctx, int G, uint64_t *d_y, const uint64_t *d_x, size_t ms, size_t n, const uint64_t *d_consts) {
    HALO_LAUNCH(ctx, "k_axpy_batch", k_axpy_batch, dim3((unsigned)((n + 255) / 256), (unsigned)G), dim3(256), 0, d_y, d_x, (uint64_t)ms, d_consts);
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}
int open_batch_expand(halo_ctx *ctx, int G, const uint64_t *d_c, const uint64_t *d_s, size_t ms, size_t m, size_t M, uint64_t *d_L, uint64_t *d_R) {
    HALO_LAUNCH(ctx, "k_nofold_expand_batch", k_nofold_expand_batch, dim3((unsigned)((M + 255) / 256), (unsigned)G), dim3(256), 0, d_c, d_s, (uint64_t)ms,
                (uint32_t)m, ceil_log2(m), (uint32_t)M, d_L, d_R);
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}
int open_batch_dots(halo_ctx *ctx, int G, const uint64_t *d_c, const uint64_t *d_z, size_t ms, size_t m, uint64_t *d_parts, uint64_t *d_outs) {
    unsigned nb = plan_dot(m).blocks;
    // (the sums are exact: any grid gives the same field elements; from m = 2^16 on the 128 blocks' lanes make several trips)
    if (nb > OPEN_PART_WORDS / 8) nb = OPEN_PART_WORDS / 8;
    if (m > OPEN_MAX_N / 2) { set_error("open_batch_dots: bad shape"); return HALO_E_ARG; }
    HALO_LAUNCH(ctx, "k_dot2_partial_batch", k_dot2_partial_batch, dim3(nb, (unsigned)G), dim3(256), 0, d_c, d_z, (uint64_t)ms, (uint32_t)m, d_parts);
    HALO_LAUNCH(ctx, "k_sum_partials_batch", k_sum_partials_batch, dim3(1, (unsigned)G), dim3(256), 0, d_parts, nb, 2u, 1, d_outs + 4);
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}
int pad_members_batch(halo_ctx *ctx, const PadMembers &t, int count, size_t n, uint64_t *d_out, size_t ms) {
    if (count < 1 || count > MSM_MAX_BATCH || n == 0 || n > ((size_t)1 << 30)) { set_error("pad_members: bad shape"); return HALO_E_ARG; }
    for (int k = 0; k < count; ++k)
        if (t.len[k] > n || t.row[k] >= (uint32_t)MSM_MAX_BATCH || (t.len[k] && !t.src[k])) { set_error("pad_members: bad member"); return HALO_E_ARG; }
    HALO_LAUNCH(ctx, "k_pad_members_batch", k_pad_members_batch, dim3((unsigned)((2 * n + 255) / 256), (unsigned)count), dim3(256), 0, t, (uint32_t)n,
                d_out, (uint64_t)ms);
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}

// The degrees of m device rows (pointers and lengths checked by the caller: dev_rows_ok): the table goes up in one copy, with
// every `top` zero, and comes back in one; launches of at most 65535 rows (the grid's y limit), each as wide as its longest row.
// On ctx->stream, which is idle again on return.  The table's buffer is the context's own and only grows (24 bytes a row).
int poly_degrees_dev(halo_ctx *ctx, const void *const *d_coeffs, const size_t *lens, size_t m, size_t *degrees_out) {
    if (m == 0) return HALO_OK;
    if (m > ((size_t)1 << 40) / sizeof(DegreeRow)) { set_error("poly_degrees: too many rows"); return HALO_E_ARG; }
    std::vector<DegreeRow> rows(m);
    for (size_t i = 0; i < m; ++i) {
        if (lens[i] >= ((size_t)1 << 32) - 1) { set_error("poly_degrees: a row of 2^32 - 1 scalars or more"); return HALO_E_ARG; }
        rows[i] = DegreeRow{static_cast<const uint64_t *>(d_coeffs[i]), lens[i], 0, 0};
    }
    const size_t bytes = m * sizeof(DegreeRow);
    if (bytes > ctx->degree_bytes) {
        alloc_epoch_bump(ctx);
        (void)hipFree(ctx->d_degree_rows);
        ctx->d_degree_rows = nullptr;
        ctx->degree_bytes = 0;
        HALO_HIP(hipMalloc(&ctx->d_degree_rows, bytes));
        ctx->degree_bytes = bytes;
    }
    HALO_HIP(hipMemcpyAsync(ctx->d_degree_rows, rows.data(), bytes, hipMemcpyHostToDevice, ctx->stream));
    constexpr size_t kGridY = 65535;
    for (size_t first = 0; first < m; first += kGridY) {
        const size_t cnt = m - first < kGridY ? m - first : kGridY;
        size_t longest = 0;
        for (size_t i = first; i < first + cnt; ++i) longest = lens[i] > longest ? lens[i] : longest;
        if (longest == 0) continue;  // (zero polynomials only: their `top` stays 0)
        HALO_LAUNCH(ctx, "k_poly_degree_batch", k_poly_degree_batch, dim3((unsigned)((longest + DEG_CHUNK - 1) / DEG_CHUNK), (unsigned)cnt),
                    dim3(DEG_LANES), 0, ctx->d_degree_rows + first);
    }
    HALO_HIP(hipGetLastError());
    HALO_HIP(hipMemcpyAsync(rows.data(), ctx->d_degree_rows, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HALO_HIP(hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < m; ++i) degrees_out[i] = rows[i].top ? rows[i].top - 1 : 0;
    return HALO_OK;
}

int fr_sum_rows(halo_ctx *ctx, uint64_t *d_rows, size_t stride, size_t P, size_t n) {
    if (P <= 1 || n == 0) return HALO_OK;  // (one row is the sum)
    if (P > 65535 || n > ((size_t)1 << 30) || stride < n * 4) { set_error("fr_sum_rows: bad shape"); return HALO_E_ARG; }
    HALO_LAUNCH(ctx, "k_fr_sum_rows", k_fr_sum_rows, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, d_rows, (uint64_t)stride, (uint32_t)P, (uint32_t)n);
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}

int open_batch_fold(halo_ctx *ctx, int G, uint64_t *d_c, uint64_t *d_z, const uint64_t *d_s_in, uint64_t *d_s_out, size_t ms, size_t m, size_t s_len,
                    const uint64_t *d_consts) {
    HALO_LAUNCH(ctx, "k_nofold_s_update_batch", k_nofold_s_update_batch, dim3((unsigned)((2 * s_len + 255) / 256), (unsigned)G), dim3(256), 0, d_s_in,
                d_s_out, (uint64_t)ms, (uint32_t)s_len, d_consts);
    HALO_LAUNCH(ctx, "k_fold_scalars_batch", k_fold_scalars_batch, dim3((unsigned)((m + 255) / 256), (unsigned)G), dim3(256), 0, d_c, d_z, (uint64_t)ms,
                (uint32_t)m, d_consts);
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}

// Measurement hook (halo_bench_fr_kernel): `reps` back-to-back launches of ONE of the bandwidth-side kernels over n elements
// of the context's scratch buffers (any 256-bit patterns are valid operands), nothing else on the stream and no host
// round trip in between -- the steady-state duration a profiler reads off, not the first launch after an idle gap.
// (which = 4 measures a kernel of hpoly.hip)
__global__ __launch_bounds__(256) void k_h_coeffs(const uint64_t *__restrict__ tab, uint32_t n, int E, int accumulate, uint64_t *__restrict__ out);
int bench_fr_kernel(halo_ctx *ctx, int which, size_t n, int reps) {
    if (n == 0 || n > ctx_capacity(ctx) || reps < 1) { set_error("bench_fr_kernel: n must be in [1, context size]"); return HALO_E_ARG; }
    if (which < 0 || which > 6) { set_error("bench_fr_kernel: which must be 0..6"); return HALO_E_ARG; }
    uint64_t *a = ctx->d_tmp_a, *b = ctx->d_tmp_b, *c = ctx->d_tmp_b + 4 * n, *d = ctx->d_tmp_b + 8 * n;  // n x 4 words each (d_tmp_b: 16 n words)
    host::Fr z = host::Fr::from_u64(0x1234567) * host::Fr::from_u64(0x89abcdef), z64;
    uint64_t *d_tab = ctx->d_tmp_c + 8 * 1024 + 64, *partial = ctx->d_tmp_c;
    int nwin = window_count(n);
    int rc = rng_scalars_dev(ctx, 0xF00D, n, b);
    if (!rc) rc = rng_scalars_dev(ctx, 0xBEEF, n, c);
    if (!rc) rc = rng_scalars_dev(ctx, 0xCAFE, n, d);
    if (!rc) rc = upload_window_table(ctx, z, nwin, d_tab, &z64, which == 1 ? plan_poly_eval(n).E : 0);
    if (rc) return rc;
    size_t m = n / 2 ? n / 2 : 1;
    // launch -1 is not profiled: it loads the kernel's code object if this is its first use in the process (k_h_coeffs is the
    // only kernel of its file that the hook runs), so every profiled launch is a steady-state one
    const bool prof_on = ctx->prof.on;
    for (int r = -1; r < reps; ++r) {
        ctx->prof.on = prof_on && r >= 0;
        switch (which) {
            case 0: { const FrPlan p = plan_powers(n); HALO_LAUNCH(ctx, "k_powers", k_powers, dim3(p.blocks), dim3(256), 0, d_tab, nwin, p.E, (uint32_t)n, to_nform(z64), a); break; }
            case 1: {
                const FrPlan p = plan_poly_eval(n);
                HALO_LAUNCH(ctx, "k_poly_eval_partial", k_poly_eval_partial, dim3(p.blocks), dim3(256), 0, b, (uint32_t)n, d_tab, nwin, p.E,
                            d_tab + 4 * (size_t)(16 * (1 + nwin)), partial);
                break;
            }
            case 2: HALO_LAUNCH(ctx, "k_dot2_partial", k_dot2_partial<false>, dim3(plan_dot(n).blocks), dim3(256), 0, b, c, (const uint64_t *)nullptr,
                                (const uint64_t *)nullptr, (uint32_t)n, partial); break;
            case 3: HALO_LAUNCH(ctx, "k_dot2_partial", k_dot2_partial<true>, dim3(plan_dot(m).blocks), dim3(256), 0, b + 4 * m, c, b, c + 4 * m, (uint32_t)m, partial); break;
            case 4: {
                const FrPlan p = plan_h_coeffs(n);
                // (the table region holds the window table: valid field elements, which is all the kernel needs)
                HALO_LAUNCH(ctx, "k_h_coeffs", k_h_coeffs, dim3(p.blocks), dim3(256), 0, ctx->d_tmp_c + 8 * 1024 + 1024, (uint32_t)n, p.E, 0, a);
                break;
            }
            case 5: HALO_LAUNCH(ctx, "k_fold_scalars", k_fold_scalars, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, b, c, (uint32_t)m, to_nform(z), to_nform(z64)); break;
            case 6: HALO_LAUNCH(ctx, "k_axpy", k_axpy, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, b, c, (uint32_t)n, to_nform(z)); break;
        }
    }
    HALO_HIP(hipGetLastError());
    HALO_HIP(hipStreamSynchronize(ctx->stream));
    if (ctx->prof.on) ctx->prof.collect();
    return HALO_OK;
}

}  // namespace halo
