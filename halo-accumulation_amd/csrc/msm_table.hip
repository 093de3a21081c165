// The fixed-base-table pipeline of the MSM (K1/K2 over the context's own key): table plans, the table's build, its recode and
// two-level sort kernels and its launch sequence in pieces.  Behind the sort it shares msm_buckets.hip with the general pipeline.
#include <atomic>
#include <cstring>
#include <thread>

#include "msm_kernels.hpp"
#include "slide_lane.hpp"

namespace halo {

// ------------------------------------------------------------------------------ fixed-base tables (the commitment key is constant)
// The key of a context never changes (consts.rs:68: GS is a compile-time constant of the reference), and a 288 GB device has
// room to spare, so for large MSMs over the context's own bases the context keeps T[w][i] = 2^(c w) G_i for every window w
// (c = 20: 13 windows, 13 x 128 B per point).  A signed digit d of window w then sends the point T[w][i] to bucket |d| of ONE
// set of 2^19 buckets shared by all windows:
//   * 13 n mixed additions instead of 16 n (the general pipeline cannot go past c = 16: every window would need its own
//     2^(c-1) buckets reduced);
//   * the weighted bucket sum is taken once over 2^19 buckets -- as many as 16 windows x 2^15 today -- and the host no longer
//     runs a 240-doubling Horner chain: it combines 24 (plain, weighted) pairs with ~70 additions.
// The sort is the two-level one (coarse: 512 bucket ranges, runs advance sequentially; fine: one block per range, 1024 buckets,
// staged in LDS, which also writes the bucket kernel's task records); the bucket kernel and the combine behind it are the
// general pipeline's, the window sums are taken over the rows and columns of the bucket index (k_msm_reduce_rc, table_rc_shape).
//
// Two plans (TblPlan, fixed when a context builds its table):
//   key of >= 2^20 points: c = 20, 13 windows, 2^19 buckets, 512 coarse ranges of 1024 buckets;
//   key of 2^17 .. 2^19 points (a rank's index shard of a 2^20-point MSM): c = 17, 15 windows (15 x 17 = 255 bits exactly),
//     2^16 buckets, n / 2048 coarse ranges (so that a range's 15 n / ranges entries fit the fine sort's LDS stage) -- 15 n
//     additions against 16 n, an eighth of the buckets of the general plan's 16 x 2^15.
//
// Third plan, the default of a c = 20 key whose ALL-SHIFTS table could be had (255 rows T[j][i] = 2^j G_i, 255 x 128 B per point:
// optional memory like the 13 rows): sliding windows of at most 21 bits that start at set bits only (slide_lane.hpp).  Every digit
// is odd, bucket m holds the digits +-(2 m + 1) -- the same 2^19 buckets --, a digit names its own table row, and a uniform scalar
// has 12.0 digits instead of 13: 12/13 of the sort's entries and of the bucket kernel's additions.  The window widths vary (19 ..
// 21 bits), so low buckets fill more than high ones: the coarse range is the bucket's LOW nine bits and the fine key its high ten
// (every range gets the same mix); the bucket array keeps the index range * 1024 + fine and msm_combine_member weighs rows and
// columns accordingly.  Rows 20 w of that table are the 13-row table: the fixed plan, the tagged launch and the pieces of an MSM
// of more than TBL_PIECE points read it through row_step = 20.
size_t table_slide_min() { return dev_hooks().slide_min > 0 ? (size_t)dev_hooks().slide_min : (size_t)1 << 20; }
TblPlan table_plan(size_t key_n) {
    TblPlan t{};
    t.row_step = 1; t.slide = 0;
    if (key_n >= table_slide_min()) {
        t.c = 20; t.W = 13; t.B = 1u << 19; t.fbits = 10; t.spread = 31; t.fold_top = 0;
    } else {
        t.c = 17; t.W = 15; t.B = 1u << 16; t.spread = 0; t.fold_top = 1;
        uint32_t ranges = 64;
        while ((size_t)ranges * 2048 < key_n && ranges < 256) ranges <<= 1;
        t.fbits = 16;
        for (uint32_t r = ranges; r > 1; r >>= 1) t.fbits--;
    }
    t.ranges = t.B >> t.fbits;
    t.rbits = 0;
    while ((1u << t.rbits) < t.ranges) t.rbits++;
    t.rows = t.W;
    return t;
}
// the default plan of a key whose table holds every shift
static TblPlan table_plan_slide(size_t key_n) {
    TblPlan t = table_plan(key_n);
    t.rows = SLIDE_BITS; t.slide = 21; t.spread = 0; t.row_step = t.c;
    return t;
}
// ... and the fixed windows on the same table
static TblPlan table_plan_fixed_on(const TblPlan &built, size_t key_n) {
    TblPlan t = table_plan(key_n);
    t.rows = built.rows;
    t.row_step = built.rows == SLIDE_BITS ? t.c : 1;
    return t;
}

// next[i] = 2^c * prev[i], affine in, affine out.  A lane takes TBL_E points (i, i + stride, ...) and brings them back to
// affine with one shared inversion (curve.hpp jac_batch_to_aff): the inversion was 70 % of a point's work.
__global__ __launch_bounds__(256) void k_table_step(const uint32_t *__restrict__ prev, uint32_t n, int c, uint32_t *__restrict__ next) {
    uint32_t t = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
    if (t >= n) return;
    JacN p[TBL_E];
    static_for<0, TBL_E>([&](auto ic) {
        constexpr int e = decltype(ic)::value;
        uint32_t i = t + (uint32_t)e * stride;
        p[e] = i < n ? jac_from_aff(aff_load(prev + AFF_STRIDE * (size_t)i)) : jac_inf();
    });
#pragma unroll 1
    for (int k = 0; k < c; k++) static_for<0, TBL_E>([&](auto ic) { p[decltype(ic)::value] = jac_dbl(p[decltype(ic)::value]); });
    AffN a[TBL_E];
    jac_batch_to_aff(p, a);
    static_for<0, TBL_E>([&](auto ic) {
        constexpr int e = decltype(ic)::value;
        uint32_t i = t + (uint32_t)e * stride;
        if (i < n) aff_store(next + AFF_STRIDE * (size_t)i, a[e]);
    });
}

// The all-shifts table: rows 1 .. rows - 1 from row 0, T[j] = 2 T[j - 1], one doubling and a return to affine per row.  A block owns
// ALLS_E x 256 points through all the rows and shares ONE inversion per row among them (k_table_step shares one among 4 points:
// at one doubling per row the inversion would be 97 % of the build).  The Z of the doubled point is 2 y, so a first pass over
// the previous row needs the y's only: every lane multiplies up the Z's of its own points (prefix products, as
// jac_batch_to_aff), the 256 lane products go through LDS -- sixteen lanes take prefix products over sixteen of them each, lane 0
// over the sixteen group products, inverts once and walks back down --, and a second pass doubles each point and unwinds its 1 / Z
// from the inverse of the lane's product.  A lane reads back only what it wrote itself.
constexpr int ALLS_E = 16;  // points per lane
constexpr int ALLS_G = 16;  // lane products per group, groups per block
HALO_DEV Fq<2> lds_get(const uint32_t *p) { Fq<2> r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.v[i] = p[i];
    return r; }
HALO_DEV void lds_put(uint32_t *p, const Fq<2> &a) {
#pragma unroll
    for (int i = 0; i < 9; i++) p[i] = a.v[i]; }
// Z of jac_dbl(jac_from_aff(a)) up to the representation: 2 y (1 for the point at infinity, whose y is 0: the curve has no point of order 2)
HALO_DEV Fq<2> alls_z(const uint32_t *entry) {
    Fq<2> y;
#pragma unroll
    for (int i = 0; i < 9; i++) y.v[i] = entry[10 + i];
    if (fq_limbs_zero(y)) return fq_widen<2>(fq_one());
    return fq_tighten(fq_muls<2>(y));
}
__global__ __launch_bounds__(256) void k_table_all_shifts(uint32_t *__restrict__ tbl, uint32_t n, int rows) {
    __shared__ uint32_t prod[256 * 9], pre[256 * 9], gpre[ALLS_G * 9], inv[256 * 9];
    const uint32_t tid = threadIdx.x, base = blockIdx.x * (256u * ALLS_E);
#pragma unroll 1
    for (int j = 1; j < rows; j++) {
        const uint32_t *prev = tbl + AFF_STRIDE * ((size_t)(j - 1) * n);
        uint32_t *next = tbl + AFF_STRIDE * ((size_t)j * n);
        Fq<2> lp[ALLS_E];  // lp[e] = z_0 ... z_e
        static_for<0, ALLS_E>([&](auto ic) {
            constexpr int e = decltype(ic)::value;
            uint32_t i = base + (uint32_t)e * 256u + tid;
            Fq<2> z = i < n ? alls_z(prev + AFF_STRIDE * (size_t)i) : fq_widen<2>(fq_one());
            if constexpr (e == 0) lp[0] = z;
            else lp[e] = fq_mul(lp[e - 1], z);
        });
        lds_put(prod + 9 * tid, lp[ALLS_E - 1]);
        __syncthreads();
        if (tid < ALLS_G) {  // prefix products inside group tid
            Fq<2> run = lds_get(prod + 9 * (tid * ALLS_G));
            lds_put(pre + 9 * (tid * ALLS_G), run);
#pragma unroll 1
            for (int k = 1; k < ALLS_G; k++) {
                run = fq_mul(run, lds_get(prod + 9 * (tid * ALLS_G + k)));
                lds_put(pre + 9 * (tid * ALLS_G + k), run);
            }
        }
        __syncthreads();
        if (tid == 0) {  // over the groups' products; gpre[g] ends as the inverse of group g's product
            Fq<2> run = lds_get(pre + 9 * (ALLS_G - 1));
            lds_put(gpre, run);
#pragma unroll 1
            for (int g = 1; g < ALLS_G; g++) {
                run = fq_mul(run, lds_get(pre + 9 * (g * ALLS_G + ALLS_G - 1)));
                lds_put(gpre + 9 * g, run);
            }
            Fq<2> iv = fq_inv(run);
#pragma unroll 1
            for (int g = ALLS_G - 1; g >= 1; g--) {
                Fq<2> gi = fq_mul(iv, lds_get(gpre + 9 * (g - 1)));
                iv = fq_mul(iv, lds_get(pre + 9 * (g * ALLS_G + ALLS_G - 1)));
                lds_put(gpre + 9 * g, gi);
            }
            lds_put(gpre, iv);
        }
        __syncthreads();
        if (tid < ALLS_G) {  // inverses of the lane products of group tid
            Fq<2> iv = lds_get(gpre + 9 * tid);
#pragma unroll 1
            for (int k = ALLS_G - 1; k >= 1; k--) {
                lds_put(inv + 9 * (tid * ALLS_G + k), fq_mul(iv, lds_get(pre + 9 * (tid * ALLS_G + k - 1))));
                iv = fq_mul(iv, lds_get(prod + 9 * (tid * ALLS_G + k)));
            }
            lds_put(inv + 9 * (tid * ALLS_G), iv);
        }
        __syncthreads();
        Fq<2> iv = lds_get(inv + 9 * tid);
        static_for_down<ALLS_E - 1>([&](auto ic) {
            constexpr int e = decltype(ic)::value;
            uint32_t i = base + (uint32_t)e * 256u + tid;
            if (i < n) {  // (a point past the end entered the product as 1)
                JacN p = jac_dbl(jac_from_aff(aff_load(prev + AFF_STRIDE * (size_t)i)));
                Fq<2> z = jac_is_inf(p) ? fq_widen<2>(fq_one()) : fq_tighten(p.z);
                Fq<2> zi = iv;
                if constexpr (e > 0) { zi = fq_mul(iv, lp[e - 1]); iv = fq_mul(iv, z); }
                Fq<2> zi2 = fq_sqr(zi);
                AffN a;
                a.x = fq_mul(p.x, zi2);
                a.y = fq_mul(p.y, fq_mul(zi2, zi));
                if (jac_is_inf(p)) a = aff_inf();
                aff_store(next + AFF_STRIDE * (size_t)i, a);
            }
        });
        // (the next row's first barrier orders this row's reads of `inv` before its writes)
    }
}

// signed 20-bit digits, u32 [w][i]: (|d| - 1) | sign << 31, TDIGIT_NONE for zero; block 0 clears the launch's small state
// blockIdx.y = member of a batched launch (small-key plan): its digits go to rows [member W, (member + 1) W) and carry
// member * B on top of the bucket number, so that every later kernel sees one MSM with count * B buckets.
// tagged (MsmBatch::tagged): ONE scalar array, canonical, whose bit 255 picks the bucket set of point i (0 / 1) the way blockIdx.y
// does for the members of a batch: rows stay W, buckets become 2 B.
__global__ __launch_bounds__(256) void k_tmsm_recode(TblScalars members, int mont, int tagged, uint32_t n, TblPlan tp, uint32_t *__restrict__ digits,
                                                     uint32_t *__restrict__ meta, uint32_t *__restrict__ zero_b, uint32_t *__restrict__ zero_t) {
    __shared__ uint32_t sw[256 * 9];
    __shared__ uint8_t wtab[256];  // sliding plan: window width by bits left (slide_lane.hpp)
    if (tp.slide) {
        wtab[threadIdx.x] = (uint8_t)slide_width(threadIdx.x ? (int)threadIdx.x : 1, tp.slide);
        __syncthreads();
    }
    const uint64_t *__restrict__ scalars = members.p[blockIdx.y];
    if (blockIdx.x == 0 && blockIdx.y == 0) {
        meta[threadIdx.x] = 0;
        for (int k = 0; k < 4; k++) { zero_b[threadIdx.x + 256 * k] = 0; zero_t[threadIdx.x + 256 * k] = 0; }
    }
    uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    Fe s = fe_load(scalars + 4 * (size_t)i);
    if (mont) s = fe_from_mont<FrCfg>(s);
    uint32_t *my = sw + threadIdx.x * 9;
#pragma unroll
    for (int k = 0; k < 8; k++) my[k] = s.v[k];
    my[8] = 0;
    if (tp.slide) {
        // sliding odd digits (slide_lane.hpp; one member, one bucket set): slot k holds bucket (|d| - 1) / 2 | row << 19 | sign << 31,
        // the slots behind the last digit TDIGIT_NONE (row <= 254: no live slot reads as TDIGIT_NONE)
        if (!mont) slide_canon(my);  // (out of Montgomery form a scalar is canonical already)
        int cnt = slide_recode(my, tp.slide, wtab, [&](int k, uint32_t mag, uint32_t neg, uint32_t row) {
            if (k < SLIDE_SLOTS) digits[(size_t)k * n + i] = ((mag - 1u) >> 1) | (row << TBL_ROW_SHIFT) | (neg << 31);
        });
        for (int k = cnt; k < SLIDE_SLOTS; k++) digits[(size_t)k * n + i] = TDIGIT_NONE;
        return;
    }
    uint32_t set = blockIdx.y;
    if (tagged) { set = my[7] >> 31; my[7] &= 0x7fffffffu; }
    uint32_t flip = 0;
    if (tp.fold_top && (my[7] >> 30) != 0) {
        // c = 17: the top window would hold 2^16 (+ carry) = B + 1 for a scalar >= 2^254 -- one value too many.  Such a
        // scalar is within 2^126 of r: take r - s with every digit's sign flipped (or s - r for an unreduced input).
        bool ge = true;  // s >= r ?
#pragma unroll
        for (int j = 7; j >= 0; j--) {
            if (my[j] != FrCfg::P[j]) { ge = my[j] > FrCfg::P[j]; break; }
        }
        uint64_t borrow = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            uint64_t a = ge ? my[j] : FrCfg::P[j], b = ge ? FrCfg::P[j] : my[j];
            uint64_t d = a - b - borrow;
            my[j] = (uint32_t)d;
            borrow = (d >> 32) & 1u;
        }
        flip = ge ? 0u : 1u;
    }
    if (tp.spread) {
        // The top window holds 255 - 240 = 15 scalar bits: its 2^20 digits would all land in the lowest 16 of the 512
        // coarse ranges (3.7 x the entries of the others: their fine-sort blocks ran 110-160 us against 15 us, and the
        // kernel waited for them).  Every base has order r, so s + k r gives the same point for any k: k = i mod 31
        // spreads the top digit floor((s + k r) / 2^240) evenly over [0, 31 * 2^14] <= 2^19 at no cost.  Scalars with an
        // empty top window (zero, short challenges) add nothing to it and stay as they are; so does anything >= 2^254 + 2^240.
        // (plan c = 20 only: tp.spread = 31)
        uint32_t top = my[7] >> 16;
        uint32_t k = (top != 0 && top <= 16384u) ? i % tp.spread : 0u;
        uint64_t acc = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            acc += (uint64_t)k * FrCfg::P[j] + my[j];
            my[j] = (uint32_t)acc;
            acc >>= 32;
        }
        my[8] = (uint32_t)acc;
    }
    uint32_t carry = 0;
    for (int w = 0; w < tp.W; w++) {
        Digit d = next_digit(my, w, tp.c, tp.B, carry);
        digits[((size_t)blockIdx.y * tp.W + w) * n + i] = d.mag ? ((d.mag - 1 + set * tp.B) | ((d.neg ^ flip) << 31)) : TDIGIT_NONE;
    }
}
// coarse range and fine key of a digit word (B = buckets of the whole launch, a power of two): the high and the low bits of the
// bucket -- or, under the sliding plan, the low and the high ones
HALO_DEV uint32_t tbl_range(uint32_t v, const TblPlan &tp) { return tp.slide ? v & (tp.ranges - 1u) : (v & (tp.B - 1u)) >> tp.fbits; }
HALO_DEV uint32_t tbl_fine(uint32_t v, const TblPlan &tp) { return tp.slide ? (v & (tp.B - 1u)) >> tp.rbits : v & ((1u << tp.fbits) - 1u); }
// block (w, chunk): counts of the 512 coarse ranges, one private row per wave
// (MAXR = 1024: the c = 20 plan with TWO bucket sets, a `tagged` launch -- the kernels with a 2 in their names)
template <uint32_t MAXR>
HALO_DEV void tmsm_coarse_hist_body(const uint32_t *__restrict__ digits, uint32_t n, uint32_t nchunks, uint32_t chunk_len, const TblPlan &tp,
                                    uint32_t *__restrict__ chist) {
    __shared__ uint32_t cnt[16 * MAXR];
    uint32_t w = blockIdx.x / nchunks, chunk = blockIdx.x % nchunks;
    for (uint32_t k = threadIdx.x; k < 16 * MAXR; k += 1024) cnt[k] = 0;
    __syncthreads();
    uint32_t *mine = cnt + MAXR * (threadIdx.x >> 6);
    uint32_t lo = chunk * chunk_len, hi = lo + chunk_len < n ? lo + chunk_len : n;
    const uint32_t *dg = digits + (size_t)w * n;
    for (uint32_t i = lo + 4 * threadIdx.x; i < hi; i += 4 * 1024) {  // n and chunk_len are multiples of 4
        uint4 q = *reinterpret_cast<const uint4 *>(dg + i);
        uint32_t v[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (v[k] != TDIGIT_NONE) atomicAdd(&mine[tbl_range(v[k], tp)], 1u);
    }
    __syncthreads();
    if (threadIdx.x < tp.ranges) {
        uint32_t t = 0;
        for (int r = 0; r < 16; r++) t += cnt[MAXR * r + threadIdx.x];
        chist[(size_t)blockIdx.x * tp.ranges + threadIdx.x] = t;
    }
}
__global__ __launch_bounds__(1024) void k_tmsm_coarse_hist(const uint32_t *__restrict__ digits, uint32_t n, uint32_t nchunks, uint32_t chunk_len,
                                                           TblPlan tp, uint32_t *__restrict__ chist) {
    tmsm_coarse_hist_body<TBL_MAX_RANGES>(digits, n, nchunks, chunk_len, tp, chist);
}
__global__ __launch_bounds__(1024) void k_tmsm_coarse_hist2(const uint32_t *__restrict__ digits, uint32_t n, uint32_t nchunks, uint32_t chunk_len,
                                                            TblPlan tp, uint32_t *__restrict__ chist) {
    tmsm_coarse_hist_body<2 * TBL_MAX_RANGES>(digits, n, nchunks, chunk_len, tp, chist);
}
// chist[chunk][range] -> exclusive prefix over the chunks of each range (in place); rtotal[range] = the range's size.
// One block per range: 247 counters, loaded once, scanned in LDS.
__global__ __launch_bounds__(256) void k_tmsm_scan_chunks(uint32_t *__restrict__ chist, uint32_t nchunks_all, uint32_t ranges, uint32_t *__restrict__ rtotal) {
    __shared__ uint32_t part[256];
    uint32_t r = blockIdx.x, t = threadIdx.x;
    uint32_t v = t < nchunks_all ? chist[(size_t)t * ranges + r] : 0u;  // nchunks_all <= 256
    part[t] = v;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        uint32_t o = t >= (uint32_t)off ? part[t - off] : 0u;
        __syncthreads();
        part[t] += o;
        __syncthreads();
    }
    if (t < nchunks_all) chist[(size_t)t * ranges + r] = part[t] - v;
    if (t == 255) rtotal[r] = part[255];
}
// cstart[r] = start of run r in the presorted array, cstart[512] = number of entries
__global__ __launch_bounds__(1024) void k_tmsm_scan_ranges(const uint32_t *__restrict__ rtotal, uint32_t *__restrict__ cstart) {
    __shared__ uint32_t part[2 * TBL_MAX_RANGES];
    const uint32_t ranges = blockDim.x;  // one thread per range
    uint32_t t = threadIdx.x, v = rtotal[t];
    part[t] = v;
    __syncthreads();
    for (uint32_t off = 1; off < ranges; off <<= 1) {
        uint32_t o = t >= off ? part[t - off] : 0u;
        __syncthreads();
        part[t] += o;
        __syncthreads();
    }
    cstart[t] = part[t] - v;
    if (t == ranges - 1) cstart[ranges] = part[t];
}
// Block (w, chunk) appends its entries to the 512 runs: table index | sign << 31, and the bucket's low 10 bits beside it.
// 247 blocks x 512 runs are too many open cache lines for direct appends (partially filled lines would be evicted and
// rewritten), so the block goes through its chunk in tiles of 8192 entries: a tile is grouped by range in LDS (local
// ranks from an LDS histogram), then written out in that order -- entries of one range land on consecutive addresses.
constexpr uint32_t TBL_TILE = 8192;
template <uint32_t MAXR>
HALO_DEV void tmsm_coarse_scatter_body(const uint32_t *__restrict__ digits, uint32_t n, uint32_t nchunks, uint32_t chunk_len,
                                       const uint32_t *__restrict__ chist, const uint32_t *__restrict__ cstart, uint32_t table_n, uint32_t base_off,
                                       const TblPlan &tp, uint32_t *__restrict__ presort, uint16_t *__restrict__ presort_fine) {
    __shared__ uint32_t cur[MAXR], tcount[MAXR], toff[MAXR], wsum[MAXR / 64];
    const uint32_t ranges = tp.ranges;
    __shared__ uint32_t t_idx[TBL_TILE], t_dest[TBL_TILE];
    __shared__ uint16_t t_fine[TBL_TILE];
    uint32_t row = blockIdx.x / nchunks, chunk = blockIdx.x % nchunks, tid = threadIdx.x;  // row = member * W + w
    if (tid < ranges) cur[tid] = cstart[tid] + chist[(size_t)blockIdx.x * ranges + tid];
    uint32_t lo = chunk * chunk_len, hi = lo + chunk_len < n ? lo + chunk_len : n;
    const uint32_t *dg = digits + (size_t)row * n;
    // the table row of the entries: the window's (fixed plans), or the one each digit names (sliding plan: < 2^28 with the index)
    const uint32_t tbase = (row % (uint32_t)tp.W) * (uint32_t)tp.row_step * table_n + base_off;
    for (uint32_t t0 = lo; t0 < hi; t0 += TBL_TILE) {
        if (tid < ranges) tcount[tid] = 0;
        __syncthreads();
        // eight digits per thread: two 16-byte loads (n, chunk_len and the tile are multiples of 4)
        uint32_t v[8], rank[8];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            uint32_t i = t0 + 4 * tid + (uint32_t)h * 4096;
            uint4 q = i < hi ? *reinterpret_cast<const uint4 *>(dg + i) : make_uint4(TDIGIT_NONE, TDIGIT_NONE, TDIGIT_NONE, TDIGIT_NONE);
            v[4 * h] = q.x; v[4 * h + 1] = q.y; v[4 * h + 2] = q.z; v[4 * h + 3] = q.w;
        }
#pragma unroll
        for (int k = 0; k < 8; k++) rank[k] = v[k] != TDIGIT_NONE ? atomicAdd(&tcount[tbl_range(v[k], tp)], 1u) : 0u;
        __syncthreads();
        {   // inclusive scan of the tile's counts: shuffles within a wave, the <= 8 wave totals through LDS -- two barriers
            // (a Hillis-Steele pass over LDS took 18, per tile, for sixteen waves)
            uint32_t x = tid < ranges ? tcount[tid] : 0u;
            uint32_t lane = tid & 63u;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                uint32_t o = (uint32_t)__shfl_up((int)x, off, 64);
                if (lane >= (uint32_t)off) x += o;
            }
            if (lane == 63 && tid < MAXR) wsum[tid >> 6] = x;
            __syncthreads();
            uint32_t before = 0;
#pragma unroll
            for (uint32_t wv = 0; wv < MAXR / 64; wv++) before += (wv < (tid >> 6)) ? wsum[wv] : 0u;
            if (tid < ranges) toff[tid] = x + before;
            __syncthreads();
        }
        uint32_t total = toff[ranges - 1];
#pragma unroll
        for (int k = 0; k < 8; k++)
            if (v[k] != TDIGIT_NONE) {
                uint32_t r = tbl_range(v[k], tp);
                uint32_t slot = toff[r] - tcount[r] + rank[k];
                uint32_t i = t0 + 4 * tid + (uint32_t)(k >> 2) * 4096 + (uint32_t)(k & 3);
                uint32_t at = tp.slide ? ((v[k] >> TBL_ROW_SHIFT) & 0xffu) * table_n + base_off : tbase;
                t_idx[slot] = (at + i) | (v[k] & 0x80000000u);
                t_fine[slot] = (uint16_t)tbl_fine(v[k], tp);
                t_dest[slot] = cur[r] + rank[k];
            }
        __syncthreads();
        for (uint32_t j = tid; j < total; j += 1024) {
            uint32_t d = t_dest[j];
            presort[d] = t_idx[j];
            presort_fine[d] = t_fine[j];
        }
        __syncthreads();
        if (tid < ranges) cur[tid] += tcount[tid];
    }
}
__global__ __launch_bounds__(1024) void k_tmsm_coarse_scatter(const uint32_t *__restrict__ digits, uint32_t n, uint32_t nchunks, uint32_t chunk_len,
                                                              const uint32_t *__restrict__ chist, const uint32_t *__restrict__ cstart,
                                                              uint32_t table_n, uint32_t base_off, TblPlan tp, uint32_t *__restrict__ presort,
                                                              uint16_t *__restrict__ presort_fine) {
    tmsm_coarse_scatter_body<TBL_MAX_RANGES>(digits, n, nchunks, chunk_len, chist, cstart, table_n, base_off, tp, presort, presort_fine);
}
__global__ __launch_bounds__(1024) void k_tmsm_coarse_scatter2(const uint32_t *__restrict__ digits, uint32_t n, uint32_t nchunks, uint32_t chunk_len,
                                                               const uint32_t *__restrict__ chist, const uint32_t *__restrict__ cstart,
                                                               uint32_t table_n, uint32_t base_off, TblPlan tp, uint32_t *__restrict__ presort,
                                                               uint16_t *__restrict__ presort_fine) {
    tmsm_coarse_scatter_body<2 * TBL_MAX_RANGES>(digits, n, nchunks, chunk_len, chist, cstart, table_n, base_off, tp, presort, presort_fine);
}
// Fine sort of run r: counts and absolute starts of its 1024 buckets, entries placed in [lo, hi) of `sorted` -- and the
// task lists the general pipeline builds with four more kernels (k_scan_blocks/_top, k_msm_task_bins, k_msm_task_order):
// a bucket of c entries is ceil(c / kmax) tasks with consecutive ids; the block reserves its ids with one atomic
// (meta[0]) and writes toff[g] = first id (absolute: the block offsets of the two-level scan format stay zero).
// Multi-task buckets are listed for k_msm_combine (meta[1], meta[140]).
//
// The block also writes the bucket kernel's records (`order`, the format of k_msm_task_order) for its own buckets, into a
// STATIC layout that needs no global length histogram -- and so no launch between the sort and the bucket kernel:
//   * every bucket has one slot in [obase, obase + ranges * 2^fbits): its LAST task (the only one, for uniform scalars), or a
//     record of length 0 for an empty bucket.  Inside the block a bucket gets rank rho by decreasing length of that task (a
//     counting sort over the 65 lengths, lbin); the slot is rank-major over the whole launch: ranks [8 q, 8 q + 8) of every
//     range come before ranks [8 q + 8, ..) of any range, and a wave of the bucket kernel holds TBL_ORDER_RUN = 8 consecutive
//     ranks of 64 / 8 = 8 neighbouring ranges (tmsm_order_slot).  Ranges are statistically alike, so the lanes of a wave run
//     chains of near-equal length and the longest waves of all ranges are dispatched first (a per-block order, each range's
//     tasks contiguous, had the long waves last: +35 % on k_msm_accumulate);
//   * the tasks in front of a bucket's last (buckets of more than kmax entries: skewed scalars, a short forced task length) are
//     all of the full length kmax and go to the overflow region [0, obase), reserved per block with one atomic on
//     meta[META_OVF]: they run first.
// The records carry a task's first entry, so they are written after the placement.
HALO_DEV uint32_t tmsm_order_slot(uint32_t rho, uint32_t r, uint32_t ranges) {
    constexpr uint32_t G = 64u / TBL_ORDER_RUN;  // ranges side by side in a wave
    return ((rho / TBL_ORDER_RUN) * (ranges / G) + r / G) * 64u + (r % G) * TBL_ORDER_RUN + rho % TBL_ORDER_RUN;
}
__global__ __launch_bounds__(1024) void k_tmsm_fine_sort(const uint32_t *__restrict__ presort, const uint16_t *__restrict__ presort_fine,
                                                         const uint32_t *__restrict__ cstart, uint32_t kmax, TblPlan tp, uint32_t *__restrict__ counts,
                                                         uint32_t *__restrict__ starts, uint32_t *__restrict__ ntask, uint32_t *__restrict__ toff,
                                                         uint32_t *__restrict__ biglist, uint32_t *__restrict__ meta, uint32_t *sorted,
                                                         uint32_t obase, uint4 *__restrict__ order) {
    // lbin: [0, 65) buckets per length of the last task (64 - length), then the counters of the block's lists (LB_*)
    constexpr uint32_t LB_BIG = KMAX + 1, LB_SMALL = KMAX + 2, LB_BIG0 = KMAX + 3, LB_SMALL0 = KMAX + 4, LB_OVF0 = KMAX + 5;
    __shared__ uint32_t hist[1024], scan[1024], tscan[1024], lbin[KMAX + 8], lbase[KMAX + 1], wlive[16], misc[2];
    uint32_t r = blockIdx.x, lo = cstart[r], hi = cstart[r + 1], tid = threadIdx.x;
#ifdef TMSM_TIMING
    uint64_t tm[10]; int tmi = 0;
#define TMARK() do { __syncthreads(); tm[tmi++] = wall_clock64(); } while (0)
#else
#define TMARK() do {} while (0)
#endif
    TMARK();
    hist[tid] = 0;
    if (tid < KMAX + 8) lbin[tid] = 0;
    // A run that fits the LDS stage (every run, for uniform scalars) is read ONCE, all loads in flight together, and kept
    // in registers across the counting and the placement: the kernel is bound by global-load latency (one block of 16
    // waves per CU), not by LDS or bandwidth.
    constexpr int PER = TBL_STAGE / 1024;
    bool staged = hi - lo <= TBL_STAGE;
    uint32_t rv[PER], rf[PER];
    if (staged) {
#pragma unroll
        for (int k = 0; k < PER; k++) {
            uint32_t e = lo + tid + (uint32_t)k * 1024;
            bool in = e < hi;
            rv[k] = in ? presort[e] : 0u;
            rf[k] = in ? (uint32_t)presort_fine[e] : 0xffffffffu;
        }
    }
    __syncthreads();
    TMARK();
    if (staged) {
#pragma unroll
        for (int k = 0; k < PER; k++)
            if (rf[k] != 0xffffffffu) atomicAdd(&hist[rf[k]], 1u);
    } else {
        for (uint32_t e = lo + tid; e < hi; e += 4 * 1024) {
            uint32_t f[4];
#pragma unroll
            for (int k = 0; k < 4; k++) f[k] = e + k * 1024 < hi ? presort_fine[e + k * 1024] : 0u;
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (e + k * 1024 < hi) atomicAdd(&hist[f[k]], 1u);
        }
    }
    __syncthreads();
    TMARK();
    const uint32_t nb = 1u << tp.fbits;
    bool owner = tid < nb;  // one bucket per thread
    uint32_t mine = owner ? hist[tid] : 0u, nt = (mine + kmax - 1) / kmax;
    scan[tid] = mine;
    tscan[tid] = nt;
    // the bucket's last task: its length, and the bucket's rank among the block's buckets of that length
    const uint32_t llen = nt ? mine - (nt - 1) * kmax : 0u;
    uint32_t rho = owner ? atomicAdd(&lbin[KMAX - llen], 1u) : 0u;
    // non-empty buckets in front of this one (ballots, wave totals through LDS): with the task scan, the tasks in front that
    // go to the overflow region
    uint32_t live_before;
    {
        unsigned long long bal = __ballot(nt != 0);
        uint32_t lane = tid & 63u;
        live_before = (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wlive[tid >> 6] = (uint32_t)__popcll(bal);
    }
    __syncthreads();
    for (uint32_t o = 1; o < 1024; o <<= 1) {
        uint32_t a = tid >= o ? scan[tid - o] : 0u, b = tid >= o ? tscan[tid - o] : 0u;
        __syncthreads();
        scan[tid] += a;
        tscan[tid] += b;
        __syncthreads();
    }
    TMARK();
    for (uint32_t wv = 0; wv < (tid >> 6); wv++) live_before += wlive[wv];
    if (tid == 1023) {
        misc[0] = atomicAdd(&meta[0], tscan[1023]);  // this block's task ids: [base, base + total)
        misc[1] = tscan[1023] - (live_before + (nt != 0));  // its overflow tasks
        lbin[LB_OVF0] = misc[1] ? atomicAdd(&meta[META_OVF], misc[1]) : 0u;
    }
    if (tid <= KMAX) {
        uint32_t start = 0;  // buckets with a longer last task
        for (uint32_t k = 0; k < tid; k++) start += lbin[k];
        lbase[tid] = start;
    }
    __syncthreads();
    TMARK();
    const uint32_t begin = lo + scan[tid] - mine, tfirst = misc[0] + tscan[tid] - nt, ofirst = tscan[tid] - nt - live_before;
    rho += lbase[KMAX - llen];
    __syncthreads();
    if (owner) {
        uint32_t g = (r << tp.fbits) + tid;
        counts[g] = mine;
        ntask[g] = nt;
        starts[g] = begin;  // absolute: the block offsets of the two-level scan format are zeroed by the recode kernel
        toff[g] = tfirst;   // likewise
        hist[tid] = begin;
    }
    // for the overflow records, written by the whole block after the placement: first overflow task and first task id per bucket
    scan[tid] = owner ? ofirst : 0xffffffffu;
    tscan[tid] = tfirst;
    // multi-task buckets for k_msm_combine: counted in LDS, one reservation per block and list (a global atomic per bucket
    // serialises on one address: 1 ms when a third of the buckets hold more than kmax entries)
    TMARK();
    uint32_t big_rank = 0, small_rank = 0;
    if (owner && nt > 8) big_rank = atomicAdd(&lbin[LB_BIG], 1u);
    else if (owner && nt > 1) small_rank = atomicAdd(&lbin[LB_SMALL], 1u);
    __syncthreads();
    if (tid == 0) {
        lbin[LB_BIG0] = lbin[LB_BIG] ? atomicAdd(&meta[1], lbin[LB_BIG]) : 0u;
        lbin[LB_SMALL0] = lbin[LB_SMALL] ? atomicAdd(&meta[140], lbin[LB_SMALL]) : 0u;
    }
    __syncthreads();
    if (owner && nt > 8) biglist[lbin[LB_BIG0] + big_rank] = (r << tp.fbits) + tid;
    else if (owner && nt > 1) biglist[tp.B - 1 - (lbin[LB_SMALL0] + small_rank)] = (r << tp.fbits) + tid;
    extern __shared__ uint32_t stage[];  // TBL_STAGE entries
    TMARK();
    if (staged) {
#pragma unroll
        for (int k = 0; k < PER; k++)
            if (rf[k] != 0xffffffffu) stage[atomicAdd(&hist[rf[k]], 1u) - lo] = rv[k];
        __syncthreads();
        TMARK();
        for (uint32_t e = lo + tid; e < hi; e += 1024) sorted[e] = stage[e - lo];
    } else {
        for (uint32_t e = lo + tid; e < hi; e += 4 * 1024) {  // an oversized run (skewed scalars): placed directly
            uint32_t v[4], f[4], pos[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                bool in = e + k * 1024 < hi;
                v[k] = in ? presort[e + k * 1024] : 0u;
                f[k] = in ? presort_fine[e + k * 1024] : 0u;
            }
#pragma unroll
            for (int k = 0; k < 4; k++) pos[k] = e + k * 1024 < hi ? atomicAdd(&hist[f[k]], 1u) : 0u;
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (e + k * 1024 < hi) sorted[pos[k]] = v[k];
        }
        __threadfence();  // the records below read entries that other threads of the block have just placed
        __syncthreads();
    }
    // a placed entry: from the stage, or from `sorted` past this CU's vector cache
    auto entry = [&](uint32_t e) -> uint32_t { return staged ? stage[e - lo] : __hip_atomic_load(&sorted[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    // the bucket's slot in the static region: its last task, or an empty record
    if (owner) {
        uint4 rec = make_uint4(0u, 0u, 0u, 0u);
        if (nt) {
            uint32_t st = begin + (nt - 1) * kmax;
            rec = make_uint4(tfirst + nt - 1, st, llen, entry(st));
        }
        order[obase + tmsm_order_slot(rho, r, gridDim.x)] = rec;
    }
    // the overflow region: task i of the block's overflow tasks belongs to the last bucket b with scan[b] <= i (hist[b] is
    // the end of bucket b's entries by now: the start of bucket b + 1)
    const uint32_t novf = misc[1], ovf0 = lbin[LB_OVF0];
    for (uint32_t i = tid; i < novf; i += 1024) {
        uint32_t b0 = 0, b1 = nb - 1;
        while (b0 < b1) {
            uint32_t mid = (b0 + b1 + 1) >> 1;
            if (scan[mid] <= i) b0 = mid; else b1 = mid - 1;
        }
        uint32_t j = i - scan[b0], st = (b0 ? hist[b0 - 1] : lo) + j * kmax;
        order[ovf0 + i] = make_uint4(tscan[b0] + j, st, kmax, entry(st));
    }
#ifdef TMSM_TIMING
    TMARK();
    if (tid == 0 && (blockIdx.x % 100 == 0 || tm[tmi - 1] - tm[0] > 3000))
        printf("fine block %u (%u entries, %s): total %llu (x10 ns)\n", blockIdx.x, hi - lo, staged ? "staged" : "UNSTAGED", (unsigned long long)(tm[tmi - 1] - tm[0]));
#endif
}

int msm_table_prepare() {
    HALO_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k_tmsm_fine_sort), hipFuncAttributeMaxDynamicSharedMemorySize, TBL_STAGE * 4));
    return HALO_OK;
}

static int tmsm_enqueue_piece(halo_ctx *ctx, MsmWorkspace &ws, const TblPlan &plan, const uint32_t *d_bases, const MsmBatch &members, size_t soff, bool mont,
                              size_t n, int piece, uint64_t *h_dst);
// The table over the whole key, built on the context's first table MSM (one-off).  A c = 20 key of one device asks for the
// all-shifts table first (255 rows, k_table_all_shifts: 34 GB at n = 2^20) unless table mode 1 forces the fixed windows; if the
// optional-memory budget or the allocation refuses that, it builds T[w][i] = 2^(c w) G_i window by window like every other key
// (W - 1 passes of c doublings and an inversion per point, ~10 ms at n = 2^20) and runs the fixed plan -- never an error.
int table_build(halo_ctx *ctx) {
    if (ctx->d_table) return HALO_OK;
    // a table that could not be had is tried again after table_backoff more eligible MSMs (64, 128, ... 4096), not never:
    // the memory may have come back, the budget may have been raised
    {   // a clone of this context (halo_ctx_clone) may have built the table already, or be building it right now
        std::lock_guard<std::mutex> lk(ctx->share->mu);
        if (ctx->share->d_table) {
            alloc_epoch_bump(ctx);
            ctx->tbl = ctx->share->tbl;
            ctx->d_table = ctx->share->d_table;
            ctx->table_status = 2;
            return HALO_OK;
        }
        if (ctx->share->table_busy) return HALO_OK;  // (this MSM takes the table-free pipeline; the next one looks again)
        if (ctx->table_calls + 1 < ctx->table_retry_at) { ++ctx->table_calls; return HALO_OK; }
        ctx->share->table_busy = true;
    }
    struct Busy { KeyShare *k; ~Busy() { std::lock_guard<std::mutex> lk(k->mu); k->table_busy = false; } } busy{ctx->share.get()};
    ++ctx->table_calls;
    const size_t n = ctx->n;
    const TblPlan fixed = table_plan(n);
    // (entry references are row * n + index: below 2^28 for the all-shifts table, which leaves the digit word's row field its 8 bits)
    bool key_fixed_only, key_shared;
    { std::lock_guard<std::mutex> lk(ctx->share->mu); key_fixed_only = ctx->share->table_fixed_only; key_shared = ctx->share->users > 1; }
    const bool all_shifts = fixed.c == 20 && ctx->table_mode != 1 && !key_fixed_only && !ctx->parent && ctx->shards.empty() && (size_t)SLIDE_BITS * n <= ((size_t)1 << 28);
    // (a caller that has asked for the fold table and not got it yet keeps the room for it, and so does a key with clones, from
    // whom the table could not be taken back: internal.hpp table_demote)
    const bool fold_first = fold_table_wanted(ctx) && (ctx->fold_table_mode == 1 || key_shared);
    const TblPlan plans[2] = {table_plan_slide(n), fixed};
    int status = 0;
    size_t bytes = 0;
    std::string why;
    for (int k = all_shifts ? 0 : 1; k < 2; ++k) {
        const TblPlan &tp = plans[k];
        bytes = (size_t)tp.rows * n * 128;
        if (k == 0 && fold_first && !table_budget_room(ctx, bytes + foldtab_need_bytes(n))) continue;
        if (!table_budget_reserve(ctx, bytes)) { status = 3; why = "over the budget for optional memory, halo_set_memory_budget"; continue; }
        alloc_epoch_bump(ctx);
        // built into a local pointer and published (d_table + tbl together) only after the last step has succeeded: a
        // half-built table is never visible to table_eligible / tmsm_enqueue_piece
        uint32_t *tbl = nullptr;
        hipError_t e = dev_hooks().table_fail ? hipErrorOutOfMemory : hipMalloc(&tbl, bytes);  // (development library's hook: the failure path)
        if (e == hipSuccess) {
            if (debug_trace()) fprintf(stderr, "[halo] table ctx=%p c=%d rows=%d [%p, +%zu)\n", (void *)ctx, tp.c, tp.rows, (void *)tbl, bytes);
            const auto t0 = std::chrono::steady_clock::now();
            e = hipMemcpyAsync(tbl, ctx->d_bases, n * 128, hipMemcpyDeviceToDevice, ctx->stream);
            if (tp.rows == SLIDE_BITS && e == hipSuccess) {
                HALO_LAUNCH(ctx, "k_table_all_shifts", k_table_all_shifts, dim3((unsigned)((n + 256 * ALLS_E - 1) / (256 * ALLS_E))), dim3(256), 0, tbl, (uint32_t)n, tp.rows);
                e = hipGetLastError();
            }
            for (int w = 1; tp.rows != SLIDE_BITS && w < tp.W && e == hipSuccess; ++w) {
                HALO_LAUNCH(ctx, "k_table_step", k_table_step, dim3((unsigned)(((n + TBL_E - 1) / TBL_E + 255) / 256)), dim3(256), 0,
                            tbl + (size_t)(w - 1) * n * AFF_STRIDE, (uint32_t)n, tp.c, tbl + (size_t)w * n * AFF_STRIDE);
                e = hipGetLastError();
            }
            hipError_t e2 = hipStreamSynchronize(ctx->stream);
            if (e == hipSuccess) e = e2;
            if (e == hipSuccess) ctx->share->table_build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        }
        if (e != hipSuccess) {
            // No table, no problem: the general pipeline needs no table memory and gives the same point.
            (void)hipGetLastError();
            if (tbl) (void)hipFree(tbl);
            table_budget_release(ctx, bytes);
            status = 4; why = hipGetErrorString(e);
            continue;
        }
        {
            std::lock_guard<std::mutex> lk(ctx->share->mu);
            ctx->share->tbl = tp;
            ctx->share->d_table = tbl;
        }
        ctx->tbl = tp;
        ctx->d_table = tbl;
        ctx->table_status = 2;
        return HALO_OK;
    }
    ctx->table_status = status;
    ctx->table_retry_at = ctx->table_calls + ctx->table_backoff;
    if (ctx->table_backoff < 4096) ctx->table_backoff *= 2;
    if (!ctx->table_said)
        fprintf(stderr, "[halo] fixed-base table of %zu bytes not built (%s): the table-free pipeline runs, same results (halo_ctx_info 6; tried again later)\n", bytes, why.c_str());
    ctx->table_said = true;
    return HALO_OK;
}
// A tagged launch (MsmBatch::tagged) has no table-free form: the caller asks first and keeps its two plain launches otherwise
// (no table yet -- the first MSM over the key builds it --, table mode off, a forced window size, the small-key plan).
bool msm_tagged_ready(const halo_ctx *ctx, const uint32_t *d_bases, size_t n) {
    if (!ctx->d_table || ctx->tbl.c != 20) return false;
    MsmBatch one;
    one.tagged = true;
    return table_eligible(ctx, d_bases, one, n);
}
// halo_set_table_mode(ctx, 0): the table's memory goes back to the device (its launches have drained: every slot is idle)
int table_release(halo_ctx *ctx) {
    if (!ctx->d_table) return HALO_OK;
    for (int k = 0; k < HALO_SLOTS; ++k) {
        if (ctx->wss[k].in_flight) { set_error("table mode: an MSM is in flight on this context"); return HALO_E_ARG; }
        HALO_HIP(hipStreamSynchronize(ctx->streams[k]));
    }
    alloc_epoch_bump(ctx);  // cached launch graphs name the table
    table_detach(ctx);
    return HALO_OK;
}
bool fold_table_wanted(const halo_ctx *ctx) {
    if (ctx->d_foldtab || ctx->fold_table_mode == 0 || !ctx->shards.empty() || ctx->parent) return false;
    return ctx->fold_table_mode == 1 || (tuning().fold_table_after > 0 && ctx->n >= ((size_t)1 << 18) && ctx->n <= ((size_t)1 << 21));
}
bool table_should_demote(halo_ctx *ctx) {
    if (!ctx->d_table || ctx->tbl.rows <= ctx->tbl.W) return false;
    {
        std::lock_guard<std::mutex> lk(ctx->share->mu);
        if (ctx->share->users != 1 || ctx->share->d_table != ctx->d_table) return false;
    }
    return table_budget_room(ctx, foldtab_need_bytes(ctx->n), (size_t)(ctx->tbl.rows - ctx->tbl.W) * ctx->n * 128);
}
int table_demote_now(halo_ctx *ctx) {
    ctx->table_demote = false;
    if (!table_should_demote(ctx)) return HALO_OK;
    for (int k = 0; k < HALO_SLOTS; ++k)
        if (ctx->wss[k].in_flight) return HALO_OK;  // (not now: asked for again by the next refusal)
    int rc = table_release(ctx);  // (the only user: the memory and its reservation go back)
    if (rc) return rc;
    { std::lock_guard<std::mutex> lk(ctx->share->mu); ctx->share->table_fixed_only = true; }
    ctx->table_retry_at = 0;
    ctx->table_status = 0;
    return HALO_OK;
}
// this context stops using the table; the memory goes back when no clone uses it either (each user's view is its own d_table:
// a user that still holds one is counted by looking at the share's other users -- conservatively: freed by the last user of the key)
void table_detach(halo_ctx *ctx) {
    if (!ctx->d_table) return;
    bool free_it = false;
    {
        std::lock_guard<std::mutex> lk(ctx->share->mu);
        if (ctx->share->users == 1 && ctx->share->d_table == ctx->d_table) { ctx->share->d_table = nullptr; ctx->share->tbl = TblPlan{}; free_it = true; }
    }
    if (free_it) {
        (void)hipFree(ctx->d_table);
        table_budget_release(ctx, (size_t)ctx->tbl.rows * ctx->n * 128);
    }
    ctx->d_table = nullptr;
    ctx->tbl = TblPlan{};
}
// can this launch take the table pipeline?  One MSM, all windows, over a stretch of the context's own key -- of at least 2^20
// points, or at least half of a smaller key (that plan's coarse ranges are sized for the key) -- indices within 31 bits.
bool table_eligible(const halo_ctx *ctx, const uint32_t *d_bases, const MsmBatch &members, size_t n) {
    if (ctx->table_mode == 0 || ctx->window_bits != 0 || members.parts != 1) return false;
    TblPlan tp = table_plan(ctx->n);
    if (members.tagged && (tp.c != 20 || n > TBL_PIECE || members.count != 1)) return false;  // (one piece, 2 x 512 coarse ranges)
    if (members.count != 1) {  // batches: small-key plan only, members over the same points, count * ranges coarse ranges at most 512
        uint32_t cpow = 1;
        while ((int)cpow < members.count) cpow <<= 1;
        if (tp.c == 20 || cpow * tp.ranges > TBL_MAX_RANGES) return false;
        for (int b = 1; b < members.count; ++b)
            if (members.base_off[b] != members.base_off[0]) return false;
    }
    size_t least = tp.c == 20 ? table_slide_min() : ((size_t)1 << 17);
    const size_t rows = ctx->d_table ? (size_t)ctx->tbl.rows : (size_t)tp.W;
    if (ctx->n < least || (n < least && !(members.sub && tp.c == 20 && n >= 4096)) || (tp.c != 20 && 2 * n < ctx->n) || n % 4 != 0 || rows * ctx->n >= ((size_t)1 << 31)) return false;
    return d_bases >= ctx->d_bases && d_bases + AFF_STRIDE * n <= ctx->d_bases + AFF_STRIDE * ctx->n;
}
// the shape of the row / column window sums (k_msm_reduce_rc) for a launch of `sets` bucket sets of B buckets each: every launch
// table_eligible accepts has one (c = 20: one set, or the two of a tagged launch; c = 17: a power of two of at most 8)
static RcShape table_rc_shape(int c, uint32_t B, uint32_t sets) {
    RcShape r;
    if (c == 20 && (sets == 1 || sets == 2) && B == (1u << 19)) { r.lg_rows = 9; r.lg_cols = 10; r.per = 16; }  // (2 sets: a tagged launch, 2048 waves)
    else if (c == 17 && B == (1u << 16) && (sets == 1 || sets == 2 || sets == 4 || sets == 8)) { r.lg_rows = 8; r.lg_cols = 8; r.per = sets == 1 ? 4 : (int)(2 * sets); }
    return r;
}
// A context whose table holds every shift slides (ctx->tbl.slide) -- one MSM in one piece with the row / column window sums; the
// tagged launch, the pieces of a larger MSM and table mode 1 take the fixed windows on rows 20 w of the same table.
static TblPlan table_launch_plan(const halo_ctx *ctx, const MsmBatch &members, size_t n) {
    const int count = members.count;
    TblPlan tp = ctx->tbl;
    if (tp.rows == SLIDE_BITS && (members.tagged || count != 1 || n > TBL_PIECE || ctx->table_mode == 1)) tp = table_plan_fixed_on(ctx->tbl, ctx->n);
    return tp;
}
// task length of the bucket kernel for a table launch of `entries` digits: the chain bound per lane, the W n additions over the
// chip's 2048 x 64 lanes in one round
static uint32_t tmsm_kmax(const halo_ctx *ctx, size_t entries) {
    if (ctx->task_len > 0) return (uint32_t)ctx->task_len;
    if (entries <= (size_t)16 * 131072) return 16;
    if (entries <= (size_t)32 * 131072) return 32;
    return KMAX;
}
// records in front of the static layout of `order`: one per kmax entries at most (the bound of the tasks beyond one per
// bucket), rounded so that the blocks of the bucket kernel line up with the static layout
static size_t tmsm_ovf_records(size_t entries, uint32_t kmax) { return (entries / kmax + 1 + 255) / 256 * 256; }
// records of `order` a piece of `entries` digits over `buckets` buckets takes (tmsm_enqueue_piece: overflow region + one per bucket):
// what the slot's cap_tasks has to hold, at the task length the piece will run with
size_t tmsm_order_records(const halo_ctx *ctx, size_t entries, size_t buckets) { return tmsm_ovf_records(entries, tmsm_kmax(ctx, entries)) + buckets; }
int tmsm_enqueue_launches(halo_ctx *ctx, MsmWorkspace &ws, const uint32_t *d_bases, const MsmBatch &members, bool mont, size_t n, int partner) {
    const TblPlan tp = table_launch_plan(ctx, members, n);
    size_t pieces = tp.c == 20 ? (n + TBL_PIECE - 1) / TBL_PIECE : 1;
    uint32_t cpow = 1;  // a batch (small-key plan, one piece) lays its members' bucket sets side by side: a power of two of them
    while ((int)cpow < msm_outputs(members)) cpow <<= 1;
    const RcShape rcs = table_rc_shape(tp.c, tp.B, cpow);
    if (!rcs.per || rc_points(rcs) * cpow * pieces > ws.cap_windows) {
        set_error("msm: table plan exceeds workspace");
        return HALO_E_ARG;
    }
    size_t len = ((n + pieces - 1) / pieces + 3) / 4 * 4, off = 0;
    // `partner` >= 0: the odd pieces run on that slot's workspace and stream (forked off this stream here, joined below) and
    // leave their window sums in THIS slot's pinned buffer, where msm_combine_member adds the pieces up.
    if (pieces < 2) partner = -1;
    int slot = (int)(&ws - ctx->wss);
    hipStream_t mine = ctx->stream;
    if (partner >= 0) {
        const size_t entries = (size_t)tp.W * len * members.count;
        if (rc_points(rcs) * cpow > ctx->wss[partner].cap_windows ||
            tmsm_ovf_records(entries, tmsm_kmax(ctx, entries)) + (size_t)tp.B * cpow > ctx->wss[partner].cap_tasks)
            partner = -1;  // (the pieces then run one after the other on this slot: same result)
    }
    if (partner >= 0) {
        HALO_HIP(hipEventRecord(ctx->ev_piece[slot][0], mine));
        HALO_HIP(hipStreamWaitEvent(ctx->streams[partner], ctx->ev_piece[slot][0], 0));
    }
    for (size_t k = 0; k < pieces; ++k, off += len) {
        size_t m = off + len <= n ? len : n - off;  // (n and len are multiples of 4)
        bool alt = partner >= 0 && (k & 1);
        StreamGuard on(ctx, alt ? ctx->streams[partner] : mine);
        int rc = tmsm_enqueue_piece(ctx, alt ? ctx->wss[partner] : ws, tp, d_bases + AFF_STRIDE * off, members, off, mont, m, (int)k, ws.h_winsum);
        if (rc) return rc;
    }
    if (partner >= 0) {
        HALO_HIP(hipEventRecord(ctx->ev_piece[slot][1], ctx->streams[partner]));
        HALO_HIP(hipStreamWaitEvent(mine, ctx->ev_piece[slot][1], 0));
    }
    MsmPlan p;
    p.c = tp.c; p.W = tp.W; p.B = tp.B; p.batch = msm_outputs(members); p.w0 = 0; p.w1 = tp.W;
    p.table_pieces = (int)pieces;
    p.table_sets = (int)cpow;
    p.table_rc_lg_rows = rcs.lg_rows;
    p.table_rc_lg_cols = rcs.lg_cols;
    p.table_slide = tp.slide;
    // (the pieces are of one length but for the last: the task length class is noted from the first)
    p.pipeline = tp.slide ? 3 : 2;
    p.kmax = tmsm_kmax(ctx, (size_t)tp.W * (len < n ? len : n) * members.count);
    p.winsum_form = 2;
    p.table_rc_per = rcs.per;
    ws.plan = p;
    return HALO_OK;
}
// one piece: its (S, T) pairs to slot `piece` of d_winsum / h_winsum (rc_points(rcs) records per set)
static int tmsm_enqueue_piece(halo_ctx *ctx, MsmWorkspace &ws, const TblPlan &plan, const uint32_t *d_bases, const MsmBatch &members, size_t soff, bool mont,
                              size_t n, int piece, uint64_t *h_dst) {
    TblPlan tp = plan;
    uint32_t cpow = 1;
    while ((int)cpow < msm_outputs(members)) cpow <<= 1;
    size_t entries = (size_t)tp.W * n * members.count;
    if (n > ws.cap_n || entries > ws.cap_sorted || (size_t)tp.B * cpow > ws.cap_counts) { set_error("msm: table plan exceeds workspace"); return HALO_E_ARG; }
    if (!ws.d_fine16) {
        alloc_epoch_bump(ctx);
        HALO_HIP(hipMalloc(&ws.d_fine16, ws.cap_sorted * 2));
    }
    hipStream_t s = ctx->stream;
    uint32_t base_off = (uint32_t)((d_bases - ctx->d_bases) / AFF_STRIDE);
    uint32_t *d_digits = reinterpret_cast<uint32_t *>(ws.d_canon);  // 4 * W n bytes per member <= 2 * cap_sorted
    TblScalars srcs{};
    for (int b = 0; b < members.count; ++b) srcs.p[b] = members.scalars[b] + 4 * soff;
    HALO_LAUNCH(ctx, "k_tmsm_recode", k_tmsm_recode, dim3((unsigned)((n + 255) / 256), (unsigned)members.count), dim3(256), 0, srcs, mont ? 1 : 0,
                members.tagged ? 1 : 0, (uint32_t)n, tp, d_digits, ws.d_meta, ws.d_blockoff, ws.d_tblockoff);
    // from here on: ONE MSM of rows = count * W digit rows over sets * B buckets
    const uint32_t rows = (uint32_t)tp.W * (uint32_t)members.count;
    tp.B *= cpow; tp.ranges *= cpow;
    for (uint32_t k = cpow; k > 1; k >>= 1) tp.rbits++;
    uint32_t nchunks = 256u / rows;  // 19 (17) chunks per window: about one block per CU
    uint32_t chunk_len = (uint32_t)((n + nchunks - 1) / nchunks);
    chunk_len = (chunk_len + 3) / 4 * 4;
    dim3 gridc((unsigned)(rows * nchunks)), b1024(1024), b256(256);
    uint32_t *chist = ws.d_hist, *cstart = ws.d_hist + (size_t)rows * nchunks * tp.ranges;  // <= 255 * 512 + 513 words <= cap_hist
    const uint32_t kmax = tmsm_kmax(ctx, entries);
    const bool wide = tp.ranges > TBL_MAX_RANGES;  // (two bucket sets of the c = 20 plan: 1024 coarse ranges)
    if (wide) HALO_LAUNCH(ctx, "k_tmsm_coarse_hist2", k_tmsm_coarse_hist2, gridc, b1024, 0, d_digits, (uint32_t)n, nchunks, chunk_len, tp, chist);
    else HALO_LAUNCH(ctx, "k_tmsm_coarse_hist", k_tmsm_coarse_hist, gridc, b1024, 0, d_digits, (uint32_t)n, nchunks, chunk_len, tp, chist);
    uint32_t *rtotal = cstart + tp.ranges + 1;
    HALO_LAUNCH(ctx, "k_tmsm_scan_chunks", k_tmsm_scan_chunks, dim3(tp.ranges), b256, 0, chist, rows * nchunks, tp.ranges, rtotal);
    HALO_LAUNCH(ctx, "k_tmsm_scan_ranges", k_tmsm_scan_ranges, dim3(1), dim3(tp.ranges), 0, rtotal, cstart);
    if (wide) HALO_LAUNCH(ctx, "k_tmsm_coarse_scatter2", k_tmsm_coarse_scatter2, gridc, b1024, 0, d_digits, (uint32_t)n, nchunks, chunk_len, chist, cstart,
                          (uint32_t)ctx->n, base_off, tp, ws.d_presort, ws.d_fine16);
    else HALO_LAUNCH(ctx, "k_tmsm_coarse_scatter", k_tmsm_coarse_scatter, gridc, b1024, 0, d_digits, (uint32_t)n, nchunks, chunk_len, chist, cstart,
                     (uint32_t)ctx->n, base_off, tp, ws.d_presort, ws.d_fine16);
    // `order` (d_order): an overflow region of `ovf` records, then one record per bucket (k_tmsm_fine_sort).  No global task
    // order, no task_g: the table pipeline has no launch between sort and bucket kernel.
    const uint32_t total = tp.B;
    const size_t ovf = tmsm_ovf_records(entries, kmax);
    if (ovf + total > ws.cap_tasks) { set_error("msm: table plan exceeds workspace"); return HALO_E_ARG; }
    HALO_LAUNCH(ctx, "k_tmsm_fine_sort", k_tmsm_fine_sort, dim3(tp.ranges), b1024, TBL_STAGE * 4, ws.d_presort, ws.d_fine16, cstart, kmax, tp, ws.d_counts,
                ws.d_starts, ws.d_ntask, ws.d_toff, ws.d_biglist, ws.d_meta, ws.d_sorted, (uint32_t)ovf, reinterpret_cast<uint4 *>(ws.d_order));
    dim3 gridt((unsigned)((ovf + total) / 256));  // (a multiple of 256 records: no lane past the last one)
    HALO_LAUNCH(ctx, "k_msm_accumulate", k_msm_accumulate, gridt, b256, 0, ctx->d_table, ws.d_sorted, ws.d_meta + META_OVF, (uint32_t)ovf,
                reinterpret_cast<const uint4 *>(ws.d_order), ws.d_buckets);
    HALO_LAUNCH(ctx, "k_msm_combine", k_msm_combine, dim3(512 + 1024), dim3(64), 0, ws.d_ntask, ws.d_toff, ws.d_tblockoff, ws.d_meta, ws.d_biglist,
                total, 512u, ws.d_buckets);
    // window sums by rows and columns of the bucket index (k_msm_reduce_rc): rows + columns entries per set, then blocks of 64
    // entries -> (S, T) pairs, combined on the host (msm_combine_member)
    const RcShape rcs = table_rc_shape(tp.c, tp.B / cpow, cpow);
    const uint32_t pts = rc_points(rcs) * cpow, nb = (tp.B / cpow) / (64u * (uint32_t)rcs.per);
    uint64_t *d_rc = ws.d_winsum + (size_t)piece * pts * 12;
    HALO_LAUNCH(ctx, "k_msm_reduce_rc", k_msm_reduce_rc, dim3(cpow * 2 * nb), dim3(64), 0, ws.d_buckets, ws.d_ntask, ws.d_toff, ws.d_tblockoff, rcs, ws.d_seg);
    uint64_t *h_rc = h_dst + (size_t)piece * pts * 12;
    int rc = rc_mid_enqueue(ctx, ws.d_seg, pts / 2, ctx->sink_done ? h_rc : d_rc, ctx->sink_done, ws.d_meta + 255);
    if (rc) return rc;
    HALO_HIP(hipGetLastError());
    if (!ctx->sink_done) HALO_HIP(hipMemcpyAsync(h_rc, d_rc, (size_t)pts * 96, hipMemcpyDeviceToHost, s));
    return HALO_OK;
}

}  // namespace halo
