// K3: the key folds of pcdl::open's halving loop (pcdl.rs:216-219), one and two rounds per pass, single and member-batched.
//
// The point fold uses ONE scalar for the whole launch (one per member in the batched forms), so every lane runs the same
// double-and-add schedule with no divergence.
#include <algorithm>

#include "curve_quad.hpp"
#include "fold_lane.hpp"
#include "internal.hpp"

namespace halo {

// The member-batched forms (halo_pcdl_open_batch above the no-fold size: once folded, a key is its member's own) are the single
// kernels with blockIdx.y = member.  Member b reads src + b * src_stride points (0: every member reads the same key -- the first
// fold, from the context's) and writes dst + b * dst_stride; src and dst may be the same array, as for the single kernels.  Its
// digits are record b of `digs` (FOLD_DIG_WORDS words of device memory: a GlvArg for one level, a GlvArg3 for two), not a kernel
// argument.  The record's address depends on blockIdx.y and kernel arguments only, so it is copied into scalar registers once and
// the branches the digits steer stay wave-uniform, exactly as with the single kernels' by-value argument.
template <class Arg>
HALO_DEV Arg fold_digits_of(const uint32_t *__restrict__ digs) {
    static_assert(sizeof(Arg) <= FOLD_DIG_WORDS * 4, "fold digit record");
    return *reinterpret_cast<const Arg *>(digs + FOLD_DIG_WORDS * (size_t)blockIdx.y);
}

// ------------------------------------------------------------------ K3: G'[j] = G[j] + xi * G[j+m]
// fold_one (fold_lane.hpp) is one lane's G[j] + xi * G[j + m] as a Jacobian point.
// Each lane folds two points (j and j + half) and brings both back to affine with ONE Fermat inversion
// (of Z_a * Z_b): the inversion is ~15 % of a single fold.
// (src and dst may be the same array: a lane reads j, j + m, j + half, j + half + m and writes j and j + half only)
HALO_DEV void fold_points_lane(const uint32_t *src, uint32_t *dst, uint32_t j, uint32_t m, uint32_t half, const GlvArg &a) {
    bool two = j + half < m;
    JacN ra = fold_one(src, j, m, a);
    JacN rb = jac_inf();
    if (two) rb = fold_one(src, j + half, m, a);
    bool ia = jac_is_inf(ra), ib = jac_is_inf(rb);
    Fq<4> za = ia ? fq_widen<4>(fq_one()) : ra.z, zb = ib ? fq_widen<4>(fq_one()) : rb.z;
    Fq<2> zi = fq_inv(fq_mul(za, zb));
    Fq<2> zia = fq_mul(zi, zb), zib = fq_mul(zi, za);
    AffN oa = aff_inf(), ob = aff_inf();
    if (!ia) {
        Fq<2> z2 = fq_sqr(zia);
        oa.x = fq_mul(ra.x, z2);
        oa.y = fq_mul(ra.y, fq_mul(z2, zia));
    }
    if (!ib) {
        Fq<2> z2 = fq_sqr(zib);
        ob.x = fq_mul(rb.x, z2);
        ob.y = fq_mul(rb.y, fq_mul(z2, zib));
    }
    aff_store(dst + AFF_STRIDE * (size_t)j, oa);
    if (two) aff_store(dst + AFF_STRIDE * (size_t)(j + half), ob);
}
__global__ __launch_bounds__(256) void k_fold_points(uint32_t *__restrict__ G, uint32_t m, uint32_t half, GlvArg a) {
    uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= half) return;
    fold_points_lane(G, G, j, m, half, a);
}
__global__ __launch_bounds__(256) void k_fold_points_batch(const uint32_t *src, uint64_t src_stride, uint32_t *dst, uint64_t dst_stride, uint32_t m,
                                                           uint32_t half, const uint32_t *__restrict__ digs) {
    uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= half) return;
    const GlvArg a = fold_digits_of<GlvArg>(digs);
    fold_points_lane(src + AFF_STRIDE * src_stride * blockIdx.y, dst + AFF_STRIDE * dst_stride * blockIdx.y, j, m, half, a);
}

// ------------------------------------------------------------------ K3': two halving rounds of G in one pass
// fold_one4 (fold_lane.hpp) is one lane's G[j] + s1 G[j+m] + s2 G[j+2m] + s3 G[j+3m].
// G (read) and out (written) may be the same array: a lane reads the indices j + t m and writes index j only
// park: 27 x 256 words of LDS.  The first result waits there while the second ladder runs (three bases + the accumulator + a
// mixed addition's temporaries fill the 256 registers that two waves per SIMD allow); word k of thread t at park[256 k + t]
// (the tail repeats fold_points_lane's on purpose: as a shared function, by reference or by value, it costs k_fold_points4 and
// its batch twin 15 to 21 more VGPRs at the same two waves per SIMD, which leaves no margin below the cap of 256)
HALO_DEV void fold_points4_lane(const uint32_t *G, uint32_t *out, uint32_t j, uint32_t m, uint32_t half, const GlvArg3 &a, uint32_t *park) {
    bool two = j + half < m;
    JacN rb = jac_inf();
    {
        JacN ra0 = fold_one4(G, j, m, a);
        uint32_t *mine = park + threadIdx.x;
#pragma unroll
        for (int k = 0; k < 9; k++) { mine[256 * k] = ra0.x.v[k]; mine[256 * (9 + k)] = ra0.y.v[k]; mine[256 * (18 + k)] = ra0.z.v[k]; }
    }
    if (two) rb = fold_one4(G, j + half, m, a);
    JacN ra;
    {
        const uint32_t *mine = park + threadIdx.x;
#pragma unroll
        for (int k = 0; k < 9; k++) { ra.x.v[k] = mine[256 * k]; ra.y.v[k] = mine[256 * (9 + k)]; ra.z.v[k] = mine[256 * (18 + k)]; }
    }
    bool ia = jac_is_inf(ra), ib = jac_is_inf(rb);
    Fq<4> za = ia ? fq_widen<4>(fq_one()) : ra.z, zb = ib ? fq_widen<4>(fq_one()) : rb.z;
    Fq<2> zi = fq_inv(fq_mul(za, zb));
    Fq<2> zia = fq_mul(zi, zb), zib = fq_mul(zi, za);
    AffN oa = aff_inf(), ob = aff_inf();
    if (!ia) {
        Fq<2> z2 = fq_sqr(zia);
        oa.x = fq_mul(ra.x, z2);
        oa.y = fq_mul(ra.y, fq_mul(z2, zia));
    }
    if (!ib) {
        Fq<2> z2 = fq_sqr(zib);
        ob.x = fq_mul(rb.x, z2);
        ob.y = fq_mul(rb.y, fq_mul(z2, zib));
    }
    aff_store(out + AFF_STRIDE * (size_t)j, oa);
    if (two) aff_store(out + AFF_STRIDE * (size_t)(j + half), ob);
}
__global__ __launch_bounds__(256, 2) void k_fold_points4(const uint32_t *G, uint32_t *out, uint32_t m, uint32_t half, GlvArg3 a) {
    __shared__ uint32_t park[27 * 256];
    uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= half) return;
    fold_points4_lane(G, out, j, m, half, a, park);
}
__global__ __launch_bounds__(256, 2) void k_fold_points4_batch(const uint32_t *src, uint64_t src_stride, uint32_t *dst, uint64_t dst_stride, uint32_t m,
                                                               uint32_t half, const uint32_t *__restrict__ digs) {
    __shared__ uint32_t park[27 * 256];
    uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= half) return;
    const GlvArg3 a = fold_digits_of<GlvArg3>(digs);
    fold_points4_lane(src + AFF_STRIDE * src_stride * blockIdx.y, dst + AFF_STRIDE * dst_stride * blockIdx.y, j, m, half, a, park);
}

// The same two-level fold for SMALL keys (fewer than 2^16 outputs): there the pass is one latency chain (~128 doublings,
// ~210 additions, one inversion: 1.5 ms whatever m is), so the 4 lanes of a quad share every group operation
// (curve_quad.hpp: 3 product levels per doubling, 5 per mixed addition instead of 7 and 11 products) -- one output per quad.
// t = the lane's index in its (member's) launch, 4 lanes per output
HALO_DEV void fold_points4_quad_lane(const uint32_t *G, uint32_t *out, uint32_t t, uint32_t m, const GlvArg3 &a) {
    constexpr uint32_t BETA[9] = {0x1342a796, 0x3fdac51, 0x54dab11, 0x5b221a6, 0xccd27ac, 0x15cc87a4, 0x1b1533b6, 0x169e85e1, 0x3b0093};
    constexpr uint32_t BETA2[9] = {0xcbd58eb, 0x1a2f8f16, 0xd140efa, 0x7bdfb9, 0x1333ecad, 0xa33785b, 0x4eacc49, 0x9617a1e, 0x4ff6c};
    uint32_t j = t >> 2;
    int ql = (int)(t & 3);
    bool in = j < m;
    if (!in) j = m - 1;  // whole quads and waves stay busy (DPP); the surplus quads recompute the last output and do not store
    AffN p1 = aff_load(G + AFF_STRIDE * (size_t)(j + m)), p2 = aff_load(G + AFF_STRIDE * (size_t)(j + 2 * m)),
         p3 = aff_load(G + AFF_STRIDE * (size_t)(j + 3 * m));
    bool live1 = !aff_is_inf(p1), live2 = !aff_is_inf(p2), live3 = !aff_is_inf(p3);
    Fq<2> one = fq_widen<2>(fq_one()), beta = fq_const(BETA), beta2 = fq_const(BETA2);
    auto step = [&](JacN &acc, const AffN &p, bool live, uint32_t code) {
        if (!code) return;  // wave-uniform
        int e = (int)((code - 1) % 3);
        Fq<2> bc = e == 0 ? one : (e == 1 ? beta : beta2);
        Fq<2> y = code > 3 ? fq_neg<2>(p.y) : p.y;
        acc = jac_madd_quad(acc, p.x, y, bc, live, ql);
    };
    JacN acc = jac_inf();
    int top = a.ndigits - 1;
#pragma unroll 1
    for (int word = top / 10; word >= 0; word--) {
        uint32_t w1 = 0, w2 = 0, w3 = 0;
#pragma unroll
        for (int q = 0; q < 14; q++) {
            w1 = (q == word) ? a.dig[0][q] : w1;
            w2 = (q == word) ? a.dig[1][q] : w2;
            w3 = (q == word) ? a.dig[2][q] : w3;
        }
#pragma unroll 1
        for (int k = (word == top / 10) ? (top % 10) : 9; k >= 0; k--) {
            acc = jac_dbl_quad(acc, ql);
            step(acc, p1, live1, (w1 >> (3 * k)) & 7u);
            step(acc, p2, live2, (w2 >> (3 * k)) & 7u);
            step(acc, p3, live3, (w3 >> (3 * k)) & 7u);
        }
    }
    AffN lo = aff_load(G + AFF_STRIDE * (size_t)j);
    acc = jac_madd_quad(acc, lo.x, lo.y, one, !aff_is_inf(lo), ql);
    if (in && ql == 0) aff_store(out + AFF_STRIDE * (size_t)j, jac_to_aff(acc));  // the inversion: one lane of the quad
}
__global__ __launch_bounds__(256, 2) void k_fold_points4_quad(const uint32_t *G, uint32_t *out, uint32_t m, GlvArg3 a) {
    fold_points4_quad_lane(G, out, blockIdx.x * 256 + threadIdx.x, m, a);
}
__global__ __launch_bounds__(256, 2) void k_fold_points4_quad_batch(const uint32_t *src, uint64_t src_stride, uint32_t *dst, uint64_t dst_stride, uint32_t m,
                                                                    const uint32_t *__restrict__ digs) {
    const GlvArg3 a = fold_digits_of<GlvArg3>(digs);
    fold_points4_quad_lane(src + AFF_STRIDE * src_stride * blockIdx.y, dst + AFF_STRIDE * dst_stride * blockIdx.y, blockIdx.x * 256 + threadIdx.x, m, a);
}

// ================================================================== host launchers
// the digits of one scalar as 3-bit codes, ten to a word, least significant first (fold_lane.hpp GlvArg); returns their number
static int pack_glv_digits(const host::Fr &s_mont, uint32_t (&dig)[14]) {
    host::GlvDigits dg = host::glv_digits(s_mont);
    for (int i = 0; i < 14; ++i) dig[i] = 0;
    for (int i = 0; i < dg.n; ++i) dig[i / 10] |= (uint32_t)dg.d[i] << (3 * (i % 10));
    return dg.n;
}
static GlvArg glv_arg(const host::Fr &xi_mont) {
    GlvArg a;
    a.ndigits = pack_glv_digits(xi_mont, a.dig);
    return a;
}
static GlvArg3 glv_arg3(const host::Fr s[3]) {
    GlvArg3 a;
    a.ndigits = 0;
    for (int t = 0; t < 3; ++t) a.ndigits = std::max(a.ndigits, pack_glv_digits(s[t], a.dig[t]));
    return a;
}
// form (development hook, halo_dev_fold_points): 0 = the size decides; 1 / 2 = one / two outputs per lane whatever m is
int ipa_fold_points(halo_ctx *ctx, uint32_t *d_G, size_t m, const host::Fr &xi_mont, int form) {
    if (m == 0) return HALO_OK;
    GlvArg a = glv_arg(xi_mont);
    // a lane folds the points j and j + half where that still leaves >= 4 waves per SIMD; below, one point per lane
    size_t half = (form ? form == 2 : m >= ((size_t)1 << 18)) ? (m + 1) / 2 : m;
    HALO_LAUNCH(ctx, "k_fold_points", k_fold_points, dim3((unsigned)((half + 255) / 256)), dim3(256), 0, d_G, (uint32_t)m, (uint32_t)half, a);
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}
// dst[j] <- src[j] + s[0] src[j+m] + s[1] src[j+2m] + s[2] src[j+3m], j < m (dst may be src)
// form (development hook): 0 = the sizes decide; 1 / 2 = k_fold_points4 with one / two outputs per lane; 3 = the quad kernel;
// 4 / 5 = the table kernel with one / two outputs per lane, an error where it cannot run
int ipa_fold_points4(halo_ctx *ctx, const uint32_t *d_src, uint32_t *d_dst, size_t m, const host::Fr s[3], int form) {
    if (m == 0) return HALO_OK;
    if (form == 0 || form >= 4) {  // the fold from the context's own (constant) key: a comb table replaces the doubling chain (foldtab.hip)
        int done = fold_points4_tab(ctx, d_src, d_dst, m, s, form);
        if (done < 0) return done;
        if (done) return HALO_OK;
        if (form) { set_error("fold_points4: the table kernel cannot run here (not the context's own key, in place, or no table)"); return HALO_E_ARG; }
    }
    GlvArg3 a = glv_arg3(s);
    if (form ? form == 3 : m < ((size_t)1 << 16)) {  // a latency chain at this size: one output per quad (in place is fine: a quad reads j + t m, writes j)
        HALO_LAUNCH(ctx, "k_fold_points4_quad", k_fold_points4_quad, dim3((unsigned)((4 * m + 255) / 256)), dim3(256), 0, d_src, d_dst, (uint32_t)m, a);
        HALO_HIP(hipGetLastError());
        return HALO_OK;
    }
    size_t half = (form ? form == 2 : m >= ((size_t)1 << 17)) ? (m + 1) / 2 : m;
    HALO_LAUNCH(ctx, "k_fold_points4", k_fold_points4, dim3((unsigned)((half + 255) / 256)), dim3(256), 0, d_src, d_dst, (uint32_t)m, (uint32_t)half, a);
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}

// ---- the member-batched key folds: G members in one launch, member b's digits in record b of d_digs (fold_digits: the host side,
// the very digit strings the single launchers pass by value).  Strides in points; src_stride 0: one shared source.
// form: 0 = the rule of the single launchers applied to all G x m outputs of the launch; 1 / 2 = one / two outputs per lane;
// 3 = one output per quad (two levels only)
void fold_digits(const host::Fr *s, int levels, uint32_t *rec) {
    std::memset(rec, 0, FOLD_DIG_WORDS * 4);
    if (levels == 1) { GlvArg a = glv_arg(s[0]); std::memcpy(rec, &a, sizeof a); }
    else { GlvArg3 a = glv_arg3(s); std::memcpy(rec, &a, sizeof a); }
}
int ipa_fold_points_batch(halo_ctx *ctx, int G, const uint32_t *d_src, size_t src_stride, uint32_t *d_dst, size_t dst_stride, size_t m,
                          const uint32_t *d_digs, int form) {
    if (m == 0 || G == 0) return HALO_OK;
    const size_t outs = (size_t)G * m;
    size_t half = (form ? form == 2 : outs >= ((size_t)1 << 18)) ? (m + 1) / 2 : m;
    HALO_LAUNCH(ctx, "k_fold_points_batch", k_fold_points_batch, dim3((unsigned)((half + 255) / 256), (unsigned)G), dim3(256), 0, d_src, (uint64_t)src_stride,
                d_dst, (uint64_t)dst_stride, (uint32_t)m, (uint32_t)half, d_digs);
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}
int ipa_fold_points4_batch(halo_ctx *ctx, int G, const uint32_t *d_src, size_t src_stride, uint32_t *d_dst, size_t dst_stride, size_t m,
                           const uint32_t *d_digs, int form) {
    if (m == 0 || G == 0) return HALO_OK;
    const size_t outs = (size_t)G * m;
    if (form ? form == 3 : outs < ((size_t)1 << 16)) {
        HALO_LAUNCH(ctx, "k_fold_points4_quad_batch", k_fold_points4_quad_batch, dim3((unsigned)((4 * m + 255) / 256), (unsigned)G), dim3(256), 0, d_src,
                    (uint64_t)src_stride, d_dst, (uint64_t)dst_stride, (uint32_t)m, d_digs);
        HALO_HIP(hipGetLastError());
        return HALO_OK;
    }
    size_t half = (form ? form == 2 : outs >= ((size_t)1 << 17)) ? (m + 1) / 2 : m;
    HALO_LAUNCH(ctx, "k_fold_points4_batch", k_fold_points4_batch, dim3((unsigned)((half + 255) / 256), (unsigned)G), dim3(256), 0, d_src, (uint64_t)src_stride,
                d_dst, (uint64_t)dst_stride, (uint32_t)m, (uint32_t)half, d_digs);
    HALO_HIP(hipGetLastError());
    return HALO_OK;
}

}  // namespace halo
