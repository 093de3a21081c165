// One lane's share of the fused check batch (halo_pcdl_check_batch_fused; pcdl_batch.hip check_members_fused): the scalars of ONE
// member's terms in the relation  sum_a r_a E_a + sum_a s_a F_a = 0  (include/halo_accumulation.h).  fused_check.hip's k_fused_terms
// calls it once per lane; tests/native/fused_lane_host.cpp compiles the same text for the CPU (HALO_DEV = inline) and runs it
// under ASan + UBSan.  Needs fr29.hpp only.
//
// The member's record, FUSED_REC_EXTRA + lg + 1 elements as arkworks keeps them (x 2^256 mod r, 4 words each):
//     xi_0 .. xi_lg | z | v | c | r | s
// Its 2 lg + 2 scalars, canonical integers in [0, r) of 4 words each, in the order of the member's points C' | L_0 .. | R_0 .. | U:
//     r | r xi_1^-1 .. r xi_lg^-1 | r xi_1 .. r xi_lg | s - r c
// and its share of H's scalar, r (v - c h(z)) xi_0, h(z) = prod_k (1 + xi_(lg - k) z^(2^k)) as h_eval_lane multiplies it (hpoly.hip).
//
// The inverses come from Montgomery's trick with ONE fs_inv: the prefix products xi_1 .. xi_(j - 1) wait in the output slots of the
// L scalars (this lane's own words of global memory, read back before they are overwritten), so nothing is indexed in registers
// and the lane needs no LDS and no scratch whatever lg is.  All arithmetic is in the N-form of fr29.hpp (x 2^261: closed under
// fs_mul), entered by one product with 2^266 per loaded element; r is kept plain, so r * N(y) is the canonical r y directly.
// A zero challenge (the transcripts reject it before any record is written) makes the shared inverse 0: every xi_j^-1 comes out
// as 0 and the lane ends like any other.
#pragma once
#include "fr29.hpp"

namespace halo {

constexpr int FUSED_REC_EXTRA = 5;  // z | v | c | r | s behind the lg + 1 challenges
constexpr int FUSED_MAX_LG = 24;
constexpr size_t fused_rec_words(int lg) { return 4 * (size_t)(lg + 1 + FUSED_REC_EXTRA); }
constexpr size_t fused_term_count(int lg) { return 2 * (size_t)lg + 2; }

// `out` is read and written by this lane only; it must not alias rec
HALO_DEV void fused_terms_lane(const uint64_t *rec, int lg, uint64_t *out, uint64_t *share) {
    const Fs<1> c266 = fs_c266(), unit = fs_unit(), one = fs_n_one();
    const uint64_t *tail = rec + 4 * (size_t)(lg + 1);
    const Fs<2> z = fs_mul(fs_load(tail), c266), v = fs_mul(fs_load(tail + 4), c266), c = fs_mul(fs_load(tail + 8), c266);
    const Fs<2> rp = fs_mul(fs_mul(fs_load(tail + 12), c266), unit), sp = fs_mul(fs_mul(fs_load(tail + 16), c266), unit);  // r, s themselves
    // h(z), and the prefix products of xi_1 .. xi_lg into the L slots (slot j holds xi_1 .. xi_(j - 1), j = 1 .. lg)
    Fs<2> hz = fs_tighten(fs_add(one, fs_mul(fs_mul(fs_load(rec + 4 * (size_t)lg), c266), z)));
    Fs<2> zi = z;
#pragma unroll 1
    for (int k = 1; k < lg; k++) {
        zi = fs_mul(zi, zi);
        hz = fs_mul(hz, fs_add(one, fs_mul(fs_mul(fs_load(rec + 4 * (size_t)(lg - k)), c266), zi)));
    }
    Fs<2> p = fs_widen<2>(one);
#pragma unroll 1
    for (int j = 1; j <= lg; j++) {
        fs_store(out + 4 * (size_t)j, p);
        p = fs_mul(p, fs_mul(fs_load(rec + 4 * (size_t)j), c266));
    }
    Fs<2> inv = fs_inv(p);  // (xi_1 .. xi_lg)^-1
#pragma unroll 1
    for (int j = lg; j >= 1; j--) {
        const Fs<2> xj = fs_mul(fs_load(rec + 4 * (size_t)j), c266);
        const Fs<2> xinv = fs_mul(inv, fs_load(out + 4 * (size_t)j));  // (xi_1 .. xi_j)^-1 xi_1 .. xi_(j - 1)
        inv = fs_mul(inv, xj);
        fs_store(out + 4 * (size_t)j, fs_mul(rp, xinv));
        fs_store(out + 4 * (size_t)(lg + j), fs_mul(rp, xj));
    }
    fs_store(out, rp);
    fs_store(out + 4 * (2 * (size_t)lg + 1), fs_sub<2>(sp, fs_mul(rp, c)));
    const Fs<4> t = fs_sub<2>(v, fs_mul(c, hz));  // N(v - c h(z))
    fs_store(share, fs_mul(fs_mul(rp, t), fs_mul(fs_load(rec), c266)));
}

}  // namespace halo
