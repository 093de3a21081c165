// One member's share of the mixed fused check batch (halo_pcdl_check_batch_mixed_fused; pcdl_batch.hip check_members_mixed_fused):
// the members of the relation have their own sizes, so their records and scalars lie DENSE, one behind the other, and a lane finds
// its own through a descriptor.  mixed_terms.hip's k_mixed_terms calls mixed_terms_member once per lane;
// tests/native/mixed_terms_host.cpp compiles the same text for the CPU (HALO_DEV = inline) and runs it under ASan + UBSan over heap
// blocks of exactly the needed size.  Needs fused_lane.hpp only: the arithmetic is fused_terms_lane's, with lg taken per member.
//
// Member a's descriptor, MIXED_DESC_WORDS 32-bit words at desc + MIXED_DESC_WORDS a:
//     lg_a | the offset of its record in 64-bit words | the offset of its first term in terms
// both offsets prefix sums over the members in front of it (fused_rec_words(lg) words, fused_term_count(lg) terms each).  They fit 32
// bits because a call holds at most 65535 members of lg <= 24 and fewer than 2^32 terms.
#pragma once
#include "fused_lane.hpp"

namespace halo {

constexpr int MIXED_DESC_WORDS = 3;

// recs, scalars: the dense records and the dense scalars (4 words a term) of ALL members; shares: 4 words per member.  The lane
// reads its own record and writes its own scalars and share only.
HALO_DEV void mixed_terms_member(const uint64_t *recs, const uint32_t *desc, uint32_t a, uint64_t *scalars, uint64_t *shares) {
    const uint32_t *d = desc + (size_t)MIXED_DESC_WORDS * a;
    fused_terms_lane(recs + (size_t)d[1], (int)d[0], scalars + 4 * (size_t)d[2], shares + 4 * (size_t)a);
}

// The host side of the same layout: the descriptors of M members of sizes lgs[0 .. M); *rec_words and *terms are the totals
inline void mixed_terms_describe(const uint32_t *lgs, size_t M, uint32_t *desc, size_t *rec_words, size_t *terms) {
    size_t ro = 0, to = 0;
    for (size_t a = 0; a < M; ++a) {
        desc[MIXED_DESC_WORDS * a] = lgs[a];
        desc[MIXED_DESC_WORDS * a + 1] = (uint32_t)ro;
        desc[MIXED_DESC_WORDS * a + 2] = (uint32_t)to;
        ro += fused_rec_words((int)lgs[a]);
        to += fused_term_count((int)lgs[a]);
    }
    *rec_words = ro;
    *terms = to;
}

}  // namespace halo
