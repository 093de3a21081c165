// One lane's share of the small MSMs of the verifier (pcdl.rs:288-310): k P by a 256-step ladder.  small_sums.hip's k_batch_small_msm and
// k_small_msm_seg call it once per lane; tests/native/small_msm_host.cpp compiles the same text for the CPU (HALO_DEV = inline,
// field.hpp) and runs it under ASan + UBSan.  Needs curve.hpp only.
#pragma once
#include "curve.hpp"

namespace halo {

// k P for one lane's term: the 256-step ladder (double, add, keep the sum if the bit is set -- no divergence although the
// scalars differ); k canonical (not Montgomery), a dead lane keeps infinity
HALO_DEV JacN small_msm_ladder(const AffN &p, const Fe &k, bool live) {
    JacN acc = jac_inf();
#pragma unroll 1
    for (int limb = 7; limb >= 0; limb--) {
        uint32_t word = 0;
#pragma unroll
        for (int q = 0; q < 8; q++) word = (q == limb) ? k.v[q] : word;
#pragma unroll 1
        for (int bit = 31; bit >= 0; bit--) {
            acc = jac_dbl(acc);
            JacN s = jac_madd(acc, p);
            bool take = live && ((word >> bit) & 1u);
#pragma unroll
            for (int i = 0; i < 9; i++) {
                acc.x.v[i] = take ? s.x.v[i] : acc.x.v[i];
                acc.y.v[i] = take ? s.y.v[i] : acc.y.v[i];
                acc.z.v[i] = take ? s.z.v[i] : acc.z.v[i];
            }
        }
    }
    return acc;
}

}  // namespace halo
