// Field constants as the kernels receive them: by value as a kernel argument (SGPRs) or as the members of a record in device
// memory (internal.hpp OpenConst).  The host fills them (to_nform, to_arg); a kernel turns them back into the types it
// computes with (from_nform, from_arg).  The device half needs fr29.hpp and is left out of a host-only compile.
#pragma once
#include "host_math.hpp"
#ifdef __HIPCC__
#include "fr29.hpp"
#endif

namespace halo {

// An Fr multiplier in N-form (fr29.hpp: k 2^261 mod r = the Montgomery limbs of 32 k), 9 x 29-bit limbs
struct FsArg { uint32_t v[9]; };
inline FsArg to_nform(const host::Fr &k) {
    host::Fr t = k * host::Fr::from_u64(32);
    FsArg a;
    for (int i = 0; i < 9; ++i) {
        int bit = 29 * i, w = bit >> 6, sh = bit & 63;
        uint64_t lo = t.l[w] >> sh;
        if (sh > 35 && w + 1 < 4) lo |= t.l[w + 1] << (64 - sh);
        a.v[i] = (uint32_t)(i < 8 ? (lo & ((1u << 29) - 1)) : lo);
    }
    return a;
}
// An Fr element as its Montgomery limbs, 8 x 32 bits
struct FeArg { uint32_t v[8]; };
inline FeArg to_arg(const host::Fr &f) {
    FeArg a;
    for (int i = 0; i < 4; ++i) { a.v[2 * i] = (uint32_t)f.l[i]; a.v[2 * i + 1] = (uint32_t)(f.l[i] >> 32); }
    return a;
}

#ifdef __HIPCC__
HALO_DEV Fs<1> from_nform(const FsArg &a) {
    Fs<1> r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.v[i] = a.v[i];
    return r;
}
HALO_DEV Fe from_arg(const FeArg &a) {
    Fe r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = a.v[i];
    return r;
}
#endif

}  // namespace halo
