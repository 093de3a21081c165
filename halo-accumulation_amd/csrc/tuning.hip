// tuning(): the environment is read here and nowhere else in the library (tests/test_abi_cpu.py greps for it).
#include "tuning.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace halo {
namespace {
size_t parse_bytes(const char *e) {  // "48G", "512M", plain bytes
    char *rest = nullptr;
    double v = strtod(e, &rest);
    if (rest && (*rest == 'K' || *rest == 'k')) v *= 1024.0;
    else if (rest && (*rest == 'M' || *rest == 'm')) v *= 1024.0 * 1024.0;
    else if (rest && (*rest == 'G' || *rest == 'g')) v *= 1024.0 * 1024.0 * 1024.0;
    return v > 0 ? (size_t)v : 0;
}
int env_int(const char *name, int dflt) { const char *e = getenv(name); return e ? atoi(e) : dflt; }
Tuning read_env() {
    Tuning t;
    t.trace = getenv("HALO_TRACE") != nullptr;
    t.ipa_timing = getenv("HALO_IPA_TIMING") != nullptr;
    if (const char *e = getenv("HALO_MEMORY_BUDGET")) { t.memory_budget_set = true; t.memory_budget = parse_bytes(e); }
    t.graphs = env_int("HALO_GRAPHS", -1);
    t.fold_async = env_int("HALO_FOLD_ASYNC", -2);
    if (const char *e = getenv("HALO_HOST_SPLIT")) {
        // "a,b[,c[,d]]": 1 to 4 positive numbers of sixteenths that add up to 16, nothing else in the string
        int v[4] = {0, 0, 0, 0}, k = 0, sum = 0;
        bool ok = true;
        const char *q = e;
        while (ok) {
            char *rest = nullptr;
            long x = strtol(q, &rest, 10);
            if (rest == q || x < 1 || x > 16 || k == 4) { ok = false; break; }
            v[k++] = (int)x;
            sum += (int)x;
            if (*rest == 0) break;
            if (*rest != ',') { ok = false; break; }
            q = rest + 1;
        }
        ok = ok && k >= 1 && sum == 16;
        if (ok) { t.host_split_set = true; t.host_pieces = k; for (int i = 0; i < 4; ++i) t.host_split[i] = v[i]; }
        else fprintf(stderr, "[halo] HALO_HOST_SPLIT=%s ignored: 1 to 4 positive numbers of sixteenths that add up to 16\n", e);
    }
    t.fold_table_after = env_int("HALO_FOLD_TABLE_AFTER", t.fold_table_after);
    t.pow_e = env_int("HALO_POW_E", 0);
    if (t.pow_e != 0 && (t.pow_e < 4 || t.pow_e > 64 || (t.pow_e & (t.pow_e - 1)) != 0)) {
        // k_h_coeffs relies on a chain length that is a power of two (its mid * high factor is wave-uniform and changes every
        // fourth step): another value would give wrong coefficients
        fprintf(stderr, "[halo] HALO_POW_E=%d ignored: the chain length must be a power of two in [4, 64]\n", t.pow_e);
        t.pow_e = 0;
    }
    t.dot_blocks = env_int("HALO_DOT_BLOCKS", 0);
    if (t.dot_blocks < 0 || t.dot_blocks > FR_GRID_CAP) {
        // k_dot2_partial writes a record per block below the result slot at 8 * FR_GRID_CAP words: a larger grid would write over it
        const int clamped = t.dot_blocks < 0 ? 1 : FR_GRID_CAP;
        fprintf(stderr, "[halo] HALO_DOT_BLOCKS=%d clamped to %d: the block cap must be in [1, %d]\n", t.dot_blocks, clamped, FR_GRID_CAP);
        t.dot_blocks = clamped;
    }
    t.spin_us = env_int("HALO_SPIN_US", t.spin_us);
    return t;
}
}  // namespace

const Tuning &tuning() {
    static const Tuning t = read_env();
    return t;
}
DevHooks &dev_hooks() {
    static DevHooks h;
    return h;
}

}  // namespace halo
