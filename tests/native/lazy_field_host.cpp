// The lazy radix-2^29 fields and the group law of the GPU kernels (csrc/fq29.hpp, fr29.hpp, curve.hpp), compiled for the CPU:
// HALO_DEV becomes `inline` and the register pins (HALO_PIN_VGPR) vanish, everything else is the text the device compiler
// sees.  Built with -fsanitize=address,undefined by tests/test_host_sanitizers.py, which writes the cases and checks the
// results against Python big integers; the GPU test compares what the device computes with this program's output limb for
// limb.  No HIP call is made: the HIP headers are included for their types (uint4, make_uint4).
//
//   lazy_field_host <cases> <results>
//
// <cases>: blocks of three 32-bit words (kind: 0 field, 1 point; operation number of csrc/dev_lazy_ops.hpp; number of cases)
// followed by the operands (field: 40 words per case; point: 40 words per case of the first operand, then 40 per case of the
// second).  <results>: the raw results block after block (field: 10 words per case; point: 40).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define HALO_DEV inline
#define HALO_PIN_VGPR(x) ((void)(x))
#include <hip/hip_runtime.h>
static inline int __shfl(int v, int, int) { return v; }  // the cross-lane moves of curve.hpp are not exercised here

#include "dev_lazy_ops.hpp"

static uint32_t *aligned_words(size_t n) {
    void *p = nullptr;
    if (posix_memalign(&p, 16, (n ? n : 1) * 4 + 16)) { fprintf(stderr, "out of memory\n"); exit(2); }
    memset(p, 0, (n ? n : 1) * 4 + 16);
    return static_cast<uint32_t *>(p);
}

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s <cases> <results>\n", argv[0]); return 2; }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open files\n"); return 2; }
    size_t blocks = 0, cases = 0;
    uint32_t head[3];
    while (fread(head, 4, 3, in) == 3) {
        const uint32_t kind = head[0], op = head[1], n = head[2];
        if (kind > 1 || n > (1u << 22)) { fprintf(stderr, "bad block header\n"); return 2; }
        const size_t in_words = kind == 0 ? (size_t)n * halo::LAZY_FIELD_IN : (size_t)n * 2 * halo::LAZY_POINT_WORDS;
        const size_t out_words = kind == 0 ? (size_t)n * halo::LAZY_SLOT : (size_t)n * halo::LAZY_POINT_WORDS;
        uint32_t *a = aligned_words(in_words), *o = aligned_words(out_words);
        if (fread(a, 4, in_words, in) != in_words) { fprintf(stderr, "short block\n"); return 2; }
        const uint32_t *b = a + (size_t)n * halo::LAZY_POINT_WORDS;
        for (size_t i = 0; i < n; i++) {
            bool known = kind == 0 ? halo::lazy_field_op((int)op, a + i * halo::LAZY_FIELD_IN, o + i * halo::LAZY_SLOT)
                                   : halo::lazy_point_op((int)op, a + i * halo::LAZY_POINT_WORDS, b + i * halo::LAZY_POINT_WORDS,
                                                         o + i * halo::LAZY_POINT_WORDS);
            if (!known) { fprintf(stderr, "unknown operation %u of kind %u\n", op, kind); return 2; }
        }
        if (fwrite(o, 4, out_words, out) != out_words) { fprintf(stderr, "write failed\n"); return 2; }
        free(a);
        free(o);
        blocks++;
        cases += n;
    }
    fclose(in);
    if (fclose(out)) { fprintf(stderr, "write failed\n"); return 2; }
    printf("ok %zu blocks %zu cases\n", blocks, cases);
    return 0;
}
