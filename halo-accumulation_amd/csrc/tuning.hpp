// Every environment switch of the library in ONE place, read ONCE (the first call of tuning()), plus the hooks of the
// development library.  INTEGRATION.md section 6 documents the same list for the user.
//
//   * None of the switches changes a result: they size or schedule work whose result the GPU suite holds bit-equal, or print.
//   * The product library (libhalo_hip.so) reads NO fault injector from the environment.  DevHooks are plain fields that only
//     libhalo_hip_dev.so's halo_dev_hook() writes (include/halo_accumulation_dev.h): a process that does not load and call the
//     development library cannot be made to fail or to take a test path by a stray variable.
#pragma once
#include <cstddef>

namespace halo {

// most blocks of k_poly_eval_partial and k_dot2_partial (fr_plan.hpp): their partial records end below the result slot at 8 * 1024
// words; the range of HALO_DOT_BLOCKS and of the hooks "dot_blocks" / "poly_blocks"
constexpr int FR_GRID_CAP = 1024;

struct Tuning {
    // ---- operator-facing
    bool trace = false;            // HALO_TRACE=1          log allocations (address ranges), graph captures and replays to stderr
    bool ipa_timing = false;       // HALO_IPA_TIMING=1     print where the host side of the IPA rounds went when a state is destroyed
    bool memory_budget_set = false;
    size_t memory_budget = 0;      // HALO_MEMORY_BUDGET=48G  optional-memory budget per device for hosts that cannot call halo_set_memory_budget
    int graphs = -1;               // HALO_GRAPHS=0         never replay launch graphs (default: on; halo_set_graphs overrides)
    int fold_async = -2;           // HALO_FOLD_ASYNC=-1|0|1  folds beside the rounds: automatic / never / wherever possible (halo_set_fold_async)
    bool host_split_set = false;   // HALO_HOST_SPLIT="4,12"  a host-scalar halo_msm runs as stretches of these many sixteenths of its points, each behind
    int host_pieces = 2;           //   the copy of its own scalars (at most 4 entries, sum 16; "16": one copy in front of one launch sequence).  Unset:
    int host_split[4] = {4, 12, 0, 0};  //   4,12 below 2^21 points, 2,4,4,6 from there on (msm_entry.hip host_split_for: measured, HISTORY.md)
    int fold_table_after = 8;      // HALO_FOLD_TABLE_AFTER=k  automatic mode builds the fold table after k full-size opens on a key (0: never automatically)
    int spin_us = 50;              // HALO_SPIN_US          how long msm_wait polls before it starts yielding the core
    // ---- the launch plan of the Fr kernels (fr_plan.hpp; the Fr-plan suites assert the refusal and the clamp)
    int pow_e = 0;                 // HALO_POW_E=4..64      chain length of k_powers / k_h_coeffs (power of two)
    int dot_blocks = 0;            // HALO_DOT_BLOCKS=1..1024  block cap of k_dot2_partial (default 512; clamped: its partial records end at 8 * 1024 words)
};
const Tuning &tuning();

// Fault injectors and test paths: zero unless the development library sets them.
struct DevHooks {
    int table_fail = 0;        // "table_fail"       the allocation of a fixed-base / fold table reports out-of-memory
    int force_peer_copy = 0;   // "force_peer_copy"  multi-device contexts stage device scalars through a peer copy even on the same GPU
    int shard_fail_rank = -1;  // "shard_fail_rank" / "shard_fail_at": that rank fails locally before its collective number `at`
    int shard_fail_at = -1;    //   (at = -2: in a sharded check, -3: before a sharded MSM's collective)
    int batch_stage_fail = 0;  // "batch_stage_fail"   the staging of the check and open batches is refused: one member at a time
    int check_group = 0;       // "check_batch_group"  members per MSM launch of halo_pcdl_check_batch (1..8; 0: the measured default)
    int open_group = 0;        // "open_batch_group"   members per launch of halo_pcdl_open_batch (1..4; 0: the measured default)
    int open_fold = 0;         // "open_batch_fold"    the open batches above the no-fold size: 1 the folded schedule wherever it applies, 2 the loop (0: the measured default)
    int commit_group = 0;      // "commit_batch_group" members per MSM launch of halo_pcdl_commit_batch / _dev_batch (1..8; 0: the rule of the check batch)
    int combined_parts = 0;    // "check_combined_parts" parts the polynomials of a combined check's scalars are cut into (>= 1, clamped to the members; 0: a wave per SIMD)
    int combined_cap = 0;      // "check_combined_cap"   tables per pass of those scalars (>= 1; 0: the default)
    int combined_usum = 0;     // "check_combined_usum"  the right side sum r_a U_a of a combined check: 1 the host pool, 2 the device (0: by the member count)
    int fused_chunk = 0;       // "check_fused_chunk"    terms per MSM of a fused check's left side (>= 8, clamped to the context's capacity; 0: the capacity)
    int verifier_min = 0;      // "verifier_batch_min" relations from which halo_acc_verifier_batch launches (>= 1; 0: the measured default)
    long transcript_min = 0;   // "transcript_min"     members from which a batched check's transcripts run on the device (>= 1; 0: the measured default)
    long slide_min = 0;        // "table_slide_min"    keys from this many points take the c = 20 table plans and the all-shifts table (>= 4096; 0: 2^20)
    long decode_min = 0;       // "decode_batch_min"   finite points from which halo_*_decode_batch decompresses on the device (>= 1; 0: the measured default)
    // the launch plan of the Fr kernels (fr_plan.hpp), each before the environment's value and the measured default; 0: not set
    int pow_e = 0;             // "pow_e"        chain length of k_powers / k_poly_eval_partial / k_h_coeffs / k_h_accumulate_batch (a power of two in [4, 64])
    int dot_blocks = 0;        // "dot_blocks"   block cap of k_dot2_partial (1..1024)
    int poly_blocks = 0;       // "poly_blocks"  block cap of k_poly_eval_partial (1..1024; the batched open: at most OPEN_PART_WORDS / 4 of them)
};
DevHooks &dev_hooks();

inline bool debug_trace() { return tuning().trace; }

}  // namespace halo
