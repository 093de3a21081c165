/* Development interface of the MI355X MSM / IPA library: libhalo_hip_dev.so (csrc/dev.hip).
 *
 * NOT part of the drop-in boundary (include/halo_accumulation.h, libhalo_hip.so): a production host neither links nor loads
 * this library.  It links against libhalo_hip.so (one copy of the library's state per process) and adds
 *   - the per-context experiment knobs behind the measurements of DESIGN.md / HISTORY.md (every setting gives bit-identical
 *     results; the GPU suite holds them against each other),
 *   - the primitive test hooks of tests/test_gpu_parity.py (one field / group operation per lane),
 *   - halo_bench_fr_kernel for the profiler,
 *   - halo_dev_hook: fault injectors and forced test paths.  The product library has no other way to switch them on: it reads
 *     no HALO_TEST_* variable (csrc/tuning.hpp).
 */
#ifndef HALO_ACCUMULATION_DEV_H
#define HALO_ACCUMULATION_DEV_H
#include "halo_accumulation.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Fault injectors / forced paths, process-wide.  name: "table_fail" (value != 0: the allocation of a fixed-base or fold table
 * reports out-of-memory), "force_peer_copy" (multi-device contexts stage device scalars through a peer copy even on one GPU),
 * "shard_fail_rank" + "shard_fail_at" (the rank with that offset fails locally before collective number `at` of a sharded open:
 * 0 = the share of p(z), 1.. = the rounds, then the tail; at = -2: in a sharded check; at = -3: the rank with that `rank`
 * before the collective of halo_msm_sharded / _dev_sharded / _end_sharded), "batch_stage_fail" (value != 0: the staging of
 * halo_pcdl_check_batch / halo_acc_decider_batch / halo_pcdl_open_batch / halo_random_instance_batch / halo_acc_prover_batch /
 * halo_pcdl_commit_batch / halo_pcdl_commit_dev_batch / halo_instance_from_poly_batch is refused, as over the
 * memory budget: one member at a time; halo_acc_verifier_batch: its sums on the host pool), "check_batch_group" (members per MSM launch of the check batch, 1..8; 0: the measured
 * default), "open_batch_group" (members per launch of the open and prover batches and of halo_instance_from_poly_batch, 1..4; 0: the
 * measured default), "open_batch_fold" (halo_pcdl_open_batch / halo_random_instance_batch / halo_instance_from_poly_batch above the
 * no-fold size: 0 the measured default, 1 the folded schedule with member-batched key folds wherever it applies, 2 never: one member
 * at a time; another value is HALO_E_ARG), "commit_batch_group" (members per MSM launch of halo_pcdl_commit_batch / halo_pcdl_commit_dev_batch, 1..8; 0: the
 * rule of the check batch), "verifier_batch_min" (relations
 * from which halo_acc_verifier_batch runs its sums on the device, >= 1; 0: the measured default), "transcript_min" (members from
 * which the batched checks -- halo_pcdl_succinct_check_batch, halo_pcdl_check_batch and its _combined and _fused forms, the
 * halo_acc_decider_batch calls, the succinct half of halo_acc_prover_batch -- run their Fiat-Shamir transcripts on the device,
 * >= 1; 0: the measured default; a negative value is HALO_E_ARG; "batch_stage_fail" refuses its staging too: the host pool;
 * codes, statuses, messages and outputs are the same under every value), "table_slide_min" (keys from this many points, >= 4096, take the c = 20 table plans and
 * the all-shifts table with its sliding-window recode; 0: 2^20), "decode_batch_min" (finite points
 * from which halo_*_decode_batch decompresses on the device, >= 1; 0: the measured default; "batch_stage_fail" refuses its staging
 * too: the host pool), "check_combined_parts" (parts the polynomials of halo_pcdl_check_batch_combined's
 * scalars are cut into, >= 1, clamped to the accepted members; 0: a wave per SIMD), "check_combined_cap" (their tables per pass, >= 1;
 * 0: the default) -- the scalars are the same words under every value of the two; the mixed combined and the mixed fused calls read both hooks too --, "check_combined_usum" (the right side
 * sum r_a U_a of a combined check: 1 the host pool, 2 the device where a second slot is idle; 0: by the member count; another
 * value is HALO_E_ARG; "batch_stage_fail" makes the combined and the fused calls, the mixed ones included, take the exact path), "check_fused_chunk" (terms per
 * MSM of the left side of halo_pcdl_check_batch_fused and of halo_pcdl_check_batch_mixed_fused: at least 8, clamped to the context's size; 0: that size; 1..7 or a negative
 * value is HALO_E_ARG -- the statuses are the same under every value), "reset" (all off).
 * The launch plan of the Fr kernels (csrc/fr_plan.hpp), each taken before the environment's value and the measured default, every
 * plan giving the same field elements: "pow_e" (elements per lane of k_powers, k_poly_eval_partial, k_h_coeffs and
 * k_h_accumulate_batch and of their batch forms: a power of two in [4, 64], the rule of HALO_POW_E), "dot_blocks" (block cap of
 * k_dot2_partial, 1..1024: its partial records end below the result slot at 8 * 1024 words; the batched open clamps to its own
 * room), "poly_blocks" (block cap of k_poly_eval_partial, 1..1024; the batched open takes at most 256 of them: with fewer blocks
 * than waves of 64 E coefficients the waves stride over the polynomial).  A value outside its range is HALO_E_ARG with the rule in
 * halo_last_error and leaves the hook as it was; "reset" clears them. */
int halo_dev_hook(const char *name, long value);
/* Host only: the plan one Fr launcher computes at size n NOW (hooks, environment, defaults), from the very functions the launcher
 * calls: out = { E, nwin, blocks, trips }.  which = 0 halo_powers (k_powers; E elements per lane, nwin 4-bit windows of the
 * exponent, trips 1), 1 halo_poly_eval (k_poly_eval_partial; trips = passes of a wave through its grid-stride loop), 2
 * halo_scalar_dot and the rounds' dot products over n elements per vector (k_dot2_partial; E = 2 elements per lane and trip, nwin 0,
 * trips = the most passes of a lane), 3 halo_h_coeffs / halo_h_accumulate and their batch forms over n = 2^lg_n coefficients
 * (nwin = the 256-entry tables low, mid, high with more than one entry, trips 1), 4 the p(z) of halo_pcdl_open_batch
 * (k_poly_eval_partial_batch and its window table: as 1, but at most 256 blocks per member, the room of its partial records; 1
 * is the plan of halo_poly_eval and of a single open, up to 1024 blocks).  ctx may be NULL: no plan depends on the context.
 * HALO_E_ARG: another `which`, a null `out`. */
int halo_dev_fr_plan(halo_ctx *ctx, int which, size_t n, long out[4]);
/* The two dot products of an IPA round on their own (k_dot2_partial over both pairs of vectors, one launch): c, z = 2 m x 4
 * Montgomery words, out = <c[m..2m), z[0..m)> | <c[0..m), z[m..2m)>.  Any m with 2 m <= the context's size (64 at least) -- the
 * rounds themselves only ever reach powers of two; m = 0 gives zeros. */
int halo_dev_dot2_cross(halo_ctx *ctx, const uint64_t *c, const uint64_t *z, size_t m, uint64_t out[8]);
/* What the library read from the environment at its first use (csrc/tuning.hip), by field: "host_split_set", "host_pieces", "host_split0".."host_split3",
 * "fold_table_after", "pow_e", "dot_blocks", "spin_us", "graphs", "memory_budget" (MiB, -1 unset), "trace"; -1 for an
 * unknown name.  Also "commit_batch_group", "open_batch_fold" and "transcript_min": those hooks of halo_dev_hook as they stand now (0 after "reset").
 * Host only. */
long halo_dev_tuning(const char *name);

/* `reps` back-to-back launches of one bandwidth-side Fr kernel over n elements of the context's scratch memory (no host
 * round trip in between): which = 0 k_powers, 1 k_poly_eval_partial, 2 k_dot2_partial (one pair of vectors), 3 k_dot2_partial
 * (the two pairs of an IPA round, m = n / 2), 4 k_h_coeffs, 5 k_fold_scalars (m = n / 2), 6 k_axpy.  For rocprofv3 / the
 * event profiler: steady-state kernel durations, the figures of bench.py's hbm_kernels block. */
int halo_bench_fr_kernel(halo_ctx *ctx, int which, size_t n, int reps);

/* The batched h expansion of halo_pcdl_check_batch (k_h_tables + k_h_coeffs_batch) on its own: xis = m x (lg_n + 1) x 4
 * Montgomery words, out = m x 2^lg_n x 4 words; member b's block equals halo_h_coeffs(xis_b, lg_n).  2^lg_n <= the context's
 * size (64 at least). */
int halo_dev_h_coeffs_batch(halo_ctx *ctx, const uint64_t *xis, size_t m, size_t lg_n, uint64_t *out);

/* The prover batch's accumulated polynomials (k_h_tables with scales + k_h_accumulate_batch) on their own: member j of `members`
 * has counts[j] polynomials h_i (0 allowed), given one after the other in xis ((lg_n + 1) x 4 Montgomery words each) and alphas
 * (their scales, 4 words each), and h0s[8 j ..] = its two h_0 coefficients.  out = members x 2^lg_n x 4 words: member j's block is
 * h_0 + sum_i alphas_i h_i(X).  max_tables: polynomials per pass (0: all in one pass; fewer than a member brings: the later
 * passes add to what is there).  1 <= lg_n, 2^lg_n <= the context's size (64 at least). */
int halo_dev_h_accumulate_batch(halo_ctx *ctx, const uint64_t *h0s, const uint64_t *xis, const uint64_t *alphas, const size_t *counts,
                                size_t members, size_t lg_n, size_t max_tables, uint64_t *out);

/* The weights of halo_pcdl_check_batch_combined / halo_acc_decider_batch_combined (the rule: include/halo_accumulation.h) for
 * the A accepted members idx[0 .. A) of the blobs at stride_words, degree bound d, seed = 32 bytes or NULL: out = A x 4
 * Montgomery words.  Host only, no context.  HALO_E_ARG: a null pointer, d + 1 not a power of two, stride_words below
 * halo_instance_words(lg(d + 1)). */
int halo_dev_check_weights(const uint64_t *blobs, size_t stride_words, const size_t *idx, size_t A, size_t d, const uint8_t seed[32] /*nullable*/,
                           uint64_t *out);
/* The scalar step of the combined check on its own (k_h_tables with scales, k_h_accumulate_batch over the parts, k_fr_sum_rows):
 * xis = A x (lg_n + 1) x 4 and weights = A x 4 Montgomery words, out = 2^lg_n x 4 words = sum_a weights_a h_a(X), canonical.  Parts
 * and tables per pass are the product's (the hooks "check_combined_parts" / "check_combined_cap" first).  1 <= A <= 65535,
 * 1 <= lg_n, 2^lg_n <= the context's size (64 at least); temporary device buffers of this call only. */
int halo_dev_check_combined_scalars(halo_ctx *ctx, const uint64_t *xis, const uint64_t *weights, size_t A, size_t lg_n, uint64_t *out);
/* The weights of halo_pcdl_check_batch_mixed_combined / halo_acc_decider_batch_mixed_combined (the mixed rule of
 * include/halo_accumulation.h) for the A accepted members idx[0 .. A) of a call whose member i is the blob blobs[i] of degree bound
 * ds[i], seed = 32 bytes or NULL: out = A x 4 Montgomery words.  Host only, no context.  HALO_E_ARG: a null pointer, a null
 * blobs[idx[a]], some ds[idx[a]] + 1 not a power of two. */
int halo_dev_check_mixed_weights(const uint64_t *const *blobs, const size_t *ds, const size_t *idx, size_t A, const uint8_t seed[32] /*nullable*/,
                                 uint64_t *out);
/* The scalar step of the mixed combined check on its own (k_h_tables_mixed, k_h_accumulate_mixed over the parts, k_fr_sum_rows): A
 * polynomials in the CALLER's order, polynomial a of 2^lgs[a] coefficients (the launcher sorts them by decreasing length).  With
 * lg_max = the largest lgs[a]: xis = A records at the fixed stride of (lg_max + 1) x 4 Montgomery words, record a's first lgs[a] + 1
 * elements its challenges (the rest is not read); weights = A x 4; out = 2^lg_max x 4 words, out[k] = the sum of weights_a h_a[k]
 * over the a with k < 2^lgs[a], canonical.  Parts and tables per pass as in halo_dev_check_combined_scalars, for 2^lg_max
 * coefficients.  1 <= A <= 65535, 1 <= lgs[a], 2^lg_max <= the context's size (64 at least); temporary device buffers of this call
 * only. */
int halo_dev_check_mixed_scalars(halo_ctx *ctx, const uint64_t *xis, const size_t *lgs, const uint64_t *weights, size_t A, uint64_t *out);
/* The weights of halo_pcdl_check_batch_fused / halo_acc_decider_batch_fused (the fused rule of include/halo_accumulation.h),
 * arguments as halo_dev_check_weights: out = 2 A x 4 Montgomery words, r_0 | s_0 | r_1 | s_1 | ..  Host only, no context. */
int halo_dev_check_fused_weights(const uint64_t *blobs, size_t stride_words, const size_t *idx, size_t A, size_t d,
                                 const uint8_t seed[32] /*nullable*/, uint64_t *out);
/* The term kernel of the fused check on its own (k_fused_terms, then the sum of H's shares: k_fr_sum_rows): recs = M records of
 * lg_n + 6 elements of 4 Montgomery words (xi_0 .. xi_lg | z | v | c | r | s); scalars_out = M x (2 lg_n + 2) x 4 words, member a's
 * scalars r | r xi_1^-1 .. r xi_lg^-1 | r xi_1 .. r xi_lg | s - r c as canonical integers below the group order (NOT Montgomery: what
 * the left side's MSM reads); h_out = sum_a r_a (v_a - c_a h_a(z_a)) xi_a,0 likewise.  1 <= M <= 65535, 1 <= lg_n <= 24; a zero
 * challenge gives zeros for its inverses.  Temporary device buffers of this call only. */
int halo_dev_check_fused_terms(halo_ctx *ctx, const uint64_t *recs, size_t M, size_t lg_n, uint64_t *scalars_out, uint64_t h_out[4]);
/* The weights of halo_pcdl_check_batch_mixed_fused / halo_acc_decider_batch_mixed_fused (the mixed fused rule of
 * include/halo_accumulation.h), arguments and errors as halo_dev_check_mixed_weights: out = 2 A x 4 Montgomery words, r_0 | s_0 |
 * r_1 | s_1 | ..  Host only, no context. */
int halo_dev_check_mixed_fused_weights(const uint64_t *const *blobs, const size_t *ds, const size_t *idx, size_t A,
                                       const uint8_t seed[32] /*nullable*/, uint64_t *out);
/* The term kernel of the mixed fused check on its own (k_mixed_terms, then the sum of H's shares: k_fr_sum_rows): M members of their
 * own sizes lgs[a].  recs = their records one behind the other, member a's of lgs[a] + 6 elements laid out as for
 * halo_dev_check_fused_terms; scalars_out = their scalars one behind the other, (2 lgs[a] + 2) x 4 words for member a, canonical;
 * h_out = the sum of their shares of H's scalar.  The descriptors (offsets as prefix sums) are the product's.  1 <= M <= 65535,
 * 1 <= lgs[a] <= 24, no null pointer: else HALO_E_ARG.  Temporary device buffers of this call only. */
int halo_dev_check_mixed_terms(halo_ctx *ctx, const uint64_t *recs, const size_t *lgs, size_t M, uint64_t *scalars_out, uint64_t h_out[4]);

/* replay cached hipGraphs of the MSM launch sequence when the same shape repeats (default on) */
int halo_set_graphs(halo_ctx *ctx, int on);  /* also: environment HALO_GRAPHS=0 at context creation; HALO_TRACE=1 logs every launch */

/* IPA tuning: key size at which halo_ipa_* stops folding G and switches to MSMs over the fixed
 * folded key (default 2^14; 0 or 1 = always fold).  Results are identical either way. */
int halo_set_ipa_switch(halo_ctx *ctx, size_t size);

/* IPA tuning: 2 (default) folds G every other round, two halvings at once with one shared doubling chain, the rounds in
 * between taking L, R from MSMs over the unfolded key; 1 folds G every round.  Results are identical either way. */
int halo_set_fold_levels(halo_ctx *ctx, int levels);

/* IPA tuning: a two-level fold of a key of at most 2^18 points (a latency chain on one wave per SIMD) can run on the context's
 * fourth stream BESIDE the next two rounds, which then take their L, R from the key it reads.  -1 (default): in opens of at
 * most 2^18 points, where it pays (9.3 -> 9.0 ms at 2^18; at 2^20 the rounds over the larger key lose more than the hidden
 * fold returns: 15.7 -> 16.4 ms); 0: every fold in line; 1: wherever possible.  Environment
 * HALO_FOLD_ASYNC=-1/0/1 at context creation.  Results are identical either way. */
int halo_set_fold_async(halo_ctx *ctx, int mode);

/* verifier tuning: 1 (default) = succinct checks of >= 64 instances on the device, 0 = always the host thread pool */
int halo_set_batch_verify(halo_ctx *ctx, int on);

/* MSM tuning: window bits (0 = automatic) */
int halo_set_window_bits(halo_ctx *ctx, int c);

/* MSM tuning: buckets per lane in the window-sum kernel (0 = automatic, else a power of two) */
int halo_set_reduce_span(halo_ctx *ctx, int span);

/* MSM tuning: bucket sort in one pass (0), in two (coarse runs, then a fine sort per run: 1, where the shape allows),
 * or chosen by size (-1, default: two levels from n = 2^17) */
int halo_set_sort_mode(halo_ctx *ctx, int mode);

/* MSM tuning: the 4-launch pipeline for MSMs of up to 2^16 points (sort per window in LDS, quad-parallel window sums):
 * -1 automatic (default), 0 never (the general pipeline at every size).  Results are identical. */
int halo_set_small_path(halo_ctx *ctx, int mode);

/* MSM tuning: longest chain of mixed additions one lane runs in the bucket kernel (0 = automatic; 8, 16, 32, 64) */
int halo_set_task_len(halo_ctx *ctx, int len);

/* The verifier batch's segmented small MSM (k_small_msm_seg) on its own, in one launch: nsums sums, sum s of lens[s] in 1..64
 * terms; points = the terms' arkworks affine points (8 words, (0, 0) = infinity), scalars = their canonical scalars (4 words),
 * sum after sum; out_jac = nsums x 12 Jacobian words */
int halo_dev_small_msm_seg(halo_ctx *ctx, const uint64_t *points, const uint64_t *scalars, const size_t *lens, size_t nsums,
                           uint64_t *out_jac);

/* The relation kernel of the device-side succinct checks (k_batch_small_msm) on its own, in one launch through the product's
 * batch_small_msm: m sums of K terms each, one wave per sum; points = m x K x 8 words (arkworks affine, (0, 0) = infinity),
 * scalars = m x K x 4 canonical words, out_jac = m x 12 Jacobian words.  m = 0 is HALO_OK.  HALO_E_ARG: a null pointer, m above
 * 65535, K outside 1..64 (the product's message). */
int halo_dev_batch_small_msm(halo_ctx *ctx, const uint64_t *points, const uint64_t *scalars, size_t m, size_t K, uint64_t *out_jac);

/* The transcripts of pcdl::succinct_check (pcdl.rs:272-296) for m Instance blobs of degree bound d on their own, no relation:
 * on_device = 0 on the host pool, as every single call runs them; on_device != 0 through the device route of the batched checks
 * (k_transcript_points, k_transcript_head, k_batch_small_msm with K = 3, k_transcript_chain) whatever "transcript_min" says.
 * xis_out = m x (lg + 1) x 4 Montgomery words (xi_0 .. xi_lg), cprime_out = m x 12 words (C', normalised), both zero in the rows
 * of a rejected member; status_out[i] = 0 accepted, 1 the instance holds an invalid point or scalar, 2 the proof does, 3 a challenge
 * is zero, 4 the member's d or proof length does not fit d.  A member with a point that is not normalised (Z neither 0 nor 1) is
 * finished on the host pool before the call returns.  m = 0 is HALO_OK.  HALO_E_ARG: a null pointer, d + 1 not a power of two;
 * HALO_E_DEVICE: on_device and the staging refused ("batch_stage_fail", the memory budget). */
int halo_dev_transcripts(halo_ctx *ctx, size_t d, const uint64_t *instances, size_t m, int on_device, uint64_t *xis_out, uint64_t *cprime_out,
                         int *status_out);

/* halo_msm_points' normalisation on its own: upload, the product's batch_to_affine (k_batch_to_affine: four points per lane, one
 * shared inversion), k_native_to_aff, download.  pts_jac = m x 12 arkworks Jacobian words (any Z; Z = 0 is infinity whatever X
 * and Y hold), out_affine = m x 8 affine words, (0, 0) = infinity.  m = 0 is HALO_OK.  HALO_E_ARG: a null pointer, m above 2^22. */
int halo_dev_batch_to_affine(halo_ctx *ctx, const uint64_t *pts_jac, size_t m, uint64_t *out_affine);

/* One point fold of pcdl::open's halving loop on its own, through the product's launcher: out[j] = G[j] + xi G[j+m] (levels 1,
 * m = n / 2) or G[j] + s1 G[j+m] + s2 G[j+2m] + s3 G[j+3m] (levels 2, m = n / 4; two rounds xi1, xi2 are (s1, s2, s3) =
 * (xi2, xi1, xi1 xi2)).  key_affine = n x 8 words, (0, 0) = infinity -- any points, m may be odd -- or NULL: the first n points of
 * the context's own key.  scalars: xi, or s1 | s2 | s3, Montgomery words.  The path is upload, k_aff_to_native, ipa_fold_points /
 * ipa_fold_points4, k_native_to_aff, download; out_affine = m x 8 words.
 * form picks the kernel form whatever m is: 0 = what the product chooses at this m; 1 = one output per lane; 2 = two outputs per
 * lane (j and j + (m + 1) / 2, one shared inversion); 3 = one output per quad (levels 2); 4 / 5 = the comb-table kernel with one /
 * two outputs per lane (levels 2, key_affine == NULL, n = the context's size >= 64; the table is built as halo_set_fold_table(ctx,
 * 1) would at the next open, and released again if the context's mode is 0).
 * in_place != 0 (levels 2): destination == source (a lane reads j + t m and writes j); the table kernel never allows it.  The
 * one-level kernel always folds in place: in a copy of the key.  The context's own key is never written.
 * HALO_E_ARG: n not a positive multiple of 2 levels (or above 2^24, or above the context's size with NULL), levels not 1 / 2, a
 * form the levels do not have, a table form with a foreign key, another size or in_place. */
int halo_dev_fold_points(halo_ctx *ctx, const uint64_t *key_affine, size_t n, int levels, const uint64_t *scalars, int form, int in_place,
                         uint64_t *out_affine);

/* The member-batched key folds of the open batches (k_fold_points_batch, k_fold_points4_batch, k_fold_points4_quad_batch: blockIdx.y =
 * member, each member's digits in a record in device memory) on their own, through the product's launchers ipa_fold_points_batch /
 * ipa_fold_points4_batch: `members` (1 .. 4) folds in ONE launch, member b's result -- out_affine + b * m * 8 words -- the one
 * halo_dev_fold_points gives for its key and its scalars.  scalars: members x (xi | s1 s2 s3) x 4 Montgomery words.
 * key_affine = NULL: the first n points of the context's own key, read by every member (shared must be non-zero); else n x 8 words
 * read by every member (shared != 0), or members x n x 8 words, member b's key at b * n points (shared == 0).  A shared source is
 * folded into a destination of members x m points; per-member sources are folded in place, as the open batch folds its staged keys.
 * The context's own key is never written.  form: 0 = the launchers' rule over all members x m outputs; 1 / 2 = one / two outputs per
 * lane; 3 = one output per quad (levels 2).  n, levels and the null checks as for halo_dev_fold_points; HALO_E_ARG also for members
 * outside 1 .. 4, a form the levels do not have, key_affine = NULL with shared == 0. */
int halo_dev_fold_points_batch(halo_ctx *ctx, const uint64_t *key_affine /*NULL: the context's key, shared*/, size_t n, int levels,
                               const uint64_t *scalars /*members x (1 | 3) x 4*/, int members /*1..4*/, int shared /*0: key_affine holds members x n points*/,
                               int form, uint64_t *out_affine /*members x m x 8*/);

/* One batched MSM launch sequence (msm_enqueue_batch) over the context's key with one base offset per member, on slot 0: member b
 * is sum_i scalars[b][i] * G[offs[b] + i], i < n -- what halo_msm(ctx, offs[b], n, scalars_b) gives, limb for limb.  Up to 2^16
 * points the members run through the small pipeline whatever their offsets (k_smsm_sort takes one per member).  HALO_E_ARG: count
 * outside 1 .. 8, a null pointer, a range that leaves the key, slot 0 busy. */
int halo_dev_msm_offsets(halo_ctx *ctx, const size_t *offs /*count entries, points*/, size_t n, const uint64_t *scalars /*host, count x n x 4*/,
                         int count /*1..8*/, int scalars_are_mont, uint64_t *out_jac /*count x 12*/);

/* One tagged launch (MsmBatch::tagged: the L and R of an open's first rounds over 2^20 points) over the key's points [off, off + n),
 * on slot 0, with scalars of the caller's choice: scalars = n x 4 canonical words whose bit 255 names the bucket set of point i, so
 * out_jac[12 t ..] = sum over the i with tag t of (scalars[i] mod 2^255) * G[off + i], t = 0, 1 -- what halo_msm gives for the
 * scalars of that tag with zeros elsewhere, limb for limb (normalised).  n = 0 gives two infinities.  The launch is the product's
 * msm_enqueue_batch with its own refusals and messages (no table yet -- the first table MSM builds it --, table mode 0, a forced
 * window size, the small-key plan, n no multiple of 4 or below the least table stretch).  HALO_E_ARG also: a null pointer, a
 * range that leaves the key, slot 0 busy. */
int halo_dev_msm_tagged(halo_ctx *ctx, size_t off, size_t n, const uint64_t *scalars /*host, n x 4, canonical, bit 255 = set*/,
                        uint64_t *out_jac /*2 x 12*/);

/* Entries [off, off + count) of row `row` of the context's MSM table (csrc/msm_table.hip: T[w][i] = 2^(c w) G_i for the 13 and 15
 * rows, T[j][i] = 2^j G_i for the 255) as arkworks affine words, count x 8, Montgomery form, (0, 0) = infinity: what
 * halo_ctx_read_bases gives for the key, through the same conversion.  It reads and waits for the context's stream; it builds
 * nothing.  HALO_E_ARG: the context has no table (its first table MSM builds it), row >= halo_ctx_info(ctx, 8), a range that
 * leaves the key, an MSM in flight on any slot. */
int halo_dev_table_read(halo_ctx *ctx, size_t row, size_t off, size_t count, uint64_t *out_affine);

/* Host only: the plan of the MSM launch enqueued last on `slot`, as the launch sequence noted it (MsmPlan: reported, not
 * recomputed; a graph replay reports the plan it was captured with).  out =
 *   [0] pipeline: 0 general, 1 small (smsm.hip), 2 table with fixed windows, 3 table sliding
 *   [1] c  [2] W  [3] B            window bits, windows, buckets per window (table plans: per set)
 *   [4] members  [5] sets          MSMs of the launch; bucket sets of a table launch (members rounded up to a power of two)
 *   [6] pieces                     consecutive pieces of a large table MSM
 *   [7] kmax                       longest chain of the bucket kernel: a bucket of more entries is several tasks
 *   [8] window-sum form: 0 k_msm_reduce1 + k_smsm_final, 1 k_smsm_reduce (+ k_smsm_final beyond one segment), 2 k_msm_reduce_rc +
 *       k_rc_mid (every table launch)
 *   [9] L  [10] logL  [11] nseg  [12] live_seg    forms 0 and 1: buckets per lane (quad), segments per window, the final stage's width
 *   [13] form 2: lg_rows | lg_cols << 8 | per << 16 (rows x columns of the bucket index, buckets per lane); else 0
 *   [14] [15] 0 (not used)
 * A launch of no points, or a window shard without windows, reports W = 0.  HALO_E_ARG: a slot out of range, a slot in flight, no
 * launch on the slot yet (or its last one refused), a null `out`. */
int halo_dev_msm_last_plan(halo_ctx *ctx, int slot, long out[16]);
/* Host only: the records the last finished launch of `slot` left in the slot's pinned buffer, copied as they are -- 12-word Jacobian
 * points (X | Y | Z, Montgomery words, Z = 0: infinity), exactly what the host's combination (msm_combine_member) reads.  *count =
 * their number; by window-sum form of halo_dev_msm_last_plan:
 *   general and small pipeline   members x (w1 - w0) weighted sums sum_b (b + 1) B_b, [member][w]
 *   table (both pipelines)       per piece and set: the pairs (S, T) = (sum_Q E_Q, sum_Q (Q + 1) E_Q) of the 64-entry blocks of the
 *                                columns' plain sums C_lo (2^lg_cols / 64 pairs), then those of the rows' R_hi (2^lg_rows / 64 pairs)
 * HALO_E_ARG: a slot out of range, a slot in flight, no launch yet, a null pointer, cap_points below the number of records -- *count
 * is set in that case too. */
int halo_dev_msm_window_sums(halo_ctx *ctx, int slot, uint64_t *out_jac, size_t cap_points, size_t *count);

/* The decode batch's square root in Fq (the routine of k_point_decompress) on its own, one lane per element: a = m x 4
 * Montgomery words; ok_out[i] = 1 and root_out[i]^2 = a[i] if a[i] is a square, else ok_out[i] = 0 */
int halo_dev_fq_sqrt(halo_ctx *ctx, const uint64_t *a, size_t m, uint64_t *root_out, uint32_t *ok_out);
/* host only: that square root's torsion tables as the kernels get them, 8448 32-bit words: S[i][d] = g^(-d 2^(8 i) / 2) for
 * i < 4, d < 256 (S[0][d] = g^-(d >> 1); 8 Montgomery words each; g = 5^t, p - 1 = 2^32 t), then limb 0 of (g^(2^24))^d, d < 256 */
int halo_dev_sqrt_tables(uint32_t *out, size_t cap_words);

/* ---- primitive hooks used by the parity tests (elementwise over n) ----------------------- */
/* host-only: base-2 expansion of the fold scalar over the Eisenstein units (host_math.hpp glv_digits):
 * out[i] = digit code of 2^i (0 none, 1..3 = +lambda^0..2, 4..6 = -lambda^0..2), *n = number of digits */
int halo_test_glv_digits(const uint64_t xi[4], uint8_t out[144], int *n);
/* host-only: the comb digits of the table fold (foldtab.hip): s = k1 + k2 lambda, out[0..22) = signed base-64 digits of k1
 * (each in [-32, 32]), out[22..44) = those of k2 */
int halo_test_fold_digits(const uint64_t s[4], int8_t out[44]);
int halo_test_field_op(halo_ctx *ctx, int field /*0 Fq, 1 Fr*/, int op /*0 mul,1 add,2 sub,3 inv,4 from_mont,5 to_mont*/,
                       const uint64_t *a, const uint64_t *b, size_t n, uint64_t *out);
/* op 0: jacobian(a) + jacobian(b) via XYZZ add; 1: a + affine b (mixed); 2: double a; 3: a * scalar b (4 limbs);
 * 4, 5, 6: the quad-parallel forms (curve_quad.cuh): a + b, 2a, a + b with every fourth b replaced by a */
int halo_test_point_op(halo_ctx *ctx, int op, const uint64_t *a_jac, const uint64_t *b, size_t n, uint64_t *out_jac);

/* ---- raw-limb hooks (csrc/dev_lazy_ops.hpp): one operation of the lazy radix-2^29 fields or of the group law per case, over
 * NATIVE operands whose limbs the caller chooses -- any representative below the declared bound K*p, which the word forms
 * above cannot produce.  The tables of operations and bounds are in csrc/dev_lazy_ops.hpp and tests/lazy_cases.py.
 * Field: in = n x 40 words (four operands of 9 limbs + pad), out = n x 10 words (raw limbs; a predicate is 0 / 1 in word 0;
 * an 8-word form uses words 0..7). */
int halo_test_lazy_field_op(halo_ctx *ctx, int op, const uint32_t *in, size_t n, uint32_t *out);
/* Point: a, b, out = n x 40 words each: XYZZ as x | y | zz | zzz, Jacobian as x | y | z, affine as x | y (10 words per
 * coordinate).  quad != 0: the quad-parallel form of curve_quad.hpp (operations 0 xyzz_add, 2 xyzz_dbl, 3 jac_madd, 4 jac_dbl),
 * one case per 4 lanes, neighbouring cases in one wave. */
int halo_test_lazy_point_op(halo_ctx *ctx, int op, int quad, const uint32_t *a, const uint32_t *b, size_t n, uint32_t *out);

#ifdef __cplusplus
}
#endif
#endif
