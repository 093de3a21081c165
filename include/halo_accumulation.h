/* halo_accumulation.h -- C ABI of the MI355X (gfx950) MSM / IPA hot path.
 *
 * Drop-in boundary for rasmus-kirk/halo-accumulation's `group.rs` function set plus the
 * fold loop of `pcdl::open`.  The reference has no FFI seam of its
 * own; each entry point below names the reference code (file:line under code/src/) that a
 * Rust shim would replace with a call to it (the shim is shown in INTEGRATION.md).
 *
 * Data conventions -- exactly what arkworks keeps in memory, so a shim passes `x.0.0`:
 *   scalar (Fr)   4 x u64, little-endian limbs, Montgomery form (R = 2^256)
 *   affine base   8 x u64 = x limbs | y limbs (Fq Montgomery).  (0,0) = point at infinity
 *   Jacobian pt  12 x u64 = X | Y | Z (Fq Montgomery), what `Projective::new_unchecked`
 *                takes (consts.rs:13-21).  Z = 0 = infinity.
 *   Every point WRITTEN by the library is normalised: (x, y, 1), or (1, 1, 0) for infinity,
 *   so outputs are bit-reproducible run to run.
 *
 * Errors: 0 = ok, negative = HALO_E_*; halo_last_error() returns a thread-local message.
 * A shim maps HALO_E_ASSERT to panic! (the reference's assert!, pcdl.rs:102-104,130-132,
 * pedersen.rs:7-12) and HALO_E_REJECT to anyhow::Error (its ensure!, pcdl.rs:261-262,
 * 307-310,339; acc.rs:152-155,169,237-240).
 *
 * Ownership: inputs are borrowed for the call; outputs go to caller buffers; only ctx / ipa
 * handles are library-owned.  A ctx is bound to one HIP device (halo_ctx_create_multi: one per shard) and its streams:
 * calls on the same ctx must not overlap; different ctxs are independent.  No global init.
 * There is NO CPU fallback: without a gfx950 device every compute entry point fails with
 * HALO_E_DEVICE.
 */
#ifndef HALO_ACCUMULATION_H
#define HALO_ACCUMULATION_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HALO_OK 0
#define HALO_E_ASSERT (-1) /* reference would panic (assert!) */
#define HALO_E_REJECT (-2) /* reference would return Err (ensure!) */
#define HALO_E_ARG (-3)    /* bad pointer / size for this library */
#define HALO_E_DEVICE (-4) /* HIP / RCCL failure, or no GPU */

typedef struct halo_ctx halo_ctx;
typedef struct halo_ipa halo_ipa;

const char *halo_last_error(void);
int halo_device_count(void);

/* ---- context: the commitment key, device resident (consts.rs:23-24,68: N, GS) ---------- */
/* Upload n affine bases (n x 8 limbs). */
int halo_ctx_create(int device, const uint64_t *bases_affine, size_t n, halo_ctx **out);
/* Derive G_i = [SHA3-256(genesis || LE64(first_index + i)) mod r] * (-1, 2) on the device
 * (main.rs:18-45; GS[i] of consts.rs is first_index = 2).  Hashing on host, scalar-mul in HIP. */
int halo_ctx_create_urs(int device, uint64_t first_index, size_t n, halo_ctx **out);
/* same with G_j = hash(first_index + j * stride): a rank's cyclic shard of the key (stride = world size) */
int halo_ctx_create_urs_strided(int device, uint64_t first_index, uint64_t stride, size_t n, halo_ctx **out);
/* Multi-device contexts (one process, n_dev GPUs of one node; a device id may repeat).  The handle is a full context on
 * devices[0] over the whole key -- every entry point works on it -- that also owns one shard context per device over that
 * device's index block of the key (block k = [k n / n_dev, (k + 1) n / n_dev), derived or uploaded once).  halo_msm,
 * halo_msm_dev, the begin/end halves of both and the library's own MSMs over the key (commit, check, h_commit) of at least
 * 2^16 points are cut along the block boundaries: each shard runs its stretch on its own device and stream, the partial
 * points are added on the host in block order -- the same normalised point as on one device.  Device-resident scalars
 * are read in place on their own GPU and copied peer-to-peer (xGMI) to the others; host scalars go to each device over its
 * own PCIe link.  halo_msm_dev_batch_begin/_end fan out the same way (every shard runs its stretch of all members as one batched
 * launch); the window-shard form (part / parts != 0 / 1) stays on devices[0]. */
int halo_ctx_create_multi(const int *devices, int n_dev, const uint64_t *bases_affine, size_t n, halo_ctx **out);
int halo_ctx_create_urs_multi(const int *devices, int n_dev, uint64_t first_index, size_t n, halo_ctx **out);
int halo_ctx_devices(const halo_ctx *ctx); /* shards of a multi-device context, 1 for a plain one */
/* A second context over the SAME resident key, for another host thread (the reference is single-threaded; a service that runs
 * several provers side by side is not): it shares `ctx`'s key and -- whichever of the contexts builds them -- the fixed-base MSM
 * table and the fold table (immutable, reference-counted: freed with the last context over the key), and owns its streams,
 * workspaces, scratch and IPA buffers: ~2.3 GB at 2^20 points instead of the 37 GB of an independent context with both
 * tables.  Contexts over one key are as independent as any two contexts: calls on ONE context must not overlap, calls on
 * different ones may (two open + check pairs in flight on a context and its clone: ~14 ms per pair against ~17 ms one at a time).  The
 * tuning knobs are copied at this moment.  Not for multi-device contexts.  halo_set_table_mode(ctx, 0) /
 * halo_set_fold_table(ctx, 0) on one of them stop THAT context's use of the table; the memory goes back when no context
 * over the key is left to use it. */
int halo_ctx_clone(halo_ctx *ctx, halo_ctx **out);
void halo_ctx_destroy(halo_ctx *ctx);
size_t halo_ctx_size(const halo_ctx *ctx);
/* copy bases [off, off+n) back to the host (n x 8 limbs) */
int halo_ctx_read_bases(halo_ctx *ctx, size_t off, size_t n, uint64_t *out_affine);
/* device pointer of the base table and the ctx's hipStream_t (for callers holding device memory) */
void *halo_ctx_bases_dev(halo_ctx *ctx);
void *halo_ctx_stream(halo_ctx *ctx);
/* S = hash(0), H = hash(1) of main.rs:35-45 as normalised Jacobian limbs (host computed) */
int halo_public_points(uint64_t S_out[12], uint64_t H_out[12]);

/* ---- group.rs ------------------------------------------------------------------------- */
/* point_dot_affine (group.rs:24-26): sum_i scalars[i] * GS[off + i], Pippenger in HIP.
 * scalars_are_mont = 1: arkworks' in-memory Fr (Montgomery limbs); 0: plain little-endian integers below 2^255
 * (canonical Fr values; an unreduced value in [r, 2^255) is taken as it is, which gives the same point).
 * `scalars` is host memory (pageable is fine) and is read only during the call.  Synchronous; over the context's fixed-base table
 * an MSM of >= 2^19 points runs as two index stretches on slots 0 and 1 (four on slots 0..3 from 2^21 points on), every later
 * stretch's copy under the earlier ones' kernels (these slots must be idle, else one copy + one launch sequence on slot 0; environment HALO_HOST_SPLIT). */
int halo_msm(halo_ctx *ctx, size_t off, size_t n, const uint64_t *scalars, int scalars_are_mont, uint64_t out_jac[12]);
/* Asynchronous halves of halo_msm (scalars in HOST memory): begin() copies the scalars to the device on the slot's own
 * stream and enqueues the launch sequence behind the copy, end() waits and combines.  With two or more slots a caller
 * overlaps the copy of the next MSM (32 MiB at n = 2^20: PCIe time) with the kernels of the current one.  The scalars must
 * stay untouched until end() returns, whatever memory they live in: begin() only ENQUEUES the copy (hipMemcpyAsync from
 * the caller's pointer; the runtime may pin a pageable range in place and DMA from it later rather than stage it). */
int halo_msm_begin(halo_ctx *ctx, int slot, size_t off, size_t n, const uint64_t *scalars, int scalars_are_mont);
int halo_msm_end(halo_ctx *ctx, int slot, uint64_t out_jac[12]);
/* same, scalars already in device memory (n x 4 limbs, 32-byte aligned device pointer) */
int halo_msm_dev(halo_ctx *ctx, size_t off, size_t n, const void *d_scalars, int scalars_are_mont, uint64_t out_jac[12]);
/* Asynchronous halves of halo_msm_dev, for overlapping independent MSMs: `slot` (0..3) selects
 * one of the context's four workspaces/streams (allocated on first use); begin() only enqueues, end() waits and combines.
 * At most one MSM per slot in flight; the scalars must stay untouched until end(). */
int halo_msm_dev_begin(halo_ctx *ctx, int slot, size_t off, size_t n, const void *d_scalars, int scalars_are_mont);
int halo_msm_dev_end(halo_ctx *ctx, int slot, uint64_t out_jac[12]);
/* Window shard `part` of `parts`: the same MSM restricted to the scalar windows [part*W/parts, (part+1)*W/parts)
 * of the W Pippenger windows, already weighted by its power of two -- the results of all parts (any order,
 * any GPU holding the same bases and scalars) add up to halo_msm_dev's point (halo_point_sum).  A GPU then
 * does 1/parts of the bucket work at the bucket efficiency of the full-size MSM, which index-sharding an
 * n <= 2^21 MSM does not.  end() is halo_msm_dev_end. */
int halo_msm_dev_begin_part(halo_ctx *ctx, int slot, size_t off, size_t n, const void *d_scalars, int scalars_are_mont, int part,
                            int parts);
/* Batched form: `batch` (1..8) independent MSMs over the same bases G[off .. off+n), one resident scalar
 * array each (d_scalars[b]), issued as ONE launch sequence on `slot`: the members' windows go through the
 * sort / bucket / window-sum kernels side by side, which fills the GPU where one launch alone is
 * latency-bound (a rank's window shard of a sharded MSM).  part/parts as in halo_msm_dev_begin_part (0, 1 =
 * whole MSMs).  end() writes batch x 12 limbs; member b's result is bit-identical to the unbatched call on
 * d_scalars[b].  The slot's workspace grows on first use. */
int halo_msm_dev_batch_begin(halo_ctx *ctx, int slot, size_t off, size_t n, const void *const *d_scalars, size_t batch,
                             int scalars_are_mont, int part, int parts);
int halo_msm_dev_batch_end(halo_ctx *ctx, int slot, size_t batch, uint64_t *out_jac);
/* point_dot (group.rs:18-21): arbitrary Jacobian points (m x 12 limbs); they are brought to
 * affine on the device (Montgomery batch inversion: one field inversion per four points; the reference runs m). */
int halo_msm_points(halo_ctx *ctx, const uint64_t *pts_jac, const uint64_t *scalars, size_t m, uint64_t out_jac[12]);
/* point_dot_affine (group.rs:24-26) for bases that are NOT a stretch of the context's key: pedersen::commit
 * (pedersen.rs:6-20) is public API over any `&[PallasAffine]`, and the reference's own test_homomorphism_property
 * (pedersen.rs:30-63) is free to pass other generators.  bases_affine = m x 8 limbs, uploaded for this call
 * ((0,0) = infinity); more generators than the context holds points run as consecutive chunks.  The general
 * (table-free) Pippenger pipeline runs. */
int halo_msm_affine(halo_ctx *ctx, const uint64_t *bases_affine, const uint64_t *scalars, size_t m, int scalars_are_mont,
                    uint64_t out_jac[12]);
/* scalar_dot (group.rs:13-15) */
int halo_scalar_dot(halo_ctx *ctx, const uint64_t *xs, const uint64_t *ys, size_t m, uint64_t out[4]);
/* construct_powers (group.rs:29-37): [1, z, ..., z^(n-1)] */
int halo_powers(halo_ctx *ctx, const uint64_t z[4], size_t n, uint64_t *out);
/* DensePolynomial::evaluate as called at pcdl.rs:135 */
int halo_poly_eval(halo_ctx *ctx, const uint64_t *coeffs, size_t len, const uint64_t z[4], uint64_t out[4]);

/* ---- pcdl.rs: h(X) -------------------------------------------------------------------- */
/* HPoly::get_poly().coeffs (pcdl.rs:56-77): 2^lg_n coefficients from xis[0..lg_n] (xis[0] unused) */
int halo_h_coeffs(halo_ctx *ctx, const uint64_t *xis, size_t lg_n, uint64_t *out);
/* pedersen::commit(None, GS[0..2^lg_n], h.get_poly().coeffs) of pcdl.rs:338, fused on device */
int halo_h_commit(halo_ctx *ctx, const uint64_t *xis, size_t lg_n, uint64_t out_jac[12]);
/* HPoly::eval (pcdl.rs:79-91) for m polynomials at one point (acc.rs:102-104) */
int halo_h_eval_batch(halo_ctx *ctx, const uint64_t *xis, size_t m, size_t lg_n, const uint64_t z[4], uint64_t *out);
/* AccumulatedHPolys::get_poly (acc.rs:85-94): out = h0 (2 coeffs) + sum_i alphas[i] * h_i(X) */
int halo_h_accumulate(halo_ctx *ctx, const uint64_t *h0, const uint64_t *xis, const uint64_t *alphas, size_t m,
                      size_t lg_n, uint64_t *out);

/* ---- pcdl.rs:183-231: the IPA halving loop, state device resident ------------------------ */
/* G = GS[0..n), c = coeffs zero-padded to n, z-powers of z (pcdl.rs:183-186) */
int halo_ipa_begin(halo_ctx *ctx, size_t n, const uint64_t *coeffs, size_t len, const uint64_t z[4], halo_ipa **out);
/* ---- sharded open: rank r of P holds the cyclic shard i = r (mod P) of G, c, z-powers ----
 * local state over n_local = n / P elements with z-vector z^(offset + j * stride) */
int halo_ipa_begin_strided(halo_ctx *ctx, size_t n_local, const uint64_t *coeffs_local, size_t len, const uint64_t z[4],
                           uint64_t stride, uint64_t offset, halo_ipa **out);
/* state from explicit c and z vectors (the last lg P rounds on the gathered P elements) */
int halo_ipa_begin_vectors(halo_ctx *ctx, size_t n, const uint64_t *c_vec, const uint64_t *z_vec, halo_ipa **out);
/* <c, z> of the current state (a shard's share of p(z) before the first round) */
int halo_ipa_dot_cz(halo_ipa *st, uint64_t out[4]);
/* this shard's <c_r, G_l>, <c_l, G_r> (no H' term) and dots = <c_r, z_l> | <c_l, z_r> */
int halo_ipa_round_lr_partial(halo_ipa *st, uint64_t L[12], uint64_t R[12], uint64_t dots[8]);
/* hiding branch (pcdl.rs:137-164): this shard's slice of p_bar = q (X - z), q = `deg` scalars of the stream
 * after rng_state, and its share of <p_bar, G> */
int halo_ipa_hiding_partial(halo_ipa *st, uint64_t rng_state, size_t deg, const uint64_t z[4], uint64_t stride, uint64_t offset,
                            uint64_t Cbar_part[12]);
/* c <- c + alpha p_bar on this shard */
int halo_ipa_apply_hiding(halo_ipa *st, const uint64_t alpha[4]);
/* host step of the hiding branch: C_bar, alpha, w', C' from the gathered parts; advances *rng_state past q and w_bar */
int halo_open_hiding_combine(const uint64_t C[12], const uint64_t z[4], const uint64_t *v_parts, const uint64_t *Cbar_parts, size_t P,
                             const uint64_t w[4], uint64_t *rng_state, size_t deg, uint64_t Cbar[12], uint64_t alpha[4],
                             uint64_t w_prime[4], uint64_t C_prime[12]);
/* halo_ipa_finish plus z[0] */
int halo_ipa_finish_z(halo_ipa *st, uint64_t U[12], uint64_t c[4], uint64_t z0[4]);
/* host steps between collectives: v = sum of the shards' <c, z>, xi_0 = rho_0(C, z, v), H' = xi_0 H (pcdl.rs:135,180-181) */
int halo_open_start(const uint64_t C[12], const uint64_t z[4], const uint64_t *v_parts, size_t P, uint64_t v_out[4], uint64_t xi0[4],
                    uint64_t Hp_out[12]);
/* parts = P records (L 12 | R 12 | dot_l 4 | dot_r 4) in rank order -> L, R with the H' terms, the next
 * challenge rho_0(xi_prev, L, R) and its inverse (pcdl.rs:203-213) */
int halo_open_combine(const uint64_t *parts, size_t P, const uint64_t Hp[12], const uint64_t xi_prev[4], uint64_t L[12], uint64_t R[12],
                      uint64_t xi[4], uint64_t xi_inv[4]);
/* the last lg P rounds of a sharded open, on the host: after lg(n / P) rounds every rank holds ONE element of G, c and z;
 * recs = the P gathered records (G_i Jacobian 12 | c_i 4 | z_i 4) in index order, P a power of two <= 64.  Runs pcdl.rs:195-227
 * over them (challenges chained from xi_prev) and returns the lg P pairs L, R (12 words each, round order), U and c
 * (pcdl.rs:230-231).  Identical on every rank. */
int halo_open_tail(const uint64_t *recs, size_t P, const uint64_t Hp[12], const uint64_t xi_prev[4], uint64_t *Ls, uint64_t *Rs,
                   uint64_t U[12], uint64_t c_out[4]);
/* L = <c_r, G_l> + <c_r, z_l> H', R = <c_l, G_r> + <c_l, z_r> H'   (pcdl.rs:203-208) */
int halo_ipa_round_lr(halo_ipa *st, const uint64_t H_prime[12], uint64_t L[12], uint64_t R[12]);
/* G, c, z folds with the challenge the host hashed from (xi_prev, L, R)   (pcdl.rs:216-224) */
int halo_ipa_round_fold(halo_ipa *st, const uint64_t xi[4], const uint64_t xi_inv[4]);
/* U = G[0], c = c[0]   (pcdl.rs:230-231) */
int halo_ipa_finish(halo_ipa *st, uint64_t U[12], uint64_t c[4]);
void halo_ipa_destroy(halo_ipa *st);
size_t halo_ipa_len(const halo_ipa *st);

/* ---- pcdl / acc level: the reference's public functions, host glue in C++, linear work in HIP
 *
 * Flat layouts (u64 words), lg = log2(d + 1):
 *   EvalProof (pcdl.rs:22-30): [0] hiding flag | [1] lg | Ls lg*12 | Rs lg*12 | U 12 | c 4 | C_bar 12 | w' 4
 *   Instance  (acc.rs:21-28) : C 12 | d 1 | z 4 | v 4 | EvalProof
 *   Accumulator (acc.rs:43-59): Instance fields (C_bar, d, z, v, pi) | h0 8 (two Fr) | U0 12 | w 4
 * `rng_state` is a SplitMix64 state (the reference takes `rng: &mut R`): scalars are 4 draws,
 * little-endian, reduced mod r; the state is advanced exactly as a sequential stream would be. */
size_t halo_proof_words(size_t lg_n);
size_t halo_instance_words(size_t lg_n);
size_t halo_accumulator_words(size_t lg_n);
/* pedersen::commit (pedersen.rs:6-20) over GS[0..n_bases) */
int halo_pedersen_commit(halo_ctx *ctx, const uint64_t *w /*nullable*/, size_t n_bases, const uint64_t *ms, size_t n_ms,
                         uint64_t out[12]);
/* pedersen::commit (pedersen.rs:6-20) over generators the caller passes (n_bases x 8 limbs; not the context's key):
 * the signature takes any `&[PallasAffine]` (pedersen.rs:6), this is that case; halo_msm_affine underneath */
int halo_pedersen_commit_affine(halo_ctx *ctx, const uint64_t *w /*nullable*/, const uint64_t *bases_affine, size_t n_bases,
                                const uint64_t *ms, size_t n_ms, uint64_t out[12]);
/* pcdl::commit (pcdl.rs:99-110) */
int halo_pcdl_commit(halo_ctx *ctx, const uint64_t *coeffs, size_t len, size_t d, const uint64_t *w /*nullable*/, uint64_t out[12]);
/* pcdl::open (pcdl.rs:120-242) */
int halo_pcdl_open(halo_ctx *ctx, uint64_t *rng_state, const uint64_t *coeffs, size_t len, const uint64_t C[12], size_t d,
                   const uint64_t z[4], const uint64_t *w /*nullable*/, uint64_t *proof_out);
/* The same two for a polynomial already resident in device memory (len x 4 limbs, Montgomery; len = p.degree() + 1,
 * i.e. the top coefficient is non-zero as ark-poly's DensePolynomial guarantees).  The coefficients are read, not
 * modified.  No host-to-device transfer of the polynomial: this is the form whose rate bench.py reports.  (A zero-padded
 * buffer: halo_poly_degrees_dev gives len without a download; halo_pcdl_open_dev_batch takes the padded buffer as it is.) */
int halo_pcdl_commit_dev(halo_ctx *ctx, const void *d_coeffs, size_t len, size_t d, const uint64_t *w /*nullable*/, uint64_t out[12]);
int halo_pcdl_open_dev(halo_ctx *ctx, uint64_t *rng_state, const void *d_coeffs, size_t len, const uint64_t C[12], size_t d,
                       const uint64_t z[4], const uint64_t *w /*nullable*/, uint64_t *proof_out);
/* pcdl::succinct_check (pcdl.rs:252-314): xis_out (lg+1) x 4, U_out */
int halo_pcdl_succinct_check(halo_ctx *ctx, const uint64_t C[12], size_t d, const uint64_t z[4], const uint64_t v[4],
                             const uint64_t *proof, uint64_t *xis_out, uint64_t U_out[12]);
/* m succinct checks at once (acc.rs:158-170 runs them in a loop): instances = m Instance blobs of degree bound d.  From 64
 * instances on the m relations are evaluated in two device launches (h_i(z_i) for all i; the 2 lg n + 2 scalar multiples
 * of every relation, one wave per instance), the transcripts on a pool of host threads.  status[i] (nullable) = 0 or
 * HALO_E_REJECT per instance; xis_out m x (lg+1) x 4 and U_out m x 12 (nullable) as halo_pcdl_succinct_check. */
int halo_pcdl_succinct_check_batch(halo_ctx *ctx, size_t d, const uint64_t *instances, size_t m, uint64_t *xis_out, uint64_t *U_out,
                                   int *status);
/* pcdl::check (pcdl.rs:323-342) */
int halo_pcdl_check(halo_ctx *ctx, const uint64_t C[12], size_t d, const uint64_t z[4], const uint64_t v[4], const uint64_t *proof);
/* pcdl::check (pcdl.rs:323-342) of m instances at once.  instances = m Instance blobs at stride halo_instance_words(lg(d+1)),
 * all of degree bound d.  The succinct checks run as in halo_pcdl_succinct_check_batch; the accepted members' h coefficients
 * are expanded on the device and their n-point MSMs (pcdl.rs:338) run in batched launches of up to 8, rotating over the slots
 * that are idle on entry (a caller's MSM in flight on another slot is left alone; no idle slot: HALO_E_ARG).  Every member gets
 * its own exact MSM.  status[i] (nullable) = what halo_pcdl_check returns for member i alone; returns 0 if every member was
 * accepted, else the first non-zero status in member order, halo_last_error() = "instance i: <its message>".  A null ctx, or a
 * null `instances` with m > 0: HALO_E_ARG.  d + 1 not a power of two, or a member whose d or proof length differs from d:
 * HALO_E_REJECT ("d_i != d") before any work, status not written.  m = 0: HALO_OK.  The staging of the members in flight is
 * optional memory (halo_set_memory_budget): without it the members run one at a time, same results. */
int halo_pcdl_check_batch(halo_ctx *ctx, size_t d, const uint64_t *instances, size_t m, int *status /*nullable*/);
/* The same m checks with ONE MSM: the second half of pcdl::check (pcdl.rs:338-339) is the linear relation <h_i, G> = U_i, so the
 * members are checked together as <sum r_i h_i, G> = sum r_i U_i with unpredictable weights r_i.  Layouts, whole-call errors
 * (null ctx, null blobs, d + 1 not a power of two, d_i != d, m = 0, no idle slot), the "instance i: ..." message and the return
 * rule are halo_pcdl_check_batch's.  The contract:
 *  1. The succinct half runs for every member exactly as in halo_pcdl_check_batch.  A member it rejects gets its status there
 *     and takes no further part.
 *  2. A = the number of accepted members.  A <= 1 (or d = 0): the exact path of halo_pcdl_check_batch, nothing to combine.
 *     A >= 2: the combined relation over the accepted members -- the scalars sum_a r_a h_a(X) formed on the device, one n-point
 *     MSM over the key (the fixed-base table where the key has one), sum_a r_a U_a on the host pool or as a small MSM beside it.
 *  3. If the combined relation HOLDS, every accepted member's status is 0.
 *  4. If it FAILS, the accepted members go through the exact per-member path of halo_pcdl_check_batch and get its statuses.  So
 *     a reject never depends on the weights, and whenever any member is bad, status[] and the return code equal
 *     halo_pcdl_check_batch's on the same blobs.
 *  5. The one difference from the exact batch: a set of blobs in which some accepted member has <h_i, G> != U_i is wrongly
 *     accepted with probability 1/r (r = the group order, ~2^-254) per hash evaluation an adversary spends: the weights are a
 *     random-oracle output over ALL the blobs, and the relation is linear in them.
 *  6. The scalars live in optional staging memory (halo_set_memory_budget): without it the exact path runs, with the same
 *     statuses.  A multi-device context runs the call on its own device (devices[0]); a caller's MSM in flight on another slot
 *     is left alone.
 * Weight rule.  lg = log2(d + 1), W = halo_instance_words(lg), seed32 = the caller's 32 bytes or, for seed = NULL, 32 zero bytes.
 *   D   = SHA3-256("halo-accumulation/check-batch-combined/v1" || seed32 || LE64(d) || LE64(A) || for every accepted member in
 *         member order: LE64(i) || its W Instance words as little-endian bytes)     (i = its index among the m members)
 *   r_a = (SHA3-256(D || LE64(a)) read as a little-endian integer) mod r,  a = 0 .. A - 1 its position among the accepted ones.
 * A caller that wants weights no prover could have anticipated passes fresh random bytes as seed; the result never depends on it.
 * When to call it (one MI355X, tools/time_decider_batch.py --combined): on a key of 2^20 points, where the exact
 * batch runs one table MSM per member -- 4.0 times its speed at m = 10, 10.9 times at m = 100; on keys of 2^9 .. 2^14 points from
 * about a hundred members on -- 1.3 to 1.7 times at m = 100, 1.5 to 2.1 times at m = 1000, where the succinct half is what remains.
 * At m = 10 on those keys it is NOT faster than halo_pcdl_check_batch (the runs' ranges overlap). */
int halo_pcdl_check_batch_combined(halo_ctx *ctx, size_t d, const uint64_t *instances, size_t m, const uint8_t seed[32] /*nullable*/,
                                   int *status /*nullable*/);
/* The same m checks as ONE relation, the succinct half included: pcdl.rs:307-310 is as linear in the proof's points as :339.  For
 * a member a whose transcript was accepted (xi_a,0 .. xi_a,lg and C'_a as halo_pcdl_succinct_check computes them; c_a, z_a, v_a, U_a,
 * L_a,j, R_a,j from its blob; hz_a = h_a(z_a)) let
 *   E_a = C'_a + sum_j (xi_a,j+1^-1 L_a,j + xi_a,j+1 R_a,j) + (v_a - c_a hz_a) xi_a,0 H - c_a U_a      (0 iff :307-310 accepts)
 *   F_a = U_a - <h_a, G>                                                                               (0 iff :339 accepts)
 * and check  sum_a r_a E_a + sum_a s_a F_a = 0  with two independent hashed weights per member, i.e.
 *   sum_a [ r_a C'_a + sum_j (r_a xi_a,j+1^-1 L_a,j + r_a xi_a,j+1 R_a,j) + (s_a - r_a c_a) U_a ] + (sum_a r_a (v_a - c_a hz_a) xi_a,0) H
 *       ==  < sum_a s_a h_a , G >.
 * Left: one variable-base MSM over M (2 lg + 2) + 1 points of the caller's; right: the combined call's n-point MSM over the key.
 * (With s_a tied to r_a a shifted U whose two defects are in ratio -c_a : 1 would cancel: hence two weights.)  The contract:
 *  1. Layouts, whole-call errors (null ctx, null blobs, d + 1 not a power of two, d_i != d, m = 0, no idle slot), the
 *     "instance i: ..." message and the return rule are halo_pcdl_check_batch's.
 *  2. Every member's structure and transcript run exactly as in halo_pcdl_succinct_check, on the host pool: validity of every point
 *     and scalar, d, the proof length, a zero challenge.  A member rejected there gets that status and takes no further part.
 *  3. M = the number of members accepted so far.  M <= 1 or d = 0: the exact path of halo_pcdl_check_batch.  M >= 2 (at most 65535,
 *     lg <= 24; beyond: the exact path): the relation above.  The term scalars are computed on the device, one lane per member, with
 *     one field inversion each; the left side's terms are cut into MSMs of at most the key's size, which run on a second idle slot
 *     beside the key's MSM (one idle slot: after it), their sums added in order.
 *  4. If the relation HOLDS, every such member's status is 0.
 *  5. If it FAILS, the exact batch decides: the per-member relations and per-member MSMs of halo_pcdl_check_batch.  So a reject
 *     never depends on the weights, and whenever any member is bad, status[], the return code and the message equal
 *     halo_pcdl_check_batch's on the same blobs.
 *  6. The one difference from the exact batch: a set of blobs with some E_a != 0 or F_a != 0 is wrongly accepted with probability
 *     1/r (r = the group order, ~2^-254) per hash evaluation an adversary spends.
 *  7. All device memory the call takes is optional staging (halo_set_memory_budget): without it the exact path runs and gives the
 *     same statuses.  A multi-device context runs the call on its own device (devices[0]); a caller's MSM in flight on another slot
 *     is left alone.
 * Weight rule (fused).  lg, W and seed32 as above.
 *   D   = SHA3-256("halo-accumulation/check-batch-fused/v1" || seed32 || LE64(d) || LE64(M) || for every member taking part, in
 *         member order: LE64(i) || its W Instance words as little-endian bytes)      (i = its index among the m members)
 *   r_a = (SHA3-256(D || LE64(2 a)) read as a little-endian integer) mod r,
 *   s_a = (SHA3-256(D || LE64(2 a + 1)) read as a little-endian integer) mod r,      a = 0 .. M - 1 its position among them.
 * When to call it (one MI355X, tools/time_decider_batch.py --fused --big, profiles/r19_check_fused.json; against
 * halo_acc_decider_batch_combined in the same run, medians of 5): 1.36 to 1.54 times its speed at m = 10 and 1.28 to 1.37 times at
 * m = 100 on keys of 2^9 .. 2^14 and of 2^20 points, 1.05 times at m = 1000 (that run had the members' transcripts on the host
 * pool; from 1000 members on they now run on the device, which takes 29.0 to 26.6 ms off halo_acc_decider_batch_fused at 2^9
 * points and 38.7 to 37.4 ms at 2^14 -- tools/time_transcripts.py, profiles/r20_transcripts.json; the ratio against the combined
 * call has not been measured again).  Every fused run was faster than every combined run in each row but two, which are NOT won: 2^9 points with m = 100 and
 * 2^14 points with m = 1000 (one fused run of five inside the combined call's range). */
int halo_pcdl_check_batch_fused(halo_ctx *ctx, size_t d, const uint64_t *instances, size_t m, const uint8_t seed[32] /*nullable*/,
                                int *status /*nullable*/);
/* pcdl::check of m instances, EACH WITH ITS OWN degree bound: pcdl::check takes d per call, and a commitment of degree bound d
 * lives on the prefix G[0 .. d + 1) of the one key (pcdl.rs:99-110, :338), so a verifier that holds one key sees proofs of several
 * sizes.  instances[i] points at one Instance blob of halo_instance_words(lg(ds[i] + 1)) words; the blobs need be neither
 * contiguous nor ordered.  The contract:
 *  - Whole-call errors, before any work, status not written.  A null ctx, or a null ds, a null `instances` or a null instances[i]
 *    with m > 0: HALO_E_ARG.  Some ds[i] + 1 not a power of two: HALO_E_REJECT ("d+1 is not a power of 2!").  A blob whose d word
 *    (word 12) or proof lg word (word 22) disagrees with ds[i]: HALO_E_REJECT ("d_i != d").  m = 0: HALO_OK.  No idle slot:
 *    HALO_E_ARG.
 *  - Per member.  status[i] (nullable) = what halo_pcdl_check returns for member i alone -- a member whose d + 1 exceeds the key
 *    included: it gets the single call's reject.  Returns 0, or the first non-zero status in member order with halo_last_error() =
 *    "instance i: <the single call's message>", i the index in THIS call.
 *  - The members are grouped into classes of equal d.  Each class runs the succinct half and the exact per-member MSMs of
 *    halo_pcdl_check_batch, with its staging rule; the results are scattered back to member order. */
int halo_pcdl_check_batch_mixed(halo_ctx *ctx, const size_t *ds, const uint64_t *const *instances, size_t m, int *status /*nullable*/);
/* The same with ONE MSM for the members of every size: <h_a, G[0 .. n_a)> = U_a is linear in h_a, and a shorter h_a is a
 * zero-padded vector over the same key, so the accepted members are checked as
 *   < sum_a r_a pad(h_a), G[0 .. n_max) >  =  sum_a r_a U_a,        n_max = the largest accepted n_a.
 * Arguments, whole-call errors, message and return rule are halo_pcdl_check_batch_mixed's.  It carries points 1 - 6 of
 * halo_pcdl_check_batch_combined's contract with these changes:
 *  1. The succinct half runs per class of equal d.
 *  2. A = the accepted members with d_i >= 1, over ALL classes.  A <= 1: the exact path.  A >= 2 (at most 65535, lg <= 24; beyond:
 *     the exact path): the relation above -- the scalars formed on the device from tables of their own lengths, ONE n_max-point
 *     MSM over the key (the fixed-base table where the key has one and n_max reaches it), sum_a r_a U_a on the host pool or as a
 *     small MSM on a second idle slot, by the uniform call's rule.  Members with d_i = 0 always take their class's exact path.
 *  3. If the relation HOLDS, every such member's status is 0.
 *  4. If it FAILS -- or the optional staging is refused -- the per-class exact path decides, so a reject never depends on the
 *     weights and status[], code and message equal halo_pcdl_check_batch_mixed's on the same blobs.
 *  5., 6. as there (soundness 1/r per hash evaluation; optional staging; devices[0] of a multi-device context; a caller's MSM in
 *     flight on another slot is left alone).
 * Weight rule (mixed): a domain of its own, and every member's index and degree bound in the hash, so no digest of a uniform call
 * can be replayed.  W_i = halo_instance_words(lg(d_i + 1)), seed32 as above.
 *   D   = SHA3-256("halo-accumulation/check-batch-mixed-combined/v1" || seed32 || LE64(A) || for every accepted member in member
 *         order: LE64(i) || LE64(d_i) || its W_i Instance words as little-endian bytes)
 *   r_a = (SHA3-256(D || LE64(a)) read as a little-endian integer) mod r,  a = 0 .. A - 1 its position among the accepted ones.
 * This call itself has no fused form for mixed sizes inside it (its succinct half stays exact, per class); the fused relation over
 * mixed sizes is halo_pcdl_check_batch_mixed_fused below, whose term kernel takes a length per member.
 * When to call it (one MI355X, tools/time_check_mixed.py --big, profiles/r21_check_mixed.json; members spread evenly over lg 9 .. 14,
 * on the 2^20-point key 1 to 4 members of lg 20 as well; against the members sorted by d and one halo_pcdl_check_batch_combined, or
 * one halo_pcdl_check_batch_fused, per size; alternating runs, medians of 5): when the alternative is a combined call per size
 * it is never slower -- 1.02 to 1.28 times the per-size calls' speed -- and it spares the caller the sort, but only two of the
 * eight rows are WON against them with the ranges apart (2^14 points with 600 members, 1.05 times; 2^20 points with 13 members,
 * 1.28 times); in the other six the ranges overlap: NOT won.  Against a fused call per size it wins that one 2^20 row (13 members,
 * 1.31 times) and the median of the 12-member row at 2^14 (1.15 times, ranges overlapping: NOT won); from 60 members on the
 * per-size fused calls are faster on both keys, 0.61 to 0.79 times their speed: NOT won.  At every count
 * halo_pcdl_check_batch_mixed_fused below is faster than either (profiles/r22_check_mixed_fused.json): no sort by d is needed. */
int halo_pcdl_check_batch_mixed_combined(halo_ctx *ctx, const size_t *ds, const uint64_t *const *instances, size_t m,
                                         const uint8_t seed[32] /*nullable*/, int *status /*nullable*/);
/* The same as ONE relation over the members of every size, the succinct half included: halo_pcdl_check_batch_fused's relation with
 * a size per member.  With E_a and F_a as there, each at its own lg_a, and F_a = U_a - <pad(h_a), G[0 .. n_max)>:
 *   sum_a [ r_a C'_a + sum_j (r_a xi_a,j+1^-1 L_a,j + r_a xi_a,j+1 R_a,j) + (s_a - r_a c_a) U_a ] + (sum_a r_a (v_a - c_a hz_a) xi_a,0) H
 *       ==  < sum_a s_a pad(h_a) , G[0 .. n_max) >.
 * Left: one variable-base MSM over T = sum_a (2 lg_a + 2) + 1 points of the caller's; right: the mixed combined call's one
 * n_max-point MSM over the key.  The contract:
 *  1. Arguments, whole-call errors (before any work, status not written), the "instance i: ..." message and the return rule are
 *     halo_pcdl_check_batch_mixed's.
 *  2. Every member's structure and transcript run exactly as in halo_pcdl_succinct_check, per class of equal d (a class of 1000
 *     members or more on the device, by the uniform call's rule).  A member rejected there gets that status and takes no further
 *     part -- a member whose d + 1 exceeds the key included: it gets what halo_pcdl_check_batch_mixed reports for it.
 *  3. M = the number of members accepted so far with d_i >= 1, over ALL classes.  Members with d_i = 0 always take their class's
 *     exact path.  M <= 1: the exact path of halo_pcdl_check_batch_mixed.  M >= 2 (at most 65535, every lg <= 24, fewer than 2^32
 *     terms with the last chunk filled up; beyond: the exact path): the relation above.  The term scalars are computed on the
 *     device, one lane per member at the member's own size, with one field inversion each; the members' terms lie one behind the
 *     other with nothing between them, are cut into MSMs of at most the key's size and run in batched sequences on a second idle
 *     slot beside the key's MSM (one idle slot: after it), their sums added in order.  The right side's scalars are formed from
 *     tables of their own lengths; its MSM is the fixed-base table's where the key has one and n_max reaches it.
 *  4. If the relation HOLDS, every such member's status is 0.
 *  5. If it FAILS -- or the optional staging is refused -- halo_pcdl_check_batch_mixed's exact path decides: the succinct half
 *     per class, then the per-member MSMs.  So a reject never depends on the weights, and status[], the return code and the
 *     message equal halo_pcdl_check_batch_mixed's on the same blobs.
 *  6. The one difference from the exact call: a set of blobs with some E_a != 0 or F_a != 0 is wrongly accepted with probability
 *     1/r (r = the group order, ~2^-254) per hash evaluation an adversary spends.  Two independent weights per member, for the
 *     reason halo_pcdl_check_batch_fused gives.
 *  7. All device memory the call takes is optional staging (halo_set_memory_budget): without it the exact path runs and gives the
 *     same statuses.  A multi-device context runs the call on its own device (devices[0]); a caller's MSM in flight on another slot
 *     is left alone; no idle slot: HALO_E_ARG.
 * Weight rule (mixed fused): a domain of its own, and every member's index and degree bound in the hash.
 * W_i = halo_instance_words(lg(d_i + 1)), seed32 as above.
 *   D   = SHA3-256("halo-accumulation/check-batch-mixed-fused/v1" || seed32 || LE64(M) || for every member taking part, in member
 *         order: LE64(i) || LE64(d_i) || its W_i Instance words as little-endian bytes)
 *   r_a = (SHA3-256(D || LE64(2 a)) read as a little-endian integer) mod r,
 *   s_a = (SHA3-256(D || LE64(2 a + 1)) read as a little-endian integer) mod r,      a = 0 .. M - 1 its position among them.
 * When to call it (one MI355X, tools/time_check_mixed.py --big, profiles/r22_check_mixed_fused.json; the workloads of
 * halo_pcdl_check_batch_mixed_combined above; against one halo_pcdl_check_batch_fused per size and against
 * halo_pcdl_check_batch_mixed_combined in the same alternating runs, medians of 5): whenever members of several sizes are checked.
 * Against a fused call per size, 2^14 points: 2.40, 1.94, 1.82 and 1.22 times its speed at 12, 60, 120 and 600 members, all four
 * rows WON (every run below every run of the per-size calls); 2^20 points: 2.64, 1.92 and 1.69 times at 13, 62 and 123 members,
 * WON, and 1.20 times at 604 members, NOT won (one run of five inside the per-size calls' range).  Against
 * halo_pcdl_check_batch_mixed_combined 1.44 to 2.91 times, and against a combined call per size 1.61 to 3.11 times, all eight
 * rows WON.  At 600 members the transcripts on the host pool are what remains of every way. */
int halo_pcdl_check_batch_mixed_fused(halo_ctx *ctx, const size_t *ds, const uint64_t *const *instances, size_t m,
                                      const uint8_t seed[32] /*nullable*/, int *status /*nullable*/);
/* One rank's half of pcdl::check over a key sharded cyclically (halo_ctx_create_urs_strided: point i on rank i mod stride,
 * offset = the rank): the succinct check (pcdl.rs:333, the same on every rank; d + 1 may be up to stride * the shard's size)
 * and this rank's share of CM.Commit(ck, h) (pcdl.rs:338) over its own points.  U_out = the proof's U after the succinct
 * check, part_out = the share.  The caller adds the shares of all ranks in rank order (halo_point_sum) and accepts iff the
 * sum equals U (pcdl.rs:339); errors as halo_pcdl_check. */
int halo_pcdl_check_partial(halo_ctx *ctx, const uint64_t C[12], size_t d, const uint64_t z[4], const uint64_t v[4], const uint64_t *proof,
                            uint64_t stride, uint64_t offset, uint64_t U_out[12], uint64_t part_out[12]);

/* ---- sharded open / check in one call each --------------------------------------------------------------
 * The caller's all-gather: every rank contributes `words` u64 from `send`, `recv` receives P x words in rank order; returns
 * 0 on success.  Collectives stay outside the library (RCCL through the host language, MPI, ...): this is the only hook.
 *
 * Failure safety: the number and order of collectives of a call depend only on the arguments all ranks pass alike (P, d,
 * hiding or not).  Every record carries one status word behind its payload (the sizes below are payload + 1): a rank on
 * which something fails between two collectives (device allocation, launch, copy, a per-rank argument) does NOT return --
 * it enters the next collective with its error code there, and all P ranks return that code (the first non-zero one in rank
 * order) at the same collective.  No rank waits in an all-gather its peers never enter.  If the callback itself returns
 * non-zero the fabric has failed: the call returns HALO_E_ARG and the caller must abort its process group. */
typedef int (*halo_allgather_fn)(void *user, const uint64_t *send, size_t words, uint64_t *recv);
/* pcdl::open (pcdl.rs:120-242) with G, c and the z-powers placed cyclically: ctx = this rank's shard of the key
 * (halo_ctx_create_urs_strided with stride = P ranks, first_index + offset), coeffs_local = c[offset], c[offset + P], ...
 * (len_local of them), deg = p.degree() of the WHOLE polynomial (hiding branch only), w = commitment randomness or NULL,
 * *rng_state as halo_pcdl_open (the same on every rank, advanced alike).  Collectives, in order: the shares of p(z) (4 + 1
 * words; hiding: 16 + 1), per round L | R | dot_l | dot_r (32 + 1 words), the P last elements (20 + 1 words, P > 1 only); no
 * vector exchange; the last lg P rounds run on the host from the P gathered elements.  proof_out and v_out = p(z) are the same on
 * every rank and equal what halo_pcdl_open returns on one GPU. */
int halo_pcdl_open_sharded(halo_ctx *ctx, uint64_t stride, uint64_t offset, uint64_t *rng_state, const uint64_t *coeffs_local, size_t len_local,
                           size_t deg, const uint64_t C[12], size_t d, const uint64_t z[4], const uint64_t *w /*nullable*/,
                           halo_allgather_fn allgather, void *user, uint64_t *proof_out, uint64_t v_out[4]);
/* pcdl::check (pcdl.rs:323-342) over the same shards: halo_pcdl_check_partial, one all-gather of 12 + 1 words, the sum compared
 * with U; HALO_E_REJECT -- or the code of a rank whose half failed -- on every rank alike */
int halo_pcdl_check_sharded(halo_ctx *ctx, uint64_t stride, uint64_t offset, const uint64_t C[12], size_t d, const uint64_t z[4],
                            const uint64_t v[4], const uint64_t *proof, halo_allgather_fn allgather, void *user);
/* point_dot_affine (group.rs:24-26) sharded over `world` processes, one per GPU.  Each rank passes ITS share of the MSM:
 * sum_i scalars[i] * G[off + i] over its own ctx (halo_msm / halo_msm_dev underneath; a multi-device ctx fans out as usual).
 * The partition is the caller's: an index block over halo_ctx_create_urs(2 + lo, hi - lo), a cyclic shard, anything else.
 * n may be 0 (the point at infinity).  One all-gather of 12 + 1 words per rank, then P - 1 additions in rank order on the host:
 * out_jac is normalised and the same limbs on every rank, and equals halo_msm over the whole key when the shares partition it.
 * world in 1..64, rank below it; world == 1 with allgather == NULL: no collective, exactly halo_msm.  Failure safety as above:
 * world, rank, a missing all-gather and a null out_jac return HALO_E_ARG before the collective; a null ctx, a range past this
 * rank's key, null scalars or a device failure on one rank enter it as that rank's status, and every rank returns that code. */
int halo_msm_sharded(halo_ctx *ctx, uint64_t world, uint64_t rank, size_t off, size_t n, const uint64_t *scalars, int scalars_are_mont,
                     halo_allgather_fn allgather, void *user, uint64_t out_jac[12]);
int halo_msm_dev_sharded(halo_ctx *ctx, uint64_t world, uint64_t rank, size_t off, size_t n, const void *d_scalars, int scalars_are_mont,
                         halo_allgather_fn allgather, void *user, uint64_t out_jac[12]);
/* The asynchronous end: collect what `slot` holds and combine it across ranks with ONE collective of 12 * batch + 1 words.
 * The slot was started by halo_msm_begin, halo_msm_dev_begin, halo_msm_dev_begin_part (window shards: part = rank,
 * parts = world, every rank holding the whole key) or halo_msm_dev_batch_begin.  batch (1..8) must match what the slot
 * holds; an idle slot or a different batch is that rank's failure and rides into the collective.  out_jac = batch x 12 limbs. */
int halo_msm_end_sharded(halo_ctx *ctx, int slot, size_t batch, uint64_t world, uint64_t rank, halo_allgather_fn allgather, void *user,
                         uint64_t *out_jac);
/* acc::prover / verifier / decider (acc.rs:190-255); instances = m contiguous Instance blobs */
int halo_acc_prover(halo_ctx *ctx, uint64_t *rng_state, size_t d, const uint64_t *instances, size_t m, uint64_t *acc_out);
int halo_acc_verifier(halo_ctx *ctx, size_t d, const uint64_t *instances, size_t m, const uint64_t *acc);
int halo_acc_decider(halo_ctx *ctx, const uint64_t *acc);
/* acc::decider (acc.rs:245-255) of m accumulators at once: benches/acc.rs:100-106 in one call.  accs = m Accumulator blobs at
 * stride halo_accumulator_words(lg(d+1)); halo_pcdl_check_batch over their Instance prefixes, with its conventions. */
int halo_acc_decider_batch(halo_ctx *ctx, size_t d, const uint64_t *accs, size_t m, int *status /*nullable*/);
/* ... as one combined relation: halo_pcdl_check_batch_combined over the accumulators' Instance prefixes, with its contract (the
 * words hashed into the weights are each accumulator's Instance prefix) */
int halo_acc_decider_batch_combined(halo_ctx *ctx, size_t d, const uint64_t *accs, size_t m, const uint8_t seed[32] /*nullable*/,
                                    int *status /*nullable*/);
/* ... as one fused relation: halo_pcdl_check_batch_fused over the accumulators' Instance prefixes, with its contract (each
 * accumulator's Instance prefix is what is read, and what is hashed into the weights) */
int halo_acc_decider_batch_fused(halo_ctx *ctx, size_t d, const uint64_t *accs, size_t m, const uint8_t seed[32] /*nullable*/,
                                 int *status /*nullable*/);
/* acc::decider of m accumulators, each with its own degree bound: halo_pcdl_check_batch_mixed / .._mixed_combined / .._mixed_fused
 * over the accumulators' Instance prefixes, with their contracts.  accs[i] points at one Accumulator blob of
 * halo_accumulator_words(lg(ds[i] + 1)) words; its Instance prefix is what is checked and what is hashed into the weights. */
int halo_acc_decider_batch_mixed(halo_ctx *ctx, const size_t *ds, const uint64_t *const *accs, size_t m, int *status /*nullable*/);
int halo_acc_decider_batch_mixed_combined(halo_ctx *ctx, const size_t *ds, const uint64_t *const *accs, size_t m,
                                          const uint8_t seed[32] /*nullable*/, int *status /*nullable*/);
int halo_acc_decider_batch_mixed_fused(halo_ctx *ctx, const size_t *ds, const uint64_t *const *accs, size_t m,
                                       const uint8_t seed[32] /*nullable*/, int *status /*nullable*/);
/* acc::verifier (acc.rs:223-243) of k accumulators at once: benches/acc.rs:64-74's loop in one call.  accs = k Accumulator blobs
 * at stride halo_accumulator_words(lg(d+1)); counts[j] = the number of Instances member j verifies against accs[j] (0 allowed);
 * instances = sum(counts) Instance blobs at stride halo_instance_words(lg(d+1)), member j's right after member j - 1's.
 * status[j] = what halo_acc_verifier(ctx, d, <member j's instances>, counts[j], accs[j]) returns alone: each member's checks
 * resolve in that call's order (accumulator fields, U_0 == commit(h_0), every instance's d and proof length, the succinct
 * checks in instance order, C_bar' == C_bar, z' == z, d' == d, h(z) == v).  Returns 0 if every member is accepted, else the
 * first non-zero status in member order with halo_last_error() = "member j: <the single call's message>".  Whole-call errors
 * come first and leave status untouched: a null ctx, k > 0 with null accs or counts, or a non-zero total with null instances
 * (HALO_E_ARG); d + 1 not a power of two (HALO_E_REJECT); d + 1 above the key (HALO_E_ASSERT "commit: d > D"); k = 0 is OK.
 * A device failure returns its code.  The transcripts run on a host thread pool; every relation and member sum goes to the
 * device in one launch, on a slot idle on entry (a caller's MSM in flight is left alone), from 64 relations on.  Fewer, no
 * idle slot or no staging memory (optional memory, halo_set_memory_budget): the host pool, with the same results.  A
 * multi-device context runs the batch on devices[0]. */
int halo_acc_verifier_batch(halo_ctx *ctx, size_t d, const uint64_t *instances, const size_t *counts, size_t k,
                            const uint64_t *accs, int *status /*nullable*/);
/* acc::prover (acc.rs:190-220) of k members at once.  Layout as halo_acc_verifier_batch: counts[j] Instances for member j (0
 * allowed), member j's right after member j - 1's, at stride halo_instance_words(lg(d+1)); accs_out = k Accumulator blobs at
 * stride halo_accumulator_words(lg(d+1)).
 * - Same results as a loop: every succeeded member's blob, every status[j] and the final *rng_state equal k calls of
 *   halo_acc_prover in member order with the same rng_state pointer (NULL: state 0), continuing after a member that fails.  A
 *   member fails exactly where the single call fails (every d_i / proof length first, "d_i != d", then the succinct checks in
 *   instance order); such a member draws nothing, as the single call writes *rng_state only after its instances were accepted,
 *   and the next member starts from the same state.  The one difference from the loop: a failed member's blob is zero-filled.
 *   Returns 0 if every member succeeded, else the first non-zero status in member order, halo_last_error() = "member j:
 *   <the single call's message>".
 * - Before any work (status, *rng_state and accs_out not written): a null ctx, k > 0 with null counts or accs_out, or a non-zero
 *   total with null instances: HALO_E_ARG; d + 1 not a power of two or above the key: HALO_E_ASSERT with the single call's
 *   messages.  k = 0: HALO_OK, nothing touched.  No idle slot: HALO_E_ARG.  A device failure returns its code.
 * - Where the hiding open takes its no-fold form (2 <= d + 1 <= the no-fold size, 2^14 by default): the succinct half of all
 *   instances at once (from 64 instances on in one device launch, as halo_pcdl_succinct_check_batch), the members' sums on a
 *   host thread pool, then groups of up to 4 members through the launches of halo_pcdl_open_batch, their polynomials h(X) =
 *   h_0 + sum alpha^(i+1) h_i(X) accumulated on the device straight into the open's state.  At d + 1 = 2^16 .. 2^19 the
 *   groups' opens take the folded schedule of halo_pcdl_open_batch (its staging per slot; measured 2.5 - 3.4 times as fast as
 *   the loop up to 2^17, 1.8 times at 2^18, 1.6 at 2^19); halo_ctx_info(ctx, 10) says how many members of the last call
 *   reached their opens in member-batched launches.  Elsewhere (2^15, and above 2^19), and without the staging memory (optional
 *   memory, halo_set_memory_budget), the members run one at a time as halo_acc_prover runs them, with the same results.  A
 *   multi-device context runs the batch on devices[0]. */
int halo_acc_prover_batch(halo_ctx *ctx, uint64_t *rng_state, size_t d, const uint64_t *instances, const size_t *counts, size_t k,
                          uint64_t *accs_out, int *status /*nullable*/);
/* benches/acc.rs:15-29 random_instance: the workload generator of the reference's benchmark */
int halo_random_instance(halo_ctx *ctx, uint64_t *rng_state, size_t d, uint64_t *instance_out);

/* pcdl::open (pcdl.rs:120-242) of m polynomials of degree bound d at once.  coeffs = m x (d + 1) x 4 words (member i at
 * i * (d + 1) * 4, zero-padded; its degree is that of the padded array, found as halo_pcdl_open finds it), Cs = m x 12,
 * zs = m x 4, ws = m x 4 or NULL (NULL: no member hides; otherwise every member hides with its own w).  proofs_out = m
 * EvalProof blobs at stride halo_proof_words(lg(d+1)).
 * - Same results as a loop: every proof word and the final *rng_state equal m calls of halo_pcdl_open in member order with the
 *   same rng_state pointer (NULL: state 0, as there).  The stream is counter-based, so every member's draws (a hiding open: deg
 *   scalars for q, then w_bar) depend only on the earlier members' degrees: the host knows every start state before any device work.
 * - A member fails as the single call would (today only a hiding open of a constant polynomial: HALO_E_ASSERT, "open: hiding needs
 *   p.degree() >= 1"): it consumes no randomness, status[i] (nullable) gets its code and its blob is zero-filled; the other members
 *   are unaffected.  Returns 0 if every member succeeded, else the first non-zero status in member order, halo_last_error() =
 *   "member i: <message>".
 * - Before any work (status not written, *rng_state unchanged): a null ctx or a null array with m > 0: HALO_E_ARG; d + 1 not a
 *   power of two or above the key: HALO_E_ASSERT with the single call's messages.  m = 0: HALO_OK, nothing touched.
 * - Where the single open takes its no-fold form (2 <= d + 1 <= the no-fold size, 2^14 by default) groups of up to 4 members run
 *   in member-batched launches: one batched MSM per round for the L and R of the whole group.  At d + 1 = 2^15 .. 2^19 a group
 *   also folds its keys as the single open does -- one or two rounds over the unfolded key, then one member-batched fold launch
 *   that writes every member's folded key into the group's device state (n / 2 or n / 4 points of 128 bytes per member more), the
 *   later rounds over those keys, folded again until the no-fold size -- measured 2.4 - 3.3 times as fast as the loop up to
 *   2^17, 1.7 - 1.95 times at 2^18 and 1.5 times at 2^19; halo_ctx_info(ctx, 10) says how many members of the last call ran this
 *   way.  A slot's device state for a group of 4: 224 (d + 1) bytes per member and the keys -- 14 MiB at 2^14, 128 MiB at 2^17,
 *   256 MiB at 2^18, 512 MiB at 2^19; where the budget refuses it the call uses fewer slots or the loop.  Groups rotate over the slots that
 *   are idle on entry (a caller's MSM in flight on another slot is left alone; no idle slot: HALO_E_ARG).  Their device state is
 *   optional memory (halo_set_memory_budget; it only grows and goes with the context): without it, and above 2^19 points,
 *   the members run one at a time as halo_pcdl_open runs them, with the same results.  A multi-device context runs the batch
 *   on its first device, with the proofs halo_pcdl_open gives there. */
int halo_pcdl_open_batch(halo_ctx *ctx, uint64_t *rng_state, size_t d, const uint64_t *coeffs, size_t m, const uint64_t *Cs,
                         const uint64_t *zs, const uint64_t *ws /*nullable*/, uint64_t *proofs_out, int *status /*nullable*/);
/* benches/acc.rs:15-29 random_instance, m times: instances_out = m Instance blobs at stride halo_instance_words(lg(d+1)), every
 * word and the final *rng_state as m calls of halo_random_instance in order (draws per member: d', w, the d' + 1 coefficients,
 * z, then its hiding open's).  The conventions of halo_pcdl_open_batch, its batched sizes (d + 1 up to 2^19) and staging included; d < 2: the
 * single call's assert. */
int halo_random_instance_batch(halo_ctx *ctx, uint64_t *rng_state, size_t d, size_t m, uint64_t *instances_out);

/* pcdl::commit (pcdl.rs:99-110) of m polynomials of degree bound d at once.  coeffs = m x (d + 1) x 4 words in the layout of
 * halo_pcdl_open_batch (member i at i * (d + 1) * 4, zero-padded: the same buffer serves the commit and the open), ws = m x 4 or
 * NULL (no member hides), out_jac = m x 12, normalised: member i is what halo_pcdl_commit(ctx, coeffs_i, d + 1, d, w_i, ..) writes
 * (the zero polynomial: (1, 1, 0), or w S).  The layout bounds every degree, so no member fails alone and there is no status.
 * - Before any work, nothing written: a null ctx, or a null coeffs or out_jac with m > 0: HALO_E_ARG; d + 1 not a power of two
 *   or above the key: HALO_E_ASSERT with halo_pcdl_commit's messages; no idle slot: HALO_E_ARG; m = 0: HALO_OK.
 * - Groups of up to 8 members (within the small pipeline's bucket limit; one member where the fixed-base table takes the MSM: a key
 *   and d + 1 of at least 2^20) run as ONE batched MSM launch sequence each and rotate over the slots idle on entry (a caller's
 *   MSM in flight on another slot is left alone).  A group's padded rows are copied on its slot's own stream, so the copy of the
 *   next group runs under this group's kernels; the w_i S terms are added on the host when the group is collected.  (m = 1 at
 *   such a table size, with slots 0 and 1 idle, runs as halo_pcdl_commit itself: its split copy is faster than one copy in
 *   front of one launch.)
 * - The staging is optional memory (halo_set_memory_budget): without it the members run one at a time per idle slot, through
 *   the slots' own scalar buffers, same points.  A multi-device context runs the batch on devices[0]. */
int halo_pcdl_commit_batch(halo_ctx *ctx, size_t d, const uint64_t *coeffs, size_t m, const uint64_t *ws /*nullable*/, uint64_t *out_jac);
/* The same for device-resident polynomials: d_coeffs[i] = a 32-byte aligned device pointer to lens[i] Montgomery scalars
 * (lens[i] = 0 with a null pointer is allowed), read, not modified; the caller's writes to them are complete on entry, as for
 * halo_pcdl_commit_dev, whose result member i equals.  No host-to-device traffic: a member of d + 1 scalars is passed to the
 * launch in place, the shorter ones of a group are zero-padded into the staging by one kernel launch.  A member with
 * lens[i] > d + 1 fails alone as the single call does (HALO_E_ASSERT, "commit: p.degree() > d"): its 12 words are zero-filled and
 * status[i] (nullable) gets the code; returns the first non-zero status, halo_last_error() = "member i: <message>".  Whole-call
 * errors as above, and HALO_E_ARG for a null lens or d_coeffs with m > 0, a null pointer with a non-zero length or a misaligned
 * one. */
int halo_pcdl_commit_dev_batch(halo_ctx *ctx, size_t d, const void *const *d_coeffs, const size_t *lens, size_t m,
                               const uint64_t *ws /*nullable*/, uint64_t *out_jac, int *status /*nullable*/);
/* benches/acc.rs:15-29 for a polynomial the caller holds: C = commit(p, d, w), v = p(z), pi = open(rng, p, C, d, z, w),
 * Instance::new -- halo_pcdl_commit, halo_poly_eval over the p.degree() + 1 coefficients and halo_pcdl_open in one call, with the
 * blob and the final *rng_state of that sequence.  The polynomial is uploaded once and all three read that copy.  Errors: a null
 * ctx, coeffs (with len > 0), z or instance_out: HALO_E_ARG; then the asserts of halo_pcdl_commit in its order ("commit: d + 1 is
 * not a power of two", "commit: p.degree() > d", "commit: d > D"), which cover the other two calls'; then halo_pcdl_open's own
 * ("open: hiding needs p.degree() >= 1": no randomness consumed). */
int halo_instance_from_poly(halo_ctx *ctx, uint64_t *rng_state, const uint64_t *coeffs, size_t len, size_t d, const uint64_t z[4],
                            const uint64_t *w /*nullable*/, uint64_t *instance_out);
/* ... of m polynomials at once, in the layout of halo_pcdl_open_batch without Cs: instances_out = m Instance blobs at stride
 * halo_instance_words(lg(d+1)).  Every word of member i and the final *rng_state equal the loop over halo_instance_from_poly in
 * member order (draws per member are the open's only: a hiding member draws deg scalars for q, then w_bar).  A hiding member with a
 * constant polynomial fails as halo_pcdl_open does: no randomness consumed, blob zero-filled, status[i] = HALO_E_ASSERT, the others
 * unaffected.  The conventions of halo_pcdl_open_batch, with the commit's messages for d + 1 not a power of two or above the key.
 * Where that call batches (2 <= d + 1 <= 2^19, staging available) the members' commits join the first batched MSM
 * of their group; elsewhere, and for m = 1 with slots 0 and 1 idle (measured faster alone), the members run one at a time
 * through halo_instance_from_poly's body.  That body, like halo_pcdl_open's in halo_pcdl_open_batch, runs on slot 0 and may
 * borrow slot 1: above 2^19 points and without the staging, a caller's MSM in flight on one of these two makes the call
 * return HALO_E_ARG ("slot already has an MSM in flight") at the first member that needs the slot. */
int halo_instance_from_poly_batch(halo_ctx *ctx, uint64_t *rng_state, size_t d, const uint64_t *coeffs, size_t m, const uint64_t *zs,
                                  const uint64_t *ws /*nullable*/, uint64_t *instances_out, int *status /*nullable*/);

/* ---- the same over device-resident polynomials: no polynomial crosses to the host or back --------
 * Rows as in halo_pcdl_commit_dev_batch: d_coeffs[i] = a 32-byte aligned device pointer to lens[i] Montgomery scalars, read and
 * never modified, the caller's writes to them complete on entry; lens[i] = 0 with a null pointer is the zero polynomial.  A null
 * pointer with a non-zero length, a misaligned pointer, or a null lens or d_coeffs with m > 0: HALO_E_ARG, nothing written.  On a
 * multi-device context the pointers belong to devices[0].  A row's degree is that of its lens[i] scalars, found on the device
 * (one kernel launch for all m rows): trailing zeros are allowed, a zero-padded buffer needs no download to learn its degree. */
/* degrees_out[i] = the index of row i's last non-zero scalar, 0 for a row without one or of length 0 (DensePolynomial::degree).
 * The table of rows goes to the device in one copy and the results come back in one (24 m bytes of context-owned memory that
 * only grows); m is not bounded; a row of 2^32 - 1 scalars or more: HALO_E_ARG.  degrees_out is written only on success. */
int halo_poly_degrees_dev(halo_ctx *ctx, const void *const *d_coeffs, const size_t *lens, size_t m, size_t *degrees_out);
/* halo_poly_eval for len coefficients in device memory (a pointer as above), read in place: out = what halo_poly_eval writes for
 * the downloaded coefficients.  len is not bound by the context's size (nothing is staged); len >= 2^32: HALO_E_ARG. */
int halo_poly_eval_dev(halo_ctx *ctx, const void *d_coeffs, size_t len, const uint64_t z[4], uint64_t out[4]);
/* halo_instance_from_poly for such a row: the blob and the final *rng_state of halo_instance_from_poly over the downloaded row
 * (equally: of halo_pcdl_commit_dev, halo_poly_eval_dev and halo_pcdl_open_dev over its degree + 1 scalars).  Errors: a null ctx,
 * z or instance_out, or a bad pointer: HALO_E_ARG; then halo_pcdl_commit_dev's asserts in its order ("commit: d + 1 is not a
 * power of two", "commit: p.degree() > d" for len > d + 1, "commit: d > D"); then halo_pcdl_open's own ("open: hiding needs
 * p.degree() >= 1": no randomness consumed). */
int halo_instance_from_poly_dev(halo_ctx *ctx, uint64_t *rng_state, const void *d_coeffs, size_t len, size_t d, const uint64_t z[4],
                                const uint64_t *w /*nullable*/, uint64_t *instance_out);
/* halo_pcdl_open_batch over m such rows.  Every proof word, every status and the final *rng_state equal halo_pcdl_open_batch for
 * the same rows downloaded and zero-padded to d + 1 scalars; where every row's last scalar is non-zero they also equal the loop
 * over halo_pcdl_open_dev (which takes len for degree + 1).
 * - A member with lens[i] > d + 1 fails alone, as in halo_pcdl_commit_dev_batch: HALO_E_ASSERT, "open: p.degree() > d", no
 *   randomness consumed, blob zero-filled; a hiding member of degree 0 fails as in halo_pcdl_open_batch.
 * - Whole-call checks, messages and precedence are halo_pcdl_open_batch's, the pointer errors above among its null checks.
 * - Routes: where halo_pcdl_open_batch runs member-batched launches (2 <= d + 1 <= 2^19, staging available: 512 MiB a slot at 2^19) every group's rows
 *   reach its device state by ONE padding launch on the group's stream (a full-length row too: the open overwrites its copy);
 *   elsewhere each member is copied device to device into the context's polynomial buffer and runs through halo_pcdl_open_dev's
 *   body with the degree found.  halo_ctx_info(ctx, 10) counts the member-batched members as there. */
int halo_pcdl_open_dev_batch(halo_ctx *ctx, uint64_t *rng_state, size_t d, const void *const *d_coeffs, const size_t *lens, size_t m,
                             const uint64_t *Cs, const uint64_t *zs, const uint64_t *ws /*nullable*/, uint64_t *proofs_out,
                             int *status /*nullable*/);
/* halo_instance_from_poly_batch over m such rows, with the same equalities against it, the routes of halo_pcdl_open_dev_batch (2 <= d + 1
 * <= 2^19 and its staging; the commits join the first batched MSM of their group) and "commit: p.degree() > d" for a member with lens[i] > d + 1.  m = 1 with
 * slots 0 and 1 idle runs alone through halo_instance_from_poly_dev's body, the host form's rule (measured faster alone for
 * device rows too; a short polynomial's commit reads its at most 16 scalars back, as the host form's shortcut
 * computes it). */
int halo_instance_from_poly_dev_batch(halo_ctx *ctx, uint64_t *rng_state, size_t d, const void *const *d_coeffs, const size_t *lens,
                                      size_t m, const uint64_t *zs, const uint64_t *ws /*nullable*/, uint64_t *instances_out,
                                      int *status /*nullable*/);

/* ---- wire format (no device needed) ----------------------------------------------------------
 * EvalProof (pcdl.rs:22-30), Instance (acc.rs:21-28) and Accumulator (acc.rs:43-59) in the byte layout a derived
 * ark-serialize `CanonicalSerialize` (compressed) writes: fields in declaration order; Fr = 32 bytes LE canonical;
 * point = 33 bytes (x LE, byte 32: bit 7 = y is the larger of {y, -y}, bit 6 = infinity); usize = u64 LE; Vec = u64 LE
 * length + elements; Option = 1 byte tag + value.  decode() validates canonical scalars, flag bits and curve membership
 * and returns HALO_E_REJECT on malformed input; blobs are the flat u64 layouts above. */
size_t halo_proof_encoded_size(size_t lg_n, int hiding);
size_t halo_instance_encoded_size(size_t lg_n, int hiding);
size_t halo_accumulator_encoded_size(size_t lg_n); /* upper bound */
int halo_proof_encode(const uint64_t *proof, uint8_t *out, size_t cap, size_t *len);
int halo_proof_decode(const uint8_t *in, size_t len, uint64_t *proof_out, size_t cap_words, size_t *lg_n);
int halo_instance_encode(const uint64_t *instance, uint8_t *out, size_t cap, size_t *len);
int halo_instance_decode(const uint8_t *in, size_t len, uint64_t *instance_out, size_t cap_words, size_t *lg_n);
int halo_accumulator_encode(const uint64_t *acc, uint8_t *out, size_t cap, size_t *len);
int halo_accumulator_decode(const uint8_t *in, size_t len, uint64_t *acc_out, size_t cap_words, size_t *lg_n);
/* m blobs decoded in one call: member i is the bytes in[offs[i] .. offs[i + 1]) (offs: m + 1 non-decreasing entries) and its blob
 * goes to out + i * stride_words.
 * - Every member's outcome is the single call's with cap_words = stride_words: status[i] (nullable) its code; on success
 *   lg_out[i] (nullable) and the blob's words are the single call's and the rest of the slot is zero; a failed member's whole
 *   slot is zero-filled and its lg_out[i] is 0; the other members are unaffected.  Returns 0 if every member decoded, else
 *   the first non-zero status in member order, halo_last_error() = "member i: <the single call's message>".
 * - Before any work (status, lg_out and out untouched): m > 0 with a null in, offs or out, or offs decreasing: HALO_E_ARG.
 *   m = 0: HALO_OK.
 * - ctx may be null: the wire format stays usable without a device; the members then run on the host thread pool.  With a
 *   context the structure of every member is read on the host and, from 512 finite points in the batch on, every point is
 *   decompressed on the device (the square root in Fq that dominates a decode: one lane per point), on a slot that is idle
 *   on entry -- a caller's MSM in flight is left alone; a multi-device context uses its first device.  The staging is
 *   optional memory (halo_set_memory_budget); larger batches run in chunks of it.  With no idle slot, no staging or fewer
 *   points the host pool runs instead, with the same results. */
int halo_proof_decode_batch(halo_ctx *ctx /*nullable*/, const uint8_t *in, const size_t *offs, size_t m, uint64_t *out,
                            size_t stride_words, size_t *lg_out /*nullable*/, int *status /*nullable*/);
int halo_instance_decode_batch(halo_ctx *ctx /*nullable*/, const uint8_t *in, const size_t *offs, size_t m, uint64_t *out,
                               size_t stride_words, size_t *lg_out /*nullable*/, int *status /*nullable*/);
int halo_accumulator_decode_batch(halo_ctx *ctx /*nullable*/, const uint8_t *in, const size_t *offs, size_t m, uint64_t *out,
                                  size_t stride_words, size_t *lg_out /*nullable*/, int *status /*nullable*/);

/* ---- measurement and resource policy ------------------------------------------------------ */
/* (Experiment knobs, the primitive test hooks, halo_bench_fr_kernel and the fault injectors are NOT part of this library:
 * include/halo_accumulation_dev.h, libhalo_hip_dev.so.  Environment switches: csrc/tuning.hpp) */
/* on = 1: every kernel launch on this ctx is bracketed by hipEvents on the ctx stream;
 * on = 2: only the dominant kernels (k_msm_accumulate, k_fold_points); 0: off. */
int halo_prof_enable(halo_ctx *ctx, int on);
int halo_prof_reset(halo_ctx *ctx);
/* number of distinct kernels seen; name/total ms/launch count of entry i */
int halo_prof_count(halo_ctx *ctx);
int halo_prof_get(halo_ctx *ctx, int i, const char **name, double *total_ms, long *launches);
/* n uniform scalars (Montgomery limbs) of the SplitMix64 stream, written to DEVICE memory: the
 * synthetic-input generator of the benchmarks (element i = draws 4i+1..4i+4 after *rng_state,
 * little-endian, reduced mod r); *rng_state advances as a sequential stream would */
int halo_rng_scalars_dev(halo_ctx *ctx, uint64_t *rng_state, size_t n, void *d_out);
/* sum of k Jacobian points in index order, on the host (combine step of the sharded MSM) */
int halo_point_sum(const uint64_t *pts_jac, size_t k, uint64_t out[12]);
/* IPA tuning: comb table for the first fold of an open whose size is the context's key (E[w][d][i] = d 64^w G_i: 22
 * windows x 32 multiples x 64 bytes per point of the upper three quarters of the key = 33 KiB x n: 35.4 GB at n = 2^20, plus a
 * 4.6 GB temporary while it is built; ~0.2 s to build; the scalars are split with the curve's endomorphism, 2 x 22 entries per
 * scalar multiple; an open + check at 2^20 takes ~2.6 ms less with it, so the build pays for itself after ~64 opens).
 * -1 (default), contexts of 2^18 .. 2^21 points: nothing happens during the first 7 full-size opens over a key (counted over
 * the context and its clones) -- no memory is requested or reserved; the 8th asks for the table's memory on a helper thread
 * (40 GB at 2^20: 0.5 ms .. 2 s of hipMalloc depending on what the driver has at hand) and the first later open that finds it
 * there builds the table (environment HALO_FOLD_TABLE_AFTER=k replaces the 8; 0 = never automatically).  A caller that knows
 * it will open many times says 1: allocated and built at the next full-size open; 0: never, a table already built
 * (or requested) is released.  The table is OPTIONAL memory and subject to halo_set_memory_budget below: over the budget the
 * generic fold kernel runs (halo_ctx_info(ctx, 5) says so) and the table is considered again later.  Results are identical. */
int halo_set_fold_table(halo_ctx *ctx, int mode);
/* Budget for OPTIONAL device memory -- the MSM fixed-base table (halo_set_table_mode) and the fold table above: memory the
 * library takes on its own to be faster, never to be correct.  The budget is per DEVICE and process-wide: all contexts of
 * this process on ctx's device together never hold more optional memory than `bytes`, and no single request takes more than
 * half of what hipMemGetInfo reports free at that moment.  Default: one sixth of the device's total memory (48 GB of an
 * MI355X's 288 GB: room for the tables of ONE context over 2^20 points, 37.1 GB + the 4.6 GB temporary -- a second context
 * on the same device then runs without a fold table unless the caller raises the budget); environment
 * HALO_MEMORY_BUDGET=<bytes>[K|M|G] replaces the default for the whole process.  0 = no optional memory at all.  Lowering
 * the budget below what is held releases nothing by itself (halo_set_table_mode(ctx, 0) / halo_set_fold_table(ctx, 0) do).
 * A table that was refused or whose allocation failed is tried again later (after 8, 16, ... more opens / 64, 128, ... more
 * MSMs) and at once after this call. */
int halo_set_memory_budget(halo_ctx *ctx, size_t bytes);
/* what: 0 = bytes of the MSM fixed-base table, 1 = bytes of the fold table, 2 = microseconds the fold table took to build,
 * 3 = the budget for optional memory on this context's device, 4 = bytes of it in use (all contexts of this process on
 * that device), 5 = status of the fold table, 6 = status of the MSM table: 0 nothing yet, 1 memory requested, 2 built,
 * 3 over the budget, 4 allocation failed (tried again later), 5 switched off; 7 = microseconds the MSM table took to build
 * (without its allocation), 8 = rows of the MSM table (13 / 15: fixed windows; 255: every shift), 9 = plan of the launch
 * enqueued last (0: no table pipeline, 1: its fixed windows, w + 1: sliding windows of at most w bits), 10 = how many members of
 * the last halo_pcdl_open_batch / halo_random_instance_batch / halo_instance_from_poly_batch on this context went through
 * member-batched launches (0: they ran one at a time) */
size_t halo_ctx_info(const halo_ctx *ctx, int what);
/* MSM tuning: fixed-base tables.  -1 (default): an MSM of n >= 2^20 points over the context's own key uses the table
 * T[w][i] = 2^(20 w) G_i (13 x 128 bytes per point of the key, built on the first such MSM): 13 instead of 16 mixed
 * additions per point and one shared set of 2^19 buckets.  A context whose key has 2^17 .. 2^20 - 1 points builds
 * T[w][i] = 2^(17 w) G_i instead (15 x 128 bytes per point, 15 additions, 2^16 buckets) for MSMs over at least half of
 * its key.  0: never (no table memory).  Optional memory: subject to halo_set_memory_budget; a table that cannot be had
 * (budget, allocation) is not an error -- the table-free pipeline runs (halo_ctx_info(ctx, 6)) and the table is tried again
 * later.  Results are identical.
 * A key of >= 2^20 points on one device first asks for the ALL-SHIFTS table T[j][i] = 2^j G_i, j = 0 .. 254 (255 x 128 bytes per
 * point: 34 GB at 2^20; keys up to 2^20 points) and, with it, recodes the scalars into sliding windows of at most 21 bits that
 * start at set bits only: 12.0 additions per point instead of 13 (one MSM per launch; the IPA's tagged launch and MSMs run in
 * pieces read rows 20 w of the same table).  If the budget or the allocation refuses the 34 GB, the 13 rows are built as before.
 * The fold table has the first claim on the budget (the default budget holds one of the two), decided per key: when it is
 * refused beside an all-shifts table that only this context uses, and would fit without it, the MSM table is taken down to its
 * 13 rows -- at once by halo_set_fold_table(ctx, 1) and by halo_ctx_clone (a key with clones is a service that opens), else at
 * the next MSM enqueued with nothing in flight -- and the key keeps to 13 rows until halo_set_fold_table(ctx, 0) or a new budget.
 * A key that has clones builds the all-shifts table only if the budget holds both tables; a table that clones already share is
 * never taken from them (the fold table is then refused as over the budget, halo_ctx_info(ctx, 5) == 3).
 * 1: as -1 with the fixed windows forced: no all-shifts table is built, and one that exists is read through its row stride
 * (A/B runs, tests). */
int halo_set_table_mode(halo_ctx *ctx, int mode);


#ifdef __cplusplus
}
#endif
#endif
