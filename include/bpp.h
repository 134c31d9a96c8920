/* bpp.h -- C ABI of libbpp_hip.so, the MI355X (gfx950) engine for the Bulletproofs+ range-proof hot path.
 *
 * Drop-in boundary for tari_bulletproofs_plus 0.4.1 (reference = /root/reference, Rust).  Two seams:
 *
 *  B1 (trait level)   the three curve25519-dalek multiscalar traits the reference is generic over
 *                     (src/traits.rs:40-43, src/protocols/curve_point_protocol.rs:18-36, impl src/ristretto.rs:28-64)
 *  B2 (protocol level) the bodies of RangeProof::verify (src/range_proof.rs:756-1065, entered through
 *                     verify_batch :712-752) and RangeParameters::init (src/range_parameters.rs:32-58).
 *
 * Conventions
 *  - points cross the boundary as 32-byte canonical ristretto255 encodings, scalars as 32-byte canonical
 *    little-endian integers mod l; no C++ or torch types; caller owns every buffer; nothing is retained.
 *  - return value: 0 = Ok; 1..5 = the reference's ProofError variants (src/errors.rs:11-28); negative = engine fault.
 *  - a ctx is bound to one HIP device and one stream and serialises its own calls; batch handles belong to their ctx.
 *  - params / precomp handles are process-wide, reference-counted, read-only objects (the reference shares its
 *    generators and `Precomputation: Send + Sync` tables through Arc: src/traits.rs:42,
 *    src/generators/bulletproof_gens.rs:52,103): ANY ctx of the same device may pass a live handle, from any thread,
 *    concurrently; bpp_*_retain is Arc::clone, bpp_*_destroy is drop.  Device tables are freed when the last
 *    reference, resident batch and call in flight is gone.
 *  - every entry point fails (negative code) if no gfx950 device is usable: there is NO CPU fallback.
 */
#ifndef BPP_H
#define BPP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ProofError mapping (src/errors.rs:11-28) */
#define BPP_OK 0
#define BPP_ERR_VERIFICATION_FAILED 1
#define BPP_ERR_INVALID_ARGUMENT 2
#define BPP_ERR_INVALID_LENGTH 3
#define BPP_ERR_INVALID_BLAKE2B 4
#define BPP_ERR_SIZE_OVERFLOW 5
/* engine faults (no reference analogue) */
#define BPP_ERR_ENGINE (-1)    /* HIP runtime error, see bpp_ctx_last_error */
#define BPP_ERR_NO_DEVICE (-2) /* no usable gfx950 device */
#define BPP_ERR_BAD_HANDLE (-3)
#define BPP_ERR_COMM (-4)      /* RCCL failure (library missing, communicator error): sharded entry points only */
#define BPP_ERR_SELF_CHECK (-5) /* "prove_check" = 1: a proof the verifier rejected, made again once and rejected again;
                                   "verify_check" = 1: a group whose three verification passes gave three different outcomes */

/* Where inside RangeProof::verify (src/range_proof.rs:756-1065) a check failed.  Lower = earlier in the reference's order
 * of checks; shards of one reference batch combine their findings by (tier, rank) -- see bpp_verify_sharded. */
#define BPP_TIER_NONE 0
#define BPP_TIER_CONSTRUCTION 1     /* RangeStatement::init / RangeProof::from_bytes: before verify() is entered */
#define BPP_TIER_DEGREE 2           /* extension degree of every item (:637-659) */
#define BPP_TIER_PROMISE 3          /* minimum-value promises (:674-682) */
#define BPP_TIER_STATEMENT_POINT 4  /* a commitment does not decode (a RangeStatement holds points) */
#define BPP_TIER_PASS1 5            /* transcript replay of ANY proof (:816-850) */
#define BPP_TIER_PASS2 6            /* per proof, in proof order: decompression, L/R count (:859-888) */
#define BPP_TIER_MSM 7              /* the final multiscalar check (:1057-1062) */
#define BPP_TIER_ENGINE 255         /* an engine fault (negative code) on some rank */

/* VerifyAction (src/range_proof.rs:46-54) */
#define BPP_VERIFY_ONLY 0
#define BPP_RECOVER_AND_VERIFY 1
#define BPP_RECOVER_ONLY 2

/* MAX_RANGE_PROOF_BATCH_SIZE (src/range_proof.rs:76): pass as `chunk` for reference-sized batches */
#define BPP_REFERENCE_CHUNK 256

typedef struct bpp_ctx bpp_ctx;

/* ---- context ---- */
int bpp_ctx_create(bpp_ctx **out, int device_id);
/* same, but all work is enqueued on the caller's hipStream_t (e.g. torch's current stream) */
int bpp_ctx_create_on_stream(bpp_ctx **out, int device_id, void *hip_stream);
void bpp_ctx_destroy(bpp_ctx *ctx);
const char *bpp_ctx_last_error(bpp_ctx *ctx);
/* per-context knobs for tests and A/B timing; value -1 restores the engine's own rule.  Names: "transcripts_wave",
 * "tables_wave", "side_decompress", "msm_quad", "msm_final_quad" (0 / 1: force the one-lane or the latency form of that stage),
 * "msm_c_bias" (extra MSM window bits of small calls), "msm_c_max" (widest MSM window), "msm_c_add", "msm_rc2" (0: one window per wavefront in the bucket reduction), "msm_split",
 * "fb_threads", "prove_subs", "prove_fused" (0: three launches per prover round instead of one), "prove_prio" (1: the prover's small
 * kernels on a high-priority stream), "fused_columns" (0: per-proof generator rows + k_reduce_static instead of the column sums inside
 * k_scalars_lanes), "static_gemm" (1 / 0: those column sums as ONE integer matrix product over the proofs of a group on the
 * matrix cores, kernels_static_gemm.h, or by Montgomery products per (proof, generator); by itself the engine takes the matrix
 * product from aggregation 8 on), "lazy_columns" (0: every product of the column sums inside k_scalars_lanes reduced by itself
 * instead of one reduction per workgroup and column), "ct" (which of the SECRET-ONLY terms -- those the reference computes in
 * constant time -- take the uniform-access forms of csrc/ct.h, where no address and no branch depends on the scalar: 1 = the default:
 * bpp_pedersen_commit and the prover's witness check (src/generators/pedersen_gens.rs:112-122, src/range_proof.rs:275-284);
 * 2: A1 and B of the final round as well (:572-584; a 256-doubling ladder on the call's last stretch, see DESIGN.md for its
 * measured cost); 0: everything through the fixed-base tables, addressed by the scalars' digits).  The environment variables BPP_<NAME> give
 * "chain" (where the batch-weight chains of a verification run -- src/range_proof.rs:811,849,853,894, one strictly sequential
 * sponge per reference batch: 0 = on host cores (csrc/chain_host.h: lowest latency, 0.04 host-core-ms per 1024 proofs), 1 = on
 * the device, one wavefront per reference batch behind PASS 1 (csrc/chain_dev.h: the calling thread only enqueues and the
 * rank needs no host cores in proportion to its throughput; a zero weight, probability 2^-252, sends the call through the host
 * chains once more, which redraw as the reference does), 2 = the sponges on host cores, Scalar::from_bytes_mod_order_wide and the
 * look for a zero weight on the device (half the host time of 0), -1 = the engine's rule: 2 for calls of 4096 proofs and more, else
 * 0), "wait" (how the calling thread waits for the device: 0 = hipStreamSynchronize, which spins on a core; 1 = naps of 50 us between
 * looks at an event, 1-2 % of a core; -1 = the engine's rule: naps for calls of 4096 proofs and more), "prove_check" (1: every proof
 * bpp_prove_batch / bpp_prove_batch_mixed make on this context -- and a prove pool made from it -- is verified on this context before
 * any byte of it is returned; a rejected proof is made again once, and one rejected again fails with BPP_ERR_SELF_CHECK; see
 * bpp_prove_check_stats.  0 and -1 = off, the engine's rule), "prove_check_recovery" (1: a checked call also replays mask
 * recovery -- RecoverAndVerify, src/range_proof.rs:941-969 -- for its items that carry a seed nonce and compares the recovered
 * masks with the witness's blinding factors on the device: a proof that verifies but whose mask its owner could not get back is
 * made again once and then fails with BPP_ERR_SELF_CHECK like a rejected one; see bpp_prove_check_recovery_stats.  Acts only
 * where "prove_check" = 1; a call none of whose items carries a nonce is checked exactly as without it.  0 and -1 = off).
 * The environment variables BPP_<NAME> give
 * the initial values and are read ONCE, when the context is created: no verification path calls getenv.
 * Test knobs of "prove_check", settable here only (no environment variable, not copied to a prove pool's lanes), acting on the NEXT
 * prove call of the context and then reset: "prove_check_tamper" = i + 1 XORs "prove_check_tamper_xor" (default 0x01) into byte
 * "prove_check_tamper_byte" (default 1) of proof i in the page-locked host copy of the call's proofs, after the device wrote them and
 * before they are checked (i counts the call's items as the caller passed them); "prove_check_tamper_times" = 1 (default) alters the
 * first attempt only, 2 the remake of that proof as well.  "prove_check_tamper_nonce" = 1: the byte ("prove_check_tamper_byte"
 * 0..31) is altered in the check's own copy of item i's seed nonce instead of in the proof ("prove_check_recovery" = 1: the replay
 * then disagrees with a proof that is right; an item without a nonce is left alone).  Checked calls only.
 * "msm_plain" (1: bpp_msm_vartime, bpp_msm_vartime_batched and bpp_msm_mixed run through the plain double-and-add kernels of
 * csrc/msm_plain.h, which share nothing with the bucket method but the field and point arithmetic: a second opinion for B1
 * callers, ~30 times the work per term; 0 and -1 = off).
 * "verify_check" (1: every rejection a verification finds ON THE DEVICE is confirmed on an independent path before it is
 * returned -- see "Rechecked rejections" below, bpp_verify_check_stats; 0 and -1 = off: every call enqueues what it always did).
 * Test knobs of "verify_check", settable here only (no environment variable, never copied to a lane), acting on the NEXT verification
 * of the context -- checked or not -- and then reset: "verify_check_tamper" = bit mask of the passes to alter (1, 2, 4 = pass 1, 2, 3),
 * "verify_check_tamper_group" = the group (chunk) of the call's layout, "verify_check_tamper_kind" = 1: the group's identity flag
 * reads 0 (a false MSM rejection); 2: it reads 1 and the device bits of the group's status words are cleared (a false acceptance);
 * 3 / 4: the PASS-1 / decompression failure bit is set in the status word of the group's first proof; a value above 15 holds one
 * kind per pass, four bits each, pass 1 in the lowest.  The knobs alter bytes of
 * page-locked host memory after the wait and before findings are raised; nothing on the device is touched.  Kind 5 clears the
 * verdict of the joint final check ("verify_joint"; the group knob is not looked at), so that its fall-back runs on a valid input.
 * "verify_joint" (1: a verification pass with two or more groups, every one of them held to the final check, runs ONE multiscalar
 * multiplication over all of them and the per-group ones only when that joint check fails -- see "Joint final check" below,
 * bpp_verify_joint_stats; 0 and -1 = off: every call takes exactly the launches and buffers it always did.  For calls whose
 * batches are expected to be valid.  By rule the joint form is taken while the joint group -- 2 max_mn + t + 1 generator columns
 * and all dynamic terms of the call -- has at most 14 000 terms: pooled small calls, where it measured level or ahead; larger calls
 * stay on the per-group path, where the joint form measured slower.  2: the joint form whatever the size, for measurement).
 * "msm_prelude_slices" (S >= 2: every (group, window) sort of the bucket MSM's prelude is cut into S slices of terms, one
 * workgroup each -- histograms, a scan, the scatter, as three launches -- for every MSM of the context, bpp_msm_vartime* included;
 * at most 64.  1: the one-workgroup form for every MSM, whatever its size (A/B timing).  0 and -1 = the engine's rule: groups of
 * 200 000 terms and more, which are also the only ones that get 14-bit windows by rule). */
int bpp_ctx_set_option(bpp_ctx *ctx, const char *name, int value);
/* verifications of this context whose weights were made on the device ("chain" 1 or 2), and how many of those ran once more
 * with everything on the host because a weight came out zero */
int bpp_device_chain_stats(bpp_ctx *ctx, uint64_t *calls, uint64_t *redraws);

/* ---- runtime preconditions and the admission gate for small calls ("Runtime preconditions") ----
 * Separate callers of RangeProof::verify_batch hand over at most MAX_RANGE_PROOF_BATCH_SIZE = 256 proofs per call
 * (src/range_proof.rs:73-76,712-752).  Such a call is a chain of latency-bound kernels; the chip runs about six of them side
 * by side, and with many more in flight (every context brings a stream and a side stream onto the runtime's hardware queues)
 * all of them get slower.  The library therefore admits at most `small_call_limit` calls of <= 1024 proofs per device at a
 * time (default 12, environment BPP_SMALL_CALLS_IN_FLIGHT, 0 = no gate); the others wait their turn on the host in arrival
 * order.  Large calls pass freely.  bpp_small_call_limit sets the limit (limit < 0: query only) and returns the previous one.
 * bpp_runtime_info_get reports what the library sees: live contexts of the device, the hardware queues the HIP runtime uses
 * (GPU_MAX_HW_QUEUES as read at ITS start-up; 4 when unset -- a library cannot change it for its host), the host pool, the
 * gate's counters.  When a new context makes contexts > hw_queues, bpp_ctx_create still succeeds and leaves a note where
 * bpp_ctx_last_error finds it. */
typedef struct {
  int device;
  uint32_t contexts, contexts_peak; /* live / most ever: each owns a stream, small inputs use a second one */
  uint32_t hw_queues;               /* GPU_MAX_HW_QUEUES (4 when unset) */
  uint32_t host_threads;            /* bpp_host_threads() */
  uint32_t small_call_limit, small_calls_in_flight;
  uint64_t small_calls, small_calls_queued; /* gated calls so far; those that had to wait */
  uint32_t oversubscribed;          /* 1: contexts > hw_queues */
} bpp_runtime_info;
int bpp_runtime_info_get(bpp_ctx *ctx, bpp_runtime_info *out);
int bpp_small_call_limit(bpp_ctx *ctx, int limit);

/* ---- B1: multiscalar traits ----
 * bpp_precomp_create  = VartimePrecomputedMultiscalarMul::new(static_points)   (src/generators/bulletproof_gens.rs:103)
 * bpp_msm_mixed       = ::vartime_mixed_multiscalar_mul(static_scalars, dyn_scalars, dyn_points)
 *                        (src/range_proof.rs:339-345, :1050-1057); n_static <= table size, rest = zero padding
 * bpp_msm_vartime     = VartimeMultiscalarMul::vartime_multiscalar_mul          (src/range_proof.rs:482-495, :512-521)
 *                        VARIABLE-TIME, as the trait says: the addresses of its bucket tables are digits of its scalars.  It
 *                        is not the constant-time trait; scalars that are secrets go to bpp_msm_ct.
 * bpp_msm_ct          = MultiscalarMul::multiscalar_mul                         (src/generators/pedersen_gens.rs:112-122)
 *                        dalek's constant-time Straus, see "B1: the constant-time trait" below
 * A point that does not decode makes the call return BPP_ERR_INVALID_ARGUMENT. */
int bpp_precomp_create(bpp_ctx *ctx, const uint8_t *points32, size_t count, uint64_t *handle);
int bpp_precomp_destroy(bpp_ctx *ctx, uint64_t handle);
/* Arc::clone: `ctx` takes its own reference on a handle created by another context of the same device (dropped by
 * bpp_precomp_destroy(ctx, handle) or when ctx is destroyed) */
int bpp_precomp_retain(bpp_ctx *ctx, uint64_t handle);
int bpp_msm_mixed(bpp_ctx *ctx, uint64_t handle, const uint8_t *static_scalars32, size_t n_static,
                  const uint8_t *dyn_scalars32, const uint8_t *dyn_points32, size_t n_dyn, uint8_t out_point32[32]);
int bpp_msm_vartime(bpp_ctx *ctx, const uint8_t *scalars32, const uint8_t *points32, size_t n,
                    uint8_t out_point32[32]);
/* many independent MSMs in one launch: group g covers terms [group_off[g], group_off[g+1]) */
int bpp_msm_vartime_batched(bpp_ctx *ctx, const uint8_t *scalars32, const uint8_t *points32,
                            const uint32_t *group_off, size_t n_groups, uint8_t *out_points32 /* n_groups x 32 */);
/* diagnostics: the kernel forms the LAST multiscalar multiplication of this context took (a B1 call above, or a verification's
 * final one): out = { c (window bits), K (windows), K_wide (windows of c bits, the others have c - 1), nb (buckets per window),
 * G (groups), terms, form, dig_cap (terms per group whose digits the prelude keeps in LDS) }.  form: bit 0 = quad accumulation
 * (else one lane per bucket); bits 1-2 = the reduction, 0 rc_quad, 1 rc2, 2 rc, 3 bitsum + window; bit 3 = final_quad (else final);
 * bit 4 = 256-lane prelude (else 1024); bit 5 = the plain kernels ("msm_plain" = 1: only G, terms and this bit are set).
 * bit 6 = the constant-time kernels (bpp_msm_ct, bpp_msm_ct_batched: only G, terms and this bit are set).
 * bit 7 = the sliced prelude ("msm_prelude_slices", or by rule), bits 8-15 then hold its slices and dig_cap is 0.
 * BPP_ERR_INVALID_ARGUMENT before the first one (an empty sum launches nothing and records nothing). */
int bpp_msm_last_plan(bpp_ctx *ctx, uint32_t out[8]);

/* ---- B1: the constant-time trait, MultiscalarMul::multiscalar_mul ----
 * sum_i scalars[i] * points[i] for scalars that are SECRETS over the caller's own points: commitments under bases that are no
 * parameter set's H and G_k, blinded sums, anything written against the MultiscalarMul bound.  Arguments, group convention,
 * return codes and messages are those of bpp_msm_vartime / bpp_msm_vartime_batched, and for the same inputs so are the output
 * bytes (the canonical encoding of the same group element): a scalar that is not canonical or a point that does not decode
 * gives BPP_ERR_INVALID_ARGUMENT, an empty group 32 zero bytes, a call without terms launches nothing.
 * PUBLIC: the term counts, group_off, the points, which error is returned.  SECRET: the scalars.  No branch, no global, LDS or
 * scratch address, no launch geometry and no choice of kernel form depends on a scalar's value (csrc/ct.h: k_ct_straus -- signed
 * radix-16 digits, per term a table of the multiples 1 P .. 8 P of which EVERY entry is read for every digit and one is kept
 * under an arithmetic mask; a zero scalar, a zero digit and a term whose point is the identity cost what any other costs); the
 * canonicity check looks at every scalar of the call and decides once, at the end.  What IS data-dependent is public: the
 * doublings and additions that build a term's table are operations on the caller's points, uniform in the scalars only.
 * The scalars' host copy (page-locked), their device buffer, the per-chunk partial sums and the kernels' LDS are zeroed on every
 * exit path, error returns included; the buffers stay with the context, so a second call of the same size allocates nothing.
 * bpp_msm_ct_secret_bytes reads them back: *examined = bytes looked at (0 before the first call), *nonzero = how many were not
 * zero (0 between calls).  "msm_plain" and the bucket-method options do not reach these entry points.  Context option
 * "msm_ct_k" (BPP_MSM_CT_K): 1 / 2 = that many terms per quad of lanes (the K of k_ct_straus<K>: K terms share one accumulator's
 * doublings); 0 and -1 = the engine's rule, made from the public counts.  One launch costs what a launch costs: worth calling
 * with many outputs per call; for one commitment at a time dalek on the host is faster. */
int bpp_msm_ct(bpp_ctx *ctx, const uint8_t *scalars32, const uint8_t *points32, size_t n, uint8_t out_point32[32]);
int bpp_msm_ct_batched(bpp_ctx *ctx, const uint8_t *scalars32, const uint8_t *points32, const uint32_t *group_off,
                       size_t n_groups, uint8_t *out_points32 /* n_groups x 32 */);
int bpp_msm_ct_secret_bytes(bpp_ctx *ctx, uint64_t *examined, uint64_t *nonzero);

/* ---- B1 on the stream: constant-time sums and scalar arithmetic over DEVICE rows ----
 * What a sigma protocol around a range proof needs between the operations of bpp_transcripts_enqueue, without leaving the context's
 * stream: the commitment to a nonce that BPP_TOP_RNG_SCALARS drew (R = r G, or r0 H + r1 G0, or a sum over the caller's own bases)
 * and the response to a challenge that BPP_TOP_CHALLENGE_SCALAR left on the device (s = r + c x mod l).
 *
 * bpp_rows_msm_enqueue: out[i] = sum_{k < K} scalars[i][k] * points[i][k] for n rows, K <= BPP_ROWS_K_MAX terms each.  Rows lie at any
 * byte address; ROW SLACK (a stride above the row length) is neither read nor written.  point_stride == 0: ONE row of K bases shared
 * by every row of the call (decoded, with their multiples, once per call).
 *   live row, not void: the 32 bytes bpp_msm_ct_batched writes for a group that holds host copies of the row's K terms -- the
 *         canonical encoding of the sum, 32 zero bytes for the identity; done_mask[i] = 1; it counts in n_done.
 *   VOID  a live row with a scalar that is not canonical (>= l: BPP_ROWS_SCALAR) or a point that does not decode (BPP_ROWS_POINT; a
 *         shared base that does not decode voids every live row): 32 zero bytes, done_mask[i] = 0; it counts in n_void and competes
 *         for first_void (the lowest index wins); with both causes present both flags are set.  COMPOSITION: the zero row of a void
 *         row fed to BPP_TOP_APPEND_POINT voids that transcript row (BPP_TOPS_IDENTITY), so a void stays a void down the protocol.
 *   DEAD  live_dev[i] == 0: nothing of the row's scalars or points is read, its output row is zeroed, done_mask[i] = 0.
 * REFUSED before any launch (BPP_ERR_INVALID_ARGUMENT, the field named in bpp_ctx_last_error, the counters untouched): n or K out of
 * range; a stride below the row length (but point_stride == 0) or above 2^40; a NULL scalars_dev, points_dev or out_dev; a pointer
 * that bpp_device_pointer_check does not class BPP_PTR_THIS_DEVICE; a written range (the out rows, done_mask_dev, record_dev) that
 * overlaps any other range of the call.  live_dev, done_mask_dev, record_dev and ticket may be NULL as for bpp_transcripts_enqueue.
 * STEADY STATE: the call enqueues behind everything on the context's stream and returns -- no allocation, no copy to the host, no
 * wait (bpp_rows_stats' host_waits stays 0).  The decoded points of at most 65536 rows at a time live in a buffer of the context,
 * sized by the first call of a size; a call that grows it (or makes the ticket events) counts in first_calls.
 * PUBLIC: n, K, the strides, the points, the live mask, which rows are void.  SECRET: the scalars.  No branch, no global, LDS or
 * scratch address, no launch geometry and no choice of kernel form depends on a scalar's value (csrc/rows_msm.h: one quad of lanes
 * per term, the table walk of k_ct_straus); a row's canonicity is decided once, after all K scalars have been looked at; nothing
 * secret-derived is written to global memory but the output rows -- the row sum is reduced and compressed inside the kernel, the
 * engine keeps no copy of the scalars -- and the kernel's LDS is wiped.
 * NOT in this form: K > 16 (bpp_msm_ct_batched), a variable-time form, pool / pipeline / sharded forms.
 *
 * bpp_rows_scalar_enqueue: out[i] = a[i] * b[i] + c[i] mod l, 32 canonical little-endian bytes per row, one lane per row.  A stride of
 * 0 is one 32-byte scalar for every row; c == NULL adds nothing.  A non-canonical operand voids the row (zero output,
 * BPP_ROWS_SCALAR).  Live, dead, void, record, refusals, steady state as above; every operand is treated as a secret; out_dev may
 * alias none of the inputs (the overlap rule refuses it). */
#define BPP_ROWS_K_MAX 16
typedef struct {
  size_t n;                   /* rows, 1 .. 2^31 - 1 */
  uint32_t K;                 /* terms per row, 1 .. BPP_ROWS_K_MAX */
  const uint8_t *scalars_dev; /* DEVICE: row i = K x 32 bytes at scalars_dev + i * scalar_stride; stride >= 32 K */
  size_t scalar_stride;
  const uint8_t *points_dev;  /* DEVICE: row i = K x 32 bytes at points_dev + i * point_stride (>= 32 K), or */
  size_t point_stride;        /* point_stride == 0: ONE row of K shared bases for every row of the call */
} bpp_rows_msm;
typedef struct {
  uint32_t n_done, n_void;
  uint32_t first_void; /* 0xFFFFFFFF: none */
  uint32_t flags;      /* BPP_ROWS_WRITTEN | BPP_ROWS_SCALAR | BPP_ROWS_POINT */
} bpp_device_rows_record;
#define BPP_ROWS_WRITTEN 1u
#define BPP_ROWS_SCALAR 2u /* some live row was voided by a scalar that is not canonical */
#define BPP_ROWS_POINT 4u  /* ... by a point that does not decode */
int bpp_rows_msm_enqueue(bpp_ctx *ctx, const bpp_rows_msm *in, uint8_t *out_dev /* DEVICE: row i = 32 bytes at out_dev + i * out_stride */,
                         size_t out_stride, const uint8_t *live_dev /* DEVICE n bytes, or NULL: every row */,
                         uint8_t *done_mask_dev /* DEVICE n bytes, or NULL */, bpp_device_rows_record *record_dev /* DEVICE, or NULL */,
                         uint64_t *ticket /* or NULL; bpp_enqueue_done / bpp_enqueue_wait */);
typedef struct {
  const uint8_t *dev; /* DEVICE: row i = 32 bytes at dev + i * stride */
  size_t stride;      /* >= 32, or 0: one 32-byte scalar for every row */
} bpp_scalar_rows;
int bpp_rows_scalar_enqueue(bpp_ctx *ctx, size_t n, const bpp_scalar_rows *a, const bpp_scalar_rows *b,
                            const bpp_scalar_rows *c /* NULL: + 0 */, uint8_t *out_dev, size_t out_stride, const uint8_t *live_dev,
                            uint8_t *done_mask_dev, bpp_device_rows_record *record_dev, uint64_t *ticket);
struct bpp_rows_stats {
  uint64_t calls;       /* enqueues (of either kind) that passed the refusals */
  uint64_t first_calls; /* of them, those that made the ticket events or grew a work buffer of the context */
  uint64_t host_waits;  /* times a call waited for the device: 0 */
};
int bpp_rows_stats(bpp_ctx *ctx, struct bpp_rows_stats *out);

/* ---- B2: parameters = RangeParameters::init + BulletproofGens::new + PedersenGens ----
 * (src/range_parameters.rs:32-58, src/generators/bulletproof_gens.rs:83-112, src/ristretto.rs:67-112)
 * h_base32 / g_bases32 may be NULL: the reference's defaults (Ristretto basepoint; SHA3-512 hash-to-group of
 * "RISTRETTO_MASKING_BASEPOINT_k") are derived on the device. */
int bpp_params_create(bpp_ctx *ctx, uint32_t bit_length, uint32_t max_aggregation, uint32_t extension_degree,
                      const uint8_t *h_base32, const uint8_t *g_bases32, uint64_t *params);
int bpp_params_destroy(bpp_ctx *ctx, uint64_t params);
/* Arc::clone of a RangeParameters object (src/range_parameters.rs:20-30 holds Arc'd generators): `ctx` takes its own
 * reference on `params`, whichever context created it; one set of device tables (generators, and the prover's
 * fixed-base windows once built) serves every holder */
int bpp_params_retain(bpp_ctx *ctx, uint64_t params);
/* compressed generators, party-major like gi_base_iter()/hi_base_iter() (src/range_parameters.rs:99-106):
 * gi_out32, hi_out32: bit_length*max_aggregation x 32; h_out32: 32; g_out32: extension_degree x 32. Any may be NULL. */
int bpp_params_export(bpp_ctx *ctx, uint64_t params, uint8_t *gi_out32, uint8_t *hi_out32, uint8_t *h_out32,
                      uint8_t *g_out32);
/* PedersenGens::commit for `count` openings (src/generators/pedersen_gens.rs:112-122):
 * values[count], blindings32[count][n_blind][32] -> commitments32[count][32]; 1 <= n_blind <= extension degree */
int bpp_pedersen_commit(bpp_ctx *ctx, uint64_t params, const uint64_t *values, const uint8_t *blindings32,
                        uint32_t n_blind, size_t count, uint8_t *commitments32);

/* ---- B2: batch verification = RangeProof::verify_batch / verify ---- */
typedef struct {
  const uint8_t *proof;         /* RangeProof::to_bytes() (src/range_proof.rs:1120-1150) */
  size_t proof_len;
  const uint8_t *commitments32; /* statement.commitments_compressed, m x 32 (src/range_statement.rs:27) */
  uint32_t m;                   /* aggregation factor of this statement */
  const uint64_t *min_values;   /* m entries; value ignored where min_present[j] == 0 */
  const uint8_t *min_present;   /* m entries, Option<u64>::is_some; NULL = all None */
  const uint8_t *seed_nonce32;  /* NULL = None (src/range_statement.rs:31) */
  /* the caller's merlin::Transcript: EITHER its 203-byte STROBE state (200 state bytes, pos, pos_begin, cur_flags)
   * OR, for a fresh Transcript::new(label), the label */
  const uint8_t *transcript_state;
  const uint8_t *transcript_label;
  size_t label_len;
} bpp_verify_item;

/* One call = RangeProof::verify over every `chunk` consecutive proofs (chunk == 0: the whole batch is ONE
 * reference batch; chunk == 256 reproduces verify_batch's chunking but -- unlike src/range_proof.rs:740-751 --
 * verifies EVERY chunk, first failing chunk's error wins).
 * masks_out: n_items x extension_degree x 32 (may be NULL for BPP_VERIFY_ONLY); mask_present: n_items (may be NULL).
 * errbuf receives the reference's informational message text. */
int bpp_verify_batch(bpp_ctx *ctx, uint64_t params, const bpp_verify_item *items, size_t n_items, int action,
                     size_t chunk, uint8_t *masks_out, uint8_t *mask_present, char *errbuf, size_t errbuf_len);

/* Variant for callers that keep merlin on their side (SURVEY 8b option (i)): the Fiat-Shamir replay of PASS 1
 * (src/range_proof.rs:816-850) is done by the caller, who passes per proof
 *   challenges32[i] : (rounds_i + 3) x 32 canonical scalars  y, z, e_0 .. e_{rounds-1}, e_final   (:833-842)
 *   rng_out32       : n_items x 32, the 32 bytes drawn from transcript.to_verifier_rng(...)         (:845-848)
 * and the engine runs everything else (weight chain, decompression, PASS 2, MSM, mask recovery).  The transcript
 * fields of the items are ignored.  Identity-encoded proof members and zero challenges are still rejected. */
int bpp_verify_batch_with_challenges(bpp_ctx *ctx, uint64_t params, const bpp_verify_item *items, size_t n_items,
                                     const uint8_t *const *challenges32, const uint8_t *rng_out32, int action, size_t chunk,
                                     uint8_t *masks_out, uint8_t *mask_present, char *errbuf, size_t errbuf_len);

/* Same in two steps so a batch can stay resident in HBM: upload parses/validates/packs and copies to the device;
 * verify_resident runs only device work plus the (inherently sequential) weight chain. */
int bpp_batch_upload(bpp_ctx *ctx, uint64_t params, const bpp_verify_item *items, size_t n_items, uint64_t *batch,
                     char *errbuf, size_t errbuf_len);
int bpp_batch_destroy(bpp_ctx *ctx, uint64_t batch);
int bpp_verify_resident(bpp_ctx *ctx, uint64_t batch, int action, size_t chunk, uint8_t *masks_out,
                        uint8_t *mask_present, char *errbuf, size_t errbuf_len);
/* optional: do the one-off work of the first bpp_verify_resident(batch, ..., chunk) now -- group layout, MSM plan and
 * the allocation of every work buffer of that plan (~15 hipMallocs) -- so that no verification call pays for it */
int bpp_batch_prepare(bpp_ctx *ctx, uint64_t batch, size_t chunk);

/* ---- packed form of a homogeneous batch: what a caller of RangeProof::verify_batch(&[Transcript], &[RangeStatement],
 * &[RangeProof]) (src/range_proof.rs:712-717) holding statements and proofs of ONE shape serialises them into -- no
 * per-item pointer structs.  All proofs have the same length, all statements the same aggregation factor, one transcript
 * serves every item (benches/range_proof.rs:98, tests/ristretto.rs:225).  Same checks, same error kinds and precedence as
 * the item form (one routine checks both); results are bit-identical (tests/test_gpu_packed.py). */
typedef struct {
  size_t n_items;
  const uint8_t *proofs;           /* proof i = RangeProof::to_bytes() at proofs + i * proof_stride */
  size_t proof_len;                /* length of every proof */
  size_t proof_stride;             /* >= proof_len; == proof_len when the proofs lie back to back */
  const uint8_t *commitments32;    /* n_items x m x 32 */
  uint32_t m;                      /* aggregation factor of every statement */
  const uint64_t *min_values;      /* n_items x m */
  const uint8_t *min_present;      /* n_items x m, Option<u64>::is_some; NULL = all None */
  const uint8_t *seed_nonces32;    /* n_items x 32; NULL = all None */
  const uint8_t *seed_present;     /* n_items; NULL = every item has a nonce (when seed_nonces32 != NULL) */
  const uint8_t *transcript_state; /* 203-byte STROBE state, or NULL: Transcript::new(transcript_label) */
  const uint8_t *transcript_label;
  size_t label_len;
} bpp_packed_batch;
int bpp_batch_upload_packed(bpp_ctx *ctx, uint64_t params, const bpp_packed_batch *in, uint64_t *batch, char *errbuf,
                            size_t errbuf_len);
int bpp_verify_batch_packed(bpp_ctx *ctx, uint64_t params, const bpp_packed_batch *in, int action, size_t chunk,
                            uint8_t *masks_out, uint8_t *mask_present, char *errbuf, size_t errbuf_len);

/* ---- the packed form from arrays that already lie in DEVICE memory (a torch tensor, a buffer a NIC or another kernel wrote).
 * The struct is bpp_packed_batch as it is; for these two calls six of its fields are addresses in the memory of the context's
 * device -- proofs, commitments32, min_values, min_present, seed_nonces32, seed_present -- of the sizes given above, readable
 * until the call returns.  transcript_state, transcript_label, masks_out, mask_present and errbuf stay host memory.  The engine
 * never dereferences a caller array on the host: one kernel checks every item (first byte, canonical scalars, promises, nonce
 * present) and packs the batch where it lies; no staging, no host pass over the proofs.
 * ORDERING: whatever wrote the arrays must be complete on, or ordered before, the context's stream.  A context made with
 * bpp_ctx_create_on_stream on the producer's stream has that by construction; any other caller synchronises first.
 * POINTER KINDS: every non-null array goes through bpp_device_pointer_check before anything is allocated or launched; anything
 * but BPP_PTR_THIS_DEVICE (another device's memory, host or unknown memory, managed memory) is BPP_ERR_INVALID_ARGUMENT with the
 * field's name in errbuf.
 * RESULTS: return codes, error kinds, message texts, their precedence, chunking and masks are those of bpp_batch_upload_packed /
 * bpp_verify_batch_packed on the same bytes in host memory.  The batch is an ordinary resident batch.
 * FALLBACK: a batch whose proofs disagree in their first byte (a hostile or mixed input; the host form takes its item path for
 * it), or whose proofs / proof_len / proof_stride rule the arithmetic layout out, is copied to page-locked staging and goes
 * through the host path: same results, counted in bpp_ingest_stats.  The staged nonces are wiped on every way out.
 * SECRETS: the engine's copy of the seed nonces is the resident batch's buffer, wiped as ever; the caller's array is the caller's. */
int bpp_batch_upload_packed_device(bpp_ctx *ctx, uint64_t params, const bpp_packed_batch *in, uint64_t *batch, char *errbuf,
                                   size_t errbuf_len);
int bpp_verify_batch_packed_device(bpp_ctx *ctx, uint64_t params, const bpp_packed_batch *in, int action, size_t chunk,
                                   uint8_t *masks_out, uint8_t *mask_present, char *errbuf, size_t errbuf_len);
/* what kind of memory `p` is to this context; one runtime query, launches nothing, leaves no runtime error behind */
#define BPP_PTR_THIS_DEVICE 0     /* device memory of the context's device */
#define BPP_PTR_OTHER_DEVICE 1    /* device memory of another device */
#define BPP_PTR_HOST_OR_UNKNOWN 2 /* host memory (pageable, page-locked) or nothing the runtime knows */
#define BPP_PTR_MANAGED 3         /* managed (migrating) memory */
int bpp_device_pointer_check(bpp_ctx *ctx, const void *p, int *kind);
struct bpp_ingest_stats {
  uint64_t device_calls;        /* uploads whose check and packing ran on the device */
  uint64_t host_fallback_calls; /* uploads that were staged and took the host path */
  uint64_t fallback_bytes;      /* bytes copied to staging by those */
};
int bpp_ingest_stats(bpp_ctx *ctx, struct bpp_ingest_stats *out);

/* ---- the array form for batches of MIXED aggregation factors, in host or in device memory.  The struct has the geometry of what
 * bpp_prove_batch_mixed / bpp_prove_openings write: proofs in rows of proof_stride with proof_lens[i] bytes used, commitments in
 * rows of m_stride x 32 bytes (commit_stride = 32 x m_stride there) with m[i] entries used; the promise arrays have rows of
 * m_stride entries as well.  ROW SLACK -- proof bytes at and beyond proof_lens[i], commitment and promise entries at and beyond
 * m[i] -- is never read for a check and never copied.
 * proof_lens and m are public metadata that size the layout: they are HOST memory in every form.
 * RESULTS: for any input the four calls return what bpp_batch_upload / bpp_verify_batch return on the equivalent bpp_verify_item
 * array (item i points into the rows, all items share the one transcript source): return code, text in errbuf, the index a finding
 * names, masks and mask_present; the batch has the same bpp_batch_shape and gives the same bpp_batch_trace output.  One routine
 * decides both forms.  Two refusals are the form's own, BPP_ERR_INVALID_ARGUMENT before anything is read, with the field's name in
 * errbuf: proof_stride below a proof_lens[i], m_stride below an m[i] (and proof_lens or m null).
 * The _device calls: six fields are addresses in the memory of the context's device, as for bpp_batch_upload_packed_device --
 * proofs, commitments32, min_values, min_present, seed_nonces32, seed_present -- with the ORDERING, POINTER KINDS and SECRETS rules
 * given there; proof_lens and m are refused, field named, when the runtime knows them as device memory of any device.  One kernel
 * (k_ingest_mixed) checks every item and packs the batch where it lies; what the host can tell from m[] alone (not a power of two,
 * above the parameters' max_aggregation, a missing promise array) it tells without the kernel looking at that item, and the
 * lowest index of either kind is the call's finding.
 * FALLBACK: a batch whose proofs disagree in their first byte, or that has no proofs array, is copied to page-locked staging and
 * goes through the host form: same results, counted in bpp_ingest_stats (device uploads of this form count in the same three
 * counters).  The staged nonces are wiped on every way out.
 * THE BATCH is an ordinary resident batch: bpp_verify_resident*, the grouped forms, bpp_batch_prepare, bpp_batch_trace and
 * bpp_verify_enqueue take it.  A batch the _device upload packed on the device is refilled on the stream by
 * bpp_batch_refill_enqueue_mixed (below, behind the packed refills); bpp_batch_refill_enqueue, _count and _live, which take a
 * bpp_packed_batch, refuse it as they refuse every batch the packed device upload did not make (its shape is a vector, not four
 * numbers).  NOT BUILT: a pipeline (bpp_verify_submit_packed) or batcher form. */
typedef struct {
  size_t n_items;
  const uint8_t *proofs;           /* proof i = RangeProof::to_bytes() at proofs + i * proof_stride, proof_lens[i] bytes */
  size_t proof_stride;             /* >= every proof_lens[i] */
  const size_t *proof_lens;        /* n_items, ALWAYS HOST memory (what bpp_prove_batch_mixed writes to proof_lens) */
  const uint32_t *m;               /* n_items, ALWAYS HOST memory: aggregation factor of statement i */
  uint32_t m_stride;               /* entries per item row of the next three arrays, >= every m[i] */
  const uint8_t *commitments32;    /* n_items rows of m_stride x 32 bytes; row i holds m[i] commitments, the rest is not read */
  const uint64_t *min_values;      /* n_items x m_stride, or NULL */
  const uint8_t *min_present;      /* n_items x m_stride, or NULL = all None */
  const uint8_t *seed_nonces32;    /* n_items x 32, or NULL */
  const uint8_t *seed_present;     /* n_items, or NULL = every item has a nonce (when seed_nonces32 != NULL) */
  const uint8_t *transcript_state; /* as in bpp_packed_batch: one transcript serves every item */
  const uint8_t *transcript_label;
  size_t label_len;
} bpp_mixed_batch;
int bpp_batch_upload_mixed(bpp_ctx *ctx, uint64_t params, const bpp_mixed_batch *in, uint64_t *batch, char *errbuf, size_t errbuf_len);
int bpp_verify_batch_mixed(bpp_ctx *ctx, uint64_t params, const bpp_mixed_batch *in, int action, size_t chunk, uint8_t *masks_out,
                           uint8_t *mask_present, char *errbuf, size_t errbuf_len);
int bpp_batch_upload_mixed_device(bpp_ctx *ctx, uint64_t params, const bpp_mixed_batch *in, uint64_t *batch, char *errbuf,
                                  size_t errbuf_len);
int bpp_verify_batch_mixed_device(bpp_ctx *ctx, uint64_t params, const bpp_mixed_batch *in, int action, size_t chunk,
                                  uint8_t *masks_out, uint8_t *mask_present, char *errbuf, size_t errbuf_len);

/* Pipelined host-buffers-in verification inside ONE context.  submit parses, validates and packs `in` into page-locked
 * staging on the calling thread (construction errors are returned by submit itself, as RangeStatement::init /
 * RangeProof::from_bytes would raise them before verify_batch is entered) and returns; the caller's buffers are free again.
 * DMA, kernels and the weight chain of that call then run on one of the context's `depth` internal lanes (own stream, own
 * staging, own work buffers; default depth 3, bpp_ctx_pipeline_depth before the first submit changes it) while the caller
 * submits the next batch: upload k+1 overlaps verify k.  collect blocks until the ticket's call is done and returns exactly
 * what bpp_verify_batch_packed would have returned.  Tickets may be collected in any order; every ticket must be collected
 * (bpp_ctx_destroy waits for the ones in flight).  submit blocks while all lanes are busy. */
int bpp_ctx_pipeline_depth(bpp_ctx *ctx, uint32_t depth);
int bpp_verify_submit_packed(bpp_ctx *ctx, uint64_t params, const bpp_packed_batch *in, int action, size_t chunk,
                             uint64_t *ticket, char *errbuf, size_t errbuf_len);
int bpp_verify_collect(bpp_ctx *ctx, uint64_t ticket, uint8_t *masks_out, uint8_t *mask_present, char *errbuf,
                       size_t errbuf_len);

/* ---- phased form of the same verification, for sharding one reference batch across GPUs ----
 * phase1: PASS 1 of verify (src/range_proof.rs:816-850) for this rank's proofs -> the 32 transcript-RNG bytes per
 *         proof that feed the weight transcript (:845-849).
 * weights_from_chain: the weight transcript itself (:811,:849,:853,:894) over the WHOLE batch in global proof order
 *         (pure host function: the chain is a sequential sponge).
 * phase2: PASS 2 (:856-1033) + this rank's share of the final MSM (:1050) -> partial accumulator as 128 bytes
 *         (X,Y,Z,T canonical field elements).  Only rank 0 (include_pedersen != 0 on exactly one rank is NOT needed:
 *         every rank adds its own share of the g/h base scalars).
 * accumulators_sum_is_identity: sum of all ranks' accumulators == identity  (:1057). */
int bpp_verify_phase1(bpp_ctx *ctx, uint64_t batch, uint8_t *rng_out32 /* n_items x 32 */, char *errbuf,
                      size_t errbuf_len);
int bpp_weights_from_chain(const uint8_t *rng32_all, size_t n_total, uint8_t *weights32_out /* n_total x 32 */);
/* n_groups independent weight transcripts of n_per_group proofs each (what verify_resident runs for chunk > 0): same
 * result as n_groups calls of bpp_weights_from_chain, but the chains advance in lockstep on vector Keccak (AVX-512: 8,
 * AVX2: 4 chains per core) and bundles are spread over host threads. */
int bpp_weights_from_chains(const uint8_t *rng32_all, size_t n_groups, size_t n_per_group, uint8_t *weights32_out);
int bpp_verify_phase2(bpp_ctx *ctx, uint64_t batch, const uint8_t *weights32 /* n_items x 32 */,
                      uint8_t accumulator128[128], char *errbuf, size_t errbuf_len);
int bpp_accumulators_sum_is_identity(bpp_ctx *ctx, const uint8_t *accumulators128, size_t n, int *is_identity);

/* ---- ONE reference batch sharded over the GPUs of a node, behind the C ABI (BASELINE configs[3]) ----
 * One process (or thread) per GPU; rank r holds `counts[r]` consecutive proofs of the batch as a resident batch on its own
 * context.  bpp_verify_sharded runs RangeProof::verify (src/range_proof.rs:756-1065) over the union:
 *   PASS 1 on every rank's own proofs, decompression and the weight-free scalars right behind it
 *   -> RCCL all_gather of the 32 transcript-RNG bytes per proof (device buffers, no host hop) as soon as PASS 1 is done
 *   -> the batch-weight transcript (:811,:849,:853,:894) replayed by every rank over ALL proofs in order (a sequential
 *      sponge: cheaper to replay than to broadcast), each rank keeps the weights of its own proofs
 *   -> PASS 2 + the rank's share of the final MSM (:1050) -> one accumulator point per rank
 *   -> RCCL all_gather of the 128-byte accumulators, each with the 128-byte finding of its rank (RCCL has no group-law
 *      reduction, so the north star's "all-reduce of the accumulator" is gather + the same sum on every rank), sum and
 *      identity test (:1057) on the device; a finding of any rank comes before the final check, as in verify().
 * EVERY rank reaches both collectives whatever it found locally, and every rank returns the same result: the error the
 * single-process verify() would have raised first, decided by numeric tier (BPP_TIER_*), then lowest rank.
 * Return value: 0 Ok, 1..5 ProofError kind (same on every rank), BPP_ERR_COMM when RCCL fails (library missing,
 * communicator error: the communicator must then be destroyed), other negatives = engine fault on some rank.
 * VerifyOnly semantics (masks are per proof and need no exchange: recover them with bpp_verify_resident on the shard).
 *
 * Communicators: bpp_comm_unique_id (rank 0) -> the caller ships the 128 bytes to the other ranks over its own channel ->
 * bpp_comm_create on every rank (ncclCommInitRank: collective); or bpp_comm_adopt of an ncclComm_t the caller already
 * has; or bpp_comm_create_callbacks with the caller's own all_gather.  A communicator serialises its own calls; use one per
 * thread that verifies concurrently.
 *
 * bpp_comm_adopt does NOT take ownership: the ncclComm_t stays the caller's (it may be a framework's process-group communicator
 * in use elsewhere), bpp_comm_destroy never destroys it, and a collective that misses its deadline (bpp_comm_set_timeout) never
 * aborts it -- the handle is marked dead and the call returns BPP_ERR_COMM, and it is the OWNER who calls ncclCommAbort (which
 * also lets the collective still spinning on this rank exit).  Only communicators made by bpp_comm_create are aborted and
 * destroyed by this library. */
typedef struct bpp_comm bpp_comm;
int bpp_comm_unique_id(uint8_t id128[128]);
int bpp_comm_create(bpp_ctx *ctx, const uint8_t id128[128], int rank, int world, bpp_comm **out);
int bpp_comm_adopt(bpp_ctx *ctx, void *nccl_comm, int rank, int world, bpp_comm **out);
/* The caller's own transport instead of RCCL (its MPI / TCP / gloo channel; also how several ranks share ONE GPU, which RCCL
 * refuses): `all_gather` receives this rank's `bytes_per_rank` bytes in HOST memory and must fill recv[r * bytes_per_rank ...]
 * with rank r's block for every r (its own included), in the SAME order of calls on every rank; it blocks until that is done and
 * returns 0, or non-zero on failure (the call then returns BPP_ERR_COMM and the handle is dead).  It is called on the thread
 * that made the bpp_verify_sharded* call, two or three times per call (32 bytes per proof; weights when the chains are shared
 * out; 256 bytes per batch).  Any deadline is the transport's own: bpp_comm_set_timeout cannot interrupt a callback. */
typedef int (*bpp_all_gather_fn)(void *user, const void *send, void *recv, size_t bytes_per_rank);
int bpp_comm_create_callbacks(bpp_ctx *ctx, int rank, int world, bpp_all_gather_fn all_gather, void *user, bpp_comm **out);
/* In-process stand-in for tests on a single GPU: the `world` ranks are threads of one process, each with its own context on
 * the same device; an all_gather is a rendezvous of the threads plus device-to-device copies.  Everything else of
 * bpp_verify_sharded(_wave) is the code the RCCL form runs.  Ranks of one group pass the same (arbitrary) group_id. */
int bpp_comm_create_local(bpp_ctx *ctx, uint64_t group_id, int rank, int world, bpp_comm **out);
void bpp_comm_destroy(bpp_comm *comm);
const char *bpp_comm_last_error(bpp_comm *comm);
/* Deadline of every wait for a collective on this communicator, in ms (default 60 000, or BPP_COMM_TIMEOUT_MS at creation;
 * 0 = wait for ever; a BPP_COMM_TIMEOUT_MS that is not a number keeps the default and leaves a note in bpp_ctx_last_error).  A
 * peer that died or never made the call would leave the all_gather spinning on this rank for ever: when the deadline passes
 * the call returns BPP_ERR_COMM on every surviving rank, and so does every later call on the handle -- destroy it and build a
 * new one over the ranks that are left.  A communicator made by bpp_comm_create is aborted (ncclCommAbort) at that point; an
 * ADOPTED one is left alone, see bpp_comm_adopt. */
int bpp_comm_set_timeout(bpp_comm *comm, uint32_t timeout_ms);
int bpp_verify_sharded(bpp_comm *comm, bpp_ctx *ctx, uint64_t batch, const uint32_t *counts /* world entries */,
                       int *tier_out, int *rank_out, char *errbuf, size_t errbuf_len);
/* A WAVE of k independent sharded batches (batch i resident on ctxs[i], every rank passes its shards of the same k batches
 * in the same order, all with the same `counts`): their PASS-1 work runs concurrently on the k contexts' streams, ONE
 * coalesced all_gather carries the RNG bytes of all k, the k weight chains run side by side on the host pool, ONE all_gather
 * carries the k accumulators.  results[i] receives batch i's outcome (code as bpp_verify_sharded returns it, tier, rank,
 * message).  Return value: 0 = the wave ran (look at results), BPP_ERR_COMM / negative = the wave itself failed. */
typedef struct {
  int code, tier, rank;
  uint32_t index;       /* position in the whole batch of the proof the finding belongs to (tiers checked per proof) */
  char msg[160];
} bpp_shard_result;
int bpp_verify_sharded_wave(bpp_comm *comm, bpp_ctx *const *ctxs, const uint64_t *batches, size_t k, const uint32_t *counts,
                            bpp_shard_result *results);
/* The GROUPED form: this rank's shards of n_groups independent reference batches (same `counts` for all) are ONE resident
 * batch on ONE context -- group g = proofs [g c, (g+1) c) of it, c = counts[rank] > 0 -- so every verifier kernel is
 * launched once for all groups (as bpp_verify_resident does with chunk = c) and each of the two all_gathers carries all
 * groups.  results[g] = group g's outcome, exactly as a bpp_verify_sharded call on that batch alone would give it.  The form
 * for many batches with small shards: a wave of k contexts pays a dozen launches and a stream per batch, this pays them
 * once.  With several ranks the weight chains are shared out (rank r replays those of groups r, r + world, ...) and a third
 * all_gather hands every rank all weights: the sequential replay, not the GPUs, bounds the rate when every rank replays
 * every chain.  src/range_proof.rs:712-752 (one reference batch per group), :811-853 (its weight chain over all ranks' proofs). */
int bpp_verify_sharded_groups(bpp_comm *comm, bpp_ctx *ctx, uint64_t batch, size_t n_groups, const uint32_t *counts,
                              bpp_shard_result *results /* n_groups */);
/* k grouped batches (batch i resident on ctxs[i], every one holding n_groups x counts[rank] proofs) as a software pipeline of
 * ONE host thread on ONE communicator: phase 1 of all k is enqueued; then, batch by batch, the first exchange, the weight
 * chains and the enqueueing of phase 2 (while the other batches' kernels keep the GPU busy); then, batch by batch, the findings
 * and the second exchange.  Every rank issues its collectives in the same order by construction, which calls from several
 * host threads on several communicators cannot promise.  results: k x n_groups, batch-major. */
int bpp_verify_sharded_groups_wave(bpp_comm *comm, bpp_ctx *const *ctxs, const uint64_t *batches, size_t k, size_t n_groups,
                                   const uint32_t *counts, bpp_shard_result *results /* k x n_groups */);

/* ---- pooled small calls ----
 * Reference batches of different sizes as the groups of ONE engine call: group g = proofs [group_first[g], group_first[g+1])
 * of the resident batch (group_first[0] = 0, group_first[n_groups] = the batch size), every group verified as its own
 * verify() (VerifyOnly) with its own outcome in results[g] (code, tier, index inside the group, message; rank = -1). */
int bpp_verify_resident_groups(bpp_ctx *ctx, uint64_t batch, const uint32_t *group_first, size_t n_groups, bpp_shard_result *results);
/* The same with a VerifyAction PER GROUP (src/range_proof.rs:46-54; actions == NULL: VerifyOnly everywhere) and the masks of
 * the groups that recover them (:941-969): masks_out n_items x extension_degree x 32, mask_present n_items (either may be
 * NULL).  A group gets its masks only where its own verify() would have returned Ok; every other slot is zero / absent.  A
 * RecoverOnly group is never held to the final check (:1040-1043); when every group is RecoverOnly neither the weight chains
 * nor PASS 2 run. */
int bpp_verify_resident_groups_actions(bpp_ctx *ctx, uint64_t batch, const uint32_t *group_first, size_t n_groups, const int *actions,
                                       bpp_shard_result *results, uint8_t *masks_out, uint8_t *mask_present);

/* ---- stream-ordered calls that leave their verdicts on the device ----
 * bpp_verify_enqueue is the stream-ordered counterpart of bpp_verify_resident_groups_actions: the same groups (explicit
 * boundaries, or group_first == NULL: equal chunks of `chunk` proofs, 0 = one group), the same VerifyAction per group (actions ==
 * NULL: action_all everywhere), the same outcomes -- but it ENQUEUES on the context's stream and returns.  One 16-byte record per
 * group and the recovered masks land in DEVICE buffers the caller names; they are valid in stream order behind the call, so work
 * the caller puts on the same stream afterwards (bpp_ctx_create_on_stream) may read them with no host round trip, and one thread
 * can enqueue step after step, over one or several contexts, without waiting.
 *
 * RECORDS: verdicts_dev[g] = {code, tier, index, flags} of group g as the blocking call would report them (tier BPP_TIER_NONE and
 * code 0: its verify() returned Ok; index counts inside the group).  flags always carries BPP_VERDICT_WRITTEN (the buffer may start
 * out as anything).  BPP_VERDICT_REDRAW: one of the call's device weights came out zero (probability 2^-252 per proof); every group
 * that needed weights then claims NOTHING else -- code 0, tier 0 -- and gets no masks: run a blocking call on the batch, which
 * redraws on the host as the reference does.  bpp_verdict_result turns a host copy of a record into a bpp_shard_result with the
 * message text of the blocking calls.
 * MASKS: masks_dev n x extension_degree x 32 (16-byte aligned) and mask_present_dev n, either may be NULL.  A group gets the masks
 * of its items that carry a seed nonce when its verdict is Ok and its action recovers; every other slot is zero / absent.  A
 * RecoverOnly group is never held to the final check and keeps its masks whatever the final MSM says.  The engine's own copy is
 * wiped by the rules of every resident batch; the caller's buffer is the caller's.
 * LAUNCHES: those of the blocking call -- PASS 1, the weight chains (always as kernels, in line on the stream, whatever "chain"
 * says), decompression, PASS 2, the final MSM -- then two kernels that resolve the reference's error precedence on the device.  The
 * early-outs that depend only on what the host knows are kept: one group with a deferred finding enqueues the verdict kernels alone,
 * one group with a bad L/R count PASS 1 and those, and a call whose groups are all RecoverOnly runs neither chains nor PASS 2.
 * STEADY STATE: the call allocates nothing, copies nothing to the host and waits for nothing.  The FIRST enqueue of a (batch,
 * layout) does what bpp_batch_prepare does, stream synchronisation included (layouts_in_call counts these); a layout change on a
 * batch that has tickets in flight waits for them first (host_waits counts these, and nothing else ever does).  The same batch may
 * be enqueued again while an earlier enqueue of the same layout is in flight: the stream orders them.
 * REFUSED, before anything is launched (BPP_ERR_INVALID_ARGUMENT, the reason in bpp_ctx_last_error): a buffer that is not
 * BPP_PTR_THIS_DEVICE memory by bpp_device_pointer_check (the field is named), bad boundaries, an empty group, an unknown action;
 * "verify_check" = 1 (a promise this path cannot keep: the recheck is decided on the host); a batch whose verification hands out
 * transcript states.  An unknown batch is BPP_ERR_BAD_HANDLE.  The joint final check ("verify_joint") and stage profiling need
 * host decisions and are silently not taken.  Enqueued calls do not pass the small-call gate (they are serial on their stream)
 * and teach the wait hints nothing.
 * TICKETS: bpp_enqueue_done is one event query, bpp_enqueue_wait blocks until the call's results are there -- for callers that do
 * want the host to know.  bpp_batch_destroy and bpp_ctx_destroy synchronise the stream and thereby retire every ticket. */
typedef struct {
  int32_t code;
  uint32_t tier;
  uint32_t index;
  uint32_t flags;
} bpp_device_verdict; /* 16 bytes */
#define BPP_VERDICT_WRITTEN 1u /* set by the call: the caller's buffer may start out as anything */
#define BPP_VERDICT_REDRAW 2u  /* a device weight came out zero (2^-252): nothing claimed, run a blocking call */
int bpp_verify_enqueue(bpp_ctx *ctx, uint64_t batch, const uint32_t *group_first /* NULL: equal chunks */, size_t n_groups, size_t chunk,
                       const int *actions /* NULL: action_all */, int action_all, bpp_device_verdict *verdicts_dev /* n_groups */,
                       uint8_t *masks_dev /* n x t x 32, may be NULL */, uint8_t *mask_present_dev /* n, may be NULL */, uint64_t *ticket);
int bpp_enqueue_done(bpp_ctx *ctx, uint64_t ticket, int *done); /* one event query */
int bpp_enqueue_wait(bpp_ctx *ctx, uint64_t ticket);            /* for callers that do want the host to know */
/* code, tier, index and the blocking calls' message text of a record copied to the host (rank = -1); a redraw record comes back as
 * code 0 / tier 0 with a message that says so.  BPP_ERR_INVALID_ARGUMENT for a record the call never wrote. */
int bpp_verdict_result(const bpp_device_verdict *host_copy, bpp_shard_result *out);
struct bpp_enqueue_stats {
  uint64_t calls, groups, host_waits, layouts_in_call;
};
int bpp_enqueue_stats(bpp_ctx *ctx, struct bpp_enqueue_stats *out);

/* ---- refill a resident batch from device arrays on the stream ----
 * bpp_batch_refill_enqueue replaces the CONTENTS of a resident batch with the packed batch `in_dev` -- the six array fields are
 * addresses in the memory of the context's device, as for bpp_batch_upload_packed_device -- and keeps its SHAPE: item count,
 * aggregation factor, proof length, first byte of the proofs, whether seed_nonces32 was given, whether min_values and min_present
 * were given.  It ENQUEUES on the context's stream and returns.  A bpp_verify_enqueue on the batch afterwards gives, group for
 * group, exactly what it would give on a fresh bpp_batch_upload_packed_device of the same arrays: byte-identical records, masks
 * and mask_present.  Together the two calls are a steady state with no host round trip for a producer that writes proofs into
 * device buffers and a consumer that reads verdicts on the same stream.
 * ORDERING: the stream's.  The arrays must be complete on, or ordered before, the context's stream and stay readable until the
 * refill has run; an earlier enqueue of the batch still in flight is ordered before the refill.
 * WHICH BATCHES: one made by bpp_batch_upload_packed_device that did not take the staged fall-back.  A batch of any other origin
 * (item form, host packed form, caller-side challenges) is refused.
 * REFUSED, before anything is launched (BPP_ERR_INVALID_ARGUMENT, the reason in bpp_ctx_last_error; an unknown batch is
 * BPP_ERR_BAD_HANDLE): a shape field of `in_dev` that differs from the batch's (the field is named); proof_stride < proof_len; a
 * non-null transcript_state or transcript_label (the batch keeps its transcript); a non-null array or record_dev that is not
 * BPP_PTR_THIS_DEVICE memory (the field is named).
 * FINDINGS STAY ON THE DEVICE: where the blocking upload fails with the lowest-index construction finding, the refill writes
 * {code, message id, index} with BPP_REFILL_FINDING into record_dev and into a word of the batch.  Every verdict record of every
 * later enqueue on that batch, until the next refill, then carries BPP_VERDICT_WRITTEN | BPP_VERDICT_REFILL, the refill's code,
 * tier BPP_TIER_CONSTRUCTION, the index inside the BATCH, and no masks.  A proof whose first byte is not the batch's sets
 * BPP_REFILL_FALLBACK (it comes before any finding, as in the blocking upload, which stages such a batch and takes the host path):
 * the refill cannot plan again on the device, so nothing is claimed -- code 0, tier 0 under BPP_VERDICT_REFILL -- and the caller
 * uploads those arrays with a blocking call.  An item with a finding or a foreign first byte is NOT copied: its slot holds the
 * batch's first byte and zeros, no nonce, no promises, zero commitments, so that no verification kernel ever sees bytes the
 * blocking upload would have stopped.
 * STEADY STATE: the call allocates nothing, copies nothing to the host and waits for nothing (host_waits stays 0).  The first
 * refill of a batch allocates its few device words (first_calls).  bpp_verify_enqueue behind a refill plans nothing again when its
 * layout is the current one, and takes its general branch where it would otherwise decide by what the host knew of the old
 * contents.
 * A REFILLED BATCH IS STREAM-OWNED: the blocking verify entry points, the sharded and phased forms and bpp_batch_trace refuse it
 * (upload the arrays for a blocking call); bpp_batch_destroy, bpp_batch_shape, bpp_batch_prepare and bpp_batch_secret_bytes work.
 * SECRETS: the old nonces are overwritten by the new ones or by zeros, and the engine's mask rows of the batch are wiped.
 * TICKETS are those of bpp_verify_enqueue: bpp_enqueue_done and bpp_enqueue_wait take them. */
typedef struct {
  int32_t code;   /* ProofError kind of the finding (BPP_ERR_ENGINE for an internal one), 0 without one */
  uint32_t msg;   /* message id of the finding; bpp_refill_result gives the text */
  uint32_t index; /* the item, counted inside the batch */
  uint32_t flags;
} bpp_device_refill; /* 16 bytes */
#define BPP_REFILL_WRITTEN 1u  /* always set by the call */
#define BPP_REFILL_FINDING 2u  /* code / msg / index: the lowest-index construction finding, as the blocking upload reports it */
#define BPP_REFILL_FALLBACK 4u /* some proof's first byte is not the batch's: nothing claimed, upload with a blocking call */
#define BPP_VERDICT_REFILL 4u  /* in bpp_device_verdict.flags: the batch's last refill did not take; see its refill record */
int bpp_batch_refill_enqueue(bpp_ctx *ctx, uint64_t batch, const bpp_packed_batch *in_dev, bpp_device_refill *record_dev /* may be NULL */,
                             uint64_t *ticket /* may be NULL */);
/* code, index and message text of a record copied to the host (tier BPP_TIER_CONSTRUCTION for a finding, rank = -1); a fall-back
 * record comes back as code 0 / tier 0 with a message that says so.  BPP_ERR_INVALID_ARGUMENT for a record the call never wrote. */
int bpp_refill_result(const bpp_device_refill *host_copy, bpp_shard_result *out);
struct bpp_refill_stats {
  uint64_t calls, first_calls, host_waits;
};
int bpp_refill_stats(bpp_ctx *ctx, struct bpp_refill_stats *out);

/* ---- a refill with fewer items than the batch holds ----
 * bpp_batch_refill_enqueue_count is bpp_batch_refill_enqueue with a LIVE COUNT c that is read ON THE STREAM, when the refill kernel
 * runs: `count_dev` is one 32-bit word in BPP_PTR_THIS_DEVICE memory (anything else is refused before any launch, the field named)
 * and the host never learns it.  `in_dev` keeps the batch's shape exactly: n_items is the batch's N and the arrays are N items
 * long.  count_dev == NULL is bpp_batch_refill_enqueue: the same launches and the same bytes.
 * After a refill with c (0 <= c <= N) a bpp_verify_enqueue on the batch gives, for every group that holds a live item, byte for byte
 * what it gives on a fresh bpp_batch_upload_packed_device of the FIRST c ITEMS with the same boundaries clipped to c: the group
 * [p0, p1) runs over [p0, min(p1, c)), its weight transcript absorbs and draws those proofs alone, `index` counts inside the group.
 * A group with p0 >= c gets {0, BPP_TIER_NONE, 0, BPP_VERDICT_WRITTEN | BPP_VERDICT_EMPTY} and no masks.  masks_dev rows and
 * mask_present_dev bytes of items i >= c are zero.  BPP_VERDICT_REDRAW is raised by a zero weight of a live item only and claimed
 * by groups that hold one.
 * ITEMS i >= c are neither checked (a non-canonical scalar, a foreign first byte, a missing nonce there is neither a finding nor a
 * fall-back) nor copied: their slots hold the batch's first byte and zeros, zero commitments, no promises, no nonce -- what the
 * slot of a refused item holds -- and their mask rows are wiped.  They still pass through the per-proof kernels with weight zero:
 * a dead slot costs what a live one does.
 * c > N sets BPP_REFILL_COUNT in the refill record (before BPP_REFILL_FALLBACK and before any finding): every slot is cleared as
 * above, nothing is live, and every later verdict carries BPP_VERDICT_REFILL with code 0 and tier 0 until the next refill.
 * The batch keeps the clamped count in a device word of its own, written by the refill; later enqueues read that word and never
 * the caller's, which may be overwritten as soon as the refill has run.  STEADY STATE as for bpp_batch_refill_enqueue. */
#define BPP_REFILL_COUNT 8u   /* in bpp_device_refill.flags: the live count exceeds the batch's item count; nothing claimed */
#define BPP_VERDICT_EMPTY 8u  /* in bpp_device_verdict.flags: the group holds no live item of the batch's last refill */
int bpp_batch_refill_enqueue_count(bpp_ctx *ctx, uint64_t batch, const bpp_packed_batch *in_dev,
                                   const uint32_t *count_dev /* one word in device memory; NULL: every item */,
                                   bpp_device_refill *record_dev /* may be NULL */, uint64_t *ticket /* may be NULL */);
/* ---- a refill under a per-item live mask ----
 * bpp_batch_refill_enqueue_live is bpp_batch_refill_enqueue with a LIVE MASK that is read ON THE STREAM, when the refill kernel runs:
 * `live_dev` is N bytes in BPP_PTR_THIS_DEVICE memory (anything else is refused before any launch, the field named) and the host
 * never learns it.  Byte i non-zero means item i is live; any non-zero value counts.  The refill copies the NORMALISED mask (0 / 1)
 * into a buffer of the batch's own; later kernels read that copy and never the caller's array, which may be overwritten as soon as
 * the refill has run.  `in_dev` keeps the batch's shape exactly, as for the count form.  live_dev == NULL is
 * bpp_batch_refill_enqueue: the same launches and the same bytes.
 * DEAD ITEMS (byte zero) are neither checked (a non-canonical scalar, a foreign first byte, a missing nonce there is neither a finding
 * nor a fall-back) nor read; their slots are sanitised exactly as the count form's dead slots are: the batch's first byte and zeros,
 * zero commitments, no promise, no nonce, mask rows wiped.  The refill record's `index` for a construction finding stays the item's
 * index inside the batch, which is its slot.
 * After such a refill a bpp_verify_enqueue with boundaries group_first gives, with S_g the live slots of group g in slot order:
 *   S_g not empty: what a fresh bpp_batch_upload_packed_device of the items of S_g ALONE, in slot order, gives for them verified as
 *     one group: code, tier and flags are equal, the weight transcript absorbs and draws those proofs alone in that order.  `index`
 *     is a SLOT OFFSET inside the group, p - p0 of the proof that raised the finding: the slot of the fresh upload's k-th item,
 *     so a consumer finds the proof without a prefix sum.
 *   S_g empty: {0, BPP_TIER_NONE, 0, BPP_VERDICT_WRITTEN | BPP_VERDICT_EMPTY}, wherever the group lies -- also before live groups.
 *   masks_dev rows and mask_present_dev bytes sit at their slots, as always: live slots carry the fresh upload's, dead slots zeros.
 *   BPP_VERDICT_REDRAW is raised by a zero weight of a live item only.  bpp_enqueue_weights gives the fresh upload's weights at
 *     the live slots and 32 zero bytes at dead ones.
 * FORM: a batch is in the form of its last refill -- plain, count or mask.  A count refill after a mask refill drops the mask, and
 * the other way round.  A batch that never took a mask allocates nothing for one; the first mask refill of a batch allocates its N
 * bytes (counted under first_calls).  STEADY STATE, refused-before-launch rules, stream ownership, secrets and tickets are those of
 * bpp_batch_refill_enqueue: host_waits stays 0, and a later bpp_verify_enqueue plans nothing again (layouts_in_call does not move).
 * COST: a dead slot still passes through the per-proof kernels with weight zero and costs what a live one does. */
int bpp_batch_refill_enqueue_live(bpp_ctx *ctx, uint64_t batch, const bpp_packed_batch *in_dev,
                                  const uint8_t *live_dev /* N bytes in device memory; NULL: every item */,
                                  bpp_device_refill *record_dev /* may be NULL */, uint64_t *ticket /* may be NULL */);
/* ---- a refill of a batch of MIXED aggregation factors ----
 * bpp_batch_refill_enqueue_mixed is the three calls above for a batch that bpp_batch_upload_mixed_device packed on the device (not its
 * staged fall-back, not the host mixed form, not a packed or item batch, not one with caller-side challenges or one that hands out
 * states: refused with a text of this call's own).  The SHAPE such a refill keeps is the vector (proof_lens[i], m[i]) per slot, the
 * item count, the first byte, and which of seed_nonces32, seed_present, min_values and min_present were given.
 * `in_dev`: the six array fields are BPP_PTR_THIS_DEVICE addresses, as for the _device upload.  proof_stride and m_stride describe the
 * SOURCE rows and may differ from the upload's; they must hold the batch's longest proof and largest m.  proof_lens and m are HOST
 * memory (device memory is refused, field named) and must repeat the batch's vectors entry for entry -- the first differing index and
 * its field are named -- or are BOTH NULL, "the batch's own vectors": the steady-state form, in which the host touches nothing of
 * size N.  One without the other is refused.  The transcript fields must be NULL.
 * count_dev / live_dev: at most one of them (both: refused); NULL and NULL is the plain form.  Their meaning, DEAD SLOTS, the record,
 * the flags (a count beyond the batch before the fall-back before a finding), FORM, STEADY STATE, stream ownership, secrets and
 * tickets are those given above, with "a fresh bpp_batch_upload_mixed_device of the same rows" (all of them / the first c / each
 * group's live rows alone in slot order) in place of the packed upload.  A slot that is not taken -- dead, a construction finding, a
 * foreign first byte -- is sanitised with ITS OWN lengths: the first byte and proof_lens[i] - 1 zeros, 32 x m[i] zero commitment bytes.
 * Row slack is never read, and nothing at all of a dead row: the source arrays may end behind the last live row.
 * Everything is refused before any launch, BPP_ERR_INVALID_ARGUMENT with the reason in bpp_ctx_last_error.
 * SLOT CLASSES: a producer of mixed traffic sizes one batch as k1 slots of m = 1, k2 of m = 2, ... (each class with its proof
 * length), uploads it once and refills it under a mask every step, leaving the slots it has no proof for dead.
 * COST: a dead slot costs what a live one does. */
int bpp_batch_refill_enqueue_mixed(bpp_ctx *ctx, uint64_t batch, const bpp_mixed_batch *in_dev,
                                   const uint32_t *count_dev /* one device word, or NULL */,
                                   const uint8_t *live_dev /* N device bytes, or NULL */,
                                   bpp_device_refill *record_dev /* may be NULL */, uint64_t *ticket /* may be NULL */);
/* ---- per-item transcripts on the device paths: in at upload and refill, out at enqueue ----
 * The reference's verify_batch takes one transcript per proof and advances each in place.  The array forms above serve ONE transcript
 * to every item; these calls give the _device forms the item form's contract (bpp_verify_item.transcript_state) with no host round
 * trip.
 * IN.  item_states203: n_items rows of 203 bytes in BPP_PTR_THIS_DEVICE memory, at any byte address; row i is the STROBE state
 * (state[200] | pos | pos_begin | cur_flags, as bpp_transcript_new / _append_message leave it) item i is verified under.  The two
 * uploads return, for any input, what bpp_batch_upload returns on the item array whose item i has transcript_state = row i: return
 * code, text, the index a finding names, bpp_batch_shape, every bpp_batch_trace output, and the verdicts and masks of every later
 * call.  in->transcript_state and in->transcript_label must be NULL (refused, field named); item_states203 that is NULL or not this
 * device's memory is refused before any launch, field named.  A row with pos >= 166 (the STROBE-128 rate) is the item form's finding "transcript
 * state has pos >= rate", raised at the lowest item that has one and, among the findings of one item, after everything the proof's
 * parse raises; such a row is never copied, its slot holds 203 zero bytes.  A batch that takes the staged fall-back (first bytes that
 * disagree, no proofs) stages the state rows with the rest and goes through the item form; bpp_ingest_stats counts it as ever.
 * REFILLS.  "Uploaded with per-item transcripts" is part of the shape a batch keeps: the two refills below take only batches the two
 * uploads below made on their device path, and bpp_batch_refill_enqueue / _count / _live / _mixed refuse such a batch; either text
 * names the call to use instead.  count_dev / live_dev (at most one; NULL and NULL is the plain form), the record and its flags, DEAD
 * SLOTS, FORM, STEADY STATE, stream ownership, secrets, tickets and refused-before-launch are those of the refills above, with "a
 * fresh upload WITH TRANSCRIPTS of the rows in question" (all of them / the first c / each group's live rows alone in slot order) as
 * the reference.  Nothing of a dead row's state is read and its slot gets 203 zero bytes; a bad state there is no finding.  A bad
 * state at a live slot lands in the record under BPP_REFILL_FINDING with the item form's code and message id, with the precedence
 * given above.
 * OUT.  bpp_verify_enqueue_states is bpp_verify_enqueue plus states_out203_dev (N x 203 bytes of BPP_PTR_THIS_DEVICE memory at any
 * byte address; NULL is refused).  It takes every batch that call takes (one transcript or one per item; not caller-side challenges,
 * which ran no PASS 1 here).  Verdict records, masks and mask_present are byte for byte bpp_verify_enqueue's.  Row i is written on
 * every call: where item i's group has the record {0, BPP_TIER_NONE, 0, BPP_VERDICT_WRITTEN} exactly and slot i is live, the 203
 * bytes bpp_verify_batch_states writes for that item (the transcript after r1, s1 and every d1); everywhere else -- dead slots,
 * rejected groups, BPP_VERDICT_EMPTY, _REDRAW and _REFILL -- 203 zero bytes, which no Merlin state is.  The first such call on a
 * batch may allocate the engine's row buffer; after that it allocates nothing, copies nothing to the host and waits for nothing. */
int bpp_batch_upload_packed_device_transcripts(bpp_ctx *ctx, uint64_t params, const bpp_packed_batch *in,
                                               const uint8_t *item_states203 /* n_items x 203, device */, uint64_t *batch, char *errbuf,
                                               size_t errbuf_len);
int bpp_batch_upload_mixed_device_transcripts(bpp_ctx *ctx, uint64_t params, const bpp_mixed_batch *in,
                                              const uint8_t *item_states203 /* n_items x 203, device */, uint64_t *batch, char *errbuf,
                                              size_t errbuf_len);
int bpp_batch_refill_enqueue_transcripts(bpp_ctx *ctx, uint64_t batch, const bpp_packed_batch *in_dev,
                                         const uint8_t *item_states203_dev /* N x 203, device */,
                                         const uint32_t *count_dev /* one device word, or NULL */,
                                         const uint8_t *live_dev /* N device bytes, or NULL */,
                                         bpp_device_refill *record_dev /* may be NULL */, uint64_t *ticket /* may be NULL */);
int bpp_batch_refill_enqueue_mixed_transcripts(bpp_ctx *ctx, uint64_t batch, const bpp_mixed_batch *in_dev,
                                               const uint8_t *item_states203_dev /* N x 203, device */,
                                               const uint32_t *count_dev /* one device word, or NULL */,
                                               const uint8_t *live_dev /* N device bytes, or NULL */,
                                               bpp_device_refill *record_dev /* may be NULL */, uint64_t *ticket /* may be NULL */);
int bpp_verify_enqueue_states(bpp_ctx *ctx, uint64_t batch, const uint32_t *group_first /* NULL: equal chunks */, size_t n_groups, size_t chunk,
                              const int *actions /* NULL: action_all for every group */, int action_all, bpp_device_verdict *verdicts_dev,
                              uint8_t *masks_dev /* may be NULL */, uint8_t *mask_present_dev /* may be NULL */,
                              uint8_t *states_out203_dev /* N x 203, device */, uint64_t *ticket);
/* A diagnostic: enqueues a device-to-device copy of the batch weights that the batch's last enqueued verification used, N x 32
 * canonical bytes, into weights_dev (BPP_PTR_THIS_DEVICE memory); dead slots hold 32 zero bytes.  Allocates nothing and does not
 * wait.  BPP_ERR_INVALID_ARGUMENT for a batch whose last call on the stream was not an enqueue that drew weights. */
int bpp_enqueue_weights(bpp_ctx *ctx, uint64_t batch, uint8_t *weights_dev /* N x 32, device */, uint64_t *ticket /* may be NULL */);

/* bpp_batcher: many host threads, each with ONE reference batch per call.  Separate small calls stop at about 5 000 calls per
 * second whatever the number of callers (a small call is a chain of latency-bound kernels and the chip runs about six of those
 * side by side); the batcher pools the calls that are waiting into grouped engine calls (bpp_verify_resident_groups) on
 * `lanes` contexts of its own (the first one is `ctx`; 0 = the default of two), without a thread of its own: whichever caller finds a lane free
 * leads the next pooled call for everybody queued behind it.  bpp_batcher_verify blocks and returns exactly what
 * bpp_verify_batch_packed(ctx, params, in, BPP_VERIFY_ONLY, 0, ...) would: 0 or the ProofError kind, message in errbuf.
 * `shape` fixes what can be pooled (proof_len, m, transcript label; other inputs are verified on their own).  max_wait_us:
 * how long a leader waits for company (0: takes what is there); max_calls: most batches per pooled call (0: 64). */
typedef struct bpp_batcher bpp_batcher;
int bpp_batcher_create(bpp_ctx *ctx, uint64_t params, const bpp_packed_batch *shape, uint32_t lanes, uint32_t max_wait_us, uint32_t max_calls,
                       bpp_batcher **out);
int bpp_batcher_verify(bpp_batcher *b, const bpp_packed_batch *in, char *errbuf, size_t errbuf_len);
/* Any VerifyAction through the pool (round 4): returns exactly what bpp_verify_batch_packed(ctx, params, in, action, 0,
 * masks_out, mask_present, ...) would -- the caller's own seed nonces in (in->seed_nonces32), its own masks out.  Calls pool
 * whatever their shape (proof length, aggregation factor, transcript label or state: the pooled upload goes through the item
 * form, out of the callers' buffers); RecoverOnly calls (a wallet scanning outputs: no final check, :1040-1043) pool among
 * themselves.  `shape` of bpp_batcher_create is no longer needed and may be NULL.  Secrets: nonces are read where the caller
 * keeps them, masks pass through the lane's buffers, which are wiped before the lane is handed on. */
int bpp_batcher_verify_action(bpp_batcher *b, const bpp_packed_batch *in, int action, uint8_t *masks_out, uint8_t *mask_present,
                              char *errbuf, size_t errbuf_len);
/* most requests (0: keep) and most proofs (0: keep; default 16384) of one pooled call */
int bpp_batcher_set_limits(bpp_batcher *b, uint32_t max_calls, uint32_t max_proofs);
/* the largest pooled call so far: requests and proofs in it (never above the limits) */
int bpp_batcher_largest_pool(bpp_batcher *b, uint32_t *calls, uint32_t *proofs);
int bpp_batcher_stats(bpp_batcher *b, uint64_t *pooled_calls, uint64_t *engine_calls, uint64_t *solo_calls);
void bpp_batcher_destroy(bpp_batcher *b); /* waits for the calls in flight; no call may start once it has been called */
/* host wall-clock split of the last wave on `comm` (ms): enqueueing phase 1 on the k streams, the first exchange (waits for
 * PASS 1 only: all_gather, RNG bytes down), the k weight chains, enqueueing phase 2, waiting for the k streams, the second
 * exchange with the sum and identity test (wait1_ms is always 0 since the first exchange no longer waits for all of phase 1) */
typedef struct {
  float enqueue1_ms, wait1_ms, gather1_ms, chains_ms, enqueue2_ms, wait2_ms, gather2_ms;
  uint32_t batches;
} bpp_shard_timing;
int bpp_comm_last_timing(bpp_comm *comm, bpp_shard_timing *out);
/* host-only pieces of the above, exported for callers that bring their own transport and for the CPU tests
 * (tests/test_dist_gloo.py): the 128-byte finding a rank contributes, and the rule every rank applies to the gathered ones.
 *   bpp_shard_local_trailer: first finding of a rank's n proofs from the per-proof facts -- defer[i] (bit 0: extension
 *     degree differs, bit 1: promise too large; may be NULL), status[i] (bit 0 PASS-1 failure, bit 1 proof point does not
 *     decode, bit 2 commitment does not decode), rounds_bad[i] (0, 3 = InvalidLength, 5 = SizeOverflow) -- in the
 *     reference's order of checks; first_index = position of the rank's first proof in the whole batch
 *   bpp_shard_trailer: a finding given directly (tier, code, index, message)
 *   bpp_shard_resolve: trailer of rank r at trailers + r * stride -> the winning finding; returns its code (0: all clean) */
#define BPP_SHARD_TRAILER_BYTES 128
int bpp_shard_local_trailer(const uint8_t *defer, const uint32_t *status, const uint8_t *rounds_bad, uint32_t n,
                            uint32_t first_index, uint8_t trailer_out[BPP_SHARD_TRAILER_BYTES]);
int bpp_shard_trailer(int tier, int code, uint32_t index, const char *msg, uint8_t trailer_out[BPP_SHARD_TRAILER_BYTES]);
int bpp_shard_resolve(const uint8_t *trailers, size_t stride, int world, int *tier_out, int *rank_out, uint32_t *index_out,
                      char *errbuf, size_t errbuf_len);

/* ---- B2: batch prover = RangeProof::prove_with_rng (src/range_proof.rs:232-608), one call for n independent proofs ----
 * Every item is one (statement, witness, transcript, rng) quadruple of the reference API:
 *   values/blindings32  RangeWitness: per opening v (u64) and r[0..t) (src/commitment_opening.rs:14-37)
 *   commitments32       statement.commitments_compressed; each must equal commit(v_j, r_j) (:275-284)
 *   min_values/min_present, seed_nonce32   as in bpp_verify_item (src/range_statement.rs:21-32)
 *   transcript_*        the caller's merlin::Transcript (state or Transcript::new(label))
 *   rng_bytes           what the external `rng` would have returned: (rounds + 3) draws of 32 bytes, rounds = log2(m * n)
 *                       (the reference pulls exactly that many through TranscriptRngBuilder::finalize)
 * All items of one call must share the aggregation factor m.  Output: to_bytes() of each proof, 1 + 32*(t + 5 + 2*rounds)
 * bytes, written at proofs_out + i * proof_stride; *proof_len receives that length.  Same inputs -> same bytes as the
 * reference (any equivalent schedule yields identical canonical encodings). */
typedef struct {
  const uint64_t *values;        /* m */
  const uint8_t *blindings32;    /* m x t x 32 */
  const uint8_t *commitments32;  /* m x 32 */
  uint32_t m;
  const uint64_t *min_values;
  const uint8_t *min_present;    /* NULL = all None */
  const uint8_t *seed_nonce32;   /* NULL = None; only with m == 1 */
  const uint8_t *transcript_state;
  const uint8_t *transcript_label;
  size_t label_len;
  const uint8_t *rng_bytes;
  size_t rng_len;                /* >= (rounds + 3) * 32 */
} bpp_prove_item;
int bpp_prove_batch(bpp_ctx *ctx, uint64_t params, const bpp_prove_item *items, size_t n_items, uint8_t *proofs_out,
                    size_t proof_stride, size_t *proof_len, char *errbuf, size_t errbuf_len);
/* The same for items of DIFFERENT aggregation factors: each item's m is any power of two up to the parameters' m_max
 * (RangeProof::prove_with_rng takes any such statement).  Proof i is written at proofs_out + i * proof_stride; its length,
 * 1 + 32*(t + 5 + 2*rounds_i), goes to proof_lens[i] (0 for an m no statement can have).  item_status[i] (may be NULL) receives
 * the code a one-item bpp_prove_batch on that item would return; a failed item's slot is zeroed and never stops the others.
 * Returns 0 when every item succeeds, else the first failing item's code, with its message in errbuf.  Every proof equals, byte
 * for byte, the one bpp_prove_batch makes of the same item.  bpp_prove_batch itself still takes one m per call. */
int bpp_prove_batch_mixed(bpp_ctx *ctx, uint64_t params, const bpp_prove_item *items, size_t n_items, uint8_t *proofs_out,
                          size_t proof_stride, size_t *proof_lens, int *item_status, char *errbuf, size_t errbuf_len);
/* the message that goes with item_status[i] = `status` of a bpp_prove_batch_mixed call on `item` (same params and proof_stride):
 * what a one-item bpp_prove_batch would have written to errbuf.  Host-side work only; returns the item's code.  For
 * BPP_ERR_SELF_CHECK the text says whether the verifier rejected the proof or mask recovery did not return the witness's blinding
 * factors ("prove_check_recovery"): that is looked up in what ctx's LAST bpp_prove_batch_mixed left behind (the item is known by its
 * first commitment), so ask before the next mixed call on that context. */
int bpp_prove_item_message(bpp_ctx *ctx, uint64_t params, const bpp_prove_item *item, size_t proof_stride, int status, char *errbuf,
                           size_t errbuf_len);
/* Prove from the openings alone: bpp_prove_batch_mixed -- mixed aggregation factors, per-item status, a failed item never stops the
 * others -- with one rule added.  An item with commitments32 == NULL has its m_i commitments commit(v_j, r_j) made by the engine (the
 * witness check computes them anyway, through the uniform-access lines under "ct" >= 1), and they are the statement's commitments
 * for everything that follows: the transcript, the proof, the self-check.  An item that brings commitments32 is handled as by
 * bpp_prove_batch_mixed (its witness check can fail with "Witness opening is invalid!").  For every item that succeeds its m_i x 32
 * commitment bytes are written at commitments_out + i * commit_stride: the made ones, or the brought ones.  A failed item's slot is
 * zeroed in commitments_out and in proofs_out.  commitments_out == NULL fails the call with BPP_ERR_INVALID_ARGUMENT;
 * commit_stride < 32 * m_i fails that item with BPP_ERR_INVALID_LENGTH ("commit_stride too small", checked after proof_stride).
 * For an item without commitments, the commitment bytes and the proof bytes equal what bpp_pedersen_commit followed by a one-item
 * bpp_prove_batch on that item give.  The existing entry points still refuse an item without commitments. */
int bpp_prove_openings(bpp_ctx *ctx, uint64_t params, const bpp_prove_item *items, size_t n_items, uint8_t *commitments_out,
                       size_t commit_stride, uint8_t *proofs_out, size_t proof_stride, size_t *proof_lens, int *item_status,
                       char *errbuf, size_t errbuf_len);
/* bpp_prove_item_message for an item of a bpp_prove_openings call (same params, commit_stride and proof_stride).  The lookup behind
 * BPP_ERR_SELF_CHECK knows an item by its first commitment; for an item that brought none that is the one the engine made, which
 * the caller passes as first_commitment32 (a failed item's slot of commitments_out is zero: bpp_pedersen_commit of its first
 * opening gives it).  NULL for an item that brought its own; NULL for one that did not: the text then names the verifier's
 * rejection.  Looks at what ctx's LAST bpp_prove_openings or bpp_prove_batch_mixed left behind. */
int bpp_prove_openings_item_message(bpp_ctx *ctx, uint64_t params, const bpp_prove_item *item, const uint8_t *first_commitment32,
                                    size_t commit_stride, size_t proof_stride, int status, char *errbuf, size_t errbuf_len);
/* ---- Proving from arrays in DEVICE memory: bpp_prove_openings whose openings lie on the device and whose proofs and commitments stay
 * there, in the row geometry bpp_mixed_batch describes (bpp_batch_upload_mixed_device and bpp_batch_refill_enqueue_mixed take the
 * outputs as they are).  No witness byte -- value, blinding factor, nonce, rng byte -- exists in host memory in this form.
 * THE CONTRACT: the call writes what bpp_prove_openings writes on the equivalent bpp_prove_item array (item i points into row i of
 * host copies of the same arrays; commitments32 is its row, or NULL when the array is NULL): the return code, errbuf, item_status[i],
 * proof_lens[i], the proof and commitment bytes, the zeroed slots of failed items.  status_dev[i] carries item i's code and a
 * BPP_PROVE_MSG_* id, which bpp_prove_status_result turns into the host form's text.  A failed item never stops the others.  Row slack
 * is never read and never written: not in the inputs, not in the output rows beyond proof_lens[i] / 32 * m[i] bytes.
 * (One corner: a failed item's ranges are zeroed in EVERY call, also in one in which no item passes the host's part of the checks,
 * where bpp_prove_openings returns before it zeroes anything.)
 * TWO DIFFERENCES from the equivalent items, both because the transcript and the strides belong to the call and the host sees no
 * witness byte: a transcript_state with pos (byte 200) >= 166 refuses the WHOLE call before any launch ("transcript state has pos >=
 * rate"); and an item that has both a nonce with m > 1 and an rng_stride too short for its m reports the rng finding ("not enough
 * external randomness..."), where the host form reports "Mask recovery is not supported...".
 * REFUSED before anything is allocated or launched, BPP_ERR_INVALID_ARGUMENT with the field named in bpp_ctx_last_error: a non-NULL
 * array of in_dev, proofs_out_dev, commitments_out_dev or status_dev that is not BPP_PTR_THIS_DEVICE memory; m in device memory;
 * commitments_out_dev or proofs_out_dev NULL; m_stride == 0; "prove_check" = 1 on the context (the self-check remakes from host
 * items and is not part of this form: the call says so instead of skipping it).
 * ORDERING: whatever wrote the input arrays must be complete on, or ordered before, the context's stream.  The call is blocking: when
 * it returns the outputs are complete for every stream.
 * SECRETS: the witness is packed by a kernel into the prove arena, which is zeroed behind the call's last kernel as for every prove
 * call; bpp_prove_secret_bytes reads 0 afterwards on every exit path. */
typedef struct {
  size_t n_items;
  const uint32_t *m;              /* HOST, n_items: aggregation factor per item (it sizes the layout, like bpp_mixed_batch.m) */
  uint32_t m_stride;              /* the per-opening arrays have rows of m_stride entries */
  const uint64_t *values;         /* DEVICE  n x m_stride (little-endian words, at any byte address) */
  const uint8_t *blindings32;     /* DEVICE  n x m_stride x t x 32 */
  const uint8_t *commitments32;   /* DEVICE  n x m_stride x 32, or NULL: every item's commitments are made (bpp_prove_openings' rule) */
  const uint64_t *min_values;     /* DEVICE  n x m_stride, or NULL */
  const uint8_t *min_present;     /* DEVICE  n x m_stride, or NULL = all None (min_present without min_values: every item fails) */
  const uint8_t *seed_nonces32;   /* DEVICE  n x 32, or NULL */
  const uint8_t *seed_present;    /* DEVICE  n, or NULL = every item has one when seed_nonces32 is given */
  const uint8_t *rng_bytes;       /* DEVICE  n x rng_stride: row i holds (rounds_i + 3) x 32 bytes of external randomness */
  size_t rng_stride;
  const uint8_t *transcript_state, *transcript_label; /* HOST: ONE transcript for the call, as in bpp_packed_batch */
  size_t label_len;
} bpp_prove_arrays;
typedef struct {
  int32_t code;  /* what item_status[i] holds */
  uint32_t msg;  /* BPP_PROVE_MSG_*; bpp_prove_status_result gives the text */
} bpp_device_prove_status; /* 8 bytes */
#define BPP_PROVE_MSG_OK 0u
#define BPP_PROVE_MSG_POWER_OF_TWO 1u
#define BPP_PROVE_MSG_GENERATORS 2u
#define BPP_PROVE_MSG_BITS 3u
#define BPP_PROVE_MSG_PROOF_STRIDE 4u
#define BPP_PROVE_MSG_COMMIT_STRIDE 5u
#define BPP_PROVE_MSG_NULL_FIELD 6u
#define BPP_PROVE_MSG_SEED_AGGREGATED 7u
#define BPP_PROVE_MSG_RNG_LEN 8u
#define BPP_PROVE_MSG_VALUE 9u
#define BPP_PROVE_MSG_MINIMUM 10u
#define BPP_PROVE_MSG_BLINDING 11u
#define BPP_PROVE_MSG_SEED_NONCE 12u
#define BPP_PROVE_MSG_TRANSCRIPT_STATE 13u
#define BPP_PROVE_MSG_OPENING 14u
#define BPP_PROVE_MSG_IDENTITY 15u
#define BPP_PROVE_MSG_ENGINE 16u
int bpp_prove_openings_device(bpp_ctx *ctx, uint64_t params, const bpp_prove_arrays *in_dev,
                              uint8_t *commitments_out_dev, size_t commit_stride, /* DEVICE, row i: 32 x m[i] bytes used */
                              uint8_t *proofs_out_dev, size_t proof_stride,       /* DEVICE, row i: proof_lens[i] bytes used */
                              size_t *proof_lens,                                 /* HOST out, n_items */
                              bpp_device_prove_status *status_dev,                /* DEVICE out, n_items; may be NULL */
                              int *item_status,                                   /* HOST out, n_items; may be NULL */
                              char *errbuf, size_t errbuf_len);
/* bpp_prove_openings_device with ONE TRANSCRIPT PER ITEM in device memory going in, and the advanced transcripts coming out: the
 * reference's prove_with_rng(&mut Transcript, ...) per proof, the prover's counterpart of bpp_batch_upload_mixed_device_transcripts
 * and bpp_verify_enqueue_states.  THE CONTRACT: the call writes what bpp_prove_openings_states writes on the equivalent bpp_prove_item
 * array whose item i has transcript_state = row i of item_states_dev -- return code, errbuf, item_status, proof_lens, proof and
 * commitment bytes, zeroed slots.  Everything bpp_prove_openings_device documents holds unchanged.
 * item_states_dev given: in_dev->transcript_state and transcript_label must both be NULL (else BPP_ERR_INVALID_ARGUMENT before anything
 * is allocated or launched).  A row whose byte 200 (pos) is >= 166 is THAT ITEM's finding ("transcript state has pos >= rate",
 * BPP_PROVE_MSG_TRANSCRIPT_STATE), last in the item's precedence as in the host form; the item fails, the others go on.  Nothing of
 * such a row but byte 200 is read, and rows of items the host refuses are never read.  The call-wide head of every transcript (domain
 * separator, H, G bases, N, T, M) is applied on the device: the host never sees a state.
 * item_states_dev NULL: the call's one transcript applies exactly as in bpp_prove_openings_device (whole-call refusal at pos >= 166).
 * states_out_dev given: row i receives the 203 bytes bpp_prove_openings_states gives for an item that succeeds -- the transcript as
 * challenge_final_e leaves it -- and 203 zero bytes for every failed or refused item, also in a call in which no item passes the
 * host's checks.  Rows are dense (stride 203) at any byte address; no byte beyond row n_items - 1 is written.
 * Both NULL: identical to bpp_prove_openings_device.
 * REFUSED before any launch, in addition: either array not BPP_PTR_THIS_DEVICE memory; the two n_items x 203 ranges overlap.
 * bpp_prove_device_stats counts a transcript finding as a device finding. */
int bpp_prove_openings_device_transcripts(bpp_ctx *ctx, uint64_t params, const bpp_prove_arrays *in_dev,
                                          const uint8_t *item_states_dev,             /* DEVICE n_items x 203, row i = item i's STROBE state; or NULL */
                                          uint8_t *commitments_out_dev, size_t commit_stride, uint8_t *proofs_out_dev, size_t proof_stride,
                                          size_t *proof_lens,
                                          uint8_t *states_out_dev,                    /* DEVICE n_items x 203 out; or NULL */
                                          bpp_device_prove_status *status_dev, int *item_status, char *errbuf, size_t errbuf_len);
/* code and message text of a status record copied to the host (tier BPP_TIER_CONSTRUCTION for a finding, rank = -1, index 0) */
int bpp_prove_status_result(const bpp_device_prove_status *host_copy, bpp_shard_result *out);
struct bpp_prove_device_stats {
  uint64_t calls;           /* calls that passed the refusals */
  uint64_t items;           /* their items */
  uint64_t device_findings; /* items the ingest kernel failed (a finding that needs a witness byte) */
  uint64_t host_findings;   /* items the host failed from m[] and the strides: they never reached the device */
};
int bpp_prove_device_stats(bpp_ctx *ctx, struct bpp_prove_device_stats *out);

/* ---- Proving ON THE STREAM from a RESIDENT PLAN: bpp_prove_openings_device(_transcripts) without its host work per call.  The plan
 * keeps the shape of a call -- n_items, m[], the strides, which optional arrays are given, the call's one transcript -- and does ONCE
 * what the blocking call does per call from host knowledge: the per-item host checks, the sort by aggregation factor, the layout, the
 * sub-batch cut and the arena (the plan's own, zeroed once), the fixed-base table, the streams, the refused-items table and the
 * sorted descriptor / row / state tables, which stay in page-locked memory of the plan that no later call rewrites.
 * bpp_prove_plan_create: `shape` is read for its geometry only; no device array of it is dereferenced or classified, a non-NULL pointer
 * means "will be given".  m must be host memory and is copied.  The transcript (label, or 203-byte state: pos >= 166 refuses the plan
 * as it refuses the blocking call) is copied too.  flags: BPP_PROVE_PLAN_ITEM_STATES -- every enqueue brings one transcript row per
 * item, and shape's transcript fields must be NULL.  The plan takes the context's options as they are now ("ct", "prove_parts",
 * "prove_subs", "prove_fused", ...), as the prove lanes do; "prove_check" = 1 refuses the plan with the blocking call's text.  An
 * m_stride below an m[i] the layout holds refuses the plan, as it refuses the blocking call.
 * bpp_prove_plan_shape: proof_lens[i] and (host_status, may be NULL) the code of an item the host's part of the checks refuses, else
 * 0 -- functions of m[] and the strides: the host learns nothing per step.
 * bpp_prove_plan_destroy waits for the plan's work in flight and frees what it owns; bpp_ctx_destroy does the same for every plan.
 *
 * bpp_prove_enqueue.  THE CONTRACT: for every live item the call writes what bpp_prove_openings_device_transcripts writes on the same
 * arrays -- proof bytes, commitment bytes, the status record, the state row, zeroed slots for failed and refused items; row slack is
 * neither read nor written; the plan's strides are the call's.  in_dev must repeat the plan's shape (n_items, m_stride, rng_stride,
 * the same optional arrays given); m is NULL ("the plan's own": the host touches nothing of size N) or a HOST array equal to the
 * plan's (the first differing index is named).  in_dev's transcript fields are not read (they must be NULL on an ITEM_STATES plan):
 * the transcript is the plan's.
 * live_dev (n device bytes, or NULL = every item): byte i == 0 makes item i DEAD.  Nothing of its rows is read -- no value, blinding
 * factor, nonce, rng byte or state byte -- its slot runs the substitute witness (it costs what a live slot costs: the launch geometry
 * never depends on the mask), its proof, commitment and state ranges are zeroed and its status is {0, BPP_PROVE_MSG_EMPTY}.  (An item
 * the host refuses from m[] keeps its finding whatever the mask says.)
 * ok_mask_dev (n device bytes, or NULL): byte i = 1 where item i's outcome is OK, else 0 (failed, refused and dead items): the mask
 * bpp_batch_refill_enqueue_mixed(..., live_dev = ok_mask_dev, ...) takes as it is.
 * summary_dev (or NULL): one record written behind everything else.  index = the smallest item index whose outcome is a finding, code
 * and msg that item's -- the return code and message of the blocking call -- and the counts; without a finding {0, 0, 0, WRITTEN, ...}.
 * bpp_prove_summary_result gives a host copy the blocking call's text (tier BPP_TIER_CONSTRUCTION, index = the item).
 * ORDERING: the call enqueues behind everything on the context's stream and returns.  Its sub-batch streams fork from an event
 * recorded on the context's stream and every one of them is joined back into it behind its arena wipe: the next operation on the
 * context's stream -- a refill, a caller's kernel on a bpp_ctx_create_on_stream context, the next enqueue -- sees complete outputs.
 * Not capturable into a HIP graph.  Blocking prove calls on the same context stay legal; the shared streams order them.
 * STEADY STATE: after a plan's first enqueue the call allocates nothing, copies nothing to the host and waits for nothing
 * (bpp_prove_enqueue_stats: host_waits stays 0, allocations and first_calls stay); it enqueues small host-to-device copies of the
 * plan's constant tables from the plan's page-locked memory, which also put back what a kernel changed in them.
 * REFUSED before any launch (BPP_ERR_INVALID_ARGUMENT, the field named in bpp_ctx_last_error): a given array, output, live_dev,
 * ok_mask_dev or summary_dev that is not BPP_PTR_THIS_DEVICE memory; proofs_out_dev or commitments_out_dev NULL; item_states_dev given
 * without the flag or missing with it; an optional array given or absent against the plan; a shape field that differs; overlapping
 * state ranges.  An unknown plan is BPP_ERR_BAD_HANDLE.  A refused call leaves the counters alone.
 * TICKETS are those of bpp_enqueue_done / bpp_enqueue_wait.
 * SECRETS: nothing witness-derived exists in host memory; every sub-batch's arena range is zeroed on its stream behind its last
 * kernel.  bpp_prove_secret_bytes covers the plans' arenas and reads 0 once the ticket is done.  On a HIP error inside the call the
 * arena is wiped before the call returns (that path alone synchronises, and counts a host wait). */
#define BPP_PROVE_PLAN_ITEM_STATES 1u
int bpp_prove_plan_create(bpp_ctx *ctx, uint64_t params, const bpp_prove_arrays *shape, size_t commit_stride, size_t proof_stride,
                          uint32_t flags, uint64_t *plan, char *errbuf, size_t errbuf_len);
int bpp_prove_plan_shape(bpp_ctx *ctx, uint64_t plan, size_t *proof_lens /* HOST out, n_items */,
                         int *host_status /* HOST out, n_items; may be NULL */);
int bpp_prove_plan_destroy(bpp_ctx *ctx, uint64_t plan);
typedef struct {
  int32_t code;   /* the blocking call's return code: the first failing item's, 0 without one */
  uint32_t msg;   /* its BPP_PROVE_MSG_* id */
  uint32_t index; /* that item */
  uint32_t flags; /* BPP_PROVE_SUMMARY_WRITTEN */
  uint32_t n_ok, n_failed, n_empty, reserved;
} bpp_device_prove_summary; /* 32 bytes */
#define BPP_PROVE_SUMMARY_WRITTEN 1u
#define BPP_PROVE_MSG_EMPTY 17u /* a slot the live mask switched off: code 0 */
int bpp_prove_enqueue(bpp_ctx *ctx, uint64_t plan, const bpp_prove_arrays *in_dev,
                      const uint8_t *item_states_dev,      /* DEVICE n x 203, iff the plan has BPP_PROVE_PLAN_ITEM_STATES */
                      const uint8_t *live_dev,             /* DEVICE n bytes, or NULL: every item */
                      uint8_t *commitments_out_dev, uint8_t *proofs_out_dev,
                      uint8_t *states_out_dev,             /* DEVICE n x 203, or NULL */
                      bpp_device_prove_status *status_dev, /* DEVICE n, or NULL */
                      uint8_t *ok_mask_dev,                /* DEVICE n bytes, or NULL */
                      bpp_device_prove_summary *summary_dev /* DEVICE, or NULL */, uint64_t *ticket /* or NULL */);
int bpp_prove_summary_result(const bpp_device_prove_summary *host_copy, bpp_shard_result *out);
struct bpp_prove_enqueue_stats {
  uint64_t calls;       /* enqueues that passed the refusals */
  uint64_t first_calls; /* of them, the first of their plan */
  uint64_t host_waits;  /* times an enqueue waited for the device: 0 unless a HIP error made it wipe the arena */
  uint64_t allocations; /* allocations made inside an enqueue (the context's ticket events, once) */
};
int bpp_prove_enqueue_stats(bpp_ctx *ctx, struct bpp_prove_enqueue_stats *out);

/* bpp_prove_pool: many host threads, each with a few proofs per call (one output of a wallet service, say).  A call of one proof
 * is a chain of latency-bound launches; the pool hands the calls that are waiting to ONE bpp_prove_batch_mixed on one of `lanes`
 * contexts (the first is ctx; the others are made here with ctx's options as they are now).  No thread of its own: whichever
 * caller finds a lane free leads the next pooled call for everybody queued (plus whatever arrives within max_wait_us), up to
 * max_calls calls and max_proofs proofs (bpp_prove_pool_set_limits; 0 keeps a limit).  bpp_prove_pool_prove blocks and returns
 * exactly what bpp_prove_batch_mixed(ctx, params, its items, ..., NULL, ...) would: the same bytes, lengths, code and message.
 * Calls of more than max_proofs items, or whose stride is too short, go through a call of their own.  Secrets: witness bytes are
 * read where the caller keeps them and wiped from the engine's staging before the lane is handed on.  Stats: callers served in
 * pooled calls, engine calls, calls that ran alone, and the largest pool so far.  destroy waits for the calls in flight. */
typedef struct bpp_prove_pool bpp_prove_pool;
int bpp_prove_pool_create(bpp_ctx *ctx, uint64_t params, uint32_t lanes, uint32_t max_wait_us, uint32_t max_calls,
                          bpp_prove_pool **out);
int bpp_prove_pool_prove(bpp_prove_pool *p, const bpp_prove_item *items, size_t n_items, uint8_t *proofs_out,
                         size_t proof_stride, size_t *proof_lens, char *errbuf, size_t errbuf_len);
int bpp_prove_pool_set_limits(bpp_prove_pool *p, uint32_t max_calls, uint32_t max_proofs);
int bpp_prove_pool_stats(bpp_prove_pool *p, uint64_t *pooled_calls, uint64_t *engine_calls, uint64_t *solo_calls,
                         uint32_t *largest_calls, uint32_t *largest_proofs);
void bpp_prove_pool_destroy(bpp_prove_pool *p);
/* bpp_prove_openings through the pool: to it what bpp_prove_pool_prove is to bpp_prove_batch_mixed (the same bytes, lengths, code and
 * message).  Requests of both kinds share pooled calls.  Stats: requests of this kind so far, and pooled engine calls that held
 * requests of both kinds (either pointer may be NULL). */
int bpp_prove_pool_openings(bpp_prove_pool *p, const bpp_prove_item *items, size_t n_items, uint8_t *commitments_out,
                            size_t commit_stride, uint8_t *proofs_out, size_t proof_stride, size_t *proof_lens, char *errbuf,
                            size_t errbuf_len);
int bpp_prove_pool_openings_stats(bpp_prove_pool *p, uint64_t *openings_calls, uint64_t *both_kinds_calls);
/* What the self-check ("prove_check" = 1) of a context has done: prove calls checked, proofs checked (those the device made without
 * a finding of its own), calls whose checking batch was rejected, proofs made again, proofs that failed with BPP_ERR_SELF_CHECK.
 * The remake's own check is counted in `remade` / `failed` only.  A struct tag, like POSIX's struct stat and stat(): a typedef
 * cannot share the function's name.  bpp_prove_pool_check_stats sums the pool's lanes (its first lane is the context it was made
 * from, whose other calls count as well). */
struct bpp_prove_check_stats {
  uint64_t calls, proofs, batch_failures, remade, failed;
};
int bpp_prove_check_stats(bpp_ctx *ctx, struct bpp_prove_check_stats *out);
int bpp_prove_pool_check_stats(bpp_prove_pool *p, struct bpp_prove_check_stats *out);
/* "prove_check_recovery" = 1: proofs with a seed nonce whose mask recovery a call's first check replayed (those the verifier
 * accepted), and how many of them did not return the witness's blinding factors.  A call whose only finding is such a mismatch
 * counts in batch_failures above, its proof in remade and, if its remake's replay differs again, in failed; a remake's own replay
 * is not counted here.  Either pointer may be NULL.  The pool's form sums its lanes. */
int bpp_prove_check_recovery_stats(bpp_ctx *ctx, uint64_t *replayed, uint64_t *mismatched);
int bpp_prove_pool_check_recovery_stats(bpp_prove_pool *p, uint64_t *replayed, uint64_t *mismatched);
/* ---- Rechecked rejections ("verify_check" = 1) ----
 * A VerificationFailed or InvalidArgument found on the device rests on one run through one set of kernel forms and one MSM
 * plan; a node that rejects a valid block because of a slip in one form has forked itself off the chain.  With the option on,
 * the one verification flow behind bpp_verify_batch(_packed), bpp_verify_batch_with_challenges, bpp_verify_resident,
 * bpp_verify_resident_groups(_actions), the packed pipeline's lanes and bpp_batcher does this:
 *   pass 1  today's run, launch for launch.  No group with a device-tier finding (BPP_TIER_PASS1, BPP_TIER_PASS2, BPP_TIER_MSM):
 *           the call ends here and has enqueued nothing extra.
 *   pass 2  the same layout once more under the complementary form of every stage that has one (DESIGN.md 4.1 has the table);
 *           the final MSM of the rechecked groups -- those with a device-tier finding in pass 1 -- runs through the plain
 *           double-and-add kernels (csrc/msm_plain.h); the other groups' MSM is not run, their pass-1 Ok stands.
 *   A group is CONFIRMED when pass 2 gives the same code, tier and index.  Otherwise
 *   pass 3  under pass 1's forms breaks the tie: the outcome two passes share is returned -- it may be Ok, with that pass's masks --
 *           and a group whose three outcomes all differ gets BPP_ERR_SELF_CHECK with a message naming them.
 * A confirmed rejection returns byte for byte what the unchecked call returns: code, tier, index, message, zeroed mask slots.
 * The batch's cached plan and the context's options are as before when the call returns.  The zero-weight redraw rule applies
 * to each pass.  Lanes (pipeline, batcher) copy the option when they are made.
 * LEFT ALONE: host-tier findings (tiers 1-4: nothing ran on the device), accepted groups (re-verifying them costs a second MSM
 * per call), the sharded entry points, and the prover's self-check ("prove_check"), whose verifications always run with the
 * recheck off: a proof it rejects is made again anyway, and its counters keep their meaning.
 * Both paths share field.h / point.h, the decompression and the host sponge code: a systematic error there is wrong twice.
 *
 * bpp_verify_check_resolve is the agreement rule as pure host code, usable without a device (like bpp_shard_resolve):
 * passes[0 .. n_passes) are one group's outcomes in pass order (tier BPP_TIER_NONE = Ok; rank and msg are carried along).
 * Returns 0 when the group is decided -- *out is what to return, *kind says how -- 1 when one more pass is needed (*kind =
 * BPP_VCHECK_PENDING, *out untouched), BPP_ERR_INVALID_ARGUMENT for null arguments or n_passes outside 1..3. */
#define BPP_VCHECK_NOT_RECHECKED 0 /* pass 1 has no device-tier finding: it stands */
#define BPP_VCHECK_CONFIRMED 1     /* pass 2 agrees with pass 1 */
#define BPP_VCHECK_UPHELD 2        /* pass 2 differed, pass 3 agrees with pass 1: pass 1's outcome */
#define BPP_VCHECK_OVERTURNED 3    /* passes 2 and 3 agree with each other and not with pass 1: their outcome */
#define BPP_VCHECK_UNDECIDED 4     /* three different outcomes: BPP_ERR_SELF_CHECK, tier BPP_TIER_ENGINE */
#define BPP_VCHECK_PENDING 5
int bpp_verify_check_resolve(const bpp_shard_result *passes, int n_passes, bpp_shard_result *out, int *kind);
/* What the rechecks of a context have done: verifications that ran with the option on, groups with a device-tier finding in
 * pass 1, those whose returned outcome is pass 1's (confirmed by pass 2, or upheld by pass 3), those whose returned outcome is
 * NOT pass 1's, groups that needed pass 3, groups with three different outcomes.  bpp_verify_check_stats adds the counts of
 * the context's pipeline lanes, bpp_batcher_verify_check_stats those of a batcher's lanes (its first lane is the context it was
 * made from, whose other calls count as well). */
struct bpp_verify_check_stats {
  uint64_t calls, rechecked_groups, confirmed, overturned, tie_breaks, undecided;
};
int bpp_verify_check_stats(bpp_ctx *ctx, struct bpp_verify_check_stats *out);
int bpp_batcher_verify_check_stats(bpp_batcher *b, struct bpp_verify_check_stats *out);

/* ---- Joint final check ("verify_joint" = 1) ----
 * A call that carries G reference batches runs G multiscalar multiplications over the same 2 max_mn + t + 1 generator columns.
 * With the option on, a pass of the one verification flow (bpp_verify_batch*, bpp_verify_resident with chunk > 0,
 * bpp_verify_resident_groups(_actions), bpp_verify_resident_states, the packed pipeline's lanes, bpp_batcher) takes the joint path
 * when it has G >= 2 groups, no group's action is RecoverOnly, it is not pass 2 of "verify_check", it got as far as PASS 2 and its
 * joint group is within the rule's term bound (see the option's text):
 *   1  PASS 1, the weight chains (every group keeps the weights of ITS OWN chain), masks and the scalar stage run as always;
 *   2  the joint row J[c] = sum_g static[g][c] mod l is formed on the device and ONE MSM runs over one group: the generator columns
 *      under J, then every dynamic term of the call with the scalar it already has;
 *   3  the identity: every group counts as having passed the final check; findings from status bits, deferred checks and L/R
 *      counts are raised per group in the usual order;
 *   4  anything else: the per-group MSMs run on the same scalars (nothing in front of the MSM runs again) and the call ends
 *      exactly as with the option off -- results, error kinds, tiers, indices, messages, masks, traces, states.
 * Every rejection is therefore decided by the per-group MSMs; the joint check can only let through what those would, except
 * when the sums of two or more invalid groups cancel (about 2^126 group operations, the curve's discrete-logarithm
 * level).  A finding from status bits makes the joint sum meaningless and the fall-back runs; with "verify_check" = 1 the
 * rejection that is rechecked is the fall-back's; a zero weight from the device chain repeats the pass as always.
 * NOT COVERED: the sharded entry points and the phased form (bpp_verify_phase*), which run as they always did.
 * bpp_batch_trace: BPP_TRACE_JOINT_RESULT is the joint point of the batch's last pass that took the joint path (passes 2 and 3
 * of a recheck, a sharded or phased call, a call with the option off leave it standing); after an ACCEPTED joint pass the
 * per-group MSMs did not run and BPP_TRACE_MSM_RESULT returns BPP_ERR_INVALID_ARGUMENT saying so, until a pass runs them again.
 * Counters: passes that took the joint path, those it accepted, those that fell back, and the fall-backs after which every group
 * was Ok all the same (never expected outside the test knob).  bpp_verify_joint_stats adds the context's pipeline lanes,
 * bpp_batcher_verify_joint_stats sums a batcher's lanes. */
struct bpp_verify_joint_stats {
  uint64_t calls, accepted, fallbacks, fallback_all_ok;
};
int bpp_verify_joint_stats(bpp_ctx *ctx, struct bpp_verify_joint_stats *out);
int bpp_batcher_verify_joint_stats(bpp_batcher *b, struct bpp_verify_joint_stats *out);

/* Prove calls in flight from ONE thread and ONE context: the prover's form of bpp_verify_submit_packed / bpp_verify_collect.
 * bpp_prove_submit hands a whole prove call to one of `depth` lanes and returns a ticket; bpp_prove_collect blocks until that call
 * is done and returns EXACTLY what the blocking call over the same items returns -- bpp_prove_batch_mixed(ctx, params, items,
 * n_items, proofs_out, proof_stride, proof_lens, item_status, ...) for a ticket submitted with openings == 0 (every item brings
 * commitments32; commit_stride is ignored), bpp_prove_openings(..., commitments_out, commit_stride, proofs_out, proof_stride, ...) for
 * one submitted with openings != 0 (an item with commitments32 == NULL has them made by the engine): the proof and commitment
 * bytes, proof_lens, item_status, the zeroed slots of failed items, the return code and the message in errbuf.  A failed item
 * never stops the others.  The output buffers given to collect have the geometry declared at submit.
 * The caller's buffers are free when bpp_prove_submit returns: the items array and everything it points to (values, blinding
 * factors, commitments, promises, seed nonce, transcript state or label, rng bytes).  submit checks every item on the calling
 * thread and takes its own copy of the ones that pass; the copy's witness bytes are wiped as soon as the lane's call has returned,
 * on every path, and at bpp_ctx_destroy at the latest.
 * A lane is a context of its own (the prover's streams, arena and staging: count each against the hardware queues) with a worker
 * thread, made on the first submit with ctx's options AS THEY ARE THEN: bpp_ctx_set_option after the first submit does not reach
 * the lanes, and the self-check's tamper knobs are never copied.  With "prove_check" (and "prove_check_recovery") set before the
 * first submit every lane checks its calls as a context does; bpp_prove_check_stats, bpp_prove_check_recovery_stats and
 * bpp_prove_secret_bytes of ctx then include its lanes, and bpp_prove_collect copies the lane's note for that ticket into ctx, so that
 * bpp_prove_item_message / bpp_prove_openings_item_message on ctx right after the collect answer for that ticket.
 * Lanes are claimed round-robin in ticket order; submit blocks only while the lane whose turn it is still runs its previous job (a
 * lane is free once its job is done, collected or not).  Tickets may be collected in any order and from any thread; they are a
 * number space of their own, unknown to bpp_verify_collect.  Blocking prove and verify calls on ctx, and a bpp_prove_pool made from
 * it, keep working beside the pipeline.  bpp_ctx_destroy waits for the jobs in flight and drops results never collected.
 * bpp_prove_submit itself fails (no ticket, *ticket untouched) only for what needs no look at an item: ctx == NULL or an unknown
 * params handle -> BPP_ERR_BAD_HANDLE, no usable device -> BPP_ERR_NO_DEVICE, items == NULL, n_items == 0 or ticket == NULL ->
 * BPP_ERR_INVALID_ARGUMENT "null argument".  Everything else, per-item failures included, is reported by collect.
 * bpp_prove_collect with proofs_out == NULL or proof_lens == NULL (or commitments_out == NULL for an openings ticket) returns
 * BPP_ERR_INVALID_ARGUMENT and leaves the ticket collectable; an unknown ticket, one already collected or a ticket of the verify
 * pipeline -> BPP_ERR_BAD_HANDLE "unknown ticket", from bpp_prove_ticket_done as well.
 * Messages of bpp_prove_submit and bpp_prove_collect go to errbuf alone, as those of the verify pipeline do: they may run on any
 * thread beside a blocking call that holds the context, so they leave bpp_ctx_last_error to that call.
 * bpp_prove_pipeline_depth: lanes of the prove pipeline, 1..8, default 3; only before the first bpp_prove_submit of the context.
 * bpp_prove_ticket_done never blocks: *done = 1 once bpp_prove_collect would not wait. */
int bpp_prove_pipeline_depth(bpp_ctx *ctx, uint32_t depth);
int bpp_prove_submit(bpp_ctx *ctx, uint64_t params, const bpp_prove_item *items, size_t n_items, size_t proof_stride, int openings,
                     size_t commit_stride, uint64_t *ticket, char *errbuf, size_t errbuf_len);
int bpp_prove_collect(bpp_ctx *ctx, uint64_t ticket, uint8_t *commitments_out, uint8_t *proofs_out, size_t *proof_lens,
                      int *item_status, char *errbuf, size_t errbuf_len);
int bpp_prove_ticket_done(bpp_ctx *ctx, uint64_t ticket, int *done);

/* ---- parity / diagnostics: intermediates of the last verify on `batch`, for differential tests ---- */
#define BPP_TRACE_CHALLENGES 1     /* per proof (rmax+3) x 32: y, z, e_0.., e_final (canonical), rmax = bpp_batch_shape's max_rounds
                                      (largest round count in the batch, at most 11: proofs claiming more are refused) */
#define BPP_TRACE_RNG_OUT 2        /* n x 32 */
#define BPP_TRACE_WEIGHTS 3        /* n x 32 */
#define BPP_TRACE_STATIC_SCALARS 4 /* groups x (2*max_mn + t + 1) x 32: gi0,hi0,gi1,hi1,...,g_0..g_{t-1},h */
#define BPP_TRACE_DYNAMIC_SCALARS 5 /* total_dyn x 32, proof order: C_j.., A1, B, A, L.., R.. */
#define BPP_TRACE_MSM_RESULT 6     /* groups x 32 compressed */
#define BPP_TRACE_JOINT_RESULT 8   /* 32: the compressed point of the joint final check ("verify_joint"), of the last pass that took it; BPP_ERR_INVALID_ARGUMENT
                                      if no pass of this batch has */
#define BPP_TRACE_PLAN 7           /* four uint32: bit 0 generator columns summed in k_scalars_lanes, bit 1 taken from k_static_gemm;
                                      proofs per workgroup of k_scalars_lanes; K chunks of k_static_gemm; groups */
int bpp_batch_trace(bpp_ctx *ctx, uint64_t batch, int what, uint8_t *out, size_t out_len, size_t *written);
/* shape helpers for the above */
int bpp_batch_shape(bpp_ctx *ctx, uint64_t batch, uint32_t *n_items, uint32_t *max_rounds, uint32_t *max_mn,
                    uint32_t *total_dyn, uint32_t *groups);

/* ---- per-stage device timing of the last verify (hipEvents on the ctx stream) ---- */
typedef struct {
  float transcripts_ms, decompress_ms, chain_host_ms, scalars_ms, reduce_ms;
  float msm_digits_ms, msm_sort_ms, msm_accumulate_ms, msm_bucket_reduce_ms, msm_final_ms;
  float total_ms;
  uint32_t msm_terms, msm_window_bits, msm_windows, msm_groups;
  float masks_ms; /* k_masks (mask recovery, src/range_proof.rs:941-969); 0 for VerifyOnly */
  float chain_device_ms; /* the weight chains as kernels (option "chain" = 1: k_weight_chain + k_chain_finish); 0 with the chains on the host */
} bpp_profile;
/* on = 1: an event at every stage boundary (thirteen per verification);
 * on = 2: the two events around the roofline kernel only (msm_accumulate_ms; every other interval reads 0) */
int bpp_profile_enable(bpp_ctx *ctx, int on);
int bpp_profile_get(bpp_ctx *ctx, bpp_profile *out);

/* the batch prover's dominant kernel (k_fb_msm, fixed-base MSM) over the last bpp_prove_batch of this ctx: summed event
 * time of its launches, the terms it consumed (witness check, L/R of every round, A1/B), table geometry */
typedef struct {
  float fb_msm_ms, total_ms;
  uint64_t fb_terms;
  uint32_t fb_launches, fb_window_bits, fb_windows, sub_batches;
} bpp_prove_profile;
int bpp_prove_profile_get(bpp_ctx *ctx, bpp_prove_profile *out);

/* size of the process-wide host worker pool that runs the batch-weight chains and the upload packer
 * (BPP_HOST_THREADS, default min(usable cores, 32), usable = affinity mask capped by the cgroup CPU quota): the verifier's throughput depends on it */
int bpp_host_threads(void);
/* CPU time (ns, thread clocks, summed over the pool and the calling threads) this process has spent in the library's host jobs
 * so far: the batch weight chains (src/range_proof.rs:849-853,894 -- the one sequential part of a verification, kept on the host)
 * and the parsing of uploaded batches.  The difference over a run / (steps x step time) = host cores a rank keeps busy: with
 * several ranks on one node it tells a host-bound scaling curve from a GPU-bound one. */
uint64_t bpp_host_pool_cpu_ns(void);

/* diagnostics: the shader clock the device holds RIGHT NOW, sampled by one napping wavefront on this context's stream for
 * about `window_us` microseconds (s_memtime against the 100 MHz s_memrealtime) while other contexts' kernels run.  Under the
 * verifier's load the chip holds 2.0-2.2 GHz, not the 2.4 GHz of a light kernel: issue-rate peaks have to be priced at
 * the clock measured (bench.py reports it as shader_clock_ghz). */
int bpp_shader_clock(bpp_ctx *ctx, uint32_t window_us, double *ghz);

/* diagnostics (tests/test_gpu_round3.py): number of non-zero bytes in the device copies of the secrets a resident batch
 * holds -- the statements' seed nonces and the recovered masks (zeroized on drop by the reference: src/range_statement.rs:76-81,
 * src/extended_mask.rs:14).  batch == 0 looks at the buffers the context kept from the last destroyed batch, which the
 * next upload will adopt: must read 0. */
int bpp_batch_secret_bytes(bpp_ctx *ctx, uint64_t batch, uint64_t *nonzero);
/* the same for the prover (tests/test_gpu_round5.py): the context's prover arena on the device -- witness bytes, bit vectors, nonces,
 * blinding-factor accumulators, the transcript-RNG states keyed with the witness -- and its page-locked staging on the way IN
 * (the witness bytes; on the way out only proofs and status words travel), which bpp_prove_batch wipes on EVERY exit path (the reference
 * keeps all of it in Zeroizing<>: src/range_proof.rs:300-301,325,438-464,542-571).  *examined = bytes looked at (0 before the
 * first prove call), *nonzero = how many of them are not zero: must read 0 between calls.  The self-check's own buffers are
 * looked at as well ("prove_check_recovery"): its staging of blinding factors, page-locked and on the device, and the seed
 * nonces and recovered masks of its verification batch.  Not reachable from the host and
 * therefore not counted here: the LDS of the prover's kernels (generator states keyed with the witness, raw draws, digits of
 * witness-derived scalars) -- every such kernel clears its LDS as its last statement (kernels_prove.h: lds_wipe; ct.h). */
int bpp_prove_secret_bytes(bpp_ctx *ctx, uint64_t *examined, uint64_t *nonzero);

/* Transcript::new(label) -> 203-byte STROBE state (host helper for callers that keep merlin on their side) */
int bpp_transcript_new(const uint8_t *label, size_t label_len, uint8_t state203[203]);

/* Transcript::append_message / Transcript::challenge_bytes on a 203-byte state, IN PLACE (host only, no device, no context): what a
 * caller without a merlin of its own needs to bind context before a call and to go on with the transcript a *_states call handed
 * back.  A state with pos (byte 200) >= 166, the STROBE rate, is refused with BPP_ERR_INVALID_ARGUMENT, as the upload refuses it. */
int bpp_transcript_append_message(uint8_t state203[203], const uint8_t *label, size_t label_len, const uint8_t *msg, size_t msg_len);
int bpp_transcript_challenge_bytes(uint8_t state203[203], const uint8_t *label, size_t label_len, uint8_t *out, size_t out_len);

/* The reference's public TranscriptProtocol (src/protocols/transcript_protocol.rs) and merlin's transcript RNG on 203-byte states in
 * the caller's memory (host only, no device, no context): what the new kinds of bpp_transcripts_enqueue are held to.  pos >= 166 is
 * refused as above.  errbuf (or NULL) receives the reference's message text.
 *   _validate_and_append_point  32 zero bytes (the identity's encoding): BPP_ERR_VERIFICATION_FAILED, "Identity element cannot be added
 *                               to the transcript", the state untouched; otherwise append_message(label, point32).
 *   _challenge_scalar           challenge_bytes(label, 64) reduced wide mod l into out32 (canonical, little-endian).  Zero:
 *                               BPP_ERR_VERIFICATION_FAILED, "Transcript challenge cannot be zero" (the state has advanced, as in the
 *                               reference; out32 is 32 zero bytes).
 *   _rng_begin                  build_rng(): rng203_out := a copy of state203.  The "RNG state" of the calls below is that copy: the
 *                               builder until _rng_finalize, the TranscriptRng behind it.  It is keyed with the witness: wipe it.
 *   _rng_rekey                  rekey_with_witness_bytes(label, witness).
 *   _rng_finalize               finalize(&mut rng) with random32 the external RNG's one draw of 32 bytes; NULL: NullRng, 32 zero bytes.
 *   _rng_fill                   one fill_bytes(out_len).
 *   _rng_scalar                 Scalar::random: fill_bytes(64) reduced wide into out32.  Zero: BPP_ERR_VERIFICATION_FAILED, "Random
 *                               scalar is zero" -- this library's own words: the reference has no such error, its
 *                               ScalarProtocol::random_not_zero draws again; this call does not (the caller may). */
int bpp_transcript_validate_and_append_point(uint8_t state203[203], const uint8_t *label, size_t label_len, const uint8_t point32[32],
                                             char *errbuf, size_t errbuf_len);
int bpp_transcript_challenge_scalar(uint8_t state203[203], const uint8_t *label, size_t label_len, uint8_t out32[32], char *errbuf,
                                    size_t errbuf_len);
int bpp_transcript_rng_begin(const uint8_t state203[203], uint8_t rng203_out[203]);
int bpp_transcript_rng_rekey(uint8_t rng203[203], const uint8_t *label, size_t label_len, const uint8_t *witness, size_t witness_len);
int bpp_transcript_rng_finalize(uint8_t rng203[203], const uint8_t random32[32] /* or NULL: NullRng */);
int bpp_transcript_rng_fill(uint8_t rng203[203], uint8_t *out, size_t out_len);
int bpp_transcript_rng_scalar(uint8_t rng203[203], uint8_t out32[32], char *errbuf, size_t errbuf_len);

/* ---- Merlin on the stream: the three calls above, row-wise, on transcript rows in device memory ----
 * bpp_transcripts_enqueue runs a short program of Merlin operations on n rows of 203 bytes in device memory (any byte address, IN
 * PLACE), one wavefront per row on the context's stream: it MAKES the rows a *_transcripts / item_states_dev call takes (NEW, then
 * APPEND of a row of context each) and GOES ON with the rows a *_states call hands back (CHALLENGE), without a host round trip.
 * The call enqueues behind everything on the context's stream and returns.
 *
 * THE PROGRAM: n_ops (1 .. BPP_TOP_MAX_OPS) operations, applied to every live row in order.
 *   BPP_TOP_NEW        Transcript::new(label): the row := that state, whatever it held (it is not read).  Only as op 0, without data.
 *                      The state is public and the same for every row: the host computes it once (the routine behind
 *                      bpp_transcript_new) and it travels in the launch arguments.  Its label may have any length.
 *   BPP_TOP_APPEND     append_message(label, row i of data_dev).  data_dev is read: len bytes per row, or lens_dev[i] bytes (n words of
 *                      device memory) with len as the cap.  append_u64 is an APPEND of eight little-endian bytes, as in merlin.
 *   BPP_TOP_CHALLENGE  challenge_bytes(label, row i of data_dev).  data_dev is written: len bytes per row.
 *   Labels are HOST memory and are copied at call time (NULL with label_len 0); row i of an op's data lies at data_dev + i * stride.
 * THE CONTRACT, per row.  A row is LIVE where live_dev[i] != 0, or everywhere when live_dev is NULL.  A live row that is not void ends
 * up as the 203 bytes bpp_transcript_new / bpp_transcript_append_message / bpp_transcript_challenge_bytes leave when applied to a host
 * copy of the row in program order, and row i of every CHALLENGE holds the bytes the host call writes; its done_mask byte is 1.
 * VOID ROWS.  A live row is void -- decided by the row's first lane before any other byte of the row or of its data is read -- if
 *   the program does not begin with NEW and the row has pos >= 166 (byte 200) or cur_flags == 0 (byte 202), or
 *   some APPEND has lens_dev[i] > len.
 * A void row becomes 203 zero bytes, each of its CHALLENGE rows len zero bytes, its done_mask byte 0; it counts in n_void and
 * competes for first_void (the lowest index wins).
 * STRICTER THAN THE HOST HELPERS in one place: cur_flags == 0.  The host helpers look at pos alone.  No Merlin transcript has that
 * byte zero (Transcript::new ends behind an AD operation, and every operation sets it), but the 203 zero bytes that
 * bpp_verify_enqueue_states and bpp_prove_enqueue write for rejected, failed or dead items do: under this rule such a row stays zero
 * through this call, with a zero challenge, instead of becoming a plausible-looking transcript.
 * DEAD ROWS (live_dev[i] == 0): the state row is neither read nor written, nothing of its data rows or of lens_dev[i] is read, its
 * CHALLENGE rows are zeroed, its done_mask byte is 0.  ROW SLACK (stride > len) is neither read nor written.
 * record_dev (or NULL): {n_done, n_void, first_void (0xFFFFFFFF: none), flags = BPP_TOPS_WRITTEN}, initialised and reduced on the
 * stream.  done_mask_dev (or NULL): n bytes.
 * REFUSED before any launch (BPP_ERR_INVALID_ARGUMENT, the field named in bpp_ctx_last_error, the counters left alone): n == 0 (or
 * above 2^31 - 1); n_ops 0 or above BPP_TOP_MAX_OPS; an unknown kind; NEW anywhere but at op 0, or NEW with data; an APPEND / CHALLENGE
 * label above BPP_TOP_LABEL_MAX; len above BPP_TOP_LEN_MAX; stride < len; data_dev NULL with len > 0; lens_dev on anything but an
 * APPEND; states203_dev, a data_dev, lens_dev, live_dev, done_mask_dev or record_dev that bpp_device_pointer_check does not class
 * BPP_PTR_THIS_DEVICE; a written range (the states, a CHALLENGE's rows, done_mask_dev, record_dev) that overlaps any other range
 * of the call.
 * STEADY STATE: after a context's first call (the ticket events) the call allocates nothing, copies nothing to the host and waits
 * for nothing: bpp_transcripts_stats' host_waits stays 0.  TICKETS are those of bpp_enqueue_done / bpp_enqueue_wait.
 * The rows and everything appended here are the caller's public protocol data; the kernel wipes its LDS all the same.
 *
 * THE TRANSCRIPT PROTOCOL AND THE TRANSCRIPT RNG (the reference's public TranscriptProtocol, src/protocols/transcript_protocol.rs, and
 * merlin's TranscriptRngBuilder / TranscriptRng, call for call).  Eight more kinds; a program of NEW / APPEND / CHALLENGE alone runs
 * the kernel it always ran and behaves byte for byte as above.
 *   BPP_TOP_APPEND_POINT      validate_and_append_point(label, row i of data_dev): len must be 32, no lens_dev.  A row of 32 zero bytes
 *                             (the identity's encoding) makes the row VOID, decided up front like the other void rules; any other row
 *                             is an APPEND of its 32 bytes.  append_point and append_scalar are plain APPENDs of 32 bytes.
 *   BPP_TOP_CHALLENGE_SCALAR  challenge_scalar(label): challenge_bytes(label, 64) reduced wide mod l (Scalar::from_bytes_mod_order_wide),
 *                             the 32 canonical little-endian bytes into row i of data_dev; len must be 32.  The transcript advances
 *                             exactly as under CHALLENGE with len 64.  A ZERO result ("Transcript challenge cannot be zero") voids the
 *                             row in the middle of its program: it ends like every void row.
 *   The transcript RNG lives in the kernel's LDS for the length of the row's program and is never written to memory:
 *   BPP_TOP_RNG_BEGIN         build_rng(): the RNG := a clone of the row's transcript as it stands at this point of the program.  No
 *                             label, no data.  A second BEGIN drops the RNG before it.
 *   BPP_TOP_RNG_REKEY         rekey_with_witness_bytes(label, row i of data_dev): len bytes, or lens_dev[i] under the cap len
 *                             (lens_dev[i] > len: void, as for APPEND).
 *   BPP_TOP_RNG_FINALIZE      finalize(&mut rng): data_dev holds rows of 32 bytes, the one draw from the caller's own RNG (len must be
 *                             32); data_dev NULL with len 0 is the reference's NullRng, 32 zero bytes.
 *   BPP_TOP_RNG_FILL          one fill_bytes of len bytes into row i of data_dev.
 *   BPP_TOP_RNG_FILL32        len / 32 successive fill_bytes of 32 bytes each (len a multiple of 32): what a consumer that draws 32
 *                             bytes at a time sees, the prover's rng row under prove_with_rng(.., &mut TranscriptRng).  merlin absorbs
 *                             the length before every draw, so these are not the bytes of one FILL of len.
 *   BPP_TOP_RNG_SCALARS       len / 32 successive Scalar::random(&mut rng): fill_bytes(64) reduced wide, 32 canonical bytes each.  A
 *                             zero scalar VOIDS the row; the call does not redraw as ScalarProtocol::random_not_zero does -- a redraw
 *                             is a loop whose trip count depends on secret data, and the event has probability 2^-252.
 *   No RNG op changes the row's 203 bytes (build_rng works on a clone); APPEND / CHALLENGE between RNG ops act on the transcript and not
 *   on the RNG.  FINALIZE, FILL, FILL32 and SCALARS have no label in merlin and take none.
 * THE CONTRACT for these kinds is the same: a live row that is not void ends up as, and every output row (CHALLENGE, CHALLENGE_SCALAR,
 * RNG_FILL, RNG_FILL32, RNG_SCALARS) holds, what the host helpers below (bpp_transcript_validate_and_append_point, _challenge_scalar,
 * _rng_begin, _rng_rekey, _rng_finalize, _rng_fill, _rng_scalar; FILL32 and SCALARS are loops of _rng_fill(.., 32) and _rng_scalar)
 * leave on a host copy in program order.  Void and dead rows have EVERY output row of the program zeroed -- a row that goes void in the
 * middle of its program included, which also becomes 203 zero bytes, counts in n_void and competes for first_void -- and nothing of a
 * dead row's REKEY and FINALIZE rows is read.  Of a void row the APPEND_POINT rows alone may be read (that is how an identity is found),
 * and only where no other rule voids the row.
 * flags beside BPP_TOPS_WRITTEN: BPP_TOPS_IDENTITY -- some live row was voided by an APPEND_POINT; BPP_TOPS_ZERO_SCALAR -- by a zero
 * scalar.  A program of the three kinds above reads exactly BPP_TOPS_WRITTEN.
 * REFUSED as well: len other than 32 on APPEND_POINT, CHALLENGE_SCALAR or a FINALIZE with data; len not a multiple of 32 on FILL32 /
 * SCALARS; lens_dev on anything but APPEND / RNG_REKEY; RNG_BEGIN with a label or data; REKEY or FINALIZE without a BEGIN in front, or
 * behind that RNG's FINALIZE; FILL / FILL32 / SCALARS without a finalised RNG; a label on FINALIZE / FILL / FILL32 / SCALARS; the pointer
 * kinds and the overlap rule, with REKEY's, FINALIZE's and APPEND_POINT's rows read and every output row written.
 * SECRETS: REKEY's and FINALIZE's rows and everything FILL / FILL32 / SCALARS write.  No branch, address or launch geometry depends on
 * them but the void on a zero scalar, which is the reference's error; the kernel's LDS is wiped on every path. */
#define BPP_TOP_NEW 1
#define BPP_TOP_APPEND 2
#define BPP_TOP_CHALLENGE 3
#define BPP_TOP_APPEND_POINT 16
#define BPP_TOP_CHALLENGE_SCALAR 17
#define BPP_TOP_RNG_BEGIN 32
#define BPP_TOP_RNG_REKEY 33
#define BPP_TOP_RNG_FINALIZE 34
#define BPP_TOP_RNG_FILL 35
#define BPP_TOP_RNG_FILL32 36
#define BPP_TOP_RNG_SCALARS 37
#define BPP_TOP_MAX_OPS 8
#define BPP_TOP_LABEL_MAX 64
#define BPP_TOP_LEN_MAX 65536
typedef struct {
  uint32_t kind;
  const uint8_t *label; /* HOST memory, copied at call time; NULL with label_len 0 */
  uint32_t label_len;
  uint8_t *data_dev;    /* DEVICE rows: row i at data_dev + i * stride; may be NULL when len == 0 */
  size_t stride;
  uint32_t len;             /* bytes per row (APPEND: the cap when lens_dev is given) */
  const uint32_t *lens_dev; /* APPEND only, optional: row i's own length, n words of device memory */
} bpp_transcript_op;
typedef struct {
  uint32_t n_done, n_void;
  uint32_t first_void; /* 0xFFFFFFFF: none */
  uint32_t flags;      /* BPP_TOPS_WRITTEN | BPP_TOPS_IDENTITY | BPP_TOPS_ZERO_SCALAR */
} bpp_device_transcripts_record;
#define BPP_TOPS_WRITTEN 1u
#define BPP_TOPS_IDENTITY 2u    /* some live row was voided by an APPEND_POINT of the identity's encoding */
#define BPP_TOPS_ZERO_SCALAR 4u /* some live row was voided by a zero CHALLENGE_SCALAR or RNG_SCALARS result */
int bpp_transcripts_enqueue(bpp_ctx *ctx, uint8_t *states203_dev /* DEVICE n x 203, any byte address, IN PLACE */, size_t n,
                            const bpp_transcript_op *ops, size_t n_ops,
                            const uint8_t *live_dev /* DEVICE n bytes, or NULL: every row */,
                            uint8_t *done_mask_dev /* DEVICE n bytes, or NULL: 1 where the row was advanced */,
                            bpp_device_transcripts_record *record_dev /* DEVICE, or NULL */,
                            uint64_t *ticket /* or NULL; bpp_enqueue_done / bpp_enqueue_wait */);
struct bpp_transcripts_stats {
  uint64_t calls;       /* enqueues that passed the refusals */
  uint64_t first_calls; /* of them, the context's first (at most 1): it makes the ticket events where no enqueue has yet */
  uint64_t host_waits;  /* times a call waited for the device: 0 */
};
int bpp_transcripts_stats(bpp_ctx *ctx, struct bpp_transcripts_stats *out);

/* ---- Advanced transcripts: `&mut Transcript` on the device paths ----
 * The reference's prove_with_rng and verify_batch take `&mut Transcript` (src/range_proof.rs:222-237, :712-717, :757) and leave
 * it advanced by everything the proof appended and drew, so that the caller can go on with it.  The calls below are the named
 * existing calls plus states_out203, n_items x 203 packed bytes (st[200], pos, pos_begin, cur_flags: bpp_transcript_new's form),
 * which must not be NULL; everything else they do and return is what the call without the buffer does and returns.
 *   verifier: row i = proof i's transcript after to_verifier_rng has appended r1, s1 and every d1 (src/transcripts.rs:166-172) and
 *             before build_rng, which works on a clone.  It depends on the proof, its statement and the transcript that came in --
 *             not on the VerifyAction, on `chunk`, on the kernel forms or on whether the transcript came as a label or as a state.
 *   prover:   row i = item i's transcript after the challenge_scalar(b"e") of challenge_final_e (src/transcripts.rs:152-161).  The
 *             prover never appends r1, s1, d1: its final state and a verifier's for the same proof differ, as in the reference.
 *             Under "prove_check" = 1 the row belongs to the proof that is returned (a remade proof has the same bytes and state).
 *   failures: NARROWER than the reference, which leaves a transcript partly advanced when it returns an error.  A verify call that
 *             returns anything but BPP_OK writes NOTHING to states_out203.  A prove item whose status is not 0 -- BPP_ERR_SELF_CHECK
 *             included -- leaves its own row untouched while the other items' rows are written.
 * The rows leave the device through page-locked memory (written by PASS 1 itself / copied behind the prover's last kernel); they
 * are public data.  The calls without the buffer run the kernels' default instantiations and allocate nothing for this.
 * A batch uploaded by bpp_verify_batch_with_challenges' path has no device-side transcript: BPP_ERR_INVALID_ARGUMENT.
 * NOT covered (they hand nothing back, as before): bpp_verify_submit_packed / bpp_verify_collect, bpp_batcher, bpp_prove_pool,
 * bpp_prove_submit / bpp_prove_collect, the sharded forms, the grouped resident forms, and bpp_prove_batch (all-or-nothing). */
int bpp_verify_batch_states(bpp_ctx *ctx, uint64_t params, const bpp_verify_item *items, size_t n_items, int action, size_t chunk,
                            uint8_t *masks_out, uint8_t *mask_present, uint8_t *states_out203, char *errbuf, size_t errbuf_len);
int bpp_verify_batch_packed_states(bpp_ctx *ctx, uint64_t params, const bpp_packed_batch *in, int action, size_t chunk,
                                   uint8_t *masks_out, uint8_t *mask_present, uint8_t *states_out203, char *errbuf, size_t errbuf_len);
int bpp_verify_resident_states(bpp_ctx *ctx, uint64_t batch, int action, size_t chunk, uint8_t *masks_out, uint8_t *mask_present,
                               uint8_t *states_out203, char *errbuf, size_t errbuf_len);
int bpp_prove_batch_mixed_states(bpp_ctx *ctx, uint64_t params, const bpp_prove_item *items, size_t n_items, uint8_t *proofs_out,
                                 size_t proof_stride, size_t *proof_lens, int *item_status, uint8_t *states_out203, char *errbuf,
                                 size_t errbuf_len);
int bpp_prove_openings_states(bpp_ctx *ctx, uint64_t params, const bpp_prove_item *items, size_t n_items, uint8_t *commitments_out,
                              size_t commit_stride, uint8_t *proofs_out, size_t proof_stride, size_t *proof_lens, int *item_status,
                              uint8_t *states_out203, char *errbuf, size_t errbuf_len);

#ifdef __cplusplus
}
#endif
#endif /* BPP_H */
