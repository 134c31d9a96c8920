//! Raw declarations: one `extern "C"` item per symbol of include/bpp.h, same order, same argument meaning.
#![allow(non_camel_case_types)]
use core::ffi::{c_char, c_int, c_void};

#[repr(C)]
pub struct bpp_ctx {
    _p: [u8; 0],
}

pub const BPP_OK: c_int = 0;
pub const BPP_ERR_VERIFICATION_FAILED: c_int = 1;
pub const BPP_ERR_INVALID_ARGUMENT: c_int = 2;
pub const BPP_ERR_INVALID_LENGTH: c_int = 3;
pub const BPP_ERR_INVALID_BLAKE2B: c_int = 4;
pub const BPP_ERR_SIZE_OVERFLOW: c_int = 5;
pub const BPP_ERR_ENGINE: c_int = -1;
pub const BPP_ERR_NO_DEVICE: c_int = -2;
pub const BPP_ERR_BAD_HANDLE: c_int = -3;
pub const BPP_ERR_COMM: c_int = -4;
pub const BPP_ERR_SELF_CHECK: c_int = -5;
// where inside RangeProof::verify a check failed (src/range_proof.rs:756-1065): orders findings across shards
pub const BPP_TIER_NONE: c_int = 0;
pub const BPP_TIER_CONSTRUCTION: c_int = 1;
pub const BPP_TIER_DEGREE: c_int = 2;
pub const BPP_TIER_PROMISE: c_int = 3;
pub const BPP_TIER_STATEMENT_POINT: c_int = 4;
pub const BPP_TIER_PASS1: c_int = 5;
pub const BPP_TIER_PASS2: c_int = 6;
pub const BPP_TIER_MSM: c_int = 7;
pub const BPP_TIER_ENGINE: c_int = 255;
pub const BPP_SHARD_TRAILER_BYTES: usize = 128;
pub const BPP_REFERENCE_CHUNK: usize = 256;

/// bpp_verify_item: one (transcript, statement, proof) triple of `RangeProof::verify_batch` (src/range_proof.rs:712-717)
#[repr(C)]
pub struct bpp_verify_item {
    pub proof: *const u8,
    pub proof_len: usize,
    pub commitments32: *const u8,
    pub m: u32,
    pub min_values: *const u64,
    pub min_present: *const u8,
    pub seed_nonce32: *const u8,
    pub transcript_state: *const u8,
    pub transcript_label: *const u8,
    pub label_len: usize,
}

/// bpp_prove_item: one (transcript, statement, witness, rng) quadruple of `RangeProof::prove_with_rng` (:232-237)
#[repr(C)]
pub struct bpp_prove_item {
    pub values: *const u64,
    pub blindings32: *const u8,
    pub commitments32: *const u8,
    pub m: u32,
    pub min_values: *const u64,
    pub min_present: *const u8,
    pub seed_nonce32: *const u8,
    pub transcript_state: *const u8,
    pub transcript_label: *const u8,
    pub label_len: usize,
    pub rng_bytes: *const u8,
    pub rng_len: usize,
}

/// bpp_packed_batch: a homogeneous batch (`&[RangeStatement]`, `&[RangeProof]` of one shape) as contiguous arrays
#[repr(C)]
pub struct bpp_packed_batch {
    pub n_items: usize,
    pub proofs: *const u8,
    pub proof_len: usize,
    pub proof_stride: usize,
    pub commitments32: *const u8,
    pub m: u32,
    pub min_values: *const u64,
    pub min_present: *const u8,
    pub seed_nonces32: *const u8,
    pub seed_present: *const u8,
    pub transcript_state: *const u8,
    pub transcript_label: *const u8,
    pub label_len: usize,
}

/// bpp_mixed_batch: a batch of mixed aggregation factors as arrays of rows, the geometry of what `bpp_prove_batch_mixed` /
/// `bpp_prove_openings` write; `proof_lens` and `m` are host memory in every form
#[repr(C)]
pub struct bpp_mixed_batch {
    pub n_items: usize,
    pub proofs: *const u8,
    pub proof_stride: usize,
    pub proof_lens: *const usize,
    pub m: *const u32,
    pub m_stride: u32,
    pub commitments32: *const u8,
    pub min_values: *const u64,
    pub min_present: *const u8,
    pub seed_nonces32: *const u8,
    pub seed_present: *const u8,
    pub transcript_state: *const u8,
    pub transcript_label: *const u8,
    pub label_len: usize,
}

/// bpp_prove_arrays: the openings of a prove call as arrays of rows in DEVICE memory (`bpp_prove_openings_device`); `m` and the
/// transcript are host memory
#[repr(C)]
pub struct bpp_prove_arrays {
    pub n_items: usize,
    pub m: *const u32,
    pub m_stride: u32,
    pub values: *const u64,
    pub blindings32: *const u8,
    pub commitments32: *const u8,
    pub min_values: *const u64,
    pub min_present: *const u8,
    pub seed_nonces32: *const u8,
    pub seed_present: *const u8,
    pub rng_bytes: *const u8,
    pub rng_stride: usize,
    pub transcript_state: *const u8,
    pub transcript_label: *const u8,
    pub label_len: usize,
}

/// bpp_device_prove_status: one item's record of `bpp_prove_openings_device`, 8 bytes, as it lies in device memory
#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct bpp_device_prove_status {
    pub code: i32,
    pub msg: u32,
}

/// `struct bpp_prove_device_stats`: what the prove calls from device arrays of a context came to
#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct bpp_prove_device_stats {
    pub calls: u64,
    pub items: u64,
    pub device_findings: u64,
    pub host_findings: u64,
}

/// bpp_device_prove_summary: the one record of a `bpp_prove_enqueue`, 32 bytes, as it lies in device memory
#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct bpp_device_prove_summary {
    pub code: i32,
    pub msg: u32,
    pub index: u32,
    pub flags: u32,
    pub n_ok: u32,
    pub n_failed: u32,
    pub n_empty: u32,
    pub reserved: u32,
}
pub const BPP_PROVE_PLAN_ITEM_STATES: u32 = 1;
pub const BPP_PROVE_SUMMARY_WRITTEN: u32 = 1;
pub const BPP_PROVE_MSG_EMPTY: u32 = 17;

/// `struct bpp_prove_enqueue_stats`: what the stream-ordered prove calls of a context cost the host
#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct bpp_prove_enqueue_stats {
    pub calls: u64,
    pub first_calls: u64,
    pub host_waits: u64,
    pub allocations: u64,
}

/// bpp_transcript_op: one Merlin operation of a `bpp_transcripts_enqueue` (the label on the host, the rows in device memory)
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct bpp_transcript_op {
    pub kind: u32,
    pub label: *const u8,
    pub label_len: u32,
    pub data_dev: *mut u8,
    pub stride: usize,
    pub len: u32,
    pub lens_dev: *const u32,
}
pub const BPP_TOP_NEW: u32 = 1;
pub const BPP_TOP_APPEND: u32 = 2;
pub const BPP_TOP_CHALLENGE: u32 = 3;
pub const BPP_TOP_APPEND_POINT: u32 = 16;
pub const BPP_TOP_CHALLENGE_SCALAR: u32 = 17;
pub const BPP_TOP_RNG_BEGIN: u32 = 32;
pub const BPP_TOP_RNG_REKEY: u32 = 33;
pub const BPP_TOP_RNG_FINALIZE: u32 = 34;
pub const BPP_TOP_RNG_FILL: u32 = 35;
pub const BPP_TOP_RNG_FILL32: u32 = 36;
pub const BPP_TOP_RNG_SCALARS: u32 = 37;
pub const BPP_TOP_MAX_OPS: usize = 8;
pub const BPP_TOP_LABEL_MAX: u32 = 64;
pub const BPP_TOP_LEN_MAX: u32 = 65536;

/// bpp_device_transcripts_record: the one record of a `bpp_transcripts_enqueue`, 16 bytes, as it lies in device memory
#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct bpp_device_transcripts_record {
    pub n_done: u32,
    pub n_void: u32,
    pub first_void: u32,
    pub flags: u32,
}
pub const BPP_TOPS_WRITTEN: u32 = 1;
pub const BPP_TOPS_IDENTITY: u32 = 2;
pub const BPP_TOPS_ZERO_SCALAR: u32 = 4;

/// `struct bpp_transcripts_stats`: what the `bpp_transcripts_enqueue` calls of a context cost the host
#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct bpp_transcripts_stats {
    pub calls: u64,
    pub first_calls: u64,
    pub host_waits: u64,
}

/// bpp_rows_msm: n rows of K (scalar, point) terms in device memory for `bpp_rows_msm_enqueue`; `point_stride == 0`: one row of K shared bases
#[repr(C)]
#[derive(Clone, Copy, Debug)]
#[allow(non_snake_case)]
pub struct bpp_rows_msm {
    pub n: usize,
    pub K: u32,
    pub scalars_dev: *const u8,
    pub scalar_stride: usize,
    pub points_dev: *const u8,
    pub point_stride: usize,
}
pub const BPP_ROWS_K_MAX: u32 = 16;

/// bpp_scalar_rows: one operand of `bpp_rows_scalar_enqueue`; `stride == 0`: one 32-byte scalar for every row
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct bpp_scalar_rows {
    pub dev: *const u8,
    pub stride: usize,
}

/// bpp_device_rows_record: the one record of a `bpp_rows_*_enqueue`, 16 bytes, as it lies in device memory
#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct bpp_device_rows_record {
    pub n_done: u32,
    pub n_void: u32,
    pub first_void: u32,
    pub flags: u32,
}
pub const BPP_ROWS_WRITTEN: u32 = 1;
pub const BPP_ROWS_SCALAR: u32 = 2;
pub const BPP_ROWS_POINT: u32 = 4;

/// `struct bpp_rows_stats`: what the `bpp_rows_*_enqueue` calls of a context cost the host
#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct bpp_rows_stats {
    pub calls: u64,
    pub first_calls: u64,
    pub host_waits: u64,
}

#[repr(C)]
pub struct bpp_comm {
    _p: [u8; 0],
}
#[repr(C)]
pub struct bpp_batcher {
    _p: [u8; 0],
}
#[repr(C)]
pub struct bpp_prove_pool {
    _p: [u8; 0],
}

/// outcome of one batch of a sharded wave (bpp_verify_sharded_wave)
#[repr(C)]
#[derive(Clone, Copy)]
pub struct bpp_shard_result {
    pub code: c_int,
    pub tier: c_int,
    pub rank: c_int,
    pub index: u32,
    pub msg: [c_char; 160],
}

#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct bpp_shard_timing {
    pub enqueue1_ms: f32,
    pub wait1_ms: f32,
    pub gather1_ms: f32,
    pub chains_ms: f32,
    pub enqueue2_ms: f32,
    pub wait2_ms: f32,
    pub gather2_ms: f32,
    pub batches: u32,
}

#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct bpp_profile {
    pub transcripts_ms: f32,
    pub decompress_ms: f32,
    pub chain_host_ms: f32,
    pub scalars_ms: f32,
    pub reduce_ms: f32,
    pub msm_digits_ms: f32,
    pub msm_sort_ms: f32,
    pub msm_accumulate_ms: f32,
    pub msm_bucket_reduce_ms: f32,
    pub msm_final_ms: f32,
    pub total_ms: f32,
    pub msm_terms: u32,
    pub msm_window_bits: u32,
    pub msm_windows: u32,
    pub msm_groups: u32,
    pub masks_ms: f32,
    pub chain_device_ms: f32,
}

/// bpp_runtime_info: what the library sees of its runtime preconditions ("Runtime preconditions")
#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct bpp_runtime_info {
    pub device: c_int,
    pub contexts: u32,
    pub contexts_peak: u32,
    pub hw_queues: u32,
    pub host_threads: u32,
    pub small_call_limit: u32,
    pub small_calls_in_flight: u32,
    pub small_calls: u64,
    pub small_calls_queued: u64,
    pub oversubscribed: u32,
}

#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct bpp_prove_profile {
    pub fb_msm_ms: f32,
    pub total_ms: f32,
    pub fb_terms: u64,
    pub fb_launches: u32,
    pub fb_window_bits: u32,
    pub fb_windows: u32,
    pub sub_batches: u32,
}

/// `struct bpp_prove_check_stats`: what the prover's self-check ("prove_check" = 1) of a context (or a prove pool's lanes) has done
#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct bpp_prove_check_stats {
    pub calls: u64,
    pub proofs: u64,
    pub batch_failures: u64,
    pub remade: u64,
    pub failed: u64,
}

/// `struct bpp_verify_check_stats`: what the rechecks of rejections ("verify_check" = 1) of a context (or a batcher's lanes) have done
#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct bpp_verify_check_stats {
    pub calls: u64,
    pub rechecked_groups: u64,
    pub confirmed: u64,
    pub overturned: u64,
    pub tie_breaks: u64,
    pub undecided: u64,
}

/// `struct bpp_verify_joint_stats`: what the joint final checks ("verify_joint" = 1) of a context (or a batcher's lanes) have done
#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct bpp_verify_joint_stats {
    pub calls: u64,
    pub accepted: u64,
    pub fallbacks: u64,
    pub fallback_all_ok: u64,
}

/// `struct bpp_ingest_stats`: what the uploads from device memory (`bpp_batch_upload_packed_device`) of a context came to
#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct bpp_ingest_stats {
    pub device_calls: u64,
    pub host_fallback_calls: u64,
    pub fallback_bytes: u64,
}

/// `bpp_device_verdict`: one group's record of `bpp_verify_enqueue`, 16 bytes, as it lies in device memory
#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct bpp_device_verdict {
    pub code: i32,
    pub tier: u32,
    pub index: u32,
    pub flags: u32,
}
pub const BPP_VERDICT_WRITTEN: u32 = 1;
pub const BPP_VERDICT_REDRAW: u32 = 2;
pub const BPP_VERDICT_REFILL: u32 = 4;
pub const BPP_VERDICT_EMPTY: u32 = 8;

/// `bpp_device_refill`: the record of `bpp_batch_refill_enqueue`, 16 bytes, as it lies in device memory
#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct bpp_device_refill {
    pub code: i32,
    pub msg: u32,
    pub index: u32,
    pub flags: u32,
}
pub const BPP_REFILL_WRITTEN: u32 = 1;
pub const BPP_REFILL_FINDING: u32 = 2;
pub const BPP_REFILL_FALLBACK: u32 = 4;
pub const BPP_REFILL_COUNT: u32 = 8;

/// `struct bpp_refill_stats`: what the refills (`bpp_batch_refill_enqueue`) of a context came to
#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct bpp_refill_stats {
    pub calls: u64,
    pub first_calls: u64,
    pub host_waits: u64,
}

/// `struct bpp_enqueue_stats`: what the enqueued verifications (`bpp_verify_enqueue`) of a context came to
#[repr(C)]
#[derive(Default, Clone, Copy, Debug)]
pub struct bpp_enqueue_stats {
    pub calls: u64,
    pub groups: u64,
    pub host_waits: u64,
    pub layouts_in_call: u64,
}

/// `int (*bpp_all_gather_fn)(void *user, const void *send, void *recv, size_t bytes_per_rank)` (include/bpp.h)
pub type bpp_all_gather_fn = Option<unsafe extern "C" fn(user: *mut c_void, send: *const c_void, recv: *mut c_void, bytes_per_rank: usize) -> c_int>;

extern "C" {
    pub fn bpp_ctx_create(out: *mut *mut bpp_ctx, device_id: c_int) -> c_int;
    pub fn bpp_ctx_create_on_stream(out: *mut *mut bpp_ctx, device_id: c_int, hip_stream: *mut c_void) -> c_int;
    pub fn bpp_ctx_destroy(ctx: *mut bpp_ctx);
    pub fn bpp_ctx_last_error(ctx: *mut bpp_ctx) -> *const c_char;
    pub fn bpp_ctx_set_option(ctx: *mut bpp_ctx, name: *const c_char, value: c_int) -> c_int;
    // runtime preconditions, the admission gate for small calls
    pub fn bpp_runtime_info_get(ctx: *mut bpp_ctx, out: *mut bpp_runtime_info) -> c_int;
    pub fn bpp_small_call_limit(ctx: *mut bpp_ctx, limit: c_int) -> c_int;
    // B1: VartimePrecomputedMultiscalarMul / VartimeMultiscalarMul / MultiscalarMul (src/traits.rs:40-43, src/ristretto.rs:28-64)
    pub fn bpp_precomp_create(ctx: *mut bpp_ctx, points32: *const u8, count: usize, handle: *mut u64) -> c_int;
    pub fn bpp_precomp_destroy(ctx: *mut bpp_ctx, handle: u64) -> c_int;
    pub fn bpp_precomp_retain(ctx: *mut bpp_ctx, handle: u64) -> c_int;
    pub fn bpp_msm_mixed(ctx: *mut bpp_ctx, handle: u64, static_scalars32: *const u8, n_static: usize, dyn_scalars32: *const u8,
                         dyn_points32: *const u8, n_dyn: usize, out_point32: *mut u8) -> c_int;
    pub fn bpp_msm_vartime(ctx: *mut bpp_ctx, scalars32: *const u8, points32: *const u8, n: usize, out_point32: *mut u8) -> c_int;
    pub fn bpp_msm_vartime_batched(ctx: *mut bpp_ctx, scalars32: *const u8, points32: *const u8, group_off: *const u32,
                                   n_groups: usize, out_points32: *mut u8) -> c_int;
    pub fn bpp_msm_last_plan(ctx: *mut bpp_ctx, out: *mut u32) -> c_int;
    pub fn bpp_msm_ct(ctx: *mut bpp_ctx, scalars32: *const u8, points32: *const u8, n: usize, out_point32: *mut u8) -> c_int;
    pub fn bpp_msm_ct_batched(ctx: *mut bpp_ctx, scalars32: *const u8, points32: *const u8, group_off: *const u32,
                              n_groups: usize, out_points32: *mut u8) -> c_int;
    pub fn bpp_msm_ct_secret_bytes(ctx: *mut bpp_ctx, examined: *mut u64, nonzero: *mut u64) -> c_int;
    // B2: RangeParameters::init (src/range_parameters.rs:32-58), PedersenGens::commit (src/generators/pedersen_gens.rs:112-122)
    pub fn bpp_params_create(ctx: *mut bpp_ctx, bit_length: u32, max_aggregation: u32, extension_degree: u32, h_base32: *const u8,
                             g_bases32: *const u8, params: *mut u64) -> c_int;
    pub fn bpp_params_destroy(ctx: *mut bpp_ctx, params: u64) -> c_int;
    pub fn bpp_params_retain(ctx: *mut bpp_ctx, params: u64) -> c_int;
    pub fn bpp_params_export(ctx: *mut bpp_ctx, params: u64, gi_out32: *mut u8, hi_out32: *mut u8, h_out32: *mut u8, g_out32: *mut u8) -> c_int;
    pub fn bpp_pedersen_commit(ctx: *mut bpp_ctx, params: u64, values: *const u64, blindings32: *const u8, n_blind: u32, count: usize,
                               commitments32: *mut u8) -> c_int;
    // B2: RangeProof::verify_batch / verify (src/range_proof.rs:712-1065)
    pub fn bpp_verify_batch(ctx: *mut bpp_ctx, params: u64, items: *const bpp_verify_item, n_items: usize, action: c_int, chunk: usize,
                            masks_out: *mut u8, mask_present: *mut u8, errbuf: *mut c_char, errbuf_len: usize) -> c_int;
    pub fn bpp_verify_batch_with_challenges(ctx: *mut bpp_ctx, params: u64, items: *const bpp_verify_item, n_items: usize,
                                            challenges32: *const *const u8, rng_out32: *const u8, action: c_int, chunk: usize,
                                            masks_out: *mut u8, mask_present: *mut u8, errbuf: *mut c_char, errbuf_len: usize) -> c_int;
    pub fn bpp_batch_upload(ctx: *mut bpp_ctx, params: u64, items: *const bpp_verify_item, n_items: usize, batch: *mut u64,
                            errbuf: *mut c_char, errbuf_len: usize) -> c_int;
    pub fn bpp_batch_destroy(ctx: *mut bpp_ctx, batch: u64) -> c_int;
    pub fn bpp_batch_prepare(ctx: *mut bpp_ctx, batch: u64, chunk: usize) -> c_int;
    pub fn bpp_verify_resident(ctx: *mut bpp_ctx, batch: u64, action: c_int, chunk: usize, masks_out: *mut u8, mask_present: *mut u8,
                               errbuf: *mut c_char, errbuf_len: usize) -> c_int;
    // packed form + pipelined host-buffers-in form (upload k+1 overlaps verify k inside one context)
    pub fn bpp_batch_upload_packed(ctx: *mut bpp_ctx, params: u64, input: *const bpp_packed_batch, batch: *mut u64, errbuf: *mut c_char,
                                   errbuf_len: usize) -> c_int;
    pub fn bpp_verify_batch_packed(ctx: *mut bpp_ctx, params: u64, input: *const bpp_packed_batch, action: c_int, chunk: usize,
                                   masks_out: *mut u8, mask_present: *mut u8, errbuf: *mut c_char, errbuf_len: usize) -> c_int;
    // the packed form from arrays in DEVICE memory (six array fields of `input` are device addresses; include/bpp.h)
    pub fn bpp_batch_upload_packed_device(ctx: *mut bpp_ctx, params: u64, input: *const bpp_packed_batch, batch: *mut u64,
                                          errbuf: *mut c_char, errbuf_len: usize) -> c_int;
    pub fn bpp_verify_batch_packed_device(ctx: *mut bpp_ctx, params: u64, input: *const bpp_packed_batch, action: c_int, chunk: usize,
                                          masks_out: *mut u8, mask_present: *mut u8, errbuf: *mut c_char, errbuf_len: usize) -> c_int;
    // batches of mixed aggregation factors from arrays of rows, in host memory or (six array fields of `input`) in device memory
    pub fn bpp_batch_upload_mixed(ctx: *mut bpp_ctx, params: u64, input: *const bpp_mixed_batch, batch: *mut u64, errbuf: *mut c_char,
                                  errbuf_len: usize) -> c_int;
    pub fn bpp_verify_batch_mixed(ctx: *mut bpp_ctx, params: u64, input: *const bpp_mixed_batch, action: c_int, chunk: usize,
                                  masks_out: *mut u8, mask_present: *mut u8, errbuf: *mut c_char, errbuf_len: usize) -> c_int;
    pub fn bpp_batch_upload_mixed_device(ctx: *mut bpp_ctx, params: u64, input: *const bpp_mixed_batch, batch: *mut u64,
                                         errbuf: *mut c_char, errbuf_len: usize) -> c_int;
    pub fn bpp_verify_batch_mixed_device(ctx: *mut bpp_ctx, params: u64, input: *const bpp_mixed_batch, action: c_int, chunk: usize,
                                         masks_out: *mut u8, mask_present: *mut u8, errbuf: *mut c_char, errbuf_len: usize) -> c_int;
    pub fn bpp_device_pointer_check(ctx: *mut bpp_ctx, p: *const c_void, kind: *mut c_int) -> c_int;
    pub fn bpp_ingest_stats(ctx: *mut bpp_ctx, out: *mut bpp_ingest_stats) -> c_int;
    pub fn bpp_ctx_pipeline_depth(ctx: *mut bpp_ctx, depth: u32) -> c_int;
    pub fn bpp_verify_submit_packed(ctx: *mut bpp_ctx, params: u64, input: *const bpp_packed_batch, action: c_int, chunk: usize,
                                    ticket: *mut u64, errbuf: *mut c_char, errbuf_len: usize) -> c_int;
    pub fn bpp_verify_collect(ctx: *mut bpp_ctx, ticket: u64, masks_out: *mut u8, mask_present: *mut u8, errbuf: *mut c_char,
                              errbuf_len: usize) -> c_int;
    // ONE reference batch sharded over the GPUs of a node: RCCL all_gathers on device buffers inside the library
    pub fn bpp_comm_unique_id(id128: *mut u8) -> c_int;
    pub fn bpp_comm_create(ctx: *mut bpp_ctx, id128: *const u8, rank: c_int, world: c_int, out: *mut *mut bpp_comm) -> c_int;
    pub fn bpp_comm_adopt(ctx: *mut bpp_ctx, nccl_comm: *mut c_void, rank: c_int, world: c_int, out: *mut *mut bpp_comm) -> c_int;
    /// The caller's own transport (MPI / TCP / gloo): `all_gather` sees HOST memory, blocks, returns 0 or an error (include/bpp.h).
    pub fn bpp_comm_create_callbacks(ctx: *mut bpp_ctx, rank: c_int, world: c_int, all_gather: bpp_all_gather_fn, user: *mut c_void,
                                     out: *mut *mut bpp_comm) -> c_int;
    pub fn bpp_comm_create_local(ctx: *mut bpp_ctx, group_id: u64, rank: c_int, world: c_int, out: *mut *mut bpp_comm) -> c_int;
    pub fn bpp_comm_destroy(comm: *mut bpp_comm);
    pub fn bpp_comm_last_error(comm: *mut bpp_comm) -> *const c_char;
    pub fn bpp_comm_set_timeout(comm: *mut bpp_comm, timeout_ms: u32) -> c_int;
    pub fn bpp_comm_last_timing(comm: *mut bpp_comm, out: *mut bpp_shard_timing) -> c_int;
    pub fn bpp_verify_sharded(comm: *mut bpp_comm, ctx: *mut bpp_ctx, batch: u64, counts: *const u32, tier_out: *mut c_int,
                              rank_out: *mut c_int, errbuf: *mut c_char, errbuf_len: usize) -> c_int;
    pub fn bpp_verify_sharded_wave(comm: *mut bpp_comm, ctxs: *const *mut bpp_ctx, batches: *const u64, k: usize, counts: *const u32,
                                   results: *mut bpp_shard_result) -> c_int;
    pub fn bpp_verify_sharded_groups(comm: *mut bpp_comm, ctx: *mut bpp_ctx, batch: u64, n_groups: usize, counts: *const u32,
                                     results: *mut bpp_shard_result) -> c_int;
    pub fn bpp_verify_sharded_groups_wave(comm: *mut bpp_comm, ctxs: *const *mut bpp_ctx, batches: *const u64, k: usize, n_groups: usize,
                                          counts: *const u32, results: *mut bpp_shard_result) -> c_int;
    // reference batches of different sizes as the groups of one call; the pool of many callers' small calls
    pub fn bpp_verify_resident_groups(ctx: *mut bpp_ctx, batch: u64, group_first: *const u32, n_groups: usize, results: *mut bpp_shard_result) -> c_int;
    pub fn bpp_batcher_create(ctx: *mut bpp_ctx, params: u64, shape: *const bpp_packed_batch, lanes: u32, max_wait_us: u32, max_calls: u32,
                              out: *mut *mut bpp_batcher) -> c_int;
    pub fn bpp_batcher_verify(b: *mut bpp_batcher, input: *const bpp_packed_batch, errbuf: *mut c_char, errbuf_len: usize) -> c_int;
    pub fn bpp_verify_resident_groups_actions(ctx: *mut bpp_ctx, batch: u64, group_first: *const u32, n_groups: usize, actions: *const c_int,
                                              results: *mut bpp_shard_result, masks_out: *mut u8, mask_present: *mut u8) -> c_int;
    // stream-ordered calls that leave their verdicts (and masks) in device memory the caller names
    pub fn bpp_verify_enqueue(ctx: *mut bpp_ctx, batch: u64, group_first: *const u32, n_groups: usize, chunk: usize, actions: *const c_int,
                              action_all: c_int, verdicts_dev: *mut bpp_device_verdict, masks_dev: *mut u8, mask_present_dev: *mut u8,
                              ticket: *mut u64) -> c_int;
    pub fn bpp_enqueue_done(ctx: *mut bpp_ctx, ticket: u64, done: *mut c_int) -> c_int;
    pub fn bpp_enqueue_wait(ctx: *mut bpp_ctx, ticket: u64) -> c_int;
    pub fn bpp_verdict_result(host_copy: *const bpp_device_verdict, out: *mut bpp_shard_result) -> c_int;
    pub fn bpp_enqueue_stats(ctx: *mut bpp_ctx, out: *mut bpp_enqueue_stats) -> c_int;
    // new contents of the same shape for a resident batch, from device arrays, on the stream (tickets: those of bpp_verify_enqueue)
    pub fn bpp_batch_refill_enqueue(ctx: *mut bpp_ctx, batch: u64, in_dev: *const bpp_packed_batch, record_dev: *mut bpp_device_refill,
                                    ticket: *mut u64) -> c_int;
    pub fn bpp_refill_result(host_copy: *const bpp_device_refill, out: *mut bpp_shard_result) -> c_int;
    pub fn bpp_refill_stats(ctx: *mut bpp_ctx, out: *mut bpp_refill_stats) -> c_int;
    // ... with a live count in one word of device memory, read on the stream (null: every item); the weights of the last enqueue
    pub fn bpp_batch_refill_enqueue_count(ctx: *mut bpp_ctx, batch: u64, in_dev: *const bpp_packed_batch, count_dev: *const u32,
                                          record_dev: *mut bpp_device_refill, ticket: *mut u64) -> c_int;
    // ... under a per-item live mask, N bytes in device memory read on the stream (null: every item)
    pub fn bpp_batch_refill_enqueue_live(ctx: *mut bpp_ctx, batch: u64, in_dev: *const bpp_packed_batch, live_dev: *const u8,
                                         record_dev: *mut bpp_device_refill, ticket: *mut u64) -> c_int;
    // ... of a batch of mixed aggregation factors: in_dev's proof_lens / m repeat the batch's vectors or are both null; at most one
    // of count_dev and live_dev
    pub fn bpp_batch_refill_enqueue_mixed(ctx: *mut bpp_ctx, batch: u64, in_dev: *const bpp_mixed_batch, count_dev: *const u32,
                                          live_dev: *const u8, record_dev: *mut bpp_device_refill, ticket: *mut u64) -> c_int;
    // per-item transcripts on the device paths: item_states203 = n_items rows of 203 bytes in device memory, in at upload and
    // refill; the advanced transcripts out on the stream (states_out203_dev, n x 203)
    pub fn bpp_batch_upload_packed_device_transcripts(ctx: *mut bpp_ctx, params: u64, input: *const bpp_packed_batch, item_states203: *const u8,
                                                      batch: *mut u64, errbuf: *mut c_char, errbuf_len: usize) -> c_int;
    pub fn bpp_batch_upload_mixed_device_transcripts(ctx: *mut bpp_ctx, params: u64, input: *const bpp_mixed_batch, item_states203: *const u8,
                                                     batch: *mut u64, errbuf: *mut c_char, errbuf_len: usize) -> c_int;
    pub fn bpp_batch_refill_enqueue_transcripts(ctx: *mut bpp_ctx, batch: u64, in_dev: *const bpp_packed_batch, item_states203_dev: *const u8,
                                                count_dev: *const u32, live_dev: *const u8, record_dev: *mut bpp_device_refill,
                                                ticket: *mut u64) -> c_int;
    pub fn bpp_batch_refill_enqueue_mixed_transcripts(ctx: *mut bpp_ctx, batch: u64, in_dev: *const bpp_mixed_batch,
                                                      item_states203_dev: *const u8, count_dev: *const u32, live_dev: *const u8,
                                                      record_dev: *mut bpp_device_refill, ticket: *mut u64) -> c_int;
    pub fn bpp_verify_enqueue_states(ctx: *mut bpp_ctx, batch: u64, group_first: *const u32, n_groups: usize, chunk: usize,
                                     actions: *const c_int, action_all: c_int, verdicts_dev: *mut bpp_device_verdict, masks_dev: *mut u8,
                                     mask_present_dev: *mut u8, states_out203_dev: *mut u8, ticket: *mut u64) -> c_int;
    pub fn bpp_enqueue_weights(ctx: *mut bpp_ctx, batch: u64, weights_dev: *mut u8, ticket: *mut u64) -> c_int;
    pub fn bpp_batcher_verify_action(b: *mut bpp_batcher, input: *const bpp_packed_batch, action: c_int, masks_out: *mut u8,
                                     mask_present: *mut u8, errbuf: *mut c_char, errbuf_len: usize) -> c_int;
    pub fn bpp_batcher_set_limits(b: *mut bpp_batcher, max_calls: u32, max_proofs: u32) -> c_int;
    pub fn bpp_batcher_largest_pool(b: *mut bpp_batcher, calls: *mut u32, proofs: *mut u32) -> c_int;
    pub fn bpp_batcher_stats(b: *mut bpp_batcher, pooled_calls: *mut u64, engine_calls: *mut u64, solo_calls: *mut u64) -> c_int;
    pub fn bpp_batcher_destroy(b: *mut bpp_batcher);
    pub fn bpp_shard_local_trailer(defer: *const u8, status: *const u32, rounds_bad: *const u8, n: u32, first_index: u32,
                                   trailer_out: *mut u8) -> c_int;
    pub fn bpp_shard_trailer(tier: c_int, code: c_int, index: u32, msg: *const c_char, trailer_out: *mut u8) -> c_int;
    pub fn bpp_shard_resolve(trailers: *const u8, stride: usize, world: c_int, tier_out: *mut c_int, rank_out: *mut c_int,
                             index_out: *mut u32, errbuf: *mut c_char, errbuf_len: usize) -> c_int;
    // phased form of the same (callers that bring their own transport)
    pub fn bpp_verify_phase1(ctx: *mut bpp_ctx, batch: u64, rng_out32: *mut u8, errbuf: *mut c_char, errbuf_len: usize) -> c_int;
    pub fn bpp_weights_from_chain(rng32_all: *const u8, n_total: usize, weights32_out: *mut u8) -> c_int;
    pub fn bpp_weights_from_chains(rng32_all: *const u8, n_groups: usize, n_per_group: usize, weights32_out: *mut u8) -> c_int;
    pub fn bpp_verify_phase2(ctx: *mut bpp_ctx, batch: u64, weights32: *const u8, accumulator128: *mut u8, errbuf: *mut c_char,
                             errbuf_len: usize) -> c_int;
    pub fn bpp_accumulators_sum_is_identity(ctx: *mut bpp_ctx, accumulators128: *const u8, n: usize, is_identity: *mut c_int) -> c_int;
    // B2: RangeProof::prove_with_rng (src/range_proof.rs:232-608)
    pub fn bpp_prove_batch(ctx: *mut bpp_ctx, params: u64, items: *const bpp_prove_item, n_items: usize, proofs_out: *mut u8,
                           proof_stride: usize, proof_len: *mut usize, errbuf: *mut c_char, errbuf_len: usize) -> c_int;
    pub fn bpp_prove_batch_mixed(ctx: *mut bpp_ctx, params: u64, items: *const bpp_prove_item, n_items: usize, proofs_out: *mut u8,
                                 proof_stride: usize, proof_lens: *mut usize, item_status: *mut c_int, errbuf: *mut c_char,
                                 errbuf_len: usize) -> c_int;
    pub fn bpp_prove_item_message(ctx: *mut bpp_ctx, params: u64, item: *const bpp_prove_item, proof_stride: usize, status: c_int,
                                  errbuf: *mut c_char, errbuf_len: usize) -> c_int;
    pub fn bpp_prove_openings(ctx: *mut bpp_ctx, params: u64, items: *const bpp_prove_item, n_items: usize, commitments_out: *mut u8,
                              commit_stride: usize, proofs_out: *mut u8, proof_stride: usize, proof_lens: *mut usize,
                              item_status: *mut c_int, errbuf: *mut c_char, errbuf_len: usize) -> c_int;
    pub fn bpp_prove_openings_item_message(ctx: *mut bpp_ctx, params: u64, item: *const bpp_prove_item, first_commitment32: *const u8,
                                           commit_stride: usize, proof_stride: usize, status: c_int, errbuf: *mut c_char,
                                           errbuf_len: usize) -> c_int;
    pub fn bpp_prove_openings_device(ctx: *mut bpp_ctx, params: u64, in_dev: *const bpp_prove_arrays, commitments_out_dev: *mut u8,
                                     commit_stride: usize, proofs_out_dev: *mut u8, proof_stride: usize, proof_lens: *mut usize,
                                     status_dev: *mut bpp_device_prove_status, item_status: *mut c_int, errbuf: *mut c_char,
                                     errbuf_len: usize) -> c_int;
    pub fn bpp_prove_openings_device_transcripts(ctx: *mut bpp_ctx, params: u64, in_dev: *const bpp_prove_arrays,
                                                 item_states_dev: *const u8, commitments_out_dev: *mut u8, commit_stride: usize,
                                                 proofs_out_dev: *mut u8, proof_stride: usize, proof_lens: *mut usize,
                                                 states_out_dev: *mut u8, status_dev: *mut bpp_device_prove_status,
                                                 item_status: *mut c_int, errbuf: *mut c_char, errbuf_len: usize) -> c_int;
    pub fn bpp_prove_status_result(host_copy: *const bpp_device_prove_status, out: *mut bpp_shard_result) -> c_int;
    pub fn bpp_prove_device_stats(ctx: *mut bpp_ctx, out: *mut bpp_prove_device_stats) -> c_int;
    pub fn bpp_prove_plan_create(ctx: *mut bpp_ctx, params: u64, shape: *const bpp_prove_arrays, commit_stride: usize,
                                 proof_stride: usize, flags: u32, plan: *mut u64, errbuf: *mut c_char, errbuf_len: usize) -> c_int;
    pub fn bpp_prove_plan_shape(ctx: *mut bpp_ctx, plan: u64, proof_lens: *mut usize, host_status: *mut c_int) -> c_int;
    pub fn bpp_prove_plan_destroy(ctx: *mut bpp_ctx, plan: u64) -> c_int;
    pub fn bpp_prove_enqueue(ctx: *mut bpp_ctx, plan: u64, in_dev: *const bpp_prove_arrays, item_states_dev: *const u8,
                             live_dev: *const u8, commitments_out_dev: *mut u8, proofs_out_dev: *mut u8, states_out_dev: *mut u8,
                             status_dev: *mut bpp_device_prove_status, ok_mask_dev: *mut u8,
                             summary_dev: *mut bpp_device_prove_summary, ticket: *mut u64) -> c_int;
    pub fn bpp_prove_summary_result(host_copy: *const bpp_device_prove_summary, out: *mut bpp_shard_result) -> c_int;
    pub fn bpp_prove_enqueue_stats(ctx: *mut bpp_ctx, out: *mut bpp_prove_enqueue_stats) -> c_int;
    pub fn bpp_prove_pool_openings(p: *mut bpp_prove_pool, items: *const bpp_prove_item, n_items: usize, commitments_out: *mut u8,
                                   commit_stride: usize, proofs_out: *mut u8, proof_stride: usize, proof_lens: *mut usize,
                                   errbuf: *mut c_char, errbuf_len: usize) -> c_int;
    pub fn bpp_prove_pool_openings_stats(p: *mut bpp_prove_pool, openings_calls: *mut u64, both_kinds_calls: *mut u64) -> c_int;
    pub fn bpp_prove_pool_create(ctx: *mut bpp_ctx, params: u64, lanes: u32, max_wait_us: u32, max_calls: u32,
                                 out: *mut *mut bpp_prove_pool) -> c_int;
    pub fn bpp_prove_pool_prove(p: *mut bpp_prove_pool, items: *const bpp_prove_item, n_items: usize, proofs_out: *mut u8,
                                proof_stride: usize, proof_lens: *mut usize, errbuf: *mut c_char, errbuf_len: usize) -> c_int;
    pub fn bpp_prove_pool_set_limits(p: *mut bpp_prove_pool, max_calls: u32, max_proofs: u32) -> c_int;
    pub fn bpp_prove_pool_stats(p: *mut bpp_prove_pool, pooled_calls: *mut u64, engine_calls: *mut u64, solo_calls: *mut u64,
                                largest_calls: *mut u32, largest_proofs: *mut u32) -> c_int;
    pub fn bpp_prove_pool_destroy(p: *mut bpp_prove_pool);
    pub fn bpp_verify_check_resolve(passes: *const bpp_shard_result, n_passes: c_int, out: *mut bpp_shard_result, kind: *mut c_int) -> c_int;
    pub fn bpp_verify_check_stats(ctx: *mut bpp_ctx, out: *mut bpp_verify_check_stats) -> c_int;
    pub fn bpp_batcher_verify_check_stats(b: *mut bpp_batcher, out: *mut bpp_verify_check_stats) -> c_int;
    pub fn bpp_verify_joint_stats(ctx: *mut bpp_ctx, out: *mut bpp_verify_joint_stats) -> c_int;
    pub fn bpp_batcher_verify_joint_stats(b: *mut bpp_batcher, out: *mut bpp_verify_joint_stats) -> c_int;
    pub fn bpp_prove_check_stats(ctx: *mut bpp_ctx, out: *mut bpp_prove_check_stats) -> c_int;
    pub fn bpp_prove_pool_check_stats(p: *mut bpp_prove_pool, out: *mut bpp_prove_check_stats) -> c_int;
    pub fn bpp_prove_check_recovery_stats(ctx: *mut bpp_ctx, replayed: *mut u64, mismatched: *mut u64) -> c_int;
    pub fn bpp_prove_pool_check_recovery_stats(p: *mut bpp_prove_pool, replayed: *mut u64, mismatched: *mut u64) -> c_int;
    // prove calls in flight from one thread: lanes inside one context, tickets, results equal to the blocking calls'
    pub fn bpp_prove_pipeline_depth(ctx: *mut bpp_ctx, depth: u32) -> c_int;
    pub fn bpp_prove_submit(ctx: *mut bpp_ctx, params: u64, items: *const bpp_prove_item, n_items: usize, proof_stride: usize,
                            openings: c_int, commit_stride: usize, ticket: *mut u64, errbuf: *mut c_char, errbuf_len: usize) -> c_int;
    pub fn bpp_prove_collect(ctx: *mut bpp_ctx, ticket: u64, commitments_out: *mut u8, proofs_out: *mut u8, proof_lens: *mut usize,
                             item_status: *mut c_int, errbuf: *mut c_char, errbuf_len: usize) -> c_int;
    pub fn bpp_prove_ticket_done(ctx: *mut bpp_ctx, ticket: u64, done: *mut c_int) -> c_int;
    // diagnostics
    pub fn bpp_batch_trace(ctx: *mut bpp_ctx, batch: u64, what: c_int, out: *mut u8, out_len: usize, written: *mut usize) -> c_int;
    pub fn bpp_batch_shape(ctx: *mut bpp_ctx, batch: u64, n_items: *mut u32, max_rounds: *mut u32, max_mn: *mut u32, total_dyn: *mut u32,
                           groups: *mut u32) -> c_int;
    pub fn bpp_profile_enable(ctx: *mut bpp_ctx, on: c_int) -> c_int;
    pub fn bpp_profile_get(ctx: *mut bpp_ctx, out: *mut bpp_profile) -> c_int;
    pub fn bpp_prove_profile_get(ctx: *mut bpp_ctx, out: *mut bpp_prove_profile) -> c_int;
    pub fn bpp_host_threads() -> c_int;
    pub fn bpp_host_pool_cpu_ns() -> u64;
    pub fn bpp_device_chain_stats(ctx: *mut bpp_ctx, calls: *mut u64, redraws: *mut u64) -> c_int;
    pub fn bpp_transcript_new(label: *const u8, label_len: usize, state203: *mut u8) -> c_int;
    pub fn bpp_transcript_append_message(state203: *mut u8, label: *const u8, label_len: usize, msg: *const u8, msg_len: usize) -> c_int;
    pub fn bpp_transcript_challenge_bytes(state203: *mut u8, label: *const u8, label_len: usize, out: *mut u8, out_len: usize) -> c_int;
    // the reference's TranscriptProtocol and merlin's transcript RNG on 203-byte states (host only)
    pub fn bpp_transcript_validate_and_append_point(state203: *mut u8, label: *const u8, label_len: usize, point32: *const u8,
                                                    errbuf: *mut c_char, errbuf_len: usize) -> c_int;
    pub fn bpp_transcript_challenge_scalar(state203: *mut u8, label: *const u8, label_len: usize, out32: *mut u8, errbuf: *mut c_char,
                                           errbuf_len: usize) -> c_int;
    pub fn bpp_transcript_rng_begin(state203: *const u8, rng203_out: *mut u8) -> c_int;
    pub fn bpp_transcript_rng_rekey(rng203: *mut u8, label: *const u8, label_len: usize, witness: *const u8, witness_len: usize) -> c_int;
    pub fn bpp_transcript_rng_finalize(rng203: *mut u8, random32: *const u8) -> c_int;
    pub fn bpp_transcript_rng_fill(rng203: *mut u8, out: *mut u8, out_len: usize) -> c_int;
    pub fn bpp_transcript_rng_scalar(rng203: *mut u8, out32: *mut u8, errbuf: *mut c_char, errbuf_len: usize) -> c_int;
    pub fn bpp_transcripts_enqueue(ctx: *mut bpp_ctx, states203_dev: *mut u8, n: usize, ops: *const bpp_transcript_op, n_ops: usize,
                                   live_dev: *const u8, done_mask_dev: *mut u8, record_dev: *mut bpp_device_transcripts_record,
                                   ticket: *mut u64) -> c_int;
    pub fn bpp_transcripts_stats(ctx: *mut bpp_ctx, out: *mut bpp_transcripts_stats) -> c_int;
    pub fn bpp_rows_msm_enqueue(ctx: *mut bpp_ctx, input: *const bpp_rows_msm, out_dev: *mut u8, out_stride: usize, live_dev: *const u8,
                                done_mask_dev: *mut u8, record_dev: *mut bpp_device_rows_record, ticket: *mut u64) -> c_int;
    pub fn bpp_rows_scalar_enqueue(ctx: *mut bpp_ctx, n: usize, a: *const bpp_scalar_rows, b: *const bpp_scalar_rows, c: *const bpp_scalar_rows,
                                   out_dev: *mut u8, out_stride: usize, live_dev: *const u8, done_mask_dev: *mut u8,
                                   record_dev: *mut bpp_device_rows_record, ticket: *mut u64) -> c_int;
    pub fn bpp_rows_stats(ctx: *mut bpp_ctx, out: *mut bpp_rows_stats) -> c_int;
    pub fn bpp_verify_batch_states(ctx: *mut bpp_ctx, params: u64, items: *const bpp_verify_item, n_items: usize, action: c_int, chunk: usize,
                                   masks_out: *mut u8, mask_present: *mut u8, states_out203: *mut u8, errbuf: *mut c_char,
                                   errbuf_len: usize) -> c_int;
    pub fn bpp_verify_batch_packed_states(ctx: *mut bpp_ctx, params: u64, input: *const bpp_packed_batch, action: c_int, chunk: usize,
                                          masks_out: *mut u8, mask_present: *mut u8, states_out203: *mut u8, errbuf: *mut c_char,
                                          errbuf_len: usize) -> c_int;
    pub fn bpp_verify_resident_states(ctx: *mut bpp_ctx, batch: u64, action: c_int, chunk: usize, masks_out: *mut u8, mask_present: *mut u8,
                                      states_out203: *mut u8, errbuf: *mut c_char, errbuf_len: usize) -> c_int;
    pub fn bpp_prove_batch_mixed_states(ctx: *mut bpp_ctx, params: u64, items: *const bpp_prove_item, n_items: usize, proofs_out: *mut u8,
                                        proof_stride: usize, proof_lens: *mut usize, item_status: *mut c_int, states_out203: *mut u8,
                                        errbuf: *mut c_char, errbuf_len: usize) -> c_int;
    pub fn bpp_prove_openings_states(ctx: *mut bpp_ctx, params: u64, items: *const bpp_prove_item, n_items: usize, commitments_out: *mut u8,
                                     commit_stride: usize, proofs_out: *mut u8, proof_stride: usize, proof_lens: *mut usize,
                                     item_status: *mut c_int, states_out203: *mut u8, errbuf: *mut c_char, errbuf_len: usize) -> c_int;
    pub fn bpp_batch_secret_bytes(ctx: *mut bpp_ctx, batch: u64, nonzero: *mut u64) -> c_int;
    pub fn bpp_prove_secret_bytes(ctx: *mut bpp_ctx, examined: *mut u64, nonzero: *mut u64) -> c_int;
    pub fn bpp_shader_clock(ctx: *mut bpp_ctx, window_us: u32, ghz: *mut f64) -> c_int;
}
