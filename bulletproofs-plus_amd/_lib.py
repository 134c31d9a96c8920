"""ctypes binding of include/bpp.h.  There is no fallback: a missing or unloadable libbpp_hip.so raises."""
import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_double, c_float, c_int, c_size_t, c_uint8, c_uint32, c_uint64, c_void_p

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libbpp_hip.so")
# BPP_LIB_PATH: load ANOTHER build of the library instead (measurement builds such as -DBPP_KP_PHASES: tools/gpu_kp_phases.sh).  The
# product's own .so is never swapped in place for one; whoever sets the variable names the file and gets exactly that file.
if os.environ.get("BPP_LIB_PATH"):
    LIB_PATH = os.path.abspath(os.environ["BPP_LIB_PATH"])

u8p = POINTER(c_uint8)


class VerifyItem(Structure):
    _fields_ = [("proof", c_void_p), ("proof_len", c_size_t), ("commitments32", c_void_p), ("m", c_uint32),
                ("min_values", c_void_p), ("min_present", c_void_p), ("seed_nonce32", c_void_p),
                ("transcript_state", c_void_p), ("transcript_label", c_void_p), ("label_len", c_size_t)]


class ProveItem(Structure):
    _fields_ = [("values", c_void_p), ("blindings32", c_void_p), ("commitments32", c_void_p), ("m", c_uint32),
                ("min_values", c_void_p), ("min_present", c_void_p), ("seed_nonce32", c_void_p),
                ("transcript_state", c_void_p), ("transcript_label", c_void_p), ("label_len", c_size_t),
                ("rng_bytes", c_void_p), ("rng_len", c_size_t)]


class PackedBatch(Structure):
    """bpp_packed_batch: a homogeneous batch as contiguous arrays"""
    _fields_ = [("n_items", c_size_t), ("proofs", c_void_p), ("proof_len", c_size_t), ("proof_stride", c_size_t),
                ("commitments32", c_void_p), ("m", c_uint32), ("min_values", c_void_p), ("min_present", c_void_p),
                ("seed_nonces32", c_void_p), ("seed_present", c_void_p), ("transcript_state", c_void_p),
                ("transcript_label", c_void_p), ("label_len", c_size_t)]


class MixedBatch(Structure):
    """bpp_mixed_batch: a batch of mixed aggregation factors as arrays of rows"""
    _fields_ = [("n_items", c_size_t), ("proofs", c_void_p), ("proof_stride", c_size_t), ("proof_lens", c_void_p), ("m", c_void_p),
                ("m_stride", c_uint32), ("commitments32", c_void_p), ("min_values", c_void_p), ("min_present", c_void_p),
                ("seed_nonces32", c_void_p), ("seed_present", c_void_p), ("transcript_state", c_void_p),
                ("transcript_label", c_void_p), ("label_len", c_size_t)]


class ShardResult(Structure):
    """bpp_shard_result: outcome of one batch of a sharded wave"""
    _fields_ = [("code", c_int), ("tier", c_int), ("rank", c_int), ("index", c_uint32), ("msg", ctypes.c_char * 160)]


class ShardTiming(Structure):
    _fields_ = [(n, c_float) for n in ("enqueue1_ms", "wait1_ms", "gather1_ms", "chains_ms", "enqueue2_ms", "wait2_ms",
                                       "gather2_ms")] + [("batches", c_uint32)]


class Profile(Structure):
    _fields_ = [(n, c_float) for n in ("transcripts_ms", "decompress_ms", "chain_host_ms", "scalars_ms", "reduce_ms",
                                       "msm_digits_ms", "msm_sort_ms", "msm_accumulate_ms", "msm_bucket_reduce_ms",
                                       "msm_final_ms", "total_ms")] + \
               [(n, c_uint32) for n in ("msm_terms", "msm_window_bits", "msm_windows", "msm_groups")] + [("masks_ms", c_float), ("chain_device_ms", c_float)]


class ProveProfile(Structure):
    _fields_ = [("fb_msm_ms", c_float), ("total_ms", c_float), ("fb_terms", c_uint64), ("fb_launches", c_uint32),
                ("fb_window_bits", c_uint32), ("fb_windows", c_uint32), ("sub_batches", c_uint32)]


class ProveCheckStats(Structure):
    """struct bpp_prove_check_stats: what the prover's self-check ("prove_check" = 1) of a context has done"""
    _fields_ = [(n, c_uint64) for n in ("calls", "proofs", "batch_failures", "remade", "failed")]


class VerifyCheckStats(Structure):
    """struct bpp_verify_check_stats: what the rechecks of rejections ("verify_check" = 1) of a context have done"""
    _fields_ = [(n, c_uint64) for n in ("calls", "rechecked_groups", "confirmed", "overturned", "tie_breaks", "undecided")]


class VerifyJointStats(Structure):
    """struct bpp_verify_joint_stats: what the joint final checks ("verify_joint" = 1) of a context have done"""
    _fields_ = [(n, c_uint64) for n in ("calls", "accepted", "fallbacks", "fallback_all_ok")]


class IngestStats(Structure):
    """struct bpp_ingest_stats: what the uploads from device memory of a context came to"""
    _fields_ = [(n, c_uint64) for n in ("device_calls", "host_fallback_calls", "fallback_bytes")]


class DeviceVerdict(Structure):
    """bpp_device_verdict: one group's record of bpp_verify_enqueue, 16 bytes, as it lies in device memory"""
    _fields_ = [("code", ctypes.c_int32), ("tier", c_uint32), ("index", c_uint32), ("flags", c_uint32)]


class EnqueueStats(Structure):
    """struct bpp_enqueue_stats: what the enqueued verifications of a context came to"""
    _fields_ = [(n, c_uint64) for n in ("calls", "groups", "host_waits", "layouts_in_call")]


class DeviceRefill(Structure):
    """bpp_device_refill: the record of bpp_batch_refill_enqueue, 16 bytes, as it lies in device memory"""
    _fields_ = [("code", ctypes.c_int32), ("msg", c_uint32), ("index", c_uint32), ("flags", c_uint32)]


class RefillStats(Structure):
    """struct bpp_refill_stats: what the refills of a context came to"""
    _fields_ = [(n, c_uint64) for n in ("calls", "first_calls", "host_waits")]


class ProveArrays(Structure):
    """bpp_prove_arrays: the openings of a prove call as arrays of rows in device memory (m and the transcript on the host)"""
    _fields_ = [("n_items", c_size_t), ("m", c_void_p), ("m_stride", c_uint32), ("values", c_void_p), ("blindings32", c_void_p),
                ("commitments32", c_void_p), ("min_values", c_void_p), ("min_present", c_void_p), ("seed_nonces32", c_void_p),
                ("seed_present", c_void_p), ("rng_bytes", c_void_p), ("rng_stride", c_size_t), ("transcript_state", c_void_p),
                ("transcript_label", c_void_p), ("label_len", c_size_t)]


class DeviceProveStatus(Structure):
    """bpp_device_prove_status: one item's record of bpp_prove_openings_device, 8 bytes, as it lies in device memory"""
    _fields_ = [("code", ctypes.c_int32), ("msg", c_uint32)]


class DeviceProveSummary(Structure):
    """bpp_device_prove_summary: the one record of a bpp_prove_enqueue, 32 bytes, as it lies in device memory"""
    _fields_ = [("code", ctypes.c_int32)] + [(n, c_uint32) for n in ("msg", "index", "flags", "n_ok", "n_failed", "n_empty", "reserved")]


class ProveEnqueueStats(Structure):
    """struct bpp_prove_enqueue_stats: what the stream-ordered prove calls of a context cost the host"""
    _fields_ = [(n, c_uint64) for n in ("calls", "first_calls", "host_waits", "allocations")]


class TranscriptOp(Structure):
    """bpp_transcript_op: one Merlin operation of a bpp_transcripts_enqueue (the label on the host, the rows in device memory)"""
    _fields_ = [("kind", c_uint32), ("label", c_void_p), ("label_len", c_uint32), ("data_dev", c_void_p), ("stride", c_size_t),
                ("len", c_uint32), ("lens_dev", c_void_p)]


class DeviceTranscriptsRecord(Structure):
    """bpp_device_transcripts_record: the one record of a bpp_transcripts_enqueue, 16 bytes, as it lies in device memory"""
    _fields_ = [(n, c_uint32) for n in ("n_done", "n_void", "first_void", "flags")]


class TranscriptsStats(Structure):
    """struct bpp_transcripts_stats: what the bpp_transcripts_enqueue calls of a context cost the host"""
    _fields_ = [(n, c_uint64) for n in ("calls", "first_calls", "host_waits")]


class RowsMsm(Structure):
    """bpp_rows_msm: n rows of K (scalar, point) terms in device memory; point_stride 0 = one row of K shared bases"""
    _fields_ = [("n", c_size_t), ("K", c_uint32), ("scalars_dev", c_void_p), ("scalar_stride", c_size_t), ("points_dev", c_void_p),
                ("point_stride", c_size_t)]


class ScalarRows(Structure):
    """bpp_scalar_rows: one operand of bpp_rows_scalar_enqueue; stride 0 = one 32-byte scalar for every row"""
    _fields_ = [("dev", c_void_p), ("stride", c_size_t)]


class DeviceRowsRecord(Structure):
    """bpp_device_rows_record: the one record of a bpp_rows_*_enqueue, 16 bytes, as it lies in device memory"""
    _fields_ = [(n, c_uint32) for n in ("n_done", "n_void", "first_void", "flags")]


class RowsStats(Structure):
    """struct bpp_rows_stats: what the bpp_rows_*_enqueue calls of a context cost the host"""
    _fields_ = [(n, c_uint64) for n in ("calls", "first_calls", "host_waits")]


class ProveDeviceStats(Structure):
    """struct bpp_prove_device_stats: what the prove calls from device arrays of a context came to"""
    _fields_ = [(n, c_uint64) for n in ("calls", "items", "device_findings", "host_findings")]


class RuntimeInfo(Structure):
    """bpp_runtime_info: what the library sees of its runtime preconditions (hardware queues, contexts, the small-call gate)"""
    _fields_ = [("device", c_int), ("contexts", c_uint32), ("contexts_peak", c_uint32), ("hw_queues", c_uint32),
                ("host_threads", c_uint32), ("small_call_limit", c_uint32), ("small_calls_in_flight", c_uint32),
                ("small_calls", c_uint64), ("small_calls_queued", c_uint64), ("oversubscribed", c_uint32)]


# bpp_all_gather_fn: int (*)(void *user, const void *send, void *recv, size_t bytes_per_rank)
ALL_GATHER_FN = ctypes.CFUNCTYPE(c_int, c_void_p, c_void_p, c_void_p, c_size_t)

# every symbol include/bpp.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("bpp_ctx_create", c_int, [POINTER(c_void_p), c_int]),
    ("bpp_ctx_create_on_stream", c_int, [POINTER(c_void_p), c_int, c_void_p]),
    ("bpp_ctx_destroy", None, [c_void_p]),
    ("bpp_ctx_last_error", c_char_p, [c_void_p]),
    ("bpp_ctx_set_option", c_int, [c_void_p, c_char_p, c_int]),
    ("bpp_precomp_create", c_int, [c_void_p, c_void_p, c_size_t, POINTER(c_uint64)]),
    ("bpp_precomp_destroy", c_int, [c_void_p, c_uint64]),
    ("bpp_precomp_retain", c_int, [c_void_p, c_uint64]),
    ("bpp_msm_mixed", c_int, [c_void_p, c_uint64, c_void_p, c_size_t, c_void_p, c_void_p, c_size_t, c_void_p]),
    ("bpp_msm_vartime", c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    ("bpp_msm_vartime_batched", c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    ("bpp_msm_last_plan", c_int, [c_void_p, c_void_p]),
    ("bpp_msm_ct", c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    ("bpp_msm_ct_batched", c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    ("bpp_msm_ct_secret_bytes", c_int, [c_void_p, POINTER(c_uint64), POINTER(c_uint64)]),
    ("bpp_params_create", c_int, [c_void_p, c_uint32, c_uint32, c_uint32, c_void_p, c_void_p, POINTER(c_uint64)]),
    ("bpp_params_destroy", c_int, [c_void_p, c_uint64]),
    ("bpp_params_retain", c_int, [c_void_p, c_uint64]),
    ("bpp_params_export", c_int, [c_void_p, c_uint64, c_void_p, c_void_p, c_void_p, c_void_p]),
    ("bpp_pedersen_commit", c_int, [c_void_p, c_uint64, c_void_p, c_void_p, c_uint32, c_size_t, c_void_p]),
    ("bpp_verify_batch", c_int, [c_void_p, c_uint64, POINTER(VerifyItem), c_size_t, c_int, c_size_t, c_void_p,
                                 c_void_p, c_void_p, c_size_t]),
    ("bpp_verify_batch_with_challenges", c_int, [c_void_p, c_uint64, POINTER(VerifyItem), c_size_t, POINTER(c_void_p),
                                                 c_void_p, c_int, c_size_t, c_void_p, c_void_p, c_void_p, c_size_t]),
    ("bpp_batch_upload", c_int, [c_void_p, c_uint64, POINTER(VerifyItem), c_size_t, POINTER(c_uint64), c_void_p,
                                 c_size_t]),
    ("bpp_batch_upload_packed", c_int, [c_void_p, c_uint64, POINTER(PackedBatch), POINTER(c_uint64), c_void_p, c_size_t]),
    ("bpp_verify_batch_packed", c_int, [c_void_p, c_uint64, POINTER(PackedBatch), c_int, c_size_t, c_void_p, c_void_p,
                                        c_void_p, c_size_t]),
    ("bpp_batch_upload_packed_device", c_int, [c_void_p, c_uint64, POINTER(PackedBatch), POINTER(c_uint64), c_void_p, c_size_t]),
    ("bpp_verify_batch_packed_device", c_int, [c_void_p, c_uint64, POINTER(PackedBatch), c_int, c_size_t, c_void_p, c_void_p,
                                               c_void_p, c_size_t]),
    ("bpp_batch_upload_mixed", c_int, [c_void_p, c_uint64, POINTER(MixedBatch), POINTER(c_uint64), c_void_p, c_size_t]),
    ("bpp_verify_batch_mixed", c_int, [c_void_p, c_uint64, POINTER(MixedBatch), c_int, c_size_t, c_void_p, c_void_p, c_void_p, c_size_t]),
    ("bpp_batch_upload_mixed_device", c_int, [c_void_p, c_uint64, POINTER(MixedBatch), POINTER(c_uint64), c_void_p, c_size_t]),
    ("bpp_verify_batch_mixed_device", c_int, [c_void_p, c_uint64, POINTER(MixedBatch), c_int, c_size_t, c_void_p, c_void_p, c_void_p,
                                              c_size_t]),
    ("bpp_device_pointer_check", c_int, [c_void_p, c_void_p, POINTER(c_int)]),
    ("bpp_ingest_stats", c_int, [c_void_p, POINTER(IngestStats)]),
    ("bpp_ctx_pipeline_depth", c_int, [c_void_p, c_uint32]),
    ("bpp_verify_submit_packed", c_int, [c_void_p, c_uint64, POINTER(PackedBatch), c_int, c_size_t, POINTER(c_uint64),
                                         c_void_p, c_size_t]),
    ("bpp_verify_collect", c_int, [c_void_p, c_uint64, c_void_p, c_void_p, c_void_p, c_size_t]),
    ("bpp_batch_destroy", c_int, [c_void_p, c_uint64]),
    ("bpp_verify_resident", c_int, [c_void_p, c_uint64, c_int, c_size_t, c_void_p, c_void_p, c_void_p, c_size_t]),
    ("bpp_verify_phase1", c_int, [c_void_p, c_uint64, c_void_p, c_void_p, c_size_t]),
    ("bpp_weights_from_chain", c_int, [c_void_p, c_size_t, c_void_p]),
    ("bpp_weights_from_chains", c_int, [c_void_p, c_size_t, c_size_t, c_void_p]),
    ("bpp_verify_phase2", c_int, [c_void_p, c_uint64, c_void_p, c_void_p, c_void_p, c_size_t]),
    ("bpp_accumulators_sum_is_identity", c_int, [c_void_p, c_void_p, c_size_t, POINTER(c_int)]),
    ("bpp_comm_unique_id", c_int, [c_void_p]),
    ("bpp_comm_create", c_int, [c_void_p, c_void_p, c_int, c_int, POINTER(c_void_p)]),
    ("bpp_comm_adopt", c_int, [c_void_p, c_void_p, c_int, c_int, POINTER(c_void_p)]),
    ("bpp_comm_create_callbacks", c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, POINTER(c_void_p)]),
    ("bpp_comm_create_local", c_int, [c_void_p, c_uint64, c_int, c_int, POINTER(c_void_p)]),
    ("bpp_comm_destroy", None, [c_void_p]),
    ("bpp_comm_last_error", c_char_p, [c_void_p]),
    ("bpp_comm_set_timeout", c_int, [c_void_p, c_uint32]),
    ("bpp_comm_last_timing", c_int, [c_void_p, POINTER(ShardTiming)]),
    ("bpp_verify_sharded", c_int, [c_void_p, c_void_p, c_uint64, POINTER(c_uint32), POINTER(c_int), POINTER(c_int), c_void_p,
                                   c_size_t]),
    ("bpp_verify_sharded_wave", c_int, [c_void_p, POINTER(c_void_p), POINTER(c_uint64), c_size_t, POINTER(c_uint32),
                                        POINTER(ShardResult)]),
    ("bpp_verify_sharded_groups", c_int, [c_void_p, c_void_p, c_uint64, c_size_t, POINTER(c_uint32), POINTER(ShardResult)]),
    ("bpp_verify_sharded_groups_wave", c_int, [c_void_p, POINTER(c_void_p), POINTER(c_uint64), c_size_t, c_size_t, POINTER(c_uint32),
                                               POINTER(ShardResult)]),
    ("bpp_verify_resident_groups", c_int, [c_void_p, c_uint64, POINTER(c_uint32), c_size_t, POINTER(ShardResult)]),
    ("bpp_verify_resident_groups_actions", c_int, [c_void_p, c_uint64, POINTER(c_uint32), c_size_t, POINTER(c_int), POINTER(ShardResult),
                                                   c_void_p, c_void_p]),
    ("bpp_verify_enqueue", c_int, [c_void_p, c_uint64, POINTER(c_uint32), c_size_t, c_size_t, POINTER(c_int), c_int, c_void_p, c_void_p,
                                   c_void_p, POINTER(c_uint64)]),
    ("bpp_enqueue_done", c_int, [c_void_p, c_uint64, POINTER(c_int)]),
    ("bpp_enqueue_wait", c_int, [c_void_p, c_uint64]),
    ("bpp_verdict_result", c_int, [POINTER(DeviceVerdict), POINTER(ShardResult)]),
    ("bpp_enqueue_stats", c_int, [c_void_p, POINTER(EnqueueStats)]),
    ("bpp_batch_refill_enqueue", c_int, [c_void_p, c_uint64, POINTER(PackedBatch), c_void_p, POINTER(c_uint64)]),
    ("bpp_refill_result", c_int, [POINTER(DeviceRefill), POINTER(ShardResult)]),
    ("bpp_refill_stats", c_int, [c_void_p, POINTER(RefillStats)]),
    ("bpp_batch_refill_enqueue_count", c_int, [c_void_p, c_uint64, POINTER(PackedBatch), c_void_p, c_void_p, POINTER(c_uint64)]),
    ("bpp_batch_refill_enqueue_live", c_int, [c_void_p, c_uint64, POINTER(PackedBatch), c_void_p, c_void_p, POINTER(c_uint64)]),
    ("bpp_batch_refill_enqueue_mixed", c_int, [c_void_p, c_uint64, POINTER(MixedBatch), c_void_p, c_void_p, c_void_p, POINTER(c_uint64)]),
    ("bpp_batch_upload_packed_device_transcripts", c_int, [c_void_p, c_uint64, POINTER(PackedBatch), c_void_p, POINTER(c_uint64), c_void_p,
                                                           c_size_t]),
    ("bpp_batch_upload_mixed_device_transcripts", c_int, [c_void_p, c_uint64, POINTER(MixedBatch), c_void_p, POINTER(c_uint64), c_void_p,
                                                          c_size_t]),
    ("bpp_batch_refill_enqueue_transcripts", c_int, [c_void_p, c_uint64, POINTER(PackedBatch), c_void_p, c_void_p, c_void_p, c_void_p,
                                                     POINTER(c_uint64)]),
    ("bpp_batch_refill_enqueue_mixed_transcripts", c_int, [c_void_p, c_uint64, POINTER(MixedBatch), c_void_p, c_void_p, c_void_p, c_void_p,
                                                           POINTER(c_uint64)]),
    ("bpp_verify_enqueue_states", c_int, [c_void_p, c_uint64, POINTER(c_uint32), c_size_t, c_size_t, POINTER(c_int), c_int, c_void_p, c_void_p,
                                          c_void_p, c_void_p, POINTER(c_uint64)]),
    ("bpp_enqueue_weights", c_int, [c_void_p, c_uint64, c_void_p, POINTER(c_uint64)]),
    ("bpp_batcher_verify_action", c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_char_p, c_size_t]),
    ("bpp_batcher_set_limits", c_int, [c_void_p, c_uint32, c_uint32]),
    ("bpp_batcher_largest_pool", c_int, [c_void_p, POINTER(c_uint32), POINTER(c_uint32)]),
    ("bpp_runtime_info_get", c_int, [c_void_p, POINTER(RuntimeInfo)]),
    ("bpp_small_call_limit", c_int, [c_void_p, c_int]),
    ("bpp_batcher_create", c_int, [c_void_p, c_uint64, c_void_p, c_uint32, c_uint32, c_uint32, POINTER(c_void_p)]),
    ("bpp_batcher_verify", c_int, [c_void_p, c_void_p, c_char_p, c_size_t]),
    ("bpp_batcher_stats", c_int, [c_void_p, POINTER(c_uint64), POINTER(c_uint64), POINTER(c_uint64)]),
    ("bpp_batcher_destroy", None, [c_void_p]),
    ("bpp_shard_local_trailer", c_int, [c_void_p, c_void_p, c_void_p, c_uint32, c_uint32, c_void_p]),
    ("bpp_shard_trailer", c_int, [c_int, c_int, c_uint32, c_char_p, c_void_p]),
    ("bpp_shard_resolve", c_int, [c_void_p, c_size_t, c_int, POINTER(c_int), POINTER(c_int), POINTER(c_uint32), c_void_p,
                                  c_size_t]),
    ("bpp_prove_batch", c_int, [c_void_p, c_uint64, POINTER(ProveItem), c_size_t, c_void_p, c_size_t, POINTER(c_size_t),
                                c_void_p, c_size_t]),
    ("bpp_prove_batch_mixed", c_int, [c_void_p, c_uint64, POINTER(ProveItem), c_size_t, c_void_p, c_size_t, POINTER(c_size_t),
                                      POINTER(c_int), c_void_p, c_size_t]),
    ("bpp_prove_item_message", c_int, [c_void_p, c_uint64, POINTER(ProveItem), c_size_t, c_int, c_void_p, c_size_t]),
    ("bpp_prove_openings", c_int, [c_void_p, c_uint64, POINTER(ProveItem), c_size_t, c_void_p, c_size_t, c_void_p, c_size_t,
                                   POINTER(c_size_t), POINTER(c_int), c_void_p, c_size_t]),
    ("bpp_prove_openings_item_message", c_int, [c_void_p, c_uint64, POINTER(ProveItem), c_void_p, c_size_t, c_size_t, c_int, c_void_p,
                                                c_size_t]),
    ("bpp_prove_openings_device", c_int, [c_void_p, c_uint64, POINTER(ProveArrays), c_void_p, c_size_t, c_void_p, c_size_t,
                                          POINTER(c_size_t), c_void_p, POINTER(c_int), c_void_p, c_size_t]),
    ("bpp_prove_openings_device_transcripts", c_int, [c_void_p, c_uint64, POINTER(ProveArrays), c_void_p, c_void_p, c_size_t, c_void_p,
                                                      c_size_t, POINTER(c_size_t), c_void_p, c_void_p, POINTER(c_int), c_void_p, c_size_t]),
    ("bpp_prove_status_result", c_int, [POINTER(DeviceProveStatus), POINTER(ShardResult)]),
    ("bpp_prove_device_stats", c_int, [c_void_p, POINTER(ProveDeviceStats)]),
    ("bpp_prove_plan_create", c_int, [c_void_p, c_uint64, POINTER(ProveArrays), c_size_t, c_size_t, c_uint32, POINTER(c_uint64), c_void_p,
                                      c_size_t]),
    ("bpp_prove_plan_shape", c_int, [c_void_p, c_uint64, POINTER(c_size_t), POINTER(c_int)]),
    ("bpp_prove_plan_destroy", c_int, [c_void_p, c_uint64]),
    ("bpp_prove_enqueue", c_int, [c_void_p, c_uint64, POINTER(ProveArrays), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_void_p, c_void_p, POINTER(c_uint64)]),
    ("bpp_prove_summary_result", c_int, [POINTER(DeviceProveSummary), POINTER(ShardResult)]),
    ("bpp_prove_enqueue_stats", c_int, [c_void_p, POINTER(ProveEnqueueStats)]),
    ("bpp_prove_pool_openings", c_int, [c_void_p, POINTER(ProveItem), c_size_t, c_void_p, c_size_t, c_void_p, c_size_t,
                                        POINTER(c_size_t), c_void_p, c_size_t]),
    ("bpp_prove_pool_openings_stats", c_int, [c_void_p, POINTER(c_uint64), POINTER(c_uint64)]),
    ("bpp_prove_pool_create", c_int, [c_void_p, c_uint64, c_uint32, c_uint32, c_uint32, POINTER(c_void_p)]),
    ("bpp_prove_pool_prove", c_int, [c_void_p, POINTER(ProveItem), c_size_t, c_void_p, c_size_t, POINTER(c_size_t), c_void_p, c_size_t]),
    ("bpp_prove_pool_set_limits", c_int, [c_void_p, c_uint32, c_uint32]),
    ("bpp_prove_pool_stats", c_int, [c_void_p, POINTER(c_uint64), POINTER(c_uint64), POINTER(c_uint64), POINTER(c_uint32),
                                     POINTER(c_uint32)]),
    ("bpp_prove_pool_destroy", None, [c_void_p]),
    ("bpp_prove_check_stats", c_int, [c_void_p, POINTER(ProveCheckStats)]),
    ("bpp_prove_pool_check_stats", c_int, [c_void_p, POINTER(ProveCheckStats)]),
    ("bpp_prove_check_recovery_stats", c_int, [c_void_p, POINTER(c_uint64), POINTER(c_uint64)]),
    ("bpp_prove_pool_check_recovery_stats", c_int, [c_void_p, POINTER(c_uint64), POINTER(c_uint64)]),
    ("bpp_verify_check_resolve", c_int, [POINTER(ShardResult), c_int, POINTER(ShardResult), POINTER(c_int)]),
    ("bpp_verify_check_stats", c_int, [c_void_p, POINTER(VerifyCheckStats)]),
    ("bpp_batcher_verify_check_stats", c_int, [c_void_p, POINTER(VerifyCheckStats)]),
    ("bpp_verify_joint_stats", c_int, [c_void_p, POINTER(VerifyJointStats)]),
    ("bpp_batcher_verify_joint_stats", c_int, [c_void_p, POINTER(VerifyJointStats)]),
    ("bpp_prove_pipeline_depth", c_int, [c_void_p, c_uint32]),
    ("bpp_prove_submit", c_int, [c_void_p, c_uint64, POINTER(ProveItem), c_size_t, c_size_t, c_int, c_size_t, POINTER(c_uint64),
                                 c_void_p, c_size_t]),
    ("bpp_prove_collect", c_int, [c_void_p, c_uint64, c_void_p, c_void_p, POINTER(c_size_t), POINTER(c_int), c_void_p, c_size_t]),
    ("bpp_prove_ticket_done", c_int, [c_void_p, c_uint64, POINTER(c_int)]),
    ("bpp_batch_trace", c_int, [c_void_p, c_uint64, c_int, c_void_p, c_size_t, POINTER(c_size_t)]),
    ("bpp_batch_shape", c_int, [c_void_p, c_uint64, POINTER(c_uint32), POINTER(c_uint32), POINTER(c_uint32),
                                POINTER(c_uint32), POINTER(c_uint32)]),
    ("bpp_profile_enable", c_int, [c_void_p, c_int]),
    ("bpp_profile_get", c_int, [c_void_p, POINTER(Profile)]),
    ("bpp_prove_profile_get", c_int, [c_void_p, POINTER(ProveProfile)]),
    ("bpp_batch_prepare", c_int, [c_void_p, c_uint64, c_size_t]),
    ("bpp_host_threads", c_int, []),
    ("bpp_host_pool_cpu_ns", c_uint64, []),
    ("bpp_device_chain_stats", c_int, [c_void_p, POINTER(c_uint64), POINTER(c_uint64)]),
    ("bpp_shader_clock", c_int, [c_void_p, c_uint32, POINTER(c_double)]),
    ("bpp_transcript_new", c_int, [c_void_p, c_size_t, c_void_p]),
    ("bpp_transcript_append_message", c_int, [c_void_p, c_void_p, c_size_t, c_void_p, c_size_t]),
    ("bpp_transcript_challenge_bytes", c_int, [c_void_p, c_void_p, c_size_t, c_void_p, c_size_t]),
    ("bpp_transcript_validate_and_append_point", c_int, [c_void_p, c_void_p, c_size_t, c_void_p, c_char_p, c_size_t]),
    ("bpp_transcript_challenge_scalar", c_int, [c_void_p, c_void_p, c_size_t, c_void_p, c_char_p, c_size_t]),
    ("bpp_transcript_rng_begin", c_int, [c_void_p, c_void_p]),
    ("bpp_transcript_rng_rekey", c_int, [c_void_p, c_void_p, c_size_t, c_void_p, c_size_t]),
    ("bpp_transcript_rng_finalize", c_int, [c_void_p, c_void_p]),
    ("bpp_transcript_rng_fill", c_int, [c_void_p, c_void_p, c_size_t]),
    ("bpp_transcript_rng_scalar", c_int, [c_void_p, c_void_p, c_char_p, c_size_t]),
    ("bpp_transcripts_enqueue", c_int, [c_void_p, c_void_p, c_size_t, POINTER(TranscriptOp), c_size_t, c_void_p, c_void_p, c_void_p,
                                        POINTER(c_uint64)]),
    ("bpp_transcripts_stats", c_int, [c_void_p, POINTER(TranscriptsStats)]),
    ("bpp_rows_msm_enqueue", c_int, [c_void_p, POINTER(RowsMsm), c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, POINTER(c_uint64)]),
    ("bpp_rows_scalar_enqueue", c_int, [c_void_p, c_size_t, POINTER(ScalarRows), POINTER(ScalarRows), POINTER(ScalarRows), c_void_p, c_size_t,
                                        c_void_p, c_void_p, c_void_p, POINTER(c_uint64)]),
    ("bpp_rows_stats", c_int, [c_void_p, POINTER(RowsStats)]),
    ("bpp_verify_batch_states", c_int, [c_void_p, c_uint64, POINTER(VerifyItem), c_size_t, c_int, c_size_t, c_void_p, c_void_p,
                                        c_void_p, c_void_p, c_size_t]),
    ("bpp_verify_batch_packed_states", c_int, [c_void_p, c_uint64, POINTER(PackedBatch), c_int, c_size_t, c_void_p, c_void_p,
                                               c_void_p, c_void_p, c_size_t]),
    ("bpp_verify_resident_states", c_int, [c_void_p, c_uint64, c_int, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t]),
    ("bpp_prove_batch_mixed_states", c_int, [c_void_p, c_uint64, POINTER(ProveItem), c_size_t, c_void_p, c_size_t, POINTER(c_size_t),
                                             POINTER(c_int), c_void_p, c_void_p, c_size_t]),
    ("bpp_prove_openings_states", c_int, [c_void_p, c_uint64, POINTER(ProveItem), c_size_t, c_void_p, c_size_t, c_void_p, c_size_t,
                                          POINTER(c_size_t), POINTER(c_int), c_void_p, c_void_p, c_size_t]),
    ("bpp_batch_secret_bytes", c_int, [c_void_p, c_uint64, POINTER(c_uint64)]),
    ("bpp_prove_secret_bytes", c_int, [c_void_p, POINTER(c_uint64), POINTER(c_uint64)]),
]

_lib = None


def load():
    """Load libbpp_hip.so and bind every declared symbol; raises if the extension is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("libbpp_hip.so is missing (%s): run __graft_entry__.build(); there is no CPU fallback"
                           % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    other_build = bool(os.environ.get("BPP_LIB_PATH"))
    for name, res, args in SYMBOLS:
        if other_build and not hasattr(lib, name):
            continue  # an OLDER build named by BPP_LIB_PATH (the parent arm of an A/B) lacks the newest entry points: calling one raises
        fn = getattr(lib, name)  # AttributeError if the library does not export it
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib
