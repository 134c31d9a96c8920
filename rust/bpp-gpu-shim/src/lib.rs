//! Safe wrappers over libbpp_hip.so for the two calls the reference crate routes through the GPU:
//! `RangeProof::verify_batch` (src/range_proof.rs:712-752) and `RangeProof::prove_with_rng` (:232-608).
//!
//! Everything crosses as bytes (32-byte ristretto255 encodings, 32-byte canonical scalars, `RangeProof::to_bytes()`), so
//! this crate does not depend on curve25519-dalek or on the reference crate; `patch/range_proof_gpu.rs` is the code that
//! lives INSIDE the reference crate (its fields and `RangeProofTranscript` are private) and calls into here.
pub mod ffi;

use core::ffi::c_int;
use std::{collections::HashMap, ffi::{CStr, CString}, ptr, sync::{Arc, Mutex, OnceLock}};

/// Mirror of `tari_bulletproofs_plus::errors::ProofError` (src/errors.rs:11-28) plus engine faults.
#[derive(Debug, Clone, PartialEq, Eq)]
pub enum GpuError {
    VerificationFailed(String),
    InvalidArgument(String),
    InvalidLength(String),
    InvalidBlake2b,
    SizeOverflow,
    /// HIP failure, no gfx950 device, bad handle, a proof that failed the prover's self-check (`ffi::BPP_ERR_SELF_CHECK`): no
    /// reference analogue
    Engine(i32, String),
}

fn map_rc(rc: c_int, msg: String) -> Result<(), GpuError> {
    match rc {
        ffi::BPP_OK => Ok(()),
        ffi::BPP_ERR_VERIFICATION_FAILED => Err(GpuError::VerificationFailed(msg)),
        ffi::BPP_ERR_INVALID_ARGUMENT => Err(GpuError::InvalidArgument(msg)),
        ffi::BPP_ERR_INVALID_LENGTH => Err(GpuError::InvalidLength(msg)),
        ffi::BPP_ERR_INVALID_BLAKE2B => Err(GpuError::InvalidBlake2b),
        ffi::BPP_ERR_SIZE_OVERFLOW => Err(GpuError::SizeOverflow),
        ffi::BPP_ERR_SELF_CHECK => Err(GpuError::Engine(ffi::BPP_ERR_SELF_CHECK, msg)),
        other => Err(GpuError::Engine(other, msg)),
    }
}

/// VerifyAction (src/range_proof.rs:46-54)
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
#[repr(i32)]
pub enum Action {
    VerifyOnly = 0,
    RecoverAndVerify = 1,
    RecoverOnly = 2,
}

/// One device context (device + stream + work buffers).  Calls on one context are serialised by the engine; use one
/// context per host thread for concurrency.  `Params` handles are shared between contexts (Arc semantics).
pub struct Engine {
    ctx: *mut ffi::bpp_ctx,
}
unsafe impl Send for Engine {}

impl Engine {
    pub fn new(device_id: i32) -> Result<Self, GpuError> {
        let mut ctx = ptr::null_mut();
        map_rc(unsafe { ffi::bpp_ctx_create(&mut ctx, device_id) }, "bpp_ctx_create: a gfx950 device is required".into())?;
        Ok(Engine { ctx })
    }

    fn last_error(&self) -> String {
        unsafe { CStr::from_ptr(ffi::bpp_ctx_last_error(self.ctx)).to_string_lossy().into_owned() }
    }

    /// `bpp_ctx_set_option`: a per-context knob (include/bpp.h lists them; -1 restores the engine's rule), e.g. "prove_check" = 1
    pub fn set_option(&self, name: &str, value: i32) -> Result<(), GpuError> {
        let c = CString::new(name).map_err(|_| GpuError::InvalidArgument(String::from("option name holds a NUL byte")))?;
        map_rc(unsafe { ffi::bpp_ctx_set_option(self.ctx, c.as_ptr(), value) }, self.last_error())
    }

    /// RangeParameters::init (src/range_parameters.rs:32-58); `h_base` / `g_bases` = None: the reference's defaults.
    /// Derives the generators and builds the device tables: expensive (milliseconds).  Callers go through
    /// `cached_params`, which does it once per parameter set and process.
    pub fn params(&self, bit_length: usize, max_aggregation: usize, extension_degree: usize, h_base: Option<&[u8; 32]>,
                  g_bases: Option<&[u8]>) -> Result<Params, GpuError> {
        let mut handle = 0u64;
        let rc = unsafe {
            ffi::bpp_params_create(self.ctx, bit_length as u32, max_aggregation as u32, extension_degree as u32,
                                   h_base.map_or(ptr::null(), |h| h.as_ptr()), g_bases.map_or(ptr::null(), |g| g.as_ptr()), &mut handle)
        };
        map_rc(rc, self.last_error())?;
        Ok(Params { handle, extension_degree, owner: self.ctx })
    }

    /// `RangeProof::verify_batch` over a homogeneous batch handed over as contiguous arrays (bpp_verify_batch_packed): what
    /// the in-crate patch uses whenever all statements share the aggregation factor and all proofs the length.
    pub fn verify_batch_packed(&self, params: &Params, input: &PackedBatch<'_>, action: Action, chunk: usize)
                               -> Result<Vec<Option<Vec<[u8; 32]>>>, GpuError> {
        let t = params.extension_degree;
        let raw = input.raw();
        let mut masks = vec![0u8; input.n_items * t * 32];
        let mut present = vec![0u8; input.n_items];
        let mut err = [0 as core::ffi::c_char; 256];
        let rc = unsafe {
            ffi::bpp_verify_batch_packed(self.ctx, params.handle, &raw, action as c_int, chunk, masks.as_mut_ptr(), present.as_mut_ptr(),
                                         err.as_mut_ptr(), err.len())
        };
        let out = map_rc(rc, unsafe { CStr::from_ptr(err.as_ptr()) }.to_string_lossy().into_owned()).map(|_| unpack_masks(&masks, &present, t));
        masks.iter_mut().for_each(|b| *b = 0); // recovered masks are secrets (src/extended_mask.rs:14)
        out
    }

    /// Pipelined form: returns at once with a ticket; `collect` blocks for the verdict.  Upload k+1 overlaps verify k
    /// inside this one context (bpp_verify_submit_packed / bpp_verify_collect).
    pub fn submit_packed(&self, params: &Params, input: &PackedBatch<'_>, action: Action, chunk: usize) -> Result<Ticket, GpuError> {
        let raw = input.raw();
        let mut ticket = 0u64;
        let mut err = [0 as core::ffi::c_char; 256];
        let rc = unsafe {
            ffi::bpp_verify_submit_packed(self.ctx, params.handle, &raw, action as c_int, chunk, &mut ticket, err.as_mut_ptr(), err.len())
        };
        map_rc(rc, unsafe { CStr::from_ptr(err.as_ptr()) }.to_string_lossy().into_owned())?;
        Ok(Ticket { id: ticket, n_items: input.n_items, t: params.extension_degree })
    }

    pub fn collect(&self, ticket: Ticket) -> Result<Vec<Option<Vec<[u8; 32]>>>, GpuError> {
        let mut masks = vec![0u8; ticket.n_items * ticket.t * 32];
        let mut present = vec![0u8; ticket.n_items];
        let mut err = [0 as core::ffi::c_char; 256];
        let rc = unsafe { ffi::bpp_verify_collect(self.ctx, ticket.id, masks.as_mut_ptr(), present.as_mut_ptr(), err.as_mut_ptr(), err.len()) };
        let out = map_rc(rc, unsafe { CStr::from_ptr(err.as_ptr()) }.to_string_lossy().into_owned()).map(|_| unpack_masks(&masks, &present, ticket.t));
        masks.iter_mut().for_each(|b| *b = 0);
        out
    }

    /// This rank's shard of ONE reference batch spread over `counts.len()` GPUs: uploads `input` (counts[rank] proofs) and
    /// runs bpp_verify_sharded on `comm`.  Every rank returns the same result; `ShardError` carries the numeric tier.
    pub fn verify_sharded(&self, comm: &ShardComm, params: &Params, input: &PackedBatch<'_>, counts: &[u32]) -> Result<(), ShardError> {
        let raw = input.raw();
        let mut batch = 0u64;
        let mut err = [0 as core::ffi::c_char; 256];
        let up = unsafe { ffi::bpp_batch_upload_packed(self.ctx, params.handle, &raw, &mut batch, err.as_mut_ptr(), err.len()) };
        // NOTE: a construction error here is rank-local: the caller must still let the other ranks know (they would wait in
        // the first all_gather).  RangeStatement / RangeProof objects that exist have passed these checks already.
        map_rc(up, unsafe { CStr::from_ptr(err.as_ptr()) }.to_string_lossy().into_owned()).map_err(|e| ShardError { error: e, tier: ffi::BPP_TIER_CONSTRUCTION, rank: comm.rank })?;
        let (mut tier, mut rank) = (0 as c_int, -1 as c_int);
        let rc = unsafe { ffi::bpp_verify_sharded(comm.raw, self.ctx, batch, counts.as_ptr(), &mut tier, &mut rank, err.as_mut_ptr(), err.len()) };
        unsafe { ffi::bpp_batch_destroy(self.ctx, batch) };
        map_rc(rc, unsafe { CStr::from_ptr(err.as_ptr()) }.to_string_lossy().into_owned()).map_err(|e| ShardError { error: e, tier, rank })
    }

    /// This rank's shards of `n_groups` reference batches at once: `input` holds n_groups x counts[rank] proofs, group g =
    /// proofs [g c, (g + 1) c).  One set of kernel launches and two all_gathers for all groups (bpp_verify_sharded_groups);
    /// per group the result a `verify_sharded` call on that batch alone would give.
    pub fn verify_sharded_groups(&self, comm: &ShardComm, params: &Params, input: &PackedBatch<'_>, n_groups: usize, counts: &[u32])
                                 -> Result<Vec<Result<(), ShardError>>, GpuError> {
        let raw = input.raw();
        let mut batch = 0u64;
        let mut err = [0 as core::ffi::c_char; 256];
        let up = unsafe { ffi::bpp_batch_upload_packed(self.ctx, params.handle, &raw, &mut batch, err.as_mut_ptr(), err.len()) };
        map_rc(up, unsafe { CStr::from_ptr(err.as_ptr()) }.to_string_lossy().into_owned())?;  // rank-local: see verify_sharded
        let mut res: Vec<ffi::bpp_shard_result> = (0..n_groups).map(|_| unsafe { core::mem::zeroed() }).collect();
        let rc = unsafe { ffi::bpp_verify_sharded_groups(comm.raw, self.ctx, batch, n_groups, counts.as_ptr(), res.as_mut_ptr()) };
        unsafe { ffi::bpp_batch_destroy(self.ctx, batch) };
        map_rc(rc, unsafe { CStr::from_ptr(ffi::bpp_comm_last_error(comm.raw)) }.to_string_lossy().into_owned())?;
        Ok(res.iter().map(|r| {
            let msg = unsafe { CStr::from_ptr(r.msg.as_ptr()) }.to_string_lossy().into_owned();
            map_rc(r.code, msg).map_err(|e| ShardError { error: e, tier: r.tier, rank: r.rank })
        }).collect())
    }

    /// k grouped inputs as ONE pipelined call (bpp_verify_sharded_groups_wave): `inputs[i]` is uploaded to `engines[i]` (distinct
    /// contexts of the communicator's device; `self` is not used beyond being one of them) and the k batches advance as a
    /// software pipeline of this one thread -- one batch's weight chains and exchanges under the other batches' kernels, every
    /// rank issuing its collectives in the same order.  Result: per input, per group, as `verify_sharded_groups`.
    pub fn verify_sharded_groups_wave(comm: &ShardComm, engines: &[&Engine], params: &[&Params], inputs: &[PackedBatch<'_>], n_groups: usize,
                                      counts: &[u32]) -> Result<Vec<Vec<Result<(), ShardError>>>, GpuError> {
        let k = inputs.len();
        assert!(k > 0 && engines.len() == k && params.len() == k);
        let mut err = [0 as core::ffi::c_char; 256];
        let mut batches = vec![0u64; k];
        let ctxs: Vec<*mut ffi::bpp_ctx> = engines.iter().map(|e| e.ctx).collect();
        let release = |upto: usize, batches: &[u64]| for i in 0..upto { unsafe { ffi::bpp_batch_destroy(ctxs[i], batches[i]) }; };
        for i in 0..k {
            let raw = inputs[i].raw();
            let up = unsafe { ffi::bpp_batch_upload_packed(ctxs[i], params[i].handle, &raw, &mut batches[i], err.as_mut_ptr(), err.len()) };
            if let Err(e) = map_rc(up, unsafe { CStr::from_ptr(err.as_ptr()) }.to_string_lossy().into_owned()) {
                release(i, &batches);
                return Err(e);  // rank-local: see verify_sharded
            }
        }
        let mut res: Vec<ffi::bpp_shard_result> = (0..k * n_groups).map(|_| unsafe { core::mem::zeroed() }).collect();
        let rc = unsafe { ffi::bpp_verify_sharded_groups_wave(comm.raw, ctxs.as_ptr(), batches.as_ptr(), k, n_groups, counts.as_ptr(), res.as_mut_ptr()) };
        release(k, &batches);
        map_rc(rc, unsafe { CStr::from_ptr(ffi::bpp_comm_last_error(comm.raw)) }.to_string_lossy().into_owned())?;
        Ok(res.chunks(n_groups).map(|part| part.iter().map(|r| {
            let msg = unsafe { CStr::from_ptr(r.msg.as_ptr()) }.to_string_lossy().into_owned();
            map_rc(r.code, msg).map_err(|e| ShardError { error: e, tier: r.tier, rank: r.rank })
        }).collect()).collect())
    }

    /// `RangeProof::verify` with PASS 1 (src/range_proof.rs:811-850) done by the CALLER on its own merlin transcripts
    /// (bpp_verify_batch_with_challenges, SURVEY 8b option (i)): `challenges[i]` = proof i's y, z, e_0.., e_final as
    /// (rounds_i + 3) x 32 canonical bytes (:833-842), `rng_out` = n x 32 bytes drawn from each `to_verifier_rng` (:845-848).
    /// Everything else of verify() runs on the engine; the transcript fields of `items` are ignored.
    pub fn verify_batch_with_challenges(&self, params: &Params, items: &[VerifyItem<'_>], challenges: &[Vec<u8>], rng_out: &[u8],
                                        action: Action, chunk: usize) -> Result<Vec<Option<Vec<[u8; 32]>>>, GpuError> {
        assert!(challenges.len() == items.len() && rng_out.len() == 32 * items.len());
        let t = params.extension_degree;
        let present_in: Vec<Vec<u8>> = items.iter().map(|i| i.min_values.iter().map(|v| v.is_some() as u8).collect()).collect();
        let mins: Vec<Vec<u64>> = items.iter().map(|i| i.min_values.iter().map(|v| v.unwrap_or(0)).collect()).collect();
        let raw: Vec<ffi::bpp_verify_item> = items.iter().enumerate().map(|(k, i)| ffi::bpp_verify_item {
            proof: i.proof.as_ptr(),
            proof_len: i.proof.len(),
            commitments32: i.commitments.as_ptr(),
            m: (i.commitments.len() / 32) as u32,
            min_values: mins[k].as_ptr(),
            min_present: present_in[k].as_ptr(),
            seed_nonce32: i.seed_nonce.map_or(ptr::null(), |s| s.as_ptr()),
            transcript_state: ptr::null(),
            transcript_label: ptr::null(),
            label_len: 0,
        }).collect();
        let chal_ptrs: Vec<*const u8> = challenges.iter().map(|c| c.as_ptr()).collect();
        let mut masks = vec![0u8; items.len() * t * 32];
        let mut present = vec![0u8; items.len()];
        let mut err = [0 as core::ffi::c_char; 256];
        let rc = unsafe {
            ffi::bpp_verify_batch_with_challenges(self.ctx, params.handle, raw.as_ptr(), raw.len(), chal_ptrs.as_ptr(), rng_out.as_ptr(),
                                                  action as c_int, chunk, masks.as_mut_ptr(), present.as_mut_ptr(), err.as_mut_ptr(), err.len())
        };
        let out = map_rc(rc, unsafe { CStr::from_ptr(err.as_ptr()) }.to_string_lossy().into_owned()).map(|_| unpack_masks(&masks, &present, t));
        masks.iter_mut().for_each(|b| *b = 0); // recovered masks are secrets (src/extended_mask.rs:14)
        out
    }

    // ---- seam B1: the three dalek multiscalar traits the reference is generic over (src/traits.rs:40-43, src/ristretto.rs:28-64);
    // rust/bpp-gpu-ristretto implements them for a point type of its own on top of these three calls

    /// `VartimePrecomputedMultiscalarMul::new(static_points)` (src/generators/bulletproof_gens.rs:103): `points` = count x 32 bytes
    pub fn precomp(&self, points: &[u8]) -> Result<Precomp, GpuError> {
        assert!(points.len() % 32 == 0);
        let mut handle = 0u64;
        map_rc(unsafe { ffi::bpp_precomp_create(self.ctx, points.as_ptr(), points.len() / 32, &mut handle) }, self.last_error())?;
        Ok(Precomp { handle, count: points.len() / 32, owner: self.ctx })
    }

    /// `vartime_mixed_multiscalar_mul(static_scalars, dynamic_scalars, dynamic_points)` (src/range_proof.rs:339-345, :1050-1057):
    /// scalars 32 canonical bytes each, points 32-byte ristretto255 encodings; static_scalars.len() / 32 <= table size
    pub fn msm_mixed(&self, table: &Precomp, static_scalars: &[u8], dyn_scalars: &[u8], dyn_points: &[u8]) -> Result<[u8; 32], GpuError> {
        assert!(static_scalars.len() % 32 == 0 && dyn_scalars.len() == dyn_points.len() && dyn_scalars.len() % 32 == 0);
        let mut out = [0u8; 32];
        let rc = unsafe {
            ffi::bpp_msm_mixed(self.ctx, table.handle, static_scalars.as_ptr(), static_scalars.len() / 32, dyn_scalars.as_ptr(),
                               dyn_points.as_ptr(), dyn_scalars.len() / 32, out.as_mut_ptr())
        };
        map_rc(rc, self.last_error())?;
        Ok(out)
    }

    /// `VartimeMultiscalarMul::vartime_multiscalar_mul` / `MultiscalarMul::multiscalar_mul` (src/range_proof.rs:482-495, :512-521,
    /// src/generators/pedersen_gens.rs:120)
    pub fn msm_vartime(&self, scalars: &[u8], points: &[u8]) -> Result<[u8; 32], GpuError> {
        assert!(scalars.len() == points.len() && scalars.len() % 32 == 0);
        let mut out = [0u8; 32];
        map_rc(unsafe { ffi::bpp_msm_vartime(self.ctx, scalars.as_ptr(), points.as_ptr(), scalars.len() / 32, out.as_mut_ptr()) }, self.last_error())?;
        Ok(out)
    }

    /// what the library sees of its runtime preconditions: hardware queues (GPU_MAX_HW_QUEUES as the HIP runtime read it), live
    /// contexts, the small-call gate ("Runtime preconditions")
    pub fn runtime_info(&self) -> ffi::bpp_runtime_info {
        let mut info = ffi::bpp_runtime_info::default();
        unsafe { ffi::bpp_runtime_info_get(self.ctx, &mut info) };
        info
    }

    /// what the prover's self-check ("prove_check" = 1, `bpp_ctx_set_option` or BPP_PROVE_CHECK) of this context has done
    pub fn prove_check_stats(&self) -> Result<ffi::bpp_prove_check_stats, GpuError> {
        let mut s = ffi::bpp_prove_check_stats::default();
        map_rc(unsafe { ffi::bpp_prove_check_stats(self.ctx, &mut s) }, String::from("bpp_prove_check_stats"))?;
        Ok(s)
    }

    /// "prove_check_recovery" = 1 (with "prove_check" = 1): (proofs with a seed nonce whose mask recovery the self-check replayed,
    /// those whose recovered masks were not the witness's blinding factors)
    pub fn prove_check_recovery_stats(&self) -> Result<(u64, u64), GpuError> {
        let (mut replayed, mut mismatched) = (0u64, 0u64);
        map_rc(unsafe { ffi::bpp_prove_check_recovery_stats(self.ctx, &mut replayed, &mut mismatched) },
               String::from("bpp_prove_check_recovery_stats"))?;
        Ok((replayed, mismatched))
    }

    /// `RangeProof::verify_batch`: every `chunk` consecutive items are one reference batch (256 = MAX_RANGE_PROOF_BATCH_SIZE,
    /// 0 = the whole input).  Returns per item `Some(mask blindings, t x 32 bytes)` or `None`.
    pub fn verify_batch(&self, params: &Params, items: &[VerifyItem<'_>], action: Action, chunk: usize)
                        -> Result<Vec<Option<Vec<[u8; 32]>>>, GpuError> {
        let t = params.extension_degree;
        let present_in: Vec<Vec<u8>> = items.iter().map(|i| i.min_values.iter().map(|v| v.is_some() as u8).collect()).collect();
        let mins: Vec<Vec<u64>> = items.iter().map(|i| i.min_values.iter().map(|v| v.unwrap_or(0)).collect()).collect();
        let raw: Vec<ffi::bpp_verify_item> = items.iter().enumerate().map(|(k, i)| ffi::bpp_verify_item {
            proof: i.proof.as_ptr(),
            proof_len: i.proof.len(),
            commitments32: i.commitments.as_ptr(),
            m: (i.commitments.len() / 32) as u32,
            min_values: mins[k].as_ptr(),
            min_present: present_in[k].as_ptr(),
            seed_nonce32: i.seed_nonce.map_or(ptr::null(), |s| s.as_ptr()),
            transcript_state: i.transcript_state.map_or(ptr::null(), |s| s.as_ptr()),
            transcript_label: i.transcript_label.as_ptr(),
            label_len: i.transcript_label.len(),
        }).collect();
        let mut masks = vec![0u8; items.len() * t * 32];
        let mut present = vec![0u8; items.len()];
        let mut err = [0 as core::ffi::c_char; 256];
        let rc = unsafe {
            ffi::bpp_verify_batch(self.ctx, params.handle, raw.as_ptr(), raw.len(), action as c_int, chunk, masks.as_mut_ptr(),
                                  present.as_mut_ptr(), err.as_mut_ptr(), err.len())
        };
        map_rc(rc, unsafe { CStr::from_ptr(err.as_ptr()) }.to_string_lossy().into_owned())?;
        Ok((0..items.len()).map(|k| if present[k] != 0 {
            Some((0..t).map(|j| { let mut b = [0u8; 32]; b.copy_from_slice(&masks[(k * t + j) * 32..(k * t + j + 1) * 32]); b }).collect())
        } else { None }).collect())
    }

    /// n x `RangeProof::prove_with_rng` in one call; all items share the aggregation factor.  Returns `to_bytes()` of each proof.
    pub fn prove_batch(&self, params: &Params, items: &[ProveItem<'_>]) -> Result<Vec<Vec<u8>>, GpuError> {
        let keep = RawProveItems::new(items);
        let raw = &keep.raw;
        let stride = 1 + 32 * (6 + 5 + 2 * 12);
        let mut out = vec![0u8; stride * items.len()];
        let mut plen = 0usize;
        let mut err = [0 as core::ffi::c_char; 256];
        let rc = unsafe {
            ffi::bpp_prove_batch(self.ctx, params.handle, raw.as_ptr(), raw.len(), out.as_mut_ptr(), stride, &mut plen, err.as_mut_ptr(), err.len())
        };
        map_rc(rc, unsafe { CStr::from_ptr(err.as_ptr()) }.to_string_lossy().into_owned())?;
        Ok((0..items.len()).map(|k| out[k * stride..k * stride + plen].to_vec()).collect())
    }

    /// n x `RangeProof::prove_with_rng` of any aggregation factors (powers of two up to the parameters' maximum) in one call
    /// (bpp_prove_batch_mixed).  One entry per item: its `to_bytes()`, or the error `prove_batch` on that item alone returns, or
    /// (self-check on) `GpuError::Engine(ffi::BPP_ERR_SELF_CHECK, ..)` for a proof the verifier rejected twice.
    pub fn prove_batch_mixed(&self, params: &Params, items: &[ProveItem<'_>]) -> Result<Vec<Result<Vec<u8>, GpuError>>, GpuError> {
        let keep = RawProveItems::new(items);
        let stride = 1 + 32 * (6 + 5 + 2 * 12);
        let mut out = vec![0u8; stride * items.len()];
        let mut lens = vec![0usize; items.len()];
        let mut status = vec![0 as c_int; items.len()];
        let mut err = [0 as core::ffi::c_char; 256];
        let rc = unsafe {
            ffi::bpp_prove_batch_mixed(self.ctx, params.handle, keep.raw.as_ptr(), keep.raw.len(), out.as_mut_ptr(), stride, lens.as_mut_ptr(),
                                       status.as_mut_ptr(), err.as_mut_ptr(), err.len())
        };
        if rc < 0 && rc != ffi::BPP_ERR_SELF_CHECK {  // (an engine fault of the call; a self-check failure is an item's own outcome)
            map_rc(rc, unsafe { CStr::from_ptr(err.as_ptr()) }.to_string_lossy().into_owned())?;
        }
        Ok((0..items.len()).map(|k| {
            if status[k] == 0 {
                return Ok(out[k * stride..k * stride + lens[k]].to_vec());
            }
            // the failed item's own message (host-side work only)
            let mut e1 = [0 as core::ffi::c_char; 256];
            unsafe { ffi::bpp_prove_item_message(self.ctx, params.handle, &keep.raw[k], stride, status[k], e1.as_mut_ptr(), e1.len()) };
            map_rc(status[k], unsafe { CStr::from_ptr(e1.as_ptr()) }.to_string_lossy().into_owned()).map(|_| Vec::new())
        }).collect())
    }

    /// Prove from the openings alone (bpp_prove_openings): `prove_batch_mixed` whose items may come with an EMPTY `commitments`
    /// slice; the engine then makes commit(v_j, r_j) for every opening of that item -- in the same call, where the prover's witness
    /// check computes them anyway -- and proves over them.  One entry per item: (its m x 32 commitment bytes, made or brought, its
    /// `to_bytes()`), or the item's error.
    #[allow(clippy::type_complexity)]
    pub fn prove_openings(&self, params: &Params, items: &[ProveItem<'_>]) -> Result<Vec<Result<(Vec<u8>, Vec<u8>), GpuError>>, GpuError> {
        let keep = RawProveItems::new_openings(items);
        let stride = 1 + 32 * (6 + 5 + 2 * 12);
        let cstride = 32 * items.iter().map(|i| i.values.len()).max().unwrap_or(1);
        let mut out = vec![0u8; stride * items.len()];
        let mut comms = vec![0u8; cstride * items.len()];
        let mut lens = vec![0usize; items.len()];
        let mut status = vec![0 as c_int; items.len()];
        let mut err = [0 as core::ffi::c_char; 256];
        let rc = unsafe {
            ffi::bpp_prove_openings(self.ctx, params.handle, keep.raw.as_ptr(), keep.raw.len(), comms.as_mut_ptr(), cstride, out.as_mut_ptr(),
                                    stride, lens.as_mut_ptr(), status.as_mut_ptr(), err.as_mut_ptr(), err.len())
        };
        if rc < 0 && rc != ffi::BPP_ERR_SELF_CHECK {
            map_rc(rc, unsafe { CStr::from_ptr(err.as_ptr()) }.to_string_lossy().into_owned())?;
        }
        Ok((0..items.len()).map(|k| {
            if status[k] == 0 {
                return Ok((comms[k * cstride..k * cstride + 32 * items[k].values.len()].to_vec(), out[k * stride..k * stride + lens[k]].to_vec()));
            }
            // (first_commitment32 = NULL: a self-check failure's text names the verifier's rejection unless the item brought its own)
            let mut e1 = [0 as core::ffi::c_char; 256];
            unsafe {
                ffi::bpp_prove_openings_item_message(self.ctx, params.handle, &keep.raw[k], ptr::null(), cstride, stride, status[k], e1.as_mut_ptr(),
                                                     e1.len())
            };
            map_rc(status[k], unsafe { CStr::from_ptr(e1.as_ptr()) }.to_string_lossy().into_owned()).map(|_| (Vec::new(), Vec::new()))
        }).collect())
    }

    /// lanes of the prove pipeline (1..8, default 3); only before the first `prove_submit` of this engine
    pub fn prove_pipeline_depth(&self, depth: u32) -> Result<(), GpuError> {
        map_rc(unsafe { ffi::bpp_prove_pipeline_depth(self.ctx, depth) }, self.last_error())
    }

    /// A whole prove call handed to a lane of this engine (bpp_prove_submit): returns at once with a ticket, and `items` -- and
    /// everything they borrow -- are free again then (the engine has checked every item and keeps its own copy of the ones that
    /// pass, wiped as soon as the lane's call has returned).  `openings`: the ticket is a `prove_openings` call (an item may come
    /// with an empty `commitments` slice), else a `prove_batch_mixed` call.  Several tickets may be outstanding: with as many as
    /// lanes, one thread keeps the device as busy as several threads with an engine each.
    pub fn prove_submit(&self, params: &Params, items: &[ProveItem<'_>], openings: bool) -> Result<ProveTicket, GpuError> {
        let keep = if openings { RawProveItems::new_openings(items) } else { RawProveItems::new(items) };
        let stride = 1 + 32 * (6 + 5 + 2 * 12);
        let cstride = if openings { 32 * items.iter().map(|i| i.values.len()).max().unwrap_or(1) } else { 0 };
        let mut id = 0u64;
        let mut err = [0 as core::ffi::c_char; 256];
        let rc = unsafe {
            ffi::bpp_prove_submit(self.ctx, params.handle, keep.raw.as_ptr(), keep.raw.len(), stride, openings as c_int, cstride, &mut id,
                                  err.as_mut_ptr(), err.len())
        };
        map_rc(rc, unsafe { CStr::from_ptr(err.as_ptr()) }.to_string_lossy().into_owned())?;
        Ok(ProveTicket { id, openings, stride, cstride, m: items.iter().map(|i| i.values.len()).collect() })
    }

    /// true once `prove_collect` on this ticket would not wait; never blocks
    pub fn prove_ticket_done(&self, ticket: &ProveTicket) -> Result<bool, GpuError> {
        let mut done: c_int = 0;
        map_rc(unsafe { ffi::bpp_prove_ticket_done(self.ctx, ticket.id, &mut done) }, String::from("unknown ticket"))?;
        Ok(done != 0)
    }

    /// Blocks until the ticket's call is done (bpp_prove_collect) and returns what `prove_openings` / `prove_batch_mixed` over the
    /// same items return: per item (its m x 32 commitment bytes -- empty for a ticket without `openings` --, its `to_bytes()`), or
    /// the item's error.  The items are gone by now, so only the call's first failing item carries its message; the others carry
    /// their code.  Any order, any thread.
    #[allow(clippy::type_complexity)]
    pub fn prove_collect(&self, ticket: ProveTicket) -> Result<Vec<Result<(Vec<u8>, Vec<u8>), GpuError>>, GpuError> {
        let n = ticket.m.len();
        let (stride, cstride) = (ticket.stride, ticket.cstride);
        let mut out = vec![0u8; stride * n];
        let mut comms = vec![0u8; cstride * n];
        let mut lens = vec![0usize; n];
        let mut status = vec![0 as c_int; n];
        let mut err = [0 as core::ffi::c_char; 256];
        let rc = unsafe {
            ffi::bpp_prove_collect(self.ctx, ticket.id, if ticket.openings { comms.as_mut_ptr() } else { ptr::null_mut() }, out.as_mut_ptr(),
                                   lens.as_mut_ptr(), status.as_mut_ptr(), err.as_mut_ptr(), err.len())
        };
        let msg = unsafe { CStr::from_ptr(err.as_ptr()) }.to_string_lossy().into_owned();
        if rc != 0 && status.iter().all(|&s| s == 0) {  // (a finding of the call itself: an unknown ticket, an engine fault)
            map_rc(rc, msg.clone())?;
        }
        let first = status.iter().position(|&s| s != 0);
        Ok((0..n).map(|k| {
            if status[k] == 0 {
                let c = if ticket.openings { comms[k * cstride..k * cstride + 32 * ticket.m[k]].to_vec() } else { Vec::new() };
                return Ok((c, out[k * stride..k * stride + lens[k]].to_vec()));
            }
            map_rc(status[k], if Some(k) == first { msg.clone() } else { String::new() }).map(|_| (Vec::new(), Vec::new()))
        }).collect())
    }

    /// Arc::clone of a parameter set created on another context of the same device
    pub fn retain(&self, params: &Params) -> Result<Params, GpuError> {
        map_rc(unsafe { ffi::bpp_params_retain(self.ctx, params.handle) }, self.last_error())?;
        Ok(Params { handle: params.handle, extension_degree: params.extension_degree, owner: self.ctx })
    }
}

fn unpack_masks(masks: &[u8], present: &[u8], t: usize) -> Vec<Option<Vec<[u8; 32]>>> {
    (0..present.len()).map(|k| if present[k] != 0 {
        Some((0..t).map(|j| { let mut b = [0u8; 32]; b.copy_from_slice(&masks[(k * t + j) * 32..(k * t + j + 1) * 32]); b }).collect())
    } else { None }).collect()
}

impl Drop for Engine {
    fn drop(&mut self) {
        unsafe { ffi::bpp_ctx_destroy(self.ctx) }
    }
}

/// Device-resident generator tables of one `RangeParameters` (src/range_parameters.rs:20-30): process-wide, shared.
/// Dropping it drops this holder's reference (bpp_params_destroy = Arc drop) -- on every path, including `?` returns.
pub struct Params {
    handle: u64,
    extension_degree: usize,
    owner: *mut ffi::bpp_ctx, // the context that holds this reference (must outlive it: the cache below lives for the process)
}
unsafe impl Send for Params {}
unsafe impl Sync for Params {}
impl Params {
    pub fn extension_degree(&self) -> usize {
        self.extension_degree
    }
    /// the library's handle of this parameter set (a key for per-parameter caches such as a process-wide prove pool)
    pub fn handle(&self) -> u64 {
        self.handle
    }
}
impl Drop for Params {
    fn drop(&mut self) {
        unsafe { ffi::bpp_params_destroy(self.owner, self.handle) };
    }
}

/// A precomputed generator table on the device (bpp_precomp_*): `Precomputation: Send + Sync`, shared through Arc by the
/// reference (src/traits.rs:42, src/generators/bulletproof_gens.rs:52).  Dropping it drops this holder's reference.
pub struct Precomp {
    handle: u64,
    count: usize,
    owner: *mut ffi::bpp_ctx, // the context that holds this reference (must outlive it)
}
unsafe impl Send for Precomp {}
unsafe impl Sync for Precomp {}
impl Precomp {
    pub fn len(&self) -> usize {
        self.count
    }
    pub fn is_empty(&self) -> bool {
        self.count == 0
    }
}
impl Drop for Precomp {
    fn drop(&mut self) {
        unsafe { ffi::bpp_precomp_destroy(self.owner, self.handle) };
    }
}

/// key of the process-wide parameter cache: (bit length, max aggregation, extension degree, H, G bases)
type ParamsKey = (usize, usize, usize, [u8; 32], Vec<u8>);

/// `RangeParameters` -> device tables, created ONCE per parameter set and process (the reference shares its generators
/// through Arc: src/range_parameters.rs:20-30): bpp_params_create derives every generator and builds the tables, which
/// must not happen per verify call, and a handle created per call would leak on every early return.
pub fn cached_params(bit_length: usize, max_aggregation: usize, extension_degree: usize, h_base: &[u8; 32], g_bases: &[u8])
                     -> Result<Arc<Params>, GpuError> {
    static CACHE: OnceLock<Mutex<HashMap<ParamsKey, Arc<Params>>>> = OnceLock::new();
    let key: ParamsKey = (bit_length, max_aggregation, extension_degree, *h_base, g_bases.to_vec());
    let mut cache = CACHE.get_or_init(|| Mutex::new(HashMap::new())).lock().unwrap();
    if let Some(p) = cache.get(&key) {
        return Ok(p.clone());
    }
    let p = Arc::new(default_engine().lock().unwrap().params(bit_length, max_aggregation, extension_degree, Some(h_base), Some(g_bases))?);
    cache.insert(key, p.clone());
    Ok(p)
}

/// A homogeneous batch as contiguous arrays (bpp_packed_batch)
pub struct PackedBatch<'a> {
    pub n_items: usize,
    /// n_items proofs of `proof_len` bytes each, back to back
    pub proofs: &'a [u8],
    pub proof_len: usize,
    /// n_items x m x 32
    pub commitments: &'a [u8],
    pub m: usize,
    /// n_items x m
    pub min_values: &'a [u64],
    pub min_present: &'a [u8],
    /// n_items x 32 + n_items presence flags, or None
    pub seed_nonces: Option<(&'a [u8], &'a [u8])>,
    /// the label of the callers' fresh `Transcript::new(label)` ...
    pub transcript_label: &'a [u8],
    /// ... or the 203-byte STROBE state all their transcripts are in
    pub transcript_state: Option<&'a [u8; 203]>,
}
impl PackedBatch<'_> {
    fn raw(&self) -> ffi::bpp_packed_batch {
        assert!(self.proofs.len() == self.n_items * self.proof_len && self.commitments.len() == self.n_items * self.m * 32);
        assert!(self.min_values.len() == self.n_items * self.m && self.min_present.len() == self.n_items * self.m);
        ffi::bpp_packed_batch {
            n_items: self.n_items,
            proofs: self.proofs.as_ptr(),
            proof_len: self.proof_len,
            proof_stride: self.proof_len,
            commitments32: self.commitments.as_ptr(),
            m: self.m as u32,
            min_values: self.min_values.as_ptr(),
            min_present: self.min_present.as_ptr(),
            seed_nonces32: self.seed_nonces.map_or(ptr::null(), |s| s.0.as_ptr()),
            seed_present: self.seed_nonces.map_or(ptr::null(), |s| s.1.as_ptr()),
            transcript_state: self.transcript_state.map_or(ptr::null(), |s| s.as_ptr()),
            transcript_label: self.transcript_label.as_ptr(),
            label_len: self.transcript_label.len(),
        }
    }
}

pub struct Ticket {
    id: u64,
    n_items: usize,
    t: usize,
}

/// One RCCL communicator for sharded verification (bpp_comm).  `unique_id` on rank 0, shipped to the other ranks by the
/// caller's own channel, then `create` on every rank (collective).
pub struct ShardComm {
    raw: *mut ffi::bpp_comm,
    pub rank: i32,
    /// the caller's transport, kept alive (and at a fixed address) as long as the communicator (`with_transport`)
    #[allow(dead_code)]
    transport: Option<Box<Transport>>,
}
unsafe impl Send for ShardComm {}

/// A caller-supplied all_gather: `send` = this rank's block, `recv` = `world` blocks in rank order (this rank's included);
/// `Err` = the exchange failed (the verify call then returns `GpuError::Comm` and the communicator is dead).
pub type AllGather = dyn FnMut(&[u8], &mut [u8]) -> Result<(), ()> + Send;
struct Transport {
    f: Box<AllGather>,
    world: usize,
}
unsafe extern "C" fn transport_trampoline(user: *mut std::os::raw::c_void, send: *const std::os::raw::c_void, recv: *mut std::os::raw::c_void,
                                          bytes_per_rank: usize) -> std::os::raw::c_int {
    // (a panic must not unwind into C)
    let r = std::panic::catch_unwind(std::panic::AssertUnwindSafe(|| {
        let t = &mut *(user as *mut Transport);
        let s = std::slice::from_raw_parts(send as *const u8, bytes_per_rank);
        let d = std::slice::from_raw_parts_mut(recv as *mut u8, bytes_per_rank * t.world);
        (t.f)(s, d)
    }));
    match r {
        Ok(Ok(())) => 0,
        Ok(Err(())) => 1,
        Err(_) => 2,
    }
}

impl ShardComm {
    /// `bpp_comm_create_callbacks`: the sharded entry points over the caller's own channel (MPI, TCP, ...) instead of RCCL --
    /// the exchanges are 32 bytes per proof and 256 bytes per batch, staged through host memory by the engine.  `all_gather` is
    /// called on the thread that makes the verify call, in the same order on every rank.
    pub fn with_transport(engine: &Engine, rank: i32, world: i32, all_gather: Box<AllGather>) -> Result<Self, GpuError> {
        let mut t = Box::new(Transport { f: all_gather, world: world as usize });
        let mut raw = ptr::null_mut();
        map_rc(unsafe {
            ffi::bpp_comm_create_callbacks(engine.ctx, rank, world, Some(transport_trampoline), &mut *t as *mut Transport as *mut std::os::raw::c_void, &mut raw)
        }, engine.last_error())?;
        Ok(ShardComm { raw, rank, transport: Some(t) })
    }
    pub fn unique_id() -> Result<[u8; 128], GpuError> {
        let mut id = [0u8; 128];
        map_rc(unsafe { ffi::bpp_comm_unique_id(id.as_mut_ptr()) }, "RCCL not loadable".into())?;
        Ok(id)
    }
    pub fn create(engine: &Engine, id: &[u8; 128], rank: i32, world: i32) -> Result<Self, GpuError> {
        let mut raw = ptr::null_mut();
        map_rc(unsafe { ffi::bpp_comm_create(engine.ctx, id.as_ptr(), rank, world, &mut raw) }, engine.last_error())?;
        Ok(ShardComm { raw, rank, transport: None })
    }
}
impl Drop for ShardComm {
    fn drop(&mut self) {
        unsafe { ffi::bpp_comm_destroy(self.raw) }  // (before `transport` goes: no call can be inside the callback any more)
    }
}

/// a sharded verification's error: the same on every rank; `tier` = where in the reference's order of checks
/// (ffi::BPP_TIER_*), `rank` = whose proofs (-1: the final check over all of them)
#[derive(Debug)]
pub struct ShardError {
    pub error: GpuError,
    pub tier: i32,
    pub rank: i32,
}

pub struct VerifyItem<'a> {
    pub proof: &'a [u8],
    /// m x 32 bytes: statement.commitments_compressed
    pub commitments: &'a [u8],
    pub min_values: &'a [Option<u64>],
    pub seed_nonce: Option<&'a [u8; 32]>,
    /// a fresh `Transcript::new(label)` ...
    pub transcript_label: &'a [u8],
    /// ... or the 203-byte STROBE state of an arbitrary transcript
    pub transcript_state: Option<&'a [u8; 203]>,
}

pub struct ProveItem<'a> {
    pub values: &'a [u64],
    /// m x t x 32 bytes
    pub blindings: &'a [u8],
    pub commitments: &'a [u8],
    pub min_values: &'a [Option<u64>],
    pub seed_nonce: Option<&'a [u8; 32]>,
    pub transcript_label: &'a [u8],
    pub transcript_state: Option<&'a [u8; 203]>,
    /// (rounds + 3) x 32 bytes drawn from the caller's `CryptoRngCore`, in order (what `TranscriptRngBuilder::finalize` pulls)
    pub rng_bytes: &'a [u8],
}

/// Process-wide default engine on device 0 for the in-crate patch (one context; callers that want concurrency hold their own).
pub fn default_engine() -> &'static Mutex<Engine> {
    static ENGINE: OnceLock<Mutex<Engine>> = OnceLock::new();
    ENGINE.get_or_init(|| Mutex::new(Engine::new(0).expect("bpp-gpu-shim: no usable gfx950 device")))
}

/// `bpp_batcher`: many threads, each with one reference batch per call; the library pools the calls that are waiting into
/// grouped engine calls (a small call alone is a chain of latency-bound kernels: separate 256-proof calls stop at about 5 000
/// per second whatever the number of callers).  `verify` / `verify_action` block and return what
/// `Engine::verify_batch_packed(.., action, 0)` would for that input alone.  Shareable between threads (`&self`).
pub struct Batcher {
    raw: *mut ffi::bpp_batcher,
    _engine: Option<Engine>,  // the context of the first lane, when the batcher owns it (dropped after the batcher itself)
}
unsafe impl Send for Batcher {}
unsafe impl Sync for Batcher {}

impl Batcher {
    /// every shape and every VerifyAction pools (round 4: the `shape` argument of bpp_batcher_create is no longer needed)
    pub fn new(engine: &Engine, params: &Params, lanes: u32, max_wait_us: u32, max_calls: u32) -> Result<Batcher, GpuError> {
        let mut raw = core::ptr::null_mut();
        let rc = unsafe { ffi::bpp_batcher_create(engine.ctx, params.handle, core::ptr::null(), lanes, max_wait_us, max_calls, &mut raw) };
        map_rc(rc, String::from("bpp_batcher_create"))?;
        Ok(Batcher { raw, _engine: None })
    }
    /// the same, taking ownership of `engine` (a context that exists for this batcher only); `params` is retained on it first
    pub fn new_owning(engine: Engine, params: &Params, lanes: u32, max_wait_us: u32, max_calls: u32) -> Result<Batcher, GpuError> {
        map_rc(unsafe { ffi::bpp_params_retain(engine.ctx, params.handle) }, String::from("bpp_params_retain"))?;
        let mut b = Batcher::new(&engine, params, lanes, max_wait_us, max_calls)?;
        b._engine = Some(engine);
        Ok(b)
    }
    /// any VerifyAction through the pool (bpp_batcher_verify_action): what `Engine::verify_batch_packed(.., action, 0)` returns for
    /// this input alone -- its own seed nonces in (`input.seed_nonces`), its own masks out; `t` = the parameters' extension degree
    pub fn verify_action(&self, input: &PackedBatch<'_>, action: Action, t: usize) -> Result<Vec<Option<Vec<[u8; 32]>>>, GpuError> {
        let raw_in = input.raw();
        let mut masks = vec![0u8; input.n_items * t * 32];
        let mut present = vec![0u8; input.n_items];
        let mut err = [0 as core::ffi::c_char; 256];
        let rc = unsafe {
            ffi::bpp_batcher_verify_action(self.raw, &raw_in, action as c_int, masks.as_mut_ptr(), present.as_mut_ptr(), err.as_mut_ptr(), err.len())
        };
        let out = map_rc(rc, unsafe { CStr::from_ptr(err.as_ptr()) }.to_string_lossy().into_owned()).map(|_| unpack_masks(&masks, &present, t));
        masks.iter_mut().for_each(|b| *b = 0); // recovered masks are secrets (src/extended_mask.rs:14)
        out
    }
    pub fn verify(&self, input: &PackedBatch<'_>) -> Result<(), GpuError> {
        let raw_in = input.raw();
        let mut err = [0 as core::ffi::c_char; 256];
        let rc = unsafe { ffi::bpp_batcher_verify(self.raw, &raw_in, err.as_mut_ptr(), err.len()) };
        map_rc(rc, unsafe { CStr::from_ptr(err.as_ptr()) }.to_string_lossy().into_owned())
    }
}

/// a prove call in flight (`Engine::prove_submit`); collect it on the engine that issued it
pub struct ProveTicket {
    id: u64,
    openings: bool,
    stride: usize,
    cstride: usize,
    m: Vec<usize>,  // per item: its aggregation factor
}

/// `bpp_prove_item`s of borrowed `ProveItem`s, with the promise arrays they point into
struct RawProveItems {
    raw: Vec<ffi::bpp_prove_item>,
    _mins: Vec<Vec<u64>>,
    _present: Vec<Vec<u8>>,
}
impl RawProveItems {
    fn new(items: &[ProveItem<'_>]) -> RawProveItems {
        RawProveItems::build(items, false)
    }
    /// for bpp_prove_openings / bpp_prove_pool_openings: an empty `commitments` slice becomes NULL ("to be made")
    fn new_openings(items: &[ProveItem<'_>]) -> RawProveItems {
        RawProveItems::build(items, true)
    }
    fn build(items: &[ProveItem<'_>], openings: bool) -> RawProveItems {
        let present: Vec<Vec<u8>> = items.iter().map(|i| i.min_values.iter().map(|v| v.is_some() as u8).collect()).collect();
        let mins: Vec<Vec<u64>> = items.iter().map(|i| i.min_values.iter().map(|v| v.unwrap_or(0)).collect()).collect();
        let raw = items.iter().enumerate().map(|(k, i)| ffi::bpp_prove_item {
            values: i.values.as_ptr(),
            blindings32: i.blindings.as_ptr(),
            commitments32: if openings && i.commitments.is_empty() { ptr::null() } else { i.commitments.as_ptr() },
            m: i.values.len() as u32,
            min_values: mins[k].as_ptr(),
            min_present: present[k].as_ptr(),
            seed_nonce32: i.seed_nonce.map_or(ptr::null(), |s| s.as_ptr()),
            transcript_state: i.transcript_state.map_or(ptr::null(), |s| s.as_ptr()),
            transcript_label: i.transcript_label.as_ptr(),
            label_len: i.transcript_label.len(),
            rng_bytes: i.rng_bytes.as_ptr(),
            rng_len: i.rng_bytes.len(),
        }).collect();
        RawProveItems { raw, _mins: mins, _present: present }
    }
}

/// `bpp_prove_pool`: many threads, each with a few proofs (of any aggregation factors) per call; the library proves the calls
/// that are waiting as ONE mixed-aggregation engine call.  `prove` blocks and returns what `Engine::prove_batch_mixed` on this
/// call's items would, as the call's first error or all of its proofs.  Shareable between threads (`&self`).
pub struct ProvePool {
    raw: *mut ffi::bpp_prove_pool,
    _engine: Option<Engine>,  // the context of the first lane, when the pool owns it (dropped after the pool itself)
}
unsafe impl Send for ProvePool {}
unsafe impl Sync for ProvePool {}

impl ProvePool {
    pub fn new(engine: &Engine, params: &Params, lanes: u32, max_wait_us: u32, max_calls: u32) -> Result<ProvePool, GpuError> {
        let mut raw = core::ptr::null_mut();
        let rc = unsafe { ffi::bpp_prove_pool_create(engine.ctx, params.handle, lanes, max_wait_us, max_calls, &mut raw) };
        map_rc(rc, String::from("bpp_prove_pool_create"))?;
        Ok(ProvePool { raw, _engine: None })
    }
    /// the same, taking ownership of `engine` (a context that exists for this pool only); `params` is retained on it first
    pub fn new_owning(engine: Engine, params: &Params, lanes: u32, max_wait_us: u32, max_calls: u32) -> Result<ProvePool, GpuError> {
        map_rc(unsafe { ffi::bpp_params_retain(engine.ctx, params.handle) }, String::from("bpp_params_retain"))?;
        let mut p = ProvePool::new(&engine, params, lanes, max_wait_us, max_calls)?;
        p._engine = Some(engine);
        Ok(p)
    }
    pub fn prove(&self, items: &[ProveItem<'_>]) -> Result<Vec<Vec<u8>>, GpuError> {
        let keep = RawProveItems::new(items);
        let stride = 1 + 32 * (6 + 5 + 2 * 12);
        let mut out = vec![0u8; stride * items.len()];
        let mut lens = vec![0usize; items.len()];
        let mut err = [0 as core::ffi::c_char; 256];
        let rc = unsafe {
            ffi::bpp_prove_pool_prove(self.raw, keep.raw.as_ptr(), keep.raw.len(), out.as_mut_ptr(), stride, lens.as_mut_ptr(), err.as_mut_ptr(),
                                      err.len())
        };
        map_rc(rc, unsafe { CStr::from_ptr(err.as_ptr()) }.to_string_lossy().into_owned())?;
        Ok((0..items.len()).map(|k| out[k * stride..k * stride + lens[k]].to_vec()).collect())
    }
    /// `Engine::prove_openings` through the pool (bpp_prove_pool_openings): per item (commitment bytes, proof bytes), or the call's
    /// first error.  Calls of this kind and `prove` calls share pooled engine calls.
    pub fn prove_openings(&self, items: &[ProveItem<'_>]) -> Result<Vec<(Vec<u8>, Vec<u8>)>, GpuError> {
        let keep = RawProveItems::new_openings(items);
        let stride = 1 + 32 * (6 + 5 + 2 * 12);
        let cstride = 32 * items.iter().map(|i| i.values.len()).max().unwrap_or(1);
        let mut out = vec![0u8; stride * items.len()];
        let mut comms = vec![0u8; cstride * items.len()];
        let mut lens = vec![0usize; items.len()];
        let mut err = [0 as core::ffi::c_char; 256];
        let rc = unsafe {
            ffi::bpp_prove_pool_openings(self.raw, keep.raw.as_ptr(), keep.raw.len(), comms.as_mut_ptr(), cstride, out.as_mut_ptr(), stride,
                                         lens.as_mut_ptr(), err.as_mut_ptr(), err.len())
        };
        map_rc(rc, unsafe { CStr::from_ptr(err.as_ptr()) }.to_string_lossy().into_owned())?;
        Ok((0..items.len()).map(|k| (comms[k * cstride..k * cstride + 32 * items[k].values.len()].to_vec(),
                                     out[k * stride..k * stride + lens[k]].to_vec())).collect())
    }
    /// (requests of `prove_openings` so far, pooled engine calls that held requests of both kinds)
    pub fn openings_stats(&self) -> (u64, u64) {
        let (mut a, mut b) = (0u64, 0u64);
        unsafe { ffi::bpp_prove_pool_openings_stats(self.raw, &mut a, &mut b) };
        (a, b)
    }
    pub fn set_limits(&self, max_calls: u32, max_proofs: u32) -> Result<(), GpuError> {
        map_rc(unsafe { ffi::bpp_prove_pool_set_limits(self.raw, max_calls, max_proofs) }, String::from("bpp_prove_pool_set_limits"))
    }
    /// the self-check counters of every lane, summed (`Engine::prove_check_stats`; the first lane is the engine the pool was made from)
    pub fn check_stats(&self) -> Result<ffi::bpp_prove_check_stats, GpuError> {
        let mut s = ffi::bpp_prove_check_stats::default();
        map_rc(unsafe { ffi::bpp_prove_pool_check_stats(self.raw, &mut s) }, String::from("bpp_prove_pool_check_stats"))?;
        Ok(s)
    }
    /// `Engine::prove_check_recovery_stats` summed over the lanes: (replayed, mismatched)
    pub fn check_recovery_stats(&self) -> Result<(u64, u64), GpuError> {
        let (mut replayed, mut mismatched) = (0u64, 0u64);
        map_rc(unsafe { ffi::bpp_prove_pool_check_recovery_stats(self.raw, &mut replayed, &mut mismatched) },
               String::from("bpp_prove_pool_check_recovery_stats"))?;
        Ok((replayed, mismatched))
    }
    /// (callers served in pooled calls, engine calls, calls that ran alone, largest pool in calls, in proofs)
    pub fn stats(&self) -> (u64, u64, u64, u32, u32) {
        let (mut a, mut b, mut c, mut d, mut e) = (0u64, 0u64, 0u64, 0u32, 0u32);
        unsafe { ffi::bpp_prove_pool_stats(self.raw, &mut a, &mut b, &mut c, &mut d, &mut e) };
        (a, b, c, d, e)
    }
}

impl Drop for ProvePool {
    fn drop(&mut self) {
        unsafe { ffi::bpp_prove_pool_destroy(self.raw) }  // (fields drop afterwards: the owned engine outlives the pool)
    }
}

impl Drop for Batcher {
    fn drop(&mut self) {
        unsafe { ffi::bpp_batcher_destroy(self.raw) }  // (fields drop afterwards: the owned engine outlives the batcher)
    }
}
