// bpp.hpp -- header-only C++17 host-side mirror of the reference's public interface for the hot path, above the
// C ABI of include/bpp.h.  Same names, argument meaning and error behaviour as tari_bulletproofs_plus 0.4.1:
//
//   reference (Rust)                                          here (namespace bpp_host)
//   ---------------------------------------------------------  --------------------------------------------
//   ristretto::create_pedersen_gens_with_extension_degree      create_pedersen_gens_with_extension_degree
//   RangeParameters::init            src/range_parameters.rs:32  RangeParameters::init
//   PedersenGens::commit             pedersen_gens.rs:112        RangeParameters::commit
//   RangeStatement::init             src/range_statement.rs:36   RangeStatement::init
//   CommitmentOpening::new / RangeWitness::init                  same
//   RangeProof::{prove_with_rng, verify_batch, to_bytes, from_bytes}   same (src/range_proof.rs:232,712,1120,1155)
//   VerifyAction, ExtendedMask, ProofError{VerificationFailed,...}     same (ProofError is an exception)
//   merlin::Transcript::new(label)                               Transcript::create(label)
//   Transcript::{append_message, append_u64, challenge_bytes}    same (on the 203-byte state, host only)
//   `&mut Transcript` of prove_with_rng / verify_batch           the overloads that take the transcript(s) by pointer
//
// Scalars and points are 32-byte arrays (canonical little-endian scalar / ristretto255 encoding).
#pragma once
#include <algorithm>
#include <array>
#include <climits>
#include <cstdint>
#include <cstring>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "bpp.h"

namespace bpp_host {

using Bytes32 = std::array<uint8_t, 32>;

enum class ProofErrorKind { VerificationFailed = 1, InvalidArgument = 2, InvalidLength = 3, InvalidBlake2b = 4, SizeOverflow = 5 };

// src/errors.rs:11-28
struct ProofError : std::runtime_error {
  ProofErrorKind kind;
  ProofError(ProofErrorKind k, const std::string &m) : std::runtime_error(m), kind(k) {}
};
struct EngineFault : std::runtime_error {
  int code;
  EngineFault(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

enum class VerifyAction { VerifyOnly = 0, RecoverAndVerify = 1, RecoverOnly = 2 };  // src/range_proof.rs:46-54
enum class ExtensionDegree { DefaultPedersen = 1, AddOneBasePoint, AddTwoBasePoints, AddThreeBasePoints, AddFourBasePoints, AddFiveBasePoints };

inline void check(int rc, const char *err) {
  if (rc == 0) return;
  if (rc > 0) throw ProofError(static_cast<ProofErrorKind>(rc), err ? err : "");
  throw EngineFault(rc, err ? err : "");
}

class Engine {
 public:
  explicit Engine(int device = 0) {
    int rc = bpp_ctx_create(&ctx_, device);
    if (rc != 0) throw EngineFault(rc, "bpp_ctx_create failed: a gfx950 device is required (no CPU fallback)");
  }
  ~Engine() { bpp_ctx_destroy(ctx_); }
  Engine(const Engine &) = delete;
  Engine &operator=(const Engine &) = delete;
  bpp_ctx *ctx() const { return ctx_; }

  // "verify_check" = 1 (bpp.h, "Rechecked rejections"): every rejection this engine's verifications find on the device is
  // confirmed on an independent path -- the complementary kernel forms and the plain MSM -- before it is returned
  void verify_check(bool on) { check(bpp_ctx_set_option(ctx_, "verify_check", on ? 1 : 0), bpp_ctx_last_error(ctx_)); }
  struct bpp_verify_check_stats verify_check_stats() const {
    struct bpp_verify_check_stats s{};
    check(::bpp_verify_check_stats(ctx_, &s), bpp_ctx_last_error(ctx_));
    return s;
  }

  // "verify_joint" = 1 (bpp.h, "Joint final check"): a call with several reference batches runs one multiscalar multiplication
  // over all of them and the per-batch ones only when that check fails; for calls whose batches are expected to be valid
  void verify_joint(bool on) { check(bpp_ctx_set_option(ctx_, "verify_joint", on ? 1 : 0), bpp_ctx_last_error(ctx_)); }
  struct bpp_verify_joint_stats verify_joint_stats() const {
    struct bpp_verify_joint_stats s{};
    check(::bpp_verify_joint_stats(ctx_, &s), bpp_ctx_last_error(ctx_));
    return s;
  }

  // Prove calls in flight from ONE thread (bpp_prove_submit / bpp_prove_collect).  prove_submit hands a whole call -- the items of
  // a bpp_prove_batch_mixed, or with openings = true of a bpp_prove_openings (an item may come without commitments) -- to a lane of
  // this engine and returns at once; the items and everything they point to are free again then.  prove_collect blocks and gives
  // what the blocking call over the same items gives, item by item; an item that fails never stops the others.
  struct ProveTicket {
    uint64_t id = 0;
    size_t n_items = 0, commit_stride = 0;
    bool openings = false;
  };
  struct ProveResult {
    std::vector<std::vector<uint8_t>> proofs;       // per item; empty for an item that failed
    std::vector<std::vector<uint8_t>> commitments;  // openings tickets: per item 32 bytes per opening, as the call returned them
    std::vector<int> status;                        // per item: 0, a ProofErrorKind, or a negative engine code
    int code = 0;                                   // the call's return value: the first failing item's
    std::string message;
  };
  static constexpr size_t kProofStride = 1 + 32 * (6 + 5 + 2 * 12);  // the longest proof any parameters make
  void prove_pipeline_depth(uint32_t depth) { check(bpp_prove_pipeline_depth(ctx_, depth), bpp_ctx_last_error(ctx_)); }
  ProveTicket prove_submit(uint64_t params, const bpp_prove_item *items, size_t n_items, bool openings = false, size_t commit_stride = 0) {
    ProveTicket t;
    t.n_items = n_items;
    t.openings = openings;
    t.commit_stride = openings ? commit_stride : 0;
    char err[256] = {0};
    check(bpp_prove_submit(ctx_, params, items, n_items, kProofStride, openings ? 1 : 0, commit_stride, &t.id, err, sizeof(err)), err);
    return t;
  }
  bool prove_ticket_done(const ProveTicket &t) {
    int done = 0;
    check(bpp_prove_ticket_done(ctx_, t.id, &done), "unknown ticket");
    return done != 0;
  }
  ProveResult prove_collect(const ProveTicket &t) {
    std::vector<uint8_t> out(kProofStride * t.n_items), comm(t.openings ? t.commit_stride * t.n_items : 0);
    std::vector<size_t> lens(t.n_items, 0);
    ProveResult r;
    r.status.assign(t.n_items, 0);
    char err[256] = {0};
    r.code = bpp_prove_collect(ctx_, t.id, t.openings ? comm.data() : nullptr, out.data(), lens.data(), r.status.data(), err, sizeof(err));
    r.message = err;
    bool any_status = false;
    for (int s : r.status) any_status = any_status || s != 0;
    if (r.code != 0 && !any_status) check(r.code, err);  // (a finding of the call itself: an unknown ticket, an engine fault)
    for (size_t i = 0; i < t.n_items; i++) {
      const bool ok = r.status[i] == 0;
      r.proofs.emplace_back(out.begin() + i * kProofStride, out.begin() + i * kProofStride + (ok ? lens[i] : 0));
      if (t.openings) r.commitments.emplace_back(comm.begin() + i * t.commit_stride, comm.begin() + (i + 1) * t.commit_stride);
    }
    return r;
  }

  // Stream-ordered verification of a resident batch (bpp_verify_enqueue): the call enqueues on the engine's stream and returns; one
  // 16-byte record per group and the recovered masks land in the DEVICE buffers the caller names, valid in stream order behind the
  // call.  The ticket is for callers that do want the host to know: done() is one event query, wait() blocks, results(host_copy)
  // turns records the caller has copied to the host into the outcomes of the blocking call (code, tier, index, message text).
  class EnqueueTicket {
   public:
    uint64_t id = 0;
    size_t n_groups = 0;
    bool done() const {
      int d = 0;
      check(bpp_enqueue_done(ctx_, id, &d), "unknown ticket");
      return d != 0;
    }
    void wait() const { check(bpp_enqueue_wait(ctx_, id), bpp_ctx_last_error(ctx_)); }
    std::vector<bpp_shard_result> results(const bpp_device_verdict *host_copy) const {
      std::vector<bpp_shard_result> out(n_groups);
      for (size_t g = 0; g < n_groups; g++) check(bpp_verdict_result(&host_copy[g], &out[g]), "a record the call never wrote");
      return out;
    }

   private:
    friend class Engine;
    bpp_ctx *ctx_ = nullptr;
  };
  // group_first == nullptr: equal chunks of `chunk` proofs (0: one group) and n_groups = their number; actions == nullptr:
  // `action` for every group
  EnqueueTicket verify_enqueue(uint64_t batch, const uint32_t *group_first, size_t n_groups, size_t chunk, const int *actions,
                               VerifyAction action, bpp_device_verdict *verdicts_dev, uint8_t *masks_dev = nullptr,
                               uint8_t *mask_present_dev = nullptr) {
    EnqueueTicket t;
    t.ctx_ = ctx_;
    t.n_groups = n_groups;
    check(bpp_verify_enqueue(ctx_, batch, group_first, n_groups, chunk, actions, (int)action, verdicts_dev, masks_dev, mask_present_dev, &t.id),
          bpp_ctx_last_error(ctx_));
    return t;
  }
  // New contents of the same shape for a resident batch made by upload_packed_device, from arrays in device memory, enqueued on the
  // engine's stream (bpp_batch_refill_enqueue): a verify_enqueue afterwards gives what it would give on a fresh upload of those
  // arrays.  record_dev (may be null) receives the 16-byte refill record in stream order; the ticket is an enqueue ticket.
  EnqueueTicket batch_refill_enqueue(uint64_t batch, const bpp_packed_batch &in_dev, bpp_device_refill *record_dev = nullptr) {
    EnqueueTicket t;
    t.ctx_ = ctx_;
    // (the call first, the text afterwards: the order in which arguments are evaluated is not specified, and the call replaces the text)
    const int rc = bpp_batch_refill_enqueue(ctx_, batch, &in_dev, record_dev, &t.id);
    check(rc, bpp_ctx_last_error(ctx_));
    return t;
  }
  // ... with a live count read on the stream (bpp_batch_refill_enqueue_count): count_dev is one word in device memory, null means
  // every item.  Items at and beyond the count are dead slots; a group without a live item gets a BPP_VERDICT_EMPTY record.
  EnqueueTicket batch_refill_enqueue(uint64_t batch, const bpp_packed_batch &in_dev, const uint32_t *count_dev, bpp_device_refill *record_dev) {
    EnqueueTicket t;
    t.ctx_ = ctx_;
    const int rc = bpp_batch_refill_enqueue_count(ctx_, batch, &in_dev, count_dev, record_dev, &t.id);
    check(rc, bpp_ctx_last_error(ctx_));
    return t;
  }
  // ... under a per-item live mask read on the stream (bpp_batch_refill_enqueue_live): live_dev is n bytes in device memory, non-zero
  // means live, null means every item.  Dead slots may lie anywhere; a group without a live item gets a BPP_VERDICT_EMPTY record,
  // and a finding's index is the slot offset inside its group.
  EnqueueTicket batch_refill_enqueue_live(uint64_t batch, const bpp_packed_batch &in_dev, const uint8_t *live_dev, bpp_device_refill *record_dev) {
    EnqueueTicket t;
    t.ctx_ = ctx_;
    const int rc = bpp_batch_refill_enqueue_live(ctx_, batch, &in_dev, live_dev, record_dev, &t.id);
    check(rc, bpp_ctx_last_error(ctx_));
    return t;
  }
  // The refill of a batch of MIXED aggregation factors made by the device form of the mixed upload (bpp_batch_refill_enqueue_mixed):
  // in_dev's six arrays are device memory, its proof_lens / m repeat the batch's vectors or are both null (the batch's own).  At most
  // one of count_dev (one device word) and live_dev (n device bytes) is set; both null: every item.
  EnqueueTicket batch_refill_enqueue_mixed(uint64_t batch, const bpp_mixed_batch &in_dev, const uint32_t *count_dev = nullptr,
                                           const uint8_t *live_dev = nullptr, bpp_device_refill *record_dev = nullptr) {
    EnqueueTicket t;
    t.ctx_ = ctx_;
    const int rc = bpp_batch_refill_enqueue_mixed(ctx_, batch, &in_dev, count_dev, live_dev, record_dev, &t.id);
    check(rc, bpp_ctx_last_error(ctx_));
    return t;
  }
  // Per-item transcripts (bpp.h, "per-item transcripts on the device paths").  The refills of a batch that
  // bpp_batch_upload_packed_device_transcripts / _mixed_device_transcripts made: item_states203_dev is n rows of 203 bytes in device
  // memory, row i the STROBE state item i is verified under; count_dev / live_dev as above, at most one of them.
  EnqueueTicket batch_refill_enqueue(uint64_t batch, const bpp_packed_batch &in_dev, const uint8_t *item_states203_dev, const uint32_t *count_dev,
                                     const uint8_t *live_dev, bpp_device_refill *record_dev) {
    EnqueueTicket t;
    t.ctx_ = ctx_;
    const int rc = bpp_batch_refill_enqueue_transcripts(ctx_, batch, &in_dev, item_states203_dev, count_dev, live_dev, record_dev, &t.id);
    check(rc, bpp_ctx_last_error(ctx_));
    return t;
  }
  EnqueueTicket batch_refill_enqueue_mixed(uint64_t batch, const bpp_mixed_batch &in_dev, const uint8_t *item_states203_dev,
                                           const uint32_t *count_dev, const uint8_t *live_dev, bpp_device_refill *record_dev) {
    EnqueueTicket t;
    t.ctx_ = ctx_;
    const int rc = bpp_batch_refill_enqueue_mixed_transcripts(ctx_, batch, &in_dev, item_states203_dev, count_dev, live_dev, record_dev, &t.id);
    check(rc, bpp_ctx_last_error(ctx_));
    return t;
  }
  // verify_enqueue that also hands the advanced transcripts back on the stream (bpp_verify_enqueue_states): states_out203_dev is n x
  // 203 bytes of device memory; row i is item i's transcript after the proof where its group's record is Ok and the slot is live,
  // 203 zero bytes everywhere else.
  EnqueueTicket verify_enqueue_states(uint64_t batch, const uint32_t *group_first, size_t n_groups, size_t chunk, const int *actions,
                                      VerifyAction action, bpp_device_verdict *verdicts_dev, uint8_t *states_out203_dev,
                                      uint8_t *masks_dev = nullptr, uint8_t *mask_present_dev = nullptr) {
    EnqueueTicket t;
    t.ctx_ = ctx_;
    t.n_groups = n_groups;
    const int rc = bpp_verify_enqueue_states(ctx_, batch, group_first, n_groups, chunk, actions, (int)action, verdicts_dev, masks_dev,
                                             mask_present_dev, states_out203_dev, &t.id);
    check(rc, bpp_ctx_last_error(ctx_));
    return t;
  }
  // A diagnostic: the weights of the batch's last enqueued verification, n x 32 bytes into device memory, in stream order
  // (bpp_enqueue_weights); dead slots hold zeros.
  EnqueueTicket enqueue_weights(uint64_t batch, uint8_t *weights_dev) {
    EnqueueTicket t;
    t.ctx_ = ctx_;
    const int rc = bpp_enqueue_weights(ctx_, batch, weights_dev, &t.id);
    check(rc, bpp_ctx_last_error(ctx_));
    return t;
  }
  struct bpp_refill_stats refill_stats() const {
    struct bpp_refill_stats s{};
    const int rc = ::bpp_refill_stats(ctx_, &s);
    check(rc, bpp_ctx_last_error(ctx_));
    return s;
  }
  struct bpp_enqueue_stats enqueue_stats() const {
    struct bpp_enqueue_stats s{};
    check(::bpp_enqueue_stats(ctx_, &s), bpp_ctx_last_error(ctx_));
    return s;
  }

  // Stream-ordered proving from device arrays on a resident plan (bpp_prove_plan_create / bpp_prove_enqueue).  The plan keeps the
  // shape of a call -- `shape` is read for its geometry alone: n_items, the host array m, the strides, which arrays are non-null, the
  // call's one transcript -- and does the blocking call's host work once.  It is destroyed with the object (bpp_prove_plan_destroy,
  // which waits for its work in flight) and must not outlive the engine.
  class ProvePlan {
   public:
    ProvePlan() = default;
    ProvePlan(ProvePlan &&o) noexcept : ctx_(o.ctx_), handle_(o.handle_), n_(o.n_) { o.handle_ = 0; }
    ProvePlan &operator=(ProvePlan &&o) noexcept {
      if (this != &o) {
        reset();
        ctx_ = o.ctx_, handle_ = o.handle_, n_ = o.n_;
        o.handle_ = 0;
      }
      return *this;
    }
    ProvePlan(const ProvePlan &) = delete;
    ProvePlan &operator=(const ProvePlan &) = delete;
    ~ProvePlan() { reset(); }
    uint64_t handle() const { return handle_; }
    size_t n_items() const { return n_; }
    // proof_lens[i], and the code of an item the host refuses from m[] and the strides (0 for every other one)
    std::vector<size_t> proof_lens(std::vector<int> *host_status = nullptr) const {
      std::vector<size_t> lens(n_);
      if (host_status) host_status->assign(n_, 0);
      const int rc = bpp_prove_plan_shape(ctx_, handle_, lens.data(), host_status ? host_status->data() : nullptr);
      check(rc, bpp_ctx_last_error(ctx_));
      return lens;
    }
    void reset() {
      if (handle_) (void)bpp_prove_plan_destroy(ctx_, handle_);
      handle_ = 0;
    }

   private:
    friend class Engine;
    bpp_ctx *ctx_ = nullptr;
    uint64_t handle_ = 0;
    size_t n_ = 0;
  };
  ProvePlan prove_plan_create(uint64_t params, const bpp_prove_arrays &shape, size_t commit_stride, size_t proof_stride, uint32_t flags = 0) {
    ProvePlan p;
    char err[256] = {0};
    check(bpp_prove_plan_create(ctx_, params, &shape, commit_stride, proof_stride, flags, &p.handle_, err, sizeof(err)), err);
    p.ctx_ = ctx_;
    p.n_ = shape.n_items;
    return p;
  }
  // What an enqueue writes, all of it DEVICE memory; only the first two are required
  struct ProveEnqueueOutputs {
    uint8_t *commitments = nullptr, *proofs = nullptr;
    uint8_t *states = nullptr;                   // n x 203
    bpp_device_prove_status *status = nullptr;   // n
    uint8_t *ok_mask = nullptr;                  // n bytes: the live mask of the verifier's refill
    bpp_device_prove_summary *summary = nullptr;
  };
  // in_dev repeats the plan's shape (m may be null: the plan's own); item_states_dev iff the plan has BPP_PROVE_PLAN_ITEM_STATES;
  // live_dev: n device bytes, 0 = dead, or null.  Enqueues behind everything on the engine's stream and returns; the ticket is an
  // enqueue ticket (results() is not for it: bpp_prove_summary_result reads a host copy of the summary).
  EnqueueTicket prove_enqueue(const ProvePlan &plan, const bpp_prove_arrays &in_dev, const ProveEnqueueOutputs &out,
                              const uint8_t *item_states_dev = nullptr, const uint8_t *live_dev = nullptr) {
    EnqueueTicket t;
    t.ctx_ = ctx_;
    const int rc = bpp_prove_enqueue(ctx_, plan.handle(), &in_dev, item_states_dev, live_dev, out.commitments, out.proofs, out.states, out.status,
                                     out.ok_mask, out.summary, &t.id);
    check(rc, bpp_ctx_last_error(ctx_));
    return t;
  }
  struct bpp_prove_enqueue_stats prove_enqueue_stats() const {
    struct bpp_prove_enqueue_stats s{};
    check(::bpp_prove_enqueue_stats(ctx_, &s), bpp_ctx_last_error(ctx_));
    return s;
  }

  // Merlin on the stream (bpp_transcripts_enqueue): a program of at most BPP_TOP_MAX_OPS operations on n transcript rows of 203 bytes
  // in DEVICE memory, in place, one wavefront per row -- the rows a *_transcripts call takes are made here (op_new, op_append), the
  // rows a *_states call hands back are continued here (op_challenge).  Labels are host memory and are copied by the call; data rows
  // are device memory, row i at data_dev + i * stride (stride 0: back to back).  A row that is no transcript (pos >= 166, or
  // cur_flags == 0: the zero rows of rejected and failed items) stays 203 zero bytes with zero challenges.
  static bpp_transcript_op op_new(const uint8_t *label, uint32_t label_len) {
    bpp_transcript_op o{};
    o.kind = BPP_TOP_NEW, o.label = label, o.label_len = label_len;
    return o;
  }
  static bpp_transcript_op op_append(const uint8_t *label, uint32_t label_len, const uint8_t *data_dev, uint32_t len, size_t stride = 0,
                                     const uint32_t *lens_dev = nullptr) {
    bpp_transcript_op o{};
    o.kind = BPP_TOP_APPEND, o.label = label, o.label_len = label_len;
    o.data_dev = const_cast<uint8_t *>(data_dev), o.len = len, o.stride = stride ? stride : len, o.lens_dev = lens_dev;
    return o;
  }
  static bpp_transcript_op op_challenge(const uint8_t *label, uint32_t label_len, uint8_t *out_dev, uint32_t len, size_t stride = 0) {
    bpp_transcript_op o{};
    o.kind = BPP_TOP_CHALLENGE, o.label = label, o.label_len = label_len;
    o.data_dev = out_dev, o.len = len, o.stride = stride ? stride : len;
    return o;
  }
  // The reference's TranscriptProtocol and merlin's transcript RNG as operations of the same program (bpp.h: BPP_TOP_APPEND_POINT ..
  // BPP_TOP_RNG_SCALARS).  op_append_point voids a row whose point is 32 zero bytes; op_challenge_scalar and op_rng_scalars void a row
  // on a zero scalar.  The RNG lives for the length of the program: op_rng_begin, op_rng_rekey (any number), op_rng_finalize, then
  // op_rng_fill / op_rng_fill32 / op_rng_scalars; none of them changes the row's 203 bytes.
  static bpp_transcript_op op_append_point(const uint8_t *label, uint32_t label_len, const uint8_t *points_dev, size_t stride = 0) {
    bpp_transcript_op o = op_append(label, label_len, points_dev, 32, stride);
    o.kind = BPP_TOP_APPEND_POINT;
    return o;
  }
  static bpp_transcript_op op_challenge_scalar(const uint8_t *label, uint32_t label_len, uint8_t *out_dev, size_t stride = 0) {
    bpp_transcript_op o = op_challenge(label, label_len, out_dev, 32, stride);
    o.kind = BPP_TOP_CHALLENGE_SCALAR;
    return o;
  }
  static bpp_transcript_op op_rng_begin() {
    bpp_transcript_op o{};
    o.kind = BPP_TOP_RNG_BEGIN;
    return o;
  }
  static bpp_transcript_op op_rng_rekey(const uint8_t *label, uint32_t label_len, const uint8_t *witness_dev, uint32_t len, size_t stride = 0,
                                        const uint32_t *lens_dev = nullptr) {
    bpp_transcript_op o = op_append(label, label_len, witness_dev, len, stride, lens_dev);
    o.kind = BPP_TOP_RNG_REKEY;
    return o;
  }
  // entropy_dev: n rows of 32 bytes, the one draw from the caller's own RNG; null: the reference's NullRng
  static bpp_transcript_op op_rng_finalize(const uint8_t *entropy_dev = nullptr, size_t stride = 0) {
    bpp_transcript_op o{};
    o.kind = BPP_TOP_RNG_FINALIZE;
    if (entropy_dev) o.data_dev = const_cast<uint8_t *>(entropy_dev), o.len = 32, o.stride = stride ? stride : 32;
    return o;
  }
  static bpp_transcript_op op_rng_fill(uint8_t *out_dev, uint32_t len, size_t stride = 0) {
    bpp_transcript_op o = op_challenge(nullptr, 0, out_dev, len, stride);
    o.kind = BPP_TOP_RNG_FILL;
    return o;
  }
  static bpp_transcript_op op_rng_fill32(uint8_t *out_dev, uint32_t len, size_t stride = 0) {
    bpp_transcript_op o = op_challenge(nullptr, 0, out_dev, len, stride);
    o.kind = BPP_TOP_RNG_FILL32;
    return o;
  }
  static bpp_transcript_op op_rng_scalars(uint8_t *out_dev, uint32_t count, size_t stride = 0) {
    bpp_transcript_op o = op_challenge(nullptr, 0, out_dev, 32 * count, stride);
    o.kind = BPP_TOP_RNG_SCALARS;
    return o;
  }
  // live (n device bytes, 0 = dead: the row is neither read nor written), done_mask (n device bytes) and record may be null.  Enqueues
  // behind everything on the engine's stream and returns; the ticket is an enqueue ticket (results() is not for it).
  EnqueueTicket transcripts_enqueue(uint8_t *states203_dev, size_t n, const std::vector<bpp_transcript_op> &ops, const uint8_t *live_dev = nullptr,
                                    uint8_t *done_mask_dev = nullptr, bpp_device_transcripts_record *record_dev = nullptr) {
    EnqueueTicket t;
    t.ctx_ = ctx_;
    const int rc = bpp_transcripts_enqueue(ctx_, states203_dev, n, ops.data(), ops.size(), live_dev, done_mask_dev, record_dev, &t.id);
    check(rc, bpp_ctx_last_error(ctx_));  // (the message is read behind the call, not while its arguments are evaluated)
    return t;
  }
  struct bpp_transcripts_stats transcripts_stats() const {
    struct bpp_transcripts_stats s{};
    check(::bpp_transcripts_stats(ctx_, &s), bpp_ctx_last_error(ctx_));
    return s;
  }

  // B1 on the stream (bpp_rows_msm_enqueue, bpp_rows_scalar_enqueue): what consumes the rows transcripts_enqueue makes.
  // rows_msm_enqueue: out[i] = sum_{k < K} scalars[i][k] * points[i][k], constant-time in the scalars, K <= BPP_ROWS_K_MAX; a
  // point_stride of 0 in `in` is one row of K bases shared by every row.  rows_scalar_enqueue: out[i] = a[i] * b[i] + c[i] mod l (c
  // null: + 0; a stride of 0 is one scalar for every row).  A live row with a non-canonical scalar or an undecodable point is void:
  // zero output, done_mask 0, BPP_ROWS_SCALAR / BPP_ROWS_POINT in the record.  live, done_mask and record may be null.  Both enqueue
  // behind everything on the engine's stream and return; the ticket is an enqueue ticket.
  EnqueueTicket rows_msm_enqueue(const bpp_rows_msm &in, uint8_t *out_dev, size_t out_stride = 32, const uint8_t *live_dev = nullptr,
                                 uint8_t *done_mask_dev = nullptr, bpp_device_rows_record *record_dev = nullptr) {
    EnqueueTicket t;
    t.ctx_ = ctx_;
    const int rc = bpp_rows_msm_enqueue(ctx_, &in, out_dev, out_stride, live_dev, done_mask_dev, record_dev, &t.id);
    check(rc, bpp_ctx_last_error(ctx_));
    return t;
  }
  EnqueueTicket rows_scalar_enqueue(size_t n, const bpp_scalar_rows &a, const bpp_scalar_rows &b, const bpp_scalar_rows *c, uint8_t *out_dev,
                                    size_t out_stride = 32, const uint8_t *live_dev = nullptr, uint8_t *done_mask_dev = nullptr,
                                    bpp_device_rows_record *record_dev = nullptr) {
    EnqueueTicket t;
    t.ctx_ = ctx_;
    const int rc = bpp_rows_scalar_enqueue(ctx_, n, &a, &b, c, out_dev, out_stride, live_dev, done_mask_dev, record_dev, &t.id);
    check(rc, bpp_ctx_last_error(ctx_));
    return t;
  }
  struct bpp_rows_stats rows_stats() const {
    struct bpp_rows_stats s{};
    check(::bpp_rows_stats(ctx_, &s), bpp_ctx_last_error(ctx_));
    return s;
  }

 private:
  bpp_ctx *ctx_ = nullptr;
};

struct PedersenGens {
  ExtensionDegree extension_degree;
};
inline PedersenGens create_pedersen_gens_with_extension_degree(ExtensionDegree d) { return PedersenGens{d}; }

class Transcript {
 public:
  static Transcript create(const std::string &label) {
    Transcript t;
    t.label_ = label;
    return t;
  }
  static Transcript from_state(const uint8_t state203[203]) {
    Transcript t;
    t.state_.assign(state203, state203 + 203);
    return t;
  }
  const std::string &label() const { return label_; }
  const std::vector<uint8_t> &state() const { return state_; }

  // merlin's own operations, on the 203-byte state (host only: bpp_transcript_append_message / bpp_transcript_challenge_bytes).  A
  // label-only transcript becomes a state-carrying one first.
  void append_message(const std::string &label, const uint8_t *message, size_t len) {
    materialise();
    check(bpp_transcript_append_message(state_.data(), reinterpret_cast<const uint8_t *>(label.data()), label.size(), message, len),
          "transcript state has pos >= rate");
  }
  void append_message(const std::string &label, const std::vector<uint8_t> &message) { append_message(label, message.data(), message.size()); }
  void append_u64(const std::string &label, uint64_t x) {
    uint8_t b[8];
    for (int k = 0; k < 8; k++) b[k] = static_cast<uint8_t>(x >> (8 * k));
    append_message(label, b, 8);
  }
  std::vector<uint8_t> challenge_bytes(const std::string &label, size_t n) {
    materialise();
    std::vector<uint8_t> out(n);
    check(bpp_transcript_challenge_bytes(state_.data(), reinterpret_cast<const uint8_t *>(label.data()), label.size(), out.data(), n),
          "transcript state has pos >= rate");
    return out;
  }
  // The reference's TranscriptProtocol (src/protocols/transcript_protocol.rs) on the state: thin wrappers of the host helpers that the
  // device kinds BPP_TOP_APPEND_POINT / BPP_TOP_CHALLENGE_SCALAR are held to.  They throw the reference's ProofError.
  void validate_and_append_point(const std::string &label, const Bytes32 &point) {
    materialise();
    char err[128] = "transcript state has pos >= rate";
    check(bpp_transcript_validate_and_append_point(state_.data(), reinterpret_cast<const uint8_t *>(label.data()), label.size(), point.data(), err,
                                                   sizeof(err)), err);
  }
  Bytes32 challenge_scalar(const std::string &label) {
    materialise();
    Bytes32 out{};
    char err[128] = "transcript state has pos >= rate";
    check(bpp_transcript_challenge_scalar(state_.data(), reinterpret_cast<const uint8_t *>(label.data()), label.size(), out.data(), err, sizeof(err)),
          err);
    return out;
  }
  // merlin's TranscriptRngBuilder / TranscriptRng on a clone of the state (bpp_transcript_rng_*): build_rng(), then rekey_with_witness_bytes
  // any number of times, finalize (null: the reference's NullRng), then fill_bytes / scalar.  The state is keyed with the witness: it is
  // wiped when the object goes.
  class Rng {
   public:
    ~Rng() {
      volatile uint8_t *p = st_.data();
      for (size_t k = 0; k < st_.size(); k++) p[k] = 0;
    }
    Rng &rekey_with_witness_bytes(const std::string &label, const uint8_t *witness, size_t len) {
      check(bpp_transcript_rng_rekey(st_.data(), reinterpret_cast<const uint8_t *>(label.data()), label.size(), witness, len), "bpp_transcript_rng_rekey");
      return *this;
    }
    Rng &finalize(const uint8_t *random32 = nullptr) {
      check(bpp_transcript_rng_finalize(st_.data(), random32), "bpp_transcript_rng_finalize");
      return *this;
    }
    void fill_bytes(uint8_t *out, size_t len) { check(bpp_transcript_rng_fill(st_.data(), out, len), "bpp_transcript_rng_fill"); }
    Bytes32 scalar() {
      Bytes32 out{};
      char err[128] = "bpp_transcript_rng_scalar";
      check(bpp_transcript_rng_scalar(st_.data(), out.data(), err, sizeof(err)), err);
      return out;
    }

   private:
    friend class Transcript;
    std::array<uint8_t, 203> st_{};
  };
  Rng build_rng() {
    materialise();
    Rng r;
    check(bpp_transcript_rng_begin(state_.data(), r.st_.data()), "transcript state has pos >= rate");
    return r;
  }
  // what an advancing call (RangeProof::verify_batch / prove_batch / prove_with_rng with a transcript POINTER) leaves behind
  void advance_to(const uint8_t state203[203]) {
    state_.assign(state203, state203 + 203);
    label_.clear();
  }

 private:
  void materialise() {
    if (!state_.empty()) return;
    state_.resize(203);
    check(bpp_transcript_new(reinterpret_cast<const uint8_t *>(label_.data()), label_.size(), state_.data()), "bpp_transcript_new");
    label_.clear();
  }
  std::string label_;
  std::vector<uint8_t> state_;
};

class RangeParameters {
 public:
  static std::shared_ptr<RangeParameters> init(Engine &eng, uint32_t bit_length, uint32_t max_aggregation_factor, PedersenGens pc) {
    auto p = std::shared_ptr<RangeParameters>(new RangeParameters(eng));
    check(bpp_params_create(eng.ctx(), bit_length, max_aggregation_factor, static_cast<uint32_t>(pc.extension_degree), nullptr, nullptr,
                            &p->handle_), bpp_ctx_last_error(eng.ctx()));
    p->n_ = bit_length;
    p->m_ = max_aggregation_factor;
    p->t_ = static_cast<uint32_t>(pc.extension_degree);
    return p;
  }
  // Arc::clone for another context of the same device (bpp_params_retain): the same device tables, usable from `eng`
  // concurrently with every other holder (`Precomputation: Send + Sync`, src/traits.rs:42)
  std::shared_ptr<RangeParameters> share(Engine &eng) const {
    check(bpp_params_retain(eng.ctx(), handle_), bpp_ctx_last_error(eng.ctx()));
    auto p = std::shared_ptr<RangeParameters>(new RangeParameters(eng));
    p->handle_ = handle_;
    p->n_ = n_;
    p->m_ = m_;
    p->t_ = t_;
    return p;
  }
  ~RangeParameters() {
    if (handle_) bpp_params_destroy(eng_.ctx(), handle_);
  }
  uint32_t bit_length() const { return n_; }
  uint32_t max_aggregation_factor() const { return m_; }
  ExtensionDegree extension_degree() const { return static_cast<ExtensionDegree>(t_); }
  uint64_t handle() const { return handle_; }
  Engine &engine() const { return eng_; }
  // PedersenGens::commit(value, blindings)
  Bytes32 commit(uint64_t value, const std::vector<Bytes32> &blindings) const {
    Bytes32 out{};
    check(bpp_pedersen_commit(eng_.ctx(), handle_, &value, blindings.empty() ? nullptr : blindings[0].data(),
                              static_cast<uint32_t>(blindings.size()), 1, out.data()), bpp_ctx_last_error(eng_.ctx()));
    return out;
  }

 private:
  explicit RangeParameters(Engine &e) : eng_(e) {}
  Engine &eng_;
  uint64_t handle_ = 0;
  uint32_t n_ = 0, m_ = 0, t_ = 0;
};

struct RangeStatement {
  std::shared_ptr<RangeParameters> generators;
  std::vector<Bytes32> commitments_compressed;
  std::vector<std::optional<uint64_t>> minimum_value_promises;
  std::optional<Bytes32> seed_nonce;
  // src/range_statement.rs:36-73
  static RangeStatement init(std::shared_ptr<RangeParameters> generators, std::vector<Bytes32> commitments,
                             std::vector<std::optional<uint64_t>> minimum_value_promises, std::optional<Bytes32> seed_nonce) {
    const size_t n = commitments.size();
    if (n == 0 || (n & (n - 1))) throw ProofError(ProofErrorKind::InvalidArgument, "Number of commitments must be a power of two");
    if (minimum_value_promises.size() != n) throw ProofError(ProofErrorKind::InvalidArgument, "Incorrect number of minimum value promises");
    if (generators->max_aggregation_factor() < n) throw ProofError(ProofErrorKind::InvalidArgument, "Not enough generators for this statement");
    if (seed_nonce && n > 1) throw ProofError(ProofErrorKind::InvalidArgument, "Mask recovery is not supported with an aggregated statement");
    return RangeStatement{std::move(generators), std::move(commitments), std::move(minimum_value_promises), seed_nonce};
  }
};

struct CommitmentOpening {
  uint64_t v;
  std::vector<Bytes32> r;
  static CommitmentOpening create(uint64_t v, std::vector<Bytes32> r) { return CommitmentOpening{v, std::move(r)}; }
};

struct RangeWitness {
  std::vector<CommitmentOpening> openings;
  uint32_t extension_degree;
  // src/range_witness.rs:24-41
  static RangeWitness init(std::vector<CommitmentOpening> openings) {
    if (openings.empty()) throw ProofError(ProofErrorKind::InvalidLength, "Vector openings cannot be empty");
    const size_t t = openings[0].r.size();
    for (const auto &o : openings) {
      if (o.r.empty()) throw ProofError(ProofErrorKind::InvalidLength, "Extended blinding factors cannot be empty");
      if (o.r.size() != t) throw ProofError(ProofErrorKind::InvalidLength, "Extended blinding factors must have consistent length");
    }
    if (t < 1 || t > 6) throw ProofError(ProofErrorKind::InvalidArgument, "Extension degree not valid");
    return RangeWitness{std::move(openings), static_cast<uint32_t>(t)};
  }
};

// a bpp_packed_batch whose six array fields are addresses in DEVICE memory (bpp.h: bpp_verify_batch_packed_device)
struct DevicePackedBatch {
  bpp_packed_batch arrays;
};

// a bpp_mixed_batch whose six array fields are addresses in DEVICE memory (bpp.h: bpp_verify_batch_mixed_device); proof_lens and m
// stay host memory
struct DeviceMixedBatch {
  bpp_mixed_batch arrays;
};

// a bpp_prove_arrays whose array fields are addresses in DEVICE memory (bpp.h: bpp_prove_openings_device); m and the transcript
// stay host memory
struct DeviceProveArrays {
  bpp_prove_arrays arrays;
};

// where RangeProof::prove_openings over a DeviceProveArrays writes, all of it DEVICE memory (status may be null), and what comes
// back on the host
struct DeviceProveOutputs {
  uint8_t *commitments;
  size_t commit_stride;
  uint8_t *proofs;
  size_t proof_stride;
  bpp_device_prove_status *status;
};
struct DeviceProveResult {
  int code;                       // 0, or the first failing item's code
  std::string message;            // its message
  std::vector<size_t> proof_lens;
  std::vector<int> item_status;
};

struct ExtendedMask {
  std::vector<Bytes32> blindings;
  bool operator==(const ExtendedMask &o) const { return blindings == o.blindings; }
};

class RangeProof {
 public:
  const std::vector<uint8_t> &to_bytes() const { return raw_; }
  bool operator==(const RangeProof &o) const { return raw_ == o.raw_; }

  // src/range_proof.rs:1155-1257 (structure only here; canonical-scalar checks are repeated by the engine on upload)
  static RangeProof from_bytes(const std::vector<uint8_t> &bytes) {
    if (bytes.empty()) throw ProofError(ProofErrorKind::InvalidLength, "Serialized proof is too short");
    const uint32_t t = bytes[0];
    if (t < 1 || t > 6) throw ProofError(ProofErrorKind::InvalidArgument, "Extension degree not valid");
    const size_t body = bytes.size() - 1, chunks = body / 32;
    if (chunks < t + 5 + 2) throw ProofError(ProofErrorKind::InvalidLength, "Serialized proof is too short");
    if ((body % 32) || ((chunks - t - 5) % 2)) throw ProofError(ProofErrorKind::InvalidLength, "Unused data after deserialization");
    RangeProof p;
    p.raw_ = bytes;
    return p;
  }

  static uint32_t rounds_for(const RangeStatement &st) {
    uint32_t mn = st.generators->bit_length() * static_cast<uint32_t>(st.commitments_compressed.size()), r = 0;
    while ((1u << r) < mn) r++;
    return r;
  }

  // n x prove_with_rng in one engine call; rng_bytes[i] = (rounds + 3) x 32 bytes from the caller's RNG
  static std::vector<RangeProof> prove_batch(const std::vector<Transcript> &transcripts, const std::vector<RangeStatement> &statements,
                                             const std::vector<RangeWitness> &witnesses, const std::vector<std::vector<uint8_t>> &rng_bytes) {
    return prove_batch_impl(transcripts, statements, witnesses, rng_bytes, nullptr);
  }
  // The reference's `&mut Transcript` (src/range_proof.rs:222-237): the forms that take their transcripts by POINTER advance them --
  // on success every transcript is left as the prover left it (after the last challenge), on an error all are untouched.  A pointer
  // and not a non-const reference: callers of the const forms above hold ordinary, non-const objects, and an overload on constness
  // would silently start advancing theirs.  (A template, so that a braced `{}` for the transcripts still means the const form's empty
  // vector and never a null pointer.)  One call of bpp_prove_batch_mixed_states; throws the first failing item's error.
  template <class T, class = std::enable_if_t<std::is_same<T, Transcript>::value>>
  static std::vector<RangeProof> prove_batch(std::vector<T> *transcripts, const std::vector<RangeStatement> &statements,
                                             const std::vector<RangeWitness> &witnesses, const std::vector<std::vector<uint8_t>> &rng_bytes) {
    if (!transcripts) throw ProofError(ProofErrorKind::InvalidArgument, "null transcripts");
    std::vector<uint8_t> states;
    auto proofs = prove_batch_impl(*transcripts, statements, witnesses, rng_bytes, &states);
    for (size_t i = 0; i < transcripts->size(); i++) (*transcripts)[i].advance_to(&states[203 * i]);
    return proofs;
  }
  static RangeProof prove_with_rng(Transcript *transcript, const RangeStatement &statement, const RangeWitness &witness,
                                   const std::vector<uint8_t> &rng_bytes) {
    if (!transcript) throw ProofError(ProofErrorKind::InvalidArgument, "null transcript");
    std::vector<uint8_t> states;
    auto proofs = prove_batch_impl({*transcript}, {statement}, {witness}, {rng_bytes}, &states);
    transcript->advance_to(states.data());
    return proofs[0];
  }

 private:
  // states != nullptr: bpp_prove_batch_mixed_states, 203 bytes per item into *states
  static std::vector<RangeProof> prove_batch_impl(const std::vector<Transcript> &transcripts, const std::vector<RangeStatement> &statements,
                                                  const std::vector<RangeWitness> &witnesses, const std::vector<std::vector<uint8_t>> &rng_bytes,
                                                  std::vector<uint8_t> *states) {
    const size_t n = statements.size();
    if (n == 0 || witnesses.size() != n || transcripts.size() != n || rng_bytes.size() != n)
      throw ProofError(ProofErrorKind::InvalidArgument, "Range statements, witnesses, transcripts length mismatch");
    auto &params = *statements[0].generators;
    std::vector<bpp_prove_item> items(n);
    std::vector<std::vector<uint64_t>> vals(n), mins(n);
    std::vector<std::vector<uint8_t>> blind(n), comm(n), pres(n);
    for (size_t i = 0; i < n; i++) {
      const auto &st = statements[i];
      const auto &w = witnesses[i];
      const size_t m = st.commitments_compressed.size();
      if (w.openings.size() != m) throw ProofError(ProofErrorKind::InvalidLength, "Witness openings and statement commitments do not match!");
      if (w.extension_degree != static_cast<uint32_t>(params.extension_degree()))
        throw ProofError(ProofErrorKind::InvalidLength, "Witness and statement extension degrees do not match!");
      for (size_t j = 0; j < m; j++) {
        vals[i].push_back(w.openings[j].v);
        for (const auto &r : w.openings[j].r) blind[i].insert(blind[i].end(), r.begin(), r.end());
        comm[i].insert(comm[i].end(), st.commitments_compressed[j].begin(), st.commitments_compressed[j].end());
        mins[i].push_back(st.minimum_value_promises[j].value_or(0));
        pres[i].push_back(st.minimum_value_promises[j] ? 1 : 0);
      }
      bpp_prove_item &it = items[i];
      memset(&it, 0, sizeof(it));
      it.values = vals[i].data();
      it.blindings32 = blind[i].data();
      it.commitments32 = comm[i].data();
      it.m = static_cast<uint32_t>(m);
      it.min_values = mins[i].data();
      it.min_present = pres[i].data();
      it.seed_nonce32 = st.seed_nonce ? st.seed_nonce->data() : nullptr;
      fill_transcript(transcripts[i], it.transcript_state, it.transcript_label, it.label_len);
      it.rng_bytes = rng_bytes[i].data();
      it.rng_len = rng_bytes[i].size();
    }
    const size_t stride = 1 + 32 * (6 + 5 + 2 * 12);
    std::vector<uint8_t> out(stride * n);
    size_t plen = 0;
    char err[256] = {0};
    std::vector<RangeProof> proofs;
    if (states) {
      states->assign(203 * n, 0);
      std::vector<size_t> lens(n, 0);
      check(bpp_prove_batch_mixed_states(params.engine().ctx(), params.handle(), items.data(), n, out.data(), stride, lens.data(), nullptr,
                                         states->data(), err, sizeof(err)), err);
      for (size_t i = 0; i < n; i++) proofs.push_back(from_bytes(std::vector<uint8_t>(out.begin() + i * stride, out.begin() + i * stride + lens[i])));
      return proofs;
    }
    check(bpp_prove_batch(params.engine().ctx(), params.handle(), items.data(), n, out.data(), stride, &plen, err, sizeof(err)), err);
    for (size_t i = 0; i < n; i++) proofs.push_back(from_bytes(std::vector<uint8_t>(out.begin() + i * stride, out.begin() + i * stride + plen)));
    return proofs;
  }

 public:
  static RangeProof prove_with_rng(const Transcript &transcript, const RangeStatement &statement, const RangeWitness &witness,
                                   const std::vector<uint8_t> &rng_bytes) {
    return prove_batch({transcript}, {statement}, {witness}, {rng_bytes})[0];
  }

  // Prove from the openings alone (bpp_prove_openings): the engine makes commit(v, r) for every opening, in the same call, and the
  // statements are built from what it returns.  Any aggregation factors (powers of two up to the parameters' maximum) in one call;
  // minimum_value_promises[i] has one entry per opening of witnesses[i], seed_nonces[i] only with one opening.  Throws the first
  // failing item's error.
  static std::pair<std::vector<RangeStatement>, std::vector<RangeProof>> prove_openings(
      const std::vector<Transcript> &transcripts, const std::vector<RangeWitness> &witnesses,
      const std::vector<std::vector<std::optional<uint64_t>>> &minimum_value_promises, const std::vector<std::optional<Bytes32>> &seed_nonces,
      const std::vector<std::vector<uint8_t>> &rng_bytes, const std::shared_ptr<RangeParameters> &generators) {
    const size_t n = witnesses.size();
    if (n == 0 || transcripts.size() != n || minimum_value_promises.size() != n || seed_nonces.size() != n || rng_bytes.size() != n)
      throw ProofError(ProofErrorKind::InvalidArgument, "Range statements, witnesses, transcripts length mismatch");
    auto &params = *generators;
    std::vector<bpp_prove_item> items(n);
    std::vector<std::vector<uint64_t>> vals(n), mins(n);
    std::vector<std::vector<uint8_t>> blind(n), pres(n);
    size_t m_max = 1;
    for (size_t i = 0; i < n; i++) {
      const auto &w = witnesses[i];
      const size_t m = w.openings.size();
      m_max = std::max(m_max, m);
      if (minimum_value_promises[i].size() != m) throw ProofError(ProofErrorKind::InvalidArgument, "Incorrect number of minimum value promises");
      if (w.extension_degree != static_cast<uint32_t>(params.extension_degree()))
        throw ProofError(ProofErrorKind::InvalidLength, "Witness and statement extension degrees do not match!");
      for (size_t j = 0; j < m; j++) {
        vals[i].push_back(w.openings[j].v);
        for (const auto &r : w.openings[j].r) blind[i].insert(blind[i].end(), r.begin(), r.end());
        mins[i].push_back(minimum_value_promises[i][j].value_or(0));
        pres[i].push_back(minimum_value_promises[i][j] ? 1 : 0);
      }
      bpp_prove_item &it = items[i];
      memset(&it, 0, sizeof(it));  // (commitments32 stays NULL: to be made)
      it.values = vals[i].data();
      it.blindings32 = blind[i].data();
      it.m = static_cast<uint32_t>(m);
      it.min_values = mins[i].data();
      it.min_present = pres[i].data();
      it.seed_nonce32 = seed_nonces[i] ? seed_nonces[i]->data() : nullptr;
      fill_transcript(transcripts[i], it.transcript_state, it.transcript_label, it.label_len);
      it.rng_bytes = rng_bytes[i].data();
      it.rng_len = rng_bytes[i].size();
    }
    const size_t stride = 1 + 32 * (6 + 5 + 2 * 12), cstride = 32 * m_max;
    std::vector<uint8_t> out(stride * n), comm(cstride * n);
    std::vector<size_t> lens(n, 0);
    char err[256] = {0};
    check(bpp_prove_openings(params.engine().ctx(), params.handle(), items.data(), n, comm.data(), cstride, out.data(), stride, lens.data(),
                             nullptr, err, sizeof(err)), err);
    std::pair<std::vector<RangeStatement>, std::vector<RangeProof>> res;
    for (size_t i = 0; i < n; i++) {
      std::vector<Bytes32> cs(items[i].m);
      for (size_t j = 0; j < cs.size(); j++) std::copy_n(comm.begin() + i * cstride + 32 * j, 32, cs[j].begin());
      res.first.push_back(RangeStatement::init(generators, std::move(cs), minimum_value_promises[i], seed_nonces[i]));
      res.second.push_back(from_bytes(std::vector<uint8_t>(out.begin() + i * stride, out.begin() + i * stride + lens[i])));
    }
    return res;
  }

  // The same from openings that lie in DEVICE memory (bpp_prove_openings_device): what bpp_prove_openings writes on host copies of
  // the same arrays, with the proofs and commitments left in device memory, in the geometry a DeviceMixedBatch describes.  A failed
  // item never stops the others and does not throw: look at the result.  Throws when the whole call is refused or the engine faults.
  static DeviceProveResult prove_openings(const DeviceProveArrays &openings, const DeviceProveOutputs &out,
                                          const std::shared_ptr<RangeParameters> &generators) {
    auto &params = *generators;
    const size_t n = openings.arrays.n_items;
    const int unset = INT_MIN;
    DeviceProveResult res{0, std::string(), std::vector<size_t>(n, 0), std::vector<int>(n, unset)};
    char err[256] = {0};
    res.code = bpp_prove_openings_device(params.engine().ctx(), params.handle(), &openings.arrays, out.commitments, out.commit_stride,
                                         out.proofs, out.proof_stride, res.proof_lens.data(), out.status, res.item_status.data(), err,
                                         sizeof(err));
    bool refused = res.code != 0;  // (a refusal writes no item's status)
    for (int s : res.item_status) refused = refused && s == unset;
    if (res.code < 0 || refused) check(res.code, err);
    res.message = err;
    return res;
  }

  // ... with one transcript per item going in and the advanced transcripts coming out (bpp_prove_openings_device_transcripts):
  // item_states_dev is n rows of 203 bytes in DEVICE memory, row i the STROBE state item i's proof continues (openings.arrays then
  // names no transcript), or null: the call's one transcript; states_out_dev is n rows of 203 bytes of DEVICE memory that receive
  // the transcripts as the proofs left them (zeros for an item that fails), or null.  A row with pos >= 166 is its item's finding.
  static DeviceProveResult prove_openings(const DeviceProveArrays &openings, const uint8_t *item_states_dev, const DeviceProveOutputs &out,
                                          uint8_t *states_out_dev, const std::shared_ptr<RangeParameters> &generators) {
    auto &params = *generators;
    const size_t n = openings.arrays.n_items;
    const int unset = INT_MIN;
    DeviceProveResult res{0, std::string(), std::vector<size_t>(n, 0), std::vector<int>(n, unset)};
    char err[256] = {0};
    res.code = bpp_prove_openings_device_transcripts(params.engine().ctx(), params.handle(), &openings.arrays, item_states_dev, out.commitments,
                                                     out.commit_stride, out.proofs, out.proof_stride, res.proof_lens.data(), states_out_dev,
                                                     out.status, res.item_status.data(), err, sizeof(err));
    bool refused = res.code != 0;  // (a refusal writes no item's status)
    for (int s : res.item_status) refused = refused && s == unset;
    if (res.code < 0 || refused) check(res.code, err);
    res.message = err;
    return res;
  }

  // src/range_proof.rs:712-752; every `chunk` proofs are one reference batch (all chunks are verified)
  static std::vector<std::optional<ExtendedMask>> verify_batch(const std::vector<Transcript> &transcripts,
                                                                const std::vector<RangeStatement> &statements,
                                                                const std::vector<RangeProof> &proofs, VerifyAction action,
                                                                size_t chunk = BPP_REFERENCE_CHUNK) {
    return verify_batch_impl(transcripts, statements, proofs, action, chunk, nullptr);
  }
  // `&mut [Transcript]` (src/range_proof.rs:712-717): with the transcripts by POINTER (see prove_batch) a call that succeeds leaves
  // every transcript as the verifier left it -- r1, s1 and every d1 appended (src/transcripts.rs:166-172); an error leaves all untouched
  template <class T, class = std::enable_if_t<std::is_same<T, Transcript>::value>>
  static std::vector<std::optional<ExtendedMask>> verify_batch(std::vector<T> *transcripts,
                                                                const std::vector<RangeStatement> &statements,
                                                                const std::vector<RangeProof> &proofs, VerifyAction action,
                                                                size_t chunk = BPP_REFERENCE_CHUNK) {
    if (!transcripts) throw ProofError(ProofErrorKind::InvalidArgument, "null transcripts");
    std::vector<uint8_t> states;
    auto masks = verify_batch_impl(*transcripts, statements, proofs, action, chunk, &states);
    for (size_t i = 0; i < transcripts->size(); i++) (*transcripts)[i].advance_to(&states[203 * i]);
    return masks;
  }

  // The packed form of a homogeneous batch (bpp.h: bpp_packed_batch), as an overload pair: arrays in host memory, or --
  // DevicePackedBatch -- arrays that already lie in the memory of the engine's device (bpp_verify_batch_packed_device: checked
  // and packed on the device, never read on the host; whatever wrote them must be ordered before the engine's stream).
  // Same results either way.
  static std::vector<std::optional<ExtendedMask>> verify_batch(const RangeParameters &params, const bpp_packed_batch &in, VerifyAction action,
                                                                size_t chunk = BPP_REFERENCE_CHUNK) {
    return verify_packed_impl(params, in, action, chunk, false);
  }
  static std::vector<std::optional<ExtendedMask>> verify_batch(const RangeParameters &params, const DevicePackedBatch &in, VerifyAction action,
                                                                size_t chunk = BPP_REFERENCE_CHUNK) {
    return verify_packed_impl(params, in.arrays, action, chunk, true);
  }

  // The array form for batches of MIXED aggregation factors (bpp.h: bpp_mixed_batch, the geometry of the prover's mixed output), as
  // an overload pair of the same kind: arrays in host memory, or -- DeviceMixedBatch -- arrays in the memory of the engine's device
  // (bpp_verify_batch_mixed_device).  The results of the item form on the same rows either way.
  static std::vector<std::optional<ExtendedMask>> verify_batch(const RangeParameters &params, const bpp_mixed_batch &in, VerifyAction action,
                                                                size_t chunk = BPP_REFERENCE_CHUNK) {
    return verify_mixed_impl(params, in, action, chunk, false);
  }
  static std::vector<std::optional<ExtendedMask>> verify_batch(const RangeParameters &params, const DeviceMixedBatch &in, VerifyAction action,
                                                                size_t chunk = BPP_REFERENCE_CHUNK) {
    return verify_mixed_impl(params, in.arrays, action, chunk, true);
  }

 private:
  static std::vector<std::optional<ExtendedMask>> verify_mixed_impl(const RangeParameters &params, const bpp_mixed_batch &in, VerifyAction action,
                                                                     size_t chunk, bool on_device) {
    const uint32_t t = static_cast<uint32_t>(params.extension_degree());
    std::vector<uint8_t> masks(in.n_items * t * 32), present(in.n_items);
    char err[256] = {0};
    check((on_device ? bpp_verify_batch_mixed_device : bpp_verify_batch_mixed)(params.engine().ctx(), params.handle(), &in, static_cast<int>(action),
                                                                                 chunk, masks.data(), present.data(), err, sizeof(err)), err);
    return masks_of(masks, present, t);
  }
  static std::vector<std::optional<ExtendedMask>> verify_packed_impl(const RangeParameters &params, const bpp_packed_batch &in, VerifyAction action,
                                                                      size_t chunk, bool on_device) {
    const uint32_t t = static_cast<uint32_t>(params.extension_degree());
    std::vector<uint8_t> masks(in.n_items * t * 32), present(in.n_items);
    char err[256] = {0};
    check((on_device ? bpp_verify_batch_packed_device : bpp_verify_batch_packed)(params.engine().ctx(), params.handle(), &in, static_cast<int>(action),
                                                                                   chunk, masks.data(), present.data(), err, sizeof(err)), err);
    return masks_of(masks, present, t);
  }
  static std::vector<std::optional<ExtendedMask>> verify_batch_impl(const std::vector<Transcript> &transcripts,
                                                                     const std::vector<RangeStatement> &statements,
                                                                     const std::vector<RangeProof> &proofs, VerifyAction action, size_t chunk,
                                                                     std::vector<uint8_t> *states) {
    if (statements.empty() || proofs.empty() || transcripts.empty())
      throw ProofError(ProofErrorKind::InvalidArgument, "Range statements or proofs length empty");
    if (statements.size() != proofs.size()) throw ProofError(ProofErrorKind::InvalidArgument, "Range statements and proofs length mismatch");
    if (transcripts.size() != statements.size())
      throw ProofError(ProofErrorKind::InvalidArgument, "Range statements and transcripts length mismatch");
    const size_t n = proofs.size();
    // the statement with the largest generator capacity carries the tables (src/range_proof.rs:666-673, :778);
    // generators of smaller capacities are prefixes of it (bulletproof_gens.rs:24-41)
    const RangeParameters *largest = statements[0].generators.get();
    for (const auto &st : statements)
      if (st.generators->max_aggregation_factor() > largest->max_aggregation_factor()) largest = st.generators.get();
    const RangeParameters &params = *largest;
    const uint32_t t = static_cast<uint32_t>(params.extension_degree());
    std::vector<bpp_verify_item> items(n);
    std::vector<std::vector<uint64_t>> mins(n);
    std::vector<std::vector<uint8_t>> comm(n), pres(n);
    for (size_t i = 0; i < n; i++) {
      const auto &st = statements[i];
      if (st.generators->bit_length() != params.bit_length())
        throw ProofError(ProofErrorKind::InvalidArgument, "Inconsistent bit length in batch statement");
      if (st.generators->extension_degree() != params.extension_degree())
        throw ProofError(ProofErrorKind::InvalidArgument, "Inconsistent extension degree");
      for (size_t j = 0; j < st.commitments_compressed.size(); j++) {
        comm[i].insert(comm[i].end(), st.commitments_compressed[j].begin(), st.commitments_compressed[j].end());
        mins[i].push_back(st.minimum_value_promises[j].value_or(0));
        pres[i].push_back(st.minimum_value_promises[j] ? 1 : 0);
      }
      bpp_verify_item &it = items[i];
      memset(&it, 0, sizeof(it));
      it.proof = proofs[i].raw_.data();
      it.proof_len = proofs[i].raw_.size();
      it.commitments32 = comm[i].data();
      it.m = static_cast<uint32_t>(st.commitments_compressed.size());
      it.min_values = mins[i].data();
      it.min_present = pres[i].data();
      it.seed_nonce32 = st.seed_nonce ? st.seed_nonce->data() : nullptr;
      fill_transcript(transcripts[i], it.transcript_state, it.transcript_label, it.label_len);
    }
    std::vector<uint8_t> masks(n * t * 32), present(n);
    char err[256] = {0};
    if (states) {
      states->assign(203 * n, 0);
      check(bpp_verify_batch_states(params.engine().ctx(), params.handle(), items.data(), n, static_cast<int>(action), chunk, masks.data(),
                                    present.data(), states->data(), err, sizeof(err)), err);
    } else {
      check(bpp_verify_batch(params.engine().ctx(), params.handle(), items.data(), n, static_cast<int>(action), chunk, masks.data(),
                             present.data(), err, sizeof(err)), err);
    }
    return masks_of(masks, present, t);
  }

  static std::vector<std::optional<ExtendedMask>> masks_of(const std::vector<uint8_t> &masks, const std::vector<uint8_t> &present, uint32_t t) {
    const size_t n = present.size();
    std::vector<std::optional<ExtendedMask>> out(n);
    for (size_t i = 0; i < n; i++) {
      if (!present[i]) continue;
      ExtendedMask em;
      for (uint32_t k = 0; k < t; k++) {
        Bytes32 b;
        memcpy(b.data(), &masks[(i * t + k) * 32], 32);
        em.blindings.push_back(b);
      }
      out[i] = em;
    }
    return out;
  }

  static void fill_transcript(const Transcript &tr, const uint8_t *&state, const uint8_t *&label, size_t &len) {
    if (!tr.state().empty()) {
      state = tr.state().data();
    } else {
      label = reinterpret_cast<const uint8_t *>(tr.label().data());
      len = tr.label().size();
    }
  }
  std::vector<uint8_t> raw_;
};

}  // namespace bpp_host
