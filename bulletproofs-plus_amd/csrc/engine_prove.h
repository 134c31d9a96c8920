// Host side of the batch prover (bpp_prove_batch, include/bpp.h): the fixed-base tables, the round schedule of the WIP argument
// (src/range_proof.rs:401-607) as kernel launches over two sub-batches, zeroization of everything witness-derived.  The checks of
// RangeStatement / RangeWitness construction (src/range_statement.rs:43-62, src/range_proof.rs:238-311) and the witness packing are
// prove_pack_host.h's: pure host code, which the CPU suite drives under AddressSanitizer / UBSan.  Included at the end of
// engine.hip (it uses the context, the parameter registry and the staging buffers defined there); kernels: kernels_prove.h.
#pragma once

// ================================================================= batch prover
namespace {
// the proof length of an item whose m passes RangeStatement::init, 0 otherwise
size_t prove_item_len(const Params &P, uint32_t m) { return prove_item_len_host(ParamShape{P.n_bits, P.m_max, P.t}, m); }

// the host-side checks of a one-item bpp_prove_batch on `it`, in the same order and with the same codes and messages
// (prove_job_host.h has them: bpp_prove_submit runs the same routine before it copies an item, and so does the packer).
// openings: an item of bpp_prove_openings / bpp_prove_pool_openings, which may come without commitments and whose commitments go
// to a slot of commit_stride bytes.
void prove_item_check(const Params &P, const bpp_prove_item &it, size_t proof_stride, bool openings = false, size_t commit_stride = 0) {
  prove_item_check_host(ParamShape{P.n_bits, P.m_max, P.t}, it, proof_stride, openings, commit_stride);
}

void prove_self_check(bpp_ctx *ctx, uint64_t params, const Params &P, const bpp_prove_item *items, uint32_t B, size_t plen, uint8_t *&proofs,
                      uint32_t *&status, const bpp_ctx::CheckTamper &tamper, bool remake, std::vector<uint8_t> &kept_proofs,
                      std::vector<uint32_t> &kept_status, uint8_t *made32, size_t made_stride, uint8_t *tstates203);
// what follows "proof %u failed the engine's self-check: " / "the proof failed the engine's self-check: "
const char *const kSelfCheckRejectedWhy = "the verifier rejected it and its remake";
const char *const kSelfCheckRecoveryWhy =
    "mask recovery under its seed nonce does not return the witness's blinding factors, for it and for its remake";
// (a host-side flag next to the device's PV_STATUS_* bits: the proof failed the self-check, after its remake if there was one)
#define PV_STATUS_SELF_CHECK 0x100u
// (with it: what failed was the replay of mask recovery, not the verifier's verdict -- "prove_check_recovery" = 1)
#define PV_STATUS_SELF_CHECK_RECOVERY 0x200u

// What a caller of prove_uniform gives and wants back.
// dev_status == nullptr: bpp_prove_batch itself, which turns the first device-side status word into the call's error.  Otherwise
// (bpp_prove_batch_mixed) the status words go to dev_status[i] and every proof is copied out at proof_stride (*proof_len: the
// longest): whoever called sorts the items out.
// mixed: the items may have different aggregation factors, sorted largest first (bpp_prove_batch_mixed has checked each one).
// They run as ragged launches aligned at the end: R = items[0]'s rounds global steps, proof i joins at step R - rounds_i
// (ProveDesc::roff), and as the proofs are sorted, those active at a step are a prefix of every sub-batch: each round's kernels
// and fixed-base MSM cover only that prefix.  Every proof reaches the final step in the same launch.
// "prove_check" = 1: the proofs are verified before any of them is copied out (prove_self_check; `tamper`: the test knobs taken by
// the call's entry point, proof = index + 1 in `items`; remake = false: the call IS a remake, whose failure is final).
// made32 != nullptr (bpp_prove_openings): an item may come without commitments (commitments32 == NULL); the ones the witness check
// computes are then its statement's (ProveDesc::flags bit 1, kp_adopt_commitments in front of kp_init).  What the check computed
// for EVERY item of the call comes back at made32 + i * 32 * items[0].m: for an item whose status word is 0 those are its
// statement's commitments, made or brought.  A sub-batch without such an item -- every call with made32 == nullptr -- is enqueued
// exactly as before.
// states203 != nullptr (bpp_prove_*_states): kp_finish's other instantiation also writes every proof's transcript as
// challenge_final_e leaves it; row i of states203 (203 bytes, call order) is written for every item whose status word ends as 0 --
// after the self-check, whose remake of a proof brings its own row -- and left alone for every other item.  A call without it
// carves, enqueues and copies exactly what it did.
// dev != nullptr (bpp_prove_openings_device): the witness does not come from `items` but from arrays in device memory, and the
// proofs, commitments and outcomes go to rows in device memory (ProveDeviceIO below): the call's SOURCE is the ingest kernel in
// place of the packer, the staging and the uploads, its SINK the emit kernel in place of the copies to the host.  Everything between
// -- plan, arena, streams, every step -- is the same.  A call without it enqueues launch for launch what it did.
struct ProveDeviceIO {
  const bpp_prove_arrays *in;      // the caller's struct: device addresses, the host's m[] and transcript
  ProveDeviceShape shape;          // prove_device_shape of its m[] and strides: the slots (rows, m_sorted) and the refused items
  uint8_t *commitments_out;
  size_t commit_stride;
  uint8_t *proofs_out;
  size_t proof_stride;
  bpp_device_prove_status *status_dev;
  std::vector<bpp_device_prove_status> outcome;  // by slot: what came back
  // bpp_prove_openings_device_transcripts: row i of item_states (device memory, n x 203) is the transcript item i continues -- the
  // call-wide head runs on the device (k_prove_item_states) and no state table is uploaded; row i of states_out (device memory)
  // receives the advanced transcript of an item that succeeds, zeros otherwise.  Either may be null.
  const uint8_t *item_states = nullptr;
  uint8_t *states_out = nullptr;
  // bpp_prove_enqueue (engine_prove_plan.h): the call is one of a resident plan, whose ProveCall lives as long as the plan and is
  // enqueued again and again.  per_item: every enqueue brings item_states (the plan is carved for them before the first rows exist);
  // live: the caller's mask by item; ok_mask / outcome_item: what k_prove_emit writes by item beside status_dev.  All null otherwise.
  bool per_item = false;
  const uint8_t *live = nullptr;
  uint8_t *ok_mask = nullptr;
  bpp_device_prove_status *outcome_item = nullptr;
};

struct ProveRequest {
  uint64_t params;
  const bpp_prove_item *items;
  size_t n_items;
  uint8_t *proofs_out;
  size_t proof_stride;
  size_t *proof_len;
  uint32_t *dev_status = nullptr;
  bool mixed = false;
  bpp_ctx::CheckTamper tamper{};
  bool remake = true;
  uint8_t *made32 = nullptr;
  uint8_t *states203 = nullptr;
  ProveDeviceIO *dev = nullptr;
};

// One prove call (the context's lock held, its device current): its packed witness, its plan, its sub-batches and its staging,
// and the stages prove_uniform runs over them, in the order they are defined.
struct ProveCall {
  struct Sub {
    uint32_t lo, nb;
    bool adopts;  // holds an item whose commitments are to be made: its kp_init waits for the witness check
    size_t bytes_lo, bytes_len, arena_lo, arena_len;
    uint8_t *d_bytes, *d_states, *d_minpres, *d_a32, *d_lr, *d_a1b, *d_proofs, *d_commit32;
    uint32_t *d_tstates = nullptr;  // the advanced transcripts, rows of BPP_STATE_ROW_WORDS words (states203 only)
    ProveDesc *d_desc;
    // (device arrays only) the slots' rows, the ingest kernel's finding words, the outcomes on their way to the host
    ProveDevRow *d_rows = nullptr;
    uint32_t *d_finding = nullptr;
    bpp_device_prove_status *d_outcome = nullptr;
    uint64_t *d_minvals;
    ProveState *d_ps;
    sc *d_vec, *d_ts, *d_cts;
    uint32_t *d_tg, *d_tc, *d_ctg, *d_ctc, *d_ftg, *d_ftc;
    sc *d_fts;
    ge *d_ge, *d_ge_ct, *d_part;
    // "ct" = 2: the four public points per proof of the last round (GE, GO, HE, HO: kp_wave_body) as term lists, slice sums, points,
    // and their multiples by 16^w
    sc *d_exs;
    uint32_t *d_exg, *d_exc;
    ge *d_expart, *d_expts, *d_pow, *d_ctprod;
  };
  struct Fix {  // a pointer of a Sub that is arena base + off once the arena exists
    void *field;
    size_t off;
    void (*set)(void *field, uint8_t *p);
  };

  bpp_ctx *const ctx;
  Params &P;
  const ProveRequest &r;
  ProvePack pk;
  uint32_t n = 0, t = 0, m = 0, B = 0, mn = 0, rounds = 0, stride = 0, n_gen = 0;
  size_t plen = 0;
  // plan
  uint32_t sub_size = 0, n_sub = 0, parts = 0, kp_waves = 1, ex_back = 0, ex_nt = 0, ex_terms = 0, ex_parts = 0;
  bool ct_check = false, ct = false, fused = false, prio = false, fifo = false;
  std::vector<Sub> subs;
  std::vector<Fix> fixes;
  size_t arena_need = 0;
  uint8_t *pin_bytes = nullptr, *pin_states = nullptr, *pin_minpres = nullptr, *pin_minvals = nullptr, *pin_desc = nullptr;
  uint8_t *pin_proofs = nullptr, *pin_made = nullptr, *pin_rows = nullptr;
  bpp_device_prove_status *pin_outcome = nullptr;
  uint32_t *pin_status = nullptr, *pin_tstates = nullptr;
  const dim3 b64{64};
  size_t ev_used = 0;
  std::chrono::steady_clock::time_point t_begin;
  bool arena_clean = true, staging_clean = false;
  // where the arena and the staging on the way in live: the context's, shared by its blocking calls -- or (resident) a plan's own,
  // carved and staged ONCE: the staging then holds the plan's public tables alone, is never rewritten and never wiped, nothing comes
  // back to the host, and the arena holds a state row per slot whether or not an enqueue asks for the advanced transcripts
  DevBuf<uint8_t> *arena;
  PinnedBuf<uint8_t> *pin_in;
  bool resident = false;

  ProveCall(bpp_ctx *c, Params &p, const ProveRequest &req) : ctx(c), P(p), r(req), arena(&c->prove_arena), pin_in(&c->prove_pin_in) {}

  // kp_finish's instantiation that leaves the advanced transcripts in the arena: for the host (states203) or for the emit kernel
  bool wants_states() const { return r.states203 || (r.dev && r.dev->states_out); }
  // per-item transcripts from device memory: the slots of a sub-batch (each reads its own row of the sub-batch's table), else 0
  uint32_t per_item_sub() const { return r.dev && (r.dev->item_states || r.dev->per_item) ? prove_sub_size((uint32_t)r.n_items, ctx->opt.prove_subs) : 0u; }

  // pk.bytes (values, blinding factors, seed nonces), the page-locked staging in both directions (witness bytes in,
  // ProveState out) and the device arena hold witness-derived data: wiped on EVERY exit path, including the
  // "Witness opening is invalid!" and HIP-error ones
  // (the page-locked staging on the way OUT carries proofs and status words only -- nothing secret: the per-proof states stay on
  // the device and are wiped there)
  void wipe_secrets() {
    if (!staging_clean) {
      pk.wipe();
      wipe(pin_in->p, pin_in->n);
    }
    if (!arena_clean && arena->p) {
      for (auto &ps : ctx->prove_aux_streams) (void)hipStreamSynchronize(ps);
      for (auto &ps : ctx->prove_streams) (void)hipStreamSynchronize(ps);
      for (auto &ps : ctx->prove_lane_streams) (void)hipStreamSynchronize(ps);
      if (ctx->prove_msm_stream) (void)hipStreamSynchronize(ctx->prove_msm_stream);
      (void)hipMemsetAsync(arena->p, 0, arena->n, ctx->stream);  // (stream-ordered and waited for: the next
      (void)hipStreamSynchronize(ctx->stream);                                           // call's streams do not wait for the null stream)
    }
  }

  // lane(q): the stream of sub-batch q's small kernels; msm(q): of its fixed-base MSMs (the same stream without prove_prio)
  hipStream_t lane_stream(uint32_t q) const { return prio ? ctx->prove_lane_streams[q] : ctx->prove_streams[q]; }
  hipStream_t msm_stream(uint32_t q) const { return fifo ? ctx->prove_msm_stream : ctx->prove_streams[q]; }
  void to_msm(uint32_t q) {  // the MSM stream continues behind everything enqueued on the lane stream so far
    if (!prio && !fifo) return;
    HIP_CHECK(hipEventRecord(ctx->prove_sync_events[2 * q], lane_stream(q)));
    HIP_CHECK(hipStreamWaitEvent(msm_stream(q), ctx->prove_sync_events[2 * q], 0));
  }
  void to_lane(uint32_t q) {  // and back
    if (!prio && !fifo) return;
    HIP_CHECK(hipEventRecord(ctx->prove_sync_events[2 * q + 1], msm_stream(q)));
    HIP_CHECK(hipStreamWaitEvent(lane_stream(q), ctx->prove_sync_events[2 * q + 1], 0));
  }
  // profiling: an event pair around every k_fb_msm launch (the prover's dominant kernel), summed after the call
  void fb_mark(hipStream_t st) {
    if (!ctx->profile) return;
    if (ev_used == ctx->prove_events.size()) {
      hipEvent_t e;
      HIP_CHECK(hipEventCreate(&e));
      ctx->prove_events.push_back(e);
    }
    HIP_CHECK(hipEventRecord(ctx->prove_events[ev_used++], st));
  }

  // ---- the witness: checked and packed by prove_pack_host.h; *proof_len is written before the stride is looked at
  void pack() {
    const ParamShape shape{P.n_bits, P.m_max, P.t};
    if (r.dev) {  // (every slot has passed the host's part of the checks; the rest is the ingest kernel's)
      const bpp_prove_arrays &in = *r.dev->in;
      prove_plan_device(shape, P.hg32.data(), r.dev->shape.m_sorted.data(), r.n_items, in.commitments32 != nullptr, in.transcript_state,
                        in.transcript_label, in.label_len, pk, per_item_sub());
      set_shape();
      return;
    }
    const size_t len0 = prove_item_len_host(shape, r.items[0].m);  // (0: items[0] has no proof length, and the packer says why)
    if (len0 && r.proof_len) *r.proof_len = len0;
    if (len0 && r.proof_stride < len0) throw ProofErr{BPP_ERR_INVALID_LENGTH, "proof_stride too small"};
    pk.pack(shape, P.hg32.data(), r.items, r.n_items, r.mixed, r.made32 != nullptr);
    set_shape();
  }
  void set_shape() {
    n = P.n_bits, t = P.t, m = pk.m, B = (uint32_t)r.n_items, mn = m * n, rounds = pk.rounds, plen = pk.plen;
    stride = 2 * mn + t + 1;
    n_gen = 2 * P.n_bits * P.m_max;
  }

  // ---- the plan: what the options make of this call
  void plan() {
    // The batch runs as up to PROVE_SUBS sub-batches, each on its own stream: a round is lane step (one lane per proof,
    // Fiat-Shamir latency, a handful of wavefronts) -> wave step -> fixed-base MSM (fills the chip), so one sub-batch's
    // lane step overlaps another's MSM.  All device buffers come out of one arena allocation per call.
    sub_size = prove_sub_size(B, ctx->opt.prove_subs);  // (2 unless "prove_subs" says otherwise, at most 16; never fewer than 64 slots)
    constexpr size_t PROVE_PART_BUDGET = (size_t)2 << 30;
    n_sub = cdiv(B, sub_size);
    // A round of a sub-batch is [point encoding, Fiat-Shamir step, vector fold] -> [fixed-base MSM]: three latency-bound
    // kernels of a few wavefronts, then one that fills the chip.  While one sub-batch's MSM runs, the other's small kernels
    // queue for wave slots behind its 1024 workgroups and take 2-3x their own time (point encoding 70 -> 200 us, fold 45 -> 175:
    // profiles/r04_prover_launches.txt), the MSMs of the two sub-batches drift into each other, and every period has ~110 us
    // in which no MSM runs.  With prove_prio the small kernels go to a HIGH-priority stream of their own (the hardware hands
    // freed wave slots to that queue first), joined to the MSM stream by an event each way per round.
    // Secret-only terms through the uniform-access forms of ct.h, where the reference is constant-time:
    //   "ct" >= 1 (the default): the witness check's commit(v, r) (src/generators/pedersen_gens.rs:112-122, src/range_proof.rs:275-284)
    //   "ct" == 2: A1 and B as well (:572-584): no secret scalar of theirs reaches a fixed-base table.  The Pedersen-base terms go
    //              through the uniform-access lines (k_ct_fixed); the folded generators of the final step are written as
    //              Gf[0] = e^-1 GE + e y^-1 GO, Hf[0] = e HE + e^-1 HO over four PUBLIC points of the last round, whose fixed-base MSM
    //              and 16^w multiples (k_ct_pow16: 252 doublings) run on the side stream beside the last round and the final step,
    //              and the secrets r e^-1, r e y^-1, s e, s e^-1 meet them in k_ct_var: seven additions, a select and a tree (ct.h)
    //   "ct" == 0: everything through the fixed-base tables, whose addresses are the scalars' digits
    ct_check = ctx->opt.ct != 0, ct = ctx->opt.ct == 2;
    fused = ctx->opt.prove_fused != 0;
    // wavefronts per proof in the fused round kernel: 1 (the three phases in a row: the default), 2 or 4 (kernels_prove.h: kp_round:
    // each workgroup's own chain gets 35 % shorter, the call does not -- a round kernel's wavefronts need 174 registers each and
    // find no room on a SIMD beside three of the other sub-batch's MSM wavefronts, so more of them per proof only wait longer:
    // profiles/r05_prover_waves_ab.txt)
    kp_waves = ctx->opt.prove_waves == 2 ? 2u : (ctx->opt.prove_waves == 4 ? 4u : 1u);
    // The rounds' fixed-base MSMs as independent one-wavefront slices (k_fb_part) whose partial sums the next round kernel adds
    // up, instead of one four-wavefront workgroup per output with a reduction tree at its end (k_fb_msm).  `parts` slices per
    // output: enough workgroups for ~4 wavefronts per SIMD, never more than FBP_MAX_PER terms in a slice.  "prove_parts" = 0 keeps
    // the workgroup form (tests run both), a positive value fixes the number of slices.
    parts = 0;
    if (ctx->opt.prove_parts != 0) {
      const uint32_t outs = 2 * sub_size;  // (a round's outputs per sub-batch as it really is cut)
      parts = ctx->opt.prove_parts > 0 ? (uint32_t)ctx->opt.prove_parts : cdiv(3072u, outs);
      parts = std::max(parts, cdiv(mn + t + 1, (uint32_t)FBP_MAX_PER));
      parts = std::min<uint32_t>(std::max<uint32_t>(parts, 1u), FBP_MAX_PARTS);
      if (cdiv(mn + t + 1, parts) > FBP_MAX_PER) parts = 0;  // (aggregations whose rounds do not fit the slices: the workgroup form)
      // the slices' partial sums are 3 x proofs x parts x 64 points per sub-batch (30 KB per proof and slice), zeroed with the rest
      // of the arena after every call: beyond PROVE_PART_BUDGET per sub-batch (a call of more than ~20 000 proofs per sub-batch) the
      // workgroup form, whose sums stay in LDS, takes over
      if (parts && (size_t)3 * sub_size * parts * 64 * sizeof(ge) > PROVE_PART_BUDGET) parts = 0;
    }  // one launch per round for encoding + Fiat-Shamir step + vector step (tests run both)
    prio = ctx->opt.prove_prio > 0;  // (off by default: measured, no gain -- profiles/r04_prover_prio_ab.txt)
    // The fixed-base MSMs of ALL sub-batches on ONE stream, in the order they are enqueued (round by round, sub-batch by
    // sub-batch), each behind its own round kernel by an event: first in, first out.  On a stream per sub-batch two MSM launches
    // that are both ready SHARE the chip: the later one ends when it would have ended anyway, but the earlier one ends later by
    // the time they overlapped -- and its sub-batch's next round kernel, the chain that bounds the call, starts later by as much.
    // Measured (profiles/r05_prover_waves_ab.txt, (d)): the MSMs' own event time drops 4 %, the call gets 4 % SLOWER -- two more
    // cross-stream events per round and sub-batch cost more than the sharing did.  Off unless asked for ("prove_fifo" = 1).
    fifo = !prio && n_sub > 1 && ctx->opt.prove_fifo > 0;
    // "ct" = 2: the public points behind A1's folded generators are made ex_back rounds before the end (kernels_prove.h): their
    // fixed-base MSM, the slices' sums and the 252 doublings of their 16^w multiples then have ex_back rounds of time beside the
    // call's own chain.  2^ex_back points per side and proof; ex_parts slices of <= 128 terms per point.  One round back is the
    // rule ("ct_back" = 2, 3 for the A/B): earlier, the points' MSM doubles the load of a round whose own MSM the chain waits for,
    // and the time the final step no longer spends in an MSM is not given back (profiles/r06_ct_back_ab.txt).
    // (mixed calls: at most the smallest class's rounds, so that every proof is active at step R - ex_back; the bytes do not depend
    // on ex_back)
    ex_back = std::min<uint32_t>(pk.rounds_min, ctx->opt.ct_back > 0 ? std::min(3, ctx->opt.ct_back) : 1u);
    ex_nt = 2 * (1u << ex_back), ex_terms = mn >> ex_back, ex_parts = cdiv(ex_terms, 128u);
  }

  // ---- the arena: one pass lays out every sub-batch's buffers; the pointers follow once the arena is there
  template <class T>
  void take(T *&field, size_t nbytes) {
    arena_need = (arena_need + 255) & ~(size_t)255;
    fixes.push_back(Fix{&field, arena_need, [](void *f, uint8_t *p) { *(T **)f = (T *)p; }});
    arena_need += nbytes;
  }
  void carve() {
    subs.resize(n_sub);
    fixes.reserve((size_t)n_sub * 40);
    for (uint32_t q = 0; q < n_sub; q++) {
      Sub &u = subs[q];
      u.lo = q * sub_size;
      u.nb = std::min(sub_size, B - u.lo);
      u.bytes_lo = pk.desc[u.lo].wit_off;
      u.bytes_len = (u.lo + u.nb < B ? pk.desc[u.lo + u.nb].wit_off : pk.bytes_len) - u.bytes_lo;
      const size_t nb = u.nb;
      arena_need = (arena_need + 255) & ~(size_t)255;
      u.arena_lo = arena_need;
      take(u.d_bytes, u.bytes_len);
      take(u.d_states, prove_states_table_bytes(pk, per_item_sub(), u.nb));
      take(u.d_minpres, nb * m);
      take(u.d_minvals, nb * m * 8);
      take(u.d_desc, nb * sizeof(ProveDesc));
      take(u.d_ps, nb * sizeof(ProveState));
      take(u.d_vec, nb * (size_t)KP_VEC_LEN(mn) * sizeof(sc));
      take(u.d_ts, nb * 2 * stride * sizeof(sc));
      take(u.d_tg, nb * 2 * stride * 4);
      take(u.d_tc, nb * 3 * 4);  // (three outputs per proof in the last launch)
      take(u.d_a32, nb * 32);
      take(u.d_lr, (size_t)rounds * nb * 64);
      take(u.d_a1b, nb * 64);
      take(u.d_proofs, nb * plen);
      take(u.d_commit32, nb * m * 32);
      take(u.d_cts, nb * m * (1 + t) * sizeof(sc));
      take(u.d_ctg, nb * m * (1 + t) * 4);
      take(u.d_ctc, nb * m * 4);
      take(u.d_ge, std::max<size_t>(nb * m, 3 * nb) * sizeof(ge));
      take(u.d_fts, nb * 2 * CT_ROW * sizeof(sc));
      take(u.d_ftg, nb * 2 * CT_ROW * 4);
      take(u.d_ftc, nb * 2 * 4);
      take(u.d_ge_ct, 2 * nb * sizeof(ge));
      take(u.d_part, parts ? (size_t)3 * nb * parts * 64 * sizeof(ge) : 16);
      take(u.d_exs, ct ? nb * 2 * (size_t)mn * sizeof(sc) : 16);
      take(u.d_exg, ct ? nb * 2 * (size_t)mn * 4 : 16);
      take(u.d_exc, nb * ex_nt * 4);
      take(u.d_expart, ct ? (size_t)ex_nt * nb * ex_parts * 64 * sizeof(ge) : 16);
      take(u.d_expts, ct ? (size_t)ex_nt * nb * sizeof(ge) : 16);
      take(u.d_pow, ct ? (size_t)ex_nt * nb * BPP_CT_DIGITS * sizeof(ge) : 16);
      take(u.d_ctprod, ct ? (size_t)ex_nt * nb * sizeof(ge) : 16);
      if (wants_states() || resident) take(u.d_tstates, nb * BPP_STATE_ROW_WORDS * 4);  // (last, and only when asked for -- a plan always asks: the arena of every other call is laid out as before)
      if (r.dev) {  // (as above)
        take(u.d_rows, nb * sizeof(ProveDevRow));
        take(u.d_finding, nb * 4);
        take(u.d_outcome, nb * sizeof(bpp_device_prove_status));
      }
      u.arena_len = arena_need - u.arena_lo;
      u.adopts = false;
      // descriptors are relative to each sub-batch's own byte block / minimum-value rows
      for (uint32_t i = 0; i < u.nb; i++) {
        ProveDesc &d = pk.desc[u.lo + i];
        u.adopts = u.adopts || (d.flags & PV_FLAG_MAKE_COMMITMENTS);
        d.wit_off -= (uint32_t)u.bytes_lo;
        d.commit_off -= (uint32_t)u.bytes_lo;
        d.ext_off -= (uint32_t)u.bytes_lo;
        d.seed_off -= (uint32_t)u.bytes_lo;
        d.minval_idx = i * m;
      }
    }
    // a fresh arena starts out zero as a whole: the alignment gaps between the sub-batches' ranges and the slack at its end
    // are written by nothing and wiped by nothing, and what hipMalloc hands out is not zero -- bpp_prove_secret_bytes (and
    // anyone reading the arena) must see zeros there, not somebody's left-overs
    // (a regrown arena may come back at the address the freed one had: the size tells, not the pointer alone)
    const uint8_t *before = arena->p;
    const size_t before_n = arena->n;
    arena->alloc(arena_need + 256);
    if (arena->p != before || arena->n != before_n) {  // (on a stream of ours and waited for: the sub-batch streams do not wait for the null stream)
      HIP_CHECK(hipMemsetAsync(arena->p, 0, arena->n, ctx->stream));
      HIP_CHECK(hipStreamSynchronize(ctx->stream));
    }
    for (const Fix &f : fixes) f.set(f.field, arena->p + f.off);
  }

  // ---- fixed-base window tables for every generator of these parameters (one-off; contexts sharing P serialise here)
  void ensure_fb_table() {
    std::lock_guard<std::mutex> fb_lock(P.fb_mu);
    if (P.fb_table.p) return;
    P.fb_geo = fb_geometry(P.table_len);
    P.fb_table.alloc((size_t)P.table_len * fb_stride(P.fb_geo));
    hipLaunchKernelGGL(k_fb_build, dim3(cdiv(P.table_len * P.fb_geo.windows * cdiv(P.fb_geo.entries, FB_BUILD_BLOCK), 64)), dim3(64), 0,
                       ctx->stream, P.table.p, P.table_len, P.fb_geo, P.fb_table.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
  }

  // ---- the context's streams and events, as many as this call's sub-batches need (they stay with the context)
  template <class T, class Make>
  static void ensure(std::vector<T> &have, size_t want, Make make) {
    while (have.size() < want) {
      T x;
      HIP_CHECK(make(&x));
      have.push_back(x);
    }
  }
  void ensure_streams() {
    auto stream = [](hipStream_t *s) { return hipStreamCreateWithFlags(s, hipStreamNonBlocking); };
    auto event = [](hipEvent_t *e) { return hipEventCreateWithFlags(e, hipEventDisableTiming); };
    ensure(ctx->prove_streams, n_sub, stream);
    if (fifo && !ctx->prove_msm_stream) HIP_CHECK(stream(&ctx->prove_msm_stream));
    if (prio || fifo) ensure(ctx->prove_sync_events, 2 * (size_t)n_sub, event);
    if (prio) {
      int least = 0, greatest = 0;
      HIP_CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
      ensure(ctx->prove_lane_streams, n_sub, [&](hipStream_t *s) { return hipStreamCreateWithPriority(s, hipStreamNonBlocking, greatest); });
    }
    ensure(ctx->prove_aux_streams, n_sub, stream);
    // per sub-batch: inputs resident, witness check done; ("ct" = 2) last round's lists written, 16^w multiples made
    ensure(ctx->prove_aux_events, 4 * (size_t)n_sub, event);
  }

  // ---- page-locked staging so that no copy stalls the enqueue of the next sub-batch
  void stage_in() {
    if (r.dev) return stage_in_device();
    const size_t in_need = pk.bytes.size() + pk.states.size() + pk.minpres.size() + pk.minvals.size() * 8 + (size_t)B * sizeof(ProveDesc) + 64;
    ctx->prove_pin_in.resize(in_need);
    // (on the way out: proofs, status words and -- made32 -- the commitments the witness check computed: nothing secret)
    ctx->prove_pin_out.resize((size_t)B * plen + (size_t)B * sizeof(uint32_t) + 64 + (r.made32 ? (size_t)B * m * 32 : 0) +
                              (r.states203 ? (size_t)B * BPP_STATE_ROW_WORDS * 4 + 16 : 0));
    pin_bytes = ctx->prove_pin_in.p;
    memcpy(pin_bytes, pk.bytes.data(), pk.bytes.size());
    pin_states = pin_bytes + pk.bytes.size();
    memcpy(pin_states, pk.states.data(), pk.states.size());
    pin_minpres = pin_states + pk.states.size();
    memcpy(pin_minpres, pk.minpres.data(), pk.minpres.size());
    pin_minvals = pin_minpres + ((pk.minpres.size() + 7) & ~(size_t)7);
    memcpy(pin_minvals, pk.minvals.data(), pk.minvals.size() * 8);
    pin_desc = pin_minvals + pk.minvals.size() * 8;
    memcpy(pin_desc, pk.desc.data(), (size_t)B * sizeof(ProveDesc));
    pin_proofs = ctx->prove_pin_out.p;
    pin_status = (uint32_t *)(pin_proofs + (((size_t)B * plen + 15) & ~(size_t)15));
    pin_made = (uint8_t *)pin_status + (((size_t)B * sizeof(uint32_t) + 15) & ~(size_t)15);
    pin_tstates = (uint32_t *)(pin_made + (r.made32 ? (((size_t)B * m * 32 + 15) & ~(size_t)15) : 0));  // (public data)
  }

  // ---- the device-arrays form of the staging: the plan's public tables alone -- states, descriptors, rows -- on the way in (no
  // witness byte passes through prove_pin_in), one outcome record per slot on the way out
  void stage_in_device() {
    auto up8 = [](size_t v) { return (v + 7) & ~(size_t)7; };
    pin_in->resize(up8(pk.states.size()) + (size_t)B * (sizeof(ProveDesc) + sizeof(ProveDevRow)) + 64);
    if (!resident) ctx->prove_pin_out.resize((size_t)B * sizeof(bpp_device_prove_status) + 64);
    pin_states = pin_in->p;
    memcpy(pin_states, pk.states.data(), pk.states.size());
    pin_desc = pin_states + up8(pk.states.size());
    memcpy(pin_desc, pk.desc.data(), (size_t)B * sizeof(ProveDesc));
    pin_rows = pin_desc + (size_t)B * sizeof(ProveDesc);
    memcpy(pin_rows, r.dev->shape.rows.data(), (size_t)B * sizeof(ProveDevRow));
    if (resident) return;  // (a plan forks per enqueue, and nothing of it comes back to the host)
    pin_outcome = (bpp_device_prove_status *)ctx->prove_pin_out.p;
    fork_from_ctx();
  }
  // whatever wrote the caller's arrays is complete on, or ordered before, the context's stream: every sub-batch's ingest kernel
  // waits for this point of it
  void fork_from_ctx() {
    if (!ctx->prove_dev_event) HIP_CHECK(hipEventCreateWithFlags(&ctx->prove_dev_event, hipEventDisableTiming));
    HIP_CHECK(hipEventRecord(ctx->prove_dev_event, ctx->stream));
  }

  // ---- sub-batch q's inputs from the page-locked staging ...
  void upload_inputs(uint32_t q) {
    Sub &u = subs[q];
    hipStream_t s = lane_stream(q);
    const uint32_t nb = u.nb;
    HIP_CHECK(hipMemcpyAsync(u.d_bytes, pin_bytes + u.bytes_lo, u.bytes_len, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(u.d_states, pin_states, pk.states.size(), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(u.d_minpres, pin_minpres + (size_t)u.lo * m, (size_t)nb * m, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(u.d_minvals, pin_minvals + (size_t)u.lo * m * 8, (size_t)nb * m * 8, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(u.d_desc, pin_desc + (size_t)u.lo * sizeof(ProveDesc), (size_t)nb * sizeof(ProveDesc),
                             hipMemcpyHostToDevice, s));
  }
  // ---- ... or from the caller's arrays where they lie: k_prove_ingest writes d_bytes, d_minvals and d_minpres (the arena is zero
  // where it writes nothing: the promise rows beyond an item's m) and sets the nonce bit of the uploaded descriptors
  void ingest_inputs(uint32_t q) {
    Sub &u = subs[q];
    hipStream_t s = lane_stream(q);
    const uint32_t nb = u.nb;
    const bpp_prove_arrays &in = *r.dev->in;
    // (a plan's enqueue: the whole sub-batch behind the fork -- the tables land in an arena range the previous enqueue's wipe, on this
    // very stream, has left zero, and they bring back bit 0 of every descriptor's flags, which the ingest kernel sets)
    if (resident) HIP_CHECK(hipStreamWaitEvent(s, ctx->prove_dev_event, 0));
    if (!pk.states.empty()) HIP_CHECK(hipMemcpyAsync(u.d_states, pin_states, pk.states.size(), hipMemcpyHostToDevice, s));  // (per-item transcripts: none)
    HIP_CHECK(hipMemcpyAsync(u.d_desc, pin_desc + (size_t)u.lo * sizeof(ProveDesc), (size_t)nb * sizeof(ProveDesc), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(u.d_rows, pin_rows + (size_t)u.lo * sizeof(ProveDevRow), (size_t)nb * sizeof(ProveDevRow), hipMemcpyHostToDevice, s));
    if (!resident) HIP_CHECK(hipStreamWaitEvent(s, ctx->prove_dev_event, 0));
    ProveIngest a;
    memset(&a, 0, sizeof(a));
    a.values = (const uint8_t *)in.values;
    a.blindings32 = in.blindings32;
    a.commitments32 = in.commitments32;
    a.min_values = (const uint8_t *)in.min_values;
    a.min_present = in.min_present;
    a.seed_nonces32 = in.seed_nonces32;
    a.seed_present = in.seed_present;
    a.rng_bytes = in.rng_bytes;
    a.rng_stride = in.rng_stride;
    a.m_stride = in.m_stride;
    a.n_bits = n, a.t = t, a.nb = nb;
    a.g0_32 = P.d_hg32.p + 32;
    a.rows = u.d_rows;
    a.desc = u.d_desc;
    a.bytes = u.d_bytes;
    a.minvals = u.d_minvals;
    a.minpres = u.d_minpres;
    a.finding = u.d_finding;
    a.item_states = r.dev->item_states;
    a.live = r.dev->live;
    hipLaunchKernelGGL(k_prove_ingest, dim3(cdiv(nb, BPP_INGEST_BLOCK / BPP_INGEST_LANES)), dim3(BPP_INGEST_BLOCK), 0, s, a);
    HIP_CHECK(hipGetLastError());
  }

  // ---- per-item transcripts: the call-wide head of every slot's transcript, from the caller's row into row k of d_states.  Behind
  // the ingest kernel (its finding words say which rows are read) and the point the witness check branches off at, in front of kp_init.
  void item_states_in(uint32_t q) {
    Sub &u = subs[q];
    ProveItemStates a;
    memset(&a, 0, sizeof(a));
    a.src = r.dev->item_states;
    a.rows = u.d_rows;
    a.desc = u.d_desc;
    a.finding = u.d_finding;
    a.hg32 = P.d_hg32.p;
    a.n_bits = n, a.t = t, a.nb = u.nb;
    a.states = u.d_states;
    hipLaunchKernelGGL(k_prove_item_states, dim3(u.nb), b64, 0, lane_stream(q), a);
    HIP_CHECK(hipGetLastError());
  }

  // ---- sub-batch q's inputs, its witness check on the side stream, kp_init and kp_A
  void enqueue_init(uint32_t q) {
    Sub &u = subs[q];
    hipStream_t s = lane_stream(q);
    const uint32_t nb = u.nb;
    if (r.dev) ingest_inputs(q);
    else upload_inputs(q);
    // witness check (:275-284): commit(v_j, r_j) for every opening, compared with the statement's commitments.  Nothing of the
    // proof depends on it (a mismatch is a status bit read after the call), so its three kernels run on a stream of their own
    // beside kp_init / kp_A / the first round's small kernels (in line they were 0.2 ms of the call's first 0.75 ms, in which no
    // round's MSM runs yet) and are joined in front of the first round's MSM, which reuses their output buffer
    hipStream_t sx = ctx->prove_aux_streams[q];
    HIP_CHECK(hipEventRecord(ctx->prove_aux_events[4 * q], s));
    HIP_CHECK(hipStreamWaitEvent(sx, ctx->prove_aux_events[4 * q], 0));
    hipLaunchKernelGGL(kp_commit_terms, dim3(cdiv(nb * m, 64)), b64, 0, sx, u.d_bytes, u.d_desc, t, n_gen, nb, m, 1 + t, u.d_cts,
                       u.d_ctg, u.d_ctc);
    if (ct_check) {
      hipLaunchKernelGGL(k_ct_fixed, dim3(nb * m), b64, 0, sx, u.d_cts, u.d_ctg, u.d_ctc, 1 + t, n_gen, (const niels *)P.fb_ct.p, u.d_ge);
    } else {
      fb_mark(sx);
      hipLaunchKernelGGL(k_fb_msm, dim3(nb * m), dim3(fb_threads(ctx, 1 + t, P.fb_geo)), 0, sx, u.d_cts, u.d_ctg, u.d_ctc, 1 + t, P.fb_table.p,
                         P.fb_geo, u.d_ge, 0u);
      fb_mark(sx);
    }
    hipLaunchKernelGGL(k_compress_ge, dim3(cdiv(nb * m, 64)), b64, 0, sx, u.d_ge, nb * m, u.d_commit32);
    HIP_CHECK(hipEventRecord(ctx->prove_aux_events[4 * q + 1], sx));
    if (per_item_sub()) item_states_in(q);
    if (u.adopts) {
      // bpp_prove_openings: the transcript starts with the statement's commitments, and for a flagged proof those are what the
      // check has just computed: here kp_init waits for the check instead of running beside it.  (The first round's MSM waits for
      // the same event again, as in every call: a wait for an event that has fired.)
      HIP_CHECK(hipStreamWaitEvent(s, ctx->prove_aux_events[4 * q + 1], 0));
      hipLaunchKernelGGL(kp_adopt_commitments, dim3(cdiv(nb * m, 64)), b64, 0, s, u.d_bytes, u.d_desc, u.d_commit32, nb, m);
    }
    hipLaunchKernelGGL(kp_init, dim3(nb), b64, 0, s, u.d_bytes, u.d_desc, u.d_minvals, u.d_states, P.d_hg32.p, n, t, nb, u.d_ps);
    hipLaunchKernelGGL(kp_A, dim3(nb), b64, 0, s, u.d_bytes, u.d_desc, u.d_minvals, u.d_minpres, P.table.p, P.fb_table.p, P.fb_geo, n_gen, n,
                       t, u.d_ps, u.d_a32);
  }

  // ---- global step j (0 .. rounds: the rounds and the final step) of sub-batch q
  void enqueue_step(uint32_t j, uint32_t q) {
    Sub &u = subs[q];
    hipStream_t s = lane_stream(q), sm = msm_stream(q);
    const uint32_t nb = u.nb;
    uint8_t *lr_prev = j ? u.d_lr + (size_t)(j - 1) * nb * 64 : nullptr;
    // the proofs of this sub-batch that take part in step j (all of them in a uniform call): a prefix, roff ascending
    uint32_t na = nb;
    while (na && pk.roff[u.lo + na - 1] > j) na--;
    if (na == 0) {
      if (j == 0) {  // (the witness check joins all the same: see below)
        HIP_CHECK(hipStreamWaitEvent(s, ctx->prove_aux_events[4 * q + 1], 0));
        hipLaunchKernelGGL(kp_check_commitments, dim3(cdiv(nb, 64)), b64, 0, s, u.d_bytes, u.d_desc, u.d_commit32, nb, u.d_ps);
      }
      return;
    }
    if (fused) {  // the previous round's L / R are encoded by the same launch (kernels_prove.h: kp_round)
      auto launch_round = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(na), dim3(64 * kp_waves), 0, s, u.d_bytes, u.d_desc, u.d_minvals, u.d_minpres, n, t, n_gen, na, j, rounds,
                           stride, u.d_a32, j ? (parts ? u.d_part : u.d_ge) : (const ge *)nullptr, parts, lr_prev, u.d_ps, u.d_vec, u.d_ts, u.d_tg,
                           u.d_tc, ct ? u.d_fts : (sc *)nullptr, u.d_ftg, u.d_ftc, ct ? u.d_exs : (sc *)nullptr, u.d_exg, u.d_exc, ex_back);
      };
      if (kp_waves == 1) launch_round(kp_round<1>);
      else if (kp_waves == 2) launch_round(kp_round<2>);
      else launch_round(kp_round<4>);
    } else {
      hipLaunchKernelGGL(kp_lane, dim3(na), b64, 0, s, u.d_bytes, u.d_desc, n, t, na, j, rounds, u.d_a32, lr_prev, u.d_ps);
      hipLaunchKernelGGL(kp_wave, dim3(na), b64, 0, s, u.d_bytes, u.d_desc, u.d_minvals, u.d_minpres, n, t, n_gen, j, rounds,
                         stride, u.d_ps, u.d_vec, u.d_ts, u.d_tg, u.d_tc, ct ? u.d_fts : (sc *)nullptr, u.d_ftg, u.d_ftc,
                         ct ? u.d_exs : (sc *)nullptr, u.d_exg, u.d_exc, ex_back);
    }
    uint8_t *out = (j < rounds) ? u.d_lr + (size_t)j * nb * 64 : u.d_a1b;
    if (j == 0) {  // the witness check joins here: its verdict into the proof's status, its buffer free for the round's MSM
      HIP_CHECK(hipStreamWaitEvent(s, ctx->prove_aux_events[4 * q + 1], 0));
      hipLaunchKernelGGL(kp_check_commitments, dim3(cdiv(nb, 64)), b64, 0, s, u.d_bytes, u.d_desc, u.d_commit32, nb, u.d_ps);
    }
    if (ct && j == rounds) {
      // the final step has no fixed-base MSM: the Pedersen-base terms of A1 and B through the uniform-access tables, A1's two
      // folded generators as 2 x 2^ex_back digit-parallel products over the multiples made above (ct.h), the encodings
      hipLaunchKernelGGL(k_ct_fixed, dim3(2 * nb), b64, 0, s, u.d_fts, u.d_ftg, u.d_ftc, CT_ROW, n_gen, (const niels *)P.fb_ct.p, u.d_ge_ct);
      HIP_CHECK(hipStreamWaitEvent(s, ctx->prove_aux_events[4 * q + 3], 0));
      hipLaunchKernelGGL(k_ct_var, dim3(nb * ex_nt), b64, 0, s, u.d_pow, u.d_fts, CT_ROW, ex_nt, u.d_ctprod);
      hipLaunchKernelGGL(k_ct_sum, dim3(cdiv(nb, 64)), b64, 0, s, u.d_ctprod, ex_nt, nb, u.d_ge_ct, 2u);
      hipLaunchKernelGGL(k_compress_ge, dim3(cdiv(2 * nb, 64)), b64, 0, s, u.d_ge_ct, 2 * nb, u.d_a1b);
      return;
    }
    to_msm(q);
    fb_mark(sm);
    // (the last launch: three outputs per proof in rows of mn + t + 1 terms, see kp_wave_body)
    const bool three = j == rounds;
    const uint32_t n_out = (three ? 3 : 2) * na, row = three ? mn + t + 1 : stride;  // (na = nb in the last launch)
    if (parts) {
      hipLaunchKernelGGL(k_fb_part, dim3(n_out * parts), b64, 0, sm, u.d_ts, u.d_tg, u.d_tc, row, parts, P.fb_table.p, P.fb_geo, u.d_part, 1u);
      // a plain point per output where the consumer is not the fused round kernel: the last launch, the unfused form
      if (j == rounds || !fused) hipLaunchKernelGGL(k_fb_sum, dim3(n_out), b64, 0, sm, u.d_part, parts, u.d_ge);
    } else {
      hipLaunchKernelGGL(k_fb_msm, dim3(n_out), dim3(fb_threads(ctx, mn + t + 1, P.fb_geo)), 0, sm, u.d_ts, u.d_tg, u.d_tc, row, P.fb_table.p,
                         P.fb_geo, u.d_ge, 1u);
    }
    fb_mark(sm);
    to_lane(q);
    if (ct && j + ex_back == rounds) {
      // "ct" = 2: the public points behind the final step's folded generators -- their fixed-base MSM (as much work as a round's L
      // and R), the slices' sums and the 252 doublings that make their multiples by 16^w -- on the sub-batch's side stream,
      // beside the remaining rounds: nothing of it waits for a secret, and nothing secret waits for it before k_ct_var.  Enqueued
      // BEHIND this round's own MSM (the event is recorded after its launch): side by side, the two would share the chip and the
      // round's L and R -- which the chain waits for -- would arrive late by as much as the points' MSM takes (measured: + 0.6 ms
      // per call); behind it, the points' MSM fills the chip while this sub-batch's next step is a lone round kernel, the slot the
      // final step's MSM has without "ct" = 2
      hipStream_t sx = ctx->prove_aux_streams[q];  // (no stream of its own: with several calls in flight every further stream per
                                                   // call is one more tenant of the runtime's hardware queues -- measured: 4 calls x 6
                                                   // streams fall to half the rate of 4 x 4, profiles/r06_ct_inflight.jsonl)
      HIP_CHECK(hipEventRecord(ctx->prove_aux_events[4 * q + 2], sm));
      HIP_CHECK(hipStreamWaitEvent(sx, ctx->prove_aux_events[4 * q + 2], 0));
      fb_mark(sx);
      hipLaunchKernelGGL(k_fb_part, dim3(ex_nt * nb * ex_parts), b64, 0, sx, u.d_exs, u.d_exg, u.d_exc, ex_terms, ex_parts, P.fb_table.p,
                         P.fb_geo, u.d_expart, 1u);
      fb_mark(sx);
      hipLaunchKernelGGL(k_fb_sum, dim3(ex_nt * nb), b64, 0, sx, u.d_expart, ex_parts, u.d_expts);
      hipLaunchKernelGGL(k_ct_pow16, dim3(cdiv(ex_nt * nb, 16)), b64, 0, sx, u.d_expts, ex_nt * nb, u.d_pow);
      HIP_CHECK(hipEventRecord(ctx->prove_aux_events[4 * q + 3], sx));
    }
    if (j == rounds) {  // A1 = A1g + A1h and B
      hipLaunchKernelGGL(kp_final_points, dim3(cdiv(2 * nb, 64)), b64, 0, s, u.d_ge, nb, out);
    } else if (!fused) {
      hipLaunchKernelGGL(k_compress_ge, dim3(cdiv(2 * na, 64)), b64, 0, s, u.d_ge, 2 * na, out);
    }
  }

  // ---- sub-batch q's proofs assembled and on their way out, its arena range zeroed behind them
  void enqueue_finish(uint32_t q) {
    Sub &u = subs[q];
    hipStream_t s = lane_stream(q);
    const uint32_t nb = u.nb;
    if (wants_states())
      hipLaunchKernelGGL(kp_finish<true>, dim3(nb), b64, 0, s, u.d_desc, n, t, nb, rounds, u.d_a32, u.d_lr, u.d_a1b, u.d_vec, u.d_ps,
                         u.d_proofs, (uint32_t)plen, u.d_tstates);
    else
      hipLaunchKernelGGL(kp_finish<false>, dim3(nb), b64, 0, s, u.d_desc, n, t, nb, rounds, u.d_a32, u.d_lr, u.d_a1b, u.d_vec, u.d_ps,
                         u.d_proofs, (uint32_t)plen, (uint32_t *)nullptr);
    HIP_CHECK(hipGetLastError());
    if (r.dev) emit_out(q);
    else copy_out(q);
    // zeroize the device copies of witness-derived data (the reference uses Zeroizing<> for these)
    HIP_CHECK(hipMemsetAsync(arena->p + u.arena_lo, 0, u.arena_len, s));
  }

  // ---- sub-batch q's proofs, status words and made commitments to the page-locked staging ...
  void copy_out(uint32_t q) {
    Sub &u = subs[q];
    hipStream_t s = lane_stream(q);
    const uint32_t nb = u.nb;
    if (r.states203)
      HIP_CHECK(hipMemcpyAsync(pin_tstates + (size_t)u.lo * BPP_STATE_ROW_WORDS, u.d_tstates, (size_t)nb * BPP_STATE_ROW_WORDS * 4,
                               hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipMemcpyAsync(pin_proofs + (size_t)u.lo * plen, u.d_proofs, (size_t)nb * plen, hipMemcpyDeviceToHost, s));
    // only the status word of each (secret-bearing) ProveState leaves the device
    HIP_CHECK(hipMemcpy2DAsync(pin_status + u.lo, sizeof(uint32_t), &u.d_ps[0].status, sizeof(ProveState), sizeof(uint32_t), nb,
                               hipMemcpyDeviceToHost, s));
    if (r.made32)
      HIP_CHECK(hipMemcpyAsync(pin_made + (size_t)u.lo * m * 32, u.d_commit32, (size_t)nb * m * 32, hipMemcpyDeviceToHost, s));
  }
  // ---- ... or scattered into the caller's rows in device memory by k_prove_emit; one outcome record per slot -- a code and a message
  // id, public -- is all that travels to the host
  void emit_out(uint32_t q) {
    Sub &u = subs[q];
    hipStream_t s = lane_stream(q);
    const uint32_t nb = u.nb;
    ProveEmit e;
    memset(&e, 0, sizeof(e));
    e.rows = u.d_rows;
    e.n = nb;
    e.slots = 1;
    e.finding = u.d_finding;
    e.status = (const uint8_t *)&u.d_ps[0].status;
    e.status_stride = (uint32_t)sizeof(ProveState);
    e.proofs = u.d_proofs;
    e.plen = (uint32_t)plen;
    e.commit32 = u.d_commit32;
    e.mslot = m;
    e.proofs_out = r.dev->proofs_out;
    e.proof_stride = r.dev->proof_stride;
    e.commitments_out = r.dev->commitments_out;
    e.commit_stride = r.dev->commit_stride;
    e.status_dev = r.dev->status_dev;
    e.outcome = resident ? nullptr : u.d_outcome;
    e.ok_mask = r.dev->ok_mask;
    e.outcome_item = r.dev->outcome_item;
    e.tstates = u.d_tstates;
    e.tstate_words = BPP_STATE_ROW_WORDS;
    e.states_out = r.dev->states_out;
    hipLaunchKernelGGL(k_prove_emit, dim3(cdiv(nb, BPP_INGEST_BLOCK / BPP_INGEST_LANES)), dim3(BPP_INGEST_BLOCK), 0, s, e);
    HIP_CHECK(hipGetLastError());
    if (resident) return;  // (the outcomes stay on the device: outcome_item, for k_prove_summary)
    HIP_CHECK(hipMemcpyAsync(pin_outcome + u.lo, u.d_outcome, (size_t)nb * sizeof(bpp_device_prove_status), hipMemcpyDeviceToHost, s));
  }

  // ---- Everything is enqueued and this thread has nothing to do for the call's ~6 ms: the host copies of the witness (the packed
  // bytes and their page-locked staging) are wiped NOW, behind the events that say the staging has been read -- not after the
  // call's last kernel, where three megabytes of explicit_bzero were 0.2 ms on the caller's clock.
  void wait_and_wipe() {
    const bool nap = ctx->opt.wait >= 0 ? ctx->opt.wait != 0 : r.n_items >= 256;  // (a call of a few proofs is a latency chain: the runtime's spinning wait)
    for (uint32_t q = 0; q < n_sub; q++) gpu_wait_event(ctx->prove_aux_events[4 * q], nap);
    pk.wipe();
    wipe(ctx->prove_pin_in.p, ctx->prove_pin_in.n);
    staging_clean = true;
    for (uint32_t q = 0; q < n_sub; q++) {
      // (everything of the MSM stream lies in front of the lane stream's tail; the first of these waits is the call's: it remembers how
      // long calls of this context take, sleeps 70 % of that in one piece and -- by the engine's own rule -- looks through the rest
      // without napping: a prover call is something its caller waits FOR (+ 3 % proofs/s one call at a time against naps to the end;
      // "wait" = 1 naps to the end, 0 leaves the whole wait to the runtime's spinning)
      gpu_wait_stream(ctx, lane_stream(q), nap, q == 0 ? &ctx->wait_hint_prove : nullptr, ((uint64_t)B << 32) | ((uint64_t)m << 8) | t, ctx->opt.wait < 0);
      gpu_wait_stream(ctx, ctx->prove_streams[q], nap, nullptr, 0, ctx->opt.wait < 0);
    }
    if (fifo) gpu_wait_stream(ctx, ctx->prove_msm_stream, nap);
    arena_clean = true;  // every sub-batch's arena range was zeroed on its stream
  }

  void profile() {
    bpp_prove_profile &pp = ctx->pprof;
    memset(&pp, 0, sizeof(pp));
    for (size_t k = 0; k + 1 < ev_used; k += 2) {
      float ms = 0;
      HIP_CHECK(hipEventElapsedTime(&ms, ctx->prove_events[k], ctx->prove_events[k + 1]));
      pp.fb_msm_ms += ms;
    }
    pp.total_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    // terms handed to k_fb_msm: witness check m x (1 + t); per round L and R of mn + t + 1 terms each (every generator
    // lands in exactly one of the two); the final step's A1 (every generator once more: 2 mn + t + 1 terms) and B (t + 1)
    pp.fb_terms = (uint64_t)B * ((ct_check ? 0ull : (uint64_t)m * (1 + t)) + (uint64_t)rounds * 2 * (mn + t + 1) + 2 * mn + (ct ? 0u : 2 * t + 2));
    pp.fb_launches = (uint32_t)(ev_used / 2);
    pp.fb_window_bits = P.fb_geo.wbits;
    pp.fb_windows = P.fb_geo.items;  // additions per term
    pp.sub_batches = n_sub;
  }

  // ---- status words -> errors, the made commitments, the transcripts, the self-check, the proofs
  void results() {
    if (r.dev) {  // (the proofs and commitments are where they belong; the entry point sorts the outcomes out)
      r.dev->outcome.assign(pin_outcome, pin_outcome + B);
      return;
    }
    if (!r.dev_status) {
      for (uint32_t i = 0; i < B; i++) {
        if (pin_status[i] & PV_STATUS_COMMIT_MISMATCH) throw ProofErr{BPP_ERR_INVALID_ARGUMENT, "Witness opening is invalid!"};
        if (pin_status[i] & PV_STATUS_TRANSCRIPT)
          throw ProofErr{BPP_ERR_VERIFICATION_FAILED, "Identity element cannot be added to the transcript / zero challenge"};
      }
    }
    // (out of the staging before the self-check, whose remakes reuse it)
    if (r.made32) memcpy(r.made32, pin_made, (size_t)B * m * 32);
    std::vector<uint8_t> tstates(r.states203 ? (size_t)B * 203 : 0);
    for (uint32_t i = 0; r.states203 && i < B; i++) state_row_to_bytes(&tstates[(size_t)i * 203], pin_tstates + (size_t)i * BPP_STATE_ROW_WORDS);
    std::vector<uint8_t> kept_proofs;  // (where the proofs and status words move when a remake needs the staging)
    std::vector<uint32_t> kept_status;
    if (ctx->opt.prove_check > 0)
      prove_self_check(ctx, r.params, P, r.items, B, plen, pin_proofs, pin_status, r.tamper, r.remake, kept_proofs, kept_status, r.made32,
                       (size_t)m * 32, r.states203 ? tstates.data() : nullptr);
    for (uint32_t i = 0; r.states203 && i < B; i++)
      if (pin_status[i] == 0) memcpy(r.states203 + (size_t)i * 203, &tstates[(size_t)i * 203], 203);
    if (r.dev_status) {
      memcpy(r.dev_status, pin_status, (size_t)B * sizeof(uint32_t));
    } else {
      for (uint32_t i = 0; i < B; i++)
        if (pin_status[i] & PV_STATUS_SELF_CHECK) {
          char msg[224];
          snprintf(msg, sizeof(msg), "proof %u failed the engine's self-check: %s", i,
                   (pin_status[i] & PV_STATUS_SELF_CHECK_RECOVERY) ? kSelfCheckRecoveryWhy : kSelfCheckRejectedWhy);
          throw ProofErr{BPP_ERR_SELF_CHECK, msg, BPP_TIER_ENGINE, i};
        }
    }
    for (uint32_t i = 0; i < B; i++) memcpy(r.proofs_out + (size_t)i * r.proof_stride, &pin_proofs[(size_t)i * plen], plen);
  }
};

// The body of bpp_prove_batch and of every other prove call: the stages of ProveCall, in order.
int prove_uniform(bpp_ctx *ctx, const ProveRequest &r, char *errbuf, size_t errbuf_len) {
  try {
    const std::shared_ptr<Params> Pp = params_registry().get(r.params);
    if (!Pp || Pp->device != ctx->device) return fail(ctx, BPP_ERR_BAD_HANDLE, "unknown params handle", errbuf, errbuf_len);
    if ((!r.dev && (!r.items || !r.proofs_out)) || r.n_items == 0) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "null argument", errbuf, errbuf_len);
    ProveCall c(ctx, *Pp, r);
    ScopeExit wipe_secrets{[&] { c.wipe_secrets(); }};
    c.pack();
    c.plan();
    c.carve();
    c.ensure_fb_table();
    c.ensure_streams();
    c.stage_in();
    c.t_begin = std::chrono::steady_clock::now();
    c.arena_clean = false;
    // The sub-batches advance together: every phase is enqueued for all of them before the next one (enqueued one
    // sub-batch after the other, the second stream started ~60 launches late and the call ended with one stream running
    // alone: its latency-bound Fiat-Shamir kernels with nothing beside them).
    for (uint32_t q = 0; q < c.n_sub; q++) c.enqueue_init(q);
    for (uint32_t j = 0; j <= c.rounds; j++)
      for (uint32_t q = 0; q < c.n_sub; q++) c.enqueue_step(j, q);
    for (uint32_t q = 0; q < c.n_sub; q++) c.enqueue_finish(q);
    c.wait_and_wipe();
    if (ctx->profile) c.profile();
    c.results();
    return BPP_OK;
  }
  BPP_CATCH(ctx, errbuf, errbuf_len)
}

// ================================================================= self-check ("prove_check" = 1)
// The proofs a prove call made are verified on the same context before any byte of them leaves the engine: the verifier's own
// upload (upload_host.h) and resident path (verify_chunked_locked / verify_groups_locked), no parser or kernel of its own.  Only public inputs are
// looked at -- the proof bytes and the item's statement and transcript -- and nothing is written but status words.  With
// "prove_check_recovery" = 1 the items that carry a seed nonce take it along and their blinding factors are compared with the masks
// the verifier recovers (check_verify): two secrets the check then holds, in buffers of its own that it wipes before it returns.
//
// Locks: the context's lock is held (the prove call's).  The check does NOT pass the device's small-call gate (GateHold): the gate
// is always taken BEFORE a context's lock, and a thread that holds a context's lock and then waits for the gate deadlocks against
// small verify calls that hold the gate and wait for this context's lock.  A prove call never passes the gate either; its check is
// part of it.

// The test knobs of the context's NEXT prove call (bpp_ctx_set_option), reset as they are taken
bpp_ctx::CheckTamper take_tamper(bpp_ctx *ctx) {
  const bpp_ctx::CheckTamper t = ctx->tamper;
  ctx->tamper = bpp_ctx::CheckTamper{};
  return t;
}

// One verification of the check as ONE reference batch (chunk 0), or -- with `single` -- every proof as a group of its own
// (bpp_verify_resident_groups' path: group_first = 0, 1, ..., n), its code in codes[k].  The batch is the check's own: its
// buffers come from ctx->check_spare and go back there, the caller's resident batches and the spare batch that the caller's next
// upload adopts are left as they were.  Returns 0, or the upload's code when it refuses the batch (a proof of the wrong length, a
// non-canonical scalar: nothing was verified, `codes` untouched), or the verification's finding; an engine fault throws.
//
// blind == nullptr: VerifyOnly, no item carries a seed nonce.  Otherwise ("prove_check_recovery" = 1 and some item of `vi` carries
// one) the verification runs under RecoverAndVerify: k_masks derives the nonces on its own from the uploaded seed nonce and the
// proof's challenges and leaves the recovered masks in the batch's device buffer.  (*blind)[k] != nullptr: the t blinding factors
// of item k's opening; they go through the check's page-locked staging into its device buffer, kp_check_recovery compares them
// with the masks there and one word per such item comes back: (*mismatch)[k] = 1 where they differ (meaningful for the items
// whose verification passed; without `single`, when the whole batch passed).  The recovered masks also pass through the
// verification flow's page-locked mask bytes, which its outcome object wipes; nothing of them is copied anywhere else.
// Wiped before this returns, on every way out: the batch's seed nonces and masks (give_back), the staging of blinding factors.
int check_verify(bpp_ctx *ctx, uint64_t params, const std::vector<bpp_verify_item> &vi, bool single, std::vector<int> *codes,
                 const std::vector<const uint8_t *> *blind = nullptr, std::vector<uint8_t> *mismatch = nullptr) {
  char err[256];
  err[0] = 0;
  uint64_t h = 0;
  hipStream_t s = ctx->stream;
  const int action = blind ? BPP_RECOVER_AND_VERIFY : BPP_VERIFY_ONLY;
  std::swap(ctx->spare_batch, ctx->check_spare);  // (the upload adopts the check's buffers; the caller's spare waits in check_spare)
  ScopeExit give_back{[&] {
    std::unique_ptr<Batch> mine;
    auto it = h ? ctx->batches.find(h) : ctx->batches.end();
    if (it != ctx->batches.end()) {
      (void)hipStreamSynchronize(s);
      Batch &b = *it->second;
      // (a fresh allocation is zeroed once, whether or not this check wrote to it: bpp_prove_secret_bytes reads these buffers)
      if (b.seeds.p != ctx->check_zeroed_seeds || b.seeds.n != ctx->check_zeroed_seeds_n) b.seeds_dirty = true;
      if (b.masks.p != ctx->check_zeroed_masks || b.masks.n != ctx->check_zeroed_masks_n) b.masks_dirty = true;
      wipe_batch_secrets(b, s);  // the items' seed nonces, the recovered masks
      (void)hipStreamSynchronize(s);
      ctx->check_zeroed_seeds = b.seeds.p;
      ctx->check_zeroed_seeds_n = b.seeds.n;
      ctx->check_zeroed_masks = b.masks.p;
      ctx->check_zeroed_masks_n = b.masks.n;
      mine = std::move(it->second);
      ctx->batches.erase(it);
    } else {
      mine = std::move(ctx->spare_batch);  // (the upload refused the batch before it adopted anything)
    }
    ctx->spare_batch = std::move(ctx->check_spare);
    ctx->check_spare = std::move(mine);
  }};
  bool staged = false;
  ScopeExit wipe_staging{[&] {  // (runs before give_back: the batch is still resident, the stream may still be reading the staging)
    if (!staged) return;
    if (ctx->check_dev.p) (void)hipMemsetAsync(ctx->check_dev.p, 0, ctx->check_dev.n, s);
    (void)hipStreamSynchronize(s);
    wipe(ctx->check_pin.p, ctx->check_pin.n);
  }};
  auto compare = [&] {
    Batch &b = *ctx->batches.at(h);
    if (!b.masks_dirty) throw EngineError{BPP_ERR_ENGINE, "self-check: the verification recovered no masks"};
    std::vector<uint32_t> idx;
    for (size_t k = 0; k < vi.size(); k++)
      if ((*blind)[k]) idx.push_back((uint32_t)k);
    const size_t n = idx.size(), row = (size_t)b.params->t * 32;
    mismatch->assign(vi.size(), 0);
    if (n == 0) return;
    ctx->check_pin.resize(n * row + n * 4);
    ctx->check_dev.alloc(n * row + n * 4);
    ctx->check_words.resize(n);
    staged = true;
    for (size_t q = 0; q < n; q++) {
      memcpy(ctx->check_pin.p + q * row, (*blind)[idx[q]], row);
      ctx->check_words[q] = 0xffffffffu;  // (a word the kernel did not write is a difference)
    }
    memcpy(ctx->check_pin.p + n * row, idx.data(), n * 4);
    HIP_CHECK(hipMemcpyAsync(ctx->check_dev.p, ctx->check_pin.p, n * row + n * 4, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(kp_check_recovery, dim3(cdiv((uint32_t)n, 64)), dim3(64), 0, s, b.masks.p, ctx->check_dev.p,
                       (const uint32_t *)(ctx->check_dev.p + n * row), (uint32_t)n, b.params->t, b.B, ctx->check_words.dev());
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(s));
    for (size_t q = 0; q < n; q++) (*mismatch)[idx[q]] = ctx->check_words[q] != 0 ? 1 : 0;
  };
  int rc = upload_impl(ctx, params, vi.data(), vi.size(), nullptr, &h, nullptr, nullptr, err, sizeof(err));
  if (rc < 0) throw ProofErr{rc, err, BPP_TIER_ENGINE};
  if (rc != BPP_OK) return rc;
  // the self-check's verifications run with "verify_check" off: a proof they reject is made again anyway
  ctx->verify_check_off++;
  ScopeExit recheck_back{[&] { ctx->verify_check_off--; }};
  if (!single) {
    rc = verify_chunked_locked(ctx, h, action, 0, nullptr, nullptr, err, sizeof(err));
    if (rc < 0) throw ProofErr{rc, err, BPP_TIER_ENGINE};
    if (rc == BPP_OK && blind) compare();
    return rc;
  }
  std::vector<uint32_t> first(vi.size() + 1);
  for (size_t k = 0; k <= vi.size(); k++) first[k] = (uint32_t)k;
  std::vector<bpp_shard_result> res(vi.size());
  const std::vector<int> actions(vi.size(), action);
  rc = verify_groups_locked(ctx, h, first.data(), vi.size(), blind ? actions.data() : nullptr, res.data(), nullptr, nullptr);
  if (rc != BPP_OK) throw ProofErr{rc < 0 ? rc : BPP_ERR_ENGINE, ctx->err, BPP_TIER_ENGINE};
  for (size_t k = 0; k < vi.size(); k++) (*codes)[k] = res[k].code;
  if (blind) compare();
  return BPP_OK;
}

// The check of one prove_uniform call.  The proofs whose status word is 0 -- at proofs + i * plen, each of its own item's length --
// are verified as ONE reference batch.  When that batch is rejected (the upload refuses it, a PASS-1 finding, a point that does not
// decode, the final MSM), the proofs that fail on their own are located: every proof as a group of its own, or, where the upload
// refused the batch, as one-item verifications.  Each of them is made again, alone, by a one-item prove_uniform with the check on
// (remake = false there): its bytes depend on its item alone, so a device that computes correctly gives the same bytes.  A remake
// that passes replaces the proof; one that fails sets PV_STATUS_SELF_CHECK in the item's status word.  With "prove_check_recovery"
// = 1 a proof the verifier accepts whose replayed mask recovery (check_verify) does not return the witness's blinding factors is a
// finding of the same kind: made again once from the same inputs (nothing is drawn again), failed if its remake's replay differs
// too (PV_STATUS_SELF_CHECK_RECOVERY says which of the two the failure was).  A remake reuses the call's
// staging: the proofs and status words move to kept_* first, and `proofs` / `status` point there afterwards.
// made32 (bpp_prove_openings, else nullptr): the commitments the call computed, item i's at made32 + i * made_stride.  An item that
// brought none is checked against those -- the checking batch never sees a NULL statement -- and its remake makes them again.
void prove_self_check(bpp_ctx *ctx, uint64_t params, const Params &P, const bpp_prove_item *items, uint32_t B, size_t plen, uint8_t *&proofs,
                      uint32_t *&status, const bpp_ctx::CheckTamper &tamper, bool remake, std::vector<uint8_t> &kept_proofs,
                      std::vector<uint32_t> &kept_status, uint8_t *made32, size_t made_stride, uint8_t *tstates203) {
  // (tstates203, else nullptr: the call's advanced transcripts, 203 bytes per item; a remake that passes brings the row of the
  // proof that replaces the first one)
  std::vector<uint32_t> which;  // the items the device made a proof for
  for (uint32_t i = 0; i < B; i++)
    if (status[i] == 0) which.push_back(i);
  if (which.empty()) return;
  // (test knob: a byte of the host copy, never the device's work; with `nonce` a byte of the check's copy of the seed nonce, below)
  if (tamper.proof > 0 && (uint32_t)tamper.proof <= B && tamper.nonce <= 0) {
    const uint32_t i = (uint32_t)tamper.proof - 1;
    if ((size_t)tamper.byte < prove_item_len(P, items[i].m)) proofs[(size_t)i * plen + tamper.byte] ^= (uint8_t)tamper.mask;
  }
  // "prove_check_recovery" = 1: an item's seed nonce travels with it, and its blinding factors are what the recovered masks are
  // compared with (check_verify).  A call none of whose items carries a nonce is checked exactly as without the option.
  const bool recovery = ctx->opt.prove_check_recovery > 0;
  uint8_t nonce_copy[32];  // (test knob "prove_check_tamper_nonce": the check's own copy of one item's nonce, one byte altered)
  ScopeExit wipe_nonce{[&] { wipe(nonce_copy, sizeof(nonce_copy)); }};
  std::vector<bpp_verify_item> vi(which.size());
  std::vector<const uint8_t *> blind(which.size(), nullptr);
  size_t n_nonce = 0;
  for (size_t k = 0; k < which.size(); k++) {
    const bpp_prove_item &it = items[which[k]];
    bpp_verify_item &v = vi[k];
    memset(&v, 0, sizeof(v));
    v.proof = proofs + (size_t)which[k] * plen;
    v.proof_len = prove_item_len(P, it.m);
    v.commitments32 = it.commitments32 ? it.commitments32 : made32 + (size_t)which[k] * made_stride;
    v.m = it.m;
    v.min_values = it.min_values;
    v.min_present = it.min_present;
    // (without the replay the blinding factors stay the prover's secret and mask recovery is not what is checked)
    v.seed_nonce32 = recovery ? it.seed_nonce32 : nullptr;
    if (v.seed_nonce32) {
      blind[k] = it.blindings32;  // (m = 1: one opening, t blinding factors)
      n_nonce++;
      if (tamper.nonce > 0 && tamper.proof == (int)which[k] + 1 && tamper.byte >= 0 && tamper.byte < 32) {
        memcpy(nonce_copy, it.seed_nonce32, 32);
        nonce_copy[tamper.byte] ^= (uint8_t)tamper.mask;
        v.seed_nonce32 = nonce_copy;
      }
    }
    v.transcript_state = it.transcript_state;
    v.transcript_label = it.transcript_label;
    v.label_len = it.transcript_label ? it.label_len : 0;
  }
  const std::vector<const uint8_t *> *replay = n_nonce ? &blind : nullptr;
  std::vector<uint32_t> bad;          // the proofs that fail on their own
  std::vector<uint8_t> bad_recovery;  // ... on the replay of mask recovery (the verifier accepted them)
  {
    // the check leaves no trace on what the context remembers: its own waits (not the prover's nor the caller's verifications'), the
    // caller's last profile and last error
    std::swap(ctx->wait_hint_rng, ctx->check_hint_rng);
    std::swap(ctx->wait_hint_end, ctx->check_hint_end);
    const bpp_profile prof = ctx->prof;
    const std::string err_before = ctx->err;
    ScopeExit restore{[&] {
      std::swap(ctx->wait_hint_rng, ctx->check_hint_rng);
      std::swap(ctx->wait_hint_end, ctx->check_hint_end);
      ctx->prof = prof;
      ctx->err = err_before;
    }};
    if (remake) {
      ctx->check_stats.calls++;
      ctx->check_stats.proofs += which.size();
    }
    // (a remake's own replay is counted no more than its proof is)
    auto replayed = [&](size_t k, bool differs) {
      if (remake) {
        ctx->check_replayed++;
        if (differs) ctx->check_mismatched++;
      }
      if (differs) {
        bad.push_back(which[k]);
        bad_recovery.push_back(1);
      }
    };
    std::vector<uint8_t> mismatch(vi.size(), 0);
    if (check_verify(ctx, params, vi, false, nullptr, replay, &mismatch) == BPP_OK) {
      for (size_t k = 0; replay && k < vi.size(); k++)
        if (blind[k]) replayed(k, mismatch[k] != 0);
      if (bad.empty()) return;
      if (remake) ctx->check_stats.batch_failures++;  // (a recovery that differs is a finding of the checking batch like a rejection)
    } else {
      if (remake) ctx->check_stats.batch_failures++;
      std::vector<int> codes(vi.size(), BPP_OK);
      if (check_verify(ctx, params, vi, true, &codes, replay, &mismatch) != BPP_OK) {  // the upload refused the batch: one-item verifications
        for (size_t k = 0; k < vi.size(); k++) {
          const std::vector<const uint8_t *> one_blind(1, blind[k]);
          std::vector<uint8_t> one_mismatch(1, 0);
          codes[k] = check_verify(ctx, params, std::vector<bpp_verify_item>(1, vi[k]), false, nullptr, blind[k] ? &one_blind : nullptr,
                                  &one_mismatch);
          mismatch[k] = one_mismatch[0];
        }
      }
      for (size_t k = 0; k < vi.size(); k++) {
        if (codes[k] != BPP_OK) {
          bad.push_back(which[k]);
          bad_recovery.push_back(0);
        } else if (blind[k]) {  // (a located proof that passes on its own still has its recovery compared)
          replayed(k, mismatch[k] != 0);
        }
      }
    }
  }
  // (a batch rejected while every proof passes on its own: each proof has then passed a complete verification of its own, and
  // none is made again)
  if (bad.empty()) return;
  if (!remake) {
    for (size_t q = 0; q < bad.size(); q++) status[bad[q]] |= PV_STATUS_SELF_CHECK | (bad_recovery[q] ? PV_STATUS_SELF_CHECK_RECOVERY : 0u);
    return;
  }
  kept_proofs.assign(proofs, proofs + (size_t)B * plen);
  kept_status.assign(status, status + B);
  proofs = kept_proofs.data();
  status = kept_status.data();
  const WaitHint hint = ctx->wait_hint_prove;  // (a remake must not teach the call's wait the time of a one-proof call)
  const bpp_prove_profile pprof = ctx->pprof;
  ScopeExit restore_prove{[&] {
    ctx->wait_hint_prove = hint;
    ctx->pprof = pprof;
  }};
  for (uint32_t i : bad) {
    const size_t len = prove_item_len(P, items[i].m);
    std::vector<uint8_t> one(len, 0);
    uint32_t st = 0;
    size_t got = 0;
    char err[256];
    err[0] = 0;
    bpp_ctx::CheckTamper again{};
    if (tamper.proof == (int)i + 1 && tamper.times >= 2) {
      again = tamper;
      again.proof = 1;
    }
    ctx->check_stats.remade++;
    std::vector<uint8_t> made_one((size_t)32 * items[i].m, 0);
    const ProveRequest one_item{params, &items[i], 1, one.data(), len, &got, &st, false, again, false, made32 ? made_one.data() : nullptr,
                                tstates203 ? tstates203 + (size_t)i * 203 : nullptr};
    const int rc = prove_uniform(ctx, one_item, err, sizeof(err));
    if (rc != BPP_OK) throw ProofErr{rc, err, rc < 0 ? BPP_TIER_ENGINE : BPP_TIER_CONSTRUCTION};
    if (st != 0 || got != len) {  // (which of the two the remake failed on: its own check says)
      status[i] |= PV_STATUS_SELF_CHECK | (st & PV_STATUS_SELF_CHECK_RECOVERY);
      ctx->check_stats.failed++;
    } else {
      memcpy(proofs + (size_t)i * plen, one.data(), len);
      if (made32) memcpy(made32 + (size_t)i * made_stride, made_one.data(), made_one.size());  // (the remake's proof is over the remake's commitments)
    }
  }
}
}  // namespace

extern "C" int bpp_prove_batch(bpp_ctx *ctx, uint64_t params, const bpp_prove_item *items, size_t n_items, uint8_t *proofs_out,
                               size_t proof_stride, size_t *proof_len, char *errbuf, size_t errbuf_len) {
  BPP_ENTRY(ctx);
  const bpp_ctx::CheckTamper tamper = take_tamper(ctx);
  return prove_uniform(ctx, ProveRequest{params, items, n_items, proofs_out, proof_stride, proof_len, nullptr, false, tamper}, errbuf, errbuf_len);
}

// ================================================================= mixed aggregation factors
// bpp_prove_batch_mixed: items of any power-of-two m up to P.m_max in one call.  Every item is checked on its own, in the order a
// one-item bpp_prove_batch checks it (the first finding is its status and message); the items that pass are proved as ONE call of
// ragged launches (prove_uniform with mixed = true, largest m first), whose device-side status words are read item by item.
// A proof's bytes depend on nothing but its own item (its transcript, its witness, its randomness, and the parameters' N, T and
// its own M), so every proof equals the one a bpp_prove_batch of its class would make.  DESIGN.md 4.2 has the choice of this form.
namespace {

const std::string kSelfCheckMsg = std::string("the proof failed the engine's self-check: ") + kSelfCheckRejectedWhy;
const std::string kSelfCheckRecoveryMsg = std::string("the proof failed the engine's self-check: ") + kSelfCheckRecoveryWhy;

struct MixedOutcome {
  std::vector<int> code;
  std::vector<std::string> msg;
};

// The mixed call (the context's lock held, its device current): proof i at proofs_out + i * proof_stride, its length in
// proof_lens[i] (0 for an m that no statement can have), its outcome in out.code[i] / out.msg[i].  A failed item's slot is zeroed.
// Throws only what concerns the whole call (an unknown params handle, a null argument).
// commit_slots (bpp_prove_openings and the pool; nullptr: none of the items is of that kind): (*commit_slots)[i] != nullptr marks
// item i as one of bpp_prove_openings -- it may come without commitments -- and is where its 32 m_i commitment bytes go, a slot of
// (*commit_caps)[i] bytes; an item with a null slot is one of the existing entry points (a pooled call may hold both kinds).
void prove_mixed(bpp_ctx *ctx, uint64_t params, const bpp_prove_item *items, size_t n_items, uint8_t *proofs_out, size_t proof_stride,
                 size_t *proof_lens, MixedOutcome &out, const std::vector<uint8_t *> *commit_slots = nullptr,
                 const std::vector<size_t> *commit_caps = nullptr, uint8_t *states_out203 = nullptr) {
  // states_out203 (bpp_prove_*_states, else nullptr): row i receives item i's advanced transcript when the item succeeds
  const std::shared_ptr<Params> Pp = params_registry().get(params);
  if (!Pp || Pp->device != ctx->device) throw ProofErr{BPP_ERR_BAD_HANDLE, "unknown params handle"};
  const Params &P = *Pp;
  if (!items || n_items == 0 || !proofs_out || !proof_lens) throw ProofErr{BPP_ERR_INVALID_ARGUMENT, "null argument"};
  out.code.assign(n_items, BPP_OK);
  out.msg.assign(n_items, std::string());
  // (what bpp_prove_item_message looks up: left behind by every mixed call, empty where no self-check failed on mask recovery)
  std::vector<std::array<uint8_t, 32>> recovery_failed;
  ScopeExit note{[&] {
    std::lock_guard<std::mutex> lk(ctx->check_note_mu);
    ctx->check_recovery_failed.swap(recovery_failed);
  }};
  std::map<uint32_t, std::vector<uint32_t>, std::greater<uint32_t>> classes;  // m -> the items that passed the host checks
  auto slot = [&](size_t i) -> uint8_t * { return commit_slots ? (*commit_slots)[i] : nullptr; };
  bool any_openings = false;  // (among the items that reach the device)
  for (size_t i = 0; i < n_items; i++) {
    proof_lens[i] = prove_item_len(P, items[i].m);
    try {
      prove_item_check(P, items[i], proof_stride, slot(i) != nullptr, slot(i) ? (*commit_caps)[i] : 0);
      classes[items[i].m].push_back((uint32_t)i);
      any_openings = any_openings || slot(i) != nullptr;
    } catch (const ProofErr &e) {
      out.code[i] = e.code;
      out.msg[i] = e.msg;
    }
  }
  // ONE ragged call over every class, largest aggregation factor first (prove_uniform with mixed = true)
  std::vector<uint32_t> idx;
  for (auto &kv : classes) idx.insert(idx.end(), kv.second.begin(), kv.second.end());
  if (idx.empty()) return;
  std::vector<bpp_prove_item> sub(idx.size());
  for (size_t k = 0; k < idx.size(); k++) sub[k] = items[idx[k]];
  bpp_ctx::CheckTamper tamper = take_tamper(ctx);  // (the knob names the caller's item: here, its place in the sorted call)
  const int tampered = tamper.proof;
  tamper.proof = 0;
  for (size_t k = 0; k < idx.size(); k++)
    if ((int)idx[k] + 1 == tampered) tamper.proof = (int)k + 1;
  const size_t plen = prove_item_len(P, sub[0].m);
  std::vector<uint8_t> buf(idx.size() * plen, 0);
  std::vector<uint32_t> status(idx.size(), 0);
  // what the witness check computed for every item of the sorted call, in rows of the largest m (a call without an item of the
  // new kind asks for nothing and runs exactly as before)
  const size_t made_stride = (size_t)32 * sub[0].m;
  std::vector<uint8_t> made(any_openings ? idx.size() * made_stride : 0, 0);
  char err[256];
  err[0] = 0;
  size_t len = 0;
  std::vector<uint8_t> tstates(states_out203 ? idx.size() * 203 : 0);
  const ProveRequest sorted{params, sub.data(), sub.size(), buf.data(), plen, &len, status.data(), true, tamper, true,
                            any_openings ? made.data() : nullptr, states_out203 ? tstates.data() : nullptr};
  const int rc = prove_uniform(ctx, sorted, err, sizeof(err));
  {
    for (size_t k = 0; k < idx.size(); k++) {
      const uint32_t i = idx[k];
      if (rc != BPP_OK) {  // (an engine fault: every item of the call shares it)
        out.code[i] = rc;
        out.msg[i] = err;
      } else if (status[k] & PV_STATUS_COMMIT_MISMATCH) {
        out.code[i] = BPP_ERR_INVALID_ARGUMENT;
        out.msg[i] = "Witness opening is invalid!";
      } else if (status[k] & PV_STATUS_TRANSCRIPT) {
        out.code[i] = BPP_ERR_VERIFICATION_FAILED;
        out.msg[i] = "Identity element cannot be added to the transcript / zero challenge";
      } else if (status[k] & PV_STATUS_SELF_CHECK) {
        out.code[i] = BPP_ERR_SELF_CHECK;
        out.msg[i] = (status[k] & PV_STATUS_SELF_CHECK_RECOVERY) ? kSelfCheckRecoveryMsg : kSelfCheckMsg;
        if (status[k] & PV_STATUS_SELF_CHECK_RECOVERY) {  // (for bpp_prove_item_message: the item's first commitment, public)
          std::array<uint8_t, 32> c;
          memcpy(c.data(), items[i].commitments32 ? items[i].commitments32 : &made[k * made_stride], 32);  // (or the one made for it)
          recovery_failed.push_back(c);
        }
      } else {
        memcpy(proofs_out + (size_t)i * proof_stride, &buf[k * plen], proof_lens[i]);
        // (status 0: what the check computed IS what the item brought, where it brought any)
        if (slot(i)) memcpy(slot(i), &made[k * made_stride], (size_t)32 * items[i].m);
        if (states_out203) memcpy(states_out203 + (size_t)i * 203, &tstates[k * 203], 203);
      }
    }
  }
  for (size_t i = 0; i < n_items; i++)
    if (out.code[i] != BPP_OK && proof_lens[i] && proof_stride >= proof_lens[i]) memset(proofs_out + i * proof_stride, 0, proof_lens[i]);
  for (size_t i = 0; i < n_items; i++)
    if (out.code[i] != BPP_OK && slot(i) && proof_lens[i] && (*commit_caps)[i] >= (size_t)32 * items[i].m)
      memset(slot(i), 0, (size_t)32 * items[i].m);
}

}  // namespace

namespace {
// The body of the four mixed entry points.  commitments_out (bpp_prove_openings*, else nullptr): an item may come as openings alone.
// An item with commitments32 == NULL has its commitments made by the engine -- the witness check computes commit(v_j, r_j) for
// every opening anyway -- and they are its statement's for the transcript, the proof and the self-check; an item that brings
// commitments is checked against them as ever.  Every successful item's commitments are written at commitments_out + i *
// commit_stride.  states_out203 (bpp_prove_*_states, else nullptr): row i receives item i's advanced transcript.
int prove_mixed_entry(bpp_ctx *ctx, uint64_t params, const bpp_prove_item *items, size_t n_items, uint8_t *commitments_out, size_t commit_stride,
                      uint8_t *proofs_out, size_t proof_stride, size_t *proof_lens, int *item_status, uint8_t *states_out203, char *errbuf,
                      size_t errbuf_len) {
  try {
    std::vector<uint8_t *> slots(commitments_out ? n_items : 0);
    for (size_t i = 0; i < slots.size(); i++) slots[i] = commitments_out + i * commit_stride;
    const std::vector<size_t> caps(slots.size(), commit_stride);
    MixedOutcome out;
    prove_mixed(ctx, params, items, n_items, proofs_out, proof_stride, proof_lens, out, commitments_out ? &slots : nullptr,
                commitments_out ? &caps : nullptr, states_out203);
    if (item_status) memcpy(item_status, out.code.data(), n_items * sizeof(int));
    for (size_t i = 0; i < n_items; i++)
      if (out.code[i] != BPP_OK) return fail(ctx, out.code[i], out.msg[i], errbuf, errbuf_len);
    set_err(errbuf, errbuf_len, "");
    return BPP_OK;
  }
  BPP_CATCH(ctx, errbuf, errbuf_len)
}
}  // namespace

extern "C" int bpp_prove_batch_mixed(bpp_ctx *ctx, uint64_t params, const bpp_prove_item *items, size_t n_items, uint8_t *proofs_out,
                                     size_t proof_stride, size_t *proof_lens, int *item_status, char *errbuf, size_t errbuf_len) {
  BPP_ENTRY(ctx);
  return prove_mixed_entry(ctx, params, items, n_items, nullptr, 0, proofs_out, proof_stride, proof_lens, item_status, nullptr, errbuf, errbuf_len);
}

extern "C" int bpp_prove_batch_mixed_states(bpp_ctx *ctx, uint64_t params, const bpp_prove_item *items, size_t n_items, uint8_t *proofs_out,
                                            size_t proof_stride, size_t *proof_lens, int *item_status, uint8_t *states_out203,
                                            char *errbuf, size_t errbuf_len) {
  BPP_ENTRY(ctx);
  if (!states_out203) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "null argument", errbuf, errbuf_len);
  return prove_mixed_entry(ctx, params, items, n_items, nullptr, 0, proofs_out, proof_stride, proof_lens, item_status, states_out203, errbuf,
                           errbuf_len);
}

extern "C" int bpp_prove_openings(bpp_ctx *ctx, uint64_t params, const bpp_prove_item *items, size_t n_items, uint8_t *commitments_out,
                                  size_t commit_stride, uint8_t *proofs_out, size_t proof_stride, size_t *proof_lens, int *item_status,
                                  char *errbuf, size_t errbuf_len) {
  BPP_ENTRY(ctx);
  if (!commitments_out) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "null argument", errbuf, errbuf_len);
  return prove_mixed_entry(ctx, params, items, n_items, commitments_out, commit_stride, proofs_out, proof_stride, proof_lens, item_status, nullptr,
                           errbuf, errbuf_len);
}

extern "C" int bpp_prove_openings_states(bpp_ctx *ctx, uint64_t params, const bpp_prove_item *items, size_t n_items, uint8_t *commitments_out,
                                         size_t commit_stride, uint8_t *proofs_out, size_t proof_stride, size_t *proof_lens,
                                         int *item_status, uint8_t *states_out203, char *errbuf, size_t errbuf_len) {
  BPP_ENTRY(ctx);
  if (!commitments_out || !states_out203) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "null argument", errbuf, errbuf_len);
  return prove_mixed_entry(ctx, params, items, n_items, commitments_out, commit_stride, proofs_out, proof_stride, proof_lens, item_status,
                           states_out203, errbuf, errbuf_len);
}

// The message that goes with item_status of bpp_prove_batch_mixed: the item's host-side checks run again (no device work), and an
// item that passes them failed on the device, whose two findings have one message each, or the self-check (BPP_ERR_SELF_CHECK).
// Any thread, any time.  The one thing it looks up: whether the item (by its first commitment) is among those of the context's
// last mixed call whose self-check failed on the replay of mask recovery -- the code alone does not say which of the two it was.
namespace {
// openings: an item of bpp_prove_openings (commit_stride: its call's); first_commitment32: what an item that brought no commitments
// is known by -- the first commitment the engine made for it (nullptr for an item that brought its own)
int prove_item_message(bpp_ctx *ctx, uint64_t params, const bpp_prove_item *item, size_t proof_stride, int status, char *errbuf,
                       size_t errbuf_len, bool openings, size_t commit_stride, const uint8_t *first_commitment32) {
  if (!ctx || !item) return BPP_ERR_BAD_HANDLE;
  const std::shared_ptr<Params> Pp = params_registry().get(params);
  if (!Pp || Pp->device != ctx->device) return BPP_ERR_BAD_HANDLE;
  try {
    prove_item_check(*Pp, *item, proof_stride, openings, commit_stride);
  } catch (const ProofErr &e) {
    set_err(errbuf, errbuf_len, e.msg);
    return e.code;
  }
  const uint8_t *key = item->commitments32 ? item->commitments32 : first_commitment32;
  bool recovery = false;
  if (status == BPP_ERR_SELF_CHECK && item->seed_nonce32 && key) {
    std::lock_guard<std::mutex> lk(ctx->check_note_mu);
    for (const auto &c : ctx->check_recovery_failed) recovery = recovery || memcmp(c.data(), key, 32) == 0;
  }
  set_err(errbuf, errbuf_len, status == BPP_ERR_INVALID_ARGUMENT ? "Witness opening is invalid!"
                              : status == BPP_ERR_VERIFICATION_FAILED ? "Identity element cannot be added to the transcript / zero challenge"
                              : status == BPP_ERR_SELF_CHECK ? (recovery ? kSelfCheckRecoveryMsg : kSelfCheckMsg)
                              : "");
  return status;
}
}  // namespace

extern "C" int bpp_prove_item_message(bpp_ctx *ctx, uint64_t params, const bpp_prove_item *item, size_t proof_stride, int status,
                                      char *errbuf, size_t errbuf_len) {
  return prove_item_message(ctx, params, item, proof_stride, status, errbuf, errbuf_len, false, 0, nullptr);
}

// The same for an item of a bpp_prove_openings call.  An item that brought no commitments is known to the lookup by the first
// commitment the engine made for it: the caller passes it (a failed item's slot of commitments_out is zero; commit(v, r) of its
// first opening, bpp_pedersen_commit, is that commitment).  NULL there, or for an item that brought its own: the item's own first.
extern "C" int bpp_prove_openings_item_message(bpp_ctx *ctx, uint64_t params, const bpp_prove_item *item, const uint8_t *first_commitment32,
                                               size_t commit_stride, size_t proof_stride, int status, char *errbuf, size_t errbuf_len) {
  return prove_item_message(ctx, params, item, proof_stride, status, errbuf, errbuf_len, true, commit_stride, first_commitment32);
}

// ================================================================= openings in device memory
// bpp_prove_openings_device (include/bpp.h; prove_ingest.h has the split of the checks and the two kernels).  prove_mixed's shape
// with the witness left where it is: the host checks every item from m[] and the strides, sorts the ones that pass largest m first
// and runs them as ONE ragged call whose source is k_prove_ingest and whose sink is k_prove_emit.  The items it refuses get their
// status record and their zeroed slots from one launch of the emit kernel over a small table, in front of the call.
// bpp_prove_openings_device_transcripts is the same call with one transcript per item IN (item_states: device rows of 203 bytes; the
// pos >= rate finding is then the item's, raised by the ingest kernel, and the call-wide head of every transcript runs on the device)
// and the advanced transcripts OUT (states_out: device rows of 203 bytes, zeros for every item that fails or is refused).
// The blocking calls and the resident plan (engine_prove_plan.h) share the shape step (prove_device_shape, prove_ingest.h) and the
// helpers below: the pointer kinds, the whole-call refusals, the overlap of the two state ranges, the refused items' launch.
namespace {
// one of the call's named arrays that this device cannot reach, in the order of the list (the last three: bpp_prove_enqueue's).
// Empty: nothing to refuse.
std::string prove_arrays_refusal(bpp_ctx *ctx, const bpp_prove_arrays &in, const void *commitments_out, const void *proofs_out,
                                 const void *status_dev, const void *item_states, const void *states_out, const void *live = nullptr,
                                 const void *ok_mask = nullptr, const void *summary = nullptr) {
  const struct {
    const char *name;
    const void *p;
  } arrays[] = {{"values", in.values},
                {"blindings32", in.blindings32},
                {"commitments32", in.commitments32},
                {"min_values", in.min_values},
                {"min_present", in.min_present},
                {"seed_nonces32", in.seed_nonces32},
                {"seed_present", in.seed_present},
                {"rng_bytes", in.rng_bytes},
                {"commitments_out_dev", commitments_out},
                {"proofs_out_dev", proofs_out},
                {"status_dev", status_dev},
                {"item_states_dev", item_states},
                {"states_out_dev", states_out},
                {"live_dev", live},
                {"ok_mask_dev", ok_mask},
                {"summary_dev", summary}};
  for (const auto &a : arrays) {
    if (!a.p) continue;
    const int kind = device_pointer_kind(ctx->device, a.p);
    if (kind != BPP_PTR_THIS_DEVICE)
      return std::string(a.name) + " is not device memory of this context's device (" + upload_pointer_kinds[kind] + ")";
  }
  return std::string();
}

// n_rows rows of item_states_dev and of states_out_dev share a byte (either may be null: no overlap)
bool prove_states_overlap(const uint8_t *item_states, const uint8_t *states_out, size_t n_rows) {
  const uintptr_t a = (uintptr_t)item_states, b = (uintptr_t)states_out, len = (uintptr_t)n_rows * BPP_ITEM_STATE_BYTES;
  return item_states && states_out && a < b + len && b < a + len;
}

// What the blocking calls and bpp_prove_plan_create refuse of a whole call behind their own null checks, in this order; BPP_OK with
// the parameters in Pp: nothing to refuse.  per_item: one transcript per item (item_states_dev, or the plan's flag); states_out: the
// blocking call's (a plan has no rows yet).  The overlap cannot coincide with the state's position -- it needs item_states, under
// which a transcript_state is refused before -- but it can with the two refusals behind it.  m[] is not read here.
int prove_device_refusals(bpp_ctx *ctx, uint64_t params, const bpp_prove_arrays &in, bool per_item, const uint8_t *item_states,
                          const uint8_t *states_out, std::shared_ptr<Params> &Pp, char *errbuf, size_t errbuf_len) {
  if (device_pointer_kind(ctx->device, in.m) != BPP_PTR_HOST_OR_UNKNOWN)
    return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "m must be host memory: it sizes the call's layout", errbuf, errbuf_len);
  if (in.m_stride == 0) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "m_stride is 0", errbuf, errbuf_len);
  if (ctx->opt.prove_check > 0)
    return fail(ctx, BPP_ERR_INVALID_ARGUMENT,
                "prove_check = 1 is not supported by bpp_prove_openings_device: the self-check remakes from host items; verify the outputs "
                "with bpp_verify_batch_mixed_device",
                errbuf, errbuf_len);
  if (per_item && (in.transcript_state || in.transcript_label))
    return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "transcript_state / transcript_label must be null: item i continues row i of item_states_dev",
                errbuf, errbuf_len);
  if (in.transcript_state && in.transcript_state[200] >= BPP_STROBE_R)
    return fail(ctx, prove_err(BPP_PROVE_MSG_TRANSCRIPT_STATE).code, prove_msg_text(BPP_PROVE_MSG_TRANSCRIPT_STATE), errbuf, errbuf_len);
  // (n_items <= 2^24 is checked below: a range is at most a few gigabytes, no overflow here)
  if (prove_states_overlap(item_states, states_out, std::min<size_t>(in.n_items, (size_t)1 << 24)))
    return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "item_states_dev and states_out_dev overlap", errbuf, errbuf_len);
  Pp = params_registry().get(params);
  if (!Pp || Pp->device != ctx->device) return fail(ctx, BPP_ERR_BAD_HANDLE, "unknown params handle", errbuf, errbuf_len);
  if (in.n_items > (1u << 24)) return fail(ctx, BPP_ERR_SIZE_OVERFLOW, "batch too large", errbuf, errbuf_len);
  return BPP_OK;
}

// the refused items' records and zeroed slots: one launch of the emit kernel over their table (device memory, n rows) in front of
// the call's own launches.  A refused item's state row is zeroed: its rows carry their finding.
void launch_prove_refused(hipStream_t s, const ProveDevRow *rows_dev, uint32_t n, const ProveDeviceIO &io) {
  ProveEmit e;
  memset(&e, 0, sizeof(e));
  e.rows = rows_dev;
  e.n = n;
  e.proofs_out = io.proofs_out;
  e.proof_stride = io.proof_stride;
  e.commitments_out = io.commitments_out;
  e.commit_stride = io.commit_stride;
  e.status_dev = io.status_dev;
  e.states_out = io.states_out;
  e.ok_mask = io.ok_mask;
  e.outcome_item = io.outcome_item;
  hipLaunchKernelGGL(k_prove_emit, dim3(cdiv(n, BPP_INGEST_BLOCK / BPP_INGEST_LANES)), dim3(BPP_INGEST_BLOCK), 0, s, e);
  HIP_CHECK(hipGetLastError());
}

int prove_openings_device(bpp_ctx *ctx, uint64_t params, const bpp_prove_arrays *in, uint8_t *commitments_out, size_t commit_stride,
                          uint8_t *proofs_out, size_t proof_stride, size_t *proof_lens, bpp_device_prove_status *status_dev, int *item_status,
                          char *errbuf, size_t errbuf_len, const uint8_t *item_states = nullptr, uint8_t *states_out = nullptr) {
  try {
    if (!in) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "null argument", errbuf, errbuf_len);
    // pointer kinds first: nothing is allocated or launched for an array this device cannot reach, and no array is ever
    // dereferenced on the host
    if (!commitments_out) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "commitments_out_dev is null", errbuf, errbuf_len);
    if (!proofs_out) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "proofs_out_dev is null", errbuf, errbuf_len);
    const std::string why = prove_arrays_refusal(ctx, *in, commitments_out, proofs_out, status_dev, item_states, states_out);
    if (!why.empty()) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, why, errbuf, errbuf_len);
    if (!in->m || in->n_items == 0 || !proof_lens) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "null argument", errbuf, errbuf_len);
    std::shared_ptr<Params> Pp;
    if (const int rc = prove_device_refusals(ctx, params, *in, item_states != nullptr, item_states, states_out, Pp, errbuf, errbuf_len)) return rc;
    const size_t n_items = in->n_items;

    // the host's part of the checks, per item; the ones that pass by aggregation factor, largest first, in the caller's order
    ProveDeviceIO io{in, {}, commitments_out, commit_stride, proofs_out, proof_stride, status_dev, {}};
    io.item_states = item_states;
    io.states_out = states_out;
    ProveDeviceShape &sh = io.shape;
    const bool fields_ok = in->values && in->blindings32 && in->rng_bytes && (in->min_values || !in->min_present);
    const bool fits = prove_device_shape(ParamShape{Pp->n_bits, Pp->m_max, Pp->t}, in->m, n_items, in->m_stride, in->rng_stride, proof_stride,
                                         commit_stride, fields_ok, sh);
    std::copy_n(sh.proof_lens.begin(), fits ? n_items : sh.m_stride_below + 1, proof_lens);
    if (!fits) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "m_stride is below an aggregation factor", errbuf, errbuf_len);
    std::vector<uint32_t> &msg = sh.msg;
    struct bpp_prove_device_stats &stats = ctx->prove_dev_stats;
    stats.calls++;
    stats.items += n_items;
    stats.host_findings += sh.refused.size();
    hipStream_t s = ctx->stream;
    if (!sh.refused.empty()) {
      ctx->prove_dev_refused.alloc(sh.refused.size() * sizeof(ProveDevRow));
      HIP_CHECK(hipMemcpyAsync(ctx->prove_dev_refused.p, sh.refused.data(), sh.refused.size() * sizeof(ProveDevRow), hipMemcpyHostToDevice, s));
      launch_prove_refused(s, (const ProveDevRow *)ctx->prove_dev_refused.p, (uint32_t)sh.refused.size(), io);
      HIP_CHECK(hipStreamSynchronize(s));  // (the table is pageable host memory of this frame)
    }

    std::string engine_err;
    int engine_rc = BPP_OK;
    if (!sh.rows.empty()) {
      (void)take_tamper(ctx);  // (the self-check's test knobs name a call that checks: this one does not)
      char err[256];
      err[0] = 0;
      ProveRequest req{params, nullptr, sh.rows.size(), nullptr, 0, nullptr};
      req.mixed = true;
      req.dev = &io;
      engine_rc = prove_uniform(ctx, req, err, sizeof(err));
      engine_err = err;
      for (size_t k = 0; k < sh.rows.size(); k++) {
        const uint32_t i = sh.rows[k].item;
        msg[i] = engine_rc != BPP_OK ? BPP_PROVE_MSG_ENGINE : io.outcome[k].msg;
        if (engine_rc == BPP_OK && msg[i] >= BPP_PROVE_MSG_SEED_AGGREGATED && msg[i] <= BPP_PROVE_MSG_TRANSCRIPT_STATE) stats.device_findings++;
      }
    }
    for (size_t i = 0; item_status && i < n_items; i++) item_status[i] = msg[i] == BPP_PROVE_MSG_ENGINE ? engine_rc : prove_msg_code(msg[i]);
    for (size_t i = 0; i < n_items; i++) {
      if (msg[i] == BPP_PROVE_MSG_ENGINE) return fail(ctx, engine_rc, engine_err, errbuf, errbuf_len);
      if (msg[i]) return fail(ctx, prove_msg_code(msg[i]), prove_msg_text(msg[i]), errbuf, errbuf_len);
    }
    set_err(errbuf, errbuf_len, "");
    return BPP_OK;
  }
  BPP_CATCH(ctx, errbuf, errbuf_len)
}
}  // namespace

extern "C" int bpp_prove_openings_device(bpp_ctx *ctx, uint64_t params, const bpp_prove_arrays *in_dev, uint8_t *commitments_out_dev,
                                         size_t commit_stride, uint8_t *proofs_out_dev, size_t proof_stride, size_t *proof_lens,
                                         bpp_device_prove_status *status_dev, int *item_status, char *errbuf, size_t errbuf_len) {
  BPP_ENTRY(ctx);
  return prove_openings_device(ctx, params, in_dev, commitments_out_dev, commit_stride, proofs_out_dev, proof_stride, proof_lens, status_dev,
                               item_status, errbuf, errbuf_len);
}

extern "C" int bpp_prove_openings_device_transcripts(bpp_ctx *ctx, uint64_t params, const bpp_prove_arrays *in_dev, const uint8_t *item_states_dev,
                                                     uint8_t *commitments_out_dev, size_t commit_stride, uint8_t *proofs_out_dev,
                                                     size_t proof_stride, size_t *proof_lens, uint8_t *states_out_dev,
                                                     bpp_device_prove_status *status_dev, int *item_status, char *errbuf, size_t errbuf_len) {
  BPP_ENTRY(ctx);
  return prove_openings_device(ctx, params, in_dev, commitments_out_dev, commit_stride, proofs_out_dev, proof_stride, proof_lens, status_dev,
                               item_status, errbuf, errbuf_len, item_states_dev, states_out_dev);
}

extern "C" int bpp_prove_status_result(const bpp_device_prove_status *host_copy, bpp_shard_result *out) {
  if (!host_copy || !out || host_copy->msg > BPP_PROVE_MSG_EMPTY) return BPP_ERR_INVALID_ARGUMENT;
  memset(out, 0, sizeof(*out));
  // (BPP_PROVE_MSG_EMPTY, a slot bpp_prove_enqueue's live mask switched off, is no finding: code 0, no tier, no text)
  const bool finding = host_copy->msg != BPP_PROVE_MSG_OK && host_copy->msg != BPP_PROVE_MSG_EMPTY;
  shard_result_set(*out, host_copy->code, finding ? BPP_TIER_CONSTRUCTION : BPP_TIER_NONE, -1, 0, prove_msg_text(host_copy->msg));
  return BPP_OK;
}

extern "C" int bpp_prove_device_stats(bpp_ctx *ctx, struct bpp_prove_device_stats *out) {
  BPP_ENTRY(ctx);
  if (!out) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "null argument");
  *out = ctx->prove_dev_stats;
  return BPP_OK;
}

#ifdef BPP_KP_PHASES
// measurement build only (tools/gpu_kp_phases.sh): the summed shader-clock cycles per phase of kp_round; reset != 0 clears them
extern "C" int bpp_debug_kp_phases(unsigned long long out[32], int reset) {
  if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(bpp::g_kp_phase), sizeof(unsigned long long) * 32) != hipSuccess) return -1;
  if (reset) {
    unsigned long long z[32] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(bpp::g_kp_phase), z, sizeof(z)) != hipSuccess) return -1;
  }
  return 0;
}
#endif
