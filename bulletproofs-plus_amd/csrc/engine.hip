// libbpp_hip.so -- host side of the C ABI in include/bpp.h.  No CPU fallback: every entry point needs a gfx950 device.
//
// Host responsibilities (mirroring what the reference does around its hot loops):
//   * argument / wire-format checks with the reference's error kinds and precedence
//     (src/range_proof.rs:719-734, :610-709, :875-888, :1155-1257; src/range_statement.rs:36-73)
//   * packing a batch into the HBM layout documented in kernels_verify.h
//   * the batch-weight transcript (src/range_proof.rs:811,849,853,894): a sequential sponge, run on the host
//   * SHAKE256 / SHA3-512 byte streams for generator derivation (src/generators/generators_chain.rs:23-33,
//     src/protocols/curve_point_protocol.rs:31-35); the hash-to-group map itself runs on the device
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <time.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <map>
#include <set>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/bpp.h"
#include "chain_dev.h"
#include "chain_host.h"
#include "ct.h"
#include "kernels_prove.h"
#include "kernels_verify.h"
#include "lanes_host.h"
#include "msm.h"
#include "msm_plain.h"
#include "prove_job_host.h"
#include "prove_pack_host.h"
#include "runtime_host.h"
#include "upload_host.h"
#include "ingest.h"
#include "ingest_mixed.h"
#include "verdict.h"
#include "refill.h"
#include "item_states.h"
#include "prove_ingest.h"
#include "transcript_ops.h"
#include "rows_msm.h"

using namespace bpp;

namespace {

// ------------------------------------------------------------------ utilities
struct EngineError {
  int code;
  std::string msg;
};

#define HIP_CHECK(expr)                                                                          \
  do {                                                                                           \
    hipError_t _e = (expr);                                                                      \
    if (_e != hipSuccess) {                                                                      \
      char _b[256];                                                                              \
      snprintf(_b, sizeof(_b), "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
      throw EngineError{BPP_ERR_ENGINE, _b};                                                     \
    }                                                                                            \
  } while (0)

template <typename T>
struct DevBuf {
  T *p = nullptr;
  size_t n = 0;
  DevBuf() {}
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
  void alloc(size_t count) {
    if (count <= n && p) return;
    release();
    if (count == 0) count = 1;
    HIP_CHECK(hipMalloc((void **)&p, count * sizeof(T)));
    n = count;
  }
  void swap(DevBuf &o) {
    std::swap(p, o.p);
    std::swap(n, o.n);
  }
};

// page-locked host memory: asynchronous copies to/from it do not stall other streams or host threads.  It is also MAPPED
// into the device's address space (coherent, never cached by the GPU): the verifier's kernels write their small results --
// transcript-RNG bytes, status words, identity flags, masks -- straight into it and read the batch weights from it, so a
// verification enqueues no copy at all (each hipMemcpyAsync of a few KB ran as a blit kernel of its own that queued behind
// the other steps' 15 k-wavefront launches: five per step, 0.19 ms each with four steps in flight, two of them on the
// PASS 1 -> weight chain -> PASS 2 critical path)
template <typename T>
struct PinnedBuf {
  T *p = nullptr;
  T *d = nullptr;  // the same memory as the device sees it
  size_t n = 0;
  PinnedBuf() {}
  PinnedBuf(const PinnedBuf &) = delete;
  PinnedBuf &operator=(const PinnedBuf &) = delete;
  ~PinnedBuf() {
    if (p) (void)hipHostFree(p);
  }
  void resize(size_t count) {
    if (count <= n && p) return;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    d = nullptr;
    if (count == 0) count = 1;
    HIP_CHECK(hipHostMalloc((void **)&p, count * sizeof(T), hipHostMallocMapped | hipHostMallocPortable));
    HIP_CHECK(hipHostGetDevicePointer((void **)&d, p, 0));
    n = count;
  }
  T *dev() { return d; }
  T *data() { return p; }
  const T *data() const { return p; }
  T &operator[](size_t i) { return p[i]; }
  const T &operator[](size_t i) const { return p[i]; }
  void swap(PinnedBuf &o) {
    std::swap(p, o.p);
    std::swap(d, o.d);
    std::swap(n, o.n);
  }
};

// runs on every exit path of a scope (return, ProofErr, EngineError): used to wipe secret-bearing buffers, as the
// reference does with Zeroizing<> (src/range_proof.rs:300-301,325,438-464, src/commitment_opening.rs:14)
struct ScopeExit {
  std::function<void()> f;
  ~ScopeExit() {
    if (f) f();
  }
};
inline void wipe(void *p, size_t n) {
  if (p && n) explicit_bzero(p, n);
}

// a row of BPP_STATE_ROW_WORDS words as the kernels write an advanced transcript (kernels_verify.h) -> the ABI's 203 bytes
inline void state_row_to_bytes(uint8_t *out203, const uint32_t *row) {
  memcpy(out203, row, 200);  // little-endian host, as everywhere in this file
  out203[200] = (uint8_t)row[50];
  out203[201] = (uint8_t)(row[50] >> 8);
  out203[202] = (uint8_t)(row[50] >> 16);
}

// a lane's counters into a sum over lanes (contexts' own, a pipeline's, a pool's)
inline void add_stats(struct bpp_prove_check_stats &sum, const struct bpp_prove_check_stats &s) {
  sum.calls += s.calls;
  sum.proofs += s.proofs;
  sum.batch_failures += s.batch_failures;
  sum.remade += s.remade;
  sum.failed += s.failed;
}
inline void add_stats(struct bpp_verify_joint_stats &sum, const struct bpp_verify_joint_stats &s) {
  sum.calls += s.calls;
  sum.accepted += s.accepted;
  sum.fallbacks += s.fallbacks;
  sum.fallback_all_ok += s.fallback_all_ok;
}
inline void add_stats(struct bpp_verify_check_stats &sum, const struct bpp_verify_check_stats &s) {
  sum.calls += s.calls;
  sum.rechecked_groups += s.rechecked_groups;
  sum.confirmed += s.confirmed;
  sum.overturned += s.overturned;
  sum.tie_breaks += s.tie_breaks;
  sum.undecided += s.undecided;
}
// a context's self-check counters added to a sum over lanes (the prove pool's, the prove pipeline's); the context's code
inline int add_check_stats(bpp_ctx *c, struct bpp_prove_check_stats &sum) {
  struct bpp_prove_check_stats s;
  const int rc = bpp_prove_check_stats(c, &s);
  if (rc == BPP_OK) add_stats(sum, s);
  return rc;
}
inline int add_recovery_stats(bpp_ctx *c, uint64_t &replayed, uint64_t &mismatched) {
  uint64_t r = 0, m = 0;
  const int rc = bpp_prove_check_recovery_stats(c, &r, &m);
  replayed += rc == BPP_OK ? r : 0;
  mismatched += rc == BPP_OK ? m : 0;
  return rc;
}

void set_err(char *errbuf, size_t len, const std::string &m) {
  if (errbuf && len) {
    snprintf(errbuf, len, "%s", m.c_str());
  }
}

// ------------------------------------------------------------------ host hashing helpers (keccak from merlin.h)
void keccak_sponge(const uint8_t *in, size_t inlen, uint8_t *out, size_t outlen, uint32_t rate, uint8_t pad) {
  uint64_t st[25];
  memset(st, 0, sizeof(st));
  uint8_t *sb = (uint8_t *)st;  // little-endian host
  size_t off = 0;
  while (inlen - off >= rate) {
    for (uint32_t i = 0; i < rate; i++) sb[i] ^= in[off + i];
    keccak_f1600(st);
    off += rate;
  }
  for (size_t i = 0; i < inlen - off; i++) sb[i] ^= in[off + i];
  sb[inlen - off] ^= pad;
  sb[rate - 1] ^= 0x80;
  keccak_f1600(st);
  size_t o = 0;
  while (o < outlen) {
    size_t take = (outlen - o < rate) ? outlen - o : rate;
    memcpy(out + o, sb, take);
    o += take;
    if (o < outlen) keccak_f1600(st);
  }
}
void shake256(const uint8_t *in, size_t inlen, uint8_t *out, size_t outlen) { keccak_sponge(in, inlen, out, outlen, 136, 0x1f); }
void sha3_512(const uint8_t *in, size_t inlen, uint8_t out[64]) { keccak_sponge(in, inlen, out, 64, 72, 0x06); }

// ------------------------------------------------------------------ objects
// RangeParameters / Precomputation objects are process-wide, reference-counted and read-only once built (the reference
// shares them through Arc, `Precomputation: Send + Sync`, src/traits.rs:42, src/generators/bulletproof_gens.rs:52,103):
// any context of the same device may use a handle concurrently; only work buffers are per context.
struct Params {
  int device = 0;
  std::mutex fb_mu;  // serialises the one-off build of the prover's fixed-base table
  uint32_t n_bits, m_max, t;
  DevBuf<niels> table;  // [2*n*m_max interleaved G,H | t g_bases | h_base]
  DevBuf<niels> table_hi;  // the same points times 2^126: the half-scalar MSM plan of small calls (msm.h)
  uint32_t table_len;
  DevBuf<uint8_t> d_hg32;           // compressed H, G_0..G_{t-1}
  std::vector<uint8_t> hg32;        // host copy
  std::vector<uint8_t> gi32, hi32;  // compressed generators, party-major
  DevBuf<fbent> fb_table;           // prover's fixed-base window table, built on first use (geometry fb_geo)
  FbGeom fb_geo{}, fb_ped_geo{};
  DevBuf<fbent> fb_ped;             // same for the Pedersen bases only [G_0..G_{t-1}, H], always resident (commit)
  DevBuf<fbent> fb_ct;              // the Pedersen bases' 4-bit lines for the uniform-access form (ct.h: k_ct_fixed), [base][64][8]
};

struct Precomp {
  int device = 0;
  DevBuf<niels> table;
  uint32_t count;
};

template <typename T>
struct SharedRegistry {
  struct Entry {
    std::shared_ptr<T> obj;
    uint32_t refs;
  };
  std::mutex mu;
  std::map<uint64_t, Entry> live;
  uint64_t add(std::shared_ptr<T> o);
  std::shared_ptr<T> get(uint64_t h) {
    std::lock_guard<std::mutex> lk(mu);
    auto it = live.find(h);
    return it == live.end() ? nullptr : it->second.obj;
  }
  bool retain(uint64_t h) {
    std::lock_guard<std::mutex> lk(mu);
    auto it = live.find(h);
    if (it == live.end()) return false;
    it->second.refs++;
    return true;
  }
  // drops one reference; the object itself lives on while a call or a resident batch still holds its shared_ptr
  bool release(uint64_t h) {
    std::shared_ptr<T> dying;
    std::lock_guard<std::mutex> lk(mu);
    auto it = live.find(h);
    if (it == live.end()) return false;
    if (--it->second.refs == 0) {
      dying = std::move(it->second.obj);
      live.erase(it);
    }
    return true;
  }
};
std::atomic<uint64_t> g_next_handle{1};
template <typename T>
uint64_t SharedRegistry<T>::add(std::shared_ptr<T> o) {
  const uint64_t h = g_next_handle.fetch_add(1);
  std::lock_guard<std::mutex> lk(mu);
  live[h] = Entry{std::move(o), 1};
  return h;
}
SharedRegistry<Params> &params_registry() {
  static SharedRegistry<Params> *r = new SharedRegistry<Params>();  // leaked: contexts may outlive static destruction
  return *r;
}
SharedRegistry<Precomp> &precomp_registry() {
  static SharedRegistry<Precomp> *r = new SharedRegistry<Precomp>();
  return *r;
}

// calls of up to this many proofs are "small" for the gate (their MSM has at most ~20 000 terms: BPP_SMALL_CALL_TERMS)
#define BPP_GATE_SMALL_PROOFS 1024u
// proof + commitment bytes of an upload up to this size travel with the small arrays in k_ingest; above it by DMA
#define BPP_INGEST_MAX_BYTES (1u << 20)

struct MsmWork {
  DevBuf<uint32_t> counts, starts, sorted, order, order_win, cls_hist;
  DevBuf<ge> buckets, Q, W, R;
  DevBuf<uint8_t> comp32;
  DevBuf<uint32_t> is_identity;
  DevBuf<uint32_t> term_sidx, term_pidx, group_off;
  MsmPlan plan{};
  uint32_t max_group_terms = 0;
  bool split = false;  // half-scalar plan (small verifier calls): every term twice, 127-bit windows
  // the plain MSM (msm_plain.h: "msm_plain" = 1, pass 2 of "verify_check"): the group offsets as the host made them, one partial
  // sum per wavefront, the ids of the groups to evaluate (mapped: the kernels read them where the host wrote them)
  std::vector<uint32_t> h_goff;
  // the sliced prelude (msm.h: k_msm_slice_*): slices per (group, window) sort, 0 = the one-workgroup form; per-slice bucket
  // histograms, turned into write offsets in place
  uint32_t slices = 0;
  DevBuf<uint32_t> slice_hist;
  DevBuf<ge> plain_part;
  PinnedBuf<uint32_t> plain_list;
};

struct Batch {
  std::shared_ptr<Params> params;
  uint64_t params_handle = 0;
  uint32_t B = 0, rmax = 0, cs = 0, max_mn = 0, total_dyn = 0, sum_m = 0, cols = 0;
  // shape of the per-proof table block of the scalar stage (kernels_verify.h: lanes_tab_stride)
  // A proof that claims more rounds than its statement's m * n_bits has bits is refused on the host; the table blocks are
  // sized for the statements (max_mn), so that one such proof cannot inflate the allocation of the whole batch.
  uint32_t lanes_nhi_max(uint32_t n_bits) const {
    uint32_t cap = 0;
    while ((2u << cap) <= std::max<uint32_t>(max_mn, 1)) cap++;  // floor(log2(max_mn))
    const uint32_t rm = std::min({rmax, (uint32_t)BPP_MAX_ROUNDS - 1, cap}), lb = lanes_lb(n_bits);
    return 1u << (rm > lb ? rm - lb : 0);
  }
  std::vector<ProofDesc> desc;
  std::vector<uint8_t> rounds_bad;  // 0 ok, 3 InvalidLength, 5 SizeOverflow  (src/range_proof.rs:875-888)
  std::vector<uint8_t> defer;       // BPP_DEFER_* findings of verify()'s consistency loops (:637-682), raised per chunk
  bool any_seed = false, any_rounds_bad = false, any_defer = false, ext_challenges = false, uniform_rounds = true;
  std::vector<uint32_t> ext_status;
  DevBuf<uint32_t> d_ext_status;
  // device-resident inputs
  DevBuf<uint8_t> bytes, states, seeds;
  DevBuf<ProofDesc> d_desc;
  DevBuf<uint64_t> minvals;
  DevBuf<uint32_t> src_off, owner;
  DevBuf<uint32_t> idx_commit, idx_proof, status0;  // dynamic slots of the commitments / of the proof points; initial status
  // device work buffers
  DevBuf<sc> chal, rows, scal, shr, tab;
  DevBuf<uint64_t> parts;      // per-workgroup limb sums of the generator columns (k_scalars_lanes -> k_reduce_parts)
  bool fused_columns = false;  // this layout sums the generator columns inside k_scalars_lanes (layout_groups decides)
  uint32_t lanes_ppw = 1;      // proofs per workgroup of k_scalars_lanes for this batch
  // generator columns as a matrix product over the proofs of a group (kernels_static_gemm.h): digit tables, anti-diagonal sums
  DevBuf<int8_t> gemm_lo, gemm_hi;
  DevBuf<int32_t> gparts;
  DevBuf<sc> gemm_mult;        // per proof: w, -w e^2 (Montgomery), -w e^2, -w e^2 y^(mn+1) (canonical), the weight as it came
  bool static_gemm = false;    // this layout takes the generator columns from k_static_gemm (plan_lanes decides)
  uint32_t gemm_nkc = 1;       // K chunks (256 proofs each) of the largest group
  int uniform_mn = -1;         // -1 not looked at yet; 0 the proofs differ in shape; else the common m * n_bits
  bool gemm_hi_ready = false;  // the last k_scalars_shared of this batch wrote the high digit tables
  DevBuf<uint8_t> rng_out, weights, masks, chal_bytes;
  DevBuf<uint32_t> chain_wide;  // device chain: the 64 PRF bytes per proof as k_weight_chain leaves them (chain_dev.h)
  DevBuf<uint32_t> status, group_first, group_dlo;
  DevBuf<uint32_t> dec_spill;  // k_decompress parks three field elements per proof point here across its squaring chain
  DevBuf<niels> dynpts;
  DevBuf<pniels> dyn_hi;  // 2^126 x dynpts as projective Niels entries (half-scalar plan only)
  MsmWork msm;
  // "verify_joint" = 1: the one-group MSM over all reference batches of the call (kernels_verify.h: k_joint_row), planned by
  // layout_groups beside the per-group one.  joint_G: the group count its term lists were written for (0: none);
  // need_dyn_hi: a plan the pass may run is a half-scalar one; joint_ran: a pass took the joint path and msm_joint holds its result;
  // joint_accepted: the last MSM this batch ran was an accepted joint check, so msm holds no results of it (bpp_batch_trace)
  MsmWork msm_joint;
  uint32_t joint_G = 0;
  bool need_dyn_hi = false, joint_ran = false, joint_accepted = false;
  // layout of the last verify
  size_t last_chunk = (size_t)-1;
  uint32_t G = 0;
  std::vector<uint32_t> h_group_first;
  PinnedBuf<uint8_t> h_rng, h_weights, h_masks;  // mapped: written / read by the kernels directly (PinnedBuf)
  PinnedBuf<uint8_t> h_masks_check;  // "verify_check": where passes 2 and 3 leave their masks (verify_flow wipes it before it returns)
  PinnedBuf<uint8_t> h_wide;  // chain mode 2: the host sponges' 64 bytes per proof, reduced on the device
  PinnedBuf<uint32_t> h_status, h_ident;
  // bpp_verify_*_states: the advanced transcripts as PASS 1 writes them, rows of BPP_STATE_ROW_WORDS words (mapped, public data);
  // allocated by the first call that asks for them, written only while want_states is set (verify_chunked_locked)
  PinnedBuf<uint32_t> h_states;
  bool want_states = false;
  // k_results_out writes one summary word per BPP_STATUS_BLOCK proofs and a block's words only when there is something in them;
  // settle_status() makes h_status whole again on the host (a block the kernel skipped is all zero: cleared here if it was not)
  PinnedBuf<uint32_t> h_status_any;
  std::vector<uint8_t> h_status_dirty;
  const uint32_t *h_status_dirty_of = nullptr;  // the allocation those flags describe (a re-allocated h_status holds anything)
  bool status_settled = true;
  bool have_trace = false, phase1_done = false;
  bool status_clean = false;     // status[] == status0[]: k_results_out resets it behind every verification
  bool dev_chain_pending = false;  // k_weight_chain of this call is on the chain stream: enqueue_phase2 waits for it
  bool weights_on_host = false;  // the last PASS 2 read its weights from h_weights (b.weights holds them only in the sharded forms)
  bool seeds_dirty = false, masks_dirty = false;  // device copies of seed nonces / recovered masks not yet wiped
  // bpp_verify_enqueue (verdict.h): device copies of rounds_bad / defer, made by the batch's first enqueue and only where the host
  // vector holds a finding (a null pointer means all clear); word 0 of enq_words holds the call's zero-weight word (low half) and
  // the count of groups that have read it (high half), words 1 .. the groups' key words.  The whole allocation is kept as an
  // enqueue expects it -- word 0 zero, every key all ones: k_verdict_finish leaves it so -- whatever the layout, so enqueues of the
  // same batch follow each other on the stream with nothing in between.  enq_actions: four slots of per-group actions in mapped
  // page-locked memory, read by k_verdict_finish where the host wrote them; a slot is rewritten only once the ticket that last
  // used it is done.
  DevBuf<uint8_t> d_rounds_bad, d_defer;
  bool enq_findings_ready = false;
  DevBuf<unsigned long long> enq_words;
  PinnedBuf<int> enq_actions;
  uint32_t enq_actions_G = 0, enq_actions_next = 0;
  uint64_t enq_slot_ticket[4] = {0, 0, 0, 0};
  uint64_t enq_last_ticket = 0;  // the batch's last enqueue (0: none): a layout change waits for it
  // bpp_batch_refill_enqueue (refill.h).  refillable: made by bpp_batch_upload_packed_device on its device path, which records the
  // shape a refill must keep.  refilled: the contents are the stream's -- the host copies of what depends on the bytes (desc[].flags,
  // defer, any_defer, any_seed) describe the upload's contents and are not looked at any more; d_defer is written by the refill
  // kernel alone.  refill_red: the kernel's reduction words, zero between refills; refill_state: the word k_verdict_finish reads.
  bool refillable = false, refilled = false;
  struct RefillShape {
    uint64_t n_items = 0, proof_len = 0;
    uint32_t m = 0, t0 = 0;
    bool nonces = false, min_values = false, min_present = false;
  } refill_shape;
  DevBuf<uint32_t> refill_red;
  DevBuf<unsigned long long> refill_state;
  // bpp_batch_refill_enqueue_count: the batch's own live count, allocated with the words above and written by k_refill_finish.
  // has_live: some refill of the batch took a count -- from then on every refill writes the word (N without a count) and the
  // enqueue driver hands it to the chain and verdict kernels; before that they get a null pointer and compute what they always did.
  DevBuf<uint32_t> refill_live;
  bool has_live = false;
  const uint32_t *live_word() const { return has_live ? (const uint32_t *)refill_live.p : (const uint32_t *)nullptr; }
  // bpp_batch_refill_enqueue_live: the batch's own normalised mask, N bytes, allocated by the first refill that takes a mask and
  // written by k_refill_packed<true>.  mask_form: the batch's LAST refill took a mask -- the chain and verdict kernels then run in
  // their MASKED forms on these bytes and get no count word; a plain or count refill afterwards drops the form (the bytes go stale
  // and are not read).  Freed with the batch; it holds no secret.
  DevBuf<uint8_t> refill_mask;
  bool mask_form = false;
  LiveView live_view() const {
    return mask_form ? LiveView{nullptr, (const uint8_t *)refill_mask.p} : LiveView{live_word(), (const uint8_t *)nullptr};
  }
  // bpp_batch_upload_mixed_device on its device path: the per-item table k_ingest_mixed packed the batch by (ingest.h), kept for
  // bpp_batch_refill_enqueue_mixed (refill.h), whose kernel reads it.  The shape such a refill must keep is this vector, not four
  // numbers: mixed_shape is the host's copy of it (rows empty: not refillable by that call; `refillable` stays the packed form's).
  // refill_shape holds n_items, t0 and the three array flags of a mixed batch as well, where verify_enqueue_locked finds them.
  DevBuf<IngestMixedRow> mixed_table;
  bool mixed = false;
  struct MixedShape {
    std::vector<IngestMixedRow> rows;
    uint64_t proof_bytes = 0;
    uint32_t max_proof_len = 0, max_m = 0;
    bool seed_present = false;
  } mixed_shape;
  // the batch's last refill carried a live count or a live mask: some slots may be dead, so a host decision that follows from the
  // per-slot shape of a mixed batch (rounds_bad) no longer holds for the call as a whole (verify_enqueue_locked)
  bool partial_form = false;
  bool enq_weights = false;  // b.weights holds the weights of the batch's last enqueue (bpp_enqueue_weights)
  // per-item transcripts (item_states.h).  item_states: made by bpp_batch_upload_*_device_transcripts on its device path -- `states`
  // holds one row per slot, written by k_item_states, and desc[i].state_idx = i; part of the shape the batch keeps: only the
  // *_transcripts refills take it.  d_state_rows: the rows PASS 1 writes for bpp_verify_enqueue_states, allocated by the first such
  // call; state_rows_dst: set for the length of that call, the destination of the kernels' STATES instantiation in place of h_states.
  bool item_states = false;
  DevBuf<uint32_t> d_state_rows;
  uint32_t *state_rows_dst = nullptr;
};
// what the blocking verify entry points, the sharded and phased forms and the traces answer for a refilled batch: they decide by the
// host copies above, which describe other contents
#define BPP_REFILLED_MSG "the batch was refilled on the stream (bpp_batch_refill_enqueue) and takes enqueued calls only: upload the arrays for a blocking call"

// A destroyed batch leaves its device and pinned allocations to the next upload on the same context (a caller that
// verifies fresh host buffers call after call would otherwise pay ~30 hipMalloc/hipFree pairs, 15-25 ms, per call).
void adopt_buffers(Batch &dst, Batch &src) {
#define BPP_ADOPT(f) dst.f.swap(src.f)
  BPP_ADOPT(d_ext_status); BPP_ADOPT(bytes); BPP_ADOPT(states); BPP_ADOPT(seeds); BPP_ADOPT(d_desc); BPP_ADOPT(minvals);
  BPP_ADOPT(src_off); BPP_ADOPT(owner); BPP_ADOPT(idx_commit); BPP_ADOPT(idx_proof); BPP_ADOPT(status0); BPP_ADOPT(chal);
  BPP_ADOPT(rows); BPP_ADOPT(parts); BPP_ADOPT(gemm_lo); BPP_ADOPT(gemm_hi); BPP_ADOPT(gparts); BPP_ADOPT(gemm_mult); BPP_ADOPT(scal); BPP_ADOPT(shr); BPP_ADOPT(tab); BPP_ADOPT(rng_out); BPP_ADOPT(weights); BPP_ADOPT(chain_wide);
  BPP_ADOPT(masks); BPP_ADOPT(chal_bytes); BPP_ADOPT(status); BPP_ADOPT(group_first); BPP_ADOPT(group_dlo); BPP_ADOPT(dynpts); BPP_ADOPT(dyn_hi); BPP_ADOPT(dec_spill);
  BPP_ADOPT(msm.counts); BPP_ADOPT(msm.starts); BPP_ADOPT(msm.sorted); BPP_ADOPT(msm.order); BPP_ADOPT(msm.order_win);
  BPP_ADOPT(msm.cls_hist);
  BPP_ADOPT(msm.buckets); BPP_ADOPT(msm.Q); BPP_ADOPT(msm.W); BPP_ADOPT(msm.R); BPP_ADOPT(msm.comp32);
  BPP_ADOPT(msm.is_identity); BPP_ADOPT(msm.term_sidx); BPP_ADOPT(msm.term_pidx); BPP_ADOPT(msm.group_off);
  BPP_ADOPT(h_rng); BPP_ADOPT(h_weights); BPP_ADOPT(h_wide); BPP_ADOPT(h_status); BPP_ADOPT(h_status_any); BPP_ADOPT(h_ident); BPP_ADOPT(h_masks); BPP_ADOPT(h_states);
#undef BPP_ADOPT
  // what is known about the adopted status words travels with them (settle_status clears only the blocks that may hold something);
  // a verification whose results were never looked at leaves them unknown
  dst.h_status_dirty.swap(src.h_status_dirty);
  std::swap(dst.h_status_dirty_of, src.h_status_dirty_of);
  if (!src.status_settled) std::fill(dst.h_status_dirty.begin(), dst.h_status_dirty.end(), (uint8_t)1);
}

void wipe_batch_secrets(Batch &b, hipStream_t s);

}  // namespace

// pipelined host-buffers-in form (bpp_verify_submit_packed / bpp_verify_collect), implemented further down
struct PipeJob {
  uint64_t ticket = 0;
  int action = 0;
  size_t chunk = 0;
  std::shared_ptr<Params> Pp;
  uint64_t params = 0;
  UploadPlan pl;
  size_t n_items = 0;
  uint32_t t = 0;
  int rc = 0;
  std::string err;
  std::vector<uint8_t> masks, present;
  bool done = false;
};

struct PipeLane {
  bpp_ctx *child = nullptr;
  std::thread th;
  std::shared_ptr<PipeJob> job;  // posted by submit, taken by the worker
  bool busy = false;             // from the moment submit claims the lane until its job is done
};

// (the ticket protocol of lanes_host.h written out: the depth-1 submit/collect cycle measured 9 % slower through TicketLanes and
// the cause was not found, profiles/lanes_refactor_ab.txt; the prove pipeline, which measured no slower, runs on it)
struct Pipeline {
  std::mutex mu;                  // lanes' state, tickets
  std::condition_variable cv;
  std::mutex submit_mu;           // one submit at a time: lanes are claimed in ticket order
  std::vector<std::unique_ptr<PipeLane>> lanes;  // fixed once the pipeline exists
  std::map<uint64_t, std::shared_ptr<PipeJob>> tickets;
  uint64_t next_ticket = 1;
  uint32_t next_lane = 0;
  bool quit = false;
};

void pipeline_shutdown(bpp_ctx *ctx);

// the same for prove calls (bpp_prove_submit / bpp_prove_collect, engine_prove_pipe.h): lanes and tickets of their own
struct ProveJob;
using ProvePipeline = lanes::TicketLanes<bpp_ctx *, ProveJob>;
void prove_pipeline_shutdown(bpp_ctx *ctx);
// what the lanes add to the context's own answers (bpp_prove_check_stats, bpp_prove_check_recovery_stats, bpp_prove_secret_bytes);
// nothing for a context that never used the prove pipeline
int prove_pipeline_check_stats(bpp_ctx *ctx, struct bpp_prove_check_stats *sum);
int prove_pipeline_recovery_stats(bpp_ctx *ctx, uint64_t *replayed, uint64_t *mismatched);
int prove_pipeline_secret_bytes(bpp_ctx *ctx, uint64_t *examined, uint64_t *nonzero);

// The kernel forms the last bucket MSM of a context took (msm_run decides them once and launches by them; msm_plain_run
// records the plain kernels): bpp_msm_last_plan reads this, so that a test can tell WHICH kernels gave it its bytes
enum MsmReduce : uint32_t { MSM_RC_QUAD = 0, MSM_RC2 = 1, MSM_RC = 2, MSM_BITSUM = 3 };
struct MsmForm {
  bool valid = false;       // a B1 call or a verification has run an MSM on this context
  bool plain = false;       // msm_plain.h; nothing below applies
  bool ct = false;          // ct.h: k_ct_straus (bpp_msm_ct); only G and terms apply
  bool quad = false;        // k_msm_accumulate_quad, else k_msm_accumulate
  MsmReduce reduce = MSM_RC_QUAD;
  bool final_quad = false;  // k_msm_final_quad, else k_msm_final
  bool narrow = false;      // 256-lane prelude and order kernels, else 1024
  uint32_t dig_cap = 0;     // terms per group whose digits k_msm_prelude keeps in LDS
  uint32_t slices = 0;      // the sliced prelude (k_msm_slice_*) with this many slices; 0: k_msm_prelude
  uint32_t c = 0, K = 0, K_wide = 0, nb = 0, G = 0, terms = 0;
};

// the work buffers of bpp_msm_ct / bpp_msm_ct_batched: kept between calls (a second call of the same size allocates nothing).
// sc, part and pin_sc hold secrets during a call and are zero between calls (bpp_msm_ct_secret_bytes reads them back)
struct CtMsmWork {
  bool used = false;
  DevBuf<sc> sc_dev;         // the scalars
  DevBuf<ge> part;           // one partial sum per chunk
  PinnedBuf<uint8_t> pin_sc; // the one host copy of the scalars: checked here, uploaded from here
  DevBuf<niels> pts;
  DevBuf<uint8_t> pts_in;
  DevBuf<uint32_t> pts_bad;
  DevBuf<CtChunk> plan;
  DevBuf<uint32_t> chunk_off;
  DevBuf<ge> R;
  DevBuf<uint8_t> out32;
  PinnedBuf<uint32_t> pin_plan;
  PinnedBuf<uint8_t> pin_out;
};

struct bpp_ctx {
  int device = 0;
  MsmForm msm_form;
  CtMsmWork ct_msm;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  std::string err;
  std::mutex mu;
  // references this context holds on shared objects (created or retained here): released when the context dies
  std::multiset<uint64_t> held_params, held_precomps;
  std::map<uint64_t, std::unique_ptr<Batch>> batches;
  std::unique_ptr<Batch> spare_batch;  // buffers of the last destroyed batch (adopt_buffers)
  PinnedBuf<uint8_t> pin_upload, pin_upload2;  // page-locked staging of bpp_batch_upload (bytes; descriptors etc.)
  PinnedBuf<uint32_t> pin_small;       // staging for small host->device arrays (a pageable hipMemcpyAsync of a few
                                       // hundred bytes was measured at ~10 ms on this stack)
  // the device form of the packed upload (ingest.h): the kernel's result words and per-item info bytes, where they are fetched
  // to, the staging of the host fall-back, and what the calls came to
  DevBuf<uint32_t> ingest_res;
  DevBuf<uint8_t> ingest_info;
  PinnedBuf<uint32_t> pin_ingest;
  PinnedBuf<uint8_t> pin_ingest_info, pin_fallback;
  PinnedBuf<IngestMixedRow> pin_mixed_table;
  struct bpp_ingest_stats ingest_stats{};
  bool profile = false;
  bool profile_light = false;  // bpp_profile_enable(ctx, 2): events around the roofline kernel (k_msm_accumulate) only
  bpp_profile prof{};
  hipEvent_t ev[16];
  bool ev_ready = false;
  hipEvent_t ev_rng;
  bool ev_rng_ready = false;
  hipEvent_t ev_wait;  // gpu_wait_stream's marker
  bool ev_wait_ready = false;
  WaitHint wait_hint_rng, wait_hint_end, wait_hint_prove;  // a verification's two waits, a prover call's wait (gpu_wait_event)
  // small inputs: decompression runs beside PASS 1 on a second stream (enqueue_phase1)
  hipStream_t side_stream = nullptr;
  hipEvent_t ev_fork, ev_join;
  // the weight chains as a kernel (chain_dev.h): their own stream beside decompression and the weight-free scalars, the
  // transcript Transcript::new(b"Bulletproofs+ verifier weights") leaves, and the "a weight was zero" word the host looks at
  // with the results
  hipStream_t chain_stream = nullptr;
  hipEvent_t ev_chain_fork, ev_chain_done;
  DevBuf<Strobe> d_chain_t0;
  PinnedBuf<uint32_t> h_chain_zero;
  uint64_t device_chain_calls = 0, device_chain_redraws = 0, wide_chain_calls = 0;
  DevBuf<uint8_t> scratch128;
  // batch prover: one device arena, page-locked staging and the sub-batch streams, all reused across calls
  DevBuf<uint8_t> prove_arena;
  PinnedBuf<uint8_t> prove_pin_in, prove_pin_out;
  std::vector<hipStream_t> prove_streams;
  // high-priority twins of the sub-batch streams: the prover's small latency-bound kernels (Fiat-Shamir step, vector fold,
  // point encoding) run on them so that they are not starved by the other sub-batch's chip-filling fixed-base MSM
  std::vector<hipStream_t> prove_lane_streams;
  hipStream_t prove_msm_stream = nullptr;  // the one stream every sub-batch's fixed-base MSM runs on, first in first out ("prove_fifo")
  std::vector<hipEvent_t> prove_sync_events;  // two per sub-batch: lane step done / fixed-base MSM done
  // the witness check of a sub-batch (commit(v_j, r_j) against the statement's commitments, :275-284) runs on a stream of its own
  // beside the call's first steps; two events per sub-batch: inputs resident / check done
  std::vector<hipStream_t> prove_aux_streams;
  std::vector<hipEvent_t> prove_aux_events;
  std::vector<hipEvent_t> prove_events;  // pairs around every k_fb_msm launch of the last bpp_prove_batch (profiling only)
  // bpp_prove_openings_device: the event that orders the caller's arrays (complete on ctx->stream) before every sub-batch's ingest
  // kernel, the table of the items the host refused (public: item, lengths, finding), what the calls came to
  hipEvent_t prove_dev_event = nullptr;
  DevBuf<uint8_t> prove_dev_refused;
  struct bpp_prove_device_stats prove_dev_stats{};
  // bpp_prove_plan_create / bpp_prove_enqueue (engine_prove_plan.h): the resident plans by handle -- what the context itself needs of
  // one is its arena, which bpp_prove_secret_bytes reads -- and the counters of bpp_prove_enqueue_stats
  struct ProvePlanBase {
    DevBuf<uint8_t> arena;
    virtual ~ProvePlanBase() {}
  };
  std::map<uint64_t, std::unique_ptr<ProvePlanBase>> prove_plans;
  uint64_t prove_plan_next = 1;
  struct bpp_prove_enqueue_stats prove_enq_stats{};
  struct bpp_transcripts_stats tops_stats{};  // bpp_transcripts_enqueue (engine_transcript_ops.h)
  // bpp_rows_msm_enqueue / bpp_rows_scalar_enqueue (engine_rows.h): the decoded points of a slab of rows or the shared bases' multiples
  // -- public data; no scalar is ever copied here -- and the counters of bpp_rows_stats
  struct RowsWork {
    DevBuf<niels> pts;
    DevBuf<uint32_t> bad, base_tab;
    struct bpp_rows_stats stats{};
  } rows;
  bpp_prove_profile pprof{};
  // knobs (tests, A/B timing).  -1 = the engine's own rule.  The BPP_* environment variables of the same names are read
  // ONCE, when the context is created (no getenv on any verification path: a host that calls setenv from another thread
  // would race with it); bpp_ctx_set_option changes them afterwards.
  struct Options {
    int transcripts_wave = -1, tables_wave = -1, side_decompress = -1, msm_c_bias = -1, msm_c_max = -1, msm_c_add = -1, msm_rc2 = -1, msm_quad = -1, msm_final_quad = -1,
        fb_threads = -1, prove_subs = -1, msm_split = -1, fused_columns = -1, prove_prio = -1, prove_fused = -1, static_gemm = -1, lazy_columns = -1, ct = -1, prove_parts = -1, prove_waves = -1, prove_fifo = -1, chain = -1, chain_test_zero = 0, wait = -1, ct_back = -1, chain_inline = -1, wide_in_lanes = -1,
        prove_check = -1, prove_check_recovery = -1, msm_plain = -1, verify_check = -1, msm_ct_k = -1, verify_joint = 0, msm_prelude_slices = 0;
  } opt;
  // "verify_check" = 1 (verify_flow): what the rechecks of this context's verifications have done; the prover's self-check runs
  // its verifications with the recheck off (verify_check_off > 0) -- a rejection there is already answered by a remake
  struct bpp_verify_check_stats vcheck_stats{};
  int verify_check_off = 0;
  // "verify_joint" = 1: passes that took the joint final check, how they ended; the remembered wait of a fall-back's second wait
  struct bpp_verify_joint_stats vjoint_stats{};
  WaitHint wait_hint_fallback;
  // test knobs of the recheck (bpp_ctx_set_option only, never copied to a lane): on the context's NEXT verification, in the passes
  // of the bit mask `passes` (1, 2, 4), the host copy of the results of group `group` is altered after the wait and before findings
  // are raised -- kind 1: identity flag 0; 2: identity flag 1 and the device bits of the group's status words cleared; 3 / 4:
  // BPP_ST_TRANSCRIPT_FAIL / BPP_ST_DECOMPRESS_FAIL set in the status word of the group's first proof; 5: the verdict of the joint
  // final check ("verify_joint") cleared, whatever `group` says, so that the fall-back runs on a valid input.  A kind above 15 holds one
  // kind per pass, four bits each, pass 1 in the lowest (three different outcomes need two different alterations)
  struct VerifyTamper {
    int passes = 0, group = 0, kind = 0;
  } vtamper;
  // the prover's self-check ("prove_check" = 1, engine_prove.h: prove_self_check): the verification batch it keeps between calls
  // (the next check's upload adopts its buffers, as the next upload adopts spare_batch's), the remembered waits of ITS
  // verifications (the prover's and the caller's verifications keep theirs), its counters
  std::unique_ptr<Batch> check_spare;
  WaitHint check_hint_rng, check_hint_end;
  struct bpp_prove_check_stats check_stats{};
  // the check's replay of mask recovery ("prove_check_recovery" = 1, engine_prove.h: check_verify): the witness's blinding factors of
  // the nonce-bearing items and their places in the checking batch, page-locked and on the device (both the check's own, wiped
  // before the prove call returns), the one word per compared proof that comes back, the counters
  PinnedBuf<uint8_t> check_pin;
  DevBuf<uint8_t> check_dev;
  PinnedBuf<uint32_t> check_words;
  uint64_t check_replayed = 0, check_mismatched = 0;
  // the seed-nonce and mask buffers of the check's batch as they were last seen zeroed (give_back in check_verify zeroes a fresh
  // allocation once: bpp_prove_secret_bytes reads them, and what hipMalloc hands out is not zero)
  const void *check_zeroed_seeds = nullptr, *check_zeroed_masks = nullptr;
  size_t check_zeroed_seeds_n = 0, check_zeroed_masks_n = 0;
  // the statements (first commitment: public) of the context's last mixed prove call whose self-check failed on mask recovery and
  // not on the verifier's verdict: bpp_prove_item_message, which is given an item and a code, tells the two apart by it
  std::mutex check_note_mu;
  std::vector<std::array<uint8_t, 32>> check_recovery_failed;
  // test knobs of the self-check (bpp_ctx_set_option only, no environment variable, not copied to a prove pool's lanes): XOR
  // `mask` into byte `byte` of proof `proof` - 1 in the page-locked host copy of the NEXT checked prove call, before the check; `times`
  // = 2 alters the remake of that proof as well.  `nonce` = 1: the byte is altered in the check's own copy of that item's seed
  // nonce instead (byte 0..31; "prove_check_recovery" = 1: the replayed recovery then disagrees with a proof that is right).  The
  // call's entry point takes them and puts the defaults back.
  struct CheckTamper {
    int proof = 0, byte = 1, mask = 1, times = 1, nonce = 0;
  } tamper;
  // bpp_verify_enqueue: a ring of events, ticket t in slot t % size (a slot that a later ticket has taken over answers for that one,
  // which is behind t on the same stream); the counters of bpp_enqueue_stats
  std::vector<hipEvent_t> enq_events;
  uint64_t enq_next = 1;
  struct bpp_enqueue_stats enq_stats{};
  struct bpp_refill_stats refill_stats{};  // bpp_batch_refill_enqueue: its tickets are the enqueue tickets
  std::shared_ptr<Pipeline> pipe;  // bpp_verify_submit_packed / bpp_verify_collect: lanes, tickets (built on first submit)
  std::mutex pipe_init_mu;
  uint32_t pipe_depth = 3;
  std::shared_ptr<ProvePipeline> prove_pipe;  // bpp_prove_submit / bpp_prove_collect: lanes, tickets (built on first submit)
  std::mutex prove_pipe_init_mu;
  uint32_t prove_pipe_depth = 3;
};

namespace {

// lanes per output point of k_fb_msm: enough (term, window) items per lane to outweigh the log2(lanes) reduction tree
static uint32_t fb_threads(const bpp_ctx *ctx, uint32_t terms, const FbGeom &g) {
  if (ctx->opt.fb_threads > 0) {  // any whole number of wavefronts up to the kernel's launch bound
    const uint32_t t = ((uint32_t)ctx->opt.fb_threads + 63u) & ~63u;
    return t > FB_THREADS ? FB_THREADS : t;
  }
  const uint32_t items = terms * g.windows;
  return items >= 4096 ? 256u : (items >= 1024 ? 128u : 64u);
}

struct OptionName {
  const char *name, *env;
  int bpp_ctx::Options::*field;
};
const OptionName kOptions[] = {
    {"transcripts_wave", "BPP_TRANSCRIPTS_WAVE", &bpp_ctx::Options::transcripts_wave},
    {"tables_wave", "BPP_TABLES_WAVE", &bpp_ctx::Options::tables_wave},
    {"side_decompress", "BPP_SIDE_DECOMPRESS", &bpp_ctx::Options::side_decompress},
    {"msm_c_bias", "BPP_MSM_C_BIAS", &bpp_ctx::Options::msm_c_bias},
    {"msm_c_max", "BPP_MSM_C_MAX", &bpp_ctx::Options::msm_c_max},
    {"msm_c_add", "BPP_MSM_C_ADD", &bpp_ctx::Options::msm_c_add},
    {"msm_rc2", "BPP_MSM_RC2", &bpp_ctx::Options::msm_rc2},
    {"msm_quad", "BPP_MSM_QUAD", &bpp_ctx::Options::msm_quad},
    {"msm_final_quad", "BPP_MSM_FINAL_QUAD", &bpp_ctx::Options::msm_final_quad},
    {"fb_threads", "BPP_FB_THREADS", &bpp_ctx::Options::fb_threads},
    {"prove_subs", "BPP_PROVE_SUBS", &bpp_ctx::Options::prove_subs},
    {"msm_split", "BPP_MSM_SPLIT", &bpp_ctx::Options::msm_split},
    {"fused_columns", "BPP_FUSED_COLUMNS", &bpp_ctx::Options::fused_columns},
    {"prove_prio", "BPP_PROVE_PRIO", &bpp_ctx::Options::prove_prio},
    {"prove_fused", "BPP_PROVE_FUSED", &bpp_ctx::Options::prove_fused},
    {"ct", "BPP_CT", &bpp_ctx::Options::ct},
    // "ct" = 2: how many rounds before the end the public points behind A1's folded generators are made (1..3; the engine's rule: 1)
    {"ct_back", "BPP_CT_BACK", &bpp_ctx::Options::ct_back},
    {"prove_parts", "BPP_PROVE_PARTS", &bpp_ctx::Options::prove_parts},
    {"prove_waves", "BPP_PROVE_WAVES", &bpp_ctx::Options::prove_waves},
    {"prove_fifo", "BPP_PROVE_FIFO", &bpp_ctx::Options::prove_fifo},
    {"static_gemm", "BPP_STATIC_GEMM", &bpp_ctx::Options::static_gemm},
    {"lazy_columns", "BPP_LAZY_COLUMNS", &bpp_ctx::Options::lazy_columns},
    // where the batch-weight chains run: 0 host cores (chain_host.h), 1 the device (chain_dev.h), 2 the sponges on host cores and the
    // reduction mod l on the device, -1 the engine's rule (chain_mode)
    {"chain", "BPP_CHAIN", &bpp_ctx::Options::chain},
    // tests: the device chain reports the weight of proof (value - 1) as zero, so that the redraw fall-back runs
    {"chain_test_zero", "BPP_CHAIN_TEST_ZERO", &bpp_ctx::Options::chain_test_zero},
    // how a calling thread waits for the device: 0 the runtime's wait (spins on a core until the stream is done), 1 naps between
    // looks at an event (gpu_wait), -1 the engine's rule: naps for calls of BPP_WAIT_NAP_MIN_PROOFS proofs and more
    {"wait", "BPP_WAIT", &bpp_ctx::Options::wait},
    // the device chains (chain = 1) behind PASS 1 on the call's own stream (1) instead of a stream of their own beside the decompression (0)
    {"chain_inline", "BPP_CHAIN_INLINE", &bpp_ctx::Options::chain_inline},
    // chain = 2: the reduction mod l of the host sponges' bytes in k_scalars_lanes' prologue (1, the rule) or as a launch of its own (0)
    {"wide_in_lanes", "BPP_WIDE_IN_LANES", &bpp_ctx::Options::wide_in_lanes},
    // 1: every proof of bpp_prove_batch / bpp_prove_batch_mixed (and of a prove pool made from this context) is verified on this
    // context before it is returned, a rejected one made again once (engine_prove.h: prove_self_check); 0 / -1: off
    {"prove_check", "BPP_PROVE_CHECK", &bpp_ctx::Options::prove_check},
    // 1: a checked call ("prove_check" = 1) also replays mask recovery for its items that carry a seed nonce and compares the
    // recovered masks with the witness's blinding factors on the device (engine_prove.h: check_verify); 0 / -1: off.  Without
    // "prove_check" it does nothing
    {"prove_check_recovery", "BPP_PROVE_CHECK_RECOVERY", &bpp_ctx::Options::prove_check_recovery},
    // 1: bpp_msm_vartime, bpp_msm_vartime_batched and bpp_msm_mixed through the plain double-and-add kernels (msm_plain.h) instead
    // of the bucket method; 0 / -1: off
    {"msm_plain", "BPP_MSM_PLAIN", &bpp_ctx::Options::msm_plain},
    // 1: a group that a verification rejects on the device (tiers PASS1, PASS2, MSM) is verified once more under the complementary
    // kernel forms with the plain MSM, and a third time when the two disagree (verify_flow); 0 / -1: off
    {"verify_check", "BPP_VERIFY_CHECK", &bpp_ctx::Options::verify_check},
    // the kernel form of bpp_msm_ct / bpp_msm_ct_batched: 1 / 2 terms per quad (k_ct_straus<K>); 0 / -1: the engine's rule, from
    // the call's public counts (ct_plan.h: ct_form_rule)
    {"msm_ct_k", "BPP_MSM_CT_K", &bpp_ctx::Options::msm_ct_k},
    // 1: a verification pass with two or more groups, all of them held to the final check, runs ONE multiscalar multiplication over
    // all of them and falls back to the per-group ones only when that joint check fails (verify_flow_once), while the joint group
    // has at most BPP_JOINT_MAX_TERMS terms; 2: whatever its size (measurement); 0 / -1: off
    {"verify_joint", "BPP_VERIFY_JOINT", &bpp_ctx::Options::verify_joint},
    // the bucket MSM's prelude: S >= 2 cuts every (group, window) sort into S slices (msm.h: k_msm_slice_*), bpp_msm_vartime* included;
    // 1: the one-workgroup form whatever the size; 0 / -1: the engine's rule (recode.h: msm_prelude_slices)
    {"msm_prelude_slices", "BPP_MSM_PRELUDE_SLICES", &bpp_ctx::Options::msm_prelude_slices},
};
struct TamperName {
  const char *name;
  int bpp_ctx::CheckTamper::*field;
};
const TamperName kTamperKnobs[] = {
    {"prove_check_tamper", &bpp_ctx::CheckTamper::proof},
    {"prove_check_tamper_byte", &bpp_ctx::CheckTamper::byte},
    {"prove_check_tamper_xor", &bpp_ctx::CheckTamper::mask},
    {"prove_check_tamper_times", &bpp_ctx::CheckTamper::times},
    {"prove_check_tamper_nonce", &bpp_ctx::CheckTamper::nonce},
};
struct VerifyTamperName {
  const char *name;
  int bpp_ctx::VerifyTamper::*field;
};
const VerifyTamperName kVerifyTamperKnobs[] = {
    {"verify_check_tamper", &bpp_ctx::VerifyTamper::passes},
    {"verify_check_tamper_group", &bpp_ctx::VerifyTamper::group},
    {"verify_check_tamper_kind", &bpp_ctx::VerifyTamper::kind},
};
void options_from_env(bpp_ctx *c) {
  for (const OptionName &o : kOptions)
    if (const char *e = getenv(o.env)) c->opt.*(o.field) = atoi(e);
}

int fail(bpp_ctx *ctx, int code, const std::string &m, char *errbuf = nullptr, size_t len = 0) {
  if (ctx) ctx->err = m;
  set_err(errbuf, len, m);
  return code;
}

enum Mark { M_START = 0, M_TRANSCRIPTS, M_DECOMPRESS, M_SCALARS, M_WEIGHTS_IN, M_LANES, M_REDUCE, M_DIGITS, M_SORT, M_ORDER, M_ACC,
            M_BUCKET, M_FINAL, M_MASKS0, M_MASKS, M_CHAIN, M_COUNT };

struct StageTimer {
  bpp_ctx *ctx;
  bool have[16] = {false};
  bool on = true;  // false (bpp_verify_enqueue): no stage events, whatever the context's profiling says
  explicit StageTimer(bpp_ctx *c, bool enabled = true) : ctx(c), on(enabled) {
    if (on && ctx->profile && !ctx->ev_ready) {
      for (auto &e : ctx->ev) HIP_CHECK(hipEventCreate(&e));
      ctx->ev_ready = true;
    }
  }
  void mark(int idx) {
    if (on && ctx->profile && idx < 16) {
      // light form: the two events that bracket the roofline kernel and nothing else (every mark is a barrier packet with a
      // timestamp in the queue; thirteen per step read 0-4 % lower than two, inside the run-to-run spread: profiles/r06_stage_events_ab.txt)
      if (ctx->profile_light && idx != M_ORDER && idx != M_ACC) return;
      HIP_CHECK(hipEventRecord(ctx->ev[idx], ctx->stream));
      have[idx] = true;
    }
  }
  float between(int a, int b) {
    float ms = 0;
    if (ctx->profile && have[a] && have[b]) HIP_CHECK(hipEventElapsedTime(&ms, ctx->ev[a], ctx->ev[b]));
    return ms;
  }
};

inline uint32_t cdiv(uint32_t a, uint32_t b) { return (a + b - 1) / b; }

// ---- how a calling thread waits for the device.  hipStreamSynchronize / hipEventSynchronize spin: measured on the GPU boxes
// (tools/microbench/wait_modes.hip) a waiting thread burns 100 % of a core with either, whatever flags the event was created
// with, unless the PROCESS-WIDE device flag hipDeviceScheduleBlockingSync is set (then 25 % / 6 %) -- which is the host
// application's to set, not a library's.  A verification of tens of thousands of proofs takes milliseconds and several are in
// flight, so its caller naps instead: hipEventQuery every 50 us costs 1-2 % of a core and wakes up ~70 us late, which such a
// call does not notice (bench.py: 3.7 -> 0.3 host cores per rank for the callers of the headline).  Calls of a few
// hundred proofs (0.5-0.7 ms, one at a time) keep the runtime's spinning wait: there 70 us are 10 %.
#define BPP_WAIT_NAP_MIN_PROOFS 4096u
inline bool wait_naps(const bpp_ctx *ctx, size_t proofs) {
  return ctx->opt.wait >= 0 ? ctx->opt.wait != 0 : proofs >= BPP_WAIT_NAP_MIN_PROOFS;
}
// hint (optional): the caller's memory of how long THIS wait took the last times, microseconds (updated here), for the work `key`
// names.  When and how long the caller naps between two looks is runtime_host.h's (WaitSchedule); the looking is done here.
inline void gpu_wait_event(hipEvent_t ev, bool nap, WaitHint *wh = nullptr, uint64_t key = 0, bool tail_spin = false) {
  wait_hint_begin(wh, key);
  if (!nap) {
    HIP_CHECK(hipEventSynchronize(ev));
    return;
  }
  const auto t0 = std::chrono::steady_clock::now();
  WaitSchedule sched{wh ? wh->us : 0u, tail_spin};
  for (;;) {
    const hipError_t e = hipEventQuery(ev);
    const long waited = (long)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    if (e == hipSuccess) {
      wait_hint_fold(wh, waited);
      return;
    }
    if (e != hipErrorNotReady) HIP_CHECK(e);
    if (const long us = sched.next_nap_us(waited)) nap_us(us);
  }
}
inline void gpu_wait_stream(bpp_ctx *ctx, hipStream_t s, bool nap, WaitHint *hint = nullptr, uint64_t key = 0, bool tail_spin = false);
inline bool gpu_wait_stream_ok(bpp_ctx *ctx, hipStream_t s, bool nap) {  // false instead of an exception (the sharded forms carry faults along)
  try {
    gpu_wait_stream(ctx, s, nap);
    return true;
  } catch (const EngineError &) {
    (void)hipGetLastError();
    return false;
  }
}
inline void gpu_wait_stream(bpp_ctx *ctx, hipStream_t s, bool nap, WaitHint *hint, uint64_t key, bool tail_spin) {
  if (!nap) {
    HIP_CHECK(hipStreamSynchronize(s));
    return;
  }
  // (NOT hipStreamQuery as a first look: measured -- tools/microbench/wait_modes.hip -- a stream query on a busy stream leaves a
  // helper thread of the runtime spinning until that work is done, 70-90 % of a core that no thread of the caller's shows; an
  // event that is already complete costs the ~30 us look of gpu_wait_event at most)
  if (!ctx->ev_wait_ready) {
    HIP_CHECK(hipEventCreateWithFlags(&ctx->ev_wait, hipEventDisableTiming));
    ctx->ev_wait_ready = true;
  }
  HIP_CHECK(hipEventRecord(ctx->ev_wait, s));
  gpu_wait_event(ctx->ev_wait, true, hint, key, tail_spin);
}

static bool decompress_spill_enabled() {
  static const bool on = [] {
    const char *e = getenv("BPP_DECOMPRESS_SPILL");
    return e ? atoi(e) != 0 : true;
  }();
  return on;
}


// ------------------------------------------------------------------ MSM driver
// A call of up to this many MSM terms is "small": it has the chip to itself, its time is the length of its dependency chains
// (BPP_SMALL_CALL_TERMS and the rule itself: recode.h, msm_choose_window -- host-compiled by the tests as well)
uint32_t choose_window(const bpp_ctx *ctx, uint32_t group_terms, uint32_t all_terms) {
  return msm_choose_window(group_terms, all_terms, ctx->opt.msm_c_max, ctx->opt.msm_c_add, ctx->opt.msm_c_bias);
}

// plan + work buffers for G groups with term offsets goff[0..G]; the term lists (term_sidx / term_pidx) are filled by
// the caller, from host vectors (msm_prepare) or by a kernel (layout_groups)
// half-scalar plan (msm.h: k_split_shift_quad): small verifier calls, unless the one-lane kernels are forced.  It halves the
// final Horner step (0.26 -> 0.13 ms) and doubles every bucket's list (quad accumulation: 0.034 -> 0.066 ms at 256 proofs,
// 0.07 -> 0.18 at 1024).  Measured on non-aggregated 64-bit proofs (profiles/r03_v4_bench_latency*.jsonl): 1 proof 0.63 -> 0.47
// ms, 64: 0.65 -> 0.52, 256: 0.67 -> 0.62, 512: 0.79 -> 0.73.  The two plans cross at about 900 proofs (896: 0.94 / 0.96 ms with /
// without, 1024: 1.00-1.03 / 0.98-1.00, 1280: 1.16-1.21 / 1.11-1.12; same box, alternating): up to 14 000 terms.
#define BPP_SPLIT_CALL_TERMS 14000u
bool msm_wants_split(const bpp_ctx *ctx, uint32_t n_terms) {
  if (ctx->opt.msm_split >= 0) return ctx->opt.msm_split != 0 && ctx->opt.msm_quad != 0;
  return n_terms <= BPP_SPLIT_CALL_TERMS && ctx->opt.msm_quad != 0;
}
// goff: term offsets of the groups as the kernels will see them (already doubled for a split plan)
// copy_goff: the group offsets go to the device by a copy of their own (msm_prepare); layout_groups hands them to
// k_layout_terms through mapped host memory instead
void msm_plan_alloc(bpp_ctx *ctx, MsmWork &w, const std::vector<uint32_t> &goff, bool split = false, bool copy_goff = true) {
  const uint32_t G = (uint32_t)goff.size() - 1, n = goff[G];
  uint32_t maxg = 0;
  for (uint32_t g = 0; g < G; g++) maxg = std::max(maxg, goff[g + 1] - goff[g]);
  const MsmPlan plan = msm_make_plan(choose_window(ctx, maxg, split ? n / 2 : n), G, n, split ? BPP_MSM_SPLIT_BITS : 253u);
  // which prelude (recode.h has the LDS table): refused here, before anything is allocated or launched, when neither form can hold
  // the plan's bucket tables in a workgroup's LDS
  const uint32_t sort_threads = BPP_SORT_THREADS;  // (the wider form's need: a plan that fits it fits the 256-lane form)
  const uint32_t slices = msm_prelude_slices(maxg, G, plan.K, plan.nb, sort_threads, ctx->opt.msm_prelude_slices);
  if (!msm_prelude_fits(plan.nb, sort_threads, slices ? 1u : 0u))
    throw EngineError{BPP_ERR_ENGINE, "MSM plan: the prelude's bucket tables (" + std::to_string(plan.c) + "-bit windows) do not fit a workgroup's LDS"};
  w.plan = plan;
  w.split = split;
  w.max_group_terms = maxg;
  w.h_goff = goff;
  w.slices = slices;
  if (slices) w.slice_hist.alloc((size_t)G * plan.K * slices * plan.nb);
  const size_t nbk = (size_t)G * plan.K * plan.nb;
  w.counts.alloc(nbk);
  w.starts.alloc(nbk);
  w.sorted.alloc((size_t)n * plan.K);
  w.order.alloc(nbk);
  w.order_win.alloc(nbk);
  w.cls_hist.alloc((size_t)G * plan.K * 768);
  w.buckets.alloc(nbk);
  w.Q.alloc((size_t)G * plan.K * plan.c);
  w.W.alloc((size_t)G * plan.K);
  w.R.alloc(G);
  w.comp32.alloc((size_t)G * 32);
  w.is_identity.alloc(G);
  w.term_sidx.alloc(n);
  w.term_pidx.alloc(n);
  w.group_off.alloc(G + 1);
  HIP_CHECK(hipStreamSynchronize(ctx->stream));  // pin_small may still feed an earlier copy / kernel
  ctx->pin_small.resize(3 * (size_t)(G + 1));
  memcpy(ctx->pin_small.data(), goff.data(), (G + 1) * 4);
  if (copy_goff) HIP_CHECK(hipMemcpyAsync(w.group_off.p, ctx->pin_small.data(), (G + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
}

void msm_prepare(bpp_ctx *ctx, MsmWork &w, const std::vector<uint32_t> &sidx, const std::vector<uint32_t> &pidx,
                 const std::vector<uint32_t> &goff) {
  msm_plan_alloc(ctx, w, goff);
  const uint32_t n = (uint32_t)sidx.size(), G1 = (uint32_t)goff.size();
  HIP_CHECK(hipStreamSynchronize(ctx->stream));
  ctx->pin_small.resize(3 * (size_t)G1 + 2 * (size_t)n);  // (may move the buffer: goff's copy has completed)
  uint32_t *pin = ctx->pin_small.data() + 3 * (size_t)G1;
  memcpy(pin, sidx.data(), (size_t)n * 4);
  memcpy(pin + n, pidx.data(), (size_t)n * 4);
  HIP_CHECK(hipMemcpyAsync(w.term_sidx.p, pin, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
  HIP_CHECK(hipMemcpyAsync(w.term_pidx.p, pin + n, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
  HIP_CHECK(hipStreamSynchronize(ctx->stream));
}

void msm_run(bpp_ctx *ctx, MsmWork &w, const sc *scalars, PointTables tabs, StageTimer *tm) {
  const MsmPlan plan = w.plan;
  hipStream_t s = ctx->stream;
  // digits + counting sort + per-window size ordering in one launch (msm.h: k_msm_prelude), then the group-level order
  const uint32_t per_group = plan.K * plan.nb;
  // many small groups of a throughput call: four-wavefront workgroups (msm.h); a small call (latency) and large groups: sixteen
  // few buckets on an idle chip (one batch per call): quad forms, ~3x shorter dependency chains (tests force either form)
  // The selection is made once, here, and kept in the context (bpp_msm_last_plan); the launches below switch on it.
  MsmForm f;
  f.valid = true;
  f.quad = w.split || (ctx->opt.msm_quad >= 0 ? ctx->opt.msm_quad != 0 : (size_t)plan.G * per_group <= 100000);
  f.narrow = !f.quad && w.max_group_terms <= BPP_SORT_SMALL_GROUP_TERMS;
  f.slices = w.slices;
  f.dig_cap = f.slices ? 0u : (f.narrow ? msm_prelude_dig_cap(plan, w.max_group_terms, BPP_SORT_THREADS_SMALL) : msm_prelude_dig_cap(plan, w.max_group_terms));
  if (plan.c <= 11 && f.quad)
    f.reduce = MSM_RC_QUAD;
  else if (plan.nb <= 256 && ctx->opt.msm_rc2 != 0)  // two windows per wavefront (msm.h)
    f.reduce = MSM_RC2;
  else if (plan.c <= 11)
    f.reduce = MSM_RC;
  else
    f.reduce = MSM_BITSUM;
  f.final_quad = ctx->opt.msm_final_quad != 0;  // (tests force either kernel)
  f.c = plan.c, f.K = plan.K, f.K_wide = plan.K_wide, f.nb = plan.nb, f.G = plan.G, f.terms = plan.n_terms;
  ctx->msm_form = f;
  const uint32_t dig_cap = f.dig_cap;
  if (f.slices) {  // large groups, or forced: histogram per slice, scan, scatter (msm.h), then the same group-level order
    const uint32_t S = f.slices, n_wg = plan.G * plan.K * S;
    hipLaunchKernelGGL(k_msm_slice_hist, dim3(n_wg), dim3(BPP_SLICE_THREADS), (size_t)plan.nb * 4, s, scalars, w.term_sidx.p, w.group_off.p, plan, S,
                       w.slice_hist.p);
    hipLaunchKernelGGL(k_msm_slice_scan, dim3(plan.G * plan.K), dim3(BPP_SLICE_SCAN_THREADS), 0, s, w.slice_hist.p, w.group_off.p, plan, S, w.counts.p,
                       w.starts.p, w.order_win.p, w.cls_hist.p);
    hipLaunchKernelGGL(k_msm_slice_scatter, dim3(n_wg), dim3(BPP_SLICE_THREADS), (size_t)plan.nb * 4, s, scalars, w.term_sidx.p, w.term_pidx.p,
                       w.group_off.p, plan, S, w.slice_hist.p, w.sorted.p);
    if (f.narrow)
      hipLaunchKernelGGL(k_msm_order<BPP_SORT_THREADS_SMALL>, dim3(plan.G), dim3(BPP_SORT_THREADS_SMALL), 0, s, w.counts.p, w.order_win.p, w.cls_hist.p, plan,
                         w.order.p);
    else
      hipLaunchKernelGGL(k_msm_order<BPP_SORT_THREADS>, dim3(plan.G), dim3(BPP_SORT_THREADS), 0, s, w.counts.p, w.order_win.p, w.cls_hist.p, plan, w.order.p);
  } else if (f.narrow) {
    hipLaunchKernelGGL(k_msm_prelude<BPP_SORT_THREADS_SMALL>, dim3(8 * cdiv(plan.G, 8) * plan.K), dim3(BPP_SORT_THREADS_SMALL), msm_prelude_lds(plan, dig_cap), s,
                       scalars, w.term_sidx.p, w.term_pidx.p, w.group_off.p, plan, dig_cap, w.counts.p, w.starts.p, w.sorted.p, w.order_win.p, w.cls_hist.p);
    hipLaunchKernelGGL(k_msm_order<BPP_SORT_THREADS_SMALL>, dim3(plan.G), dim3(BPP_SORT_THREADS_SMALL), 0, s, w.counts.p, w.order_win.p, w.cls_hist.p, plan,
                       w.order.p);
  } else {
    hipLaunchKernelGGL(k_msm_prelude<BPP_SORT_THREADS>, dim3(8 * cdiv(plan.G, 8) * plan.K), dim3(BPP_SORT_THREADS), msm_prelude_lds(plan, dig_cap), s, scalars,
                       w.term_sidx.p, w.term_pidx.p, w.group_off.p, plan, dig_cap, w.counts.p, w.starts.p, w.sorted.p, w.order_win.p, w.cls_hist.p);
    hipLaunchKernelGGL(k_msm_order<BPP_SORT_THREADS>, dim3(plan.G), dim3(BPP_SORT_THREADS), 0, s, w.counts.p, w.order_win.p, w.cls_hist.p, plan, w.order.p);
  }
  if (tm) tm->mark(M_ORDER);  // msm_accumulate_ms brackets k_msm_accumulate alone (the roofline kernel)
  if (f.quad)
    hipLaunchKernelGGL(k_msm_accumulate_quad, dim3(cdiv(plan.G * per_group, 16)), dim3(64), 0, s, w.sorted.p, w.starts.p,
                       w.counts.p, w.order.p, tabs, plan.G * per_group, w.buckets.p);
  else
    hipLaunchKernelGGL(k_msm_accumulate, dim3(8 * cdiv(plan.G, 8) * cdiv(per_group, 64)), dim3(64), 0, s, w.sorted.p, w.starts.p,
                       w.counts.p, w.order.p, tabs, per_group, plan.G, w.buckets.p);
  if (tm) tm->mark(M_ACC);
  switch (f.reduce) {
    case MSM_RC_QUAD:
      hipLaunchKernelGGL(k_msm_window_rc_quad, dim3(plan.G * plan.K), dim3(1024), 0, s, w.buckets.p, w.counts.p, plan, w.W.p);
      break;
    case MSM_RC2:
      hipLaunchKernelGGL(k_msm_window_rc2, dim3(cdiv(plan.G * plan.K, 2)), dim3(64), 0, s, w.buckets.p, w.counts.p, plan, plan.G * plan.K, w.W.p);
      break;
    case MSM_RC:
      hipLaunchKernelGGL(k_msm_window_rc, dim3(plan.G * plan.K), dim3(64), 0, s, w.buckets.p, w.counts.p, plan, w.W.p);
      break;
    case MSM_BITSUM:
      hipLaunchKernelGGL(k_msm_bitsum, dim3(plan.c, plan.K, plan.G), dim3(64), 0, s, w.buckets.p, w.counts.p, plan, w.Q.p);
      hipLaunchKernelGGL(k_msm_window, dim3(cdiv(plan.G * plan.K, 64)), dim3(64), 0, s, w.Q.p, plan, w.W.p);
      break;
  }
  if (tm) tm->mark(M_BUCKET);
  if (f.final_quad)
    hipLaunchKernelGGL(k_msm_final_quad, dim3(cdiv(plan.G, 16)), dim3(64), 0, s, w.W.p, plan, w.R.p, w.is_identity.p);
  else
    hipLaunchKernelGGL(k_msm_final, dim3(cdiv(plan.G, 64)), dim3(64), 0, s, w.W.p, plan, w.R.p, w.is_identity.p);
  if (tm) tm->mark(M_FINAL);
  HIP_CHECK(hipGetLastError());
}

// The plain MSM (msm_plain.h) over the groups `groups` of term lists that are already on the device (w.term_sidx, w.term_pidx,
// w.group_off, unsplit; goff = the same offsets on the host): R[g] and is_identity[g] of those groups, every other group's
// entries untouched.  Nothing of msm.h's plan is looked at.
void msm_plain_run(bpp_ctx *ctx, MsmWork &w, const std::vector<uint32_t> &goff, const sc *scalars, const niels *tab_a, const niels *tab_b,
                   uint32_t n_a, const std::vector<uint32_t> &groups) {
  if (groups.empty()) return;
  uint32_t maxg = 0;
  for (uint32_t g : groups) {
    if ((size_t)g + 1 >= goff.size()) throw EngineError{BPP_ERR_ENGINE, "plain MSM: group out of range"};
    maxg = std::max(maxg, goff[g + 1] - goff[g]);
  }
  const uint32_t waves = std::max<uint32_t>(1, cdiv(maxg, 64)), n = (uint32_t)groups.size();
  {
    MsmForm f;
    f.valid = f.plain = true;
    f.G = n, f.terms = goff.back();
    ctx->msm_form = f;
  }
  w.plain_part.alloc((size_t)n * waves);
  w.plain_list.resize(n);
  memcpy(w.plain_list.data(), groups.data(), (size_t)n * 4);
  hipStream_t s = ctx->stream;
  for (uint32_t lo = 0; lo < n; lo += 65535u) {  // (grid.y)
    const uint32_t ny = std::min<uint32_t>(65535u, n - lo);
    ge *part = w.plain_part.p + (size_t)lo * waves;
    hipLaunchKernelGGL(k_msm_plain, dim3(waves, ny), dim3(64), 0, s, (const uint32_t *)scalars, w.term_sidx.p, w.term_pidx.p, w.group_off.p, tab_a,
                       tab_b, n_a, w.plain_list.dev() + lo, waves, part);
    hipLaunchKernelGGL(k_msm_plain_sum, dim3(ny), dim3(64), 0, s, part, w.group_off.p, w.plain_list.dev() + lo, waves, w.R.p, w.is_identity.p);
  }
  HIP_CHECK(hipGetLastError());
}

// term lists and result buffers of a plain MSM from host vectors: what msm_prepare does for the bucket method, without a plan
void msm_plain_prepare(bpp_ctx *ctx, MsmWork &w, const std::vector<uint32_t> &sidx, const std::vector<uint32_t> &pidx,
                       const std::vector<uint32_t> &goff) {
  const uint32_t n = (uint32_t)sidx.size(), G1 = (uint32_t)goff.size();
  w.split = false;
  w.h_goff = goff;
  w.term_sidx.alloc(n);
  w.term_pidx.alloc(n);
  w.group_off.alloc(G1);
  w.R.alloc(G1 - 1);
  w.comp32.alloc((size_t)(G1 - 1) * 32);
  w.is_identity.alloc(G1 - 1);
  HIP_CHECK(hipStreamSynchronize(ctx->stream));  // pin_small may still feed an earlier copy / kernel
  ctx->pin_small.resize((size_t)G1 + 2 * (size_t)n);
  uint32_t *pin = ctx->pin_small.data();
  memcpy(pin, goff.data(), (size_t)G1 * 4);
  memcpy(pin + G1, sidx.data(), (size_t)n * 4);
  memcpy(pin + G1 + n, pidx.data(), (size_t)n * 4);
  HIP_CHECK(hipMemcpyAsync(w.group_off.p, pin, (size_t)G1 * 4, hipMemcpyHostToDevice, ctx->stream));
  HIP_CHECK(hipMemcpyAsync(w.term_sidx.p, pin + G1, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
  HIP_CHECK(hipMemcpyAsync(w.term_pidx.p, pin + G1 + n, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
  HIP_CHECK(hipStreamSynchronize(ctx->stream));
}

// decompress `n` host points into a device niels table; returns number of bad encodings
// (keep_in / keep_bad: buffers the caller keeps between calls, instead of two allocations per call)
uint32_t decompress_to_device(bpp_ctx *ctx, const uint8_t *pts32, size_t n, niels *out, DevBuf<uint8_t> *keep_in = nullptr,
                              DevBuf<uint32_t> *keep_bad = nullptr) {
  DevBuf<uint8_t> own_in;
  DevBuf<uint32_t> own_bad;
  DevBuf<uint8_t> &d_in = keep_in ? *keep_in : own_in;
  DevBuf<uint32_t> &d_bad = keep_bad ? *keep_bad : own_bad;
  d_in.alloc(n * 32);
  d_bad.alloc(1);
  HIP_CHECK(hipMemcpyAsync(d_in.p, pts32, n * 32, hipMemcpyHostToDevice, ctx->stream));
  HIP_CHECK(hipMemsetAsync(d_bad.p, 0, 4, ctx->stream));
  hipLaunchKernelGGL(k_decompress_plain, dim3(cdiv((uint32_t)n, 64)), dim3(64), 0, ctx->stream, d_in.p, (uint32_t)n, out,
                     d_bad.p);
  uint32_t bad = 0;
  HIP_CHECK(hipMemcpyAsync(&bad, d_bad.p, 4, hipMemcpyDeviceToHost, ctx->stream));
  HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return bad;
}

// generic MSM over host scalars with a prepared device point table layout
int msm_host_entry(bpp_ctx *ctx, const niels *tab_a, uint32_t n_a, const uint8_t *static_scalars32, size_t n_static,
                   const uint8_t *dyn_scalars32, const uint8_t *dyn_points32, size_t n_dyn,
                   const uint32_t *group_off_in, size_t n_groups, uint8_t *out32) {
  // scalars: [static | dynamic], canonical check
  const size_t n = n_static + n_dyn;
  std::vector<uint8_t> sb(n * 32 + 32);
  if (n_static) memcpy(sb.data(), static_scalars32, n_static * 32);
  if (n_dyn) memcpy(sb.data() + n_static * 32, dyn_scalars32, n_dyn * 32);
  for (size_t i = 0; i < n; i++)
    if (!sc_is_canonical(sb.data() + 32 * i)) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "scalar is not canonical");
  if (n == 0 || n_groups == 0) {  // empty sum = identity
    for (size_t g = 0; g < (n_groups ? n_groups : 1); g++) memset(out32 + 32 * g, 0, 32);
    return BPP_OK;
  }
  DevBuf<sc> d_sc;
  DevBuf<niels> d_dyn;
  d_sc.alloc(n);
  d_dyn.alloc(n_dyn);
  HIP_CHECK(hipMemcpyAsync(d_sc.p, sb.data(), n * 32, hipMemcpyHostToDevice, ctx->stream));
  if (n_dyn) {
    uint32_t bad = decompress_to_device(ctx, dyn_points32, n_dyn, d_dyn.p);
    if (bad) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "point is not a canonical ristretto255 encoding");
  }
  std::vector<uint32_t> sidx(n), pidx(n), goff;
  for (size_t i = 0; i < n; i++) {
    sidx[i] = (uint32_t)i;
    pidx[i] = (i < n_static) ? (uint32_t)i : (uint32_t)(n_a + (i - n_static));
  }
  if (group_off_in) {
    goff.assign(group_off_in, group_off_in + n_groups + 1);
  } else {
    goff = {0u, (uint32_t)n};
  }
  MsmWork w;
  const uint32_t G = (uint32_t)goff.size() - 1;
  if (ctx->opt.msm_plain == 1) {  // every group through the double-and-add kernels (msm_plain.h)
    msm_plain_prepare(ctx, w, sidx, pidx, goff);
    std::vector<uint32_t> all(G);
    for (uint32_t g = 0; g < G; g++) all[g] = g;
    msm_plain_run(ctx, w, goff, d_sc.p, tab_a, d_dyn.p, n_a, all);
  } else {
    msm_prepare(ctx, w, sidx, pidx, goff);
    PointTables tabs{tab_a, d_dyn.p, n_a, nullptr, nullptr};
    msm_run(ctx, w, d_sc.p, tabs, nullptr);
  }
  hipLaunchKernelGGL(k_compress_ge, dim3(cdiv(G, 64)), dim3(64), 0, ctx->stream, w.R.p, G, w.comp32.p);
  HIP_CHECK(hipMemcpyAsync(out32, w.comp32.p, 32 * (goff.size() - 1), hipMemcpyDeviceToHost, ctx->stream));
  HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return BPP_OK;
}

// The constant-time MSM over host scalars and host points (bpp_msm_ct, bpp_msm_ct_batched).  PUBLIC: n, the group offsets, the
// points, which error comes back.  SECRET: the scalars -- nothing here or in the kernels (ct.h) branches on them, addresses by
// them, or sizes a launch by them; the chunk plan and the kernel form come from the offsets alone.  The scalars' one host copy
// (page-locked), their device buffer and the chunks' partial sums are zeroed on every way out.
int msm_ct_entry(bpp_ctx *ctx, const uint8_t *scalars32, const uint8_t *points32, size_t n, const uint32_t *group_off_in, size_t n_groups,
                 uint8_t *out32) {
  CtMsmWork &w = ctx->ct_msm;
  if (n == 0 || n_groups == 0) {  // empty sum = identity; nothing is launched
    for (size_t g = 0; g < (n_groups ? n_groups : 1); g++) memset(out32 + 32 * g, 0, 32);
    return BPP_OK;
  }
  if (!scalars32 || !points32) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "null argument");
  hipStream_t s = ctx->stream;
  // a fresh allocation is zeroed once as a whole: bpp_msm_ct_secret_bytes reads all of it, and what hipMalloc hands out is not zero
  auto fresh_zero = [&](auto &buf, size_t count) {
    const void *before = buf.p;
    buf.alloc(count);
    if (buf.p != before) HIP_CHECK(hipMemsetAsync(buf.p, 0, buf.n * sizeof(*buf.p), s));
  };
  ScopeExit wipe_secrets{[&] {
    // (on the call's own stream, then waited for: the next call's upload must not overtake them, and the staging is not zeroed
    // under an upload that is still reading it)
    if (w.sc_dev.p) (void)hipMemsetAsync(w.sc_dev.p, 0, w.sc_dev.n * sizeof(sc), s);
    if (w.part.p) (void)hipMemsetAsync(w.part.p, 0, w.part.n * sizeof(ge), s);
    (void)hipStreamSynchronize(s);
    wipe(w.pin_sc.p, w.pin_sc.n);
  }};
  {
    const void *before = w.pin_sc.p;
    w.pin_sc.resize(n * 32);
    if (w.pin_sc.p != before) memset(w.pin_sc.p, 0, w.pin_sc.n);
  }
  w.used = true;
  memcpy(w.pin_sc.p, scalars32, n * 32);
  // every scalar is looked at, ONE decision at the end
  uint32_t all_canonical = 1;
  for (size_t i = 0; i < n; i++) {
    sc a;
    sc_load_words(a, w.pin_sc.p + 32 * i);
    all_canonical &= ct_sc_is_canonical(a);
    wipe(&a, sizeof a);
  }
  if (!all_canonical) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "scalar is not canonical");
  const uint32_t one_group[2] = {0u, (uint32_t)n};
  const uint32_t *goff = group_off_in ? group_off_in : one_group;
  uint32_t largest = 0;
  uint64_t chunks_k1 = 0;
  for (size_t g = 0; g < n_groups; g++) {
    const uint32_t len = goff[g + 1] - goff[g];
    largest = std::max(largest, len);
    chunks_k1 += (len + BPP_CT_QUADS - 1) / BPP_CT_QUADS;
  }
  const uint32_t K = ct_form_rule(largest, chunks_k1, ctx->opt.msm_ct_k);
  std::vector<CtChunk> chunks;
  std::vector<uint32_t> chunk_off;
  if (ct_chunk_plan(goff, n_groups, n, K, chunks, chunk_off) != 0) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "group offsets not monotone");
  const uint32_t G = (uint32_t)n_groups, C = (uint32_t)chunks.size();
  w.pts.alloc(n);
  if (decompress_to_device(ctx, points32, n, w.pts.p, &w.pts_in, &w.pts_bad))
    return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "point is not a canonical ristretto255 encoding");
  fresh_zero(w.sc_dev, n);
  fresh_zero(w.part, C);
  w.plan.alloc(C);
  w.chunk_off.alloc(G + 1);
  w.R.alloc(G);
  w.out32.alloc((size_t)G * 32);
  w.pin_plan.resize((size_t)C * 3 + G + 1);
  w.pin_out.resize((size_t)G * 32);
  static_assert(sizeof(CtChunk) == 12, "three words per chunk");
  memcpy(w.pin_plan.p, chunks.data(), (size_t)C * 12);
  memcpy(w.pin_plan.p + (size_t)C * 3, chunk_off.data(), (size_t)(G + 1) * 4);
  HIP_CHECK(hipMemcpyAsync(w.sc_dev.p, w.pin_sc.p, n * 32, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(w.plan.p, w.pin_plan.p, (size_t)C * 12, hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(w.chunk_off.p, w.pin_plan.p + (size_t)C * 3, (size_t)(G + 1) * 4, hipMemcpyHostToDevice, s));
  if (C) {
    if (K == 1)
      hipLaunchKernelGGL(k_ct_straus<1>, dim3(C), dim3(64), 0, s, w.sc_dev.p, w.pts.p, w.plan.p, w.part.p);
    else
      hipLaunchKernelGGL(k_ct_straus<2>, dim3(C), dim3(64), 0, s, w.sc_dev.p, w.pts.p, w.plan.p, w.part.p);
  }
  hipLaunchKernelGGL(k_ct_straus_sum, dim3(G), dim3(64), 0, s, w.part.p, w.chunk_off.p, w.R.p);
  hipLaunchKernelGGL(k_compress_ge, dim3(cdiv(G, 64)), dim3(64), 0, s, w.R.p, G, w.out32.p);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(w.pin_out.p, w.out32.p, (size_t)G * 32, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  memcpy(out32, w.pin_out.p, (size_t)G * 32);
  MsmForm f;
  f.valid = true;
  f.ct = true;
  f.K = K;
  f.G = G;
  f.terms = (uint32_t)n;
  ctx->msm_form = f;
  return BPP_OK;
}

}  // namespace

// =================================================================== C ABI
extern "C" {

int bpp_ctx_create_on_stream(bpp_ctx **out, int device_id, void *hip_stream) {
  if (!out) return BPP_ERR_BAD_HANDLE;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device_id < 0 || device_id >= count) return BPP_ERR_NO_DEVICE;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device_id) != hipSuccess) return BPP_ERR_NO_DEVICE;
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return BPP_ERR_NO_DEVICE;  // code object is gfx950 only
  if (hipSetDevice(device_id) != hipSuccess) return BPP_ERR_NO_DEVICE;
  bpp_ctx *c = new bpp_ctx();
  c->device = device_id;
  options_from_env(c);
  if (hip_stream) {
    c->stream = (hipStream_t)hip_stream;
  } else {
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
      delete c;
      return BPP_ERR_ENGINE;
    }
    c->own_stream = true;
  }
  {  // bookkeeping: every context brings a stream (and, for small inputs, a side stream) onto the runtime's hardware queues
    DeviceState &D = device_state(device_id);
    std::lock_guard<std::mutex> lk(D.mu);
    D.contexts++;
    D.contexts_peak = std::max(D.contexts_peak, D.contexts);
    const uint32_t q = runtime_hw_queues();
    if (D.contexts > q) {  // not an error: the call succeeds, the note sits where bpp_ctx_last_error finds it
      char note[256];
      snprintf(note, sizeof(note), "note: %u contexts on %u hardware queues (GPU_MAX_HW_QUEUES=%u, read by the HIP runtime at start-up): "
               "streams beyond that share queues and their kernels serialise; see INTEGRATION.md, runtime preconditions", D.contexts, q, q);
      c->err = note;
      D.warned = true;
    }
    if (!D.env_note.empty()) c->err = D.env_note;
  }
  *out = c;
  return BPP_OK;
}

int bpp_ctx_create(bpp_ctx **out, int device_id) { return bpp_ctx_create_on_stream(out, device_id, nullptr); }

void bpp_ctx_destroy(bpp_ctx *ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  pipeline_shutdown(ctx);  // waits for the calls in flight on the lanes, joins their threads, destroys their contexts
  prove_pipeline_shutdown(ctx);  // the same for the prove pipeline; results never collected are dropped, what it still holds is wiped
  // a call of another thread that is still inside this context (it holds the context's lock while it waits for the device) ends
  // first: destroying a context under a running call is the caller's bug, but it must not become a use of freed events
  { std::lock_guard<std::mutex> lk(ctx->mu); }
  (void)hipStreamSynchronize(ctx->stream);
  for (auto &kv : ctx->batches) wipe_batch_secrets(*kv.second, ctx->stream);  // seed nonces / masks of batches never destroyed
  (void)hipStreamSynchronize(ctx->stream);
  ctx->batches.clear();
  ctx->spare_batch.reset();
  ctx->check_spare.reset();
  for (uint64_t h : ctx->held_precomps) (void)precomp_registry().release(h);
  for (uint64_t h : ctx->held_params) (void)params_registry().release(h);
  if (ctx->ev_ready)
    for (auto &e : ctx->ev) (void)hipEventDestroy(e);
  if (ctx->ev_rng_ready) (void)hipEventDestroy(ctx->ev_rng);
  if (ctx->ev_wait_ready) (void)hipEventDestroy(ctx->ev_wait);
  for (auto &e : ctx->enq_events) (void)hipEventDestroy(e);  // (the stream has been synchronised: every ticket is retired)
  if (ctx->side_stream) {
    (void)hipStreamSynchronize(ctx->side_stream);
    (void)hipStreamDestroy(ctx->side_stream);
    (void)hipEventDestroy(ctx->ev_fork);
    (void)hipEventDestroy(ctx->ev_join);
  }
  if (ctx->chain_stream) {
    (void)hipStreamSynchronize(ctx->chain_stream);
    (void)hipStreamDestroy(ctx->chain_stream);
    (void)hipEventDestroy(ctx->ev_chain_fork);
    (void)hipEventDestroy(ctx->ev_chain_done);
  }
  ctx->scratch128.release();
  for (auto &ps : ctx->prove_streams) {
    (void)hipStreamSynchronize(ps);
    (void)hipStreamDestroy(ps);
  }
  for (auto &e : ctx->prove_events) (void)hipEventDestroy(e);
  for (auto &ps : ctx->prove_lane_streams) {
    (void)hipStreamSynchronize(ps);
    (void)hipStreamDestroy(ps);
  }
  for (auto &e : ctx->prove_sync_events) (void)hipEventDestroy(e);
  if (ctx->prove_msm_stream) {
    (void)hipStreamSynchronize(ctx->prove_msm_stream);
    (void)hipStreamDestroy(ctx->prove_msm_stream);
  }
  for (auto &ps : ctx->prove_aux_streams) {
    (void)hipStreamSynchronize(ps);
    (void)hipStreamDestroy(ps);
  }
  for (auto &e : ctx->prove_aux_events) (void)hipEventDestroy(e);
  if (ctx->prove_dev_event) (void)hipEventDestroy(ctx->prove_dev_event);
  ctx->prove_plans.clear();  // (every stream a plan's work ran on has been synchronised above)
  ctx->prove_arena.release();
  if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
  {
    DeviceState &D = device_state(ctx->device);
    std::lock_guard<std::mutex> lk(D.mu);
    if (D.contexts) D.contexts--;
  }
  delete ctx;
}

int bpp_runtime_info_get(bpp_ctx *ctx, bpp_runtime_info *out) {
  if (!ctx || !out) return BPP_ERR_BAD_HANDLE;
  memset(out, 0, sizeof(*out));
  DeviceState &D = device_state(ctx->device);
  std::lock_guard<std::mutex> lk(D.mu);
  out->device = ctx->device;
  out->contexts = D.contexts;
  out->contexts_peak = D.contexts_peak;
  out->hw_queues = runtime_hw_queues();
  out->host_threads = host_pool_size();
  out->small_call_limit = D.limit;
  out->small_calls_in_flight = D.in_flight;
  out->small_calls = D.small_calls;
  out->small_calls_queued = D.small_calls_queued;
  out->oversubscribed = D.contexts > out->hw_queues ? 1u : 0u;
  return BPP_OK;
}

int bpp_device_chain_stats(bpp_ctx *ctx, uint64_t *calls, uint64_t *redraws) {
  if (!ctx) return BPP_ERR_BAD_HANDLE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (calls) *calls = ctx->device_chain_calls + ctx->wide_chain_calls;
  if (redraws) *redraws = ctx->device_chain_redraws;
  return BPP_OK;
}

int bpp_small_call_limit(bpp_ctx *ctx, int limit) {
  if (!ctx) return BPP_ERR_BAD_HANDLE;
  return device_state(ctx->device).set_limit(limit);
}

const char *bpp_ctx_last_error(bpp_ctx *ctx) { return ctx ? ctx->err.c_str() : "null ctx"; }

int bpp_ctx_set_option(bpp_ctx *ctx, const char *name, int value) {
  if (!ctx || !name) return BPP_ERR_BAD_HANDLE;
  std::lock_guard<std::mutex> lk(ctx->mu);
  for (const OptionName &o : kOptions)
    if (strcmp(name, o.name) == 0) {
      ctx->opt.*(o.field) = value;
      return BPP_OK;
    }
  for (const TamperName &o : kTamperKnobs)
    if (strcmp(name, o.name) == 0) {  // (-1: the knob's default)
      ctx->tamper.*(o.field) = value >= 0 ? value : bpp_ctx::CheckTamper{}.*(o.field);
      return BPP_OK;
    }
  for (const VerifyTamperName &o : kVerifyTamperKnobs)
    if (strcmp(name, o.name) == 0) {
      ctx->vtamper.*(o.field) = value >= 0 ? value : 0;
      return BPP_OK;
    }
  return fail(ctx, BPP_ERR_INVALID_ARGUMENT, std::string("unknown option: ") + name);
}

#define BPP_ENTRY(ctx)                         \
  if (!(ctx)) return BPP_ERR_BAD_HANDLE;       \
  std::lock_guard<std::mutex> _lk((ctx)->mu);  \
  if (hipSetDevice((ctx)->device) != hipSuccess) return BPP_ERR_NO_DEVICE;
#define BPP_CATCH(ctx, errbuf, len)                                \
  catch (const EngineError &e) { return fail(ctx, e.code, e.msg, errbuf, len); } \
  catch (const ProofErr &e) { return fail(ctx, e.code, e.msg, errbuf, len); }    \
  catch (const std::exception &e) { return fail(ctx, BPP_ERR_ENGINE, e.what(), errbuf, len); }

// ---------------------------------------------------------------- B1
int bpp_precomp_create(bpp_ctx *ctx, const uint8_t *points32, size_t count, uint64_t *handle) {
  BPP_ENTRY(ctx);
  try {
    if (!handle || (!points32 && count)) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "null argument");
    auto pc = std::make_shared<Precomp>();
    pc->device = ctx->device;
    pc->count = (uint32_t)count;
    pc->table.alloc(count);
    if (count) {
      uint32_t bad = decompress_to_device(ctx, points32, count, pc->table.p);
      if (bad) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "point is not a canonical ristretto255 encoding");
    }
    const uint64_t h = precomp_registry().add(std::move(pc));
    ctx->held_precomps.insert(h);
    *handle = h;
    return BPP_OK;
  }
  BPP_CATCH(ctx, nullptr, 0)
}

int bpp_precomp_destroy(bpp_ctx *ctx, uint64_t handle) {
  BPP_ENTRY(ctx);
  auto it = ctx->held_precomps.find(handle);
  if (it == ctx->held_precomps.end()) return BPP_ERR_BAD_HANDLE;  // this context holds no reference on it
  ctx->held_precomps.erase(it);
  return precomp_registry().release(handle) ? BPP_OK : BPP_ERR_BAD_HANDLE;
}

int bpp_msm_mixed(bpp_ctx *ctx, uint64_t handle, const uint8_t *static_scalars32, size_t n_static,
                  const uint8_t *dyn_scalars32, const uint8_t *dyn_points32, size_t n_dyn, uint8_t out_point32[32]) {
  BPP_ENTRY(ctx);
  try {
    const std::shared_ptr<Precomp> pcp = precomp_registry().get(handle);
    if (!pcp || pcp->device != ctx->device) return fail(ctx, BPP_ERR_BAD_HANDLE, "unknown precomputation handle");
    Precomp &pc = *pcp;
    if (n_static > pc.count) return fail(ctx, BPP_ERR_INVALID_LENGTH, "more static scalars than precomputed points");
    return msm_host_entry(ctx, pc.table.p, pc.count, static_scalars32, n_static, dyn_scalars32, dyn_points32, n_dyn,
                          nullptr, 1, out_point32);
  }
  BPP_CATCH(ctx, nullptr, 0)
}

int bpp_msm_vartime(bpp_ctx *ctx, const uint8_t *scalars32, const uint8_t *points32, size_t n, uint8_t out_point32[32]) {
  BPP_ENTRY(ctx);
  try {
    return msm_host_entry(ctx, nullptr, 0, nullptr, 0, scalars32, points32, n, nullptr, 1, out_point32);
  }
  BPP_CATCH(ctx, nullptr, 0)
}

int bpp_msm_vartime_batched(bpp_ctx *ctx, const uint8_t *scalars32, const uint8_t *points32, const uint32_t *group_off,
                            size_t n_groups, uint8_t *out_points32) {
  BPP_ENTRY(ctx);
  try {
    if (!group_off || n_groups == 0) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "no groups");
    for (size_t g = 0; g < n_groups; g++)
      if (group_off[g + 1] < group_off[g]) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "group offsets not monotone");
    if (group_off[0] != 0) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "group offsets must start at 0");
    return msm_host_entry(ctx, nullptr, 0, nullptr, 0, scalars32, points32, group_off[n_groups], group_off, n_groups,
                          out_points32);
  }
  BPP_CATCH(ctx, nullptr, 0)
}

int bpp_msm_ct(bpp_ctx *ctx, const uint8_t *scalars32, const uint8_t *points32, size_t n, uint8_t out_point32[32]) {
  BPP_ENTRY(ctx);
  try {
    return msm_ct_entry(ctx, scalars32, points32, n, nullptr, 1, out_point32);
  }
  BPP_CATCH(ctx, nullptr, 0)
}

int bpp_msm_ct_batched(bpp_ctx *ctx, const uint8_t *scalars32, const uint8_t *points32, const uint32_t *group_off, size_t n_groups,
                       uint8_t *out_points32) {
  BPP_ENTRY(ctx);
  try {
    if (!group_off || n_groups == 0) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "no groups");
    for (size_t g = 0; g < n_groups; g++)
      if (group_off[g + 1] < group_off[g]) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "group offsets not monotone");
    if (group_off[0] != 0) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "group offsets must start at 0");
    return msm_ct_entry(ctx, scalars32, points32, group_off[n_groups], group_off, n_groups, out_points32);
  }
  BPP_CATCH(ctx, nullptr, 0)
}

int bpp_msm_ct_secret_bytes(bpp_ctx *ctx, uint64_t *examined, uint64_t *nonzero) {
  BPP_ENTRY(ctx);
  try {
    if (!examined || !nonzero) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "null argument");
    CtMsmWork &w = ctx->ct_msm;
    uint64_t seen = 0, cnt = 0;
    if (w.used) {
      HIP_CHECK(hipStreamSynchronize(ctx->stream));
      if (w.pin_sc.p) {
        for (size_t i = 0; i < w.pin_sc.n; i++) cnt += w.pin_sc.p[i] != 0;
        seen += w.pin_sc.n;
      }
      const std::pair<const void *, size_t> dev[2] = {{w.sc_dev.p, w.sc_dev.n * sizeof(sc)}, {w.part.p, w.part.n * sizeof(ge)}};
      for (const auto &b : dev) {
        if (!b.first || !b.second) continue;
        std::vector<uint8_t> h(b.second);
        HIP_CHECK(hipMemcpy(h.data(), b.first, b.second, hipMemcpyDeviceToHost));
        for (uint8_t v : h) cnt += v != 0;
        seen += h.size();
        wipe(h.data(), h.size());
      }
    }
    *examined = seen;
    *nonzero = cnt;
    return BPP_OK;
  }
  BPP_CATCH(ctx, nullptr, 0)
}

int bpp_msm_last_plan(bpp_ctx *ctx, uint32_t out[8]) {
  BPP_ENTRY(ctx);
  if (!out) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "null argument");
  const MsmForm &f = ctx->msm_form;
  if (!f.valid) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "no MSM has run on this context");
  if (f.ct) {  // bit 6 and the call's counts; no bucket-method word applies
    const uint32_t v[8] = {0, 0, 0, 0, f.G, f.terms, 64u, 0};
    memcpy(out, v, sizeof v);
    return BPP_OK;
  }
  const uint32_t bits = f.plain ? 32u : (f.quad ? 1u : 0u) | ((uint32_t)f.reduce << 1) | (f.final_quad ? 8u : 0u) | (f.narrow ? 16u : 0u) |
                        (f.slices ? 128u | (f.slices << 8) : 0u);  // bit 7: the sliced prelude, bits 8-15: its slices
  const uint32_t v[8] = {f.c, f.K, f.K_wide, f.nb, f.G, f.terms, bits, f.dig_cap};
  memcpy(out, v, sizeof v);
  return BPP_OK;
}

// ---------------------------------------------------------------- B2: parameters
int bpp_params_create(bpp_ctx *ctx, uint32_t bit_length, uint32_t max_aggregation, uint32_t extension_degree,
                      const uint8_t *h_base32, const uint8_t *g_bases32, uint64_t *params) {
  BPP_ENTRY(ctx);
  try {
    // RangeParameters::init checks (src/range_parameters.rs:37-51), ExtensionDegree::try_from (pedersen_gens.rs:68-82)
    if (!params) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "null argument");
    if (max_aggregation == 0 || (max_aggregation & (max_aggregation - 1)))
      return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "Aggregation factor size must be a power of two");
    if (bit_length == 0 || (bit_length & (bit_length - 1)))
      return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "Bit length must be a power of two");
    if (bit_length > 64) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "Bit length must be <= 64");
    if (extension_degree < 1 || extension_degree > 6)
      return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "Extension degree not valid");
    if ((uint64_t)bit_length * max_aggregation > 2048)
      return fail(ctx, BPP_ERR_SIZE_OVERFLOW, "bit_length * max_aggregation > 2048 is not supported by this engine");
    auto P = std::make_shared<Params>();
    P->device = ctx->device;
    P->n_bits = bit_length;
    P->m_max = max_aggregation;
    P->t = extension_degree;
    const uint32_t n = bit_length, m = max_aggregation, t = extension_degree;
    const uint32_t n_gen = 2 * n * m;
    P->table_len = n_gen + t + 1;
    P->table.alloc(P->table_len);

    // uniform bytes for every derived point: interleaved G,H (party-major), then default masking points
    const uint32_t n_uni = n_gen + 6;
    std::vector<uint8_t> uni((size_t)n_uni * 64);
    for (uint32_t party = 0; party < m; party++) {
      for (int which = 0; which < 2; which++) {
        uint8_t seed[15 + 5];
        memcpy(seed, "GeneratorsChain", 15);
        seed[15] = which ? 'H' : 'G';
        seed[16] = (uint8_t)party;
        seed[17] = (uint8_t)(party >> 8);
        seed[18] = (uint8_t)(party >> 16);
        seed[19] = (uint8_t)(party >> 24);
        std::vector<uint8_t> stream((size_t)n * 64);
        shake256(seed, sizeof(seed), stream.data(), stream.size());
        for (uint32_t i = 0; i < n; i++) memcpy(&uni[(size_t)(2 * (party * n + i) + which) * 64], &stream[(size_t)i * 64], 64);
      }
    }
    for (int k = 1; k <= 6; k++) {
      char label[64];
      int ll = snprintf(label, sizeof(label), "RISTRETTO_MASKING_BASEPOINT_%d", k);
      sha3_512((const uint8_t *)label, (size_t)ll, &uni[(size_t)(n_gen + k - 1) * 64]);
    }
    DevBuf<uint8_t> d_uni, d_comp;
    DevBuf<niels> d_pts;
    d_uni.alloc(uni.size());
    d_comp.alloc((size_t)n_uni * 32);
    d_pts.alloc(n_uni);
    HIP_CHECK(hipMemcpyAsync(d_uni.p, uni.data(), uni.size(), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_from_uniform, dim3(cdiv(n_uni, 64)), dim3(64), 0, ctx->stream, d_uni.p, n_uni, d_pts.p, d_comp.p);
    std::vector<uint8_t> comp((size_t)n_uni * 32);
    HIP_CHECK(hipMemcpyAsync(comp.data(), d_comp.p, comp.size(), hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipMemcpyAsync(P->table.p, d_pts.p, (size_t)n_gen * sizeof(niels), hipMemcpyDeviceToDevice, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    P->gi32.resize((size_t)n * m * 32);
    P->hi32.resize((size_t)n * m * 32);
    for (uint32_t i = 0; i < n * m; i++) {
      memcpy(&P->gi32[(size_t)i * 32], &comp[(size_t)(2 * i) * 32], 32);
      memcpy(&P->hi32[(size_t)i * 32], &comp[(size_t)(2 * i + 1) * 32], 32);
    }
    // Pedersen bases: H then G_k (src/ristretto.rs:67-76)
    P->hg32.resize((size_t)(1 + t) * 32);
    static const uint8_t BASEPOINT32[32] = {0xe2, 0xf2, 0xae, 0x0a, 0x6a, 0xbc, 0x4e, 0x71, 0xa8, 0x84, 0xa9,
                                            0x61, 0xc5, 0x00, 0x51, 0x5f, 0x58, 0xe3, 0x0b, 0x6a, 0xa5, 0x82,
                                            0xdd, 0x8d, 0xb6, 0xa6, 0x59, 0x45, 0xe0, 0x8d, 0x2d, 0x76};
    memcpy(&P->hg32[0], h_base32 ? h_base32 : BASEPOINT32, 32);
    for (uint32_t k = 0; k < t; k++)
      memcpy(&P->hg32[(size_t)(1 + k) * 32], g_bases32 ? g_bases32 + 32 * k : &comp[(size_t)(n_gen + k) * 32], 32);
    // table tail = [G_0..G_{t-1}, H]
    std::vector<uint8_t> tail((size_t)(t + 1) * 32);
    memcpy(&tail[0], &P->hg32[32], (size_t)t * 32);
    memcpy(&tail[(size_t)t * 32], &P->hg32[0], 32);
    uint32_t bad = decompress_to_device(ctx, tail.data(), t + 1, P->table.p + n_gen);
    if (bad) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "Pedersen base point is not a canonical ristretto255 encoding");
    // validate_and_append_point(H / G) (src/transcripts.rs:72-75): identity encodings are rejected once, here
    for (uint32_t k = 0; k < 1 + t; k++) {
      bool z = true;
      for (int i = 0; i < 32; i++) z = z && P->hg32[(size_t)k * 32 + i] == 0;
      if (z) return fail(ctx, BPP_ERR_VERIFICATION_FAILED, "Identity element cannot be added to the transcript");
    }
    P->table_hi.alloc(P->table_len);
    hipLaunchKernelGGL(k_split_shift_table, dim3(cdiv(P->table_len, 64)), dim3(64), 0, ctx->stream, P->table.p, P->table_len, P->table_hi.p);
    P->fb_ped_geo = fb_geometry(t + 1);
    P->fb_ped.alloc((size_t)(t + 1) * fb_stride(P->fb_ped_geo));
    hipLaunchKernelGGL(k_fb_build,
                       dim3(cdiv((t + 1) * P->fb_ped_geo.windows * cdiv(P->fb_ped_geo.entries, FB_BUILD_BLOCK), 64)), dim3(64), 0,
                       ctx->stream, P->table.p + n_gen, t + 1, P->fb_ped_geo, P->fb_ped.p);
    {  // j * 16^w * Base, j = 1..8, w = 0..63: the lines k_ct_fixed reads (all eight of a position, every time)
      FbGeom g4;
      g4.wbits = 4;
      g4.windows = BPP_CT_DIGITS;
      g4.entries = BPP_CTF_ENTRIES;
      g4.items = BPP_CT_DIGITS;
      P->fb_ct.alloc((size_t)(t + 1) * fb_stride(g4));
      hipLaunchKernelGGL(k_fb_build, dim3(cdiv((t + 1) * g4.windows, 64)), dim3(64), 0, ctx->stream, P->table.p + n_gen, t + 1, g4, P->fb_ct.p);
    }
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    P->d_hg32.alloc(P->hg32.size());
    HIP_CHECK(hipMemcpy(P->d_hg32.p, P->hg32.data(), P->hg32.size(), hipMemcpyHostToDevice));
    const uint64_t h = params_registry().add(std::move(P));
    ctx->held_params.insert(h);
    *params = h;
    return BPP_OK;
  }
  BPP_CATCH(ctx, nullptr, 0)
}

int bpp_params_destroy(bpp_ctx *ctx, uint64_t params) {
  BPP_ENTRY(ctx);
  auto it = ctx->held_params.find(params);
  if (it == ctx->held_params.end()) return BPP_ERR_BAD_HANDLE;  // this context holds no reference on it
  ctx->held_params.erase(it);
  // resident batches and calls in flight keep their own shared_ptr: the tables are freed when the last user is gone
  return params_registry().release(params) ? BPP_OK : BPP_ERR_BAD_HANDLE;
}

int bpp_params_retain(bpp_ctx *ctx, uint64_t params) {
  BPP_ENTRY(ctx);
  const std::shared_ptr<Params> P = params_registry().get(params);
  if (!P || P->device != ctx->device) return fail(ctx, BPP_ERR_BAD_HANDLE, "unknown params handle (or another device's)");
  if (!params_registry().retain(params)) return BPP_ERR_BAD_HANDLE;
  ctx->held_params.insert(params);
  return BPP_OK;
}

int bpp_precomp_retain(bpp_ctx *ctx, uint64_t handle) {
  BPP_ENTRY(ctx);
  const std::shared_ptr<Precomp> pc = precomp_registry().get(handle);
  if (!pc || pc->device != ctx->device) return fail(ctx, BPP_ERR_BAD_HANDLE, "unknown precomputation handle (or another device's)");
  if (!precomp_registry().retain(handle)) return BPP_ERR_BAD_HANDLE;
  ctx->held_precomps.insert(handle);
  return BPP_OK;
}

int bpp_params_export(bpp_ctx *ctx, uint64_t params, uint8_t *gi_out32, uint8_t *hi_out32, uint8_t *h_out32,
                      uint8_t *g_out32) {
  BPP_ENTRY(ctx);
  const std::shared_ptr<Params> Pp = params_registry().get(params);
  if (!Pp || Pp->device != ctx->device) return fail(ctx, BPP_ERR_BAD_HANDLE, "unknown params handle");
  Params &P = *Pp;
  if (gi_out32) memcpy(gi_out32, P.gi32.data(), P.gi32.size());
  if (hi_out32) memcpy(hi_out32, P.hi32.data(), P.hi32.size());
  if (h_out32) memcpy(h_out32, P.hg32.data(), 32);
  if (g_out32) memcpy(g_out32, P.hg32.data() + 32, (size_t)P.t * 32);
  return BPP_OK;
}

int bpp_pedersen_commit(bpp_ctx *ctx, uint64_t params, const uint64_t *values, const uint8_t *blindings32,
                        uint32_t n_blind, size_t count, uint8_t *commitments32) {
  BPP_ENTRY(ctx);
  try {
    const std::shared_ptr<Params> Pp = params_registry().get(params);
    if (!Pp || Pp->device != ctx->device) return fail(ctx, BPP_ERR_BAD_HANDLE, "unknown params handle");
    Params &P = *Pp;
    if (n_blind == 0 || n_blind > P.t) return fail(ctx, BPP_ERR_INVALID_LENGTH, "blinding vector");
    if (count == 0) return BPP_OK;
    // output j = value*H + sum_k r_k G_k over the resident fixed-base table of the Pedersen bases
    const uint32_t per = 1 + n_blind;
    std::vector<uint8_t> sb(count * per * 32, 0);  // values and blinding factors: wiped on every exit path
    DevBuf<sc> d_sc;
    ScopeExit wipe_secrets{[&] {
      wipe(sb.data(), sb.size());
      if (d_sc.p) {
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipMemset(d_sc.p, 0, d_sc.n * sizeof(sc));
      }
    }};
    std::vector<uint32_t> gidx(count * per), cnt(count, per);
    for (size_t j = 0; j < count; j++) {
      uint8_t *v = &sb[(j * per) * 32];
      for (int k = 0; k < 8; k++) v[k] = (uint8_t)(values[j] >> (8 * k));
      memcpy(v + 32, blindings32 + j * n_blind * 32, (size_t)n_blind * 32);
      for (uint32_t k = 0; k < n_blind; k++)
        if (!sc_is_canonical(v + 32 + 32 * k)) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "scalar is not canonical");
      gidx[j * per] = P.t;  // H is the last entry of fb_ped
      for (uint32_t k = 0; k < n_blind; k++) gidx[j * per + 1 + k] = k;
    }
    // value and blinding factors are secrets and nothing else: the reference commits with dalek's CONSTANT-TIME multiscalar_mul
    // (src/generators/pedersen_gens.rs:112-122).  Default here: the uniform-access form (ct.h: every table entry read, masked
    // select, no scalar-dependent address or branch).  Option "ct" = 0 takes the fixed-base tables instead, whose addresses are
    // the scalars' digits (faster by far; for callers whose values are public, e.g. the bench's input generation).
    const bool ct = ctx->opt.ct != 0;
    const uint32_t n_gen = 2 * P.n_bits * P.m_max;
    if (ct)  // indices into the parameter set's generator table: G_k at n_gen + k, H at n_gen + t
      for (size_t j = 0; j < count; j++) {
        gidx[j * per] = n_gen + P.t;
        for (uint32_t k = 0; k < n_blind; k++) gidx[j * per + 1 + k] = n_gen + k;
      }
    DevBuf<uint32_t> d_g, d_c;
    DevBuf<uint8_t> d_out;
    d_sc.alloc(count * per);
    d_g.alloc(count * per);
    d_c.alloc(count);
    d_out.alloc(count * 32);
    hipStream_t s = ctx->stream;
    HIP_CHECK(hipMemcpyAsync(d_sc.p, sb.data(), sb.size(), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_g.p, gidx.data(), gidx.size() * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(d_c.p, cnt.data(), cnt.size() * 4, hipMemcpyHostToDevice, s));
    DevBuf<ge> d_ge;
    d_ge.alloc(count);
    if (ct)
      hipLaunchKernelGGL(k_ct_fixed, dim3((uint32_t)count), dim3(64), 0, s, d_sc.p, d_g.p, d_c.p, per, n_gen, (const niels *)P.fb_ct.p, d_ge.p);
    else
      hipLaunchKernelGGL(k_fb_msm, dim3((uint32_t)count), dim3(fb_threads(ctx, per, P.fb_ped_geo)), 0, s, d_sc.p, d_g.p, d_c.p, per, P.fb_ped.p,
                         P.fb_ped_geo, d_ge.p, 0u);
    hipLaunchKernelGGL(k_compress_ge, dim3(cdiv((uint32_t)count, 64)), dim3(64), 0, s, d_ge.p, (uint32_t)count, d_out.p);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(commitments32, d_out.p, count * 32, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    return BPP_OK;
  }
  BPP_CATCH(ctx, nullptr, 0)
}

int bpp_transcript_new(const uint8_t *label, size_t label_len, uint8_t state203[203]) {
  if (!state203 || (!label && label_len)) return BPP_ERR_INVALID_ARGUMENT;
  Strobe s;
  merlin_new(s, label, (uint32_t)label_len);
  strobe_to_bytes(state203, s);
  return BPP_OK;
}

// Transcript::append_message / challenge_bytes on a 203-byte state, in place (host only: merlin.h).  A state whose position is not
// inside the block is refused, as the upload refuses it.
int bpp_transcript_append_message(uint8_t state203[203], const uint8_t *label, size_t label_len, const uint8_t *msg, size_t msg_len) {
  if (!state203 || (!label && label_len) || (!msg && msg_len)) return BPP_ERR_INVALID_ARGUMENT;
  if (label_len > 0xffffffffu || msg_len > 0xffffffffu) return BPP_ERR_INVALID_LENGTH;
  if (state203[200] >= BPP_STROBE_R) return BPP_ERR_INVALID_ARGUMENT;
  Strobe s;
  strobe_from_bytes(s, state203);
  merlin_append_message(s, label, (uint32_t)label_len, msg, (uint32_t)msg_len);
  strobe_to_bytes(state203, s);
  return BPP_OK;
}

int bpp_transcript_challenge_bytes(uint8_t state203[203], const uint8_t *label, size_t label_len, uint8_t *out, size_t out_len) {
  if (!state203 || (!label && label_len) || (!out && out_len)) return BPP_ERR_INVALID_ARGUMENT;
  if (label_len > 0xffffffffu || out_len > 0xffffffffu) return BPP_ERR_INVALID_LENGTH;
  if (state203[200] >= BPP_STROBE_R) return BPP_ERR_INVALID_ARGUMENT;
  Strobe s;
  strobe_from_bytes(s, state203);
  merlin_challenge_bytes(s, label, (uint32_t)label_len, out, (uint32_t)out_len);
  strobe_to_bytes(state203, s);
  return BPP_OK;
}

// The reference's TranscriptProtocol and merlin's transcript RNG on 203-byte states (host only): merlin.h's routines and the scalar
// routine the kernel of bpp_transcripts_enqueue runs (transcript_ops.h: top_scalar_from_wide).
int bpp_transcript_validate_and_append_point(uint8_t state203[203], const uint8_t *label, size_t label_len, const uint8_t point32[32],
                                             char *errbuf, size_t errbuf_len) {
  if (!state203 || (!label && label_len) || !point32) return BPP_ERR_INVALID_ARGUMENT;
  if (label_len > 0xffffffffu) return BPP_ERR_INVALID_LENGTH;
  if (state203[200] >= BPP_STROBE_R) return BPP_ERR_INVALID_ARGUMENT;
  uint8_t any = 0;
  for (int k = 0; k < 32; k++) any |= point32[k];
  if (!any) {
    set_err(errbuf, errbuf_len, "Identity element cannot be added to the transcript");
    return BPP_ERR_VERIFICATION_FAILED;
  }
  return bpp_transcript_append_message(state203, label, label_len, point32, 32);
}

int bpp_transcript_challenge_scalar(uint8_t state203[203], const uint8_t *label, size_t label_len, uint8_t out32[32], char *errbuf,
                                    size_t errbuf_len) {
  if (!out32) return BPP_ERR_INVALID_ARGUMENT;
  uint8_t wide[64];
  const int rc = bpp_transcript_challenge_bytes(state203, label, label_len, wide, 64);
  if (rc != BPP_OK) return rc;
  const uint32_t zero = top_scalar_from_wide(out32, wide);
  if (zero) set_err(errbuf, errbuf_len, "Transcript challenge cannot be zero");
  return zero ? BPP_ERR_VERIFICATION_FAILED : BPP_OK;
}

int bpp_transcript_rng_begin(const uint8_t state203[203], uint8_t rng203_out[203]) {
  if (!state203 || !rng203_out || state203[200] >= BPP_STROBE_R) return BPP_ERR_INVALID_ARGUMENT;
  memmove(rng203_out, state203, 203);
  return BPP_OK;
}

int bpp_transcript_rng_rekey(uint8_t rng203[203], const uint8_t *label, size_t label_len, const uint8_t *witness, size_t witness_len) {
  if (!rng203 || (!label && label_len) || (!witness && witness_len)) return BPP_ERR_INVALID_ARGUMENT;
  if (label_len > 0xffffffffu || witness_len > 0xffffffffu) return BPP_ERR_INVALID_LENGTH;
  if (rng203[200] >= BPP_STROBE_R) return BPP_ERR_INVALID_ARGUMENT;
  Strobe s;
  strobe_from_bytes(s, rng203);
  merlin_rng_rekey(s, label, (uint32_t)label_len, witness, (uint32_t)witness_len);
  strobe_to_bytes(rng203, s);
  return BPP_OK;
}

int bpp_transcript_rng_finalize(uint8_t rng203[203], const uint8_t random32[32]) {
  if (!rng203 || rng203[200] >= BPP_STROBE_R) return BPP_ERR_INVALID_ARGUMENT;
  const uint8_t zeros[32] = {0};
  Strobe s;
  strobe_from_bytes(s, rng203);
  merlin_rng_finalize(s, random32 ? random32 : zeros);
  strobe_to_bytes(rng203, s);
  return BPP_OK;
}

int bpp_transcript_rng_fill(uint8_t rng203[203], uint8_t *out, size_t out_len) {
  if (!rng203 || (!out && out_len)) return BPP_ERR_INVALID_ARGUMENT;
  if (out_len > 0xffffffffu) return BPP_ERR_INVALID_LENGTH;
  if (rng203[200] >= BPP_STROBE_R) return BPP_ERR_INVALID_ARGUMENT;
  Strobe s;
  strobe_from_bytes(s, rng203);
  merlin_rng_fill(s, out, (uint32_t)out_len);
  strobe_to_bytes(rng203, s);
  return BPP_OK;
}

int bpp_transcript_rng_scalar(uint8_t rng203[203], uint8_t out32[32], char *errbuf, size_t errbuf_len) {
  if (!out32) return BPP_ERR_INVALID_ARGUMENT;
  uint8_t wide[64];
  const int rc = bpp_transcript_rng_fill(rng203, wide, 64);
  if (rc != BPP_OK) return rc;
  const uint32_t zero = top_scalar_from_wide(out32, wide);
  volatile uint8_t *w = wide;
  for (int k = 0; k < 64; k++) w[k] = 0;
  if (zero) set_err(errbuf, errbuf_len, "Random scalar is zero");
  return zero ? BPP_ERR_VERIFICATION_FAILED : BPP_OK;
}

int bpp_weights_from_chains(const uint8_t *rng32_all, size_t n_groups, size_t n_per_group, uint8_t *weights32_out) {
  if ((!rng32_all || !weights32_out) && n_groups * n_per_group) return BPP_ERR_INVALID_ARGUMENT;
  if (n_groups == 0 || n_per_group == 0) return BPP_OK;
  if (n_groups * n_per_group > (1u << 30)) return BPP_ERR_SIZE_OVERFLOW;
  std::vector<uint32_t> first(n_groups + 1);
  for (size_t g = 0; g <= n_groups; g++) first[g] = (uint32_t)(g * n_per_group);
  run_weight_chains_generic(rng32_all, weights32_out, first.data(), (uint32_t)n_groups);
  return BPP_OK;
}

int bpp_weights_from_chain(const uint8_t *rng32_all, size_t n_total, uint8_t *weights32_out) {
  if ((!rng32_all || !weights32_out) && n_total) return BPP_ERR_INVALID_ARGUMENT;
  weights_from_chain_host(rng32_all, n_total, weights32_out);
  return BPP_OK;
}

// ---------------------------------------------------------------- B2: batches
}  // extern "C"

namespace {

// Secrets a resident batch holds on the device: the statements' seed nonces and the recovered masks (the reference wipes
// both on drop: src/range_statement.rs:76-81 `Zeroize for RangeStatement`, src/extended_mask.rs:14 `ZeroizeOnDrop`).
// Enqueued on `s`; the caller synchronises before the buffers change hands.
void wipe_batch_secrets(Batch &b, hipStream_t s) {
  if (b.seeds.p && b.seeds_dirty) (void)hipMemsetAsync(b.seeds.p, 0, b.seeds.n, s);
  if (b.masks.p && b.masks_dirty) (void)hipMemsetAsync(b.masks.p, 0, b.masks.n, s);
  b.seeds_dirty = b.masks_dirty = false;
}

// ---- host half of an upload: everything that reads the caller's buffers.  Validates and packs into ctx->pin_upload
// (proof and commitment bytes) and `pl` (descriptors, promises, seed nonces, transcript states).  Pure host work: the
// pipelined entry runs it on the submitting thread while the context's lanes are busy with earlier calls.
void upload_host_pack(bpp_ctx *ctx, const Params &P, const bpp_verify_item *items, size_t n_items, const bpp_packed_batch *packed,
                      UploadPlan &pl) {
  const ParallelFor pf = [](uint32_t n, const std::function<void(uint32_t)> &fn) { host_parallel_for(n, fn); };
  const ParamShape shape{P.n_bits, P.m_max, P.t};
  std::vector<bpp_verify_item> synth;  // packed input that is not uniform after all (hostile / mixed): the item form
  const bool arithmetic = packed && upload_pass_a_packed(*packed, pl, pf);
  if (packed && !arithmetic) {
    upload_packed_as_items(*packed, synth);
    items = synth.data();
    n_items = synth.size();
  }
  if (!arithmetic) upload_pass_a(items, n_items, pl);
  // Proof and commitment bytes are assembled directly in page-locked staging: a pageable source makes hipMemcpyAsync
  // return early and the 40 MB transfer trickle on at ~2.4 GB/s behind the call (it showed up as 23 ms in the first
  // verification of every freshly uploaded batch)
  ctx->pin_upload.resize(pl.bytes_total + BPP_BYTES_SLACK);
  uint8_t *bytes = ctx->pin_upload.data();
  memset(bytes + pl.bytes_total, 0, BPP_BYTES_SLACK);
  if (arithmetic) upload_pass_b_packed(*packed, shape, pl, bytes, pf);
  else upload_pass_b(items, shape, pl, bytes, pf);
}

// a batch to fill: the buffers of the last destroyed one serve again
std::unique_ptr<Batch> new_batch(bpp_ctx *ctx) {
  auto B = std::make_unique<Batch>();
  if (ctx->spare_batch) {
    adopt_buffers(*B, *ctx->spare_batch);
    ctx->spare_batch.reset();
  }
  return B;
}

// ---- device half: staging -> HBM, slot lists, statement commitments decoded; consumes `pl`.
// `filled`: a batch whose proof and commitment bytes, promises and seed nonces k_ingest_packed has already written where they
// belong (upload_packed_device); only the descriptors and the transcript state then come from the host.
uint64_t upload_device(bpp_ctx *ctx, const std::shared_ptr<Params> &Pp, uint64_t params, UploadPlan &pl,
                       const uint8_t *const *challenges32, const uint8_t *rng_out32, std::unique_ptr<Batch> filled = nullptr) {
    Params &P = *Pp;
    const size_t n_items = pl.n_items;
    const bool resident = filled != nullptr;
    std::unique_ptr<Batch> B = resident ? std::move(filled) : new_batch(ctx);
    hipStream_t s = ctx->stream;
    // seed nonces pass through page-locked staging and reach the device: both are wiped on EVERY way out of here
    SmallStaging L;
    bool registered = false;
    ScopeExit wipe_secrets{[&] {
      if (L.n_seed) {
        (void)hipStreamSynchronize(s);  // the copy out of the staging may still be running
        upload_wipe_small(ctx->pin_upload2.data(), L);
      }
      secure_wipe(pl.seeds.data(), pl.seeds.size());
      if (!registered && B) {  // an error exit: the half-built batch dies here and must not leave nonces behind
        wipe_batch_secrets(*B, s);
        (void)hipStreamSynchronize(s);
      }
    }};
    B->params = Pp;
    B->params_handle = params;
    B->B = (uint32_t)n_items;
    const uint8_t *bytes = ctx->pin_upload.data();
    const size_t bytes_len = pl.bytes_total + BPP_BYTES_SLACK;
    B->desc.swap(pl.desc);
    B->rounds_bad.swap(pl.rounds_bad);
    B->defer.swap(pl.defer);
    B->any_seed = pl.any_seed;
    B->any_rounds_bad = pl.any_rounds_bad;
    B->any_defer = pl.any_defer;
    B->uniform_rounds = pl.uniform_rounds;
    B->rmax = pl.rmax;
    B->max_mn = pl.max_mn;
    const std::vector<uint8_t> &seeds = pl.seeds, &states = pl.states;
    const std::vector<uint64_t> &minvals = pl.minvals;
    const size_t sum_m = pl.sum_m;
    const uint32_t dyn = pl.total_dyn;
    B->total_dyn = dyn;
    B->sum_m = (uint32_t)sum_m;
    // challenge slots per proof: y, z, e_0.., e_final.  A proof claiming more rounds than any statement can have (mn <= 2048)
    // is refused on the host; its transcript is still replayed for the error precedence, its challenges are not kept, so
    // one such proof cannot inflate the whole batch's buffers.
    B->cs = std::min(B->rmax, (uint32_t)BPP_MAX_ROUNDS - 1) + 3;
    B->cols = 2 * B->max_mn + P.t + 1;
    // device copies (all sources page-locked: the copies are real stream-ordered DMA)
    B->bytes.alloc(bytes_len);
    if (!(resident && B->item_states)) B->states.alloc(states.size());  // (else: one row per item, written by k_item_states)
    // (a buffer that holds secrets at times starts out zero: a batch that fails before anything is written to it leaves no stale
    // bytes of an earlier allocation there for bpp_batch_secret_bytes to count)
    auto alloc_zeroed = [&](DevBuf<uint8_t> &buf, size_t count) {
      const bool fresh = !(buf.p && count <= buf.n);
      buf.alloc(count);
      if (fresh) HIP_CHECK(hipMemsetAsync(buf.p, 0, buf.n, s));
    };
    if (!resident) alloc_zeroed(B->seeds, B->any_seed ? seeds.size() : 0);
    B->d_desc.alloc(n_items);
    if (!resident) B->minvals.alloc(minvals.size());
    B->src_off.alloc(dyn);
    B->owner.alloc(dyn);
    B->idx_commit.alloc(sum_m);
    B->idx_proof.alloc(dyn - sum_m);
    {
      const SmallStaging Lp = upload_small_layout(pl, n_items);
      ctx->pin_upload2.resize(Lp.total + 64);
      uint8_t *st = ctx->pin_upload2.data();
      L = Lp;  // from here on the staging holds nonces (if any)
      upload_fill_small(pl, B->desc.data(), n_items, st, L);
      // ONE launch reads the pieces out of the mapped staging (k_ingest) and clears the two status arrays; only the proof
      // bytes of a large batch (tens of MB) go by DMA.  (Six copies / memsets were six blit kernels in front of every call.)
      B->status0.alloc(n_items);
      B->status.alloc(n_items);
      uint8_t *st_dev = ctx->pin_upload2.dev();
      IngestArgs ia;
      memset(&ia, 0, sizeof(ia));
      auto seg = [&](const uint8_t *src, void *dst, size_t nbytes) {
        if (nbytes) ia.seg[ia.n_seg++] = IngestSeg{src, (uint8_t *)dst, nbytes};
      };
      const bool bytes_by_dma = bytes_len > BPP_INGEST_MAX_BYTES;
      if (resident) {
        // (already in B->bytes / minvals / seeds: pl.minvals and pl.seeds are empty)
      } else if (bytes_by_dma) {
        HIP_CHECK(hipMemcpyAsync(B->bytes.p, bytes, bytes_len, hipMemcpyHostToDevice, s));
      } else {
        seg(ctx->pin_upload.dev(), B->bytes.p, bytes_len);
      }
      seg(st_dev + L.o_desc, B->d_desc.p, n_items * sizeof(ProofDesc));
      seg(st_dev + L.o_min, B->minvals.p, minvals.size() * 8);
      seg(st_dev + L.o_state, B->states.p, states.size());
      if (L.n_seed) {
        B->seeds_dirty = true;
        seg(st_dev + L.o_seed, B->seeds.p, L.n_seed);
      }
      ia.zero[0] = B->status0.p;
      ia.zero[1] = B->status.p;
      ia.zero_words = (uint32_t)n_items;
      size_t most = n_items * 4;
      for (uint32_t q = 0; q < ia.n_seg; q++) most = std::max<size_t>(most, ia.seg[q].bytes);
      hipLaunchKernelGGL(k_ingest, dim3((uint32_t)std::min<size_t>(2048, std::max<size_t>(1, most / (16 * 256)))), dim3(256), 0, s, ia);
      HIP_CHECK(hipGetLastError());
    }
    // point sources in dynamic-slot order C_j.., A1, B, A, L.., R.. and the two slot lists, written by one lane per proof
    hipLaunchKernelGGL(k_build_slots, dim3(cdiv((uint32_t)n_items, 64)), dim3(64), 0, s, B->d_desc.p, (uint32_t)n_items, P.t,
                       B->src_off.p, B->owner.p, B->idx_commit.p, B->idx_proof.p);
    HIP_CHECK(hipGetLastError());
    // work buffers
    B->chal.alloc((size_t)n_items * B->cs);
    B->rng_out.alloc(n_items * 32);
    B->weights.alloc(n_items * 32);
    B->dynpts.alloc(dyn);
    if (decompress_spill_enabled()) B->dec_spill.alloc((size_t)30 * (dyn - B->sum_m));
    // (rows / parts: sized by layout_groups, which knows whether the generator columns are summed inside k_scalars_lanes)
    B->shr.alloc((size_t)n_items * SH_STRIDE);
    B->tab.alloc((size_t)n_items * lanes_tab_stride(B->lanes_nhi_max(P.n_bits)));
    alloc_zeroed(B->masks, n_items * P.t * 32);
    B->h_rng.resize(n_items * 32);
    B->h_weights.resize(n_items * 32);
    B->h_status.resize(n_items);
    if (challenges32) {
      // caller-side Fiat-Shamir: challenges arrive canonical, are kept in Montgomery form like k_transcripts' output
      if (!rng_out32) throw ProofErr{BPP_ERR_INVALID_ARGUMENT, "rng_out32 is required with external challenges"};
      B->ext_challenges = true;
      B->ext_status.assign(n_items, 0);
      std::vector<sc> hc((size_t)n_items * B->cs);
      memset(hc.data(), 0, hc.size() * sizeof(sc));
      for (size_t i = 0; i < n_items; i++) {
        const ProofDesc &d = B->desc[i];
        if (!challenges32[i]) throw ProofErr{BPP_ERR_INVALID_ARGUMENT, "missing challenges for a proof"};
        for (uint32_t k = 0; k < d.rounds + 3; k++) {
          const uint8_t *c = challenges32[i] + 32 * (size_t)k;
          if (!sc_is_canonical(c)) throw ProofErr{BPP_ERR_INVALID_ARGUMENT, "challenge is not canonical"};
          sc v;
          sc_load_words(v, c);
          if (sc_iszero(v)) B->ext_status[i] |= BPP_ST_TRANSCRIPT_FAIL;  // transcript_protocol.rs:71-77
          sc_to_mont(v, v);
          if (k < B->cs) hc[i * B->cs + k] = v;
        }
        // validate_and_append_point (transcript_protocol.rs:48-61): A, A1, B, L_j, R_j must not be the identity encoding
        if (B->defer[i] & BPP_DEFER_DEGREE) continue;  // other layout: its chunk fails before PASS 1 is looked at
        const uint8_t *pA = bytes + d.proof_off + 1 + 32 * P.t;  // the staged copy of the proof
        auto zero32 = [](const uint8_t *p) {
          uint8_t r = 0;
          for (int k = 0; k < 32; k++) r |= p[k];
          return r == 0;
        };
        bool ident = zero32(pA) || zero32(pA + 32) || zero32(pA + 64);
        for (uint32_t j = 0; j < 2 * d.rounds; j++) ident = ident || zero32(pA + 160 + 32 * j);
        if (ident) B->ext_status[i] |= BPP_ST_TRANSCRIPT_FAIL;
      }
      HIP_CHECK(hipMemcpyAsync(B->chal.p, hc.data(), hc.size() * sizeof(sc), hipMemcpyHostToDevice, s));
      memcpy(B->h_rng.data(), rng_out32, n_items * 32);
      HIP_CHECK(hipMemcpyAsync(B->rng_out.p, rng_out32, n_items * 32, hipMemcpyHostToDevice, s));
      B->d_ext_status.alloc(n_items);
      HIP_CHECK(hipMemcpyAsync(B->d_ext_status.p, B->ext_status.data(), n_items * 4, hipMemcpyHostToDevice, s));
    }
    // initial per-proof status of every verification of this batch: caller-side PASS-1 findings (if any) and the
    // statement's commitments, decoded here once (the reference's RangeStatement holds decompressed points)
    // (k_ingest cleared status0[] and status[]; commitments that do not decode are recorded in both: every verification finds
    // status[] == status0[] and leaves it so (k_results_out), no copy in front of PASS 1)
    if (B->ext_challenges) {
      HIP_CHECK(hipMemcpyAsync(B->status0.p, B->d_ext_status.p, n_items * 4, hipMemcpyDeviceToDevice, s));
      HIP_CHECK(hipMemcpyAsync(B->status.p, B->d_ext_status.p, n_items * 4, hipMemcpyDeviceToDevice, s));
    }
    if (B->sum_m)
      hipLaunchKernelGGL(k_decompress, dim3(cdiv(B->sum_m, 64)), dim3(64), 0, s, B->bytes.p, B->src_off.p, B->owner.p,
                         B->idx_commit.p, B->sum_m, B->dynpts.p, B->status0.p, (uint32_t *)nullptr, B->status.p);
    HIP_CHECK(hipGetLastError());
    B->status_clean = true;
    HIP_CHECK(hipStreamSynchronize(s));
    const uint64_t h = g_next_handle.fetch_add(1);
    ctx->batches[h] = std::move(B);
    registered = true;
    return h;
}

int upload_impl(bpp_ctx *ctx, uint64_t params, const bpp_verify_item *items, size_t n_items, const bpp_packed_batch *packed,
                uint64_t *batch, const uint8_t *const *challenges32, const uint8_t *rng_out32, char *errbuf, size_t errbuf_len) {
  try {
    const std::shared_ptr<Params> Pp = params_registry().get(params);
    if (!Pp || Pp->device != ctx->device) return fail(ctx, BPP_ERR_BAD_HANDLE, "unknown params handle", errbuf, errbuf_len);
    if (packed) n_items = packed->n_items;
    // verify_batch: by definition an empty batch fails (src/range_proof.rs:719-723)
    if ((!items && !packed) || n_items == 0 || !batch)
      return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "Range statements or proofs length empty", errbuf, errbuf_len);
    if (n_items > (1u << 24)) return fail(ctx, BPP_ERR_SIZE_OVERFLOW, "batch too large", errbuf, errbuf_len);
    UploadPlan pl;
    PlanWipe wipe_plan{pl};
    upload_host_pack(ctx, *Pp, items, n_items, packed, pl);
    *batch = upload_device(ctx, Pp, params, pl, challenges32, rng_out32);
    return BPP_OK;
  }
  BPP_CATCH(ctx, errbuf, errbuf_len)
}

// ---- the packed form from arrays in device memory (ingest.h)
// one host function over hipPointerGetAttributes; a pointer the runtime does not know makes it fail, and that error must not
// stay behind for the next hipGetLastError
int device_pointer_kind(int device, const void *p) {
  hipPointerAttribute_t at;
  memset(&at, 0, sizeof(at));
  if (!p || hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();
    return BPP_PTR_HOST_OR_UNKNOWN;
  }
  if (at.isManaged || at.type == hipMemoryTypeManaged) return BPP_PTR_MANAGED;
  if (at.type == hipMemoryTypeDevice) return at.device == device ? BPP_PTR_THIS_DEVICE : BPP_PTR_OTHER_DEVICE;
  return BPP_PTR_HOST_OR_UNKNOWN;
}

// the words of the upload refusals for a pointer that is not BPP_PTR_THIS_DEVICE, by kind
const char *const upload_pointer_kinds[] = {"", "memory of another device", "host memory or memory the runtime does not know", "managed memory"};

// what both device uploads refuse first: one of the caller's six arrays this device cannot read.  Nothing is allocated or launched for
// such an array, and no array is ever dereferenced on the host.  Empty: nothing to refuse.
template <class In>  // bpp_packed_batch or bpp_mixed_batch
std::string upload_arrays_refusal(bpp_ctx *ctx, const In &in) {
  const struct {
    const char *name;
    const void *p;
  } arrays[] = {{"proofs", in.proofs},           {"commitments32", in.commitments32}, {"min_values", in.min_values},
                {"min_present", in.min_present}, {"seed_nonces32", in.seed_nonces32}, {"seed_present", in.seed_present}};
  for (const auto &a : arrays) {
    if (!a.p) continue;
    const int kind = device_pointer_kind(ctx->device, a.p);
    if (kind != BPP_PTR_THIS_DEVICE)
      return std::string(a.name) + " is not device memory of this context's device (" + upload_pointer_kinds[kind] + ")";
  }
  return std::string();
}

// The staging behind both fall-backs: the caller's arrays are copied to page-locked memory -- proofs_n bytes of proofs as they lie, or
// gathered back to back, gather_len of every row, when gather_len is not 0; `entries` entries of the three per-commitment arrays; the
// per-item arrays; the state rows of a *_transcripts upload (item_states, else null) -- and `pack(host, states)` makes the batch of the
// staged copy `host` of `in`.  The staged nonces are wiped on every way out.
template <class In, class Pack>
uint64_t upload_staged(bpp_ctx *ctx, const In &in, size_t proofs_n, size_t entries, size_t gather_len, const uint8_t *item_states, Pack &&pack) {
  const size_t n = in.n_items, n_states = item_states ? n * (size_t)BPP_ITEM_STATE_BYTES : 0;
  auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
  const size_t o_proofs = 0, o_commit = up16(proofs_n), o_minv = up16(o_commit + (in.commitments32 ? entries * 32 : 0)),
               o_minp = up16(o_minv + (in.min_values ? entries * 8 : 0)), o_seedp = up16(o_minp + (in.min_present ? entries : 0)),
               o_states = up16(o_seedp + (in.seed_present ? n : 0)), o_seed = up16(o_states + n_states), n_seed = in.seed_nonces32 ? n * 32 : 0,
               total = o_seed + n_seed;
  ctx->pin_fallback.resize(total + 16);
  uint8_t *st = ctx->pin_fallback.data();
  hipStream_t s = ctx->stream;
  ScopeExit wipe_staged{[&] {
    if (n_seed) {
      (void)hipStreamSynchronize(s);  // the copy into the staging may still be running
      secure_wipe(st + o_seed, n_seed);
    }
  }};
  In host = in;
  auto fetch = [&](const void *src, size_t off, size_t bytes) -> const uint8_t * {
    if (!src) return nullptr;
    if (bytes) HIP_CHECK(hipMemcpyAsync(st + off, src, bytes, hipMemcpyDeviceToHost, s));
    return st + off;
  };
  if (gather_len) {
    HIP_CHECK(hipMemcpy2DAsync(st + o_proofs, gather_len, in.proofs, in.proof_stride, gather_len, n, hipMemcpyDeviceToHost, s));
    host.proofs = st + o_proofs;
    host.proof_stride = gather_len;
  } else {
    host.proofs = fetch(in.proofs, o_proofs, proofs_n);
  }
  host.commitments32 = fetch(in.commitments32, o_commit, entries * 32);
  host.min_values = (const uint64_t *)fetch(in.min_values, o_minv, entries * 8);
  host.min_present = fetch(in.min_present, o_minp, entries);
  host.seed_present = fetch(in.seed_present, o_seedp, n);
  host.seed_nonces32 = fetch(in.seed_nonces32, o_seed, n_seed);
  const uint8_t *states = fetch(item_states, o_states, n_states);
  HIP_CHECK(hipStreamSynchronize(s));
  ctx->ingest_stats.host_fallback_calls++;
  ctx->ingest_stats.fallback_bytes += proofs_n + (in.commitments32 ? entries * 32 : 0) + (in.min_values ? entries * 8 : 0) +
                                      (in.min_present ? entries : 0) + (in.seed_present ? n : 0) + n_seed + n_states;
  return pack(host, states);
}

// the staged batch through the item form, item i under row i of `states` where there are any
uint64_t upload_staged_items(bpp_ctx *ctx, const std::shared_ptr<Params> &Pp, uint64_t params, std::vector<bpp_verify_item> &items,
                             const uint8_t *states) {
  for (size_t i = 0; states && i < items.size(); i++) items[i].transcript_state = states + i * (size_t)BPP_ITEM_STATE_BYTES;
  UploadPlan pl;
  PlanWipe wipe_plan{pl};
  upload_host_pack(ctx, *Pp, items.data(), items.size(), nullptr, pl);
  return upload_device(ctx, Pp, params, pl, nullptr, nullptr);
}

// what the two *_transcripts uploads refuse before anything else is looked at: the struct's own transcript fields, and a state array
// that is null or not this device's memory.  Empty: nothing to refuse.
std::string item_states_refusal(bpp_ctx *ctx, const uint8_t *transcript_state, const uint8_t *transcript_label, const uint8_t *item_states,
                                const char *name) {
  if (transcript_state) return std::string("transcript_state must be null: item i is verified under row i of ") + name;
  if (transcript_label) return std::string("transcript_label must be null: item i is verified under row i of ") + name;
  if (!item_states) return std::string(name) + " is null";
  const int kind = device_pointer_kind(ctx->device, item_states);
  if (kind != BPP_PTR_THIS_DEVICE) return std::string(name) + " is not device memory of this context's device (" + upload_pointer_kinds[kind] + ")";
  return std::string();
}

// k_item_states behind the ingest kernel of an upload: every row of the run is live; the finding goes into the ingest result word
void launch_item_states_upload(bpp_ctx *ctx, Batch &B, const uint8_t *item_states, size_t n_items, size_t n_run) {
  B.states.alloc(n_items * (size_t)BPP_ITEM_STATE_BYTES);
  const ItemStates a{item_states, B.states.p, (uint32_t)n_items, (uint32_t)n_run, ctx->ingest_res.p + BPP_ING_RES_FINDING, nullptr, nullptr};
  hipLaunchKernelGGL(k_item_states, dim3((uint32_t)cdiv((uint32_t)n_items, BPP_INGEST_BLOCK / BPP_INGEST_LANES)), dim3(BPP_INGEST_BLOCK), 0,
                     ctx->stream, a);
  HIP_CHECK(hipGetLastError());
}

// the plan of such a batch: no table from the host, item i under row i
void plan_item_states(UploadPlan &pl) {
  pl.states.clear();
  for (size_t i = 0; i < pl.desc.size(); i++) pl.desc[i].state_idx = (uint32_t)i;
}

// ---- the mixed form (bpp_mixed_batch): host arrays through the item form, device arrays through upload_device_form below
int upload_mixed_impl(bpp_ctx *ctx, uint64_t params, const bpp_mixed_batch *in, uint64_t *batch, char *errbuf, size_t errbuf_len) {
  try {
    if (!in) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "Range statements or proofs length empty", errbuf, errbuf_len);
    const std::shared_ptr<Params> Pp = params_registry().get(params);
    if (!Pp || Pp->device != ctx->device) return fail(ctx, BPP_ERR_BAD_HANDLE, "unknown params handle", errbuf, errbuf_len);
    const size_t n_items = in->n_items;
    if (n_items == 0 || !batch) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "Range statements or proofs length empty", errbuf, errbuf_len);
    if (n_items > (1u << 24)) return fail(ctx, BPP_ERR_SIZE_OVERFLOW, "batch too large", errbuf, errbuf_len);
    upload_mixed_geometry(*in);
    std::vector<bpp_verify_item> items;
    upload_mixed_as_items(*in, items);
    UploadPlan pl;
    PlanWipe wipe_plan{pl};
    upload_host_pack(ctx, *Pp, items.data(), n_items, nullptr, pl);
    *batch = upload_device(ctx, Pp, params, pl, nullptr, nullptr);
    return BPP_OK;
  }
  BPP_CATCH(ctx, errbuf, errbuf_len)
}

// ---- the two device uploads (ingest.h): one flow, upload_device_form, over what the packed and the mixed form supply -- the prelude,
// the sizes, the kernel and its arguments, the plan, the staged fall-back and the shape a refill must keep.
struct PackedUpload {
  const bpp_packed_batch &in;
  ParamShape shape{};

  std::string host_arrays_refusal(bpp_ctx *) const { return std::string(); }
  bool prelude(const ParamShape &P) {  // false: the arithmetic layout does not fit (no proofs, a stride below the length)
    shape = P;
    return ingest_host_prelude(in, P);
  }
  size_t sum_m() const { return in.n_items * (size_t)in.m; }
  size_t bytes_total() const { return in.n_items * in.proof_len + sum_m() * 32; }
  Ingest args(bpp_ctx *ctx, Batch &B, hipStream_t, bool) const {
    return ingest_args(in, shape, B.bytes.p, B.minvals.p, B.seeds.p, ctx->ingest_info.p, ctx->ingest_res.p);
  }
  static auto kernel() { return k_ingest_packed; }
  void plan(const uint32_t *res, const uint8_t *info, UploadPlan &pl) const { ingest_finish_plan(in, shape, res, info, pl); }
  // a stride above the length is gathered back to back; empty proofs: the item form reads none of them, whatever the stride
  uint64_t fallback(bpp_ctx *ctx, const std::shared_ptr<Params> &Pp, uint64_t params, const uint8_t *item_states) const {
    const size_t n = in.n_items;
    const bool no_bytes = !in.proofs || in.proof_len < 1, strided = !no_bytes && in.proof_stride > in.proof_len;
    const size_t proofs_n = no_bytes ? 0 : (strided ? n * in.proof_len : (n - 1) * in.proof_stride + in.proof_len);
    return upload_staged(ctx, in, proofs_n, n * (size_t)in.m, strided ? in.proof_len : 0, item_states,
                         [&](bpp_packed_batch &host, const uint8_t *states) {
                           if (no_bytes) host.proof_stride = 0;
                           if (states) {
                             std::vector<bpp_verify_item> items;
                             upload_packed_as_items(host, items);
                             return upload_staged_items(ctx, Pp, params, items, states);
                           }
                           UploadPlan pl;
                           PlanWipe wipe_plan{pl};
                           upload_host_pack(ctx, *Pp, nullptr, n, &host, pl);
                           return upload_device(ctx, Pp, params, pl, nullptr, nullptr);
                         });
  }
  void record_shape(Batch &made) {  // (bpp_batch_refill_enqueue: everything the plan was made from but the bytes)
    made.refillable = true;
    made.refill_shape.proof_len = in.proof_len;
    made.refill_shape.m = in.m;
  }
};

// the two host arrays of a mixed batch are dereferenced on the host, and so must not be memory of a device.  Empty: nothing to refuse.
std::string mixed_host_arrays_refusal(bpp_ctx *ctx, const bpp_mixed_batch &in, const char *what_it_does) {
  const struct {
    const char *name;
    const void *p;
  } host_arrays[] = {{"proof_lens", in.proof_lens}, {"m", in.m}};
  for (const auto &a : host_arrays) {
    const int kind = device_pointer_kind(ctx->device, a.p);
    if (kind == BPP_PTR_THIS_DEVICE || kind == BPP_PTR_OTHER_DEVICE)
      return std::string(a.name) + " is device memory: it " + what_it_does + " and stays host memory in every form";
  }
  return std::string();
}

struct MixedUpload {
  const bpp_mixed_batch &in;
  ParamShape shape{};
  IngestMixedPrelude pre{};

  std::string host_arrays_refusal(bpp_ctx *ctx) const { return mixed_host_arrays_refusal(ctx, in, "sizes the layout"); }
  bool prelude(const ParamShape &P) {  // false: no proofs array
    shape = P;
    if (!ingest_mixed_host_prelude(in, P, pre)) return false;
    if (pre.h == 0) ingest_mixed_throw_finding(pre, in.n_items, nullptr);  // item 0's, host-known: nothing to run
    return true;
  }
  size_t sum_m() const { return (size_t)pre.sum_m; }
  size_t bytes_total() const { return (size_t)(pre.proof_bytes + pre.sum_m * 32); }
  // mixed only: the table goes up in front of the run, and a fresh nonce buffer starts out zero -- the run may stop short of the last
  // item, and every buffer that holds secrets at times starts that way
  Ingest args(bpp_ctx *ctx, Batch &B, hipStream_t s, bool fresh_seeds) const {
    const size_t n = in.n_items;
    if (fresh_seeds) HIP_CHECK(hipMemsetAsync(B.seeds.p, 0, B.seeds.n, s));
    B.mixed_table.alloc(n);
    ctx->pin_mixed_table.resize(n);
    memcpy(ctx->pin_mixed_table.data(), pre.rows.data(), n * sizeof(IngestMixedRow));
    HIP_CHECK(hipMemcpyAsync(B.mixed_table.p, ctx->pin_mixed_table.data(), n * sizeof(IngestMixedRow), hipMemcpyHostToDevice, s));
    return ingest_mixed_args(in, shape, pre, B.mixed_table.p, B.bytes.p, B.minvals.p, B.seeds.p, ctx->ingest_info.p, ctx->ingest_res.p);
  }
  static auto kernel() { return k_ingest_mixed; }
  // (with h < n_items the plan throws the call's finding, the device's before the host's at h, before it looks at anything else)
  void plan(const uint32_t *res, const uint8_t *info, UploadPlan &pl) const { ingest_mixed_finish_plan(in, shape, pre, res, info, pl); }
  // the arrays are staged as they lie: rows, slack and all, up to the last byte the last row uses
  uint64_t fallback(bpp_ctx *ctx, const std::shared_ptr<Params> &Pp, uint64_t params, const uint8_t *item_states) const {
    const size_t n = in.n_items;
    return upload_staged(ctx, in, in.proofs ? (n - 1) * in.proof_stride + in.proof_lens[n - 1] : 0, (n - 1) * (size_t)in.m_stride + in.m[n - 1], 0,
                         item_states, [&](bpp_mixed_batch &host, const uint8_t *states) {
                           std::vector<bpp_verify_item> items;
                           upload_mixed_as_items(host, items);
                           return upload_staged_items(ctx, Pp, params, items, states);
                         });
  }
  void record_shape(Batch &made) {  // (bpp_batch_refill_enqueue_mixed: the vector the plan was made from)
    made.mixed = true;
    made.mixed_shape.seed_present = in.seed_present != nullptr;
    made.mixed_shape.proof_bytes = pre.proof_bytes;
    for (const IngestMixedRow &r : pre.rows) {
      made.mixed_shape.max_proof_len = std::max(made.mixed_shape.max_proof_len, r.proof_len);
      made.mixed_shape.max_m = std::max(made.mixed_shape.max_m, r.m);
    }
    made.mixed_shape.rows = std::move(pre.rows);
  }
};

// with_states (the *_transcripts uploads): item i is verified under row i of item_states (item_states.h)
template <class Form, class In>
int upload_device_form(bpp_ctx *ctx, uint64_t params, const In *in, uint64_t *batch, char *errbuf, size_t errbuf_len, bool with_states = false,
                       const uint8_t *item_states = nullptr) {
  try {
    if (!in) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "Range statements or proofs length empty", errbuf, errbuf_len);
    Form form{*in};
    std::string refusal = with_states ? item_states_refusal(ctx, in->transcript_state, in->transcript_label, item_states, "item_states203") : std::string();
    if (refusal.empty()) refusal = upload_arrays_refusal(ctx, *in);  // pointer kinds before anything is allocated or launched
    if (refusal.empty()) refusal = form.host_arrays_refusal(ctx);
    if (!refusal.empty()) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, refusal, errbuf, errbuf_len);
    const std::shared_ptr<Params> Pp = params_registry().get(params);
    if (!Pp || Pp->device != ctx->device) return fail(ctx, BPP_ERR_BAD_HANDLE, "unknown params handle", errbuf, errbuf_len);
    const size_t n_items = in->n_items;
    if (n_items == 0 || !batch) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "Range statements or proofs length empty", errbuf, errbuf_len);
    if (n_items > (1u << 24)) return fail(ctx, BPP_ERR_SIZE_OVERFLOW, "batch too large", errbuf, errbuf_len);
    if (!form.prelude(ParamShape{Pp->n_bits, Pp->m_max, Pp->t})) {
      *batch = form.fallback(ctx, Pp, params, item_states);
      return BPP_OK;
    }
    hipStream_t s = ctx->stream;
    std::unique_ptr<Batch> B = new_batch(ctx);
    ScopeExit wipe_unfinished{[&] {  // B still here: an error or the fall-back.  The nonces the kernel brought in go before its buffers do
      if (B) {
        wipe_batch_secrets(*B, s);
        (void)hipStreamSynchronize(s);
      }
    }};
    B->bytes.alloc(form.bytes_total() + BPP_BYTES_SLACK);  // (< 4 GB: the prelude)
    B->minvals.alloc(form.sum_m());
    const bool fresh_seeds = in->seed_nonces32 && !(B->seeds.p && n_items * 32 <= B->seeds.n);
    if (in->seed_nonces32) B->seeds.alloc(n_items * 32);
    ctx->ingest_res.alloc(BPP_ING_RES_WORDS);
    ctx->ingest_info.alloc(n_items);
    ctx->pin_ingest.resize(BPP_ING_RES_WORDS);
    const Ingest a = form.args(ctx, *B, s, fresh_seeds);
    HIP_CHECK(hipMemsetAsync(ctx->ingest_res.p, 0, BPP_ING_RES_WORDS * 4, s));
    B->seeds_dirty = in->seed_nonces32 != nullptr;
    hipLaunchKernelGGL(Form::kernel(), dim3((uint32_t)cdiv(a.n_run, BPP_INGEST_BLOCK / BPP_INGEST_LANES)), dim3(BPP_INGEST_BLOCK), 0, s, a);
    HIP_CHECK(hipGetLastError());
    if (with_states) launch_item_states_upload(ctx, *B, item_states, n_items, a.n_run);  // (rows at and beyond a host finding: not read)
    uint32_t *res = ctx->pin_ingest.data();
    HIP_CHECK(hipMemcpyAsync(res, ctx->ingest_res.p, BPP_ING_RES_WORDS * 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (res[BPP_ING_RES_DIFFERS]) {  // mixed first bytes: the host path, item form and all
      wipe_batch_secrets(*B, s);
      (void)hipStreamSynchronize(s);
      ctx->spare_batch = std::move(B);  // its buffers serve the host path's batch
      *batch = form.fallback(ctx, Pp, params, item_states);
      return BPP_OK;
    }
    const uint8_t *info = nullptr;
    if (!res[BPP_ING_RES_FINDING] && ingest_needs_info(*in, res)) {  // (with a finding the call ends in the plan: nothing else is fetched)
      ctx->pin_ingest_info.resize(n_items);
      HIP_CHECK(hipMemcpyAsync(ctx->pin_ingest_info.data(), ctx->ingest_info.p, n_items, hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
      info = ctx->pin_ingest_info.data();
    }
    UploadPlan pl;
    form.plan(res, info, pl);  // throws the lowest-index construction finding
    if (with_states) plan_item_states(pl);
    B->item_states = with_states;
    ctx->ingest_stats.device_calls++;
    *batch = upload_device(ctx, Pp, params, pl, nullptr, nullptr, std::move(B));
    // the shape a refill of this batch must keep: the form's own, the first byte and which optional arrays exist
    Batch &made = *ctx->batches[*batch];
    made.refill_shape.n_items = n_items;
    made.refill_shape.t0 = res[BPP_ING_RES_T0] & 255u;
    made.refill_shape.nonces = in->seed_nonces32 != nullptr;
    made.refill_shape.min_values = in->min_values != nullptr;
    made.refill_shape.min_present = in->min_present != nullptr;
    form.record_shape(made);
    return BPP_OK;
  }
  BPP_CATCH(ctx, errbuf, errbuf_len)
}
}  // namespace

extern "C" {

int bpp_batch_upload_mixed(bpp_ctx *ctx, uint64_t params, const bpp_mixed_batch *in, uint64_t *batch, char *errbuf, size_t errbuf_len) {
  BPP_ENTRY(ctx);
  return upload_mixed_impl(ctx, params, in, batch, errbuf, errbuf_len);
}

int bpp_batch_upload_mixed_device(bpp_ctx *ctx, uint64_t params, const bpp_mixed_batch *in, uint64_t *batch, char *errbuf,
                                  size_t errbuf_len) {
  BPP_ENTRY(ctx);
  return upload_device_form<MixedUpload>(ctx, params, in, batch, errbuf, errbuf_len);
}

int bpp_batch_upload_packed_device(bpp_ctx *ctx, uint64_t params, const bpp_packed_batch *in, uint64_t *batch, char *errbuf,
                                   size_t errbuf_len) {
  BPP_ENTRY(ctx);
  return upload_device_form<PackedUpload>(ctx, params, in, batch, errbuf, errbuf_len);
}

int bpp_batch_upload_packed_device_transcripts(bpp_ctx *ctx, uint64_t params, const bpp_packed_batch *in, const uint8_t *item_states203,
                                               uint64_t *batch, char *errbuf, size_t errbuf_len) {
  BPP_ENTRY(ctx);
  return upload_device_form<PackedUpload>(ctx, params, in, batch, errbuf, errbuf_len, true, item_states203);
}

int bpp_batch_upload_mixed_device_transcripts(bpp_ctx *ctx, uint64_t params, const bpp_mixed_batch *in, const uint8_t *item_states203,
                                              uint64_t *batch, char *errbuf, size_t errbuf_len) {
  BPP_ENTRY(ctx);
  return upload_device_form<MixedUpload>(ctx, params, in, batch, errbuf, errbuf_len, true, item_states203);
}

int bpp_device_pointer_check(bpp_ctx *ctx, const void *p, int *kind) {
  BPP_ENTRY(ctx);
  if (!kind) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "null argument");
  *kind = device_pointer_kind(ctx->device, p);
  return BPP_OK;
}

int bpp_ingest_stats(bpp_ctx *ctx, struct bpp_ingest_stats *out) {
  BPP_ENTRY(ctx);
  if (!out) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "null argument");
  *out = ctx->ingest_stats;
  return BPP_OK;
}

int bpp_batch_upload(bpp_ctx *ctx, uint64_t params, const bpp_verify_item *items, size_t n_items, uint64_t *batch,
                     char *errbuf, size_t errbuf_len) {
  BPP_ENTRY(ctx);
  return upload_impl(ctx, params, items, n_items, nullptr, batch, nullptr, nullptr, errbuf, errbuf_len);
}

int bpp_batch_upload_packed(bpp_ctx *ctx, uint64_t params, const bpp_packed_batch *in, uint64_t *batch, char *errbuf,
                            size_t errbuf_len) {
  BPP_ENTRY(ctx);
  if (!in) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "Range statements or proofs length empty", errbuf, errbuf_len);
  return upload_impl(ctx, params, nullptr, 0, in, batch, nullptr, nullptr, errbuf, errbuf_len);
}

int bpp_host_threads(void) { return (int)host_pool_size(); }
uint64_t bpp_host_pool_cpu_ns(void) { return host_pool_cpu_ns(); }

int bpp_shader_clock(bpp_ctx *ctx, uint32_t window_us, double *ghz) {
  BPP_ENTRY(ctx);
  try {
    if (!ghz) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "null argument");
    DevBuf<uint64_t> d;
    d.alloc(2);
    // s_sleep 127 naps for 127 x 64 clocks: ~3.5 us at 2.3 GHz
    const uint32_t naps = std::max<uint32_t>(1, std::min<uint32_t>(window_us, 2000000u) * 2 / 7);
    hipLaunchKernelGGL(k_shader_clock, dim3(1), dim3(64), 0, ctx->stream, d.p, naps);
    uint64_t h[2] = {0, 0};
    gpu_wait_stream(ctx, ctx->stream, true);  // (naps: a sampling thread that spins for the whole window shows up as a busy host core)
    HIP_CHECK(hipMemcpy(h, d.p, 16, hipMemcpyDeviceToHost));
    *ghz = h[1] ? (double)h[0] / (double)h[1] * 0.1 : 0.0;
    return BPP_OK;
  }
  BPP_CATCH(ctx, nullptr, 0)
}

int bpp_batch_destroy(bpp_ctx *ctx, uint64_t batch) {
  BPP_ENTRY(ctx);
  (void)hipStreamSynchronize(ctx->stream);
  auto it = ctx->batches.find(batch);
  if (it == ctx->batches.end()) return BPP_ERR_BAD_HANDLE;
  wipe_batch_secrets(*it->second, ctx->stream);  // seed nonces, recovered masks: gone before the buffers change hands
  (void)hipStreamSynchronize(ctx->stream);
  ctx->spare_batch = std::move(it->second);  // nothing of it is in flight any more; its allocations serve the next upload
  ctx->batches.erase(it);
  return BPP_OK;
}

}  // extern "C"

namespace {

// Weight-independent device work for the whole resident batch: PASS 1, decompression and -- unless `pass1_only` --
// the per-proof scalar block (k_scalars_shared).  Returns after the transcript-RNG bytes have reached the host (h_rng); the rest is
// still running on the stream (it overlaps the host weight chain).
// rng_dev_dst != nullptr (the sharded form): the transcript-RNG bytes are copied device -> device right behind PASS 1 and
// ev_rng is recorded there; nothing comes to the host and the function does not wait
void plan_lanes(bpp_ctx *ctx, Batch &b, bool for_phase2 = false);

// ev_rng marks the transcript-RNG bytes of a context's PASS 1; made when a context first needs it
void ensure_ev_rng(bpp_ctx *ctx) {
  if (ctx->ev_rng_ready) return;
  HIP_CHECK(hipEventCreateWithFlags(&ctx->ev_rng, hipEventDisableTiming));
  ctx->ev_rng_ready = true;
}

// Where a call's weight chains run (option "chain" / BPP_CHAIN: 0 host, 1 device, -1 this rule).  The host runs a chain five
// to eight times faster than a wavefront does (chain_host.h: 0.27 us per proof, chain_dev.h: ~2), so a call that WAITS for its
// chains -- one call at a time, few groups -- keeps them on the host.  The device form is for callers that keep several
// calls in flight and want the host left alone (a rank of an 8-GPU node: bench.py): it is chosen explicitly.
enum ChainMode { CHAIN_HOST = 0, CHAIN_DEVICE = 1, CHAIN_HOST_WIDE = 2 };
// CHAIN_HOST_WIDE: the sponges on host cores, Scalar::from_bytes_mod_order_wide (half of a lock-step bundle's CPU time, and
// perfectly parallel) on the device: the default for calls of BPP_WAIT_NAP_MIN_PROOFS proofs and more -- their callers keep
// several calls in flight, and there a host core counts for more than the extra launch.
ChainMode chain_mode(const bpp_ctx *ctx, const Batch &b, bool allow_device_work) {
  if (!allow_device_work) return CHAIN_HOST;  // the second run after a zero weight: everything as the reference does it
  if (ctx->opt.chain >= 0 && ctx->opt.chain <= 2) return (ChainMode)ctx->opt.chain;
  return b.B >= BPP_WAIT_NAP_MIN_PROOFS ? CHAIN_HOST_WIDE : CHAIN_HOST;
}
// the wide bytes of the host sponges (b.h_wide, mapped) -> b.weights.  launch = false: k_scalars_lanes does it in its prologue
// (enqueue_phase2), this only arms the zero flag
void enqueue_finish_wide(bpp_ctx *ctx, Batch &b, hipStream_t st, bool launch = true) {
  if (!ctx->h_chain_zero.p) ctx->h_chain_zero.resize(1);
  ctx->h_chain_zero[0] = 0;
  const uint32_t test_zero = ctx->opt.chain_test_zero > 0 ? (uint32_t)ctx->opt.chain_test_zero : 0u;
  if (launch)
    hipLaunchKernelGGL(k_chain_finish_bytes, dim3(cdiv(b.B, 64)), dim3(64), 0, st, b.h_wide.dev(), b.B, b.weights.p, ctx->h_chain_zero.dev(), test_zero);
  ctx->wide_chain_calls++;
}

// k_weight_chain + k_chain_finish on `st`: b.rng_out -> b.weights (canonical bytes), one wavefront per group
// zero_word != nullptr (bpp_verify_enqueue): the call's zero-weight finding goes to that device word, which belongs to the enqueue;
// the context's host-visible word is neither reset nor written (another call may be in flight behind it)
void enqueue_device_chain(bpp_ctx *ctx, Batch &b, hipStream_t st, uint32_t *zero_word = nullptr) {
  if (!ctx->d_chain_t0.p) {  // once per context: the weight transcript as Transcript::new leaves it (src/range_proof.rs:811)
    Strobe t0;
    const char *lbl = "Bulletproofs+ verifier weights";
    merlin_new(t0, (const uint8_t *)lbl, (uint32_t)strlen(lbl));
    ctx->d_chain_t0.alloc(1);
    HIP_CHECK(hipMemcpy(ctx->d_chain_t0.p, &t0, sizeof(t0), hipMemcpyHostToDevice));
    ctx->h_chain_zero.resize(1);
  }
  b.chain_wide.alloc((size_t)b.B * 16);
  if (!zero_word) ctx->h_chain_zero[0] = 0;
  const uint32_t test_zero = ctx->opt.chain_test_zero > 0 ? (uint32_t)ctx->opt.chain_test_zero : 0u;
  // (the view is non-null only for a batch refilled with a count or under a mask, which takes enqueued calls alone)
  const LiveView lv = b.live_view();
  uint32_t *zero_dst = zero_word ? zero_word : ctx->h_chain_zero.dev();
  if (lv.mask) {
    hipLaunchKernelGGL(k_weight_chain<true>, dim3(b.G), dim3(64), 0, st, b.rng_out.p, b.group_first.p, b.G, ctx->d_chain_t0.p, b.chain_wide.p, lv);
    hipLaunchKernelGGL(k_chain_finish<true>, dim3(cdiv(b.B, 64)), dim3(64), 0, st, b.chain_wide.p, b.B, b.weights.p, zero_dst, test_zero, lv);
  } else {
    hipLaunchKernelGGL(k_weight_chain<false>, dim3(b.G), dim3(64), 0, st, b.rng_out.p, b.group_first.p, b.G, ctx->d_chain_t0.p, b.chain_wide.p, lv);
    hipLaunchKernelGGL(k_chain_finish<false>, dim3(cdiv(b.B, 64)), dim3(64), 0, st, b.chain_wide.p, b.B, b.weights.p, zero_dst, test_zero, lv);
  }
  ctx->device_chain_calls++;
}

// dev_chain: the weight chains follow PASS 1 as kernels (option "chain_inline" = 0: on a stream of their own beside the decompression
// and the weight-free scalars, joined by enqueue_phase2): nothing comes to the host and the function does not wait
void enqueue_phase1(bpp_ctx *ctx, Batch &b, StageTimer &tm, bool pass1_only, uint8_t *rng_dev_dst = nullptr, size_t rng_row_bytes = 0,
                    size_t rng_dst_pitch = 0, bool dev_chain = false, uint32_t *chain_zero_word = nullptr) {
  // chain_zero_word != nullptr (bpp_verify_enqueue): the device chain, where the call runs one, runs in line on the call's stream
  // whatever "chain_inline" says and reports a zero weight there (enqueue_device_chain); nothing comes to the host and the function
  // does not wait, with or without a chain
  const bool fetch_rng = rng_dev_dst == nullptr && !dev_chain && !chain_zero_word;
  b.dev_chain_pending = false;
  b.enq_weights = false;  // (verify_enqueue_locked sets it behind its own call)
  Params &P = *b.params;
  hipStream_t s = ctx->stream;
  if (!pass1_only) plan_lanes(ctx, b);  // (an option may have changed since the layout was built: k_scalars_shared writes what PASS 2 will read)
  ensure_ev_rng(ctx);
  // status[] starts as status0[]: the previous verification's last kernel left it so (k_results_out), unless that call died
  // half way
  if (!b.status_clean) HIP_CHECK(hipMemcpyAsync(b.status.p, b.status0.p, (size_t)b.B * 4, hipMemcpyDeviceToDevice, s));
  b.status_clean = false;
  // Decompression needs nothing PASS 1 produces (both only OR bits into status[]).  A small input leaves most of the chip
  // idle, so its decompression runs beside PASS 1 and the weight-free scalars on a second stream and joins before the
  // weights are needed (one 256-proof call 0.84 -> 0.79 ms).  Large inputs fill the chip either way: one stream, less
  // bookkeeping (measured: no gain, HISTORY.md 3).  Stage profiling keeps the serial order so that its intervals mean something.
  const bool side = (ctx->opt.side_decompress >= 0 ? ctx->opt.side_decompress != 0 : b.B <= BPP_SIDE_DECOMPRESS_MAX) && !(ctx->profile && !ctx->profile_light);
  const uint32_t n_proof_pts = b.total_dyn - b.sum_m;
  auto launch_decompress = [&](hipStream_t st) {
    hipLaunchKernelGGL(k_decompress, dim3(cdiv(n_proof_pts, 64)), dim3(64), 0, st, b.bytes.p, b.src_off.p, b.owner.p,
                       b.idx_proof.p, n_proof_pts, b.dynpts.p, b.status.p, b.dec_spill.p, (uint32_t *)nullptr);
    // half-scalar plan of small calls: the 2^126 multiples of every dynamic point (the statements' commitments were decoded
    // at upload), 126 doublings each, right behind the decompression and -- for small inputs -- beside PASS 1 and the scalars.
    // A point that did not decode left an arbitrary entry: its multiple is never looked at (the call fails on the status).
    if (b.need_dyn_hi && !pass1_only)  // (the per-group plan's, or the joint check's: layout_joint)
      hipLaunchKernelGGL(k_split_shift_quad, dim3(cdiv(b.total_dyn, 16)), dim3(64), 0, st, b.dynpts.p, b.total_dyn, b.dyn_hi.p);
  };
  if (side) {
    if (!ctx->side_stream) {
      HIP_CHECK(hipStreamCreateWithFlags(&ctx->side_stream, hipStreamNonBlocking));
      HIP_CHECK(hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
      HIP_CHECK(hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming));
    }
    HIP_CHECK(hipEventRecord(ctx->ev_fork, s));
    HIP_CHECK(hipStreamWaitEvent(ctx->side_stream, ctx->ev_fork, 0));
    launch_decompress(ctx->side_stream);
    HIP_CHECK(hipEventRecord(ctx->ev_join, ctx->side_stream));
  }
  if (b.ext_challenges) {  // caller did PASS 1: challenges + rng bytes are already resident
    tm.mark(M_START);
  } else {
    if (!b.uniform_rounds) HIP_CHECK(hipMemsetAsync(b.chal.p, 0, (size_t)b.B * b.cs * sizeof(sc), s));  // trace padding only
    tm.mark(M_START);
    // small inputs: one proof per wavefront (latency); large inputs: one proof per lane (issue slots)
    const int force_wave = ctx->opt.transcripts_wave;  // (tests force either kernel)
    const bool wave = force_wave >= 0 ? force_wave != 0 : b.B <= BPP_TRANSCRIPTS_WAVE_MAX;
    uint8_t *rng_host = fetch_rng ? b.h_rng.dev() : nullptr;  // mapped page-locked memory: no device-to-host copy behind PASS 1
    if (b.want_states || b.state_rows_dst) {  // the kernels' other instantiation: every proof's advanced transcript into b.h_states as well
      uint32_t *rows_dst = b.state_rows_dst;  // (bpp_verify_enqueue_states: device memory of the batch, nothing for the host)
      if (!rows_dst) {
        b.h_states.resize((size_t)b.B * BPP_STATE_ROW_WORDS);
        rows_dst = b.h_states.dev();
      }
      if (wave)
        hipLaunchKernelGGL(k_transcripts_wave<true>, dim3(b.B), dim3(64), 0, s, b.bytes.p, b.d_desc.p, b.minvals.p, b.states.p,
                           P.d_hg32.p, P.n_bits, P.t, b.B, b.cs, b.chal.p, b.rng_out.p, b.status.p, rng_host, rows_dst);
      else
        hipLaunchKernelGGL(k_transcripts<true>, dim3(cdiv(b.B, 64)), dim3(64), 0, s, b.bytes.p, b.d_desc.p, b.minvals.p, b.states.p,
                           P.d_hg32.p, P.n_bits, P.t, b.B, b.cs, b.chal.p, b.rng_out.p, b.status.p, rng_host, rows_dst);
    } else if (wave)
      hipLaunchKernelGGL(k_transcripts_wave<false>, dim3(b.B), dim3(64), 0, s, b.bytes.p, b.d_desc.p, b.minvals.p, b.states.p,
                         P.d_hg32.p, P.n_bits, P.t, b.B, b.cs, b.chal.p, b.rng_out.p, b.status.p, rng_host, (uint32_t *)nullptr);
    else
      hipLaunchKernelGGL(k_transcripts<false>, dim3(cdiv(b.B, 64)), dim3(64), 0, s, b.bytes.p, b.d_desc.p, b.minvals.p, b.states.p,
                         P.d_hg32.p, P.n_bits, P.t, b.B, b.cs, b.chal.p, b.rng_out.p, b.status.p, rng_host, (uint32_t *)nullptr);
  }
  tm.mark(M_TRANSCRIPTS);
  if (dev_chain) {
    // On the call's own stream (the rule): measured against a high-priority stream of their own beside the decompression -- the same
    // rate once one more step is in flight, and the cross-stream events of that form leave a helper thread of the runtime at 80 %
    // of a core (profiles/r06_chain_inline_ab.txt); "chain_inline" = 0 brings the side stream back
    if (ctx->profile || ctx->opt.chain_inline != 0 || chain_zero_word) {
      enqueue_device_chain(ctx, b, s, chain_zero_word);
      tm.mark(M_CHAIN);
    } else {
      if (!ctx->chain_stream) {
        int least = 0, greatest = 0;  // the chains are 64 lone wavefronts on the call's critical path: first in line for a slot
        HIP_CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIP_CHECK(hipStreamCreateWithPriority(&ctx->chain_stream, hipStreamNonBlocking, greatest));
        HIP_CHECK(hipEventCreateWithFlags(&ctx->ev_chain_fork, hipEventDisableTiming));
        HIP_CHECK(hipEventCreateWithFlags(&ctx->ev_chain_done, hipEventDisableTiming));
      }
      HIP_CHECK(hipEventRecord(ctx->ev_chain_fork, s));
      HIP_CHECK(hipStreamWaitEvent(ctx->chain_stream, ctx->ev_chain_fork, 0));
      enqueue_device_chain(ctx, b, ctx->chain_stream);
      HIP_CHECK(hipEventRecord(ctx->ev_chain_done, ctx->chain_stream));
      b.dev_chain_pending = true;
    }
  }
  if (fetch_rng || !rng_dev_dst) {
    // (nothing to copy: PASS 1 wrote the bytes the weight chain reads into h_rng itself -- or the chain runs on the device; the
    // event below tells the host)
  } else if (rng_dst_pitch && rng_dst_pitch != rng_row_bytes)  // rows of one group each, padded to the widest rank's shard
    HIP_CHECK(hipMemcpy2DAsync(rng_dev_dst, rng_dst_pitch, b.rng_out.p, rng_row_bytes, rng_row_bytes, ((size_t)b.B * 32) / rng_row_bytes,
                               hipMemcpyDeviceToDevice, s));
  else HIP_CHECK(hipMemcpyAsync(rng_dev_dst, b.rng_out.p, (size_t)b.B * 32, hipMemcpyDeviceToDevice, s));  // gathered over RCCL
  HIP_CHECK(hipEventRecord(ctx->ev_rng, s));
  if (!side) launch_decompress(s);
  tm.mark(M_DECOMPRESS);
  if (!pass1_only) {  // the weight-independent part of the PASS-2 scalars; the rest (k_scalars_lanes) takes the weights
    // tables of the generator-row kernel: by the same lane for large inputs, one wavefront per proof for small ones
    const bool tw = ctx->opt.tables_wave >= 0 ? ctx->opt.tables_wave != 0 : b.B <= BPP_TABLES_WAVE_MAX;  // (tests force either form)
    b.gemm_hi_ready = b.static_gemm && !tw;
    if (b.gemm_hi_ready)  // the high tables once more as digit tables (kernels_static_gemm.h)
      hipLaunchKernelGGL(k_scalars_shared<true>, dim3(cdiv(b.B, 64)), dim3(64), 0, s, b.bytes.p, b.d_desc.p, b.minvals.p, b.chal.p, P.n_bits,
                         P.t, b.cs, b.B, b.shr.p, b.lanes_nhi_max(P.n_bits), b.tab.p, b.gemm_hi.p, cdiv(b.B, SGEMM_BLOCK));
    else
      hipLaunchKernelGGL(k_scalars_shared<false>, dim3(cdiv(b.B, 64)), dim3(64), 0, s, b.bytes.p, b.d_desc.p, b.minvals.p, b.chal.p, P.n_bits,
                         P.t, b.cs, b.B, b.shr.p, b.lanes_nhi_max(P.n_bits), tw ? (sc *)nullptr : b.tab.p, (int8_t *)nullptr, 0u);
    if (tw)
      hipLaunchKernelGGL(k_scalars_tables_wave, dim3(b.B), dim3(64), 0, s, b.d_desc.p, b.shr.p, P.n_bits, b.B,
                         b.lanes_nhi_max(P.n_bits), b.tab.p);
    tm.mark(M_SCALARS);
  }
  if (side) HIP_CHECK(hipStreamWaitEvent(s, ctx->ev_join, 0));
  HIP_CHECK(hipGetLastError());
  if (fetch_rng) gpu_wait_event(ctx->ev_rng, wait_naps(ctx, b.B), &ctx->wait_hint_rng, ((uint64_t)b.B << 32) | b.G);
}

// Weight chains of all groups (src/range_proof.rs:811,849,853,894).  Chunks are independent reference batches: groups of
// equal size run W at a time in lockstep on vector Keccak (chain_host.h), bundles are spread over host threads.
void run_weight_chains(Batch &b) { run_weight_chains_generic(b.h_rng.data(), b.h_weights.data(), b.h_group_first.data(), b.G); }
// the sponges alone: 64 PRF bytes per proof into b.h_wide, reduced (and looked at for zeros) by k_chain_finish_bytes
void run_weight_chains_wide(Batch &b) {
  b.h_wide.resize((size_t)b.B * 64);
  run_weight_chains_generic(b.h_rng.data(), b.h_wide.data(), b.h_group_first.data(), b.G, true);
}

// status words (and, where asked for, the groups' identity flags and the recovered masks) -> mapped host memory, status[]
// back to its initial value: one launch, no copy (kernels_verify.h: k_results_out).  Valid on the host once the stream has
// been synchronised.
// joint: the one identity flag of the joint final check instead of the groups' (it lands in h_ident[0])
void fetch_results(bpp_ctx *ctx, Batch &b, bool ident, bool masks, bool joint = false) {
  if (ident) b.h_ident.resize(b.G);
  const uint32_t *ident_src = joint ? b.msm_joint.is_identity.p : b.msm.is_identity.p;
  const uint32_t n_ident = joint ? 1u : b.G;
  const uint32_t pieces = masks ? (uint32_t)(((size_t)b.B * b.params->t * 32) / 16) : 0u;
  if (masks) b.h_masks.resize((size_t)pieces * 16);
  const uint32_t items = std::max(b.B, ident ? b.G : 0u);
  b.h_status_any.resize(cdiv(b.B, BPP_STATUS_BLOCK));
  b.status_settled = false;
  hipLaunchKernelGGL(k_results_out, dim3(cdiv(items, BPP_STATUS_BLOCK)), dim3(BPP_STATUS_BLOCK), 0, ctx->stream, b.status.p, b.status0.p,
                     b.h_status.dev(), b.h_status_any.dev(), b.B,
                     ident ? ident_src : (const uint32_t *)nullptr, ident ? b.h_ident.dev() : (uint32_t *)nullptr, n_ident,
                     masks ? (const uint4 *)b.masks.p : (const uint4 *)nullptr, masks ? (uint4 *)b.h_masks.dev() : (uint4 *)nullptr, pieces);
  HIP_CHECK(hipGetLastError());
  b.status_clean = true;  // (in stream order: whatever is enqueued behind this launch finds status0)
}
void fetch_status(bpp_ctx *ctx, Batch &b) { fetch_results(ctx, b, false, false); }
// After the stream has been synchronised behind fetch_results: h_status as every reader expects it.  The kernel wrote the words
// of the blocks that hold a finding; every other block is zero by its summary word and is cleared here only if an earlier
// verification left something in it -- on the accept path this touches one word per 256 proofs.
void settle_status(Batch &b) {
  if (b.status_settled) return;
  const uint32_t n_blk = cdiv(b.B, BPP_STATUS_BLOCK);
  if (b.h_status_dirty.size() != n_blk || b.h_status_dirty_of != b.h_status.data()) {  // fresh page-locked memory: contents unknown
    b.h_status_dirty.assign(n_blk, 1);
    b.h_status_dirty_of = b.h_status.data();
  }
  for (uint32_t k = 0; k < n_blk; k++) {
    if (b.h_status_any[k]) {
      b.h_status_dirty[k] = 1;
    } else if (b.h_status_dirty[k]) {
      // the WHOLE block of the allocation, not just this batch's proofs: the flags travel with the buffer to batches of other sizes
      const size_t lo = (size_t)k * BPP_STATUS_BLOCK, hi = std::min<size_t>(b.h_status.n, lo + BPP_STATUS_BLOCK);
      memset(b.h_status.data() + lo, 0, (hi - lo) * 4);
      b.h_status_dirty[k] = 0;
    }
  }
  b.status_settled = true;
}

// reference error precedence for proofs [p0, p1) treated as one verify() call (upload_host.h: check_chunk_errors)
void check_chunk_errors(Batch &b, uint32_t p0, uint32_t p1) {
  settle_status(b);
  bpp::check_chunk_errors(b.h_status.data(), b.rounds_bad.data(), p0, p1);
}

// Shape of k_scalars_lanes for the current group layout, and the buffers that go with it (called when a layout is built and
// again in front of every PASS 2: the option may have changed; nothing is reallocated once the sizes have been seen).
void plan_lanes(bpp_ctx *ctx, Batch &b, bool for_phase2) {
  // proofs per workgroup: enough (proof, generator pair) items for four passes of the 64 lanes.  Large inputs take sixteen
  // 64-bit proofs per workgroup (the prologue's product jobs, 43 per proof, then fill whole wavefronts); small inputs keep four
  // (more workgroups, shorter chains: the chip is idle anyway).
  const uint32_t per_wg = b.B <= BPP_TABLES_WAVE_MAX ? 256u : 1024u;
  b.lanes_ppw = std::max<uint32_t>(1, std::min<uint32_t>(BPP_LANES_MAX_PPW, per_wg / std::max<uint32_t>(1, b.max_mn)));
  // Generator columns summed inside k_scalars_lanes (no per-proof rows at all) when a lane can own a generator index across the
  // workgroup's proofs (max_mn a multiple of 64) and no workgroup straddles a group boundary
  bool aligned = b.max_mn >= 64 && b.max_mn % 64 == 0;
  for (uint32_t g = 1; g < b.G && aligned; g++) aligned = b.h_group_first[g] % b.lanes_ppw == 0;
  b.fused_columns = aligned && ctx->opt.fused_columns != 0;  // (tests force the per-proof rows with fused_columns = 0)
  // The generator columns as a matrix product over the proofs of each group on the matrix cores (kernels_static_gemm.h) when
  // every proof has the same shape, the tables are built by k_scalars_shared (large inputs) and every group starts on a block
  // of the digit tables; otherwise summed in k_scalars_lanes as before (tests run both: static_gemm = 0)
  if (b.uniform_mn < 0) {
    uint32_t mn0 = b.B ? b.desc[0].m * b.params->n_bits : 0;
    for (uint32_t p = 1; p < b.B && mn0; p++)
      if (b.desc[p].m * b.params->n_bits != mn0 || b.desc[p].rounds != b.desc[0].rounds) mn0 = 0;
    if (mn0 && (b.any_rounds_bad || (1u << b.desc[0].rounds) != mn0)) mn0 = 0;
    b.uniform_mn = (int)mn0;
  }
  const bool tables_wave = ctx->opt.tables_wave >= 0 ? ctx->opt.tables_wave != 0 : b.B <= BPP_TABLES_WAVE_MAX;
  const uint32_t lb = lanes_lb(b.params->n_bits);
  // (by itself from aggregation 8 on: measured with three steps in flight, 64 x 256 proofs per step, the matrix product gains 10 %
  // at m = 8, nothing at m = 2 and loses 3 - 5 % at m = 1 and 4 -- tools/agg_probe.py, profiles/r04_agg_probe.jsonl)
  const bool gemm_wanted = ctx->opt.static_gemm >= 0 ? ctx->opt.static_gemm != 0 : b.uniform_mn >= 512;
  bool gemm = b.fused_columns && gemm_wanted && !tables_wave && b.uniform_mn >= 64 && lb == 3 &&
              ((uint32_t)b.uniform_mn >> lb) >= SGEMM_HI_PER_WAVE && ((uint32_t)b.uniform_mn >> lb) <= b.lanes_nhi_max(b.params->n_bits);
  uint32_t max_group = 0;
  for (uint32_t g = 0; g < b.G && gemm; g++) {
    gemm = b.h_group_first[g] % SGEMM_BLOCK == 0;
    max_group = std::max(max_group, b.h_group_first[g + 1] - b.h_group_first[g]);
  }
  if (for_phase2 && !b.gemm_hi_ready) gemm = false;  // (PASS 1 of this verification ran under another setting)
  b.static_gemm = gemm;
  if (b.static_gemm) {
    b.gemm_mult.alloc((size_t)b.B * 5);
    const uint32_t nblk = cdiv(b.B, SGEMM_BLOCK);
    b.gemm_nkc = std::max<uint32_t>(1, cdiv(cdiv(max_group, SGEMM_BLOCK), SGEMM_KBLOCKS));
    b.rows.alloc((size_t)b.B * (b.params->t + 2));
    b.gemm_lo.alloc(3 * sgemm_table_bytes(SGEMM_LO_ENTRIES, nblk));
    b.gemm_hi.alloc(3 * sgemm_table_bytes(b.lanes_nhi_max(b.params->n_bits), nblk));
    b.gparts.alloc((size_t)b.G * b.gemm_nkc * b.max_mn * 2 * 64);
  } else if (b.fused_columns) {
    b.rows.alloc((size_t)b.B * (b.params->t + 1));
    b.parts.alloc((size_t)cdiv(b.B, b.lanes_ppw) * 2 * b.max_mn * 8);
  } else {
    b.rows.alloc((size_t)b.B * b.cols);
  }
}

// (re)build the group layout + MSM term lists for `chunk`
// `bounds` (optional): explicit group boundaries first[0..G] (0 = first[0] < ... < first[G] = B) instead of equal chunks --
// the reference batches of different callers pooled into one call (bpp_verify_resident_groups)
// "verify_joint" = 1 and a layout of two or more groups: plan, buffers and term lists of the joint check (one group: the `cols`
// generator columns under the joint row, then every dynamic slot), by the rules any group of its size gets -- half-scalar split for
// small calls included, whether or not the per-group plan is split.  Nothing happens with the option off.
// The rule (measured, DESIGN.md 4.1 "Joint final check"): the joint form is taken while the joint group has at most
// BPP_JOINT_MAX_TERMS terms -- pooled small calls, where it is level or ahead (8 x 2 proofs: 0.170 against 0.169 ms per call, 16 x 16:
// 0.23 against 0.26).  Above, it loses on every shape measured (16 x 256: + 15 %, 4 x 1024 at m = 8: + 14 %, 64 x 1024: + 104 %):
// k_msm_accumulate gives a group to ONE XCD, so a single group of any size runs its additions on an eighth of the chip.  "verify_joint"
// = 2 takes the joint form whatever the size (measurement: tools/bench_verify_joint.py).
#define BPP_JOINT_MAX_TERMS 14000u
bool joint_wanted(const bpp_ctx *ctx, const Batch &b) {
  if (b.G < 2) return false;
  return ctx->opt.verify_joint == 2 || (ctx->opt.verify_joint == 1 && b.cols + b.total_dyn <= BPP_JOINT_MAX_TERMS);
}
void layout_joint(bpp_ctx *ctx, Batch &b) {
  b.need_dyn_hi = b.msm.split;
  if (!joint_wanted(ctx, b)) return;
  if (b.joint_G == b.G) {  // (the plan is there: what the pass needs is said again, a pass without the joint check may lie between)
    b.need_dyn_hi = b.msm.split || b.msm_joint.split;
    return;
  }
  // (an earlier pass's joint point outlives a new plan: msm_joint.R is one point whatever the plan, and buffers only ever grow)
  Params &P = *b.params;
  const uint32_t ng = b.cols + b.total_dyn;
  const bool split = msm_wants_split(ctx, ng);
  b.scal.alloc((size_t)b.G * b.cols + b.total_dyn + b.cols);  // the joint row behind the dynamic scalars
  if (split) b.dyn_hi.alloc(b.total_dyn);
  b.need_dyn_hi = b.msm.split || split;
  msm_plan_alloc(ctx, b.msm_joint, std::vector<uint32_t>{0u, split ? 2 * ng : ng}, split, false);
  hipLaunchKernelGGL(k_layout_terms_joint, dim3(cdiv(ng, 256)), dim3(256), 0, ctx->stream, b.G, b.cols, b.total_dyn, b.max_mn,
                     2 * P.n_bits * P.m_max, P.table_len, split ? 1u : 0u, b.msm_joint.term_sidx.p, b.msm_joint.term_pidx.p, b.msm_joint.group_off.p);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(ctx->stream));
  b.joint_G = b.G;
}

// `joint`: the caller's pass may take the joint final check (verify_flow_once, bpp_batch_prepare); every other caller -- the sharded
// and the phased forms, a recheck's plain pass -- gets the per-group plan alone, with no launch and no buffer of the joint one
void layout_groups(bpp_ctx *ctx, Batch &b, size_t chunk, const std::vector<uint32_t> *bounds = nullptr, bool joint = false) {
  if (!bounds && chunk == (size_t)-1) chunk = 0;  // ((size_t)-1 marks an explicit layout in last_chunk)
  auto tail = [&] {
    if (joint) layout_joint(ctx, b);
    else b.need_dyn_hi = b.msm.split;
  };
  if (bounds) {
    if (b.last_chunk == (size_t)-1 && b.G && b.h_group_first == *bounds) return tail();
  } else if (b.last_chunk == chunk && b.G) {
    return tail();
  }
  b.joint_G = 0;
  Params &P = *b.params;
  uint32_t G;
  if (bounds) {
    G = (uint32_t)bounds->size() - 1;
    b.h_group_first = *bounds;
  } else {
    const uint32_t cz = (chunk == 0 || chunk >= b.B) ? b.B : (uint32_t)chunk;
    G = cdiv(b.B, cz);
    b.h_group_first.resize(G + 1);
    for (uint32_t g = 0; g <= G; g++) b.h_group_first[g] = std::min(g * cz, b.B);
  }
  b.G = G;
  b.group_first.alloc(G + 1);
  b.scal.alloc((size_t)G * b.cols + b.total_dyn);
  plan_lanes(ctx, b);
  // terms of group g: static columns (first 2*max_mn generators, then g bases, then h) + its proofs' dynamic slots.
  // Only the G + 1 offsets come from the host; the ~1 M term entries are written by k_layout_terms (building them on the
  // host and copying two pageable vectors cost ~20 ms per freshly uploaded batch)
  const uint32_t n_gen = 2 * P.n_bits * P.m_max;
  std::vector<uint32_t> goff(G + 1), dlo(G + 1);
  uint32_t run = 0, maxg = 0;
  for (uint32_t g = 0; g < G; g++) {
    goff[g] = run;
    const uint32_t p0 = b.h_group_first[g], p1 = b.h_group_first[g + 1];
    const uint32_t d0 = b.desc[p0].dyn_off, d1 = (p1 < b.B) ? b.desc[p1].dyn_off : b.total_dyn;
    dlo[g] = d0;
    run += b.cols + (d1 - d0);
    maxg = std::max(maxg, b.cols + (d1 - d0));
  }
  goff[G] = run;
  dlo[G] = b.total_dyn;
  const bool split = msm_wants_split(ctx, run);
  if (split) {  // every term twice: (low half, P), (high half, 2^126 P)
    for (uint32_t g = 0; g <= G; g++) goff[g] *= 2;
    maxg *= 2;
    b.dyn_hi.alloc(b.total_dyn);
  }
  msm_plan_alloc(ctx, b.msm, goff, split, false);  // leaves goff in pin_small[0 .. G]
  b.group_dlo.alloc(G + 1);
  uint32_t *pin = ctx->pin_small.data();
  memcpy(pin + (G + 1), b.h_group_first.data(), (G + 1) * 4);
  memcpy(pin + 2 * (size_t)(G + 1), dlo.data(), (G + 1) * 4);
  // the three small arrays are read by k_layout_terms where they are (mapped host memory); it also leaves the device copies
  const uint32_t *pin_dev = ctx->pin_small.dev();
  hipLaunchKernelGGL(k_layout_terms, dim3(cdiv(split ? maxg / 2 : maxg, 256), G), dim3(256), 0, ctx->stream, pin_dev, pin_dev + 2 * (size_t)(G + 1),
                     pin_dev + (G + 1), G, b.cols, b.max_mn, n_gen, P.table_len, split ? 1u : 0u, b.msm.term_sidx.p, b.msm.term_pidx.p,
                     b.msm.group_off.p, b.group_dlo.p, b.group_first.p);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(ctx->stream));  // pin_small is reused by the next plan
  b.last_chunk = bounds ? (size_t)-1 : chunk;
  tail();
}

// Weight-dependent tail: h_weights -> device, the weighted generator rows and dynamic scalars (k_scalars_lanes), the
// per-group column sums, final MSM.
// wide: chain = 2, the host sponges' 64 bytes per proof stand in b.h_wide (mapped).  When k_scalars_lanes is the kernel that takes
// the weights it reads and reduces them itself and leaves the canonical weights in b.weights (option "wide_in_lanes", on by
// rule: one launch fewer on the step's latency chain -- between two synchronisations the steps in flight run in step and every
// launch of the chain counts: the driver's 20-step form + 1-2 %, profiles/r06_wait_ahead_ab.txt); the matrix-product form of the
// generator columns keeps k_chain_finish_bytes in front
// plain_groups (pass 2 of "verify_check"): the final MSM of those groups alone, through the plain kernels (msm_plain.h); the layout is
// then an unsplit one
// joint ("verify_joint"): the joint row and ONE MSM over all groups (b.msm_joint) instead of the per-group MSMs
void enqueue_phase2(bpp_ctx *ctx, Batch &b, StageTimer &tm, bool weights_resident = false, bool wide = false,
                    const std::vector<uint32_t> *plain_groups = nullptr, bool joint = false) {
  Params &P = *b.params;
  hipStream_t s = ctx->stream;
  // (weights_resident: the grouped sharded form has put them into b.weights device -> device already)
  // otherwise k_scalars_lanes reads them where the chains wrote them: h_weights is mapped, each weight is read once
  plan_lanes(ctx, b, true);
  const bool wide_in_lanes = wide && !b.static_gemm && ctx->opt.wide_in_lanes != 0;
  if (wide) enqueue_finish_wide(ctx, b, s, !wide_in_lanes);
  if (b.dev_chain_pending) {  // the device chain of this call (enqueue_phase1) has written b.weights
    HIP_CHECK(hipStreamWaitEvent(s, ctx->ev_chain_done, 0));
    b.dev_chain_pending = false;
  }
  b.weights_on_host = !weights_resident;
  const uint8_t *weights = weights_resident ? b.weights.p : b.h_weights.dev();
  tm.mark(M_WEIGHTS_IN);
  sc *dyn_scal = b.scal.p + (size_t)b.G * b.cols;
  {
    const uint32_t nhi_max = b.lanes_nhi_max(P.n_bits);
    // The weighted part of the scalar block (dynamic scalars, base columns, w into the low tables) is this kernel's prologue;
    // proofs per workgroup and whether the generator columns are summed in it: layout_groups
    const uint32_t ppw = b.lanes_ppw;
    if (b.static_gemm) {  // the weighted part alone, flat over (proof, job): digit tables of the low entries, dynamic scalars, base columns
      const uint32_t rounds = b.desc[0].rounds, m0 = b.desc[0].m;
      const uint32_t n_jobs = 3u * (1u << lanes_lb(P.n_bits)) + 1u + m0 + 3u + 2u * rounds + P.t + 1u, nblk = cdiv(b.B, SGEMM_BLOCK);
      hipLaunchKernelGGL(k_gemm_mult, dim3(cdiv(4 * b.B, 64)), dim3(64), 0, s, b.shr.p, weights, b.B, b.gemm_mult.p);
      hipLaunchKernelGGL(k_gemm_jobs, dim3(nblk, cdiv(n_jobs, 4)), dim3(64), 0, s, b.d_desc.p, b.tab.p, b.shr.p, b.gemm_mult.p, P.n_bits, P.t,
                         b.B, nhi_max, n_jobs, b.rows.p, dyn_scal, b.gemm_lo.p, nblk);
    } else
      hipLaunchKernelGGL(k_scalars_lanes, dim3(cdiv(b.B, ppw)), dim3(64), ppw * lanes_lds_bytes(nhi_max), s, b.d_desc.p, b.tab.p, b.shr.p,
                         weights, P.n_bits, P.t, b.max_mn, b.cols, b.B, nhi_max, ppw, b.rows.p, dyn_scal,
                         b.fused_columns ? b.parts.p : (uint64_t *)nullptr, ctx->opt.lazy_columns != 0 ? 1u : 0u,
                         wide_in_lanes ? b.h_wide.dev() : (const uint8_t *)nullptr, b.weights.p, ctx->h_chain_zero.dev(),
                         ctx->opt.chain_test_zero > 0 ? (uint32_t)ctx->opt.chain_test_zero : 0u);
  }
  tm.mark(M_LANES);
  if (b.static_gemm) {
    const uint32_t lb = lanes_lb(P.n_bits), nhi = (uint32_t)b.uniform_mn >> lb, nblk = cdiv(b.B, SGEMM_BLOCK);
    const uint32_t nhi_max = b.lanes_nhi_max(P.n_bits);
    hipLaunchKernelGGL(k_static_gemm, dim3(8 * cdiv(b.G, 8) * SGEMM_LO_ENTRIES * (nhi / SGEMM_HI_PER_WAVE), b.gemm_nkc), dim3(64), 0, s, b.gemm_lo.p,
                       b.gemm_hi.p, b.group_first.p, nblk, nhi, nhi_max, b.gemm_nkc, b.max_mn, b.G, b.gparts.p);
    hipLaunchKernelGGL(k_static_finish, dim3(cdiv(2 * b.max_mn, 64) + 1, b.G), dim3(64), 0, s, b.gparts.p, b.rows.p, b.group_first.p, b.cols, b.max_mn,
                       (uint32_t)b.uniform_mn, P.t, b.gemm_nkc, b.scal.p);
  } else if (b.fused_columns)
    hipLaunchKernelGGL(k_reduce_parts, dim3(cdiv(b.cols, BPP_REDUCE_TILE), b.G), dim3(64), 0, s, b.parts.p, b.rows.p, b.group_first.p, b.cols,
                       b.max_mn, P.t, b.lanes_ppw, b.scal.p);
  else
    hipLaunchKernelGGL(k_reduce_static, dim3(cdiv(b.cols, BPP_REDUCE_TILE), b.G), dim3(64), 0, s, b.rows.p, b.group_first.p, b.cols,
                       b.scal.p);
  tm.mark(M_REDUCE);
  if (plain_groups) {
    if (b.msm.split) throw EngineError{BPP_ERR_ENGINE, "plain MSM over a half-scalar layout"};
    msm_plain_run(ctx, b.msm, b.msm.h_goff, b.scal.p, P.table.p, b.dynpts.p, P.table_len, *plain_groups);
    return;
  }
  PointTables tabs{P.table.p, b.dynpts.p, P.table_len, P.table_hi.p, b.dyn_hi.p};
  if (joint) {
    hipLaunchKernelGGL(k_joint_row, dim3(cdiv(b.cols, 64)), dim3(64), 0, s, b.scal.p, b.G, b.cols, b.scal.p + (size_t)b.G * b.cols + b.total_dyn);
    msm_run(ctx, b.msm_joint, b.scal.p, tabs, &tm);
  } else {
    b.joint_accepted = false;  // (whichever entry point runs them: the per-group results are this pass's again)
    msm_run(ctx, b.msm, b.scal.p, tabs, &tm);
  }
  HIP_CHECK(hipGetLastError());
}

void collect_profile(bpp_ctx *ctx, Batch &b, StageTimer &tm, float chain_ms, float total_host_ms) {
  if (!ctx->profile) return;
  bpp_profile &pf = ctx->prof;
  memset(&pf, 0, sizeof(pf));
  pf.transcripts_ms = tm.between(M_START, M_TRANSCRIPTS);
  pf.chain_device_ms = tm.between(M_TRANSCRIPTS, M_CHAIN);  // k_weight_chain + k_chain_finish (0 with the chains on the host)
  pf.decompress_ms = tm.between(tm.have[M_CHAIN] ? M_CHAIN : M_TRANSCRIPTS, M_DECOMPRESS);  // includes the 32 B/proof device-to-host copy
  pf.scalars_ms = tm.between(M_DECOMPRESS, M_SCALARS) + tm.between(M_WEIGHTS_IN, M_LANES);  // shared + lanes
  pf.chain_host_ms = chain_ms;
  pf.reduce_ms = tm.between(M_LANES, M_REDUCE);
  pf.msm_digits_ms = 0;                             // (digits are part of the sort kernel since round 3)
  pf.msm_sort_ms = tm.between(M_REDUCE, M_ORDER);   // k_msm_prelude: digits + counting sort + size ordering of the buckets
  pf.msm_accumulate_ms = tm.between(M_ORDER, M_ACC);
  pf.msm_bucket_reduce_ms = tm.between(M_ACC, M_BUCKET);
  pf.msm_final_ms = tm.between(M_BUCKET, M_FINAL);
  pf.masks_ms = tm.between(M_MASKS0, M_MASKS);
  pf.total_ms = total_host_ms;
  pf.msm_terms = b.msm.plan.n_terms;
  pf.msm_window_bits = b.msm.plan.c;
  pf.msm_windows = b.msm.plan.K;
  pf.msm_groups = b.msm.plan.G;
}

}  // namespace

extern "C" {

int bpp_batch_prepare(bpp_ctx *ctx, uint64_t batch, size_t chunk) {
  BPP_ENTRY(ctx);
  try {
    auto it = ctx->batches.find(batch);
    if (it == ctx->batches.end()) return fail(ctx, BPP_ERR_BAD_HANDLE, "unknown batch handle");
    StageTimer tm(ctx);  // creates the profiling events when profiling is on
    ensure_ev_rng(ctx);
    layout_groups(ctx, *it->second, chunk, nullptr, true);  // group layout, both MSM plans and every work buffer of theirs
    it->second->h_ident.resize(it->second->G);
    return BPP_OK;
  }
  BPP_CATCH(ctx, nullptr, 0)
}

}  // extern "C"

namespace {

// proofs of a resident batch (0: unknown handle), read under the context's lock: the gate is always taken BEFORE that lock
uint32_t batch_size_peek(bpp_ctx *ctx, uint64_t batch) {
  std::lock_guard<std::mutex> lk(ctx->mu);
  auto it = ctx->batches.find(batch);
  return it == ctx->batches.end() ? 0u : it->second->B;
}

void shard_result_set(bpp_shard_result &r, int code, int tier, int rank, uint32_t index, const std::string &msg) {
  r.code = code;
  r.tier = tier;
  r.rank = rank;
  r.index = index;
  snprintf(r.msg, sizeof(r.msg), "%s", msg.c_str());
}

// What one verification of a resident batch leaves behind: per group of its layout the finding of the reference's verify() on
// that group alone (tier NONE: it returned Ok; `index` counts inside the group, `rank` is not used), and the recovered masks
// in b.h_masks where some group asked for them.
struct ResidentRun {
  Batch &b;
  std::vector<ShardFinding> found;
  bool have_masks = false;
  // "verify_check" (verify_flow): the groups whose final MSM this pass takes through the plain kernels -- the others' is not run
  // and their identity flag is not looked at -- and the test knob that alters this pass's results on the host
  const std::vector<uint32_t> *plain_groups = nullptr;
  const bpp_ctx::VerifyTamper *tamper = nullptr;
  int tamper_kind = 0;
  explicit ResidentRun(Batch &batch) : b(batch) {}
  // recovered masks on their way to the caller (page-locked, written by k_results_out): wiped on every exit (src/extended_mask.rs:14)
  void wipe_masks() {
    if (have_masks) wipe(b.h_masks.data(), std::min(b.h_masks.n, (size_t)b.B * b.params->t * 32));
    have_masks = false;
  }
  ~ResidentRun() { wipe_masks(); }
};

// (the context's lock is held.)  BPP_REDRAW_ON_HOST: the device chain drew a zero weight (probability 2^-252 per proof): the
// caller runs the call again with the chains on the host, which redraw as the reference does (scalar_protocol.rs:23-30)
#define BPP_REDRAW_ON_HOST (-0x7fff0001)
// One pass over a resident batch: the group layout (equal chunks, or explicit `bounds`: layout_groups), group g under
// actions[g] (actions == nullptr: `action_all` for every group), every group verified as its own verify() call by the same
// kernel launches.  A RecoverOnly group never looks at the final check (:1040-1043); when EVERY group is RecoverOnly the weight
// chains and PASS 2 are not run at all.  Engine faults throw.
int verify_flow_once(bpp_ctx *ctx, ResidentRun &run, size_t chunk, const std::vector<uint32_t> *bounds, const int *actions, int action_all,
                     bool allow_dev_chain) {
  Batch &b = run.b;
  Params &P = *b.params;
  auto t_begin = std::chrono::steady_clock::now();
  StageTimer tm(ctx);
  hipStream_t s = ctx->stream;
  layout_groups(ctx, b, chunk, bounds);
  auto action_of = [&](uint32_t g) { return actions ? actions[g] : action_all; };
  run.found.assign(b.G, ShardFinding{});
  auto find = [&](uint32_t g, auto &&checks) {
    try {
      checks();
    } catch (const ProofErr &e) {
      ShardFinding &f = run.found[g];
      f.code = e.code;
      f.tier = e.tier;
      f.index = e.index - b.h_group_first[g];  // position inside the group's own batch
      f.msg = e.msg;
    }
  };
  // verify()'s own consistency loops (:637-682) come before anything else of the call: with one group nothing needs to run
  if (b.any_defer && b.G == 1) {
    find(0, [&] { check_deferred(b.defer, 0, b.B); });
    if (run.found[0].tier != BPP_TIER_NONE) return BPP_OK;
  }
  bool any_msm = false, any_masks = false;
  for (uint32_t g = 0; g < b.G; g++) {
    any_msm = any_msm || action_of(g) != BPP_RECOVER_ONLY;
    any_masks = any_masks || action_of(g) != BPP_VERIFY_ONLY;
  }
  // a proof whose L/R count does not fit its statement makes the call fail (src/range_proof.rs:875-888).  With a
  // single group only the precedence against PASS-1 / decompression errors is still open, so PASS 2 is skipped;
  // with several groups the earlier groups' MSM verdicts still matter (the kernels tolerate the odd shapes and run on every
  // item; findings are raised per group afterwards, in the reference's order).
  const bool pass1_only = b.any_rounds_bad && b.G == 1;
  const bool want_msm = !pass1_only && any_msm;
  const bool want_masks = !pass1_only && any_masks && b.any_seed;
  // "verify_joint": one MSM over all groups of the pass when every group is held to the final check (a RecoverOnly group is not)
  // and the pass is no recheck's plain pass; its failure is answered by the per-group MSMs below (bpp.h, "Joint final check")
  bool joint = want_msm && joint_wanted(ctx, b) && !run.plain_groups;
  for (uint32_t g = 0; g < b.G && joint; g++) joint = action_of(g) != BPP_RECOVER_ONLY;
  if (joint) layout_joint(ctx, b);  // (its plan and term lists exist from the first pass on that can take it, or from bpp_batch_prepare)
  const ChainMode cmode = want_msm ? chain_mode(ctx, b, allow_dev_chain) : CHAIN_HOST;
  enqueue_phase1(ctx, b, tm, !want_msm, nullptr, 0, 0, cmode == CHAIN_DEVICE);

  b.h_ident.resize(b.G);
  for (uint32_t g = 0; g < b.G; g++) b.h_ident[g] = 1;
  float chain_ms = 0;
  if (want_msm && cmode != CHAIN_DEVICE) {
    // weight chains: one per chunk (src/range_proof.rs:811,849,853,894); the device keeps working meanwhile
    auto c0 = std::chrono::steady_clock::now();
    if (cmode == CHAIN_HOST_WIDE) run_weight_chains_wide(b);
    else run_weight_chains(b);
    chain_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - c0).count();
  }
  if (want_masks) {  // masks (:941-969)
    tm.mark(M_MASKS0);
    hipLaunchKernelGGL(k_masks, dim3(cdiv(b.B, 64)), dim3(64), 0, s, b.bytes.p, b.d_desc.p, b.chal.p, b.seeds.p,
                       P.n_bits, P.t, b.cs, b.B, b.masks.p);
    tm.mark(M_MASKS);
    b.masks_dirty = true;
    run.have_masks = true;
  }
  if (want_msm) {
    enqueue_phase2(ctx, b, tm, cmode != CHAIN_HOST, cmode == CHAIN_HOST_WIDE, run.plain_groups, joint);
    b.have_trace = true;
  }
  fetch_results(ctx, b, want_msm, want_masks, joint);
  // (the remembered wait belongs to the batch's size and group count and to what actually ran: equal work shares it)
  gpu_wait_stream(ctx, s, wait_naps(ctx, b.B), &ctx->wait_hint_end,
                  ((uint64_t)b.B << 32) | ((uint64_t)b.G << 2) | (uint64_t)((want_msm ? 1 : 0) | (want_masks ? 2 : 0)) |
                      (run.plain_groups ? 1ull << 63 : 0ull) | (joint ? 1ull << 62 : 0ull));  // (a recheck's pass 2 and a joint pass are other
                                                                                               // work: they do not teach the next call how long to nap)
  if (want_msm && cmode != CHAIN_HOST && ctx->h_chain_zero[0]) {
    ctx->device_chain_redraws++;
    return BPP_REDRAW_ON_HOST;
  }
  bool joint_fell_back = false;
  if (joint) {
    struct bpp_verify_joint_stats &js = ctx->vjoint_stats;
    js.calls++;
    b.joint_ran = true;  // (stays: a recheck's passes 2 and 3, a sharded or phased call after it do not run the joint check)
    b.joint_accepted = false;
    bool ok = b.h_ident[0] != 0;
    if (run.tamper && run.tamper_kind == 5) ok = false;  // test knob: the verdict as the host holds it, nothing else
    if (ok) {
      js.accepted++;
      b.joint_accepted = true;
      for (uint32_t g = 0; g < b.G; g++) b.h_ident[g] = 1;
    } else {
      // the per-group MSMs of today over the same scalars (nothing in front of the MSM runs again); their flags come back by
      // k_results_out with no proof to look at: status words and masks are the first wait's
      js.fallbacks++;
      joint_fell_back = true;
      PointTables tabs{P.table.p, b.dynpts.p, P.table_len, P.table_hi.p, b.dyn_hi.p};
      msm_run(ctx, b.msm, b.scal.p, tabs, nullptr);
      hipLaunchKernelGGL(k_results_out, dim3(cdiv(b.G, BPP_STATUS_BLOCK)), dim3(BPP_STATUS_BLOCK), 0, s, b.status.p, b.status0.p, b.h_status.dev(),
                         b.h_status_any.dev(), 0u, b.msm.is_identity.p, b.h_ident.dev(), b.G, (const uint4 *)nullptr, (uint4 *)nullptr, 0u);
      HIP_CHECK(hipGetLastError());
      // (a memory of its own, keyed as joint + fall-back: a rejected call does not teach the accepted ones how long to nap)
      gpu_wait_stream(ctx, s, wait_naps(ctx, b.B), &ctx->wait_hint_fallback, ((uint64_t)b.B << 32) | ((uint64_t)b.G << 2) | (3ull << 61));
    }
  }
  collect_profile(ctx, b, tm, chain_ms, std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_begin).count());
  if (run.plain_groups) {  // groups whose MSM this pass did not run: nothing is claimed about them
    std::vector<uint8_t> ran(b.G, 0);
    for (uint32_t g : *run.plain_groups) ran[g] = 1;
    for (uint32_t g = 0; g < b.G; g++)
      if (!ran[g]) b.h_ident[g] = 1;
  }
  if (run.tamper && run.tamper_kind && (uint32_t)run.tamper->group < b.G) {  // test knob: bytes of page-locked host memory only
    const uint32_t g = (uint32_t)run.tamper->group, p0 = b.h_group_first[g], p1 = b.h_group_first[g + 1];
    settle_status(b);
    auto dirty = [&](uint32_t p) { b.h_status_dirty[p / BPP_STATUS_BLOCK] = 1; };
    switch (run.tamper_kind) {
      case 1: b.h_ident[g] = 0; break;
      case 2:
        b.h_ident[g] = 1;
        for (uint32_t p = p0; p < p1; p++) {
          b.h_status[p] &= ~(BPP_ST_TRANSCRIPT_FAIL | BPP_ST_DECOMPRESS_FAIL);
          dirty(p);
        }
        break;
      case 3: b.h_status[p0] |= BPP_ST_TRANSCRIPT_FAIL; dirty(p0); break;
      case 4: b.h_status[p0] |= BPP_ST_DECOMPRESS_FAIL; dirty(p0); break;
      default: break;
    }
  }

  // errors surface chunk by chunk, in the reference's order; a chunk's MSM verdict precedes later chunks' errors
  for (uint32_t g = 0; g < b.G; g++) {
    const uint32_t p0 = b.h_group_first[g], p1 = b.h_group_first[g + 1];
    find(g, [&] {
      if (b.any_defer) check_deferred(b.defer, p0, p1);  // :637-682
      check_chunk_errors(b, p0, p1);
      if (want_msm && action_of(g) != BPP_RECOVER_ONLY && !b.h_ident[g])
        throw ProofErr{BPP_ERR_VERIFICATION_FAILED, "Range proof batch not valid", BPP_TIER_MSM, p0};
    });
  }
  if (joint_fell_back) {
    bool all_ok = true;
    for (uint32_t g = 0; g < b.G; g++) all_ok = all_ok && run.found[g].tier == BPP_TIER_NONE;
    if (all_ok) ctx->vjoint_stats.fallback_all_ok++;
  }
  return BPP_OK;
}

// first with the device's share of the weight chains, and on a zero weight once more without
void verify_flow_pass(bpp_ctx *ctx, ResidentRun &run, size_t chunk, const std::vector<uint32_t> *bounds, const int *actions, int action_all) {
  if (verify_flow_once(ctx, run, chunk, bounds, actions, action_all, true) != BPP_REDRAW_ON_HOST) return;
  run.wipe_masks();
  (void)verify_flow_once(ctx, run, chunk, bounds, actions, action_all, false);
}

inline bool device_tier(int tier) { return tier == BPP_TIER_PASS1 || tier == BPP_TIER_PASS2 || tier == BPP_TIER_MSM; }

// The agreement rule of "verify_check" over one group's outcomes in pass order (bpp.h: bpp_verify_check_resolve).  Two outcomes
// agree when code, tier and index are the same.  Returns the BPP_VCHECK_* kind; `out` is set unless the answer is PENDING.
int verify_check_resolve(const ShardFinding *passes, int n_passes, ShardFinding &out) {
  auto same = [](const ShardFinding &a, const ShardFinding &c) { return a.code == c.code && a.tier == c.tier && a.index == c.index; };
  if (!device_tier(passes[0].tier)) {
    out = passes[0];
    return BPP_VCHECK_NOT_RECHECKED;
  }
  if (n_passes < 2) return BPP_VCHECK_PENDING;
  if (same(passes[0], passes[1])) {
    out = passes[0];
    return BPP_VCHECK_CONFIRMED;
  }
  if (n_passes < 3) return BPP_VCHECK_PENDING;
  if (same(passes[0], passes[2])) {
    out = passes[0];
    return BPP_VCHECK_UPHELD;
  }
  if (same(passes[1], passes[2])) {
    out = passes[2];
    return BPP_VCHECK_OVERTURNED;
  }
  char m[160];
  snprintf(m, sizeof(m), "verify_check: three passes, three outcomes (code/tier/index): %d/%d/%u, %d/%d/%u, %d/%d/%u", passes[0].code,
           passes[0].tier, passes[0].index, passes[1].code, passes[1].tier, passes[1].index, passes[2].code, passes[2].tier, passes[2].index);
  out = ShardFinding{};
  out.code = BPP_ERR_SELF_CHECK;
  out.tier = BPP_TIER_ENGINE;
  out.rank = passes[0].rank;
  out.index = passes[0].index;
  out.msg = m;
  return BPP_VCHECK_UNDECIDED;
}

// The other form of every verifier stage that has one, given the forms pass 1 took for this batch (DESIGN.md 4.1 has the table).
// Where the shape permits no other form the engine's own rules quietly keep the one there is (plan_lanes, chain_mode).  The
// layout is an unsplit one: the plain MSM reads the term lists as they are before any half-scalar split.
void complementary_forms(bpp_ctx::Options &o, const Batch &b) {
  auto on = [](int opt, bool rule) { return opt >= 0 ? opt != 0 : rule; };
  o.transcripts_wave = on(o.transcripts_wave, b.B <= BPP_TRANSCRIPTS_WAVE_MAX) ? 0 : 1;
  o.tables_wave = on(o.tables_wave, b.B <= BPP_TABLES_WAVE_MAX) ? 0 : 1;
  o.side_decompress = on(o.side_decompress, b.B <= BPP_SIDE_DECOMPRESS_MAX) ? 0 : 1;
  o.fused_columns = b.fused_columns ? 0 : 1;
  o.static_gemm = b.static_gemm ? 0 : 1;
  const int chain = (o.chain >= 0 && o.chain <= 2) ? o.chain : (b.B >= BPP_WAIT_NAP_MIN_PROOFS ? 2 : 0);
  o.chain = chain == 0 ? 2 : 0;  // host sponges either way; the reduction mod l changes sides (a pass that runs the device chain: 0)
  o.msm_split = 0;
}

// One verification of a resident batch.  "verify_check" = 1: pass 1 is the run below, launch for launch; when it leaves a group
// with a device-tier finding, that group is verified again under the complementary forms with the plain MSM (pass 2), a third time
// under pass 1's forms when the two disagree, and the outcome two passes share is the group's (bpp.h, "Rechecked rejections").
void verify_flow(bpp_ctx *ctx, ResidentRun &run, size_t chunk, const std::vector<uint32_t> *bounds, const int *actions, int action_all) {
  const bpp_ctx::VerifyTamper tam = ctx->vtamper;  // acts on this call, checked or not, and is reset
  ctx->vtamper = bpp_ctx::VerifyTamper{};
  auto pass = [&](int k) {
    run.tamper = (tam.passes >> (k - 1)) & 1 ? &tam : nullptr;
    run.tamper_kind = tam.kind > 15 ? (tam.kind >> (4 * (k - 1))) & 15 : tam.kind;  // (above 15: a kind per pass, four bits each)
    verify_flow_pass(ctx, run, chunk, bounds, actions, action_all);
    run.tamper = nullptr;
  };
  pass(1);
  if (ctx->opt.verify_check != 1 || ctx->verify_check_off > 0) return;
  Batch &b = run.b;
  struct bpp_verify_check_stats &st = ctx->vcheck_stats;
  st.calls++;
  std::vector<uint32_t> re;
  for (uint32_t g = 0; g < b.G; g++)
    if (device_tier(run.found[g].tier)) re.push_back(g);
  if (re.empty()) return;
  st.rechecked_groups += re.size();

  const std::vector<ShardFinding> p1 = run.found;
  std::vector<ShardFinding> p2, p3;
  const bpp_ctx::Options saved = ctx->opt;
  const bool had_masks = run.have_masks;
  // passes 2 and 3 leave their masks in a buffer of their own: pass 1's stay where the accepted groups' callers get them from
  b.h_masks.swap(b.h_masks_check);
  bool swapped = true;
  auto unswap = [&] {
    if (!swapped) return;
    swapped = false;
    b.h_masks.swap(b.h_masks_check);
  };
  ScopeExit restore{[&] {  // every exit: the options as they were, no mask byte left in the check's buffer
    ctx->opt = saved;
    run.plain_groups = nullptr;
    unswap();
    if (b.h_masks_check.p) wipe(b.h_masks_check.data(), b.h_masks_check.n);
    run.have_masks = had_masks;
  }};
  complementary_forms(ctx->opt, b);
  b.G = 0;  // (the layout is built again: unsplit term lists, the lanes' shape under the other forms)
  run.plain_groups = &re;
  pass(2);
  p2 = run.found;
  run.plain_groups = nullptr;
  ctx->opt = saved;
  b.G = 0;  // and once more as pass 1 had it, whether a pass follows or not: the batch's cached plan is as before
  bool need3 = false;
  for (uint32_t g : re) {
    const ShardFinding two[2] = {p1[g], p2[g]};
    ShardFinding o;
    need3 = need3 || verify_check_resolve(two, 2, o) == BPP_VCHECK_PENDING;
  }
  if (need3) {
    pass(3);
    p3 = run.found;
  } else {
    layout_groups(ctx, b, chunk, bounds, true);
  }
  unswap();
  run.found = p1;
  const size_t row = (size_t)b.params->t * 32;
  for (uint32_t g : re) {
    const ShardFinding three[3] = {p1[g], p2[g], need3 ? p3[g] : ShardFinding{}};
    ShardFinding o;
    const int kind = verify_check_resolve(three, need3 ? 3 : 2, o);
    run.found[g] = o;
    if (kind != BPP_VCHECK_CONFIRMED) st.tie_breaks++;
    if (kind == BPP_VCHECK_CONFIRMED || kind == BPP_VCHECK_UPHELD) st.confirmed++;
    else if (kind == BPP_VCHECK_OVERTURNED) st.overturned++;
    else st.undecided++;
    // an overturned group that is Ok after all takes the masks of the pass that said so last (pass 3), through page-locked bytes only
    if (kind == BPP_VCHECK_OVERTURNED && o.tier == BPP_TIER_NONE && had_masks && b.h_masks_check.p && b.h_masks.p) {
      const size_t lo = (size_t)b.h_group_first[g] * row, hi = (size_t)b.h_group_first[g + 1] * row;
      if (hi <= b.h_masks.n && hi <= b.h_masks_check.n) memcpy(b.h_masks.data() + lo, b.h_masks_check.data() + lo, hi - lo);
    }
  }
}

// outputs: Vec<Option<ExtendedMask>> for the proofs [p0, p1): with `give`, the masks of the items that carry a seed nonce; every
// other item's slot is zero / absent
void give_masks(const ResidentRun &run, uint32_t p0, uint32_t p1, bool give, uint8_t *masks_out, uint8_t *mask_present) {
  const Batch &b = run.b;
  const size_t row = (size_t)b.params->t * 32;
  for (uint32_t p = p0; p < p1; p++) {
    const bool present = give && (b.desc[p].flags & 1u);
    if (mask_present) mask_present[p] = present ? 1 : 0;
    if (masks_out) {
      if (present) memcpy(masks_out + p * row, b.h_masks.data() + p * row, row);
      else memset(masks_out + p * row, 0, row);
    }
  }
}

// (the context's lock is held.)  The chunked form: equal chunks under one action; the first chunk with a finding ends the call
// with that finding, and masks are handed out only when no chunk had one.
// states_out203 != nullptr (bpp_verify_*_states): PASS 1 also writes every proof's advanced transcript (b.h_states), and a call that
// returns BPP_OK hands them out as rows of 203 bytes; any other outcome leaves the caller's buffer alone.
int verify_chunked_locked(bpp_ctx *ctx, uint64_t batch, int action, size_t chunk, uint8_t *masks_out, uint8_t *mask_present, char *errbuf,
                          size_t errbuf_len, uint8_t *states_out203 = nullptr) {
  try {
    auto it = ctx->batches.find(batch);
    if (it == ctx->batches.end()) return fail(ctx, BPP_ERR_BAD_HANDLE, "unknown batch handle", errbuf, errbuf_len);
    if (action < 0 || action > 2) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "unknown verify action", errbuf, errbuf_len);
    Batch &b = *it->second;
    if (b.refilled) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, BPP_REFILLED_MSG, errbuf, errbuf_len);
    if (states_out203 && b.ext_challenges)
      return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "no transcript states: the caller replayed PASS 1 of this batch", errbuf, errbuf_len);
    b.want_states = states_out203 != nullptr;
    ScopeExit states_off{[&] { b.want_states = false; }};
    ResidentRun run(b);
    verify_flow(ctx, run, chunk, nullptr, nullptr, action);
    for (const ShardFinding &f : run.found)
      if (f.tier != BPP_TIER_NONE) return fail(ctx, f.code, f.msg, errbuf, errbuf_len);
    give_masks(run, 0, run.b.B, action != BPP_VERIFY_ONLY, masks_out, mask_present);
    if (states_out203) {
      if (!b.h_states.p || b.h_states.n < (size_t)b.B * BPP_STATE_ROW_WORDS) throw EngineError{BPP_ERR_ENGINE, "transcript states were not written"};
      for (uint32_t p = 0; p < b.B; p++) state_row_to_bytes(states_out203 + (size_t)p * 203, b.h_states.data() + (size_t)p * BPP_STATE_ROW_WORDS);
    }
    return BPP_OK;
  }
  BPP_CATCH(ctx, errbuf, errbuf_len)
}

// (the context's lock is held.)  Reference batches of DIFFERENT sizes in one call: group g = proofs [group_first[g],
// group_first[g + 1]) of the resident batch, every group with its own outcome and its own VerifyAction
// (src/range_proof.rs:46-54) -- where the chunked form cuts equal chunks and stops at the first failing one.
// What a pool of small calls needs (bpp_batcher below).  actions == nullptr: VerifyOnly for every group.
// Masks (:941-969): a group whose action recovers them and whose verify() would have returned Ok gets the masks of its items
// that carry a seed nonce (an Err returns no masks).
int verify_groups_locked(bpp_ctx *ctx, uint64_t batch, const uint32_t *group_first, size_t n_groups, const int *actions,
                         bpp_shard_result *results, uint8_t *masks_out, uint8_t *mask_present) {
  try {
    auto it = ctx->batches.find(batch);
    if (it == ctx->batches.end()) return fail(ctx, BPP_ERR_BAD_HANDLE, "unknown batch handle");
    if (!group_first || !results || n_groups == 0) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "null argument");
    Batch &b = *it->second;
    if (b.refilled) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, BPP_REFILLED_MSG);
    std::vector<uint32_t> bounds(group_first, group_first + n_groups + 1);
    if (bounds.front() != 0 || bounds.back() != b.B) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "group boundaries must run from 0 to the batch size");
    for (size_t g = 0; g < n_groups; g++)
      if (bounds[g] >= bounds[g + 1]) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "empty or unordered group");
    for (size_t g = 0; actions && g < n_groups; g++)
      if (actions[g] < 0 || actions[g] > 2) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "unknown verify action");
    ResidentRun run(b);
    verify_flow(ctx, run, 0, &bounds, actions, BPP_VERIFY_ONLY);
    for (uint32_t g = 0; g < b.G; g++) {
      const ShardFinding &f = run.found[g];
      memset(&results[g], 0, sizeof(results[g]));
      shard_result_set(results[g], f.code, f.tier, -1, f.index, f.msg);
      const bool give = (actions ? actions[g] : BPP_VERIFY_ONLY) != BPP_VERIFY_ONLY && f.tier == BPP_TIER_NONE;
      give_masks(run, bounds[g], bounds[g + 1], give, masks_out, mask_present);
    }
    return BPP_OK;
  }
  BPP_CATCH(ctx, nullptr, 0)
}

// The host-buffers-in forms: `upload` makes the batch resident, then bpp_verify_resident and the release.  The small-call gate
// is held across all three and taken here, BEFORE any of them takes the context's lock.
template <class Upload>
int verify_uploaded(bpp_ctx *ctx, size_t n_items, Upload upload, int action, size_t chunk, uint8_t *masks_out, uint8_t *mask_present,
                    char *errbuf, size_t errbuf_len, uint8_t *states_out203 = nullptr) {
  if (!ctx) return BPP_ERR_BAD_HANDLE;
  GateHold gate(device_state(ctx->device), n_items <= BPP_GATE_SMALL_PROOFS);  // held across upload and verification of a small call
  uint64_t h = 0;
  int rc = upload(&h);
  if (rc != BPP_OK) return rc;
  rc = states_out203 ? bpp_verify_resident_states(ctx, h, action, chunk, masks_out, mask_present, states_out203, errbuf, errbuf_len)
                     : bpp_verify_resident(ctx, h, action, chunk, masks_out, mask_present, errbuf, errbuf_len);
  (void)bpp_batch_destroy(ctx, h);
  return rc;
}

// ---- bpp_verify_enqueue: the launches of verify_flow_once with the outcome resolved on the device (verdict.h) and no wait.
//
// Context-level, host-written state a call in flight reads, and why a second call behind it may go ahead:
//   h_chain_zero   not used: the zero-weight word is word 0 of the batch's enq_words, reset by k_verdict_finish in stream order.
//   pin_small      read by k_layout_terms only; every writer (msm_plan_alloc, layout_groups) synchronises the stream before it
//                  writes and layout_groups again before it returns, so no call in flight ever reads it.  Layouts are built by
//                  the first enqueue of a (batch, layout) alone.
//   ev_fork, ev_join, ev_rng   re-recorded by every call.  hipStreamWaitEvent waits for the record that was the event's latest
//                  WHEN THE WAIT WAS ENQUEUED; a later record does not move it.  Both streams are in order, so the side stream's
//                  decompression of call k + 1 starts behind call k's last kernel on the main stream (ev_fork) and behind call k's
//                  decompression (same stream): the two calls may even be of the same batch.
//   h_wide, h_weights, h_rng   the host chains' buffers: the device chain reads b.rng_out and writes b.weights, both device
//                  memory of the batch, ordered by the stream.
//   h_status, h_ident, h_masks   k_results_out's targets: that kernel is not launched here.
//   the per-group actions   mapped host memory of the BATCH, four slots (Batch::enq_actions): a slot is rewritten only once the
//                  ticket that last read it is done.
bool enqueue_ticket_done(bpp_ctx *ctx, uint64_t ticket) {
  if (ticket == 0 || ctx->enq_events.empty()) return true;
  const hipError_t e = hipEventQuery(ctx->enq_events[ticket % ctx->enq_events.size()]);
  if (e == hipSuccess) return true;
  if (e != hipErrorNotReady) HIP_CHECK(e);
  return false;
}
void enqueue_ticket_wait(bpp_ctx *ctx, uint64_t ticket) {
  if (ticket == 0 || ctx->enq_events.empty()) return;
  HIP_CHECK(hipEventSynchronize(ctx->enq_events[ticket % ctx->enq_events.size()]));
}
// the context's 64 ticket events, made by whichever stream call comes first; true: this call made them
bool enqueue_events_ensure(bpp_ctx *ctx) {
  if (!ctx->enq_events.empty()) return false;
  ctx->enq_events.resize(64);
  for (auto &e : ctx->enq_events) HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  return true;
}
// the next ticket, its event recorded behind what is on `s` now (the events exist: enqueue_events_ensure)
uint64_t enqueue_ticket_issue(bpp_ctx *ctx, hipStream_t s) {
  const uint64_t t = ctx->enq_next++;
  HIP_CHECK(hipEventRecord(ctx->enq_events[t % ctx->enq_events.size()], s));
  return t;
}

// would layout_groups(ctx, b, chunk, bounds) find its layout there?  (the same test)
bool layout_is_current(const Batch &b, size_t chunk, const std::vector<uint32_t> *bounds) {
  if (!b.G) return false;
  if (bounds) return b.last_chunk == (size_t)-1 && b.h_group_first == *bounds;
  return b.last_chunk == (chunk == (size_t)-1 ? 0 : chunk);
}

// with_states (bpp_verify_enqueue_states): PASS 1 runs in its STATES form into device rows of the batch, and k_states_out hands the
// rows of Ok groups' live slots to states_out_dev behind k_verdict_finish (item_states.h); everything else is the same call.
int verify_enqueue_locked(bpp_ctx *ctx, uint64_t batch, const uint32_t *group_first, size_t n_groups, size_t chunk, const int *actions,
                          int action_all, bpp_device_verdict *verdicts_dev, uint8_t *masks_dev, uint8_t *mask_present_dev, uint64_t *ticket,
                          bool with_states = false, uint8_t *states_out_dev = nullptr) {
  try {
    auto it = ctx->batches.find(batch);
    if (it == ctx->batches.end()) return fail(ctx, BPP_ERR_BAD_HANDLE, "unknown batch handle");
    if (!verdicts_dev || !ticket) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "null argument");
    if (with_states && !states_out_dev) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "states_out203_dev is null");
    Batch &b = *it->second;
    if (with_states && b.ext_challenges)
      return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "no transcript states: the caller replayed PASS 1 of this batch");
    std::vector<uint32_t> bounds;
    if (group_first) {
      if (n_groups == 0) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "null argument");
      bounds.assign(group_first, group_first + n_groups + 1);
      if (bounds.front() != 0 || bounds.back() != b.B) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "group boundaries must run from 0 to the batch size");
      for (size_t g = 0; g < n_groups; g++)
        if (bounds[g] >= bounds[g + 1]) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "empty or unordered group");
    } else {
      const uint32_t cz = (chunk == 0 || chunk >= b.B) ? b.B : (uint32_t)chunk;
      if (n_groups != 0 && n_groups != cdiv(b.B, cz))
        return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "n_groups is not the number of chunks (0: whatever it is)");
      n_groups = cdiv(b.B, cz);
    }
    if (action_all < 0 || action_all > 2) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "unknown verify action");
    for (size_t g = 0; actions && g < n_groups; g++)
      if (actions[g] < 0 || actions[g] > 2) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "unknown verify action");
    if (ctx->opt.verify_check == 1 && ctx->verify_check_off <= 0)
      return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "\"verify_check\" = 1: a rejection is rechecked by decisions of the host, which an enqueued call cannot make");
    if (b.want_states) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "the batch hands out transcript states: an enqueued call cannot");
    const struct { const void *p; const char *name; bool required; } bufs[4] = {
        {verdicts_dev, "verdicts_dev", true}, {masks_dev, "masks_dev", false}, {mask_present_dev, "mask_present_dev", false},
        {states_out_dev, "states_out203_dev", with_states}};
    for (const auto &f : bufs) {
      if (!f.p && !f.required) continue;
      const int kind = device_pointer_kind(ctx->device, f.p);
      if (kind != BPP_PTR_THIS_DEVICE)
        return fail(ctx, BPP_ERR_INVALID_ARGUMENT, std::string(f.name) + ": not device memory of the context's device (pointer kind " + std::to_string(kind) + ")");
    }
    if (((uintptr_t)verdicts_dev & 15u) || ((uintptr_t)masks_dev & 15u))
      return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "verdicts_dev / masks_dev: not 16-byte aligned");

    Params &P = *b.params;
    hipStream_t s = ctx->stream;
    struct bpp_enqueue_stats &es = ctx->enq_stats;
    const std::vector<uint32_t> *bp = group_first ? &bounds : nullptr;
    // ---- the first enqueue of a (batch, layout): what bpp_batch_prepare does, and the buffers of this path
    const bool fresh = !layout_is_current(b, chunk, bp) || !b.enq_words.p || b.enq_words.n < n_groups + 1 || !b.enq_findings_ready ||
                       b.enq_actions_G < n_groups || ctx->enq_events.empty() || !b.chain_wide.p || !ctx->d_chain_t0.p;
    if (fresh) {
      if (!enqueue_ticket_done(ctx, b.enq_last_ticket)) {  // its kernels read the layout that is about to go
        enqueue_ticket_wait(ctx, b.enq_last_ticket);
        es.host_waits++;
      }
      (void)enqueue_events_ensure(ctx);
      ensure_ev_rng(ctx);
      layout_groups(ctx, b, chunk, bp);
      b.chain_wide.alloc((size_t)b.B * 16);
      if (!ctx->d_chain_t0.p) {  // (as enqueue_device_chain makes it)
        Strobe t0;
        const char *lbl = "Bulletproofs+ verifier weights";
        merlin_new(t0, (const uint8_t *)lbl, (uint32_t)strlen(lbl));
        ctx->d_chain_t0.alloc(1);
        HIP_CHECK(hipMemcpy(ctx->d_chain_t0.p, &t0, sizeof(t0), hipMemcpyHostToDevice));
        ctx->h_chain_zero.resize(1);
      }
      if (!b.enq_words.p || b.enq_words.n < (size_t)b.G + 1) {
        b.enq_words.alloc((size_t)b.G + 1);
        HIP_CHECK(hipMemsetAsync(b.enq_words.p, 0xff, b.enq_words.n * 8, s));
        HIP_CHECK(hipMemsetAsync(b.enq_words.p, 0, 8, s));
      }
      if (!b.enq_findings_ready) {  // uploaded once, and only where there is a finding
        if (b.any_rounds_bad) {
          b.d_rounds_bad.alloc(b.B);
          HIP_CHECK(hipMemcpy(b.d_rounds_bad.p, b.rounds_bad.data(), b.B, hipMemcpyHostToDevice));
        }
        if (b.any_defer && !b.refilled) {  // (a refilled batch: d_defer is the refill kernel's, the host vector is the upload's)
          b.d_defer.alloc(b.B);
          HIP_CHECK(hipMemcpy(b.d_defer.p, b.defer.data(), b.B, hipMemcpyHostToDevice));
        }
        b.enq_findings_ready = true;
      }
      if (b.enq_actions_G < b.G) {  // (no ticket of this batch is in flight here)
        b.enq_actions.resize(4 * (size_t)b.G);
        b.enq_actions_G = b.G;
        for (auto &t : b.enq_slot_ticket) t = 0;
        b.enq_actions_next = 0;
      }
      HIP_CHECK(hipStreamSynchronize(s));
      es.layouts_in_call++;
    }
    const uint32_t G = b.G;
    // the rows PASS 1 writes for this call (the batch's first such call allocates them; no kernel in flight reads them)
    if (with_states) b.d_state_rows.alloc((size_t)b.B * BPP_STATE_ROW_WORDS);
    b.state_rows_dst = with_states ? b.d_state_rows.p : nullptr;
    ScopeExit rows_off{[&] { b.state_rows_dst = nullptr; }};
    // ---- the per-group actions where the last kernel reads them
    const int *actions_dev = nullptr;
    if (actions) {
      const size_t stride = b.enq_actions_G;
      int slot = -1;
      for (int k = 0; k < 4 && slot < 0; k++)  // a slot that holds these very actions is shared
        if (b.enq_slot_ticket[k] && memcmp(b.enq_actions.data() + k * stride, actions, (size_t)G * sizeof(int)) == 0) slot = k;
      if (slot < 0) {
        slot = (int)(b.enq_actions_next++ % 4);
        if (!enqueue_ticket_done(ctx, b.enq_slot_ticket[slot])) {
          enqueue_ticket_wait(ctx, b.enq_slot_ticket[slot]);
          es.host_waits++;
        }
        memcpy(b.enq_actions.data() + slot * stride, actions, (size_t)G * sizeof(int));
      }
      b.enq_slot_ticket[slot] = ctx->enq_next;
      actions_dev = b.enq_actions.dev() + slot * stride;
    }
    auto action_of = [&](uint32_t g) { return actions ? actions[g] : action_all; };
    bool any_msm = false, any_masks = false;
    for (uint32_t g = 0; g < G; g++) {
      any_msm = any_msm || action_of(g) != BPP_RECOVER_ONLY;
      any_masks = any_masks || action_of(g) != BPP_VERIFY_ONLY;
    }
    // the early-outs of verify_flow_once that depend on what the host knows alone
    // A refilled batch (bpp_batch_refill_enqueue): what the host knows of promises and nonces describes the upload's contents, so
    // those two decisions take the general branch -- everything runs and the verdict kernels resolve the precedence, as for G > 1;
    // masks whenever the batch has a nonce buffer.  The degree finding and rounds_bad follow from the shape and stay as they are.
    const bool any_defer = b.refilled ? b.refill_shape.t0 != P.t : b.any_defer;
    const bool any_seed = b.refilled ? b.refill_shape.nonces : b.any_seed;
    const bool deferred_only = any_defer && G == 1;  // (any_defer: some proof carries a deferred finding)
    // rounds_bad follows from the shape, which in a packed batch is uniform.  In a MIXED batch it is per slot, and under a count or a
    // mask the offending slot may be dead: the live proofs are then held to the final check as on a fresh upload of them alone, so such
    // a call takes the general branch as well (k_verdict_scan drops rounds_bad of dead slots).
    const bool pass1_only = b.any_rounds_bad && G == 1 && !(b.mixed && b.refilled && b.partial_form);
    const bool want_msm = !deferred_only && !pass1_only && any_msm;
    const bool want_masks = !deferred_only && !pass1_only && any_masks && any_seed;
    uint32_t *zero_word = reinterpret_cast<uint32_t *>(b.enq_words.p);
    unsigned long long *keys = b.enq_words.p + 1;
    StageTimer tm(ctx, false);
    // A live count (bpp_batch_refill_enqueue_count) is the device's alone: nothing here depends on it.  The chains and the two
    // verdict kernels read the batch's word; every other kernel runs over all slots, dead ones with weight zero.
    b.enq_weights = false;
    if (deferred_only) {
      if (!b.status_clean) HIP_CHECK(hipMemcpyAsync(b.status.p, b.status0.p, (size_t)b.B * 4, hipMemcpyDeviceToDevice, s));
    } else {
      enqueue_phase1(ctx, b, tm, !want_msm, nullptr, 0, 0, want_msm, zero_word);
      b.enq_weights = want_msm;
      if (want_masks) {
        hipLaunchKernelGGL(k_masks, dim3(cdiv(b.B, 64)), dim3(64), 0, s, b.bytes.p, b.d_desc.p, b.chal.p, b.seeds.p, P.n_bits, P.t, b.cs, b.B,
                           b.masks.p);
        b.masks_dirty = true;
      }
      if (want_msm) {
        enqueue_phase2(ctx, b, tm, true, false, nullptr, false);
        b.have_trace = true;
      }
    }
    const LiveView lv = b.live_view();  // the form of the batch's last refill: a count word, mask bytes (the MASKED kernels), or neither
    const uint8_t *rounds_bad = b.d_rounds_bad.p ? (const uint8_t *)b.d_rounds_bad.p : (const uint8_t *)nullptr;
    const uint8_t *defer = b.d_defer.p ? (const uint8_t *)b.d_defer.p : (const uint8_t *)nullptr;
    if (lv.mask)
      hipLaunchKernelGGL(k_verdict_scan<true>, dim3(cdiv(b.B, BPP_VERDICT_BLOCK)), dim3(BPP_VERDICT_BLOCK), 0, s, b.status.p, b.status0.p,
                         rounds_bad, defer, b.B, b.group_first.p, G, keys, lv);
    else
      hipLaunchKernelGGL(k_verdict_scan<false>, dim3(cdiv(b.B, BPP_VERDICT_BLOCK)), dim3(BPP_VERDICT_BLOCK), 0, s, b.status.p, b.status0.p,
                         rounds_bad, defer, b.B, b.group_first.p, G, keys, lv);
    b.status_clean = true;  // (in stream order, as behind k_results_out)
    const uint32_t *identity = want_msm ? b.msm.is_identity.p : (const uint32_t *)nullptr;
    const uint4 *mask_rows = want_masks ? (const uint4 *)b.masks.p : (const uint4 *)nullptr;
    const unsigned long long *state = b.refill_state.p ? (const unsigned long long *)b.refill_state.p : (const unsigned long long *)nullptr;
    if (lv.mask)
      hipLaunchKernelGGL(k_verdict_finish<true>, dim3(G), dim3(64), 0, s, keys, identity, actions_dev, action_all, zero_word, zero_word + 1,
                         b.group_first.p, G, b.d_desc.p, mask_rows, (uint32_t)(P.t * 2), verdicts_dev, (uint4 *)masks_dev, mask_present_dev, state, lv);
    else
      hipLaunchKernelGGL(k_verdict_finish<false>, dim3(G), dim3(64), 0, s, keys, identity, actions_dev, action_all, zero_word, zero_word + 1,
                         b.group_first.p, G, b.d_desc.p, mask_rows, (uint32_t)(P.t * 2), verdicts_dev, (uint4 *)masks_dev, mask_present_dev, state, lv);
    if (with_states) {  // (a call that ran no PASS 1 has no Ok group: every row is zero and the rows buffer is not looked at)
      const StatesOut so{b.d_state_rows.p, BPP_STATE_ROW_WORDS, states_out_dev, verdicts_dev, b.group_first.p, G, b.B, lv};
      hipLaunchKernelGGL(k_states_out, dim3(cdiv(b.B, BPP_INGEST_BLOCK / BPP_INGEST_LANES)), dim3(BPP_INGEST_BLOCK), 0, s, so);
    }
    HIP_CHECK(hipGetLastError());
    *ticket = b.enq_last_ticket = enqueue_ticket_issue(ctx, s);
    es.calls++;
    es.groups += G;
    return BPP_OK;
  }
  BPP_CATCH(ctx, nullptr, 0)
}

// ---- bpp_batch_refill_enqueue (refill.h): new contents of the same shape for a resident batch, on the stream, no wait.
//
// The list above verify_enqueue_locked, for a refill: it writes nothing the host owns and reads nothing the host writes -- its
// arguments travel by value, its reduction words and the state word are device memory of the batch, kept clear by k_refill_finish.
// An enqueue in flight on the batch is in front of it on the stream, side stream included: every enqueue ends with the main stream
// waiting for ev_join; the next enqueue's side-stream decompression waits for an ev_fork recorded behind the refill.  The action slots
// and the layout are the shape's and stay.
// count_dev and live_dev (at most one of them): the count form and the mask form of the refill.  The batch is in the form of its last
// refill: a mask refill switches the chain and verdict kernels to their MASKED forms on the batch's own copy of the mask, any other
// refill switches them back.  batch_refill_locked is the driver of every refill call, over what PackedRefill and MixedRefill supply;
// it ends in refill_enqueue_tail.

// what every refill refuses alike: the kind of memory behind the caller's six arrays and
// behind record_dev / count_dev / live_dev, and the alignment of the two that are read or written as words.  Empty: nothing to refuse.
std::string refill_pointer_refusal(bpp_ctx *ctx, const void *proofs, const void *commitments32, const void *min_values, const void *min_present,
                                   const void *seed_nonces32, const void *seed_present, const bpp_device_refill *record_dev,
                                   const uint32_t *count_dev, const uint8_t *live_dev) {
  const struct {
    const char *name;
    const void *p;
  } arrays[] = {{"proofs", proofs},           {"commitments32", commitments32}, {"min_values", min_values},
                {"min_present", min_present}, {"seed_nonces32", seed_nonces32}, {"seed_present", seed_present},
                {"record_dev", record_dev},   {"count_dev", count_dev},         {"live_dev", live_dev}};
  for (const auto &a : arrays) {
    if (!a.p) continue;
    const int kind = device_pointer_kind(ctx->device, a.p);
    if (kind != BPP_PTR_THIS_DEVICE)
      return std::string(a.name) + ": not device memory of the context's device (pointer kind " + std::to_string(kind) + ")";
  }
  if ((uintptr_t)record_dev & 3u) return "record_dev: not 4-byte aligned";
  if ((uintptr_t)count_dev & 3u) return "count_dev: not 4-byte aligned";
  return std::string();
}

// per-item transcripts are part of the shape a batch keeps: the *_transcripts refills take only batches the *_transcripts uploads made,
// the other refills refuse those; either text names the call to use instead.  Then the call's own state pointer.  Empty: nothing to refuse.
std::string refill_item_states_refusal(bpp_ctx *ctx, const Batch &b, bool with_states, const uint8_t *item_states_dev, bool mixed) {
  const std::string with = mixed ? "bpp_batch_refill_enqueue_mixed_transcripts" : "bpp_batch_refill_enqueue_transcripts";
  const std::string without = mixed ? "bpp_batch_refill_enqueue_mixed" : "bpp_batch_refill_enqueue / _count / _live";
  if (b.item_states && !with_states)
    return "the batch was uploaded with per-item transcripts and every refill brings its rows: use " + with;
  if (!b.item_states && with_states)
    return "the batch was not uploaded with per-item transcripts (bpp_batch_upload_*_device_transcripts) and keeps its one transcript: use " + without;
  if (!with_states) return std::string();
  if (!item_states_dev) return "item_states203_dev is null";
  const int kind = device_pointer_kind(ctx->device, item_states_dev);
  if (kind != BPP_PTR_THIS_DEVICE) return "item_states203_dev: not device memory of the context's device (pointer kind " + std::to_string(kind) + ")";
  if (b.states.n < (size_t)b.B * BPP_ITEM_STATE_BYTES) return "refill: the batch's state table does not fit its recorded shape";
  return std::string();
}

// The common tail of the two refill drivers, behind their refusals: the batch's first-call allocations, the form flags, the launches
// and the ticket.  `launch_refill(s, masked)` makes the driver's kernel arguments -- the batch's words and mask exist by then -- and
// launches its refill kernel in the plain/count or the masked form; k_refill_finish and the decompression of the commitments follow it.
// item_states_dev (a batch with per-item transcripts, else null): k_item_states follows the refill kernel -- it reads the batch's
// normalised mask that kernel wrote -- and reduces into the same finding word in front of k_refill_finish.
template <class LaunchRefill>
void refill_enqueue_tail(bpp_ctx *ctx, Batch &b, bool nonces, const uint32_t *count_dev, const uint8_t *live_dev, bpp_device_refill *record_dev,
                         uint64_t *ticket, const uint8_t *item_states_dev, LaunchRefill &&launch_refill) {
  const size_t n = b.B;
  hipStream_t s = ctx->stream;
  struct bpp_refill_stats &rs = ctx->refill_stats;
  bool first = false;
  if (!b.refill_red.p) {  // the first refill of this batch: its few device words, and d_defer where no enqueue made it
    b.refill_red.alloc(BPP_REFILL_RED_WORDS);
    b.refill_state.alloc(1);
    b.refill_live.alloc(1);  // (written by the first refill that takes a count, read only from then on)
    b.d_defer.alloc(n);
    HIP_CHECK(hipMemsetAsync(b.refill_red.p, 0, BPP_REFILL_RED_WORDS * 4, s));
    HIP_CHECK(hipMemsetAsync(b.refill_state.p, 0, 8, s));
    first = true;
  }
  if (live_dev && !b.refill_mask.p) {  // the first refill of this batch under a mask: its N bytes, written by the kernel below
    b.refill_mask.alloc(n);
    first = true;
  }
  if (first) rs.first_calls++;
  (void)enqueue_events_ensure(ctx);
  if (count_dev) b.has_live = true;
  b.mask_form = live_dev != nullptr;
  b.partial_form = count_dev != nullptr || live_dev != nullptr;
  b.enq_weights = false;
  b.refilled = true;  // from here on the contents are the stream's, whatever becomes of the launches
  b.seeds_dirty = nonces;
  launch_refill(s, b.mask_form);
  if (item_states_dev) {
    const ItemStates a{item_states_dev, b.states.p, (uint32_t)n, (uint32_t)n, b.refill_red.p + BPP_REFILL_RED_FINDING, count_dev,
                       b.mask_form ? (const uint8_t *)b.refill_mask.p : (const uint8_t *)nullptr};
    hipLaunchKernelGGL(k_item_states, dim3((uint32_t)cdiv((uint32_t)n, BPP_INGEST_BLOCK / BPP_INGEST_LANES)), dim3(BPP_INGEST_BLOCK), 0, s, a);
  }
  // (under a mask nothing is clamped and the batch's count word is left alone: the later kernels do not read it in that form)
  hipLaunchKernelGGL(k_refill_finish, dim3(1), dim3(64), 0, s, b.refill_red.p, b.refill_state.p, record_dev, count_dev, (uint32_t)n,
                     (b.has_live && !b.mask_form) ? b.refill_live.p : (uint32_t *)nullptr);
  // the statements' commitments, decoded as at the end of upload_device: COMMIT_FAIL goes to status0[] and status[]
  hipLaunchKernelGGL(k_decompress, dim3(cdiv(b.sum_m, 64)), dim3(64), 0, s, b.bytes.p, b.src_off.p, b.owner.p, b.idx_commit.p, b.sum_m,
                     b.dynpts.p, b.status0.p, (uint32_t *)nullptr, b.status.p);
  HIP_CHECK(hipGetLastError());
  b.status_clean = true;
  b.masks_dirty = false;  // (the kernel wiped every row)
  b.have_trace = b.phase1_done = false;
  b.enq_last_ticket = enqueue_ticket_issue(ctx, s);
  if (ticket) *ticket = b.enq_last_ticket;
  rs.calls++;
}

// the fields of a refill that must repeat the batch's shape, in the order they are refused.  Empty: nothing to refuse.
struct RefillShapeField {
  const char *name;
  bool same;
};
std::string refill_shape_refusal(std::initializer_list<RefillShapeField> fields) {
  for (const auto &f : fields)
    if (!f.same) return std::string(f.name) + " differs from the batch's shape: a refill keeps the shape of the upload";
  return std::string();
}

// What the packed and the mixed refill supply to batch_refill_locked: which batches they take, what of the caller's struct must repeat
// the batch's shape, what the kernel writes against what the upload allocated, and the kernel with its arguments.
struct PackedRefill {
  const bpp_packed_batch &in;
  static constexpr bool mixed = false;
  static bool takes(const Batch &b) { return b.refillable; }
  static const char *cannot() {
    return "the batch cannot be refilled: only a batch that bpp_batch_upload_packed_device packed on the device records its shape (not the "
           "item form, the host packed form, the staged fall-back, caller-side challenges or a batch that hands out states)";
  }
  std::string shape_refusal(bpp_ctx *, const Batch &b) const {
    const Batch::RefillShape &sh = b.refill_shape;
    const std::string refusal = refill_shape_refusal({{"n_items", (uint64_t)in.n_items == sh.n_items},
                                                      {"m", in.m == sh.m},
                                                      {"proof_len", (uint64_t)in.proof_len == sh.proof_len},
                                                      {"seed_nonces32", (in.seed_nonces32 != nullptr) == sh.nonces},
                                                      {"min_values", (in.min_values != nullptr) == sh.min_values},
                                                      {"min_present", (in.min_present != nullptr) == sh.min_present}});
    if (!refusal.empty()) return refusal;
    return in.proof_stride < in.proof_len ? "proof_stride is below proof_len" : std::string();
  }
  std::string vector_refusal(const Batch &) const { return std::string(); }
  bool fits(const Batch &b) const {
    const Batch::RefillShape &sh = b.refill_shape;
    const size_t n = b.B;
    return b.bytes.n >= n * sh.proof_len + n * (size_t)sh.m * 32 + BPP_BYTES_SLACK && b.minvals.n >= n * (size_t)sh.m && b.sum_m == n * sh.m;
  }
  Refill args(Batch &b, const ParamShape &P, const uint32_t *count_dev, const uint8_t *live_dev) const {
    return refill_args(in, P, (uint8_t)b.refill_shape.t0, b.bytes.p, b.minvals.p, b.seeds.p, b.d_defer.p, b.d_desc.p, b.status0.p, b.status.p,
                       reinterpret_cast<uint32_t *>(b.masks.p), b.refill_red.p, count_dev, live_dev, b.refill_mask.p);
  }
  static auto kernel(bool masked) { return masked ? k_refill_packed<true> : k_refill_packed<false>; }
};

// The mixed batch's shape is the vector (proof_lens[i], m[i]) the upload recorded (Batch::mixed_shape, on the device Batch::mixed_table);
// in.proof_lens / in.m are host arrays that must repeat it, or both null -- then nothing of size N is touched here.  The strides are the
// SOURCE's and need only hold the batch's longest row.
struct MixedRefill {
  const bpp_mixed_batch &in;
  static constexpr bool mixed = true;
  static bool takes(const Batch &b) { return b.mixed && b.mixed_table.p && !b.mixed_shape.rows.empty(); }
  static const char *cannot() {
    return "the batch cannot be refilled from a mixed batch: only a batch that bpp_batch_upload_mixed_device packed on the device records "
           "its shape vector (not its staged fall-back, the host mixed form, a packed or item batch, caller-side challenges or a batch "
           "that hands out states)";
  }
  std::string shape_refusal(bpp_ctx *ctx, const Batch &b) const {
    const Batch::RefillShape &sh = b.refill_shape;
    const Batch::MixedShape &ms = b.mixed_shape;
    std::string refusal = refill_shape_refusal({{"n_items", (uint64_t)in.n_items == sh.n_items},
                                                {"seed_nonces32", (in.seed_nonces32 != nullptr) == sh.nonces},
                                                {"seed_present", (in.seed_present != nullptr) == ms.seed_present},
                                                {"min_values", (in.min_values != nullptr) == sh.min_values},
                                                {"min_present", (in.min_present != nullptr) == sh.min_present}});
    if (!refusal.empty()) return refusal;
    if ((in.proof_lens != nullptr) != (in.m != nullptr))
      return "proof_lens and m: give both (they must repeat the batch's vectors) or neither (the batch's own)";
    refusal = mixed_host_arrays_refusal(ctx, in, "names the batch's shape");
    if (!refusal.empty()) return refusal;
    if (in.proof_stride < ms.max_proof_len) return "proof_stride is below the batch's largest proof_len (" + std::to_string(ms.max_proof_len) + ")";
    if (in.m_stride < ms.max_m) return "m_stride is below the batch's largest m (" + std::to_string(ms.max_m) + ")";
    return std::string();
  }
  std::string vector_refusal(const Batch &b) const {
    for (size_t i = 0; in.proof_lens && i < b.B; i++) {
      const IngestMixedRow &row = b.mixed_shape.rows[i];
      const char *field = (uint64_t)in.proof_lens[i] != row.proof_len ? "proof_lens" : (in.m[i] != row.m ? "m" : nullptr);
      if (field) return std::string(field) + "[" + std::to_string(i) + "] differs from the batch's shape: a refill keeps the shape of the upload";
    }
    return std::string();
  }
  bool fits(const Batch &b) const {
    const Batch::MixedShape &ms = b.mixed_shape;
    const size_t n = b.B;
    return ms.rows.size() == n && b.mixed_table.n >= n && b.bytes.n >= ms.proof_bytes + (size_t)b.sum_m * 32 + BPP_BYTES_SLACK &&
           b.minvals.n >= b.sum_m && (uint64_t)ms.rows[n - 1].minval_idx + ms.rows[n - 1].m == b.sum_m &&
           (uint64_t)ms.rows[n - 1].proof_off + ms.rows[n - 1].proof_len == ms.proof_bytes;
  }
  Refill args(Batch &b, const ParamShape &P, const uint32_t *count_dev, const uint8_t *live_dev) const {
    return refill_mixed_args(in, P, (uint8_t)b.refill_shape.t0, b.mixed_table.p, b.B, b.mixed_shape.proof_bytes, b.sum_m, b.bytes.p, b.minvals.p,
                             b.seeds.p, b.d_defer.p, b.d_desc.p, b.status0.p, b.status.p, reinterpret_cast<uint32_t *>(b.masks.p), b.refill_red.p,
                             count_dev, live_dev, b.refill_mask.p);
  }
  static auto kernel(bool masked) { return masked ? k_refill_mixed<true> : k_refill_mixed<false>; }
};

// the driver of every refill call.  Everything is refused before the tail.
template <class Form, class In>
int batch_refill_locked(bpp_ctx *ctx, uint64_t batch, const In *in, const uint32_t *count_dev, const uint8_t *live_dev, bpp_device_refill *record_dev,
                        uint64_t *ticket, bool with_states = false, const uint8_t *item_states_dev = nullptr) {
  try {
    auto it = ctx->batches.find(batch);
    if (it == ctx->batches.end()) return fail(ctx, BPP_ERR_BAD_HANDLE, "unknown batch handle");
    if (!in) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "null argument");
    Batch &b = *it->second;
    const Form form{*in};
    if (!Form::takes(b) || b.ext_challenges || b.want_states) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, Form::cannot());
    if (count_dev && live_dev) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "count_dev and live_dev: a refill takes a live count or a live mask, not both");
    std::string refusal = refill_item_states_refusal(ctx, b, with_states, item_states_dev, Form::mixed);
    if (refusal.empty()) refusal = form.shape_refusal(ctx, b);
    if (refusal.empty() && (in->transcript_state || in->transcript_label))
      refusal = with_states ? "transcript_state / transcript_label must be null: item i is verified under row i of item_states203_dev"
                            : "transcript_state / transcript_label must be null: a refilled batch keeps its transcript";
    if (refusal.empty() && (!in->proofs || !in->commitments32)) refusal = "proofs / commitments32: null";
    if (refusal.empty())
      refusal = refill_pointer_refusal(ctx, in->proofs, in->commitments32, in->min_values, in->min_present, in->seed_nonces32, in->seed_present,
                                       record_dev, count_dev, live_dev);
    if (refusal.empty()) refusal = form.vector_refusal(b);
    if (!refusal.empty()) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, refusal);
    Params &P = *b.params;
    const size_t n = b.B;
    const bool nonces = b.refill_shape.nonces;
    // what the kernel writes, against what the upload allocated (the shape says they fit; a kernel is not launched on less)
    if (!form.fits(b) || (nonces && b.seeds.n < n * 32) || b.d_desc.n < n || b.status0.n < n || b.status.n < n || b.masks.n < n * (size_t)P.t * 32)
      throw EngineError{BPP_ERR_ENGINE, "refill: the batch's buffers do not fit its recorded shape"};
    const ParamShape shape_p{P.n_bits, P.m_max, P.t};
    refill_enqueue_tail(ctx, b, nonces, count_dev, live_dev, record_dev, ticket, item_states_dev, [&](hipStream_t s, bool masked) {
      const Refill r = form.args(b, shape_p, count_dev, live_dev);
      hipLaunchKernelGGL(Form::kernel(masked), dim3((uint32_t)cdiv((uint32_t)n, BPP_INGEST_BLOCK / BPP_INGEST_LANES)), dim3(BPP_INGEST_BLOCK), 0, s, r);
    });
    return BPP_OK;
  }
  BPP_CATCH(ctx, nullptr, 0)
}

}  // namespace

extern "C" {

int bpp_verify_resident(bpp_ctx *ctx, uint64_t batch, int action, size_t chunk, uint8_t *masks_out, uint8_t *mask_present,
                        char *errbuf, size_t errbuf_len) {
  if (!ctx) return BPP_ERR_BAD_HANDLE;
  const uint32_t n_peek = batch_size_peek(ctx, batch);
  GateHold gate(device_state(ctx->device), n_peek && n_peek <= BPP_GATE_SMALL_PROOFS);  // small calls queue for the device (DeviceState)
  BPP_ENTRY(ctx);
  return verify_chunked_locked(ctx, batch, action, chunk, masks_out, mask_present, errbuf, errbuf_len);
}

int bpp_verify_resident_states(bpp_ctx *ctx, uint64_t batch, int action, size_t chunk, uint8_t *masks_out, uint8_t *mask_present,
                               uint8_t *states_out203, char *errbuf, size_t errbuf_len) {
  if (!ctx) return BPP_ERR_BAD_HANDLE;
  const uint32_t n_peek = batch_size_peek(ctx, batch);
  GateHold gate(device_state(ctx->device), n_peek && n_peek <= BPP_GATE_SMALL_PROOFS);
  BPP_ENTRY(ctx);
  if (!states_out203) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "null argument", errbuf, errbuf_len);
  return verify_chunked_locked(ctx, batch, action, chunk, masks_out, mask_present, errbuf, errbuf_len, states_out203);
}

int bpp_verify_resident_groups_actions(bpp_ctx *ctx, uint64_t batch, const uint32_t *group_first, size_t n_groups, const int *actions,
                                       bpp_shard_result *results, uint8_t *masks_out, uint8_t *mask_present) {
  if (!ctx) return BPP_ERR_BAD_HANDLE;
  const uint32_t n_peek = batch_size_peek(ctx, batch);
  GateHold gate(device_state(ctx->device), n_peek && n_peek <= BPP_GATE_SMALL_PROOFS);  // small calls queue for the device (DeviceState)
  BPP_ENTRY(ctx);
  return verify_groups_locked(ctx, batch, group_first, n_groups, actions, results, masks_out, mask_present);
}

int bpp_verify_resident_groups(bpp_ctx *ctx, uint64_t batch, const uint32_t *group_first, size_t n_groups, bpp_shard_result *results) {
  return bpp_verify_resident_groups_actions(ctx, batch, group_first, n_groups, nullptr, results, nullptr, nullptr);
}

// (no gate: enqueued calls are serial on their stream, and the gate has no place to release them)
int bpp_verify_enqueue(bpp_ctx *ctx, uint64_t batch, const uint32_t *group_first, size_t n_groups, size_t chunk, const int *actions, int action_all,
                       bpp_device_verdict *verdicts_dev, uint8_t *masks_dev, uint8_t *mask_present_dev, uint64_t *ticket) {
  BPP_ENTRY(ctx);
  return verify_enqueue_locked(ctx, batch, group_first, n_groups, chunk, actions, action_all, verdicts_dev, masks_dev, mask_present_dev, ticket);
}

int bpp_enqueue_done(bpp_ctx *ctx, uint64_t ticket, int *done) {
  BPP_ENTRY(ctx);
  try {
    if (!done) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "null argument");
    if (ticket == 0 || ticket >= ctx->enq_next) return fail(ctx, BPP_ERR_BAD_HANDLE, "unknown ticket");
    *done = enqueue_ticket_done(ctx, ticket) ? 1 : 0;
    return BPP_OK;
  }
  BPP_CATCH(ctx, nullptr, 0)
}

int bpp_enqueue_wait(bpp_ctx *ctx, uint64_t ticket) {
  BPP_ENTRY(ctx);
  try {
    if (ticket == 0 || ticket >= ctx->enq_next) return fail(ctx, BPP_ERR_BAD_HANDLE, "unknown ticket");
    enqueue_ticket_wait(ctx, ticket);
    return BPP_OK;
  }
  BPP_CATCH(ctx, nullptr, 0)
}

int bpp_verdict_result(const bpp_device_verdict *host_copy, bpp_shard_result *out) {
  if (!host_copy || !out || !(host_copy->flags & BPP_VERDICT_WRITTEN)) return BPP_ERR_INVALID_ARGUMENT;
  memset(out, 0, sizeof(*out));
  if (host_copy->flags & BPP_VERDICT_EMPTY)
    shard_result_set(*out, BPP_OK, BPP_TIER_NONE, -1, 0, "the group held no live item of the batch's last refill: nothing was verified");
  else if (host_copy->flags & BPP_VERDICT_REFILL)
    shard_result_set(*out, host_copy->code, (int)host_copy->tier, -1, host_copy->index,
                     "the batch's last refill did not take: nothing of this verification is claimed, see the refill record (bpp_refill_result)");
  else if (host_copy->flags & BPP_VERDICT_REDRAW)
    shard_result_set(*out, BPP_OK, BPP_TIER_NONE, -1, 0, "a device weight came out zero: nothing is claimed, run a blocking call");
  else
    shard_result_set(*out, host_copy->code, (int)host_copy->tier, -1, host_copy->index, verdict_message(host_copy->tier, host_copy->code));
  return BPP_OK;
}

// (no gate, as bpp_verify_enqueue)
int bpp_batch_refill_enqueue(bpp_ctx *ctx, uint64_t batch, const bpp_packed_batch *in_dev, bpp_device_refill *record_dev, uint64_t *ticket) {
  BPP_ENTRY(ctx);
  return batch_refill_locked<PackedRefill>(ctx, batch, in_dev, nullptr, nullptr, record_dev, ticket);
}

int bpp_batch_refill_enqueue_count(bpp_ctx *ctx, uint64_t batch, const bpp_packed_batch *in_dev, const uint32_t *count_dev,
                                   bpp_device_refill *record_dev, uint64_t *ticket) {
  BPP_ENTRY(ctx);
  return batch_refill_locked<PackedRefill>(ctx, batch, in_dev, count_dev, nullptr, record_dev, ticket);
}

int bpp_batch_refill_enqueue_live(bpp_ctx *ctx, uint64_t batch, const bpp_packed_batch *in_dev, const uint8_t *live_dev,
                                  bpp_device_refill *record_dev, uint64_t *ticket) {
  BPP_ENTRY(ctx);
  return batch_refill_locked<PackedRefill>(ctx, batch, in_dev, nullptr, live_dev, record_dev, ticket);
}

int bpp_batch_refill_enqueue_mixed(bpp_ctx *ctx, uint64_t batch, const bpp_mixed_batch *in_dev, const uint32_t *count_dev, const uint8_t *live_dev,
                                   bpp_device_refill *record_dev, uint64_t *ticket) {
  BPP_ENTRY(ctx);
  return batch_refill_locked<MixedRefill>(ctx, batch, in_dev, count_dev, live_dev, record_dev, ticket);
}

// ---- per-item transcripts (item_states.h): the refills of a batch the *_transcripts uploads made, and the enqueue that hands the
// advanced transcripts back on the stream
int bpp_batch_refill_enqueue_transcripts(bpp_ctx *ctx, uint64_t batch, const bpp_packed_batch *in_dev, const uint8_t *item_states203_dev,
                                         const uint32_t *count_dev, const uint8_t *live_dev, bpp_device_refill *record_dev, uint64_t *ticket) {
  BPP_ENTRY(ctx);
  return batch_refill_locked<PackedRefill>(ctx, batch, in_dev, count_dev, live_dev, record_dev, ticket, true, item_states203_dev);
}

int bpp_batch_refill_enqueue_mixed_transcripts(bpp_ctx *ctx, uint64_t batch, const bpp_mixed_batch *in_dev, const uint8_t *item_states203_dev,
                                               const uint32_t *count_dev, const uint8_t *live_dev, bpp_device_refill *record_dev,
                                               uint64_t *ticket) {
  BPP_ENTRY(ctx);
  return batch_refill_locked<MixedRefill>(ctx, batch, in_dev, count_dev, live_dev, record_dev, ticket, true, item_states203_dev);
}

int bpp_verify_enqueue_states(bpp_ctx *ctx, uint64_t batch, const uint32_t *group_first, size_t n_groups, size_t chunk, const int *actions,
                              int action_all, bpp_device_verdict *verdicts_dev, uint8_t *masks_dev, uint8_t *mask_present_dev,
                              uint8_t *states_out203_dev, uint64_t *ticket) {
  BPP_ENTRY(ctx);
  return verify_enqueue_locked(ctx, batch, group_first, n_groups, chunk, actions, action_all, verdicts_dev, masks_dev, mask_present_dev, ticket,
                               true, states_out203_dev);
}

// (a diagnostic: one device-to-device copy on the stream behind the batch's last enqueue)
int bpp_enqueue_weights(bpp_ctx *ctx, uint64_t batch, uint8_t *weights_dev, uint64_t *ticket) {
  BPP_ENTRY(ctx);
  try {
    auto it = ctx->batches.find(batch);
    if (it == ctx->batches.end()) return fail(ctx, BPP_ERR_BAD_HANDLE, "unknown batch handle");
    Batch &b = *it->second;
    if (!weights_dev) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "null argument");
    if (!b.enq_weights || !b.weights.p || ctx->enq_events.empty())
      return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "the batch's last call on the stream was not a bpp_verify_enqueue that drew weights");
    const int kind = device_pointer_kind(ctx->device, weights_dev);
    if (kind != BPP_PTR_THIS_DEVICE)
      return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "weights_dev: not device memory of the context's device (pointer kind " + std::to_string(kind) + ")");
    HIP_CHECK(hipMemcpyAsync(weights_dev, b.weights.p, (size_t)b.B * 32, hipMemcpyDeviceToDevice, ctx->stream));
    b.enq_last_ticket = enqueue_ticket_issue(ctx, ctx->stream);
    if (ticket) *ticket = b.enq_last_ticket;
    return BPP_OK;
  }
  BPP_CATCH(ctx, nullptr, 0)
}

int bpp_refill_result(const bpp_device_refill *host_copy, bpp_shard_result *out) {
  if (!host_copy || !out || !(host_copy->flags & BPP_REFILL_WRITTEN)) return BPP_ERR_INVALID_ARGUMENT;
  memset(out, 0, sizeof(*out));
  if (host_copy->flags & BPP_REFILL_COUNT)
    shard_result_set(*out, BPP_OK, BPP_TIER_NONE, -1, 0,
                     "the live count exceeds the batch's item count: no item was taken and nothing is claimed, refill with a count the batch holds");
  else if (host_copy->flags & BPP_REFILL_FALLBACK)
    shard_result_set(*out, BPP_OK, BPP_TIER_NONE, -1, 0,
                     "some proof's first byte is not the batch's: nothing is claimed, upload the arrays with a blocking call");
  else if (host_copy->flags & BPP_REFILL_FINDING)
    shard_result_set(*out, host_copy->code, BPP_TIER_CONSTRUCTION, -1, host_copy->index, ingest_message(host_copy->msg));
  else
    shard_result_set(*out, BPP_OK, BPP_TIER_NONE, -1, 0, "");
  return BPP_OK;
}

int bpp_refill_stats(bpp_ctx *ctx, struct bpp_refill_stats *out) {
  BPP_ENTRY(ctx);
  if (!out) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "null argument");
  *out = ctx->refill_stats;
  return BPP_OK;
}

int bpp_enqueue_stats(bpp_ctx *ctx, struct bpp_enqueue_stats *out) {
  BPP_ENTRY(ctx);
  if (!out) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "null argument");
  *out = ctx->enq_stats;
  return BPP_OK;
}

int bpp_verify_batch_with_challenges(bpp_ctx *ctx, uint64_t params, const bpp_verify_item *items, size_t n_items,
                                     const uint8_t *const *challenges32, const uint8_t *rng_out32, int action, size_t chunk,
                                     uint8_t *masks_out, uint8_t *mask_present, char *errbuf, size_t errbuf_len) {
  auto upload = [&](uint64_t *h) -> int {
    BPP_ENTRY(ctx);
    if (!challenges32 || !rng_out32) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "null argument", errbuf, errbuf_len);
    return upload_impl(ctx, params, items, n_items, nullptr, h, challenges32, rng_out32, errbuf, errbuf_len);
  };
  return verify_uploaded(ctx, n_items, upload, action, chunk, masks_out, mask_present, errbuf, errbuf_len);
}

int bpp_verify_batch(bpp_ctx *ctx, uint64_t params, const bpp_verify_item *items, size_t n_items, int action,
                     size_t chunk, uint8_t *masks_out, uint8_t *mask_present, char *errbuf, size_t errbuf_len) {
  auto upload = [&](uint64_t *h) -> int { return bpp_batch_upload(ctx, params, items, n_items, h, errbuf, errbuf_len); };
  return verify_uploaded(ctx, n_items, upload, action, chunk, masks_out, mask_present, errbuf, errbuf_len);
}

int bpp_verify_batch_packed(bpp_ctx *ctx, uint64_t params, const bpp_packed_batch *in, int action, size_t chunk,
                            uint8_t *masks_out, uint8_t *mask_present, char *errbuf, size_t errbuf_len) {
  auto upload = [&](uint64_t *h) -> int { return bpp_batch_upload_packed(ctx, params, in, h, errbuf, errbuf_len); };
  return verify_uploaded(ctx, in ? in->n_items : SIZE_MAX, upload, action, chunk, masks_out, mask_present, errbuf, errbuf_len);
}

int bpp_verify_batch_packed_device(bpp_ctx *ctx, uint64_t params, const bpp_packed_batch *in, int action, size_t chunk,
                                   uint8_t *masks_out, uint8_t *mask_present, char *errbuf, size_t errbuf_len) {
  auto upload = [&](uint64_t *h) -> int { return bpp_batch_upload_packed_device(ctx, params, in, h, errbuf, errbuf_len); };
  return verify_uploaded(ctx, in ? in->n_items : SIZE_MAX, upload, action, chunk, masks_out, mask_present, errbuf, errbuf_len);
}

int bpp_verify_batch_mixed(bpp_ctx *ctx, uint64_t params, const bpp_mixed_batch *in, int action, size_t chunk, uint8_t *masks_out,
                           uint8_t *mask_present, char *errbuf, size_t errbuf_len) {
  auto upload = [&](uint64_t *h) -> int { return bpp_batch_upload_mixed(ctx, params, in, h, errbuf, errbuf_len); };
  return verify_uploaded(ctx, in ? in->n_items : SIZE_MAX, upload, action, chunk, masks_out, mask_present, errbuf, errbuf_len);
}

int bpp_verify_batch_mixed_device(bpp_ctx *ctx, uint64_t params, const bpp_mixed_batch *in, int action, size_t chunk,
                                  uint8_t *masks_out, uint8_t *mask_present, char *errbuf, size_t errbuf_len) {
  auto upload = [&](uint64_t *h) -> int { return bpp_batch_upload_mixed_device(ctx, params, in, h, errbuf, errbuf_len); };
  return verify_uploaded(ctx, in ? in->n_items : SIZE_MAX, upload, action, chunk, masks_out, mask_present, errbuf, errbuf_len);
}

// the same calls with the advanced transcripts handed back (bpp.h, "Advanced transcripts")
int bpp_verify_batch_states(bpp_ctx *ctx, uint64_t params, const bpp_verify_item *items, size_t n_items, int action, size_t chunk,
                            uint8_t *masks_out, uint8_t *mask_present, uint8_t *states_out203, char *errbuf, size_t errbuf_len) {
  if (!ctx) return BPP_ERR_BAD_HANDLE;
  if (!states_out203) {
    BPP_ENTRY(ctx);
    return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "null argument", errbuf, errbuf_len);
  }
  auto upload = [&](uint64_t *h) -> int { return bpp_batch_upload(ctx, params, items, n_items, h, errbuf, errbuf_len); };
  return verify_uploaded(ctx, n_items, upload, action, chunk, masks_out, mask_present, errbuf, errbuf_len, states_out203);
}

int bpp_verify_batch_packed_states(bpp_ctx *ctx, uint64_t params, const bpp_packed_batch *in, int action, size_t chunk,
                                   uint8_t *masks_out, uint8_t *mask_present, uint8_t *states_out203, char *errbuf, size_t errbuf_len) {
  if (!ctx) return BPP_ERR_BAD_HANDLE;
  if (!states_out203) {
    BPP_ENTRY(ctx);
    return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "null argument", errbuf, errbuf_len);
  }
  auto upload = [&](uint64_t *h) -> int { return bpp_batch_upload_packed(ctx, params, in, h, errbuf, errbuf_len); };
  return verify_uploaded(ctx, in ? in->n_items : SIZE_MAX, upload, action, chunk, masks_out, mask_present, errbuf, errbuf_len, states_out203);
}

}  // extern "C"

// ---------------------------------------------------------------- pipelined host-buffers-in form
// One context, `depth` lanes.  A lane is a private child context (own stream, page-locked staging, recycled work buffers)
// plus a worker thread (lanes::TicketLanes).  submit packs the caller's buffers into the next lane's staging ON THE CALLING
// THREAD -- the lanes of earlier tickets are busy with DMA, kernels and weight chains meanwhile -- and hands the plan to the
// lane's worker, which runs the device half of the upload, the verification and the release exactly as bpp_verify_batch_packed does.
namespace {

// ---- what the lanes of the two pipelines (this one, engine_prove_pipe.h) and of the two pools (engine_batcher.h,
// engine_prove_pool.h) are made of.  Lock order: ctx->mu is never taken while a pipeline's or a pool's mutex is held.
bpp_ctx::Options ctx_options(bpp_ctx *ctx) {
  std::lock_guard<std::mutex> lk(ctx->mu);
  return ctx->opt;
}

// n new contexts on `device`, each retaining `params` if given and then handed to `adopt`.  All or nothing: the ones already
// made are destroyed when one fails.
template <class Adopt>
int make_lane_contexts(int device, uint32_t n, const uint64_t *params, Adopt adopt, std::vector<bpp_ctx *> &out) {
  for (uint32_t i = 0; i < n; i++) {
    bpp_ctx *c = nullptr;
    int rc = bpp_ctx_create(&c, device);
    if (rc == BPP_OK && params) rc = bpp_params_retain(c, *params);
    if (rc != BPP_OK) {
      if (c) bpp_ctx_destroy(c);
      for (bpp_ctx *made : out) bpp_ctx_destroy(made);
      out.clear();
      return rc;
    }
    adopt(c);
    out.push_back(c);
  }
  return BPP_OK;
}

// the contexts of a pool's lanes: the caller's own first, then lanes - 1 that the pool owns
template <class Lane, class Adopt>
int make_pool_lanes(bpp_ctx *ctx, uint64_t params, uint32_t lanes, Adopt adopt, std::vector<Lane> &out) {
  const bpp_ctx::Options opt = ctx_options(ctx);
  std::vector<bpp_ctx *> own;
  const int rc = make_lane_contexts(ctx->device, lanes - 1, &params, [&](bpp_ctx *c) { adopt(c, opt); }, own);
  if (rc != BPP_OK) return rc;
  out.resize(lanes);
  out[0].ctx = ctx;
  for (uint32_t i = 1; i < lanes; i++) {
    out[i].ctx = own[i - 1];
    out[i].own = true;
  }
  return BPP_OK;
}

// a context's pipeline (`slot`, guarded by `init_mu`), made on the first submit: `depth` child contexts with the knobs of the
// caller's context as they are now (the tamper knobs stay behind), read BEFORE the pipeline's own lock is taken
template <class P, class Make>
std::shared_ptr<P> pipeline_get(bpp_ctx *ctx, std::mutex &init_mu, std::shared_ptr<P> &slot, const uint32_t &depth, const char *what, Make make) {
  {
    std::lock_guard<std::mutex> lk(init_mu);
    if (slot) return slot;
  }
  const bpp_ctx::Options opt = ctx_options(ctx);
  std::lock_guard<std::mutex> lk(init_mu);
  if (slot) return slot;  // (another thread's first submit was quicker)
  std::vector<bpp_ctx *> children;
  if (make_lane_contexts(ctx->device, depth, nullptr, [&](bpp_ctx *c) { c->opt = opt; }, children) != BPP_OK) throw EngineError{BPP_ERR_ENGINE, what};
  try {
    slot = make(children);
  } catch (...) {  // (an allocation, a worker thread that could not be started: the children go with it)
    for (bpp_ctx *c : children) bpp_ctx_destroy(c);
    throw;
  }
  return slot;
}

// every reader's reference: the pipeline outlives a context destroyed meanwhile
template <class P>
std::shared_ptr<P> pipeline_peek(std::mutex &init_mu, const std::shared_ptr<P> &slot) {
  std::lock_guard<std::mutex> lk(init_mu);
  return slot;
}

// waits for the calls in flight on the lanes, joins their threads, hands what nobody collected to `on_uncollected`, destroys the lanes
template <class P, class F>
void pipeline_end(std::mutex &init_mu, std::shared_ptr<P> &slot, F on_uncollected) {
  std::shared_ptr<P> pp;
  {
    std::lock_guard<std::mutex> lk(init_mu);
    pp = std::move(slot);
    slot.reset();
  }
  if (!pp) return;
  pp->shutdown(on_uncollected);
  pp->for_each_lane([](bpp_ctx *c) { bpp_ctx_destroy(c); });
}

void pipe_worker(bpp_ctx *owner, Pipeline *pp, PipeLane *lane) {
  (void)hipSetDevice(owner->device);
  for (;;) {
    std::shared_ptr<PipeJob> job;
    {
      std::unique_lock<std::mutex> lk(pp->mu);
      pp->cv.wait(lk, [&] { return pp->quit || lane->job; });
      if (!lane->job) return;  // quit with nothing posted
      job = std::move(lane->job);
      lane->job.reset();
    }
    bpp_ctx *c = lane->child;
    char err[256];
    err[0] = 0;
    uint64_t h = 0;
    int rc = BPP_OK;
    GateHold gate(device_state(owner->device), job->n_items <= BPP_GATE_SMALL_PROOFS);
    {
      std::lock_guard<std::mutex> lk(c->mu);
      try {
        h = upload_device(c, job->Pp, job->params, job->pl, nullptr, nullptr);
      } catch (const EngineError &e) {
        rc = fail(c, e.code, e.msg, err, sizeof(err));
      } catch (const ProofErr &e) {
        rc = fail(c, e.code, e.msg, err, sizeof(err));
      } catch (const std::exception &e) {
        rc = fail(c, BPP_ERR_ENGINE, e.what(), err, sizeof(err));
      }
    }
    if (rc == BPP_OK) {
      const bool want_masks = job->action != BPP_VERIFY_ONLY;
      if (want_masks) {
        job->masks.assign(job->n_items * job->t * 32, 0);
        job->present.assign(job->n_items, 0);
      }
      rc = bpp_verify_resident(c, h, job->action, job->chunk, want_masks ? job->masks.data() : nullptr,
                               want_masks ? job->present.data() : nullptr, err, sizeof(err));
      (void)bpp_batch_destroy(c, h);
    }
    {
      std::lock_guard<std::mutex> lk(pp->mu);
      job->rc = rc;
      job->err = err;
      job->done = true;
      lane->busy = false;
    }
    pp->cv.notify_all();
  }
}

std::shared_ptr<Pipeline> make_pipeline(bpp_ctx *owner, const std::vector<bpp_ctx *> &children) {
  auto pp = std::make_shared<Pipeline>();
  for (bpp_ctx *c : children) {
    pp->lanes.push_back(std::make_unique<PipeLane>());
    pp->lanes.back()->child = c;
  }
  try {
    for (auto &lane : pp->lanes) lane->th = std::thread(pipe_worker, owner, pp.get(), lane.get());
  } catch (...) {  // a thread that could not be started: the ones that were are ended, not abandoned while joinable
    {
      std::lock_guard<std::mutex> lk(pp->mu);
      pp->quit = true;
    }
    pp->cv.notify_all();
    for (auto &lane : pp->lanes)
      if (lane->th.joinable()) lane->th.join();
    throw;
  }
  return pp;
}

}  // namespace

void pipeline_shutdown(bpp_ctx *ctx) {
  std::shared_ptr<Pipeline> pp;
  {
    std::lock_guard<std::mutex> lk(ctx->pipe_init_mu);
    pp = std::move(ctx->pipe);
    ctx->pipe.reset();
  }
  if (!pp) return;
  {
    std::unique_lock<std::mutex> lk(pp->mu);
    pp->cv.wait(lk, [&] {  // calls in flight finish first (their results are simply dropped)
      for (auto &l : pp->lanes)
        if (l->busy) return false;
      return true;
    });
    pp->quit = true;
  }
  pp->cv.notify_all();
  for (auto &l : pp->lanes) {
    if (l->th.joinable()) l->th.join();
    bpp_ctx_destroy(l->child);
  }
  std::lock_guard<std::mutex> lk(pp->mu);
  for (auto &kv : pp->tickets) wipe(kv.second->masks.data(), kv.second->masks.size());
  pp->tickets.clear();
}

extern "C" {

int bpp_ctx_pipeline_depth(bpp_ctx *ctx, uint32_t depth) {
  if (!ctx) return BPP_ERR_BAD_HANDLE;
  std::lock_guard<std::mutex> lk(ctx->pipe_init_mu);
  if (ctx->pipe) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "the pipeline is already running");
  if (depth < 1 || depth > 16) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "pipeline depth must be 1..16");
  ctx->pipe_depth = depth;
  return BPP_OK;
}

int bpp_verify_submit_packed(bpp_ctx *ctx, uint64_t params, const bpp_packed_batch *in, int action, size_t chunk,
                             uint64_t *ticket, char *errbuf, size_t errbuf_len) {
  if (!ctx) return BPP_ERR_BAD_HANDLE;
  if (hipSetDevice(ctx->device) != hipSuccess) return BPP_ERR_NO_DEVICE;
  try {
    if (!in || !ticket || in->n_items == 0)
      return fail(nullptr, BPP_ERR_INVALID_ARGUMENT, "Range statements or proofs length empty", errbuf, errbuf_len);
    if (action < 0 || action > 2) return fail(nullptr, BPP_ERR_INVALID_ARGUMENT, "unknown verify action", errbuf, errbuf_len);
    if (in->n_items > (1u << 24)) return fail(nullptr, BPP_ERR_SIZE_OVERFLOW, "batch too large", errbuf, errbuf_len);
    const std::shared_ptr<Params> Pp = params_registry().get(params);
    if (!Pp || Pp->device != ctx->device) return fail(nullptr, BPP_ERR_BAD_HANDLE, "unknown params handle", errbuf, errbuf_len);
    const std::shared_ptr<Pipeline> pp = pipeline_get(ctx, ctx->pipe_init_mu, ctx->pipe, ctx->pipe_depth, "pipeline lane: context creation failed",
                                                      [&](const std::vector<bpp_ctx *> &children) { return make_pipeline(ctx, children); });
    std::lock_guard<std::mutex> submit_lock(pp->submit_mu);
    PipeLane *lane;
    {
      std::unique_lock<std::mutex> lk(pp->mu);
      lane = pp->lanes[pp->next_lane].get();
      pp->cv.wait(lk, [&] { return !lane->busy; });  // its previous call is done: staging and work buffers are free
      lane->busy = true;
      pp->next_lane = (pp->next_lane + 1) % (uint32_t)pp->lanes.size();
    }
    auto job = std::make_shared<PipeJob>();
    job->action = action;
    job->chunk = chunk;
    job->Pp = Pp;
    job->params = params;
    job->n_items = in->n_items;
    job->t = Pp->t;
    try {
      upload_host_pack(lane->child, *Pp, nullptr, 0, in, job->pl);  // into the lane's staging; throws construction errors
    } catch (...) {
      secure_wipe(job->pl.seeds.data(), job->pl.seeds.size());
      {
        std::lock_guard<std::mutex> lk(pp->mu);
        lane->busy = false;
      }
      pp->cv.notify_all();
      throw;
    }
    {
      std::lock_guard<std::mutex> lk(pp->mu);
      job->ticket = pp->next_ticket++;
      pp->tickets[job->ticket] = job;
      lane->job = job;
      *ticket = job->ticket;
    }
    pp->cv.notify_all();
    return BPP_OK;
  }
  BPP_CATCH(nullptr, errbuf, errbuf_len)
}

int bpp_verify_collect(bpp_ctx *ctx, uint64_t ticket, uint8_t *masks_out, uint8_t *mask_present, char *errbuf,
                       size_t errbuf_len) {
  if (!ctx) return BPP_ERR_BAD_HANDLE;
  const std::shared_ptr<Pipeline> pp = pipeline_peek(ctx->pipe_init_mu, ctx->pipe);
  if (!pp) return fail(nullptr, BPP_ERR_BAD_HANDLE, "unknown ticket", errbuf, errbuf_len);
  std::shared_ptr<PipeJob> job;
  {
    std::unique_lock<std::mutex> lk(pp->mu);
    auto it = pp->tickets.find(ticket);
    if (it == pp->tickets.end()) return fail(nullptr, BPP_ERR_BAD_HANDLE, "unknown ticket", errbuf, errbuf_len);
    job = it->second;
    pp->cv.wait(lk, [&] { return job->done; });  // (the lock is released in the wait: `it` is not used again)
    if (!pp->tickets.erase(ticket)) return fail(nullptr, BPP_ERR_BAD_HANDLE, "unknown ticket", errbuf, errbuf_len);  // (another thread was first)
  }
  ScopeExit wipe_masks{[&] { wipe(job->masks.data(), job->masks.size()); }};
  if (job->rc != BPP_OK) {
    set_err(errbuf, errbuf_len, job->err);
    return job->rc;
  }
  const size_t n = job->n_items, t = job->t;
  const bool have = job->action != BPP_VERIFY_ONLY;
  if (mask_present) {
    if (have) memcpy(mask_present, job->present.data(), n);
    else memset(mask_present, 0, n);
  }
  if (masks_out) {
    if (have) memcpy(masks_out, job->masks.data(), n * t * 32);
    else memset(masks_out, 0, n * t * 32);
  }
  return BPP_OK;
}

// ---------------------------------------------------------------- phased form
int bpp_verify_phase1(bpp_ctx *ctx, uint64_t batch, uint8_t *rng_out32, char *errbuf, size_t errbuf_len) {
  BPP_ENTRY(ctx);
  try {
    auto it = ctx->batches.find(batch);
    if (it == ctx->batches.end()) return fail(ctx, BPP_ERR_BAD_HANDLE, "unknown batch handle", errbuf, errbuf_len);
    Batch &b = *it->second;
    if (b.refilled) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, BPP_REFILLED_MSG, errbuf, errbuf_len);
    StageTimer tm(ctx);
    layout_groups(ctx, b, 0);
    if (b.any_defer) check_deferred(b.defer, 0, b.B);
    enqueue_phase1(ctx, b, tm, b.any_rounds_bad);
    fetch_status(ctx, b);
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (rng_out32) memcpy(rng_out32, b.h_rng.data(), (size_t)b.B * 32);
    check_chunk_errors(b, 0, b.B);
    b.phase1_done = true;
    return BPP_OK;
  }
  BPP_CATCH(ctx, errbuf, errbuf_len)
}

int bpp_verify_phase2(bpp_ctx *ctx, uint64_t batch, const uint8_t *weights32, uint8_t accumulator128[128], char *errbuf,
                      size_t errbuf_len) {
  BPP_ENTRY(ctx);
  try {
    auto it = ctx->batches.find(batch);
    if (it == ctx->batches.end()) return fail(ctx, BPP_ERR_BAD_HANDLE, "unknown batch handle", errbuf, errbuf_len);
    if (!weights32 || !accumulator128) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "null argument", errbuf, errbuf_len);
    Batch &b = *it->second;
    if (b.refilled) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, BPP_REFILLED_MSG, errbuf, errbuf_len);
    if (!b.phase1_done) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "bpp_verify_phase1 must succeed first", errbuf, errbuf_len);
    for (uint32_t p = 0; p < b.B; p++)
      if (!sc_is_canonical(weights32 + 32 * (size_t)p))
        return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "weight is not canonical", errbuf, errbuf_len);
    StageTimer tm(ctx);
    hipStream_t s = ctx->stream;
    layout_groups(ctx, b, 0);
    memcpy(b.h_weights.data(), weights32, (size_t)b.B * 32);
    enqueue_phase2(ctx, b, tm);
    if (!ctx->scratch128.p) ctx->scratch128.alloc(128);
    hipLaunchKernelGGL(k_ge_to_bytes, dim3(1), dim3(64), 0, s, b.msm.R.p, 1u, ctx->scratch128.p);
    HIP_CHECK(hipMemcpyAsync(accumulator128, ctx->scratch128.p, 128, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    b.have_trace = true;
    return BPP_OK;
  }
  BPP_CATCH(ctx, errbuf, errbuf_len)
}

int bpp_accumulators_sum_is_identity(bpp_ctx *ctx, const uint8_t *accumulators128, size_t n, int *is_identity) {
  BPP_ENTRY(ctx);
  try {
    if (!accumulators128 || !is_identity || n == 0) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "null argument");
    DevBuf<uint8_t> d_in, d_comp;
    DevBuf<uint32_t> d_flag;
    d_in.alloc(n * 128);
    d_comp.alloc(32);
    d_flag.alloc(1);
    HIP_CHECK(hipMemcpyAsync(d_in.p, accumulators128, n * 128, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_sum_accumulators, dim3(1), dim3(64), 0, ctx->stream, d_in.p, (uint32_t)n, d_comp.p, d_flag.p);
    uint32_t flag = 0;
    HIP_CHECK(hipMemcpyAsync(&flag, d_flag.p, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    *is_identity = flag ? 1 : 0;
    return BPP_OK;
  }
  BPP_CATCH(ctx, nullptr, 0)
}

// ---------------------------------------------------------------- trace / shape / profile
int bpp_batch_shape(bpp_ctx *ctx, uint64_t batch, uint32_t *n_items, uint32_t *max_rounds, uint32_t *max_mn,
                    uint32_t *total_dyn, uint32_t *groups) {
  BPP_ENTRY(ctx);
  auto it = ctx->batches.find(batch);
  if (it == ctx->batches.end()) return fail(ctx, BPP_ERR_BAD_HANDLE, "unknown batch handle");
  Batch &b = *it->second;
  if (n_items) *n_items = b.B;
  if (max_rounds) *max_rounds = b.cs - 3;  // rounds the challenge trace has slots for (capped at BPP_MAX_ROUNDS - 1)
  if (max_mn) *max_mn = b.max_mn;
  if (total_dyn) *total_dyn = b.total_dyn;
  if (groups) *groups = b.G;
  return BPP_OK;
}

int bpp_batch_trace(bpp_ctx *ctx, uint64_t batch, int what, uint8_t *out, size_t out_len, size_t *written) {
  BPP_ENTRY(ctx);
  try {
    auto it = ctx->batches.find(batch);
    if (it == ctx->batches.end()) return fail(ctx, BPP_ERR_BAD_HANDLE, "unknown batch handle");
    Batch &b = *it->second;
    if (b.refilled) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, BPP_REFILLED_MSG);
    hipStream_t s = ctx->stream;
    size_t need = 0;
    const void *src = nullptr;
    DevBuf<uint8_t> tmp;
    switch (what) {
      case BPP_TRACE_CHALLENGES: {
        const uint32_t n = b.B * b.cs;
        need = (size_t)n * 32;
        tmp.alloc(need);
        hipLaunchKernelGGL(k_chal_canonical, dim3(cdiv(n, 64)), dim3(64), 0, s, b.chal.p, n, tmp.p);
        src = tmp.p;
        break;
      }
      case BPP_TRACE_RNG_OUT:
        need = (size_t)b.B * 32;
        src = b.rng_out.p;
        break;
      case BPP_TRACE_WEIGHTS:
        need = (size_t)b.B * 32;
        if (b.weights_on_host) {  // PASS 2 read them from the mapped host buffer the chains wrote
          if (written) *written = need;
          if (!out || out_len < need) return fail(ctx, BPP_ERR_INVALID_LENGTH, "trace buffer too small");
          HIP_CHECK(hipStreamSynchronize(s));
          memcpy(out, b.h_weights.data(), need);
          return BPP_OK;
        }
        src = b.weights.p;
        break;
      case BPP_TRACE_STATIC_SCALARS:
        need = (size_t)b.G * b.cols * 32;
        src = b.scal.p;
        break;
      case BPP_TRACE_DYNAMIC_SCALARS:
        need = (size_t)b.total_dyn * 32;
        src = b.scal.p + (size_t)b.G * b.cols;
        break;
      case BPP_TRACE_JOINT_RESULT:  // the joint final check's point, of the last pass that took it
        if (!b.joint_ran) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "no verification pass of this batch has taken the joint final check");
        need = 32;
        hipLaunchKernelGGL(k_compress_ge, dim3(1), dim3(64), 0, s, b.msm_joint.R.p, 1u, b.msm_joint.comp32.p);
        src = b.msm_joint.comp32.p;
        break;
      case BPP_TRACE_MSM_RESULT:  // encoded on demand: verification itself only tests for the identity
        if (b.joint_accepted)
          return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "no per-group MSM results: the joint final check accepted and the per-group MSMs did not run");
        need = (size_t)b.G * 32;
        hipLaunchKernelGGL(k_compress_ge, dim3(cdiv(b.G, 64)), dim3(64), 0, s, b.msm.R.p, b.G, b.msm.comp32.p);
        src = b.msm.comp32.p;
        break;
      case BPP_TRACE_PLAN: {  // host-side: which form of the scalar stage the last layout / verification chose
        const uint32_t w[4] = {(b.fused_columns ? 1u : 0u) | (b.static_gemm ? 2u : 0u), b.lanes_ppw, b.gemm_nkc, b.G};
        if (written) *written = sizeof(w);
        if (!out || out_len < sizeof(w)) return fail(ctx, BPP_ERR_INVALID_LENGTH, "trace buffer too small");
        memcpy(out, w, sizeof(w));
        return BPP_OK;
      }
      default:
        return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "unknown trace selector");
    }
    if (written) *written = need;
    if (!out || out_len < need) return fail(ctx, BPP_ERR_INVALID_LENGTH, "trace buffer too small");
    HIP_CHECK(hipMemcpyAsync(out, src, need, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    return BPP_OK;
  }
  BPP_CATCH(ctx, nullptr, 0)
}

int bpp_batch_secret_bytes(bpp_ctx *ctx, uint64_t batch, uint64_t *nonzero) {
  BPP_ENTRY(ctx);
  try {
    if (!nonzero) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "null argument");
    Batch *b = nullptr;
    if (batch == 0) {
      b = ctx->spare_batch.get();
    } else {
      auto it = ctx->batches.find(batch);
      if (it == ctx->batches.end()) return fail(ctx, BPP_ERR_BAD_HANDLE, "unknown batch handle");
      b = it->second.get();
    }
    uint64_t cnt = 0;
    if (b) {
      HIP_CHECK(hipStreamSynchronize(ctx->stream));
      for (DevBuf<uint8_t> *buf : {&b->seeds, &b->masks}) {
        if (!buf->p || !buf->n) continue;
        std::vector<uint8_t> h(buf->n);
        HIP_CHECK(hipMemcpy(h.data(), buf->p, buf->n, hipMemcpyDeviceToHost));
        for (uint8_t v : h) cnt += v != 0;
        wipe(h.data(), h.size());
      }
    }
    *nonzero = cnt;
    return BPP_OK;
  }
  BPP_CATCH(ctx, nullptr, 0)
}

// the context's own buffers (its lock held); the lanes of its prove pipeline are looked at afterwards, without it
static int prove_secret_bytes_own(bpp_ctx *ctx, uint64_t *examined, uint64_t *nonzero) {
  BPP_ENTRY(ctx);
  try {
    if (!examined || !nonzero) return fail(ctx, BPP_ERR_INVALID_ARGUMENT, "null argument");
    uint64_t seen = 0, cnt = 0;
    if (ctx->prove_arena.p && ctx->prove_arena.n) {
      for (auto &ps : ctx->prove_streams) HIP_CHECK(hipStreamSynchronize(ps));
      std::vector<uint8_t> h(ctx->prove_arena.n);
      HIP_CHECK(hipMemcpy(h.data(), ctx->prove_arena.p, h.size(), hipMemcpyDeviceToHost));
      for (uint8_t v : h) cnt += v != 0;
      seen += h.size();
      wipe(h.data(), h.size());
    }
    // (the staging on the way out holds proofs and status words: nothing secret, not looked at)
    if (ctx->prove_pin_in.p && ctx->prove_pin_in.n) {
      for (size_t i = 0; i < ctx->prove_pin_in.n; i++) cnt += ctx->prove_pin_in.p[i] != 0;
      seen += ctx->prove_pin_in.n;
    }
    // the self-check's replay of mask recovery: its staging of blinding factors (page-locked and on the device) and the seed
    // nonces and recovered masks of its own verification batch, which waits in check_spare between calls
    if (ctx->check_pin.p && ctx->check_pin.n) {
      for (size_t i = 0; i < ctx->check_pin.n; i++) cnt += ctx->check_pin.p[i] != 0;
      seen += ctx->check_pin.n;
    }
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    std::vector<const DevBuf<uint8_t> *> dev{&ctx->check_dev};
    // the arenas of the resident prove plans: every stream of an enqueue is joined into the context's stream, waited for above
    for (auto &kv : ctx->prove_plans) dev.push_back(&kv.second->arena);
    if (ctx->check_spare && ctx->check_spare->seeds.p == ctx->check_zeroed_seeds) dev.push_back(&ctx->check_spare->seeds);
    if (ctx->check_spare && ctx->check_spare->masks.p == ctx->check_zeroed_masks) dev.push_back(&ctx->check_spare->masks);
    for (const DevBuf<uint8_t> *buf : dev) {
      if (!buf->p || !buf->n) continue;
      std::vector<uint8_t> h(buf->n);
      HIP_CHECK(hipMemcpy(h.data(), buf->p, buf->n, hipMemcpyDeviceToHost));
      for (uint8_t v : h) cnt += v != 0;
      seen += h.size();
      wipe(h.data(), h.size());
    }
    *examined = seen;
    *nonzero = cnt;
    return BPP_OK;
  }
  BPP_CATCH(ctx, nullptr, 0)
}

int bpp_prove_secret_bytes(bpp_ctx *ctx, uint64_t *examined, uint64_t *nonzero) {
  uint64_t seen = 0, cnt = 0;
  int rc = prove_secret_bytes_own(ctx, examined ? &seen : nullptr, nonzero ? &cnt : nullptr);
  if (rc != BPP_OK) return rc;
  // the prove pipeline's lanes, their arenas and staging: each under its own lock (a lane's running call is waited for), the
  // parent's released, so that nothing ever holds a context's lock while it asks for the pipeline's
  rc = prove_pipeline_secret_bytes(ctx, &seen, &cnt);
  if (rc != BPP_OK) return rc;
  *examined = seen;
  *nonzero = cnt;
  return BPP_OK;
}

int bpp_profile_enable(bpp_ctx *ctx, int on) {
  if (!ctx) return BPP_ERR_BAD_HANDLE;
  ctx->profile = on != 0;
  ctx->profile_light = on == 2;
  return BPP_OK;
}

int bpp_verify_check_resolve(const bpp_shard_result *passes, int n_passes, bpp_shard_result *out, int *kind) {
  if (!passes || !out || !kind || n_passes < 1 || n_passes > 3) return BPP_ERR_INVALID_ARGUMENT;
  ShardFinding f[3], o;
  for (int k = 0; k < n_passes; k++) {
    f[k].code = passes[k].code;
    f[k].tier = passes[k].tier;
    f[k].rank = passes[k].rank;
    f[k].index = passes[k].index;
    f[k].msg.assign(passes[k].msg, strnlen(passes[k].msg, sizeof(passes[k].msg)));
  }
  *kind = verify_check_resolve(f, n_passes, o);
  if (*kind == BPP_VCHECK_PENDING) return 1;
  memset(out, 0, sizeof(*out));
  shard_result_set(*out, o.code, o.tier, o.rank, o.index, o.msg);
  return 0;
}

int bpp_verify_check_stats(bpp_ctx *ctx, struct bpp_verify_check_stats *out) {
  if (!ctx || !out) return BPP_ERR_BAD_HANDLE;
  {
    std::lock_guard<std::mutex> lk(ctx->mu);
    *out = ctx->vcheck_stats;
  }
  // the packed pipeline's lanes: contexts of their own, made on the first submit
  if (const std::shared_ptr<Pipeline> pp = pipeline_peek(ctx->pipe_init_mu, ctx->pipe))
    for (auto &l : pp->lanes) {
      std::lock_guard<std::mutex> lk(l->child->mu);
      add_stats(*out, l->child->vcheck_stats);
    }
  return BPP_OK;
}

int bpp_verify_joint_stats(bpp_ctx *ctx, struct bpp_verify_joint_stats *out) {
  if (!ctx || !out) return BPP_ERR_BAD_HANDLE;
  {
    std::lock_guard<std::mutex> lk(ctx->mu);
    *out = ctx->vjoint_stats;
  }
  // the packed pipeline's lanes: contexts of their own, made on the first submit
  if (const std::shared_ptr<Pipeline> pp = pipeline_peek(ctx->pipe_init_mu, ctx->pipe))
    for (auto &l : pp->lanes) {
      std::lock_guard<std::mutex> lk(l->child->mu);
      add_stats(*out, l->child->vjoint_stats);
    }
  return BPP_OK;
}

int bpp_prove_check_stats(bpp_ctx *ctx, struct bpp_prove_check_stats *out) {
  if (!ctx || !out) return BPP_ERR_BAD_HANDLE;
  {
    std::lock_guard<std::mutex> lk(ctx->mu);
    *out = ctx->check_stats;
  }
  return prove_pipeline_check_stats(ctx, out);
}

int bpp_prove_check_recovery_stats(bpp_ctx *ctx, uint64_t *replayed, uint64_t *mismatched) {
  if (!ctx) return BPP_ERR_BAD_HANDLE;
  uint64_t r, m;
  {
    std::lock_guard<std::mutex> lk(ctx->mu);
    r = ctx->check_replayed;
    m = ctx->check_mismatched;
  }
  const int rc = prove_pipeline_recovery_stats(ctx, &r, &m);
  if (rc != BPP_OK) return rc;
  if (replayed) *replayed = r;
  if (mismatched) *mismatched = m;
  return BPP_OK;
}

int bpp_prove_profile_get(bpp_ctx *ctx, bpp_prove_profile *out) {
  if (!ctx || !out) return BPP_ERR_BAD_HANDLE;
  *out = ctx->pprof;
  return BPP_OK;
}

int bpp_profile_get(bpp_ctx *ctx, bpp_profile *out) {
  if (!ctx || !out) return BPP_ERR_BAD_HANDLE;
  *out = ctx->prof;
  return BPP_OK;
}

}  // extern "C"

#include "engine_shard.h"
#include "engine_batcher.h"

#include "engine_prove.h"
#include "engine_prove_plan.h"
#include "engine_prove_pool.h"
#include "engine_prove_pipe.h"
#include "engine_transcript_ops.h"
#include "engine_rows.h"
