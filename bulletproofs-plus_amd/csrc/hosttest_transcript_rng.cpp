// Sanitizer harness (CPU test suite only): the transcript-protocol and transcript-RNG kinds of transcript_ops.h -- the per-row rules
// and the host model of k_transcript_ops_rng (bpp_transcripts_enqueue) -- held to merlin.h's routines and top_scalar_from_wide, which
// are what the host helpers bpp_transcript_validate_and_append_point, _challenge_scalar and _rng_* call, applied to a copy of every
// row in program order.  The cases are those of tests/test_gpu_transcript_rng.py:
//   every_position   169 rows from Transcript::new(label of 0 .. 165, 166, 167, 400 bytes): RNG_BEGIN, RNG_REKEY("w", 32),
//                    RNG_FINALIZE(entropy), RNG_FILL 32, RNG_SCALARS 2, CHALLENGE_SCALAR("e"); the rows equal CHALLENGE_SCALAR alone
//   lengths          witnesses of 0, 1, 165, 166, 167, 400 bytes, uniform and through lens; FILL of 0, 1, 165, 166, 167, 256, 257, 600;
//                    FILL32 of 32 and 13 x 32; SCALARS of 1, 4, 5, 9; labels of 0 and 64 bytes
//   builder          NullRng, two REKEYs, transcript operations between FINALIZE and FILL, a second BEGIN, FILL32 against FILL, NEW first
//   points           eight rows, two identity encodings: void, counted, BPP_TOPS_IDENTITY; without them exactly BPP_TOPS_WRITTEN
//   void_and_dead    dead rows, zero rows, pos 166, lens = len + 1 on a REKEY, at every alignment of the rows; all_dead, all_void
//   zero_scalar      the model's void in the middle of a program (a hook replaces one draw by the encoding of l): the row and every
//                    output row zero, BPP_TOPS_ZERO_SCALAR -- for a CHALLENGE_SCALAR and for the 1st, 4th and 5th of RNG_SCALARS
//   geometry         rows and data at odd addresses with slack, n = 1, 63, 64, 65
//   refusals         transcript_ops_refusal: one per new rule, the field named, on addresses inside poisoned memory
// Every array ends with the last byte the call may touch.  Two passes: in the second every dead row's state, witness row, entropy
// row and length word, every void row's inputs (but the point rows of a row nothing else voids: that is how an identity is found)
// and all row slack are poisoned with ASAN_POISON_MEMORY_REGION.
// Built with  g++ -fsanitize=address,undefined  into an executable that tests/test_transcript_rng_host.py runs.  Prints one
// "ok <case>" line per case.
#include <stdio.h>
#include <stdlib.h>

#include <array>
#include <random>
#include <string>
#include <vector>

#include "transcript_ops.h"

#if defined(__SANITIZE_ADDRESS__)
#include <sanitizer/asan_interface.h>
#define POISON(p, n) ASAN_POISON_MEMORY_REGION(p, n)
#define UNPOISON(p, n) ASAN_UNPOISON_MEMORY_REGION(p, n)
#else
#define POISON(p, n) ((void)(p), (void)(n))
#define UNPOISON(p, n) ((void)(p), (void)(n))
#endif

using namespace bpp;

namespace {

std::mt19937_64 rng(20261021);
bool g_poison = false;
int g_failures = 0;

typedef std::array<uint8_t, 203> Row;

std::string label_of(size_t length) {  // tests/transcript_sweep.py: label_of
  std::string s(length, '\0');
  for (size_t i = 0; i < length; i++) s[i] = (char)((7 * i + length) & 0xff);
  return s;
}
Row row_new(const std::string &label) {
  Strobe s;
  merlin_new(s, (const uint8_t *)label.data(), (uint32_t)label.size());
  Row r;
  strobe_to_bytes(r.data(), s);
  return r;
}
Row row_at(uint32_t pos, uint32_t salt) {
  for (uint32_t len = 0; len < BPP_STROBE_R; len++) {
    Strobe s;
    const std::string label = "row " + std::to_string(salt);
    merlin_new(s, (const uint8_t *)label.data(), (uint32_t)label.size());
    std::vector<uint8_t> msg(len, (uint8_t)salt);
    merlin_append_message(s, (const uint8_t *)"pad", 3, msg.data(), len);
    if (s.pos == pos) {
      Row r;
      strobe_to_bytes(r.data(), s);
      return r;
    }
  }
  printf("FAIL no transcript at position %u\n", pos);
  exit(1);
}

struct Op {
  uint32_t kind;
  std::string label;
  uint32_t len;
  size_t stride;
  std::vector<uint32_t> lens;     // APPEND / RNG_REKEY: one per row, or empty
  std::vector<size_t> identity;   // APPEND_POINT: the rows whose point is 32 zero bytes
};
Op op_new(const std::string &label) { return Op{BPP_TOP_NEW, label, 0, 0, {}, {}}; }
Op op_read(uint32_t kind, const std::string &label, uint32_t len, size_t slack = 0, std::vector<uint32_t> lens = {}) {
  return Op{kind, label, len, len + slack, lens, {}};
}
Op op_append(const std::string &label, uint32_t len) { return op_read(BPP_TOP_APPEND, label, len); }
Op op_point(const std::string &label, std::vector<size_t> identity = {}, size_t slack = 0) {
  return Op{BPP_TOP_APPEND_POINT, label, 32, 32 + slack, {}, identity};
}
Op op_write(uint32_t kind, const std::string &label, uint32_t len, size_t slack = 0) { return Op{kind, label, len, len + slack, {}, {}}; }
Op op_challenge(const std::string &label, uint32_t len) { return op_write(BPP_TOP_CHALLENGE, label, len); }
Op op_cscalar(const std::string &label, size_t slack = 0) { return op_write(BPP_TOP_CHALLENGE_SCALAR, label, 32, slack); }
Op op_begin() { return Op{BPP_TOP_RNG_BEGIN, "", 0, 0, {}, {}}; }
Op op_rekey(const std::string &label, uint32_t len, size_t slack = 0, std::vector<uint32_t> lens = {}) {
  return op_read(BPP_TOP_RNG_REKEY, label, len, slack, lens);
}
Op op_finalize(bool entropy = true, size_t slack = 0) { return entropy ? op_read(BPP_TOP_RNG_FINALIZE, "", 32, slack) : Op{BPP_TOP_RNG_FINALIZE, "", 0, 0, {}, {}}; }
Op op_fill(uint32_t len, size_t slack = 0) { return op_write(BPP_TOP_RNG_FILL, "", len, slack); }
Op op_fill32(uint32_t len, size_t slack = 0) { return op_write(BPP_TOP_RNG_FILL32, "", len, slack); }
Op op_scalars(uint32_t count, size_t slack = 0) { return op_write(BPP_TOP_RNG_SCALARS, "", 32 * count, slack); }

bool reads(uint32_t k) { return k == BPP_TOP_APPEND || k == BPP_TOP_APPEND_POINT || k == BPP_TOP_RNG_REKEY || k == BPP_TOP_RNG_FINALIZE; }

// the encoding of l in 64 bytes: the one wide draw known to reduce to zero
void wide_l(uint8_t w[64]) {
  memset(w, 0, 64);
  for (int i = 0; i < 8; i++)
    for (int k = 0; k < 4; k++) w[4 * i + k] = (uint8_t)(sc_l(i) >> (8 * k));
}
size_t g_hook_row = (size_t)-1;
uint32_t g_hook_op = 0, g_hook_draw = 0;
void hook(uint8_t wide[64], size_t row, uint32_t op, uint32_t draw) {
  if (row == g_hook_row && op == g_hook_op && draw == g_hook_draw) wide_l(wide);
}

struct Case {
  std::vector<Row> rows;
  std::vector<uint8_t> live;  // empty: no mask
  std::vector<Op> ops;
  size_t state_off = 0, data_off = 0;
  bool zero_hook = false;     // g_hook_* name the draw that becomes l
};

// what the run left, for the cases that compare two programs
struct Result {
  std::vector<Row> states;
  std::vector<std::vector<std::vector<uint8_t>>> outs;  // [op][row]
  bpp_device_transcripts_record rec;
};

bool run(const char *name, const Case &c, Result *res = nullptr) {
  const size_t n = c.rows.size(), n_ops = c.ops.size();
  auto bad = [&](const char *what, size_t i, size_t j) {
    printf("FAIL %s: %s at row %zu, op %zu (n %zu, offsets %zu %zu, poison %d)\n", name, what, i, j, n, c.state_off, c.data_off, (int)g_poison);
    g_failures++;
    return false;
  };
  const bool fresh = c.ops[0].kind == BPP_TOP_NEW;
  const size_t sbytes = c.state_off + n * 203;
  uint8_t *sbuf = (uint8_t *)malloc(sbytes), *states = sbuf + c.state_off;
  memset(sbuf, 0xEE, sbytes);
  for (size_t i = 0; i < n; i++) memcpy(states + i * 203, c.rows[i].data(), 203);
  uint8_t *live = c.live.empty() ? nullptr : (uint8_t *)malloc(n);
  for (size_t i = 0; live && i < n; i++) live[i] = c.live[i] ? (uint8_t)(1 + rng() % 255) : 0;
  uint8_t *done = (uint8_t *)malloc(n);
  memset(done, 0xA5, n);
  bpp_device_transcripts_record *rec = (bpp_device_transcripts_record *)malloc(sizeof(bpp_device_transcripts_record));
  memset(rec, 0xA5, sizeof(*rec));
  std::vector<uint8_t *> dbuf(n_ops, nullptr);
  std::vector<uint32_t *> lens(n_ops, nullptr);
  std::vector<bpp_transcript_op> abi(n_ops);
  // ---- what every row is, by the contract's words: 0 dead, 1 void up front (state or a length), 3 void by an identity, 2 advanced
  std::vector<int> kind(n);
  for (size_t i = 0; i < n; i++) {
    const bool dead = !c.live.empty() && !c.live[i];
    bool is_void = !fresh && (c.rows[i][200] >= 166 || c.rows[i][202] == 0), identity = false;
    for (const Op &o : c.ops) {
      if ((o.kind == BPP_TOP_APPEND || o.kind == BPP_TOP_RNG_REKEY) && !o.lens.empty() && o.lens[i] > o.len) is_void = true;
      for (size_t r : o.identity) identity = identity || r == i;
    }
    kind[i] = dead ? 0 : is_void ? 1 : identity ? 3 : 2;
  }
  for (size_t j = 0; j < n_ops; j++) {
    const Op &o = c.ops[j];
    memset(&abi[j], 0, sizeof(abi[j]));
    abi[j].kind = o.kind;
    abi[j].label = o.label.empty() ? nullptr : (const uint8_t *)o.label.data();
    abi[j].label_len = (uint32_t)o.label.size();
    if (o.kind == BPP_TOP_NEW || o.kind == BPP_TOP_RNG_BEGIN) continue;
    abi[j].len = o.len, abi[j].stride = o.stride;
    if (o.len) {
      const size_t bytes = c.data_off + (n - 1) * o.stride + o.len;
      dbuf[j] = (uint8_t *)malloc(bytes);
      memset(dbuf[j], 0xEE, bytes);
      abi[j].data_dev = dbuf[j] + c.data_off;
      for (size_t i = 0; i < n; i++) {
        uint8_t *r = abi[j].data_dev + i * o.stride;
        const bool point_read = o.kind == BPP_TOP_APPEND_POINT && kind[i] == 3;
        if (!reads(o.kind) || (kind[i] != 2 && !point_read)) memset(r, 0xFF, o.len);  // (outputs; inputs that are never read)
        else
          for (uint32_t k = 0; k < o.len; k++) r[k] = (uint8_t)(1 + rng() % 255);
        for (size_t z : o.identity)
          if (z == i && kind[i] != 0 && kind[i] != 1) memset(r, 0, 32);
      }
    }
    if (!o.lens.empty()) {
      lens[j] = (uint32_t *)malloc(4 * n);
      for (size_t i = 0; i < n; i++) lens[j][i] = kind[i] == 0 ? 0xFFFFFFFFu : o.lens[i];
      abi[j].lens_dev = lens[j];
    }
  }
  // ---- the reference: merlin.h's routines and the scalar routine on a copy of every row, in program order
  std::vector<Row> want(n);
  std::vector<std::vector<std::vector<uint8_t>>> want_out(n_ops, std::vector<std::vector<uint8_t>>(n));
  bpp_device_transcripts_record want_rec{0, 0, 0xffffffffu, BPP_TOPS_WRITTEN};
  std::vector<uint8_t> want_done(n, 0);
  for (size_t i = 0; i < n; i++) {
    for (size_t j = 0; j < n_ops; j++)
      if (top_kind_writes(c.ops[j].kind)) want_out[j][i].assign(c.ops[j].len, 0);
    if (kind[i] == 0) {
      want[i] = c.rows[i];
      continue;
    }
    auto voided = [&](uint32_t flag) {
      want[i].fill(0);
      for (size_t j = 0; j < n_ops; j++) want_out[j][i].assign(want_out[j][i].size(), 0);
      want_rec.n_void++;
      want_rec.flags |= flag;
      if (i < want_rec.first_void) want_rec.first_void = (uint32_t)i;
    };
    if (kind[i] == 1 || kind[i] == 3) {
      voided(kind[i] == 3 ? BPP_TOPS_IDENTITY : 0u);
      continue;
    }
    Strobe s, g;
    if (fresh) merlin_new(s, abi[0].label, abi[0].label_len);
    else strobe_from_bytes(s, c.rows[i].data());
    g = s;
    bool zero = false;
    const uint8_t zeros[32] = {0};
    for (size_t j = fresh ? 1 : 0; j < n_ops && !zero; j++) {
      const Op &o = c.ops[j];
      uint8_t *r = abi[j].data_dev ? abi[j].data_dev + i * o.stride : nullptr;
      uint8_t *w = want_out[j][i].data();
      uint8_t wide[64];
      switch (o.kind) {
        case BPP_TOP_APPEND:
        case BPP_TOP_APPEND_POINT: merlin_append_message(s, abi[j].label, abi[j].label_len, r, o.lens.empty() ? o.len : o.lens[i]); break;
        case BPP_TOP_CHALLENGE: merlin_challenge_bytes(s, abi[j].label, abi[j].label_len, w, o.len); break;
        case BPP_TOP_CHALLENGE_SCALAR:
          merlin_challenge_bytes(s, abi[j].label, abi[j].label_len, wide, 64);
          if (c.zero_hook) hook(wide, i, (uint32_t)j, 0);
          zero = top_scalar_from_wide(w, wide) != 0;
          break;
        case BPP_TOP_RNG_BEGIN: g = s; break;
        case BPP_TOP_RNG_REKEY: merlin_rng_rekey(g, abi[j].label, abi[j].label_len, r, o.lens.empty() ? o.len : o.lens[i]); break;
        case BPP_TOP_RNG_FINALIZE: merlin_rng_finalize(g, r ? r : zeros); break;
        case BPP_TOP_RNG_FILL: merlin_rng_fill(g, w, o.len); break;
        case BPP_TOP_RNG_FILL32:
          for (uint32_t off = 0; off < o.len; off += 32) merlin_rng_fill(g, w + off, 32);
          break;
        default:
          for (uint32_t k = 0; k < o.len / 32 && !zero; k++) {
            merlin_rng_fill(g, wide, 64);
            if (c.zero_hook) hook(wide, i, (uint32_t)j, k);
            zero = top_scalar_from_wide(w + 32 * k, wide) != 0;
          }
      }
    }
    if (zero) {
      voided(BPP_TOPS_ZERO_SCALAR);
      continue;
    }
    want_rec.n_done++;
    want_done[i] = 1;
    strobe_to_bytes(want[i].data(), s);
  }
  // ---- what nothing may touch
  auto poison = [&](bool on) {
    auto mark = [&](void *p, size_t len) {
      if (!len) return;
      if (on) POISON(p, len);
      else UNPOISON(p, len);
    };
    if (c.state_off) mark(sbuf, c.state_off);
    for (size_t i = 0; i < n; i++)
      if (kind[i] == 0) mark(states + i * 203, 203);
    for (size_t j = 0; j < n_ops; j++) {
      const Op &o = c.ops[j];
      if (!dbuf[j]) continue;
      if (c.data_off) mark(dbuf[j], c.data_off);
      for (size_t i = 0; i < n; i++) {
        uint8_t *r = abi[j].data_dev + i * o.stride;
        const size_t row_end = i + 1 < n ? o.stride : o.len;
        const bool point_read = o.kind == BPP_TOP_APPEND_POINT && kind[i] == 3;
        const bool unread = reads(o.kind) && kind[i] != 2 && !point_read;
        if (unread) mark(r, row_end);
        else mark(r + o.len, row_end - o.len);
        if (reads(o.kind) && kind[i] == 2 && !o.lens.empty()) mark(r + o.lens[i], o.len - o.lens[i]);
      }
      if (lens[j])
        for (size_t i = 0; i < n; i++)
          if (kind[i] == 0) mark(lens[j] + i, 4);
    }
  };
  if (g_poison) poison(true);
  TranscriptOps a;
  transcript_ops_args(a, states, n, abi.data(), n_ops, live, done, rec);
  transcript_ops_run_host(a, c.zero_hook ? hook : nullptr);
  if (g_poison) poison(false);
  // ---- compare
  bool ok = true;
  if (!transcript_ops_extended(a)) ok = bad("the program does not run the extended model", 0, 0);
  for (size_t i = 0; i < n && ok; i++) {
    if (memcmp(states + i * 203, want[i].data(), 203) != 0) ok = bad(kind[i] == 0 ? "a dead row was written" : "state differs", i, 0);
    if (ok && done[i] != want_done[i]) ok = bad("done mask differs", i, 0);
  }
  for (size_t k = 0; k < c.state_off && ok; k++)
    if (sbuf[k] != 0xEE) ok = bad("a byte in front of the rows was written", 0, 0);
  for (size_t j = 0; j < n_ops && ok; j++) {
    const Op &o = c.ops[j];
    if (!dbuf[j]) continue;
    for (size_t k = 0; k < c.data_off && ok; k++)
      if (dbuf[j][k] != 0xEE) ok = bad("a byte in front of the data was written", 0, j);
    for (size_t i = 0; i < n && ok; i++) {
      const uint8_t *r = abi[j].data_dev + i * o.stride;
      if (top_kind_writes(o.kind) && memcmp(r, want_out[j][i].data(), o.len) != 0) ok = bad("output bytes differ", i, j);
      const size_t row_end = i + 1 < n ? o.stride : o.len;
      for (size_t k = o.len; k < row_end && ok; k++)
        if (r[k] != 0xEE) ok = bad("row slack was written", i, j);
    }
  }
  if (ok && memcmp(rec, &want_rec, sizeof(want_rec)) != 0) {
    printf("  want {%u %u %u %u} got {%u %u %u %u}\n", want_rec.n_done, want_rec.n_void, want_rec.first_void, want_rec.flags, rec->n_done, rec->n_void,
           rec->first_void, rec->flags);
    ok = bad("record differs", 0, 0);
  }
  if (res) {
    res->states.assign(n, Row());
    for (size_t i = 0; i < n; i++) memcpy(res->states[i].data(), states + i * 203, 203);
    res->outs = want_out;
    res->rec = *rec;
  }
  free(sbuf), free(live), free(done), free(rec);
  for (auto p : dbuf) free(p);
  for (auto p : lens) free(p);
  return ok;
}

void report(const std::string &name, bool ok) {
  if (ok && !g_poison) return;  // (one line per case, after its second pass)
  printf("%s %s\n", ok ? "ok" : "FAIL", name.c_str());
}
bool fail(const char *what) {
  printf("FAIL %s\n", what);
  g_failures++;
  return false;
}

const uint32_t EDGE_POS[4] = {0, 1, 164, 165};
const uint32_t EDGE_LEN[6] = {0, 1, 165, 166, 167, 400};

std::vector<Row> edge_rows() {
  std::vector<Row> rows;
  for (uint32_t k = 0; k < 12; k++) rows.push_back(row_at(EDGE_POS[k % 4], k));
  return rows;
}

void every_position() {
  Case c;
  for (size_t k = 0; k < 166; k++) c.rows.push_back(row_new(label_of(k)));
  for (size_t k : {(size_t)166, (size_t)167, (size_t)400}) c.rows.push_back(row_new(label_of(k)));
  c.ops = {op_begin(), op_rekey("w", 32), op_finalize(), op_fill(32), op_scalars(2), op_cscalar("e")};
  Result with, alone;
  bool ok = run("every_position", c, &with);
  c.ops = {op_cscalar("e")};
  ok = run("every_position", c, &alone) && ok;
  if (ok && (with.states != alone.states || with.outs[5] != alone.outs[0])) ok = fail("every_position: the RNG operations changed the rows");
  report("every_position", ok);
}

void lengths() {
  const std::string l64 = label_of(64);
  bool ok = true;
  for (uint32_t len : EDGE_LEN)
    for (const std::string &label : {std::string(), l64}) {
      Case c;
      c.rows = edge_rows();
      c.ops = {op_begin(), op_rekey(label, len), op_finalize(), op_fill(32)};
      ok = run("lengths", c) && ok;
    }
  for (uint32_t shift = 0; shift < 6; shift++) {
    Case c;
    c.rows = edge_rows();
    std::vector<uint32_t> lens;
    for (uint32_t k = 0; k < 12; k++) lens.push_back(EDGE_LEN[(k / 4 + k + shift) % 6]);
    c.ops = {op_begin(), op_rekey("w", 400, 7, lens), op_finalize(false), op_fill32(32)};
    ok = run("lengths", c) && ok;
  }
  for (uint32_t len : {0u, 1u, 165u, 166u, 167u, 256u, 257u, 600u}) {
    Case c;
    c.rows = edge_rows();
    c.ops = {op_begin(), op_rekey(l64, 32), op_finalize(), op_fill(len, 3), op_fill(7)};
    ok = run("lengths", c) && ok;
  }
  for (uint32_t len : {32u, 13u * 32u}) {
    Case c;
    c.rows = edge_rows();
    c.ops = {op_begin(), op_finalize(), op_fill32(len, 5), op_fill(5)};
    ok = run("lengths", c) && ok;
  }
  for (uint32_t count : {1u, 4u, 5u, 9u}) {
    Case c;
    c.rows = edge_rows();
    c.ops = {op_begin(), op_rekey("w", 32), op_finalize(false), op_scalars(count, 1), op_fill(9)};
    ok = run("lengths", c) && ok;
  }
  report("lengths", ok);
}

void builder() {
  bool ok = true;
  Result between, plain, f32, f64;
  {
    Case c;
    c.rows = edge_rows();
    c.ops = {op_begin(), op_rekey("w1", 32), op_rekey("w2", 48), op_finalize(false), op_fill(64)};
    ok = run("builder", c) && ok;
    c.ops = {op_begin(), op_rekey("w", 32), op_append("a", 48), op_begin(), op_finalize(), op_fill(64)};
    ok = run("builder", c) && ok;
    Row ff;
    ff.fill(0xFF);
    c.rows.assign(5, ff);
    c.ops = {op_new("fresh rows"), op_begin(), op_rekey("w", 32), op_finalize(), op_fill32(64), op_scalars(1)};
    ok = run("builder", c) && ok;
  }
  // the same data for the two programs of a pair: the generator is put back
  const auto pair = [&](std::vector<Op> x, Result *rx, std::vector<Op> y, Result *ry) {
    Case c;
    c.rows = edge_rows();
    const std::mt19937_64 saved = rng;
    c.ops = x;
    ok = run("builder", c, rx) && ok;
    rng = saved;
    c.ops = y;
    ok = run("builder", c, ry) && ok;
  };
  pair({op_begin(), op_rekey("w", 32), op_finalize(), op_fill(64), op_challenge("c", 32), op_append("a", 48)}, &plain,
       {op_begin(), op_rekey("w", 32), op_finalize(), op_fill(64)}, &f64);
  if (ok && plain.outs[3] != f64.outs[3]) ok = fail("builder: the pair's data differ");
  pair({op_begin(), op_rekey("w", 32), op_finalize(), op_challenge("c", 32), op_fill(64)}, &between,
       {op_begin(), op_rekey("w", 32), op_finalize(), op_fill(64)}, &plain);
  if (ok && (between.outs[4] != plain.outs[3] || between.states == plain.states)) ok = fail("builder: a transcript operation reached the RNG");
  pair({op_begin(), op_finalize(), op_fill32(64)}, &f32, {op_begin(), op_finalize(), op_fill(64)}, &f64);
  if (ok && f32.outs[2] == f64.outs[2]) ok = fail("builder: FILL32 of 64 equals FILL of 64");
  report("builder", ok);
}

void points() {
  bool ok = true;
  for (size_t off = 0; off < 4; off++) {
    Case c;
    c.data_off = off;
    for (uint32_t k = 0; k < 8; k++) c.rows.push_back(row_at((k * 41) % 166, k));
    c.ops = {op_point("P", {5, 2}, 1), op_append("ctx", 16), op_cscalar("e")};
    ok = run("points", c) && ok;
    c.ops[0] = op_point("P");
    Result r;
    ok = run("points", c, &r) && ok;
    if (ok && r.rec.flags != BPP_TOPS_WRITTEN) ok = fail("points: flags without an identity");
  }
  report("points", ok);
}

void void_and_dead() {
  bool ok = true;
  for (size_t off = 0; off < 8; off++) {
    Case c;
    c.state_off = off;
    Row zeros, p166 = row_at(0, 3), p255 = row_at(0, 5);
    zeros.fill(0);
    p166.fill(0xFF), p166[200] = 166, p166[202] = 2;
    p255.fill(0xFF), p255[200] = 255, p255[202] = 2;
    c.rows = {row_at(1, 1), row_at(0, 0), zeros, p166, row_at(164, 4), p255, row_at(165, 6), row_at(83, 7), row_at(2, 8)};
    c.live = {0, 1, 1, 1, 0, 1, 1, 1, 0};
    std::vector<uint32_t> lens(9, 24);
    lens[6] = 41;  // len + 1 on a valid row's REKEY
    c.ops = {op_begin(), op_rekey("w", 40, 5, lens), op_finalize(true, 3), op_fill32(64, 1), op_point("P", {2, 7}), op_scalars(5), op_cscalar("e", 2),
             op_fill(300)};
    ok = run("void_and_dead", c) && ok;
  }
  report("void_and_dead", ok);
  for (int all_void = 0; all_void < 2; all_void++) {
    Case c;
    Row zeros;
    zeros.fill(0);
    for (uint32_t k = 0; k < 5; k++) c.rows.push_back(all_void ? zeros : row_at(k, k));
    c.live.assign(5, all_void ? 1 : 0);
    c.ops = {op_begin(), op_rekey("w", 32), op_finalize(), op_fill(32), op_scalars(2)};
    report(all_void ? "all_void" : "all_dead", run(all_void ? "all_void" : "all_dead", c));
  }
}

void zero_scalar() {
  bool ok = true;
  struct Spot {
    uint32_t op, draw;
  };
  for (Spot s : {Spot{4, 0}, Spot{4, 3}, Spot{4, 4}, Spot{6, 0}}) {
    Case c;
    for (uint32_t k = 0; k < 6; k++) c.rows.push_back(row_at((k * 29) % 166, k));
    c.ops = {op_begin(), op_rekey("w", 32), op_finalize(), op_fill(40, 1), op_scalars(6, 1), op_challenge("c", 16), op_cscalar("e"), op_fill32(32)};
    c.zero_hook = true;
    g_hook_row = 3, g_hook_op = s.op, g_hook_draw = s.draw;
    Result r;
    ok = run("zero_scalar", c, &r) && ok;
    if (ok && (r.rec.flags != (BPP_TOPS_WRITTEN | BPP_TOPS_ZERO_SCALAR) || r.rec.n_void != 1 || r.rec.first_void != 3 || r.rec.n_done != 5))
      ok = fail("zero_scalar: the record");
  }
  uint8_t w[64], out[32];
  wide_l(w);
  if (!top_scalar_from_wide(out, w)) ok = fail("zero_scalar: l does not reduce to zero");
  report("zero_scalar", ok);
}

void geometry() {
  bool ok = true;
  for (size_t n : {(size_t)1, (size_t)63, (size_t)64, (size_t)65})
    for (size_t off : {(size_t)1, (size_t)3}) {
      Case c;
      c.state_off = off, c.data_off = 1;
      for (size_t k = 0; k < n; k++) c.rows.push_back(row_at((uint32_t)(k * 37 % 166), (uint32_t)k));
      c.ops = {op_begin(), op_rekey("w", 32, 1), op_finalize(true, 1), op_fill32(64, 1), op_scalars(1, 1), op_cscalar("e", 1)};
      ok = run("geometry", c) && ok;
    }
  report("geometry", ok);
}

// transcript_ops_refusal: the addresses lie in poisoned memory -- nothing is dereferenced but ops[] itself
void refusals() {
  bool ok = true;
  uint8_t *block = (uint8_t *)malloc(16384);
  if (g_poison) POISON(block, 16384);
  uint8_t *states = block, *wit = block + 1024, *ent = block + 2048, *out = block + 3072, *out2 = block + 4096, *live = block + 5120, *done = block + 5248;
  uint32_t *lens = (uint32_t *)(block + 5376);
  bpp_device_transcripts_record *rec = (bpp_device_transcripts_record *)(block + 5504);
  const uint8_t label[65] = {0};
  // BEGIN, REKEY(3, wit 40 with lens), FINALIZE(ent), FILL32(out, 64), SCALARS(out2, 64)
  auto base = [&] {
    std::vector<bpp_transcript_op> o(5);
    memset(o.data(), 0, 5 * sizeof(bpp_transcript_op));
    o[0].kind = BPP_TOP_RNG_BEGIN;
    o[1].kind = BPP_TOP_RNG_REKEY, o[1].label = label, o[1].label_len = 3, o[1].data_dev = wit, o[1].stride = 40, o[1].len = 40, o[1].lens_dev = lens;
    o[2].kind = BPP_TOP_RNG_FINALIZE, o[2].data_dev = ent, o[2].stride = 32, o[2].len = 32;
    o[3].kind = BPP_TOP_RNG_FILL32, o[3].data_dev = out, o[3].stride = 64, o[3].len = 64;
    o[4].kind = BPP_TOP_RNG_SCALARS, o[4].data_dev = out2, o[4].stride = 64, o[4].len = 64;
    return o;
  };
  auto call = [&](const std::vector<bpp_transcript_op> &o) { return transcript_ops_refusal(states, 4, o.data(), o.size(), live, done, rec); };
  auto expect = [&](const char *what, const char *needle, const std::vector<bpp_transcript_op> &o) {
    const std::string got = call(o);
    if (got.find(needle) == std::string::npos) {
      printf("FAIL refusals: %s: \"%s\" does not name %s\n", what, got.c_str(), needle);
      g_failures++;
      ok = false;
    }
  };
  auto accept = [&](const char *what, const std::vector<bpp_transcript_op> &o) {
    if (!call(o).empty()) {
      printf("FAIL refusals: %s is refused: %s\n", what, call(o).c_str());
      g_failures++;
      ok = false;
    }
  };
  auto point = [&](uint32_t kind) {
    bpp_transcript_op p{};
    p.kind = kind, p.label = label, p.label_len = 1, p.data_dev = out2, p.stride = 32, p.len = 32;
    return p;
  };
  accept("a good program", base());
  for (uint32_t k : {0u, 4u, 7u, 15u, 18u, 31u, 38u}) { auto o = base(); o[4].kind = k; expect("an unknown kind", "ops[4].kind", o); }
  { auto o = base(); o[4] = point(BPP_TOP_APPEND_POINT); accept("APPEND_POINT", o); o[4].len = 31; expect("APPEND_POINT len 31", "ops[4].len", o);
    o[4].len = 33, o[4].stride = 33; expect("APPEND_POINT len 33", "ops[4].len", o);
    o[4] = point(BPP_TOP_APPEND_POINT), o[4].lens_dev = lens + 8; expect("APPEND_POINT with lens", "ops[4].lens_dev", o); }
  { auto o = base(); o[4] = point(BPP_TOP_CHALLENGE_SCALAR); accept("CHALLENGE_SCALAR", o); o[4].len = 64, o[4].stride = 64;
    expect("CHALLENGE_SCALAR len 64", "ops[4].len", o); o[4].len = 0, o[4].data_dev = nullptr; expect("CHALLENGE_SCALAR len 0", "ops[4].len", o); }
  { auto o = base(); o[2].len = 16; expect("FINALIZE with 16 bytes", "ops[2].len", o); }
  { auto o = base(); o[2].len = 0; expect("FINALIZE with data and len 0", "ops[2].len", o); }
  { auto o = base(); o[2].data_dev = nullptr, o[2].len = 0, o[2].stride = 0; accept("FINALIZE without data (NullRng)", o); }
  { auto o = base(); o[3].len = 48; expect("FILL32 of 48", "ops[3].len", o); }
  { auto o = base(); o[4].len = 33, o[4].stride = 64; expect("SCALARS of 33 bytes", "ops[4].len", o); }
  { auto o = base(); o[3].kind = BPP_TOP_RNG_FILL, o[3].len = 48; accept("FILL of 48", o); }
  { auto o = base(); o[3].lens_dev = lens + 8; expect("lens on a FILL32", "ops[3].lens_dev", o); }
  { auto o = base(); o[2].lens_dev = lens + 8; expect("lens on a FINALIZE", "ops[2].lens_dev", o); }
  { auto o = base(); o[0].label = label, o[0].label_len = 1; expect("BEGIN with a label", "ops[0].label", o); }
  { auto o = base(); o[0].data_dev = out2 + 512, o[0].len = 8, o[0].stride = 8; expect("BEGIN with data", "ops[0].data_dev", o); }
  { auto o = base(); o[0] = point(BPP_TOP_APPEND_POINT), o[0].data_dev = wit + 512; expect("REKEY without a BEGIN", "ops[1].kind", o); }
  { auto o = base(); std::swap(o[1], o[2]); expect("REKEY behind the FINALIZE", "ops[2].kind", o); }
  { auto o = base(); o[3] = o[2], o[3].data_dev = ent + 512; expect("a second FINALIZE", "ops[3].kind", o); }
  { auto o = base(); o[2] = point(BPP_TOP_APPEND_POINT), o[2].data_dev = ent; expect("FILL32 without a FINALIZE", "ops[3].kind", o); }
  { auto o = base(); o[3].kind = BPP_TOP_RNG_BEGIN, o[3].data_dev = nullptr, o[3].len = 0, o[3].stride = 0;
    expect("SCALARS behind a second BEGIN", "ops[4].kind", o); }
  { auto o = base(); o[0] = o[3], o[0].kind = BPP_TOP_RNG_FILL; expect("FILL as op 0", "ops[0].kind", o); }
  { auto o = base(); o[1].label_len = 65; expect("a REKEY label over the maximum", "ops[1].label_len", o); }
  for (int j = 2; j < 5; j++) { auto o = base(); o[j].label = label, o[j].label_len = 1; expect("a label on FINALIZE / FILL32 / SCALARS", "label", o); }
  { auto o = base(); o[3].kind = BPP_TOP_RNG_FILL, o[3].label = label, o[3].label_len = 1; expect("a label on FILL", "ops[3].label", o); }
  // the overlap rule: inputs read, outputs written
  { auto o = base(); o[3].data_dev = states + 203; expect("FILL32 inside the states", "overlap", o); }
  { auto o = base(); o[4].data_dev = wit + 8; expect("SCALARS inside the witness rows", "overlap", o); }
  { auto o = base(); o[4].data_dev = ent + 8; expect("SCALARS inside the entropy rows", "overlap", o); }
  { auto o = base(); o[4].data_dev = out + 32; expect("SCALARS inside FILL32's rows", "overlap", o); }
  { auto o = base(); o[4] = point(BPP_TOP_CHALLENGE_SCALAR), o[4].data_dev = out + 250; expect("CHALLENGE_SCALAR inside FILL32's rows", "overlap", o); }
  { auto o = base(); o[4] = point(BPP_TOP_APPEND_POINT), o[4].data_dev = out; expect("APPEND_POINT reading FILL32's rows", "overlap", o); }
  { auto o = base(); o[2].data_dev = wit; accept("REKEY and FINALIZE reading the same rows", o); }
  { auto o = base(); o[4].data_dev = out + 3 * 64 + 64; accept("SCALARS right behind FILL32's rows", o); }
  if (g_poison) UNPOISON(block, 16384);
  free(block);
  report("refusals", ok);
}

}  // namespace

int main() {
  for (int pass = 0; pass < 2; pass++) {
    g_poison = pass == 1;
    rng.seed(20261021);
    every_position();
    lengths();
    builder();
    points();
    void_and_dead();
    zero_scalar();
    geometry();
    refusals();
  }
  if (g_failures) {
    printf("FAILED %d\n", g_failures);
    return 1;
  }
  printf("all ok\n");
  return 0;
}
