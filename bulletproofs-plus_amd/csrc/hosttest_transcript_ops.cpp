// Sanitizer harness (CPU test suite only): transcript_ops.h, the per-row rules and the host model of k_transcript_ops
// (bpp_transcripts_enqueue), held to merlin.h's routines -- merlin_new, merlin_append_message, merlin_challenge_bytes: what
// bpp_transcript_new, bpp_transcript_append_message and bpp_transcript_challenge_bytes call -- applied to a copy of every row in
// program order.  The cases are those of tests/test_gpu_transcript_ops.py:
//   every_position    169 rows from Transcript::new(label of 0 .. 165, 166, 167, 400 bytes): APPEND("ctx", 40), CHALLENGE("c", 32),
//                     APPEND("", 40), CHALLENGE("after", 64)
//   rate_uniform      starting positions {0, 1, 164, 165} x 3 rows; a uniform len of 0, 1, 165, 166, 167, 400; op labels of 0 and 64 bytes
//   rate_lens         the same lengths per row through lens under cap 400
//   rate_challenges   challenges of 1, 32, 64, 200 bytes (and 300 and 700: more than one piece of the kernel's LDS buffer)
//   new               five rows of 0xFF; NEW with labels of 0, 17, 165, 166, 400 bytes, then APPEND and CHALLENGE
//   void_and_dead     nine rows: valid, dead, zeros, pos 166, dead, pos 255, valid with lens = len + 1, valid, dead -- at every alignment
//                     of the rows modulo 8 -- and all_dead, all_void
//   geometry          rows at byte offsets 1 and 3 of their allocation, data with stride 33 at an odd address, n = 1, 63, 64, 65
//   refusals          transcript_ops_refusal: one per rule, the field named, on addresses inside poisoned memory
// Every array ends with the last byte the call may touch.  Two passes: in the first the rows nothing may read hold bytes that are
// merely different (0xFF data, valid states); in the second every dead row's state, data and lens word, every void row's data and every
// row's slack are poisoned with ASAN_POISON_MEMORY_REGION, so that reading (or writing) one is an ASan report.  The slack and the dead
// state rows are compared byte for byte afterwards.
// Built with  g++ -fsanitize=address,undefined  into an executable that tests/test_transcript_ops_host.py runs.  Prints one
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
// a transcript whose sponge stands at `pos`: a label of its own and one message of the length that puts it there
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
  std::vector<uint32_t> lens;  // APPEND: one per row, or empty
};
Op op_new(const std::string &label) { return Op{BPP_TOP_NEW, label, 0, 0, {}}; }
Op op_append(const std::string &label, uint32_t len, size_t slack = 0, std::vector<uint32_t> lens = {}) {
  return Op{BPP_TOP_APPEND, label, len, len + slack, lens};
}
Op op_challenge(const std::string &label, uint32_t len, size_t slack = 0) { return Op{BPP_TOP_CHALLENGE, label, len, len + slack, {}}; }

struct Case {
  std::vector<Row> rows;
  std::vector<uint8_t> live;  // empty: no mask
  std::vector<Op> ops;
  size_t state_off = 0, data_off = 0;  // where the arrays begin inside their allocations
};

bool run(const char *name, const Case &c) {
  const size_t n = c.rows.size(), n_ops = c.ops.size();
  auto bad = [&](const char *what, size_t i, size_t j) {
    printf("FAIL %s: %s at row %zu, op %zu (n %zu, offsets %zu %zu, poison %d)\n", name, what, i, j, n, c.state_off, c.data_off, (int)g_poison);
    g_failures++;
    return false;
  };
  const bool fresh = c.ops[0].kind == BPP_TOP_NEW;
  // ---- the arrays
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
  std::vector<size_t> dbytes(n_ops, 0);
  std::vector<uint32_t *> lens(n_ops, nullptr);
  std::vector<bpp_transcript_op> abi(n_ops);
  // ---- what every row is, by the contract's words
  std::vector<int> kind(n);  // 0 dead, 1 void, 2 advanced
  for (size_t i = 0; i < n; i++) {
    const bool dead = !c.live.empty() && !c.live[i];
    bool is_void = !fresh && (c.rows[i][200] >= 166 || c.rows[i][202] == 0);
    for (const Op &o : c.ops)
      if (o.kind == BPP_TOP_APPEND && !o.lens.empty() && o.lens[i] > o.len) is_void = true;
    kind[i] = dead ? 0 : is_void ? 1 : 2;
  }
  for (size_t j = 0; j < n_ops; j++) {
    const Op &o = c.ops[j];
    memset(&abi[j], 0, sizeof(abi[j]));
    abi[j].kind = o.kind;
    abi[j].label = o.label.empty() ? nullptr : (const uint8_t *)o.label.data();
    abi[j].label_len = (uint32_t)o.label.size();
    if (o.kind == BPP_TOP_NEW) continue;
    abi[j].len = o.len, abi[j].stride = o.stride;
    if (o.len) {
      dbytes[j] = c.data_off + (n - 1) * o.stride + o.len;
      dbuf[j] = (uint8_t *)malloc(dbytes[j]);
      memset(dbuf[j], 0xEE, dbytes[j]);
      abi[j].data_dev = dbuf[j] + c.data_off;
      for (size_t i = 0; i < n; i++) {
        uint8_t *r = abi[j].data_dev + i * o.stride;
        if (o.kind == BPP_TOP_CHALLENGE) memset(r, 0xFF, o.len);
        else if (kind[i] != 2) memset(r, 0xFF, o.len);  // (never read)
        else
          for (uint32_t k = 0; k < o.len; k++) r[k] = (uint8_t)rng();
      }
    }
    if (!o.lens.empty()) {
      lens[j] = (uint32_t *)malloc(4 * n);
      for (size_t i = 0; i < n; i++) lens[j][i] = kind[i] == 0 ? 0xFFFFFFFFu : o.lens[i];  // (a dead row's word: void if it were read)
      abi[j].lens_dev = lens[j];
    }
  }
  // ---- the reference: merlin.h's routines on a copy of every row, in program order
  std::vector<Row> want(n);
  std::vector<std::vector<std::vector<uint8_t>>> want_out(n_ops, std::vector<std::vector<uint8_t>>(n));
  bpp_device_transcripts_record want_rec{0, 0, 0xffffffffu, BPP_TOPS_WRITTEN};
  for (size_t i = 0; i < n; i++) {
    for (size_t j = 0; j < n_ops; j++)
      if (c.ops[j].kind == BPP_TOP_CHALLENGE) want_out[j][i].assign(c.ops[j].len, 0);
    if (kind[i] == 0) {
      want[i] = c.rows[i];
      continue;
    }
    if (kind[i] == 1) {
      want[i].fill(0);
      want_rec.n_void++;
      if (i < want_rec.first_void) want_rec.first_void = (uint32_t)i;
      continue;
    }
    want_rec.n_done++;
    Strobe s;
    if (fresh) merlin_new(s, abi[0].label, abi[0].label_len);
    else strobe_from_bytes(s, c.rows[i].data());
    for (size_t j = fresh ? 1 : 0; j < n_ops; j++) {
      const Op &o = c.ops[j];
      uint8_t *r = abi[j].data_dev ? abi[j].data_dev + i * o.stride : nullptr;
      if (o.kind == BPP_TOP_APPEND) merlin_append_message(s, abi[j].label, abi[j].label_len, r, o.lens.empty() ? o.len : o.lens[i]);
      else merlin_challenge_bytes(s, abi[j].label, abi[j].label_len, want_out[j][i].data(), o.len);
    }
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
        const size_t row_end = i + 1 < n ? o.stride : o.len;  // (the array ends with the last row's last byte)
        const bool unread = o.kind == BPP_TOP_APPEND && kind[i] != 2;
        if (unread) mark(r, row_end);
        else mark(r + o.len, row_end - o.len);
        if (o.kind == BPP_TOP_APPEND && kind[i] == 2 && !o.lens.empty()) mark(r + o.lens[i], o.len - o.lens[i]);  // (behind the row's own length)
      }
      if (lens[j])
        for (size_t i = 0; i < n; i++)
          if (kind[i] == 0) mark(lens[j] + i, 4);
    }
  };
  if (g_poison) poison(true);
  TranscriptOps a;
  transcript_ops_args(a, states, n, abi.data(), n_ops, live, done, rec);
  transcript_ops_run_host(a);
  if (g_poison) poison(false);
  // ---- compare
  bool ok = true;
  for (size_t i = 0; i < n && ok; i++) {
    if (memcmp(states + i * 203, want[i].data(), 203) != 0) ok = bad(kind[i] == 0 ? "a dead row was written" : "state differs", i, 0);
    if (ok && done[i] != (kind[i] == 2 ? 1 : 0)) ok = bad("done mask differs", i, 0);
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
      if (o.kind == BPP_TOP_CHALLENGE && memcmp(r, want_out[j][i].data(), o.len) != 0) ok = bad("challenge bytes differ", i, j);
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
  free(sbuf), free(live), free(done), free(rec);
  for (auto p : dbuf) free(p);
  for (auto p : lens) free(p);
  return ok;
}

void report(const std::string &name, bool ok) {
  if (ok && !g_poison) return;  // (one line per case, after its second pass)
  printf("%s %s\n", ok ? "ok" : "FAIL", name.c_str());
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
  std::vector<bool> seen(166, false);
  for (const Row &r : c.rows) seen[r[200]] = true;
  bool ok = true;
  for (bool s : seen) ok = ok && s;
  if (!ok) printf("FAIL every_position: not every starting position is there\n"), g_failures++;
  c.ops = {op_append("ctx", 40), op_challenge("c", 32), op_append("", 40), op_challenge("after", 64)};
  report("every_position", run("every_position", c) && ok);
}

void rate() {
  const std::string l64 = label_of(64);
  bool ok = true;
  for (uint32_t len : EDGE_LEN)
    for (const std::string &label : {std::string(), l64}) {
      Case c;
      c.rows = edge_rows();
      c.ops = {op_append(label, len), op_challenge(label, 32)};
      ok = run("rate_uniform", c) && ok;
    }
  report("rate_uniform", ok);
  ok = true;
  for (uint32_t shift = 0; shift < 6; shift++) {
    Case c;
    c.rows = edge_rows();
    std::vector<uint32_t> lens;
    for (uint32_t k = 0; k < 12; k++) lens.push_back(EDGE_LEN[(k / 4 + k + shift) % 6]);
    c.ops = {op_append("ctx", 400, 0, lens), op_challenge(l64, 32), op_append(l64, 400, 7, lens)};
    ok = run("rate_lens", c) && ok;
  }
  report("rate_lens", ok);
  ok = true;
  for (uint32_t len : {1u, 32u, 64u, 200u, 300u, 700u})
    for (const std::string &label : {std::string(), l64}) {
      Case c;
      c.rows = edge_rows();
      c.ops = {op_challenge(label, len), op_append("x", 1), op_challenge(label, len, 3)};
      ok = run("rate_challenges", c) && ok;
    }
  report("rate_challenges", ok);
}

void fresh() {
  bool ok = true;
  for (size_t length : {(size_t)0, (size_t)17, (size_t)165, (size_t)166, (size_t)400}) {
    Case c;
    Row ff;
    ff.fill(0xFF);
    c.rows.assign(5, ff);
    c.ops = {op_new(label_of(length)), op_append("txid", 32), op_challenge("c", 32)};
    ok = run("new", c) && ok;
  }
  report("new", ok);
}

void void_and_dead() {
  bool ok = true;
  for (size_t off = 0; off < 8; off++) {
    Case c;
    c.state_off = off;
    Row zeros, p166 = row_at(0, 3), p255 = row_at(0, 5);
    zeros.fill(0);
    p166.fill(0xFF), p166[200] = 166, p166[202] = 2;  // (nothing of a void row but bytes 200 and 202 matters)
    p255.fill(0xFF), p255[200] = 255, p255[202] = 2;
    c.rows = {row_at(0, 0), row_at(1, 1), zeros, p166, row_at(164, 4), p255, row_at(165, 6), row_at(83, 7), row_at(2, 8)};
    c.live = {1, 0, 1, 1, 0, 1, 1, 1, 0};
    std::swap(c.rows[0], c.rows[1]), std::swap(c.live[0], c.live[1]);  // dead: first, middle, last
    std::vector<uint32_t> lens(9, 24);
    lens[6] = 41;  // len + 1 on a valid row
    c.ops = {op_append("ctx", 40, 5, lens), op_challenge("c", 32, 1), op_append("tail", 8)};
    ok = run("void_and_dead", c) && ok;
  }
  report("void_and_dead", ok);
  {
    Case c;
    for (uint32_t k = 0; k < 5; k++) c.rows.push_back(row_at(k, k));
    c.live.assign(5, 0);
    c.ops = {op_append("ctx", 40), op_challenge("c", 32)};
    report("all_dead", run("all_dead", c));
  }
  {
    Case c;
    Row zeros;
    zeros.fill(0);
    c.rows.assign(5, zeros);
    c.live.assign(5, 1);
    c.ops = {op_append("ctx", 40), op_challenge("c", 32)};
    report("all_void", run("all_void", c));
  }
}

void geometry() {
  bool ok = true;
  for (size_t n : {(size_t)1, (size_t)63, (size_t)64, (size_t)65})
    for (size_t off : {(size_t)1, (size_t)3}) {
      Case c;
      c.state_off = off, c.data_off = 1;
      for (size_t k = 0; k < n; k++) c.rows.push_back(row_at((uint32_t)(k * 37 % 166), (uint32_t)k));
      c.ops = {op_append("txid", 32, 1), op_challenge("c", 32, 1)};
      ok = run("geometry", c) && ok;
    }
  report("geometry", ok);
}

// transcript_ops_refusal: the addresses lie in poisoned memory -- nothing is dereferenced but ops[] itself
void refusals() {
  bool ok = true;
  const size_t n = 4;
  uint8_t *block = (uint8_t *)malloc(8192);
  if (g_poison) POISON(block, 8192);
  uint8_t *states = block, *data = block + 1024, *out = block + 2048, *live = block + 3072, *done = block + 3200;
  uint32_t *lens = (uint32_t *)(block + 3328);
  bpp_device_transcripts_record *rec = (bpp_device_transcripts_record *)(block + 3456);
  const uint8_t label[65] = {0};
  auto base = [&] {
    std::vector<bpp_transcript_op> ops(2);
    memset(ops.data(), 0, 2 * sizeof(bpp_transcript_op));
    ops[0].kind = BPP_TOP_APPEND, ops[0].label = label, ops[0].label_len = 3, ops[0].data_dev = data, ops[0].stride = 40, ops[0].len = 40, ops[0].lens_dev = lens;
    ops[1].kind = BPP_TOP_CHALLENGE, ops[1].label = label, ops[1].label_len = 1, ops[1].data_dev = out, ops[1].stride = 32, ops[1].len = 32;
    return ops;
  };
  auto expect = [&](const char *what, const char *needle, const std::string &got) {
    if (got.find(needle) == std::string::npos) {
      printf("FAIL refusals: %s: \"%s\" does not name %s\n", what, got.c_str(), needle);
      g_failures++;
      ok = false;
    }
  };
  auto call = [&](const std::vector<bpp_transcript_op> &ops, size_t nn = 4, size_t n_ops = 2, uint8_t *st = nullptr, uint8_t *dn = nullptr,
                  bpp_device_transcripts_record *rc = nullptr) {
    return transcript_ops_refusal(st ? st : states, nn, ops.data(), n_ops, live, dn ? dn : done, rc ? rc : rec);
  };
  (void)n;
  if (!call(base()).empty()) expect("a good call", "nothing", call(base()));
  expect("n == 0", "n is 0", call(base(), 0));
  expect("n_ops == 0", "n_ops", call(base(), 4, 0));
  expect("n_ops above the maximum", "n_ops", call(base(), 4, BPP_TOP_MAX_OPS + 1));
  { auto o = base(); o[1].kind = 7; expect("an unknown kind", "kind", call(o)); }
  { auto o = base(); o[1] = bpp_transcript_op{}; o[1].kind = BPP_TOP_NEW; expect("NEW behind op 0", "NEW", call(o)); }
  { auto o = base(); o[0] = bpp_transcript_op{}; o[0].kind = BPP_TOP_NEW; o[0].data_dev = data; expect("NEW with data", "NEW takes no data", call(o)); }
  { auto o = base(); o[0] = bpp_transcript_op{}; o[0].kind = BPP_TOP_NEW; o[0].label = label; o[0].label_len = 400;
    if (!call(o).empty()) expect("NEW with a long label", "nothing", call(o)); }
  { auto o = base(); o[0].label_len = 65; expect("a label over the maximum", "label_len", call(o)); }
  { auto o = base(); o[1].len = 65537, o[1].stride = 65537; expect("len over the maximum", "len", call(o)); }
  { auto o = base(); o[1].stride = 31; expect("stride < len", "stride", call(o)); }
  { auto o = base(); o[0].data_dev = nullptr; expect("data_dev NULL with len > 0", "data_dev", call(o)); }
  { auto o = base(); o[0].data_dev = nullptr, o[0].len = 0, o[0].stride = 0, o[0].lens_dev = nullptr;
    if (!call(o).empty()) expect("data_dev NULL with len 0", "nothing", call(o)); }
  { auto o = base(); o[1].lens_dev = lens; expect("lens_dev on a CHALLENGE", "lens_dev", call(o)); }
  { auto o = base(); o[1].data_dev = states + 203 * 3; expect("a challenge inside the states", "overlap", call(o)); }
  { auto o = base(); o[1].data_dev = data + 8; expect("a challenge inside an append's rows", "overlap", call(o)); }
  expect("done_mask inside the states", "overlap", call(base(), 4, 2, nullptr, states + 100));
  expect("the record inside the mask", "overlap", call(base(), 4, 2, nullptr, nullptr, (bpp_device_transcripts_record *)(void *)done));
  { auto o = base(); o[1].kind = BPP_TOP_APPEND, o[1].data_dev = data;  // two reads of the same rows are no overlap
    if (!call(o).empty()) expect("two appends of the same rows", "nothing", call(o)); }
  { auto o = base(); o[1].data_dev = states + 203 * 4;  // end to end is no overlap
    if (!call(o).empty()) expect("a challenge right behind the states", "nothing", call(o)); }
  if (g_poison) UNPOISON(block, 8192);
  free(block);
  report("refusals", ok);
}

}  // namespace

int main() {
  for (int pass = 0; pass < 2; pass++) {
    g_poison = pass == 1;
    rng.seed(20261021);
    every_position();
    rate();
    fresh();
    void_and_dead();
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
