// Constant-time sums and scalar arithmetic over device rows (bpp_rows_msm_enqueue, bpp_rows_scalar_enqueue; include/bpp.h, "B1 on the
// stream"): what consumes the rows bpp_transcripts_enqueue makes -- the commitment to a nonce RNG_SCALARS drew, the response to a
// challenge CHALLENGE_SCALAR left -- without a host hop.  The conventions are transcript_ops.h's: rows at any byte address, a live
// mask, void rows, one 16-byte record reduced on the stream, no slack read or written.
//
// THE SUM, out[i] = sum_{k < K} s[i][k] P[i][k], K <= 16.  k_ct_straus (ct.h) gives a whole 64-lane workgroup to ONE output: at the
// commitment shape (two terms) 14 of its 16 quads walk the neutral element.  k_rows_msm packs rows instead: with Kp = K rounded up to
// a power of two, a workgroup serves 16 / Kp rows, quad `quad` of the workgroup the term quad % Kp of row quad / Kp -- ONE term per
// quad on the K = 1 table layout of CtStrausShared (tab[entry][limb][lane], the lane fastest: no bank conflict), the 63 x 4 doublings
// and 64 additions of ct_straus_coord's selected entries on the quad forms of msm.h.  Quads beyond K (padding), quads of dead rows
// and quads of rows beyond n run the same instruction stream on the neutral element and the scalar zero.  A segmented tree of
// log2(Kp) levels then adds the quads of a row, the row's first lane compresses the sum (ristretto_compress) and stores the 32
// bytes byte-wise.  Quad occupancy is K / Kp: 1 for K in {1, 2, 4, 8, 16}, at worst 9 / 16 (K = 9).
//
// PER ROW:
//   DEAD  live[i] == 0: one byte of the mask is read, nothing of the row's scalars or points; the output row is zeroed, done_mask 0.
//   VOID  a live row with a scalar >= l (BPP_ROWS_SCALAR) or a point that does not decode (BPP_ROWS_POINT): every one of its K terms
//         is looked at, the flags are ORed, ONE decision follows; 32 zero bytes, done_mask 0, n_void, first_void, the flags.
//   else  the canonical encoding of the sum, done_mask 1, n_done.
// The points are PUBLIC and decoded ahead of the sum: k_rows_decode (per-row points: one lane per term of a live row, into a buffer
// of the context, in slabs of BPP_ROWS_SLAB rows) or k_rows_bases (shared bases: one quad per base makes the carried multiples
// 1 P .. 8 P once per call; k_rows_msm copies them into its LDS table).  An undecodable point becomes the neutral element and a flag.
// SECRETS: the scalars.  They are read byte-wise into registers by the first lane of their quad, recoded (ct_recode16) into LDS
// digits, and reach nothing else: no branch, address, loop bound or launch geometry is made of them.  What IS decided from them is
// the row's canonicity -- public by contract (which rows are void) -- after the whole walk, as a mask on the output bytes.  Nothing
// secret-derived goes to global memory but the output row; the LDS object is wiped before the workgroup ends.
//
// THE SCALAR OPERATION, out[i] = a[i] b[i] + c[i] mod l: one lane per row on scalar.h (sc_to_mont, sc_montmul, sc_add: select-based
// conditional subtractions), every operand treated as a secret; a non-canonical operand voids the row under the same rules.
//
// The per-row rules are BPP_HD and shared by the kernels, the engine's refusals and the host models (rows_msm_run_host,
// rows_scalar_run_host), which hosttest_rows_msm.cpp holds to ct_straus_model / ct_scalarmul and to big-integer arithmetic.
#pragma once
#include <stddef.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/bpp.h"
#include "ct.h"
#include "ingest.h"

namespace bpp {

#define BPP_ROWS_SLAB 65536u  // rows whose decoded points the context's buffer holds at a time (K = 16: 128 MB)

// the launch arguments of one slab of a sum: rows [row0, row0 + rows) of the call's n
struct RowsMsm {
  const uint8_t *scalars;
  uint64_t scalar_stride;
  const uint8_t *points;
  uint64_t point_stride;  // 0: shared bases
  uint8_t *out;
  uint64_t out_stride;
  const uint8_t *live;
  uint8_t *done_mask;
  bpp_device_rows_record *record;
  niels *pts;          // per-row points: [rows][K] decoded (k_rows_decode), the neutral element where bad
  uint32_t *bad;       // per-row points: [rows][K], shared bases: [K] -- 1 where the point did not decode
  uint32_t *base_tab;  // shared bases: [K][8 entries][10 limbs][4 coordinates], carried limbs (k_rows_bases)
  uint32_t n, K, row0, rows;
};
struct RowsScalar {
  const uint8_t *a, *b, *c;  // c null: + 0
  uint64_t a_stride, b_stride, c_stride;  // 0: one scalar for every row
  uint8_t *out;
  uint64_t out_stride;
  const uint8_t *live;
  uint8_t *done_mask;
  bpp_device_rows_record *record;
  uint32_t n;
};

BPP_HD uint32_t rows_kp(uint32_t K) {
  uint32_t kp = 1;
  while (kp < K) kp <<= 1;
  return kp;
}
BPP_HD bool rows_live(const uint8_t *live, size_t i) { return !live || live[i] != 0; }
BPP_HD const uint8_t *rows_scalar_at(const RowsMsm &a, size_t i, uint32_t k) { return a.scalars + i * (size_t)a.scalar_stride + 32u * k; }
BPP_HD const uint8_t *rows_point_at(const RowsMsm &a, size_t i, uint32_t k) { return a.points + i * (size_t)a.point_stride + 32u * k; }
BPP_HD uint8_t *rows_out_at(uint8_t *out, uint64_t stride, size_t i) { return out + i * (size_t)stride; }

// a point's 32 bytes at any address -> the affine Niels entry; false (and the neutral element) where it does not decode
BPP_HD bool rows_point_decode(niels &q, const uint8_t *p) {
  uint8_t s[32];
#pragma unroll
  for (int k = 0; k < 32; k++) s[k] = p[k];
  if (ristretto_decompress(q, s)) return true;
  niels_identity(q);
  return false;
}

// a * b + c mod l on 32-byte rows at any address: 1 and the canonical bytes where every operand is canonical, else 0 and zeros.
// No branch on an operand: the decision is a mask on the result.
BPP_HD uint32_t rows_scalar_eval(uint8_t out32[32], const uint8_t *pa, const uint8_t *pb, const uint8_t *pc) {
  sc x, y, z, xm, xy, r;
  sc_load_words(x, pa);
  sc_load_words(y, pb);
  sc_0(z);
  if (pc) sc_load_words(z, pc);  // (whether the call has a c is public)
  const uint32_t ok = ct_sc_is_canonical(x) & ct_sc_is_canonical(y) & ct_sc_is_canonical(z);
  sc_to_mont(xm, x);
  sc_montmul(xy, xm, y);  // x R * y * R^-1 = x y mod l, below l
  sc_add(r, xy, z);
  const uint32_t keep = 0u - ok;
#pragma unroll
  for (int k = 0; k < 8; k++) r.v[k] &= keep;
  sc_store_words(out32, r);
  return ok;
}
BPP_HD const uint8_t *rows_operand_at(const uint8_t *p, uint64_t stride, size_t i) { return p ? p + i * (size_t)stride : nullptr; }

#if defined(__HIPCC__)
// the record, on the stream: in front of the row kernels (whose rows add to it with vector atomics) and behind them
__global__ void k_rows_record_init(bpp_device_rows_record *rec) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *rec = bpp_device_rows_record{0u, 0u, 0xffffffffu, 0u};
}
__global__ void k_rows_record_finish(bpp_device_rows_record *rec) {
  if (threadIdx.x == 0 && blockIdx.x == 0) atomicOr(&rec->flags, BPP_ROWS_WRITTEN);
}
__device__ __forceinline__ void rows_record_row(bpp_device_rows_record *rec, size_t i, uint32_t void_flags) {
  if (!rec) return;
  if (void_flags) {
    atomicAdd(&rec->n_void, 1u);
    atomicMin(&rec->first_void, (uint32_t)i);
    atomicOr(&rec->flags, void_flags);
  } else {
    atomicAdd(&rec->n_done, 1u);
  }
}

// per-row points of one slab: one lane per term of a LIVE row (a dead row's points are not read, and its slots are not read either)
__global__ void __launch_bounds__(64) k_rows_decode(RowsMsm a) {
  const uint64_t t = (uint64_t)blockIdx.x * 64u + threadIdx.x;
  if (t >= (uint64_t)a.rows * a.K) return;
  const uint32_t r = (uint32_t)(t / a.K), k = (uint32_t)(t - (uint64_t)r * a.K);
  const size_t i = (size_t)a.row0 + r;
  if (!rows_live(a.live, i)) return;
  niels q;
  const bool ok = rows_point_decode(q, rows_point_at(a, i, k));
  a.pts[t] = q;
  a.bad[t] = ok ? 0u : 1u;
}

// shared bases: one quad per base, the carried multiples 1 P .. 8 P as k_ct_straus makes them, once per call
__global__ void __launch_bounds__(64) k_rows_bases(RowsMsm a) {
  const uint32_t lane = threadIdx.x, qi = lane & 3u, k = lane >> 2;
  const QuadMask q = quad_mask(qi);
  const bool active = k < a.K;  // (idle quads walk the neutral element and store nothing)
  fe d2, one;
  fe_const(d2, FE_D2);
  fe_1(one);
  ge p;
  ge_identity(p);
  if (active) {
    niels b;
    const bool ok = rows_point_decode(b, a.points + 32u * k);
    ge_from_niels(p, b);
    if (qi == 0) a.bad[k] = ok ? 0u : 1u;
  }
  fe m;
  quad_load(m, q, p);
#pragma unroll 1
  for (uint32_t j = 0; j < BPP_CTS_ENTRIES; j++) {
    if (j) quad_ge_add(m, q, p, d2, one);
    fe c = m;
    fe_carry(c);
    if (active) {
#pragma unroll
      for (int w = 0; w < 10; w++) a.base_tab[(((size_t)k * BPP_CTS_ENTRIES + j) * 10u + (uint32_t)w) * 4u + qi] = c.v[w];
    }
  }
}

struct RowsMsmShared {
  uint32_t tab[BPP_CTS_ENTRIES][10][64];       // [entry][limb][lane]: lane = 4 * quad + coordinate
  int8_t dig[BPP_CT_DIGITS][BPP_CT_QUADS];     // [position][quad]
  ge part[BPP_CT_QUADS];                       // the segmented tree
  uint32_t flags[BPP_CT_QUADS];                // BPP_ROWS_SCALAR / BPP_ROWS_POINT of the quad's term
};
// KP = rows_kp(K); SHARED: the bases' multiples come from base_tab.  grid = ceil(rows / (16 / KP)) workgroups of one wavefront.
template <int KP, bool SHARED>
__global__ void __launch_bounds__(64) k_rows_msm(RowsMsm a) {
  static_assert(KP == 1 || KP == 2 || KP == 4 || KP == 8 || KP == 16, "terms per row, padded");
  static_assert(sizeof(RowsMsmShared) <= 26 * 1024, "six workgroups per CU");
  constexpr uint32_t ROWS_PER_WG = BPP_CT_QUADS / KP;
  const uint32_t lane = threadIdx.x, qi = lane & 3u, quad = lane >> 2;
  const uint32_t k = quad & (uint32_t)(KP - 1), r = blockIdx.x * ROWS_PER_WG + quad / (uint32_t)KP;
  const QuadMask q = quad_mask(qi);
  const bool in = r < a.rows;
  const size_t i = (size_t)a.row0 + (in ? r : 0u);
  const bool live = in && rows_live(a.live, i);
  const bool active = live && k < a.K;  // (public)
  __shared__ RowsMsmShared sh;
  fe d2, one;
  fe_const(d2, FE_D2);
  fe_1(one);
  fe m;
  uint32_t flags = 0;
  if (SHARED) {
    // the multiples 1 P .. 8 P of base k, made by k_rows_bases; the neutral element's (0, 1, 1, 0) for an idle quad
#pragma unroll 1
    for (uint32_t j = 0; j < BPP_CTS_ENTRIES; j++) {
#pragma unroll
      for (int w = 0; w < 10; w++) {
        uint32_t v = (w == 0 && (qi == 1 || qi == 2)) ? 1u : 0u;
        if (active) v = a.base_tab[(((size_t)k * BPP_CTS_ENTRIES + j) * 10u + (uint32_t)w) * 4u + qi];
        sh.tab[j][w][lane] = v;
      }
    }
    if (active) flags = a.bad[k] ? BPP_ROWS_POINT : 0u;
  } else {
    ge p;
    ge_identity(p);
    if (active) {
      const size_t t = (size_t)r * a.K + k;
      const niels b = a.pts[t];
      ge_from_niels(p, b);
      flags = a.bad[t] ? BPP_ROWS_POINT : 0u;
    }
    quad_load(m, q, p);
#pragma unroll 1
    for (uint32_t j = 0; j < BPP_CTS_ENTRIES; j++) {
      if (j) quad_ge_add(m, q, p, d2, one);
      fe c = m;
      fe_carry(c);
#pragma unroll
      for (int w = 0; w < 10; w++) sh.tab[j][w][lane] = c.v[w];
    }
  }
  if (qi == 0) {
    sc sv;
    sc_0(sv);
    if (active) sc_load_words(sv, rows_scalar_at(a, i, k));  // byte-wise: the row may lie at any address
    flags |= (1u - ct_sc_is_canonical(sv)) * BPP_ROWS_SCALAR;  // (a flag, by arithmetic: no branch)
    int8_t d[BPP_CT_DIGITS];
    ct_recode16(d, sv);
#pragma unroll
    for (int p = 0; p < BPP_CT_DIGITS; p++) sh.dig[p][quad] = d[p];
    sh.flags[quad] = flags;
  }
  __syncthreads();
  {
    ge id;
    ge_identity(id);
    quad_load(m, q, id);
  }
#pragma unroll 1
  for (int p = BPP_CT_DIGITS - 1; p >= 0; p--) {
    if (p != BPP_CT_DIGITS - 1) {
#pragma unroll 1
      for (int x = 0; x < 4; x++) quad_ge_dbl(m, q);
    }
    fe mine;
    ct_straus_coord(mine, &sh.tab[0][0][lane], 10u * 64u, 64u, (int32_t)sh.dig[p][quad], qi);
    ge other;
    quad_gather(other, mine);
    quad_ge_add(m, q, other, d2, one);
  }
  // the quads of a row by a segmented tree: level `off` adds quad k + off to quad k, k < off (readers read [off, 2 off), writers write
  // [0, off) of the row's segment)
  ge acc;
  quad_gather(acc, m);
  if (qi == 0) sh.part[quad] = acc;
#pragma unroll 1
  for (uint32_t off = (uint32_t)KP / 2; off >= 1; off >>= 1) {
    __syncthreads();
    if (k < off) {
      const ge y2 = sh.part[quad + off];
      quad_ge_add(m, q, y2, d2, one);
      quad_gather(acc, m);
      if (qi == 0) sh.part[quad] = acc;
    }
  }
  __syncthreads();
  if (in && k == 0 && qi == 0) {
    // ONE decision per row, after all of its terms: the flags of its quads (idle ones hold none)
    uint32_t f = 0;
#pragma unroll
    for (int x = 0; x < KP; x++) f |= sh.flags[quad + x];
    uint8_t c32[32];
    ristretto_compress(c32, acc);
    const uint32_t keep = (live && f == 0) ? 0xffu : 0u;
    uint8_t *o = rows_out_at(a.out, a.out_stride, i);
#pragma unroll
    for (int x = 0; x < 32; x++) o[x] = (uint8_t)(c32[x] & keep);
    if (a.done_mask) a.done_mask[i] = (uint8_t)(keep & 1u);
    if (live) rows_record_row(a.record, i, f);
  }
  // digits, selected multiples and partial sums are secret-derived: leave nothing in LDS for the next workgroup on this CU
  __syncthreads();
  for (uint32_t x = lane; x < sizeof(RowsMsmShared) / 4; x += 64) ((uint32_t *)&sh)[x] = 0;
}

// one lane per row
__global__ void __launch_bounds__(64) k_rows_scalar(RowsScalar a) {
  const uint64_t g = (uint64_t)blockIdx.x * 64u + threadIdx.x;
  if (g >= a.n) return;
  const size_t i = (size_t)g;
  uint8_t *o = rows_out_at(a.out, a.out_stride, i);
  if (!rows_live(a.live, i)) {
#pragma unroll
    for (int x = 0; x < 32; x++) o[x] = 0;
    if (a.done_mask) a.done_mask[i] = 0;
    return;
  }
  uint8_t r32[32];
  const uint32_t ok = rows_scalar_eval(r32, rows_operand_at(a.a, a.a_stride, i), rows_operand_at(a.b, a.b_stride, i),
                                       rows_operand_at(a.c, a.c_stride, i));
#pragma unroll
  for (int x = 0; x < 32; x++) o[x] = r32[x];
  if (a.done_mask) a.done_mask[i] = (uint8_t)ok;
  rows_record_row(a.record, i, ok ? 0u : BPP_ROWS_SCALAR);
}
#endif

// ---- host side: the refusals in front of any launch, the models.  Pure host C++.

struct RowsRange {
  std::string name;
  uintptr_t lo, hi;
  bool written;
};
inline std::string rows_overlap(const std::vector<RowsRange> &ranges) {
  for (size_t x = 0; x < ranges.size(); x++)
    for (size_t y = x + 1; y < ranges.size(); y++)
      if ((ranges[x].written || ranges[y].written) && ranges[x].lo < ranges[y].hi && ranges[y].lo < ranges[x].hi)
        return ranges[x].name + " and " + ranges[y].name + " overlap";
  return std::string();
}
inline std::string rows_common_refusal(size_t n, const uint8_t *out, size_t out_stride) {
  if (n == 0) return "n is 0";
  if (n > 0x7fffffffu) return "n is above 2^31 - 1";
  if (!out) return "out_dev is null";
  if (out_stride < 32) return "out_stride is below 32";
  if (out_stride > ((size_t)1 << 40)) return "out_stride is above 2^40";
  return std::string();
}
inline void rows_common_ranges(std::vector<RowsRange> &ranges, size_t n, const uint8_t *out, size_t out_stride, const uint8_t *live,
                               const uint8_t *done_mask, const bpp_device_rows_record *record) {
  ranges.push_back(RowsRange{"out_dev", (uintptr_t)out, (uintptr_t)out + (n - 1) * out_stride + 32, true});
  if (live) ranges.push_back(RowsRange{"live_dev", (uintptr_t)live, (uintptr_t)live + n, false});
  if (done_mask) ranges.push_back(RowsRange{"done_mask_dev", (uintptr_t)done_mask, (uintptr_t)done_mask + n, true});
  if (record) ranges.push_back(RowsRange{"record_dev", (uintptr_t)record, (uintptr_t)record + sizeof(bpp_device_rows_record), true});
}

// What bpp_rows_msm_enqueue refuses from the arguments alone (no pointer is dereferenced but `in`): the field is named.  Empty: nothing
// to refuse.  The pointer kinds are the engine's to check.
inline std::string rows_msm_refusal(const bpp_rows_msm *in, const uint8_t *out, size_t out_stride, const uint8_t *live, const uint8_t *done_mask,
                                    const bpp_device_rows_record *record) {
  if (!in) return "in is null";
  if (in->K == 0 || in->K > BPP_ROWS_K_MAX) return "K must be 1 .. " + std::to_string(BPP_ROWS_K_MAX);
  const std::string common = rows_common_refusal(in->n, out, out_stride);
  if (!common.empty()) return common;
  const size_t n = in->n, row = 32 * (size_t)in->K;
  if (!in->scalars_dev) return "scalars_dev is null";
  if (!in->points_dev) return "points_dev is null";
  if (in->scalar_stride < row) return "scalar_stride is below 32 K";
  if (in->scalar_stride > ((size_t)1 << 40)) return "scalar_stride is above 2^40";
  if (in->point_stride != 0 && in->point_stride < row) return "point_stride is below 32 K (and not 0)";
  if (in->point_stride > ((size_t)1 << 40)) return "point_stride is above 2^40";
  std::vector<RowsRange> ranges;
  ranges.push_back(RowsRange{"scalars_dev", (uintptr_t)in->scalars_dev, (uintptr_t)in->scalars_dev + (n - 1) * in->scalar_stride + row, false});
  ranges.push_back(RowsRange{"points_dev", (uintptr_t)in->points_dev, (uintptr_t)in->points_dev + (n - 1) * in->point_stride + row, false});
  rows_common_ranges(ranges, n, out, out_stride, live, done_mask, record);
  return rows_overlap(ranges);
}
inline std::string rows_scalar_refusal(size_t n, const bpp_scalar_rows *a, const bpp_scalar_rows *b, const bpp_scalar_rows *c, const uint8_t *out,
                                       size_t out_stride, const uint8_t *live, const uint8_t *done_mask, const bpp_device_rows_record *record) {
  const std::string common = rows_common_refusal(n, out, out_stride);
  if (!common.empty()) return common;
  if (!a) return "a is null";
  if (!b) return "b is null";
  std::vector<RowsRange> ranges;
  const bpp_scalar_rows *ops[3] = {a, b, c};
  const char *names[3] = {"a", "b", "c"};
  for (int x = 0; x < 3; x++) {
    if (!ops[x]) continue;
    const std::string nm = names[x];
    if (!ops[x]->dev) return nm + ".dev is null";
    if (ops[x]->stride != 0 && ops[x]->stride < 32) return nm + ".stride is below 32 (and not 0)";
    if (ops[x]->stride > ((size_t)1 << 40)) return nm + ".stride is above 2^40";
    ranges.push_back(RowsRange{nm + ".dev", (uintptr_t)ops[x]->dev, (uintptr_t)ops[x]->dev + (n - 1) * ops[x]->stride + 32, false});
  }
  rows_common_ranges(ranges, n, out, out_stride, live, done_mask, record);
  return rows_overlap(ranges);
}

// the launch arguments of a call that passed the refusals (the context's buffers and the slab are the engine's to fill in)
inline void rows_msm_args(RowsMsm &a, const bpp_rows_msm &in, uint8_t *out, size_t out_stride, const uint8_t *live, uint8_t *done_mask,
                          bpp_device_rows_record *record) {
  memset(&a, 0, sizeof(a));
  a.scalars = in.scalars_dev, a.scalar_stride = in.scalar_stride, a.points = in.points_dev, a.point_stride = in.point_stride;
  a.out = out, a.out_stride = out_stride, a.live = live, a.done_mask = done_mask, a.record = record;
  a.n = (uint32_t)in.n, a.K = in.K, a.row0 = 0, a.rows = (uint32_t)in.n;
}
inline void rows_scalar_args(RowsScalar &s, size_t n, const bpp_scalar_rows *a, const bpp_scalar_rows *b, const bpp_scalar_rows *c, uint8_t *out,
                             size_t out_stride, const uint8_t *live, uint8_t *done_mask, bpp_device_rows_record *record) {
  memset(&s, 0, sizeof(s));
  s.a = a->dev, s.a_stride = a->stride, s.b = b->dev, s.b_stride = b->stride;
  if (c) s.c = c->dev, s.c_stride = c->stride;
  s.out = out, s.out_stride = out_stride, s.live = live, s.done_mask = done_mask, s.record = record, s.n = (uint32_t)n;
}

struct RowsRecordHost {
  bpp_device_rows_record rec{0u, 0u, 0xffffffffu, 0u};
  void row(size_t i, uint32_t void_flags) {
    if (void_flags) {
      rec.n_void++;
      if ((uint32_t)i < rec.first_void) rec.first_void = (uint32_t)i;
      rec.flags |= void_flags;
    } else {
      rec.n_done++;
    }
  }
  void finish(bpp_device_rows_record *out) {
    rec.flags |= BPP_ROWS_WRITTEN;
    if (out) *out = rec;
  }
};

// k_rows_decode / k_rows_bases, k_rows_msm and the record kernels on the host, one lane per quad: per live row the K terms -- and the
// Kp - K padding terms, on the neutral element and the scalar zero -- each through ct_straus_model on ONE term (the quad's walk: the
// table 1 P .. 8 P, 64 positions, ct_straus_coord), the padded segmented tree in the kernel's order, ristretto_compress.  A live row
// runs the whole walk whether it ends void or not, as the kernel does: the table-read trace (BPP_CT_TOUCH) of a row depends on K alone.
inline void rows_msm_run_host(const RowsMsm &a) {
  RowsRecordHost rec;
  const uint32_t K = a.K, KP = rows_kp(K);
  const bool shared = a.point_stride == 0;
  std::vector<niels> bases(K);
  uint32_t base_flags = 0;
  if (shared)
    for (uint32_t k = 0; k < K; k++)
      if (!rows_point_decode(bases[k], a.points + 32u * k)) base_flags |= BPP_ROWS_POINT;
  for (size_t i = 0; i < a.n; i++) {
    uint8_t *o = rows_out_at(a.out, a.out_stride, i);
    if (!rows_live(a.live, i)) {
      ingest_zero(o, 32, 0, 1);
      if (a.done_mask) a.done_mask[i] = 0;
      continue;
    }
    uint32_t flags = base_flags;
    ge part[BPP_ROWS_K_MAX];
    for (uint32_t k = 0; k < KP; k++) {
      ge p;
      sc s;
      ge_identity(p);
      sc_0(s);
      if (k < K) {
        niels b;
        if (shared) b = bases[k];
        else if (!rows_point_decode(b, rows_point_at(a, i, k))) flags |= BPP_ROWS_POINT;
        ge_from_niels(p, b);
        uint8_t s32[32];
        ingest_copy(s32, rows_scalar_at(a, i, k), 32, 0, 1);
        sc_load_words(s, s32);
        flags |= (1u - ct_sc_is_canonical(s)) * BPP_ROWS_SCALAR;
        for (size_t x = 0; x < 32; x++) ((volatile uint8_t *)s32)[x] = 0;
      }
      ct_straus_model(part[k], &p, &s, 1);
      for (size_t x = 0; x < sizeof(s); x++) ((volatile uint8_t *)&s)[x] = 0;
    }
    for (uint32_t off = KP / 2; off >= 1; off >>= 1)
      for (uint32_t k = 0; k < off; k++) ge_add(part[k], part[k], part[k + off]);
    uint8_t c32[32];
    ristretto_compress(c32, part[0]);
    const uint8_t keep = flags == 0 ? 0xff : 0;
    for (int x = 0; x < 32; x++) o[x] = (uint8_t)(c32[x] & keep);
    if (a.done_mask) a.done_mask[i] = (uint8_t)(keep & 1u);
    rec.row(i, flags);
  }
  rec.finish(a.record);
}

inline void rows_scalar_run_host(const RowsScalar &a) {
  RowsRecordHost rec;
  for (size_t i = 0; i < a.n; i++) {
    uint8_t *o = rows_out_at(a.out, a.out_stride, i);
    if (!rows_live(a.live, i)) {
      ingest_zero(o, 32, 0, 1);
      if (a.done_mask) a.done_mask[i] = 0;
      continue;
    }
    uint8_t r32[32];
    const uint32_t ok = rows_scalar_eval(r32, rows_operand_at(a.a, a.a_stride, i), rows_operand_at(a.b, a.b_stride, i),
                                         rows_operand_at(a.c, a.c_stride, i));
    for (int x = 0; x < 32; x++) o[x] = r32[x];
    if (a.done_mask) a.done_mask[i] = (uint8_t)ok;
    rec.row(i, ok ? 0u : BPP_ROWS_SCALAR);
  }
  rec.finish(a.record);
}

}  // namespace bpp
