// Scalar recodings shared by host and device (host-compiled by tests/: every digit string must add up to its scalar).
//   msm_recode : signed digits of the Pippenger MSM, uneven windows (MsmPlan)
//   fb_recode  : signed digits of the prover's fixed-base tables (FbGeom)
#pragma once
#include <stdlib.h>

#include "scalar.h"

namespace bpp {

// Window layout: 253 = K_wide * c + (K - K_wide) * (c - 1).  Canonical scalars are < l < 2^252 + 2^125, so 253 bits and
// no carry out of the top window; with equal widths the top window would hold only 253 mod c bits and concentrate every
// term of a group in a handful of buckets (one lane adding thousands of points in sequence) unless c divides 253 (c =
// 11).  Windows of c-1 bits simply leave the upper half of their 2^(c-1) buckets empty.
struct MsmPlan {
  uint32_t c;        // window bits (wide windows)
  uint32_t K;        // windows
  uint32_t K_wide;   // windows [0, K_wide) have c bits, windows [K_wide, K) have c - 1
  uint32_t nb;       // buckets per window = 2^(c-1)
  uint32_t G;        // groups
  uint32_t n_terms;  // total terms
  uint32_t split;    // 1: half-scalar plan -- every term appears twice, (s mod 2^126, P) and (s >> 126, 2^126 P), the windows
                     // cover 127 bits: half the doublings in the final Horner step (small calls, msm.h)
};
// Canonical scalars are < l = 2^252 + d, d < 2^125.  Split at bit 126: the low half has 126 bits; the high half has 126 bits
// too, except for s >= 2^252, where it is EXACTLY 2^126 (s - 2^252 < 2^125 leaves nothing below bit 126 of the shifted
// value).  With windows over 127 bits (BPP_MSM_SPLIT_BITS) both halves fill every window evenly -- the top window keeps its
// spare top bit, so its raw value stays under half its range and nothing carries out; the one exception, the lone bit 126,
// makes the top window's raw value exactly half with no carry coming in (everything below is zero): digit +half, a bucket
// that exists.  (Splitting at bit 127 over 128-bit windows left the top window with 7-8 significant bits: a quarter of its
// buckets got all of its terms, lists of 40-60 additions: 0.10 ms of accumulation for 256 proofs instead of 0.04.)
#define BPP_MSM_SPLIT_BIT 126u
#define BPP_MSM_SPLIT_BITS 127u
#define BPP_TERM_HI 0x80000000u   // term_sidx: take the high half of the scalar
#define BPP_POINT_HI 0x40000000u  // term_pidx / sorted[]: the point's 2^126 multiple (bit 31 of sorted[] is the sign)

// digits of one canonical scalar, written with stride `stride` (window-major layout of k_msm_digits: stride = terms of the group)
BPP_HD void msm_recode(int16_t *out, size_t stride, const sc &s, const MsmPlan &plan) {
  uint32_t carry = 0, bit = 0;
  for (uint32_t k = 0; k < plan.K; k++) {
    const uint32_t wd = k < plan.K_wide ? plan.c : plan.c - 1;  // this window's width
    const uint32_t wi = bit >> 5, sh = bit & 31;
    uint32_t raw = 0;
    if (wi < 8) {
      uint64_t two = (uint64_t)s.v[wi] | ((wi + 1 < 8) ? ((uint64_t)s.v[wi + 1] << 32) : 0ULL);
      raw = (uint32_t)(two >> sh) & ((1u << wd) - 1u);
    }
    uint32_t v = raw + carry;
    int32_t dgt;
    if (v > (1u << (wd - 1))) {  // digits in (-2^(wd-1), 2^(wd-1)]
      dgt = (int32_t)v - (int32_t)(1u << wd);
      carry = 1;
    } else {
      dgt = (int32_t)v;
      carry = 0;
    }
    out[(size_t)k * stride] = (int16_t)dgt;
    bit += wd;
  }
}

// The same digit for ONE window, computed from the words around it (what the fused sort kernel does: it owns one window of
// every term and never sees the whole digit string).  The carry into window k is decided by window k-1 alone unless that
// window's raw value is exactly half its range, in which case it is the carry into k-1 (and so on down): carry(j+1) =
// raw_j > half_j, or raw_j == half_j and carry(j).  `w` = the scalar's eight 32-bit words, read on demand.
BPP_HD uint32_t msm_window_bit(const MsmPlan &plan, uint32_t k) {
  return k <= plan.K_wide ? k * plan.c : plan.K_wide * plan.c + (k - plan.K_wide) * (plan.c - 1);
}
BPP_HD uint32_t msm_window_raw(const uint32_t *w, uint32_t bit, uint32_t wd) {
  const uint32_t wi = bit >> 5, sh = bit & 31;
  if (wi >= 8) return 0;
  uint32_t v = w[wi] >> sh;
  if (sh + wd > 32 && wi + 1 < 8) v |= w[wi + 1] << (32 - sh);
  return v & ((1u << wd) - 1u);
}
BPP_HD int32_t msm_digit_at(const uint32_t *w, const MsmPlan &plan, uint32_t k) {
  uint32_t carry = 0;
  for (uint32_t j = k; j-- > 0;) {
    const uint32_t wdj = j < plan.K_wide ? plan.c : plan.c - 1;
    const uint32_t rawj = msm_window_raw(w, msm_window_bit(plan, j), wdj), half = 1u << (wdj - 1);
    if (rawj != half) {
      carry = rawj > half ? 1u : 0u;
      break;
    }
  }
  const uint32_t wd = k < plan.K_wide ? plan.c : plan.c - 1;
  const uint32_t v = msm_window_raw(w, msm_window_bit(plan, k), wd) + carry;
  return v > (1u << (wd - 1)) ? (int32_t)v - (int32_t)(1u << wd) : (int32_t)v;
}

// plan for a group of `terms` terms with window width c
// bits = 253 (canonical scalars), or BPP_MSM_SPLIT_BITS for the half-scalar plan
inline MsmPlan msm_make_plan(uint32_t c, uint32_t G, uint32_t n_terms, uint32_t bits = 253) {
  MsmPlan plan;
  plan.c = c;
  plan.K = (bits + c - 1) / c;
  plan.K_wide = plan.K - (plan.K * c - bits);  // bits = K_wide * c + (K - K_wide) * (c - 1)
  plan.nb = 1u << (c - 1);
  plan.G = G;
  plan.n_terms = n_terms;
  plan.split = bits == 253 ? 0u : 1u;
  return plan;
}
// Window width of a group of `group_terms` terms in a call of `all_terms` (the engine's choose_window with the context's options
// spelled out: c_max_opt / bias_opt < 0 and c_add <= 0 mean the engine's own rule).  Host-compiled by the tests as well.
#define BPP_SMALL_CALL_TERMS 20000u     // a call of up to this many MSM terms has the chip to itself
#define BPP_WIDE_WINDOW_TERMS 200000u   // groups from here on may take windows above 11 bits -- and the sliced prelude (msm.h)
inline uint32_t msm_choose_window(uint32_t group_terms, uint32_t all_terms, int c_max_opt = -1, int c_add = 0, int bias_opt = -1) {
  // buckets per window ~ terms / 12  (bucket lists of ~12 points keep the per-lane chains short)
  uint32_t c = 4;
  while (c < 14 && (1u << c) * 12u <= group_terms) c++;  // nb = 2^(c-1)
  // Above 11 bits the buckets of a window no longer fit the row / column reduction (2.1 additions per bucket, k_msm_window_rc)
  // and go through the bit-plane one (c / 2 per bucket): 13 bits for a 4096-proof batch (61 k terms) is 20 x 61 k + 20 x 4096
  // x 6.5 = 1.76 M additions, 11 bits 23 x 61 k + 23 x 1024 x 2.1 = 1.47 M.  The wider windows only pay from ~200 k terms on.
  const uint32_t c_max = c_max_opt >= 0 ? (uint32_t)c_max_opt : (group_terms < BPP_WIDE_WINDOW_TERMS ? 11u : 14u);
  if (c_add > 0 && all_terms > BPP_SMALL_CALL_TERMS) c += (uint32_t)c_add;  // (A/B timing of wider windows)
  if (c > c_max && c_max >= 4) c = c_max;
  // A small call has the chip to itself: its time is the length of the dependency chains, not the number of additions.
  // Wider windows shorten the bucket lists (accumulation) and the Horner step (fewer windows to add) for a longer
  // row / column reduction: three more bits are worth 0.07-0.1 ms up to a few hundred proofs (one proof 0.79 -> 0.68 ms).
  const int bias = bias_opt >= 0 ? bias_opt : 3;  // (tests run the narrow windows as well)
  if (all_terms <= BPP_SMALL_CALL_TERMS) {
    int cb = (int)c + bias;
    c = (uint32_t)(cb < 4 ? 4 : (cb > 11 ? 11 : cb));
  }
  return c;
}

// ---- The two forms of the MSM's prelude (msm.h) and what a workgroup of each needs in LDS.
//   form 0  k_msm_prelude<T>: one workgroup of T lanes per (group, window).  Two bucket tables of nb words (histogram, write
//           cursors) in dynamic LDS, T + 3 x 256 words of static arrays (part[], cls_*), and as many cached digits (two bytes
//           each) as keep the workgroup 1 KB under 64 KB -- a BUDGET (two such workgroups per CU), not the hardware's limit.
//   form 1  the sliced prelude: k_msm_slice_hist / k_msm_slice_scatter hold ONE bucket table of nb words (256 lanes, nothing
//           static); k_msm_slice_scan holds BPP_SLICE_SCAN_THREADS + 3 x 256 words of static arrays and no table.
// A gfx950 workgroup may hold 160 KiB of LDS (the whole CU's), so the limit a plan is held to is 163 840 bytes.
// Bytes per workgroup for every (c, form) the window rule can produce (nb = 2^(c-1); "+ cache" = digits, up to 64 512 in all):
//     c      nb    form 0, T = 1024    form 0, T = 256    form 1 (hist / scatter | scan)
//   4..11  <=1024   <=15 360 + cache    <=12 288 + cache    <= 4 096 | 7 168
//    12     2048     23 552 + cache      20 480 + cache        8 192 | 7 168
//    13     4096     39 936 + cache      36 864 + cache       16 384 | 7 168
//    14     8192     72 704, no cache    69 632, no cache     32 768 | 7 168
// 14-bit windows in form 0 are past the 64 KB budget (msm_prelude_dig_cap then caches nothing) and inside the limit: one such
// workgroup per (group, window) runs -- tests/test_gpu_msm_structured.py has it at 25 000 terms -- with two per CU at most.  Groups
// that get 14 bits by rule (BPP_WIDE_WINDOW_TERMS terms and more) take form 1 by rule as well: 32 KB, five workgroups per CU.
// msm_prelude_fits is what msm_plan_alloc asks before anything is allocated or launched; forced widths above 14 bits are what
// it refuses (c = 16, form 0: 269 312 bytes).
#define BPP_LDS_LIMIT 163840u
#define BPP_SLICE_THREADS 256u
#define BPP_SLICE_SCAN_THREADS 1024u
#define BPP_SLICES_MAX 64u
// the least a workgroup of the form needs (form 0: without any cached digit)
inline uint32_t msm_prelude_min_lds(uint32_t nb, uint32_t threads, uint32_t form) {
  if (form == 0) return 2u * nb * 4u + (threads + 3u * 256u) * 4u;
  const uint32_t table = nb * 4u, scan = (BPP_SLICE_SCAN_THREADS + 3u * 256u) * 4u;
  return table > scan ? table : scan;
}
inline bool msm_prelude_fits(uint32_t nb, uint32_t threads, uint32_t form) {
  return nb != 0 && nb <= (1u << 20) && msm_prelude_min_lds(nb, threads, form) <= BPP_LDS_LIMIT;
}
// How many slices the (group, window) sorts of a plan are cut into; 0: the one-workgroup form.  forced >= 2: that many, whatever
// the size (option "msm_prelude_slices"); forced == 1: the one-workgroup form whatever the size (A/B timing of the two forms).
// By rule a group of BPP_WIDE_WINDOW_TERMS terms and more is sliced -- with one workgroup per (group, window) such a call puts ~20 workgroups on 256 CUs, each walking its group's terms twice -- and so is a
// plan whose tables fit form 1 only.  S aims at 640 workgroups per phase (two and a half per CU) and keeps 2048 terms per slice:
// measured on one group of 1 048 706 terms at 14 bits (19 windows), the three launches took 1.25 / 1.10 / 1.25 / 1.32 ms with S =
// 16 / 32 / 54 / 64 against 3.90 ms in the one-workgroup form (profiles/verify_joint.json).
inline uint32_t msm_prelude_slices(uint32_t max_group_terms, uint32_t G, uint32_t K, uint32_t nb, uint32_t threads, int forced) {
  if (forced >= 2) return (uint32_t)forced < BPP_SLICES_MAX ? (uint32_t)forced : BPP_SLICES_MAX;
  if (forced == 1) return 0;
  if (max_group_terms < BPP_WIDE_WINDOW_TERMS && msm_prelude_fits(nb, threads, 0)) return 0;
  const uint32_t gk = G * K ? G * K : 1u;
  uint32_t S = (640u + gk - 1u) / gk;
  const uint32_t by_terms = (max_group_terms + 2047u) / 2048u;
  if (S > by_terms) S = by_terms;
  if (S > BPP_SLICES_MAX) S = BPP_SLICES_MAX;
  return S < 2u ? 2u : S;
}

// the half of a canonical scalar a split plan's term stands for, as eight words (upper ones zero)
BPP_HD void msm_half_words(uint32_t h[8], const uint32_t *w, bool hi) {
  constexpr uint32_t W = BPP_MSM_SPLIT_BIT >> 5, SH = BPP_MSM_SPLIT_BIT & 31u;  // 126 = 3 * 32 + 30
  static_assert(SH != 0, "the split bit is not word-aligned");
  for (int i = 0; i < 8; i++) h[i] = 0;
  if (!hi) {
    for (uint32_t i = 0; i < W; i++) h[i] = w[i];
    h[W] = w[W] & ((1u << SH) - 1u);
  } else {
    for (uint32_t i = 0; W + i < 8; i++) h[i] = (w[W + i] >> SH) | (W + i + 1 < 8 ? w[W + i + 1] << (32u - SH) : 0u);
  }
}

// Window width is chosen per parameter set (fb_geometry): the widest window whose table stays under ~1.8 GB, because
// random 128-byte lines come at 21 G lines/s out of <= 2 GB but only ~10 G lines/s out of larger tables (TLB reach,
// tools/microbench/rand_lines.hip).  11 bits (<= 600 generators) = 23 additions per term out of 24 slots of 1024 entries.
//
// A canonical scalar has 253 bits.  Signed digits need one position more than ceil(253 / wbits) only when the top window is
// full (253 = 23 x 11): its carry would be a 24th digit that is 0 or 1 -- a whole addition per term for one bit.  In that
// case the top window is kept UNSIGNED instead (digit 0 .. 2^wbits, no carry out) and its entries 2^(wbits-1)+1 .. 2^wbits
// live in the table slot the carry digit would have used: same table size, same addressing (slot w, entry digit - 1 simply
// runs on into slot w + 1), one addition per term fewer.  `items` = digit positions, `windows` = table slots per generator.
struct FbGeom {
  uint32_t wbits;    // window width
  uint32_t windows;  // table slots per generator: ceil(254 / wbits)
  uint32_t entries;  // entries per slot: 2^(wbits-1) signed multiples 1..2^(wbits-1)
  uint32_t items;    // digit positions per scalar: windows, or windows - 1 with the unsigned top window
};
#define FB_MAX_WINDOWS 32
#define FB_BUILD_BLOCK 128  // entries per lane of k_fb_build
inline FbGeom fb_geometry(uint32_t n_gens) {  // host side
  uint32_t w = 8;
  const char *forced = getenv("BPP_FB_WBITS");  // tests: exercise every geometry on small parameter sets
  const uint32_t top = forced ? (uint32_t)atoi(forced) : 11u;
  for (uint32_t cand = (top >= 8 && top <= 11) ? top : 11u; cand > 8; cand--) {
    const uint64_t bytes = (uint64_t)n_gens * ((254 + cand - 1) / cand) * (1ull << (cand - 1)) * 128ull;
    if (bytes <= 1800ull << 20) {
      w = cand;
      break;
    }
  }
  FbGeom g;
  g.wbits = w;
  g.windows = (254 + w - 1) / w;
  g.entries = 1u << (w - 1);
  g.items = (253u % w == 0u) ? 253u / w : g.windows;
  return g;
}
BPP_HD size_t fb_stride(const FbGeom &g) { return (size_t)g.windows * g.entries; }  // entries per generator
BPP_HD bool fb_top_unsigned(const FbGeom &g) { return g.items < g.windows; }

// word i of a scalar (0 for i >= 8) without indexing its register array at run time
BPP_HD uint32_t sc_word(const sc &s, uint32_t i) {
  uint32_t r = 0;
#pragma unroll
  for (uint32_t k = 0; k < 8; k++) r = (i == k) ? s.v[k] : r;
  return r;
}

// digits of a canonical scalar: signed, in [-(2^(w-1) - 1), 2^(w-1)]; the top one in [0, 2^w] when fb_top_unsigned
BPP_HD void fb_recode(int16_t *dig, const sc &s, const FbGeom &g) {
  uint32_t carry = 0;
  for (uint32_t w = 0; w < g.items; w++) {
    const uint32_t bit = w * g.wbits, wi = bit >> 5, sh = bit & 31u;
    uint32_t raw = 0;
    if (wi < 8) {
      // (sc_word: a select chain over the eight words; s.v[wi] with a run-time wi parks the scalar in scratch memory)
      const uint64_t two = (uint64_t)sc_word(s, wi) | ((uint64_t)sc_word(s, wi + 1) << 32);
      raw = (uint32_t)(two >> sh) & ((1u << g.wbits) - 1u);
    }
    const uint32_t v = raw + carry;
    carry = (v > g.entries && !(fb_top_unsigned(g) && w + 1 == g.items)) ? 1u : 0u;
    dig[w] = (int16_t)((int32_t)v - (int32_t)(carry << g.wbits));
  }
}

}  // namespace bpp
