// Uniform-access scalar multiplication for the terms whose scalars are SECRET AND NOTHING ELSE, where the reference itself is
// constant-time:
//   PedersenGens::commit            src/generators/pedersen_gens.rs:112-122   P::multiscalar_mul (dalek's constant-time Straus)
//   the prover's witness check      src/range_proof.rs:275-284                (calls commit)
//   A1 and B of the final round     src/range_proof.rs:572-584                `&P * Scalar` (constant-time variable-base mult)
// Everything else on the prover's path is variable-time in the reference as well (A: vartime_mixed_multiscalar_mul :339-345;
// every L and R: vartime_multiscalar_mul :482-495) and runs through the engine's fixed-base tables, whose ADDRESSES are digits of
// witness-derived scalars (kernels_prove.h: k_fb_msm, kp_A) -- DESIGN.md, "What is variable-time in secrets".
//
// The form (the one dalek uses for those calls, restated): signed radix-16 digits of the scalar, a table of the multiples
// 0 P .. 8 P per term, and for every digit position four doublings and ONE addition of the entry the digit names -- found by
// reading ALL nine entries and keeping one under an arithmetic mask, the sign applied by a select.  No branch and no address
// depends on the scalar: the sequence of table reads is the same for every scalar (tests/test_host_arith.py records it through
// BPP_CT_TOUCH in a host build and compares two scalars' traces), and so is the instruction stream.
//
// On the device one term runs on one QUAD (msm.h: lane q of the quad holds coordinate q of the accumulator, a doubling or an
// addition is two rounds of four field products); k_ct_straus gives a quad K terms and one accumulator, a workgroup of 64 lanes
// sums up to 16 K terms of one output.
#pragma once
#include "point.h"
#include "scalar.h"
#include "ct_plan.h"
#if defined(__HIPCC__)
#include "msm.h"  // the quad forms of the point operations
#endif

namespace bpp {

#define BPP_CT_DIGITS 64
#define BPP_CT_ENTRIES 9  // 0 P .. 8 P

#ifndef BPP_CT_TOUCH
#define BPP_CT_TOUCH(entry) \
  do {                      \
  } while (0)
#endif

// signed radix-16 digits of a canonical scalar (< 2^253): 64 digits, d_0 .. d_62 in [-8, 8), d_63 in [0, 2].  Branch-free.
BPP_HD void ct_recode16(int8_t d[BPP_CT_DIGITS], const sc &s) {
  int32_t carry = 0;
#pragma unroll
  for (int i = 0; i < BPP_CT_DIGITS; i++) {
    int32_t v = (int32_t)((s.v[i >> 3] >> (4 * (i & 7))) & 15u) + carry;
    carry = (i + 1 < BPP_CT_DIGITS) ? ((v + 8) >> 4) : 0;
    v -= carry << 4;
    d[i] = (int8_t)v;
  }
}

// out[0..N) = the row that holds multiple `mag`, rows = multiples first, first + 1, .., first + E - 1 (zero when mag is none of
// them): EVERY row is read, one is kept.  `table` = E rows of `row_stride` words.
// Word k of a row lies `word_stride` words after word k - 1 (1: a row is contiguous).
template <int N, int E = BPP_CT_ENTRIES>
BPP_HD void ct_select_words(uint32_t (&out)[N], const uint32_t *table, uint32_t row_stride, uint32_t mag, uint32_t first = 0,
                            uint32_t word_stride = 1) {
#pragma unroll
  for (int k = 0; k < N; k++) out[k] = 0;
#pragma unroll
  for (uint32_t j = 0; j < (uint32_t)E; j++) {
    BPP_CT_TOUCH(j);
    const uint32_t keep = 0u - ((((j + first) ^ mag) - 1u) >> 31);  // all ones iff j + first == mag (the xor is < 2^31)
#pragma unroll
    for (int k = 0; k < N; k++) out[k] |= table[(size_t)j * row_stride + (size_t)k * word_stride] & keep;
  }
}

// |d| and the sign of a digit without a branch
BPP_HD void ct_digit_parts(uint32_t &mag, uint32_t &neg, int32_t d) {
  const int32_t m = d >> 31;  // 0 or -1
  mag = (uint32_t)((d ^ m) - m);
  neg = (uint32_t)m & 1u;
}

// h = neg ? -f : f by word-wise selects (f reduced)
BPP_HD void fe_cneg_select(fe &h, const fe &f, uint32_t neg) {
  fe n;
  fe_neg(n, f);
  const uint32_t keep = 0u - neg;
#pragma unroll
  for (int i = 0; i < 10; i++) h.v[i] = (n.v[i] & keep) | (f.v[i] & ~keep);
}

// ---- the whole multiplication on ONE lane: the host probe's form (and the definition the quad form is held to) ----
BPP_HD void ct_scalarmul(ge &r, const ge &p, const sc &s) {
  ge tab[BPP_CT_ENTRIES];
  ge_identity(tab[0]);
  tab[1] = p;
  for (int j = 2; j < BPP_CT_ENTRIES; j++) ge_add(tab[j], tab[j - 1], p);
  // entries with carried limbs: what ct_select_words ORs together must be valid limbs of ONE entry
  for (int j = 0; j < BPP_CT_ENTRIES; j++) {
    fe_carry(tab[j].X);
    fe_carry(tab[j].Y);
    fe_carry(tab[j].Z);
    fe_carry(tab[j].T);
  }
  int8_t d[BPP_CT_DIGITS];
  ct_recode16(d, s);
  ge acc;
  ge_identity(acc);
  for (int i = BPP_CT_DIGITS - 1; i >= 0; i--) {
    if (i != BPP_CT_DIGITS - 1)
      for (int k = 0; k < 4; k++) ge_dbl(acc, acc);
    uint32_t mag, neg;
    ct_digit_parts(mag, neg, d[i]);
    uint32_t w[40];
    ct_select_words<40>(w, (const uint32_t *)tab, 40, mag);
    ge q;
    for (int k = 0; k < 10; k++) {
      q.X.v[k] = w[k];
      q.Y.v[k] = w[10 + k];
      q.Z.v[k] = w[20 + k];
      q.T.v[k] = w[30 + k];
    }
    fe_cneg_select(q.X, q.X, neg);
    fe_cneg_select(q.T, q.T, neg);
    ge_add(acc, acc, q);
  }
  r = acc;
}

// ---- FIXED bases (the Pedersen bases H, G_k of a parameter set): no doublings at all.  Table line [base][position w][j - 1] =
// j * 16^w * Base as an affine Niels entry, j = 1..8 (64 positions x 8 lines x 128 B = 64 KB per base, built once per parameter
// set); digit position w of a term contributes the line its digit names -- all eight lines of the position are read, one is kept
// under a mask, a zero digit keeps none and becomes the neutral entry (1, 1, 0), the sign exchanges y+x / y-x and negates 2dxy by
// selects -- and the 64 positions are 64 independent mixed additions.
#define BPP_CTF_ENTRIES 8
#define BPP_CTF_LINE_WORDS 32  // one 128-byte line
BPP_HD void ct_fixed_select(niels &q, const niels *position_lines, int32_t digit) {
  uint32_t mag, neg;
  ct_digit_parts(mag, neg, digit);
  uint32_t w[30];
  ct_select_words<30, BPP_CTF_ENTRIES>(w, (const uint32_t *)position_lines, BPP_CTF_LINE_WORDS, mag, 1);
  const uint32_t isz = (mag - 1u) >> 31;  // 1 iff the digit is zero: the neutral entry
  w[0] |= isz;
  w[10] |= isz;
  const uint32_t sw = 0u - neg;
  fe t2d;
#pragma unroll
  for (int k = 0; k < 10; k++) {
    const uint32_t a = w[k], b = w[10 + k];
    q.yplusx.v[k] = (b & sw) | (a & ~sw);
    q.yminusx.v[k] = (a & sw) | (b & ~sw);
    t2d.v[k] = w[20 + k];
  }
  fe_cneg_select(q.xy2d, t2d, neg);
}
// one lane's model of the whole sum (host probe): acc = sum_w line(w, digit_w)
BPP_HD void ct_fixed_scalarmul(ge &r, const niels *base_lines /* [64][8] */, const sc &s) {
  int8_t d[BPP_CT_DIGITS];
  ct_recode16(d, s);
  ge acc;
  ge_identity(acc);
  for (int w = 0; w < BPP_CT_DIGITS; w++) {
    niels q;
    ct_fixed_select(q, base_lines + (size_t)w * BPP_CTF_ENTRIES, d[w]);
    ge_madd(acc, acc, q);
  }
  r = acc;
}

// ---- VARIABLE bases known before their secret scalars (the prover's A1: r Gf[0] + s Hf[0], src/range_proof.rs:574-576): the
// 63 x 4 doublings of the ladder above are doublings of a PUBLIC point -- they need not wait for the scalar, and they need not be
// uniform.  With pow[w] = 16^w P made ahead (k_ct_pow16), digit position w contributes d_w * pow[w], d_w in [-8, 8]: the lane of
// position w walks 1 pow[w], 2 pow[w], .. 8 pow[w] by seven additions and keeps the one its digit names under an arithmetic mask
// (all eight are computed whatever the digit; zero keeps the neutral element), the sign is a select, and the 64 positions are
// summed by a tree.  No table, no address and no branch that depends on the scalar; what follows the scalar on the call's
// critical path is 7 + 1 additions and a 6-level tree instead of 252 doublings and 64 additions.
BPP_HD void ct_pos_multiple(ge &out, const ge &pw, int32_t digit) {
  uint32_t mag, neg;
  ct_digit_parts(mag, neg, digit);
  ge m = pw, sel;
  ge_identity(sel);
#pragma unroll 1
  for (uint32_t k = 1; k <= 8; k++) {
    if (k > 1) ge_add(m, m, pw);
    ge c = m;  // (carried limbs: what the mask keeps must be valid limbs of ONE multiple)
    fe_carry(c.X);
    fe_carry(c.Y);
    fe_carry(c.Z);
    fe_carry(c.T);
    const uint32_t keep = 0u - (((k ^ mag) - 1u) >> 31);  // all ones iff k == mag
#pragma unroll
    for (int q = 0; q < 10; q++) {
      sel.X.v[q] = (c.X.v[q] & keep) | (sel.X.v[q] & ~keep);
      sel.Y.v[q] = (c.Y.v[q] & keep) | (sel.Y.v[q] & ~keep);
      sel.Z.v[q] = (c.Z.v[q] & keep) | (sel.Z.v[q] & ~keep);
      sel.T.v[q] = (c.T.v[q] & keep) | (sel.T.v[q] & ~keep);
    }
  }
  fe_cneg_select(sel.X, sel.X, neg);
  fe_cneg_select(sel.T, sel.T, neg);
  out = sel;
}
// one lane's model of the whole product (host probe): pow[w] by doublings, then the sum over the positions
BPP_HD void ct_var_scalarmul(ge &r, const ge &p, const sc &s) {
  int8_t d[BPP_CT_DIGITS];
  ct_recode16(d, s);
  ge pw = p, acc;
  ge_identity(acc);
  for (int w = 0; w < BPP_CT_DIGITS; w++) {
    if (w)
      for (int k = 0; k < 4; k++) ge_dbl(pw, pw);
    ge q;
    ct_pos_multiple(q, pw, d[w]);
    ge_add(acc, acc, q);
  }
  r = acc;
}

// ---- MANY terms with secret scalars over the caller's own points (seam B1's MultiscalarMul::multiscalar_mul, bpp_msm_ct): Straus.
// Per term the multiples 1 P .. 8 P (carried limbs; made by additions of a PUBLIC point), per digit position four doublings of ONE
// accumulator shared by the terms, then one addition per term of the entry its digit names: all eight entries read, one kept
// under a mask, a zero digit keeps none and becomes the neutral element (0, 1, 1, 0) by a mask as well, the sign is a select.
#define BPP_CTS_ENTRIES 8  // 1 P .. 8 P
// coordinate `coord` (0..3 = X, Y, Z, T; public) of the signed entry that `digit` names.  table = word 0 of that coordinate of entry 1 P,
// the entries `row_stride` words apart, a coordinate's limbs `word_stride` apart.
BPP_HD void ct_straus_coord(fe &out, const uint32_t *table, uint32_t row_stride, uint32_t word_stride, int32_t digit, uint32_t coord) {
  uint32_t mag, neg;
  ct_digit_parts(mag, neg, digit);
  uint32_t w[10];
  ct_select_words<10, BPP_CTS_ENTRIES>(w, table, row_stride, mag, 1, word_stride);
  const uint32_t isz = (mag - 1u) >> 31;                                     // 1 iff the digit is zero
  const uint32_t yz = (((coord ^ 1u) - 1u) | ((coord ^ 2u) - 1u)) >> 31;     // 1 iff the coordinate is Y or Z
  w[0] |= isz & yz;
  fe mine;
#pragma unroll
  for (int k = 0; k < 10; k++) mine.v[k] = w[k];
  // -P = (-X, Y, Z, -T)
  const uint32_t xt = (((coord ^ 0u) - 1u) | ((coord ^ 3u) - 1u)) >> 31;     // 1 iff the coordinate is X or T
  fe_cneg_select(out, mine, neg & xt);
}
// one lane's model of the whole sum (host probe, and the definition k_ct_straus is held to): blocks of 16 terms, each block one
// accumulator, the blocks' sums added in order.  n = 0: the neutral element.
#define BPP_CTS_MODEL_BLOCK 16
BPP_HD void ct_straus_model(ge &r, const ge *pts, const sc *scal, uint32_t n) {
  ge total;
  ge_identity(total);
  uint32_t tab[BPP_CTS_MODEL_BLOCK][BPP_CTS_ENTRIES][4][10];  // [term][entry][coordinate][limb]
  int8_t dig[BPP_CTS_MODEL_BLOCK][BPP_CT_DIGITS];
  for (uint32_t at = 0; at < n; at += BPP_CTS_MODEL_BLOCK) {
    const uint32_t cnt = n - at < BPP_CTS_MODEL_BLOCK ? n - at : BPP_CTS_MODEL_BLOCK;
    for (uint32_t t = 0; t < cnt; t++) {
      ge m = pts[at + t];
      for (int j = 0; j < BPP_CTS_ENTRIES; j++) {
        if (j) ge_add(m, m, pts[at + t]);
        ge c = m;
        fe_carry(c.X);
        fe_carry(c.Y);
        fe_carry(c.Z);
        fe_carry(c.T);
        for (int k = 0; k < 10; k++) {
          tab[t][j][0][k] = c.X.v[k];
          tab[t][j][1][k] = c.Y.v[k];
          tab[t][j][2][k] = c.Z.v[k];
          tab[t][j][3][k] = c.T.v[k];
        }
      }
      ct_recode16(dig[t], scal[at + t]);
    }
    ge acc;
    ge_identity(acc);
    for (int i = BPP_CT_DIGITS - 1; i >= 0; i--) {
      if (i != BPP_CT_DIGITS - 1)
        for (int k = 0; k < 4; k++) ge_dbl(acc, acc);
      for (uint32_t t = 0; t < cnt; t++) {
        ge q;
        ct_straus_coord(q.X, &tab[t][0][0][0], 40, 1, (int32_t)dig[t][i], 0);
        ct_straus_coord(q.Y, &tab[t][0][1][0], 40, 1, (int32_t)dig[t][i], 1);
        ct_straus_coord(q.Z, &tab[t][0][2][0], 40, 1, (int32_t)dig[t][i], 2);
        ct_straus_coord(q.T, &tab[t][0][3][0], 40, 1, (int32_t)dig[t][i], 3);
        ge_add(acc, acc, q);
      }
    }
    ge_add(total, total, acc);
  }
  // the digits are secret-derived (volatile stores: a plain loop over a dying array is dropped)
  for (size_t k = 0; k < sizeof(dig); k++) ((volatile int8_t *)dig)[k] = 0;
  r = total;
}

// the canonicity of a scalar without a branch or an early exit: 1 iff s < l, by the borrow of s - l over the eight words
BPP_HD uint32_t ct_sc_is_canonical(const sc &s) {
  const uint32_t l[8] = {BPP_L0, BPP_L1, BPP_L2, BPP_L3, BPP_L4, BPP_L5, BPP_L6, BPP_L7};
  uint64_t borrow = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) borrow = (((uint64_t)s.v[i] - l[i] - borrow) >> 63) & 1u;
  return (uint32_t)borrow;
}

#if defined(__HIPCC__)
#define CTF_MAX_TERMS 8
struct CtFixedShared {
  int8_t dig[CTF_MAX_TERMS][BPP_CT_DIGITS];
  ge red[64];
};
// out[o] = sum_{i < count[o]} scal[o][i] * Base[bidx[o][i] - idx_off], count[o] <= CTF_MAX_TERMS: one wavefront per output, lane w
// owns digit position w of every term.  `tbl` = [base][64][8] lines (k_fb_build with 4-bit windows).
__global__ void __launch_bounds__(64) k_ct_fixed(const sc *__restrict__ scal, const uint32_t *__restrict__ bidx,
                                                 const uint32_t *__restrict__ count, uint32_t stride, uint32_t idx_off,
                                                 const niels *__restrict__ tbl, ge *__restrict__ out) {
  const uint32_t o = blockIdx.x, lane = threadIdx.x;
  const uint32_t n = count[o] < CTF_MAX_TERMS ? count[o] : CTF_MAX_TERMS;
  __shared__ CtFixedShared sh;
  if (lane < CTF_MAX_TERMS) {  // (lanes beyond the output's terms recode its first term again: the same instructions, unused digits)
    const sc s = scal[(size_t)o * stride + (lane < n ? lane : 0u)];
    ct_recode16(sh.dig[lane], s);
  }
  __syncthreads();
  ge acc;
  ge_identity(acc);
#pragma unroll 1
  for (uint32_t i = 0; i < n; i++) {  // the number of terms is public
    const uint32_t b = bidx[(size_t)o * stride + i] - idx_off;
    niels q;
    ct_fixed_select(q, tbl + ((size_t)b * BPP_CT_DIGITS + lane) * BPP_CTF_ENTRIES, (int32_t)sh.dig[i][lane]);
    ge_madd(acc, acc, q);
  }
  sh.red[lane] = acc;
  __syncthreads();
  for (uint32_t off = 32; off >= 1; off >>= 1) {
    if (lane < off) {
      ge x = sh.red[lane], y2 = sh.red[lane + off];
      ge_add(x, x, y2);
      sh.red[lane] = x;
    }
    __syncthreads();
  }
  if (lane == 0) out[o] = sh.red[0];
  __syncthreads();
  for (uint32_t k = lane; k < sizeof(CtFixedShared) / 4; k += 64) ((uint32_t *)&sh)[k] = 0;  // digits and partial sums are secret-derived
}

// pow[pt][w] = 16^w * pts[pt], w = 0..63: one quad per point (msm.h's quad doubling), 252 dependent doublings of PUBLIC points
__global__ void __launch_bounds__(64) k_ct_pow16(const ge *__restrict__ pts, uint32_t n_pts, ge *__restrict__ pow) {
  const uint32_t lane = threadIdx.x, qi = lane & 3u;
  uint32_t pt = blockIdx.x * 16u + (lane >> 2);
  const bool live = pt < n_pts;
  if (!live) pt = n_pts - 1;  // (idle quads walk the last point again and store nothing)
  const QuadMask q = quad_mask(qi);
  const ge p = pts[pt];
  fe m;
  quad_load(m, q, p);
#pragma unroll 1
  for (uint32_t w = 0; w < BPP_CT_DIGITS; w++) {
    if (w) {
#pragma unroll 1
      for (int k = 0; k < 4; k++) quad_ge_dbl(m, q);
    }
    fe c = m;
    fe_carry(c);
    if (live) {
      uint32_t *dst = reinterpret_cast<uint32_t *>(pow + (size_t)pt * BPP_CT_DIGITS + w) + 10u * qi;  // coordinate qi of the entry
#pragma unroll
      for (int k = 0; k < 10; k++) dst[k] = c.v[k];
    }
  }
}

// prod[p * nt + v] = scal(p, v) * pts[p * nt + v], the points given as their multiples pow[p * nt + v][w] = 16^w pts[..]
// (k_ct_pow16): one wavefront per term, lane w owns digit position w (ct_pos_multiple), a six-level tree at the end.
// scal(p, v): rows of `row_stride` scalars per proof, term v at word 8 + (v & 7) of row v >> 3 (the prover's final-step rows).
struct CtVarShared {
  int8_t dig[BPP_CT_DIGITS];
  ge red[64];
};
__global__ void __launch_bounds__(64) k_ct_var(const ge *__restrict__ pow, const sc *__restrict__ scal, uint32_t row_stride, uint32_t nt,
                                               ge *__restrict__ prod) {
  const uint32_t p = blockIdx.x / nt, v = blockIdx.x - p * nt, w = threadIdx.x;
  __shared__ CtVarShared sh;
  if (w == 0) {
    const sc s = scal[((size_t)2 * p + (v >> 3)) * row_stride + 8u + (v & 7u)];
    ct_recode16(sh.dig, s);
  }
  __syncthreads();
  const ge pw = pow[((size_t)p * nt + v) * BPP_CT_DIGITS + w];
  ge mine;
  ct_pos_multiple(mine, pw, (int32_t)sh.dig[w]);
  sh.red[w] = mine;
  __syncthreads();
  for (uint32_t off = 32; off >= 1; off >>= 1) {
    if (w < off) {
      ge x = sh.red[w], y2 = sh.red[w + off];
      ge_add(x, x, y2);
      sh.red[w] = x;
    }
    __syncthreads();
  }
  if (w == 0) prod[(size_t)p * nt + v] = sh.red[0];
  __syncthreads();
  for (uint32_t k = w; k < sizeof(CtVarShared) / 4; k += 64) ((uint32_t *)&sh)[k] = 0;  // digits and partial sums are secret-derived
}
// acc[acc_stride * p] += sum_{v < nt} prod[p * nt + v]: one lane per proof (nt <= 16 additions in a row)
__global__ void __launch_bounds__(64) k_ct_sum(const ge *__restrict__ prod, uint32_t nt, uint32_t n_proofs, ge *__restrict__ acc,
                                               uint32_t acc_stride) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_proofs) return;
  ge x = acc[(size_t)acc_stride * p];
  for (uint32_t v = 0; v < nt; v++) {
    const ge y2 = prod[(size_t)p * nt + v];
    ge_add(x, x, y2);
  }
  acc[(size_t)acc_stride * p] = x;
}

// ---- the constant-time multiscalar multiplication of seam B1 (bpp_msm_ct): one chunk (ct_plan.h) of one output per workgroup of
// 64 lanes.  Quad t owns the terms t, 16 + t, .. (K of them at most: its SLOTS) of the chunk and ONE accumulator: per digit position
// four doublings, shared by the K terms, then K additions of selected entries (ct_straus_coord) -- what ct_straus_model does for
// the terms of a quad.  A slot beyond the chunk's count (public) runs the same instruction stream on the chunk's first scalar with
// the neutral element for its point, and so adds nothing.
//
// LDS layout: the lane is the FASTEST index of the table, tab[slot][entry][limb][lane].  Every lane reads its own coordinate of
// its own quad's term, all lanes the same (entry, limb) at a time: the 32 lanes that share an LDS cycle of a ds_read_b32 read 32
// consecutive words, one per bank -- no conflict, for the 80 reads of every addition.  The digits lie
// [slot][position][quad]: the 16 quads read 16 adjacent bytes, four words, each a broadcast.
// K = 1: 20 KB of table, 24 KB in all; K = 2: 40 KB of table, 45 KB in all.
template <int K>
struct CtStrausShared {
  uint32_t tab[K][BPP_CTS_ENTRIES][10][64];
  int8_t dig[K][BPP_CT_DIGITS][BPP_CT_QUADS];
  ge part[BPP_CT_QUADS];
};
// part[c] = sum over the terms i of chunk c of scal[i] * pts[i]; pts = affine Niels entries (k_decompress_plain)
template <int K>
__global__ void __launch_bounds__(64) k_ct_straus(const sc *__restrict__ scal, const niels *__restrict__ pts,
                                                  const CtChunk *__restrict__ plan, ge *__restrict__ part) {
  static_assert(K >= 1 && K <= BPP_CT_K_MAX, "kernel form");
  static_assert(sizeof(CtStrausShared<K>) <= 64 * 1024, "static LDS of one workgroup");
  const uint32_t lane = threadIdx.x, qi = lane & 3u, quad = lane >> 2;
  const QuadMask q = quad_mask(qi);
  const CtChunk ch = plan[blockIdx.x];
  __shared__ CtStrausShared<K> sh;
  fe d2, one;
  fe_const(d2, FE_D2);
  fe_1(one);
  fe m;
#pragma unroll 1
  for (uint32_t s = 0; s < (uint32_t)K; s++) {
    const uint32_t idx = s * BPP_CT_QUADS + quad;
    const bool active = idx < ch.count;  // (public)
    const uint32_t term = ch.first + (active ? idx : 0u);
    ge p;
    {
      const niels b = pts[term];
      ge_from_niels(p, b);
    }
    if (!active) ge_identity(p);
    // multiples 1 P .. 8 P by public additions, coordinate qi of every entry written by lane qi with carried limbs
    quad_load(m, q, p);
#pragma unroll 1
    for (uint32_t j = 0; j < BPP_CTS_ENTRIES; j++) {
      if (j) quad_ge_add(m, q, p, d2, one);
      fe c = m;
      fe_carry(c);
#pragma unroll
      for (int k = 0; k < 10; k++) sh.tab[s][j][k][lane] = c.v[k];
    }
    if (qi == 0) {
      const sc sv = scal[term];
      int8_t d[BPP_CT_DIGITS];
      ct_recode16(d, sv);
#pragma unroll
      for (int i = 0; i < BPP_CT_DIGITS; i++) sh.dig[s][i][quad] = d[i];
    }
  }
  __syncthreads();
  {
    ge id;
    ge_identity(id);
    quad_load(m, q, id);
  }
#pragma unroll 1
  for (int i = BPP_CT_DIGITS - 1; i >= 0; i--) {
    if (i != BPP_CT_DIGITS - 1) {
#pragma unroll 1
      for (int k = 0; k < 4; k++) quad_ge_dbl(m, q);
    }
#pragma unroll 1
    for (uint32_t s = 0; s < (uint32_t)K; s++) {
      fe mine;
      ct_straus_coord(mine, &sh.tab[s][0][0][lane], 10u * 64u, 64u, (int32_t)sh.dig[s][i][quad], qi);
      ge other;
      quad_gather(other, mine);
      quad_ge_add(m, q, other, d2, one);
    }
  }
  // the 16 quads' sums by a tree of four levels (every quad takes part in every chunk: an idle one holds the neutral element)
  ge acc;
  quad_gather(acc, m);
  if (qi == 0) sh.part[quad] = acc;
#pragma unroll 1
  for (uint32_t off = BPP_CT_QUADS / 2; off >= 1; off >>= 1) {
    __syncthreads();
    if (quad < off) {
      const ge y2 = sh.part[quad + off];
      quad_ge_add(m, q, y2, d2, one);
      quad_gather(acc, m);
      if (qi == 0) sh.part[quad] = acc;
    }
  }
  if (lane == 0) part[blockIdx.x] = acc;
  // digits, selected multiples and partial sums are secret-derived: leave nothing in LDS for the next workgroup on this CU
  __syncthreads();
  for (uint32_t k = lane; k < sizeof(CtStrausShared<K>) / 4; k += 64) ((uint32_t *)&sh)[k] = 0;
}

// R[g] = the sum of the partial sums of group g's chunks, part[chunk_off[g]] .. part[chunk_off[g + 1] - 1], in an order that the
// (public) chunk count alone decides: one workgroup per group, lane l adds the chunks l, l + 64, .., then a tree over the first
// `span` lanes, span = the power of two that covers the count (one chunk, the commitment shape: no tree at all).  A group
// without chunks gives the neutral element.
struct CtSumShared {
  ge red[64];
};
__global__ void __launch_bounds__(64) k_ct_straus_sum(const ge *__restrict__ part, const uint32_t *__restrict__ chunk_off,
                                                      ge *__restrict__ R) {
  const uint32_t g = blockIdx.x, lane = threadIdx.x;
  const uint32_t lo = chunk_off[g], n = chunk_off[g + 1] - lo;
  uint32_t span = 1;
  while (span < n && span < 64u) span <<= 1;
  __shared__ CtSumShared sh;
  ge acc;
  ge_identity(acc);
  if (lane < n) acc = part[lo + lane];
  for (uint32_t c = lane + 64u; c < n; c += 64u) {
    const ge y2 = part[lo + c];
    ge_add(acc, acc, y2);
  }
  sh.red[lane] = acc;
  __syncthreads();
  for (uint32_t off = span >> 1; off >= 1; off >>= 1) {
    if (lane < off) {
      ge x = sh.red[lane], y2 = sh.red[lane + off];
      ge_add(x, x, y2);
      sh.red[lane] = x;
    }
    __syncthreads();
  }
  if (lane == 0) R[g] = sh.red[0];
  __syncthreads();
  for (uint32_t k = lane; k < sizeof(CtSumShared) / 4; k += 64) ((uint32_t *)&sh)[k] = 0;  // partial sums are secret-derived
}
#endif

}  // namespace bpp
