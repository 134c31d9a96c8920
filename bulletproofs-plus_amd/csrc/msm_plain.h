// A deliberately plain variable-time multiscalar multiplication on gfx950: the verifier's second opinion.
//
// Every form of the engine's MSM (msm.h) shares the digit recoding, the counting sort, the bucket kernels, the window
// reduction and the plan logic.  This file shares NONE of it: its only includes are field.h and point.h.  No bucket, no sort,
// no recoded digit stream, no plan -- one lane per term runs the schoolbook left-to-right double-and-add over the 253 bits of
// its scalar.  It is ~30 times the work of the bucket method per term and is meant for the rare call that has something to
// confirm ("verify_check", engine.hip: verify_flow) and for tests ("msm_plain" = 1 sends the B1 entry points through it).
//
// Replaces (reference boundary): the same calls as msm.h -- vartime_mixed_multiscalar_mul (src/range_proof.rs:1050-1057) and
// vartime_multiscalar_mul (:482-495, :512-521).  Variable time is right here: these scalars are public (DESIGN 4.3, row
// bpp_msm_vartime).
//
// Inputs are the ones msm.h's kernels get, before any half-scalar split: canonical scalars (eight 32-bit words each, little
// endian), the term lists (term_sidx: scalar index; term_pidx: point index, bit 31 = the term is subtracted), the group offsets
// group_off[0..G], the two point tables as affine-Niels 128-byte lines (index < n_a: table A, else table B), and `list`, the
// ids of the groups to evaluate: cost is proportional to the groups asked for.
//
//   k_msm_plain      grid (waves_max, n_list) x 64 lanes: wavefront (x, y) owns terms [64 x, 64 x + 64) of group list[y] -- a
//                    wavefront never straddles two groups -- and leaves their sum in part[y * waves_max + x]
//   k_msm_plain_sum  grid n_list x 64 lanes: the partials of group list[y] added in index order into R[list[y]], with the
//                    identity flag the verifier's tail reads.  No atomics anywhere: the result is a fixed function of the input
#pragma once
#include "field.h"
#include "point.h"

namespace bpp {

#define BPP_PLAIN_SCALAR_BITS 253u  // canonical scalars are below l < 2^253

// the 64 values of a wavefront summed by a tree through LDS (64 x 160 B); the sum ends in sh[0]
__device__ __forceinline__ void plain_wave_tree(ge *sh, const ge &mine, uint32_t lane) {
  sh[lane] = mine;
  __syncthreads();
  for (uint32_t s = 32; s >= 1; s >>= 1) {
    if (lane < s) {
      ge a = sh[lane];
      const ge b = sh[lane + s];
      ge_add(a, a, b);
      sh[lane] = a;
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(64) k_msm_plain(const uint32_t *__restrict__ scalars, const uint32_t *__restrict__ term_sidx,
                                                  const uint32_t *__restrict__ term_pidx, const uint32_t *__restrict__ group_off,
                                                  const niels *__restrict__ tab_a, const niels *__restrict__ tab_b, uint32_t n_a,
                                                  const uint32_t *__restrict__ list, uint32_t waves_max, ge *__restrict__ part) {
  __shared__ ge sh[64];
  const uint32_t lane = threadIdx.x, g = list[blockIdx.y];
  const uint32_t t0 = group_off[g], t1 = group_off[g + 1];
  if (t1 - t0 <= 64u * blockIdx.x) return;  // (the whole wavefront: this group has fewer terms than the largest one asked for)
  const uint32_t t = t0 + 64u * blockIdx.x + lane;
  const bool in = t < t1;
  ge acc;
  ge_identity(acc);
  if (in) {
    uint32_t k[8];
    const uint32_t *sp = scalars + 8 * (size_t)term_sidx[t];
#pragma unroll
    for (int i = 0; i < 8; i++) k[i] = sp[i];
    const uint32_t pi = term_pidx[t], idx = pi & 0x7fffffffu;
    const bool neg = (pi >> 31) != 0;
    niels q;
    niels_load_swapped(q, idx < n_a ? tab_a + idx : tab_b + (idx - n_a), neg);  // the sign is applied by the swapped load
    // left to right: nothing happens above the scalar's top bit (variable time: public scalars)
    int top = -1;
    for (int i = 7; i >= 0 && top < 0; i--)
      if (k[i]) top = 32 * i + 31 - __builtin_clz(k[i]);
    if (top >= (int)BPP_PLAIN_SCALAR_BITS) top = (int)BPP_PLAIN_SCALAR_BITS - 1;  // (never for a canonical scalar)
    for (int i = top; i >= 0; i--) {
      ge_dbl(acc, acc);
      uint32_t w = k[0];  // word i / 32 by selects: a dynamic index would send k[] to scratch memory
#pragma unroll
      for (int j = 1; j < 8; j++) w = (i >> 5) == j ? k[j] : w;
      if ((w >> (i & 31)) & 1u) ge_madd_swapped(acc, acc, q, neg);
    }
  }
  plain_wave_tree(sh, acc, lane);
  if (lane == 0) part[(size_t)blockIdx.y * waves_max + blockIdx.x] = sh[0];
}

// one wavefront per group of the list: lane l adds a contiguous run of the group's partials in index order, the tree joins
// neighbouring runs, so the whole sum is taken in index order
__global__ void __launch_bounds__(64) k_msm_plain_sum(const ge *__restrict__ part, const uint32_t *__restrict__ group_off,
                                                      const uint32_t *__restrict__ list, uint32_t waves_max, ge *__restrict__ R,
                                                      uint32_t *__restrict__ is_identity) {
  __shared__ ge sh[64];
  const uint32_t lane = threadIdx.x, g = list[blockIdx.x];
  const uint32_t n_w = (group_off[g + 1] - group_off[g] + 63u) / 64u;  // partials k_msm_plain wrote for this group (<= waves_max)
  const uint32_t per = (n_w + 63u) / 64u;
  const ge *p = part + (size_t)blockIdx.x * waves_max;
  ge acc;
  ge_identity(acc);
  for (uint32_t j = 0; j < per; j++) {
    const uint32_t i = lane * per + j;
    if (i < n_w) {
      const ge b = p[i];
      ge_add(acc, acc, b);
    }
  }
  plain_wave_tree(sh, acc, lane);
  if (lane == 0) {
    const ge r = sh[0];
    R[g] = r;
    is_identity[g] = ge_is_ristretto_identity(r) ? 1u : 0u;
  }
}

}  // namespace bpp
