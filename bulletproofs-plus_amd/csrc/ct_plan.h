// The chunk plan of the constant-time multiscalar multiplication (ct.h: k_ct_straus<K>, engine.hip: bpp_msm_ct): every group of
// terms is cut into chunks of at most 16 K terms, one workgroup each.  A pure host function of the group offsets -- no HIP, no
// context, and above all no scalar: the plan, and with it the launch geometry, is made from public counts alone.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace bpp {

#define BPP_CT_QUADS 16  // quads of a 64-lane workgroup: terms per slot of a chunk
#define BPP_CT_K_MAX 2   // terms per quad of the widest kernel form

struct CtChunk {
  uint32_t group, first, count;  // terms [first, first + count) of the call, all of group `group`
};

// 0 and the plan in `chunks` (group order, then term order) with the chunks of group g at [chunk_off[g], chunk_off[g + 1]); -1 and
// nothing when the offsets do not start at 0, decrease, or end past n_terms, or K is no kernel form.  Empty groups make no chunk.
inline int ct_chunk_plan(const uint32_t *group_off, size_t n_groups, size_t n_terms, uint32_t K, std::vector<CtChunk> &chunks,
                         std::vector<uint32_t> &chunk_off) {
  chunks.clear();
  chunk_off.clear();
  if (!group_off || K < 1 || K > BPP_CT_K_MAX || group_off[0] != 0) return -1;
  for (size_t g = 0; g < n_groups; g++)
    if (group_off[g + 1] < group_off[g]) return -1;
  if ((size_t)group_off[n_groups] > n_terms) return -1;
  const uint32_t cap = BPP_CT_QUADS * K;
  chunk_off.reserve(n_groups + 1);
  for (size_t g = 0; g < n_groups; g++) {
    chunk_off.push_back((uint32_t)chunks.size());
    for (uint32_t at = group_off[g]; at < group_off[g + 1];) {
      const uint32_t left = group_off[g + 1] - at, take = left < cap ? left : cap;
      chunks.push_back(CtChunk{(uint32_t)g, at, take});
      at += take;
    }
  }
  chunk_off.push_back((uint32_t)chunks.size());
  return 0;
}

// The kernel form, from public counts: `largest` = the terms of the call's largest group, `chunks_k1` = the chunks the call has
// under K = 1; `forced` = the "msm_ct_k" option.  K = 2 halves the doublings per term and doubles the additions that follow one
// another in a workgroup: it pays only where a group has more than one slot's worth of terms and the chip is full either way.
// Measured: with groups of 32 terms K = 1 is ahead at 256 and at 1024 chunks, K = 2 at 1536, 2048 and 4096 -- the
// step lies at four K = 1 workgroups on each of the 256 compute units.
#define BPP_CT_K2_MIN_CHUNKS 1024
inline uint32_t ct_form_rule(uint32_t largest, uint64_t chunks_k1, int forced) {
  if (forced == 1 || forced == 2) return (uint32_t)forced;
  return (largest > BPP_CT_QUADS && chunks_k1 > BPP_CT_K2_MIN_CHUNKS) ? 2u : 1u;
}

}  // namespace bpp
