// chimera.hpp -- which of a read's hits, beside its best one, explains the read better as the second
// parent of a chimera, chosen from mc_nw_msa_crossover's values; include/meshclust_amd.h, native check
// tests/native/chimera_check.cpp.
//
// A read's hits come in mc_assign_top's order.  Hit 1 (index 0) is the first parent x; the candidate
// second parents y are the later hits whose centre differs from hit 1's.  For a candidate with the
// eight values v of mc_nw_msa_crossover(x, y):
//   best = max(v[2], v[5])          the identities of the better two-parent model; on a tie the order
//                                   xy (x left of the cut, y right)
//   gain = best - max(v[0], v[1])   what the model adds over the better single parent, >= 0
// The read reports the candidate of largest gain, the earliest hit on a tie, and is flagged where that
// gain is min_gain or more.
#pragma once
#include <algorithm>
#include <cstdint>

#include "../../../include/meshclust_amd.h"

namespace mc {

struct ChimeraCall {
  int hit = -1;         // index of the second parent among the read's hits; -1: the read has no candidate
  bool xy = true;       // hit 1 is the left parent
  int32_t best = 0, gain = 0, cut_first = 0, cut_last = 0, ids_left = 0, ids_right = 0;
  bool flag = false;    // gain >= min_gain
};

// one candidate's values -> its call (hit and flag left to the caller)
inline ChimeraCall chimera_order(const int32_t *v) {
  ChimeraCall c;
  c.xy = v[2] >= v[5];
  c.best = c.xy ? v[2] : v[5];
  c.gain = c.best - std::max(v[0], v[1]);
  c.cut_first = c.xy ? v[3] : v[6];
  c.cut_last = c.xy ? v[4] : v[7];
  c.ids_left = c.xy ? v[0] : v[1];
  c.ids_right = c.xy ? v[1] : v[0];
  return c;
}

// centres: the n hits' centres in order -> how many candidates the read has; their hit indices,
// ascending, into cand (room for n)
inline uint32_t chimera_candidates(const uint32_t *centres, uint32_t n, uint32_t *cand) {
  uint32_t k = 0;
  for (uint32_t j = 1; j < n; j++)
    if (centres[j] != centres[0]) cand[k++] = j;
  return k;
}

// cand: k hit indices, ascending; res: their k * MC_CROSS_RES values -> the read's call
inline ChimeraCall chimera_pick(const uint32_t *cand, uint32_t k, const int32_t *res, int64_t min_gain) {
  ChimeraCall out;
  for (uint32_t t = 0; t < k; t++) {
    ChimeraCall c = chimera_order(res + (uint64_t)t * MC_CROSS_RES);
    if (out.hit < 0 || c.gain > out.gain) {
      c.hit = (int)cand[t];
      out = c;
    }
  }
  out.flag = out.hit >= 0 && (int64_t)out.gain >= min_gain;
  return out;
}

}  // namespace mc
