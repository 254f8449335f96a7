// profile.hpp -- a cluster's consensus from the column profile of its multiple alignment alone
// (mc_nw_msa_counts, include/meshclust_amd.h; native check tests/native/profile_check.cpp).
//
// A centre of L bytes with W columns of MC_MSA_CH counters: channels 0..4 the pair rows' bytes by
// class, 5 the rows with a gap, 6 the centre position or site r, 7 zero for the column of a centre
// base and t + 1 for slot t of a site.  The columns come in order: the w[0] slots of site 0, base 0,
// the w[1] slots of site 1, base 1, .. , the w[L] slots of site L.  depth, the number of pairs, is
// the sum of channels 0..5 of any column.
//
// consensus_from_profile returns what consensus_of (consensus.hpp) returns from the pile-up rows and
// the reads' inserted bytes, byte for byte and field for field.  The derivation is exact:
//   - consensus_of applies a site iff 2 * (pile-up channel 6 of row r) > depth.  A pair has at most
//     one 'I' run per row, so channel 6 counts the pairs with a run at r, which are the rows that
//     hold a base in slot 0: depth - gap count of slot 0.  A site with w[r] = 0 has no run and no
//     slot; consensus_of applies nothing there either.
//   - Runs are left-justified, so nongap(slot t) -- the sum of channels 0..4 -- is the number of
//     runs longer than t.  The runs of length exactly l number nongap(slot l - 1) - nongap(slot l)
//     (nongap(slot w[r]) = 0).  consensus_of takes the most frequent length, ties to the shortest:
//     the same scan over l = 1 .. w[r] in ascending order, keeping the first maximum.
//   - Base t of the insertion is the plurality class among the runs longer than t: channels 0..4 of
//     slot t are exactly those per-class counts, ties to the lowest class as there.  Under quality
//     the per-class weights are wcounts' channels 0..4 of slot t (the sum of Qs(i + t) over the same
//     runs): the largest weight, then the larger count, then the lowest class (qconsensus_pick with
//     no own class), and the quality is qconsensus_quality over those five weights.
//   - The centre's columns hold the pile-up's channels 0..5 as they stand (counts and weights), so
//     consensus_channel / qconsensus_pick / qconsensus_quality are called on them unchanged.
// Depth 0 keeps the centre, as consensus_of does.
#pragma once
#include "consensus.hpp"

namespace mc {

namespace profile_detail {

// the slots of the site in front of column c: [c, end) while channel 7 is nonzero -> end
inline uint64_t site_end(const uint32_t *counts, uint64_t c, uint64_t W) {
  while (c < W && counts[c * MC_MSA_CH + 7] != 0) c++;
  return c;
}

inline uint64_t nongap(const uint32_t *col) { return (uint64_t)col[0] + col[1] + col[2] + col[3] + col[4]; }

// the modal run length of the site whose slots are columns [s0, s1): 0 if the site is not applied
inline uint64_t site_length(const uint32_t *counts, uint64_t s0, uint64_t s1, uint64_t depth) {
  if (s1 == s0 || 2 * (depth - counts[s0 * MC_MSA_CH + 5]) <= depth) return 0;
  uint64_t len = 0, most = 0;
  for (uint64_t t = s0; t < s1; t++) {
    const uint64_t longer = t + 1 < s1 ? nongap(counts + (t + 1) * MC_MSA_CH) : 0;
    const uint64_t exact = nongap(counts + t * MC_MSA_CH) - longer;
    if (exact > most) {
      most = exact;
      len = t - s0 + 1;
    }
  }
  return len;
}

inline uint64_t depth_of(const uint32_t *counts, uint64_t W) { return W ? nongap(counts) + counts[5] : 0; }

}  // namespace profile_detail

// centre: its L expanded bytes; counts: the W columns of its block
inline Consensus consensus_from_profile(const uint8_t *centre, uint64_t L, uint64_t W, const uint32_t *counts) {
  using namespace profile_detail;
  Consensus c;
  c.seq.reserve(L + 16);
  const uint64_t depth = depth_of(counts, W);
  if (depth == 0) {
    for (uint64_t r = 0; r < L; r++) c.seq += pileup_base_char(centre[r]);
    return c;
  }
  uint64_t at = 0;  // the column the walk stands at
  for (uint64_t r = 0; r <= L; r++) {
    const uint64_t s0 = at, s1 = site_end(counts, at, W);
    at = s1;
    const uint64_t len = site_length(counts, s0, s1, depth);
    for (uint64_t t = 0; t < len; t++) {
      const uint32_t *col = counts + (s0 + t) * MC_MSA_CH;
      uint32_t best = 0;
      for (uint32_t k = 1; k < 5; k++)
        if (col[k] > col[best]) best = k;
      c.seq += "ACGTN"[best];
    }
    if (len) c.ins++;
    if (r == L || at >= W) break;
    const uint32_t ch = consensus_channel(counts + at * MC_MSA_CH, centre[r]);
    at++;
    if (ch == 5) {
      c.del++;
      continue;
    }
    const char x = "ACGTN"[ch];
    if (x != pileup_base_char(centre[r])) c.sub++;
    c.seq += x;
  }
  return c;
}

// the same from counts and wcounts: what qconsensus_of returns
inline QConsensus qconsensus_from_profile(const uint8_t *centre, uint64_t L, uint64_t W, const uint32_t *counts,
                                          const uint32_t *wcounts) {
  using namespace profile_detail;
  QConsensus c;
  c.seq.reserve(L + 16);
  c.qual.reserve(L + 16);
  const uint64_t depth = depth_of(counts, W);
  if (depth == 0) {
    for (uint64_t r = 0; r < L; r++) c.seq += pileup_base_char(centre[r]);
    c.qual.assign(L, '!');
    return c;
  }
  uint64_t at = 0;
  for (uint64_t r = 0; r <= L; r++) {
    const uint64_t s0 = at, s1 = site_end(counts, at, W);
    at = s1;
    const uint64_t len = site_length(counts, s0, s1, depth);
    for (uint64_t t = 0; t < len; t++) {
      uint64_t w[5], n[5];
      for (uint32_t k = 0; k < 5; k++) {
        w[k] = wcounts[(s0 + t) * MC_MSA_CH + k];
        n[k] = counts[(s0 + t) * MC_MSA_CH + k];
      }
      const uint32_t win = qconsensus_pick(w, n, 5, 5);
      c.seq += "ACGTN"[win];
      c.qual += qconsensus_quality(w, 5, win);
    }
    if (len) c.ins++;
    if (r == L || at >= W) break;
    uint64_t w[6], n[6];
    for (uint32_t k = 0; k < 6; k++) {
      w[k] = wcounts[at * MC_MSA_CH + k];
      n[k] = counts[at * MC_MSA_CH + k];
    }
    at++;
    const uint32_t ch = qconsensus_pick(w, n, 6, pileup_channel(centre[r]));
    if (ch == 5) {
      c.del++;
      continue;
    }
    const char x = "ACGTN"[ch];
    if (x != pileup_base_char(centre[r])) c.sub++;
    c.seq += x;
    c.qual += qconsensus_quality(w, 6, ch);
  }
  return c;
}

}  // namespace mc
