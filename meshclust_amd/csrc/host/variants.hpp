// variants.hpp -- the columns at which a cluster disagrees with itself, chosen from the column
// profile of its multiple alignment (mc_nw_msa_counts), and the distinct allele strings its reads
// carry there (mc_nw_msa_sites); include/meshclust_amd.h, native check tests/native/variants_check.cpp.
//
// A column of MC_MSA_CH counters has five alleles: channels 0..3 (A C G T) and channel 5 (the rows
// with a gap).  Channel 4, the bytes that are none of the four, is reported by the profile but is no
// allele.  With n[c] over c in {0, 1, 2, 3, 5}, D their sum and `second` the second largest of the
// five (the largest itself where two channels tie for it), the column is a variant site iff
//   second >= min_count   and   (double)second >= min_frac * (double)D
// so a column whose rows agree, or disagree only by class 4, is never one, and depth 0 gives none for
// any min_count >= 1.
#pragma once
#include <algorithm>
#include <cstdint>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../../include/meshclust_amd.h"

namespace mc {

// the second largest of a column's five allele counts and their sum
inline void allele_second(const uint32_t *col, uint64_t &second, uint64_t &D) {
  uint64_t first = 0;
  second = D = 0;
  for (uint32_t c : {0u, 1u, 2u, 3u, 5u}) {
    const uint64_t n = col[c];
    D += n;
    if (n > first) {
      second = first;
      first = n;
    } else if (n > second) {
      second = n;
    }
  }
}

// counts: one target's ncols columns of MC_MSA_CH counters -> its variant sites, ascending
inline std::vector<uint32_t> variant_sites(const uint32_t *counts, uint64_t ncols, double min_frac, uint64_t min_count) {
  std::vector<uint32_t> sites;
  for (uint64_t c = 0; c < ncols; c++) {
    uint64_t second, D;
    allele_second(counts + c * MC_MSA_CH, second, D);
    if (second >= min_count && (double)second >= min_frac * (double)D) sites.push_back((uint32_t)c);
  }
  return sites;
}

// alleles: depth strings of S bytes, one after the other -> the distinct strings seen min_count times
// or more with their counts, by count descending, then by bytes ascending
inline std::vector<std::pair<std::string, uint64_t>> haplotypes(const uint8_t *alleles, uint64_t depth, uint64_t S, uint64_t min_count) {
  std::map<std::string, uint64_t> seen;
  for (uint64_t k = 0; k < depth; k++) seen[std::string((const char *)alleles + k * S, S)]++;
  std::vector<std::pair<std::string, uint64_t>> out;
  for (const auto &kv : seen)
    if (kv.second >= min_count) out.push_back(kv);
  std::stable_sort(out.begin(), out.end(), [](const auto &x, const auto &y) { return x.second > y.second; });
  return out;
}

}  // namespace mc
