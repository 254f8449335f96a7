// strand.hpp -- the k-mer index of the other strand.
//
// A k-mer index is written first base most significant with A 0, C 1, G 2, T 3 (gpu/kmer.hip).
// The reverse complement of k-mer i is the k-mer whose base-4 digits are those of i in reverse
// order, each digit d replaced by 3 - d.  rc_index is an involution; at odd k it has no fixed
// point, at even k it has 4^(k/2).  Shared by the device permutation kernel (gpu/assign.hip)
// and the native host check (tests/native/strand_check.cpp).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define MC_STRAND_HD __host__ __device__
#else
#define MC_STRAND_HD
#endif

namespace mc {

MC_STRAND_HD inline uint32_t rc_index(uint32_t i, int k) {
  uint32_t r = 0;
  for (int d = 0; d < k; d++) {
    r = (r << 2) | (3u - (i & 3u));
    i >>= 2;
  }
  return r;
}

}  // namespace mc
