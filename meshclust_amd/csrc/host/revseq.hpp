// revseq.hpp -- the minus-strand string of a point.
//
// A point's expanded byte string (what NW reads: 0..3 inside segments, 'N' or the raw upper-case
// byte outside, include/meshclust_amd.h mc_load_sequences) read backwards, every byte mapped by
// rc_byte: a digit d <= 3 becomes 3 - d, the raw letters swap 'A' <-> 'T' and 'C' <-> 'G' (a
// record without segments keeps its letters), every other byte ('N' included) stays.  rc_byte is
// an involution on all 256 values, so the minus strand of the minus strand is the string itself.
// Shared by the device kernel (gpu/revseq.hip) and the native host check
// (tests/native/revseq_check.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define MC_REVSEQ_HD __host__ __device__ inline
#else
#define MC_REVSEQ_HD inline
#endif

namespace mc {

MC_REVSEQ_HD uint8_t rc_byte(uint8_t d) {
  if (d <= 3) return (uint8_t)(3 - d);
  if (d == 'A') return 'T';
  if (d == 'T') return 'A';
  if (d == 'C') return 'G';
  if (d == 'G') return 'C';
  return d;
}

// four bytes at once, byte order kept: a word of digits only (the rule inside segments) is one xor
MC_REVSEQ_HD uint32_t rc_word(uint32_t w) {
  if ((w & 0xfcfcfcfcu) == 0) return w ^ 0x03030303u;
  uint32_t r = 0;
  for (int i = 0; i < 4; i++) r |= (uint32_t)rc_byte((uint8_t)(w >> (8 * i))) << (8 * i);
  return r;
}

// out[0 .. len) = the minus-strand string of src[0 .. len) (out and src do not overlap)
inline void revseq(const uint8_t *src, size_t len, uint8_t *out) {
  for (size_t i = 0; i < len; i++) out[i] = rc_byte(src[len - 1 - i]);
}

}  // namespace mc
