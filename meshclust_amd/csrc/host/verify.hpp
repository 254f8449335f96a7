// verify.hpp -- meshclust-assign --min-identity X: which candidate of a read the alignment confirms.
//
// A read's candidates are its hits in mc_assign_top's order (combo 0 descending, plus before
// minus, centre index ascending; one candidate without --top), each with the identity of its
// alignment.  The read goes to the FIRST candidate whose identity is at least X: the rank
// decides, not the identity, so of two candidates with equal identities the better-ranked one is
// taken, and a lower-ranked candidate of higher identity is not preferred to a qualifying one
// above it.  X = 0 confirms rank 1 (an identity is never negative).  Shared by host/assign.cpp
// and the native host check (tests/native/verify_check.cpp).
#pragma once
#include <cstdint>

namespace mc {

// ident[0 .. n): the candidates' identities in rank order -> the confirmed rank (from 0), or -1
// when none qualifies (n = 0 included)
inline int verify_pick(const double *ident, uint32_t n, double x) {
  for (uint32_t t = 0; t < n; t++)
    if (ident[t] >= x) return (int)t;
  return -1;
}

}  // namespace mc
