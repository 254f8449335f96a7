// topk.hpp -- the K best hits of one query, kept in order while the hits arrive.
//
// A hit is (combo 0, centre index, strand: 0 plus, 1 minus).  The list is ordered by combo 0
// descending, then plus before minus, then index ascending.  Hits arrive with ascending index
// but, with both strands, not in that order (entry by entry: the plus pass, then the minus pass),
// so the position of a new hit is decided by an explicit comparison on (value, strand): it goes
// AFTER every entry that does not compare less than it.  Equal (value, strand) therefore stay in
// arrival order, which is index ascending.  The result is the first K of a stable sort of the
// whole stream by (value descending, strand ascending), whatever the capacity: a list of
// capacity 8 cut at K equals a list of capacity K.
//
//   TopK<K> + topk_insert   the list as a value: fixed trip counts and constant indices only, so
//                           on the device it unrolls into compares and selects on registers
//                           (assign_short_kernel, gpu/assign.hip); the strands are one bit mask
//   topk_insert_row         the list in three arrays in memory, capacity and fill at run time
//                           (assign_general_kernel keeps it in the query's output row; the host's
//                           pair-list path, host/assign.cpp)
// Shared by the device kernels and the native host check (tests/native/topk_check.cpp).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define MC_TOPK_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define MC_TOPK_HD inline
#endif

namespace mc {

constexpr uint32_t TOPK_NONE = 0xffffffffu;  // an empty slot's index (MC_ASSIGN_NONE)

template <int K>
struct TopK {
  double v[K];    // combo 0, -1.0 in an empty slot
  uint32_t j[K];  // centre index, TOPK_NONE in an empty slot
  uint32_t sm;    // bit i: the strand of slot i (0 in an empty slot)
  MC_TOPK_HD void clear() {
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < K; i++) {
      v[i] = -1.0;
      j[i] = TOPK_NONE;
    }
    sm = 0;
  }
  MC_TOPK_HD uint32_t strand(int i) const { return (sm >> i) & 1u; }
};

// entry (ev, es) stays in front of a new hit (nv, ns): it does not compare less
MC_TOPK_HD bool topk_keeps(double ev, uint32_t es, double nv, uint32_t ns) {
  return ev > nv || (ev == nv && es <= ns);
}

template <int K>
MC_TOPK_HD void topk_insert(TopK<K> &t, double nv, uint32_t nj, uint32_t ns) {
  static_assert(K >= 1 && K <= 31, "the strands are bits of one word");
  bool keep[K];  // slot i is filled and stays where it is (a prefix of the list: it is ordered)
  uint32_t p = 0;  // the new hit's slot, K if it does not make the list
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int i = 0; i < K; i++) {
    keep[i] = t.j[i] != TOPK_NONE && topk_keeps(t.v[i], t.strand(i), nv, ns);
    p += keep[i] ? 1u : 0u;
  }
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int i = K - 1; i >= 1; i--)
    if (!keep[i]) {  // slot i takes the new hit (the slot above stays) or the slot above
      t.v[i] = keep[i - 1] ? nv : t.v[i - 1];
      t.j[i] = keep[i - 1] ? nj : t.j[i - 1];
    }
  if (!keep[0]) {
    t.v[0] = nv;
    t.j[0] = nj;
  }
  if (p < (uint32_t)K) {  // the strand bits from p upwards move up by one, bit p is the new hit's
    const uint32_t low = (1u << p) - 1u;
    t.sm = ((t.sm & low) | ((ns & 1u) << p) | ((t.sm & ~low) << 1)) & ((1u << K) - 1u);
  }
}

// The same on a list in memory: v, j, s hold `cap` slots of which the first n (n <= cap) are
// filled.  Reads slots below n, writes slots below cap only.
MC_TOPK_HD void topk_insert_row(double *v, uint32_t *j, uint8_t *s, uint32_t cap, uint32_t n, double nv, uint32_t nj,
                                uint32_t ns) {
  uint32_t t = n;  // the slot the new hit would take
  while (t > 0) {
    const double pv = v[t - 1];
    const uint32_t pst = s[t - 1];
    if (topk_keeps(pv, pst, nv, ns)) break;
    if (t < cap) {
      v[t] = pv;
      j[t] = j[t - 1];
      s[t] = (uint8_t)pst;
    }
    t--;
  }
  if (t < cap) {
    v[t] = nv;
    j[t] = nj;
    s[t] = (uint8_t)ns;
  }
}

}  // namespace mc
