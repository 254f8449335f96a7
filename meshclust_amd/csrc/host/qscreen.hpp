// qscreen.hpp -- an exact q-gram bound that decides "identity below the cutoff" without aligning.
//
// Lemma.  Let a global alignment of strings a and b have L columns, I of them identity columns
// (both bytes equal; nw.hip: identity = I / L), and let C_q(a, b) = sum over q-grams g of
// min(occ_a(g), occ_b(g)) be the multiset q-gram intersection.  Then
//     C_q >= q * I - (q - 1) * L - (q - 1).
// Proof.  (1) The L - I other columns cut the identity columns into at most L - I + 1 runs.
// (2) A run of r identity columns gives max(0, r - q + 1) >= r - q + 1 equal q-grams, at distinct
// starts in both strings, so C_q >= I - (q - 1) * (L - I + 1), which is the claim.
// (3) With m = max(la, lb) <= L and kappa = 1 - q * (1 - c) > 0: C_q + q + 1 < kappa * m gives
// C_q + (q - 1) * (L + 1) + 2 < c * q * L, so I / L <= (C_q + (q - 1) * (L + 1)) / (q * L) < c - 2 / (q * L):
// strictly below the cutoff c, by far more than the rounding of the quotient can move it.
//
// The bound holds for every alignment, so for the one NW picks.  Trainer::split's binary search
// reads only the side of the cutoff an identity lies on: a pair with below() true takes the
// "< cutoff" branch without being aligned.  Header-only: the CPU test harness
// links a fixed list of host objects.  The device count is mc_qgram_common (gpu/qgram.hip).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "fasta.hpp"

namespace mc {
namespace qscreen {

constexpr uint32_t NA = 0xffffffffu;  // the count is not available: the pair is aligned
constexpr int QMAX = 7, QMIN = 4;

// the largest q <= QMAX with q * (1 - c) <= 0.75 (kappa >= 0.25); below QMIN the screen is off (0)
inline int pick_q(double c) {
  for (int q = QMAX; q >= QMIN; q--)
    if ((double)q * (1.0 - c) <= 0.75) return q;
  return 0;
}

// the theorem's premise, with one more unit of margin than it needs and <=: the product's
// rounding (one part in 2^53) is far inside that unit
inline bool below(uint32_t C, uint64_t la, uint64_t lb, double c, int q) {
  return C != NA && (double)((uint64_t)C + (uint64_t)q + 2) <= (1.0 - (double)q * (1.0 - c)) * (double)std::max(la, lb);
}

// read i's expanded bytes are all 0..3: no exception byte, and its segments cover it whole
inline bool pure(const Dataset &ds, uint32_t i) {
  const uint64_t s = ds.seq_off[i], e = ds.seq_off[i + 1];
  const auto it = std::lower_bound(ds.exc_pos.begin(), ds.exc_pos.end(), s);
  if (it != ds.exc_pos.end() && *it < e) return false;
  uint64_t covered = 0;
  for (uint64_t g = ds.seg_off[i]; g < ds.seg_off[i + 1]; g++) covered += (uint64_t)(ds.seg[2 * g + 1] - ds.seg[2 * g] + 1);
  return covered == e - s;
}

// calls f(g) for every q-gram of read i (1 <= q <= 15) in order, g in 0 .. 4^q - 1 with the first
// base lowest; minus: the q-grams of the read's minus-strand string (host/revseq.hpp), in reverse
// order (the multiset is what counts)
template <typename F>
inline void grams(const Dataset &ds, uint32_t i, bool minus, int q, F f) {
  const uint64_t len = ds.seq_off[i + 1] - ds.seq_off[i];
  const uint32_t *w = ds.packed.data() + ds.pk_off[i];
  const uint32_t mask = (1u << (2 * q)) - 1;
  uint32_t fw = 0, rc = 0;  // the window ending at j, and its reverse complement
  for (uint64_t j = 0; j < len; j++) {
    const uint32_t d = (w[j >> 4] >> (2 * (j & 15))) & 3u;
    fw = (fw >> 2) | (d << (2 * (q - 1)));
    rc = ((rc << 2) | (3u - d)) & mask;
    if (j + 1 >= (uint64_t)q) f(minus ? rc : fw);
  }
}

// C_q of the byte strings mc_nw_identity_strands would align for (a, b, minus): a (its minus-strand
// string where minus) against b; NA unless both are pure and at least q long
inline uint32_t common(const Dataset &ds, uint32_t a, uint32_t b, bool minus, int q) {
  if (q < 1 || q > QMAX) return NA;
  const uint64_t la = ds.seq_off[a + 1] - ds.seq_off[a], lb = ds.seq_off[b + 1] - ds.seq_off[b];
  if (la < (uint64_t)q || lb < (uint64_t)q || !pure(ds, a) || !pure(ds, b)) return NA;
  static thread_local std::vector<uint32_t> occ;  // all zero between calls
  occ.resize((size_t)1 << (2 * QMAX), 0);
  grams(ds, a, minus, q, [&](uint32_t g) { occ[g]++; });
  uint32_t c = 0;
  grams(ds, b, false, q, [&](uint32_t g) {
    if (occ[g]) {
      occ[g]--;
      c++;
    }
  });
  grams(ds, a, minus, q, [&](uint32_t g) { occ[g] = 0; });
  return c;
}

}  // namespace qscreen
}  // namespace mc
