// band.hpp -- the geometry and the certificate of the banded choice record.
//
// A pair of la rows and lb columns, d = lb - la, scoring 1 / -1 / 2 / 1 as nw.hip.  For a width
// w >= 0 the band is the cells (i, j) with dlo <= j - i <= dhi, dlo = min(0, d) - w and
// dhi = max(0, d) + w.  The banded forward kernel (gpu/nwband.hip) works rows in blocks of BAND_ROWS;
// block k covers rows r0 = k BAND_ROWS + 1 .. r1 = min(la, (k + 1) BAND_ROWS) and sweeps the
// columns c0 = max(1, r0 + dlo) .. c1 = min(lb, r1 + dhi): a superset of the band's cells of those
// rows, fixed by (la, lb, w) alone.  Every block stores its choice words at the same stride of
// band_steps(la, lb, w) wave steps, so a pair's choice record is
//   band_choice_bytes = ceil(la / BAND_ROWS) * band_steps * 32 BAND_R  bytes.
// A path from (0, 0) to (la, lb) that leaves the band holds at least 2 (w + 1) + |d| gap columns in
// at least two runs, so it scores at most band_ub(la, lb, w); a banded score S above that bound
// and above NINF + min(la, lb) (what a path from a finite "-infinity" boundary state can reach) is
// the full matrix's score, and the chain of choices from it is the full matrix's chain.
// Shared by gpu/abi_align.hip, gpu/nwband.hip, gpu/nwtrace.hip (the full record's bytes) and the
// native host check (tests/native/band_check.cpp).
#pragma once
#include <algorithm>
#include <cstdint>

namespace mc {

#ifndef MC_BAND_R
#define MC_BAND_R 4  // (2, 4, 8 or 16: -DMC_BAND_R=<n> on every file is how DESIGN 3.13's block heights were measured)
#endif
constexpr int BAND_R = MC_BAND_R;       // rows per lane of the banded kernels
constexpr int BAND_ROWS = 64 * BAND_R;  // rows per block
constexpr int32_t BAND_SENTINEL = -(1 << 30);  // every state outside the region

// the full record (gpu/nwtrace.hip): rows per lane and choice bytes
inline int full_rows_per_lane(uint64_t la) { return la <= 256 ? 4 : la <= 512 ? 8 : 16; }
inline uint64_t full_choice_bytes(uint64_t la, uint64_t lb) {
  const uint64_t R = (uint64_t)full_rows_per_lane(la);
  return (la + 64 * R - 1) / (64 * R) * (lb + 63) * 32 * R;
}

inline int64_t band_neg_inf(int64_t la, int64_t lb) {  // nw.hip's finite "-infinity"
  const int64_t diff = la > lb ? la - lb : lb - la;
  return (diff >= 1 ? -2 - diff : 0) - std::min(la, lb) - 1;
}

// the best score of a path that leaves the band of width w
inline int64_t band_ub(int64_t la, int64_t lb, int64_t w) {
  const int64_t diff = la > lb ? la - lb : lb - la;
  return std::min(la, lb) - diff - 3 * (w + 1) - 4;
}

// (A) of the certificate: no path from a finite "-infinity" boundary state reaches S
inline bool band_above_ninf(int64_t la, int64_t lb, int64_t S) { return S > band_neg_inf(la, lb) + std::min(la, lb); }

// the banded score S at width w is certified: it is the full score, and so is the chain from it
inline bool band_certified(int64_t la, int64_t lb, int64_t w, int64_t S) {
  return band_above_ninf(la, lb, S) && S > band_ub(la, lb, w);
}

// the band of width w holds every cell of the matrix
inline bool band_is_whole(int64_t la, int64_t lb, int64_t w) { return w >= std::max(la, lb); }

// w*: the least width at which the exact score S satisfies (B)
inline int64_t band_need(int64_t la, int64_t lb, int64_t S) {
  const int64_t diff = la > lb ? la - lb : lb - la;
  const int64_t x = std::min(la, lb) - diff - 4 - S;
  return x <= 0 ? 0 : x / 3;
}

struct BandWindow {
  int64_t c0, c1;  // the columns block k sweeps
};
inline BandWindow band_window(int64_t la, int64_t lb, int64_t w, int64_t k) {
  const int64_t d = lb - la, dlo = std::min<int64_t>(0, d) - w, dhi = std::max<int64_t>(0, d) + w;
  const int64_t r0 = k * BAND_ROWS + 1, r1 = std::min(la, (k + 1) * BAND_ROWS);
  return {std::max<int64_t>(1, r0 + dlo), std::min(lb, r1 + dhi)};
}

// the columns a block sweeps at most, and the wave steps every block's choice words are strided by
inline uint64_t band_cols(uint64_t la, uint64_t lb, uint64_t w) {
  const uint64_t diff = la > lb ? la - lb : lb - la;
  return std::min<uint64_t>(lb, BAND_ROWS + diff + 2 * w);
}
inline uint64_t band_steps(uint64_t la, uint64_t lb, uint64_t w) { return band_cols(la, lb, w) + 63; }

inline uint64_t band_choice_bytes(uint64_t la, uint64_t lb, uint64_t w) {
  return (la + BAND_ROWS - 1) / BAND_ROWS * band_steps(la, lb, w) * 32 * BAND_R;
}

// ints of boundary row a pair of more than one block needs: 3 per column of a block's window
inline uint64_t band_bnd_ints(uint64_t la, uint64_t lb, uint64_t w) {
  return la > (uint64_t)BAND_ROWS ? 3 * (band_cols(la, lb, w) + 1) : 0;
}

// the planned width of a pair whose exact score is S: w*, or -1 (the full record) when a side is
// empty, (A) fails, or the band would need no fewer bytes than the full record
inline int32_t band_plan(int64_t la, int64_t lb, int64_t S) {
  if (la <= 0 || lb <= 0 || !band_above_ninf(la, lb, S)) return -1;
  const int64_t w = band_need(la, lb, S);
  if (w >= (1 << 27) || band_choice_bytes(la, lb, w) >= full_choice_bytes(la, lb)) return -1;
  return (int32_t)w;
}

}  // namespace mc
