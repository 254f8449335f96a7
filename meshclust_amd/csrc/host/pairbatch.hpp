// pairbatch.hpp -- a list of m pairs (a[i], b[i]) cut into the batches the alignment entries run.
//
// A pair with a_minus[i] set is aligned on the minus strand of its seq1 (a_minus NULL: none is),
// and a batch keeps one minus-strand string per such read, padded to 16 bytes.  Start a batch at
// i0 and take pair i1 while i1 < m and i1 - i0 < caps.pairs, with two stops:
//   - caps.scratch != 0: stop before pair i1 when i1 > i0 and the batch's scratch plus
//     scratch_of(la, lb) would exceed caps.scratch (scratch_at(i1) where it is set: a need that
//     the two lengths do not give, the width of mc_nw_msa_rows' row i1);
//   - pair i1 is minus and its read has no slot in this batch yet: stop before it when the batch
//     already holds a minus string and its padded bytes plus (la + 15) / 16 * 16 would exceed
//     caps.bytes.
// So every batch holds at least one pair, and a pair or a string that alone exceeds a cap is taken
// alone.  A read of several minus pairs of one batch has one slot; slots are numbered in order of
// first appearance and forgotten when the next batch begins.  Shared by gpu/abi_align.hip and the
// native host check (tests/native/pairbatch_check.cpp).
#pragma once
#include <algorithm>
#include <cstdint>
#include <functional>
#include <vector>

namespace mc {

struct PairBatchCaps {
  uint64_t pairs, bytes, scratch;  // pairs, padded bytes of minus strings, scratch bytes (0: no scratch rule)
};

class PairBatcher {
 public:
  static constexpr uint32_t NO_SLOT = 0xffffffffu;
  using ScratchOf = std::function<uint64_t(uint64_t, uint64_t)>;

  // seq_off: the n + 1 record offsets; b and scratch_of may be empty when caps.scratch is 0
  PairBatcher(const uint64_t *seq_off, uint64_t n, const uint32_t *a, const uint32_t *b, const uint8_t *a_minus, uint64_t m,
              PairBatchCaps caps, ScratchOf scratch_of = nullptr)
      : off_(seq_off), a_(a), b_(b), minus_(a_minus), m_(m), caps_(caps), scratch_of_(scratch_of) {
    caps_.pairs = std::max<uint64_t>(caps_.pairs, 1);
    if (a_minus) slot_.assign(n, NO_SLOT);
  }

  uint64_t i0 = 0, i1 = 0;     // the current batch, [i0, i1)
  uint64_t nminus = 0;         // its minus pairs
  std::vector<uint32_t> uniq;  // the reads whose minus-strand strings it needs: uniq[slot(id)] == id
  std::function<uint64_t(uint64_t)> scratch_at;  // if set: pair i's scratch, in place of scratch_of (b may then be empty)

  uint64_t length(uint32_t id) const { return off_[id + 1] - off_[id]; }
  bool minus(uint64_t i) const { return minus_ && minus_[i]; }
  uint32_t slot(uint32_t id) const { return slot_[id]; }  // of a read of a minus pair of the current batch

  bool next() {  // the batch after the current one; false after the last (whose slots nobody reads any more)
    if (i1 >= m_) return false;
    for (uint32_t id : uniq) slot_[id] = NO_SLOT;
    uniq.clear();
    i0 = i1;
    nminus = 0;
    uint64_t pad = 0, scr = 0;
    while (i1 < m_ && i1 - i0 < caps_.pairs) {
      const uint64_t la = length(a_[i1]);
      const uint64_t need = !caps_.scratch ? 0 : scratch_at ? scratch_at(i1) : scratch_of_(la, length(b_[i1]));
      if (caps_.scratch && i1 > i0 && scr + need > caps_.scratch) break;
      const bool is_minus = minus(i1);
      if (is_minus && slot_[a_[i1]] == NO_SLOT) {
        const uint64_t bytes = (la + 15) / 16 * 16;
        if (!uniq.empty() && pad + bytes > caps_.bytes) break;
        pad += bytes;
        slot_[a_[i1]] = (uint32_t)uniq.size();
        uniq.push_back(a_[i1]);
      }
      nminus += is_minus;
      scr += need;
      i1++;
    }
    return true;
  }

 private:
  const uint64_t *off_;
  const uint32_t *a_, *b_;
  const uint8_t *minus_;
  uint64_t m_;
  PairBatchCaps caps_;
  ScratchOf scratch_of_;
  std::vector<uint32_t> slot_;  // point id -> its string's slot in the current batch
};

}  // namespace mc
