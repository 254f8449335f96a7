// pairbatch_check.cpp -- the batch planner of host/pairbatch.hpp (the one gpu/abi_align.hip cuts
// every pair list with), without a GPU and without either library:
//   * two hand-worked lists with their boundaries and uniq lists written as numbers: every kind
//     of batch end, a read shared by two minus pairs, a 0-length record, and a minus string that
//     alone exceeds the byte cap (no other string joins it)
//   * random lists (m <= 200 pairs over 12 points of length 0 .. 100; a_minus null, all ones or
//     mixed) under pairs {1, 2, 7, 1000} x bytes {16, 48, 160, 1 << 20} x scratch {off, twice the
//     largest single need, 1 << 30} with scratch_of = la * lb + 64, against restate() below, a
//     literal restatement of the rule: equal boundaries, uniq lists and slots
//   * the properties: the batches tile [0, m) in order and none is empty; a batch of more than one
//     pair respects the pair and the scratch cap, one of more than one string the byte cap (the
//     rule takes the first string of a batch whatever its size, and plus pairs may follow it);
//     every batch is maximal (the next pair would have broken a cap); the slots of a batch are
//     distinct, dense and in order of first appearance, and forgotten by the next batch
// Header only.  Prints "OK", or says what failed.
#include <algorithm>
#include <cstdio>
#include <random>
#include <vector>

#include "pairbatch.hpp"

static int fail(const char *what, long v = 0) {
  printf("FAIL: %s (%ld)\n", what, v);
  return 1;
}

struct Batch {
  uint64_t i0, i1;
  std::vector<uint32_t> uniq;
  bool operator==(const Batch &o) const { return i0 == o.i0 && i1 == o.i1 && uniq == o.uniq; }
};

struct List {
  std::vector<uint64_t> off;  // n + 1
  std::vector<uint32_t> a, b;
  std::vector<uint8_t> minus;  // empty: a_minus NULL
  uint64_t len(uint32_t id) const { return off[id + 1] - off[id]; }
  bool is_minus(uint64_t i) const { return !minus.empty() && minus[i]; }
};

static uint64_t pad16(uint64_t l) { return (l + 15) / 16 * 16; }
static uint64_t scratch_of(uint64_t la, uint64_t lb) { return la * lb + 64; }

// the rule, word for word: no slot table, the batch's strings are looked up in its uniq list
static std::vector<Batch> restate(const List &L, mc::PairBatchCaps caps) {
  std::vector<Batch> out;
  const uint64_t m = L.a.size();
  for (uint64_t i0 = 0; i0 < m;) {
    Batch bt{i0, i0, {}};
    uint64_t scratch = 0, bytes = 0;
    while (bt.i1 < m && bt.i1 - i0 < caps.pairs) {
      const uint64_t i = bt.i1, la = L.len(L.a[i]), lb = L.len(L.b[i]);
      if (caps.scratch && i > i0 && scratch + scratch_of(la, lb) > caps.scratch) break;
      if (L.is_minus(i) && std::find(bt.uniq.begin(), bt.uniq.end(), L.a[i]) == bt.uniq.end()) {
        if (!bt.uniq.empty() && bytes + pad16(la) > caps.bytes) break;
        bytes += pad16(la);
        bt.uniq.push_back(L.a[i]);
      }
      scratch += scratch_of(la, lb);
      bt.i1++;
    }
    out.push_back(bt);
    i0 = bt.i1;
  }
  return out;
}

// the planner's batches, with the slot checks made while each batch is the current one
static int planned(const List &L, mc::PairBatchCaps caps, std::vector<Batch> &out) {
  const uint64_t m = L.a.size(), n = L.off.size() - 1;
  mc::PairBatcher pb(L.off.data(), n, L.a.data(), L.b.data(), L.minus.empty() ? nullptr : L.minus.data(), m, caps, scratch_of);
  out.clear();
  std::vector<uint32_t> before;
  while (pb.next()) {
    for (size_t r = 0; r < pb.uniq.size(); r++)
      if (pb.slot(pb.uniq[r]) != r) return fail("a slot is not its read's place in uniq", (long)pb.i0);
    std::vector<uint32_t> seen;  // the minus reads in order of first appearance
    for (uint64_t i = pb.i0; i < pb.i1; i++) {
      if (pb.minus(i) != L.is_minus(i)) return fail("minus()", (long)i);
      if (!L.is_minus(i)) continue;
      if (std::find(seen.begin(), seen.end(), L.a[i]) == seen.end()) seen.push_back(L.a[i]);
      if (pb.slot(L.a[i]) >= pb.uniq.size() || pb.uniq[pb.slot(L.a[i])] != L.a[i]) return fail("a minus pair's slot", (long)i);
    }
    if (seen != pb.uniq) return fail("uniq is not the minus reads in order of first appearance", (long)pb.i0);
    uint64_t nminus = 0;
    for (uint64_t i = pb.i0; i < pb.i1; i++) nminus += L.is_minus(i);
    if (pb.nminus != nminus) return fail("nminus", (long)pb.i0);
    for (uint32_t id : before)
      if (std::find(seen.begin(), seen.end(), id) == seen.end() && pb.slot(id) != mc::PairBatcher::NO_SLOT)
        return fail("a slot outlived its batch", (long)pb.i0);
    before = pb.uniq;
    out.push_back({pb.i0, pb.i1, pb.uniq});
  }
  return 0;
}

static int properties(const List &L, mc::PairBatchCaps caps, const std::vector<Batch> &bs) {
  const uint64_t m = L.a.size();
  uint64_t at = 0;
  for (const Batch &bt : bs) {
    if (bt.i0 != at || bt.i1 <= bt.i0 || bt.i1 > m) return fail("the batches do not tile the list", (long)bt.i0);
    at = bt.i1;
    uint64_t scratch = 0, bytes = 0;
    for (uint64_t i = bt.i0; i < bt.i1; i++) scratch += scratch_of(L.len(L.a[i]), L.len(L.b[i]));
    for (uint32_t id : bt.uniq) bytes += pad16(L.len(id));
    std::vector<uint32_t> u(bt.uniq);
    std::sort(u.begin(), u.end());
    if (std::adjacent_find(u.begin(), u.end()) != u.end()) return fail("a read with two slots", (long)bt.i0);
    if (bt.i1 - bt.i0 > caps.pairs) return fail("the pair cap", (long)bt.i0);
    if (bt.i1 - bt.i0 > 1 && caps.scratch && scratch > caps.scratch) return fail("the scratch cap", (long)bt.i0);
    if (bt.uniq.size() > 1 && bytes > caps.bytes) return fail("the byte cap", (long)bt.i0);
    if (bt.i1 == m) continue;
    // maximal: pair i1 would have broken a cap
    const uint64_t i = bt.i1, la = L.len(L.a[i]), lb = L.len(L.b[i]);
    const bool by_pairs = bt.i1 - bt.i0 == caps.pairs;
    const bool by_scratch = caps.scratch && scratch + scratch_of(la, lb) > caps.scratch;
    const bool by_bytes = L.is_minus(i) && std::find(bt.uniq.begin(), bt.uniq.end(), L.a[i]) == bt.uniq.end() &&
                          !bt.uniq.empty() && bytes + pad16(la) > caps.bytes;
    if (!by_pairs && !by_scratch && !by_bytes) return fail("a batch that could have taken one more pair", (long)bt.i0);
  }
  if (at != m) return fail("the batches end before the list", (long)at);
  return 0;
}

static int hand_worked() {
  // six points of 10, 20, 33, 0, 100 and 16 bytes: 16, 32, 48, 0, 112 and 16 when padded
  List L;
  L.off = {0, 10, 30, 63, 63, 163, 179};
  L.a = {0, 1, 1, 5, 2, 3, 0, 4, 5, 2, 0};
  L.b.assign(L.a.size(), 0);
  L.minus = {1, 1, 1, 0, 1, 1, 1, 1, 1, 0, 1};
  std::vector<Batch> got;
  // 4 pairs, 48 bytes: [0,4) ends at the pair cap with read 1 in one slot; [4,6) holds 48 + 0 bytes and ends
  // before read 0's 16; [6,7) ends before read 4's 112; read 4 is alone, whatever its size; the rest fits
  if (planned(L, {4, 48, 0}, got)) return 1;
  const std::vector<Batch> want{{0, 4, {0, 1}}, {4, 6, {2, 3}}, {6, 7, {0}}, {7, 8, {4}}, {8, 11, {5, 0}}};
  if (!(got == want)) return fail("the hand-worked list, byte cap");
  // scratch 600 against la * 10 + 64 = 164, 264, 394, 64, 1064, 224 for reads 0 .. 5: pair 7 (1064) alone
  if (planned(L, {1000, 1 << 20, 600}, got)) return 1;
  const std::vector<Batch> want2{{0, 2, {0, 1}}, {2, 4, {1}}, {4, 6, {2, 3}}, {6, 7, {0}}, {7, 8, {4}}, {8, 9, {5}}, {9, 11, {0}}};
  if (!(got == want2)) return fail("the hand-worked list, scratch cap");
  // a_minus NULL: the pair cap alone
  L.minus.clear();
  if (planned(L, {4, 16, 0}, got)) return 1;
  const std::vector<Batch> want3{{0, 4, {}}, {4, 8, {}}, {8, 11, {}}};
  if (!(got == want3)) return fail("the hand-worked list, all plus");
  // no pairs: no batch
  L.a.clear();
  L.b.clear();
  if (planned(L, {4, 16, 0}, got) || !got.empty()) return fail("an empty list");
  return 0;
}

int main() {
  if (hand_worked()) return 1;
  std::mt19937 rng(7);
  long byte_ends = 0, scratch_ends = 0, shared = 0;
  for (int rep = 0; rep < 30; rep++) {
    List L;
    L.off.push_back(0);
    for (int p = 0; p < 12; p++) L.off.push_back(L.off.back() + (p == 0 ? 0 : rng() % 101));  // (always one empty record)
    const uint64_t m = rep == 0 ? 1 : 1 + rng() % 200;
    uint64_t big = 0;
    for (uint64_t i = 0; i < m; i++) {
      L.a.push_back(rng() % 12);
      L.b.push_back(rng() % 12);
      big = std::max(big, scratch_of(L.len(L.a[i]), L.len(L.b[i])));
    }
    for (int mode = 0; mode < 3; mode++) {
      L.minus.clear();
      for (uint64_t i = 0; mode > 0 && i < m; i++) L.minus.push_back(mode == 1 ? 1 : (uint8_t)(rng() % 2 ? rng() % 255 + 1 : 0));
      for (uint64_t pairs : {(uint64_t)1, (uint64_t)2, (uint64_t)7, (uint64_t)1000})
        for (uint64_t bytes : {(uint64_t)16, (uint64_t)48, (uint64_t)160, (uint64_t)1 << 20})
          for (uint64_t scratch : {(uint64_t)0, 2 * big, (uint64_t)1 << 30}) {
            const mc::PairBatchCaps caps{pairs, bytes, scratch};
            std::vector<Batch> got;
            if (planned(L, caps, got)) return 1;
            if (!(got == restate(L, caps))) return fail("the planner differs from the rule", rep);
            if (properties(L, caps, got)) return 1;
            for (const Batch &bt : got) {  // (what the sweep reached, checked below)
              uint64_t nminus = 0, scr = 0;
              for (uint64_t i = bt.i0; i < bt.i1; i++) {
                nminus += L.is_minus(i);
                scr += scratch_of(L.len(L.a[i]), L.len(L.b[i]));
              }
              shared += nminus > bt.uniq.size();
              if (bt.i1 < m && bt.i1 - bt.i0 < pairs) {
                if (scratch && scr + scratch_of(L.len(L.a[bt.i1]), L.len(L.b[bt.i1])) > scratch) scratch_ends++;
                else byte_ends++;
              }
            }
          }
    }
  }
  if (byte_ends < 1000 || scratch_ends < 1000 || shared < 1000) return fail("the sweep did not reach every kind of batch", byte_ends);
  printf("OK\n");
  return 0;
}
