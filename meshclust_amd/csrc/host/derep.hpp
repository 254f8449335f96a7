// derep.hpp -- dereplication of points: the host side of mc_derep (include/meshclust_amd.h,
// DESIGN.md 3.17).  Header-only and free of the GPU: the device entry (gpu/derep.hip), the tool
// (derep_main.cpp) and the native check (tests/native/derep_check.cpp) share it.
//
// Two points are duplicates if their expanded byte strings are equal; with both strands also if one
// equals the other's minus-strand string (revseq.hpp).  rc_byte is an involution, so this is an
// equivalence relation, and comparing against one member of a class decides membership.
//
//   derep_host     the contract of mc_derep on the CPU: rep[i] = the smallest position whose point
//                  is a duplicate of ids[i]'s, minus[i] = 0 where the strings are equal as written
//                  (this wins), else 1.  It is no fallback of mc_derep (the ABI has none): it is what
//                  the native check compares against a brute force and what the benchmark times.
//   DerepPlanner   what mc_derep does between its kernels: candidate groups from the fingerprints,
//                  the (member, leader) pairs of a compare round, and the regrouping of the members
//                  that matched neither way.  Any keys give the same classes; equal strings must
//                  have equal keys (with both strands: a string and its minus strand too).
//   derep_classes  the classes in output order: size descending, then first position ascending.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <unordered_map>
#include <vector>

#include "revseq.hpp"

namespace mc {

struct DerepKey {  // a 128-bit fingerprint, compared hi first
  uint64_t hi, lo;
};
inline bool operator==(const DerepKey &a, const DerepKey &b) { return a.hi == b.hi && a.lo == b.lo; }
inline bool operator<(const DerepKey &a, const DerepKey &b) { return a.hi != b.hi ? a.hi < b.hi : a.lo < b.lo; }

// the first `bits` (0 .. 128) bits of a key, the rest cleared (MC_DEREP_HASH_BITS: 0 sends every
// point of one length into one group)
inline DerepKey derep_key_bits(DerepKey k, int bits) {
  if (bits >= 128) return k;
  if (bits <= 0) return DerepKey{0, 0};
  if (bits <= 64) return DerepKey{bits == 64 ? k.hi : k.hi & ~(~0ull >> bits), 0};
  return DerepKey{k.hi, k.lo & ~(~0ull >> (bits - 64))};
}

// bit 0: a == b as written; bit 1 (both only): a equals b's minus-strand string.  What the compare
// kernel returns for a pair of equal length.
inline uint8_t derep_compare(const uint8_t *a, const uint8_t *b, size_t len, bool both) {
  uint8_t r = memcmp(a, b, len) == 0 ? 1 : 0;
  if (both) {
    size_t j = 0;
    while (j < len && a[j] == rc_byte(b[len - 1 - j])) j++;
    if (j == len) r |= 2;
  }
  return r;
}

struct DerepPlanner {
  std::vector<uint32_t> rep;
  std::vector<uint8_t> minus;
  // the open round's pairs: position mem[p] is compared with its group's leader lead[p]; the pairs
  // of one group are adjacent and in ascending position
  std::vector<uint32_t> mem, lead;
  uint64_t pairs = 0, rounds = 0, collisions = 0;

  // groups = the runs of equal (key, length) among the positions sorted by (key, length, position);
  // a group's first position is its leader
  void begin(const DerepKey *keys, const uint64_t *lens, uint64_t m) {
    rep.resize(m);
    minus.assign(m, 0);
    mem.clear();
    lead.clear();
    pairs = rounds = collisions = 0;
    std::vector<uint32_t> pos(m);
    std::iota(pos.begin(), pos.end(), 0u);
    std::sort(pos.begin(), pos.end(), [&](uint32_t x, uint32_t y) {
      if (!(keys[x] == keys[y])) return keys[x] < keys[y];
      if (lens[x] != lens[y]) return lens[x] < lens[y];
      return x < y;
    });
    uint32_t leader = 0;
    for (uint64_t t = 0; t < m; t++) {
      const uint32_t p = pos[t];
      if (t == 0 || !(keys[p] == keys[leader]) || lens[p] != lens[leader]) {
        leader = p;
        rep[p] = p;
      } else {
        mem.push_back(p);
        lead.push_back(leader);
      }
    }
  }

  bool open() const { return !mem.empty(); }

  // res[p]: the compare result of pair p of the open round.  A member that matched is settled; those
  // that matched neither way are collisions: within their group the first becomes a leader, the
  // others its members in the next round.  Every round settles at least one position per open group.
  void settle(const uint8_t *res) {
    std::vector<uint32_t> nmem, nlead;
    rounds++;
    pairs += mem.size();
    uint32_t old_leader = 0, new_leader = 0;
    bool has_new = false;
    for (size_t p = 0; p < mem.size(); p++) {
      if (p == 0 || lead[p] != old_leader) {
        old_leader = lead[p];
        has_new = false;
      }
      const uint32_t q = mem[p];
      if (res[p] & 1) {
        rep[q] = old_leader;
        minus[q] = 0;
      } else if (res[p] & 2) {
        rep[q] = old_leader;
        minus[q] = 1;
      } else {
        collisions++;
        if (!has_new) {
          has_new = true;
          new_leader = q;
          rep[q] = q;
          minus[q] = 0;
        } else {
          nmem.push_back(q);
          nlead.push_back(new_leader);
        }
      }
    }
    mem.swap(nmem);
    lead.swap(nlead);
  }
};

namespace derep_detail {

// s < rc(s) decides the orientation a class is keyed by: flip = the minus-strand string is the
// lexicographically smaller one (a string that is its own minus strand is not flipped)
inline bool flipped(const uint8_t *s, size_t len) {
  for (size_t j = 0; j < len; j++) {
    const uint8_t a = s[j], b = rc_byte(s[len - 1 - j]);
    if (a != b) return b < a;
  }
  return false;
}

inline uint64_t mix(uint64_t x) {
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdull;
  x ^= x >> 29;
  return x;
}

// a 64-bit hash of the string in the orientation `flip` selects (the map's bucket only: equality is
// decided on the bytes)
inline uint64_t hash_oriented(const uint8_t *s, size_t len, bool flip) {
  uint64_t h = 0x9e3779b97f4a7c15ull ^ len;
  size_t j = 0;
  if (!flip) {
    for (; j + 8 <= len; j += 8) {
      uint64_t w;
      memcpy(&w, s + j, 8);
      h = mix(h ^ w) * 0x9fb21c651e98df25ull;
    }
    for (; j < len; j++) h = (h ^ s[j]) * 0x100000001b3ull;
  } else {
    for (; j + 8 <= len; j += 8) {
      uint64_t w = 0;
      for (int b = 0; b < 8; b++) w |= (uint64_t)rc_byte(s[len - 1 - j - b]) << (8 * b);
      h = mix(h ^ w) * 0x9fb21c651e98df25ull;
    }
    for (; j < len; j++) h = (h ^ rc_byte(s[len - 1 - j])) * 0x100000001b3ull;
  }
  return mix(h);
}

}  // namespace derep_detail

// The contract of mc_derep on the host.  both: strands == 3.  minus may be null when !both.
// The orientation and the bucket hash of every position are computed in parallel where OpenMP is on;
// the classes are then formed by one thread in position order.
inline void derep_host(const uint8_t *codes, const uint64_t *seq_off, const uint32_t *ids, uint64_t m, bool both, uint32_t *rep,
                       uint8_t *minus) {
  using namespace derep_detail;
  std::vector<uint8_t> flip(m, 0);
  std::vector<uint64_t> hash(m);
#pragma omp parallel for schedule(dynamic, 256)
  for (int64_t i = 0; i < (int64_t)m; i++) {
    const uint8_t *s = codes + seq_off[ids[i]];
    const size_t len = seq_off[ids[i] + 1] - seq_off[ids[i]];
    flip[i] = both && flipped(s, len);
    hash[i] = hash_oriented(s, len, flip[i]);
  }
  // bucket hash -> the first position of the last class seen with it; `chain` links the classes
  // that share a hash (a 64-bit collision between different strings)
  std::unordered_map<uint64_t, uint32_t> first;
  first.reserve(m);
  std::vector<uint32_t> chain(m, UINT32_MAX);
  for (uint64_t i = 0; i < m; i++) {
    const uint8_t *s = codes + seq_off[ids[i]];
    const size_t len = seq_off[ids[i] + 1] - seq_off[ids[i]];
    auto it = first.find(hash[i]);
    uint32_t r = UINT32_MAX;
    if (it != first.end())
      for (uint32_t c = it->second; c != UINT32_MAX; c = chain[c]) {
        const uint8_t *t = codes + seq_off[ids[c]];
        const size_t tl = seq_off[ids[c] + 1] - seq_off[ids[c]];
        if (tl != len) continue;
        // equal in their keyed orientations: as written if both are flipped alike, else across
        const uint8_t want = flip[i] == flip[c] ? 1 : 2;
        if (ids[c] == ids[i] || (derep_compare(s, t, len, want == 2) & want)) {
          r = c;
          break;
        }
      }
    if (r == UINT32_MAX) {
      rep[i] = (uint32_t)i;
      if (minus) minus[i] = 0;
      if (it != first.end()) {
        chain[i] = it->second;
        it->second = (uint32_t)i;
      } else {
        first.emplace(hash[i], (uint32_t)i);
      }
    } else {
      rep[i] = r;
      if (minus) minus[i] = flip[i] != flip[r];
    }
  }
}

// The classes of rep[0 .. m) (rep[rep[i]] == rep[i]) in output order: size descending, then first
// position ascending.  first[c]: the class's representative position, size[c]: its members.
inline void derep_classes(const uint32_t *rep, uint64_t m, std::vector<uint32_t> &first, std::vector<uint64_t> &size) {
  std::vector<uint64_t> count(m, 0);
  for (uint64_t i = 0; i < m; i++) count[rep[i]]++;
  first.clear();
  for (uint64_t i = 0; i < m; i++)
    if (rep[i] == i) first.push_back((uint32_t)i);
  std::stable_sort(first.begin(), first.end(), [&](uint32_t x, uint32_t y) { return count[x] > count[y]; });
  size.resize(first.size());
  for (size_t c = 0; c < first.size(); c++) size[c] = count[first[c]];
}

}  // namespace mc
