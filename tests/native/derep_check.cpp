// derep_check.cpp -- host/derep.hpp without a GPU:
//   derep_host against an O(m^2) brute force of the definition on seeded sets (short strings over few
//   bytes, so duplicates, minus-strand duplicates, strings that are their own minus strand and repeated
//   ids are all common), both strand modes;
//   DerepPlanner, driven with derep_compare where the device has its compare kernel, ending in the same
//   classes with keys cut to 0, 1, 4 and all 128 bits;
//   derep_classes' order, with ties.
// Prints "OK" and a census line, or the first difference (exit 1).
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "derep.hpp"

using namespace mc;

static int fail(const char *what, int set, uint64_t i) {
  printf("FAIL %s set %d position %llu\n", what, set, (unsigned long long)i);
  return 1;
}

int main() {
  std::mt19937_64 rng(20251);
  const uint8_t alphabet[] = {0, 1, 2, 3, 'N', 'A', 'T', 'C', 'G'};
  uint64_t census_dup = 0, census_minus = 0, census_self = 0, census_rounds = 0, census_coll = 0, census_repeat = 0;
  for (int set = 0; set < 300; set++) {
    const uint64_t n = 1 + rng() % 60;
    const int nsym = set % 3 == 0 ? 2 : (set % 3 == 1 ? 4 : 9);
    const uint64_t maxlen = set % 5 == 0 ? 40 : 5;
    std::vector<uint8_t> codes;
    std::vector<uint64_t> off{0};
    for (uint64_t p = 0; p < n; p++) {
      const uint64_t len = rng() % (maxlen + 1);
      const uint64_t mode = rng() % 4;
      if (p > 0 && mode == 0) {  // a copy or a minus-strand copy of an earlier point
        const uint64_t q = rng() % p;
        const uint64_t ql = off[q + 1] - off[q];
        std::vector<uint8_t> s(codes.begin() + off[q], codes.begin() + off[q + 1]), r(ql);
        if (rng() % 2) {
          revseq(s.data(), ql, r.data());
          s = r;
        }
        codes.insert(codes.end(), s.begin(), s.end());
      } else {
        for (uint64_t j = 0; j < len; j++) codes.push_back(alphabet[rng() % nsym]);
      }
      off.push_back(codes.size());
    }
    codes.resize(codes.size() + 16);
    const uint64_t m = rng() % (2 * n + 1);
    std::vector<uint32_t> ids(m);
    for (auto &v : ids) v = (uint32_t)(rng() % n);
    auto str = [&](uint64_t i) { return codes.data() + off[ids[i]]; };
    auto len = [&](uint64_t i) { return off[ids[i] + 1] - off[ids[i]]; };
    for (int both = 0; both < 2; both++) {
      // the definition, pair by pair
      std::vector<uint32_t> want(m);
      std::vector<uint8_t> wminus(m);
      for (uint64_t i = 0; i < m; i++) {
        want[i] = (uint32_t)i;
        wminus[i] = 0;
        for (uint64_t j = 0; j < i; j++) {
          if (len(j) != len(i)) continue;
          const uint8_t r = derep_compare(str(i), str(j), len(i), both != 0);
          if (r) {
            want[i] = (uint32_t)j;
            wminus[i] = (r & 1) ? 0 : 1;
            census_dup++;
            census_minus += wminus[i];
            census_self += r == 3 && len(i) > 0;
            census_repeat += ids[i] == ids[j];
            break;
          }
        }
      }
      std::vector<uint32_t> rep(m, 77);
      std::vector<uint8_t> minus(m, 77);
      derep_host(codes.data(), off.data(), ids.data(), m, both != 0, rep.data(), minus.data());
      for (uint64_t i = 0; i < m; i++)
        if (rep[i] != want[i] || minus[i] != wminus[i]) return fail(both ? "derep_host both" : "derep_host plus", set, i);
      if (!both) {  // minus may be null with one strand
        std::vector<uint32_t> rep2(m, 77);
        derep_host(codes.data(), off.data(), ids.data(), m, false, rep2.data(), nullptr);
        if (rep2 != rep) return fail("derep_host null minus", set, 0);
      }
      // the planner: keys that equal strings (and, with both strands, minus strands) share
      std::vector<DerepKey> full(m);
      std::vector<uint64_t> lens(m);
      for (uint64_t i = 0; i < m; i++) {
        const bool flip = both && derep_detail::flipped(str(i), len(i));
        const uint64_t h = derep_detail::hash_oriented(str(i), len(i), flip);
        full[i] = DerepKey{h, derep_detail::mix(h + 12345)};
        lens[i] = len(i);
      }
      for (int bits : {0, 1, 4, 128}) {
        std::vector<DerepKey> keys(m);
        for (uint64_t i = 0; i < m; i++) keys[i] = derep_key_bits(full[i], bits);
        DerepPlanner plan;
        plan.begin(keys.data(), lens.data(), m);
        uint64_t guard = 0;
        while (plan.open()) {
          std::vector<uint8_t> res(plan.mem.size());
          for (size_t p = 0; p < res.size(); p++) {
            if (plan.lead[p] >= plan.mem[p]) return fail("planner leader not first", set, p);
            res[p] = len(plan.mem[p]) == len(plan.lead[p]) ? derep_compare(str(plan.mem[p]), str(plan.lead[p]), len(plan.mem[p]), both != 0) : 0;
          }
          plan.settle(res.data());
          if (++guard > m + 1) return fail("planner does not end", set, 0);
        }
        for (uint64_t i = 0; i < m; i++)
          if (plan.rep[i] != want[i] || plan.minus[i] != wminus[i]) return fail("planner", set * 1000 + bits, i);
        if (bits == 0) {
          census_rounds += plan.rounds > 1;
          census_coll += plan.collisions;
        }
        if (bits == 128 && plan.collisions) return fail("planner: a 128-bit collision", set, 0);
      }
    }
  }
  {  // key bits
    const DerepKey k{0xfedcba9876543210ull, 0x0123456789abcdefull};
    if (!(derep_key_bits(k, 128) == k) || !(derep_key_bits(k, 0) == DerepKey{0, 0}) || !(derep_key_bits(k, 4) == DerepKey{0xf000000000000000ull, 0}) ||
        !(derep_key_bits(k, 64) == DerepKey{k.hi, 0}) || !(derep_key_bits(k, 72) == DerepKey{k.hi, 0x0100000000000000ull}))
      return fail("derep_key_bits", 0, 0);
  }
  {  // derep_classes: size descending, ties by first position
    const uint32_t rep[] = {0, 1, 0, 3, 1, 5, 3, 7, 3, 1};  // sizes: 0 -> 2, 1 -> 3, 3 -> 3, 5 -> 1, 7 -> 1
    std::vector<uint32_t> first;
    std::vector<uint64_t> size;
    derep_classes(rep, 10, first, size);
    if (first != std::vector<uint32_t>{1, 3, 0, 5, 7} || size != std::vector<uint64_t>{3, 3, 2, 1, 1}) return fail("derep_classes", 0, 0);
    derep_classes(rep, 0, first, size);
    if (!first.empty() || !size.empty()) return fail("derep_classes empty", 0, 0);
  }
  printf("OK\n%llu %llu %llu %llu %llu %llu\n", (unsigned long long)census_dup, (unsigned long long)census_minus, (unsigned long long)census_self,
         (unsigned long long)census_rounds, (unsigned long long)census_coll, (unsigned long long)census_repeat);
  return 0;
}
