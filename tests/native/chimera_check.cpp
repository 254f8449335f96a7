// chimera_check.cpp -- host/chimera.hpp against a second statement of its choice and flag rules
// (tests/test_crossover_host.py builds and runs it, writes the cases and reads the answers).
//
// A case is a read's hits and, for every hit after the first, the eight values of mc_nw_msa_crossover
// (first hit, that hit).  The header's answer (chimera_candidates, chimera_pick) must equal the plain
// restatement here: all candidates listed with their better order, the list sorted by gain descending
// and hit ascending, its head taken.  The census counts what the cases held: reads without a
// candidate, hits skipped for having the first hit's centre, best_xy == best_yx, two candidates tied
// for the largest gain, gain == min_gain and gain == min_gain - 1.
// Without a file: seeded cases, "OK" if every answer is equal and every census entry is positive.
// With a file, one case per line (decimal numbers, separated by blanks):
//   n min_gain centres[n] values[(n - 1) * 8]
// Output: "OK", the number of cases, the census (six numbers), then per case
//   "hit xy best gain cut_first cut_last ids_left ids_right flag"   or   "-1".
#include <algorithm>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "chimera.hpp"

namespace {

struct Census {
  uint64_t none = 0, same_centre = 0, tie_order = 0, tie_gain = 0, at_gain = 0, below_gain = 0;
};

struct Case {
  int64_t min_gain;
  std::vector<uint32_t> centres;
  std::vector<int32_t> values;  // (n - 1) * 8: hit j's at (j - 1) * 8
};

struct Row {
  int hit, xy, best, gain, first, last, left, right;
};

// the rules restated
bool plain(const Case &c, Row &out, Census &cs) {
  std::vector<Row> rows;
  for (size_t j = 1; j < c.centres.size(); j++) {
    if (c.centres[j] == c.centres[0]) {
      cs.same_centre++;
      continue;
    }
    const int32_t *v = &c.values[(j - 1) * MC_CROSS_RES];
    const int single = std::max(v[0], v[1]);
    cs.tie_order += v[2] == v[5];
    if (v[5] > v[2]) rows.push_back({(int)j, 0, v[5], v[5] - single, v[6], v[7], v[1], v[0]});
    else rows.push_back({(int)j, 1, v[2], v[2] - single, v[3], v[4], v[0], v[1]});
  }
  if (rows.empty()) {
    cs.none++;
    return false;
  }
  std::stable_sort(rows.begin(), rows.end(), [](const Row &a, const Row &b) { return a.gain > b.gain; });
  cs.tie_gain += rows.size() > 1 && rows[0].gain == rows[1].gain;
  cs.at_gain += rows[0].gain == c.min_gain;
  cs.below_gain += rows[0].gain + 1 == c.min_gain;
  out = rows[0];
  return true;
}

// -> the case's output line; empty: the header and the restatement disagree
std::string check(const Case &c, Census &cs) {
  const uint32_t n = (uint32_t)c.centres.size();
  std::vector<uint32_t> cand(n ? n : 1);
  const uint32_t k = n ? mc::chimera_candidates(c.centres.data(), n, cand.data()) : 0;
  std::vector<int32_t> res;
  for (uint32_t t = 0; t < k; t++)
    res.insert(res.end(), c.values.begin() + (cand[t] - 1) * MC_CROSS_RES, c.values.begin() + cand[t] * MC_CROSS_RES);
  const mc::ChimeraCall got = mc::chimera_pick(cand.data(), k, res.data(), c.min_gain);
  Row want{};
  const bool any = plain(c, want, cs);
  if (!any) return got.hit == -1 && !got.flag ? "-1" : "";
  const bool flag = want.gain >= c.min_gain;
  if (got.hit != want.hit || (int)got.xy != want.xy || got.best != want.best || got.gain != want.gain || got.cut_first != want.first ||
      got.cut_last != want.last || got.ids_left != want.left || got.ids_right != want.right || got.flag != flag)
    return "";
  char b[160];
  std::snprintf(b, sizeof b, "%d %d %d %d %d %d %d %d %d", got.hit, (int)got.xy, got.best, got.gain, got.cut_first, got.cut_last,
                got.ids_left, got.ids_right, (int)got.flag);
  return b;
}

}  // namespace

int main(int argc, char **argv) {
  std::vector<Case> cases;
  if (argc > 1) {
    std::ifstream in(argv[1]);
    std::string line;
    while (std::getline(in, line)) {
      std::istringstream ss(line);
      long long n, g, v;
      if (!(ss >> n >> g)) continue;
      Case c;
      c.min_gain = g;
      for (long long j = 0; j < n && ss >> v; j++) c.centres.push_back((uint32_t)v);
      while (ss >> v) c.values.push_back((int32_t)v);
      if ((long long)c.centres.size() != n || c.values.size() != (size_t)(n > 0 ? n - 1 : 0) * MC_CROSS_RES) {
        std::printf("bad case line: %s\n", line.c_str());
        return 1;
      }
      cases.push_back(c);
    }
  } else {
    std::mt19937 rng(4);
    auto draw = [&](int lo, int hi) { return lo + (int)(rng() % (uint32_t)(hi - lo + 1)); };
    for (int it = 0; it < 4000; it++) {
      Case c;
      c.min_gain = draw(1, 4);
      const int n = draw(0, 5);
      for (int j = 0; j < n; j++) c.centres.push_back((uint32_t)draw(0, 3));
      for (int j = 1; j < n; j++) {
        const int ix = draw(90, 100), iy = draw(90, 100), single = std::max(ix, iy);
        const int32_t v[8] = {ix, iy, single + draw(0, 4), draw(0, 50), draw(50, 100), single + draw(0, 4), draw(0, 50), draw(50, 100)};
        c.values.insert(c.values.end(), v, v + 8);
      }
      cases.push_back(c);
    }
  }
  Census cs;
  std::vector<std::string> lines;
  for (size_t k = 0; k < cases.size(); k++) {
    lines.push_back(check(cases[k], cs));
    if (lines.back().empty()) {
      std::printf("case %zu: chimera.hpp and the restatement disagree\n", k);
      return 1;
    }
  }
  if (argc <= 1 && !(cs.none && cs.same_centre && cs.tie_order && cs.tie_gain && cs.at_gain && cs.below_gain)) {
    std::printf("the seeded cases miss a census entry\n");
    return 1;
  }
  std::printf("OK\n%zu\n%llu %llu %llu %llu %llu %llu\n", cases.size(), (unsigned long long)cs.none, (unsigned long long)cs.same_centre,
              (unsigned long long)cs.tie_order, (unsigned long long)cs.tie_gain, (unsigned long long)cs.at_gain,
              (unsigned long long)cs.below_gain);
  for (const std::string &s : lines) std::printf("%s\n", s.c_str());
  return 0;
}
