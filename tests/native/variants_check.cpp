// variants_check.cpp -- host/variants.hpp against a second statement of its two rules
// (tests/test_sites_host.py builds and runs it, writes further cases and reads the answers).
//
// Without a file: seeded random tables and the planted edge cases below go through variant_sites and
// haplotypes and through the plain restatements here (the five allele counts sorted; the strings
// counted in a sorted vector).  Every answer must be equal, and the census of what the cases held
// must be complete: ties between the first and second allele, depth 0, columns with only channel 4,
// second == min_count and second == min_frac * D exactly, each on both sides of the boundary.
// With a file, one case per line (every number decimal, separated by blanks):
//   T ncols min_frac min_count counts[ncols * 8]
//   H depth S min_count bytes[depth * S]
// Output: "OK", the number of cases, then per case "T n site .." or "H n hex:count ..".
#include <algorithm>
#include <cstdio>
#include <fstream>
#include <functional>
#include <iostream>
#include <random>
#include <sstream>

#include "variants.hpp"

namespace {

struct Census {
  uint64_t tie = 0, depth0 = 0, only4 = 0, at_count = 0, below_count = 0, at_frac = 0, below_frac = 0, sites = 0;
};

// the rule restated: the five counts sorted, the second of them
std::vector<uint32_t> sites_plain(const std::vector<uint32_t> &counts, uint64_t ncols, double min_frac, uint64_t min_count, Census &cs) {
  std::vector<uint32_t> out;
  for (uint64_t c = 0; c < ncols; c++) {
    const uint32_t *x = &counts[c * MC_MSA_CH];
    std::vector<uint64_t> v{x[0], x[1], x[2], x[3], x[5]};
    std::sort(v.begin(), v.end(), std::greater<uint64_t>());
    const uint64_t D = v[0] + v[1] + v[2] + v[3] + v[4], second = v[1];
    const double need = min_frac * (double)D;
    cs.tie += v[0] == v[1] && v[0] > 0;
    cs.depth0 += D == 0 && x[4] == 0;
    cs.only4 += D == 0 && x[4] > 0;
    cs.at_count += second == min_count && (double)second >= need;
    cs.below_count += second + 1 == min_count;
    cs.at_frac += second >= min_count && (double)second == need && D > 0;
    cs.below_frac += second >= min_count && (double)second < need && (double)(second + 1) >= need;
    if (second >= min_count && (double)second >= need) out.push_back((uint32_t)c);
  }
  cs.sites += out.size();
  return out;
}

std::vector<std::pair<std::string, uint64_t>> haplotypes_plain(const std::vector<uint8_t> &al, uint64_t depth, uint64_t S, uint64_t min_count) {
  std::vector<std::vector<uint8_t>> rows;
  for (uint64_t k = 0; k < depth; k++) rows.emplace_back(al.begin() + k * S, al.begin() + (k + 1) * S);
  std::sort(rows.begin(), rows.end());
  std::vector<std::pair<std::string, uint64_t>> out;
  for (size_t k = 0; k < rows.size();) {
    size_t e = k;
    while (e < rows.size() && rows[e] == rows[k]) e++;
    if (e - k >= min_count) out.push_back({std::string(rows[k].begin(), rows[k].end()), e - k});
    k = e;
  }
  // by count descending, then by bytes ascending: a selection sort that states the order outright
  for (size_t a = 0; a < out.size(); a++)
    for (size_t b = a + 1; b < out.size(); b++) {
      const bool less = std::lexicographical_compare(out[b].first.begin(), out[b].first.end(), out[a].first.begin(), out[a].first.end(),
                                                     [](char x, char y) { return (uint8_t)x < (uint8_t)y; });
      if (out[b].second > out[a].second || (out[b].second == out[a].second && less)) std::swap(out[a], out[b]);
    }
  return out;
}

int check_table(const std::vector<uint32_t> &counts, uint64_t ncols, double min_frac, uint64_t min_count, Census &cs, const char *what) {
  const std::vector<uint32_t> want = sites_plain(counts, ncols, min_frac, min_count, cs);
  const std::vector<uint32_t> got = mc::variant_sites(counts.data(), ncols, min_frac, min_count);
  if (got != want) {
    std::printf("%s: variant_sites gives %zu sites, the restatement %zu (min_frac %.17g, min_count %llu)\n", what, got.size(),
                want.size(), min_frac, (unsigned long long)min_count);
    return 1;
  }
  return 0;
}

int self_check() {
  Census cs;
  std::mt19937_64 rng(20261);
  auto below = [&](uint64_t n) { return (uint64_t)(rng() % n); };
  // seeded random tables: small counts (ties and zeros are common), every threshold in turn
  const double fracs[] = {0.05, 0.2, 0.25, 0.5, 1.0};
  for (int k = 0; k < 400; k++) {
    const uint64_t ncols = below(40);
    std::vector<uint32_t> counts(ncols * MC_MSA_CH);
    for (uint64_t c = 0; c < ncols; c++) {
      const uint64_t kind = below(8);
      for (uint32_t ch = 0; ch < 6; ch++)
        counts[c * MC_MSA_CH + ch] = kind == 0 ? 0u : kind == 1 ? (ch == 4 ? 1u + (uint32_t)below(5) : 0u) : (uint32_t)below(kind == 2 ? 3 : 12);
      counts[c * MC_MSA_CH + 6] = (uint32_t)c;
    }
    if (check_table(counts, ncols, fracs[k % 5], 1 + below(4), cs, "random table")) return 1;
  }
  // the boundaries, planted: second == min_count and one less; second == min_frac * D exactly and one less
  struct Planted {
    uint32_t n[6];
    double frac;
    uint64_t count;
    bool site;
  };
  const Planted planted[] = {
      {{8, 2, 0, 0, 0, 0}, 0.2, 2, true},    // second == min_count, 2 == 0.2 * 10
      {{8, 1, 0, 0, 0, 0}, 0.05, 2, false},  // second == min_count - 1
      {{6, 0, 0, 0, 0, 2}, 0.25, 1, true},   // the gap is an allele: 2 == 0.25 * 8
      {{7, 0, 0, 0, 0, 2}, 0.25, 1, false},  // 2 < 0.25 * 9
      {{3, 3, 0, 0, 0, 0}, 0.5, 3, true},    // a tie for the first place: second is that count; 3 == 0.5 * 6
      {{3, 3, 1, 0, 0, 0}, 0.5, 3, false},   // 3 < 0.5 * 7
      {{5, 0, 0, 0, 4, 0}, 0.05, 1, false},  // channel 4 is no allele
      {{0, 0, 0, 0, 4, 0}, 0.05, 1, false},  // only channel 4
      {{0, 0, 0, 0, 0, 0}, 0.05, 1, false},  // depth 0
      {{4, 0, 0, 4, 0, 0}, 1.0, 4, false},   // min_frac 1: second would have to be all of D
      {{0, 0, 0, 0, 0, 0}, 1.0, 1, false},
  };
  for (const Planted &p : planted) {
    std::vector<uint32_t> counts(MC_MSA_CH, 0);
    for (int ch = 0; ch < 6; ch++) counts[ch] = p.n[ch];
    if (check_table(counts, 1, p.frac, p.count, cs, "planted column")) return 1;
    if ((mc::variant_sites(counts.data(), 1, p.frac, p.count).size() == 1) != p.site) {
      std::printf("planted column %u %u %u %u %u %u at %.3g / %llu: expected %s\n", p.n[0], p.n[1], p.n[2], p.n[3], p.n[4], p.n[5], p.frac,
                  (unsigned long long)p.count, p.site ? "a site" : "no site");
      return 1;
    }
  }
  if (!cs.tie || !cs.depth0 || !cs.only4 || !cs.at_count || !cs.below_count || !cs.at_frac || !cs.below_frac || !cs.sites) {
    std::printf("the census is incomplete: tie %llu depth0 %llu only4 %llu count %llu/%llu frac %llu/%llu\n", (unsigned long long)cs.tie,
                (unsigned long long)cs.depth0, (unsigned long long)cs.only4, (unsigned long long)cs.at_count,
                (unsigned long long)cs.below_count, (unsigned long long)cs.at_frac, (unsigned long long)cs.below_frac);
    return 1;
  }
  // haplotypes: few distinct strings over a small alphabet (equal counts are common), bytes above 127
  uint64_t ties = 0, dropped = 0;
  for (int k = 0; k < 300; k++) {
    const uint64_t depth = below(30), S = below(5), min_count = 1 + below(3);
    std::vector<uint8_t> al(depth * S);
    const uint8_t letters[] = {'A', 'C', '-', 200};
    for (uint8_t &x : al) x = letters[below(k % 3 ? 2 : 4)];
    const auto want = haplotypes_plain(al, depth, S, min_count);
    const auto got = mc::haplotypes(al.data(), depth, S, min_count);
    if (got != want) {
      std::printf("haplotypes: case %d (depth %llu, S %llu, min_count %llu) differs\n", k, (unsigned long long)depth, (unsigned long long)S,
                  (unsigned long long)min_count);
      return 1;
    }
    uint64_t kept = 0;
    for (size_t a = 0; a < got.size(); a++) {
      kept += got[a].second;
      ties += a > 0 && got[a].second == got[a - 1].second;
    }
    dropped += kept < depth;
  }
  if (!ties || !dropped) {
    std::printf("the haplotype cases hold no tie or drop nothing\n");
    return 1;
  }
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  if (self_check()) return 1;
  std::ostringstream out;
  size_t ncases = 0;
  if (argc > 1) {
    std::ifstream in(argv[1]);
    std::string line;
    while (std::getline(in, line)) {
      std::istringstream ss(line);
      std::string tag;
      ss >> tag;
      if (tag == "T") {
        uint64_t ncols, min_count, v;
        double frac;
        ss >> ncols >> frac >> min_count;
        std::vector<uint32_t> counts;
        for (uint64_t k = 0; k < ncols * MC_MSA_CH; k++) {
          ss >> v;
          counts.push_back((uint32_t)v);
        }
        if (!ss) return 3;
        Census cs;
        if (check_table(counts, ncols, frac, min_count, cs, "file table")) return 1;
        const std::vector<uint32_t> s = mc::variant_sites(counts.data(), ncols, frac, min_count);
        out << "T " << s.size();
        for (uint32_t c : s) out << ' ' << c;
        out << '\n';
        ncases++;
      } else if (tag == "H") {
        uint64_t depth, S, min_count, v;
        ss >> depth >> S >> min_count;
        std::vector<uint8_t> al;
        for (uint64_t k = 0; k < depth * S; k++) {
          ss >> v;
          al.push_back((uint8_t)v);
        }
        if (!ss) return 3;
        const auto h = mc::haplotypes(al.data(), depth, S, min_count);
        if (h != haplotypes_plain(al, depth, S, min_count)) return 1;
        out << "H " << h.size();
        for (const auto &kv : h) {
          out << ' ';
          char buf[4];
          for (char x : kv.first) {
            std::snprintf(buf, sizeof buf, "%02x", (unsigned)(uint8_t)x);
            out << buf;
          }
          out << ':' << kv.second;
        }
        out << '\n';
        ncases++;
      }
    }
  }
  std::cout << "OK\n" << ncases << '\n' << out.str();
  return 0;
}
