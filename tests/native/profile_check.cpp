// profile_check.cpp -- host/profile.hpp against host/consensus.hpp on the same alignments
// (tests/test_profile_host.py writes the cases and reads the answers).
//
// Input, one case after the other (every number decimal, separated by blanks):
//   C L c[0] .. c[L - 1]                    a centre
//   P nw w[0..nw) la a[0..la) q[0..la)      one of its pairs: the operation words, seq1 and its
//                                           qualities as aligned
//   E                                       the end of the case
// Per case the pile-up rows, the weight rows and the inserted runs are built as the header defines
// them and go through consensus_of / qconsensus_of; the column profile is built from the same words
// and goes through consensus_from_profile / qconsensus_from_profile.  Every field must be equal.
// Output: "OK", then per case "seq sub del ins qseq qqual qsub qdel qins" of the profile's answer.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "profile.hpp"

namespace {

struct Pair {
  std::vector<uint32_t> words;
  std::vector<uint8_t> read, qual;
};

struct Case {
  std::vector<uint8_t> centre;
  std::vector<Pair> pairs;
};

uint32_t gap_quality(const Pair &p, uint64_t i) {
  uint32_t v = 0xffffffffu;
  if (i > 0) v = p.qual[i - 1];
  if (i < p.read.size()) v = std::min<uint32_t>(v, p.qual[i]);
  return v == 0xffffffffu ? 0 : v;
}

// the pile-up table and weight table of include/meshclust_amd.h
void pileup(const Case &cs, std::vector<uint32_t> &rows, std::vector<uint32_t> &wrows) {
  const uint64_t L = cs.centre.size();
  rows.assign((L + 1) * MC_PILEUP_CH, 0);
  wrows.assign((L + 1) * MC_PILEUP_CH, 0);
  for (const Pair &p : cs.pairs) {
    uint64_t i = 0, j = 0;
    for (uint32_t wd : p.words) {
      const uint64_t n = wd >> 4;
      const uint32_t op = wd & 15u;
      if (op == MC_CIGAR_EQ || op == MC_CIGAR_X) {
        for (uint64_t t = 0; t < n; t++) {
          rows[(j + t) * MC_PILEUP_CH + mc::pileup_channel(p.read[i + t])]++;
          wrows[(j + t) * MC_PILEUP_CH + mc::pileup_channel(p.read[i + t])] += p.qual[i + t];
        }
        i += n;
        j += n;
      } else if (op == MC_CIGAR_D) {
        for (uint64_t t = 0; t < n; t++) {
          rows[(j + t) * MC_PILEUP_CH + 5]++;
          wrows[(j + t) * MC_PILEUP_CH + 5] += gap_quality(p, i);
        }
        j += n;
      } else {
        uint32_t q = 0xffffffffu;
        for (uint64_t t = 0; t < n; t++) q = std::min<uint32_t>(q, p.qual[i + t]);
        rows[j * MC_PILEUP_CH + 6]++;
        rows[j * MC_PILEUP_CH + 7] += (uint32_t)n;
        wrows[j * MC_PILEUP_CH + 6] += q;
        i += n;
      }
    }
  }
}

// the column profile of include/meshclust_amd.h (mc_nw_msa_counts) -> W
uint64_t profile(const Case &cs, std::vector<uint32_t> &counts, std::vector<uint32_t> &wcounts) {
  const uint64_t L = cs.centre.size();
  std::vector<uint64_t> w(L + 1, 0), col(L + 1, 0);
  for (const Pair &p : cs.pairs) {
    uint64_t j = 0;
    for (uint32_t wd : p.words) {
      const uint64_t n = wd >> 4;
      const uint32_t op = wd & 15u;
      if (op == MC_CIGAR_I) w[j] = std::max(w[j], n);
      else if (op != MC_CIGAR_I) j += n;
    }
  }
  uint64_t sum = 0;
  for (uint64_t r = 0; r <= L; r++) {
    sum += w[r];
    col[r] = r + sum;
  }
  const uint64_t W = col[L];
  counts.assign(W * MC_MSA_CH, 0);
  wcounts.assign(W * MC_MSA_CH, 0);
  for (const Pair &p : cs.pairs) {
    uint64_t i = 0, j = 0;
    for (uint32_t wd : p.words) {
      const uint64_t n = wd >> 4;
      const uint32_t op = wd & 15u;
      if (op == MC_CIGAR_EQ || op == MC_CIGAR_X) {
        for (uint64_t t = 0; t < n; t++) {
          counts[col[j + t] * MC_MSA_CH + mc::pileup_channel(p.read[i + t])]++;
          wcounts[col[j + t] * MC_MSA_CH + mc::pileup_channel(p.read[i + t])] += p.qual[i + t];
        }
        i += n;
        j += n;
      } else if (op == MC_CIGAR_D) {
        for (uint64_t t = 0; t < n; t++) {
          counts[col[j + t] * MC_MSA_CH + 5]++;
          wcounts[col[j + t] * MC_MSA_CH + 5] += gap_quality(p, i);
        }
        j += n;
      } else {
        for (uint64_t t = 0; t < n; t++) {
          counts[(col[j] - w[j] + t) * MC_MSA_CH + mc::pileup_channel(p.read[i + t])]++;
          wcounts[(col[j] - w[j] + t) * MC_MSA_CH + mc::pileup_channel(p.read[i + t])] += p.qual[i + t];
        }
        i += n;
      }
    }
  }
  for (uint64_t r = 0; r <= L; r++) {
    for (uint64_t t = 0; t < w[r]; t++) {
      uint32_t *c = &counts[(col[r] - w[r] + t) * MC_MSA_CH];
      c[5] = (uint32_t)cs.pairs.size() - (c[0] + c[1] + c[2] + c[3] + c[4]);
      c[6] = (uint32_t)r;
      c[7] = (uint32_t)t + 1;
    }
    if (r < L) counts[col[r] * MC_MSA_CH + 6] = (uint32_t)r;
  }
  return W;
}

int check(const Case &cs, size_t index) {
  const uint64_t L = cs.centre.size(), depth = cs.pairs.size();
  std::vector<uint32_t> rows, wrows, counts, wcounts;
  pileup(cs, rows, wrows);
  const std::vector<uint64_t> sites = mc::insertion_sites(rows.data(), L, depth);
  mc::InsertionRuns runs;
  mc::QInsertionRuns qruns;
  for (const Pair &p : cs.pairs) {
    mc::insertion_runs(p.words.data(), p.words.size(), p.read.data(), sites, runs);
    mc::qinsertion_runs(p.words.data(), p.words.size(), p.read.data(), p.qual.data(), sites, qruns);
  }
  const mc::Consensus want = mc::consensus_of(cs.centre.data(), L, rows.data(), depth, runs);
  const mc::QConsensus qwant = mc::qconsensus_of(cs.centre.data(), L, rows.data(), wrows.data(), depth, qruns);
  const uint64_t W = profile(cs, counts, wcounts);
  const mc::Consensus got = mc::consensus_from_profile(cs.centre.data(), L, W, counts.data());
  const mc::QConsensus qgot = mc::qconsensus_from_profile(cs.centre.data(), L, W, counts.data(), wcounts.data());
  if (got.seq != want.seq || got.sub != want.sub || got.del != want.del || got.ins != want.ins) {
    std::printf("case %zu: consensus_from_profile %s %llu %llu %llu, consensus_of %s %llu %llu %llu\n", index, got.seq.c_str(),
                (unsigned long long)got.sub, (unsigned long long)got.del, (unsigned long long)got.ins, want.seq.c_str(),
                (unsigned long long)want.sub, (unsigned long long)want.del, (unsigned long long)want.ins);
    return 1;
  }
  if (qgot.seq != qwant.seq || qgot.qual != qwant.qual || qgot.sub != qwant.sub || qgot.del != qwant.del || qgot.ins != qwant.ins) {
    std::printf("case %zu: qconsensus_from_profile %s %s, qconsensus_of %s %s\n", index, qgot.seq.c_str(), qgot.qual.c_str(),
                qwant.seq.c_str(), qwant.qual.c_str());
    return 1;
  }
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  std::ifstream in(argv[1]);
  std::vector<Case> cases;
  std::string line;
  Case cur;
  while (std::getline(in, line)) {
    std::istringstream ss(line);
    std::string tag;
    ss >> tag;
    if (tag == "C") {
      cur = Case{};
      uint64_t L, v;
      ss >> L;
      for (uint64_t r = 0; r < L; r++) {
        ss >> v;
        cur.centre.push_back((uint8_t)v);
      }
    } else if (tag == "P") {
      Pair p;
      uint64_t nw, la, v;
      ss >> nw;
      for (uint64_t k = 0; k < nw; k++) {
        ss >> v;
        p.words.push_back((uint32_t)v);
      }
      ss >> la;
      for (uint64_t k = 0; k < la; k++) {
        ss >> v;
        p.read.push_back((uint8_t)v);
      }
      for (uint64_t k = 0; k < la; k++) {
        ss >> v;
        p.qual.push_back((uint8_t)v);
      }
      if (!ss) return 3;
      cur.pairs.push_back(p);
    } else if (tag == "E") {
      cases.push_back(cur);
    }
  }
  std::ostringstream out;
  for (size_t k = 0; k < cases.size(); k++) {
    if (check(cases[k], k)) return 1;
    const Case &cs = cases[k];
    std::vector<uint32_t> counts, wcounts;
    const uint64_t W = profile(cs, counts, wcounts);
    const mc::Consensus c = mc::consensus_from_profile(cs.centre.data(), cs.centre.size(), W, counts.data());
    const mc::QConsensus q = mc::qconsensus_from_profile(cs.centre.data(), cs.centre.size(), W, counts.data(), wcounts.data());
    // (an empty string is written as "." so that the line keeps its nine fields)
    out << (c.seq.empty() ? "." : c.seq) << ' ' << c.sub << ' ' << c.del << ' ' << c.ins << ' ' << (q.seq.empty() ? "." : q.seq) << ' '
        << (q.qual.empty() ? "." : q.qual) << ' ' << q.sub << ' ' << q.del << ' ' << q.ins << '\n';
  }
  std::cout << "OK\n" << cases.size() << '\n' << out.str();
  return 0;
}
