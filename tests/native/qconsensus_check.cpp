// qconsensus_check.cpp -- host/consensus.hpp's weighted consensus and the --quality option, the
// parts that need no GPU:
//   * qconsensus_pick: the largest weight, ties to the larger count, then to the centre's own
//     channel if it is among the tied, else to the lowest; qconsensus_quality: the clamp
//   * qconsensus_of over the tables of a fixture file (written by tests/test_qpileup_host.py, which
//     compares the lines printed here with its Python restatement)
//   * parse_assign_options: --quality is stored and needs --consensus or --pileup
//   * assign_stats_json: "quality" appears only with the option
// Fixture: per centre "centre L depth nruns", a line of L bytes, a line of (L + 1) * 8 counters, a
// line of (L + 1) * 8 weights, then nruns lines "run row n b0 .. bn-1 q0 .. qn-1".  Prints "OK", a
// line "sub del ins [sequence] [qualities]" per centre, then two JSON lines; or says what failed.
// Linked against libmeshclust.so.
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "assign.hpp"
#include "consensus.hpp"

static int fail(const char *what) {
  printf("FAIL: %s\n", what);
  return 1;
}

int main(int argc, char **argv) {
  if (argc < 3) return fail("usage: qconsensus_check <fixture> <an existing file>");
  if (MC_QUAL_MAX != 93) return fail("MC_QUAL_MAX is 93");
  {
    const uint64_t w[6] = {4, 80, 4, 0, 0, 0}, n[6] = {2, 1, 2, 0, 0, 0};
    if (mc::qconsensus_pick(w, n, 6, 0) != 1) return fail("the largest weight wins, whatever the counts");
    if (mc::qconsensus_quality(w, 6, 1) != (char)(33 + 72)) return fail("quality: the winner's weight less the others'");
    const uint64_t tw[6] = {10, 10, 10, 0, 0, 10}, tn[6] = {1, 2, 2, 0, 0, 2};
    if (mc::qconsensus_pick(tw, tn, 6, 0) != 1) return fail("a weight tie goes to the larger count, then to the lowest");
    if (mc::qconsensus_pick(tw, tn, 6, 2) != 2 || mc::qconsensus_pick(tw, tn, 6, 5) != 5) return fail("then to the centre's own channel");
    if (mc::qconsensus_pick(tw, tn, 6, 4) != 1) return fail("an own channel outside the tie does not win");
    if (mc::qconsensus_quality(tw, 6, 1) != '!') return fail("quality: clamped at 0");
    const uint64_t big[6] = {5000, 3, 0, 0, 0, 0}, zn[6] = {60, 1, 0, 0, 0, 0}, none[6] = {0, 0, 0, 0, 0, 0}, cnt[6] = {0, 0, 3, 0, 0, 1};
    if (mc::qconsensus_quality(big, 6, 0) != (char)(33 + 93)) return fail("quality: clamped at 93");
    if (mc::qconsensus_pick(big, zn, 6, 3) != 0) return fail("the largest weight");
    if (mc::qconsensus_pick(none, cnt, 6, 0) != 2) return fail("all weights 0: the counts decide");
  }
  std::ifstream in(argv[1]);
  if (!in) return fail("cannot read the fixture");
  std::vector<std::string> lines;
  std::string word;
  while (in >> word) {
    if (word != "centre") return fail("fixture: centre expected");
    uint64_t L, depth, nruns;
    in >> L >> depth >> nruns;
    std::vector<uint8_t> cen(L);
    std::vector<uint32_t> rows((L + 1) * MC_PILEUP_CH), wrows((L + 1) * MC_PILEUP_CH);
    for (auto &x : cen) {
      unsigned v;
      in >> v;
      x = (uint8_t)v;
    }
    for (auto &x : rows) in >> x;
    for (auto &x : wrows) in >> x;
    const std::vector<uint64_t> sites = mc::insertion_sites(rows.data(), L, depth);
    mc::QInsertionRuns runs;
    for (uint64_t k = 0; k < nruns; k++) {
      uint64_t row, n;
      in >> word >> row >> n;
      if (word != "run") return fail("fixture: run expected");
      mc::QRun r;
      r.base.resize(n);
      r.qual.resize(n);
      for (auto *v : {&r.base, &r.qual})
        for (auto &x : *v) {
          unsigned u;
          in >> u;
          x = (uint8_t)u;
        }
      if (std::binary_search(sites.begin(), sites.end(), row)) runs[row].push_back(r);
    }
    if (!in) return fail("fixture: short");
    const mc::QConsensus c = mc::qconsensus_of(cen.data(), L, rows.data(), wrows.data(), depth, runs);
    if (c.seq.size() != c.qual.size()) return fail("a quality per base");
    lines.push_back(std::to_string(c.sub) + " " + std::to_string(c.del) + " " + std::to_string(c.ins) + " [" + c.seq + "] [" + c.qual + "]");
  }
  const std::string f = argv[2];
  std::vector<std::string> args{"meshclust-assign", "--model", f, "--centres", f, f};
  auto parse = [](std::vector<std::string> v) {
    std::vector<char *> av;
    for (auto &s : v) av.push_back(&s[0]);
    return mc::parse_assign_options((int)av.size(), av.data());
  };
  if (parse(args).quality) return fail("--quality is off by default");
  auto with = args;
  with.push_back("--quality");
  try {
    parse(with);
    return fail("--quality alone is a usage error");
  } catch (const mc::Error &e) {
    if (e.code != 1 || std::string(e.what()).find("--quality needs") == std::string::npos) return fail("the usage error's text");
  }
  with.push_back("--pileup");
  with.push_back("p.tsv");
  const mc::AssignOptions o = parse(with);
  if (!o.quality || o.pileup != "p.tsv" || !o.consensus.empty() || !o.identity) return fail("--quality with --pileup");
  mc::AssignResult r;
  r.reads = 10;
  r.assigned = 7;
  r.path = "device";
  r.identity = true;
  r.identity_pairs = 7;
  r.consensus = true;
  r.consensus_pairs = 7;
  r.consensus_centres = 3;
  r.consensus_passes = 1;
  printf("OK\n");
  for (const auto &l : lines) printf("%s\n", l.c_str());
  printf("%s\n", mc::assign_stats_json(r).c_str());
  r.quality = true;
  printf("%s\n", mc::assign_stats_json(r).c_str());
  return 0;
}
