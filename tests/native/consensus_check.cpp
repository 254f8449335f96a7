// consensus_check.cpp -- host/consensus.hpp and the --consensus / --pileup options, the parts that
// need no GPU:
//   * consensus_channel: the largest of channels 0..5, the centre's own channel on a tie it is part
//     of, else the lowest; insertion_consensus: the most frequent length (ties: the shortest), the
//     plurality class per base (ties: the lowest), other bytes as N; insertion_runs over words
//   * consensus_of over the tables of a fixture file (written by tests/test_pileup_host.py, which
//     compares the lines printed here with its Python restatement)
//   * parse_assign_options: --consensus FILE and --pileup FILE are stored, each implies --identity
//   * assign_stats_json: the consensus keys appear only with the options
// Fixture: per centre "centre L depth nruns", a line of L bytes, a line of (L + 1) * 8 counters,
// then nruns lines "run row n b0 .. bn-1".  Prints "OK", a line "sub del ins [sequence]" per centre,
// then two JSON lines; or says what failed.  Linked against libmeshclust.so.
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
  if (argc < 3) return fail("usage: consensus_check <fixture> <an existing file>");
  if (MC_PILEUP_CH != 8) return fail("MC_PILEUP_CH is 8");
  {
    const uint32_t clear[8] = {1, 7, 2, 0, 0, 3, 9, 9}, tie_own[8] = {4, 1, 4, 0, 0, 4, 0, 0}, tie_other[8] = {0, 3, 0, 3, 0, 3, 0, 0};
    const uint32_t del[8] = {1, 1, 0, 0, 0, 5, 0, 0}, none[8] = {0, 0, 0, 0, 0, 0, 0, 0}, other[8] = {1, 0, 0, 0, 2, 0, 0, 0};
    if (mc::consensus_channel(clear, 0) != 1) return fail("the largest channel wins (channels 6 and 7 do not vote)");
    if (mc::consensus_channel(tie_own, 2) != 2 || mc::consensus_channel(tie_own, 0) != 0) return fail("a tie goes to the centre's own channel");
    if (mc::consensus_channel(tie_own, 'N') != 0 || mc::consensus_channel(tie_other, 0) != 1) return fail("else to the lowest channel");
    if (mc::consensus_channel(tie_other, 3) != 3 || mc::consensus_channel(del, 0) != 5) return fail("a deletion can win");
    if (mc::consensus_channel(none, 2) != 2 || mc::consensus_channel(none, 'N') != 4) return fail("no reads: the centre's channel");
    if (mc::consensus_channel(other, 1) != 4) return fail("other bytes vote as one class");
  }
  {
    using R = std::vector<uint8_t>;
    if (mc::insertion_consensus({R{1}, R{2, 2}, R{3, 3}, R{0}}) != "A") return fail("length ties go to the shortest, class ties to the lowest");
    if (mc::insertion_consensus({R{1, 2}, R{1, 3}, R{1, 3, 0}, R{2}}) != "CT") return fail("the most frequent length, the plurality per base");
    if (mc::insertion_consensus({R{'N', 1}, R{'A', 1}, R{0, 2}}) != "NC") return fail("other bytes are one class, written N");
    //  read 0 1 [2 3] 0 - 1 [2]   centre 0 1 0 3 1:  2= 2I 1= 1D 1X 1I  -> runs at rows 2 and 5
    const uint8_t read[7] = {0, 1, 2, 3, 0, 2, 2};
    const uint32_t w[6] = {2u << 4 | MC_CIGAR_EQ, 2u << 4 | MC_CIGAR_I, 1u << 4 | MC_CIGAR_EQ, 1u << 4 | MC_CIGAR_D,
                           1u << 4 | MC_CIGAR_X, 1u << 4 | MC_CIGAR_I};
    mc::InsertionRuns runs;
    mc::insertion_runs(w, 6, read, {2, 5}, runs);
    if (runs.size() != 2 || runs[2] != std::vector<R>{R{2, 3}} || runs[5] != std::vector<R>{R{2}}) return fail("insertion_runs");
    mc::InsertionRuns only;
    mc::insertion_runs(w, 6, read, {5}, only);
    if (only.size() != 1 || only[5] != std::vector<R>{R{2}}) return fail("insertion_runs keeps the listed rows only");
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
    std::vector<uint32_t> rows((L + 1) * MC_PILEUP_CH);
    for (auto &x : cen) {
      unsigned v;
      in >> v;
      x = (uint8_t)v;
    }
    for (auto &x : rows) in >> x;
    const std::vector<uint64_t> sites = mc::insertion_sites(rows.data(), L, depth);
    mc::InsertionRuns runs;
    for (uint64_t k = 0; k < nruns; k++) {
      uint64_t row, n;
      in >> word >> row >> n;
      if (word != "run") return fail("fixture: run expected");
      std::vector<uint8_t> b(n);
      for (auto &x : b) {
        unsigned v;
        in >> v;
        x = (uint8_t)v;
      }
      if (std::binary_search(sites.begin(), sites.end(), row)) runs[row].push_back(b);
    }
    if (!in) return fail("fixture: short");
    const mc::Consensus c = mc::consensus_of(cen.data(), L, rows.data(), depth, runs);
    lines.push_back(std::to_string(c.sub) + " " + std::to_string(c.del) + " " + std::to_string(c.ins) + " [" + c.seq + "]");
  }
  const std::string f = argv[2];
  std::vector<std::string> args{"meshclust-assign", "--model", f, "--centres", f, f};
  auto parse = [](std::vector<std::string> v) {
    std::vector<char *> av;
    for (auto &s : v) av.push_back(&s[0]);
    return mc::parse_assign_options((int)av.size(), av.data());
  };
  const mc::AssignOptions plain = parse(args);
  if (!plain.consensus.empty() || !plain.pileup.empty() || plain.identity) return fail("the options are off by default");
  auto with = args;
  with.push_back("--consensus");
  with.push_back("c.fa");
  const mc::AssignOptions o = parse(with);
  if (o.consensus != "c.fa" || !o.pileup.empty() || !o.identity || !o.paf.empty() || o.min_identity >= 0 || o.top != 0)
    return fail("--consensus FILE implies --identity");
  with = args;
  with.push_back("--pileup");
  with.push_back("p.tsv");
  const mc::AssignOptions o2 = parse(with);
  if (o2.pileup != "p.tsv" || !o2.consensus.empty() || !o2.identity) return fail("--pileup FILE may be given alone and implies --identity");
  mc::AssignResult r;
  r.reads = 10;
  r.assigned = 7;
  r.path = "device";
  r.identity = true;
  r.identity_pairs = 7;
  printf("OK\n");
  for (const auto &l : lines) printf("%s\n", l.c_str());
  printf("%s\n", mc::assign_stats_json(r).c_str());
  r.consensus = true;
  r.consensus_pairs = 7;
  r.consensus_centres = 3;
  r.consensus_passes = 1;
  r.realigned_centres = 1;
  r.insertion_sites = 2;
  printf("%s\n", mc::assign_stats_json(r).c_str());
  return 0;
}
