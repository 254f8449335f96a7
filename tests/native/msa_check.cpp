// msa_check.cpp -- the --msa option of meshclust-assign, the parts that need no GPU:
//   * parse_assign_options: --msa FILE is stored and implies --identity, and nothing else
//   * assign_stats_json: the msa keys appear only with the option, and after every other key
// Prints "OK" and two JSON lines (without and with the option), or says what failed.  Linked
// against libmeshclust.so.  argv[1]: an existing file (stands for the model, the centres and the reads).
#include <cstdio>
#include <string>
#include <vector>

#include "assign.hpp"

static int fail(const char *what) {
  printf("FAIL: %s\n", what);
  return 1;
}

int main(int argc, char **argv) {
  if (argc < 2) return fail("usage: msa_check <an existing file>");
  if (MC_MSA_GAP != '-') return fail("MC_MSA_GAP is '-'");
  const std::string f = argv[1];
  std::vector<std::string> args{"meshclust-assign", "--model", f, "--centres", f, f};
  auto parse = [](std::vector<std::string> v) {
    std::vector<char *> av;
    for (auto &s : v) av.push_back(&s[0]);
    return mc::parse_assign_options((int)av.size(), av.data());
  };
  const mc::AssignOptions plain = parse(args);
  if (!plain.msa.empty() || plain.identity) return fail("the option is off by default");
  auto with = args;
  with.push_back("--msa");
  with.push_back("m.fa");
  const mc::AssignOptions o = parse(with);
  if (o.msa != "m.fa" || !o.identity) return fail("--msa FILE implies --identity");
  if (!o.paf.empty() || !o.consensus.empty() || !o.pileup.empty() || o.quality || o.min_identity >= 0 || o.top != 0 || o.both_strands)
    return fail("--msa FILE sets nothing else");
  with.push_back("--consensus");
  with.push_back("c.fa");
  const mc::AssignOptions both = parse(with);
  if (both.msa != "m.fa" || both.consensus != "c.fa") return fail("--msa and --consensus are given together");
  try {
    auto bad = args;
    bad.push_back("--msa");  // no file
    parse(bad);
    return fail("--msa without a file is a usage error");
  } catch (const mc::Error &e) {
    if (std::string(e.what()).find("--msa FILE") == std::string::npos) return fail("the usage text names --msa FILE");
  }
  mc::AssignResult r;
  r.reads = 10;
  r.assigned = 7;
  r.path = "device";
  r.identity = true;
  r.identity_pairs = 7;
  r.consensus = true;
  r.consensus_pairs = 7;
  r.consensus_centres = 3;
  r.consensus_passes = 2;
  printf("OK\n");
  printf("%s\n", mc::assign_stats_json(r).c_str());
  r.msa = true;
  r.msa_pairs = 7;
  r.msa_centres = 3;
  r.msa_columns = 412;
  r.msa_bytes = 1480;
  r.msa_ms = 1.5;
  printf("%s\n", mc::assign_stats_json(r).c_str());
  return 0;
}
