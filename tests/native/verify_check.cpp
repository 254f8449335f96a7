// verify_check.cpp -- meshclust-assign --identity / --min-identity, the parts that need no GPU:
//   * verify_pick (host/verify.hpp): the first candidate in rank order whose identity is at least
//     X -- not the best identity; X = 0 confirms rank 1, X = 1 only an exact 1.0, the empty list
//     gives none, and of two equal identities the better rank is taken
//   * parse_assign_options: --identity and --min-identity X are stored, --min-identity implies
//     --identity and is accepted without --top; X outside 0 .. 1 or not a number is an Error of
//     code 1 that carries the usage text
//   * assign_stats_json: "identity_pairs", "identity_cells", "rejected" and the "identity" phase
//     appear only with the options (the test compares the keys)
// Linked against libmeshclust.so.  Prints "OK", then two JSON lines; or says what failed.
#include <cstdio>
#include <string>
#include <vector>

#include "assign.hpp"
#include "verify.hpp"

static int fail(const char *what) {
  printf("FAIL: %s\n", what);
  return 1;
}

static mc::AssignOptions parse(std::vector<std::string> args) {
  std::vector<char *> argv;
  for (auto &a : args) argv.push_back(&a[0]);
  return mc::parse_assign_options((int)argv.size(), argv.data());
}

// 1 when the options are refused with code 1 and the usage text
static int refused(std::vector<std::string> args) {
  try {
    parse(args);
  } catch (const mc::Error &e) {
    const std::string w = e.what();
    return e.code == 1 && w.find("--min-identity") != std::string::npos && w.find("Usage:") != std::string::npos;
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 2) return fail("usage: verify_check <an existing file>");
  {
    const double id[4] = {0.70, 0.95, 0.80, 0.95};
    if (mc::verify_pick(id, 4, 0.75) != 1) return fail("the first qualifying rank");
    if (mc::verify_pick(id, 4, 0.70) != 0) return fail("an identity equal to X qualifies");
    if (mc::verify_pick(id, 4, 0.0) != 0) return fail("X = 0 confirms rank 1");
    if (mc::verify_pick(id, 4, 0.96) != -1 || mc::verify_pick(id, 4, 1.0) != -1) return fail("none qualifies");
    if (mc::verify_pick(id, 0, 0.0) != -1 || mc::verify_pick(nullptr, 0, 0.5) != -1) return fail("the empty list");
    if (mc::verify_pick(id, 1, 0.75) != -1) return fail("only the listed candidates count");
    const double tie[3] = {0.5, 0.9, 0.9};  // equal identities: the better rank
    if (mc::verify_pick(tie, 3, 0.9) != 1) return fail("a tie in identity goes to the better rank");
    const double one[3] = {0.999999, 1.0, 1.0};
    if (mc::verify_pick(one, 3, 1.0) != 1) return fail("X = 1 takes an exact 1.0 only");
    const double zero[2] = {0.0, 0.3};
    if (mc::verify_pick(zero, 2, 0.0) != 0) return fail("X = 0 and identity 0");
  }
  const std::string f = argv[1];
  const std::vector<std::string> base{"meshclust-assign", "--model", f, "--centres", f, f};
  auto with = [&](std::vector<std::string> extra) {
    std::vector<std::string> a = base;
    a.insert(a.end(), extra.begin(), extra.end());
    return a;
  };
  const mc::AssignOptions a = parse(base);
  if (a.identity || a.min_identity >= 0) return fail("--identity / --min-identity are on by default");
  const mc::AssignOptions b = parse(with({"--identity"}));
  if (!b.identity || b.min_identity >= 0 || b.top != 0 || b.both_strands || b.output != a.output)
    return fail("--identity not stored, or it changed another option");
  const mc::AssignOptions c = parse(with({"--min-identity", "0.8"}));  // without --top: K = 1
  if (!c.identity || c.min_identity != 0.8 || c.top != 0 || !c.hits.empty()) return fail("--min-identity 0.8");
  const mc::AssignOptions d = parse(with({"--min-identity", "0", "--top", "3", "--hits", "h.tsv", "--both-strands"}));
  if (!d.identity || d.min_identity != 0.0 || d.top != 3 || d.hits != "h.tsv" || !d.both_strands) return fail("--min-identity 0 with --top");
  if (parse(with({"--min-identity", "1"})).min_identity != 1.0) return fail("--min-identity 1");
  for (const char *bad : {"1.5", "-0.1", "x", "0.5x", "nan", ""})
    if (!refused(with({"--min-identity", bad}))) return fail("a bad --min-identity is not refused with code 1 and the usage text");
  mc::AssignResult r;
  r.reads = 10;
  r.assigned = 7;
  r.path = "device";
  printf("OK\n%s\n", mc::assign_stats_json(r).c_str());
  r.identity = true;
  r.identity_pairs = 21;
  r.identity_cells = 21000000;
  r.rejected = 2;
  r.identity_ms = 1.5;
  printf("%s\n", mc::assign_stats_json(r).c_str());
  return 0;
}
