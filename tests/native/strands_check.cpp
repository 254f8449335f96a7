// strands_check.cpp -- the host side of meshclust-assign --both-strands, without a GPU:
//   * mc::rc_index (strand.hpp, the function the permutation kernel calls) against the digit
//     definition for k = 1..6: reverse the k base-4 digits, complement each; an involution; no
//     fixed point at odd k, 4^(k/2) at even k
//   * parse_assign_options: the flag is stored, is off by default, and the usage text names it
//   * assign_stats_json: printed for a one-strand and a both-strands result (the test compares
//     the keys)
// Linked against libmeshclust.so.  Prints "OK", then the two JSON lines; or says what failed.
#include <cstdio>
#include <string>
#include <vector>

#include "assign.hpp"
#include "strand.hpp"

static int fail(const char *what) {
  printf("FAIL: %s\n", what);
  return 1;
}

static uint32_t rc_by_digits(uint32_t i, int k) {
  std::vector<int> d(k);
  for (int p = k - 1; p >= 0; p--) {  // d[0] is the first base (most significant)
    d[p] = (int)(i % 4);
    i /= 4;
  }
  uint32_t r = 0;
  for (int p = k - 1; p >= 0; p--) r = r * 4 + (uint32_t)(3 - d[p]);  // last base first, complemented
  return r;
}

static mc::AssignOptions parse(std::vector<std::string> args) {
  std::vector<char *> argv;
  for (auto &a : args) argv.push_back(&a[0]);
  return mc::parse_assign_options((int)argv.size(), argv.data());
}

int main(int argc, char **argv) {
  if (argc < 2) return fail("usage: strands_check <an existing file>");
  for (int k = 1; k <= 6; k++) {
    const uint32_t B = 1u << (2 * k);
    uint32_t fixed = 0;
    for (uint32_t i = 0; i < B; i++) {
      const uint32_t r = mc::rc_index(i, k);
      if (r >= B || r != rc_by_digits(i, k)) return fail("rc_index differs from the digit definition");
      if (mc::rc_index(r, k) != i) return fail("rc_index is not an involution");
      fixed += r == i;
    }
    if (fixed != (k % 2 ? 0u : 1u << k)) return fail("fixed points");
  }
  if (mc::rc_index(0, 3) != 63 || mc::rc_index(1, 2) != 11) return fail("AAA -> TTT, AC -> GT");
  const std::string f = argv[1];
  const mc::AssignOptions a = parse({"meshclust-assign", "--model", f, "--centres", f, f});
  if (a.both_strands) return fail("--both-strands is on by default");
  const mc::AssignOptions b = parse({"meshclust-assign", "--model", f, "--both-strands", "--centres", f, f, "--quiet"});
  if (!b.both_strands || !b.quiet || b.model != f || b.centres != f || b.reads.size() != 1 || b.output != a.output)
    return fail("--both-strands not stored, or it changed another option");
  bool named = false;
  try {
    parse({"meshclust-assign"});
  } catch (const mc::Error &e) {
    named = std::string(e.what()).find("--both-strands") != std::string::npos;
  }
  if (!named) return fail("the usage text does not name --both-strands");
  mc::AssignResult r;
  r.reads = 10;
  r.assigned = 7;
  r.path = "device";
  printf("OK\n%s\n", mc::assign_stats_json(r).c_str());
  r.strands = MC_STRAND_PLUS | MC_STRAND_MINUS;
  r.assigned_minus = 3;
  printf("%s\n", mc::assign_stats_json(r).c_str());
  return 0;
}
