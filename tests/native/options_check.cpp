// options_check.cpp -- parse_options (runner.cpp) with and without --save-model / --save-centres:
// the new options are accepted and every earlier default stays what it was.  Linked against the
// host objects of the CPU test harness.  Prints "OK" and exits 0, or says what failed.
#include <cstdio>
#include <string>
#include <vector>

#include "runner.hpp"

static int fail(const char *what) {
  printf("FAIL: %s\n", what);
  return 1;
}

static bool defaults(const mc::Options &o) {
  return o.k == -1 && o.similarity == 0.90 && o.iterations == 15 && o.delta == 5 && !o.align && o.sample_size == 0 &&
         o.pivots == 20 && o.threads == 0 && o.output == "output.clstr" && o.files.empty() && o.device == 0 &&
         o.devices.empty() && !o.quiet && o.stats_json.empty();
}

static mc::Options parse(std::vector<std::string> args) {
  std::vector<char *> argv;
  for (auto &a : args) argv.push_back(&a[0]);
  return mc::parse_options((int)argv.size(), argv.data(), false);
}

int main() {
  const mc::Options a = parse({"meshclust"});
  if (!defaults(a) || !a.save_model.empty() || !a.save_centres.empty()) return fail("defaults changed");
  const mc::Options b = parse({"meshclust", "--save-model", "m.txt", "--save-centres", "c.fa"});
  if (!defaults(b)) return fail("the new options changed an old default");
  if (b.save_model != "m.txt" || b.save_centres != "c.fa") return fail("new options not stored");
  const mc::Options c = parse({"meshclust", "--id", "0.8", "--save-centres", "c.fa", "--kmer", "4", "--quiet"});
  if (c.similarity != 0.8 || c.k != 4 || !c.quiet || c.save_centres != "c.fa" || !c.save_model.empty())
    return fail("mixed options");
  bool threw = false;
  try {
    parse({"meshclust", "--save-model"});  // no value: not an option, not a file
  } catch (const mc::Error &) {
    threw = true;
  }
  if (!threw) return fail("--save-model without a value was accepted");
  printf("OK\n");
  return 0;
}
