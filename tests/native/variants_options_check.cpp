// variants_options_check.cpp -- the --variants / --alleles / --haplotypes options of meshclust-assign, the
// parts that need no GPU:
//   * parse_assign_options: each FILE option is stored and implies --identity, and nothing else; the two
//     thresholds have their defaults, are stored, and refuse values outside their ranges; --band and
//     --quality are accepted beside any of the three
//   * assign_stats_json: the variant keys appear only with the options, and after every other key
// Prints "OK" and two JSON lines (without and with the options), or says what failed.  Linked
// against libmeshclust.so.  argv[1]: an existing file (stands for the model, the centres and the reads).
#include <cstdio>
#include <string>
#include <vector>

#include "assign.hpp"

static int fail(const std::string &what) {
  printf("FAIL: %s\n", what.c_str());
  return 1;
}

int main(int argc, char **argv) {
  if (argc < 2) return fail("usage: variants_options_check <an existing file>");
  const std::string f = argv[1];
  const std::vector<std::string> args{"meshclust-assign", "--model", f, "--centres", f, f};
  auto parse = [&](std::vector<std::string> more) {
    std::vector<std::string> v = args;
    v.insert(v.end(), more.begin(), more.end());
    std::vector<char *> av;
    for (auto &s : v) av.push_back(&s[0]);
    return mc::parse_assign_options((int)av.size(), av.data());
  };
  auto refused = [&](std::vector<std::string> more, const char *names) {
    try {
      parse(more);
    } catch (const mc::Error &e) {
      return e.code == 1 && std::string(e.what()).find(names) != std::string::npos;
    }
    return false;
  };
  const mc::AssignOptions plain = parse({});
  if (plain.any_variants() || plain.identity || plain.min_allele_frac != 0.2 || plain.min_allele_count != 2)
    return fail("the options are off by default, the thresholds 0.2 and 2");
  for (const char *name : {"--variants", "--alleles", "--haplotypes"}) {
    const mc::AssignOptions o = parse({name, "x.tsv"});
    const std::string &got = name[2] == 'v' ? o.variants : name[2] == 'a' ? o.alleles : o.haplotypes;
    if (got != "x.tsv" || !o.identity || !o.any_variants()) return fail(std::string(name) + " FILE is stored and implies --identity");
    if ((int)!o.variants.empty() + (int)!o.alleles.empty() + (int)!o.haplotypes.empty() != 1) return fail(std::string(name) + " sets one file");
    if (!o.paf.empty() || !o.consensus.empty() || !o.pileup.empty() || !o.msa.empty() || !o.profile.empty() || o.quality || o.band ||
        o.min_identity >= 0 || o.top != 0 || o.both_strands || o.min_allele_frac != 0.2 || o.min_allele_count != 2)
      return fail(std::string(name) + " FILE sets nothing else");
    if (!refused({name}, (std::string(name) + " FILE").c_str())) return fail(std::string(name) + " without a file is a usage error that names it");
    const mc::AssignOptions b = parse({name, "x.tsv", "--band", "--quality"});
    if (!b.band || !b.quality) return fail(std::string("--band and --quality are accepted beside ") + name);
  }
  const mc::AssignOptions all = parse({"--variants", "v", "--alleles", "a", "--haplotypes", "h", "--msa", "m", "--profile", "p",
                                       "--min-allele-frac", "0.05", "--min-allele-count", "1"});
  if (all.variants != "v" || all.alleles != "a" || all.haplotypes != "h" || all.msa != "m" || all.profile != "p" ||
      all.min_allele_frac != 0.05 || all.min_allele_count != 1)
    return fail("all of them together");
  if (parse({"--min-allele-frac", "1"}).min_allele_frac != 1.0 || parse({"--min-allele-count", "7"}).min_allele_count != 7)
    return fail("the ends of the ranges");
  if (parse({"--min-allele-frac", "0.5"}).identity) return fail("a threshold alone implies nothing");
  for (const char *bad : {"0", "-0.1", "1.5", "x", "0.2x", "nan"})
    if (!refused({"--min-allele-frac", bad}, "--min-allele-frac must be")) return fail(std::string("--min-allele-frac ") + bad + " is refused");
  for (const char *bad : {"0", "-3", "x", "2.5"})
    if (!refused({"--min-allele-count", bad}, "--min-allele-count must be")) return fail(std::string("--min-allele-count ") + bad + " is refused");
  if (!refused({"--band"}, "--band needs") || !refused({"--quality"}, "--quality needs")) return fail("--band and --quality alone are still refused");
  mc::AssignResult r;
  r.reads = 10;
  r.assigned = 7;
  r.path = "device";
  r.identity = true;
  r.identity_pairs = 7;
  r.msa = true;
  r.msa_pairs = 7;
  r.profile = true;
  r.profile_centres = 3;
  r.band = true;
  r.band_pairs = 7;
  printf("OK\n");
  printf("%s\n", mc::assign_stats_json(r).c_str());
  r.variants = true;
  r.variant_centres = 2;
  r.variant_sites = 9;
  r.allele_bytes = 63;
  r.variants_ms = 1.5;
  printf("%s\n", mc::assign_stats_json(r).c_str());
  return 0;
}
