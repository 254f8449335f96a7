// cluster_strands_check.cpp -- meshclust --both-strands, the host parts that need no engine: the
// model text (version 1 byte-identical to what it was, version 2 with its `strands` line, a
// version 2 without it refused), the options, and find_k's formula on the doubled length.  Linked
// against the host objects of the CPU test harness.  Prints "OK" and exits 0, or says what failed.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "model.hpp"
#include "runner.hpp"

static int fail(const char *what) {
  printf("FAIL: %s\n", what);
  return 1;
}

static mc::Options parse(std::vector<std::string> args) {
  std::vector<char *> argv;
  for (auto &a : args) argv.push_back(&a[0]);
  return mc::parse_options((int)argv.size(), argv.data(), false);
}

template <typename F>
static std::string message(F f) {
  try {
    f();
  } catch (const mc::Error &e) {
    return e.code == EXIT_FAILURE ? e.what() : "";
  }
  return "";
}

int main() {
  mc::Model m;
  m.k = 5;
  m.id = 0.85;
  m.cls.n_single = 4;
  m.cls.n_combo = 3;
  for (int i = 0; i < MC_MAX_SINGLE; i++) {
    m.cls.lookup[i] = (uint16_t)(i + 1);
    m.cls.mins[i] = i / 3.0;
    m.cls.maxs[i] = 1 + i / 7.0;
  }
  for (int i = 0; i <= MC_MAX_COMBO; i++) m.cls.weights[i] = -0.25 * i;
  m.centres = 60;
  // version 1: the text of a model without the new field, line for line what it was
  const std::string v1 = mc::model_text(m);
  if (v1.compare(0, 18, "meshclust-model 1\n") != 0 || v1.find("strands") != std::string::npos) return fail("version 1 text");
  const mc::Model r1 = mc::parse_model(v1, "v1");
  if (r1.strands != 1 || mc::model_text(r1) != v1) return fail("version 1 round trip");
  // version 2
  m.strands = 3;
  const std::string v2 = mc::model_text(m);
  if (v2.compare(0, 18, "meshclust-model 2\n") != 0) return fail("version 2 first line");
  const size_t at = v2.find("strands 3\n");
  if (at == std::string::npos) return fail("version 2 has no strands line");
  if ("meshclust-model 1\n" + v2.substr(18, at - 18) + v2.substr(at + 10) != v1) return fail("version 2 differs elsewhere");
  const mc::Model r2 = mc::parse_model(v2, "v2");
  if (r2.strands != 3 || r2.k != 5 || r2.centres != 60 || mc::model_text(r2) != v2) return fail("version 2 round trip");
  if (memcmp(&r2.cls, &m.cls, sizeof m.cls) != 0) return fail("version 2 classifier");
  if (message([&] { mc::parse_model(v2.substr(0, at) + v2.substr(at + 10), "nostrands"); }).find("strands") == std::string::npos)
    return fail("a version 2 without strands was accepted");
  if (message([&] { mc::parse_model(v2.substr(0, at) + "strands 2\n" + v2.substr(at + 10), "bad"); }).empty())
    return fail("strands 2 was accepted");
  printf("%s", v1.c_str());
  // options
  const mc::Options a = parse({"meshclust"});
  if (a.both_strands || !a.strands_file.empty()) return fail("defaults");
  const mc::Options b = parse({"meshclust", "--both-strands", "--strands", "s.tsv", "--kmer", "4"});
  if (!b.both_strands || b.strands_file != "s.tsv" || b.k != 4 || b.align) return fail("the new options");
  const std::string e1 = message([&] { parse({"meshclust", "--both-strands", "--align"}); });
  if (e1.find("--both-strands") == std::string::npos || e1.find("--align") == std::string::npos) return fail("flag with --align");
  const std::string e2 = message([&] { parse({"meshclust", "--id", "0.5", "--both-strands"}); });
  if (e2.find("--both-strands") == std::string::npos || e2.find("--id") == std::string::npos || e2.find("--align") == std::string::npos)
    return fail("flag with --id below 0.6");
  const std::string e3 = message([&] { parse({"meshclust", "--strands", "s.tsv"}); });
  if (e3.find("--strands needs --both-strands") == std::string::npos) return fail("--strands without the flag");
  // find_k on the doubled length
  if (mc::recommended_k(2 * 1000) != 5 || mc::recommended_k(2 * 400) != 4) return fail("k of the doubled length");
  if (mc::recommended_k(1000) != 4 || mc::recommended_k(400) != 4 || mc::recommended_k(500) != 4) return fail("k of the length");
  printf("OK\n");
  return 0;
}
