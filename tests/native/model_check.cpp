// model_check.cpp -- model.hpp's writer and reader, stand-alone: an mc_classifier holding -0.0,
// a denormal, 1/3 and 1e300 must come back memcmp-equal; a truncated file and a wrong first
// line must be rejected.  Prints "OK" and exits 0, or says what failed.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

#include "model.hpp"

static int fail(const char *what) {
  printf("FAIL: %s\n", what);
  return 1;
}

template <typename F>
static bool rejects(F f) {
  try {
    f();
  } catch (const mc::Error &) {
    return true;
  }
  return false;
}

int main(int argc, char **argv) {
  if (argc < 2) return fail("usage: model_check DIR");
  const std::string dir = argv[1];
  mc::Model m;  // (the constructor zeroes the classifier, padding included)
  m.k = 3;
  m.id = 0.9;
  m.align = 0;
  m.centres = 123456789012ull;
  mc_classifier &c = m.cls;
  c.n_single = 5;
  const uint16_t lk[5] = {MC_FEAT_LD, MC_FEAT_INTERSECTION, MC_FEAT_MANHATTAN, MC_FEAT_PEARSON, MC_FEAT_KULCZYNSKI2};
  for (int i = 0; i < 5; i++) {
    c.lookup[i] = lk[i];
    c.is_sim[i] = i & 1;
  }
  c.mins[0] = -0.0;
  c.mins[1] = 4.9406564584124654e-324;  // the smallest denormal
  c.mins[2] = 1.0 / 3.0;
  c.mins[3] = 1e300;
  c.mins[4] = -2.2250738585072009e-308;  // the largest denormal, negative
  c.maxs[0] = 0.1;
  c.maxs[1] = 1.7976931348623157e308;
  c.maxs[2] = 3.0000000000000004;
  c.maxs[3] = -1e-300;
  c.maxs[4] = 515.0;
  c.n_combo = 4;
  for (int i = 0; i < 4; i++) {
    c.combo_kind[i] = i % 2 ? MC_COMBO_SQUARED : MC_COMBO_SELF;
    c.combo_len[i] = 1 + i % 2;
    for (int j = 0; j < MC_MAX_COMBO_LEN; j++) c.combo_idx[i][j] = (i + j) % 5;
  }
  const double w[5] = {-12.345678901234567, 1.0 / 3.0, -0.0, 1e300, 4.9406564584124654e-324};
  for (int i = 0; i < 5; i++) c.weights[i] = w[i];
  const std::string path = dir + "/model.txt";
  mc::write_model(path, m);
  const mc::Model r = mc::read_model(path);
  if (memcmp(&r.cls, &m.cls, sizeof(mc_classifier)) != 0) return fail("classifier differs after the round trip");
  if (r.k != m.k || memcmp(&r.id, &m.id, 8) != 0 || r.align != m.align || r.centres != m.centres)
    return fail("k / id / align / centres differ after the round trip");
  if (!std::signbit(r.cls.mins[0]) || !std::signbit(r.cls.weights[2])) return fail("-0.0 lost its sign");
  const std::string text = mc::model_text(m);
  if (text.compare(0, 18, "meshclust-model 1\n") != 0) return fail("first line");
  // truncated: at every line end but the last, in the middle of a number, and without the newline
  size_t cuts = 0;
  for (size_t p = text.find('\n'); p != std::string::npos && p + 1 < text.size(); p = text.find('\n', p + 1), cuts++)
    if (!rejects([&] { mc::parse_model(text.substr(0, p + 1), "cut"); })) return fail("a file cut at a line end was accepted");
  if (cuts < 10) return fail("too few lines");
  if (!rejects([&] { mc::parse_model(text.substr(0, text.size() - 1), "cut"); })) return fail("missing final newline accepted");
  if (!rejects([&] { mc::parse_model(text.substr(0, text.size() / 2), "cut"); })) return fail("half a file accepted");
  if (!rejects([&] { mc::parse_model("", "empty"); })) return fail("empty file accepted");
  // a wrong first line
  if (!rejects([&] { mc::parse_model("meshclust-model 2\n" + text.substr(18), "v2"); })) return fail("version 2 accepted");
  if (!rejects([&] { mc::parse_model(text.substr(18), "nohdr"); })) return fail("missing first line accepted");
  if (!rejects([&] { mc::read_model(dir + "/does-not-exist"); })) return fail("missing file accepted");
  printf("OK\n");
  return 0;
}
