// model.hpp -- what read assignment needs from a finished clustering, as two files:
//   the model   a text file, first line "meshclust-model 1", then `key value...` lines: k, id,
//               align, every field of mc_classifier, the number of centres.  Doubles are C99 hex
//               floats (%a), so a reload is bit-exact.  A clustering on both strands (meshclust
//               --both-strands: canonical rows) writes "meshclust-model 2" and a line "strands 3"
//               after align; version 1 means strands 1, a version 2 without `strands` is refused.
//   the centres a FASTA of the final centres in cluster order: header lines unchanged, each
//               sequence on one line, ACGT for the codes 0..3 and the stored exception byte
//               elsewhere -- re-parsing gives the same lengths, segments and in-segment codes.
// Header-only: bin/meshclust's objects are also linked against the CPU oracle engine by the
// test harness, so they may not depend on any new translation unit.
#pragma once
#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "common.hpp"
#include "fasta.hpp"

namespace mc {

struct Model {
  int k = 0;
  double id = 0;
  int align = 0;
  int strands = 1;  // 3: trained and clustered on canonical rows (version 2)
  mc_classifier cls;
  uint64_t centres = 0;
  Model() { memset(&cls, 0, sizeof cls); }
};

inline std::string model_text(const Model &m) {
  std::string o = m.strands == 1 ? "meshclust-model 1\n" : "meshclust-model 2\n";
  char b[64];
  auto ints = [&](const char *key, const long long *v, int n) {
    o += key;
    for (int i = 0; i < n; i++) {
      snprintf(b, sizeof b, " %lld", v[i]);
      o += b;
    }
    o += '\n';
  };
  auto dbls = [&](const char *key, const double *v, int n) {
    o += key;
    for (int i = 0; i < n; i++) {
      snprintf(b, sizeof b, " %a", v[i]);
      o += b;
    }
    o += '\n';
  };
  auto one = [&](const char *key, long long v) { ints(key, &v, 1); };
  const mc_classifier &c = m.cls;
  long long t[MC_MAX_COMBO * MC_MAX_COMBO_LEN];
  one("k", m.k);
  dbls("id", &m.id, 1);
  one("align", m.align);
  if (m.strands != 1) one("strands", m.strands);
  one("n_single", c.n_single);
  for (int i = 0; i < MC_MAX_SINGLE; i++) t[i] = c.lookup[i];
  ints("lookup", t, MC_MAX_SINGLE);
  for (int i = 0; i < MC_MAX_SINGLE; i++) t[i] = c.is_sim[i];
  ints("is_sim", t, MC_MAX_SINGLE);
  dbls("mins", c.mins, MC_MAX_SINGLE);
  dbls("maxs", c.maxs, MC_MAX_SINGLE);
  one("n_combo", c.n_combo);
  for (int i = 0; i < MC_MAX_COMBO; i++) t[i] = c.combo_kind[i];
  ints("combo_kind", t, MC_MAX_COMBO);
  for (int i = 0; i < MC_MAX_COMBO; i++) t[i] = c.combo_len[i];
  ints("combo_len", t, MC_MAX_COMBO);
  for (int i = 0; i < MC_MAX_COMBO; i++)
    for (int j = 0; j < MC_MAX_COMBO_LEN; j++) t[i * MC_MAX_COMBO_LEN + j] = c.combo_idx[i][j];
  ints("combo_idx", t, MC_MAX_COMBO * MC_MAX_COMBO_LEN);
  dbls("weights", c.weights, MC_MAX_COMBO + 1);
  one("centres", (long long)m.centres);
  return o;
}

inline void write_model(const std::string &path, const Model &m) {
  FILE *f = fopen(path.c_str(), "w");
  if (!f) throw Error("cannot write model file " + path + ": " + strerror(errno));
  const std::string t = model_text(m);
  const bool ok = fwrite(t.data(), 1, t.size(), f) == t.size();
  if (fclose(f) != 0 || !ok) throw Error("cannot write model file " + path);
}

// Throws mc::Error on a wrong first line, a missing or repeated key, or a wrong value count
// (a truncated file misses its last keys or values).
inline Model parse_model(const std::string &text, const std::string &name) {
  std::istringstream in(text);
  std::string line;
  if (!std::getline(in, line) || (line != "meshclust-model 1" && line != "meshclust-model 2"))
    throw Error(name + ": not a meshclust model (first line must be \"meshclust-model 1\" or \"meshclust-model 2\")");
  const int version = line.back() - '0';
  std::map<std::string, std::vector<std::string>> kv;
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    std::string key, v;
    if (!(ls >> key)) continue;
    if (kv.count(key)) throw Error(name + ": key " + key + " appears twice");
    auto &vals = kv[key];
    while (ls >> v) vals.push_back(v);
  }
  if (text.empty() || text.back() != '\n') throw Error(name + ": truncated model file (no final newline)");
  auto get = [&](const char *key, size_t n) -> const std::vector<std::string> & {
    auto it = kv.find(key);
    if (it == kv.end()) throw Error(name + ": truncated or incomplete model file (no " + key + ")");
    if (it->second.size() != n) throw Error(name + ": key " + key + " has the wrong number of values");
    return it->second;
  };
  auto to_ll = [&](const std::string &s) {
    char *end = nullptr;
    errno = 0;
    const long long v = strtoll(s.c_str(), &end, 10);
    if (errno || end == s.c_str() || *end) throw Error(name + ": bad integer " + s);
    return v;
  };
  auto to_d = [&](const std::string &s) {
    char *end = nullptr;
    const double v = strtod(s.c_str(), &end);  // (hex floats included)
    if (end == s.c_str() || *end) throw Error(name + ": bad number " + s);
    return v;
  };
  Model m;
  mc_classifier &c = m.cls;
  m.k = (int)to_ll(get("k", 1)[0]);
  m.id = to_d(get("id", 1)[0]);
  m.align = (int)to_ll(get("align", 1)[0]);
  if (version >= 2) {
    m.strands = (int)to_ll(get("strands", 1)[0]);
    if (m.strands != 1 && m.strands != 3) throw Error(name + ": strands must be 1 or 3");
  }
  c.n_single = (int32_t)to_ll(get("n_single", 1)[0]);
  c.n_combo = (int32_t)to_ll(get("n_combo", 1)[0]);
  for (int i = 0; i < MC_MAX_SINGLE; i++) {
    c.lookup[i] = (uint16_t)to_ll(get("lookup", MC_MAX_SINGLE)[i]);
    c.is_sim[i] = (int32_t)to_ll(get("is_sim", MC_MAX_SINGLE)[i]);
    c.mins[i] = to_d(get("mins", MC_MAX_SINGLE)[i]);
    c.maxs[i] = to_d(get("maxs", MC_MAX_SINGLE)[i]);
  }
  for (int i = 0; i < MC_MAX_COMBO; i++) {
    c.combo_kind[i] = (int32_t)to_ll(get("combo_kind", MC_MAX_COMBO)[i]);
    c.combo_len[i] = (int32_t)to_ll(get("combo_len", MC_MAX_COMBO)[i]);
    for (int j = 0; j < MC_MAX_COMBO_LEN; j++)
      c.combo_idx[i][j] = (int32_t)to_ll(get("combo_idx", MC_MAX_COMBO * MC_MAX_COMBO_LEN)[i * MC_MAX_COMBO_LEN + j]);
  }
  for (int i = 0; i <= MC_MAX_COMBO; i++) c.weights[i] = to_d(get("weights", MC_MAX_COMBO + 1)[i]);
  m.centres = (uint64_t)to_ll(get("centres", 1)[0]);
  if (m.k < 0 || m.k > 12 || c.n_single < 1 || c.n_single > MC_MAX_SINGLE || c.n_combo < 1 || c.n_combo > MC_MAX_COMBO)
    throw Error(name + ": model values out of range");
  return m;
}

inline Model read_model(const std::string &path) {
  FILE *f = fopen(path.c_str(), "r");
  if (!f) throw Error("cannot read model file " + path + ": " + strerror(errno));
  std::string text;
  char buf[4096];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, n);
  fclose(f);
  return parse_model(text, path);
}

// Records ids[0..n) of a parsed dataset as FASTA text: the header line as read, then the
// upper-cased sequence on one line.
inline void append_fasta(std::string &out, const Dataset &ds, const uint32_t *ids, size_t n) {
  static const char L[4] = {'A', 'C', 'G', 'T'};
  for (size_t q = 0; q < n; q++) {
    const uint32_t i = ids[q];
    if (i >= ds.size()) throw Error("FASTA writer: record id out of range");
    out.append(ds.headers[i]);
    out += '\n';
    const uint64_t len = ds.seq_off[i + 1] - ds.seq_off[i];
    const size_t at = out.size();
    out.resize(at + len);
    const uint32_t *w = ds.packed.data() + ds.pk_off[i];
    for (uint64_t j = 0; j < len; j++) out[at + j] = L[(w[j / 16] >> (2 * (j % 16))) & 3u];
    auto e = std::lower_bound(ds.exc_pos.begin(), ds.exc_pos.end(), ds.seq_off[i]);
    for (; e != ds.exc_pos.end() && *e < ds.seq_off[i + 1]; ++e)
      out[at + (*e - ds.seq_off[i])] = (char)ds.exc_val[e - ds.exc_pos.begin()];
    out += '\n';
  }
}

inline void write_fasta(const std::string &path, const Dataset &ds, const uint32_t *ids, size_t n) {
  std::string text;
  append_fasta(text, ds, ids, n);
  FILE *f = fopen(path.c_str(), "w");
  if (!f) throw Error("cannot write " + path + ": " + strerror(errno));
  const bool ok = fwrite(text.data(), 1, text.size(), f) == text.size();
  if (fclose(f) != 0 || !ok) throw Error("cannot write " + path);
}

}  // namespace mc
