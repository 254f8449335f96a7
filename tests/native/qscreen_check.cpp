// qscreen_check.cpp -- host/qscreen.hpp against the CPU oracle's NW identity (oracle/mc_oracle.c).
// Stand-alone: g++ -I meshclust_amd/csrc/host -I oracle qscreen_check.cpp mc_oracle.o [-fopenmp].
//   safety      below() never holds for a pair whose oracle identity is >= c
//   edge cases  identity == c exactly, identical strings, lengths 2x apart, length q - 1, an 'N'
//   not vacuous unrelated 1 kb pairs are screened at c = 0.9, reads 3 % from one template never
// Prints counts and "OK"; any failure prints the case and exits 1.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "qscreen.hpp"

extern "C" {
#include "mc_oracle.h"
}

using Str = std::vector<uint8_t>;  // one-digit bytes: 0..3, or 'N'

static mc::Dataset make_ds(const std::vector<Str> &recs) {
  mc::Dataset ds;
  const size_t n = recs.size();
  ds.seq_off.assign(1, 0);
  ds.pk_off.assign(1, 0);
  ds.seg_off.assign(1, 0);
  for (const Str &r : recs) {
    ds.seq_off.push_back(ds.seq_off.back() + r.size());
    ds.pk_off.push_back(ds.pk_off.back() + (r.size() + 15) / 16);
    ds.lengths.push_back(r.size());
  }
  ds.packed.resize(ds.pk_off[n]);
  for (size_t w = 0; w < ds.pk_off[n]; w++) ds.packed[w] = 0;
  for (size_t i = 0; i < n; i++) {
    const Str &r = recs[i];
    int64_t start = -1;  // segments: the maximal runs of digits, as the parser leaves them
    for (size_t j = 0; j <= r.size(); j++) {
      const bool digit = j < r.size() && r[j] <= 3;
      if (digit) ds.packed[ds.pk_off[i] + j / 16] |= (uint32_t)r[j] << (2 * (j % 16));
      if (j < r.size() && !digit) {
        ds.exc_pos.push_back(ds.seq_off[i] + j);
        ds.exc_val.push_back(r[j]);
      }
      if (digit && start < 0) start = (int64_t)j;
      if (!digit && start >= 0) {
        ds.seg.push_back((int32_t)start);
        ds.seg.push_back((int32_t)j - 1);
        start = -1;
      }
    }
    ds.seg_off.push_back(ds.seg.size() / 2);
  }
  return ds;
}

static double oracle_identity(const Str &a, const Str &b) {
  int sc, len, ids;
  double id;
  mco_nw(a.data(), (int)a.size(), b.data(), (int)b.size(), 1, -1, 2, 1, &sc, &len, &ids, &id);
  return id;
}

// the count, restated: a map of q-gram strings
static uint32_t common_naive(const Str &a, const Str &b, int q) {
  if ((int)a.size() < q || (int)b.size() < q) return mc::qscreen::NA;
  for (const Str *s : {&a, &b})
    for (uint8_t c : *s)
      if (c > 3) return mc::qscreen::NA;
  std::map<std::string, int> occ;
  for (size_t j = 0; j + q <= a.size(); j++) occ[std::string(a.begin() + j, a.begin() + j + q)]++;
  uint32_t c = 0;
  for (size_t j = 0; j + q <= b.size(); j++) {
    auto it = occ.find(std::string(b.begin() + j, b.begin() + j + q));
    if (it != occ.end() && it->second > 0) {
      it->second--;
      c++;
    }
  }
  return c;
}

static Str revcomp(const Str &a) {
  Str r(a.rbegin(), a.rend());
  for (uint8_t &c : r)
    if (c <= 3) c = (uint8_t)(3 - c);
  return r;
}

static Str uniform(std::mt19937_64 &rng, size_t len) {
  Str s(len);
  for (auto &c : s) c = (uint8_t)(rng() & 3);
  return s;
}

// substitutions and indels, each base touched with probability div (a third each: substitute, delete, insert)
static Str mutate(std::mt19937_64 &rng, const Str &a, double div) {
  std::uniform_real_distribution<double> u(0, 1);
  Str b;
  for (uint8_t c : a) {
    if (u(rng) >= div) {
      b.push_back(c);
      continue;
    }
    const int kind = (int)(rng() % 3);
    if (kind == 0) b.push_back((uint8_t)((c + 1 + rng() % 3) & 3));
    else if (kind == 2) {
      b.push_back(c);
      b.push_back((uint8_t)(rng() & 3));
    }
  }
  return b;
}

#define FAIL(...)                 \
  do {                            \
    printf("FAIL: " __VA_ARGS__); \
    printf("\n");                 \
    exit(1);                      \
  } while (0)

int main() {
  using namespace mc::qscreen;
  const double cut[5] = {0.6, 0.8, 0.9, 0.95, 0.97};
  if (pick_q(0.6) != 0 || pick_q(0.8) != 0 || pick_q(0.9) != 7 || pick_q(0.95) != 7 || pick_q(0.97) != 7)
    FAIL("pick_q");
  std::mt19937_64 rng(20261021);

  // ---- safety: 20,000 random pairs, lengths 7-600, 0-40 % divergence (and some unrelated ones)
  const size_t M = 20000;
  std::vector<Str> recs(2 * M);
  for (size_t p = 0; p < M; p++) {
    Str a = uniform(rng, 7 + rng() % 594);
    Str b;
    if (p % 10 == 9) b = uniform(rng, 7 + rng() % 594);
    else
      do b = mutate(rng, a, 0.4 * (double)(rng() % 1001) / 1000.0);
      while (b.size() < 7 || b.size() > 600);
    recs[2 * p] = a;
    recs[2 * p + 1] = b;
  }
  const mc::Dataset ds = make_ds(recs);
  std::vector<double> ident(M);
#pragma omp parallel for schedule(dynamic, 64)
  for (size_t p = 0; p < M; p++) ident[p] = oracle_identity(recs[2 * p], recs[2 * p + 1]);
  size_t screened[5] = {0, 0, 0, 0, 0}, below_cut[5] = {0, 0, 0, 0, 0}, naive_checked = 0;
  for (size_t p = 0; p < M; p++) {
    const uint32_t ia = (uint32_t)(2 * p), ib = ia + 1;
    for (int q = 1; q <= QMAX; q++) {
      const uint32_t C = common(ds, ia, ib, false, q);
      if (p % 50 == 0) {  // the count itself, both strands, against the restatement
        if (C != common_naive(recs[ia], recs[ib], q)) FAIL("count, pair %zu q %d", p, q);
        if (common(ds, ia, ib, true, q) != common_naive(revcomp(recs[ia]), recs[ib], q)) FAIL("minus count, pair %zu q %d", p, q);
        naive_checked++;
      }
      for (int k = 0; k < 5; k++) {
        if (q == 1) below_cut[k] += ident[p] < cut[k];
        if (!below(C, recs[ia].size(), recs[ib].size(), cut[k], q)) continue;
        if (!(ident[p] < cut[k])) FAIL("pair %zu (la %zu lb %zu) screened at c %.2f q %d, identity %.6f", p, recs[ia].size(), recs[ib].size(), cut[k], q, ident[p]);
        if (q == pick_q(cut[k])) screened[k]++;
      }
    }
  }
  for (int k = 0; k < 5; k++) printf("safety c %.2f q %d : %zu below the cutoff, %zu screened\n", cut[k], pick_q(cut[k]), below_cut[k], screened[k]);
  printf("counts checked %zu\n", naive_checked);
  if (screened[2] < 1000 || screened[3] < 1000 || screened[4] < 1000) FAIL("the safety set screens too few pairs to test anything");

  // ---- constructed edge cases
  {
    Str a = uniform(rng, 500), b = a;
    for (size_t j = 4; j < b.size(); j += 5) b[j] = (uint8_t)((b[j] + 1) & 3);  // every 5th base: identity 0.8 exactly
    Str half(a.begin(), a.begin() + 250), shortq = uniform(rng, 6), withn = a;
    withn[77] = 'N';
    Str far = uniform(rng, 250);
    const std::vector<Str> e = {a, b, half, shortq, withn, far};
    const mc::Dataset d = make_ds(e);
    if (oracle_identity(a, b) != 0.8) FAIL("every-5th pair: identity %.17g, expected 0.8", oracle_identity(a, b));
    for (int q = 1; q <= QMAX; q++) {
      if (below(common(d, 0, 1, false, q), 500, 500, 0.8, q)) FAIL("identity == c screened, q %d", q);
      if (common(d, 0, 0, false, q) != 500u - (uint32_t)q + 1) FAIL("identical strings: count, q %d", q);
      for (double c : cut) {
        if (below(common(d, 0, 0, false, q), 500, 500, c, q)) FAIL("identical strings screened");
        // lengths 2x apart: a prefix (identity 0.5) and an unrelated half-length string
        for (uint32_t o : {2u, 5u})
          if (below(common(d, 0, o, false, q), 500, 250, c, q) && !(oracle_identity(e[0], e[o]) < c)) FAIL("2x lengths, q %d c %.2f", q, c);
      }
      if (common(d, 0, 4, false, q) != NA || common(d, 4, 0, true, q) != NA) FAIL("a read with N must be not available");
      if (below(NA, 500, 500, 0.9, q)) FAIL("not available screened");
    }
    if (common(d, 0, 3, false, 7) != NA || common(d, 3, 0, false, 7) != NA) FAIL("length q - 1 must be not available");
    if (common(d, 0, 3, false, 6) == NA) FAIL("length q is available");
    if (!below(common(d, 0, 5, false, 7), 500, 250, 0.9, 7)) FAIL("an unrelated string of half the length is screened at 0.9");
    if (common(d, 0, 1, false, 0) != NA || common(d, 0, 1, false, 8) != NA) FAIL("q out of range");
  }

  // ---- not vacuous at c = 0.9, 1 kb, q = 7
  {
    const int q = pick_q(0.9);
    std::vector<Str> u, r;
    for (int p = 0; p < 200; p++) {
      u.push_back(uniform(rng, 1000));
      u.push_back(uniform(rng, 1000));
      const Str t = uniform(rng, 1000);
      r.push_back(mutate(rng, t, 0.03));
      r.push_back(mutate(rng, t, 0.03));
    }
    const mc::Dataset du = make_ds(u), dr = make_ds(r);
    int su = 0, sr = 0;
    uint32_t umax = 0, rmin = NA;
    for (uint32_t p = 0; p < 200; p++) {
      const uint32_t cu = common(du, 2 * p, 2 * p + 1, false, q), cr = common(dr, 2 * p, 2 * p + 1, false, q);
      umax = std::max(umax, cu);
      rmin = std::min(rmin, cr);
      su += below(cu, u[2 * p].size(), u[2 * p + 1].size(), 0.9, q);
      sr += below(cr, r[2 * p].size(), r[2 * p + 1].size(), 0.9, q);
    }
    printf("1 kb c 0.90 q %d : unrelated screened %d / 200 (max C %u), related screened %d / 200 (min C %u)\n", q, su, umax, sr, rmin);
    if (su < 198) FAIL("fewer than 99 %% of the unrelated pairs screened");
    if (sr != 0) FAIL("a related pair screened");
  }
  printf("OK\n");
  return 0;
}
