// topk_check.cpp -- the ordered insertion of host/topk.hpp (the one the assignment kernels and
// the pair-list path use), without a GPU:
//   * TopK<K> + topk_insert for the capacities 2, 4 and 8, and topk_insert_row for every run-time
//     capacity 1..8, on random streams of (value, strand) hits that arrive in index order, the
//     values drawn from a handful of distinct doubles so that ties are the rule
//   * the expectation: std::stable_sort of the whole stream by (value descending, strand
//     ascending) -- stable, so equal (value, strand) keep their arrival order, which is index
//     ascending -- cut at K and padded with (TOPK_NONE, -1.0, 0)
//   * streams shorter than K (the empty one included), a stream that is all one value on one
//     strand, and the issue's example: (j 3, minus) arrives before (j 5, plus) with equal values
//   * parse_assign_options / assign_stats_json: --top and --hits are stored, and the summary gains
//     "top" and "hits" only with them (the test compares the keys)
// Linked against libmeshclust.so.  Prints "OK", then two JSON lines; or says what failed.
#include <algorithm>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "assign.hpp"
#include "topk.hpp"

struct Hit {
  double v;
  uint32_t j, s;
};

static int fail(const char *what, int k = 0, int n = 0) {
  printf("FAIL: %s (capacity %d, stream of %d)\n", what, k, n);
  return 1;
}

static std::vector<Hit> expect(std::vector<Hit> h, int K) {
  std::stable_sort(h.begin(), h.end(), [](const Hit &a, const Hit &b) { return a.v > b.v || (a.v == b.v && a.s < b.s); });
  h.resize(K, Hit{-1.0, mc::TOPK_NONE, 0});
  return h;
}

template <int K>
static bool check_value(const std::vector<Hit> &stream) {
  mc::TopK<K> t;
  t.clear();
  for (const Hit &h : stream) mc::topk_insert(t, h.v, h.j, h.s);
  const std::vector<Hit> want = expect(stream, K);
  for (int i = 0; i < K; i++)
    if (t.v[i] != want[i].v || t.j[i] != want[i].j || t.strand(i) != want[i].s) return false;
  return (t.sm >> K) == 0;
}

static bool check_row(const std::vector<Hit> &stream, int K) {
  // guard slots on both sides: the insertion must stay inside its K slots
  std::vector<double> v(K + 2, -1.0);
  std::vector<uint32_t> j(K + 2, mc::TOPK_NONE);
  std::vector<uint8_t> s(K + 2, 0);
  v[0] = v[K + 1] = 77.0;
  j[0] = j[K + 1] = 77;
  s[0] = s[K + 1] = 7;
  uint32_t n = 0;
  for (const Hit &h : stream) {
    mc::topk_insert_row(&v[1], &j[1], &s[1], (uint32_t)K, std::min<uint32_t>(n, (uint32_t)K), h.v, h.j, h.s);
    n++;
  }
  const std::vector<Hit> want = expect(stream, K);
  for (int i = 0; i < K; i++)
    if (v[i + 1] != want[i].v || j[i + 1] != want[i].j || s[i + 1] != want[i].s) return false;
  return v[0] == 77.0 && v[K + 1] == 77.0 && j[0] == 77 && j[K + 1] == 77 && s[0] == 7 && s[K + 1] == 7;
}

static bool check_all(const std::vector<Hit> &stream, int *bad) {
  for (int K = 1; K <= 8; K++)
    if (!check_row(stream, K)) return *bad = K, false;
  if (!check_value<2>(stream)) return *bad = 2, false;
  if (!check_value<4>(stream)) return *bad = 4, false;
  if (!check_value<8>(stream)) return *bad = 8, false;
  return true;
}

static mc::AssignOptions parse(std::vector<std::string> args) {
  std::vector<char *> argv;
  for (auto &a : args) argv.push_back(&a[0]);
  return mc::parse_assign_options((int)argv.size(), argv.data());
}

int main(int argc, char **argv) {
  if (argc < 2) return fail("usage: topk_check <an existing file>");
  int bad = 0;
  // the example: equal values, the minus hit arrives first, the plus hit is listed first
  {
    const std::vector<Hit> ex{{0.75, 3, 1}, {0.75, 5, 0}};
    mc::TopK<2> t;
    t.clear();
    for (const Hit &h : ex) mc::topk_insert(t, h.v, h.j, h.s);
    if (t.j[0] != 5 || t.strand(0) != 0 || t.j[1] != 3 || t.strand(1) != 1) return fail("plus before minus on a tie", 2, 2);
    if (!check_all(ex, &bad)) return fail("the example", bad, 2);
  }
  const double values[5] = {0.5, 0.625, 0.75, 0.9990234375, 1.0};
  std::mt19937 rng(12345);
  for (int both = 0; both < 2; both++)
    for (int len = 0; len <= 40; len++)
      for (int rep = 0; rep < 25; rep++) {
        // index order: with both strands an entry's plus hit arrives before its minus hit
        std::vector<Hit> stream;
        uint32_t j = 0;
        const int nv = 1 + (int)(rng() % 5);
        while ((int)stream.size() < len) {
          const double v0 = values[rng() % nv], v1 = values[rng() % nv];
          const unsigned kind = both ? rng() % 3 : 0;  // plus alone, minus alone, both
          if (kind != 1) stream.push_back(Hit{v0, j, 0});
          if (kind != 0 && (int)stream.size() < len) stream.push_back(Hit{rng() % 2 ? v0 : v1, j, 1});
          j += 1 + rng() % 3;
        }
        if (!check_all(stream, &bad)) return fail("random stream", bad, len);
      }
  for (int len : {1, 3, 8, 9, 20}) {  // all one value: the list is the first K indices
    std::vector<Hit> stream;
    for (int i = 0; i < len; i++) stream.push_back(Hit{1.0, (uint32_t)(2 * i), 0});
    if (!check_all(stream, &bad)) return fail("a stream of one value", bad, len);
    for (int i = 0; i < len; i++) stream[i].s = 1;
    if (!check_all(stream, &bad)) return fail("a stream of one value on the minus strand", bad, len);
  }
  const std::string f = argv[1];
  const mc::AssignOptions a = parse({"meshclust-assign", "--model", f, "--centres", f, f});
  if (a.top != 0 || !a.hits.empty()) return fail("--top / --hits are on by default");
  const mc::AssignOptions b = parse({"meshclust-assign", "--model", f, "--top", "3", "--centres", f, f, "--hits", "h.tsv"});
  if (b.top != 3 || b.hits != "h.tsv" || b.both_strands || b.model != f || b.reads.size() != 1 || b.output != a.output)
    return fail("--top / --hits not stored, or they changed another option");
  mc::AssignResult r;
  r.reads = 10;
  r.assigned = 7;
  r.path = "device";
  printf("OK\n%s\n", mc::assign_stats_json(r).c_str());
  r.top = 3;
  r.hits = 17;
  printf("%s\n", mc::assign_stats_json(r).c_str());
  return 0;
}
