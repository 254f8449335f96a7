// cigar_check.cpp -- host/cigar.hpp, the parts of mc_nw_align_strands / --paf that need no GPU:
//   * cigar_append: operation words to the cg:Z: text, "*" for none
//   * cigar_replay: columns, '=' count, score under 1 / -1 / 2 / 1, bases consumed, and whether
//     every '=' / 'X' is truthful -- on hand-made alignments, on what it must refuse (an '=' over
//     different bytes, an 'X' over equal ones, a run past an end, an unknown operation, an empty
//     run), and on 2,000 random alignments built column by column with their own bookkeeping
//   * parse_assign_options: --paf FILE is stored and implies --identity
//   * assign_stats_json: "paf_pairs" and "cigar_ops" appear only with --paf
// Linked against libmeshclust.so.  Prints "OK", then two JSON lines; or says what failed.
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "assign.hpp"
#include "cigar.hpp"

static int fail(const char *what) {
  printf("FAIL: %s\n", what);
  return 1;
}

static uint32_t W(uint32_t run, uint32_t op) { return run << 4 | op; }

int main(int argc, char **argv) {
  if (argc < 2) return fail("usage: cigar_check <an existing file>");
  const uint32_t EQ = MC_CIGAR_EQ, X = MC_CIGAR_X, I = MC_CIGAR_I, D = MC_CIGAR_D;
  if (I != 1 || D != 2 || EQ != 7 || X != 8) return fail("the operation codes are BAM's");
  {
    std::string s = "cg:Z:";
    const uint32_t w[5] = {W(57, EQ), W(1, X), W(12, I), W(3, D), W(100000, EQ)};
    mc::cigar_append(s, w, 5);
    if (s != "cg:Z:57=1X12I3D100000=") return fail("cigar_append");
    std::string e;
    mc::cigar_append(e, w, 0);
    if (e != "*") return fail("an empty CIGAR is *");
  }
  {
    //  a  0 1 2 - - 3 0 1     b  0 1 3 2 2 3 1      2= 1X 2D 1= 1X 1I
    const uint8_t a[7] = {0, 1, 2, 3, 0, 1, 9}, b[7] = {0, 1, 3, 2, 2, 3, 1};
    const uint32_t w[6] = {W(2, EQ), W(1, X), W(2, D), W(1, EQ), W(1, X), W(1, I)};
    mc::CigarReplay r = mc::cigar_replay(w, 6, a, 6, b, 7);
    if (!r.truthful || r.columns != 8 || r.eq != 3 || r.a_used != 6 || r.b_used != 7) return fail("replay of a hand-made alignment");
    if (r.score != 3 - 2 - (2 + 2) - (2 + 1)) return fail("replayed score");
    const uint32_t lie1[1] = {W(3, EQ)};  // the third pair differs
    if (mc::cigar_replay(lie1, 1, a, 6, b, 7).truthful) return fail("an = over different bytes");
    const uint32_t lie2[1] = {W(1, X)};
    if (mc::cigar_replay(lie2, 1, a, 6, b, 7).truthful) return fail("an X over equal bytes");
    const uint32_t past[2] = {W(2, EQ), W(6, I)};
    if (mc::cigar_replay(past, 2, a, 6, b, 7).truthful) return fail("a run past the end of seq1");
    const uint32_t past2[2] = {W(2, EQ), W(5, X)};
    if (mc::cigar_replay(past2, 2, a, 6, b, 7).truthful) return fail("an X run past the end");
    const uint32_t unk[1] = {W(2, 0)};  // 'M' is not used
    if (mc::cigar_replay(unk, 1, a, 6, b, 7).truthful) return fail("an unknown operation");
    const uint32_t empty[2] = {W(0, EQ), W(2, EQ)};
    if (mc::cigar_replay(empty, 2, a, 6, b, 7).truthful) return fail("an empty run");
    mc::CigarReplay part = mc::cigar_replay(w, 3, a, 6, b, 7);  // incomplete: truthful, but not la / lb
    if (!part.truthful || part.a_used != 3 || part.b_used != 5) return fail("an incomplete CIGAR");
    mc::CigarReplay none = mc::cigar_replay(nullptr, 0, a, 0, b, 0);
    if (!none.truthful || none.columns || none.score) return fail("no operations");
  }
  std::mt19937 rng(7);
  const uint32_t kinds[4] = {EQ, X, I, D};
  for (int it = 0; it < 2000; it++) {  // random alignments, column by column
    std::vector<uint8_t> a, b;
    std::vector<uint32_t> w;
    long score = 0;
    uint64_t cols = 0, eq = 0;
    const int nruns = 1 + (int)(rng() % 12);
    uint32_t last = 99;
    for (int k = 0; k < nruns; k++) {
      uint32_t op;
      do op = kinds[rng() % 4];
      while (op == last);
      last = op;
      const uint32_t run = 1 + rng() % 40;
      for (uint32_t t = 0; t < run; t++) {
        const uint8_t c = (uint8_t)(rng() % 4);
        if (op == EQ) a.push_back(c), b.push_back(c);
        else if (op == X) a.push_back(c), b.push_back((uint8_t)((c + 1 + rng() % 3) % 4));
        else if (op == I) a.push_back(c);
        else b.push_back(c);
      }
      cols += run;
      if (op == EQ) eq += run, score += run;
      else if (op == X) score -= run;
      else score -= 2 + (long)run;
      w.push_back(W(run, op));
    }
    const mc::CigarReplay r = mc::cigar_replay(w.data(), w.size(), a.data(), a.size(), b.data(), b.size());
    if (!r.truthful || r.columns != cols || r.eq != eq || r.score != score || r.a_used != a.size() || r.b_used != b.size())
      return fail("a random alignment");
  }
  const std::string f = argv[1];
  std::vector<std::string> args{"meshclust-assign", "--model", f, "--centres", f, f};
  auto parse = [](std::vector<std::string> v) {
    std::vector<char *> av;
    for (auto &s : v) av.push_back(&s[0]);
    return mc::parse_assign_options((int)av.size(), av.data());
  };
  const mc::AssignOptions plain = parse(args);
  if (!plain.paf.empty() || plain.identity) return fail("--paf is off by default");
  args.push_back("--paf");
  args.push_back("out.paf");
  const mc::AssignOptions o = parse(args);
  if (o.paf != "out.paf" || !o.identity || o.min_identity >= 0 || o.top != 0) return fail("--paf FILE implies --identity");
  mc::AssignResult r;
  r.reads = 10;
  r.assigned = 7;
  r.path = "device";
  r.identity = true;
  r.identity_pairs = 21;
  printf("OK\n%s\n", mc::assign_stats_json(r).c_str());
  r.paf = true;
  r.paf_pairs = 21;
  r.cigar_ops = 88;
  printf("%s\n", mc::assign_stats_json(r).c_str());
  return 0;
}
