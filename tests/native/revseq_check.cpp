// revseq_check.cpp -- the minus-strand byte rule of host/revseq.hpp (the one gpu/revseq.hip
// applies), without a GPU:
//   * rc_byte on all 256 values: digits d <= 3 -> 3 - d, A <-> T, C <-> G, everything else
//     ('N', lower case, 0xFF) unchanged; an involution
//   * rc_word, the kernel's four-bytes-at-once form, equals rc_byte on every byte: words of digits
//     only (the one-xor path), and words that mix digits, letters, 'N' and other bytes
//   * revseq: the string reversed and mapped; the reverse of the reverse is the string itself,
//     for lengths 0 .. 70 and 1,000, on strings of digits with N runs and on raw letters; a
//     reverse palindrome s + revseq(s) is its own minus strand
// Header only.  Prints "OK", or says what failed.
#include <cstdio>
#include <random>
#include <vector>

#include "revseq.hpp"

static int fail(const char *what, long v = 0) {
  printf("FAIL: %s (%ld)\n", what, v);
  return 1;
}

int main() {
  for (int v = 0; v < 256; v++) {
    const uint8_t d = (uint8_t)v, r = mc::rc_byte(d);
    uint8_t want = d;
    if (v <= 3) want = (uint8_t)(3 - v);
    else if (v == 'A') want = 'T';
    else if (v == 'T') want = 'A';
    else if (v == 'C') want = 'G';
    else if (v == 'G') want = 'C';
    if (r != want) return fail("rc_byte", v);
    if (mc::rc_byte(r) != d) return fail("rc_byte is not an involution", v);
  }
  if (mc::rc_byte('N') != 'N' || mc::rc_byte('a') != 'a' || mc::rc_byte(0xFF) != 0xFF) return fail("a byte that stays");
  std::mt19937 rng(2024);
  const uint8_t alphabet[12] = {0, 1, 2, 3, 'A', 'C', 'G', 'T', 'N', 'a', 4, 0xFF};
  for (int rep = 0; rep < 20000; rep++) {
    uint32_t w = 0;
    const bool digits = rep % 2 == 0;
    for (int i = 0; i < 4; i++) w |= (uint32_t)alphabet[rng() % (digits ? 4 : 12)] << (8 * i);
    const uint32_t r = mc::rc_word(w);
    for (int i = 0; i < 4; i++)
      if ((uint8_t)(r >> (8 * i)) != mc::rc_byte((uint8_t)(w >> (8 * i)))) return fail("rc_word", (long)w);
    if (mc::rc_word(r) != w) return fail("rc_word is not an involution", (long)w);
  }
  std::vector<int> lens;
  for (int l = 0; l <= 70; l++) lens.push_back(l);
  lens.push_back(1000);
  for (int raw = 0; raw < 2; raw++)
    for (int len : lens) {
      std::vector<uint8_t> s(len), r(len), rr(len);
      for (int i = 0; i < len; i++) s[i] = raw ? alphabet[4 + rng() % 5] : (rng() % 11 == 0 ? (uint8_t)'N' : (uint8_t)(rng() % 4));
      mc::revseq(s.data(), s.size(), r.data());
      for (int i = 0; i < len; i++)
        if (r[i] != mc::rc_byte(s[len - 1 - i])) return fail("revseq", len);
      mc::revseq(r.data(), r.size(), rr.data());
      if (rr != s) return fail("the reverse of the reverse", len);
      std::vector<uint8_t> p(s);  // s + revseq(s) is its own minus strand
      p.insert(p.end(), r.begin(), r.end());
      std::vector<uint8_t> pr(p.size());
      mc::revseq(p.data(), p.size(), pr.data());
      if (pr != p) return fail("a reverse palindrome", len);
    }
  printf("OK\n");
  return 0;
}
