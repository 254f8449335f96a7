// cigar.hpp -- mc_nw_align_strands' operation words on the host: the cg:Z: text of a PAF line,
// and a replay of a CIGAR over two byte strings (what a consumer would do with it; the tests'
// check that an alignment is complete and truthful).
//
// A word is run << 4 | op with BAM's codes: '=' (7) and 'X' (8) consume a base of each string,
// 'I' (1) a base of seq1 (the read) alone, 'D' (2) a base of seq2 (the centre) alone.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>

#include "../../../include/meshclust_amd.h"

namespace mc {

inline char cigar_op_char(uint32_t op) {
  return op == MC_CIGAR_EQ ? '=' : op == MC_CIGAR_X ? 'X' : op == MC_CIGAR_I ? 'I' : op == MC_CIGAR_D ? 'D' : '?';
}

// appends n words as text ("57=1X12=3D..."); an empty CIGAR is "*", as in SAM
inline void cigar_append(std::string &out, const uint32_t *words, uint64_t n) {
  if (n == 0) {
    out += '*';
    return;
  }
  char num[16];
  for (uint64_t k = 0; k < n; k++) {
    snprintf(num, sizeof num, "%u", words[k] >> 4);
    out += num;
    out += cigar_op_char(words[k] & 15u);
  }
}

struct CigarReplay {
  uint64_t columns = 0, eq = 0;      // alignment columns, '=' columns
  int64_t score = 0;                 // match 1, mismatch -1, a gap run of n: -(2 + n)
  uint64_t a_used = 0, b_used = 0;   // bases consumed (a complete CIGAR: la and lb)
  bool truthful = true;              // every '=' over equal bytes, every 'X' over different ones,
                                     // no unknown operation, no empty run, nothing past an end
};

inline CigarReplay cigar_replay(const uint32_t *words, uint64_t n, const uint8_t *a, uint64_t la, const uint8_t *b,
                                uint64_t lb) {
  CigarReplay r;
  for (uint64_t k = 0; k < n; k++) {
    const uint64_t run = words[k] >> 4;
    const uint32_t op = words[k] & 15u;
    if (run == 0) r.truthful = false;
    r.columns += run;
    if (op == MC_CIGAR_EQ || op == MC_CIGAR_X) {
      for (uint64_t t = 0; t < run; t++) {
        const uint64_t i = r.a_used + t, j = r.b_used + t;
        if (i >= la || j >= lb) {
          r.truthful = false;
          break;
        }
        if ((a[i] == b[j]) != (op == MC_CIGAR_EQ)) r.truthful = false;
      }
      r.a_used += run;
      r.b_used += run;
      if (op == MC_CIGAR_EQ) r.eq += run;
      r.score += op == MC_CIGAR_EQ ? (int64_t)run : -(int64_t)run;
    } else if (op == MC_CIGAR_I) {
      r.a_used += run;
      r.score -= 2 + (int64_t)run;
    } else if (op == MC_CIGAR_D) {
      r.b_used += run;
      r.score -= 2 + (int64_t)run;
    } else {
      r.truthful = false;
    }
  }
  if (r.a_used > la || r.b_used > lb) r.truthful = false;
  return r;
}

}  // namespace mc
