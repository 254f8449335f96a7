// consensus.hpp -- a cluster's consensus from its centre and mc_nw_pileup_strands' rows (host
// side of meshclust-assign --consensus / --pileup; native check tests/native/consensus_check.cpp).
//
// A centre of L bytes has L + 1 rows of MC_PILEUP_CH counters: channels 0..3 the reads' digits
// over that column, 4 any other read byte (N, raw letters), 5 reads that skip the column ('D'),
// 6 reads with an insertion before it, 7 the bases they insert (include/meshclust_amd.h).
//   column r < L   the largest of channels 0..5 wins; on a tie the centre's own channel if it is
//                  among the tied, else the lowest; depth 0 keeps the centre's byte.  Channels
//                  0..3 write A C G T, 4 writes N, 5 leaves the column out.
//   site r <= L    an insertion is applied before column r (r = L: after the last) iff
//                  2 * channel 6 > depth.  Its length is the most frequent length among the
//                  reads' 'I' runs there (ties: the shortest); its base t the plurality class
//                  (0..3, anything else N) among the runs longer than t (ties: the lowest class).
// The table does not hold the inserted bases: the caller reads them from the operation words of
// the centre's pairs (insertion_runs) -- only centres with a site need that.
// qconsensus_of (below; native check tests/native/qconsensus_check.cpp) is the same consensus
// decided by mc_nw_qpileup_strands' quality weights, with a quality per emitted base.
#pragma once
#include <algorithm>
#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "../../../include/meshclust_amd.h"

namespace mc {

inline uint32_t pileup_channel(uint8_t b) { return b <= 3 ? b : 4u; }
inline char pileup_base_char(uint8_t b) { return b <= 3 ? "ACGT"[b] : (char)b; }  // (as the FASTA writer, model.hpp)

// the winning channel (0..5) of a column over the centre byte b
inline uint32_t consensus_channel(const uint32_t *row, uint8_t b) {
  uint32_t top = 0;
  for (uint32_t ch = 0; ch < 6; ch++) top = std::max(top, row[ch]);
  const uint32_t own = pileup_channel(b);
  if (row[own] == top) return own;
  for (uint32_t ch = 0; ch < 6; ch++)
    if (row[ch] == top) return ch;
  return own;
}

// the rows 0 .. L of a centre at which an insertion is applied
inline std::vector<uint64_t> insertion_sites(const uint32_t *rows, uint64_t L, uint64_t depth) {
  std::vector<uint64_t> sites;
  for (uint64_t r = 0; r <= L; r++)
    if (2 * (uint64_t)rows[r * MC_PILEUP_CH + 6] > depth) sites.push_back(r);
  return sites;
}

using InsertionRuns = std::map<uint64_t, std::vector<std::vector<uint8_t>>>;  // row -> the reads' inserted bytes

// the 'I' runs of one alignment (words, read bytes as aligned: the minus-strand string of a minus
// pair) at the rows listed in `sites` (ascending), appended to runs[row]
inline void insertion_runs(const uint32_t *words, uint64_t n, const uint8_t *read, const std::vector<uint64_t> &sites,
                           InsertionRuns &runs) {
  uint64_t i = 0, j = 0;
  for (uint64_t k = 0; k < n; k++) {
    const uint64_t run = words[k] >> 4;
    const uint32_t op = words[k] & 15u;
    if (op == MC_CIGAR_I) {
      if (std::binary_search(sites.begin(), sites.end(), j)) runs[j].emplace_back(read + i, read + i + run);
      i += run;
    } else if (op == MC_CIGAR_D) {
      j += run;
    } else {
      i += run;
      j += run;
    }
  }
}

// the consensus of the runs at one site
inline std::string insertion_consensus(const std::vector<std::vector<uint8_t>> &runs) {
  std::map<size_t, size_t> count;  // length -> runs (ascending: the first maximum is the shortest)
  for (const auto &r : runs) count[r.size()]++;
  size_t len = 0, most = 0;
  for (const auto &kv : count)
    if (kv.second > most) {
      most = kv.second;
      len = kv.first;
    }
  std::string out;
  for (size_t t = 0; t < len; t++) {
    size_t cls[5] = {0, 0, 0, 0, 0};
    for (const auto &r : runs)
      if (r.size() > t) cls[pileup_channel(r[t])]++;
    size_t best = 0;
    for (size_t k = 1; k < 5; k++)
      if (cls[k] > cls[best]) best = k;
    out += "ACGTN"[best];
  }
  return out;
}

struct Consensus {
  std::string seq;
  uint64_t sub = 0, del = 0, ins = 0;  // columns that differ from the centre, columns left out, sites applied
};

// centre: its L expanded bytes; rows: its L + 1 rows; runs: the inserted bytes at its sites (a
// site without runs applies nothing)
inline Consensus consensus_of(const uint8_t *centre, uint64_t L, const uint32_t *rows, uint64_t depth, const InsertionRuns &runs) {
  Consensus c;
  c.seq.reserve(L + 16);
  if (depth == 0) {
    for (uint64_t r = 0; r < L; r++) c.seq += pileup_base_char(centre[r]);
    return c;
  }
  for (uint64_t r = 0; r <= L; r++) {
    if (2 * (uint64_t)rows[r * MC_PILEUP_CH + 6] > depth) {
      const auto it = runs.find(r);
      if (it != runs.end() && !it->second.empty()) {
        c.seq += insertion_consensus(it->second);
        c.ins++;
      }
    }
    if (r == L) break;
    const uint32_t ch = consensus_channel(rows + r * MC_PILEUP_CH, centre[r]);
    if (ch == 5) {
      c.del++;
      continue;
    }
    const char x = "ACGTN"[ch];
    if (x != pileup_base_char(centre[r])) c.sub++;
    c.seq += x;
  }
  return c;
}

// ---- the consensus weighed by base quality (mc_nw_qpileup_strands' second table, --quality) ----
// wrows: the centre's L + 1 rows of weights beside its rows of counts.
//   column r < L   the channel 0..5 of the largest weight wins; ties go to the larger count, then to
//                  the centre's own channel if it is among the tied, else to the lowest.  Depth 0
//                  keeps the centre's byte.
//   its quality    clamp(W_win - the other five channels' W, 0, 93), written + 33; depth 0: '!'
//   site r <= L    applied, and as long, as consensus_of's (counts); base t: among the runs longer
//                  than t the class (0..3, anything else N) of the largest summed quality, ties to
//                  the larger count, then to the lowest class; its quality the same clamp over the
//                  classes.
inline uint32_t qconsensus_pick(const uint64_t *w, const uint64_t *n, uint32_t classes, uint32_t own) {
  uint32_t best = 0;
  bool own_tied = own == 0;
  for (uint32_t ch = 1; ch < classes; ch++) {
    if (w[ch] > w[best] || (w[ch] == w[best] && n[ch] > n[best])) {
      best = ch;
      own_tied = ch == own;
    } else if (w[ch] == w[best] && n[ch] == n[best] && ch == own) {
      own_tied = true;
    }
  }
  return own_tied && own < classes ? own : best;
}

inline char qconsensus_quality(const uint64_t *w, uint32_t classes, uint32_t win) {
  uint64_t rest = 0;
  for (uint32_t ch = 0; ch < classes; ch++)
    if (ch != win) rest += w[ch];
  const uint64_t q = w[win] > rest ? std::min<uint64_t>(w[win] - rest, 93) : 0;
  return (char)(33 + q);
}

struct QRun {
  std::vector<uint8_t> base, qual;  // an 'I' run's read bytes and their qualities, as aligned
};
using QInsertionRuns = std::map<uint64_t, std::vector<QRun>>;

// insertion_runs with the qualities (qual: the read's, in the aligned string's order)
inline void qinsertion_runs(const uint32_t *words, uint64_t n, const uint8_t *read, const uint8_t *qual,
                            const std::vector<uint64_t> &sites, QInsertionRuns &runs) {
  uint64_t i = 0, j = 0;
  for (uint64_t k = 0; k < n; k++) {
    const uint64_t run = words[k] >> 4;
    const uint32_t op = words[k] & 15u;
    if (op == MC_CIGAR_I) {
      if (std::binary_search(sites.begin(), sites.end(), j))
        runs[j].push_back({std::vector<uint8_t>(read + i, read + i + run), std::vector<uint8_t>(qual + i, qual + i + run)});
      i += run;
    } else if (op == MC_CIGAR_D) {
      j += run;
    } else {
      i += run;
      j += run;
    }
  }
}

struct QConsensus {
  std::string seq, qual;
  uint64_t sub = 0, del = 0, ins = 0;
};

inline void qinsertion_consensus(const std::vector<QRun> &runs, QConsensus &c) {
  std::map<size_t, size_t> count;  // length -> runs (ascending: the first maximum is the shortest)
  for (const auto &r : runs) count[r.base.size()]++;
  size_t len = 0, most = 0;
  for (const auto &kv : count)
    if (kv.second > most) {
      most = kv.second;
      len = kv.first;
    }
  for (size_t t = 0; t < len; t++) {
    uint64_t w[5] = {0, 0, 0, 0, 0}, n[5] = {0, 0, 0, 0, 0};
    for (const auto &r : runs)
      if (r.base.size() > t) {
        w[pileup_channel(r.base[t])] += r.qual[t];
        n[pileup_channel(r.base[t])]++;
      }
    const uint32_t win = qconsensus_pick(w, n, 5, 5);  // (no own class: ties end at the lowest)
    c.seq += "ACGTN"[win];
    c.qual += qconsensus_quality(w, 5, win);
  }
}

inline QConsensus qconsensus_of(const uint8_t *centre, uint64_t L, const uint32_t *rows, const uint32_t *wrows, uint64_t depth,
                                const QInsertionRuns &runs) {
  QConsensus c;
  c.seq.reserve(L + 16);
  c.qual.reserve(L + 16);
  if (depth == 0) {
    for (uint64_t r = 0; r < L; r++) c.seq += pileup_base_char(centre[r]);
    c.qual.assign(L, '!');
    return c;
  }
  for (uint64_t r = 0; r <= L; r++) {
    if (2 * (uint64_t)rows[r * MC_PILEUP_CH + 6] > depth) {
      const auto it = runs.find(r);
      if (it != runs.end() && !it->second.empty()) {
        qinsertion_consensus(it->second, c);
        c.ins++;
      }
    }
    if (r == L) break;
    uint64_t w[6], n[6];
    for (uint32_t ch = 0; ch < 6; ch++) {
      w[ch] = wrows[r * MC_PILEUP_CH + ch];
      n[ch] = rows[r * MC_PILEUP_CH + ch];
    }
    const uint32_t ch = qconsensus_pick(w, n, 6, pileup_channel(centre[r]));
    if (ch == 5) {
      c.del++;
      continue;
    }
    const char x = "ACGTN"[ch];
    if (x != pileup_base_char(centre[r])) c.sub++;
    c.seq += x;
    c.qual += qconsensus_quality(w, 6, ch);
  }
  return c;
}

}  // namespace mc
