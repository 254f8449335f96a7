// capi_derep.cpp -- libmeshclust.so's C entries for dereplication (derep_run.hpp, derep.hpp).
#include <cstring>
#include <string>
#include <vector>

#include "derep_run.hpp"

extern "C" {

// meshclust-derep on an open context: the reads of reads[0..nreads) collapsed by mc_derep, the
// representatives to `output` (FASTA, ;size=N), one line per read to `table` if non-NULL; classes of
// fewer than min_size reads are left out of `output`.  The JSON summary goes to stats (cap bytes).
// Returns 0 or an error code with {"error": ...} in stats; an error never ends the calling process.
int mcl_derep(mc_ctx *ctx, const char *const *reads, int nreads, int threads, const char *output, const char *table,
              int both_strands, long long min_size, char *stats, int cap) {
  try {
    mc::DerepOptions opt;
    for (int i = 0; i < nreads; i++) opt.reads.push_back(reads[i]);
    if (opt.reads.empty() || !output) throw mc::Error("mcl_derep: reads and output are required", 1);
    if (min_size < 1) throw mc::Error("mcl_derep: min_size is 1 or more", 1);
    opt.output = output;
    if (table) opt.table = table;
    opt.both_strands = both_strands != 0;
    opt.min_size = (uint64_t)min_size;
    if (threads > 0) opt.threads = threads;
    opt.quiet = true;
    const mc::DerepResult r = mc::run_derep(ctx, opt);
    if (stats && cap > 0) snprintf(stats, cap, "%s", mc::derep_stats_json(r).c_str());
    return 0;
  } catch (const std::exception &e) {
    std::string m;
    for (const char *c = e.what(); *c; c++) {
      if (*c == '"' || *c == '\\') m += '\\';
      m += (unsigned char)*c < 0x20 ? ' ' : *c;
    }
    if (stats && cap > 0) snprintf(stats, cap, "{\"error\": \"%s\"}", m.c_str());
    const mc::Error *me = dynamic_cast<const mc::Error *>(&e);
    return me && me->code ? me->code : 1;
  }
}

// derep_host (derep.hpp) on caller-provided bytes: the contract of mc_derep on the CPU, for the
// benchmark's host route and the tests.  It is no fallback of mc_derep.
int mcl_derep_host(const uint8_t *codes, const uint64_t *seq_off, const uint32_t *ids, uint64_t m, int strands, uint32_t *rep,
                   uint8_t *minus) {
  if (strands != 1 && strands != 3) return 1;
  if (m == 0) return 0;
  if (!seq_off || !ids || !rep) return 1;
  std::vector<uint8_t> own;
  if (!minus) {
    own.resize(m);
    minus = own.data();
  }
  mc::derep_host(codes, seq_off, ids, m, strands == 3, rep, minus);
  return 0;
}
}
