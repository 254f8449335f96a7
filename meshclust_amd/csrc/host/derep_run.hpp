// derep_run.hpp -- meshclust-derep: collapse the identical reads of FASTA / FASTQ files, on either
// strand, to one representative with an abundance (mc_derep; derep.hpp has the definition).
// Header-only: bin/meshclust-derep (derep_main.cpp) and libmeshclust's mcl_derep (capi_derep.cpp)
// share it.
#pragma once
#include <cerrno>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "common.hpp"
#include "derep.hpp"
#include "fasta.hpp"
#include "model.hpp"

namespace mc {

struct DerepOptions {
  std::vector<std::string> reads;
  std::string output = "derep.fa", table, stats_json;
  bool both_strands = false, quiet = false;
  uint64_t min_size = 1;
  int device = 0, threads = 8;
};

struct DerepResult {
  uint64_t reads = 0, uniques = 0, written = 0, largest = 0, minus = 0;
  int strands = 1;
  uint64_t compare_pairs = 0, rounds = 0, collisions = 0;
  double parse_ms = 0, upload_ms = 0, derep_ms = 0, write_ms = 0;
};

static const char *kDerepUsage =
    "Usage: meshclust-derep [--output uniq.fa] [--table FILE] [--both-strands] [--min-size N] [--device N] [--threads N] "
    "[--stats-json FILE] [--quiet] READS.fa|fq [MORE ...]\n"
    "  collapses reads whose sequences are identical to one record per class, most abundant first (ties: the class\n"
    "  whose first read comes first); the representative is the class's first read in input order\n"
    "  --output FILE   (default derep.fa) the representatives as FASTA, the header line extended by ;size=N\n"
    "  --table FILE    one line per read in input order: read, representative, strand (+ or -), size of its class\n"
    "  --both-strands  a read that is the reverse complement of another is its duplicate too (strand -)\n"
    "  --min-size N    (N >= 1, default 1) leave classes of fewer than N reads out of --output (not out of --table)\n"
    "  reads may be FASTA or FASTQ files (decided per file); qualities are skipped\n";

inline DerepOptions parse_derep_options(int argc, char **argv) {
  DerepOptions o;
  for (int i = 1; i < argc; i++) {
    const std::string arg = argv[i];
    const bool has = i + 1 < argc;
    if ((arg == "-o" || arg == "--output") && has) o.output = argv[++i];
    else if (arg == "--table" && has) o.table = argv[++i];
    else if (arg == "--stats-json" && has) o.stats_json = argv[++i];
    else if (arg == "--device" && has) o.device = atoi(argv[++i]);
    else if ((arg == "-t" || arg == "--threads") && has) {
      o.threads = atoi(argv[++i]);
      if (o.threads <= 0) throw Error("Number of threads must be greater than 0.", 1);
    } else if (arg == "--quiet") o.quiet = true;
    else if (arg == "--both-strands") o.both_strands = true;
    else if (arg == "--min-size" && has) {
      char *end = nullptr;
      const char *txt = argv[++i];
      const long long v = strtoll(txt, &end, 10);
      if (end == txt || *end || v < 1) throw Error(std::string("--min-size must be 1 or more\n") + kDerepUsage, 1);
      o.min_size = (uint64_t)v;
    } else if (!arg.empty() && arg[0] != '-') o.reads.push_back(arg);
    else throw Error(std::string("unknown option or missing value: ") + argv[i] + "\n" + kDerepUsage, 1);
  }
  if (o.reads.empty()) throw Error(std::string("at least one reads file is required\n") + kDerepUsage, 1);
  return o;
}

// ctx null: a context of its own on opt.device, destroyed at the end
inline DerepResult run_derep(mc_ctx *ctx, const DerepOptions &opt) {
  auto ms_since = [](std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  };
  auto write_text = [](const std::string &path, const std::string &text) {
    FILE *f = fopen(path.c_str(), "w");
    if (!f) throw Error("cannot write " + path + ": " + strerror(errno), 1);
    const bool ok = fwrite(text.data(), 1, text.size(), f) == text.size();
    if (fclose(f) != 0 || !ok) throw Error("cannot write " + path, 1);
  };
  struct Own {
    mc_ctx *c = nullptr;
    ~Own() {
      if (c) mc_ctx_destroy(c);
    }
  } own;
  DerepResult r;
  r.strands = opt.both_strands ? 3 : 1;
  for (const std::string &p : opt.reads) {
    FILE *f = fopen(p.c_str(), "r");
    if (!f) throw Error("meshclust-derep: cannot read " + p + ": " + strerror(errno), 2);
    const bool empty = fgetc(f) == EOF;
    fclose(f);
    if (empty) throw Error("meshclust-derep: no reads in " + p, 2);
  }
  auto t0 = std::chrono::steady_clock::now();
  Dataset ds;
  parse_fasta_files(opt.reads, ds, opt.threads);
  r.parse_ms = ms_since(t0);
  const uint64_t n = ds.size();
  if (n == 0) throw Error("meshclust-derep: no reads", 2);
  if (n >= (1ull << 32)) throw Error("meshclust-derep: more than 2^32 - 1 reads", 2);
  r.reads = n;
  if (!ctx) {
    check(mc_ctx_create(opt.device, &own.c), "mc_ctx_create");
    ctx = own.c;
  }
  t0 = std::chrono::steady_clock::now();
  check(mc_load_packed(ctx, ds.packed.data(), ds.pk_off.data(), ds.seq_off.data(), n, ds.exc_pos.data(), ds.exc_val.data(),
                       ds.exc_pos.size(), ds.seg.data(), ds.seg_off.data()),
        "mc_load_packed");
  r.upload_ms = ms_since(t0);

  t0 = std::chrono::steady_clock::now();
  std::vector<uint32_t> ids(n), rep(n);
  std::vector<uint8_t> minus(n, 0);
  for (uint64_t i = 0; i < n; i++) ids[i] = (uint32_t)i;
  double prof[5];
  check(mc_derep_profile(ctx, prof, 1), "mc_derep_profile");
  check(mc_derep(ctx, ids.data(), n, r.strands, rep.data(), minus.data()), "mc_derep");
  check(mc_derep_profile(ctx, prof, 0), "mc_derep_profile");
  r.compare_pairs = (uint64_t)prof[2];
  r.rounds = (uint64_t)prof[3];
  r.collisions = (uint64_t)prof[4];
  std::vector<uint32_t> first;
  std::vector<uint64_t> size;
  derep_classes(rep.data(), n, first, size);
  r.uniques = first.size();
  r.largest = size.empty() ? 0 : size[0];
  for (uint64_t i = 0; i < n; i++) r.minus += minus[i];
  r.derep_ms = ms_since(t0);

  t0 = std::chrono::steady_clock::now();
  {
    std::string text, rec;
    for (size_t c = 0; c < first.size(); c++) {
      if (size[c] < opt.min_size) break;  // (size descending)
      rec.clear();
      append_fasta(rec, ds, &first[c], 1);
      const size_t eol = rec.find('\n');
      text.append(rec, 0, eol);
      text += ";size=" + std::to_string(size[c]);
      text.append(rec, eol, std::string::npos);
      r.written++;
    }
    write_text(opt.output, text);
  }
  if (!opt.table.empty()) {
    std::vector<uint64_t> count(n, 0);
    for (uint64_t i = 0; i < n; i++) count[rep[i]]++;
    std::string text;
    for (uint64_t i = 0; i < n; i++) {  // names: the header without '>', as meshclust-assign's TSV has them
      text.append(ds.headers[i].substr(1));
      text += '\t';
      text.append(ds.headers[rep[i]].substr(1));
      text += minus[i] ? "\t-\t" : "\t+\t";
      text += std::to_string(count[rep[i]]);
      text += '\n';
    }
    write_text(opt.table, text);
  }
  r.write_ms = ms_since(t0);
  return r;
}

inline std::string derep_stats_json(const DerepResult &r) {
  char b[1024];
  snprintf(b, sizeof b,
           "{\"reads\": %llu, \"uniques\": %llu, \"written\": %llu, \"largest\": %llu, \"minus\": %llu, \"strands\": %d, "
           "\"compare_pairs\": %llu, \"rounds\": %llu, \"collisions\": %llu, "
           "\"phases_ms\": {\"parse\": %.3f, \"upload\": %.3f, \"derep\": %.3f, \"write\": %.3f}}",
           (unsigned long long)r.reads, (unsigned long long)r.uniques, (unsigned long long)r.written, (unsigned long long)r.largest,
           (unsigned long long)r.minus, r.strands, (unsigned long long)r.compare_pairs, (unsigned long long)r.rounds,
           (unsigned long long)r.collisions, r.parse_ms, r.upload_ms, r.derep_ms, r.write_ms);
  return b;
}

}  // namespace mc
