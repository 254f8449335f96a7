// fastq_check.cpp -- the FASTQ reader of host/fasta.cpp against the FASTA reader, field by field
// (tests/test_fastq_parser.py writes the files):
//   fastq_check <a.fastq> <its FASTA twin>
// parses each file alone with 1 and 8 threads, with the qualities kept and skipped, and compares
// every array of the Dataset: headers, lengths, seq_off, packed, pk_off, exc_pos, exc_val, seg,
// seg_off, file_count, file_len_sum.  The qualities must not depend on the threads, are bases()
// long for the FASTQ file and are absent without the flag.  Prints "OK <records> <bases>" or what
// differs.  Linked against libmeshclust.so.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "fasta.hpp"

static int fail(const std::string &what) {
  printf("FAIL: %s\n", what.c_str());
  return 1;
}

static const char *differ(const mc::Dataset &x, const mc::Dataset &y) {
  if (x.headers.blob != y.headers.blob || x.headers.off != y.headers.off) return "headers";
  if (x.lengths != y.lengths) return "lengths";
  if (x.seq_off != y.seq_off) return "seq_off";
  if (x.pk_off != y.pk_off) return "pk_off";
  if (x.packed.size() != y.packed.size() || memcmp(x.packed.data(), y.packed.data(), x.packed.size() * 4)) return "packed";
  if (x.exc_pos != y.exc_pos) return "exc_pos";
  if (x.exc_val != y.exc_val) return "exc_val";
  if (x.seg != y.seg) return "seg";
  if (x.seg_off != y.seg_off) return "seg_off";
  if (x.file_count != y.file_count) return "file_count";
  if (x.file_len_sum != y.file_len_sum) return "file_len_sum";
  return nullptr;
}

int main(int argc, char **argv) {
  if (argc < 3) return fail("usage: fastq_check <fastq> <fasta twin>");
  try {
    mc::Dataset twin;
    mc::parse_fasta_files({argv[2]}, twin, 1);
    if (twin.file_fastq != std::vector<uint8_t>{0} || !twin.qual.empty()) return fail("the twin is FASTA");
    mc::Dataset first;
    for (int threads : {1, 8})
      for (int keep = 0; keep < 2; keep++) {
        const std::string tag = " (threads " + std::to_string(threads) + ", keep " + std::to_string(keep) + ")";
        mc::Dataset q, a;
        mc::parse_fasta_files({argv[1]}, q, threads, keep != 0);
        mc::parse_fasta_files({argv[2]}, a, threads, keep != 0);
        if (const char *w = differ(q, twin)) return fail(std::string("FASTQ against its twin: ") + w + tag);
        if (const char *w = differ(a, twin)) return fail(std::string("the twin against itself: ") + w + tag);
        if (q.file_fastq != std::vector<uint8_t>{1}) return fail("file_fastq" + tag);
        if (!keep && !q.qual.empty()) return fail("qualities kept without the flag" + tag);
        if (keep && (q.qual.size() != q.bases() || a.qual != std::vector<uint8_t>(a.bases(), 0))) return fail("qual's size" + tag);
        if (keep && first.qual.empty()) first.qual = q.qual;
        if (keep && q.qual != first.qual) return fail("qual depends on the threads" + tag);
      }
    printf("OK %zu %llu\n", twin.size(), (unsigned long long)twin.bases());
    return 0;
  } catch (const std::exception &e) {
    return fail(e.what());
  }
}
