// assign.cpp -- see assign.hpp.
#include "assign.hpp"

#include <sys/stat.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>

#ifdef _OPENMP
#include <omp.h>
#endif

#include "cigar.hpp"
#include "consensus.hpp"
#include "fasta.hpp"
#include "model.hpp"
#include "revseq.hpp"
#include "topk.hpp"
#include "variants.hpp"
#include "chimera.hpp"
#include "verify.hpp"

namespace mc {

static const char *kUsage =
    "Usage: meshclust-assign --model FILE --centres FILE reads.fa [more.fa] --output assign.tsv "
    "[--unassigned rest.fa] [--both-strands] [--top K --hits FILE] [--identity] [--min-identity X] [--paf FILE] [--consensus FILE] "
    "[--pileup FILE] [--quality] [--msa FILE] [--profile FILE] [--band] [--variants FILE] [--alleles FILE] [--haplotypes FILE] [--min-allele-frac X] "
    "[--min-allele-count N] [--chimeras FILE] [--min-chimera-gain N] [--device N] [--threads N] [--stats-json FILE] [--quiet]\n"
    "  --both-strands  score every read as written and reverse-complemented; the TSV gains a strand column\n"
    "                  (implied by a version-2 model, saved by meshclust --both-strands: reads and centres are then\n"
    "                  scored once on their canonical rows and every hit's strand comes from mc_orient_pairs; with\n"
    "                  such a model MC_ASSIGN_PAIRS scores the pair list on the canonical rows too, and 32/64-bit\n"
    "                  histograms or k >= 8 are refused with exit code 2)\n"
    "  --top K --hits FILE  (given together, K = 1..8) also write the K best similar centres of every read to\n"
    "                  FILE: read, rank, centre, cluster index, combo 0 (and the strand with --both-strands)\n"
    "  --identity      align every reported (read, centre) pair, the read reverse-complemented where it was\n"
    "                  assigned on the minus strand; the TSV and the hits file gain a last column, the identity\n"
    "  --min-identity X  (0 <= X <= 1, implies --identity) assign a read to the first of its hits (the --top K\n"
    "                  best, or the best one) that aligns at identity X or more; none: the read is unassigned\n"
    "  --paf FILE      (implies --identity) also write every aligned (read, centre) pair as a PAF line with its\n"
    "                  CIGAR (cg:Z:, = X I D); on - the CIGAR runs along the reverse-complemented read\n"
    "  --consensus FILE  (implies --identity) pile the assigned reads up on their centres and write every centre's\n"
    "                  consensus as FASTA: >NAME depth=D sub=S del=X ins=I (a centre without reads: its own sequence)\n"
    "  --pileup FILE   (implies the --consensus pass) the counts behind it, for centres with reads: centre, column\n"
    "                  (the row after the last base: L+1, base *), centre base, depth, A, C, G, T, N, del, ins_reads,\n"
    "                  ins_bases\n"
    "  --quality       (with --consensus and/or --pileup; every reads file FASTQ) weigh the pile-up by base quality:\n"
    "                  a column goes to the channel of the largest summed Phred value, the consensus is written as\n"
    "                  FASTQ (@NAME depth=D sub=S del=X ins=I) with a quality per base, the pile-up rows gain wA wC wG\n"
    "                  wT wN wdel\n"
    "  --msa FILE      (implies --identity) the assigned reads of every centre laid out in common columns, as aligned\n"
    "                  FASTA: >CENTRE depth=D width=W and the centre's row, then >READ strand=+ (or -) and its row per\n"
    "                  read; inserted bases get columns of their own, gaps are -\n"
    "  --profile FILE  (implies --identity) that alignment counted per column, for centres with reads: centre, column,\n"
    "                  centre_pos, slot (0: a centre base; from 1: an inserted column before it), base (- inserted),\n"
    "                  depth, A, C, G, T, N, gap; with --quality (FASTQ reads) also wA wC wG wT wN wgap\n"
    "  --band          (with --paf, --consensus, --pileup, --msa, --profile, --variants, --alleles, --haplotypes or\n"
    "                  --chimeras) record\n"
    "                  only a certified band of every alignment's choices (mc_set_align_band): less scratch, more pairs per\n"
    "                  batch, no output file changes\n"
    "  --variants FILE  (implies --identity) the --profile lines of the variant sites of every centre with reads: the\n"
    "                  columns whose second most frequent allele (A, C, G, T or gap) is seen --min-allele-count times or\n"
    "                  more and in --min-allele-frac of the rows or more\n"
    "  --alleles FILE  (implies --identity) one line per assigned read: read, centre, strand, its characters at its\n"
    "                  centre's variant sites (. if it has none); with --quality a fifth column, their weights as Phred+33\n"
    "  --haplotypes FILE  (implies --identity) per centre with a site, one line per distinct allele string seen\n"
    "                  --min-allele-count times or more: centre, rank, count, depth, alleles\n"
    "  --min-allele-frac X  (0 < X <= 1, default 0.2)   --min-allele-count N  (N >= 1, default 2)\n"
    "  --chimeras FILE  (needs --top K with K >= 2, implies --identity) compare every read's best hit with each later hit\n"
    "                  of another centre, base by base along the read, and write the second parent that adds most: read,\n"
    "                  left_centre, right_centre, left_strand, right_strand, cut_first, cut_last (0-based positions in the\n"
    "                  read as written), ids_left, ids_right, best, gain, read_len, flag\n"
    "  --min-chimera-gain N  (N >= 1, default 3) flag Y where the two-parent model has N identities or more above the\n"
    "                  better single parent.  3 is a convention and is not tuned: on error-free planted reads of 120\n"
    "                  bases from parents 10 % apart the gains were 3 .. 8; with parents 5 % apart and 3 % read error\n"
    "                  only 2 .. 3, so the flag is weak there.  Real data was not measured\n"
    "  reads and centres may be FASTA or FASTQ files (decided per file); without --quality the qualities are skipped\n";

AssignOptions parse_assign_options(int argc, char **argv) {
  AssignOptions o;
  for (int i = 1; i < argc; i++) {
    const std::string arg = argv[i];
    const bool has = i + 1 < argc;
    if (arg == "--model" && has) o.model = argv[++i];
    else if (arg == "--centres" && has) o.centres = argv[++i];
    else if ((arg == "-o" || arg == "--output") && has) o.output = argv[++i];
    else if (arg == "--unassigned" && has) o.unassigned = argv[++i];
    else if (arg == "--stats-json" && has) o.stats_json = argv[++i];
    else if (arg == "--device" && has) o.device = atoi(argv[++i]);
    else if ((arg == "-t" || arg == "--threads") && has) {
      o.threads = atoi(argv[++i]);
      if (o.threads <= 0) throw Error("Number of threads must be greater than 0.", 1);
    } else if (arg == "--quiet") o.quiet = true;
    else if (arg == "--both-strands") o.both_strands = true;
    else if (arg == "--top" && has) {
      o.top = atoi(argv[++i]);
      if (o.top < 1 || o.top > MC_ASSIGN_MAX_TOP)
        throw Error(std::string("--top must be 1 .. ") + std::to_string(MC_ASSIGN_MAX_TOP) + "\n" + kUsage, 1);
    } else if (arg == "--hits" && has) o.hits = argv[++i];
    else if (arg == "--identity") o.identity = true;
    else if (arg == "--min-identity" && has) {
      char *end = nullptr;
      const char *txt = argv[++i];
      o.min_identity = strtod(txt, &end);
      if (end == txt || *end || !(o.min_identity >= 0 && o.min_identity <= 1))
        throw Error(std::string("--min-identity must be 0 .. 1\n") + kUsage, 1);
      o.identity = true;
    } else if (arg == "--paf" && has) {
      o.paf = argv[++i];
      o.identity = true;
    } else if (arg == "--consensus" && has) {
      o.consensus = argv[++i];
      o.identity = true;
    } else if (arg == "--pileup" && has) {
      o.pileup = argv[++i];
      o.identity = true;
    } else if (arg == "--quality") {
      o.quality = true;
    } else if (arg == "--band") {
      o.band = true;
    } else if (arg == "--msa" && has) {
      o.msa = argv[++i];
      o.identity = true;
    } else if (arg == "--profile" && has) {
      o.profile = argv[++i];
      o.identity = true;
    } else if (arg == "--variants" && has) {
      o.variants = argv[++i];
      o.identity = true;
    } else if (arg == "--alleles" && has) {
      o.alleles = argv[++i];
      o.identity = true;
    } else if (arg == "--haplotypes" && has) {
      o.haplotypes = argv[++i];
      o.identity = true;
    } else if (arg == "--chimeras" && has) {
      o.chimeras = argv[++i];
      o.identity = true;
    } else if (arg == "--min-chimera-gain" && has) {
      char *end = nullptr;
      const char *txt = argv[++i];
      const long long v = strtoll(txt, &end, 10);
      if (end == txt || *end || v < 1) throw Error(std::string("--min-chimera-gain must be 1 or more\n") + kUsage, 1);
      o.min_chimera_gain = v;
    } else if (arg == "--min-allele-frac" && has) {
      char *end = nullptr;
      const char *txt = argv[++i];
      o.min_allele_frac = strtod(txt, &end);
      if (end == txt || *end || !(o.min_allele_frac > 0 && o.min_allele_frac <= 1))
        throw Error(std::string("--min-allele-frac must be above 0 and at most 1\n") + kUsage, 1);
    } else if (arg == "--min-allele-count" && has) {
      char *end = nullptr;
      const char *txt = argv[++i];
      const long long v = strtoll(txt, &end, 10);
      if (end == txt || *end || v < 1) throw Error(std::string("--min-allele-count must be 1 or more\n") + kUsage, 1);
      o.min_allele_count = (uint64_t)v;
    } else {
      struct stat st;
      if (stat(argv[i], &st) == 0 && S_ISREG(st.st_mode)) o.reads.push_back(argv[i]);
      else throw Error(std::string("unknown option or missing file: ") + argv[i] + "\n" + kUsage, 1);
    }
  }
  if (o.model.empty() || o.centres.empty() || o.reads.empty())
    throw Error(std::string("--model, --centres and at least one reads file are required\n") + kUsage, 1);
  if ((o.top > 0) != !o.hits.empty()) throw Error(std::string("--top K and --hits FILE are given together\n") + kUsage, 1);
  if (!o.chimeras.empty() && o.top < 2) throw Error(std::string("--chimeras FILE needs --top K with K >= 2\n") + kUsage, 1);
  if (o.quality && o.consensus.empty() && o.pileup.empty() && o.profile.empty() && !o.any_variants())
    throw Error(std::string("--quality needs --consensus FILE and/or --pileup FILE (or --profile FILE)\n") + kUsage, 1);
  if (o.band && o.paf.empty() && o.consensus.empty() && o.pileup.empty() && o.msa.empty() && o.profile.empty() && !o.any_variants() && o.chimeras.empty())
    throw Error(std::string("--band needs --paf, --consensus, --pileup, --msa or --profile\n") + kUsage, 1);
  return o;
}

static double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// The same job through mc_classify_pairs: the candidate pairs of the length gate in batches,
// the argmax on the host (largest combo 0 among the similar centres, lowest index on ties).
// K > 0: also the K best similar centres of every query into rows of K slots (hit, hit_val), kept
// in mc_assign_top's order by the insertion the kernels use (topk.hpp); one strand, so every
// hit's strand is 0.
static void assign_by_pairs(mc_ctx *ctx, const Dataset &ds, uint32_t C, uint64_t M, double sim,
                            std::vector<uint32_t> &best, std::vector<double> &val, std::vector<uint32_t> &nsim,
                            uint64_t *candidates, uint32_t K, std::vector<uint32_t> &hit, std::vector<double> &hit_val) {
  std::vector<uint8_t> hit_strand((size_t)M * K, 0);
  std::vector<uint64_t> lo(C, 0), hi(C, ~0ull);
  if (sim > 0)
    for (uint32_t j = 0; j < C; j++) {
      lo[j] = (uint64_t)(ds.lengths[j] * sim);
      hi[j] = (uint64_t)(ds.lengths[j] / sim);
    }
  const size_t batch = 1u << 22;
  std::vector<uint32_t> a, b;
  std::vector<uint8_t> d;
  std::vector<double> c0;
  a.reserve(batch + C);
  b.reserve(batch + C);
  auto flush = [&]() {
    if (a.empty()) return;
    d.resize(a.size());
    c0.resize(a.size());
    check(mc_classify_pairs(ctx, a.data(), b.data(), a.size(), d.data(), c0.data(), nullptr), "mc_classify_pairs");
    for (size_t p = 0; p < a.size(); p++) {  // (pairs are query-major, centres ascending)
      if (!d[p]) continue;
      const uint64_t q = a[p] - C;
      if (K > 0)
        topk_insert_row(&hit_val[q * K], &hit[q * K], &hit_strand[q * K], K, std::min<uint32_t>(nsim[q], K), c0[p], b[p], 0);
      nsim[q]++;
      if (best[q] == MC_ASSIGN_NONE || c0[p] > val[q]) {
        best[q] = b[p];
        val[q] = c0[p];
      }
    }
    *candidates += a.size();
    a.clear();
    b.clear();
  };
  for (uint64_t q = 0; q < M; q++) {
    const uint64_t len = ds.lengths[C + q];
    for (uint32_t j = 0; j < C; j++)
      if (lo[j] <= len && len <= hi[j]) {
        a.push_back((uint32_t)(C + q));
        b.push_back(j);
      }
    if (a.size() >= batch) flush();
  }
  flush();
}

static void write_text(const std::string &path, const std::string &text) {
  FILE *f = fopen(path.c_str(), "w");
  if (!f) throw Error("cannot write " + path + ": " + strerror(errno), 1);
  const bool ok = fwrite(text.data(), 1, text.size(), f) == text.size();
  if (fclose(f) != 0 || !ok) throw Error("cannot write " + path, 1);
}

// the expanded bytes of one record (fasta.hpp unpack_codes, for one id)
static std::vector<uint8_t> expanded_bytes(const Dataset &ds, uint32_t id) {
  const uint64_t len = ds.seq_off[id + 1] - ds.seq_off[id];
  std::vector<uint8_t> out(len);
  const uint32_t *w = ds.packed.data() + ds.pk_off[id];
  for (uint64_t j = 0; j < len; j++) out[j] = (uint8_t)((w[j / 16] >> (2 * (j % 16))) & 3u);
  auto e = std::lower_bound(ds.exc_pos.begin(), ds.exc_pos.end(), ds.seq_off[id]);
  for (; e != ds.exc_pos.end() && *e < ds.seq_off[id + 1]; ++e) out[*e - ds.seq_off[id]] = ds.exc_val[e - ds.exc_pos.begin()];
  return out;
}

// --consensus / --pileup: the pairs (read pa, centre pb < C, strand pm) piled up on the centres
// 0 .. C-1 in one mc_nw_pileup_strands call; pid (if given) receives every pair's ids / len.
// Centres with an insertion site have their pairs aligned again for the inserted bases.
// opt.quality: mc_nw_qpileup_strands and consensus.hpp's weighted consensus over ds.qual instead;
// the consensus is then FASTQ and every pile-up row gains the weights of channels 0..5.
static void pileup_outputs(mc_ctx *ctx, const Dataset &ds, uint32_t C, const std::vector<uint32_t> &pa,
                           const std::vector<uint32_t> &pb, const std::vector<uint8_t> &pm, const AssignOptions &opt,
                           AssignResult &r, std::vector<double> *pid) {
  const size_t m = pa.size();
  std::vector<uint32_t> targets(C);
  std::vector<uint64_t> row_off((size_t)C + 1, 0);
  uint64_t rows = 0;
  for (uint32_t j = 0; j < C; j++) {
    targets[j] = j;
    rows += ds.lengths[j] + 1;
  }
  std::vector<uint32_t> table(rows * MC_PILEUP_CH), wtable(opt.quality ? rows * MC_PILEUP_CH : 0);
  std::vector<int32_t> ln(m), idn(m);
  if (opt.quality)
    check(mc_nw_qpileup_strands(ctx, pa.data(), pb.data(), pm.data(), m, targets.data(), C, row_off.data(), table.data(),
                                wtable.data(), rows, nullptr, ln.data(), idn.data()),
          "mc_nw_qpileup_strands");
  else
    check(mc_nw_pileup_strands(ctx, pa.data(), pb.data(), pm.data(), m, targets.data(), C, row_off.data(), table.data(), rows,
                               nullptr, ln.data(), idn.data()),
          "mc_nw_pileup_strands");
  if (pid)
    for (size_t p = 0; p < m; p++) (*pid)[p] = (double)idn[p] / (double)ln[p];
  r.consensus = true;
  r.consensus_pairs = m;
  // a centre's pairs: from[c] .. from[c + 1] of `of` (a counting sort, input order kept)
  std::vector<uint64_t> from((size_t)C + 1, 0);
  for (size_t p = 0; p < m; p++) from[pb[p] + 1]++;
  for (uint32_t j = 0; j < C; j++) from[j + 1] += from[j];
  std::vector<size_t> of(m);
  {
    std::vector<uint64_t> at(from.begin(), from.end() - 1);
    for (size_t p = 0; p < m; p++) of[at[pb[p]]++] = p;
  }
  std::string fa, tsv;
  char num[160];
  std::vector<uint32_t> qa, qb, cig;
  std::vector<uint8_t> qm, rcb, rq;
  std::vector<uint64_t> off;
  for (uint32_t j = 0; j < C; j++) {
    const uint64_t L = ds.lengths[j], depth = from[j + 1] - from[j];
    const uint32_t *rw = table.data() + row_off[j] * MC_PILEUP_CH;
    const std::vector<uint8_t> cen = expanded_bytes(ds, j);
    const uint32_t *ww = opt.quality ? wtable.data() + row_off[j] * MC_PILEUP_CH : nullptr;
    InsertionRuns runs;
    QInsertionRuns qruns;
    if (depth > 0) {
      r.consensus_centres++;
      const std::vector<uint64_t> sites = insertion_sites(rw, L, depth);
      if (!sites.empty()) {  // the inserted bases are not in the table: this centre's alignments once more
        r.realigned_centres++;
        qa.clear(), qb.clear(), qm.clear();
        uint64_t cap = 0;
        for (uint64_t k = from[j]; k < from[j + 1]; k++) {
          qa.push_back(pa[of[k]]);
          qb.push_back(j);
          qm.push_back(pm[of[k]]);
          cap += ds.lengths[pa[of[k]]] + L;
        }
        cig.resize(cap);
        off.assign(depth + 1, 0);
        check(mc_nw_align_strands(ctx, qa.data(), qb.data(), qm.data(), depth, cig.data(), cap, off.data(), nullptr, nullptr,
                                  nullptr),
              "mc_nw_align_strands");
        for (uint64_t k = 0; k < depth; k++) {
          std::vector<uint8_t> rd = expanded_bytes(ds, qa[k]);
          if (qm[k]) {
            rcb.resize(rd.size());
            revseq(rd.data(), rd.size(), rcb.data());
            rd.swap(rcb);
          }
          if (opt.quality) {  // the read's qualities in the aligned string's order
            rq.assign(ds.qual.begin() + ds.seq_off[qa[k]], ds.qual.begin() + ds.seq_off[qa[k] + 1]);
            if (qm[k]) std::reverse(rq.begin(), rq.end());
            qinsertion_runs(cig.data() + off[k], off[k + 1] - off[k], rd.data(), rq.data(), sites, qruns);
          } else {
            insertion_runs(cig.data() + off[k], off[k + 1] - off[k], rd.data(), sites, runs);
          }
        }
      }
    }
    Consensus cs;
    std::string cq;  // --quality: the consensus's quality line
    if (opt.quality) {
      QConsensus q = qconsensus_of(cen.data(), L, rw, ww, depth, qruns);
      cs.seq.swap(q.seq);
      cq.swap(q.qual);
      cs.sub = q.sub, cs.del = q.del, cs.ins = q.ins;
    } else {
      cs = consensus_of(cen.data(), L, rw, depth, runs);
    }
    r.insertion_sites += cs.ins;
    if (!opt.consensus.empty()) {
      if (opt.quality) {
        fa += '@';
        fa.append(ds.headers[j].substr(1));
      } else {
        fa.append(ds.headers[j]);
      }
      snprintf(num, sizeof num, " depth=%llu sub=%llu del=%llu ins=%llu\n", (unsigned long long)depth, (unsigned long long)cs.sub,
               (unsigned long long)cs.del, (unsigned long long)cs.ins);
      fa += num;
      fa += cs.seq;
      fa += '\n';
      if (opt.quality) {
        fa += "+\n";
        fa += cq;
        fa += '\n';
      }
    }
    if (!opt.pileup.empty() && depth > 0)
      for (uint64_t t = 0; t <= L; t++) {
        const uint32_t *x = rw + t * MC_PILEUP_CH;
        tsv.append(ds.headers[j].substr(1));
        snprintf(num, sizeof num, "\t%llu\t%c\t%llu\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u", (unsigned long long)(t + 1),
                 t < L ? pileup_base_char(cen[t]) : '*', (unsigned long long)depth, x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7]);
        tsv += num;
        if (opt.quality) {
          const uint32_t *y = ww + t * MC_PILEUP_CH;
          snprintf(num, sizeof num, "\t%u\t%u\t%u\t%u\t%u\t%u", y[0], y[1], y[2], y[3], y[4], y[5]);
          tsv += num;
        }
        tsv += '\n';
      }
  }
  if (!opt.consensus.empty()) write_text(opt.consensus, fa);
  if (!opt.pileup.empty()) write_text(opt.pileup, tsv);
}

// one line of --profile (and of --variants): column c (0-based) of the centre `name` with bytes cen, x its
// MC_MSA_CH counters, y its weights or NULL
static void profile_line(std::string &text, const std::string &name, const std::vector<uint8_t> &cen, uint64_t c, uint64_t depth,
                         const uint32_t *x, const uint32_t *y) {
  char num[256];
  text.append(name);
  snprintf(num, sizeof num, "\t%llu\t%u\t%u\t%c\t%llu\t%u\t%u\t%u\t%u\t%u\t%u", (unsigned long long)(c + 1), x[6] + 1, x[7],
           x[7] == 0 && x[6] < cen.size() ? pileup_base_char(cen[x[6]]) : '-', (unsigned long long)depth, x[0], x[1], x[2], x[3], x[4],
           x[5]);
  text += num;
  if (y) {
    snprintf(num, sizeof num, "\t%u\t%u\t%u\t%u\t%u\t%u", y[0], y[1], y[2], y[3], y[4], y[5]);
    text += num;
  }
  text += '\n';
}

// a text file written through a buffer of about 1 MiB; an empty path opens nothing and drops what is written
struct TextFile {
  std::string path, text;
  FILE *f = nullptr;
  explicit TextFile(const std::string &p) : path(p) {
    if (path.empty()) return;
    f = fopen(path.c_str(), "w");
    if (!f) throw Error("cannot write " + path + ": " + strerror(errno), 1);
  }
  ~TextFile() {
    if (f) fclose(f);
  }
  bool on() const { return f != nullptr; }
  void flush(bool all) {
    if (!f) text.clear();
    if (text.size() < (all ? 1u : 1u << 20)) return;
    if (fwrite(text.data(), 1, text.size(), f) != text.size()) throw Error("cannot write " + path, 1);
    text.clear();
  }
  void close() {
    flush(true);
    FILE *done = f;
    f = nullptr;
    if (done && fclose(done) != 0) throw Error("cannot write " + path, 1);
  }
};

// every target's variant sites (variants.hpp), mc_nw_msa_sites' two arguments
struct SiteLists {
  std::vector<uint64_t> site_off;
  std::vector<uint32_t> sites;
};

// One pass over the plan of msa_output counted per column (mc_nw_msa_counts), read in ranges of targets
// whose tables stay within 64 MiB on the host (a wider target alone).  write_profile: --profile, one line per
// column.  sl given (--variants / --alleles / --haplotypes): every target's sites by variant_sites into *sl,
// and their lines, the profile's own, to --variants.  Both in one run share the pass: the tables come back once.
static void profile_output(mc_ctx *ctx, const Dataset &ds, const std::vector<uint32_t> &targets, const std::vector<uint64_t> &W,
                           const std::vector<uint64_t> &depth, const AssignOptions &opt, AssignResult &r, bool write_profile,
                           SiteLists *sl) {
  const uint32_t nt = (uint32_t)targets.size();
  TextFile pf(write_profile ? opt.profile : std::string()), vf(sl ? opt.variants : std::string());
  const bool weights = opt.quality && (pf.on() || vf.on());
  const uint64_t col_bytes = (uint64_t)MC_MSA_CH * 4 * (opt.quality ? 2 : 1), kWindow = 64ull << 20;
  if (write_profile) {
    r.profile = true;
    r.profile_centres = nt;
  }
  if (sl) sl->site_off.assign((size_t)nt + 1, 0);
  std::vector<uint32_t> counts, wcounts, st;
  std::vector<uint64_t> off;
  for (uint32_t t0 = 0, t1; t0 < nt; t0 = t1) {
    uint64_t cols = 0;
    for (t1 = t0; t1 < nt && (t1 == t0 || (cols + W[t1]) * col_bytes <= kWindow); t1++) cols += W[t1];
    counts.resize(cols * MC_MSA_CH);
    if (weights) wcounts.resize(cols * MC_MSA_CH);
    off.resize((size_t)(t1 - t0) + 1);
    check(mc_nw_msa_counts(ctx, t0, t1 - t0, off.data(), counts.data(), weights ? wcounts.data() : nullptr, cols), "mc_nw_msa_counts");
    for (uint32_t t = t0; t < t1; t++) {
      const uint32_t *tab = counts.data() + off[t - t0] * MC_MSA_CH;
      const uint32_t *wtab = weights ? wcounts.data() + off[t - t0] * MC_MSA_CH : nullptr;
      st.clear();
      if (sl) {
        st = variant_sites(tab, W[t], opt.min_allele_frac, opt.min_allele_count);
        sl->sites.insert(sl->sites.end(), st.begin(), st.end());
        sl->site_off[t + 1] = sl->sites.size();
        r.variant_centres += !st.empty();
        r.variant_sites += st.size();
      }
      if (write_profile) r.profile_columns += W[t];
      if (!pf.on() && (!vf.on() || st.empty())) continue;
      const std::vector<uint8_t> cen = expanded_bytes(ds, targets[t]);
      const std::string name(ds.headers[targets[t]].substr(1));
      if (pf.on())
        for (uint64_t c = 0; c < W[t]; c++)
          profile_line(pf.text, name, cen, c, depth[t], tab + c * MC_MSA_CH, wtab ? wtab + c * MC_MSA_CH : nullptr);
      if (vf.on())
        for (uint32_t c : st)
          profile_line(vf.text, name, cen, c, depth[t], tab + (uint64_t)c * MC_MSA_CH, wtab ? wtab + (uint64_t)c * MC_MSA_CH : nullptr);
      pf.flush(false);
      vf.flush(false);
    }
  }
  pf.close();
  vf.close();
}

// --alleles / --haplotypes on the plan of msa_output, at the sites profile_output left in sl: mc_nw_msa_sites
// over ranges of pairs whose bytes stay within 32 MiB (a pair of more alone): a line per pair to --alleles, and
// a target's strings, complete once its last pair is read (the pairs are sorted by target), through haplotypes
// to --haplotypes.
static void variants_output(mc_ctx *ctx, const Dataset &ds, const std::vector<uint32_t> &targets, const std::vector<uint64_t> &depth,
                            const std::vector<uint32_t> &qa, const std::vector<uint8_t> &qm, const std::vector<uint32_t> &tof,
                            const SiteLists &sl, const AssignOptions &opt, AssignResult &r) {
  const uint64_t m = qa.size(), kWindow = 32ull << 20;
  const std::vector<uint64_t> &site_off = sl.site_off;
  const std::vector<uint32_t> &sites = sl.sites;
  r.variants = true;
  TextFile af(opt.alleles), hf(opt.haplotypes);
  std::vector<uint64_t> off;
  if (!af.on() && !hf.on()) return;
  auto nsite = [&](uint64_t k) { return site_off[tof[k] + 1] - site_off[tof[k]]; };
  const uint64_t per = opt.quality && af.on() ? 2 : 1;
  std::vector<uint8_t> al, ql, strings;  // strings: the allele strings of the target being read, one after the other
  char num[96];
  for (uint64_t k0 = 0, k1; k0 < m; k0 = k1) {
    uint64_t bytes = 0;
    for (k1 = k0; k1 < m && (k1 == k0 || (bytes + nsite(k1)) * per <= kWindow); k1++) bytes += nsite(k1);
    al.resize(bytes);
    if (per == 2) ql.resize(bytes);
    off.resize((size_t)(k1 - k0) + 1);
    check(mc_nw_msa_sites(ctx, site_off.data(), sites.data(), k0, k1 - k0, al.data(), per == 2 ? ql.data() : nullptr, bytes, off.data()),
          "mc_nw_msa_sites");
    r.allele_bytes += bytes * per;
    for (uint64_t k = k0; k < k1; k++) {
      const uint32_t t = tof[k];
      const uint64_t S = nsite(k);
      const uint8_t *x = al.data() + off[k - k0];
      if (af.on()) {
        af.text.append(ds.headers[qa[k]].substr(1));
        af.text += '\t';
        af.text.append(ds.headers[targets[t]].substr(1));
        af.text += qm[k] ? "\t-\t" : "\t+\t";
        if (S) af.text.append((const char *)x, S);
        else af.text += '.';
        if (per == 2) {
          af.text += '\t';
          for (uint64_t s = 0; s < S; s++) af.text += (char)(ql[off[k - k0] + s] + 33);
          if (!S) af.text += '.';
        }
        af.text += '\n';
        af.flush(false);
      }
      if (hf.on() && S) {
        strings.insert(strings.end(), x, x + S);
        if (k + 1 == m || tof[k + 1] != t) {  // the target's last pair
          const std::string name(ds.headers[targets[t]].substr(1));
          uint32_t rank = 0;
          for (const auto &h : haplotypes(strings.data(), depth[t], S, opt.min_allele_count)) {
            hf.text.append(name);
            snprintf(num, sizeof num, "\t%u\t%llu\t%llu\t", ++rank, (unsigned long long)h.second, (unsigned long long)depth[t]);
            hf.text += num;
            hf.text += h.first;
            hf.text += '\n';
          }
          strings.clear();
          hf.flush(false);
        }
      }
    }
  }
  af.close();
  hf.close();
}

// --msa / --profile: the pairs (read pa, centre pb < C, strand pm) of the assigned reads, sorted by
// centre (input order kept), through one mc_nw_msa_begin with the centres that have a read as
// targets.  --msa: the rows come back through two windows of at most 32 MiB, one over the centre rows
// and one over the pair rows, and are written block by block.  --profile: profile_output on the same
// plan; --variants / --alleles / --haplotypes: variants_output on it.  t0: when the caller began to list the
// pairs; that, the sort and the begin are timed with the first output that is asked for, the others on their
// own (r.msa_ms, r.profile_ms, r.variants_ms; the caller adds what follows the last of them).
static void msa_output(mc_ctx *ctx, const Dataset &ds, uint32_t C, const std::vector<uint32_t> &pa, const std::vector<uint32_t> &pb,
                       const std::vector<uint8_t> &pm, const AssignOptions &opt, AssignResult &r,
                       std::chrono::steady_clock::time_point t0) {
  const size_t m = pa.size();
  std::vector<uint64_t> from((size_t)C + 1, 0);  // a centre's pairs after the sort: from[c] .. from[c + 1]
  for (size_t p = 0; p < m; p++) from[pb[p] + 1]++;
  for (uint32_t j = 0; j < C; j++) from[j + 1] += from[j];
  std::vector<uint32_t> qa(m), qb(m), targets;
  std::vector<uint8_t> qm(m);
  {
    std::vector<uint64_t> at(from.begin(), from.end() - 1);
    for (size_t p = 0; p < m; p++) {
      const uint64_t k = at[pb[p]]++;
      qa[k] = pa[p], qb[k] = pb[p], qm[k] = pm[p];
    }
  }
  std::vector<uint32_t> tof(m);  // a sorted pair's place among the targets
  for (uint32_t j = 0; j < C; j++)
    if (from[j + 1] > from[j]) {
      std::fill(tof.begin() + from[j], tof.begin() + from[j + 1], (uint32_t)targets.size());
      targets.push_back(j);
    }
  const uint32_t nt = (uint32_t)targets.size();
  std::vector<uint64_t> row_off((size_t)nt + 1), W(nt);
  check(mc_nw_msa_begin(ctx, qa.data(), qb.data(), qm.data(), m, targets.data(), nt, row_off.data(), nullptr, W.data(), nullptr, nullptr,
                        nullptr),
        "mc_nw_msa_begin");
  struct End {
    mc_ctx *c;
    ~End() { mc_nw_msa_end(c); }
  } ender{ctx};
  std::vector<uint64_t> depths(nt);
  for (uint32_t t = 0; t < nt; t++) depths[t] = from[targets[t] + 1] - from[targets[t]];
  // the sort and the begin count with the first output (mark starts at the caller's t0); every later one is timed on its own
  auto mark = t0;
  auto lap = [&](double &ms) {
    ms = ms_since(mark);
    mark = std::chrono::steady_clock::now();
  };
  auto rest = [&]() {  // --profile, then the three variant files, on the same plan and, given together, one pass over its tables
    const bool var = opt.any_variants();
    SiteLists sl;
    if (!opt.profile.empty()) {
      profile_output(ctx, ds, targets, W, depths, opt, r, true, var ? &sl : nullptr);
      lap(r.profile_ms);
    }
    if (var) {
      if (opt.profile.empty()) profile_output(ctx, ds, targets, W, depths, opt, r, false, &sl);
      variants_output(ctx, ds, targets, depths, qa, qm, tof, sl, opt, r);
      lap(r.variants_ms);
    }
  };
  if (opt.msa.empty()) {
    rest();
    return;
  }
  r.msa = true;
  r.msa_pairs = m;
  r.msa_centres = nt;
  FILE *f = fopen(opt.msa.c_str(), "w");
  if (!f) throw Error("cannot write " + opt.msa + ": " + strerror(errno), 1);
  struct Close {
    FILE *&f;
    ~Close() {
      if (f) fclose(f);
    }
  } closer{f};
  // a window over rows [lo, hi) of mc_nw_msa_rows' numbering; width_of(row) is the row's W
  const uint64_t kWindow = 32ull << 20;
  struct Window {
    uint64_t lo = 0, hi = 0;
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> off;
  } win[2];
  auto row = [&](Window &w, uint64_t k, uint64_t end, const std::function<uint64_t(uint64_t)> &width_of) -> const uint8_t * {
    if (k >= w.hi) {  // the rows from k on that fit the window (one at least)
      uint64_t n = 0, sum = 0;
      while (k + n < end && (n == 0 || sum + width_of(k + n) <= kWindow)) sum += width_of(k + n++);
      w.bytes.resize(sum);
      w.off.resize(n + 1);
      check(mc_nw_msa_rows(ctx, k, n, w.bytes.data(), sum, w.off.data()), "mc_nw_msa_rows");
      w.lo = k;
      w.hi = k + n;
    }
    return w.bytes.data() + w.off[k - w.lo];
  };
  std::string text;
  char num[96];
  auto flush = [&](bool all) {
    if (text.size() < (all ? 1u : 1u << 20)) return;
    if (fwrite(text.data(), 1, text.size(), f) != text.size()) throw Error("cannot write " + opt.msa, 1);
    text.clear();
  };
  for (uint32_t t = 0; t < nt; t++) {
    const uint32_t j = targets[t];
    const uint64_t depth = from[j + 1] - from[j];
    r.msa_columns += W[t];
    r.msa_bytes += (depth + 1) * W[t];
    text.append(ds.headers[j]);
    snprintf(num, sizeof num, " depth=%llu width=%llu\n", (unsigned long long)depth, (unsigned long long)W[t]);
    text += num;
    text.append((const char *)row(win[0], t, nt, [&](uint64_t k) { return W[k]; }), W[t]);
    text += '\n';
    for (uint64_t k = from[j]; k < from[j + 1]; k++) {
      text.append(ds.headers[qa[k]]);
      text += qm[k] ? " strand=-\n" : " strand=+\n";
      text.append((const char *)row(win[1], nt + k, nt + m, [&](uint64_t x) { return W[tof[x - nt]]; }), W[t]);
      text += '\n';
      flush(false);
    }
  }
  flush(true);
  FILE *done = f;
  f = nullptr;
  if (fclose(done) != 0) throw Error("cannot write " + opt.msa, 1);
  lap(r.msa_ms);
  rest();
}

// --chimeras: chimera.hpp over the reads' hits (rows of K slots, mc_assign_top's order), in plans of its own.  The
// reads with a candidate go in ranges whose pairs stay within kPairs; a read's pairs are its first hit and its
// candidates, the plan's targets the centres among a range's pairs.
static void chimera_output(mc_ctx *ctx, const Dataset &ds, uint64_t C, uint64_t M, uint32_t K, const std::vector<uint32_t> &hit,
                           const std::vector<uint8_t> &hit_strand, const AssignOptions &opt, AssignResult &r) {
  r.chimeras = true;
  TextFile cf(opt.chimeras);
  const uint64_t kPairs = 1ull << 18;
  std::vector<uint32_t> pa, pb, targets, cand(K), rcand;  // rcand: the candidates' hit indices, read after read
  std::vector<uint8_t> pm;
  std::vector<uint64_t> x, y, reads, rfirst;  // reads: the range's reads; rfirst: where a read's candidates start
  std::vector<int32_t> res;
  char num[160];
  auto flush = [&]() {
    if (reads.empty()) return;
    targets = pb;
    std::sort(targets.begin(), targets.end());
    targets.erase(std::unique(targets.begin(), targets.end()), targets.end());
    const uint32_t nt = (uint32_t)targets.size();
    std::vector<uint64_t> row_off((size_t)nt + 1), W(nt);
    check(mc_nw_msa_begin(ctx, pa.data(), pb.data(), pm.data(), pa.size(), targets.data(), nt, row_off.data(), nullptr, W.data(),
                          nullptr, nullptr, nullptr),
          "mc_nw_msa_begin");
    struct End {
      mc_ctx *c;
      ~End() { mc_nw_msa_end(c); }
    } ender{ctx};
    res.assign(x.size() * MC_CROSS_RES, 0);
    check(mc_nw_msa_crossover(ctx, x.data(), y.data(), x.size(), res.data()), "mc_nw_msa_crossover");
    rfirst.push_back(x.size());
    for (size_t n = 0; n < reads.size(); n++) {
      const uint64_t q = reads[n], k0 = rfirst[n], k = rfirst[n + 1] - k0;
      const ChimeraCall c = chimera_pick(rcand.data() + k0, (uint32_t)k, res.data() + k0 * MC_CROSS_RES, opt.min_chimera_gain);
      const uint64_t h1 = q * K, h2 = q * K + (uint64_t)c.hit, left = c.xy ? h1 : h2, right = c.xy ? h2 : h1;
      std::string &text = cf.text;
      text.append(ds.headers[C + q].substr(1));
      text += '\t';
      text.append(ds.headers[hit[left]].substr(1));
      text += '\t';
      text.append(ds.headers[hit[right]].substr(1));
      snprintf(num, sizeof num, "\t%c\t%c\t%d\t%d\t%d\t%d\t%d\t%d\t%llu\t%c\n", hit_strand[left] ? '-' : '+',
               hit_strand[right] ? '-' : '+', c.cut_first, c.cut_last, c.ids_left, c.ids_right, c.best, c.gain,
               (unsigned long long)ds.lengths[C + q], c.flag ? 'Y' : 'N');
      text += num;
      r.chimera_candidates++;
      if (c.flag) r.chimera_flagged++;
      cf.flush(false);
    }
    pa.clear(), pb.clear(), pm.clear(), x.clear(), y.clear(), reads.clear(), rfirst.clear(), rcand.clear();
  };
  for (uint64_t q = 0; q < M; q++) {
    uint32_t n = 0;
    while (n < K && hit[q * K + n] != MC_ASSIGN_NONE) n++;
    const uint32_t k = n ? chimera_candidates(&hit[q * K], n, cand.data()) : 0;
    if (k == 0) continue;
    if (!pa.empty() && pa.size() + k + 1 > kPairs) flush();
    reads.push_back(q);
    rfirst.push_back(x.size());
    const uint64_t first = pa.size();
    for (uint32_t t = 0; t <= k; t++) {  // the first hit, then the candidates
      const uint32_t j = t ? cand[t - 1] : 0;
      pa.push_back((uint32_t)(C + q));
      pb.push_back(hit[q * K + j]);
      pm.push_back(hit_strand[q * K + j]);
      if (t) {
        x.push_back(first);
        y.push_back(first + t);
        rcand.push_back(j);
      }
    }
  }
  flush();
  cf.close();
}

AssignResult run_assign(mc_ctx *ctx, const AssignOptions &opt_in) {
  AssignOptions opt = opt_in;
  AssignResult r;
  struct Own {  // a context of the tool's own, opened only once the inputs are accepted
    mc_ctx *c = nullptr;
    ~Own() {
      if (c) mc_ctx_destroy(c);
    }
  } own;
  int threads = opt.threads;
#ifdef _OPENMP
  if (threads <= 0) threads = omp_get_max_threads();
#else
  threads = 1;
#endif
  bool by_pairs = getenv("MC_ASSIGN_PAIRS") && atoi(getenv("MC_ASSIGN_PAIRS")) != 0;
  // the pair list has no permuted rows: never score one strand where two were asked for
  const char *no_strands = "meshclust-assign: --both-strands needs the device kernel (mc_assign_strands), which does not apply here: ";
  if (by_pairs && opt.both_strands) {  // (refused before anything else is read; a version-2 model has its own rows)
    bool v2 = false;
    try {
      v2 = read_model(opt.model).strands != 1;
    } catch (const Error &) {
    }
    if (!v2) throw Error(std::string(no_strands) + "MC_ASSIGN_PAIRS is set", 2);
  }
  const Model model = read_model(opt.model);
  // a version-2 model (meshclust --both-strands): reads and centres as canonical rows, scored once
  // (the rows are symmetric: a minus pass would list every hit twice), every reported hit's strand
  // from mc_orient_pairs on the forward rows; from there on the job runs as with --both-strands
  const bool canon = model.strands != 1;
  if (canon) opt.both_strands = true;
  if (model.align)
    throw Error("meshclust-assign: " + opt.model +
                    " is an alignment-mode model (--align or --id below 0.6); only k-mer classifiers can be assigned against",
                2);
  auto t0 = std::chrono::steady_clock::now();
  std::vector<std::string> files{opt.centres};
  files.insert(files.end(), opt.reads.begin(), opt.reads.end());
  Dataset ds;
  parse_fasta_files(files, ds, threads, opt.quality);  // centres first: their ids are 0 .. C-1
  if (opt.quality)
    for (size_t f = 1; f < files.size(); f++)
      if (!ds.file_fastq[f]) throw Error("meshclust-assign: --quality needs FASTQ reads, " + files[f] + " is FASTA", 2);
  r.parse_ms = ms_since(t0);
  const uint64_t C = ds.file_count.empty() ? 0 : ds.file_count[0];
  if (C != model.centres)
    throw Error("meshclust-assign: " + opt.centres + " holds " + std::to_string(C) + " records, the model was saved with " +
                    std::to_string(model.centres) + " centres",
                2);
  if (C == 0) throw Error("meshclust-assign: no centres", 2);
  const uint64_t M = ds.size() - C;
  r.reads = M;
  r.centres = C;
  r.k = model.k;
  if (!ctx) {
    check(mc_ctx_create(opt.device, &own.c), "mc_ctx_create");
    ctx = own.c;
  }
  struct BandOff {  // --band: the certified band for this run's alignments, the context left at the full record
    mc_ctx *c = nullptr;
    ~BandOff() {
      if (c) mc_set_align_band(c, 0);
    }
  } band_off;
  if (opt.band) {
    double unused[5];
    check(mc_set_align_band(ctx, 1), "mc_set_align_band");
    band_off.c = ctx;
    check(mc_nw_band_profile(ctx, unused, 1), "mc_nw_band_profile");
  }
  t0 = std::chrono::steady_clock::now();
  check(mc_load_packed(ctx, ds.packed.data(), ds.pk_off.data(), ds.seq_off.data(), ds.size(), ds.exc_pos.data(),
                       ds.exc_val.data(), ds.exc_pos.size(), ds.seg.data(), ds.seg_off.data()),
        "mc_load_packed");
  if (opt.quality) {
    check(mc_load_qualities(ctx, ds.qual.data(), ds.bases()), "mc_load_qualities");
    r.quality = true;
  }
  r.upload_ms = ms_since(t0);
  t0 = std::chrono::steady_clock::now();
  uint64_t largest = 0;
  const char *no_canon = "meshclust-assign: a version-2 model (meshclust --both-strands) needs canonical rows, which this input cannot have: ";
  if (canon) {
    const int rc = mc_kmer_max_strands(ctx, model.k, model.strands, &largest);
    if (rc == MC_ERR_UNSUPPORTED) throw Error(std::string(no_canon) + mc_last_error(), 2);
    check(rc, "mc_kmer_max_strands");
  } else {
    check(mc_kmer_max(ctx, model.k, &largest), "mc_kmer_max");
  }
  int width = largest <= 0xff ? 1 : largest <= 0xffff ? 2 : largest <= 0xffffffffull ? 4 : 8;  // as run_pipeline
  if (const char *fw = getenv("MC_FORCE_WIDTH")) width = std::max(width, atoi(fw));
  r.width = width;
  if (canon) {
    const int rc = mc_kmer_build_strands(ctx, model.k, width, model.strands);
    if (rc == MC_ERR_UNSUPPORTED) throw Error(std::string(no_canon) + mc_last_error(), 2);
    check(rc, "mc_kmer_build_strands");
  } else {
    check(mc_kmer_build(ctx, model.k, width), "mc_kmer_build");
  }
  check(mc_set_classifier(ctx, &model.cls), "mc_set_classifier");
  r.kmer_ms = ms_since(t0);
  t0 = std::chrono::steady_clock::now();
  std::vector<uint32_t> best(M, MC_ASSIGN_NONE), nsim(M, 0);
  std::vector<double> val(M, -1.0);
  std::vector<uint8_t> strand;
  if (opt.both_strands) {
    r.strands = MC_STRAND_PLUS | MC_STRAND_MINUS;
    strand.assign(M, 0);
  }
  // --top: rows of K slots per read, in mc_assign_top's order; the main TSV's row is rank 1
  const uint32_t K = (uint32_t)opt.top;
  r.top = opt.top;
  std::vector<uint32_t> hit((size_t)M * K, MC_ASSIGN_NONE);
  std::vector<double> hit_val((size_t)M * K, -1.0);
  std::vector<uint8_t> hit_strand((size_t)M * K, 0);
  if (!by_pairs) {
    std::vector<uint32_t> cid(C), qid(M);
    for (uint64_t j = 0; j < C; j++) cid[j] = (uint32_t)j;
    for (uint64_t q = 0; q < M; q++) qid[q] = (uint32_t)(C + q);
    uint64_t st[3] = {0, 0, 0};
    const int score = canon ? MC_STRAND_PLUS : r.strands;  // canonical rows: the plus strand set only
    const int rc = K > 0
                       ? mc_assign_top(ctx, cid.data(), (uint32_t)C, qid.data(), M, model.id, score, K, hit.data(),
                                       hit_val.data(), hit_strand.data(), nsim.data(), st)
                   : opt.both_strands && !canon
                       ? mc_assign_strands(ctx, cid.data(), (uint32_t)C, qid.data(), M, model.id, score, best.data(),
                                           val.data(), strand.data(), nsim.data(), st)
                       : mc_assign(ctx, cid.data(), (uint32_t)C, qid.data(), M, model.id, best.data(), val.data(),
                                   nsim.data(), st);
    if (rc == MC_ERR_UNSUPPORTED && opt.both_strands && !canon) throw Error(std::string(no_strands) + mc_last_error(), 2);
    if (rc == MC_ERR_UNSUPPORTED) {  // wide bins or rows: the pair list does the same job
      if (!opt.quiet) fprintf(stderr, "meshclust-assign: %s; scoring with mc_classify_pairs\n", mc_last_error());
      by_pairs = true;
    } else {
      check(rc, "mc_assign");
      if (K > 0)
        for (uint64_t q = 0; q < M; q++) {
          best[q] = hit[q * K];
          val[q] = hit_val[q * K];
          if (opt.both_strands) strand[q] = hit_strand[q * K];
        }
      r.candidates = st[0];
      r.fallbacks = st[1];
      r.device_us = st[2];
    }
  }
  if (by_pairs) {
    assign_by_pairs(ctx, ds, (uint32_t)C, M, model.id, best, val, nsim, &r.candidates, K, hit, hit_val);
  }
  if (canon) {
    // the strand of every reported (read, centre): mc_orient_pairs, the pairs grouped by centre
    const uint32_t Kr = K > 0 ? K : 1;
    const uint32_t *cj = K > 0 ? hit.data() : best.data();
    std::vector<uint64_t> slot;
    for (uint64_t q = 0; q < M; q++)
      for (uint32_t t = 0; t < Kr && cj[q * Kr + t] != MC_ASSIGN_NONE; t++) slot.push_back(q * Kr + t);
    std::stable_sort(slot.begin(), slot.end(), [&](uint64_t x, uint64_t y) { return cj[x] < cj[y]; });
    std::vector<uint32_t> oa(slot.size()), ob(slot.size());
    for (size_t p = 0; p < slot.size(); p++) {
      oa[p] = (uint32_t)(C + slot[p] / Kr);
      ob[p] = cj[slot[p]];
    }
    std::vector<uint8_t> os(slot.size(), 0);
    check(mc_orient_pairs(ctx, oa.data(), ob.data(), slot.size(), os.data(), nullptr), "mc_orient_pairs");
    for (size_t p = 0; p < slot.size(); p++) {
      if (K > 0) hit_strand[slot[p]] = os[p];
      if (slot[p] % Kr == 0) strand[slot[p] / Kr] = os[p];
    }
  }
  r.path = by_pairs ? "pairs" : "device";
  r.assign_ms = ms_since(t0);
  t0 = std::chrono::steady_clock::now();
  // --identity: every reported (read, centre, strand) aligned in one call, the read as seq1 and
  // reverse-complemented where the strand is minus.  A read's candidates are its hits (rank 1 is
  // the TSV's row: aligned once), or its one assignment without --top.
  const uint32_t Kc = K > 0 ? K : 1;
  std::vector<double> cand_id;  // Kc slots per read, as hit / hit_val
  std::vector<double> ident_q(M, -1.0);
  const bool pile = !opt.consensus.empty() || !opt.pileup.empty();
  const bool pile_only = pile && K == 0 && opt.min_identity < 0 && opt.paf.empty();
  if (opt.identity || pile) {
    r.identity = true;
    const uint32_t *cj = K > 0 ? hit.data() : best.data();
    const double *cv = K > 0 ? hit_val.data() : val.data();
    const uint8_t *cs = K > 0 ? hit_strand.data() : opt.both_strands ? strand.data() : nullptr;
    std::vector<uint32_t> pa, pb;
    std::vector<uint8_t> pm;
    std::vector<uint64_t> first(M + 1, 0);  // a read's candidates are pairs first[q] .. first[q + 1]
    for (uint64_t q = 0; q < M; q++) {
      for (uint32_t t = 0; t < Kc && cj[q * Kc + t] != MC_ASSIGN_NONE; t++) {
        pa.push_back((uint32_t)(C + q));
        pb.push_back(cj[q * Kc + t]);
        pm.push_back(cs ? cs[q * Kc + t] : 0);
        r.identity_cells += ds.lengths[C + q] * ds.lengths[cj[q * Kc + t]];
      }
      first[q + 1] = pa.size();
    }
    r.identity_pairs = pa.size();
    std::vector<double> pid(pa.size(), 0.0);
    if (pile_only) {
      // the reported pairs are the assigned reads' own: the pile-up is the one alignment pass, and
      // the identity its ids / len, the division mc_nw_identity does
      r.consensus_passes = 1;
      pileup_outputs(ctx, ds, (uint32_t)C, pa, pb, pm, opt, r, &pid);
    } else if (opt.paf.empty()) {
      check(mc_nw_identity_strands(ctx, pa.data(), pb.data(), pm.data(), pa.size(), pid.data(), nullptr, nullptr),
            "mc_nw_identity_strands");
    } else {
      // --paf: the same pairs through mc_nw_align_strands, in chunks whose strings hold at most
      // 2^26 bases together -- an upper bound on a chunk's operation words, so one buffer serves
      // every chunk.  The identity is ids / len of that call, the division mc_nw_identity does.
      r.paf = true;
      const uint64_t kChunk = 1ull << 26;
      std::vector<size_t> cut{0};  // chunk c is pairs cut[c] .. cut[c + 1]
      uint64_t cap = 0, sum = 0;   // the largest chunk's bound (one pair may exceed 2^26 alone)
      for (size_t p = 0; p < pa.size(); p++) {
        const uint64_t w = ds.lengths[pa[p]] + ds.lengths[pb[p]];
        if (p > cut.back() && sum + w > kChunk) {
          cut.push_back(p);
          sum = 0;
        }
        sum += w;
        cap = std::max(cap, sum);
      }
      cut.push_back(pa.size());
      FILE *pf = fopen(opt.paf.c_str(), "w");
      if (!pf) throw Error("cannot write " + opt.paf + ": " + strerror(errno), 1);
      struct Close {
        FILE *&f;
        ~Close() {
          if (f) fclose(f);
        }
      } closer{pf};
      std::vector<uint32_t> cig(cap);
      std::vector<uint64_t> off;
      std::vector<int32_t> sc, ln, idn;
      std::string paf;
      char num[96];
      uint64_t q = 0;  // the read of the pair being written
      for (size_t c = 0; c + 1 < cut.size(); c++) {
        const size_t p0 = cut[c], n = cut[c + 1] - p0;
        if (n == 0) continue;
        off.assign(n + 1, 0);
        sc.assign(n, 0);
        ln.assign(n, 0);
        idn.assign(n, 0);
        check(mc_nw_align_strands(ctx, pa.data() + p0, pb.data() + p0, pm.data() + p0, n, cig.data(), cig.size(), off.data(),
                                  sc.data(), ln.data(), idn.data()),
              "mc_nw_align_strands");
        paf.clear();
        for (size_t k = 0; k < n; k++) {
          const size_t p = p0 + k;
          pid[p] = (double)idn[k] / (double)ln[k];
          while (first[q + 1] <= p) q++;
          const unsigned long long lq = ds.lengths[pa[p]], lc = ds.lengths[pb[p]];
          paf.append(ds.headers[pa[p]].substr(1));
          snprintf(num, sizeof num, "\t%llu\t0\t%llu\t%c\t", lq, lq, pm[p] ? '-' : '+');
          paf += num;
          paf.append(ds.headers[pb[p]].substr(1));
          snprintf(num, sizeof num, "\t%llu\t0\t%llu\t%d\t%d\t255\tAS:i:%d\trk:i:%llu\tcg:Z:", lc, lc, idn[k], ln[k], sc[k],
                   (unsigned long long)(p - first[q] + 1));
          paf += num;
          cigar_append(paf, cig.data() + off[k], off[k + 1] - off[k]);
          paf += '\n';
        }
        if (fwrite(paf.data(), 1, paf.size(), pf) != paf.size()) throw Error("cannot write " + opt.paf, 1);
        r.cigar_ops += off[n];
      }
      r.paf_pairs = pa.size();
      FILE *done = pf;
      pf = nullptr;
      if (fclose(done) != 0) throw Error("cannot write " + opt.paf, 1);
    }
    cand_id.assign((size_t)M * Kc, -1.0);
    for (uint64_t q = 0; q < M; q++) {
      const uint32_t n = (uint32_t)(first[q + 1] - first[q]);
      std::copy(pid.begin() + first[q], pid.begin() + first[q + 1], cand_id.begin() + q * Kc);
      int pick = n ? 0 : -1;
      if (opt.min_identity >= 0) {  // the first candidate the alignment confirms (verify.hpp), or none
        pick = verify_pick(&cand_id[q * Kc], n, opt.min_identity);
        if (n && pick < 0) r.rejected++;
        best[q] = pick < 0 ? MC_ASSIGN_NONE : cj[q * Kc + pick];
        val[q] = pick < 0 ? -1.0 : cv[q * Kc + pick];
        if (opt.both_strands) strand[q] = pick < 0 ? 0 : cs[q * Kc + pick];
      }
      if (pick >= 0) ident_q[q] = cand_id[q * Kc + pick];
    }
    if (pile && !pile_only) {  // a second pass, over the pairs the selection kept
      r.consensus_passes = 2;
      pa.clear(), pb.clear(), pm.clear();
      for (uint64_t q = 0; q < M; q++)
        if (best[q] != MC_ASSIGN_NONE) {
          pa.push_back((uint32_t)(C + q));
          pb.push_back(best[q]);
          pm.push_back(opt.both_strands ? strand[q] : 0);
        }
      pileup_outputs(ctx, ds, (uint32_t)C, pa, pb, pm, opt, r, nullptr);
    }
  }
  r.identity_ms = ms_since(t0);
  if (!opt.msa.empty() || !opt.profile.empty() || opt.any_variants()) {  // a pass of its own, over the pairs --consensus takes
    t0 = std::chrono::steady_clock::now();
    std::vector<uint32_t> pa, pb;
    std::vector<uint8_t> pm;
    for (uint64_t q = 0; q < M; q++)
      if (best[q] != MC_ASSIGN_NONE) {
        pa.push_back((uint32_t)(C + q));
        pb.push_back(best[q]);
        pm.push_back(opt.both_strands ? strand[q] : 0);
      }
    msa_output(ctx, ds, (uint32_t)C, pa, pb, pm, opt, r, t0);
    // the whole pass is accounted for: what follows the last output (mc_nw_msa_end) goes where it went before
    // the variant files, to msa beside --msa, else to profile
    const double tail = ms_since(t0) - (r.msa_ms + r.profile_ms + r.variants_ms);
    (r.msa ? r.msa_ms : r.profile ? r.profile_ms : r.variants_ms) += tail;
  }
  if (!opt.chimeras.empty()) {  // after every other user of the plan: its begins drop theirs
    t0 = std::chrono::steady_clock::now();
    chimera_output(ctx, ds, C, M, K, hit, hit_strand, opt, r);
    r.chimeras_ms = ms_since(t0);
  }
  t0 = std::chrono::steady_clock::now();
  // one line per read, in input order: read header, centre header or *, cluster index or -1,
  // combo 0, similar centres (headers without their '>'); with both strands a sixth column: the
  // strand the read was assigned on (+ or -), or * for an unassigned read; with --identity a last
  // column: the identity of the row's alignment, or *
  std::string out;
  std::vector<uint32_t> rest;
  char num[64];
  for (uint64_t q = 0; q < M; q++) {
    const bool has = best[q] != MC_ASSIGN_NONE;
    out.append(ds.headers[C + q].substr(1));
    out += '\t';
    if (has) out.append(ds.headers[best[q]].substr(1));
    else out += '*';
    snprintf(num, sizeof num, "\t%d\t%.17g\t%u", has ? (int)best[q] : -1, val[q], nsim[q]);
    out += num;
    if (opt.both_strands) {
      out += '\t';
      out += !has ? '*' : strand[q] ? '-' : '+';
      if (has && strand[q]) r.assigned_minus++;
    }
    if (opt.identity) {  // the last column: the alignment identity of the row's pair, or *
      if (has) snprintf(num, sizeof num, "\t%.17g", ident_q[q]);
      out += has ? num : "\t*";
    }
    out += '\n';
    if (has) r.assigned++;
    else rest.push_back((uint32_t)(C + q));
  }
  FILE *f = fopen(opt.output.c_str(), "w");
  if (!f) throw Error("cannot write " + opt.output + ": " + strerror(errno), 1);
  const bool ok = fwrite(out.data(), 1, out.size(), f) == out.size();
  if (fclose(f) != 0 || !ok) throw Error("cannot write " + opt.output, 1);
  if (!opt.unassigned.empty()) write_fasta(opt.unassigned, ds, rest.data(), rest.size());
  if (K > 0) {
    // one line per hit, reads in input order, ranks ascending: read header, rank (from 1), centre
    // header, cluster index, combo 0; with both strands the hit's strand (+ or -); with --identity
    // the identity of the hit's alignment
    out.clear();
    for (uint64_t q = 0; q < M; q++)
      for (uint32_t t = 0; t < K && hit[q * K + t] != MC_ASSIGN_NONE; t++) {
        const uint32_t j = hit[q * K + t];
        out.append(ds.headers[C + q].substr(1));
        snprintf(num, sizeof num, "\t%u\t", t + 1);
        out += num;
        out.append(ds.headers[j].substr(1));
        snprintf(num, sizeof num, "\t%u\t%.17g", j, hit_val[q * K + t]);
        out += num;
        if (opt.both_strands) out += hit_strand[q * K + t] ? "\t-" : "\t+";
        if (opt.identity) {
          snprintf(num, sizeof num, "\t%.17g", cand_id[q * K + t]);
          out += num;
        }
        out += '\n';
        r.hits++;
      }
    FILE *h = fopen(opt.hits.c_str(), "w");
    if (!h) throw Error("cannot write " + opt.hits + ": " + strerror(errno), 1);
    const bool hok = fwrite(out.data(), 1, out.size(), h) == out.size();
    if (fclose(h) != 0 || !hok) throw Error("cannot write " + opt.hits, 1);
  }
  r.write_ms = ms_since(t0);
  if (opt.band) {
    double bp[5];
    check(mc_nw_band_profile(ctx, bp, 0), "mc_nw_band_profile");
    r.band = true;
    r.band_pairs = (uint64_t)bp[0];
    r.band_full = (uint64_t)bp[1];
    r.band_launches = (uint64_t)bp[2];
    r.band_w_sum = (uint64_t)bp[4];
  }
  return r;
}

std::string assign_stats_json(const AssignResult &r) {
  // (one strand, no --top, no --identity: exactly the keys there were before any of the options)
  char b[2560], s[704] = "", idms[48] = "", msa[224] = "", msams[48] = "", prof[128] = "", profms[48] = "", band[224] = "";
  char var[192] = "", varms[48] = "", chim[128] = "", chimms[48] = "";
  int n = 0;
  if (r.strands != MC_STRAND_PLUS)
    n = snprintf(s, sizeof s, "\"strands\": %d, \"assigned_minus\": %llu, ", r.strands, (unsigned long long)r.assigned_minus);
  if (r.top > 0) n += snprintf(s + n, sizeof s - n, "\"top\": %d, \"hits\": %llu, ", r.top, (unsigned long long)r.hits);
  if (r.identity) {
    n += snprintf(s + n, sizeof s - n, "\"identity_pairs\": %llu, \"identity_cells\": %llu, \"rejected\": %llu, ",
                  (unsigned long long)r.identity_pairs, (unsigned long long)r.identity_cells, (unsigned long long)r.rejected);
    if (r.paf)
      n += snprintf(s + n, sizeof s - n, "\"paf_pairs\": %llu, \"cigar_ops\": %llu, ", (unsigned long long)r.paf_pairs,
                    (unsigned long long)r.cigar_ops);
    if (r.consensus)
      snprintf(s + n, sizeof s - n,
               "\"consensus_pairs\": %llu, \"consensus_centres\": %llu, \"consensus_passes\": %d, \"realigned_centres\": %llu, "
               "\"insertion_sites\": %llu, %s",
               (unsigned long long)r.consensus_pairs, (unsigned long long)r.consensus_centres, r.consensus_passes,
               (unsigned long long)r.realigned_centres, (unsigned long long)r.insertion_sites, r.quality ? "\"quality\": 1, " : "");
    snprintf(idms, sizeof idms, "\"identity\": %.3f, ", r.identity_ms);
  }
  if (r.msa) {  // after every key there was before --msa
    snprintf(msa, sizeof msa, ", \"msa_pairs\": %llu, \"msa_centres\": %llu, \"msa_columns\": %llu, \"msa_bytes\": %llu",
             (unsigned long long)r.msa_pairs, (unsigned long long)r.msa_centres, (unsigned long long)r.msa_columns,
             (unsigned long long)r.msa_bytes);
    snprintf(msams, sizeof msams, ", \"msa\": %.3f", r.msa_ms);
  }
  if (r.profile) {  // after every key there was before --profile
    snprintf(prof, sizeof prof, ", \"profile_centres\": %llu, \"profile_columns\": %llu", (unsigned long long)r.profile_centres,
             (unsigned long long)r.profile_columns);
    snprintf(profms, sizeof profms, ", \"profile\": %.3f", r.profile_ms);
  }
  if (r.band)  // after every key there was before --band
    snprintf(band, sizeof band, ", \"band_pairs\": %llu, \"band_full\": %llu, \"band_launches\": %llu, \"band_w_sum\": %llu",
             (unsigned long long)r.band_pairs, (unsigned long long)r.band_full, (unsigned long long)r.band_launches,
             (unsigned long long)r.band_w_sum);
  if (r.variants) {  // after every key there was before --variants / --alleles / --haplotypes
    snprintf(var, sizeof var, ", \"variant_centres\": %llu, \"variant_sites\": %llu, \"allele_bytes\": %llu",
             (unsigned long long)r.variant_centres, (unsigned long long)r.variant_sites, (unsigned long long)r.allele_bytes);
    snprintf(varms, sizeof varms, ", \"variants\": %.3f", r.variants_ms);
  }
  if (r.chimeras) {  // after every key there was before --chimeras
    snprintf(chim, sizeof chim, ", \"chimera_candidates\": %llu, \"chimeras\": %llu", (unsigned long long)r.chimera_candidates,
             (unsigned long long)r.chimera_flagged);
    snprintf(chimms, sizeof chimms, ", \"chimeras\": %.3f", r.chimeras_ms);
  }
  snprintf(b, sizeof b,
           "{\"reads\": %llu, \"centres\": %llu, \"assigned\": %llu, \"unassigned\": %llu, %s\"k\": %d, \"width\": %d, "
           "\"path\": \"%s\", \"candidate_pairs\": %llu, \"fallback_pairs\": %llu, \"device_us\": %llu, "
           "\"phases_ms\": {\"parse\": %.3f, \"upload\": %.3f, \"kmer\": %.3f, \"assign\": %.3f, %s\"write\": %.3f%s%s%s%s}%s%s%s%s%s}",
           (unsigned long long)r.reads, (unsigned long long)r.centres, (unsigned long long)r.assigned,
           (unsigned long long)(r.reads - r.assigned), s, r.k, r.width, r.path.c_str(), (unsigned long long)r.candidates,
           (unsigned long long)r.fallbacks, (unsigned long long)r.device_us, r.parse_ms, r.upload_ms, r.kmer_ms,
           r.assign_ms, idms, r.write_ms, msams, profms, varms, chimms, msa, prof, band, var, chim);
  return b;
}

int assign_main(int argc, char **argv) {
  try {
    const AssignOptions opt = parse_assign_options(argc, argv);
#ifdef _OPENMP
    if (opt.threads > 0) omp_set_num_threads(opt.threads);
#endif
    const AssignResult r = run_assign(nullptr, opt);
    if (!opt.quiet)
      printf("%llu reads, %llu centres: %llu assigned, %llu unassigned (%s)\n", (unsigned long long)r.reads,
             (unsigned long long)r.centres, (unsigned long long)r.assigned, (unsigned long long)(r.reads - r.assigned),
             r.path.c_str());
    if (!opt.stats_json.empty()) {
      if (FILE *f = fopen(opt.stats_json.c_str(), "w")) {
        fprintf(f, "%s\n", assign_stats_json(r).c_str());
        fclose(f);
      }
    }
    return 0;
  } catch (const Error &e) {
    fprintf(stderr, "%s\n", e.what());
    return e.code ? e.code : 1;
  } catch (const std::exception &e) {
    fprintf(stderr, "meshclust-assign: %s\n", e.what());
    return 1;
  }
}

}  // namespace mc
