// capi_assign.cpp -- libmeshclust.so's C entries for read assignment (assign.hpp) and the
// FASTA writer of model.hpp (used by the Python package and the tests).
#include <cstring>
#include <string>
#include <vector>

#include "assign.hpp"
#include "fasta.hpp"
#include "model.hpp"

extern "C" {

// Assign the reads of reads[0..nreads) to the centres of a saved clustering on an open context
// (assign.hpp run_assign): writes the TSV to `tsv` and, if `unassigned` is non-NULL, the
// unassigned reads as FASTA.  The JSON summary goes to stats (cap bytes).  Returns 0 or an
// error code with {"error": ...} in stats; an error never ends the calling process.
struct VariantArgs {  // mcl_assign_variants' own arguments; the defaults are "none of them"
  const char *variants = nullptr, *alleles = nullptr, *haplotypes = nullptr;
  double min_allele_frac = 0.2;
  long long min_allele_count = 2;
  const char *chimeras = nullptr;  // mcl_assign_chimeras' own
  long long min_chimera_gain = 3;
};

static int assign_entry(mc_ctx *ctx, const char *model, const char *centres, const char *const *reads, int nreads,
                        int threads, const char *tsv, const char *unassigned, bool both_strands, int top, const char *hits,
                        int identity, double min_identity, const char *paf, const char *consensus, const char *pileup,
                        bool quality, const char *msa, const char *profile, bool band, char *stats, int cap,
                        const VariantArgs &va = VariantArgs()) {
  try {
    mc::AssignOptions opt;
    if (va.variants) opt.variants = va.variants;
    if (va.alleles) opt.alleles = va.alleles;
    if (va.haplotypes) opt.haplotypes = va.haplotypes;
    if (!(va.min_allele_frac > 0 && va.min_allele_frac <= 1) || va.min_allele_count < 1)
      throw mc::Error("mcl_assign_variants: min_allele_frac is above 0 and at most 1, min_allele_count 1 or more", 1);
    opt.min_allele_frac = va.min_allele_frac;
    opt.min_allele_count = (uint64_t)va.min_allele_count;
    if (va.chimeras) opt.chimeras = va.chimeras;
    if (va.min_chimera_gain < 1) throw mc::Error("mcl_assign_chimeras: min_chimera_gain is 1 or more", 1);
    opt.min_chimera_gain = va.min_chimera_gain;
    opt.quality = quality;
    opt.band = band;
    if (msa) opt.msa = msa;
    if (profile) opt.profile = profile;
    if (paf) opt.paf = paf;
    if (consensus) opt.consensus = consensus;
    if (pileup) opt.pileup = pileup;
    opt.both_strands = both_strands;
    opt.top = top;
    if (hits) opt.hits = hits;
    if (top < 0 || top > MC_ASSIGN_MAX_TOP || (top > 0) != !opt.hits.empty())
      throw mc::Error("mcl_assign_top: top (1 .. MC_ASSIGN_MAX_TOP) and hits are given together", 1);
    if (!(min_identity <= 1)) throw mc::Error("mcl_assign_identity: min_identity is 0 .. 1 (negative: off)", 1);
    opt.min_identity = min_identity < 0 ? -1 : min_identity;
    opt.identity = identity != 0 || min_identity >= 0 || !opt.paf.empty() || !opt.consensus.empty() || !opt.pileup.empty() || !opt.msa.empty() || !opt.profile.empty() || opt.any_variants() || !opt.chimeras.empty();
    opt.model = model ? model : "";
    opt.centres = centres ? centres : "";
    for (int i = 0; i < nreads; i++) opt.reads.push_back(reads[i]);
    opt.threads = threads;
    if (tsv) opt.output = tsv;
    if (unassigned) opt.unassigned = unassigned;
    opt.quiet = true;
    if (opt.model.empty() || opt.centres.empty() || opt.reads.empty()) throw mc::Error("mcl_assign: model, centres and reads are required", 1);
    if (quality && opt.consensus.empty() && opt.pileup.empty() && opt.profile.empty() && !opt.any_variants())
      throw mc::Error("mcl_assign_qconsensus: quality needs consensus and/or pileup (or profile)", 1);
    if (!opt.chimeras.empty() && top < 2) throw mc::Error("mcl_assign_chimeras: chimeras needs top of 2 or more (and hits)", 1);
    if (band && opt.paf.empty() && opt.consensus.empty() && opt.pileup.empty() && opt.msa.empty() && opt.profile.empty() && !opt.any_variants() &&
        opt.chimeras.empty())
      throw mc::Error("mcl_assign_band: band needs paf, consensus, pileup, msa or profile", 1);
    const mc::AssignResult r = mc::run_assign(ctx, opt);
    if (stats && cap > 0) snprintf(stats, cap, "%s", mc::assign_stats_json(r).c_str());
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

int mcl_assign(mc_ctx *ctx, const char *model, const char *centres, const char *const *reads, int nreads, int threads,
               const char *tsv, const char *unassigned, char *stats, int cap) {
  return assign_entry(ctx, model, centres, reads, nreads, threads, tsv, unassigned, false, 0, nullptr, 0, -1.0, nullptr, nullptr, nullptr, false, nullptr, nullptr, false, stats, cap);
}

// mcl_assign with meshclust-assign's --both-strands when both_strands is non-zero (mc_assign_strands
// on both strands): the TSV gains the strand column, the summary "strands" and "assigned_minus".
// Where only the pair list applies it returns 2 with the reason in stats.
int mcl_assign_strands(mc_ctx *ctx, const char *model, const char *centres, const char *const *reads, int nreads,
                       int threads, const char *tsv, const char *unassigned, int both_strands, char *stats, int cap) {
  return assign_entry(ctx, model, centres, reads, nreads, threads, tsv, unassigned, both_strands != 0, 0, nullptr, 0, -1.0, nullptr, nullptr, nullptr, false, nullptr, nullptr, false, stats, cap);
}

// mcl_assign_strands with meshclust-assign's --top `top` --hits `hits` (mc_assign_top): the TSV is
// unchanged, `hits` gets one line per hit of the `top` best similar centres of every read, the
// summary gains "top" and "hits".  top = 0 with hits NULL is mcl_assign_strands.
int mcl_assign_top(mc_ctx *ctx, const char *model, const char *centres, const char *const *reads, int nreads, int threads,
                   const char *tsv, const char *unassigned, int both_strands, int top, const char *hits, char *stats,
                   int cap) {
  return assign_entry(ctx, model, centres, reads, nreads, threads, tsv, unassigned, both_strands != 0, top, hits, 0, -1.0, nullptr, nullptr,
                      nullptr, false, nullptr, nullptr, false, stats, cap);
}

// mcl_assign_top with meshclust-assign's --identity (identity non-zero) and --min-identity
// (min_identity in 0 .. 1, which implies identity; negative: off): the TSV and the hits file gain
// the identity column, the summary "identity_pairs", "identity_cells", "rejected" and the
// "identity" phase.  identity = 0 with a negative min_identity is mcl_assign_top.
int mcl_assign_identity(mc_ctx *ctx, const char *model, const char *centres, const char *const *reads, int nreads, int threads,
                        const char *tsv, const char *unassigned, int both_strands, int top, const char *hits, int identity,
                        double min_identity, char *stats, int cap) {
  return assign_entry(ctx, model, centres, reads, nreads, threads, tsv, unassigned, both_strands != 0, top, hits, identity,
                      min_identity, nullptr, nullptr, nullptr, false, nullptr, nullptr, false, stats, cap);
}

// mcl_assign_identity with meshclust-assign's --paf `paf` (mc_nw_align_strands; implies identity):
// `paf` gets one PAF line with a CIGAR per aligned pair, the summary gains "paf_pairs" and
// "cigar_ops".  paf NULL is mcl_assign_identity.
int mcl_assign_paf(mc_ctx *ctx, const char *model, const char *centres, const char *const *reads, int nreads, int threads,
                   const char *tsv, const char *unassigned, int both_strands, int top, const char *hits, int identity,
                   double min_identity, const char *paf, char *stats, int cap) {
  return assign_entry(ctx, model, centres, reads, nreads, threads, tsv, unassigned, both_strands != 0, top, hits, identity,
                      min_identity, paf, nullptr, nullptr, false, nullptr, nullptr, false, stats, cap);
}

// mcl_assign_paf with meshclust-assign's --consensus `consensus` and --pileup `pileup`
// (mc_nw_pileup_strands; either implies identity, either may be NULL): the consensus FASTA of every
// centre and the per-column counts of the centres with reads; the summary gains "consensus_pairs",
// "consensus_centres", "consensus_passes", "realigned_centres" and "insertion_sites".  Both NULL is
// mcl_assign_paf.
int mcl_assign_consensus(mc_ctx *ctx, const char *model, const char *centres, const char *const *reads, int nreads, int threads,
                         const char *tsv, const char *unassigned, int both_strands, int top, const char *hits, int identity,
                         double min_identity, const char *paf, const char *consensus, const char *pileup, char *stats, int cap) {
  return assign_entry(ctx, model, centres, reads, nreads, threads, tsv, unassigned, both_strands != 0, top, hits, identity,
                      min_identity, paf, consensus, pileup, false, nullptr, nullptr, false, stats, cap);
}

// mcl_assign_consensus with meshclust-assign's --quality when quality is non-zero (mc_load_qualities,
// mc_nw_qpileup_strands): it needs consensus and/or pileup and FASTQ reads; the consensus is written
// as FASTQ with a quality per base, the pile-up rows gain the six weights, the summary "quality": 1.
// quality = 0 is mcl_assign_consensus.
int mcl_assign_qconsensus(mc_ctx *ctx, const char *model, const char *centres, const char *const *reads, int nreads, int threads,
                          const char *tsv, const char *unassigned, int both_strands, int top, const char *hits, int identity,
                          double min_identity, const char *paf, const char *consensus, const char *pileup, int quality,
                          char *stats, int cap) {
  return assign_entry(ctx, model, centres, reads, nreads, threads, tsv, unassigned, both_strands != 0, top, hits, identity,
                      min_identity, paf, consensus, pileup, quality != 0, nullptr, nullptr, false, stats, cap);
}

// mcl_assign_qconsensus with meshclust-assign's --msa `msa` (mc_nw_msa_begin / mc_nw_msa_rows; implies
// identity): `msa` gets the assigned reads of every centre laid out in common columns as aligned
// FASTA, the summary gains, after every other key, "msa_pairs", "msa_centres", "msa_columns",
// "msa_bytes" and the "msa" phase.  msa NULL is mcl_assign_qconsensus.
int mcl_assign_msa(mc_ctx *ctx, const char *model, const char *centres, const char *const *reads, int nreads, int threads,
                   const char *tsv, const char *unassigned, int both_strands, int top, const char *hits, int identity,
                   double min_identity, const char *paf, const char *consensus, const char *pileup, int quality, const char *msa,
                   char *stats, int cap) {
  return assign_entry(ctx, model, centres, reads, nreads, threads, tsv, unassigned, both_strands != 0, top, hits, identity,
                      min_identity, paf, consensus, pileup, quality != 0, msa, nullptr, false, stats, cap);
}

// mcl_assign_msa with meshclust-assign's --profile `profile` (mc_nw_msa_counts over the plan --msa
// uses; implies identity): `profile` gets one TSV line per column of every centre that has a read,
// with quality six weights more per line (quality is then accepted beside profile alone); the summary
// gains, after every other key, "profile_centres", "profile_columns" and the "profile" phase.
// profile NULL is mcl_assign_msa.
int mcl_assign_profile(mc_ctx *ctx, const char *model, const char *centres, const char *const *reads, int nreads, int threads,
                       const char *tsv, const char *unassigned, int both_strands, int top, const char *hits, int identity,
                       double min_identity, const char *paf, const char *consensus, const char *pileup, int quality, const char *msa,
                       const char *profile, char *stats, int cap) {
  return assign_entry(ctx, model, centres, reads, nreads, threads, tsv, unassigned, both_strands != 0, top, hits, identity,
                      min_identity, paf, consensus, pileup, quality != 0, msa, profile, false, stats, cap);
}

// mcl_assign_profile with meshclust-assign's --band when band is non-zero (mc_set_align_band 1 for the run, 0
// again at its end): it needs paf, consensus, pileup, msa or profile; every alignment records the certified
// band alone, no output file changes, the summary gains, after every other key, "band_pairs", "band_full",
// "band_launches" and "band_w_sum".  band = 0 is mcl_assign_profile.
int mcl_assign_band(mc_ctx *ctx, const char *model, const char *centres, const char *const *reads, int nreads, int threads,
                    const char *tsv, const char *unassigned, int both_strands, int top, const char *hits, int identity,
                    double min_identity, const char *paf, const char *consensus, const char *pileup, int quality, const char *msa,
                    const char *profile, int band, char *stats, int cap) {
  return assign_entry(ctx, model, centres, reads, nreads, threads, tsv, unassigned, both_strands != 0, top, hits, identity,
                      min_identity, paf, consensus, pileup, quality != 0, msa, profile, band != 0, stats, cap);
}

// mcl_assign_band with meshclust-assign's --variants `variants`, --alleles `alleles` and --haplotypes `haplotypes`
// (mc_nw_msa_counts, variants.hpp and mc_nw_msa_sites over the plan --msa and --profile use; each implies identity,
// each may be NULL) at --min-allele-frac `min_allele_frac` (above 0, at most 1) and --min-allele-count
// `min_allele_count` (1 or more): the profile lines of every centre's variant sites, every assigned read's
// characters there, and the distinct allele strings per centre; quality and band are then accepted beside any
// of the three.  The summary gains, after every other key, "variant_centres", "variant_sites", "allele_bytes"
// and the "variants" phase.  All three NULL (at any valid thresholds; the defaults are 0.2 and 2) is mcl_assign_band.
int mcl_assign_variants(mc_ctx *ctx, const char *model, const char *centres, const char *const *reads, int nreads, int threads,
                        const char *tsv, const char *unassigned, int both_strands, int top, const char *hits, int identity,
                        double min_identity, const char *paf, const char *consensus, const char *pileup, int quality, const char *msa,
                        const char *profile, int band, const char *variants, const char *alleles, const char *haplotypes,
                        double min_allele_frac, long long min_allele_count, char *stats, int cap) {
  VariantArgs va;
  va.variants = variants;
  va.alleles = alleles;
  va.haplotypes = haplotypes;
  va.min_allele_frac = min_allele_frac;
  va.min_allele_count = min_allele_count;
  return assign_entry(ctx, model, centres, reads, nreads, threads, tsv, unassigned, both_strands != 0, top, hits, identity,
                      min_identity, paf, consensus, pileup, quality != 0, msa, profile, band != 0, stats, cap, va);
}

// mcl_assign_variants with meshclust-assign's --chimeras `chimeras` (mc_nw_msa_crossover and chimera.hpp over every
// read's hits, in plans of its own after every other output; needs top of 2 or more, implies identity, may be NULL)
// at --min-chimera-gain `min_chimera_gain` (1 or more): one line per read with a candidate second parent; band is
// then accepted beside it.  The summary gains, after every other key, "chimera_candidates", "chimeras" and the
// "chimeras" phase.  chimeras NULL (at any valid gain; the default is 3) is mcl_assign_variants.
int mcl_assign_chimeras(mc_ctx *ctx, const char *model, const char *centres, const char *const *reads, int nreads, int threads,
                        const char *tsv, const char *unassigned, int both_strands, int top, const char *hits, int identity,
                        double min_identity, const char *paf, const char *consensus, const char *pileup, int quality, const char *msa,
                        const char *profile, int band, const char *variants, const char *alleles, const char *haplotypes,
                        double min_allele_frac, long long min_allele_count, const char *chimeras, long long min_chimera_gain,
                        char *stats, int cap) {
  VariantArgs va;
  va.variants = variants;
  va.alleles = alleles;
  va.haplotypes = haplotypes;
  va.min_allele_frac = min_allele_frac;
  va.min_allele_count = min_allele_count;
  va.chimeras = chimeras;
  va.min_chimera_gain = min_chimera_gain;
  return assign_entry(ctx, model, centres, reads, nreads, threads, tsv, unassigned, both_strands != 0, top, hits, identity,
                      min_identity, paf, consensus, pileup, quality != 0, msa, profile, band != 0, stats, cap, va);
}

// Records ids[0..n) of a parsed dataset (mcl_parse) as FASTA: header lines unchanged, each
// sequence upper-cased on one line.  Returns 0, or 1 with the message in err.
int mcl_write_fasta(void *dsv, const uint32_t *ids, uint64_t n, const char *path, char *err, int errcap) {
  try {
    mc::write_fasta(path, *(const mc::Dataset *)dsv, ids, n);
    return 0;
  } catch (const std::exception &e) {
    if (err && errcap > 0) snprintf(err, errcap, "%s", e.what());
    return 1;
  }
}
}
