// assign.hpp -- bin/meshclust-assign: place reads into an existing clustering (the model and
// centres files bin/meshclust saves, model.hpp) with mc_assign on the GPU.
#pragma once
#include <string>
#include <vector>

#include "common.hpp"

namespace mc {

struct AssignOptions {
  std::string model, centres, output = "assign.tsv", unassigned, stats_json;
  std::vector<std::string> reads;  // in the order given
  int device = 0;
  int threads = 0;  // 0 = OpenMP default
  bool quiet = false;
  bool both_strands = false;  // --both-strands: score every read as written and reverse-complemented
  int top = 0;                // --top K (1..MC_ASSIGN_MAX_TOP) with --hits FILE: the K best centres per read
  std::string hits;
  bool identity = false;      // --identity: align every reported (read, centre, strand), report the identity
  double min_identity = -1;   // --min-identity X (0..1, implies identity; negative: off): verify.hpp
  std::string paf;            // --paf FILE (implies identity): the alignments of the reported pairs as PAF
  std::string consensus;      // --consensus FILE (implies identity): a consensus per centre from its assigned reads, FASTA
  std::string pileup;         // --pileup FILE (implies the consensus pass): the per-column counts behind it, TSV
  bool quality = false;       // --quality (with consensus and/or pileup; FASTQ reads): the pile-up weighed by base quality
  std::string msa;            // --msa FILE (implies identity): every centre's reads laid out in common columns, aligned FASTA
  std::string profile;        // --profile FILE (implies identity): the column profile of every centre's alignment, TSV
  bool band = false;          // --band (with paf, consensus, pileup, msa, profile or one of the three below): the certified band
  std::string variants;       // --variants FILE (implies identity): the profile's lines of every centre's variant sites, TSV
  std::string alleles;        // --alleles FILE (implies identity): every assigned read's characters at its centre's sites, TSV
  std::string haplotypes;     // --haplotypes FILE (implies identity): the distinct allele strings of every centre with sites, TSV
  double min_allele_frac = 0.2;    // --min-allele-frac X (0 < X <= 1) and --min-allele-count N (N >= 1): variants.hpp's rule
  uint64_t min_allele_count = 2;
  bool any_variants() const { return !variants.empty() || !alleles.empty() || !haplotypes.empty(); }
  std::string chimeras;       // --chimeras FILE (needs top >= 2, implies identity): every read's best second parent, TSV
  int64_t min_chimera_gain = 3;  // --min-chimera-gain N (N >= 1): chimera.hpp's flag; 3 is a convention, not tuned
};

struct AssignResult {
  uint64_t reads = 0, centres = 0, assigned = 0;
  uint64_t candidates = 0;  // pairs after the length gate
  uint64_t fallbacks = 0;   // mc_assign: pairs decided by the full scorer
  uint64_t device_us = 0;   // mc_assign: kernel time from HIP events
  int k = 0, width = 0;
  int strands = MC_STRAND_PLUS;  // MC_STRAND_PLUS, or both (3) with --both-strands
  uint64_t assigned_minus = 0;   // both strands: reads assigned on their reverse complement
  int top = 0;                   // --top: K, and the lines written to the hits file
  uint64_t hits = 0;
  bool identity = false;         // --identity / --min-identity: pairs aligned, their cells (sum of len1 * len2),
  uint64_t identity_pairs = 0, identity_cells = 0, rejected = 0;  // reads with a hit but none at >= X
  bool paf = false;              // --paf: lines written, operation words of their CIGARs
  uint64_t paf_pairs = 0, cigar_ops = 0;
  bool consensus = false;        // --consensus / --pileup: pairs piled up, centres with a read, alignment passes
  uint64_t consensus_pairs = 0, consensus_centres = 0;  // (1: the pile-up gave the identities too; 2: it came second),
  int consensus_passes = 0;                             // centres re-aligned for their inserted bases, sites applied
  uint64_t realigned_centres = 0, insertion_sites = 0;
  bool quality = false;          // --quality: the qualities were uploaded and the weighted pile-up ran
  bool msa = false;              // --msa: pairs laid out, centres with a read, the sum of their widths, bytes of all rows
  uint64_t msa_pairs = 0, msa_centres = 0, msa_columns = 0, msa_bytes = 0;
  bool profile = false;          // --profile: centres with a read, the columns written
  uint64_t profile_centres = 0, profile_columns = 0;
  bool band = false;             // --band: pairs planned banded and full, search launches, the sum of the planned widths
  uint64_t band_pairs = 0, band_full = 0, band_launches = 0, band_w_sum = 0;
  bool variants = false;         // --variants / --alleles / --haplotypes: centres with a site, their sites, bytes of mc_nw_msa_sites
  uint64_t variant_centres = 0, variant_sites = 0, allele_bytes = 0;
  bool chimeras = false;         // --chimeras: reads with a second-parent candidate (lines written), those flagged Y
  uint64_t chimera_candidates = 0, chimera_flagged = 0;
  std::string path;  // "device" (mc_assign) or "pairs" (mc_classify_pairs batches)
  double parse_ms = 0, upload_ms = 0, kmer_ms = 0, assign_ms = 0, identity_ms = 0, write_ms = 0, msa_ms = 0, profile_ms = 0, variants_ms = 0, chimeras_ms = 0;
};

// Throws mc::Error (bad options: code 1 with the usage text in what()).
AssignOptions parse_assign_options(int argc, char **argv);
// The whole job; writes the TSV (and the unassigned FASTA).  With both_strands the TSV has a sixth
// column (+, -, or * for an unassigned read); where only the pair list applies (MC_ASSIGN_PAIRS,
// wide bins or rows) both_strands throws an Error of code 2: the pair list has no permuted rows.  ctx NULL: a context on opt.device is
// opened once the model and the centres file are accepted, and closed at the end.
// A version-2 model (meshclust --both-strands, model.hpp: strands 3) implies both_strands: reads and
// centres get canonical rows (mc_kmer_max_strands / mc_kmer_build_strands), the plus strand set
// alone is scored (the rows are symmetric: a minus pass would list every hit twice), and the strand
// of every reported (read, centre) comes from mc_orient_pairs; everything after that runs as with
// both_strands.  There the pair list (MC_ASSIGN_PAIRS, rows too wide for the kernel) runs on the
// canonical rows too; an input that cannot have canonical rows (32/64-bit bins, k >= 8) throws an
// Error of code 2.  A version-1 model behaves as before.
// With top / hits (mc_assign_top; on the pair list the same ordered insertion on the host) the
// hits file gets one line per hit (read, rank, centre, cluster index, combo 0, and the strand
// with both_strands); the TSV is the one written without them.
// With identity (mc_nw_identity_strands, one call: every reported (read, centre, strand), the
// read reverse-complemented where the strand is minus) the TSV and the hits file gain a last
// column, the identity as %.17g or * for an unassigned read.  With min_identity >= 0 a read goes
// to the first of its candidates (its hits; one without top) whose identity is at least that
// (verify.hpp), else it is unassigned; n_similar and the hits file do not change.
// With paf (implies identity) the same pairs go through mc_nw_align_strands instead, in chunks of
// at most 2^26 bases of both strings together; the identity columns are its ids / len (the same
// doubles), and the file gets one PAF line per aligned pair, reads in input order, ranks
// ascending: read, its length, 0, its length, strand, centre, its length, 0, its length, ids, len,
// 255, AS:i:score, rk:i:rank, cg:Z:CIGAR (cigar.hpp).  On '-' the CIGAR runs along the
// reverse-complemented read.  min_identity selects as without paf; the PAF lists every aligned pair.
// With consensus / pileup (mc_nw_pileup_strands; either implies identity) the pair (read, its final
// centre, its strand) of every assigned read -- after min_identity's selection -- is piled up per
// centre column.  consensus gets every centre in centres-file order as FASTA, ">NAME depth=D sub=S
// del=X ins=I" and the consensus of consensus.hpp (a centre without reads: its own sequence); pileup
// gets, for centres with a read, one line per row: centre, column from 1 (L + 1 with base *), centre
// base, depth, A, C, G, T, N, del, ins_reads, ins_bases.  With no top, min_identity or paf the
// pile-up is the only alignment pass and the identity column is its ids / len (the same doubles);
// otherwise it is a second pass over the selected pairs ("consensus_passes" 1 or 2 in the stats).
// Centres with an insertion site are re-aligned with mc_nw_align_strands for the inserted bases
// ("realigned_centres").
// Reads and centres may be FASTA or FASTQ files (fasta.hpp); the qualities are skipped unless
// quality is set, which needs consensus, pileup or profile (parse_assign_options: usage error) and every
// reads file to be FASTQ (Error of code 2 naming the file).  The qualities are then uploaded
// (mc_load_qualities), the pile-up pass goes through mc_nw_qpileup_strands, consensus is written as
// FASTQ ("@NAME depth=D sub=S del=X ins=I", sequence, "+", a quality per base; consensus.hpp
// qconsensus_of; a centre without reads: its own sequence at '!'), every pileup row gains the six
// weights wA wC wG wT wN wdel, and the stats "quality": 1.
// With msa (implies identity; a pass of its own after every other, which changes none of their
// outputs) the pairs consensus takes -- (read, final centre, strand) of every assigned read -- are
// sorted by centre and go through one mc_nw_msa_begin; the rows are streamed to the file in chunks
// of at most 64 MiB.  The file is aligned FASTA, one block per centre that has a read, in
// centres-file order: ">CENTRE depth=D width=W" and the centre's row, then per read in input order
// ">READ strand=+" (or -) and its row; every row of a block is W characters, gaps '-'.  The stats
// gain, after every other key, "msa_pairs", "msa_centres", "msa_columns" (the sum of W) and
// "msa_bytes" (the sum of rows * W), and the phases "msa".
// With profile (implies identity; it shares msa's mc_nw_msa_begin when both are given and changes no
// other output) the same plan is counted per column by mc_nw_msa_counts, read in ranges of targets
// of at most 64 MiB.  The file is a TSV, for centres with a read, in centres-file order, one line per
// column: centre, column (from 1), centre_pos, slot, base, depth, A, C, G, T, N, gap.  A centre's own
// column has centre_pos r + 1, slot 0 and the centre's character; an inserted column has the site
// r + 1 (L + 1 after the last base), slot t + 1 and base '-'.  With quality (then also accepted
// beside profile alone) every line gains wA wC wG wT wN wgap.  The stats gain, after every other
// key, "profile_centres" and "profile_columns", and the phases "profile".
// With variants, alleles or haplotypes (each implies identity; they share msa's and profile's mc_nw_msa_begin and
// change no other output) every centre's profile goes through variant_sites (variants.hpp) at min_allele_frac and
// min_allele_count, whichever of the three files is asked for.  variants gets, for every centre with reads, the
// lines profile would write for its site columns and no others, byte for byte (six weights more with quality,
// which is then accepted beside any of the three).  alleles gets one line per assigned read, centres in
// centres-file order and their reads in input order: read, centre, strand (+ or -), and the read's characters at
// its centre's sites (mc_nw_msa_sites, read in ranges of pairs whose bytes stay within 32 MiB), "." for a centre
// without sites; with quality a fifth column, the weights as Phred+33.  haplotypes gets, per centre with a site,
// one line per distinct allele string seen min_allele_count times or more, by count descending and then by
// bytes: centre, rank (from 1), count, depth, alleles.  The stats gain, after every other key, "variant_centres"
// (centres with a site), "variant_sites" and "allele_bytes" (the bytes mc_nw_msa_sites returned), and the phases
// "variants".
// With chimeras (it needs top >= 2: parse_assign_options, usage error; implies identity; changes no other output) a
// phase of its own runs after every other user of mc_nw_msa_begin's plan, because its begins drop theirs.  The reads
// with a candidate second parent (chimera.hpp: a hit after the first whose centre differs from the first hit's) go in
// input order in ranges whose pairs stay within 2^18 (a read's pairs together); a range's pairs are those reads'
// first hit and candidate hits on the hits' strands, its targets the centres among them, through one
// mc_nw_msa_begin and one mc_nw_msa_crossover of (first hit, candidate) per candidate.  chimeras gets one line per
// such read: read, left_centre, right_centre, left_strand, right_strand (+ or -), cut_first, cut_last (0-based
// positions in the read as written: the right parent starts there), ids_left, ids_right (the single parents'
// identities), best, gain, read_len, flag (Y where gain >= min_chimera_gain, else N) for the candidate chimera_pick
// chooses.  The stats gain, after every other key, "chimera_candidates" (the lines) and "chimeras" (those flagged
// Y), and the phases "chimeras".
// With band (it needs paf, consensus, pileup, msa, profile, variants, alleles, haplotypes or chimeras: parse_assign_options, usage error) the context is
// set to mc_set_align_band 1 for the run and back to 0 at its end: every alignment pass plans a width per pair
// and records the certified band alone.  No output file changes.  The stats gain, after every other key,
// "band_pairs", "band_full", "band_launches" and "band_w_sum" (mc_nw_band_profile over the run).
AssignResult run_assign(mc_ctx *ctx, const AssignOptions &opt);
std::string assign_stats_json(const AssignResult &r);
int assign_main(int argc, char **argv);

}  // namespace mc
