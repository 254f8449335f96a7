/*
 * meshclust_amd.h -- C-ABI of libmcgpu, the MI355X (gfx950) engine for MeShClust's
 * data-parallel hot path.  Plain pointers and sizes only; no C++ or torch types.
 *
 * MeShClust v1 has no plugin/FFI API: its hot path is reached through C++ template
 * seams inside one binary.  Each entry point below replaces one of those
 * seams; the reference interface it stands in for is cited as file:line relative to the
 * reference tree (src/...).  The host program (bin/meshclust, meshclust_amd/csrc/host)
 * restates the reference control flow and calls only these functions for the hot path.
 *
 * Conventions
 *   - every function returns MC_OK (0) or an MC_ERR_* code; mc_last_error() gives text.
 *     Nothing throws across the ABI.  Errors are loud: there is no CPU fallback.
 *   - point ids are the reference's ids: input order over all files (Runner.cpp:345-349).
 *   - one host thread per context; calls are synchronous at the ABI (HIP streams inside).
 *   - the caller owns every host array; the library owns device memory.
 */
#ifndef MESHCLUST_AMD_H
#define MESHCLUST_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MC_ABI_VERSION 1

#define MC_OK 0
#define MC_ERR_ARG 1     /* bad argument / shape                                  */
#define MC_ERR_HIP 2     /* HIP runtime or kernel failure                         */
#define MC_ERR_STATE 3   /* call made in the wrong order (e.g. no sequences yet)  */
#define MC_ERR_OOM 4     /* device allocation failed                              */
#define MC_ERR_INPUT 5   /* input the reference would reject (bad nucleotide ...) */
#define MC_ERR_UNSUPPORTED 6 /* this device path cannot take the request; use the step API  */
#define MC_ERR_TIMEOUT 7 /* a persistent kernel's hand-off deadline expired (a peer never answered) */

/* Feature flags and combo kinds: identical values to src/cluster/src/Feature.h:9-22. */
#define MC_FEAT_ALIGN (1 << 0)
#define MC_FEAT_LD (1 << 1)
#define MC_FEAT_MANHATTAN (1 << 2)
#define MC_FEAT_INTERSECTION (1 << 4)
#define MC_FEAT_PEARSON (1 << 5)
#define MC_FEAT_KULCZYNSKI2 (1 << 10)
#define MC_COMBO_SQUARED 1
#define MC_COMBO_SELF 2

#define MC_MAX_SINGLE 8
#define MC_MAX_COMBO 8
#define MC_MAX_COMBO_LEN 4

/*
 * Trained classifier = Feature<T> state after normalize()/finalize() plus the GLM weight
 * column (Feature.h:122-130, Trainer.h:45-46).  `lookup` is the single-feature order,
 * `combo_*` the products of Feature::operator() (Feature.h:69-88), `weights[0]` the
 * intercept and `weights[1+c]` the weight of combo c (Trainer.cpp:84-95).
 */
typedef struct mc_classifier {
  int32_t n_single;
  uint16_t lookup[MC_MAX_SINGLE];
  int32_t is_sim[MC_MAX_SINGLE];
  double mins[MC_MAX_SINGLE];
  double maxs[MC_MAX_SINGLE];
  int32_t n_combo;
  int32_t combo_kind[MC_MAX_COMBO];
  int32_t combo_len[MC_MAX_COMBO];
  int32_t combo_idx[MC_MAX_COMBO][MC_MAX_COMBO_LEN];
  double weights[MC_MAX_COMBO + 1];
} mc_classifier;

/* Result of one accumulation step (Trainer::get_close + ClusterFactory get_mean). */
typedef struct mc_scan_result {
  int32_t is_min;       /* get_close's is_min_r: no candidate classified similar      */
  int32_t has_best;     /* get<0>(result) != NULL (some combo-0 value > -1)            */
  uint64_t best_pos;    /* static position of the first maximum of combo 0            */
  double best_val;      /* that maximum                                                */
  uint64_t n_flagged;   /* candidates marked similar (removed from the window)         */
  uint32_t new_centre;  /* get_mean's argmin distance_d over the cluster (if !is_min)  */
  uint32_t n_members;   /* cluster size after this step                                */
  uint64_t nw_pairs;    /* alignment mode: NW alignments run for this step (else 0)    */
  uint64_t nw_cells;    /* alignment mode: their DP cells, sum of len1 * len2          */
} mc_scan_result;

typedef struct mc_ctx mc_ctx;

const char *mc_last_error(void);
int mc_abi_version(void);

/* Context on one GPU (hipSetDevice(device)); one process per GPU. */
int mc_ctx_create(int device, mc_ctx **out);
int mc_ctx_destroy(mc_ctx *ctx);

/*
 * Upload the encoded sequences.  codes: concatenation of every sequence's one-digit
 * string as ChromosomeOneDigit leaves it (0..3 inside segments, 'N' or the raw upper-case
 * byte outside; ChromosomeOneDigit.cpp:95-144).  seq_off[n+1] byte offsets.  seg: int32
 * pairs [start,end] (inclusive) per segment (Chromosome.cpp:162-258), seg_off[n+1] pair
 * offsets.  Replaces the Chromosome objects consumed by fill_table (ClusterFactory.h:40-55)
 * and by GlobAlignE through Point::get_data_str (Trainer.cpp:18-27).
 */
int mc_load_sequences(mc_ctx *ctx, const uint8_t *codes, const uint64_t *seq_off, uint64_t n,
                      const int32_t *seg, const uint64_t *seg_off);

/*
 * The same sequences in the form the host parser produces (meshclust_amd/csrc/host/fasta.cpp):
 * 2-bit codes, 16 bases per 32-bit word (base j of a record at bits 2*(j % 16) of word
 * pk_off[i] + j / 16; pk_off[i+1] - pk_off[i] = ceil(length_i / 16)), plus the nexc bytes that
 * are not 0..3 (the 'N' ChromosomeOneDigit leaves outside segments, ChromosomeOneDigit.cpp:
 * 122-144, or the raw bytes of a record without segments) at ascending global byte positions
 * exc_pos.  seq_off/seg/seg_off as for mc_load_sequences.  A quarter of the bytes cross PCIe;
 * the device keeps both the packed form (K1 input) and the expanded bytes (NW input).
 */
int mc_load_packed(mc_ctx *ctx, const uint32_t *packed, const uint64_t *pk_off, const uint64_t *seq_off, uint64_t n,
                   const uint64_t *exc_pos, const uint8_t *exc_val, uint64_t nexc, const int32_t *seg,
                   const uint64_t *seg_off);

/*
 * Largest k-mer count of the pseudocount-1 uint64 tables (Runner.cpp:57-67).  The pass also
 * writes the 8-bit histograms, so when the count fits 8 bits the following
 * mc_kmer_build(ctx, k, 1) costs nothing (K1 reads the sequences once).  1 <= k <= 12.
 */
int mc_kmer_max(mc_ctx *ctx, int k, uint64_t *largest);

/*
 * Device-resident histograms, pseudocount 1, of width 1/2/4/8 bytes, plus their
 * magnitudes (DivergencePoint mag incl. pseudocounts).  Replaces
 * ClusterFactory::get_divergence_point (ClusterFactory.cpp:989-1010) + KmerHashTable
 * wholesaleIncrement (KmerHashTable.cpp:193-223).
 */
int mc_kmer_build(mc_ctx *ctx, int k, int width_bytes);

/* Copy histograms (n * 4^k * width bytes, id order) and magnitudes to the host. */
int mc_get_histograms(mc_ctx *ctx, void *hist, uint64_t *mags);

/*
 * keys[p * m + i] = points[ids[i]]->distance(*points[pivots[p]])
 * (DivergencePoint::distance, DivergencePoint.cpp:68-81; used by Trainer::split's sort
 * comparators, Trainer.cpp:681-701).  Keys are <= 10000.
 */
int mc_distance_keys(mc_ctx *ctx, const uint32_t *pivots, uint32_t npiv, const uint32_t *ids,
                     uint64_t m, uint16_t *keys);

/*
 * Trainer::split's per-pivot sorts on the device (Trainer.cpp:691-701: std::sort of the
 * points by distance to each pivot, then reads of ~35 positions of each sorted array by the
 * alignment binary search, :703-721, and the sampler, :732-755).
 *   mc_split_begin: for pivot p, the array std::sort is called on is (key << 32 | id) over
 *     `order` (keys as mc_distance_keys); it stays in HBM.
 *   mc_split_select: ids[i] = the id std::sort (libstdc++ introsort, ties included) puts at
 *     position pos[i] of pivot arr[i]'s array; only the ranges holding the queried positions
 *     are partitioned, and the partitions persist for later calls.
 *   mc_split_begin_words / mc_split_select_words: the same on arbitrary word arrays compared
 *     by their upper 32 bits (depth < 0: std::sort's 2 floor(log2 n) limit), returning words.
 *   mc_split_end: ends the queries (the device buffers stay with the context for reuse).
 */
int mc_split_begin(mc_ctx *ctx, const uint32_t *pivots, uint32_t npiv, const uint32_t *order, uint64_t n);
int mc_split_begin_words(mc_ctx *ctx, const uint64_t *words, uint32_t narr, uint64_t n, int depth);
int mc_split_select(mc_ctx *ctx, uint64_t nq, const uint32_t *arr, const uint64_t *pos, uint32_t *ids);
int mc_split_select_words(mc_ctx *ctx, uint64_t nq, const uint32_t *arr, const uint64_t *pos, uint64_t *words);
int mc_split_end(mc_ctx *ctx);

/*
 * raw[i * nflag + f] = Feature<T>::raw(flags[f], *points[a[i]], *points[b[i]])
 * (Feature.cpp:117-160) for the k-mer features LD/MANHATTAN/INTERSECTION/PEARSON/
 * KULCZYNSKI2.  Used by Feature::normalize (Feature.cpp:86-114).
 */
int mc_pair_features(mc_ctx *ctx, const uint32_t *a, const uint32_t *b, uint64_t m,
                     const uint16_t *flags, int nflag, double *raw);

/* Install the trained classifier used by every classify/scan/mean-shift call. */
int mc_set_classifier(mc_ctx *ctx, const mc_classifier *cls);

/*
 * For each pair i: cache = feat->compute(*points[a[i]], *points[b[i]]); sum = w0 + fma
 * chain over combos; similar = round(1/(1+exp(-sum))) == 1.  Replaces the per-pair body
 * of Trainer::merge (Trainer.cpp:129-157), filter (:334-349) and generate_feat_mat
 * (:367-414).  Any output pointer may be NULL.
 */
int mc_classify_pairs(mc_ctx *ctx, const uint32_t *a, const uint32_t *b, uint64_t m,
                      uint8_t *similar, double *combo0, double *sum);

/*
 * Assign queries to the centres of an existing clustering: all M x C pairs scored on the
 * device, the best similar centre kept per query.  Centres and queries are point ids of the
 * loaded sequences (histograms built, a k-mer classifier installed).  Pair (q, j) is a
 * candidate when sim <= 0, or when (uint64_t)(len_c * sim) <= len_q <= (uint64_t)(len_c / sim)
 * in double -- the window accumulate gives bvec::get_range (ClusterFactory.cpp:637-654), per
 * point.  A candidate is scored as feat->compute(query, centre), the candidate-first order of
 * Trainer::get_close (Trainer.cpp:34-114); decision and combo 0 are bit for bit what
 * mc_classify_pairs(query, centre) returns.
 *   best[q]       index j into centre_ids (not the id) of the largest combo 0 among the centres
 *                 classified similar, ties to the lowest j; MC_ASSIGN_NONE if none is similar
 *   best_val[q]   that combo 0, or -1.0
 *   n_similar[q]  how many centres are similar
 *   stats         (may be NULL, else 3 entries) {candidate pairs after the length gate, pairs
 *                 whose decision fell back from the short scorer to the full one, device time
 *                 in us from HIP events}
 * Any output pointer may be NULL.  M = 0 is MC_OK; C = 0 or an id >= n is MC_ERR_ARG.
 * MC_ERR_UNSUPPORTED: 32/64-bit histograms, a row that does not fit an LDS tile (k >= 8), an
 * alignment-mode classifier -- the caller then scores the pairs with mc_classify_pairs.
 * Environment, read per call: MC_ASSIGN_TILE=<centres per LDS tile>, MC_ASSIGN_FORM=general
 * (the 16-lanes-per-query kernel also where the lane-per-query one applies).
 */
#define MC_ASSIGN_NONE 0xffffffffu
int mc_assign(mc_ctx *ctx, const uint32_t *centre_ids, uint32_t C, const uint32_t *query_ids, uint64_t M,
              double sim, uint32_t *best, double *best_val, uint32_t *n_similar, uint64_t *stats);

/*
 * The histogram rows of the other strand.  With the k-mer index written first base most
 * significant (A 0, C 1, G 2, T 3), the reverse complement of k-mer i is rc(i): the k base-4
 * digits of i reversed, each digit d replaced by 3 - d.  rows[r][i] = hist[ids[r]][rc(i)] for the
 * m points ids, m * 4^k bins of the histograms' width, packed.  For a record whose segments are
 * all at least k long (every record of the FASTA parser: its segments are at least 20 bases)
 * this is exactly the histogram of the reverse-complemented record with its segments mirrored,
 * pseudocounts included; magnitude, sum of squares and length are those of the point itself.
 * THE MINUS STRAND IS DEFINED AS THIS PERMUTED ROW.  A caller of mc_load_sequences can hand in a
 * segment shorter than k; such a segment is hashed at its first position only, which is not
 * mirror-symmetric, so there the permuted row is not the histogram of the mirrored record.
 * MC_ERR_UNSUPPORTED: 32/64-bit histograms, a row that does not fit an LDS tile (k >= 8).
 */
int mc_revcomp_rows(mc_ctx *ctx, const uint32_t *ids, uint64_t m, void *rows /* m * 4^k * width */);

/*
 * mc_assign on either strand of the queries.  Every scorer input is a bin-wise sum and rc is an
 * involution, so score(rc(query), centre) == score(query, rc(centre)) bit for bit: the C centre
 * rows are permuted once per call (mc_revcomp_rows' kernel), not the M query rows.
 *   strands == MC_STRAND_PLUS    exactly mc_assign; strand[q] = 0
 *   strands == MC_STRAND_MINUS   what mc_assign returns for the reverse-complemented queries
 *                                (minus strand as defined above); strand[q] = 1
 *   strands == both (3)          per query the plus result (j+, v+, n+) and the minus result
 *                                (j-, v-, n-), each by mc_assign's own rule (largest combo 0, ties
 *                                to the lowest j).  Minus wins only if j- != MC_ASSIGN_NONE and
 *                                (j+ == MC_ASSIGN_NONE or v- > v+); a tie goes to plus.
 *                                strand[q] = 1 where minus wins, else 0 (0 when unassigned);
 *                                n_similar[q] = n+ + n-.
 * The length gate does not depend on the strand.  stats[0] stays the (query, centre) pairs after
 * the gate, stats[1] counts fall-backs per scored (pair, strand), stats[2] is device time
 * including the permutation kernel.  With both strands a tile entry holds two rows, so rows must
 * fit twice (k <= 6 at 16 bits, k <= 7 at 8 bits) and MC_ASSIGN_TILE's default roughly halves.
 * strands outside 1..3 is MC_ERR_ARG; otherwise errors are mc_assign's.
 */
#define MC_STRAND_PLUS 1
#define MC_STRAND_MINUS 2
int mc_assign_strands(mc_ctx *ctx, const uint32_t *centre_ids, uint32_t C, const uint32_t *query_ids, uint64_t M,
                      double sim, int strands /* 1, 2 or 3 */, uint32_t *best, double *best_val,
                      uint8_t *strand /* 0 plus, 1 minus; 0 when unassigned */, uint32_t *n_similar, uint64_t *stats);

/*
 * Strand-blind histograms: clustering reads whatever strand they were sequenced from.
 *
 * THE CANONICAL ROW of a point is canon[i] = row[i] + row[rc(i)] - 1, with row its pseudocount-1
 * forward histogram and rc the index map of mc_revcomp_rows (host/strand.hpp): the pseudocount-1
 * histogram of the record's k-mers counted on both strands.  It equals bit for bit the forward
 * histogram of the record r || N x 30 || rc(r) with its second segment mirrored.  Its magnitude
 * is 2 * mag - 4^k, its sum of squares is recomputed, the length stays the record's.  A record
 * and its reverse complement have equal canonical rows wherever every segment is at least k long
 * (every record of the parser; the exception is mc_revcomp_rows').  The largest canonical bin can
 * need 16 bits where the forward one fits 8 (A x 150 || T x 150 at k = 4: 148 forward, 295
 * canonical), so the width is chosen from the canonical maximum.
 *
 * mc_kmer_max_strands / mc_kmer_build_strands are mc_kmer_max / mc_kmer_build with a strand set:
 *   strands == MC_STRAND_PLUS   forwards to mc_kmer_max / mc_kmer_build: the same kernels, the
 *                               same results
 *   strands == 3 (both)         `largest` is the largest canonical bin; the build leaves the
 *                               canonical rows, their magnitudes and sums of squares as the
 *                               context's histograms (K1, then one out-of-place fold kernel), so
 *                               mc_get_histograms, mc_set_order, the scans, mean shift, mc_assign*
 *                               and mc_classify_pairs work on them unchanged; the forward rows are
 *                               kept in a second buffer for mc_orient_pairs.
 * The width contract is mc_kmer_build's: the caller passes a width that holds `largest`.  strands
 * outside {1, 3} is MC_ERR_ARG; with both strands 32/64-bit histograms and k >= 8 are
 * MC_ERR_UNSUPPORTED.  A later mc_kmer_max / mc_kmer_build returns the context to forward rows and
 * drops the second buffer.
 *
 * THE ORIENTATION OF A PAIR (a, b) is decided on the forward rows:
 *   sad_plus = sum |row_a[i] - row_b[i]|,  sad_minus = sum |row_a[i] - row_b[rc(i)]|
 * (exact integers); the strand is minus iff sad_minus < sad_plus, a tie is plus.
 * mc_orient_pairs writes strand[p] (0 plus, 1 minus) and, sad given, sad[2p] = sad_plus and
 * sad[2p + 1] = sad_minus for the m pairs.  Callers pass pairs grouped by b (many reads per
 * centre): a workgroup stages row_b and its permuted row once per run of equal b; the results do
 * not depend on the grouping.  MC_ERR_STATE unless the histograms were built with strands == 3;
 * an id >= n (or m >= 2^32) is MC_ERR_ARG; m = 0 is MC_OK.
 */
int mc_kmer_max_strands(mc_ctx *ctx, int k, int strands /* 1 or 3 */, uint64_t *largest);
int mc_kmer_build_strands(mc_ctx *ctx, int k, int width_bytes, int strands /* 1 or 3 */);
int mc_orient_pairs(mc_ctx *ctx, const uint32_t *a, const uint32_t *b, uint64_t m, uint8_t *strand /* m */,
                    uint64_t *sad /* 2m, may be NULL */);

/*
 * mc_assign_strands reporting the K best centres of every query instead of one.
 * A HIT of query q is a (centre index j, strand s) whose pair passes the length gate and is
 * classified similar: exactly the event that n_similar counts in mc_assign_strands.  With both
 * strands one centre can give two hits.  Row q of hit / hit_val / hit_strand (K entries each)
 * holds the first min(K, n_similar[q]) hits of q in THE ORDER
 *   1. combo 0 descending,
 *   2. then the plus strand (0) before the minus strand (1),
 *   3. then the centre index j ascending;
 * the remaining slots hold MC_ASSIGN_NONE, -1.0 and 0.  n_similar (not capped at K), stats, the
 * gate, the strand sets and MC_ERR_UNSUPPORTED are mc_assign_strands'.  K = 0 or
 * K > MC_ASSIGN_MAX_TOP is MC_ERR_ARG.  Any output pointer may be NULL.
 * Column 0 at any K, and so the whole result at K = 1, is mc_assign_strands' best / best_val /
 * strand: the largest value wins, a tie between strands goes to plus, a tie within a strand to
 * the lowest index.  (One difference: on MC_STRAND_MINUS alone mc_assign_strands reports strand 1
 * also for an unassigned query; here an empty slot's strand is 0.)
 * Where the lane-per-query kernel applies the list is kept in registers (capacity 2, 4 or 8, the
 * next one up from K); the 16-lanes-per-query kernel keeps it in the query's output row.
 */
#define MC_ASSIGN_MAX_TOP 8
int mc_assign_top(mc_ctx *ctx, const uint32_t *centre_ids, uint32_t C, const uint32_t *query_ids, uint64_t M,
                  double sim, int strands /* 1, 2 or 3 */, uint32_t K /* 1..MC_ASSIGN_MAX_TOP */,
                  uint32_t *hit /* M*K */, double *hit_val /* M*K */, uint8_t *hit_strand /* M*K */,
                  uint32_t *n_similar /* M */, uint64_t *stats /* 3 */);

/*
 * Batched utility::GlobAlignE(seqA,0,la-1,seqB,0,lb-1,1,-1,2,1).getIdentity() on the loaded
 * sequences (GlobAlignE.cpp:123-305; called by Trainer::align, Trainer.cpp:15-31, and
 * Feature::align, Feature.cpp:221-243).  len/ids may be NULL.
 */
int mc_nw_identity(mc_ctx *ctx, const uint32_t *a, const uint32_t *b, uint64_t m, double *ident,
                   int32_t *len, int32_t *ids);

/* The same on caller-provided byte strings (no loaded sequences needed). */
int mc_nw_identity_raw(mc_ctx *ctx, const uint8_t *a, const uint64_t *a_off, const uint8_t *b,
                       const uint64_t *b_off, uint64_t m, double *ident, int32_t *len,
                       int32_t *ids, int32_t *score);

/*
 * THE MINUS-STRAND STRING of a point is its expanded byte string (what mc_nw_identity reads: 0..3
 * inside segments, 'N' or the raw upper-case byte outside) reversed, every byte mapped: a digit
 * d <= 3 becomes 3 - d, 'A' <-> 'T' and 'C' <-> 'G' (the raw letters of a record without
 * segments), every other byte ('N' included) stays.  THE MINUS STRAND IS DEFINED AS THIS STRING,
 * as it is defined as the permuted row above.  For a record of A, C, G, T and N it is the string
 * the FASTA parser gives for the reverse-complemented record (the parser encodes every non-N byte
 * of a record that has a segment, and none of a record that has none).  The map is an
 * involution, so the minus strand of the minus strand is the string itself.
 * mc_revcomp_sequences: the minus-strand strings of the points ids, concatenated; off[m+1] byte
 * offsets into bytes (no padding at the ABI).  bytes may be NULL to get the offsets only.
 * No sequences loaded is MC_ERR_STATE, an id >= n MC_ERR_ARG.
 */
int mc_revcomp_sequences(mc_ctx *ctx, const uint32_t *ids, uint64_t m, uint8_t *bytes, uint64_t *off);

/*
 * mc_nw_identity with a strand per pair: pair i aligns seq1 = point a[i] as written
 * (a_minus[i] == 0) or its minus-strand string (a_minus[i] != 0) against seq2 = point b[i] as
 * written.  a_minus == NULL is all plus.  With no minus pair the results are mc_nw_identity's bit
 * for bit.  The read is the operand that is reverse-complemented, never the centre: GlobAlignE's
 * tie-breaks (M before X before Y, the first maximum) are not mirror-symmetric, so
 * identity(rc(a), b) need not be identity(a, rc(b)).
 * The pairs are worked in batches: per batch the distinct ids among its minus pairs are
 * reverse-complemented once on the device (a read with K hits once, not K times) into a buffer
 * the context owns, then one NW launch set runs for the minus pairs and one for the plus pairs,
 * every result going to its pair's own slot.  A batch ends at MC_IDENT_BATCH_PAIRS pairs or
 * before the read whose string would take the buffer past MC_IDENT_BATCH_BYTES (records padded
 * to 16 bytes; a single longer read still gets its own batch), so the scratch stays bounded for
 * any m.  Environment, read per call: MC_IDENT_BATCH=<pairs> lowers the pair cap and
 * MC_IDENT_BYTES=<bytes> the cap on the buffer of minus-strand strings (the latter also in
 * mc_revcomp_sequences, mc_nw_align_strands and the pile-ups, which share the buffer).  Batching
 * changes no result.  Errors are mc_nw_identity's: no sequences MC_ERR_STATE, an id >= n
 * MC_ERR_ARG, m = 0 MC_OK.  len/ids may be NULL.  The alignments are timed as "nw", the
 * reverse-complement kernel as "layout" (mc_timers).
 */
#define MC_IDENT_BATCH_PAIRS (1ull << 20)
#define MC_IDENT_BATCH_BYTES (256ull << 20)
int mc_nw_identity_strands(mc_ctx *ctx, const uint32_t *a, const uint32_t *b, const uint8_t *a_minus, uint64_t m,
                           double *ident, int32_t *len, int32_t *ids);

/*
 * The multiset q-gram intersection of mc_nw_identity_strands' pairs: common[i] = the sum over the
 * 4^q q-grams g of min(occurrences of g in seq1, occurrences of g in seq2), seq1 = point a[i] or
 * its minus-strand string (a_minus[i] != 0; NULL: all plus), seq2 = point b[i].  q is 1 .. 7.
 * common[i] is MC_QGRAM_NA where either string holds a byte outside 0..3 or is shorter than q.
 * An alignment with L columns, I of them identities, has C_q >= q * I - (q - 1) * (L + 1), so a
 * small count proves an identity below a cutoff without aligning (host/qscreen.hpp, DESIGN.md
 * 3.15).  One workgroup per pair, a 4^q-entry table of counters in LDS.  Errors are
 * mc_nw_identity's: no sequences MC_ERR_STATE, an id >= n or q out of range MC_ERR_ARG, m = 0
 * MC_OK; a read of 2^31 bases or more MC_ERR_UNSUPPORTED.  Timed as "pairs" (mc_timers).
 */
#define MC_QGRAM_NA 0xffffffffu
int mc_qgram_common(mc_ctx *ctx, const uint32_t *a, const uint32_t *b, const uint8_t *a_minus, uint64_t m, int q,
                    uint32_t *common);

/*
 * THE ALIGNMENT of a pair is the chain of predecessor choices along which GlobAlignE's (path
 * length, identities) payload reaches (la, lb): the reference keeps no path, but with its fixed
 * tie rules (M before X before Y into M, M before the gap into a gap, the first maximum of M, X, Y
 * at the end) that chain is one path, and its columns and '=' are the len and ids mc_nw_identity
 * reports.  mc_nw_align_strands returns it for the pairs of mc_nw_identity_strands (the same
 * operand rule: seq1 = point a[i], its minus-strand string where a_minus[i] != 0; seq2 = point
 * b[i] as written; the distinct minus reads of a batch reverse-complemented once).
 * Operations are words run << 4 | op with BAM's codes, in alignment order from the first column
 * to the last: '=' and 'X' consume a base of each (state M), 'I' a base of seq1 alone (state X,
 * lowerGap), 'D' a base of seq2 alone (state Y, upperGap).  Pair i's words are
 * cigar[cig_off[i] .. cig_off[i + 1]); cig_off (m + 1, required) always receives the prefix sums
 * of the counts.  cigar == NULL gives the offsets and score / len (columns) / ids ('=') only;
 * cigar != NULL with cap < cig_off[m] is MC_ERR_ARG with cig_off valid and nothing written to
 * cigar.  score, len and ids may be NULL.  An empty seq1 against lb bases is lb 'D' (and 0 words
 * for two empty strings); the score is mc_nw_identity_raw's.
 * Device: a forward pass records 4 bits per cell (a wavefront per pair, R = 4 / 8 / 16 rows per
 * lane for la <= 256 / <= 512 / longer), ceil(la / (64 R)) * (lb + 63) * 32 R bytes per pair; a
 * second kernel walks them back, a thread per pair, at most la + lb steps (a walk that has not
 * reached the matrix's edge by then: MC_ERR_HIP).  The pairs are worked in batches: a batch ends at
 * MC_ALIGN_BATCH_PAIRS pairs, before the pair that would take the choice words past
 * MC_ALIGN_SCRATCH_BYTES, or where mc_nw_identity_strands' buffer of minus-strand strings would
 * overflow; the context owns the scratch and reuses it.  A pair that alone needs more than the
 * cap is MC_ERR_UNSUPPORTED, checked before any launch, no output written.  Environment, read per
 * call: MC_ALIGN_BATCH=<pairs> and MC_ALIGN_SCRATCH=<bytes> lower the two caps, MC_IDENT_BYTES=<bytes>
 * that of the minus-strand strings.  Batching changes no result.  m = 0 is MC_OK, no sequences MC_ERR_STATE, an id >= n MC_ERR_ARG.  The forward and
 * traceback kernels are timed as "nw", the reverse-complement kernel as "layout" (mc_timers).
 * mc_nw_align_profile (a measurement aid): out[0], out[1] = device ms of the forward and of the
 * traceback (+ packing) kernels, out[2] = choice bytes the batches held, since the last reset.
 */
#define MC_CIGAR_I 1u   /* consumes seq1 (the read) only  : state X / lowerGap */
#define MC_CIGAR_D 2u   /* consumes seq2 (the centre) only: state Y / upperGap */
#define MC_CIGAR_EQ 7u
#define MC_CIGAR_X 8u   /* BAM's codes; word = run << 4 | op */
#define MC_ALIGN_BATCH_PAIRS (1ull << 16)
#define MC_ALIGN_SCRATCH_BYTES (1ull << 30)
int mc_nw_align_strands(mc_ctx *ctx, const uint32_t *a, const uint32_t *b, const uint8_t *a_minus, uint64_t m,
                        uint32_t *cigar, uint64_t cap, uint64_t *cig_off /* m + 1 */,
                        int32_t *score, int32_t *len, int32_t *ids);
int mc_nw_align_profile(mc_ctx *ctx, double *out /* 3 */, int reset);

/*
 * THE CERTIFIED BAND: a smaller choice record for the same alignments.  The forward pass above
 * records 4 bits for every cell of the la x lb matrix; the chain of a read against its centre stays
 * near the main diagonal.  With d = lb - la and a width w >= 0 the band is the cells with
 * min(0, d) - w <= j - i <= max(0, d) + w.  A path that leaves it holds at least 2 (w + 1) + |d| gap
 * columns in at least two runs and scores at most UB(w) = min(la, lb) - |d| - 3 (w + 1) - 4.  A banded
 * score S_w (every state outside the computed region at -2^30) is certified when
 *   (A) S_w > NINF + min(la, lb)   (no path from a finite "-infinity" boundary state reaches it), and
 *   (B) S_w > UB(w);
 * then S_w is the full score S, every optimal path lies in the band, and the chain of choices is
 * the full matrix's, choice for choice.  The width a pair needs is
 * w*(S) = max(0, floor((min(la, lb) - |d| - 4 - S) / 3)).
 * mc_set_align_band: mode 0 (the default) keeps the full record: every call is bit for bit and byte
 * for byte what it is without this entry, mc_nw_align_profile's choice bytes included.  Mode 1 makes
 * mc_nw_align_strands, mc_nw_pileup_strands, mc_nw_qpileup_strands and mc_nw_msa_begin plan a width
 * per pair first and record the band alone; their results do not change by a bit.  Any other mode
 * is MC_ERR_ARG.  The mode stays with the context.
 * The plan (mc_nw_band_plan is the search alone): the pairs go through a score-only form of the
 * banded forward kernel in mc_nw_identity_strands' batches (MC_IDENT_BATCH, MC_IDENT_BYTES).  Within
 * a batch every pair starts at w0 = 64 and the uncertified ones are launched again at twice the
 * width, until (A) and (B) hold or the band holds the whole matrix, at most 1 + ceil(log2(longest /
 * w0)) rounds; S is then exact and the planned width is w*(S), whatever w0 and the schedule were.
 * A pair is planned full (w = -1: the record and the forward kernel above) when (A) fails, when
 * either string is empty, or when the band at w* would take no fewer bytes than the full record.
 * Banded pairs are worked in row blocks of 256 (4 rows per lane); block k sweeps the columns its
 * rows' band cells lie in, and the record is ceil(la / 256) * (min(lb, 256 + |d| + 2 w) + 63) * 128
 * bytes.  The trace batches are planned on these bytes, and MC_ERR_UNSUPPORTED (a pair above
 * MC_ALIGN_SCRATCH) is decided on them, after the search and before any trace launch or output.
 * A walk that would leave its window is MC_ERR_HIP: the certificate says there is none.
 * Environment, read per call: MC_BAND_W0=<n> (n >= 1) replaces w0, for tests.
 * mc_nw_band_plan: w[i] = the planned width of pair i (-1: full), score[i] = S, mc_nw_identity_raw's
 * score.  Errors are mc_nw_identity_strands'; a pair of 2^27 bases or more is MC_ERR_UNSUPPORTED.
 * mc_nw_band_profile (a measurement aid): out[0] = pairs planned banded, out[1] = pairs planned
 * full, out[2] = search launches, out[3] = device ms of the search (timed as "nw"), out[4] = the sum
 * of the planned w over the banded pairs, since the last reset.
 */
int mc_set_align_band(mc_ctx *ctx, int mode /* 0 or 1 */);
int mc_nw_band_plan(mc_ctx *ctx, const uint32_t *a, const uint32_t *b, const uint8_t *a_minus, uint64_t m,
                    int32_t *w /* m */, int32_t *score /* m */);
int mc_nw_band_profile(mc_ctx *ctx, double *out /* 5 */, int reset);

/*
 * THE ALIGNMENTS of mc_nw_align_strands piled up per centre column.  The pairs, the operand rule
 * (seq1 = the read a[i], its minus-strand string where a_minus[i] != 0; seq2 = the centre b[i] as
 * written), the batching and its environment caps are mc_nw_align_strands' own; score, len and ids
 * (m each, may be NULL) are its results bit for bit.
 * targets: nt distinct point ids, the centres.  A target of L bytes owns L + 1 rows of
 * MC_PILEUP_CH counters, target t's rows being row_off[t] .. row_off[t + 1]; row_off (nt + 1,
 * required) receives the prefix sums of L + 1.  Walking a pair's alignment from its first column
 * with j centre bases consumed so far:
 *   '=' or 'X'   row j, channel x (the read's byte; x > 3, an N or a raw letter: channel 4); j++
 *   'D'          row j, channel 5; j++
 *   an 'I' run of n bases   row j, channel 6 += 1 (reads with an insertion before centre base j;
 *                row L: after the last base), channel 7 += n (inserted bases); j stays
 * The alignment is global, so in rows 0 .. L - 1 channels 0 .. 5 add up to the centre's number of
 * pairs, and row L has channels 0 .. 5 zero.  The counts are integers: the table does not depend
 * on the order of the pairs or on the batches.
 * table == NULL: the offsets only, nothing is aligned.  table != NULL with cap_rows < row_off[nt]:
 * MC_ERR_ARG, row_off valid, table untouched.  Otherwise the table is overwritten (not added to);
 * a target with no pair gets zero rows, m = 0 a zeroed table.  A duplicate target, an id >= n or a
 * b[i] that is not a target is MC_ERR_ARG; a pair that alone exceeds the scratch cap
 * MC_ERR_UNSUPPORTED; both are found before any launch and write nothing, row_off included.  No
 * sequences: MC_ERR_STATE.
 * Device: mc_nw_align_strands' forward and traceback kernels; then, instead of copying the
 * operation words out, a wavefront per pair adds them to a table the context keeps on the device
 * for the whole call -- two atomics per '=' or 'D' run on per-centre difference arrays, one per
 * mismatched column, two per 'I' run -- and one kernel per call turns the difference arrays into
 * counts.  32 bytes per centre base come back, once.  Environment, read per call:
 * MC_PILEUP_NAIVE=1 issues an atomic per column instead (a measurement aid; the same table).
 * Timers as mc_nw_align_strands, the pile-up kernels counting as "nw".  mc_nw_pileup_profile:
 * out[0 .. 2] = device ms of the forward, the traceback and the pile-up kernels since the last reset
 * (a reset also clears mc_nw_align_profile's two times).
 */
#define MC_PILEUP_CH 8
int mc_nw_pileup_strands(mc_ctx *ctx, const uint32_t *a, const uint32_t *b, const uint8_t *a_minus, uint64_t m,
                         const uint32_t *targets, uint32_t nt, uint64_t *row_off /* nt + 1, required */,
                         uint32_t *table /* row_off[nt] * MC_PILEUP_CH */, uint64_t cap_rows,
                         int32_t *score, int32_t *len, int32_t *ids /* m each, may be NULL */);
int mc_nw_pileup_profile(mc_ctx *ctx, double *out /* 3 */, int reset);

/*
 * THE PILE-UP WEIGHED BY BASE QUALITY.  mc_load_qualities: a Phred value (0 .. MC_QUAL_MAX, a FASTQ
 * byte - 33) per byte of the loaded sequences, qual[seq_off[i] + t] belonging to base t of point i
 * as written (points without qualities, the centres, hold 0).  bytes must equal the loaded
 * seq_off[n] and no value may exceed MC_QUAL_MAX (MC_ERR_ARG, the qualities loaded before stay);
 * no sequences: MC_ERR_STATE.  A later mc_load_sequences / mc_load_packed drops the qualities.
 * mc_nw_qpileup_strands: mc_nw_pileup_strands -- the pairs, the operand rule, the batching and its
 * environment caps, the errors, row_off, score / len / ids and the count table are that call's, bit
 * for bit -- with a second table of the same shape, wtable, that receives weights.  Qs(i), the
 * quality of base i of seq1 as aligned, is the read's quality at i on plus and at la - 1 - i on
 * minus.  Walking the alignment with i read bases and j centre bases consumed:
 *   '=' or 'X'   wtable row j, the channel of the read's byte += Qs(i); i++, j++
 *   a 'D' run of n   every one of its n rows, channel 5 += min(Qs(i - 1) if i > 0, Qs(i) if i < la)
 *                (0 if neither exists); j += n
 *   an 'I' run of n   row j, channel 6 += min Qs(i .. i + n - 1); i += n
 * Channel 7 is reserved and stays 0.  The weights are integer sums: wtable does not depend on the
 * order of the pairs or on the batches; with every quality 1 (and no empty read), wtable's
 * channels 0 .. 6 equal table's.
 * table and wtable both NULL: the offsets only.  Exactly one of them NULL: MC_ERR_ARG.  No
 * qualities loaded: MC_ERR_STATE.  Weights are uint32_t: a target that receives more than
 * (2^32 - 1) / MC_QUAL_MAX = 46,182,038 pairs is MC_ERR_ARG.  These are found before any launch and
 * write nothing.
 * Device: a kernel of its own beside mc_nw_pileup_strands' (which that call keeps launching): the
 * counts go the same way; the weights take an atomic per column -- a lane walks a run of at most 8
 * columns, longer runs are taken by the whole wave, 64 consecutive columns per step.
 */
#define MC_QUAL_MAX 93
int mc_load_qualities(mc_ctx *ctx, const uint8_t *qual, uint64_t bytes);
int mc_nw_qpileup_strands(mc_ctx *ctx, const uint32_t *a, const uint32_t *b, const uint8_t *a_minus, uint64_t m,
                          const uint32_t *targets, uint32_t nt, uint64_t *row_off /* nt + 1, required */,
                          uint32_t *table, uint32_t *wtable /* each row_off[nt] * MC_PILEUP_CH */, uint64_t cap_rows,
                          int32_t *score, int32_t *len, int32_t *ids /* m each, may be NULL */);

/*
 * THE ALIGNMENTS of mc_nw_align_strands laid out in common columns per centre: a centre-anchored
 * multiple alignment, the pile-up's sibling that keeps the inserted bases.  Pairs, operand rule,
 * strands, batching and caps are mc_nw_align_strands' own: seq1 is the read a[i], or its minus-strand
 * string where a_minus[i] != 0; seq2 is the centre b[i] as written.  targets are nt distinct centre
 * ids, as for mc_nw_pileup_strands; target t of L bytes owns rows row_off[t] .. row_off[t + 1],
 * L + 1 of them.  For target t with centre bytes c[0 .. L) and its pairs (those with b[i] == targets[t]):
 *   ins(i, r)   the length of pair i's 'I' run met with r centre bases consumed, 0 if there is none
 *               (a pair has at most one 'I' run per r)
 *   w[r]        max over the pairs of ins(i, r), r = 0 .. L; 0 for a target without pairs
 *   col[r]      r + w[0] + .. + w[r] for r < L: the column of centre base r; its w[r] insertion
 *               slots are the columns col[r] - w[r] .. col[r] - 1
 *   W           L + w[0] + .. + w[L], the block's width; col[L] = W, the trailing slots are
 *               W - w[L] .. W - 1
 * The character of a byte x is "ACGT"[x] for x <= 3, else the byte itself (the FASTA writer's
 * rule); the gap is MC_MSA_GAP.
 *   centre row  the centre's characters at col[r], gaps elsewhere
 *   pair row    walking the alignment with i read bases and j centre bases consumed: '=' / 'X' writes
 *               the character of seq1[i] at col[j]; 'D' leaves a gap at col[j]; an 'I' run of n writes
 *               the characters of seq1[i .. i + n) at col[j] - w[j] + t for t < n (left-justified, the
 *               remaining w[j] - n slots are gaps); every slot where the pair has no 'I' run is a gap
 * Every row of a block has exactly W bytes.  Removing the gaps from a pair row gives seq1 as aligned,
 * from the centre row the centre; every column holds a non-gap in at least one row of the block.
 * The bytes depend neither on the order of the pairs nor on any batching.
 *
 * mc_nw_msa_begin aligns every pair once (mc_nw_align_strands' forward and traceback kernels, its
 * batches and environment caps) and leaves a plan with the context: w and col of every row and
 * every pair's packed operation words, in device buffers the plan owns (no other entry touches them;
 * other alignment entries may be called between begin and rows), the pair list on the host.
 * row_off (nt + 1, required) receives the prefix sums of L + 1, width (row_off[nt], may be NULL)
 * every w[r], block_width (nt, required) every W; score / len / ids (m each, may be NULL) are
 * mc_nw_align_strands' bit for bit.  Errors are mc_nw_pileup_strands': a duplicate target, an id >= n
 * or a b[i] that is no target is MC_ERR_ARG, a pair above the scratch cap MC_ERR_UNSUPPORTED, both
 * found before any launch, nothing written, row_off included; no sequences: MC_ERR_STATE.  A
 * W >= 2^31 is MC_ERR_UNSUPPORTED and leaves no plan.  m = 0 is MC_OK: every block is its centre
 * alone (W = L).  A begin drops the plan before it whether it succeeds or not; mc_nw_msa_end (which
 * also frees the plan's device buffers), mc_load_sequences, mc_load_packed and mc_ctx_destroy drop it too.
 *
 * mc_nw_msa_rows renders rows first .. first + count: row k < nt is target k's centre row, row
 * nt + i pair i's.  off (count + 1, required) receives the prefix sums of the rows' lengths, each
 * the W of the row's target.  out == NULL: the offsets only, no device work.  out != NULL with
 * cap < off[count]: MC_ERR_ARG, off valid, nothing written to out.  A range past nt + m:
 * MC_ERR_ARG.  No plan: MC_ERR_STATE.  count = 0: MC_OK.  The rows are rendered in batches: a batch
 * ends before the row that would take its output past MC_MSA_BATCH_BYTES (a longer row gets a batch
 * of its own) and where MC_IDENT_BYTES ends a batch of minus-strand strings (the distinct minus
 * reads of a batch are reverse-complemented once).  Environment, read per call: MC_MSA_BYTES=<bytes>
 * lowers the first cap.  Batching, and the split of the rows over calls, change no byte.
 * Device: a wavefront per pair max-es its 'I' runs into w (integer atomics), a wavefront per target
 * scans w into col and W, a wavefront per row renders it, every byte stored exactly once.  All are
 * timed as "nw", the reverse complement as "layout".  mc_nw_msa_profile: out[0 .. 3] = device ms of
 * the forward, the traceback (+ packing), the width + column and the render kernels since the last
 * reset (a reset also clears mc_nw_align_profile's two times).
 */
#define MC_MSA_GAP '-'
#define MC_MSA_BATCH_BYTES (256ull << 20)
int mc_nw_msa_begin(mc_ctx *ctx, const uint32_t *a, const uint32_t *b, const uint8_t *a_minus, uint64_t m,
                    const uint32_t *targets, uint32_t nt, uint64_t *row_off /* nt + 1, required */,
                    uint32_t *width /* row_off[nt], may be NULL */, uint64_t *block_width /* nt, required: W per target */,
                    int32_t *score, int32_t *len, int32_t *ids /* m each, may be NULL */);
int mc_nw_msa_rows(mc_ctx *ctx, uint64_t first, uint64_t count, uint8_t *out, uint64_t cap, uint64_t *off /* count + 1, required */);
int mc_nw_msa_end(mc_ctx *ctx);
int mc_nw_msa_profile(mc_ctx *ctx, double *out /* 4 */, int reset);

/*
 * THE COLUMN PROFILE of the multiple alignment: every column of a block counted on the device, so
 * that 32 bytes per column come back instead of one byte per row and column.  mc_nw_msa_counts works
 * on the plan of the last mc_nw_msa_begin, for targets first_target .. first_target + ntargets in
 * the plan's target order.  Target t owns W_t columns (begin's block_width) of MC_MSA_CH counters;
 * col_off (ntargets + 1, required) receives the prefix sums of W_t.  In begin's terms, with depth the
 * number of the target's pairs and the class of a byte x being x for x <= 3, else 4:
 *   the column of centre base r (col[r], r < L)
 *       channels 0..5   row r, channels 0..5, of mc_nw_pileup_strands' table for the same pairs, bit
 *                       for bit: 0..4 the reads' bytes by class, 5 the reads with a 'D'
 *       channel 6       r;  channel 7: 0
 *   slot t (0-based) of site r (column col[r] - w[r] + t, r = 0 .. L, t < w[r])
 *       channel c <= 4  the pairs whose 'I' run at r is longer than t and whose inserted byte
 *                       seq1[i + t] has class c
 *       channel 5       depth less the sum of channels 0..4: the rows that hold a gap there
 *       channel 6       r;  channel 7: t + 1
 * Invariants: channels 0..5 of every column add up to depth; channel 5 of slot 0 equals depth less
 * pile-up channel 6 of row r; over a site's slots the sum of channels 0..4 is pile-up channel 7 of
 * row r; a target without pairs has L columns of zeros apart from channel 6; the counts are integers,
 * so nothing depends on the pair order, the batches or the split of targets over calls; the counts
 * equal the per-column histogram of the pair rows mc_nw_msa_rows renders (the centre row is not
 * counted; a read byte above 3 that is itself one of the characters A C G T - is class 4 here, as in
 * the pile-up, and shows as that character there).
 * wcounts, the same shape, holds weights from mc_load_qualities (Qs as for mc_nw_qpileup_strands):
 *   centre column r   channels 0..5 equal mc_nw_qpileup_strands' wtable row r, channels 0..5,
 *                     its rule for 'D' included
 *   slot t of site r  channel c <= 4: the sum of Qs(i + t) over the pairs counted in counts'
 *                     channel c; channel 5: 0
 *   channels 6 and 7  0 everywhere
 * counts and wcounts both NULL: the offsets only, no device work.  wcounts alone non-NULL:
 * MC_ERR_ARG.  wcounts non-NULL with no qualities loaded: MC_ERR_STATE.  Either non-NULL with
 * cap_cols < col_off[ntargets]: MC_ERR_ARG, col_off valid, nothing written.  A range past the plan's
 * nt: MC_ERR_ARG.  No plan: MC_ERR_STATE.  ntargets = 0: MC_OK.  With wcounts, a target of more than
 * (2^32 - 1) / MC_QUAL_MAX = 46,182,038 pairs: MC_ERR_ARG.  All of these are found before any launch.
 * The tables are overwritten, not added to; the plan is unchanged, so rows and counts may be called
 * in any order and any number of times.
 * Device: the targets go in batches whose column tables (a context-owned buffer) stay within
 * MC_MSA_BATCH_BYTES (MC_MSA_BYTES lowers it; a wider target is taken alone); the pairs of a batch of
 * targets in batches of minus-strand strings as mc_nw_msa_rows' (MC_IDENT_BYTES).  A wavefront per pair
 * walks the plan's operation words: two atomics per '=' or 'D' run on per-centre difference arrays,
 * one per mismatched column and per inserted base on the column table; with wcounts one more per
 * column (a lane walks a run of at most 8 columns, longer runs are taken by the whole wave).  A
 * wavefront per target then turns the differences into counts, writes channels 6 and 7 and every
 * slot's gap count, with no atomics.  Nothing is aligned again.  Timed as "nw", the reverse
 * complement as "layout".  mc_nw_msa_counts_profile: out[0] = device ms of the counts kernels since
 * the last reset; mc_nw_msa_profile's four values do not include them.
 */
#define MC_MSA_CH 8
int mc_nw_msa_counts(mc_ctx *ctx, uint32_t first_target, uint32_t ntargets, uint64_t *col_off /* ntargets + 1, required */,
                     uint32_t *counts, uint32_t *wcounts /* each col_off[ntargets] * MC_MSA_CH */, uint64_t cap_cols);
int mc_nw_msa_counts_profile(mc_ctx *ctx, double *out /* 1 */, int reset);

/*
 * THE ALLELES AT CHOSEN COLUMNS of the multiple alignment: what every read carries at the few columns
 * where its cluster disagrees with itself, so that S bytes per pair come back instead of its whole
 * row.  mc_nw_msa_sites works on the plan of the last mc_nw_msa_begin; nt and m are the plan's.
 * Target t owns the sites sites[site_off[t] .. site_off[t + 1]), S_t columns of its block: strictly
 * ascending, each < W_t; S_t may be 0 and may be W_t.  Pairs are numbered as mc_nw_msa_rows numbers
 * them: pair i is row nt + i, in the list order of begin.  For pairs first .. first + count, with
 * t(i) the target of pair i:
 *   off (count + 1, required)   the prefix sums of S_t(i)
 *   alleles[off[k] + s]         byte sites[site_off[t] + s] of the row mc_nw_msa_rows renders for pair
 *                               first + k: that row restricted to the chosen columns, byte for byte,
 *                               MC_MSA_GAP included
 *   quals[off[k] + s]           (may be NULL) the weight pair first + k adds to that column of
 *                               mc_nw_msa_counts' wcounts: where the column holds a base of the pair
 *                               ('=', 'X', or an inserted base in its slot) Qs of that base as aligned;
 *                               at a centre column the pair deletes mc_nw_qpileup_strands' 'D' rule
 *                               (the smaller quality around the gap); in a slot the pair leaves
 *                               empty 0
 * The bytes depend neither on batching nor on the split of the pairs over calls.  The plan is
 * unchanged: the entry may be mixed freely with rows, counts and the other alignment entries.
 * No plan: MC_ERR_STATE.  A range past m, a site_off that does not start at 0 or decreases, a site
 * list that is not strictly ascending within a target or holds a site >= W_t: MC_ERR_ARG.  alleles
 * NULL: the offsets only, no device work; quals non-NULL with alleles NULL: MC_ERR_ARG.  quals non-NULL
 * with no qualities loaded: MC_ERR_STATE.  alleles non-NULL with cap < off[count]: MC_ERR_ARG, off
 * valid, nothing else written.  count = 0: MC_OK.  All of these are found before any launch, and
 * nothing is written except where said.
 * Device: for the targets the requested pairs have, a lane per site finds its (row, slot) in the target's
 * columns by bisection, into a context-owned buffer kept for the call (every list is validated, only the
 * span of the site list those targets cover is uploaded).  The pairs go in batches whose outputs stay within
 * MC_MSA_BATCH_BYTES (MC_MSA_BYTES lowers it) and whose minus-strand strings are batched as
 * mc_nw_msa_rows' (MC_IDENT_BYTES, the distinct minus reads of a batch reverse-complemented once).
 * A batch's alleles are filled with the gap and its weights with 0; a wavefront per pair then walks the
 * plan's operation words, and the lane that owns a run stores the bytes of the sites inside it: every
 * non-gap byte is stored exactly once.  Nothing is aligned again.  Timed as "nw", the reverse
 * complement as "layout".  mc_nw_msa_sites_profile: out[0] = device ms of these kernels since the last
 * reset; mc_nw_msa_profile's and mc_nw_msa_counts_profile's values do not include them.
 */
int mc_nw_msa_sites(mc_ctx *ctx, const uint64_t *site_off /* nt + 1 */, const uint32_t *sites /* site_off[nt] */,
                    uint64_t first, uint64_t count, uint8_t *alleles, uint8_t *quals /* may be NULL */, uint64_t cap,
                    uint64_t *off /* count + 1, required */);
int mc_nw_msa_sites_profile(mc_ctx *ctx, double *out /* 1 */, int reset);

/*
 * TWO ALIGNMENTS OF ONE READ, BASE BY BASE: the evidence that a read copies one centre on its left and
 * another on its right (a chimera).  mc_nw_msa_crossover works on the plan of the last mc_nw_msa_begin;
 * x[c] and y[c] are pair indices of its list (pair i is row nt + i of mc_nw_msa_rows) and name two
 * pairs of the same read, a[x[c]] == a[y[c]]; their centres and their strands may differ.
 * For a pair p whose read has la bases and u in [0, la), e_p(u) is 1 if base u of the read AS WRITTEN
 * lies in an '=' column of p's alignment and 0 otherwise: for a pair begun with a_minus != 0, base i
 * of seq1 as aligned is base la - 1 - i as written; 'X' and 'I' bases have e = 0, 'D' columns hold no
 * read base, so the sum of e_p is the ids begin reports for p.  With
 *   D(s) = sum over u < s of (e_x(u) - e_y(u)),   s = 0 .. la
 * ids_y + D(s) counts the identities of a two-parent model that follows x on the read's bases [0, s)
 * and y on [s, la).  Candidate c's MC_CROSS_RES values, out[c * MC_CROSS_RES + slot]:
 *   0, 1   ids_x, ids_y
 *   2      best_xy = ids_y + max over s of D(s)   (x left of the cut, y right)
 *   3, 4   the smallest and the largest s attaining that maximum
 *   5      best_yx = ids_x - min over s of D(s)   (y left, x right)
 *   6, 7   the smallest and the largest s attaining that minimum
 * s = 0 and s = la are allowed, so both best values are at least max(ids_x, ids_y); x == y gives
 * ids, cuts 0 and la; exchanging x and y exchanges slots 0 <-> 1 and (2, 3, 4) <-> (5, 6, 7); a read
 * of 0 bases gives eight zeros.  All values are integer sums: nothing depends on batching, on the
 * order of the candidates or on their split over calls.
 * No plan: MC_ERR_STATE.  nc = 0: MC_OK.  x, y or out NULL with nc > 0, an index >= m, or
 * a[x[c]] != a[y[c]]: MC_ERR_ARG.  A read longer than MC_CROSS_MAX_READ bases (what two bitmaps in
 * 64 KiB of LDS hold; the environment variable MC_CROSS_MAX=<bases>, read per call, lowers it):
 * MC_ERR_UNSUPPORTED.  All of these are found before any launch, and nothing is written.  The plan is
 * unchanged and nothing is aligned again: the entry may be mixed freely with rows, counts, sites and
 * the other alignment entries, and the band mode (mc_set_align_band) changes nothing.
 * Device: the candidates go in batches of at most MC_CROSS_BATCH_CANDS (MC_CROSS_BATCH=<n> lowers it),
 * within a batch in launches by read length (at most 1024 << g bases, g = 0 .. 8), each with the LDS
 * its own longest read needs.  A wavefront per candidate fills two bitmaps of la bits in LDS from the
 * plan's operation words and scans their difference; 32 bytes per candidate come back.  Timed as
 * "nw".  mc_nw_msa_crossover_profile: out[0] = device ms of this kernel since the last reset; the
 * other msa profile entries' values do not include it.
 */
#define MC_CROSS_RES 8
#define MC_CROSS_MAX_READ (1u << 18)
#define MC_CROSS_BATCH_CANDS (1ull << 20)
int mc_nw_msa_crossover(mc_ctx *ctx, const uint64_t *x, const uint64_t *y, uint64_t nc, int32_t *out /* nc * MC_CROSS_RES */);
int mc_nw_msa_crossover_profile(mc_ctx *ctx, double *out /* 1 */, int reset);

/*
 * DEREPLICATION.  Two points are DUPLICATES if their expanded byte strings (what mc_nw_identity reads:
 * 0..3 inside segments, 'N' or the raw upper-case byte outside) are equal; with both strands also if
 * one string equals the other's minus-strand string (above).  The map of the minus strand is an
 * involution, so this is an equivalence relation and comparing against one member of a class decides
 * membership.  The bytes decide, not the letters: a record kept as raw letters and the same bases as
 * digits are not duplicates (lower case is folded by the parser before anything is loaded).
 * mc_derep, for the m points ids (an id may occur more than once: the occurrences are duplicates of
 * each other; two empty strings are duplicates):
 *   rep[i]    the smallest position j of the list such that point ids[j] is a duplicate of point
 *             ids[i]; so rep[rep[i]] == rep[i] and rep[i] == i for a class's first member
 *   minus[i]  0 where ids[i]'s string equals that of ids[rep[i]] as written -- this wins, so a string
 *             that is its own minus strand gives 0 --, else 1: it equals the representative's
 *             minus-strand string.  With strands == MC_STRAND_PLUS minus may be NULL and is all zeros.
 * The result is exact and a function of the strings alone: it does not depend on where a string lies
 * in the buffer, on the order of ids beyond the rule of the smallest position, on batching, on the grid
 * or on the fingerprint function; no hash collision can merge or split a class.
 * Device (gpu/derep.hip): one fingerprint kernel over the listed points, a wavefront
 * per point, gives every point a 128-bit key, a position-keyed integer sum of its bytes with the
 * length mixed in; with both strands the key is the smaller of the string's and its minus strand's,
 * both from the same loads.  The host sorts the positions by (key, length, position); a run of equal
 * (key, length) is a candidate group, its first position the leader.  The compare kernel, a wavefront
 * per pair, returns for every other member a byte: bit 0 equal to the leader as written, bit 1 equal
 * to the leader's minus-strand string.  Members that match neither way (a collision of keys) form a
 * new group under their own first position and are compared again, until none is left; every round
 * settles at least the leader of every open group.  The pairs of a round go in batches of
 * MC_DEREP_BATCH_PAIRS.  Environment, read per call: MC_DEREP_BATCH=<pairs> lowers the batch,
 * MC_DEREP_HASH_BITS=<0..128> keeps only that many leading bits of every key (0: all points of one
 * length form one group) -- the test hook of the collision rounds; neither changes a result.
 * No sequences: MC_ERR_STATE.  strands other than MC_STRAND_PLUS or MC_STRAND_PLUS | MC_STRAND_MINUS,
 * an id >= n, ids or rep NULL with m > 0, minus NULL with both strands, m >= 2^32: MC_ERR_ARG.  m = 0:
 * MC_OK.  All of these are found before any launch; rep and minus are written only by a call that
 * returns MC_OK.  There is no host fallback.
 * mc_derep_profile, since the last reset: out[0] device ms of the fingerprint kernel, out[1] device ms
 * of the compare kernel, out[2] pairs compared, out[3] compare rounds, out[4] pairs whose compare said
 * "not equal" (collisions).  The two kernels are counted in no family of mc_timers.
 */
#define MC_DEREP_BATCH_PAIRS (1ull << 22)
int mc_derep(mc_ctx *ctx, const uint32_t *ids, uint64_t m, int strands /* MC_STRAND_PLUS or PLUS | MINUS */,
             uint32_t *rep /* m */, uint8_t *minus /* m; may be NULL when strands is plus only */);
int mc_derep_profile(mc_ctx *ctx, double *out /* 5 */, int reset);

/*
 * Accumulation (ClusterFactory::accumulate, ClusterFactory.cpp:637-714).
 * The bvec of Runner.cpp:342-350 is only ever shrunk after insert_finalize, so the device
 * holds one static candidate order (bin-major, length-sorted within bins) plus an alive
 * mask.  order[pos] = point id.
 */
int mc_set_order(mc_ctx *ctx, const uint32_t *order, uint64_t n);
/* bvec::pop / bvec::erase of one static position (bvec.cpp:95-106, 349-353). */
int mc_kill(mc_ctx *ctx, uint64_t pos);
/* Start a new cluster whose member list is {first} (accumulate's `current = {last}`). */
int mc_cluster_begin(mc_ctx *ctx, uint32_t first_id);
/*
 * One get_close step (Trainer.cpp:34-114) of centre `centre_id` over the alive static
 * positions S..E (inclusive; the bvec_iterator range of ClusterFactory.cpp:650-654), then,
 * if some candidate was similar, bvec::remove_available (bvec.cpp:289-318) + get_mean
 * (ClusterFactory.cpp:382-425).  flagged_pos receives the removed static positions in
 * ascending (bvec) order; cap is its capacity.  cap < n_flagged is MC_ERR_ARG, and the step has
 * then been applied in part: THE CONTEXT'S BVEC STATE (alive mask, cluster members) IS UNDEFINED
 * after that error until the next mc_set_order.  A bad window (S > E, E >= n) or centre is
 * MC_ERR_ARG with nothing changed.
 * A step that flags nothing (is_min) leaves the cluster as it is, a new cluster included: further
 * steps without an mc_cluster_begin in between go on growing the same cluster.
 */
int mc_scan(mc_ctx *ctx, uint32_t centre_id, uint64_t S, uint64_t E, uint32_t *flagged_pos,
            uint64_t cap, mc_scan_result *res);

/*
 * One get_close step sharded by record over `nparts` GPUs (Trainer.cpp:34-114
 * is an OpenMP loop over the window, ClusterFactory.cpp:650-654).  Every rank holds the same
 * bvec state; rank `part` scans only the alive positions of S..E in its static blocks: block
 * b = [b * MC_SHARD_BLOCK, (b + 1) * MC_SHARD_BLOCK) belongs to part b % nparts.  Nothing is
 * removed: flagged_pos receives this part's similar candidates (ascending); res holds this
 * part's is_min / has_best / best_pos / best_val / n_flagged.  The ranks then combine the
 * parts (is_min AND, first maximum = largest best_val, ties to the lowest best_pos, flagged
 * lists merged) and all call mc_scan_commit with the union.  8/16-bit histograms, k-mer
 * classifier (else MC_ERR_UNSUPPORTED).
 */
#define MC_SHARD_BLOCK 256
int mc_scan_part(mc_ctx *ctx, uint32_t centre_id, uint64_t S, uint64_t E, uint32_t part, uint32_t nparts,
                 uint32_t *flagged_pos, uint64_t cap, mc_scan_result *res);
/*
 * Second half of a sharded step: bvec::remove_available (bvec.cpp:289-318) of the union of
 * every part's flagged positions (ascending, n may be 0) and get_mean (ClusterFactory.cpp:
 * 382-425) over the grown cluster: res->new_centre, res->n_members, res->is_min = (n == 0).
 */
int mc_scan_commit(mc_ctx *ctx, const uint32_t *flagged_pos, uint64_t n, mc_scan_result *res);

/*
 * Alignment mode (--align, or an identity below 0.6: Runner.cpp:231-236), a get_close step's
 * Feature::align(*pt, *p) values (Feature.cpp:221-243; Trainer.cpp:34-114's OpenMP loop over
 * the window) sharded over `nparts` ranks: of the alive static positions of S..E in ascending
 * order, candidate i is aligned (GlobAlignE, the candidate as seq1, the centre as seq2) by part
 * i % nparts.  ident[0 .. *n_part) receives this part's identities in candidate order (cap: its
 * capacity); *pairs / *cells count the WHOLE window's alignments (the same on every part).
 * Nothing changes on the context.
 */
int mc_align_part(mc_ctx *ctx, uint32_t centre_id, uint64_t S, uint64_t E, uint32_t part, uint32_t nparts,
                  double *ident, uint64_t cap, uint64_t *n_part, uint64_t *pairs, uint64_t *cells);
/*
 * The rest of mc_scan's alignment-mode step with the identities given: ident[i] is
 * Feature::align of the window's i-th alive candidate (ascending static position, as the
 * parts of mc_align_part interleave back).  Flags, removes and re-centres exactly as mc_scan;
 * res->nw_pairs / nw_cells are 0 (mc_align_part counted them).
 */
int mc_scan_ident(mc_ctx *ctx, uint32_t centre_id, uint64_t S, uint64_t E, const double *ident,
                  uint32_t *flagged_pos, uint64_t cap, mc_scan_result *res);

/*
 * The whole accumulation phase on the device: ClusterFactory::MS's loop
 * `last = points.pop(); while (last) accumulate(&last, ...)` (ClusterFactory.cpp:717-730,
 * accumulate :637-714) run by one persistent kernel, bvec included -- no host round trip per
 * get_close step.  Call after mc_set_order on the fresh bvec: bin b holds the static
 * positions [bin_lo[b], bin_lo[b+1]) (bin_lo[nbins] = n) and bounds[b] is its begin bound
 * (bvec.cpp:9-24, 208-218).  sim is --id.  Output: *nclusters clusters in creation order;
 * cluster c has centre centre_ids[c] and members member_ids[member_off[c] ..
 * member_off[c+1]) in the reference's `current` order.  stats (may be NULL, else 5 entries)
 * receives {get_close steps, sum of window sizes, then the device controller's time in us:
 * bvec window + publish, waiting for the scanning workgroups, collect + get_mean}.  Returns MC_ERR_UNSUPPORTED when this bvec does not
 * fit the device controller (alignment mode, 32/64-bit histograms, very large n); the caller
 * then drives accumulation with mc_scan.
 */
int mc_accumulate(mc_ctx *ctx, const uint32_t *bin_lo, const uint64_t *bounds, uint32_t nbins, double sim,
                  uint32_t *centre_ids, uint64_t *member_off, uint32_t *member_ids, uint64_t *nclusters,
                  uint64_t *stats);

/*
 * One accumulation shared by `world` ranks, one GPU each (the loop of
 * ClusterFactory.cpp:717-730 whose get_close steps, Trainer.cpp:81-106, are split by record).
 * Every rank registers the same host-memory mailbox of mc_mailbox_bytes(world, n) zeroed bytes
 * (a POSIX shared-memory segment mapped by each rank's process, or one buffer shared by the
 * threads of one process) with mc_set_mailbox, after mc_set_order; then all ranks call
 * mc_accumulate with identical arguments.  Each rank's persistent kernel scans only its
 * interleaved tiles of every window (tile t of the static order belongs to rank t mod world);
 * per step the kernels exchange {first maximum of combo 0, flagged positions} through the
 * mailbox without the host, and every rank applies the same remove_available + get_mean, so
 * every rank returns the same partition as a single-rank run.  A rank that fails stops the
 * others after the exchange's deadline (MC_ERR_TIMEOUT).  world 0 detaches.
 */
uint64_t mc_mailbox_bytes(int world, uint64_t n);
/* share: how many ranks' kernels run on this rank's GPU (>= 1; each then takes that share of
   the CUs, so they are co-resident: tests put two ranks on one GPU) */
int mc_set_mailbox(mc_ctx *ctx, void *host, uint64_t bytes, int rank, int world, int share);
/* the PCI bus id of the context's GPU (ranks sharing a GPU find each other with it) */
int mc_ctx_pci_bus_id(mc_ctx *ctx, char *buf, int len);
/*
 * The accumulation kernel's plan for this context and bvec (call after mc_set_order and
 * mc_set_mailbox): info[0] workgroups, info[1] static positions per tile of ownership (every
 * rank sharing a mailbox must use the same tile: tile t belongs to rank t mod world), info[2]
 * flags {1 dense resident workers, 2 wide rows, 4 resident rows, 8 streaming rows}, info[3]
 * the dynamic LDS bytes.  MC_ERR_UNSUPPORTED when mc_accumulate would not take it.
 * mc_set_accum_grid caps the workgroups (0: one per CU, or the CU share of the ranks on this
 * GPU): ranks sharing a mailbox take the smallest grid among them, so each derives the same plan.
 */
int mc_accum_plan_info(mc_ctx *ctx, uint32_t nbins, uint32_t info[4]);
int mc_set_accum_grid(mc_ctx *ctx, uint32_t grid);
/*
 * Allocate now every device buffer mc_accumulate needs for this bvec (call after
 * mc_set_accum_grid): mc_accumulate then allocates and frees nothing.  Ranks that share one
 * GPU in one process call it before a common barrier, so that no rank's hipFree -- which waits
 * for the whole device -- runs while a peer's persistent kernel spins on this rank's step
 * records (the Trainer.cpp:81-106 loop split by record).
 */
int mc_accum_reserve(mc_ctx *ctx, uint32_t nbins);
/*
 * Confine the context to slot `slot` of `share` disjoint CU sets of its GPU (ranks sharing one
 * GPU: the one-GPU rehearsal of the record-sharded loops, ClusterFactory.cpp:744-749 and
 * Trainer.cpp:81-106).  The context's stream is re-created with a CU mask (a hardware queue of
 * its own), so every kernel of the rank -- the persistent accumulation grid included, sized to
 * the mask -- runs on those CUs only and never waits behind a peer rank's spinning kernel.
 * share 1 restores the whole GPU.  Call while the context is idle.
 */
int mc_ctx_partition(mc_ctx *ctx, int slot, int share);

/*
 * One mean-shift iteration over all centres (the omp parallel for of ClusterFactory.cpp:
 * 744-749 around mean_shift_update, :289-380): for centre j, the members of clusters
 * j-delta..j+delta (CSR member_off[C+1]/members, cluster order) are filtered by the
 * classifier (Trainer::filter) and the first member closest (distance_d) to their mean
 * becomes new_centre[j] (Trainer::closest, Trainer.cpp:351-365); unchanged if none pass.
 */
int mc_mean_shift(mc_ctx *ctx, const uint32_t *centre_ids, uint32_t C, const uint64_t *member_off,
                  const uint32_t *members, int delta, uint32_t *new_centre);

/*
 * One iteration of MS's update loop (ClusterFactory.cpp:740-760) in one device round trip:
 * mc_mean_shift over all centres, then the classifier pairs of merge (ClusterFactory.cpp:
 * 427-493, Trainer::merge Trainer.cpp:129-157) over the NEW centres: for i in [0, C) and t in
 * (i, min(C-1, i+delta)], pair q (i-major, t ascending) = feat->compute(new_centre[t],
 * new_centre[i]); similar[q] / combo0[q] as mc_classify_pairs.  *npairs receives the pair
 * count (sum over i of min(delta, C-1-i)); similar and combo0 need room for it.
 */
int mc_update_iteration(mc_ctx *ctx, const uint32_t *centre_ids, uint32_t C, const uint64_t *member_off,
                        const uint32_t *members, int delta, uint32_t *new_centre, uint8_t *similar,
                        double *combo0, uint64_t *npairs);

/*
 * The same for centres j0 <= j < j1 only (new_centre holds j1 - j0 entries): the per-rank
 * share of one iteration when the update is sharded over GPUs by centre; the ranks then
 * all-gather the new centres (the centre-reassignment exchange).
 */
int mc_mean_shift_range(mc_ctx *ctx, const uint32_t *centre_ids, uint32_t C, const uint64_t *member_off,
                        const uint32_t *members, int delta, uint32_t j0, uint32_t j1, uint32_t *new_centre);

/*
 * ---- alignment mode (--align, or --id < 0.6: Runner.cpp:32-34, 332) ---------------------
 * The trainer then installs a classifier whose only feature is MC_FEAT_ALIGN (identity of
 * utility::GlobAlignE, normalised with min 0 / max 1, weights {-cutoff, 1}; Trainer.cpp:
 * 570-577, Feature.cpp:90-95).  With such a classifier:
 *   - mc_scan runs the batched NW kernel of every alive window candidate (seq1) against the
 *     centre (seq2) -- Feature::align(*pt, *p) inside Trainer::get_close -- and classifies
 *     the identities; remove_available + get_mean are unchanged (k-mer histograms).
 *   - mc_classify_pairs / mc_mean_shift are not available (their pairs go through the
 *     reference's Feature::align memo, which the host replays): use mc_nw_identity +
 *     mc_classify_values + mc_mean_shift_select instead.
 */

/*
 * Classify precomputed single-feature values: raw[i * n_single + f] is feature lookup[f] of
 * pair i (Feature::compute_all_raw, Feature.cpp:54-84).  Same normalisation, combos, fma GLM
 * sum and decision as mc_classify_pairs.  Any output pointer may be NULL.
 */
int mc_classify_values(mc_ctx *ctx, const double *raw, uint64_t m, uint8_t *similar, double *combo0,
                       double *sum);

/*
 * mean_shift_update (ClusterFactory.cpp:289-380) with the Trainer::filter decision supplied
 * by the caller: for centre j the neighbourhood is members[member_off[b_j] .. member_off[e_j+1])
 * (b_j = max(0, j-delta), e_j = min(C-1, j+delta)); keep holds one byte per neighbourhood
 * entry, neighbourhoods concatenated in j order.  new_centre[j] = the first kept member
 * closest (distance_d) to the kept members' mean, or centre_ids[j] if none is kept.
 */
int mc_mean_shift_select(mc_ctx *ctx, const uint32_t *centre_ids, uint32_t C, const uint64_t *member_off,
                         const uint32_t *members, int delta, const uint8_t *keep, uint32_t *new_centre);

/*
 * ---- ranks sharing one clustering --------------------------------------
 * The reference runs on one host (OpenMP); here one process (or thread) per GPU shares a
 * clustering.  mc_comm is an RCCL communicator (librccl opened at run time) whose only
 * operation is an all-gather of equal host blocks in rank order, staged through the rank's
 * GPU and carried by RCCL over xGMI.  Rank 0 makes the id, the caller distributes it (e.g.
 * torch.distributed broadcast), every rank calls mc_comm_create (it blocks until all joined).
 * mc_comm_allgather's signature is the host driver's exchange callback
 * (mcl_run_sharded(..., allgather = mc_comm_allgather, user = comm)).
 */
typedef struct mc_comm mc_comm;
#define MC_COMM_ID_BYTES 128
int mc_comm_unique_id(uint8_t *id /* MC_COMM_ID_BYTES */);
int mc_comm_create(int device, int rank, int world, const uint8_t *id, mc_comm **out);
int mc_comm_allgather(mc_comm *comm, const void *in, uint64_t bytes, void *out /* world * bytes */);
int mc_comm_stats(const mc_comm *comm, uint64_t *calls, uint64_t *bytes);
/* abort != 0: ncclCommAbort (a peer failed), else ncclCommDestroy. */
int mc_comm_destroy(mc_comm *comm, int abort);

/* Wait for all work on the context's GPU (every stream; benchmark boundaries). */
int mc_sync(mc_ctx *ctx);

/* Device time (ms) and launches accumulated per kernel family since the last reset
   (diagnostics): ms_out[2f], ms_out[2f+1] for f = k-mer, keys, pairs, scan, finalize,
   mean shift, NW, static layout. */
int mc_timers(mc_ctx *ctx, double *ms_out, int n, int reset);

#ifdef __cplusplus
}
#endif
#endif
