// mcgpu.hpp -- internal header of libmcgpu (MI355X / gfx950 engine behind include/meshclust_amd.h).
//
// Data layout in HBM (one context = one GPU):
//   codes      n sequences' one-digit bytes, concatenated (the NW input, Point::get_data_str)
//   packed     the same as 2-bit codes, 16 bases per 32-bit word, records word-aligned (K1 input)
//   seq_off    byte offsets (n+1), seg/seg_off: k-mer segments per sequence
//   hist       n rows of B = 4^k bins of width w bytes, id order, row pitch 16-byte aligned
//   mag/sumsq  per row: sum of bins (pseudo magnitude) and sum of squared bins
//   len        per row: sequence length (incl. N) for the length-difference feature
//   order/alive  static bvec order (position -> id) and the alive mask of accumulation
//   members    the growing cluster of the current accumulation (ids + tie-break keys)
#pragma once
#include <hip/hip_runtime.h>

#include <array>
#include <cstdint>
#include <string>
#include <vector>

#include "../../../include/meshclust_amd.h"

namespace mcg {

// This wave's index in its workgroup, as a wave-uniform (SGPR) value: threadIdx.x >> 6 is
// uniform per wave, but the compiler's divergence analysis cannot see that, and everything
// derived from it (loop bounds, wave roles) would otherwise be computed per lane with
// exec-mask branches.
__device__ __forceinline__ int wave_id() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// Kernel families for the device timers (mc_timers): ms and launch count per family.
// F_LAYOUT: the static bvec-order copies of the rows (build_static), after K1
// F_NW_FWD / F_NW_TB: the forward and traceback kernels of nwtrace.hip; they count as F_NW in
// mc_timers and are kept apart only for mc_nw_align_profile; F_NW_PU: the pile-up kernels of
// pileup.hip, likewise part of F_NW and kept apart for mc_nw_pileup_profile; F_NW_MSAW / F_NW_MSAR:
// the width + column kernels and the render kernel of msa.hip, part of F_NW, for mc_nw_msa_profile;
// F_NW_MSAC: the counts kernels of msa.hip (mc_nw_msa_counts), part of F_NW, for mc_nw_msa_counts_profile;
// F_NW_BAND: the score-only launches of the width search (nwband.hip), part of F_NW, for mc_nw_band_profile;
// F_NW_MSAS: the resolve and gather kernels of msa.hip (mc_nw_msa_sites), part of F_NW, for mc_nw_msa_sites_profile;
// F_NW_CROSS: the kernel of crossover.hip (mc_nw_msa_crossover), part of F_NW, for mc_nw_msa_crossover_profile;
// F_DEREP_FP / F_DEREP_CMP: the fingerprint and compare kernels of derep.hip (mc_derep), past F_NW_END: part of no
// family of mc_timers, read by mc_derep_profile alone
enum Family { F_KMER = 0, F_KEYS, F_PAIRS, F_SCAN, F_FINAL, F_MSHIFT, F_NW, F_LAYOUT, F_NFAM, F_NW_FWD = F_NFAM, F_NW_TB, F_NW_PU, F_NW_MSAW, F_NW_MSAR, F_NW_MSAC, F_NW_BAND, F_NW_MSAS, F_NW_CROSS, F_NW_END, F_DEREP_FP = F_NW_END, F_DEREP_CMP, F_NALL };

// Classifier in the form the kernels consume (mc_classifier + the exact decision threshold).
struct DevClassifier {
  mc_classifier c;
  double thr;  // round(1/(1+exp(-sum))) == 1  <=>  sum >= thr   (host glibc exp, see abi.hip)
  int align;   // the only feature is MC_FEAT_ALIGN: raw[0] is an NW identity (Trainer.cpp:570-577)
  // layout 3 / 4: the feature set Trainer::train builds (feat_set = 1, Trainer.cpp:583-588):
  // lookup [LD, INT, MAN, PEARSON(, KUL)], combos [LD*INT, (LD*MAN)^2, PEARSON(, (LD*KUL)^2)]
  // with 3 or 4 combos (features.hpp classify_std); 0 = any other (classify_raw)
  int layout;
};

// The accumulation workers' division-light decision (features.hpp classify_fast), passed to
// the accumulation kernel only: rinv[i] = RN(1 / (maxs[i] - mins[i])) on the host, and
// is_sim ? n : 1 - n == noff + nsgn * n; on = 1 when the classifier has the trainer's layout
// and every range of features 2..4 is finite and nonzero.
// classify_small (8-bit bins, small magnitudes) also takes range[i] = RN(maxs[i] - mins[i]) and
// divides features 0 / 1 by it as mk_div (mk = 1 when those ranges and minima keep every operand
// of the division normal), and rB = RN(1 / B) for the centre's PTerms (set by the launcher).
struct FastCls {
  double rinv[MC_MAX_SINGLE], noff[MC_MAX_SINGLE], nsgn[MC_MAX_SINGLE], range[MC_MAX_SINGLE];
  double rB;
  int on, mk;
};

// Read-only view of the device histogram matrix passed to kernels by value.
struct HistView {
  const uint8_t *hist;
  const uint64_t *mag;
  const uint64_t *sumsq;
  const uint64_t *len;
  uint64_t pitch;  // bytes per row
  int B;           // bins
  int width;       // bytes per bin
};

struct ScanPartial {
  double val;
  uint64_t pos;
  int32_t has;
  int32_t pad;
};

// Device-side result record of one accumulation step (mirrors mc_scan_result).
struct ScanDev {
  mc_scan_result r;
  uint32_t nflag;     // atomic counter of flagged candidates this step
  uint32_t nmembers;  // members in the current cluster
};

struct Buf {
  void *p = nullptr;
  size_t bytes = 0;
};

// One pair of mc_nw_align_strands' batch (nwtrace.hip): seq1 at a_off of the minus-strand buffer
// (a_rc) or of the loaded codes, seq2 at b_off of the codes; r rows per lane; where the pair's
// choice words (bytes), boundary row (ints) and operation words (uint32, la + lb of them) start.
// w < 0: the full record of nwtrace.hip; w >= 0: the banded record of nwband.hip at that width
// (host/band.hpp; r is then BAND_R).
struct TracePair {
  uint64_t a_off, b_off, ch_off, bnd_off, ops_off;
  uint32_t la, lb, a_rc, r;
  int32_t w = -1;
  uint32_t pad = 0;
};
constexpr int TRACE_RES = 5;  // per pair: score, columns, identities, operation words, final state

// what the kernels of nwtrace.hip and nwband.hip are launched with
struct TraceArgs {
  const uint8_t *codes;  // the loaded sequences (seq2 always, seq1 of a plus pair)
  const uint8_t *rc;     // the batch's minus-strand strings (seq1 of a minus pair)
  const TracePair *pairs;
  const uint32_t *pidx;  // forward: the pairs of this launch (one R)
  uint32_t npairs;
  uint8_t *choice;
  int *bnd;
  int32_t *res;  // TRACE_RES ints per pair
  uint32_t *ops;
  int *err;
};

// One row of a render batch of mc_nw_msa_rows (msa.hip): W bytes at out_off of the batch's output;
// seq1 at a_off of the minus-strand buffer (a_rc) or of the loaded codes; its nw operation words at
// w_off of the plan's words (centre: none, the row is one '=' run of lb over the centre's own bytes);
// row0: the first of its target's lb + 1 widths and columns.
struct MsaRow {
  uint64_t out_off, a_off, w_off, row0;
  uint32_t la, lb, nw, W, a_rc, centre;
};

// One pair of a counts batch of mc_nw_msa_counts (msa.hip): seq1 and its words as in MsaRow; row0:
// the first of its target's lb + 1 widths and columns in the plan; col0 / drow0: where the target's
// W columns and lb + 1 difference entries start in the batch's tables; q_off: the read's offset in
// the loaded qualities (as loaded, whatever the strand).
struct MsaCountPair {
  uint64_t a_off, w_off, row0, col0, drow0, q_off;
  uint32_t la, lb, nw, W, a_rc, pad;
};

// One target of a counts batch: its centre's bytes at c_off of the loaded codes, row0 / col0 / drow0
// as in MsaCountPair, L bytes, W columns, depth pairs.
struct MsaCountTarget {
  uint64_t c_off, row0, col0, drow0;
  uint32_t L, W, depth, pad;
};

// One target of mc_nw_msa_sites (msa.hip): its S chosen columns at s_off of the call's site
// buffers, row0 the first of its L + 1 widths and columns in the plan.
struct MsaSiteTarget {
  uint64_t row0, s_off;
  uint32_t L, S;
};

// One pair of a gather batch of mc_nw_msa_sites: seq1 and its words as in MsaRow, row0 / s_off / S its
// target's (MsaSiteTarget), lb the centre's length; its S bytes at out_off of the batch's outputs;
// q_off: the read's offset in the loaded qualities (as loaded, whatever the strand).
struct MsaSitePair {
  uint64_t a_off, w_off, row0, s_off, out_off, q_off;
  uint32_t la, lb, nw, S, a_rc, pad;
};

// One candidate of a batch of mc_nw_msa_crossover (crossover.hip): the packed words of its two plan
// pairs x and y, la the bases of the read both have, minus bit 0 / bit 1: x / y was aligned
// reverse-complemented; its MC_CROSS_RES values go to slot `out` of the batch's output.
struct CrossPair {
  uint64_t xw_off, yw_off;
  uint32_t la, xnw, ynw, minus, out, pad;
};

// mc_nw_msa_begin's plan, kept until the next begin, mc_nw_msa_end or a load of
// sequences.  Its host half: the pairs (a_minus empty: none is minus), every pair's target, word
// count and word offset, the targets, their row offsets and block widths; tp_off / tp: every
// target's pairs in list order (nt + 1 offsets into m pair indices).  msa_drop assigns a fresh one.
struct MsaPlanHost {
  bool on = false;
  std::vector<uint32_t> a, b, targets, tof, nops, tp;
  std::vector<uint64_t> tp_off, woff, row_off, W;
  std::vector<uint8_t> a_minus;
  uint64_t npairs() const { return a.size(); }
  uint64_t ntargets() const { return targets.size(); }
  uint64_t target_len(uint64_t t) const { return row_off[t + 1] - row_off[t] - 1; }
  bool minus(uint64_t p) const { return !a_minus.empty() && a_minus[p]; }
  uint64_t row_width(uint64_t s) const { return W[s < ntargets() ? s : tof[s - ntargets()]]; }  // row s of mc_nw_msa_rows
};
// On the device, owned by the plan and touched by no other entry; they outlive a drop and are freed
// by mc_nw_msa_end or with the context.  width / col / words: a width and a column per pile-up row
// (uint32), every pair's packed operation words; bw: the block widths.
// rec / out: a render batch's row records and rendered bytes (mc_nw_msa_rows only).
// cnt / wcnt / cdiff / crec / ctgt: a counts batch's column tables, its two difference arrays, pair
// records and target records (mc_nw_msa_counts only).
// scol / sres / stgt / srec / sout / sq: a call's site columns, their resolved (row, slot + 1 or 0)
// and target records, a gather batch's pair records, alleles and weights (mc_nw_msa_sites only).
// xrec / xout: a batch's candidate records and results (mc_nw_msa_crossover only).
struct MsaPlan : MsaPlanHost {
  Buf width, col, words, bw, rec, out, cnt, wcnt, cdiff, crec, ctgt, scol, sres, stgt, srec, sout, sq, xrec, xout;
  std::array<Buf *, 19> bufs() {
    return {&width, &col, &words, &bw, &rec, &out, &cnt, &wcnt, &cdiff, &crec, &ctgt, &scol, &sres, &stgt, &srec, &sout, &sq, &xrec, &xout};
  }
};

// A range of one array of the device lazy introsort (split.hip): partitioned (left >= 0:
// children left, left + 1, cut between them) or finished (fin: a sorted leaf).
struct SplitNode {
  int64_t lo, hi, cut;
  int32_t depth, left, fin, pad;
};

// Pinned, device-mapped record the fused scan publishes (zero-copy; seq written last).
struct HostScan {
  mc_scan_result r;
  uint32_t seq;
  uint32_t pad;
  uint32_t flags[1];  // n_flagged static positions follow
};

}  // namespace mcg

struct mc_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  uint8_t *h_stage = nullptr;  // pinned staging ring for small uploads (abi_util.hpp stage_copy)
  uint8_t *h_dstage = nullptr;  // pinned landing buffer for a call's results (abi_util.hpp download_pinned)
  size_t h_dstage_cap = 0;
  size_t stage_off = 0;
  // sequences
  uint64_t n = 0;
  std::vector<uint64_t> h_seq_off;
  mcg::Buf codes, seq_off, seg, seg_off;
  mcg::Buf packed, pk_off, impure;  // 2-bit codes (16 bases per word, records word-aligned), impure flags
  int kmer_spec_k = 0;              // K1 rows already written at 8 bits for this k (mc_kmer_max's pass)
  // histograms
  int k = 0, B = 0, width = 0;
  uint64_t pitch = 0;
  mcg::Buf hist, mag, sumsq, len;
  // mc_kmer_build_strands(strands == 3): hist / mag / sumsq hold the canonical rows (canon.hip) and
  // hist_fwd keeps K1's forward rows at the same width and pitch for mc_orient_pairs; any later
  // K1 pass returns the context to forward rows and frees hist_fwd
  bool canon = false;
  mcg::Buf hist_fwd, or_runs;
  // classifier
  mcg::DevClassifier cls{};
  mcg::FastCls fcls{};
  bool has_cls = false;
  // accumulation state
  uint64_t norder = 0;
  mcg::Buf order, alive, members, member_keys, partials, scan_dev, flags_out;
  uint32_t step = 0;
  mcg::ScanDev *h_scan = nullptr;  // pinned mirror of scan_dev + flagged prefix (generic path)
  size_t h_scan_cap = 0;
  // fused path (8/16-bit bins): static chunk-major layout + zero-copy result
  mcg::Buf hs, mag_s, sumsq_s, len_s, ticket, msum;
  uint64_t npad = 0;
  mcg::HostScan *h_res = nullptr, *h_res_dev = nullptr;
  size_t h_res_cap = 0;
  uint32_t seq = 0;
  std::vector<uint64_t> pending_kills;
  bool pending_begin = false;
  uint64_t pending_first_pos = 0;
  std::vector<uint64_t> h_spos;  // id -> static position
  // alignment mode: host mirror of order/alive (builds the NW pair list of a window) and the
  // per-static-position identity the scan kernels classify
  std::vector<uint32_t> h_order;
  std::vector<uint8_t> h_alive;
  mcg::Buf ident_s, al_a, al_b, al_out, al_id, ord_ids;
  mcg::Buf acc_out;  // device-resident accumulation: counters / error word
  // Trainer::split's sorted arrays (mc_split_*): words, stopper scratch, range trees, queries
  mcg::Buf sp_words, sp_keys, sp_scr, sp_nodes, sp_nn, sp_q, sp_err;
  uint64_t sp_n = 0;
  uint32_t sp_narr = 0;
  int sp_depth0 = 0;
  // several ranks sharing one accumulation (mc_set_mailbox): host-memory mailbox, mapped
  void *mb_host = nullptr, *mb_dev = nullptr;
  uint64_t mb_bytes = 0;
  int mb_rank = 0, mb_world = 0, mb_share = 1;
  uint32_t acc_grid = 0;  // mc_set_accum_grid: cap on the accumulation kernel's workgroups (0: none)
  // mc_ctx_partition: this context's stream runs on slot `part_slot` of `part_share` disjoint CU
  // sets of its GPU (ranks sharing one GPU); part_cus CUs in the mask (0: the whole GPU)
  int part_slot = 0, part_share = 1, part_cus = 0;
  // scratch
  mcg::Buf s_a, s_b, s_c, s_d, s_e, s_f, s_g, s_h, s_i, s_j, s_k;
  mcg::Buf nw_items, nw_gran;  // NW chained row blocks: work items, bottom-row granules
  mcg::Buf rc_seq;             // mc_nw_identity_strands / mc_revcomp_sequences: a batch's minus-strand strings
  // mc_nw_align_strands: a batch's choice words, boundary rows, operation words, pair records,
  // results, launch lists, output offsets and packed operations; the error word
  mcg::Buf tr_choice, tr_bnd, tr_ops, tr_pairs, tr_res, tr_idx, tr_dst, tr_out, tr_err;
  double tr_choice_bytes = 0;  // choice bytes written since the last mc_nw_align_profile reset
  // mc_set_align_band: 0 the full record, 1 the certified band.  The width search's
  // pair records, boundary rows and scores of a launch; mc_nw_band_profile's counters: pairs
  // banded, pairs full, search launches, the sum of the planned w
  int align_band = 0;
  mcg::Buf bs_pairs, bs_bnd, bs_score;
  double band_stat[4] = {0, 0, 0, 0};
  // mc_nw_pileup_strands: the call's table (8 counters per row) and its two difference arrays
  // ('=' and 'D' coverage, an int per row), a batch's row base per pair, the targets' code offsets
  // and row offsets
  mcg::Buf pu_table, pu_diff, pu_rows, pu_toff, pu_roff;
  // mc_load_qualities: a Phred value per loaded byte (dropped by the next load of sequences);
  // mc_nw_qpileup_strands: the call's weight table and a batch's read offset per pair
  mcg::Buf qual, pu_wtable, pu_qoff;
  bool has_qual = false;
  mcg::MsaPlan msa;  // mc_nw_msa_begin's plan
  // mc_derep: the call's ids and keys, a compare batch's pair records and result bytes; since the last
  // mc_derep_profile reset: pairs compared, compare rounds, pairs that matched neither way
  mcg::Buf dr_ids, dr_keys, dr_pairs, dr_res;
  double dr_stat[3] = {0, 0, 0};
  // mc_update_iteration's member lists on the device and their host shadow: re-uploaded only
  // when a merge changed them (cleared when sequences are loaded: the ids were checked against n)
  mcg::Buf u_off, u_mem;
  std::vector<uint64_t> h_uoff;
  std::vector<uint32_t> h_umem;
  std::vector<void *> pinned;
  // timers: event pairs recorded around kernels, resolved lazily after the next stream sync
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  std::vector<hipEvent_t> ev_pool;
  std::vector<std::pair<int, int>> ev_pending;  // (family, pool index of the begin event)
  int ev_open = -1;
  double fam_ms[mcg::F_NALL] = {0};
  double fam_n[mcg::F_NALL] = {0};
};

namespace mcg {

void set_error(const std::string &m);
int hip_fail(hipError_t e, const char *what);
int ensure(Buf &b, size_t bytes);  // grow-only device buffer
void timed_begin(mc_ctx *c);
void timed_end(mc_ctx *c, Family f);
void flush_timers(mc_ctx *c);  // after a stream synchronisation

HistView hist_view(const mc_ctx *c);

// ---- launchers (defined in kmer.hip, k2.hip, nw.hip) -------------------------------------
int launch_expand(mc_ctx *c, uint64_t nexc, const uint64_t *d_exc_pos, const uint8_t *d_exc_val);
int launch_pack(mc_ctx *c);
int launch_kmer(mc_ctx *c, int k, int width, bool write, uint64_t *d_max, int *d_err);
int launch_distance_keys(mc_ctx *c, const uint32_t *d_piv, uint32_t npiv, const uint32_t *d_ids, uint64_t m,
                         uint16_t *d_keys);
// split.hip: words[p * n + t] = keys[p * n + t] << 32 | order[t]; the lazy introsort's queries
constexpr int32_t SPLIT_MAXNODE = 32768;
int split_build_words(mc_ctx *c, const uint32_t *d_order, uint64_t n, uint32_t npiv, const uint16_t *d_keys,
                      uint64_t *d_words);
// each accumulation cluster's members sorted by key and mapped to ids (k2.hip); clusters of
// more than order_members_max() members are left untouched
int launch_order_members(mc_ctx *c, const uint64_t *d_keys, const uint32_t *d_pos, const uint64_t *d_cl_off, uint64_t ncl,
                         uint32_t *d_ids);
uint64_t order_members_max();
// a small host array to device memory through the context's pinned staging ring (abi_util.hpp stage_copy)
int stage_h2d(mc_ctx *c, void *dst, const void *src, size_t bytes);
int launch_select(mc_ctx *c, uint64_t *d_words, uint64_t n, uint32_t *d_scr, SplitNode *d_nodes, int32_t *d_nnodes,
                  int32_t maxnode, int32_t depth0, uint32_t ngroups, const uint32_t *d_qarr, const uint64_t *d_qoff,
                  const uint64_t *d_qpos, uint64_t *d_qout, int *d_err);
int launch_pairs(mc_ctx *c, const uint32_t *d_a, const uint32_t *d_b, uint64_t m, const uint16_t *flags, int nflag,
                 double *d_raw, uint8_t *d_sim, double *d_c0, double *d_sum, bool classify);
int launch_scan(mc_ctx *c, uint32_t centre, uint64_t S, uint64_t E, const double *d_ident, int *nblocks);
int launch_merge_pairs(mc_ctx *c, const uint32_t *d_new, uint32_t C, const uint64_t *d_poff, uint32_t *d_a,
                       uint32_t *d_b);
int launch_values(mc_ctx *c, const double *d_raw, uint64_t m, uint8_t *d_sim, double *d_c0, double *d_sum);
int launch_finalize(mc_ctx *c, int nblocks);
int launch_mean_shift(mc_ctx *c, const uint32_t *d_cid, uint32_t C, const uint64_t *d_off, const uint64_t *h_off,
                      const uint32_t *d_mem, int delta, const uint8_t *d_keep, uint32_t *d_new, uint32_t j0,
                      uint32_t j1);
int build_static(mc_ctx *c);
bool accum_supported(const mc_ctx *c, uint32_t nb);
bool accum_plan_info(const mc_ctx *c, uint32_t nb, uint32_t info[4]);
uint64_t mailbox_slot_granules(uint32_t world, uint64_t n);  // mailbox granules per rank slot
// accum_kernel instantiations (accum_impl.hpp), one translation unit per worker form; width 1 / 2
// bytes per bin, nch 16 selects the compile-time 16-chunk rows (8-bit k = 4), prof the twin with
// the MC_ACCUM_PROFILE timers (the chunk forms have none: their profile runs carry no timers)
const void *accum_fn_dense(int width, int nch, bool prof);
const void *accum_fn_dstream(int width, int nch, bool prof);
const void *accum_fn_wide(int width, bool prof);
const void *accum_fn_chunk(int width, int nch, bool compact);
// every device buffer launch_accum needs for `nb` bins, allocated now (mc_accum_reserve: ranks
// sharing a GPU allocate before any rank launches, so no hipFree waits on a spinning peer kernel)
int accum_reserve(mc_ctx *c, uint32_t nb);
int launch_accum(mc_ctx *c, const uint32_t *d_bin_lo, const uint64_t *d_bounds, uint32_t nb, double sim,
                 uint32_t *d_mem_pos, uint64_t *d_mkeys, uint32_t *d_cl_centre, uint64_t *d_cl_off, uint64_t *d_out);
// nparts > 0: a sharded step (mc_scan_part) over this rank's static blocks only
int launch_fused_scan(mc_ctx *c, uint32_t centre, uint64_t S, uint64_t E, uint32_t seq, const double *d_ident,
                      uint32_t part = 0, uint32_t nparts = 0);
// mc_scan_commit: d_flags[0, nflag) ascending static positions (all ranks' flagged)
int launch_commit(mc_ctx *c, const uint32_t *d_flags, uint32_t nflag, uint32_t seq);
// NW on byte strings: pair p aligns A[aoff[ai[p]] .. aoff[ai[p]+1]) against B[...] (rows = A).
// Results go to slot p, or to slot d_out[p] when d_out is given.
int launch_nw(mc_ctx *c, const uint8_t *d_A, const uint64_t *d_aoff, const uint32_t *d_ai, const uint8_t *d_B,
              const uint64_t *d_boff, const uint32_t *d_bi, uint64_t m, const std::vector<uint64_t> &h_alen,
              const std::vector<uint64_t> &h_blen, double *d_ident, int32_t *d_len, int32_t *d_ids,
              int32_t *d_score, const uint32_t *d_out = nullptr);
// revseq.hip: the minus-strand strings (host/revseq.hpp) of the u points d_ids into d_out at the
// 16-byte-padded offsets d_out_off[u + 1] (out_bytes = its last entry); timed as F_LAYOUT
int launch_revseq(mc_ctx *c, const uint32_t *d_ids, uint32_t u, const uint64_t *d_out_off, uint64_t out_bytes,
                  uint8_t *d_out);

// canon.hip: the fold over the n forward rows d_in (the context's k, width, pitch) -- canonical
// rows to d_out with their mag / sumsq to the context's (d_out null: neither), the largest
// canonical bin max-ed into *d_max; the strands (d_sad given: and both sums) of the m pairs
// (d_a[p], h_b[p]) on the forward rows d_fwd, h_b cut into runs of equal b (uploaded to `runs`)
int launch_canon_rows(mc_ctx *c, const uint8_t *d_in, uint8_t *d_out, uint64_t *d_max);
int launch_orient(mc_ctx *c, const uint8_t *d_fwd, const uint32_t *d_a, const uint32_t *h_b, uint64_t m, Buf &runs,
                  uint8_t *d_strand, uint64_t *d_sad);

// nwtrace.hip: rows per lane and choice bytes of a pair; the forward and traceback kernels over
// a batch (results to d_res, TRACE_RES ints per pair; operation words to each pair's region of
// d_ops; *d_err set by a walk that found no path); the copy of every pair's words to d_out[d_dst[p]]
int nw_trace_rows(uint64_t la);
uint64_t nw_trace_choice_bytes(uint64_t la, uint64_t lb);
int launch_nw_trace(mc_ctx *c, const std::vector<TracePair> &h_pairs, const TracePair *d_pairs, const uint8_t *d_rc,
                    uint8_t *d_choice, int *d_bnd, uint32_t *d_ops, int32_t *d_res, int *d_err);
int launch_nw_pack(mc_ctx *c, uint32_t m, const TracePair *d_pairs, const uint32_t *d_ops, const int32_t *d_res,
                   const uint64_t *d_dst, uint32_t *d_out);

// nwband.hip: the banded forward kernel over the pairs q.pidx[0 .. q.npairs) (every one with w >= 0;
// called by launch_nw_trace inside its forward timer), the traceback of a batch that holds a banded
// pair (a thread per pair, either record), and the width search's score-only launch: the banded
// score of pair p at its w to d_score[p]
int launch_nwband_forward(mc_ctx *c, const TraceArgs &q);
int launch_nwband_traceback(mc_ctx *c, const TraceArgs &q);
int launch_nwband_scores(mc_ctx *c, uint32_t m, const TracePair *d_pairs, const uint8_t *d_rc, int *d_bnd, int32_t *d_score);

// pileup.hip: the pairs of a batch (after launch_nw_trace) added to the call's table and
// difference arrays, pair p's rows starting at d_rowbase[p]; naive: every column its own atomic.
// launch_nw_pileup_finish turns the difference arrays of every target into the '=' and 'D' counts.
int launch_nw_pileup(mc_ctx *c, uint32_t m, const TracePair *d_pairs, const uint8_t *d_rc, const uint32_t *d_ops,
                     const int32_t *d_res, const uint64_t *d_rowbase, uint32_t *d_table, int32_t *d_deq, int32_t *d_ddel,
                     bool naive);
int launch_nw_pileup_finish(mc_ctx *c, uint32_t nt, const uint64_t *d_tgt_off, const uint64_t *d_row_off, uint32_t *d_table,
                            const int32_t *d_deq, const int32_t *d_ddel);
// the same counts and, beside them, the loaded qualities (c->qual) summed per column into d_wtable
// (mc_nw_qpileup_strands); d_qoff[p]: the offset of pair p's read in the loaded sequences
int launch_nw_qpileup(mc_ctx *c, uint32_t m, const TracePair *d_pairs, const uint8_t *d_rc, const uint32_t *d_ops,
                      const int32_t *d_res, const uint64_t *d_rowbase, const uint64_t *d_qoff, uint32_t *d_table,
                      uint32_t *d_wtable, int32_t *d_deq, int32_t *d_ddel);

// msa.hip (mc_nw_msa_*): per pair of a batch (after launch_nw_trace) the length of every 'I' run
// max-ed into d_width[d_rowbase[p] + row]; per target the columns d_col and the block width d_bw
// from the widths; a render batch's rows (d_rows, nrows of them) into d_out.
int launch_msa_width(mc_ctx *c, uint32_t m, const TracePair *d_pairs, const uint32_t *d_ops, const int32_t *d_res,
                     const uint64_t *d_rowbase, uint32_t *d_width);
int launch_msa_columns(mc_ctx *c, uint32_t nt, const uint64_t *d_row_off, const uint32_t *d_width, uint32_t *d_col, uint64_t *d_bw);
int launch_msa_render(mc_ctx *c, uint64_t nrows, const MsaRow *d_rows, const uint8_t *d_rc, const uint32_t *d_words,
                      const uint32_t *d_width, const uint32_t *d_col, uint8_t *d_out);
// the pairs of a counts batch (d_pairs, npairs of them) added to the batch's column table d_counts
// (MC_MSA_CH counters per column) and difference arrays d_deq / d_ddel; d_wcounts given: the loaded
// qualities summed beside them.  launch_msa_counts_finish: per target of the batch the differences
// turned into counts, channels 6 and 7, and every slot's gap count.
int launch_msa_counts(mc_ctx *c, uint64_t npairs, const MsaCountPair *d_pairs, const uint8_t *d_rc, const uint32_t *d_words,
                      const uint32_t *d_width, const uint32_t *d_col, uint32_t *d_counts, uint32_t *d_wcounts, int32_t *d_deq,
                      int32_t *d_ddel);
int launch_msa_counts_finish(mc_ctx *c, uint32_t nt, const MsaCountTarget *d_tgts, const uint32_t *d_width, const uint32_t *d_col,
                             uint32_t *d_counts, const int32_t *d_deq, const int32_t *d_ddel);
// msa.hip (mc_nw_msa_sites): per target the chosen columns d_sites resolved against the plan's
// columns into d_res (row, slot + 1 or 0: what the counts write to channels 6 and 7); per pair of a
// gather batch the non-gap bytes at its target's sites into d_out (pre-filled with the gap) and,
// d_qout given, the loaded qualities beside them (pre-filled with 0).
int launch_msa_sites_resolve(mc_ctx *c, uint32_t nt, const MsaSiteTarget *d_tgts, const uint32_t *d_width, const uint32_t *d_col,
                             const uint32_t *d_sites, uint2 *d_res);
int launch_msa_sites(mc_ctx *c, uint64_t npairs, const MsaSitePair *d_pairs, const uint8_t *d_rc, const uint32_t *d_words,
                     const uint32_t *d_width, const uint32_t *d_col, const uint32_t *d_sites, const uint2 *d_res, uint8_t *d_out,
                     uint8_t *d_qout);
// crossover.hip (mc_nw_msa_crossover): per candidate of d_cands, none with a read above max_la bases, the
// eight values of its two pairs' '=' bitmaps into d_out; the launch's LDS is two bitmaps of max_la bits.
int launch_crossover(mc_ctx *c, uint32_t nc, const CrossPair *d_cands, const uint32_t *d_words, uint32_t max_la, int32_t *d_out);
// abi_msa.hip: forget mc_nw_msa_begin's plan (its device buffers stay for the next one)
void msa_drop(mc_ctx *c);

}  // namespace mcg

#define MCG_CHECK(expr)                                   \
  do {                                                    \
    hipError_t _e = (expr);                               \
    if (_e != hipSuccess) return mcg::hip_fail(_e, #expr); \
  } while (0)
