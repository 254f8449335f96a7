// abi_align.hip -- the alignment entries of include/meshclust_amd.h on lists of pairs that may sit
// on either strand: minus-strand strings, identities, alignments, pile-ups, qualities and the band
// (the multiple alignment's, mc_nw_msa_*, are in abi_msa.hip, on the helpers this file gives abi_util.hpp).
// Every list is cut into batches by host/pairbatch.hpp, through strand_batches but for the
// identities; as everywhere in libmcgpu the entries are synchronous and fail loudly.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../host/band.hpp"
#include "abi_util.hpp"
#include "mcgpu.hpp"

using namespace mcg;

namespace {

// a batch's caps: pairs (lowered by `pairs_env`), string bytes (MC_IDENT_BYTES), choice scratch (MC_ALIGN_SCRATCH)
mc::PairBatchCaps batch_caps(const char *pairs_env, uint64_t pairs, bool scratch) {
  return {pairs_env ? env_cap(pairs_env, pairs) : pairs, env_cap("MC_IDENT_BYTES", MC_IDENT_BATCH_BYTES),
          scratch ? env_cap("MC_ALIGN_SCRATCH", MC_ALIGN_SCRATCH_BYTES) : 0};
}

// a pair of 2^27 bases or more: every entry that traces or bands refuses it
bool pair_too_long(const mc_ctx *c, uint32_t a, uint32_t b) { return seq_len(c, a) + seq_len(c, b) >= (1ull << 27); }

// The width search of the certified band (host/band.hpp) over the pairs of a call,
// before its trace batches are planned: w[i] = pair i's planned width (-1: the full record),
// score[i] = its exact score.  The pairs go through the score-only kernel in mc_nw_identity_strands'
// batches (the pair cap, the minus-strand strings cap, the distinct minus reads reverse-complemented
// once: strand_batches).  Within a batch every pair starts at w0 and the uncertified ones are launched again at twice
// the width, until the certificate holds or the band holds the whole matrix: the score is then exact
// and the planned width w*(score) depends on neither w0 nor the schedule.  A launch is cut where the
// boundary rows of its pairs of more than one block would pass BAND_BND_BYTES.  Writes only to
// buffers of the context.  Pairs of 2^27 bases or more are the caller's to refuse first.
constexpr uint64_t BAND_W0 = 64, BAND_BND_BYTES = 256ull << 20;

uint64_t band_w0() {  // MC_BAND_W0=<n>, read per call: the first width of the search (n >= 1)
  const char *e = getenv("MC_BAND_W0");
  const long long v = e ? atoll(e) : 0;
  return v >= 1 ? (uint64_t)std::min<long long>(v, 1 << 27) : BAND_W0;
}

int band_search(mc_ctx *c, const uint32_t *a, const uint32_t *b, const uint8_t *a_minus, uint64_t m, int32_t *w, int32_t *score) {
  const uint64_t w0 = band_w0();
  std::vector<uint64_t> wcur, todo, next;
  std::vector<TracePair> recs;
  std::vector<int32_t> sc;
  auto planned = [&](uint64_t i, int64_t la, int64_t lb, int32_t S) {
    score[i] = S;
    w[i] = mc::band_plan(la, lb, S);
    c->band_stat[w[i] >= 0 ? 0 : 1] += 1;
    if (w[i] >= 0) c->band_stat[3] += w[i];
  };
  TRY(strand_batches(c, a, a_minus, m, batch_caps("MC_IDENT_BATCH", MC_IDENT_BATCH_PAIRS, false), nullptr, [&](const StrandBatch &v) -> int {
    todo.clear();
    wcur.assign(v.i1 - v.i0, w0);
    for (uint64_t i = v.i0; i < v.i1; i++) {
      const int64_t la = (int64_t)v.la(i), lb = (int64_t)seq_len(c, b[i]);
      if (la == 0)  // (nwtrace.hip: no rows; no columns: lowerGap's column 0 wins the final maximum)
        planned(i, la, lb, lb > 0 ? (int32_t)mc::band_neg_inf(la, lb) : 0);
      else if (lb == 0)
        planned(i, la, lb, (int32_t)(-2 - la));
      else
        todo.push_back(i);
    }
    while (!todo.empty()) {
      sc.resize(todo.size());
      for (size_t at = 0, end; at < todo.size(); at = end) {
        recs.clear();
        uint64_t bnd = 0;
        for (end = at; end < todo.size(); end++) {
          const uint64_t i = todo[end], la = v.la(i), lb = seq_len(c, b[i]);
          const uint64_t need = mc::band_bnd_ints(la, lb, wcur[i - v.i0]);
          if (end > at && (bnd + need) * 4 > BAND_BND_BYTES) break;
          TracePair pr{};
          pr.a_off = v.a_off(i);
          pr.b_off = c->h_seq_off[b[i]];
          pr.bnd_off = bnd;
          pr.la = (uint32_t)la;
          pr.lb = (uint32_t)lb;
          pr.a_rc = v.a_rc(i);
          pr.r = mc::BAND_R;
          pr.w = (int32_t)wcur[i - v.i0];
          recs.push_back(pr);
          bnd += need;
        }
        const size_t n = end - at;
        TRY(ensure(c->bs_bnd, bnd * 4 + 64));
        TRY(ensure(c->bs_score, n * 4 + 64));
        TRY(upload(c, c->bs_pairs, recs.data(), n, c->stream));
        TRY(launch_nwband_scores(c, (uint32_t)n, (const TracePair *)c->bs_pairs.p, (const uint8_t *)c->rc_seq.p, (int *)c->bs_bnd.p,
                                 (int32_t *)c->bs_score.p));
        TRY(download_parts(c, {{sc.data() + at, c->bs_score.p, n * 4}}, c->stream));
        c->band_stat[2] += 1;
      }
      next.clear();
      for (size_t k = 0; k < todo.size(); k++) {
        const uint64_t i = todo[k];
        const int64_t la = (int64_t)v.la(i), lb = (int64_t)seq_len(c, b[i]), wi = (int64_t)wcur[i - v.i0];
        if (mc::band_certified(la, lb, wi, sc[k]) || mc::band_is_whole(la, lb, wi)) {
          planned(i, la, lb, sc[k]);
        } else {
          wcur[i - v.i0] = (uint64_t)std::min<int64_t>(2 * wi, std::max(la, lb));
          next.push_back(i);
        }
      }
      todo.swap(next);
    }
    return MC_OK;
  }));
  flush_timers(c);
  return MC_OK;
}

// the plan of a call's pairs: empty with the band off (mc_set_align_band), else band_search's widths
int align_plan(mc_ctx *c, const uint32_t *a, const uint32_t *b, const uint8_t *a_minus, uint64_t m, std::vector<int32_t> &plan) {
  plan.clear();
  if (!c->align_band || m == 0) return MC_OK;
  plan.assign(m, -1);
  for (uint64_t i = 0; i < m; i++)  // (align_check_caps refuses the call)
    if (pair_too_long(c, a[i], b[i])) return MC_OK;
  std::vector<int32_t> score(m);
  return band_search(c, a, b, a_minus, m, plan.data(), score.data());
}

// the choice bytes of pair i under a plan (empty: the full record)
uint64_t planned_bytes(const std::vector<int32_t> &plan, uint64_t i, uint64_t la, uint64_t lb) {
  return !plan.empty() && plan[i] >= 0 ? mc::band_choice_bytes(la, lb, (uint64_t)plan[i]) : nw_trace_choice_bytes(la, lb);
}

// before any trace launch, and before any output is written: a pair whose planned bytes alone exceed the scratch cap
int align_check_caps(mc_ctx *c, const char *who, const uint32_t *a, const uint32_t *b, uint64_t m, const std::vector<int32_t> &plan) {
  const uint64_t scr_cap = env_cap("MC_ALIGN_SCRATCH", MC_ALIGN_SCRATCH_BYTES);
  for (uint64_t i = 0; i < m; i++) {
    const uint64_t la = seq_len(c, a[i]), lb = seq_len(c, b[i]);
    if (pair_too_long(c, a[i], b[i]) || planned_bytes(plan, i, la, lb) > scr_cap) {
      set_error(std::string(who) + ": pair " + std::to_string(i) + " (" + std::to_string(la) + " x " + std::to_string(lb) +
                ") needs " + std::to_string(planned_bytes(plan, i, la, lb)) + " bytes of choices, the cap is " +
                std::to_string(scr_cap));
      return MC_ERR_UNSUPPORTED;
    }
  }
  return MC_OK;
}

// tindex[point id] = its place among the targets (NO_TARGET: none); MC_ERR_ARG for a target listed
// twice or a b[i] that is no target
constexpr uint32_t NO_TARGET = 0xffffffffu;
int index_targets(mc_ctx *c, const std::string &who, const uint32_t *targets, uint32_t nt, const uint32_t *b, uint64_t m,
                  std::vector<uint32_t> &tindex) {
  tindex.assign(c->n, NO_TARGET);
  for (uint32_t t = 0; t < nt; t++) {
    if (tindex[targets[t]] != NO_TARGET) {
      set_error(who + ": point " + std::to_string(targets[t]) + " is listed twice among the targets");
      return MC_ERR_ARG;
    }
    tindex[targets[t]] = t;
  }
  for (uint64_t i = 0; i < m; i++)
    if (tindex[b[i]] == NO_TARGET) {
      set_error(who + ": pair " + std::to_string(i) + "'s seq2, point " + std::to_string(b[i]) +
                ", is not among the targets");
      return MC_ERR_ARG;
    }
  return MC_OK;
}

// mc_nw_pileup_strands (weighted false, wtable NULL) and mc_nw_qpileup_strands (weighted: the
// same call with the weighted pile-up kernel and a second table)
int pileup_call(mc_ctx *c, const std::string &who, bool weighted, const uint32_t *a, const uint32_t *b, const uint8_t *a_minus,
                uint64_t m, const uint32_t *targets, uint32_t nt, uint64_t *row_off, uint32_t *table, uint32_t *wtable,
                uint64_t cap_rows, int32_t *score, int32_t *len, int32_t *ids) {
  if (!c || !c->codes.p) return MC_ERR_STATE;
  if (weighted && !c->has_qual) {
    set_error(who + ": no qualities are loaded (mc_load_qualities)");
    return MC_ERR_STATE;
  }
  if (!row_off || (nt && !targets) || (m && (!a || !b))) return MC_ERR_ARG;
  if (weighted && !table != !wtable) {
    set_error(who + ": table and wtable are given together (both NULL: the offsets only)");
    return MC_ERR_ARG;
  }
  MCG_CHECK(hipSetDevice(c->device));
  std::vector<uint32_t> tindex;  // point id -> its place among the targets
  std::vector<int32_t> plan;
  TRY(align_targets(c, who, weighted, a, b, a_minus, m, targets, nt, row_off, tindex, plan));
  if (!table) return MC_OK;
  const uint64_t rows = row_off[nt];
  if (cap_rows < rows) {
    set_error(who + ": table holds " + std::to_string(cap_rows) + " rows, the targets have " + std::to_string(rows));
    return MC_ERR_ARG;
  }
  if (rows == 0) return MC_OK;
  if (m == 0) {
    memset(table, 0, rows * MC_PILEUP_CH * 4);
    if (weighted) memset(wtable, 0, rows * MC_PILEUP_CH * 4);
    return MC_OK;
  }
  // the table and the two difference arrays stay on the device for the whole call: zeroed once,
  // every batch adds to them, one download at the end
  TRY(ensure(c->pu_table, rows * MC_PILEUP_CH * 4 + 64));
  TRY(ensure(c->pu_diff, rows * 8 + 64));
  uint32_t *d_table = (uint32_t *)c->pu_table.p;
  int32_t *d_deq = (int32_t *)c->pu_diff.p, *d_ddel = d_deq + rows;
  MCG_CHECK(hipMemsetAsync(d_table, 0, rows * MC_PILEUP_CH * 4, c->stream));
  MCG_CHECK(hipMemsetAsync(d_deq, 0, rows * 8, c->stream));
  uint32_t *d_wtable = nullptr;
  if (weighted) {
    TRY(ensure(c->pu_wtable, rows * MC_PILEUP_CH * 4 + 64));
    d_wtable = (uint32_t *)c->pu_wtable.p;
    MCG_CHECK(hipMemsetAsync(d_wtable, 0, rows * MC_PILEUP_CH * 4, c->stream));
  }
  const char *nv = getenv("MC_PILEUP_NAIVE");  // (a measurement aid: an atomic per column; the same table)
  const bool naive = nv && atoi(nv) != 0;
  std::vector<uint64_t> rowbase, qoff;
  TRY(align_batches(c, who.c_str(), a, b, a_minus, m, plan, [&](uint64_t i0, uint64_t mb, const std::vector<int32_t> &res) {
    scatter_res(res, i0, mb, score, len, ids);
    rowbase.resize(mb);
    for (uint64_t k = 0; k < mb; k++) rowbase[k] = row_off[tindex[b[i0 + k]]];
    TRY(upload(c, c->pu_rows, rowbase.data(), mb, c->stream));
    if (weighted) {
      qoff.resize(mb);
      for (uint64_t k = 0; k < mb; k++) qoff[k] = c->h_seq_off[a[i0 + k]];
      TRY(upload(c, c->pu_qoff, qoff.data(), mb, c->stream));
      return launch_nw_qpileup(c, (uint32_t)mb, (const TracePair *)c->tr_pairs.p, (const uint8_t *)c->rc_seq.p,
                               (const uint32_t *)c->tr_ops.p, (const int32_t *)c->tr_res.p, (const uint64_t *)c->pu_rows.p,
                               (const uint64_t *)c->pu_qoff.p, d_table, d_wtable, d_deq, d_ddel);
    }
    return launch_nw_pileup(c, (uint32_t)mb, (const TracePair *)c->tr_pairs.p, (const uint8_t *)c->rc_seq.p,
                            (const uint32_t *)c->tr_ops.p, (const int32_t *)c->tr_res.p, (const uint64_t *)c->pu_rows.p, d_table,
                            d_deq, d_ddel, naive);
  }));
  std::vector<uint64_t> toff(nt);
  for (uint32_t t = 0; t < nt; t++) toff[t] = c->h_seq_off[targets[t]];
  TRY(upload(c, c->pu_toff, toff.data(), nt, c->stream));
  TRY(upload(c, c->pu_roff, row_off, (size_t)nt + 1, c->stream));
  TRY(launch_nw_pileup_finish(c, nt, (const uint64_t *)c->pu_toff.p, (const uint64_t *)c->pu_roff.p, d_table, d_deq, d_ddel));
  MCG_CHECK(hipMemcpyAsync(table, d_table, rows * MC_PILEUP_CH * 4, hipMemcpyDeviceToHost, c->stream));
  if (weighted) MCG_CHECK(hipMemcpyAsync(wtable, d_wtable, rows * MC_PILEUP_CH * 4, hipMemcpyDeviceToHost, c->stream));
  MCG_CHECK(hipStreamSynchronize(c->stream));
  flush_timers(c);
  return MC_OK;
}

// The minus-strand strings (host/revseq.hpp) of the u points ids into c->rc_seq, record r at
// h_off[r] (filled here: lengths rounded up to 16).  ids go through c->s_h, the offsets through
// c->s_i; the caller keeps ids and h_off alive until the stream is synchronized.
int revseq_batch(mc_ctx *c, const uint32_t *ids, uint32_t u, std::vector<uint64_t> &h_off) {
  h_off.resize((size_t)u + 1);
  h_off[0] = 0;
  for (uint32_t r = 0; r < u; r++)
    h_off[r + 1] = h_off[r] + (seq_len(c, ids[r]) + 15) / 16 * 16;
  TRY(ensure(c->rc_seq, h_off[u] + 16));
  TRY(upload(c, c->s_h, ids, u, c->stream));
  TRY(upload(c, c->s_i, h_off.data(), (size_t)u + 1, c->stream));
  return launch_revseq(c, (const uint32_t *)c->s_h.p, u, (const uint64_t *)c->s_i.p, h_off[u], (uint8_t *)c->rc_seq.p);
}

}  // namespace

int mcg::strand_batches(mc_ctx *c, const uint32_t *ids, const uint8_t *minus, uint64_t m, mc::PairBatchCaps caps, std::function<uint64_t(uint64_t)> scratch_at,
                        const std::function<int(const StrandBatch &)> &per_batch, const std::function<bool(uint64_t, uint64_t)> &wanted) {
  mc::PairBatcher pb(c->h_seq_off.data(), c->n, ids, nullptr, minus, m, caps);
  pb.scratch_at = std::move(scratch_at);
  std::vector<uint64_t> h_off(1, 0);  // the batch's strings, kept here until the stream is synchronized
  while (pb.next()) {
    if (wanted && !wanted(pb.i0, pb.i1)) continue;
    const uint32_t u = (uint32_t)pb.uniq.size();
    if (u) TRY(revseq_batch(c, pb.uniq.data(), u, h_off));
    TRY(per_batch({pb.i0, pb.i1, u ? h_off[u] : 0, c, ids, pb, h_off.data()}));
  }
  return MC_OK;
}

void mcg::scatter_res(const std::vector<int32_t> &res, uint64_t i0, uint64_t mb, int32_t *score, int32_t *len, int32_t *ids) {
  for (uint64_t k = 0; k < mb; k++) {
    if (score) score[i0 + k] = res[k * TRACE_RES];
    if (len) len[i0 + k] = res[k * TRACE_RES + 1];
    if (ids) ids[i0 + k] = res[k * TRACE_RES + 2];
  }
}

// The pairs of mc_nw_align_strands / mc_nw_pileup_strands / mc_nw_msa_begin in batches: the forward
// pass and the traceback of every batch, then per_batch(i0, mb, res) with the batch's TRACE_RES ints
// per pair on the host; the batch's pair records, operation words and results are still in
// c->tr_pairs, c->tr_ops and c->tr_res, its minus-strand strings in c->rc_seq.  `who` names the
// caller in errors.  plan: align_plan's; a pair's scratch is its planned bytes, banded or full.
int mcg::align_batches(mc_ctx *c, const char *who, const uint32_t *a, const uint32_t *b, const uint8_t *a_minus, uint64_t m,
                       const std::vector<int32_t> &plan, const std::function<int(uint64_t, uint64_t, const std::vector<int32_t> &)> &per_batch) {
  std::vector<TracePair> pairs;
  std::vector<int32_t> res;
  TRY(ensure(c->tr_err, 256));
  auto scratch_at = [&](uint64_t i) { return planned_bytes(plan, i, seq_len(c, a[i]), seq_len(c, b[i])); };
  return strand_batches(c, a, a_minus, m, batch_caps("MC_ALIGN_BATCH", MC_ALIGN_BATCH_PAIRS, true), scratch_at, [&](const StrandBatch &v) -> int {
    const uint64_t mb = v.i1 - v.i0;
    pairs.clear();
    uint64_t chb = 0, bnd = 0, opw = 0;
    for (uint64_t i = v.i0; i < v.i1; i++) {
      const uint64_t la = v.la(i), lb = seq_len(c, b[i]);
      TracePair pr;
      pr.a_off = v.a_off(i);
      pr.b_off = c->h_seq_off[b[i]];
      pr.ch_off = chb;
      pr.bnd_off = bnd;
      pr.ops_off = opw;
      pr.la = (uint32_t)la;
      pr.lb = (uint32_t)lb;
      pr.a_rc = v.a_rc(i);
      pr.w = plan.empty() ? -1 : plan[i];
      pr.r = pr.w >= 0 ? (uint32_t)mc::BAND_R : (uint32_t)nw_trace_rows(la);
      pairs.push_back(pr);
      chb += scratch_at(i);
      if (pr.w >= 0) bnd += mc::band_bnd_ints(la, lb, (uint64_t)pr.w);
      else if (la > 64ull * pr.r) bnd += 3 * (lb + 1);
      opw += la + lb;
    }
    TRY(ensure(c->tr_choice, chb + 64));
    TRY(ensure(c->tr_bnd, bnd * 4 + 64));
    TRY(ensure(c->tr_ops, opw * 4 + 64));
    TRY(ensure(c->tr_res, mb * TRACE_RES * 4 + 64));
    TRY(upload(c, c->tr_pairs, pairs.data(), mb, c->stream));
    TRY(launch_nw_trace(c, pairs, (const TracePair *)c->tr_pairs.p, (const uint8_t *)c->rc_seq.p, (uint8_t *)c->tr_choice.p,
                        (int *)c->tr_bnd.p, (uint32_t *)c->tr_ops.p, (int32_t *)c->tr_res.p, (int *)c->tr_err.p));
    c->tr_choice_bytes += (double)chb;
    res.resize(mb * TRACE_RES);
    int herr = 0;
    TRY(download_parts(c, {{res.data(), c->tr_res.p, mb * TRACE_RES * 4}, {&herr, c->tr_err.p, 4}}, c->stream));
    if (herr) {
      set_error(std::string(who) + ": a traceback did not reach the matrix's edge within la + lb steps, or left its band");
      return MC_ERR_HIP;
    }
    return per_batch(v.i0, mb, res);
  });
}

int mcg::align_targets(mc_ctx *c, const std::string &who, bool weighted, const uint32_t *a, const uint32_t *b, const uint8_t *a_minus,
                       uint64_t m, const uint32_t *targets, uint32_t nt, uint64_t *row_off, std::vector<uint32_t> &tindex,
                       std::vector<int32_t> &plan) {
  TRY(check_ids(c, targets, nt));
  TRY(check_ids(c, a, m));
  TRY(check_ids(c, b, m));
  TRY(index_targets(c, who, targets, nt, b, m, tindex));
  if (weighted) {  // a column's weight is at most MC_QUAL_MAX per pair: the sums must fit 32 bits
    std::vector<uint64_t> npairs(nt, 0);
    for (uint64_t i = 0; i < m; i++)
      if (++npairs[tindex[b[i]]] > 0xffffffffull / MC_QUAL_MAX) {
        set_error(who + ": target " + std::to_string(b[i]) + " receives more than " + std::to_string(0xffffffffull / MC_QUAL_MAX) +
                  " pairs, its weights would not fit 32 bits");
        return MC_ERR_ARG;
      }
  }
  TRY(align_plan(c, a, b, a_minus, m, plan));
  TRY(align_check_caps(c, who.c_str(), a, b, m, plan));
  row_off[0] = 0;
  for (uint32_t t = 0; t < nt; t++) row_off[t + 1] = row_off[t] + seq_len(c, targets[t]) + 1;
  return MC_OK;
}

int mcg::profile_families(mc_ctx *c, double *out, int reset, std::initializer_list<int> fams) {
  if (!c || !out) return MC_ERR_ARG;
  (void)hipStreamSynchronize(c->stream);
  flush_timers(c);
  for (int f : fams) {
    *out++ = c->fam_ms[f];
    if (reset) c->fam_ms[f] = c->fam_n[f] = 0;
  }
  return MC_OK;
}

extern "C" {

int mc_revcomp_sequences(mc_ctx *c, const uint32_t *ids, uint64_t m, uint8_t *bytes, uint64_t *off) {
  if (!c || !c->codes.p) return MC_ERR_STATE;
  if (!off || (m && !ids)) return MC_ERR_ARG;
  TRY(check_ids(c, ids, m));
  off[0] = 0;
  for (uint64_t i = 0; i < m; i++) off[i + 1] = off[i] + seq_len(c, ids[i]);
  if (!bytes || m == 0) return MC_OK;
  MCG_CHECK(hipSetDevice(c->device));
  const std::vector<uint8_t> all_minus(m, 1);
  std::vector<uint8_t> host;
  // a string per distinct id of the batch, copied to every place that asks for it
  TRY(strand_batches(c, ids, all_minus.data(), m, batch_caps(nullptr, MC_IDENT_BATCH_PAIRS, false), nullptr, [&](const StrandBatch &v) -> int {
    host.resize(v.rc_bytes);
    if (v.rc_bytes) MCG_CHECK(hipMemcpyAsync(host.data(), c->rc_seq.p, v.rc_bytes, hipMemcpyDeviceToHost, c->stream));
    MCG_CHECK(hipStreamSynchronize(c->stream));
    for (uint64_t i = v.i0; i < v.i1; i++)
      if (off[i + 1] > off[i]) memcpy(bytes + off[i], host.data() + v.a_off(i), off[i + 1] - off[i]);
    return MC_OK;
  }));
  flush_timers(c);
  return MC_OK;
}

int mc_nw_identity_strands(mc_ctx *c, const uint32_t *a, const uint32_t *b, const uint8_t *a_minus, uint64_t m,
                           double *ident, int32_t *len, int32_t *ids) {
  if (!c || !c->codes.p) return MC_ERR_STATE;
  if (m == 0) return MC_OK;
  MCG_CHECK(hipSetDevice(c->device));
  TRY(check_ids(c, a, m));
  TRY(check_ids(c, b, m));
  mc::PairBatcher pb(c->h_seq_off.data(), c->n, a, b, a_minus, m, batch_caps("MC_IDENT_BATCH", MC_IDENT_BATCH_PAIRS, false));
  std::vector<uint32_t> ai, bi, out;
  std::vector<uint64_t> h_off, a_off2, la[2], lb[2];
  while (pb.next()) {
    const uint64_t i0 = pb.i0, mb = pb.i1 - pb.i0, nm = pb.nminus, np = mb - nm;
    // the minus pairs first, then the plus pairs; every result goes to its pair's own slot
    ai.resize(mb);
    bi.resize(mb);
    out.resize(mb);
    for (int s = 0; s < 2; s++) {
      la[s].clear();
      lb[s].clear();
    }
    uint64_t km = 0, kp = nm;
    for (uint64_t i = i0; i < pb.i1; i++) {
      const bool minus = pb.minus(i);
      const uint64_t k = minus ? km++ : kp++;
      ai[k] = minus ? 2 * pb.slot(a[i]) : a[i];  // (the strings' offsets come in [start, end) pairs)
      bi[k] = b[i];
      out[k] = (uint32_t)(i - i0);
      la[minus].push_back(pb.length(a[i]));
      lb[minus].push_back(pb.length(b[i]));
    }
    if (nm) {
      TRY(revseq_batch(c, pb.uniq.data(), (uint32_t)pb.uniq.size(), h_off));
      a_off2.resize(2 * pb.uniq.size());
      for (size_t r = 0; r < pb.uniq.size(); r++) {
        a_off2[2 * r] = h_off[r];
        a_off2[2 * r + 1] = h_off[r] + pb.length(pb.uniq[r]);
      }
      TRY(upload(c, c->s_j, a_off2.data(), a_off2.size(), c->stream));
    }
    TRY(upload(c, c->s_d, ai.data(), mb, c->stream));
    TRY(upload(c, c->s_e, bi.data(), mb, c->stream));
    TRY(upload(c, c->s_g, out.data(), mb, c->stream));
    TRY(ensure(c->s_f, mb * 16 + 64));
    double *d_id = (double *)c->s_f.p;
    int32_t *d_len = (int32_t *)(d_id + mb), *d_ids = d_len + mb;
    const uint32_t *d_ai = (const uint32_t *)c->s_d.p, *d_bi = (const uint32_t *)c->s_e.p, *d_out = (const uint32_t *)c->s_g.p;
    if (nm)
      TRY(launch_nw(c, (uint8_t *)c->rc_seq.p, (uint64_t *)c->s_j.p, d_ai, (uint8_t *)c->codes.p, (uint64_t *)c->seq_off.p, d_bi,
                    nm, la[1], lb[1], d_id, d_len, d_ids, nullptr, d_out));
    if (np)
      TRY(launch_nw(c, (uint8_t *)c->codes.p, (uint64_t *)c->seq_off.p, d_ai + nm, (uint8_t *)c->codes.p,
                    (uint64_t *)c->seq_off.p, d_bi + nm, np, la[0], lb[0], d_id, d_len, d_ids, nullptr, d_out + nm));
    TRY(download_parts(c, {{ident ? ident + i0 : nullptr, d_id, mb * 8}, {len ? len + i0 : nullptr, d_len, mb * 4},
                           {ids ? ids + i0 : nullptr, d_ids, mb * 4}}, c->stream));
  }
  flush_timers(c);
  return MC_OK;
}

int mc_nw_align_strands(mc_ctx *c, const uint32_t *a, const uint32_t *b, const uint8_t *a_minus, uint64_t m,
                        uint32_t *cigar, uint64_t cap, uint64_t *cig_off, int32_t *score, int32_t *len, int32_t *ids) {
  if (!c || !c->codes.p) return MC_ERR_STATE;
  if (!cig_off) return MC_ERR_ARG;
  if (m == 0) {
    cig_off[0] = 0;
    return MC_OK;
  }
  if (!a || !b) return MC_ERR_ARG;
  MCG_CHECK(hipSetDevice(c->device));
  TRY(check_ids(c, a, m));
  TRY(check_ids(c, b, m));
  std::vector<int32_t> plan;
  TRY(align_plan(c, a, b, a_minus, m, plan));
  TRY(align_check_caps(c, "mc_nw_align_strands", a, b, m, plan));
  std::vector<uint32_t> words, nops(m);
  std::vector<uint64_t> dst;
  TRY(align_batches(c, "mc_nw_align_strands", a, b, a_minus, m, plan, [&](uint64_t i0, uint64_t mb, const std::vector<int32_t> &res) {
    scatter_res(res, i0, mb, score, len, ids);
    dst.resize(mb);
    uint64_t tot = 0;
    for (uint64_t k = 0; k < mb; k++) {
      dst[k] = tot;
      nops[i0 + k] = (uint32_t)res[k * TRACE_RES + 3];
      tot += nops[i0 + k];
    }
    if (cigar && tot) {  // the batch's words, packed on the device, kept until the whole count is known
      TRY(ensure(c->tr_out, tot * 4 + 64));
      TRY(upload(c, c->tr_dst, dst.data(), mb, c->stream));
      TRY(launch_nw_pack(c, (uint32_t)mb, (const TracePair *)c->tr_pairs.p, (const uint32_t *)c->tr_ops.p,
                         (const int32_t *)c->tr_res.p, (const uint64_t *)c->tr_dst.p, (uint32_t *)c->tr_out.p));
      const size_t at = words.size();
      words.resize(at + tot);
      MCG_CHECK(hipMemcpyAsync(words.data() + at, c->tr_out.p, tot * 4, hipMemcpyDeviceToHost, c->stream));
      MCG_CHECK(hipStreamSynchronize(c->stream));
    }
    return (int)MC_OK;
  }));
  flush_timers(c);
  cig_off[0] = 0;
  for (uint64_t i = 0; i < m; i++) cig_off[i + 1] = cig_off[i] + nops[i];
  if (cigar) {
    if (cap < cig_off[m]) {
      set_error("mc_nw_align_strands: cigar holds " + std::to_string(cap) + " words, the alignments have " +
                std::to_string(cig_off[m]));
      return MC_ERR_ARG;
    }
    if (!words.empty()) memcpy(cigar, words.data(), words.size() * 4);
  }
  return MC_OK;
}

int mc_nw_pileup_strands(mc_ctx *c, const uint32_t *a, const uint32_t *b, const uint8_t *a_minus, uint64_t m,
                         const uint32_t *targets, uint32_t nt, uint64_t *row_off, uint32_t *table, uint64_t cap_rows,
                         int32_t *score, int32_t *len, int32_t *ids) {
  return pileup_call(c, "mc_nw_pileup_strands", false, a, b, a_minus, m, targets, nt, row_off, table, nullptr, cap_rows, score, len,
                     ids);
}

int mc_nw_qpileup_strands(mc_ctx *c, const uint32_t *a, const uint32_t *b, const uint8_t *a_minus, uint64_t m,
                          const uint32_t *targets, uint32_t nt, uint64_t *row_off, uint32_t *table, uint32_t *wtable,
                          uint64_t cap_rows, int32_t *score, int32_t *len, int32_t *ids) {
  return pileup_call(c, "mc_nw_qpileup_strands", true, a, b, a_minus, m, targets, nt, row_off, table, wtable, cap_rows, score, len,
                     ids);
}

// A Phred value (0 .. MC_QUAL_MAX) per byte of the loaded sequences, at their offsets.
int mc_load_qualities(mc_ctx *c, const uint8_t *qual, uint64_t bytes) {
  if (!c || !c->codes.p) return MC_ERR_STATE;
  const uint64_t want = c->h_seq_off.empty() ? 0 : c->h_seq_off.back();
  if (bytes != want || (bytes && !qual)) {
    set_error("mc_load_qualities: " + std::to_string(bytes) + " values, the loaded sequences have " + std::to_string(want) + " bytes");
    return MC_ERR_ARG;
  }
  for (uint64_t i = 0; i < bytes; i++)
    if (qual[i] > MC_QUAL_MAX) {
      set_error("mc_load_qualities: value " + std::to_string((int)qual[i]) + " at byte " + std::to_string(i) + " is above MC_QUAL_MAX");
      return MC_ERR_ARG;
    }
  MCG_CHECK(hipSetDevice(c->device));
  TRY(ensure(c->qual, bytes + 64));
  if (bytes) MCG_CHECK(hipMemcpyAsync(c->qual.p, qual, bytes, hipMemcpyHostToDevice, c->stream));
  MCG_CHECK(hipStreamSynchronize(c->stream));
  c->has_qual = true;
  return MC_OK;
}

int mc_nw_align_profile(mc_ctx *c, double *out, int reset) {
  TRY(profile_families(c, out, reset, {F_NW_FWD, F_NW_TB}));
  out[2] = c->tr_choice_bytes;
  if (reset) c->tr_choice_bytes = 0;
  return MC_OK;
}

int mc_set_align_band(mc_ctx *c, int mode) {
  if (!c) return MC_ERR_ARG;
  if (mode != 0 && mode != 1) {
    set_error("mc_set_align_band: mode " + std::to_string(mode) + " (0: the full record, 1: the certified band)");
    return MC_ERR_ARG;
  }
  c->align_band = mode;
  return MC_OK;
}

int mc_nw_band_plan(mc_ctx *c, const uint32_t *a, const uint32_t *b, const uint8_t *a_minus, uint64_t m, int32_t *w, int32_t *score) {
  if (!c || !c->codes.p) return MC_ERR_STATE;
  if (m == 0) return MC_OK;
  if (!a || !b || !w || !score) return MC_ERR_ARG;
  MCG_CHECK(hipSetDevice(c->device));
  TRY(check_ids(c, a, m));
  TRY(check_ids(c, b, m));
  for (uint64_t i = 0; i < m; i++)
    if (pair_too_long(c, a[i], b[i])) {
      set_error("mc_nw_band_plan: pair " + std::to_string(i) + " has 2^27 bases or more");
      return MC_ERR_UNSUPPORTED;
    }
  return band_search(c, a, b, a_minus, m, w, score);
}

int mc_nw_band_profile(mc_ctx *c, double *out, int reset) {
  if (!out) return MC_ERR_ARG;
  TRY(profile_families(c, out + 3, reset, {F_NW_BAND}));
  for (int k = 0; k < 3; k++) out[k] = c->band_stat[k];
  out[4] = c->band_stat[3];
  if (reset)
    for (double &v : c->band_stat) v = 0;
  return MC_OK;
}

int mc_nw_pileup_profile(mc_ctx *c, double *out, int reset) { return profile_families(c, out, reset, {F_NW_FWD, F_NW_TB, F_NW_PU}); }

}  // extern "C"
