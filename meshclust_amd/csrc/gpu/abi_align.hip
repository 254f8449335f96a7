// abi_align.hip -- the alignment entries of include/meshclust_amd.h on lists of pairs that may sit
// on either strand: minus-strand strings, identities, alignments, pile-ups, multiple alignments and
// their profiles.
// Every list is cut into batches by host/pairbatch.hpp; as everywhere in libmcgpu the entries are
// synchronous and fail loudly.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../host/band.hpp"
#include "../host/pairbatch.hpp"
#include "abi_util.hpp"
#include "mcgpu.hpp"

using namespace mcg;

namespace {

// a batch's caps: pairs (lowered by `pairs_env`), string bytes (MC_IDENT_BYTES), choice scratch (MC_ALIGN_SCRATCH)
mc::PairBatchCaps batch_caps(const char *pairs_env, uint64_t pairs, bool scratch) {
  return {pairs_env ? env_cap(pairs_env, pairs) : pairs, env_cap("MC_IDENT_BYTES", MC_IDENT_BATCH_BYTES),
          scratch ? env_cap("MC_ALIGN_SCRATCH", MC_ALIGN_SCRATCH_BYTES) : 0};
}

// The minus-strand strings (host/revseq.hpp) of the u points ids into c->rc_seq, record r at
// h_off[r] (filled here: lengths rounded up to 16).  ids go through c->s_h, the offsets through
// c->s_i; the caller keeps ids and h_off alive until the stream is synchronized.
int revseq_batch(mc_ctx *c, const uint32_t *ids, uint32_t u, std::vector<uint64_t> &h_off) {
  h_off.resize((size_t)u + 1);
  h_off[0] = 0;
  for (uint32_t r = 0; r < u; r++)
    h_off[r + 1] = h_off[r] + (c->h_seq_off[ids[r] + 1] - c->h_seq_off[ids[r]] + 15) / 16 * 16;
  TRY(ensure(c->rc_seq, h_off[u] + 16));
  TRY(upload(c, c->s_h, ids, u, c->stream));
  TRY(upload(c, c->s_i, h_off.data(), (size_t)u + 1, c->stream));
  return launch_revseq(c, (const uint32_t *)c->s_h.p, u, (const uint64_t *)c->s_i.p, h_off[u], (uint8_t *)c->rc_seq.p);
}

// score, columns and identities of a batch's TRACE_RES ints per pair to the outputs that are wanted
void scatter_res(const std::vector<int32_t> &res, uint64_t i0, uint64_t mb, int32_t *score, int32_t *len, int32_t *ids) {
  for (uint64_t k = 0; k < mb; k++) {
    if (score) score[i0 + k] = res[k * TRACE_RES];
    if (len) len[i0 + k] = res[k * TRACE_RES + 1];
    if (ids) ids[i0 + k] = res[k * TRACE_RES + 2];
  }
}

// The width search of the certified band (host/band.hpp) over the pairs of a call,
// before its trace batches are planned: w[i] = pair i's planned width (-1: the full record),
// score[i] = its exact score.  The pairs go through the score-only kernel in mc_nw_identity_strands'
// batches (the pair cap, the minus-strand strings cap, the distinct minus reads reverse-complemented
// once).  Within a batch every pair starts at w0 and the uncertified ones are launched again at twice
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
  mc::PairBatcher pb(c->h_seq_off.data(), c->n, a, b, a_minus, m, batch_caps("MC_IDENT_BATCH", MC_IDENT_BATCH_PAIRS, false));
  std::vector<uint64_t> h_off, wcur;
  std::vector<TracePair> recs;
  std::vector<uint64_t> todo, next;
  std::vector<int32_t> sc;
  auto planned = [&](uint64_t i, int64_t la, int64_t lb, int32_t S) {
    score[i] = S;
    w[i] = mc::band_plan(la, lb, S);
    c->band_stat[w[i] >= 0 ? 0 : 1] += 1;
    if (w[i] >= 0) c->band_stat[3] += w[i];
  };
  while (pb.next()) {
    if (!pb.uniq.empty()) TRY(revseq_batch(c, pb.uniq.data(), (uint32_t)pb.uniq.size(), h_off));
    todo.clear();
    wcur.assign(pb.i1 - pb.i0, w0);
    for (uint64_t i = pb.i0; i < pb.i1; i++) {
      const int64_t la = (int64_t)pb.length(a[i]), lb = (int64_t)pb.length(b[i]);
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
          const uint64_t i = todo[end], la = pb.length(a[i]), lb = pb.length(b[i]);
          const uint64_t need = mc::band_bnd_ints(la, lb, wcur[i - pb.i0]);
          if (end > at && (bnd + need) * 4 > BAND_BND_BYTES) break;
          TracePair pr{};
          pr.a_off = pb.minus(i) ? h_off[pb.slot(a[i])] : c->h_seq_off[a[i]];
          pr.b_off = c->h_seq_off[b[i]];
          pr.bnd_off = bnd;
          pr.la = (uint32_t)la;
          pr.lb = (uint32_t)lb;
          pr.a_rc = pb.minus(i) ? 1 : 0;
          pr.r = mc::BAND_R;
          pr.w = (int32_t)wcur[i - pb.i0];
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
        const int64_t la = (int64_t)pb.length(a[i]), lb = (int64_t)pb.length(b[i]), wi = (int64_t)wcur[i - pb.i0];
        if (mc::band_certified(la, lb, wi, sc[k]) || mc::band_is_whole(la, lb, wi)) {
          planned(i, la, lb, sc[k]);
        } else {
          wcur[i - pb.i0] = (uint64_t)std::min<int64_t>(2 * wi, std::max(la, lb));
          next.push_back(i);
        }
      }
      todo.swap(next);
    }
  }
  flush_timers(c);
  return MC_OK;
}

// the plan of a call's pairs: empty with the band off (mc_set_align_band), else band_search's widths
int align_plan(mc_ctx *c, const uint32_t *a, const uint32_t *b, const uint8_t *a_minus, uint64_t m, std::vector<int32_t> &plan) {
  plan.clear();
  if (!c->align_band || m == 0) return MC_OK;
  plan.assign(m, -1);
  for (uint64_t i = 0; i < m; i++)  // (align_check_caps refuses the call)
    if ((c->h_seq_off[a[i] + 1] - c->h_seq_off[a[i]]) + (c->h_seq_off[b[i] + 1] - c->h_seq_off[b[i]]) >= (1ull << 27)) return MC_OK;
  std::vector<int32_t> score(m);
  return band_search(c, a, b, a_minus, m, plan.data(), score.data());
}

// the choice bytes of pair i under a plan (empty: the full record)
uint64_t planned_bytes(const std::vector<int32_t> &plan, uint64_t i, uint64_t la, uint64_t lb) {
  return !plan.empty() && plan[i] >= 0 ? mc::band_choice_bytes(la, lb, (uint64_t)plan[i]) : nw_trace_choice_bytes(la, lb);
}

// The pairs of mc_nw_align_strands / mc_nw_pileup_strands in batches: the forward pass and the
// traceback of every batch, then per_batch(i0, mb, res) with the batch's TRACE_RES ints per pair
// on the host; the batch's pair records, operation words and results are still in c->tr_pairs,
// c->tr_ops and c->tr_res, its minus-strand strings in c->rc_seq.  `who` names the caller in errors.
// plan: align_plan's; a pair's scratch is its planned bytes, banded or full.
int align_batches(mc_ctx *c, const char *who, const uint32_t *a, const uint32_t *b, const uint8_t *a_minus, uint64_t m,
                  const std::vector<int32_t> &plan,
                  const std::function<int(uint64_t, uint64_t, const std::vector<int32_t> &)> &per_batch) {
  mc::PairBatcher pb(c->h_seq_off.data(), c->n, a, b, a_minus, m, batch_caps("MC_ALIGN_BATCH", MC_ALIGN_BATCH_PAIRS, true),
                     nw_trace_choice_bytes);
  if (!plan.empty()) pb.scratch_at = [&](uint64_t i) { return planned_bytes(plan, i, pb.length(a[i]), pb.length(b[i])); };
  std::vector<uint64_t> h_off;
  std::vector<TracePair> pairs;
  std::vector<int32_t> res;
  TRY(ensure(c->tr_err, 256));
  while (pb.next()) {
    const uint64_t mb = pb.i1 - pb.i0;
    if (!pb.uniq.empty()) TRY(revseq_batch(c, pb.uniq.data(), (uint32_t)pb.uniq.size(), h_off));
    pairs.clear();
    uint64_t chb = 0, bnd = 0, opw = 0;
    for (uint64_t i = pb.i0; i < pb.i1; i++) {
      const uint64_t la = pb.length(a[i]), lb = pb.length(b[i]);
      TracePair pr;
      pr.a_off = pb.minus(i) ? h_off[pb.slot(a[i])] : c->h_seq_off[a[i]];
      pr.b_off = c->h_seq_off[b[i]];
      pr.ch_off = chb;
      pr.bnd_off = bnd;
      pr.ops_off = opw;
      pr.la = (uint32_t)la;
      pr.lb = (uint32_t)lb;
      pr.a_rc = pb.minus(i) ? 1 : 0;
      pr.w = plan.empty() ? -1 : plan[i];
      pr.r = pr.w >= 0 ? (uint32_t)mc::BAND_R : (uint32_t)nw_trace_rows(la);
      pairs.push_back(pr);
      chb += planned_bytes(plan, i, la, lb);
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
    TRY(per_batch(pb.i0, mb, res));
  }
  return MC_OK;
}

// before any trace launch, and before any output is written: a pair whose planned bytes alone exceed the scratch cap
int align_check_caps(mc_ctx *c, const char *who, const uint32_t *a, const uint32_t *b, uint64_t m, const std::vector<int32_t> &plan) {
  const uint64_t scr_cap = env_cap("MC_ALIGN_SCRATCH", MC_ALIGN_SCRATCH_BYTES);
  auto length = [&](uint32_t id) { return c->h_seq_off[id + 1] - c->h_seq_off[id]; };
  for (uint64_t i = 0; i < m; i++) {
    const uint64_t la = length(a[i]), lb = length(b[i]);
    if (la + lb >= (1ull << 27) || planned_bytes(plan, i, la, lb) > scr_cap) {
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
  TRY(check_ids(c, targets, nt));
  TRY(check_ids(c, a, m));
  TRY(check_ids(c, b, m));
  std::vector<uint32_t> tindex;  // point id -> its place among the targets
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
  std::vector<int32_t> plan;
  TRY(align_plan(c, a, b, a_minus, m, plan));
  TRY(align_check_caps(c, who.c_str(), a, b, m, plan));
  std::vector<uint64_t> toff(nt);
  row_off[0] = 0;
  for (uint32_t t = 0; t < nt; t++) {
    toff[t] = c->h_seq_off[targets[t]];
    row_off[t + 1] = row_off[t] + (c->h_seq_off[targets[t] + 1] - c->h_seq_off[targets[t]]) + 1;
  }
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
  TRY(upload(c, c->pu_toff, toff.data(), nt, c->stream));
  TRY(upload(c, c->pu_roff, row_off, (size_t)nt + 1, c->stream));
  TRY(launch_nw_pileup_finish(c, nt, (const uint64_t *)c->pu_toff.p, (const uint64_t *)c->pu_roff.p, d_table, d_deq, d_ddel));
  MCG_CHECK(hipMemcpyAsync(table, d_table, rows * MC_PILEUP_CH * 4, hipMemcpyDeviceToHost, c->stream));
  if (weighted) MCG_CHECK(hipMemcpyAsync(wtable, d_wtable, rows * MC_PILEUP_CH * 4, hipMemcpyDeviceToHost, c->stream));
  MCG_CHECK(hipStreamSynchronize(c->stream));
  flush_timers(c);
  return MC_OK;
}

// b grown to `bytes` with its first `keep` bytes kept (ensure() keeps nothing)
int grow_keep(mc_ctx *c, Buf &b, size_t bytes, size_t keep) {
  if (bytes <= b.bytes) return MC_OK;
  Buf nb;
  TRY(ensure(nb, std::max(bytes, 2 * b.bytes)));
  hipError_t e = keep ? hipMemcpyAsync(nb.p, b.p, keep, hipMemcpyDeviceToDevice, c->stream) : hipSuccess;
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);  // (no kernel still writes the old words)
  if (e != hipSuccess) {
    (void)hipFree(nb.p);
    return hip_fail(e, "grow_keep");
  }
  if (b.p) (void)hipFree(b.p);
  b = nb;
  return MC_OK;
}

// rows [s0, s1) of mc_nw_msa_rows' numbering, all centre rows or all pair rows, rendered in batches
// to out, one after the other
int msa_render_rows(mc_ctx *c, bool centre, uint64_t s0, uint64_t s1, uint8_t *out) {
  if (s0 >= s1) return MC_OK;
  const uint64_t nt = c->msa_targets.size(), base = centre ? s0 : s0 - nt;
  const uint32_t *ids = (centre ? c->msa_targets.data() : c->msa_a.data()) + base;
  const uint8_t *minus = centre || c->msa_minus.empty() ? nullptr : c->msa_minus.data() + base;
  auto target_of = [&](uint64_t i) { return centre ? base + i : (uint64_t)c->msa_tof[base + i]; };
  mc::PairBatcher pb(c->h_seq_off.data(), c->n, ids, nullptr, minus, s1 - s0,
                     {MC_IDENT_BATCH_PAIRS, env_cap("MC_IDENT_BYTES", MC_IDENT_BATCH_BYTES), env_cap("MC_MSA_BYTES", MC_MSA_BATCH_BYTES)});
  pb.scratch_at = [&](uint64_t i) { return c->msa_W[target_of(i)]; };
  std::vector<uint64_t> h_off;
  std::vector<MsaRow> recs;
  uint64_t done = 0;  // bytes of the rows before this batch
  while (pb.next()) {
    if (!pb.uniq.empty()) TRY(revseq_batch(c, pb.uniq.data(), (uint32_t)pb.uniq.size(), h_off));
    recs.clear();
    uint64_t bytes = 0;
    for (uint64_t i = pb.i0; i < pb.i1; i++) {
      const uint64_t t = target_of(i);
      MsaRow r{};
      r.out_off = bytes;
      r.row0 = c->msa_row_off[t];
      r.lb = (uint32_t)(c->msa_row_off[t + 1] - r.row0 - 1);
      r.W = (uint32_t)c->msa_W[t];
      if (centre) {
        r.a_off = c->h_seq_off[c->msa_targets[t]];
        r.la = r.lb;
        r.nw = 1;
        r.centre = 1;
      } else {
        const uint64_t p = base + i;
        r.a_off = pb.minus(i) ? h_off[pb.slot(ids[i])] : c->h_seq_off[ids[i]];
        r.la = (uint32_t)pb.length(ids[i]);
        r.nw = c->msa_nops[p];
        r.w_off = c->msa_woff[p];
        r.a_rc = pb.minus(i) ? 1 : 0;
      }
      recs.push_back(r);
      bytes += r.W;
    }
    if (bytes == 0) continue;
    TRY(ensure(c->msa_out, bytes + 64));
    TRY(upload(c, c->msa_rec, recs.data(), recs.size(), c->stream));
    TRY(launch_msa_render(c, recs.size(), (const MsaRow *)c->msa_rec.p, (const uint8_t *)c->rc_seq.p, (const uint32_t *)c->msa_words.p,
                          (const uint32_t *)c->msa_width.p, (const uint32_t *)c->msa_col.p, (uint8_t *)c->msa_out.p));
    uint8_t *h = nullptr;  // through the pinned landing buffer while it stays small, else straight to out
    if (bytes <= (64ull << 20)) TRY(download_pinned(c, c->msa_out.p, bytes, c->stream, &h));
    if (h) {
      memcpy(out + done, h, bytes);
    } else {
      MCG_CHECK(hipMemcpyAsync(out + done, c->msa_out.p, bytes, hipMemcpyDeviceToHost, c->stream));
      MCG_CHECK(hipStreamSynchronize(c->stream));
    }
    done += bytes;
  }
  return MC_OK;
}

}  // namespace

namespace mcg {

void msa_drop(mc_ctx *c) {
  c->msa_on = false;
  for (auto *v : {&c->msa_a, &c->msa_b, &c->msa_targets, &c->msa_tof, &c->msa_nops, &c->msa_tp}) std::vector<uint32_t>().swap(*v);
  for (auto *v : {&c->msa_woff, &c->msa_row_off, &c->msa_W, &c->msa_tp_off}) std::vector<uint64_t>().swap(*v);
  std::vector<uint8_t>().swap(c->msa_minus);
}

}  // namespace mcg

extern "C" {

int mc_nw_msa_begin(mc_ctx *c, const uint32_t *a, const uint32_t *b, const uint8_t *a_minus, uint64_t m, const uint32_t *targets,
                    uint32_t nt, uint64_t *row_off, uint32_t *width, uint64_t *block_width, int32_t *score, int32_t *len,
                    int32_t *ids) {
  if (c) msa_drop(c);
  if (!c || !c->codes.p) return MC_ERR_STATE;
  const std::string who = "mc_nw_msa_begin";
  if (!row_off || !block_width || (nt && !targets) || (m && (!a || !b))) return MC_ERR_ARG;
  MCG_CHECK(hipSetDevice(c->device));
  TRY(check_ids(c, targets, nt));
  TRY(check_ids(c, a, m));
  TRY(check_ids(c, b, m));
  std::vector<uint32_t> tindex;
  TRY(index_targets(c, who, targets, nt, b, m, tindex));
  std::vector<int32_t> plan;
  TRY(align_plan(c, a, b, a_minus, m, plan));
  TRY(align_check_caps(c, who.c_str(), a, b, m, plan));
  row_off[0] = 0;
  for (uint32_t t = 0; t < nt; t++) row_off[t + 1] = row_off[t] + (c->h_seq_off[targets[t] + 1] - c->h_seq_off[targets[t]]) + 1;
  const uint64_t rows = row_off[nt];
  // the widths stay on the device for the whole call: zeroed once, every batch max-es into them
  TRY(ensure(c->msa_width, rows * 4 + 64));
  TRY(ensure(c->msa_col, rows * 4 + 64));
  TRY(ensure(c->msa_bw, (uint64_t)nt * 8 + 64));
  uint32_t *d_width = (uint32_t *)c->msa_width.p;
  if (rows) MCG_CHECK(hipMemsetAsync(d_width, 0, rows * 4, c->stream));
  std::vector<uint32_t> nops(m), tof(m);
  std::vector<uint64_t> woff(m + 1, 0), dst, rowbase;
  uint64_t total = 0;  // operation words packed so far
  TRY(grow_keep(c, c->msa_words, 64, 0));
  TRY(align_batches(c, who.c_str(), a, b, a_minus, m, plan, [&](uint64_t i0, uint64_t mb, const std::vector<int32_t> &res) {
    scatter_res(res, i0, mb, score, len, ids);
    dst.resize(mb);
    rowbase.resize(mb);
    const uint64_t before = total;
    for (uint64_t k = 0; k < mb; k++) {
      tof[i0 + k] = tindex[b[i0 + k]];
      rowbase[k] = row_off[tof[i0 + k]];
      nops[i0 + k] = (uint32_t)res[k * TRACE_RES + 3];
      woff[i0 + k] = dst[k] = total;
      total += nops[i0 + k];
    }
    // the batch's words behind those of the batches before it, in the plan's own buffer
    TRY(grow_keep(c, c->msa_words, total * 4 + 64, before * 4));
    TRY(upload(c, c->tr_dst, dst.data(), mb, c->stream));
    TRY(upload(c, c->pu_rows, rowbase.data(), mb, c->stream));
    TRY(launch_nw_pack(c, (uint32_t)mb, (const TracePair *)c->tr_pairs.p, (const uint32_t *)c->tr_ops.p, (const int32_t *)c->tr_res.p,
                       (const uint64_t *)c->tr_dst.p, (uint32_t *)c->msa_words.p));
    return launch_msa_width(c, (uint32_t)mb, (const TracePair *)c->tr_pairs.p, (const uint32_t *)c->tr_ops.p,
                            (const int32_t *)c->tr_res.p, (const uint64_t *)c->pu_rows.p, d_width);
  }));
  woff[m] = total;
  if (nt) {
    TRY(upload(c, c->pu_roff, row_off, (size_t)nt + 1, c->stream));
    TRY(launch_msa_columns(c, nt, (const uint64_t *)c->pu_roff.p, d_width, (uint32_t *)c->msa_col.p, (uint64_t *)c->msa_bw.p));
    MCG_CHECK(hipMemcpyAsync(block_width, c->msa_bw.p, (size_t)nt * 8, hipMemcpyDeviceToHost, c->stream));
    if (width && rows) MCG_CHECK(hipMemcpyAsync(width, d_width, rows * 4, hipMemcpyDeviceToHost, c->stream));
  }
  MCG_CHECK(hipStreamSynchronize(c->stream));
  flush_timers(c);
  for (uint32_t t = 0; t < nt; t++)
    if (block_width[t] >= (1ull << 31)) {
      set_error(who + ": target " + std::to_string(targets[t]) + "'s block is " + std::to_string(block_width[t]) +
                " columns wide, the limit is 2^31 - 1");
      return MC_ERR_UNSUPPORTED;
    }
  c->msa_a.assign(a, a + m);
  c->msa_b.assign(b, b + m);
  if (a_minus) c->msa_minus.assign(a_minus, a_minus + m);
  c->msa_targets.assign(targets, targets + nt);
  c->msa_row_off.assign(row_off, row_off + nt + 1);
  c->msa_W.assign(block_width, block_width + nt);
  c->msa_tof.swap(tof);
  c->msa_nops.swap(nops);
  c->msa_woff.swap(woff);
  // every target's pairs in list order (mc_nw_msa_counts walks the plan by target)
  c->msa_tp_off.assign((size_t)nt + 1, 0);
  for (uint64_t i = 0; i < m; i++) c->msa_tp_off[c->msa_tof[i] + 1]++;
  for (uint32_t t = 0; t < nt; t++) c->msa_tp_off[t + 1] += c->msa_tp_off[t];
  c->msa_tp.resize(m);
  {
    std::vector<uint64_t> at(c->msa_tp_off.begin(), c->msa_tp_off.end() - 1);
    for (uint64_t i = 0; i < m; i++) c->msa_tp[at[c->msa_tof[i]]++] = (uint32_t)i;
  }
  c->msa_on = true;
  return MC_OK;
}

int mc_nw_msa_rows(mc_ctx *c, uint64_t first, uint64_t count, uint8_t *out, uint64_t cap, uint64_t *off) {
  if (!c || !c->codes.p || !c->msa_on) return MC_ERR_STATE;
  if (!off) return MC_ERR_ARG;
  const uint64_t nt = c->msa_targets.size(), all = nt + c->msa_a.size();
  if (first > all || count > all - first) {
    set_error("mc_nw_msa_rows: rows " + std::to_string(first) + " .. " + std::to_string(first) + " + " + std::to_string(count) +
              ", the plan has " + std::to_string(all));
    return MC_ERR_ARG;
  }
  off[0] = 0;
  for (uint64_t k = 0; k < count; k++) off[k + 1] = off[k] + c->msa_W[first + k < nt ? first + k : c->msa_tof[first + k - nt]];
  if (!out || count == 0) return MC_OK;
  if (cap < off[count]) {
    set_error("mc_nw_msa_rows: out holds " + std::to_string(cap) + " bytes, the rows have " + std::to_string(off[count]));
    return MC_ERR_ARG;
  }
  MCG_CHECK(hipSetDevice(c->device));
  const uint64_t end = first + count, mid = std::min(std::max(first, nt), end);  // centre rows [first, mid), pair rows [mid, end)
  TRY(msa_render_rows(c, true, first, mid, out));
  TRY(msa_render_rows(c, false, mid, end, out + off[mid - first]));
  flush_timers(c);
  return MC_OK;
}

int mc_nw_msa_counts(mc_ctx *c, uint32_t first, uint32_t ntg, uint64_t *col_off, uint32_t *counts, uint32_t *wcounts,
                     uint64_t cap_cols) {
  if (!c || !c->codes.p || !c->msa_on) return MC_ERR_STATE;
  const std::string who = "mc_nw_msa_counts";
  if (!col_off) return MC_ERR_ARG;
  const uint64_t nt = c->msa_targets.size();
  if (first > nt || ntg > nt - first) {
    set_error(who + ": targets " + std::to_string(first) + " .. " + std::to_string(first) + " + " + std::to_string(ntg) +
              ", the plan has " + std::to_string(nt));
    return MC_ERR_ARG;
  }
  if (wcounts && !counts) {
    set_error(who + ": wcounts is given with counts (both NULL: the offsets only)");
    return MC_ERR_ARG;
  }
  if (wcounts && !c->has_qual) {
    set_error(who + ": no qualities are loaded (mc_load_qualities)");
    return MC_ERR_STATE;
  }
  const uint64_t end = (uint64_t)first + ntg;
  if (wcounts)  // a column's weight is at most MC_QUAL_MAX per pair: the sums must fit 32 bits
    for (uint64_t t = first; t < end; t++)
      if (c->msa_tp_off[t + 1] - c->msa_tp_off[t] > 0xffffffffull / MC_QUAL_MAX) {
        set_error(who + ": target " + std::to_string(c->msa_targets[t]) + " has more than " +
                  std::to_string(0xffffffffull / MC_QUAL_MAX) + " pairs, its weights would not fit 32 bits");
        return MC_ERR_ARG;
      }
  col_off[0] = 0;
  for (uint64_t k = 0; k < ntg; k++) col_off[k + 1] = col_off[k] + c->msa_W[first + k];
  if (!counts || ntg == 0) return MC_OK;
  if (cap_cols < col_off[ntg]) {
    set_error(who + ": the tables hold " + std::to_string(cap_cols) + " columns, the targets have " + std::to_string(col_off[ntg]));
    return MC_ERR_ARG;
  }
  MCG_CHECK(hipSetDevice(c->device));
  const uint64_t col_bytes = (uint64_t)MC_MSA_CH * 4 * (wcounts ? 2 : 1), cap = env_cap("MC_MSA_BYTES", MC_MSA_BATCH_BYTES);
  const uint64_t ident_cap = env_cap("MC_IDENT_BYTES", MC_IDENT_BATCH_BYTES);
  std::vector<MsaCountTarget> tgts;
  std::vector<MsaCountPair> recs;
  std::vector<uint32_t> ids;
  std::vector<uint8_t> minus;
  std::vector<uint64_t> h_off;
  for (uint64_t t0 = first, t1; t0 < end; t0 = t1) {
    // a batch of targets: it ends before the target that would take its tables past the cap (a wider one is taken alone)
    uint64_t cols = 0;
    for (t1 = t0; t1 < end && (t1 == t0 || (cols + c->msa_W[t1]) * col_bytes <= cap); t1++) cols += c->msa_W[t1];
    if (cols == 0) continue;
    const uint64_t rows = c->msa_row_off[t1] - c->msa_row_off[t0];
    TRY(ensure(c->msa_cnt, cols * MC_MSA_CH * 4 + 64));
    TRY(ensure(c->msa_cdiff, rows * 8 + 64));
    uint32_t *d_cnt = (uint32_t *)c->msa_cnt.p, *d_wcnt = nullptr;
    int32_t *d_deq = (int32_t *)c->msa_cdiff.p, *d_ddel = d_deq + rows;
    MCG_CHECK(hipMemsetAsync(d_cnt, 0, cols * MC_MSA_CH * 4, c->stream));
    MCG_CHECK(hipMemsetAsync(d_deq, 0, rows * 8, c->stream));
    if (wcounts) {
      TRY(ensure(c->msa_wcnt, cols * MC_MSA_CH * 4 + 64));
      d_wcnt = (uint32_t *)c->msa_wcnt.p;
      MCG_CHECK(hipMemsetAsync(d_wcnt, 0, cols * MC_MSA_CH * 4, c->stream));
    }
    tgts.clear();
    for (uint64_t t = t0; t < t1; t++) {
      MsaCountTarget g{};
      g.c_off = c->h_seq_off[c->msa_targets[t]];
      g.row0 = c->msa_row_off[t];
      g.col0 = col_off[t - first] - col_off[t0 - first];
      g.drow0 = c->msa_row_off[t] - c->msa_row_off[t0];
      g.L = (uint32_t)(c->msa_row_off[t + 1] - g.row0 - 1);
      g.W = (uint32_t)c->msa_W[t];
      g.depth = (uint32_t)(c->msa_tp_off[t + 1] - c->msa_tp_off[t]);
      tgts.push_back(g);
    }
    // the batch's pairs, target by target; their minus-strand strings in batches as mc_nw_msa_rows'
    const uint32_t *pidx = c->msa_tp.data() + c->msa_tp_off[t0];
    const uint64_t np = c->msa_tp_off[t1] - c->msa_tp_off[t0];
    ids.resize(np);
    minus.resize(np);
    for (uint64_t i = 0; i < np; i++) {
      ids[i] = c->msa_a[pidx[i]];
      minus[i] = c->msa_minus.empty() ? 0 : c->msa_minus[pidx[i]];
    }
    mc::PairBatcher pb(c->h_seq_off.data(), c->n, ids.data(), nullptr, c->msa_minus.empty() ? nullptr : minus.data(), np,
                       {MC_IDENT_BATCH_PAIRS, ident_cap, 0});
    while (pb.next()) {
      if (!pb.uniq.empty()) TRY(revseq_batch(c, pb.uniq.data(), (uint32_t)pb.uniq.size(), h_off));
      recs.clear();
      for (uint64_t i = pb.i0; i < pb.i1; i++) {
        const uint64_t p = pidx[i];
        const MsaCountTarget &g = tgts[c->msa_tof[p] - t0];
        MsaCountPair r{};
        r.a_off = pb.minus(i) ? h_off[pb.slot(ids[i])] : c->h_seq_off[ids[i]];
        r.w_off = c->msa_woff[p];
        r.row0 = g.row0;
        r.col0 = g.col0;
        r.drow0 = g.drow0;
        r.q_off = c->h_seq_off[ids[i]];
        r.la = (uint32_t)pb.length(ids[i]);
        r.lb = g.L;
        r.nw = c->msa_nops[p];
        r.W = g.W;
        r.a_rc = pb.minus(i) ? 1 : 0;
        recs.push_back(r);
      }
      TRY(upload(c, c->msa_crec, recs.data(), recs.size(), c->stream));
      TRY(launch_msa_counts(c, recs.size(), (const MsaCountPair *)c->msa_crec.p, (const uint8_t *)c->rc_seq.p,
                            (const uint32_t *)c->msa_words.p, (const uint32_t *)c->msa_width.p, (const uint32_t *)c->msa_col.p, d_cnt,
                            d_wcnt, d_deq, d_ddel));
      MCG_CHECK(hipStreamSynchronize(c->stream));  // (the records and the strings' offsets are reused by the next batch)
    }
    TRY(upload(c, c->msa_ctgt, tgts.data(), tgts.size(), c->stream));
    TRY(launch_msa_counts_finish(c, (uint32_t)tgts.size(), (const MsaCountTarget *)c->msa_ctgt.p, (const uint32_t *)c->msa_width.p,
                                 (const uint32_t *)c->msa_col.p, d_cnt, d_deq, d_ddel));
    const uint64_t at = (col_off[t0 - first]) * MC_MSA_CH;
    MCG_CHECK(hipMemcpyAsync(counts + at, d_cnt, cols * MC_MSA_CH * 4, hipMemcpyDeviceToHost, c->stream));
    if (wcounts) MCG_CHECK(hipMemcpyAsync(wcounts + at, d_wcnt, cols * MC_MSA_CH * 4, hipMemcpyDeviceToHost, c->stream));
    MCG_CHECK(hipStreamSynchronize(c->stream));
  }
  flush_timers(c);
  return MC_OK;
}

int mc_nw_msa_counts_profile(mc_ctx *c, double *out, int reset) {
  if (!c || !out) return MC_ERR_ARG;
  (void)hipStreamSynchronize(c->stream);
  flush_timers(c);
  out[0] = c->fam_ms[F_NW_MSAC];
  if (reset) c->fam_ms[F_NW_MSAC] = c->fam_n[F_NW_MSAC] = 0;
  return MC_OK;
}

int mc_nw_msa_sites(mc_ctx *c, const uint64_t *site_off, const uint32_t *sites, uint64_t first, uint64_t count, uint8_t *alleles,
                    uint8_t *quals, uint64_t cap, uint64_t *off) {
  if (!c || !c->codes.p || !c->msa_on) return MC_ERR_STATE;
  const std::string who = "mc_nw_msa_sites";
  if (!off || !site_off) return MC_ERR_ARG;
  const uint64_t nt = c->msa_targets.size(), m = c->msa_a.size();
  if (first > m || count > m - first) {
    set_error(who + ": pairs " + std::to_string(first) + " .. " + std::to_string(first) + " + " + std::to_string(count) +
              ", the plan has " + std::to_string(m));
    return MC_ERR_ARG;
  }
  if (site_off[0] != 0) {
    set_error(who + ": site_off starts at " + std::to_string(site_off[0]) + ", not at 0");
    return MC_ERR_ARG;
  }
  for (uint64_t t = 0; t < nt; t++)
    if (site_off[t + 1] < site_off[t]) {
      set_error(who + ": site_off decreases at target " + std::to_string(c->msa_targets[t]));
      return MC_ERR_ARG;
    }
  const uint64_t nsites = site_off[nt];
  if (nsites && !sites) return MC_ERR_ARG;
  for (uint64_t t = 0; t < nt; t++)
    for (uint64_t s = site_off[t]; s < site_off[t + 1]; s++)
      if (sites[s] >= c->msa_W[t] || (s > site_off[t] && sites[s] <= sites[s - 1])) {
        set_error(who + ": site " + std::to_string(s - site_off[t]) + " of target " + std::to_string(c->msa_targets[t]) + ", column " +
                  std::to_string(sites[s]) + ": the sites of a target ascend strictly and stay below its " +
                  std::to_string(c->msa_W[t]) + " columns");
        return MC_ERR_ARG;
      }
  if (quals && !alleles) {
    set_error(who + ": quals is given with alleles (both NULL: the offsets only)");
    return MC_ERR_ARG;
  }
  if (quals && !c->has_qual) {
    set_error(who + ": no qualities are loaded (mc_load_qualities)");
    return MC_ERR_STATE;
  }
  auto nsite = [&](uint64_t p) { return site_off[c->msa_tof[p] + 1] - site_off[c->msa_tof[p]]; };  // S of pair p's target
  off[0] = 0;
  for (uint64_t k = 0; k < count; k++) off[k + 1] = off[k] + nsite(first + k);
  if (!alleles || count == 0) return MC_OK;
  if (cap < off[count]) {
    set_error(who + ": alleles holds " + std::to_string(cap) + " bytes, the pairs have " + std::to_string(off[count]));
    return MC_ERR_ARG;
  }
  if (off[count] == 0) return MC_OK;
  MCG_CHECK(hipSetDevice(c->device));
  // the sites of the targets these pairs have and what they resolve to: kept on the device for all of the
  // call's batches.  Only the span of the site list that those targets cover is uploaded, [lo, hi) -- for pairs
  // sorted by target, as the assignment tool's are, no more than they need; the device offsets count from lo.
  std::vector<uint8_t> used(nt, 0);
  for (uint64_t k = 0; k < count; k++) used[c->msa_tof[first + k]] = 1;
  std::vector<MsaSiteTarget> tgts;
  uint64_t lo = nsites, hi = 0;
  for (uint64_t t = 0; t < nt; t++)
    if (used[t] && site_off[t + 1] > site_off[t]) {
      lo = std::min(lo, site_off[t]);
      hi = std::max(hi, site_off[t + 1]);
    }
  for (uint64_t t = 0; t < nt; t++)
    if (used[t] && site_off[t + 1] > site_off[t])
      tgts.push_back({c->msa_row_off[t], site_off[t] - lo, (uint32_t)(c->msa_row_off[t + 1] - c->msa_row_off[t] - 1),
                      (uint32_t)(site_off[t + 1] - site_off[t])});
  TRY(upload(c, c->msa_scol, sites + lo, hi - lo, c->stream));
  TRY(upload(c, c->msa_stgt, tgts.data(), tgts.size(), c->stream));
  TRY(ensure(c->msa_sres, (hi - lo) * sizeof(uint2) + 64));
  TRY(launch_msa_sites_resolve(c, (uint32_t)tgts.size(), (const MsaSiteTarget *)c->msa_stgt.p, (const uint32_t *)c->msa_width.p,
                               (const uint32_t *)c->msa_col.p, (const uint32_t *)c->msa_scol.p, (uint2 *)c->msa_sres.p));
  const uint32_t *ids = c->msa_a.data() + first;
  const uint8_t *minus = c->msa_minus.empty() ? nullptr : c->msa_minus.data() + first;
  const uint64_t per = quals ? 2 : 1;  // output bytes per site
  mc::PairBatcher pb(c->h_seq_off.data(), c->n, ids, nullptr, minus, count,
                     {MC_IDENT_BATCH_PAIRS, env_cap("MC_IDENT_BYTES", MC_IDENT_BATCH_BYTES), env_cap("MC_MSA_BYTES", MC_MSA_BATCH_BYTES)});
  pb.scratch_at = [&](uint64_t i) { return per * nsite(first + i); };
  std::vector<uint64_t> h_off;
  std::vector<MsaSitePair> recs;
  auto fetch = [&](uint8_t *dst, const void *d, uint64_t bytes) {  // through the pinned landing buffer while it stays small
    uint8_t *h = nullptr;
    if (bytes <= (64ull << 20)) TRY(download_pinned(c, d, bytes, c->stream, &h));
    if (h) {
      memcpy(dst, h, bytes);
    } else {
      MCG_CHECK(hipMemcpyAsync(dst, d, bytes, hipMemcpyDeviceToHost, c->stream));
      MCG_CHECK(hipStreamSynchronize(c->stream));
    }
    return (int)MC_OK;
  };
  while (pb.next()) {
    const uint64_t bytes = off[pb.i1] - off[pb.i0];
    if (bytes == 0) continue;
    if (!pb.uniq.empty()) TRY(revseq_batch(c, pb.uniq.data(), (uint32_t)pb.uniq.size(), h_off));
    recs.clear();
    for (uint64_t i = pb.i0; i < pb.i1; i++) {
      const uint64_t p = first + i, t = c->msa_tof[p];
      MsaSitePair r{};
      r.a_off = pb.minus(i) ? h_off[pb.slot(ids[i])] : c->h_seq_off[ids[i]];
      r.w_off = c->msa_woff[p];
      r.row0 = c->msa_row_off[t];
      r.s_off = nsite(p) ? site_off[t] - lo : 0;
      r.out_off = off[i] - off[pb.i0];
      r.q_off = c->h_seq_off[ids[i]];
      r.la = (uint32_t)pb.length(ids[i]);
      r.lb = (uint32_t)(c->msa_row_off[t + 1] - r.row0 - 1);
      r.nw = c->msa_nops[p];
      r.S = (uint32_t)nsite(p);
      r.a_rc = pb.minus(i) ? 1 : 0;
      recs.push_back(r);
    }
    TRY(ensure(c->msa_sout, bytes + 64));
    MCG_CHECK(hipMemsetAsync(c->msa_sout.p, MC_MSA_GAP, bytes, c->stream));
    if (quals) {
      TRY(ensure(c->msa_sq, bytes + 64));
      MCG_CHECK(hipMemsetAsync(c->msa_sq.p, 0, bytes, c->stream));
    }
    TRY(upload(c, c->msa_srec, recs.data(), recs.size(), c->stream));
    TRY(launch_msa_sites(c, recs.size(), (const MsaSitePair *)c->msa_srec.p, (const uint8_t *)c->rc_seq.p, (const uint32_t *)c->msa_words.p,
                         (const uint32_t *)c->msa_width.p, (const uint32_t *)c->msa_col.p, (const uint32_t *)c->msa_scol.p,
                         (const uint2 *)c->msa_sres.p, (uint8_t *)c->msa_sout.p, quals ? (uint8_t *)c->msa_sq.p : nullptr));
    TRY(fetch(alleles + off[pb.i0], c->msa_sout.p, bytes));  // (synchronizes: the records and the strings are the next batch's)
    if (quals) TRY(fetch(quals + off[pb.i0], c->msa_sq.p, bytes));
  }
  MCG_CHECK(hipStreamSynchronize(c->stream));
  flush_timers(c);
  return MC_OK;
}

int mc_nw_msa_sites_profile(mc_ctx *c, double *out, int reset) {
  if (!c || !out) return MC_ERR_ARG;
  (void)hipStreamSynchronize(c->stream);
  flush_timers(c);
  out[0] = c->fam_ms[F_NW_MSAS];
  if (reset) c->fam_ms[F_NW_MSAS] = c->fam_n[F_NW_MSAS] = 0;
  return MC_OK;
}

int mc_nw_msa_crossover(mc_ctx *c, const uint64_t *x, const uint64_t *y, uint64_t nc, int32_t *out) {
  if (!c || !c->codes.p || !c->msa_on) return MC_ERR_STATE;
  if (nc == 0) return MC_OK;
  if (!x || !y || !out) return MC_ERR_ARG;
  const std::string who = "mc_nw_msa_crossover";
  const uint64_t m = c->msa_a.size();
  const uint64_t cap = env_cap("MC_CROSS_MAX", MC_CROSS_MAX_READ);
  auto length = [&](uint64_t p) { return c->h_seq_off[c->msa_a[p] + 1] - c->h_seq_off[c->msa_a[p]]; };
  for (uint64_t k = 0; k < nc; k++) {
    if (x[k] >= m || y[k] >= m) {
      set_error(who + ": candidate " + std::to_string(k) + " names pair " + std::to_string(std::max(x[k], y[k])) + ", the plan has " +
                std::to_string(m));
      return MC_ERR_ARG;
    }
    if (c->msa_a[x[k]] != c->msa_a[y[k]]) {
      set_error(who + ": candidate " + std::to_string(k) + ": pairs " + std::to_string(x[k]) + " and " + std::to_string(y[k]) +
                " align different reads");
      return MC_ERR_ARG;
    }
  }
  for (uint64_t k = 0; k < nc; k++)
    if (length(x[k]) > cap) {
      set_error(who + ": candidate " + std::to_string(k) + "'s read has " + std::to_string(length(x[k])) + " bases, the limit is " +
                std::to_string(cap));
      return MC_ERR_UNSUPPORTED;
    }
  MCG_CHECK(hipSetDevice(c->device));
  // A batch's candidates go by the size of their bitmaps: bucket g holds the reads of at most 1024 << g bases,
  // one launch per bucket in use with the LDS its own longest read needs.  Every record names its slot
  // of the batch's output, so the values come back in the caller's order.
  constexpr uint32_t NBUCKET = 9;  // 1024 << 8 = MC_CROSS_MAX_READ
  auto bucket = [](uint64_t la) {
    uint32_t g = 0;
    while (g + 1 < NBUCKET && la > (1024ull << g)) g++;
    return g;
  };
  const uint64_t per = env_cap("MC_CROSS_BATCH", MC_CROSS_BATCH_CANDS);
  std::vector<CrossPair> recs;
  std::vector<uint32_t> order;
  for (uint64_t i0 = 0; i0 < nc; i0 += per) {
    const uint64_t nb = std::min(per, nc - i0);
    uint64_t cnt[NBUCKET + 1] = {0};
    uint32_t longest[NBUCKET] = {0};
    for (uint64_t k = 0; k < nb; k++) {
      const uint64_t la = length(x[i0 + k]);
      const uint32_t g = bucket(la);
      cnt[g + 1]++;
      longest[g] = std::max(longest[g], (uint32_t)la);
    }
    for (uint32_t g = 0; g < NBUCKET; g++) cnt[g + 1] += cnt[g];
    recs.resize(nb);
    {
      uint64_t at[NBUCKET];
      for (uint32_t g = 0; g < NBUCKET; g++) at[g] = cnt[g];
      for (uint64_t k = 0; k < nb; k++) {
        const uint64_t px = x[i0 + k], py = y[i0 + k], la = length(px);
        CrossPair r{};
        r.xw_off = c->msa_woff[px];
        r.yw_off = c->msa_woff[py];
        r.la = (uint32_t)la;
        r.xnw = c->msa_nops[px];
        r.ynw = c->msa_nops[py];
        r.minus = c->msa_minus.empty() ? 0u : (c->msa_minus[px] ? 1u : 0u) | (c->msa_minus[py] ? 2u : 0u);
        r.out = (uint32_t)k;
        recs[at[bucket(la)]++] = r;
      }
    }
    TRY(upload(c, c->msa_xrec, recs.data(), recs.size(), c->stream));
    TRY(ensure(c->msa_xout, nb * MC_CROSS_RES * 4 + 64));
    for (uint32_t g = 0; g < NBUCKET; g++)
      TRY(launch_crossover(c, (uint32_t)(cnt[g + 1] - cnt[g]), (const CrossPair *)c->msa_xrec.p + cnt[g], (const uint32_t *)c->msa_words.p,
                           longest[g], (int32_t *)c->msa_xout.p));
    const uint64_t bytes = nb * MC_CROSS_RES * 4;
    uint8_t *h = nullptr;
    TRY(download_pinned(c, c->msa_xout.p, bytes, c->stream, &h));  // (synchronizes: the records are the next batch's)
    if (h) {
      memcpy(out + i0 * MC_CROSS_RES, h, bytes);
    } else {
      MCG_CHECK(hipMemcpyAsync(out + i0 * MC_CROSS_RES, c->msa_xout.p, bytes, hipMemcpyDeviceToHost, c->stream));
      MCG_CHECK(hipStreamSynchronize(c->stream));
    }
  }
  flush_timers(c);
  return MC_OK;
}

int mc_nw_msa_crossover_profile(mc_ctx *c, double *out, int reset) {
  if (!c || !out) return MC_ERR_ARG;
  (void)hipStreamSynchronize(c->stream);
  flush_timers(c);
  out[0] = c->fam_ms[F_NW_CROSS];
  if (reset) c->fam_ms[F_NW_CROSS] = c->fam_n[F_NW_CROSS] = 0;
  return MC_OK;
}

int mc_nw_msa_end(mc_ctx *c) {
  if (!c) return MC_ERR_ARG;
  msa_drop(c);
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  for (Buf *b : {&c->msa_width, &c->msa_col, &c->msa_words, &c->msa_bw, &c->msa_rec, &c->msa_out, &c->msa_cnt, &c->msa_wcnt,
                 &c->msa_cdiff, &c->msa_crec, &c->msa_ctgt, &c->msa_scol, &c->msa_sres, &c->msa_stgt, &c->msa_srec, &c->msa_sout,
                 &c->msa_sq, &c->msa_xrec, &c->msa_xout}) {
    if (b->p) (void)hipFree(b->p);
    *b = Buf{};
  }
  return MC_OK;
}

int mc_nw_msa_profile(mc_ctx *c, double *out, int reset) {
  if (!c || !out) return MC_ERR_ARG;
  (void)hipStreamSynchronize(c->stream);
  flush_timers(c);
  int k = 0;
  for (int f : {F_NW_FWD, F_NW_TB, F_NW_MSAW, F_NW_MSAR}) out[k++] = c->fam_ms[f];
  if (reset)
    for (int f : {F_NW_FWD, F_NW_TB, F_NW_MSAW, F_NW_MSAR}) c->fam_ms[f] = c->fam_n[f] = 0;
  return MC_OK;
}

int mc_revcomp_sequences(mc_ctx *c, const uint32_t *ids, uint64_t m, uint8_t *bytes, uint64_t *off) {
  if (!c || !c->codes.p) return MC_ERR_STATE;
  if (!off || (m && !ids)) return MC_ERR_ARG;
  TRY(check_ids(c, ids, m));
  off[0] = 0;
  for (uint64_t i = 0; i < m; i++) off[i + 1] = off[i] + (c->h_seq_off[ids[i] + 1] - c->h_seq_off[ids[i]]);
  if (!bytes || m == 0) return MC_OK;
  MCG_CHECK(hipSetDevice(c->device));
  const std::vector<uint8_t> all_minus(m, 1);
  mc::PairBatcher pb(c->h_seq_off.data(), c->n, ids, nullptr, all_minus.data(), m, batch_caps(nullptr, MC_IDENT_BATCH_PAIRS, false));
  std::vector<uint64_t> h_off;
  std::vector<uint8_t> host;
  while (pb.next()) {  // a string per distinct id of the batch, copied to every place that asks for it
    const uint32_t u = (uint32_t)pb.uniq.size();
    TRY(revseq_batch(c, pb.uniq.data(), u, h_off));
    host.resize(h_off[u]);
    if (h_off[u]) MCG_CHECK(hipMemcpyAsync(host.data(), c->rc_seq.p, h_off[u], hipMemcpyDeviceToHost, c->stream));
    MCG_CHECK(hipStreamSynchronize(c->stream));
    for (uint64_t i = pb.i0; i < pb.i1; i++)
      if (off[i + 1] > off[i]) memcpy(bytes + off[i], host.data() + h_off[pb.slot(ids[i])], off[i + 1] - off[i]);
  }
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
  if (!c || !out) return MC_ERR_ARG;
  (void)hipStreamSynchronize(c->stream);
  flush_timers(c);
  out[0] = c->fam_ms[F_NW_FWD];
  out[1] = c->fam_ms[F_NW_TB];
  out[2] = c->tr_choice_bytes;
  if (reset) {
    c->fam_ms[F_NW_FWD] = c->fam_ms[F_NW_TB] = c->fam_n[F_NW_FWD] = c->fam_n[F_NW_TB] = 0;
    c->tr_choice_bytes = 0;
  }
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
    if ((c->h_seq_off[a[i] + 1] - c->h_seq_off[a[i]]) + (c->h_seq_off[b[i] + 1] - c->h_seq_off[b[i]]) >= (1ull << 27)) {
      set_error("mc_nw_band_plan: pair " + std::to_string(i) + " has 2^27 bases or more");
      return MC_ERR_UNSUPPORTED;
    }
  return band_search(c, a, b, a_minus, m, w, score);
}

int mc_nw_band_profile(mc_ctx *c, double *out, int reset) {
  if (!c || !out) return MC_ERR_ARG;
  (void)hipStreamSynchronize(c->stream);
  flush_timers(c);
  out[0] = c->band_stat[0];
  out[1] = c->band_stat[1];
  out[2] = c->band_stat[2];
  out[3] = c->fam_ms[F_NW_BAND];
  out[4] = c->band_stat[3];
  if (reset) {
    c->fam_ms[F_NW_BAND] = c->fam_n[F_NW_BAND] = 0;
    for (double &v : c->band_stat) v = 0;
  }
  return MC_OK;
}

int mc_nw_pileup_profile(mc_ctx *c, double *out, int reset) {
  if (!c || !out) return MC_ERR_ARG;
  (void)hipStreamSynchronize(c->stream);
  flush_timers(c);
  out[0] = c->fam_ms[F_NW_FWD];
  out[1] = c->fam_ms[F_NW_TB];
  out[2] = c->fam_ms[F_NW_PU];
  if (reset)
    for (int f : {F_NW_FWD, F_NW_TB, F_NW_PU}) c->fam_ms[f] = c->fam_n[f] = 0;
  return MC_OK;
}

}  // extern "C"
