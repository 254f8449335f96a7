// abi_msa.hip -- the multiple-alignment entries of include/meshclust_amd.h: mc_nw_msa_begin's plan
// (MsaPlan, mcgpu.hpp) and its readers, the rows, the counts, the sites and the crossover values, with
// their profiles.  The alignments come from abi_align.hip's align_batches; every reader that needs
// the reads themselves walks them in strand_batches' batches (abi_util.hpp).  As everywhere in
// libmcgpu the entries are synchronous and fail loudly.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "abi_util.hpp"
#include "mcgpu.hpp"

using namespace mcg;

namespace {

constexpr size_t PINNED_MAX = 64ull << 20;  // rows and sites land in pinned memory up to this many bytes a batch

// the readers' batches: MC_IDENT_BATCH_PAIRS reads, MC_IDENT_BYTES of strings, MC_MSA_BYTES of output where it is counted
mc::PairBatchCaps msa_caps(bool scratch) {
  return {MC_IDENT_BATCH_PAIRS, env_cap("MC_IDENT_BYTES", MC_IDENT_BATCH_BYTES), scratch ? env_cap("MC_MSA_BYTES", MC_MSA_BATCH_BYTES) : 0};
}

// what MsaRow, MsaCountPair and MsaSitePair share: read i of batch v is pair p of the plan
template <typename R>
void fill_pair(R &r, const StrandBatch &v, uint64_t i, const MsaPlan &pl, uint64_t p) {
  const uint64_t t = pl.tof[p];
  r.a_off = v.a_off(i);
  r.w_off = pl.woff[p];
  r.row0 = pl.row_off[t];
  r.la = (uint32_t)v.la(i);
  r.lb = (uint32_t)pl.target_len(t);
  r.nw = pl.nops[p];
  r.a_rc = v.a_rc(i);
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
  MsaPlan &pl = c->msa;
  const uint64_t base = centre ? s0 : s0 - pl.ntargets();
  const uint32_t *ids = (centre ? pl.targets.data() : pl.a.data()) + base;
  const uint8_t *minus = centre || pl.a_minus.empty() ? nullptr : pl.a_minus.data() + base;
  std::vector<MsaRow> recs;
  uint64_t done = 0;  // bytes of the rows before this batch
  return strand_batches(c, ids, minus, s1 - s0, msa_caps(true), [&](uint64_t i) { return pl.row_width(s0 + i); }, [&](const StrandBatch &v) -> int {
    recs.clear();
    uint64_t bytes = 0;
    for (uint64_t i = v.i0; i < v.i1; i++) {
      MsaRow r{};
      r.out_off = bytes;
      r.W = (uint32_t)pl.row_width(s0 + i);
      if (centre) {  // (one '=' run of lb over the centre's own bytes)
        r.a_off = v.a_off(i);
        r.row0 = pl.row_off[base + i];
        r.la = r.lb = (uint32_t)pl.target_len(base + i);
        r.nw = 1;
        r.centre = 1;
      } else {
        fill_pair(r, v, i, pl, base + i);
      }
      recs.push_back(r);
      bytes += r.W;
    }
    if (bytes == 0) return MC_OK;
    TRY(ensure(pl.out, bytes + 64));
    TRY(upload(c, pl.rec, recs.data(), recs.size(), c->stream));
    TRY(launch_msa_render(c, recs.size(), (const MsaRow *)pl.rec.p, (const uint8_t *)c->rc_seq.p, (const uint32_t *)pl.words.p,
                          (const uint32_t *)pl.width.p, (const uint32_t *)pl.col.p, (uint8_t *)pl.out.p));
    TRY(download_to(c, out + done, pl.out.p, bytes, PINNED_MAX));  // (synchronizes: the records and the strings are the next batch's)
    done += bytes;
    return MC_OK;
  });
}

}  // namespace

void mcg::msa_drop(mc_ctx *c) { static_cast<MsaPlanHost &>(c->msa) = MsaPlanHost{}; }

extern "C" {

int mc_nw_msa_begin(mc_ctx *c, const uint32_t *a, const uint32_t *b, const uint8_t *a_minus, uint64_t m, const uint32_t *targets,
                    uint32_t nt, uint64_t *row_off, uint32_t *width, uint64_t *block_width, int32_t *score, int32_t *len,
                    int32_t *ids) {
  if (c) msa_drop(c);
  if (!c || !c->codes.p) return MC_ERR_STATE;
  const std::string who = "mc_nw_msa_begin";
  if (!row_off || !block_width || (nt && !targets) || (m && (!a || !b))) return MC_ERR_ARG;
  MCG_CHECK(hipSetDevice(c->device));
  MsaPlan &pl = c->msa;
  std::vector<uint32_t> tindex;
  std::vector<int32_t> plan;
  TRY(align_targets(c, who, false, a, b, a_minus, m, targets, nt, row_off, tindex, plan));
  const uint64_t rows = row_off[nt];
  // the widths stay on the device for the whole call: zeroed once, every batch max-es into them
  TRY(ensure(pl.width, rows * 4 + 64));
  TRY(ensure(pl.col, rows * 4 + 64));
  TRY(ensure(pl.bw, (uint64_t)nt * 8 + 64));
  uint32_t *d_width = (uint32_t *)pl.width.p;
  if (rows) MCG_CHECK(hipMemsetAsync(d_width, 0, rows * 4, c->stream));
  MsaPlanHost h;  // the plan to be: the context's only once everything below has succeeded
  h.nops.resize(m);
  h.tof.resize(m);
  h.woff.assign(m + 1, 0);
  std::vector<uint64_t> dst, rowbase;
  uint64_t total = 0;  // operation words packed so far
  TRY(grow_keep(c, pl.words, 64, 0));
  TRY(align_batches(c, who.c_str(), a, b, a_minus, m, plan, [&](uint64_t i0, uint64_t mb, const std::vector<int32_t> &res) {
    scatter_res(res, i0, mb, score, len, ids);
    dst.resize(mb);
    rowbase.resize(mb);
    const uint64_t before = total;
    for (uint64_t k = 0; k < mb; k++) {
      h.tof[i0 + k] = tindex[b[i0 + k]];
      rowbase[k] = row_off[h.tof[i0 + k]];
      h.nops[i0 + k] = (uint32_t)res[k * TRACE_RES + 3];
      h.woff[i0 + k] = dst[k] = total;
      total += h.nops[i0 + k];
    }
    // the batch's words behind those of the batches before it, in the plan's own buffer
    TRY(grow_keep(c, pl.words, total * 4 + 64, before * 4));
    TRY(upload(c, c->tr_dst, dst.data(), mb, c->stream));
    TRY(upload(c, c->pu_rows, rowbase.data(), mb, c->stream));
    TRY(launch_nw_pack(c, (uint32_t)mb, (const TracePair *)c->tr_pairs.p, (const uint32_t *)c->tr_ops.p, (const int32_t *)c->tr_res.p,
                       (const uint64_t *)c->tr_dst.p, (uint32_t *)pl.words.p));
    return launch_msa_width(c, (uint32_t)mb, (const TracePair *)c->tr_pairs.p, (const uint32_t *)c->tr_ops.p,
                            (const int32_t *)c->tr_res.p, (const uint64_t *)c->pu_rows.p, d_width);
  }));
  h.woff[m] = total;
  if (nt) {
    TRY(upload(c, c->pu_roff, row_off, (size_t)nt + 1, c->stream));
    TRY(launch_msa_columns(c, nt, (const uint64_t *)c->pu_roff.p, d_width, (uint32_t *)pl.col.p, (uint64_t *)pl.bw.p));
    MCG_CHECK(hipMemcpyAsync(block_width, pl.bw.p, (size_t)nt * 8, hipMemcpyDeviceToHost, c->stream));
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
  h.a.assign(a, a + m);
  h.b.assign(b, b + m);
  if (a_minus) h.a_minus.assign(a_minus, a_minus + m);
  h.targets.assign(targets, targets + nt);
  h.row_off.assign(row_off, row_off + nt + 1);
  h.W.assign(block_width, block_width + nt);
  // every target's pairs in list order (mc_nw_msa_counts walks the plan by target)
  h.tp_off.assign((size_t)nt + 1, 0);
  for (uint64_t i = 0; i < m; i++) h.tp_off[h.tof[i] + 1]++;
  for (uint32_t t = 0; t < nt; t++) h.tp_off[t + 1] += h.tp_off[t];
  h.tp.resize(m);
  {
    std::vector<uint64_t> at(h.tp_off.begin(), h.tp_off.end() - 1);
    for (uint64_t i = 0; i < m; i++) h.tp[at[h.tof[i]]++] = (uint32_t)i;
  }
  h.on = true;
  static_cast<MsaPlanHost &>(pl) = std::move(h);
  return MC_OK;
}

int mc_nw_msa_rows(mc_ctx *c, uint64_t first, uint64_t count, uint8_t *out, uint64_t cap, uint64_t *off) {
  if (!c || !c->codes.p || !c->msa.on) return MC_ERR_STATE;
  if (!off) return MC_ERR_ARG;
  const MsaPlan &pl = c->msa;
  const uint64_t nt = pl.ntargets(), all = nt + pl.npairs();
  if (first > all || count > all - first) {
    set_error("mc_nw_msa_rows: rows " + std::to_string(first) + " .. " + std::to_string(first) + " + " + std::to_string(count) +
              ", the plan has " + std::to_string(all));
    return MC_ERR_ARG;
  }
  off[0] = 0;
  for (uint64_t k = 0; k < count; k++) off[k + 1] = off[k] + pl.row_width(first + k);
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
  if (!c || !c->codes.p || !c->msa.on) return MC_ERR_STATE;
  const std::string who = "mc_nw_msa_counts";
  if (!col_off) return MC_ERR_ARG;
  MsaPlan &pl = c->msa;
  const uint64_t nt = pl.ntargets();
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
      if (pl.tp_off[t + 1] - pl.tp_off[t] > 0xffffffffull / MC_QUAL_MAX) {
        set_error(who + ": target " + std::to_string(pl.targets[t]) + " has more than " +
                  std::to_string(0xffffffffull / MC_QUAL_MAX) + " pairs, its weights would not fit 32 bits");
        return MC_ERR_ARG;
      }
  col_off[0] = 0;
  for (uint64_t k = 0; k < ntg; k++) col_off[k + 1] = col_off[k] + pl.W[first + k];
  if (!counts || ntg == 0) return MC_OK;
  if (cap_cols < col_off[ntg]) {
    set_error(who + ": the tables hold " + std::to_string(cap_cols) + " columns, the targets have " + std::to_string(col_off[ntg]));
    return MC_ERR_ARG;
  }
  MCG_CHECK(hipSetDevice(c->device));
  const uint64_t col_bytes = (uint64_t)MC_MSA_CH * 4 * (wcounts ? 2 : 1), cap = env_cap("MC_MSA_BYTES", MC_MSA_BATCH_BYTES);
  std::vector<MsaCountTarget> tgts;
  std::vector<MsaCountPair> recs;
  std::vector<uint32_t> ids;
  std::vector<uint8_t> minus;
  for (uint64_t t0 = first, t1; t0 < end; t0 = t1) {
    // a batch of targets: it ends before the target that would take its tables past the cap (a wider one is taken alone)
    uint64_t cols = 0;
    for (t1 = t0; t1 < end && (t1 == t0 || (cols + pl.W[t1]) * col_bytes <= cap); t1++) cols += pl.W[t1];
    if (cols == 0) continue;
    const uint64_t rows = pl.row_off[t1] - pl.row_off[t0];
    TRY(ensure(pl.cnt, cols * MC_MSA_CH * 4 + 64));
    TRY(ensure(pl.cdiff, rows * 8 + 64));
    uint32_t *d_cnt = (uint32_t *)pl.cnt.p, *d_wcnt = nullptr;
    int32_t *d_deq = (int32_t *)pl.cdiff.p, *d_ddel = d_deq + rows;
    MCG_CHECK(hipMemsetAsync(d_cnt, 0, cols * MC_MSA_CH * 4, c->stream));
    MCG_CHECK(hipMemsetAsync(d_deq, 0, rows * 8, c->stream));
    if (wcounts) {
      TRY(ensure(pl.wcnt, cols * MC_MSA_CH * 4 + 64));
      d_wcnt = (uint32_t *)pl.wcnt.p;
      MCG_CHECK(hipMemsetAsync(d_wcnt, 0, cols * MC_MSA_CH * 4, c->stream));
    }
    tgts.clear();
    for (uint64_t t = t0; t < t1; t++) {
      MsaCountTarget g{};
      g.c_off = c->h_seq_off[pl.targets[t]];
      g.row0 = pl.row_off[t];
      g.col0 = col_off[t - first] - col_off[t0 - first];
      g.drow0 = pl.row_off[t] - pl.row_off[t0];
      g.L = (uint32_t)pl.target_len(t);
      g.W = (uint32_t)pl.W[t];
      g.depth = (uint32_t)(pl.tp_off[t + 1] - pl.tp_off[t]);
      tgts.push_back(g);
    }
    // the batch's pairs, target by target; their minus-strand strings in batches as mc_nw_msa_rows'
    const uint32_t *pidx = pl.tp.data() + pl.tp_off[t0];
    const uint64_t np = pl.tp_off[t1] - pl.tp_off[t0];
    ids.resize(np);
    minus.resize(np);
    for (uint64_t i = 0; i < np; i++) {
      ids[i] = pl.a[pidx[i]];
      minus[i] = pl.minus(pidx[i]);
    }
    TRY(strand_batches(c, ids.data(), pl.a_minus.empty() ? nullptr : minus.data(), np, msa_caps(false), nullptr, [&](const StrandBatch &v) -> int {
      recs.clear();
      for (uint64_t i = v.i0; i < v.i1; i++) {
        const MsaCountTarget &g = tgts[pl.tof[pidx[i]] - t0];
        MsaCountPair r{};
        fill_pair(r, v, i, pl, pidx[i]);
        r.col0 = g.col0;
        r.drow0 = g.drow0;
        r.q_off = c->h_seq_off[ids[i]];
        r.W = g.W;
        recs.push_back(r);
      }
      TRY(upload(c, pl.crec, recs.data(), recs.size(), c->stream));
      TRY(launch_msa_counts(c, recs.size(), (const MsaCountPair *)pl.crec.p, (const uint8_t *)c->rc_seq.p,
                            (const uint32_t *)pl.words.p, (const uint32_t *)pl.width.p, (const uint32_t *)pl.col.p, d_cnt,
                            d_wcnt, d_deq, d_ddel));
      MCG_CHECK(hipStreamSynchronize(c->stream));  // (the records and the strings' offsets are reused by the next batch)
      return MC_OK;
    }));
    TRY(upload(c, pl.ctgt, tgts.data(), tgts.size(), c->stream));
    TRY(launch_msa_counts_finish(c, (uint32_t)tgts.size(), (const MsaCountTarget *)pl.ctgt.p, (const uint32_t *)pl.width.p,
                                 (const uint32_t *)pl.col.p, d_cnt, d_deq, d_ddel));
    const uint64_t at = (col_off[t0 - first]) * MC_MSA_CH;
    MCG_CHECK(hipMemcpyAsync(counts + at, d_cnt, cols * MC_MSA_CH * 4, hipMemcpyDeviceToHost, c->stream));
    if (wcounts) MCG_CHECK(hipMemcpyAsync(wcounts + at, d_wcnt, cols * MC_MSA_CH * 4, hipMemcpyDeviceToHost, c->stream));
    MCG_CHECK(hipStreamSynchronize(c->stream));
  }
  flush_timers(c);
  return MC_OK;
}

int mc_nw_msa_counts_profile(mc_ctx *c, double *out, int reset) { return profile_families(c, out, reset, {F_NW_MSAC}); }

int mc_nw_msa_sites(mc_ctx *c, const uint64_t *site_off, const uint32_t *sites, uint64_t first, uint64_t count, uint8_t *alleles,
                    uint8_t *quals, uint64_t cap, uint64_t *off) {
  if (!c || !c->codes.p || !c->msa.on) return MC_ERR_STATE;
  const std::string who = "mc_nw_msa_sites";
  if (!off || !site_off) return MC_ERR_ARG;
  MsaPlan &pl = c->msa;
  const uint64_t nt = pl.ntargets(), m = pl.npairs();
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
      set_error(who + ": site_off decreases at target " + std::to_string(pl.targets[t]));
      return MC_ERR_ARG;
    }
  const uint64_t nsites = site_off[nt];
  if (nsites && !sites) return MC_ERR_ARG;
  for (uint64_t t = 0; t < nt; t++)
    for (uint64_t s = site_off[t]; s < site_off[t + 1]; s++)
      if (sites[s] >= pl.W[t] || (s > site_off[t] && sites[s] <= sites[s - 1])) {
        set_error(who + ": site " + std::to_string(s - site_off[t]) + " of target " + std::to_string(pl.targets[t]) + ", column " +
                  std::to_string(sites[s]) + ": the sites of a target ascend strictly and stay below its " +
                  std::to_string(pl.W[t]) + " columns");
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
  auto nsite = [&](uint64_t p) { return site_off[pl.tof[p] + 1] - site_off[pl.tof[p]]; };  // S of pair p's target
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
  for (uint64_t k = 0; k < count; k++) used[pl.tof[first + k]] = 1;
  std::vector<MsaSiteTarget> tgts;
  uint64_t lo = nsites, hi = 0;
  for (uint64_t t = 0; t < nt; t++)
    if (used[t] && site_off[t + 1] > site_off[t]) {
      lo = std::min(lo, site_off[t]);
      hi = std::max(hi, site_off[t + 1]);
    }
  for (uint64_t t = 0; t < nt; t++)
    if (used[t] && site_off[t + 1] > site_off[t])
      tgts.push_back({pl.row_off[t], site_off[t] - lo, (uint32_t)pl.target_len(t), (uint32_t)(site_off[t + 1] - site_off[t])});
  TRY(upload(c, pl.scol, sites + lo, hi - lo, c->stream));
  TRY(upload(c, pl.stgt, tgts.data(), tgts.size(), c->stream));
  TRY(ensure(pl.sres, (hi - lo) * sizeof(uint2) + 64));
  TRY(launch_msa_sites_resolve(c, (uint32_t)tgts.size(), (const MsaSiteTarget *)pl.stgt.p, (const uint32_t *)pl.width.p,
                               (const uint32_t *)pl.col.p, (const uint32_t *)pl.scol.p, (uint2 *)pl.sres.p));
  const uint32_t *ids = pl.a.data() + first;
  const uint8_t *minus = pl.a_minus.empty() ? nullptr : pl.a_minus.data() + first;
  const uint64_t per = quals ? 2 : 1;  // output bytes per site
  std::vector<MsaSitePair> recs;
  auto batch = [&](const StrandBatch &v) -> int {
    const uint64_t bytes = off[v.i1] - off[v.i0];
    recs.clear();
    for (uint64_t i = v.i0; i < v.i1; i++) {
      const uint64_t p = first + i;
      MsaSitePair r{};
      fill_pair(r, v, i, pl, p);
      r.s_off = nsite(p) ? site_off[pl.tof[p]] - lo : 0;
      r.out_off = off[i] - off[v.i0];
      r.q_off = c->h_seq_off[ids[i]];
      r.S = (uint32_t)nsite(p);
      recs.push_back(r);
    }
    TRY(ensure(pl.sout, bytes + 64));
    MCG_CHECK(hipMemsetAsync(pl.sout.p, MC_MSA_GAP, bytes, c->stream));
    if (quals) {
      TRY(ensure(pl.sq, bytes + 64));
      MCG_CHECK(hipMemsetAsync(pl.sq.p, 0, bytes, c->stream));
    }
    TRY(upload(c, pl.srec, recs.data(), recs.size(), c->stream));
    TRY(launch_msa_sites(c, recs.size(), (const MsaSitePair *)pl.srec.p, (const uint8_t *)c->rc_seq.p, (const uint32_t *)pl.words.p,
                         (const uint32_t *)pl.width.p, (const uint32_t *)pl.col.p, (const uint32_t *)pl.scol.p,
                         (const uint2 *)pl.sres.p, (uint8_t *)pl.sout.p, quals ? (uint8_t *)pl.sq.p : nullptr));
    TRY(download_to(c, alleles + off[v.i0], pl.sout.p, bytes, PINNED_MAX));  // (synchronizes: the records and the strings are the next batch's)
    if (quals) TRY(download_to(c, quals + off[v.i0], pl.sq.p, bytes, PINNED_MAX));
    return MC_OK;
  };
  // (a batch without a site is skipped before its reverse complement)
  TRY(strand_batches(c, ids, minus, count, msa_caps(true), [&](uint64_t i) { return per * nsite(first + i); }, batch,
                     [&](uint64_t i0, uint64_t i1) { return off[i1] > off[i0]; }));
  MCG_CHECK(hipStreamSynchronize(c->stream));
  flush_timers(c);
  return MC_OK;
}

int mc_nw_msa_sites_profile(mc_ctx *c, double *out, int reset) { return profile_families(c, out, reset, {F_NW_MSAS}); }

int mc_nw_msa_crossover(mc_ctx *c, const uint64_t *x, const uint64_t *y, uint64_t nc, int32_t *out) {
  if (!c || !c->codes.p || !c->msa.on) return MC_ERR_STATE;
  if (nc == 0) return MC_OK;
  if (!x || !y || !out) return MC_ERR_ARG;
  const std::string who = "mc_nw_msa_crossover";
  MsaPlan &pl = c->msa;
  const uint64_t m = pl.npairs();
  const uint64_t cap = env_cap("MC_CROSS_MAX", MC_CROSS_MAX_READ);
  for (uint64_t k = 0; k < nc; k++) {
    if (x[k] >= m || y[k] >= m) {
      set_error(who + ": candidate " + std::to_string(k) + " names pair " + std::to_string(std::max(x[k], y[k])) + ", the plan has " +
                std::to_string(m));
      return MC_ERR_ARG;
    }
    if (pl.a[x[k]] != pl.a[y[k]]) {
      set_error(who + ": candidate " + std::to_string(k) + ": pairs " + std::to_string(x[k]) + " and " + std::to_string(y[k]) +
                " align different reads");
      return MC_ERR_ARG;
    }
  }
  for (uint64_t k = 0; k < nc; k++)
    if (seq_len(c, pl.a[x[k]]) > cap) {
      set_error(who + ": candidate " + std::to_string(k) + "'s read has " + std::to_string(seq_len(c, pl.a[x[k]])) + " bases, the limit is " +
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
      const uint64_t la = seq_len(c, pl.a[x[i0 + k]]);
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
        const uint64_t px = x[i0 + k], py = y[i0 + k], la = seq_len(c, pl.a[px]);
        CrossPair r{};
        r.xw_off = pl.woff[px];
        r.yw_off = pl.woff[py];
        r.la = (uint32_t)la;
        r.xnw = pl.nops[px];
        r.ynw = pl.nops[py];
        r.minus = (pl.minus(px) ? 1u : 0u) | (pl.minus(py) ? 2u : 0u);
        r.out = (uint32_t)k;
        recs[at[bucket(la)]++] = r;
      }
    }
    TRY(upload(c, pl.xrec, recs.data(), recs.size(), c->stream));
    TRY(ensure(pl.xout, nb * MC_CROSS_RES * 4 + 64));
    for (uint32_t g = 0; g < NBUCKET; g++)
      TRY(launch_crossover(c, (uint32_t)(cnt[g + 1] - cnt[g]), (const CrossPair *)pl.xrec.p + cnt[g], (const uint32_t *)pl.words.p,
                           longest[g], (int32_t *)pl.xout.p));
    TRY(download_to(c, out + i0 * MC_CROSS_RES, pl.xout.p, nb * MC_CROSS_RES * 4));  // (synchronizes: the records are the next batch's)
  }
  flush_timers(c);
  return MC_OK;
}

int mc_nw_msa_crossover_profile(mc_ctx *c, double *out, int reset) { return profile_families(c, out, reset, {F_NW_CROSS}); }

int mc_nw_msa_end(mc_ctx *c) {
  if (!c) return MC_ERR_ARG;
  msa_drop(c);
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  for (Buf *b : c->msa.bufs()) {
    if (b->p) (void)hipFree(b->p);
    *b = Buf{};
  }
  return MC_OK;
}

int mc_nw_msa_profile(mc_ctx *c, double *out, int reset) { return profile_families(c, out, reset, {F_NW_FWD, F_NW_TB, F_NW_MSAW, F_NW_MSAR}); }

}  // extern "C"
