// pileup.hip -- the alignments of nwtrace.hip reduced per centre column (mc_nw_pileup_strands,
// DESIGN.md 3.8): a table of MC_PILEUP_CH counters per row, L + 1 rows for a centre of L bytes.
//
// nwt_pileup_kernel: one wavefront per pair, after the batch's traceback.  It reads the pair's
// operation words (run << 4 | op, the last res[3] words of its region of la + lb) 64 at a time; a
// wave prefix sum over the runs gives every run the read position i and the centre column j it
// starts at ('=', 'X', 'I' consume a read base, '=', 'X', 'D' a centre base), the totals of a chunk
// carried into the next.  Per run:
//   '=' of n at column j   +1 at j and -1 at j + n of the centre's '=' difference array: two
//                          atomics for the run, whatever its length
//   'D' of n at column j   the same on the 'D' difference array
//   'X' of n at column j   per column the read's byte x (from the minus-strand buffer for a minus
//                          pair), one atomic on channel x <= 3 ? x : 4 of row j + t
//   'I' of n at column j   row j: channel 6 += 1, channel 7 += n
// A lane walks an 'X' run of at most SPREAD columns itself; longer ones are taken one after the
// other by the whole wave, 64 columns at a time.  Every loop's trip count is known on entry and
// nothing waits for another workgroup.  A pair whose traceback failed has res[3] == 0 and adds
// nothing.  A run that would leave the pair's strings (the words of a sound traceback never do)
// is skipped, so no address outside the centre's rows is formed.
//
// nwt_pileup_finish_kernel: once per call, a wavefront per target.  The running sums of the two
// difference arrays over rows 0 .. L - 1 are the '=' and 'D' coverage of each column; the first is
// added to the channel of the centre's own byte, the second to channel 5.  (Entry L only ever
// receives closing -1s; row L has no '=' or 'D'.)
//
// The atomics are plain atomicAdd on 32-bit integers in global memory; integer sums do not depend
// on the order of the pairs or on how they were batched.
#include "mcgpu.hpp"

namespace mcg {

namespace {

constexpr uint32_t SPREAD = 8;  // per-column runs longer than this are shared by the wave

struct PileArgs {
  const uint8_t *codes;  // the loaded sequences
  const uint8_t *rc;     // the batch's minus-strand strings
  const TracePair *pairs;
  const int32_t *res;  // TRACE_RES ints per pair
  const uint32_t *ops;
  const uint64_t *rowbase;  // per pair: the first row of its centre
  uint32_t *table;
  int32_t *deq, *ddel;
  uint32_t npairs;
  // the weighted kernel only (null elsewhere, and never read)
  const uint8_t *qual;   // the loaded qualities, at the sequences' offsets
  const uint64_t *qoff;  // per pair: the offset of its read (as loaded, whatever the strand)
  uint32_t *wtable;
};

__device__ __forceinline__ uint32_t wave_scan(uint32_t v, int lane) {  // inclusive prefix sum over the wave
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t u = (uint32_t)__shfl_up((int)v, d, 64);
    if (lane >= d) v += u;
  }
  return v;
}

__device__ __forceinline__ uint32_t base_channel(uint8_t x) { return x <= 3 ? x : 4u; }

__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, d, 64));
  return v;
}

// NAIVE: every column of an '=' or 'D' run gets its own atomic too (the form the difference arrays
// are measured against; the same table).
//
// WEIGHTED: the pile-up with quality weights (mc_nw_qpileup_strands).  The same
// counts (the same difference arrays, per-column atomics and finish kernel) and, beside them, a
// second table of the same shape that receives the read's Phred values.  Qs(i), the quality of base
// i of seq1 as aligned, is qual[qoff + i] of a plus pair and qual[qoff + la - 1 - i] of a minus
// pair: an index, the qualities are never reversed in memory.
//   '=' / 'X' at (i, j)   wtable[j + t][channel of a[i + t]] += Qs(i + t) for every column of the run
//   'D' of n at (i, j)    channel 5 of rows j .. j + n - 1 += min(Qs(i - 1) if i > 0, Qs(i) if i < la)
//   'I' of n at (i, j)    channel 6 of row j += min Qs(i .. i + n - 1)
// Every column carries its own value, so no difference array serves: a lane walks a run of at most
// SPREAD columns itself, longer runs are taken one after the other by the whole wave, 64 columns
// (consecutive quality bytes, consecutive rows) per step; a long 'I' run's minimum is a wave
// minimum.  A zero weight issues no atomic.  (There is no naive weighted form.)
template <bool NAIVE, bool WEIGHTED>
__global__ __launch_bounds__(64) void nwt_pileup_kernel(PileArgs q) {
  static_assert(!(NAIVE && WEIGHTED), "the naive form has no weights");
  const uint32_t p = blockIdx.x;
  if (p >= q.npairs) return;
  const TracePair pr = q.pairs[p];
  const uint32_t nw = (uint32_t)q.res[(uint64_t)p * TRACE_RES + 3], cap = pr.la + pr.lb;
  if (nw == 0 || nw > cap) return;
  const uint8_t *a = (pr.a_rc ? q.rc : q.codes) + pr.a_off;
  const uint8_t *ql = WEIGHTED ? q.qual + q.qoff[p] : nullptr;
  const uint32_t la = pr.la;
  const bool rc = pr.a_rc != 0;
  auto Qs = [&](uint32_t i) -> uint32_t { return ql[rc ? la - 1 - i : i]; };  // i < la
  auto gapq = [&](uint32_t i) -> uint32_t {  // the weight of a 'D' run with i read bases before it
    uint32_t v = 0xffffffffu;
    if (i > 0) v = Qs(i - 1);
    if (i < la) v = min(v, Qs(i));
    return v == 0xffffffffu ? 0u : v;
  };
  const uint32_t *src = q.ops + pr.ops_off + (cap - nw);
  const uint64_t row0 = q.rowbase[p];
  uint32_t *tab = q.table + row0 * MC_PILEUP_CH, *wt = WEIGHTED ? q.wtable + row0 * MC_PILEUP_CH : nullptr;
  int32_t *deq = q.deq + row0, *ddel = q.ddel + row0;
  const int lane = (int)threadIdx.x;
  uint32_t ci = 0, cj = 0;  // bases consumed before this chunk
  const uint32_t nchunk = (nw + 63) / 64;
  for (uint32_t c = 0; c < nchunk; c++) {
    const uint32_t k = c * 64 + (uint32_t)lane;
    const uint32_t w = k < nw ? src[k] : 0u;
    const uint32_t n = w >> 4, op = w & 15u;
    const bool both = op == MC_CIGAR_EQ || op == MC_CIGAR_X;
    const uint32_t di = both || op == MC_CIGAR_I ? n : 0u, dj = both || op == MC_CIGAR_D ? n : 0u;
    const uint32_t si = wave_scan(di, lane), sj = wave_scan(dj, lane);
    const uint32_t i0 = ci + si - di, j0 = cj + sj - dj;
    ci += (uint32_t)__shfl((int)si, 63, 64);
    cj += (uint32_t)__shfl((int)sj, 63, 64);
    // (an unknown operation matches no branch of the counts; the weights' last branch would take it)
    const bool ok = n > 0 && i0 + di <= la && j0 + dj <= pr.lb && (!WEIGHTED || both || op == MC_CIGAR_I || op == MC_CIGAR_D);
    // the counts: per run, or per column (percol) by the run's lane when it is short
    const bool percol = ok && (op == MC_CIGAR_X || (NAIVE && (op == MC_CIGAR_EQ || op == MC_CIGAR_D)));
    if (ok && !percol) {
      if (op == MC_CIGAR_EQ) {
        atomicAdd(&deq[j0], 1);
        atomicAdd(&deq[j0 + n], -1);
      } else if (op == MC_CIGAR_D) {
        atomicAdd(&ddel[j0], 1);
        atomicAdd(&ddel[j0 + n], -1);
      } else if (op == MC_CIGAR_I) {
        atomicAdd(&tab[(uint64_t)j0 * MC_PILEUP_CH + 6], 1u);
        atomicAdd(&tab[(uint64_t)j0 * MC_PILEUP_CH + 7], n);
      }
    }
    if (percol && n <= SPREAD) {
      for (uint32_t t = 0; t < n; t++) {
        const uint32_t ch = op == MC_CIGAR_D ? 5u : base_channel(a[i0 + t]);
        atomicAdd(&tab[(uint64_t)(j0 + t) * MC_PILEUP_CH + ch], 1u);
      }
    }
    if (WEIGHTED && ok && n <= SPREAD) {  // the weights of the short runs, by their lane
      if (both) {
        for (uint32_t t = 0; t < n; t++) {
          const uint32_t v = Qs(i0 + t);
          if (v) atomicAdd(&wt[(uint64_t)(j0 + t) * MC_PILEUP_CH + base_channel(a[i0 + t])], v);
        }
      } else if (op == MC_CIGAR_D) {
        const uint32_t v = gapq(i0);
        if (v)
          for (uint32_t t = 0; t < n; t++) atomicAdd(&wt[(uint64_t)(j0 + t) * MC_PILEUP_CH + 5], v);
      } else {
        uint32_t v = Qs(i0);
        for (uint32_t t = 1; t < n; t++) v = min(v, Qs(i0 + t));
        if (v) atomicAdd(&wt[(uint64_t)j0 * MC_PILEUP_CH + 6], v);
      }
    }
    // the long runs, one after the other by the whole wave: the per-column counts and every weight
    unsigned long long wide = __ballot((WEIGHTED ? ok : percol) && n > SPREAD);
    while (wide) {  // (wave-uniform: one turn per long run of this chunk)
      const int s = __ffsll(wide) - 1;
      wide &= wide - 1;
      const uint32_t bi = (uint32_t)__shfl((int)i0, s, 64), bj = (uint32_t)__shfl((int)j0, s, 64);
      const uint32_t bn = (uint32_t)__shfl((int)n, s, 64), bop = (uint32_t)__shfl((int)op, s, 64);
      if constexpr (!WEIGHTED) {
        for (uint32_t t = (uint32_t)lane; t < bn; t += 64) {
          const uint32_t ch = bop == MC_CIGAR_D ? 5u : base_channel(a[bi + t]);
          atomicAdd(&tab[(uint64_t)(bj + t) * MC_PILEUP_CH + ch], 1u);
        }
      } else if (bop == MC_CIGAR_EQ || bop == MC_CIGAR_X) {
        for (uint32_t t = (uint32_t)lane; t < bn; t += 64) {
          const uint32_t ch = base_channel(a[bi + t]), v = Qs(bi + t);
          if (bop == MC_CIGAR_X) atomicAdd(&tab[(uint64_t)(bj + t) * MC_PILEUP_CH + ch], 1u);
          if (v) atomicAdd(&wt[(uint64_t)(bj + t) * MC_PILEUP_CH + ch], v);
        }
      } else if (bop == MC_CIGAR_D) {
        const uint32_t v = gapq(bi);
        if (v)
          for (uint32_t t = (uint32_t)lane; t < bn; t += 64) atomicAdd(&wt[(uint64_t)(bj + t) * MC_PILEUP_CH + 5], v);
      } else {
        uint32_t v = 0xffffffffu;
        for (uint32_t t = (uint32_t)lane; t < bn; t += 64) v = min(v, Qs(bi + t));
        v = wave_min(v);
        if (lane == 0 && v) atomicAdd(&wt[(uint64_t)bj * MC_PILEUP_CH + 6], v);
      }
    }
  }
}

__global__ __launch_bounds__(64) void nwt_pileup_finish_kernel(const uint8_t *__restrict__ codes, const uint64_t *__restrict__ tgt_off,
                                                               const uint64_t *__restrict__ row_off, uint32_t nt,
                                                               uint32_t *__restrict__ table, const int32_t *__restrict__ deq,
                                                               const int32_t *__restrict__ ddel) {
  const uint32_t t = blockIdx.x;
  if (t >= nt) return;
  const uint64_t row0 = row_off[t], L = row_off[t + 1] - row0 - 1;
  const uint8_t *b = codes + tgt_off[t];
  const int lane = (int)threadIdx.x;
  uint32_t ce = 0, cd = 0;  // coverage carried into this chunk
  const uint64_t nchunk = (L + 63) / 64;
  for (uint64_t c = 0; c < nchunk; c++) {
    const uint64_t r = c * 64 + (uint64_t)lane;
    const bool in = r < L;
    const uint32_t e = in ? (uint32_t)deq[row0 + r] : 0u, d = in ? (uint32_t)ddel[row0 + r] : 0u;
    const uint32_t se = ce + wave_scan(e, lane), sd = cd + wave_scan(d, lane);
    ce = (uint32_t)__shfl((int)se, 63, 64);
    cd = (uint32_t)__shfl((int)sd, 63, 64);
    if (in) {
      uint32_t *row = table + (row0 + r) * MC_PILEUP_CH;
      if (se) row[base_channel(b[r])] += se;
      if (sd) row[5] += sd;
    }
  }
}

}  // namespace

int launch_nw_pileup(mc_ctx *c, uint32_t m, const TracePair *d_pairs, const uint8_t *d_rc, const uint32_t *d_ops,
                     const int32_t *d_res, const uint64_t *d_rowbase, uint32_t *d_table, int32_t *d_deq, int32_t *d_ddel,
                     bool naive) {
  if (m == 0) return MC_OK;
  PileArgs q{(const uint8_t *)c->codes.p, d_rc, d_pairs, d_res, d_ops, d_rowbase, d_table, d_deq, d_ddel, m, nullptr, nullptr, nullptr};
  timed_begin(c);
  if (naive) nwt_pileup_kernel<true, false><<<m, 64, 0, c->stream>>>(q);
  else nwt_pileup_kernel<false, false><<<m, 64, 0, c->stream>>>(q);
  MCG_CHECK(hipGetLastError());
  timed_end(c, F_NW_PU);
  return MC_OK;
}

int launch_nw_qpileup(mc_ctx *c, uint32_t m, const TracePair *d_pairs, const uint8_t *d_rc, const uint32_t *d_ops,
                      const int32_t *d_res, const uint64_t *d_rowbase, const uint64_t *d_qoff, uint32_t *d_table,
                      uint32_t *d_wtable, int32_t *d_deq, int32_t *d_ddel) {
  if (m == 0) return MC_OK;
  PileArgs q{(const uint8_t *)c->codes.p, d_rc, d_pairs, d_res, d_ops, d_rowbase, d_table, d_deq, d_ddel, m,
             (const uint8_t *)c->qual.p, d_qoff, d_wtable};
  timed_begin(c);
  nwt_pileup_kernel<false, true><<<m, 64, 0, c->stream>>>(q);
  MCG_CHECK(hipGetLastError());
  timed_end(c, F_NW_PU);
  return MC_OK;
}

int launch_nw_pileup_finish(mc_ctx *c, uint32_t nt, const uint64_t *d_tgt_off, const uint64_t *d_row_off, uint32_t *d_table,
                            const int32_t *d_deq, const int32_t *d_ddel) {
  if (nt == 0) return MC_OK;
  timed_begin(c);
  nwt_pileup_finish_kernel<<<nt, 64, 0, c->stream>>>((const uint8_t *)c->codes.p, d_tgt_off, d_row_off, nt, d_table, d_deq, d_ddel);
  MCG_CHECK(hipGetLastError());
  timed_end(c, F_NW_PU);
  return MC_OK;
}

}  // namespace mcg
