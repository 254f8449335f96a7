// msa.hip -- the alignments of nwtrace.hip laid out in common columns per centre (mc_nw_msa_begin /
// mc_nw_msa_rows): the sibling of pileup.hip that keeps the inserted bases.
//
// A centre of L bytes owns L + 1 rows, as in the pile-up.  Row r holds w[r], the longest 'I' run any
// of the centre's pairs has with r centre bases consumed, and col[r] = r + w[0] + .. + w[r], the
// column of centre base r; its w[r] insertion slots are the columns before it.  col[L] = W, the
// width of the centre's block.
//
// msa_width_kernel: per alignment batch after the traceback, a wavefront per pair.  The pair's
// operation words 64 at a time, a wave prefix sum over the runs for the centre row j every run
// starts at (nwt_pileup_kernel's walk); an 'I' run of n at row j is atomicMax(w[j], n).  An integer
// maximum does not depend on the order of the pairs or on the batches.
//
// msa_column_kernel: once per plan, a wavefront per target.  An inclusive wave scan over w[r] + 1 in
// chunks of 64 rows with a carry; col[r] is the sum less 1, the last sum less 1 is W (64-bit: a W
// that does not fit is refused by the host).
//
// msa_render_kernel: a wavefront per row of a render batch.  Every byte of the row is written
// exactly once, so no store waits for another:
//   'I' run of n at row j          its w[j] slots: the n bases, then w[j] - n gaps
//   '=' / 'X' / 'D' run at row j   per column j + t the base (or the gap) at col[j + t] and the
//                                  w[j + t] slot gaps before it -- but not the slots of its first
//                                  column when the word before it was the 'I' run of that row
//   the end                        the w[L] trailing gaps unless the last word was an 'I' run
// A centre's own row is one '=' run of L over the centre's bytes: the same walk, no second path.
// A lane walks a run of at most SPREAD columns itself; longer runs, and slot stretches of more than
// SPREAD gaps, are taken one after the other by the whole wave, 64 bytes per step.  Every trip
// count is known on entry.  A run that would leave the pair's strings is skipped and no byte at or
// past W is stored, so no address outside the row is formed.
//
// msa_counts_kernel / msa_counts_finish_kernel (mc_nw_msa_counts): the block counted
// per column instead of rendered, MC_MSA_CH counters per column.  A wavefront per pair, the same walk:
//   '=' / 'D' run of n at row j   +1 at j and -1 at j + n of the target's '=' / 'D' difference array
//                                 (pileup.hip's two atomics per run)
//   'X' run of n at row j         per column one atomic on the class of seq1[i + t] at col[j + t]
//   'I' run of n at row j         per base one atomic on its class at col[j] - w[j] + t
// WEIGHTED: beside them the loaded qualities into a second table, an atomic per column as
// nwt_pileup_kernel<false, true> does ('=' and 'X' the base's quality, 'D' the smaller quality around
// the gap on channel 5, 'I' the inserted base's own quality in its slot); a zero weight issues none.
// A lane walks a run of at most SPREAD columns itself, longer runs are taken by the whole wave.  The
// finish kernel, a wavefront per target and no atomics: the running sums of the differences go to
// col[r] (the centre byte's class, channel 5), channels 6 and 7 are written, and every slot's
// channel 5 becomes depth less its channels 0..4.  A run that would leave the pair's strings is
// skipped and no column at or past W is touched: msa_render_kernel's rule.
//
// msa_sites_resolve_kernel / msa_sites_kernel (mc_nw_msa_sites): the block gathered at
// a caller-chosen set of columns per target instead of rendered.  The resolve kernel, a wavefront per
// target and a lane per site: the first row r with col[r] >= the column, by bisection; the site is
// centre base r (slot 0) or slot column - (col[r] - w[r]) + 1 of site r -- what the finish kernel
// writes to channels 6 and 7.  The gather kernel, a wavefront per pair over an output the host filled
// with the gap (the weights with 0), the same walk; the lane that owns a run lower-bounds its
// target's ascending site list at the run's first column and stores the bytes of the sites inside it:
//   '=' / 'X' run of n at row j   the sites with slot 0 and r in [j, j + n): the base, its quality
//   'D' run of n at row j         the same sites: the run's weight only, the byte stays a gap
//   'I' run of n at row j         the sites at columns col[j] - w[j] + t, t < min(n, w[j]): the base
//                                 seq1[i + t], its quality
// Every non-gap byte is stored exactly once, by one lane, so the result depends on no order.  A run
// that would leave the pair's strings is skipped and no offset at or past S is formed.
#include "mcgpu.hpp"

namespace mcg {

namespace {

constexpr uint32_t SPREAD = 8;  // runs and slot stretches longer than this are shared by the wave

__device__ __forceinline__ uint32_t wave_scan(uint32_t v, int lane) {  // inclusive prefix sum over the wave
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t u = (uint32_t)__shfl_up((int)v, d, 64);
    if (lane >= d) v += u;
  }
  return v;
}

__device__ __forceinline__ uint64_t wave_scan64(uint64_t v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t u = (uint64_t)__shfl_up((unsigned long long)v, d, 64);
    if (lane >= d) v += u;
  }
  return v;
}

// the FASTA writer's rule (host/consensus.hpp pileup_base_char): "ACGT"[x] for a digit, else the byte
__device__ __forceinline__ uint8_t base_char(uint8_t x) { return x <= 3 ? (uint8_t)(0x54474341u >> (8 * x)) : x; }

__global__ __launch_bounds__(64) void msa_width_kernel(const TracePair *__restrict__ pairs, const int32_t *__restrict__ res,
                                                       const uint32_t *__restrict__ ops, const uint64_t *__restrict__ rowbase,
                                                       uint32_t *__restrict__ width, uint32_t npairs) {
  const uint32_t p = blockIdx.x;
  if (p >= npairs) return;
  const TracePair pr = pairs[p];
  const uint32_t nw = (uint32_t)res[(uint64_t)p * TRACE_RES + 3], cap = pr.la + pr.lb;
  if (nw == 0 || nw > cap) return;
  const uint32_t *src = ops + pr.ops_off + (cap - nw);
  uint32_t *w = width + rowbase[p];
  const int lane = (int)threadIdx.x;
  uint32_t ci = 0, cj = 0;  // bases consumed before this chunk
  const uint32_t nchunk = (nw + 63) / 64;
  for (uint32_t c = 0; c < nchunk; c++) {
    const uint32_t k = c * 64 + (uint32_t)lane;
    const uint32_t wd = k < nw ? src[k] : 0u;
    const uint32_t n = wd >> 4, op = wd & 15u;
    const bool both = op == MC_CIGAR_EQ || op == MC_CIGAR_X;
    const uint32_t di = both || op == MC_CIGAR_I ? n : 0u, dj = both || op == MC_CIGAR_D ? n : 0u;
    const uint32_t si = wave_scan(di, lane), sj = wave_scan(dj, lane);
    const uint32_t i0 = ci + si - di, j0 = cj + sj - dj;
    ci += (uint32_t)__shfl((int)si, 63, 64);
    cj += (uint32_t)__shfl((int)sj, 63, 64);
    if (op == MC_CIGAR_I && n > 0 && i0 + n <= pr.la && j0 <= pr.lb) atomicMax(&w[j0], n);
  }
}

__global__ __launch_bounds__(64) void msa_column_kernel(const uint64_t *__restrict__ row_off, const uint32_t *__restrict__ width,
                                                        uint32_t *__restrict__ col, uint64_t *__restrict__ bw, uint32_t nt) {
  const uint32_t t = blockIdx.x;
  if (t >= nt) return;
  const uint64_t row0 = row_off[t], nrow = row_off[t + 1] - row0;  // L + 1
  const int lane = (int)threadIdx.x;
  uint64_t carry = 0;
  const uint64_t nchunk = (nrow + 63) / 64;
  for (uint64_t c = 0; c < nchunk; c++) {
    const uint64_t r = c * 64 + (uint64_t)lane;
    const bool in = r < nrow;
    const uint64_t s = carry + wave_scan64(in ? (uint64_t)width[row0 + r] + 1 : 0ull, lane);
    carry = (uint64_t)__shfl((unsigned long long)s, 63, 64);
    if (in) col[row0 + r] = (uint32_t)(s - 1);
  }
  if (lane == 0) bw[t] = nrow ? carry - 1 : 0;
}

__global__ __launch_bounds__(64) void msa_render_kernel(const MsaRow *__restrict__ rows, uint32_t nrows, const uint8_t *__restrict__ codes,
                                                        const uint8_t *__restrict__ rc, const uint32_t *__restrict__ words,
                                                        const uint32_t *__restrict__ width, const uint32_t *__restrict__ colarr,
                                                        uint8_t *__restrict__ out) {
  const uint32_t k = blockIdx.x;
  if (k >= nrows) return;
  const MsaRow rw = rows[k];
  const uint8_t *a = (rw.a_rc ? rc : codes) + rw.a_off;
  const uint32_t *w = width + rw.row0, *col = colarr + rw.row0;
  const uint32_t *src = words + rw.w_off;
  uint8_t *o = out + rw.out_off;
  const uint32_t la = rw.la, L = rw.lb, W = rw.W, nw = rw.nw;
  const bool centre = rw.centre != 0;
  const int lane = (int)threadIdx.x;
  auto put = [&](uint32_t p, uint8_t v) {
    if (p < W) o[p] = v;
  };
  auto wave_fill = [&](uint32_t p0, uint32_t cnt) {  // cnt gaps from p0, by the whole wave
    for (uint32_t t = (uint32_t)lane; t < cnt; t += 64) put(p0 + t, MC_MSA_GAP);
  };
  // One column of an '=' / 'X' / 'D' run per lane that is `on`: the base or the gap at col[j], the
  // slot gaps before it (`skip`: an 'I' run wrote them).  Called by the whole wave: a stretch of more
  // than SPREAD gaps is filled by all lanes.
  auto column = [&](bool on, uint32_t i, uint32_t j, bool del, bool skip) {
    uint32_t pc = 0, pw = 0;
    if (on) {
      pc = col[j];
      pw = skip ? 0u : w[j];
      put(pc, del ? (uint8_t)MC_MSA_GAP : base_char(a[i]));
      if (pw <= SPREAD)
        for (uint32_t s = 0; s < pw; s++) put(pc - pw + s, MC_MSA_GAP);
    }
    unsigned long long far = __ballot(on && pw > SPREAD);
    while (far) {  // (wave-uniform)
      const int s = __ffsll(far) - 1;
      far &= far - 1;
      const uint32_t bc = (uint32_t)__shfl((int)pc, s, 64), bw = (uint32_t)__shfl((int)pw, s, 64);
      wave_fill(bc - bw, bw);
    }
  };
  uint32_t ci = 0, cj = 0;  // bases consumed before this chunk
  int carry_i = 0, last_i = 0;  // the word before this chunk / the row's last word was a sound 'I' run
  const uint32_t nchunk = (nw + 63) / 64;
  for (uint32_t c = 0; c < nchunk; c++) {
    const uint32_t kk = c * 64 + (uint32_t)lane;
    const uint32_t wd = kk < nw && !centre ? src[kk] : 0u;  // (a centre row: one '=' run of L, nw = 1)
    const uint32_t n = kk >= nw ? 0u : centre ? L : wd >> 4, op = centre ? MC_CIGAR_EQ : wd & 15u;
    const bool both = op == MC_CIGAR_EQ || op == MC_CIGAR_X, del = op == MC_CIGAR_D;
    const uint32_t di = both || op == MC_CIGAR_I ? n : 0u, dj = both || del ? n : 0u;
    const uint32_t si = wave_scan(di, lane), sj = wave_scan(dj, lane);
    const uint32_t i0 = ci + si - di, j0 = cj + sj - dj;
    ci += (uint32_t)__shfl((int)si, 63, 64);
    cj += (uint32_t)__shfl((int)sj, 63, 64);
    const bool ok = n > 0 && i0 + di <= la && j0 + dj <= L;
    const int is_i = ok && op == MC_CIGAR_I ? 1 : 0;
    int prev_i = __shfl_up(is_i, 1, 64);
    if (lane == 0) prev_i = carry_i;
    carry_i = __shfl(is_i, 63, 64);
    if (c + 1 == nchunk) last_i = __shfl(is_i, (int)((nw - 1) & 63u), 64);
    // the 'I' runs: the row's w[j0] slots, bases first
    uint32_t wj = 0, s0 = 0, nn = 0;
    if (is_i) {
      wj = w[j0];
      s0 = col[j0] - wj;
      nn = min(n, wj);
      if (wj <= SPREAD)
        for (uint32_t t = 0; t < wj; t++) put(s0 + t, t < nn ? base_char(a[i0 + t]) : (uint8_t)MC_MSA_GAP);
    }
    unsigned long long wide = __ballot(is_i && wj > SPREAD);
    while (wide) {  // (wave-uniform: one turn per wide slot run of this chunk)
      const int s = __ffsll(wide) - 1;
      wide &= wide - 1;
      const uint32_t bs = (uint32_t)__shfl((int)s0, s, 64), bw = (uint32_t)__shfl((int)wj, s, 64);
      const uint32_t bn = (uint32_t)__shfl((int)nn, s, 64), bi = (uint32_t)__shfl((int)i0, s, 64);
      for (uint32_t t = (uint32_t)lane; t < bw; t += 64) put(bs + t, t < bn ? base_char(a[bi + t]) : (uint8_t)MC_MSA_GAP);
    }
    // the '=' / 'X' / 'D' runs: short ones by their lane, a column per turn
    const bool md = ok && (both || del);
    for (uint32_t t = 0; t < SPREAD; t++) {
      const bool on = md && n <= SPREAD && t < n;
      if (!__ballot(on)) break;
      column(on, i0 + t, j0 + t, del, t == 0 && prev_i);
    }
    wide = __ballot(md && n > SPREAD);
    while (wide) {  // the long ones, one after the other by the whole wave
      const int s = __ffsll(wide) - 1;
      wide &= wide - 1;
      const uint32_t bi = (uint32_t)__shfl((int)i0, s, 64), bj = (uint32_t)__shfl((int)j0, s, 64);
      const uint32_t bn = (uint32_t)__shfl((int)n, s, 64);
      const bool bdel = __shfl((int)del, s, 64) != 0, bprev = __shfl(prev_i, s, 64) != 0;
      for (uint32_t t0 = 0; t0 < bn; t0 += 64) {
        const uint32_t t = t0 + (uint32_t)lane;
        column(t < bn, bi + t, bj + t, bdel, t == 0 && bprev);
      }
    }
  }
  if (!last_i) {
    const uint32_t wl = w[L];
    wave_fill(W - wl, wl);
  }
}

__device__ __forceinline__ uint32_t base_class(uint8_t x) { return x <= 3 ? x : 4u; }

struct CountArgs {
  const MsaCountPair *pairs;
  uint32_t npairs;
  const uint8_t *codes, *rc, *qual;
  const uint32_t *words, *width, *col;
  uint32_t *counts, *wcounts;
  int32_t *deq, *ddel;
};

template <bool WEIGHTED>
__global__ __launch_bounds__(64) void msa_counts_kernel(CountArgs q) {
  const uint32_t p = blockIdx.x;
  if (p >= q.npairs) return;
  const MsaCountPair pr = q.pairs[p];
  const uint8_t *a = (pr.a_rc ? q.rc : q.codes) + pr.a_off;
  const uint8_t *ql = WEIGHTED ? q.qual + pr.q_off : nullptr;
  const uint32_t *w = q.width + pr.row0, *col = q.col + pr.row0;
  const uint32_t *src = q.words + pr.w_off;
  uint32_t *tab = q.counts + pr.col0 * MC_MSA_CH, *wt = WEIGHTED ? q.wcounts + pr.col0 * MC_MSA_CH : nullptr;
  int32_t *deq = q.deq + pr.drow0, *ddel = q.ddel + pr.drow0;
  const uint32_t la = pr.la, L = pr.lb, W = pr.W, nw = pr.nw;
  const bool rc = pr.a_rc != 0;
  const int lane = (int)threadIdx.x;
  auto Qs = [&](uint32_t i) -> uint32_t { return ql[rc ? la - 1 - i : i]; };  // i < la
  auto gapq = [&](uint32_t i) -> uint32_t {  // nwt_pileup_kernel's weight of a 'D' run with i read bases before it
    uint32_t v = 0xffffffffu;
    if (i > 0) v = Qs(i - 1);
    if (i < la) v = min(v, Qs(i));
    return v == 0xffffffffu ? 0u : v;
  };
  auto add = [&](uint32_t pc, uint32_t ch) {
    if (pc < W) atomicAdd(&tab[(uint64_t)pc * MC_MSA_CH + ch], 1u);
  };
  auto addw = [&](uint32_t pc, uint32_t ch, uint32_t v) {
    if (WEIGHTED && v && pc < W) atomicAdd(&wt[(uint64_t)pc * MC_MSA_CH + ch], v);
  };
  // column t of a run: op, the read position i0 and row j0 it starts at, s0 the first slot of an 'I'
  // run's site, gq a 'D' run's weight
  auto column = [&](uint32_t op, uint32_t i0, uint32_t j0, uint32_t s0, uint32_t gq, uint32_t t) {
    if (op == MC_CIGAR_D) {
      addw(col[j0 + t], 5u, gq);
      return;
    }
    const uint32_t ch = base_class(a[i0 + t]), pc = op == MC_CIGAR_I ? s0 + t : col[j0 + t];
    if (op != MC_CIGAR_EQ) add(pc, ch);
    if (WEIGHTED) addw(pc, ch, Qs(i0 + t));
  };
  uint32_t ci = 0, cj = 0;  // bases consumed before this chunk
  const uint32_t nchunk = (nw + 63) / 64;
  for (uint32_t c = 0; c < nchunk; c++) {
    const uint32_t kk = c * 64 + (uint32_t)lane;
    const uint32_t wd = kk < nw ? src[kk] : 0u;
    const uint32_t n = wd >> 4, op = wd & 15u;
    const bool both = op == MC_CIGAR_EQ || op == MC_CIGAR_X, del = op == MC_CIGAR_D, ins = op == MC_CIGAR_I;
    const uint32_t di = both || ins ? n : 0u, dj = both || del ? n : 0u;
    const uint32_t si = wave_scan(di, lane), sj = wave_scan(dj, lane);
    const uint32_t i0 = ci + si - di, j0 = cj + sj - dj;
    ci += (uint32_t)__shfl((int)si, 63, 64);
    cj += (uint32_t)__shfl((int)sj, 63, 64);
    const bool ok = n > 0 && i0 + di <= la && j0 + dj <= L && (both || del || ins);
    if (ok && op == MC_CIGAR_EQ) {
      atomicAdd(&deq[j0], 1);
      atomicAdd(&deq[j0 + n], -1);
    } else if (ok && del) {
      atomicAdd(&ddel[j0], 1);
      atomicAdd(&ddel[j0 + n], -1);
    }
    // the columns that take an atomic each: cnt of them (an 'I' run: no more than its site has slots)
    uint32_t cnt = 0, s0 = 0, gq = 0;
    if (ok && ins) {
      const uint32_t wj = w[j0];
      s0 = col[j0] - wj;
      cnt = min(n, wj);
    } else if (ok && (op == MC_CIGAR_X || WEIGHTED)) {
      cnt = n;
      if (WEIGHTED && del) {
        gq = gapq(i0);
        if (!gq) cnt = 0;
      }
    }
    if (cnt <= SPREAD)
      for (uint32_t t = 0; t < cnt; t++) column(op, i0, j0, s0, gq, t);
    unsigned long long wide = __ballot(cnt > SPREAD);
    while (wide) {  // (wave-uniform: one turn per long run of this chunk)
      const int s = __ffsll(wide) - 1;
      wide &= wide - 1;
      const uint32_t bi = (uint32_t)__shfl((int)i0, s, 64), bj = (uint32_t)__shfl((int)j0, s, 64);
      const uint32_t bs = (uint32_t)__shfl((int)s0, s, 64), bg = (uint32_t)__shfl((int)gq, s, 64);
      const uint32_t bn = (uint32_t)__shfl((int)cnt, s, 64), bop = (uint32_t)__shfl((int)op, s, 64);
      for (uint32_t t = (uint32_t)lane; t < bn; t += 64) column(bop, bi, bj, bs, bg, t);
    }
  }
}

__global__ __launch_bounds__(64) void msa_counts_finish_kernel(const MsaCountTarget *__restrict__ tgts, uint32_t nt,
                                                               const uint8_t *__restrict__ codes, const uint32_t *__restrict__ width,
                                                               const uint32_t *__restrict__ colarr, uint32_t *__restrict__ counts,
                                                               const int32_t *__restrict__ deq_all, const int32_t *__restrict__ ddel_all) {
  const uint32_t k = blockIdx.x;
  if (k >= nt) return;
  const MsaCountTarget tg = tgts[k];
  const uint8_t *b = codes + tg.c_off;
  const uint32_t *w = width + tg.row0, *col = colarr + tg.row0;
  uint32_t *tab = counts + tg.col0 * MC_MSA_CH;
  const int32_t *deq = deq_all + tg.drow0, *ddel = ddel_all + tg.drow0;
  const uint32_t L = tg.L, W = tg.W, depth = tg.depth;
  const int lane = (int)threadIdx.x;
  auto slot = [&](uint32_t pc, uint32_t r, uint32_t t) {  // slot t of site r: the rows with a gap, the site, the slot
    if (pc >= W) return;
    uint32_t *row = tab + (uint64_t)pc * MC_MSA_CH;
    row[5] = depth - (row[0] + row[1] + row[2] + row[3] + row[4]);
    row[6] = r;
    row[7] = t + 1;
  };
  uint32_t ce = 0, cd = 0;  // coverage carried into this chunk
  const uint32_t nchunk = L / 64 + 1;  // rows 0 .. L
  for (uint32_t c = 0; c < nchunk; c++) {
    const uint32_t r = c * 64 + (uint32_t)lane;
    const bool base = r < L, site = r <= L;
    const uint32_t e = base ? (uint32_t)deq[r] : 0u, d = base ? (uint32_t)ddel[r] : 0u;
    const uint32_t se = ce + wave_scan(e, lane), sd = cd + wave_scan(d, lane);
    ce = (uint32_t)__shfl((int)se, 63, 64);
    cd = (uint32_t)__shfl((int)sd, 63, 64);
    const uint32_t pc = site ? col[r] : 0u, wr = site ? w[r] : 0u;
    if (base && pc < W) {
      uint32_t *row = tab + (uint64_t)pc * MC_MSA_CH;
      if (se) row[base_class(b[r])] += se;
      if (sd) row[5] += sd;
      row[6] = r;
      row[7] = 0;
    }
    if (wr <= SPREAD)
      for (uint32_t t = 0; t < wr; t++) slot(pc - wr + t, r, t);
    unsigned long long wide = __ballot(wr > SPREAD);
    while (wide) {  // (wave-uniform: one turn per wide site of this chunk)
      const int s = __ffsll(wide) - 1;
      wide &= wide - 1;
      const uint32_t bc = (uint32_t)__shfl((int)pc, s, 64), bw = (uint32_t)__shfl((int)wr, s, 64);
      const uint32_t br = c * 64 + (uint32_t)s;
      for (uint32_t t = (uint32_t)lane; t < bw; t += 64) slot(bc - bw + t, br, t);
    }
  }
}

__global__ __launch_bounds__(64) void msa_sites_resolve_kernel(const MsaSiteTarget *__restrict__ tgts, uint32_t nt,
                                                               const uint32_t *__restrict__ width, const uint32_t *__restrict__ colarr,
                                                               const uint32_t *__restrict__ sites, uint2 *__restrict__ res) {
  const uint32_t k = blockIdx.x;
  if (k >= nt) return;
  const MsaSiteTarget tg = tgts[k];
  const uint32_t *w = width + tg.row0, *col = colarr + tg.row0;
  for (uint32_t s = threadIdx.x; s < tg.S; s += 64) {
    const uint32_t pc = sites[tg.s_off + s];
    uint32_t lo = 0, hi = tg.L;  // the first row whose column is not before pc (col[L] = W > pc)
    while (lo < hi) {
      const uint32_t mid = (lo + hi) / 2;
      if (col[mid] < pc) lo = mid + 1;
      else hi = mid;
    }
    const uint32_t c = col[lo];
    res[tg.s_off + s] = make_uint2(lo, c == pc && lo < tg.L ? 0u : pc - (c - w[lo]) + 1);
  }
}

struct SiteArgs {
  const MsaSitePair *pairs;
  uint32_t npairs;
  const uint8_t *codes, *rc, *qual;
  const uint32_t *words, *width, *col, *sites;
  const uint2 *res;
  uint8_t *out, *qout;
};

template <bool WEIGHTED>
__global__ __launch_bounds__(64) void msa_sites_kernel(SiteArgs q) {
  const uint32_t p = blockIdx.x;
  if (p >= q.npairs) return;
  const MsaSitePair pr = q.pairs[p];
  const uint32_t S = pr.S;
  if (S == 0) return;
  const uint8_t *a = (pr.a_rc ? q.rc : q.codes) + pr.a_off;
  const uint8_t *ql = WEIGHTED ? q.qual + pr.q_off : nullptr;
  const uint32_t *w = q.width + pr.row0, *col = q.col + pr.row0;
  const uint32_t *src = q.words + pr.w_off;
  const uint32_t *st = q.sites + pr.s_off;
  const uint2 *rs = q.res + pr.s_off;
  uint8_t *o = q.out + pr.out_off, *oq = WEIGHTED ? q.qout + pr.out_off : nullptr;
  const uint32_t la = pr.la, L = pr.lb, nw = pr.nw;
  const bool rc = pr.a_rc != 0;
  const int lane = (int)threadIdx.x;
  auto Qs = [&](uint32_t i) -> uint32_t { return ql[rc ? la - 1 - i : i]; };  // i < la
  auto lower = [&](uint32_t pc) {  // the first site at or after column pc (S: none)
    uint32_t lo = 0, hi = S;
    while (lo < hi) {
      const uint32_t mid = (lo + hi) / 2;
      if (st[mid] < pc) lo = mid + 1;
      else hi = mid;
    }
    return lo;
  };
  uint32_t ci = 0, cj = 0;  // bases consumed before this chunk
  const uint32_t nchunk = (nw + 63) / 64;
  for (uint32_t c = 0; c < nchunk; c++) {
    const uint32_t kk = c * 64 + (uint32_t)lane;
    const uint32_t wd = kk < nw ? src[kk] : 0u;
    const uint32_t n = wd >> 4, op = wd & 15u;
    const bool both = op == MC_CIGAR_EQ || op == MC_CIGAR_X, del = op == MC_CIGAR_D, ins = op == MC_CIGAR_I;
    const uint32_t di = both || ins ? n : 0u, dj = both || del ? n : 0u;
    const uint32_t si = wave_scan(di, lane), sj = wave_scan(dj, lane);
    const uint32_t i0 = ci + si - di, j0 = cj + sj - dj;
    ci += (uint32_t)__shfl((int)si, 63, 64);
    cj += (uint32_t)__shfl((int)sj, 63, 64);
    const bool ok = n > 0 && i0 + di <= la && j0 + dj <= L;
    if (ok && ins) {
      const uint32_t wj = w[j0], s0 = col[j0] - wj, cnt = min(n, wj);
      for (uint32_t s = lower(s0); s < S; s++) {
        const uint32_t t = st[s] - s0;
        if (t >= cnt) break;
        o[s] = base_char(a[i0 + t]);
        if (WEIGHTED) oq[s] = (uint8_t)Qs(i0 + t);
      }
    } else if (ok && (both || (WEIGHTED && del))) {
      uint32_t gq = 0;
      if (WEIGHTED && del) {  // nwt_pileup_kernel's weight of a 'D' run with i0 read bases before it
        uint32_t v = 0xffffffffu;
        if (i0 > 0) v = Qs(i0 - 1);
        if (i0 < la) v = min(v, Qs(i0));
        gq = v == 0xffffffffu ? 0u : v;
      }
      if (both || gq)
        for (uint32_t s = lower(col[j0]); s < S; s++) {
          const uint2 x = rs[s];
          if (x.x >= j0 + n) break;
          if (x.y) continue;  // a slot between two columns of the run: the pair has no 'I' run there
          const uint32_t i = i0 + (x.x - j0);
          if (both) o[s] = base_char(a[i]);
          if (WEIGHTED) oq[s] = (uint8_t)(both ? Qs(i) : gq);
        }
    }
  }
}

}  // namespace

int launch_msa_sites_resolve(mc_ctx *c, uint32_t nt, const MsaSiteTarget *d_tgts, const uint32_t *d_width, const uint32_t *d_col,
                             const uint32_t *d_sites, uint2 *d_res) {
  if (nt == 0) return MC_OK;
  timed_begin(c);
  msa_sites_resolve_kernel<<<nt, 64, 0, c->stream>>>(d_tgts, nt, d_width, d_col, d_sites, d_res);
  MCG_CHECK(hipGetLastError());
  timed_end(c, F_NW_MSAS);
  return MC_OK;
}

int launch_msa_sites(mc_ctx *c, uint64_t npairs, const MsaSitePair *d_pairs, const uint8_t *d_rc, const uint32_t *d_words,
                     const uint32_t *d_width, const uint32_t *d_col, const uint32_t *d_sites, const uint2 *d_res, uint8_t *d_out,
                     uint8_t *d_qout) {
  if (npairs == 0) return MC_OK;
  SiteArgs q{d_pairs, (uint32_t)npairs, (const uint8_t *)c->codes.p, d_rc, (const uint8_t *)c->qual.p, d_words, d_width, d_col,
             d_sites, d_res, d_out, d_qout};
  timed_begin(c);
  if (d_qout) msa_sites_kernel<true><<<(unsigned)npairs, 64, 0, c->stream>>>(q);
  else msa_sites_kernel<false><<<(unsigned)npairs, 64, 0, c->stream>>>(q);
  MCG_CHECK(hipGetLastError());
  timed_end(c, F_NW_MSAS);
  return MC_OK;
}

int launch_msa_width(mc_ctx *c, uint32_t m, const TracePair *d_pairs, const uint32_t *d_ops, const int32_t *d_res,
                     const uint64_t *d_rowbase, uint32_t *d_width) {
  if (m == 0) return MC_OK;
  timed_begin(c);
  msa_width_kernel<<<m, 64, 0, c->stream>>>(d_pairs, d_res, d_ops, d_rowbase, d_width, m);
  MCG_CHECK(hipGetLastError());
  timed_end(c, F_NW_MSAW);
  return MC_OK;
}

int launch_msa_columns(mc_ctx *c, uint32_t nt, const uint64_t *d_row_off, const uint32_t *d_width, uint32_t *d_col, uint64_t *d_bw) {
  if (nt == 0) return MC_OK;
  timed_begin(c);
  msa_column_kernel<<<nt, 64, 0, c->stream>>>(d_row_off, d_width, d_col, d_bw, nt);
  MCG_CHECK(hipGetLastError());
  timed_end(c, F_NW_MSAW);
  return MC_OK;
}

int launch_msa_render(mc_ctx *c, uint64_t nrows, const MsaRow *d_rows, const uint8_t *d_rc, const uint32_t *d_words,
                      const uint32_t *d_width, const uint32_t *d_col, uint8_t *d_out) {
  if (nrows == 0) return MC_OK;
  timed_begin(c);
  msa_render_kernel<<<(unsigned)nrows, 64, 0, c->stream>>>(d_rows, (uint32_t)nrows, (const uint8_t *)c->codes.p, d_rc, d_words, d_width,
                                                           d_col, d_out);
  MCG_CHECK(hipGetLastError());
  timed_end(c, F_NW_MSAR);
  return MC_OK;
}

int launch_msa_counts(mc_ctx *c, uint64_t npairs, const MsaCountPair *d_pairs, const uint8_t *d_rc, const uint32_t *d_words,
                      const uint32_t *d_width, const uint32_t *d_col, uint32_t *d_counts, uint32_t *d_wcounts, int32_t *d_deq,
                      int32_t *d_ddel) {
  if (npairs == 0) return MC_OK;
  CountArgs q{d_pairs, (uint32_t)npairs, (const uint8_t *)c->codes.p, d_rc, (const uint8_t *)c->qual.p, d_words, d_width, d_col,
              d_counts, d_wcounts, d_deq, d_ddel};
  timed_begin(c);
  if (d_wcounts) msa_counts_kernel<true><<<(unsigned)npairs, 64, 0, c->stream>>>(q);
  else msa_counts_kernel<false><<<(unsigned)npairs, 64, 0, c->stream>>>(q);
  MCG_CHECK(hipGetLastError());
  timed_end(c, F_NW_MSAC);
  return MC_OK;
}

int launch_msa_counts_finish(mc_ctx *c, uint32_t nt, const MsaCountTarget *d_tgts, const uint32_t *d_width, const uint32_t *d_col,
                             uint32_t *d_counts, const int32_t *d_deq, const int32_t *d_ddel) {
  if (nt == 0) return MC_OK;
  timed_begin(c);
  msa_counts_finish_kernel<<<nt, 64, 0, c->stream>>>(d_tgts, nt, (const uint8_t *)c->codes.p, d_width, d_col, d_counts, d_deq, d_ddel);
  MCG_CHECK(hipGetLastError());
  timed_end(c, F_NW_MSAC);
  return MC_OK;
}

}  // namespace mcg
