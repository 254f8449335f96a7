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

}  // namespace

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

}  // namespace mcg
