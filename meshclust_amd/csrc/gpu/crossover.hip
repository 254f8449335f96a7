// crossover.hip -- two alignments of one read compared base by base (mc_nw_msa_crossover, DESIGN.md
// 3.16): the third reader of mc_nw_msa_begin's plan beside msa_counts_kernel and msa_sites_kernel.
//
// For a plan pair p of a read of la bases, e_p(u) = 1 where base u of the read as written lies in an
// '=' column of p's alignment.  For two pairs x and y of the same read, D(s) = sum over u < s of
// e_x(u) - e_y(u), s = 0 .. la; the kernel returns sum e_x, sum e_y, the maximum and the minimum of D
// and the smallest and largest s attaining each (include/meshclust_amd.h has the eight slots).
//
// crossover_kernel: a wavefront per candidate, two bitmaps of ceil(la / 32) words in dynamic LDS (the
// launch's is sized from its longest read; the host buckets the candidates by length).
//   Phase 1: both bitmaps zeroed; for x and then y the pair's operation words 64 at a time, a wave
//   prefix sum over the runs for the read position i0 every run starts at (msa_counts_kernel's walk).
//   An '=' run of n at i0 is bits [i0, i0 + n), for a pair aligned reverse-complemented
//   [la - i0 - n, la - i0).  A run inside one or two words is set by its lane with LDS atomic ORs of
//   masks; longer runs are taken one after the other by the whole wave, a word per lane and step (edge
//   words by atomic OR, the words between, which no other run touches, by plain stores).  A run that
//   would leave the read is skipped, so no word at or past ceil(la / 32) is formed.
//   Phase 2: chunks of 64 word pairs (2,048 bases), a pair per lane.  A lane reduces its positions to a
//   segment (bits of x, bits of y, the maximum prefix of e_x - e_y with its first and last position,
//   the minimum likewise; positions are absolute cuts s = u + 1, and no position past la is formed).
//   Segments combine associatively -- (s1 + s2, max(m1, s1 + m2)), on a tie the first position from
//   the earlier and the last from the later segment -- in order across the wave by a shuffle tree
//   whose lane 0 ends with the whole chunk, and lane 0 carries the result over the chunks, starting
//   from the segment that holds s = 0 alone.
// Lane 0 stores the eight values.  No global atomics, no scratch, all sums are integers: nothing
// depends on the batch, the bucket or the order of the candidates.
#include "mcgpu.hpp"

namespace mcg {

namespace {

__device__ __forceinline__ uint32_t wave_scan(uint32_t v, int lane) {  // inclusive prefix sum over the wave
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t u = (uint32_t)__shfl_up((int)v, d, 64);
    if (lane >= d) v += u;
  }
  return v;
}

constexpr int32_t NONE = 1 << 29;  // no position yet: below every maximum as -NONE, above every minimum as NONE

// the positions of a stretch of the read: how many bits x and y have there, the extrema of the
// running e_x - e_y over its cuts and the first and last cut at each
struct Seg {
  int32_t cx, cy, mx, fmx, lmx, mn, fmn, lmn;
};

__device__ __forceinline__ Seg join(const Seg &a, const Seg &b) {  // a before b
  const int32_t sa = a.cx - a.cy, bmx = sa + b.mx, bmn = sa + b.mn;
  Seg r;
  r.cx = a.cx + b.cx;
  r.cy = a.cy + b.cy;
  r.mx = max(a.mx, bmx);
  r.fmx = a.mx >= bmx ? a.fmx : b.fmx;
  r.lmx = bmx >= a.mx ? b.lmx : a.lmx;
  r.mn = min(a.mn, bmn);
  r.fmn = a.mn <= bmn ? a.fmn : b.fmn;
  r.lmn = bmn <= a.mn ? b.lmn : a.lmn;
  return r;
}

__device__ __forceinline__ Seg seg_down(const Seg &v, int d) {
  Seg r;
  r.cx = __shfl_down(v.cx, d, 64);
  r.cy = __shfl_down(v.cy, d, 64);
  r.mx = __shfl_down(v.mx, d, 64);
  r.fmx = __shfl_down(v.fmx, d, 64);
  r.lmx = __shfl_down(v.lmx, d, 64);
  r.mn = __shfl_down(v.mn, d, 64);
  r.fmn = __shfl_down(v.fmn, d, 64);
  r.lmn = __shfl_down(v.lmn, d, 64);
  return r;
}

// the '=' runs of one pair's words into the bitmap bm of nbw words
__device__ __forceinline__ void fill_bitmap(const uint32_t *__restrict__ src, uint32_t nw, uint32_t la, bool minus, uint32_t *bm,
                                            uint32_t nbw, int lane) {
  uint32_t ci = 0;  // read bases consumed before this chunk
  const uint32_t nchunk = (nw + 63) / 64;
  for (uint32_t c = 0; c < nchunk; c++) {
    const uint32_t kk = c * 64 + (uint32_t)lane;
    const uint32_t wd = kk < nw ? src[kk] : 0u;
    const uint32_t n = wd >> 4, op = wd & 15u;
    const uint32_t di = op == MC_CIGAR_EQ || op == MC_CIGAR_X || op == MC_CIGAR_I ? n : 0u;
    const uint32_t si = wave_scan(di, lane);
    const uint32_t i0 = ci + si - di;
    ci += (uint32_t)__shfl((int)si, 63, 64);
    const bool ok = op == MC_CIGAR_EQ && n > 0 && i0 <= la && n <= la - i0;
    // bits [lo, lo + n) in words w0 .. w1, the first from bit b0 and the last up to bit b1
    const uint32_t lo = ok ? (minus ? la - i0 - n : i0) : 0u, hi = ok ? lo + n - 1 : 0u;
    const uint32_t w0 = lo >> 5, w1 = hi >> 5;
    const uint32_t m0 = 0xffffffffu << (lo & 31u), m1 = 0xffffffffu >> (31u - (hi & 31u));
    if (ok && w1 < nbw) {
      if (w0 == w1) {
        atomicOr(&bm[w0], m0 & m1);
      } else if (w1 == w0 + 1) {
        atomicOr(&bm[w0], m0);
        atomicOr(&bm[w1], m1);
      }
    }
    unsigned long long wide = __ballot(ok && w1 < nbw && w1 > w0 + 1);
    while (wide) {  // (wave-uniform: one turn per long run of this chunk)
      const int s = __ffsll(wide) - 1;
      wide &= wide - 1;
      const uint32_t b0 = (uint32_t)__shfl((int)w0, s, 64), b1 = (uint32_t)__shfl((int)w1, s, 64);
      const uint32_t bm0 = (uint32_t)__shfl((int)m0, s, 64), bm1 = (uint32_t)__shfl((int)m1, s, 64);
      for (uint32_t w = b0 + (uint32_t)lane; w <= b1; w += 64) {
        if (w == b0) atomicOr(&bm[w], bm0);
        else if (w == b1) atomicOr(&bm[w], bm1);
        else bm[w] = 0xffffffffu;
      }
    }
  }
}

__global__ __launch_bounds__(64) void crossover_kernel(const CrossPair *__restrict__ cands, uint32_t nc, const uint32_t *__restrict__ words,
                                                       uint32_t lds_words, int32_t *__restrict__ out) {
  extern __shared__ uint32_t bitmaps[];  // 2 * lds_words
  const uint32_t p = blockIdx.x;
  if (p >= nc) return;
  const CrossPair cp = cands[p];
  const uint32_t la = cp.la, nbw = (la + 31) / 32;
  if (2 * nbw > lds_words) return;  // (the host sized the launch from its longest read)
  uint32_t *bx = bitmaps, *by = bitmaps + nbw;
  const int lane = (int)threadIdx.x;
  for (uint32_t k = (uint32_t)lane; k < 2 * nbw; k += 64) bitmaps[k] = 0u;
  __syncthreads();
  fill_bitmap(words + cp.xw_off, cp.xnw, la, (cp.minus & 1u) != 0, bx, nbw, lane);
  fill_bitmap(words + cp.yw_off, cp.ynw, la, (cp.minus & 2u) != 0, by, nbw, lane);
  __syncthreads();
  Seg carry{0, 0, 0, 0, 0, 0, 0, 0};  // the cut s = 0
  const uint32_t nchunk = (nbw + 63) / 64;
  for (uint32_t c = 0; c < nchunk; c++) {
    const uint32_t k = c * 64 + (uint32_t)lane;
    const uint32_t wx = k < nbw ? bx[k] : 0u, wy = k < nbw ? by[k] : 0u;
    const uint32_t u0 = k * 32, nb = k < nbw ? min(32u, la - u0) : 0u;  // this lane's positions u0 .. u0 + nb
    const uint32_t up = wx & ~wy, dn = wy & ~wx;
    Seg v{(int32_t)__popc(wx), (int32_t)__popc(wy), -NONE, 0, 0, NONE, 0, 0};
    int32_t run = 0;
#pragma unroll
    for (uint32_t b = 0; b < 32; b++) {
      if (b < nb) {
        run += (int32_t)((up >> b) & 1u) - (int32_t)((dn >> b) & 1u);
        const int32_t s = (int32_t)(u0 + b + 1);
        if (run > v.mx) {
          v.mx = run;
          v.fmx = s;
        }
        if (run >= v.mx) v.lmx = s;
        if (run < v.mn) {
          v.mn = run;
          v.fmn = s;
        }
        if (run <= v.mn) v.lmn = s;
      }
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {  // lane l ends with lanes l .. l + 2d - 1 in order; lane 0 with the chunk
      const Seg o = seg_down(v, d);
      if (lane + d < 64) v = join(v, o);
    }
    carry = join(carry, v);  // (lane 0's is the candidate's)
  }
  if (lane == 0) {
    int32_t *o = out + (uint64_t)cp.out * MC_CROSS_RES;
    o[0] = carry.cx;
    o[1] = carry.cy;
    o[2] = carry.cy + carry.mx;
    o[3] = carry.fmx;
    o[4] = carry.lmx;
    o[5] = carry.cx - carry.mn;
    o[6] = carry.fmn;
    o[7] = carry.lmn;
  }
}

}  // namespace

int launch_crossover(mc_ctx *c, uint32_t nc, const CrossPair *d_cands, const uint32_t *d_words, uint32_t max_la, int32_t *d_out) {
  if (nc == 0) return MC_OK;
  const uint32_t lds_words = 2 * ((max_la + 31) / 32);
  timed_begin(c);
  crossover_kernel<<<nc, 64, (size_t)lds_words * 4, c->stream>>>(d_cands, nc, d_words, lds_words, d_out);
  MCG_CHECK(hipGetLastError());
  timed_end(c, F_NW_CROSS);
  return MC_OK;
}

}  // namespace mcg
