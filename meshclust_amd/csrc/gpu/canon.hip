// canon.hip -- strand-blind histograms: the canonical rows and the orientation of pairs.
//
// The histogram of the reverse-complemented record is the permutation row[rc(i)] of the record's
// own (host/strand.hpp).  The canonical row counts the k-mers of both strands:
//   canon[i] = row[i] + row[rc(i)] - 1        (one pseudocount, not two)
// so a record and its reverse complement have the same canonical row, mag_canon = 2 mag - B, and
// the sum of squares is recomputed.  It is bit for bit the forward histogram of the record
// r || N x 30 || rc(r) with its second segment mirrored.
//
// canon_rows_kernel is a post-pass over K1's rows (kmer.hip is not touched): a workgroup stages
// one forward row in LDS with 16-byte loads (the gather has a stride of 4^(k-1) between
// neighbouring bins, as in assign.hip's revcomp_rows_kernel), a thread writes whole 16-byte
// output chunks, and magnitude, sum of squares and the row maximum are reduced over the wave and
// then the workgroup.  Out of place: K1 filled one buffer, the fold writes the other, and the
// caller swaps the pointers (the forward rows stay for orient_kernel).  out == nullptr: the
// maximum only (mc_kmer_max_strands).
//
// orient_kernel decides the strand of a pair (a, b) on the forward rows:
//   sad_plus = sum |row_a[i] - row_b[i]|,  sad_minus = sum |row_a[i] - row_b[rc(i)]|,
//   minus iff sad_minus < sad_plus (a tie is plus).
// Callers pass pairs grouped by b; the host cuts the list into runs of equal b of at most RUN
// pairs, a workgroup takes a run, stages row_b and its permuted row in LDS once, and a 16-lane
// group scores one pair at a time: lane l takes chunks l, l + 16, ... of row_a from global memory
// (16-byte loads) against the two LDS rows (v_sad_u8 on 8-bit bins, subtraction on 16-bit ones)
// and the group's sums are folded with four shuffles.  Both sums fit 32 bits (4^7 bins of at most
// 65535).  Every trip count is uniform and known on entry.
#include <algorithm>

#include "../host/strand.hpp"
#include "mcgpu.hpp"

namespace mcg {

namespace {

constexpr int NT = 256;
constexpr int NW = NT / 64;
constexpr int RUN = 64;  // pairs of one run (orient_kernel): four per 16-lane group

__device__ __forceinline__ uint64_t wsum64(uint64_t v) {
  for (int o = 32; o >= 1; o >>= 1) {
    const uint32_t lo = __shfl_xor((uint32_t)v, o, 64), hi = __shfl_xor((uint32_t)(v >> 32), o, 64);
    v += ((uint64_t)hi << 32) | lo;
  }
  return v;
}
__device__ __forceinline__ uint32_t wmax32(uint32_t v) {
  for (int o = 32; o >= 1; o >>= 1) {
    const uint32_t x = __shfl_xor(v, o, 64);
    v = x > v ? x : v;
  }
  return v;
}

// row r of `out` = the canonical row of forward row r of `in` (both n rows at `pitch`); mag / sumsq
// of the canonical row; *gmax = the largest canonical bin of all rows.  The bins past B up to the
// pitch (k = 1) are written as zeros.
template <typename T>
__global__ __launch_bounds__(NT) void canon_rows_kernel(const uint8_t *__restrict__ in, uint64_t n, uint64_t pitch, int B,
                                                        int k, uint8_t *__restrict__ out, uint64_t *__restrict__ mag,
                                                        uint64_t *__restrict__ sumsq, unsigned long long *__restrict__ gmax) {
  extern __shared__ __attribute__((aligned(16))) uint4 tl[];
  constexpr int E = 16 / (int)sizeof(T);  // bins per chunk
  constexpr int PW = 4 / (int)sizeof(T);  // bins per 32-bit word
  const int nch = (int)(pitch / 16);
  const T *src = reinterpret_cast<const T *>(tl);
  uint64_t *red = reinterpret_cast<uint64_t *>(tl + nch);  // 3 * NW partial results, after the row
  const int lane = threadIdx.x & 63, wave = wave_id();
  uint32_t bmax = 0;  // this workgroup's largest bin (over its rows)
  for (uint64_t r = blockIdx.x; r < n; r += gridDim.x) {
    const uint4 *row = reinterpret_cast<const uint4 *>(in + r * pitch);
    __syncthreads();  // (the previous row's reads of tl and red are done)
    for (int ch = threadIdx.x; ch < nch; ch += NT) tl[ch] = row[ch];
    __syncthreads();
    uint64_t s = 0, q = 0;
    uint32_t mx = 0;
    for (int ch = threadIdx.x; ch < nch; ch += NT) {
      uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
      for (int e = 0; e < E; e++) {
        const int i = ch * E + e;
        if (i < B) {
          const uint32_t v = (uint32_t)src[i] + (uint32_t)src[mc::rc_index((uint32_t)i, k)] - 1u;
          s += v;
          q += (uint64_t)v * v;
          mx = v > mx ? v : mx;
          w[e / PW] |= (uint32_t)(T)v << (8 * (int)sizeof(T) * (e % PW));
        }
      }
      if (out) reinterpret_cast<uint4 *>(out + r * pitch)[ch] = make_uint4(w[0], w[1], w[2], w[3]);
    }
    s = wsum64(s);
    q = wsum64(q);
    mx = wmax32(mx);
    if (lane == 0) {
      red[wave] = s;
      red[NW + wave] = q;
      red[2 * NW + wave] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      uint64_t ts = 0, tq = 0, tm = 0;
#pragma unroll
      for (int w = 0; w < NW; w++) {
        ts += red[w];
        tq += red[NW + w];
        tm = red[2 * NW + w] > tm ? red[2 * NW + w] : tm;
      }
      if (out) {
        mag[r] = ts;
        sumsq[r] = tq;
      }
      bmax = (uint32_t)tm > bmax ? (uint32_t)tm : bmax;
    }
  }
  if (threadIdx.x == 0 && bmax) atomicMax(gmax, (unsigned long long)bmax);
}

struct OrientRun {
  uint64_t first;  // the run's first pair
  uint32_t count;  // 1..RUN pairs, all with this b
  uint32_t b;
};

// |x - y| summed over the four bytes / two halves of a word
template <typename T>
__device__ __forceinline__ uint32_t sad_word(uint32_t x, uint32_t y, uint32_t acc);
template <>
__device__ __forceinline__ uint32_t sad_word<uint8_t>(uint32_t x, uint32_t y, uint32_t acc) {
  return __builtin_amdgcn_sad_u8(x, y, acc);
}
template <>
__device__ __forceinline__ uint32_t sad_word<uint16_t>(uint32_t x, uint32_t y, uint32_t acc) {
  const int d0 = (int)(x & 0xffffu) - (int)(y & 0xffffu), d1 = (int)(x >> 16) - (int)(y >> 16);
  return acc + (uint32_t)(d0 < 0 ? -d0 : d0) + (uint32_t)(d1 < 0 ? -d1 : d1);
}

template <typename T>
__global__ __launch_bounds__(NT) void orient_kernel(const uint8_t *__restrict__ fwd, uint64_t pitch, int B, int k,
                                                    const uint32_t *__restrict__ a, const OrientRun *__restrict__ runs,
                                                    uint32_t nruns, uint8_t *__restrict__ strand,
                                                    uint64_t *__restrict__ sad) {
  extern __shared__ __attribute__((aligned(16))) uint4 tl[];  // row_b, then row_b permuted: nch chunks each
  constexpr int E = 16 / (int)sizeof(T);
  constexpr int PW = 4 / (int)sizeof(T);
  const int nch = (int)(pitch / 16);
  const T *src = reinterpret_cast<const T *>(tl);
  const int g = threadIdx.x >> 4, l = threadIdx.x & 15;
  for (uint32_t ri = blockIdx.x; ri < nruns; ri += gridDim.x) {
    const OrientRun R = runs[ri];
    const uint4 *rowb = reinterpret_cast<const uint4 *>(fwd + (uint64_t)R.b * pitch);
    __syncthreads();  // (the previous run's reads are done)
    for (int ch = threadIdx.x; ch < nch; ch += NT) tl[ch] = rowb[ch];
    __syncthreads();
    for (int ch = threadIdx.x; ch < nch; ch += NT) {
      uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
      for (int e = 0; e < E; e++) {
        const int i = ch * E + e;
        if (i < B) w[e / PW] |= (uint32_t)src[mc::rc_index((uint32_t)i, k)] << (8 * (int)sizeof(T) * (e % PW));
      }
      tl[nch + ch] = make_uint4(w[0], w[1], w[2], w[3]);
    }
    __syncthreads();
    for (uint32_t j = (uint32_t)g; j < R.count; j += NT / 16) {
      const uint64_t p = R.first + j;
      const uint4 *rowa = reinterpret_cast<const uint4 *>(fwd + (uint64_t)a[p] * pitch);
      uint32_t sp = 0, sm = 0;
      if (B >= E) {  // whole chunks (every k but 1)
        for (int ch = l; ch < nch; ch += 16) {
          const uint4 x = rowa[ch], y = tl[ch], z = tl[nch + ch];
          sp = sad_word<T>(x.x, y.x, sp);
          sp = sad_word<T>(x.y, y.y, sp);
          sp = sad_word<T>(x.z, y.z, sp);
          sp = sad_word<T>(x.w, y.w, sp);
          sm = sad_word<T>(x.x, z.x, sm);
          sm = sad_word<T>(x.y, z.y, sm);
          sm = sad_word<T>(x.z, z.z, sm);
          sm = sad_word<T>(x.w, z.w, sm);
        }
      } else if (l == 0) {  // k = 1: four bins of one chunk, whatever the forward row's pad holds
        const T *ra = reinterpret_cast<const T *>(rowa);
        for (int i = 0; i < B; i++) {
          const int x = (int)ra[i], dp = x - (int)src[i], dm = x - (int)src[mc::rc_index((uint32_t)i, k)];
          sp += (uint32_t)(dp < 0 ? -dp : dp);
          sm += (uint32_t)(dm < 0 ? -dm : dm);
        }
      }
#pragma unroll
      for (int o = 8; o >= 1; o >>= 1) {
        sp += __shfl_xor(sp, o, 16);
        sm += __shfl_xor(sm, o, 16);
      }
      if (l == 0) {
        strand[p] = sm < sp ? 1 : 0;
        if (sad) {
          sad[2 * p] = sp;
          sad[2 * p + 1] = sm;
        }
      }
    }
  }
}

}  // namespace

// the fold over the n forward rows d_in (the context's k, width, pitch): canonical rows, mag and
// sumsq to d_out / the context's mag and sumsq (d_out null: none of them), the largest canonical
// bin to *d_max (zeroed by the caller); timed as F_LAYOUT
int launch_canon_rows(mc_ctx *c, const uint8_t *d_in, uint8_t *d_out, uint64_t *d_max) {
  const unsigned grid = (unsigned)std::min<uint64_t>(c->n, 8192);
  const size_t lds = (size_t)c->pitch + 3 * NW * sizeof(uint64_t);
  timed_begin(c);
  if (c->width == 1)
    canon_rows_kernel<uint8_t><<<grid, NT, lds, c->stream>>>(d_in, c->n, c->pitch, c->B, c->k, d_out, (uint64_t *)c->mag.p,
                                                            (uint64_t *)c->sumsq.p, (unsigned long long *)d_max);
  else
    canon_rows_kernel<uint16_t><<<grid, NT, lds, c->stream>>>(d_in, c->n, c->pitch, c->B, c->k, d_out, (uint64_t *)c->mag.p,
                                                             (uint64_t *)c->sumsq.p, (unsigned long long *)d_max);
  timed_end(c, F_LAYOUT);
  MCG_CHECK(hipGetLastError());
  return MC_OK;
}

// the strands (and, d_sad given, both sums) of the m pairs (d_a[p], h_b[p]) on the forward rows
// d_fwd; h_b is cut into runs of equal b here and uploaded as the run list (d_runs: scratch)
int launch_orient(mc_ctx *c, const uint8_t *d_fwd, const uint32_t *d_a, const uint32_t *h_b, uint64_t m, Buf &runs_buf,
                  uint8_t *d_strand, uint64_t *d_sad) {
  std::vector<OrientRun> runs;
  for (uint64_t p = 0; p < m;) {
    uint64_t e = p + 1;
    while (e < m && e - p < (uint64_t)RUN && h_b[e] == h_b[p]) e++;
    runs.push_back(OrientRun{p, (uint32_t)(e - p), h_b[p]});
    p = e;
  }
  if (runs.empty()) return MC_OK;
  if (int rc = ensure(runs_buf, runs.size() * sizeof(OrientRun) + 16)) return rc;
  if (int rc = stage_h2d(c, runs_buf.p, runs.data(), runs.size() * sizeof(OrientRun))) return rc;
  const unsigned grid = (unsigned)std::min<uint64_t>(runs.size(), 1u << 16);
  const size_t lds = 2 * (size_t)c->pitch;
  timed_begin(c);
  if (c->width == 1)
    orient_kernel<uint8_t><<<grid, NT, lds, c->stream>>>(d_fwd, c->pitch, c->B, c->k, d_a, (const OrientRun *)runs_buf.p,
                                                        (uint32_t)runs.size(), d_strand, d_sad);
  else
    orient_kernel<uint16_t><<<grid, NT, lds, c->stream>>>(d_fwd, c->pitch, c->B, c->k, d_a, (const OrientRun *)runs_buf.p,
                                                         (uint32_t)runs.size(), d_strand, d_sad);
  timed_end(c, F_PAIRS);
  MCG_CHECK(hipGetLastError());
  return MC_OK;
}

}  // namespace mcg
