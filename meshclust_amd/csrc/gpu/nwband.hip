// nwband.hip -- the banded choice record of an alignment: nwtrace.hip's forward
// pass over a window of columns per row block instead of the whole row, its score-only form for the
// width search, and a traceback that addresses either record.
//
// Geometry, certificate and bytes are host/band.hpp's.  For a pair with w >= 0, block k covers rows
// r0 = k ROWS + 1 .. r1 = min(la, (k + 1) ROWS) and sweeps the columns c0 = max(1, r0 + dlo) ..
// c1 = min(lb, r1 + dhi) (dlo = min(0, lb - la) - w, dhi = max(0, lb - la) + w): the region.  Every
// state outside the region is the sentinel -2^30:
//   - left of c0, unless c0 = 1: then column 0's real values (GlobAlignE.cpp:150-160) apply;
//   - above the block, for the columns the block before did not sweep;
//   - row 0 is real for block 0's columns (block 0 always starts at column 1).
// A sentinel loses at most 3 per step over fewer than 2^27 steps, so it never wraps and never wins
// against a state of the full matrix; every banded value is <= the full value of the same state.
//
// Forward (nwb_forward_kernel<R, STORE>): nwtrace.hip's shape -- one wavefront per pair, lane l owns
// R consecutive rows and works column c0 + t - l at step t, the bottom row of lane l - 1 arriving
// through one DPP lane shift per value, the block's bottom row kept in global scratch, 3 ints per
// column of the window at index j - c0 (the next block reads index j - c0 of the block before while
// it writes index j - c0 of its own, which is never ahead of its reads: its c0 is no smaller).  Choice
// words as nwtrace.hip's, at
//   word[(block * steps + t) * 64 + lane],  steps = min(lb, ROWS + |lb - la| + 2 w) + 63
// for every block alike, so the traceback finds cell (i, j) in closed form.  STORE = false drops the
// choice stores: the score-only form of the width search, which writes the score alone.
// Every loop has a trip count fixed on entry; nothing waits for another workgroup.
//
// Traceback (nwb_traceback_kernel): nwtrace.hip's walk, a thread per pair, over a batch that holds
// banded pairs (w >= 0) and full ones (w < 0).  A walk that would read a cell outside its block's
// window sets the launch's error word: the certificate says it cannot happen.
#include <algorithm>

#include "../host/band.hpp"
#include "mcgpu.hpp"

namespace mcg {

namespace {

constexpr int GO = 2, GE = 1, MATCH = 1, MISMATCH = -1;
constexpr int SENT = mc::BAND_SENTINEL;

__device__ __forceinline__ int dpp_shr1(int v) { return __builtin_amdgcn_mov_dpp(v, 0x138, 0xf, 0xf, false); }

template <int R>
struct ChoiceWord;
template <>
struct ChoiceWord<2> {
  using type = uint8_t;
};
template <>
struct ChoiceWord<4> {
  using type = uint16_t;
};
template <>
struct ChoiceWord<8> {
  using type = uint32_t;
};
template <>
struct ChoiceWord<16> {
  using type = uint64_t;
};

__device__ __forceinline__ int neg_inf(int la, int lb) {  // GlobAlignE.cpp:125-135
  const int len1 = la + 1, len2 = lb + 1;
  const int shorter = (len2 < len1 ? len2 : len1) - 1;
  const int lenDiff = len2 > len1 ? len2 - len1 : len1 - len2;
  int maxDiff = 0;
  if (lenDiff >= 1) maxDiff += -GO - lenDiff * GE;
  return maxDiff + MISMATCH * shorter - 1;
}

template <int R, bool STORE>
__global__ __launch_bounds__(64) void nwb_forward_kernel(TraceArgs q) {
  using W = typename ChoiceWord<R>::type;
  constexpr int ROWS = 64 * R;
  const uint32_t slot = blockIdx.x;
  if (slot >= q.npairs) return;
  const uint32_t p = q.pidx ? q.pidx[slot] : slot;
  const TracePair pr = q.pairs[p];
  const int la = (int)pr.la, lb = (int)pr.lb, w = pr.w;
  if (la == 0 || lb == 0 || w < 0) return;  // (the host plans these as full pairs)
  const uint8_t *a = (pr.a_rc ? q.rc : q.codes) + pr.a_off;
  const uint8_t *b = q.codes + pr.b_off;
  const int lane = (int)threadIdx.x;
  const int NINF = neg_inf(la, lb);
  const int d = lb - la, dlo = (d < 0 ? d : 0) - w, dhi = (d > 0 ? d : 0) + w;
  const int cols = min(lb, ROWS + (d < 0 ? -d : d) + 2 * w);
  const int stride = cols + 63;  // wave steps between the choice words of two blocks
  int *bnd = q.bnd + pr.bnd_off;  // 3 ints per column of a window (pairs of more than one block)
  W *ch = STORE ? reinterpret_cast<W *>(q.choice + pr.ch_off) : nullptr;
  const int nblk = (la + ROWS - 1) / ROWS;
  int pc0 = 1, pc1 = 0;  // the window of the block above
  for (int blk = 0; blk < nblk; blk++) {
    const int r0 = blk * ROWS + 1, r1 = min(la, r0 + ROWS - 1);
    const int c0 = max(1, r0 + dlo), c1 = min(lb, r1 + dhi);
    const int ncol = c1 - c0 + 1, steps = ncol + 63;
    const int itop = r0 + lane * R;  // first row of this lane
    uint8_t ac[R];
    int M[R], X[R], Y[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
      const int i = itop + r;
      ac[r] = i <= la ? a[i - 1] : (uint8_t)0xFF;
      // column c0 - 1: column 0 (GlobAlignE.cpp:150-160), or outside the region
      M[r] = c0 == 1 ? NINF : SENT;
      Y[r] = c0 == 1 ? NINF : SENT;
      X[r] = c0 == 1 ? -GO - i * GE : SENT;
    }
    int dM, dX, dY;  // the cell above this lane's first row, one column back: (itop - 1, c0 - 1)
    if (c0 == 1) {
      if (itop == 1) {
        dM = 0;  // (0, 0): GlobAlignE.cpp:137-139, and upperGapLag at j = 1 (:168)
        dX = NINF;
        dY = -GO;
      } else {
        dM = NINF;
        dX = -GO - (itop - 1) * GE;
        dY = NINF;
      }
    } else if (lane == 0) {  // c0 > 1: not block 0, and pc0 <= c0 - 1 <= pc1 (the block above swept it)
      dM = bnd[3 * (c0 - 1 - pc0)];
      dX = bnd[3 * (c0 - 1 - pc0) + 1];
      dY = bnd[3 * (c0 - 1 - pc0) + 2];
    } else {
      dM = dX = dY = SENT;
    }
    int oM = SENT, oX = SENT, oY = SENT, ob = 0;
    // seq2 codes for lane 0: one 64-byte block per 64 steps, lane l holding byte l, loaded a
    // block ahead and read with a uniform readlane
    const uint8_t *bw = b + (c0 - 1);
    int bcur = 0, bnext = lane < ncol ? bw[lane] : 0;
    // lane 0's hand-in from the block above, loaded a step ahead
    int nM = SENT, nX = SENT, nY = SENT;
    if (blk > 0 && lane == 0 && c0 >= pc0 && c0 <= pc1) {
      nM = bnd[3 * (c0 - pc0)];
      nX = bnd[3 * (c0 - pc0) + 1];
      nY = bnd[3 * (c0 - pc0) + 2];
    }
    W *chb = STORE ? ch + (uint64_t)blk * (uint64_t)stride * 64u : nullptr;
    const bool mine = itop <= la;  // this lane has a row of the matrix
    for (int t = 0; t < steps; t++) {
      const int j = c0 + t - lane;  // column of this lane at this step
      if ((t & 63) == 0) {
        bcur = bnext;
        const int nx = t + 64 + lane;
        bnext = nx < ncol ? bw[nx] : 0;
      }
      const int b0 = __builtin_amdgcn_readlane(bcur, t & 63);
      int uM = dpp_shr1(oM), uX = dpp_shr1(oX), uY = dpp_shr1(oY);
      int bc = dpp_shr1(ob);
      const bool in = j >= c0 && j <= c1;
      if (lane == 0) {
        bc = in ? b0 : 0;
        if (in) {
          if (blk == 0) {  // row 0: M = X = -inf, Y = -o - j e
            uM = NINF;
            uX = NINF;
            uY = -GO - j * GE;
          } else {  // the bottom row of the block above at column j, where it swept one
            uM = nM;
            uX = nX;
            uY = nY;
            nM = nX = nY = SENT;
            if (j + 1 <= c1 && j + 1 >= pc0 && j + 1 <= pc1) {
              nM = bnd[3 * (j + 1 - pc0)];
              nX = bnd[3 * (j + 1 - pc0) + 1];
              nY = bnd[3 * (j + 1 - pc0) + 2];
            }
          }
        }
      }
      if (in) {
        int aM = uM, aX = uX;             // (i-1, j)
        int gM = dM, gX = dX, gY = dY;    // (i-1, j-1)
        W word = 0;
#pragma unroll
        for (int r = 0; r < R; r++) {
          const int pM = M[r], pX = X[r], pY = Y[r];  // (i, j-1)
          const int yb = pM - (GO + GE), yc = pY - GE;  // upperGap (GlobAlignE.cpp:175-193)
          const bool yFromM = yb >= yc;
          const int Yn = yFromM ? yb : yc;
          const int sc = ac[r] == (uint8_t)bc ? MATCH : MISMATCH;  // matches (:197-241)
          int best = gM;
          uint32_t code = 0;
          if (gX > best) {
            best = gX;
            code = 1;
          }
          if (gY > best) {
            best = gY;
            code = 2;
          }
          const int Mn = best + sc;
          const int xb = aM - (GO + GE), xc = aX - GE;  // lowerGap (:258-272)
          const bool xFromM = xb >= xc;
          const int Xn = xFromM ? xb : xc;
          if (STORE) {
            const uint32_t nib = code | (xFromM ? 0u : 4u) | (yFromM ? 0u : 8u);
            word |= (W)((W)nib << (4 * r));
          }
          M[r] = Mn;
          X[r] = Xn;
          Y[r] = Yn;
          aM = Mn;
          aX = Xn;
          gM = pM;
          gX = pX;
          gY = pY;
        }
        dM = uM;
        dX = uX;
        dY = uY;
        oM = M[R - 1];
        oX = X[R - 1];
        oY = Y[R - 1];
        if (STORE && mine) chb[(uint64_t)t * 64u + (uint32_t)lane] = word;
        if (lane == 63 && blk + 1 < nblk) {
          bnd[3 * (j - c0)] = oM;
          bnd[3 * (j - c0) + 1] = oX;
          bnd[3 * (j - c0) + 2] = oY;
        }
      }
      ob = bc;
    }
    const int fl = la - blk * ROWS - 1;  // the last row, if it is in this block
    if (fl >= 0 && fl < ROWS && lane == fl / R) {
      const int r = fl % R;
      int mM = 0, mX = 0, mY = 0;
#pragma unroll
      for (int rr = 0; rr < R; rr++)
        if (rr == r) {
          mM = M[rr];
          mX = X[rr];
          mY = Y[rr];
        }
      int sc = mM > mX ? mM : mX;  // GlobAlignE.cpp:278-291
      sc = sc > mY ? sc : mY;
      if (STORE) {
        int32_t *res = q.res + (uint64_t)p * TRACE_RES;
        res[0] = sc;
        res[4] = sc == mM ? 0 : (sc == mX ? 1 : 2);
      } else {
        q.res[p] = sc;
      }
    }
    pc0 = c0;
    pc1 = c1;
    __threadfence_block();
    __syncthreads();
  }
}

__device__ __forceinline__ uint32_t load_nibble(const uint8_t *base, uint64_t idx, int R, int r) {
  if (R == 2) return (uint32_t)(base[idx] >> (4 * r)) & 15u;
  if (R == 4) return (uint32_t)(reinterpret_cast<const uint16_t *>(base)[idx] >> (4 * r)) & 15u;
  if (R == 8) return (reinterpret_cast<const uint32_t *>(base)[idx] >> (4 * r)) & 15u;
  return (uint32_t)(reinterpret_cast<const uint64_t *>(base)[idx] >> (4 * r)) & 15u;
}

__global__ __launch_bounds__(64) void nwb_traceback_kernel(TraceArgs q) {
  const uint32_t p = blockIdx.x * 64u + threadIdx.x;
  if (p >= q.npairs) return;
  const TracePair pr = q.pairs[p];
  const uint8_t *a = (pr.a_rc ? q.rc : q.codes) + pr.a_off;
  const uint8_t *b = q.codes + pr.b_off;
  const int la = (int)pr.la, lb = (int)pr.lb, w = pr.w;
  const bool banded = w >= 0;
  const int R = banded ? mc::BAND_R : (int)pr.r, ROWS = 64 * R;
  const int d = lb - la, dlo = (d < 0 ? d : 0) - w, dhi = (d > 0 ? d : 0) + w;
  const uint64_t steps = banded ? (uint64_t)min(lb, ROWS + (d < 0 ? -d : d) + 2 * w) + 63 : (uint64_t)lb + 63;
  const uint8_t *ch = q.choice + pr.ch_off;
  int32_t *res = q.res + (uint64_t)p * TRACE_RES;
  uint32_t *ops = q.ops + pr.ops_off;
  const uint32_t cap = (uint32_t)(la + lb);  // this pair's region: at most one word per base
  uint32_t pos = cap;
  uint32_t cur = 0, run = 0;
  int ncol = 0, nid = 0;
  auto emit = [&](uint32_t op, uint32_t n) {
    if (n == 0) return;
    if (op == cur) {
      run += n;
      return;
    }
    if (run > 0 && pos > 0) ops[--pos] = run << 4 | cur;
    cur = op;
    run = n;
  };
  int i = la, j = lb, state = res[4];
  bool bad = false;
  const int limit = la + lb;
  for (int s = 0; s < limit && i > 0 && j > 0; s++) {
    const int blk = (i - 1) / ROWS, lr = (i - 1) - blk * ROWS;
    const int lane = lr / R, r = lr - lane * R;
    int first = 1;  // the column of the block's wave step 0 in lane 0
    if (banded) {
      const int r0 = blk * ROWS + 1, r1 = min(la, r0 + ROWS - 1);
      first = max(1, r0 + dlo);
      if (j < first || j > min(lb, r1 + dhi)) {  // outside the window: the certificate did not hold
        bad = true;
        break;
      }
    }
    const uint64_t idx = ((uint64_t)blk * steps + (uint64_t)(j - first + lane)) * 64u + (uint32_t)lane;
    const uint32_t nib = load_nibble(ch, idx, R, r);
    ncol++;
    if (state == 0) {
      const bool eq = a[i - 1] == b[j - 1];
      emit(eq ? MC_CIGAR_EQ : MC_CIGAR_X, 1);
      nid += eq ? 1 : 0;
      state = (int)(nib & 3u);
      if (state == 3) {
        bad = true;
        break;
      }
      i--;
      j--;
    } else if (state == 1) {
      emit(MC_CIGAR_I, 1);
      state = (nib & 4u) ? 1 : 0;
      i--;
    } else {
      emit(MC_CIGAR_D, 1);
      state = (nib & 8u) ? 2 : 0;
      j--;
    }
  }
  if (bad || (i > 0 && j > 0)) {
    atomicOr(q.err, 1);
    res[1] = res[2] = res[3] = 0;
    return;
  }
  if (i == 0) {
    emit(MC_CIGAR_D, (uint32_t)j);
    ncol += j;
  } else {
    emit(MC_CIGAR_I, (uint32_t)i);
    ncol += i;
  }
  if (run > 0 && pos > 0) ops[--pos] = run << 4 | cur;
  res[1] = ncol;
  res[2] = nid;
  res[3] = (int32_t)(cap - pos);
}

}  // namespace

int launch_nwband_forward(mc_ctx *c, const TraceArgs &q) {
  if (q.npairs == 0) return MC_OK;
  nwb_forward_kernel<mc::BAND_R, true><<<q.npairs, 64, 0, c->stream>>>(q);
  MCG_CHECK(hipGetLastError());
  return MC_OK;
}

int launch_nwband_traceback(mc_ctx *c, const TraceArgs &q) {
  if (q.npairs == 0) return MC_OK;
  nwb_traceback_kernel<<<(q.npairs + 63) / 64, 64, 0, c->stream>>>(q);
  MCG_CHECK(hipGetLastError());
  return MC_OK;
}

int launch_nwband_scores(mc_ctx *c, uint32_t m, const TracePair *d_pairs, const uint8_t *d_rc, int *d_bnd, int32_t *d_score) {
  if (m == 0) return MC_OK;
  TraceArgs q{(const uint8_t *)c->codes.p, d_rc, d_pairs, nullptr, m, nullptr, d_bnd, d_score, nullptr, nullptr};
  timed_begin(c);
  nwb_forward_kernel<mc::BAND_R, false><<<m, 64, 0, c->stream>>>(q);
  MCG_CHECK(hipGetLastError());
  timed_end(c, F_NW_BAND);
  return MC_OK;
}

}  // namespace mcg
