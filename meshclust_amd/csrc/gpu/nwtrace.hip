// nwtrace.hip -- the alignment behind an NW identity: a forward pass that records every cell's
// predecessor choices, and a traceback that turns them into CIGAR operations.
//
// utility::GlobAlignE (GlobAlignE.cpp:123-291) keeps no path: each DP state carries (score, path
// length, identities) and a cell copies the payload of the predecessor it chose.  The payload at
// (la, lb) therefore travelled along exactly one chain of choices, and with the reference's fixed
// tie rules that chain is one alignment.  The kernels of nw.hip report its length and identities;
// the kernels here return the chain itself.  
//
// Recurrences, boundary rows / columns, the finite "-infinity" and the tie rules are nw.hip's
// (rows i over seq1, columns j over seq2):
//   Y(i,j) [upperGap] = max(M(i,j-1) - (o+e), Y(i,j-1) - e)          ties: from M
//   M(i,j) [matches]  = max(M, X, Y at (i-1,j-1)) + s(i,j)           ties: M, then X, then Y
//   X(i,j) [lowerGap] = max(M(i-1,j) - (o+e), X(i-1,j) - e)          ties: from M
// in plain scores (this pass is bound by its stores, not by its VALU count).
//
// Forward (nwt_forward_kernel<R>): one wavefront per pair, lane l owns R consecutive rows and
// works column t - l + 1 at step t, the bottom row of lane l-1 arriving through one DPP lane
// shift per value; a pair of more than 64 R rows is worked in row blocks one after the other, the
// block's bottom row kept in global scratch (3 ints per column).  Scores only.  Per cell 4 bits:
//   bits 0-1  the state at (i-1,j-1) M(i,j) took: 0 = M, 1 = X, 2 = Y
//   bit 2     X(i,j) came from X(i-1,j)   (0: from M)
//   bit 3     Y(i,j) came from Y(i,j-1)   (0: from M)
// A lane's R cells of one step make one word of 4 R bits (16, 32 or 64), stored at
//   word[(block * (lb + 63) + t) * 64 + lane]
// so the 64 stores of a wave step are one contiguous run of 128, 256 or 512 bytes.  The choice
// bytes of a pair:  ceil(la / (64 R)) * (lb + 63) * 32 R.
// Every loop has a trip count fixed on entry; nothing waits for another workgroup.
//
// Traceback (nwt_traceback_kernel): a thread per pair.  From the first maximum of M, X, Y at
// (la, lb) it follows the recorded choices: in M it emits = or X and moves to (i-1,j-1), in X
// (lowerGap, a base of seq1 alone) I and (i-1,j), in Y (upperGap, a base of seq2 alone) D and
// (i,j-1); at row 0 the j bases left are one run of D, at column 0 the i left one run of I (every
// boundary state of the reference has the path length of the bases left).  Each step consumes a
// base, so the walk ends within la + lb steps; a choice word that names no state, or a walk
// that is not at a boundary by then, sets the launch's error word.  The operations are run-length
// encoded as they come, the walk filling the pair's region of la + lb words from its END downwards:
// the walk runs from the alignment's end to its start, so the words come to lie in alignment
// order.  nwt_pack_kernel then copies every pair's words to their place in the call's output.
#include <algorithm>

#include "../host/band.hpp"
#include "mcgpu.hpp"

namespace mcg {

namespace {

constexpr int GO = 2, GE = 1, MATCH = 1, MISMATCH = -1;

__device__ __forceinline__ int dpp_shr1(int v) { return __builtin_amdgcn_mov_dpp(v, 0x138, 0xf, 0xf, false); }

template <int R>
struct ChoiceWord;
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

template <int R>
__global__ __launch_bounds__(64) void nwt_forward_kernel(TraceArgs q) {
  using W = typename ChoiceWord<R>::type;
  constexpr int ROWS = 64 * R;
  const uint32_t slot = blockIdx.x;
  if (slot >= q.npairs) return;
  const uint32_t p = q.pidx[slot];
  const TracePair pr = q.pairs[p];
  const uint8_t *a = (pr.a_rc ? q.rc : q.codes) + pr.a_off;
  const uint8_t *b = q.codes + pr.b_off;
  const int la = (int)pr.la, lb = (int)pr.lb;
  const int lane = (int)threadIdx.x;
  const int NINF = neg_inf(la, lb);
  int *bnd = q.bnd + pr.bnd_off;  // 3 ints per column 0 .. lb (pairs of more than one block)
  W *ch = reinterpret_cast<W *>(q.choice + pr.ch_off);
  const int nblk = (la + ROWS - 1) / ROWS;
  const int steps = lb + 63;
  int32_t *res = q.res + (uint64_t)p * TRACE_RES;
  if (la == 0) {
    // no rows: only cell 0 of each state row exists and the final maximum picks `matches`
    // (nw.hip): score -inf with columns, 0 without; the traceback emits lb D
    if (lane == 0) {
      res[0] = lb > 0 ? NINF : 0;
      res[4] = 0;
    }
    return;
  }
  for (int blk = 0; blk < nblk; blk++) {
    const int itop = blk * ROWS + lane * R + 1;  // first row of this lane
    uint8_t ac[R];
    int M[R], X[R], Y[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
      const int i = itop + r;
      ac[r] = i <= la ? a[i - 1] : (uint8_t)0xFF;
      M[r] = NINF;  // column 0 (GlobAlignE.cpp:150-160)
      Y[r] = NINF;
      X[r] = -GO - i * GE;
    }
    int dM, dX, dY;  // the cell above this lane's first row, one column back
    if (itop == 1) {
      dM = 0;  // (0, 0): GlobAlignE.cpp:137-139, and upperGapLag at j = 1 (:168)
      dX = NINF;
      dY = -GO;
    } else {
      dM = NINF;
      dX = -GO - (itop - 1) * GE;
      dY = NINF;
    }
    int oM = NINF, oX = NINF, oY = NINF, ob = 0;
    // seq2 codes for lane 0: one 64-byte block per 64 steps, lane l holding byte l, loaded a
    // block ahead and read with a uniform readlane
    int bcur = 0, bnext = lane < lb ? b[lane] : 0;
    // lane 0's hand-in from the block above, loaded a step ahead
    int nM = NINF, nX = NINF, nY = NINF;
    if (blk > 0 && lane == 0 && lb >= 1) {
      nM = bnd[3];
      nX = bnd[4];
      nY = bnd[5];
    }
    W *chb = ch + (uint64_t)blk * (uint64_t)steps * 64u;
    const bool mine = itop <= la;  // this lane has a row of the matrix
    for (int t = 0; t < steps; t++) {
      const int j = t - lane + 1;  // column of this lane at this step
      if ((t & 63) == 0) {
        bcur = bnext;
        const int nx = t + 64 + lane;
        bnext = nx < lb ? b[nx] : 0;
      }
      const int b0 = __builtin_amdgcn_readlane(bcur, t & 63);
      int uM = dpp_shr1(oM), uX = dpp_shr1(oX), uY = dpp_shr1(oY);
      int bc = dpp_shr1(ob);
      const bool in = j >= 1 && j <= lb;
      if (lane == 0) {
        bc = in ? b0 : 0;
        if (in) {
          if (blk == 0) {  // row 0: M = X = -inf, Y = -o - j e
            uM = NINF;
            uX = NINF;
            uY = -GO - j * GE;
          } else {  // the bottom row of the block above at column j
            uM = nM;
            uX = nX;
            uY = nY;
            if (j + 1 <= lb) {
              nM = bnd[3 * (j + 1)];
              nX = bnd[3 * (j + 1) + 1];
              nY = bnd[3 * (j + 1) + 2];
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
          const uint32_t nib = code | (xFromM ? 0u : 4u) | (yFromM ? 0u : 8u);
          word |= (W)((W)nib << (4 * r));
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
        if (mine) chb[(uint64_t)t * 64u + (uint32_t)lane] = word;
        if (lane == 63 && blk + 1 < nblk) {
          bnd[3 * j] = oM;
          bnd[3 * j + 1] = oX;
          bnd[3 * j + 2] = oY;
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
      res[0] = sc;
      res[4] = sc == mM ? 0 : (sc == mX ? 1 : 2);
    }
    __threadfence_block();
    __syncthreads();
  }
}

__device__ __forceinline__ uint32_t load_nibble(const uint8_t *base, uint64_t idx, int R, int r) {
  if (R == 4) return (uint32_t)(reinterpret_cast<const uint16_t *>(base)[idx] >> (4 * r)) & 15u;
  if (R == 8) return (reinterpret_cast<const uint32_t *>(base)[idx] >> (4 * r)) & 15u;
  return (uint32_t)(reinterpret_cast<const uint64_t *>(base)[idx] >> (4 * r)) & 15u;
}

__global__ __launch_bounds__(64) void nwt_traceback_kernel(TraceArgs q) {
  const uint32_t p = blockIdx.x * 64u + threadIdx.x;
  if (p >= q.npairs) return;
  const TracePair pr = q.pairs[p];
  const uint8_t *a = (pr.a_rc ? q.rc : q.codes) + pr.a_off;
  const uint8_t *b = q.codes + pr.b_off;
  const int la = (int)pr.la, lb = (int)pr.lb;
  const int R = (int)pr.r, ROWS = 64 * R;
  const uint64_t steps = (uint64_t)lb + 63;
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
    const uint64_t idx = ((uint64_t)blk * steps + (uint64_t)(j - 1 + lane)) * 64u + (uint32_t)lane;
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

// pair p's words, the last res[3] of its region, to out[dst[p] ...): a workgroup per pair
__global__ __launch_bounds__(64) void nwt_pack_kernel(TraceArgs q, const uint64_t *__restrict__ dst, uint32_t *__restrict__ out) {
  const uint32_t p = blockIdx.x;
  if (p >= q.npairs) return;
  const TracePair pr = q.pairs[p];
  const uint32_t n = (uint32_t)q.res[(uint64_t)p * TRACE_RES + 3], cap = pr.la + pr.lb;
  if (n > cap) return;
  const uint32_t *src = q.ops + pr.ops_off + (cap - n);
  uint32_t *o = out + dst[p];
  for (uint32_t k = threadIdx.x; k < n; k += 64) o[k] = src[k];
}

}  // namespace

int nw_trace_rows(uint64_t la) { return mc::full_rows_per_lane(la); }

uint64_t nw_trace_choice_bytes(uint64_t la, uint64_t lb) { return mc::full_choice_bytes(la, lb); }

int launch_nw_trace(mc_ctx *c, const std::vector<TracePair> &h_pairs, const TracePair *d_pairs, const uint8_t *d_rc,
                    uint8_t *d_choice, int *d_bnd, uint32_t *d_ops, int32_t *d_res, int *d_err) {
  const size_t m = h_pairs.size();
  if (m == 0) return MC_OK;
  std::vector<uint32_t> bucket[4];  // R = 4, 8, 16; the banded pairs (nwband.hip)
  for (size_t i = 0; i < m; i++)
    bucket[h_pairs[i].w >= 0 ? 3 : h_pairs[i].r == 4 ? 0 : h_pairs[i].r == 8 ? 1 : 2].push_back((uint32_t)i);
  if (ensure(c->tr_idx, m * 4 + 16)) return MC_ERR_OOM;
  TraceArgs q{(const uint8_t *)c->codes.p, d_rc, d_pairs, nullptr, 0, d_choice, d_bnd, d_res, d_ops, d_err};
  MCG_CHECK(hipMemsetAsync(d_err, 0, 4, c->stream));
  timed_begin(c);
  size_t io = 0;
  for (int k = 0; k < 4; k++) {
    if (bucket[k].empty()) continue;
    uint32_t *d_idx = (uint32_t *)c->tr_idx.p + io;
    if (int rc = stage_h2d(c, d_idx, bucket[k].data(), bucket[k].size() * 4)) return rc;
    q.pidx = d_idx;
    q.npairs = (uint32_t)bucket[k].size();
    if (k == 0) nwt_forward_kernel<4><<<q.npairs, 64, 0, c->stream>>>(q);
    else if (k == 1) nwt_forward_kernel<8><<<q.npairs, 64, 0, c->stream>>>(q);
    else if (k == 2) nwt_forward_kernel<16><<<q.npairs, 64, 0, c->stream>>>(q);
    else if (int rc = launch_nwband_forward(c, q)) return rc;
    MCG_CHECK(hipGetLastError());
    io += bucket[k].size();
  }
  timed_end(c, F_NW_FWD);
  q.pidx = nullptr;
  q.npairs = (uint32_t)m;
  timed_begin(c);
  if (bucket[3].empty()) nwt_traceback_kernel<<<(unsigned)((m + 63) / 64), 64, 0, c->stream>>>(q);
  else if (int rc = launch_nwband_traceback(c, q)) return rc;  // (a batch with a banded pair: the walk that knows both records)
  MCG_CHECK(hipGetLastError());
  timed_end(c, F_NW_TB);
  return MC_OK;
}

int launch_nw_pack(mc_ctx *c, uint32_t m, const TracePair *d_pairs, const uint32_t *d_ops, const int32_t *d_res,
                   const uint64_t *d_dst, uint32_t *d_out) {
  if (m == 0) return MC_OK;
  TraceArgs q{nullptr, nullptr, d_pairs, nullptr, m, nullptr, nullptr, const_cast<int32_t *>(d_res),
              const_cast<uint32_t *>(d_ops), nullptr};
  timed_begin(c);
  nwt_pack_kernel<<<m, 64, 0, c->stream>>>(q, d_dst, d_out);
  MCG_CHECK(hipGetLastError());
  timed_end(c, F_NW_TB);
  return MC_OK;
}

}  // namespace mcg
