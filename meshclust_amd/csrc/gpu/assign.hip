// assign.hip -- mc_assign: M queries x C centres -> the best similar centre of every query.
//
// Placing new reads into an existing clustering is all-pairs scoring with an argmax per query:
// pair (q, j) is feat->compute(query q, centre j) -- the query first, as Trainer::get_close
// scores a candidate against a centre (Trainer.cpp:34-114; scan_kernel, k2.hip) -- gated by the
// length window accumulate gives get_range (ClusterFactory.cpp:637-654), applied per point.
//
//   assign_short_kernel    8-bit rows of at most 16 chunks (k <= 4), the trainer's classifier
//                          layout, classify_small available: a query per lane, its row in 16
//                          uint4 registers, a tile of centres in LDS read at the same address by
//                          every lane (broadcast), v_sad_u8 + v_dot4_u32_u8 per chunk, then
//                          classify_small, and classify_std on the spot when it is undecided.
//                          The running (combo 0, index) and the similar count stay in registers:
//                          no cross-lane reduction, no atomics on the results.
//   assign_general_kernel  wider 8-bit rows, 16-bit bins or any other k-mer classifier: 16 lanes
//                          per query (distance_keys_kernel's second form), the centre tile in
//                          LDS, Acc<T> -> reduce16 -> finish, then classify_std (layout 3 / 4) or
//                          raw_fast + classify_raw.  The running result of a query lives in its
//                          output slots between tiles (always the same lane's).
//
// LDS tile: entry e = nch row chunks + 3 info chunks, at tile[e * (nch + 3)]:
//   short    {mag, len, ap | ~0 (PSm not ok), np}, {da, kq = mag - B ap}, {gate lo, gate hi}
//   general  {mag, sumsq}, {len, gate lo}, {gate hi, -}
// Both kernels are templates on the strand set (mc_assign_strands; mc_assign is plus alone).  The
// histogram of a reverse-complemented record is its row permuted by rc_index (host/strand.hpp),
// and every scorer input is a bin-wise sum, so score(rc(query), centre) == score(query,
// rc(centre)): revcomp_rows_kernel permutes the C centre rows once per call.  Minus alone reads
// the tile rows from that buffer; with both strands an entry is the forward row, the permuted row
// and the same 3 info chunks, at tile[e * (2 nch + 3)], each strand keeps its own running result
// and the two are combined at the end (minus wins only with a strictly larger combo 0).
// mc_assign_top reports the K best hits of a query instead of one: a single list for both strands,
// ordered on insertion by (combo 0 descending, plus before minus), equal ones in arrival order,
// which is index ascending (host/topk.hpp).  The short form holds it in the lane's registers
// (capacity 2, 4 or 8 as a template parameter), the general form in the query's output row.
// Every scorer here is one of features.hpp's (classify_small / classify_std / classify_raw),
// which return the same decision and combo 0 bit for bit, so the result equals what
// mc_classify_pairs gives for the same pair.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../host/strand.hpp"
#include "../host/topk.hpp"
#include "abi_util.hpp"
#include "features.hpp"

namespace mcg {

namespace {

constexpr int NT = 256;
constexpr int INFO = 3;                     // info chunks per tile entry
constexpr size_t TILE_BYTES = 60u * 1024;   // two workgroups per CU of 160 KiB, within the 64 KiB default
constexpr uint32_t NONE = MC_ASSIGN_NONE;

struct AssignArgs {
  HistView H;
  const uint32_t *cid;  // centre ids (C)
  const uint32_t *qid;  // query ids (M)
  const uint64_t *glo, *ghi;  // per centre: the length gate's bounds
  uint64_t M;
  uint32_t C, tile;
  int gate;
  uint32_t *best;
  double *bval;
  uint32_t *nsim;
  unsigned long long *stats;  // {candidate pairs, classify_std fall-backs}
  // strands (mc_assign_strands): the centres' permuted rows, row j for centre_ids[j], at the
  // histograms' pitch; with both strands the minus strand's running result between tiles
  // (general form) and the strand of the final result
  const uint8_t *rc;
  uint32_t *best_m;
  double *bval_m;
  uint32_t *nsim_m;
  uint8_t *strand;
  // the K best hits (mc_assign_top, K >= 2): row q of hit / hval / hstr holds K slots
  uint32_t K;
  uint32_t *hit;
  double *hval;
  uint8_t *hstr;
};

// S is the strand set (MC_STRAND_PLUS, MC_STRAND_MINUS or both): rows per tile entry
template <int S>
constexpr int rows_of = S == (MC_STRAND_PLUS | MC_STRAND_MINUS) ? 2 : 1;
// the strand of the hits of pass r (row r of an entry) with strand set S
template <int S>
__device__ __forceinline__ uint32_t strand_of(uint32_t r) {
  return S == (MC_STRAND_PLUS | MC_STRAND_MINUS) ? r : S == MC_STRAND_MINUS ? 1u : 0u;
}

// The two strands' running results change places: the entry loop scores into one set and swaps
// after every pass, so after the two passes of an entry both are back in place.
__device__ __forceinline__ void swap_strands(double &bv, uint32_t &bj, uint32_t &ns, double &bvm, uint32_t &bjm,
                                             uint32_t &nsm) {
  const double v = bv;
  bv = bvm;
  bvm = v;
  const uint32_t j = bj, n = ns;
  bj = bjm;
  bjm = j;
  ns = nsm;
  nsm = n;
}

// Both strands' results of one query into one: the minus strand wins only with a strictly larger
// combo 0 (or when the plus strand has no similar centre); the counts add.
__device__ __forceinline__ uint32_t combine_strands(double &bv, uint32_t &bj, uint32_t &ns, double bvm, uint32_t bjm,
                                                    uint32_t nsm) {
  const bool minus = bjm != NONE && (bj == NONE || bvm > bv);
  if (minus) {
    bv = bvm;
    bj = bjm;
  }
  ns += nsm;
  return minus ? 1u : 0u;
}

__device__ __forceinline__ PInfo pinfo(const HistView &H, uint32_t id) {
  return PInfo{H.mag[id], H.sumsq[id], H.len[id]};
}
__device__ __forceinline__ uint4 pack2(uint64_t a, uint64_t b) {
  return make_uint4((uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32));
}
__device__ __forceinline__ uint64_t lo64(const uint4 &v) { return (uint64_t)v.x | ((uint64_t)v.y << 32); }
__device__ __forceinline__ uint64_t hi64(const uint4 &v) { return (uint64_t)v.z | ((uint64_t)v.w << 32); }

// the rows of centres c0 .. c0 + cn into the tile (every thread of the workgroup): the forward
// row, the permuted row, or the forward row followed by the permuted one
template <int S>
__device__ __forceinline__ void load_tile_rows(const AssignArgs &A, uint4 *tl, uint32_t c0, uint32_t cn, int nch) {
  const uint32_t ent = (uint32_t)(rows_of<S> * nch) + INFO;
  for (uint32_t t = threadIdx.x; t < cn * (uint32_t)nch; t += NT) {
    const uint32_t cc = t / (uint32_t)nch, ch = t % (uint32_t)nch;
    if (S & MC_STRAND_PLUS)
      tl[cc * ent + ch] = reinterpret_cast<const uint4 *>(A.H.hist + (uint64_t)A.cid[c0 + cc] * A.H.pitch)[ch];
    if (S & MC_STRAND_MINUS)
      tl[cc * ent + (rows_of<S> - 1) * nch + ch] =
          reinterpret_cast<const uint4 *>(A.rc + (uint64_t)(c0 + cc) * A.H.pitch)[ch];
  }
}

// -------------------------------------------------------------------- short form
// KC is the capacity of the list of best hits: 1 is mc_assign / mc_assign_strands (one running
// result per strand, combined at the end); 2, 4 or 8 is mc_assign_top: one list for both strands
// in the lane's registers, ordered on insertion (host/topk.hpp), of which the first A.K slots are
// stored.  ns then counts the hits of both strands and nothing is swapped.
template <int S, int KC>
__global__ __launch_bounds__(NT) void assign_short_kernel(AssignArgs A, DevClassifier C, FastCls F) {
  extern __shared__ __attribute__((aligned(16))) uint4 tl[];
  __shared__ SmallK s_sk;
  const HistView &H = A.H;
  const int nch = (H.B + 15) / 16;
  constexpr int NR = rows_of<S>;
  const uint32_t ent = (uint32_t)(NR * nch) + INFO;
  if (threadIdx.x == 0) s_sk = make_smallk(C, F);
  const uint64_t i = (uint64_t)blockIdx.x * NT + threadIdx.x;
  const bool valid = i < A.M;
  const uint32_t q = valid ? A.qid[i] : A.qid[0];  // (an idle lane scores query 0 and stores nothing)
  uint4 mine[16];
  {
    const uint4 *row = reinterpret_cast<const uint4 *>(H.hist + (uint64_t)q * H.pitch);
#pragma unroll
    for (int c = 0; c < 16; c++) mine[c] = c < nch ? row[c] : make_uint4(0, 0, 0, 0);
  }
  PSm ps;
  uint64_t lenq;
  {
    const PInfo pq = pinfo(H, q);
    ps = psmall(pq, pterms(pq.mag, pq.sumsq, H.B));
    lenq = pq.len;
  }
  const double dap = C.layout == 4 ? mk_div((double)ps.mag, (double)H.B, F.rB) : 0.0;
  double bv = -1.0, bvm = -1.0;  // (the minus strand's running result: used with both strands only)
  uint32_t bj = NONE, ns = 0, bjm = NONE, nsm = 0, ncand = 0, nfb = 0;
  mc::TopK<KC> top;  // (KC > 1 only)
  if (KC > 1) top.clear();
  for (uint32_t c0 = 0; c0 < A.C; c0 += A.tile) {
    const uint32_t cn = min(A.tile, A.C - c0);
    __syncthreads();  // (the previous tile's reads are done)
    load_tile_rows<S>(A, tl, c0, cn, nch);
    for (uint32_t t = threadIdx.x; t < cn; t += NT) {
      const uint32_t id = A.cid[c0 + t];
      const PInfo pc = pinfo(H, id);
      const PTerms tc = pterms_mk(pc.mag, pc.sumsq, H.B, F.rB);
      const PSm pm = psmall(pc, tc);
      const double kq = (double)((int64_t)pc.mag - (int64_t)H.B * tc.ap);
      uint4 *info = tl + t * ent + NR * nch;
      info[0] = make_uint4(pm.mag, pm.len, pm.ok ? pm.ap : ~0u, pm.np);
      info[1] = pack2(__builtin_bit_cast(uint64_t, tc.da), __builtin_bit_cast(uint64_t, kq));
      info[2] = pack2(A.glo[c0 + t], A.ghi[c0 + t]);
    }
    __syncthreads();
    // Pass p scores row p % NR of entry p / NR against the query's registers (with both strands a
    // second pass over the entry, not a second copy of the query).  (bv, bj, ns) is the running
    // result of the strand being scored; the other one's waits in (bvm, bjm, nsm) and the two are
    // swapped after every pass -- an entry is gated as a whole, so the passes stay in step.
    for (uint32_t p = 0; p < cn * NR; p++) {
      const uint32_t e = p / NR, r = p % NR;
      const uint4 *ce = tl + e * ent;  // (the same address in every lane: broadcast reads)
      const uint4 *ci = ce + NR * nch;  // (the info chunks: the same for both strands)
      const uint4 *row = ce + r * nch;
      const uint4 g = ci[2];
      const bool pass = valid && (!A.gate || (lo64(g) <= lenq && lenq <= hi64(g)));
      if (__ballot(pass) == 0) continue;  // (uniform: no lane of this wave passes the gate)
      Acc<uint8_t> acc;
#pragma unroll
      for (int c = 0; c < 16; c++)
        if (c < nch) acc.add(mine[c], row[c]);
      if (pass) {
        if (r == 0) ncand++;
        const uint4 inf = ci[0];
        double cv = -1.0;
        int d = 0;
        bool und = true;
        if (ps.ok && inf.z != ~0u) {
          const uint4 i1 = ci[1];
          const SmallK sk = lds_smallk(&s_sk);
          const PSm pc{inf.x, inf.y, inf.z, inf.w, true};
          acc.fold();
          d = classify_small(sk, acc.sad, acc.dot, ps, pc, __builtin_bit_cast(double, hi64(i1)), dap,
                             __builtin_bit_cast(double, lo64(i1)), H.B, &cv, &und);
        }
        if (und) {  // classify_small undecided or not applicable: classify_std from the same sums
          nfb++;
          const uint32_t id = A.cid[c0 + e];
          const PInfo pq = pinfo(H, q), pc = pinfo(H, id);
          d = classify_std(C, acc.finish(pq.mag, pc.mag), pq, pterms(pq.mag, pq.sumsq, H.B), pc,
                           pterms(pc.mag, pc.sumsq, H.B), H.B, &cv);
        }
        if (d) {
          ns++;
          if constexpr (KC > 1) {
            mc::topk_insert(top, cv, c0 + e, strand_of<S>(r));
          } else if (bj == NONE || cv > bv) {  // (ascending j: a tie keeps the lowest index)
            bv = cv;
            bj = c0 + e;
          }
        }
      }
      if (NR == 2 && KC == 1) swap_strands(bv, bj, ns, bvm, bjm, nsm);
    }
  }
  if constexpr (KC > 1) {
    if (valid) {
#pragma unroll
      for (int t = 0; t < KC; t++)
        if ((uint32_t)t < A.K) {
          A.hit[i * A.K + t] = top.j[t];
          A.hval[i * A.K + t] = top.v[t];
          A.hstr[i * A.K + t] = (uint8_t)top.strand(t);
        }
      A.nsim[i] = ns;
    }
  } else {
    uint32_t st = 0;
    if (NR == 2) st = combine_strands(bv, bj, ns, bvm, bjm, nsm);
    if (valid) {
      A.best[i] = bj;
      A.bval[i] = bv;
      A.nsim[i] = ns;
      if (NR == 2) A.strand[i] = (uint8_t)st;
    }
  }
  ncand = wave_sum32_all(ncand);  // (<= 64 * C per wave)
  nfb = wave_sum32_all(nfb);
  if ((threadIdx.x & 63) == 0) {
    if (ncand) atomicAdd(&A.stats[0], (unsigned long long)ncand);
    if (nfb) atomicAdd(&A.stats[1], (unsigned long long)nfb);
  }
}

// -------------------------------------------------------------------- general form
// TOP (mc_assign_top): the list of best hits of a query lives in row q of the output buffers,
// A.K slots, and the owner lane inserts into it in memory at the moment of a hit
// (topk_insert_row); ns counts the hits of both strands and is all that waits in A.nsim.
template <typename T, int S, bool TOP>
__global__ __launch_bounds__(NT) void assign_general_kernel(AssignArgs A, DevClassifier C) {
  extern __shared__ __attribute__((aligned(16))) uint4 tl[];
  const HistView &H = A.H;
  const int nch = (int)((H.B * (int)sizeof(T) + 15) / 16);
  constexpr int NR = rows_of<S>;
  const uint32_t ent = (uint32_t)(NR * nch) + INFO;
  const int lane = threadIdx.x & 63, group = lane >> 4, lig = lane & 15, wave = wave_id();
  const int rows_per_block = 16;  // 4 waves x 4 groups
  const int per = (nch + 15) / 16;
  // chunks of the query's row kept in registers per lane (16-bit bins: fewer, their element
  // arithmetic is 64-bit); the rest of a wider row is streamed from global memory
  constexpr int RCH = sizeof(T) == 1 ? 16 : 4;
  uint32_t ncand = 0;
  for (uint32_t c0 = 0; c0 < A.C; c0 += A.tile) {
    const uint32_t cn = min(A.tile, A.C - c0);
    __syncthreads();
    load_tile_rows<S>(A, tl, c0, cn, nch);
    for (uint32_t t = threadIdx.x; t < cn; t += NT) {
      const PInfo pc = pinfo(H, A.cid[c0 + t]);
      uint4 *info = tl + t * ent + NR * nch;
      info[0] = pack2(pc.mag, pc.sumsq);
      info[1] = pack2(pc.len, A.glo[c0 + t]);
      info[2] = pack2(A.ghi[c0 + t], 0);
    }
    __syncthreads();
    for (uint64_t base = (uint64_t)blockIdx.x * rows_per_block; base < A.M; base += (uint64_t)gridDim.x * rows_per_block) {
      const uint64_t i = base + wave * 4 + group;
      const bool valid = i < A.M;
      const uint32_t id = valid ? A.qid[i] : A.qid[0];
      const uint8_t *row = H.hist + (uint64_t)id * H.pitch;
      uint4 mine[RCH];  // chunks lig, lig + 16, ..: both loops unrolled, so it stays in registers
#pragma unroll
      for (int u = 0; u < RCH; u++) {
        const int ch = lig + 16 * u;
        mine[u] = (u < per && ch < nch) ? reinterpret_cast<const uint4 *>(row)[ch] : make_uint4(0, 0, 0, 0);
      }
      const PInfo pq = pinfo(H, id);
      const PTerms tq = pterms(pq.mag, pq.sumsq, H.B);
      // the query's running result: its output slots between tiles (this lane wrote them)
      const bool owner = valid && lig == 0;
      double bv = -1.0, bvm = -1.0;  // (the minus strand's: used with both strands only)
      uint32_t bj = NONE, ns = 0, bjm = NONE, nsm = 0;
      if constexpr (TOP) {
        if (owner && c0 > 0) ns = A.nsim[i];
        if (owner && c0 == 0)
          for (uint32_t t = 0; t < A.K; t++) {  // empty slots
            A.hit[i * A.K + t] = NONE;
            A.hval[i * A.K + t] = -1.0;
            A.hstr[i * A.K + t] = 0;
          }
      } else if (owner && c0 > 0) {
        bv = A.bval[i];
        bj = A.best[i];
        ns = A.nsim[i];
        if (NR == 2) {
          bvm = A.bval_m[i];
          bjm = A.best_m[i];
          nsm = A.nsim_m[i];
        }
      }
      // Pass p scores row p % NR of entry p / NR.  (bv, bj, ns) is the running result of the strand
      // being scored; with both strands the other one's waits in (bvm, bjm, nsm) and the two are
      // swapped after every pass -- an entry is gated as a whole, so the passes stay in step.
      for (uint32_t p = 0; p < cn * NR; p++) {
        const uint32_t e = p / NR, r = p % NR;
        const uint4 *ce = tl + e * ent;
        const uint4 *ci = ce + NR * nch;  // (the info chunks: the same for both strands)
        const uint4 *crow = ce + r * nch;
        const uint4 i0 = ci[0], i1 = ci[1], i2 = ci[2];
        const bool pass = valid && (!A.gate || (hi64(i1) <= pq.len && pq.len <= lo64(i2)));
        if (__ballot(pass) == 0) continue;  // (uniform)
        Acc<T> acc;
#pragma unroll
        for (int u = 0; u < RCH; u++) {
          const int ch = lig + 16 * u;
          if (u < per && ch < nch) acc.add(mine[u], crow[ch]);
        }
        for (int ch = lig + 16 * RCH; ch < nch; ch += 16) acc.add(reinterpret_cast<const uint4 *>(row)[ch], crow[ch]);
        acc.reduce16();
        if (pass && lig == 0) {
          if (r == 0) ncand++;
          const PInfo pc{lo64(i0), hi64(i0), lo64(i1)};
          const PS s = acc.finish(pq.mag, pc.mag);
          double cv;
          int d;
          if (C.layout) {
            d = classify_std(C, s, pq, tq, pc, pterms(pc.mag, pc.sumsq, H.B), H.B, &cv);
          } else {
            double raw[MC_MAX_SINGLE];
#pragma unroll
            for (int f = 0; f < MC_MAX_SINGLE; f++) raw[f] = f < C.c.n_single ? raw_fast(C.c.lookup[f], s, pq, pc, H.B) : 0.0;
            d = classify_raw(C, raw, &cv, nullptr);
          }
          if (d) {
            if constexpr (TOP) {  // (pass && lig == 0: the owner lane)
              mc::topk_insert_row(A.hval + i * A.K, A.hit + i * A.K, A.hstr + i * A.K, A.K, min(ns, A.K), cv, c0 + e,
                                  strand_of<S>(r));
              ns++;
            } else {
              ns++;
              if (bj == NONE || cv > bv) {
                bv = cv;
                bj = c0 + e;
              }
            }
          }
        }
        if (NR == 2 && !TOP) swap_strands(bv, bj, ns, bvm, bjm, nsm);
      }
      if constexpr (TOP) {
        if (owner) A.nsim[i] = ns;
      } else if (owner) {
        if (NR == 2) {
          if (c0 + cn == A.C) {  // the last tile: both strands' results into one
            A.strand[i] = (uint8_t)combine_strands(bv, bj, ns, bvm, bjm, nsm);
          } else {
            A.best_m[i] = bjm;
            A.bval_m[i] = bvm;
            A.nsim_m[i] = nsm;
          }
        }
        A.best[i] = bj;
        A.bval[i] = bv;
        A.nsim[i] = ns;
      }
    }
  }
  ncand = wave_sum32_all(ncand);
  if (lane == 0 && ncand) atomicAdd(&A.stats[0], (unsigned long long)ncand);
}

// -------------------------------------------------------------------- the other strand's rows
// out row r = the row of point ids[r] permuted by rc_index: out[i] = row[rc_index(i)], the
// histogram of the reverse-complemented record.  A gather with a stride of 4^(k-1)
// between neighbouring output bins, so a workgroup stages the source row in LDS with full
// 16-byte loads, a thread gathers the 16 / sizeof(T) bins of one output chunk from LDS, and the
// stores are whole chunks in thread order.  Bins past B (a row shorter than a chunk) are zero.
template <typename T>
__global__ __launch_bounds__(NT) void revcomp_rows_kernel(HistView H, const uint32_t *ids, uint64_t m, uint8_t *out, int k) {
  extern __shared__ __attribute__((aligned(16))) uint4 tl[];
  constexpr int E = 16 / (int)sizeof(T);      // bins per chunk
  constexpr int PW = 4 / (int)sizeof(T);      // bins per 32-bit word
  const int nch = (int)(H.pitch / 16);        // (the pitch is the row rounded up to whole chunks)
  const T *src = reinterpret_cast<const T *>(tl);
  for (uint64_t r = blockIdx.x; r < m; r += gridDim.x) {
    const uint4 *row = reinterpret_cast<const uint4 *>(H.hist + (uint64_t)ids[r] * H.pitch);
    __syncthreads();  // (the previous row's reads are done)
    for (int ch = threadIdx.x; ch < nch; ch += NT) tl[ch] = row[ch];
    __syncthreads();
    uint4 *orow = reinterpret_cast<uint4 *>(out + r * H.pitch);
    for (int ch = threadIdx.x; ch < nch; ch += NT) {
      uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
      for (int e = 0; e < E; e++) {
        const int i = ch * E + e;
        if (i < H.B) w[e / PW] |= (uint32_t)src[mc::rc_index((uint32_t)i, k)] << (8 * (int)sizeof(T) * (e % PW));
      }
      orow[ch] = make_uint4(w[0], w[1], w[2], w[3]);
    }
  }
}

// the permuted rows of the m points d_ids into d_out (m rows at the histograms' pitch)
int launch_revcomp(mc_ctx *c, const HistView &H, const uint32_t *d_ids, uint64_t m, uint8_t *d_out) {
  const unsigned grid = (unsigned)std::min<uint64_t>(m, 8192);
  const size_t lds = (size_t)H.pitch;
  if (c->width == 1) revcomp_rows_kernel<uint8_t><<<grid, NT, lds, c->stream>>>(H, d_ids, m, d_out, c->k);
  else revcomp_rows_kernel<uint16_t><<<grid, NT, lds, c->stream>>>(H, d_ids, m, d_out, c->k);
  MCG_CHECK(hipGetLastError());
  return MC_OK;
}

// A.K == 1: one result per query; A.K >= 2 (mc_assign_top): the short form's next capacity up
// (2, 4 or 8), the general form's list in memory
template <int S>
void launch_assign(mc_ctx *c, const AssignArgs &A, bool is_short, uint64_t M, size_t lds) {
  if (is_short) {
    FastCls F = c->fcls;
    F.rB = 1.0 / (double)A.H.B;
    const unsigned grid = (unsigned)((M + NT - 1) / NT);
    if (A.K == 1) assign_short_kernel<S, 1><<<grid, NT, lds, c->stream>>>(A, c->cls, F);
    else if (A.K <= 2) assign_short_kernel<S, 2><<<grid, NT, lds, c->stream>>>(A, c->cls, F);
    else if (A.K <= 4) assign_short_kernel<S, 4><<<grid, NT, lds, c->stream>>>(A, c->cls, F);
    else assign_short_kernel<S, 8><<<grid, NT, lds, c->stream>>>(A, c->cls, F);
  } else {
    const unsigned grid = (unsigned)std::min<uint64_t>((M + 15) / 16, 1024);
    if (A.K == 1) {
      if (c->width == 1) assign_general_kernel<uint8_t, S, false><<<grid, NT, lds, c->stream>>>(A, c->cls);
      else assign_general_kernel<uint16_t, S, false><<<grid, NT, lds, c->stream>>>(A, c->cls);
    } else {
      if (c->width == 1) assign_general_kernel<uint8_t, S, true><<<grid, NT, lds, c->stream>>>(A, c->cls);
      else assign_general_kernel<uint16_t, S, true><<<grid, NT, lds, c->stream>>>(A, c->cls);
    }
  }
}
static_assert(MC_ASSIGN_MAX_TOP == 8, "assign_short_kernel's largest capacity");

// mc_assign (strands = MC_STRAND_PLUS, strand NULL), mc_assign_strands (K = 1: best, best_val and
// strand hold one entry per query) and mc_assign_top (K >= 2: they are the rows of hit, hit_val and
// hit_strand, K entries per query); `who` names the entry in error messages
int assign_impl(mc_ctx *c, const char *who, const uint32_t *centre_ids, uint32_t C, const uint32_t *query_ids, uint64_t M,
                double sim, int strands, uint32_t K, uint32_t *best, double *best_val, uint8_t *strand, uint32_t *n_similar,
                uint64_t *stats) {
  if (!c || c->k == 0 || !c->has_cls) return MC_ERR_STATE;
  const std::string w = who;
  if (strands < MC_STRAND_PLUS || strands > (MC_STRAND_PLUS | MC_STRAND_MINUS)) {
    set_error(w + ": strands must be MC_STRAND_PLUS, MC_STRAND_MINUS or both");
    return MC_ERR_ARG;
  }
  if (K < 1 || K > MC_ASSIGN_MAX_TOP) {
    set_error(w + ": K must be 1 .. MC_ASSIGN_MAX_TOP");
    return MC_ERR_ARG;
  }
  if (c->cls.align) {
    set_error(w + ": an alignment-mode classifier has no k-mer scorer (use mc_nw_identity + mc_classify_values)");
    return MC_ERR_UNSUPPORTED;
  }
  if (c->width != 1 && c->width != 2) {
    set_error(w + ": 32/64-bit histograms are not supported (use mc_classify_pairs)");
    return MC_ERR_UNSUPPORTED;
  }
  if (!centre_ids || C == 0 || (M > 0 && !query_ids)) {
    set_error(w + ": no centres (or no query ids)");
    return MC_ERR_ARG;
  }
  TRY(check_ids(c, centre_ids, C));
  TRY(check_ids(c, query_ids, M));
  if (stats) stats[0] = stats[1] = stats[2] = 0;
  if (M == 0) return MC_OK;
  const bool both = strands == (MC_STRAND_PLUS | MC_STRAND_MINUS);
  const HistView H = hist_view(c);
  const int nch = (int)((H.B * H.width + 15) / 16);
  const size_t ent_bytes = (size_t)((both ? 2 : 1) * nch + INFO) * 16;
  if (ent_bytes > TILE_BYTES) {
    set_error(w + ": a histogram row does not fit an LDS tile (use mc_classify_pairs)");
    return MC_ERR_UNSUPPORTED;
  }
  uint32_t tile = (uint32_t)std::min<size_t>(TILE_BYTES / ent_bytes, C);
  if (const char *t = getenv("MC_ASSIGN_TILE")) {
    const long v = atol(t);
    if (v >= 1) tile = (uint32_t)std::min<long>(v, (long)tile);
  }
  const char *form = getenv("MC_ASSIGN_FORM");
  const bool general = form && !strcmp(form, "general");
  const bool is_short = !general && c->width == 1 && nch <= 16 && c->cls.layout != 0 && c->fcls.on && c->fcls.mk;
  MCG_CHECK(hipSetDevice(c->device));
  // the gate's bounds per centre: accumulate's get_range arguments (ClusterFactory.cpp:650)
  std::vector<uint64_t> gate(2 * (size_t)C, 0);
  if (sim > 0)
    for (uint32_t j = 0; j < C; j++) {
      const uint64_t len = c->h_seq_off[centre_ids[j] + 1] - c->h_seq_off[centre_ids[j]];
      gate[j] = (uint64_t)(len * sim);
      gate[C + j] = (uint64_t)(len / sim);
    }
  const size_t res_off = ((size_t)M * 4 + 15) / 16 * 16;  // s_f: best, n_similar, then the two counters
  TRY(upload(c, c->s_a, centre_ids, C, c->stream));
  TRY(upload(c, c->s_b, query_ids, (size_t)M, c->stream));
  TRY(upload(c, c->s_c, gate.data(), gate.size(), c->stream));
  if (int rc = ensure(c->s_e, (size_t)M * 8 + 16)) return rc;
  if (int rc = ensure(c->s_f, 2 * res_off + 64)) return rc;
  AssignArgs A;
  A.H = H;
  A.cid = (const uint32_t *)c->s_a.p;
  A.qid = (const uint32_t *)c->s_b.p;
  A.glo = (const uint64_t *)c->s_c.p;
  A.ghi = A.glo + C;
  A.M = M;
  A.C = C;
  A.tile = tile;
  A.gate = sim > 0 ? 1 : 0;
  A.best = (uint32_t *)c->s_f.p;
  A.nsim = (uint32_t *)((char *)c->s_f.p + res_off);
  A.stats = (unsigned long long *)((char *)c->s_f.p + 2 * res_off);
  A.bval = (double *)c->s_e.p;
  A.rc = nullptr;
  A.best_m = A.nsim_m = nullptr;
  A.bval_m = nullptr;
  A.strand = nullptr;
  A.K = K;
  A.hit = nullptr;
  A.hval = nullptr;
  A.hstr = nullptr;
  const bool top = K > 1;
  const size_t hit_off = ((size_t)M * K * 4 + 15) / 16 * 16;
  if (top) {  // s_g: the hits, then their strands; s_h: their values (no per-strand results here)
    if (int rc = ensure(c->s_g, hit_off + (size_t)M * K + 16)) return rc;
    if (int rc = ensure(c->s_h, (size_t)M * K * 8 + 16)) return rc;
    A.hit = (uint32_t *)c->s_g.p;
    A.hstr = (uint8_t *)c->s_g.p + hit_off;
    A.hval = (double *)c->s_h.p;
  }
  if (strands & MC_STRAND_MINUS) {
    if (int rc = ensure(c->s_d, (size_t)C * H.pitch + 16)) return rc;
    A.rc = (const uint8_t *)c->s_d.p;
  }
  if (both && !top) {  // s_g: the minus strand's best, n_similar, then the strands; s_h: its values
    if (int rc = ensure(c->s_g, 2 * res_off + (size_t)M + 16)) return rc;
    if (int rc = ensure(c->s_h, (size_t)M * 8 + 16)) return rc;
    A.best_m = (uint32_t *)c->s_g.p;
    A.nsim_m = (uint32_t *)((char *)c->s_g.p + res_off);
    A.strand = (uint8_t *)c->s_g.p + 2 * res_off;
    A.bval_m = (double *)c->s_h.p;
  }
  MCG_CHECK(hipMemsetAsync(A.stats, 0, 16, c->stream));
  const size_t lds = (size_t)tile * ent_bytes;
  MCG_CHECK(hipEventRecord(c->ev0, c->stream));
  if (strands & MC_STRAND_MINUS)
    if (int rc = launch_revcomp(c, H, A.cid, C, (uint8_t *)c->s_d.p)) return rc;
  if (both) launch_assign<MC_STRAND_PLUS | MC_STRAND_MINUS>(c, A, is_short, M, lds);
  else if (strands == MC_STRAND_MINUS) launch_assign<MC_STRAND_MINUS>(c, A, is_short, M, lds);
  else launch_assign<MC_STRAND_PLUS>(c, A, is_short, M, lds);
  MCG_CHECK(hipGetLastError());
  MCG_CHECK(hipEventRecord(c->ev1, c->stream));
  unsigned long long cnt[2] = {0, 0};
  if (top) {
    if (best) MCG_CHECK(hipMemcpyAsync(best, A.hit, (size_t)M * K * 4, hipMemcpyDeviceToHost, c->stream));
    if (best_val) MCG_CHECK(hipMemcpyAsync(best_val, A.hval, (size_t)M * K * 8, hipMemcpyDeviceToHost, c->stream));
    if (strand) MCG_CHECK(hipMemcpyAsync(strand, A.hstr, (size_t)M * K, hipMemcpyDeviceToHost, c->stream));
  } else {
    if (best) MCG_CHECK(hipMemcpyAsync(best, A.best, (size_t)M * 4, hipMemcpyDeviceToHost, c->stream));
    if (best_val) MCG_CHECK(hipMemcpyAsync(best_val, A.bval, (size_t)M * 8, hipMemcpyDeviceToHost, c->stream));
  }
  if (n_similar) MCG_CHECK(hipMemcpyAsync(n_similar, A.nsim, (size_t)M * 4, hipMemcpyDeviceToHost, c->stream));
  if (strand && !top) {
    if (both) MCG_CHECK(hipMemcpyAsync(strand, A.strand, (size_t)M, hipMemcpyDeviceToHost, c->stream));
    else memset(strand, strands == MC_STRAND_MINUS ? 1 : 0, (size_t)M);
  }
  MCG_CHECK(hipMemcpyAsync(cnt, A.stats, 16, hipMemcpyDeviceToHost, c->stream));
  MCG_CHECK(hipStreamSynchronize(c->stream));
  float ms = 0;
  MCG_CHECK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
  flush_timers(c);
  if (stats) {
    stats[0] = cnt[0];
    stats[1] = cnt[1];
    stats[2] = (uint64_t)((double)ms * 1000.0 + 0.5);
  }
  return MC_OK;
}

}  // namespace

}  // namespace mcg

using namespace mcg;

extern "C" int mc_assign(mc_ctx *c, const uint32_t *centre_ids, uint32_t C, const uint32_t *query_ids, uint64_t M,
                         double sim, uint32_t *best, double *best_val, uint32_t *n_similar, uint64_t *stats) {
  return assign_impl(c, "mc_assign", centre_ids, C, query_ids, M, sim, MC_STRAND_PLUS, 1, best, best_val, nullptr, n_similar, stats);
}

extern "C" int mc_assign_strands(mc_ctx *c, const uint32_t *centre_ids, uint32_t C, const uint32_t *query_ids, uint64_t M,
                                 double sim, int strands, uint32_t *best, double *best_val, uint8_t *strand,
                                 uint32_t *n_similar, uint64_t *stats) {
  return assign_impl(c, "mc_assign_strands", centre_ids, C, query_ids, M, sim, strands, 1, best, best_val, strand,
                     n_similar, stats);
}

// K >= 2: the kernels' list forms.  K = 1 is the one-result path itself (mc_assign_strands' kernels);
// only the strand of an unassigned query on the minus strand alone differs: an empty slot holds 0.
extern "C" int mc_assign_top(mc_ctx *c, const uint32_t *centre_ids, uint32_t C, const uint32_t *query_ids, uint64_t M,
                             double sim, int strands, uint32_t K, uint32_t *hit, double *hit_val, uint8_t *hit_strand,
                             uint32_t *n_similar, uint64_t *stats) {
  std::vector<uint32_t> own;
  if (K == 1 && strands == MC_STRAND_MINUS && hit_strand && !hit) {
    own.resize(M);
    hit = own.data();
  }
  const int rc = assign_impl(c, "mc_assign_top", centre_ids, C, query_ids, M, sim, strands, K, hit, hit_val, hit_strand,
                             n_similar, stats);
  if (rc == MC_OK && K == 1 && strands == MC_STRAND_MINUS && hit_strand)
    for (uint64_t i = 0; i < M; i++)
      if (hit[i] == MC_ASSIGN_NONE) hit_strand[i] = 0;
  return rc;
}

extern "C" int mc_revcomp_rows(mc_ctx *c, const uint32_t *ids, uint64_t m, void *rows) {
  if (!c || c->k == 0) return MC_ERR_STATE;
  if (c->width != 1 && c->width != 2) {
    set_error("mc_revcomp_rows: 32/64-bit histograms are not supported");
    return MC_ERR_UNSUPPORTED;
  }
  const HistView H = hist_view(c);
  if (H.pitch + INFO * 16 > TILE_BYTES) {
    set_error("mc_revcomp_rows: a histogram row does not fit an LDS tile");
    return MC_ERR_UNSUPPORTED;
  }
  if (m > 0 && (!ids || !rows)) {
    set_error("mc_revcomp_rows: no ids (or no output)");
    return MC_ERR_ARG;
  }
  TRY(check_ids(c, ids, m));
  if (m == 0) return MC_OK;
  MCG_CHECK(hipSetDevice(c->device));
  TRY(upload(c, c->s_a, ids, (size_t)m, c->stream));
  TRY(ensure(c->s_d, (size_t)m * H.pitch + 16));
  if (int rc = launch_revcomp(c, H, (const uint32_t *)c->s_a.p, m, (uint8_t *)c->s_d.p)) return rc;
  const size_t rowb = (size_t)H.B * H.width;
  MCG_CHECK(hipMemcpy2DAsync(rows, rowb, c->s_d.p, H.pitch, rowb, m, hipMemcpyDeviceToHost, c->stream));
  MCG_CHECK(hipStreamSynchronize(c->stream));
  flush_timers(c);
  return MC_OK;
}
