// derep.hip -- mc_derep: exact dereplication of points on the device (include/meshclust_amd.h,
// DESIGN.md 3.17; host/derep.hpp has the definition, the planner and the host restatement).
//
// Two kernels, a wavefront per unit of work, no LDS, no global atomics, every loop bounded by a
// record's length:
//   derep_fp_kernel   per listed point one pass over its bytes: a 128-bit fingerprint of the string
//                     as written and, with both strands, one of its minus-strand string from the same
//                     loads; the smaller of the two is the point's key, so a string and its minus
//                     strand share it.  The fingerprint is a position-keyed sum mod 2^64,
//                       F(s) = sum over j of K(j) * (s[j] + 1),   K(j) two mixed 64-bit words,
//                     an associative combine: how a record is split over lanes cannot change it.  The
//                     minus strand has rc_byte(s[L - 1 - j]) at j, so byte j of the record adds
//                     K(L - 1 - j) * (rc_byte(s[j]) + 1) to the second sum.  The length is mixed in
//                     last.  16 bytes per point come back.
//   derep_cmp_kernel  per (member, leader) pair of the planner one byte: bit 0 the strings are equal as
//                     written, bit 1 (both strands) the member equals the leader's minus-strand string,
//                     read backwards the way revseq.hip reads it.  The wave takes 1024 bytes per step
//                     and leaves at the first step after which neither can still hold.
// A lane's 16 bytes start at any byte address: they are fetched as the enclosing 4-byte-aligned 20
// bytes and shifted into place with four v_alignbyte (revseq.hip).  Such a load ends at most 4 bytes
// past the record; the codes allocation has 16 bytes of slack (abi.hip load_common).  A record's last,
// partial chunk takes byte loads.
#include <algorithm>
#include <cstdlib>
#include <string>

#include "../host/derep.hpp"
#include "../host/revseq.hpp"
#include "abi_util.hpp"
#include "mcgpu.hpp"

namespace mcg {

namespace {

constexpr int NT = 256;
constexpr int WPB = NT / 64;  // wavefronts (units of work) per workgroup

struct __attribute__((packed, aligned(4))) Quad {
  uint32_t w[4];
};

// codes[s .. s + 16) as four little-endian words; reads [s - (s & 3), s - (s & 3) + 20)
__device__ __forceinline__ void load16(const uint8_t *__restrict__ codes, uint64_t s, uint32_t w[4]) {
  const uint32_t bs = (uint32_t)s & 3u;
  const uint8_t *p = codes + (s - bs);
  const Quad v = *reinterpret_cast<const Quad *>(p);
  const uint32_t v4 = *reinterpret_cast<const uint32_t *>(p + 16);
  w[0] = __builtin_amdgcn_alignbyte(v.w[1], v.w[0], bs);
  w[1] = __builtin_amdgcn_alignbyte(v.w[2], v.w[1], bs);
  w[2] = __builtin_amdgcn_alignbyte(v.w[3], v.w[2], bs);
  w[3] = __builtin_amdgcn_alignbyte(v4, v.w[3], bs);
}

// the two key words of position j
__device__ __forceinline__ void pos_key(uint64_t j, uint64_t &k0, uint64_t &k1) {
  uint64_t x = (j + 1) * 0x9e3779b97f4a7c15ull;
  x ^= x >> 32;
  x *= 0xd6e8feb86659fd93ull;
  x ^= x >> 29;
  k0 = x;
  uint64_t y = ((x << 23) | (x >> 41)) * 0xff51afd7ed558ccdull;
  k1 = y ^ (y >> 31);
}

__device__ __forceinline__ uint64_t finish(uint64_t f, uint64_t L, uint64_t c) {
  uint64_t x = f + (L + 1) * c;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 29;
  return x;
}

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, d, 64);
  return v;
}

// keys[2 * i], keys[2 * i + 1] = the key of point ids[i] (hi, lo), i < m
template <bool BOTH>
__global__ __launch_bounds__(NT) void derep_fp_kernel(const uint8_t *__restrict__ codes, const uint64_t *__restrict__ seq_off,
                                                      const uint32_t *__restrict__ ids, uint64_t m, uint64_t *__restrict__ keys) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t nwave = (uint64_t)gridDim.x * WPB;
  for (uint64_t i = (uint64_t)blockIdx.x * WPB + wave_id(); i < m; i += nwave) {
    const uint32_t id = ids[i];
    const uint64_t src = seq_off[id], L = seq_off[id + 1] - src;
    uint64_t p0 = 0, p1 = 0, q0 = 0, q1 = 0;
    for (uint64_t o = (uint64_t)lane * 16; o < L; o += 64 * 16) {
      uint32_t w[4];
      uint32_t nb = 16;
      if (o + 16 <= L) {
        load16(codes, src + o, w);
      } else {  // the record's last chunk
        nb = (uint32_t)(L - o);
#pragma unroll
        for (int t = 0; t < 4; t++) w[t] = 0;
#pragma unroll
        for (int t = 0; t < 16; t++)
          if ((uint32_t)t < nb) w[t >> 2] |= (uint32_t)codes[src + o + t] << (8 * (t & 3));
      }
#pragma unroll
      for (int t = 0; t < 16; t++) {
        if ((uint32_t)t < nb) {
          const uint64_t j = o + t;
          uint64_t k0, k1;
          pos_key(j, k0, k1);
          const uint64_t b = ((w[t >> 2] >> (8 * (t & 3))) & 255u) + 1;
          p0 += k0 * b;
          p1 += k1 * b;
          if (BOTH) {
            pos_key(L - 1 - j, k0, k1);
            const uint64_t r = (uint64_t)mc::rc_byte((uint8_t)(b - 1)) + 1;
            q0 += k0 * r;
            q1 += k1 * r;
          }
        }
      }
    }
    p0 = wave_sum(p0);
    p1 = wave_sum(p1);
    uint64_t hi = finish(p0, L, 0xa0761d6478bd642full), lo = finish(p1, L, 0xe7037ed1a0b428dbull);
    if (BOTH) {
      q0 = wave_sum(q0);
      q1 = wave_sum(q1);
      const uint64_t mhi = finish(q0, L, 0xa0761d6478bd642full), mlo = finish(q1, L, 0xe7037ed1a0b428dbull);
      if (mhi < hi || (mhi == hi && mlo < lo)) {
        hi = mhi;
        lo = mlo;
      }
    }
    if (lane == 0) {
      keys[2 * i] = hi;
      keys[2 * i + 1] = lo;
    }
  }
}

// res[p] for the pair of points (pairs[p].x, pairs[p].y) = (member, leader): bit 0 equal as written,
// bit 1 (BOTH) the member equals the leader's minus-strand string; 0 where the lengths differ
template <bool BOTH>
__global__ __launch_bounds__(NT) void derep_cmp_kernel(const uint8_t *__restrict__ codes, const uint64_t *__restrict__ seq_off,
                                                       const uint2 *__restrict__ pairs, uint32_t npairs, uint8_t *__restrict__ res) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t p = blockIdx.x * WPB + wave_id();
  if (p >= npairs) return;
  const uint2 pr = pairs[p];
  const uint64_t a = seq_off[pr.x], L = seq_off[pr.x + 1] - a;
  const uint64_t b = seq_off[pr.y], Lb = seq_off[pr.y + 1] - b;
  bool plus = L == Lb, minus = BOTH && L == Lb;
  for (uint64_t base = 0; base < L && (plus || minus); base += 64 * 16) {
    const uint64_t o = base + (uint64_t)lane * 16;
    bool ep = true, em = true;
    if (o + 16 <= L) {
      uint32_t wa[4], wb[4];
      load16(codes, a + o, wa);
      if (plus) {
        load16(codes, b + o, wb);
        ep = wa[0] == wb[0] && wa[1] == wb[1] && wa[2] == wb[2] && wa[3] == wb[3];
      }
      if (BOTH && minus) {  // chunk o of the leader's minus strand is its span [L - 16 - o, L - o) read backwards
        load16(codes, b + L - 16 - o, wb);
#pragma unroll
        for (int t = 0; t < 4; t++) em = em && wa[t] == __builtin_bswap32(mc::rc_word(wb[3 - t]));
      }
    } else if (o < L) {  // the last chunk
      for (uint64_t pos = o; pos < L; pos++) {
        const uint8_t ca = codes[a + pos];
        ep = ep && ca == codes[b + pos];
        if (BOTH) em = em && ca == mc::rc_byte(codes[b + L - 1 - pos]);
      }
    }
    plus = plus && __all(ep);
    if (BOTH) minus = minus && __all(em);
  }
  if (lane == 0) res[p] = (uint8_t)((plus ? 1 : 0) | (minus ? 2 : 0));
}

int launch_derep_fp(mc_ctx *c, const uint32_t *d_ids, uint64_t m, bool both, uint64_t *d_keys) {
  const unsigned grid = (unsigned)std::min<uint64_t>((m + WPB - 1) / WPB, 1u << 20);
  timed_begin(c);
  if (both)
    derep_fp_kernel<true><<<grid, NT, 0, c->stream>>>((const uint8_t *)c->codes.p, (const uint64_t *)c->seq_off.p, d_ids, m, d_keys);
  else
    derep_fp_kernel<false><<<grid, NT, 0, c->stream>>>((const uint8_t *)c->codes.p, (const uint64_t *)c->seq_off.p, d_ids, m, d_keys);
  timed_end(c, F_DEREP_FP);
  MCG_CHECK(hipGetLastError());
  return MC_OK;
}

int launch_derep_cmp(mc_ctx *c, const uint2 *d_pairs, uint32_t npairs, bool both, uint8_t *d_res) {
  const unsigned grid = (npairs + WPB - 1) / WPB;
  timed_begin(c);
  if (both)
    derep_cmp_kernel<true><<<grid, NT, 0, c->stream>>>((const uint8_t *)c->codes.p, (const uint64_t *)c->seq_off.p, d_pairs, npairs, d_res);
  else
    derep_cmp_kernel<false><<<grid, NT, 0, c->stream>>>((const uint8_t *)c->codes.p, (const uint64_t *)c->seq_off.p, d_pairs, npairs, d_res);
  timed_end(c, F_DEREP_CMP);
  MCG_CHECK(hipGetLastError());
  return MC_OK;
}

// `bytes` of device memory to the host, through the pinned landing buffer where it is small enough
int fetch(mc_ctx *c, void *h, const void *d, size_t bytes) { return download_to(c, h, d, bytes, 64ull << 20); }

}  // namespace

}  // namespace mcg

using namespace mcg;

extern "C" {

int mc_derep(mc_ctx *c, const uint32_t *ids, uint64_t m, int strands, uint32_t *rep, uint8_t *minus) {
  if (!c || !c->codes.p) return MC_ERR_STATE;
  if (strands != MC_STRAND_PLUS && strands != (MC_STRAND_PLUS | MC_STRAND_MINUS)) {
    set_error("mc_derep: strands is MC_STRAND_PLUS or MC_STRAND_PLUS | MC_STRAND_MINUS");
    return MC_ERR_ARG;
  }
  const bool both = strands != MC_STRAND_PLUS;
  if (m == 0) return MC_OK;
  if (!ids || !rep || (both && !minus)) {
    set_error("mc_derep: ids and rep are required, and minus with both strands");
    return MC_ERR_ARG;
  }
  if (m >= (1ull << 32)) {
    set_error("mc_derep: positions are 32-bit, m is below 2^32");
    return MC_ERR_ARG;
  }
  TRY(check_ids(c, ids, m));
  MCG_CHECK(hipSetDevice(c->device));
  int bits = 128;
  if (const char *e = getenv("MC_DEREP_HASH_BITS")) bits = std::min(128, std::max(0, atoi(e)));
  const uint64_t per = env_cap("MC_DEREP_BATCH", MC_DEREP_BATCH_PAIRS);

  TRY(upload(c, c->dr_ids, ids, m, c->stream));
  TRY(ensure(c->dr_keys, m * 16 + 16));
  TRY(launch_derep_fp(c, (const uint32_t *)c->dr_ids.p, m, both, (uint64_t *)c->dr_keys.p));
  std::vector<mc::DerepKey> keys(m);
  TRY(fetch(c, keys.data(), c->dr_keys.p, m * 16));  // (synchronizes: ids may leave scope after the call)
  std::vector<uint64_t> lens(m);
  for (uint64_t i = 0; i < m; i++) {
    lens[i] = c->h_seq_off[ids[i] + 1] - c->h_seq_off[ids[i]];
    keys[i] = mc::derep_key_bits(keys[i], bits);
  }
  mc::DerepPlanner plan;
  plan.begin(keys.data(), lens.data(), m);
  std::vector<uint2> recs;
  std::vector<uint8_t> res;
  while (plan.open()) {
    const uint64_t np = plan.mem.size();
    res.resize(np);
    for (uint64_t p0 = 0; p0 < np; p0 += per) {
      const uint64_t nb = std::min(per, np - p0);
      recs.resize(nb);
      for (uint64_t p = 0; p < nb; p++) recs[p] = make_uint2(ids[plan.mem[p0 + p]], ids[plan.lead[p0 + p]]);
      TRY(upload(c, c->dr_pairs, recs.data(), nb, c->stream));
      TRY(ensure(c->dr_res, nb + 16));
      TRY(launch_derep_cmp(c, (const uint2 *)c->dr_pairs.p, (uint32_t)nb, both, (uint8_t *)c->dr_res.p));
      TRY(fetch(c, res.data() + p0, c->dr_res.p, nb));  // (synchronizes: the records are the next batch's)
    }
    plan.settle(res.data());
  }
  flush_timers(c);
  c->dr_stat[0] += (double)plan.pairs;
  c->dr_stat[1] += (double)plan.rounds;
  c->dr_stat[2] += (double)plan.collisions;
  memcpy(rep, plan.rep.data(), m * sizeof(uint32_t));
  if (minus) memcpy(minus, plan.minus.data(), m);
  return MC_OK;
}

int mc_derep_profile(mc_ctx *c, double *out, int reset) {
  if (!c || !out) return MC_ERR_ARG;
  (void)hipStreamSynchronize(c->stream);
  flush_timers(c);
  out[0] = c->fam_ms[F_DEREP_FP];
  out[1] = c->fam_ms[F_DEREP_CMP];
  for (int k = 0; k < 3; k++) out[2 + k] = c->dr_stat[k];
  if (reset) {
    c->fam_ms[F_DEREP_FP] = c->fam_n[F_DEREP_FP] = c->fam_ms[F_DEREP_CMP] = c->fam_n[F_DEREP_CMP] = 0;
    for (int k = 0; k < 3; k++) c->dr_stat[k] = 0;
  }
  return MC_OK;
}

}  // extern "C"
