// revseq.hip -- the minus-strand strings of points, on the device (host/revseq.hpp has the rule).
//
// mc_nw_identity_strands aligns a read assigned on the minus strand reverse-complemented, as
// seq1; this kernel writes those strings, once per read and batch, into a buffer launch_nw reads
// as its A operand.  Output records start 16-byte aligned (the offsets are padded up to 16, the
// pad bytes written as zeros), so the output is a sequence of 16-byte chunks and a thread owns
// one: one whole store per thread, in thread order.  The gather is on the load side: chunk o of a
// record of L bytes is the source span [L - 16 - o, L - o) read backwards, which starts at any
// byte address.  It is fetched as the enclosing 4-byte-aligned 20 bytes -- one 16-byte load (a
// global 16-byte load needs 4-byte alignment only) and one dword -- and shifted into place with
// four v_alignbyte; a word of digits is complemented by one xor (rc_word), reversed by one
// v_perm (bswap).  The last chunk of a record (fewer than 16 bytes left) takes byte loads.
// Per record: L bytes read (+ at most 4 per chunk of overlap, which hits the same cache lines),
// pad16(L) written.
#include <algorithm>

#include "../host/revseq.hpp"
#include "mcgpu.hpp"

namespace mcg {

namespace {

constexpr int NT = 256;

struct __attribute__((packed, aligned(4))) Quad {
  uint32_t w[4];
};

// the largest r in [lo, hi] with off[r] <= x (off[lo] <= x)
__device__ __forceinline__ uint32_t find_rec(const uint64_t *__restrict__ off, uint32_t lo, uint32_t hi, uint64_t x) {
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo + 1) / 2;
    if (off[mid] <= x) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// out[out_off[r] .. out_off[r + 1]) = the minus-strand string of point ids[r], zero padded;
// out_off[r + 1] - out_off[r] = the point's length rounded up to 16, u >= 1
__global__ __launch_bounds__(NT) void revseq_kernel(const uint8_t *__restrict__ codes, const uint64_t *__restrict__ seq_off,
                                                    const uint32_t *__restrict__ ids, uint32_t u,
                                                    const uint64_t *__restrict__ out_off, uint8_t *__restrict__ out) {
  const uint64_t nchunk = out_off[u] >> 4;
  for (uint64_t c0 = (uint64_t)blockIdx.x * NT; c0 < nchunk; c0 += (uint64_t)gridDim.x * NT) {
    // the records this workgroup's 256 chunks belong to (uniform), then each thread's own
    const uint64_t cend = c0 + NT < nchunk ? c0 + NT : nchunk;
    const uint32_t rlo = find_rec(out_off, 0, u - 1, c0 << 4);
    const uint32_t rhi = find_rec(out_off, rlo, u - 1, (cend << 4) - 1);
    const uint64_t ch = c0 + threadIdx.x;
    if (ch >= nchunk) continue;
    const uint32_t r = find_rec(out_off, rlo, rhi, ch << 4);
    const uint32_t id = ids[r];
    const uint64_t src = seq_off[id], L = seq_off[id + 1] - src;
    const uint64_t o = (ch << 4) - out_off[r];  // this chunk's first position in the output record
    uint32_t w[4];
    if (o + 16 <= L) {
      const uint64_t s = src + L - 16 - o;  // the source span [s, s + 16)
      const uint32_t bs = (uint32_t)s & 3u;
      const uint8_t *p = codes + (s - bs);  // 4-byte aligned; p + 20 <= s + 20 <= the sequences' end + 4
      const Quad v = *reinterpret_cast<const Quad *>(p);
      const uint32_t v4 = *reinterpret_cast<const uint32_t *>(p + 16);
      const uint32_t t[4] = {__builtin_amdgcn_alignbyte(v.w[1], v.w[0], bs), __builtin_amdgcn_alignbyte(v.w[2], v.w[1], bs),
                             __builtin_amdgcn_alignbyte(v.w[3], v.w[2], bs), __builtin_amdgcn_alignbyte(v4, v.w[3], bs)};
#pragma unroll
      for (int i = 0; i < 4; i++) w[i] = __builtin_bswap32(mc::rc_word(t[3 - i]));
    } else {  // the record's last chunk: the bytes past L are the pad
#pragma unroll
      for (int i = 0; i < 4; i++) {
        w[i] = 0;
#pragma unroll
        for (int b = 0; b < 4; b++) {
          const uint64_t pos = o + 4 * i + b;
          if (pos < L) w[i] |= (uint32_t)mc::rc_byte(codes[src + L - 1 - pos]) << (8 * b);
        }
      }
    }
    *reinterpret_cast<uint4 *>(out + (ch << 4)) = make_uint4(w[0], w[1], w[2], w[3]);
  }
}

}  // namespace

int launch_revseq(mc_ctx *c, const uint32_t *d_ids, uint32_t u, const uint64_t *d_out_off, uint64_t out_bytes, uint8_t *d_out) {
  if (u == 0 || out_bytes == 0) return MC_OK;
  const uint64_t blocks = (out_bytes / 16 + NT - 1) / NT;
  const unsigned grid = (unsigned)std::min<uint64_t>(blocks, 1u << 16);
  timed_begin(c);
  revseq_kernel<<<grid, NT, 0, c->stream>>>((const uint8_t *)c->codes.p, (const uint64_t *)c->seq_off.p, d_ids, u, d_out_off,
                                            d_out);
  timed_end(c, F_LAYOUT);
  MCG_CHECK(hipGetLastError());
  return MC_OK;
}

}  // namespace mcg
