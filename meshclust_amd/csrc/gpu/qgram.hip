// qgram.hip -- mc_qgram_common: the multiset q-gram intersection C_q of pairs of reads, the count
// host/qscreen.hpp's bound turns into "identity below the cutoff" without an alignment.
//
// One workgroup per pair and a 4^q-entry table of 32-bit counters in LDS (64 KB at q = 7).  The
// q-grams come from the 2-bit words (16 bases per word, records word-aligned): the one at base j is
// 2q bits of the two words around it, the first base lowest.  A minus-strand pair counts a's
// q-grams reverse-complemented (all digits complemented, their order reversed: a bit reversal and a
// swap within each digit), which is the multiset of the minus-strand string's q-grams.  a's are
// counted with LDS atomic adds; for each of b's a returning decrement counts a hit where the old
// value was positive and is undone otherwise, so every one of a's occurrences pairs with at most
// one of b's: sum over g of min(occ_a, occ_b).  A read with a byte outside 0..3 (its impure flag)
// or shorter than q gives "not available".
#include <algorithm>

#include "abi_util.hpp"
#include "mcgpu.hpp"

namespace mcg {

namespace {

constexpr int NT = 256;
constexpr int QMAX = 7;
constexpr uint32_t NA = 0xffffffffu;

// the q-gram at base j of the record whose words start at w, the first base lowest (j + q <= len)
__device__ __forceinline__ uint32_t gram_at(const uint32_t *__restrict__ w, uint32_t j, int q, uint32_t mask) {
  const uint32_t wi = j >> 4, sh = 2 * (j & 15);
  uint64_t v = w[wi];
  if (sh + 2 * (uint32_t)q > 32) v |= (uint64_t)w[wi + 1] << 32;  // (the window's last base lies in that word)
  return (uint32_t)(v >> sh) & mask;
}

__device__ __forceinline__ uint32_t revcomp_gram(uint32_t g, int q, uint32_t mask) {
  const uint32_t y = __brev(~g & mask);
  return (((y & 0x55555555u) << 1) | ((y >> 1) & 0x55555555u)) >> (32 - 2 * q);
}

__global__ __launch_bounds__(NT) void qgram_kernel(const uint32_t *__restrict__ packed, const uint64_t *__restrict__ pk_off,
                                                   const uint64_t *__restrict__ seq_off, const uint8_t *__restrict__ impure,
                                                   const uint32_t *__restrict__ a, const uint32_t *__restrict__ b,
                                                   const uint8_t *__restrict__ a_minus, uint32_t m, int q,
                                                   uint32_t *__restrict__ common) {
  __shared__ uint32_t tab[1 << (2 * QMAX)];
  const uint32_t mask = (1u << (2 * q)) - 1, nbin = 1u << (2 * q);
  for (uint32_t p = blockIdx.x; p < m; p += gridDim.x) {
    const uint32_t ia = a[p], ib = b[p];
    const uint64_t la = seq_off[ia + 1] - seq_off[ia], lb = seq_off[ib + 1] - seq_off[ib];
    if (la < (uint64_t)q || lb < (uint64_t)q || impure[ia] || impure[ib]) {  // (uniform)
      if (threadIdx.x == 0) common[p] = NA;
      continue;
    }
    const bool minus = a_minus && a_minus[p];
    for (uint32_t t = threadIdx.x; t < nbin; t += NT) tab[t] = 0;
    __syncthreads();
    const uint32_t *wa = packed + pk_off[ia], *wb = packed + pk_off[ib];
    const uint32_t na = (uint32_t)la - (uint32_t)q + 1, nb = (uint32_t)lb - (uint32_t)q + 1;
    for (uint32_t j = threadIdx.x; j < na; j += NT) {
      const uint32_t g = gram_at(wa, j, q, mask);
      atomicAdd(&tab[minus ? revcomp_gram(g, q, mask) : g], 1u);
    }
    __syncthreads();
    uint32_t hits = 0;
    for (uint32_t j = threadIdx.x; j < nb; j += NT) {
      uint32_t *e = &tab[gram_at(wb, j, q, mask)];
      // (signed: concurrent decrements of one entry may take it below zero until they are undone)
      if ((int32_t)atomicSub(e, 1u) > 0) hits++;
      else atomicAdd(e, 1u);
    }
    for (int o = 32; o > 0; o >>= 1) hits += __shfl_down(hits, o, 64);
    __syncthreads();  // every wave is done with the table: its first words take the waves' sums
    if ((threadIdx.x & 63) == 0) tab[threadIdx.x >> 6] = hits;
    __syncthreads();
    if (threadIdx.x == 0) common[p] = tab[0] + tab[1] + tab[2] + tab[3];
    __syncthreads();
  }
}

}  // namespace

static int launch_qgram(mc_ctx *c, const uint32_t *d_a, const uint32_t *d_b, const uint8_t *d_minus, uint32_t m, int q,
                        uint32_t *d_common) {
  const unsigned grid = std::min<uint32_t>(m, 1u << 16);
  timed_begin(c);
  qgram_kernel<<<grid, NT, 0, c->stream>>>((const uint32_t *)c->packed.p, (const uint64_t *)c->pk_off.p,
                                           (const uint64_t *)c->seq_off.p, (const uint8_t *)c->impure.p, d_a, d_b, d_minus, m, q,
                                           d_common);
  timed_end(c, F_PAIRS);
  MCG_CHECK(hipGetLastError());
  return MC_OK;
}

}  // namespace mcg

using namespace mcg;

extern "C" int mc_qgram_common(mc_ctx *c, const uint32_t *a, const uint32_t *b, const uint8_t *a_minus, uint64_t m, int q,
                               uint32_t *common) {
  if (!c || !c->codes.p) return MC_ERR_STATE;
  if (m == 0) return MC_OK;
  if (!a || !b || !common) return MC_ERR_ARG;
  if (q < 1 || q > QMAX) {
    set_error("mc_qgram_common: q must be in 1..7");
    return MC_ERR_ARG;
  }
  MCG_CHECK(hipSetDevice(c->device));
  TRY(check_ids(c, a, m));
  TRY(check_ids(c, b, m));
  for (uint64_t i = 0; i < m; i++)
    for (uint32_t id : {a[i], b[i]})
      if (c->h_seq_off[id + 1] - c->h_seq_off[id] >= (1ull << 31)) {
        set_error("mc_qgram_common: a read of 2^31 bases or more");
        return MC_ERR_UNSUPPORTED;
      }
  constexpr uint64_t CHUNK = 1u << 20;  // pairs per launch (the lists go through the staging ring)
  for (uint64_t i0 = 0; i0 < m; i0 += CHUNK) {
    const uint64_t mb = std::min(CHUNK, m - i0);
    TRY(upload(c, c->s_d, a + i0, mb, c->stream));
    TRY(upload(c, c->s_e, b + i0, mb, c->stream));
    if (a_minus) TRY(upload(c, c->s_g, a_minus + i0, mb, c->stream));
    TRY(ensure(c->s_f, mb * 4 + 64));
    TRY(launch_qgram(c, (const uint32_t *)c->s_d.p, (const uint32_t *)c->s_e.p, a_minus ? (const uint8_t *)c->s_g.p : nullptr,
                     (uint32_t)mb, q, (uint32_t *)c->s_f.p));
    TRY(download_parts(c, {{common + i0, c->s_f.p, mb * 4}}, c->stream));
  }
  flush_timers(c);
  return MC_OK;
}
