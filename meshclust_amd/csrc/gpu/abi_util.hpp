// abi_util.hpp -- what the files of entry points (abi.hip, abi_align.hip, abi_msa.hip, assign.hip)
// share: the id check, uploads through the context's pinned staging ring, downloads through its
// pinned landing buffer, caps a test may lower through the environment (what is no template is
// defined in abi.hip), and what abi_align.hip defines for abi_msa.hip as well.
#pragma once
#include <functional>
#include <initializer_list>

#include "../host/pairbatch.hpp"
#include "mcgpu.hpp"

#define TRY(x)                  \
  do {                          \
    int _rc = (x);              \
    if (_rc != MC_OK) return _rc; \
  } while (0)

namespace mcg {

// MC_ERR_ARG ("point id out of range") unless every id is a loaded point
int check_ids(mc_ctx *c, const uint32_t *ids, uint64_t m);

// A cap that the environment may only lower (read per call: the tests put batch ends inside small
// lists): the variable's value when it is > 0 and < dflt, else dflt.
uint64_t env_cap(const char *name, uint64_t dflt);

// `bytes` from the host to device memory on stream s.  Small inputs (the per-call id lists,
// offsets, member lists, the launch helpers' bucket lists) go through a pinned staging ring owned
// by the context: a copy from pinned memory is a plain DMA, a pageable one is staged by the
// runtime.  A region is reused only after a stream synchronize that follows its copy (the ring
// wraps behind one).  MC_PAGEABLE_UPLOADS (read once per process) turns the ring off.  sync_pageable: the
// stream is synchronized after a pageable copy, for a source that may go out of scope.
int stage_copy(mc_ctx *c, void *dst, const void *src, size_t bytes, hipStream_t s, bool sync_pageable);

// count elements into the grow-only buffer b; the caller keeps h alive until the stream is synchronized
template <typename T>
int upload(mc_ctx *c, Buf &b, const T *h, size_t count, hipStream_t s) {
  if (int rc = ensure(b, count * sizeof(T) + 16)) return rc;
  return stage_copy(c, b.p, h, count * sizeof(T), s, false);
}

template <typename T>
int download(T *h, const void *d, size_t count, hipStream_t s) {
  if (count) MCG_CHECK(hipMemcpyAsync(h, d, count * sizeof(T), hipMemcpyDeviceToHost, s));
  return MC_OK;
}

struct DPart {  // one result of a call: `bytes` from device `d` to host `h` (h null: not wanted)
  void *h;
  const void *d;
  size_t bytes;
};
// A call's results through the pinned landing buffer: one DMA per part into it, one stream
// synchronize, then the host copies (every part a pageable download was a runtime-staged copy).
// Ends with the stream synchronized, as the direct downloads it replaces did.
int download_parts(mc_ctx *c, std::initializer_list<DPart> parts, hipStream_t s);

// One device region of a call's results copied to the context's pinned landing buffer (a plain
// DMA; a pageable destination is staged by the runtime, one staged copy per download) and the
// stream synchronized: the caller then copies the parts out of *h.  *h is null only when the
// landing buffer cannot be allocated (the caller then downloads the parts directly); a failing
// copy or synchronize is reported as the error it is, with its call site.
int download_pinned(mc_ctx *c, const void *d, size_t bytes, hipStream_t s, uint8_t **h);

// `bytes` from device `d` to host `dst` on the context's stream, which ends synchronized: through the
// pinned landing buffer while bytes <= pinned_max and the buffer can be had, else straight to dst.
int download_to(mc_ctx *c, void *dst, const void *d, size_t bytes, size_t pinned_max = ~(size_t)0);

inline uint64_t seq_len(const mc_ctx *c, uint32_t id) { return c->h_seq_off[id + 1] - c->h_seq_off[id]; }

// ---- abi_align.hip, shared with abi_msa.hip ----------------------------------------------------
// One batch of strand_batches, reads [i0, i1) of the call's list: read i is la(i) bytes at a_off(i) of the batch's
// minus-strand strings in c->rc_seq (a_rc(i) = 1; rc_bytes of them, padded) or of the loaded codes (a_rc(i) = 0).
struct StrandBatch {
  uint64_t i0, i1, rc_bytes;
  const mc_ctx *c;
  const uint32_t *ids;
  const mc::PairBatcher &pb;
  const uint64_t *h_off;
  uint64_t la(uint64_t i) const { return seq_len(c, ids[i]); }
  uint32_t a_rc(uint64_t i) const { return pb.minus(i) ? 1 : 0; }
  uint64_t a_off(uint64_t i) const { return pb.minus(i) ? h_off[pb.slot(ids[i])] : c->h_seq_off[ids[i]]; }
};
// The m reads ids (minus: a flag per read, or NULL) in host/pairbatch.hpp's batches under caps
// (scratch_at(i): read i's scratch, unused with caps.scratch 0): per batch its distinct minus reads
// reverse-complemented once into c->rc_seq, then per_batch.  wanted, where given, is asked first
// with (i0, i1): false skips the batch before its reverse complement.
int strand_batches(mc_ctx *c, const uint32_t *ids, const uint8_t *minus, uint64_t m, mc::PairBatchCaps caps, std::function<uint64_t(uint64_t)> scratch_at,
                   const std::function<int(const StrandBatch &)> &per_batch, const std::function<bool(uint64_t, uint64_t)> &wanted = nullptr);
// score, columns and identities of a batch's TRACE_RES ints per pair to the outputs that are wanted
void scatter_res(const std::vector<int32_t> &res, uint64_t i0, uint64_t mb, int32_t *score, int32_t *len, int32_t *ids);
// What mc_nw_pileup_strands and mc_nw_msa_begin do with their lists before any launch of their own:
// the ids checked, tindex[point id] = its place among the targets (MC_ERR_ARG for a target listed
// twice or a b[i] that is no target), weighted: no target's weights may pass 32 bits, the plan
// (align_plan), its caps (align_check_caps), row_off[t + 1] = row_off[t] + target t's length + 1.
int align_targets(mc_ctx *c, const std::string &who, bool weighted, const uint32_t *a, const uint32_t *b, const uint8_t *a_minus, uint64_t m,
                  const uint32_t *targets, uint32_t nt, uint64_t *row_off, std::vector<uint32_t> &tindex, std::vector<int32_t> &plan);
// The pairs of a call in trace batches under align_plan's plan: see abi_align.hip.
int align_batches(mc_ctx *c, const char *who, const uint32_t *a, const uint32_t *b, const uint8_t *a_minus, uint64_t m,
                  const std::vector<int32_t> &plan, const std::function<int(uint64_t, uint64_t, const std::vector<int32_t> &)> &per_batch);
// a mc_nw_*_profile entry: out[k] = device ms of fams[k] since the last reset; reset clears those families
int profile_families(mc_ctx *c, double *out, int reset, std::initializer_list<int> fams);

}  // namespace mcg
