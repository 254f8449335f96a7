// abi_util.hpp -- what the files of entry points (abi.hip, abi_align.hip, assign.hip) share: the id
// check, uploads through the context's pinned staging ring, downloads through its pinned landing
// buffer, caps a test may lower through the environment.  What is no template is defined in abi.hip.
#pragma once
#include <initializer_list>

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

}  // namespace mcg
