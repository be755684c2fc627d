// Owners of transient device memory: what a call or a stage of the index open allocates is released when its scope ends, on every path.
#pragma once
#include <utility>
#include <vector>

#include "common.hpp"

namespace dg {

// the transient device buffers of one call: released on its stream, in the order they were made, when the call returns
struct StreamScratch {
  hipStream_t st;
  std::vector<std::pair<void*, bool>> made;  // (block, from big_alloc)
  explicit StreamScratch(hipStream_t s) : st(s) {}
  ~StreamScratch() {
    (void)hipStreamSynchronize(st);
    for (const auto& b : made) {
      if (b.second) big_free(b.first, st);
      else (void)hipFree(b.first);
    }
    (void)hipStreamSynchronize(st);
  }
  int big(void** p, size_t bytes) {
    DG_HIP(big_alloc(p, bytes, st));
    made.emplace_back(*p, true);
    return DG_OK;
  }
  int small(void** p, size_t bytes) {
    DG_HIP(hipMalloc(p, bytes));
    made.emplace_back(*p, false);
    return DG_OK;
  }
  void keep() { made.clear(); }  // the blocks have a new owner (dg_index::adopt)
};

// A 4-byte device word that a launch reports through: initialised on the stream, handed to the launch (p), read back behind a stream
// synchronise, released on every path.
struct DevWord {
  hipStream_t st;
  u32* p = nullptr;
  u32 first = 0;  // the copy's source: stays until the word goes
  explicit DevWord(hipStream_t s) : st(s) {}
  ~DevWord() {
    if (p) (void)hipFree(p);
  }
  int init(u32 v) {
    first = v;
    DG_HIP(hipMalloc((void**)&p, 4));
    DG_HIP(hipMemcpyAsync(p, &first, 4, hipMemcpyHostToDevice, st));
    return DG_OK;
  }
  int read(u32* v) {  // synchronises the stream
    DG_HIP(hipMemcpyAsync(v, p, 4, hipMemcpyDeviceToHost, st));
    DG_HIP(hipStreamSynchronize(st));
    return DG_OK;
  }
};

}  // namespace dg
