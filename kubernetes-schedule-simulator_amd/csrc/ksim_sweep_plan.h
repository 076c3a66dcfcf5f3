// ksim_sweep_plan.h — the scenario sweep's scratch planning (ksim_sweep_rt.cpp): the carver that
// measures and hands out a form's scratch arrays from one description of the layout, and the rule
// that sizes a chunk of scenarios.  Plain C++ with no device include, so it is tested on the host
// alone (tests/test_sweep_plan_host.py).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

// A form writes its layout once, as a function of the chunk size that take()s its arrays in order.
// The function runs twice: over a null base it measures (bytes() is what to allocate), over the
// allocated buffer it hands out the pointers.  Every array starts 256-byte aligned; an array of no
// elements advances nothing (its pointer is the next array's and is never dereferenced).
class KsimSweepCarver {
 public:
  static constexpr size_t ALIGN = 256;
  explicit KsimSweepCarver(void* base = nullptr) : base_(reinterpret_cast<uintptr_t>(base)) {}
  template <class T>
  T* take(size_t count) {
    T* p = reinterpret_cast<T*>(base_ + off_);
    off_ += (count * sizeof(T) + ALIGN - 1) & ~(ALIGN - 1);
    return p;
  }
  size_t bytes() const { return off_; }

 private:
  uintptr_t base_;
  size_t off_ = 0;
};

// Bytes of a layout at chunk size C.
template <class Layout>
inline size_t ksim_sweep_measure(Layout& layout, size_t C) {
  KsimSweepCarver m;
  layout(m, C);
  return m.bytes();
}

// Scenarios per launch: as many as the budget holds at `per` bytes each, one at least and S at
// most; then the cap (KSIM_SWEEP_CHUNK, null when unset), which never lowers a chunk below one.
inline int32_t ksim_sweep_chunk(size_t S, size_t budget, size_t per, const int* cap) {
  int32_t chunk = (int32_t)std::max<size_t>(1, std::min<size_t>(S, budget / per));
  if (cap) chunk = std::max(1, std::min(chunk, *cap));
  return chunk;
}

// The next chunk to try after an allocation failed (1 stays 1: the caller gives up there).
inline int32_t ksim_sweep_halve(int32_t chunk) { return (chunk + 1) / 2; }
