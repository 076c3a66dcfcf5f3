// ksim_decide.h — the end of a pod's scheduling cycle, once for every kernel: from per-reduce-class
// (max map score, count at max) to the winning classes and selectHost's index.
//
//   1. fold (max, count) partials into the class's (M, C)                      ksim_fold_max
//   2. NormalizeReduce of the TaintToleration / NodeAffinity class values over the classes that
//      still have fit nodes (priorities/reduce.go:29-64)
//   3. the weighted sum plus NodePreferAvoidPods' addend                        ksim_class_total
//      (generic_scheduler.go:632-639)
//   4. the best total and the classes that reach it       ksim_decide_serial / ksim_decide_lanes
//   5. ix = lastNodeIndex % (nodes at the best total); the counter moves only when more than one
//      node fits (generic_scheduler.go:141-198)                                ksim_select_ix
//
// The header decides.  Publishing, locating the node, committing and the kernels' mode codes stay
// in the kernels.
#pragma once
#include "ksim_common.h"
#include "ksim_wave.h"

// selectHost's round-robin index (generic_scheduler.go:192-195) with a 32-bit fast path: the
// emulated 64-bit modulo runs only once lastNodeIndex has passed 2^32.  C is a count of nodes at
// the best total: node counts are int32, so it is always below 2^32 (and > 0 when selectHost runs).
__device__ __forceinline__ int64_t ksim_select_ix(uint64_t counter, uint32_t C) {
  return (counter >> 32) ? (int64_t)(counter % (uint64_t)C) : (int64_t)((uint32_t)counter % C);
}

// Fold one partial (max score mb, cb nodes at it) into (m, n).  A partial without nodes carries no
// score.  S: int32 scores of the granule kernels, int64 of the launch kernels.
template <class S>
__device__ __forceinline__ void ksim_fold_max(S& m, int32_t& n, S mb, int32_t cb) {
  if (cb == 0) return;
  if (mb > m) { m = mb; n = cb; }
  else if (mb == m) n += cb;
}

// Total score of a reduce class once the maxima over the filtered set are known.  base: the class's
// max map score; tv / av: its TaintToleration / NodeAffinity map values; ad: NodePreferAvoidPods'
// weighted score of the class.  Go int arithmetic: wrapping.
__device__ __forceinline__ int64_t ksim_class_total(const KsimCtx& c, int64_t base, int64_t tv, int64_t av, int64_t ad,
                                                    int64_t mxT, int64_t mxA) {
  uint64_t t = (uint64_t)base + (uint64_t)ad;
  if (c.w[KSIM_W_TAINT_TOLERATION]) t += (uint64_t)c.w[KSIM_W_TAINT_TOLERATION] * (uint64_t)ksim_norm(tv, mxT, true);
  if (c.w[KSIM_W_NODE_AFFINITY]) t += (uint64_t)c.w[KSIM_W_NODE_AFFINITY] * (uint64_t)ksim_norm(av, mxA, false);
  return (int64_t)t;
}

// A maximum is read only by a term with a non-zero weight (a zero weight with more than one class
// still splits the nodes into classes, but the term adds nothing), so the lane form reduces it only
// then.  The serial form keeps the launch kernels' wider condition (k > 1 || weight), k1 / k2 being
// the pod's TaintToleration / NodeAffinity class counts.

// One thread, K <= KSIM_MAX_RCLASS classes (class q: Mq[q], Cq[q] nodes at it, 0 = no fit node).
// Returns the number of nodes at the best total; win: the classes that reach it.  UNROLL: the
// caller's arrays are private, so the loops run unrolled to the constant bound and no array is
// indexed by a run-time class (it would live in scratch memory); else (arrays in LDS) they run to K.
template <bool UNROLL>
__device__ __forceinline__ int64_t ksim_decide_serial(const KsimCtx& c, int K, int k1, int k2, const int64_t* Mq, const int32_t* Cq,
                                                      const int64_t* tv, const int64_t* av, const int64_t* ad,
                                                      uint32_t& win, int64_t& best) {
  constexpr int U = UNROLL ? KSIM_MAX_RCLASS : 1;
  const int n = UNROLL ? KSIM_MAX_RCLASS : K;
  int64_t mxT = 0, mxA = 0;
#pragma unroll U
  for (int q = 0; q < n; ++q) {
    if (q >= K || Cq[q] == 0) continue;
    if (k1 > 1 || c.w[KSIM_W_TAINT_TOLERATION]) mxT = tv[q] > mxT ? tv[q] : mxT;
    if (k2 > 1 || c.w[KSIM_W_NODE_AFFINITY]) mxA = av[q] > mxA ? av[q] : mxA;
  }
  int64_t C = 0;
  best = INT64_MIN;
  win = 0;
#pragma unroll U
  for (int q = 0; q < n; ++q) {
    if (q >= K || Cq[q] == 0) continue;
    const int64_t t = ksim_class_total(c, Mq[q], tv[q], av[q], ad[q], mxT, mxA);
    if (t > best) { best = t; win = 1u << q; C = Cq[q]; }
    else if (t == best) { win |= 1u << q; C += Cq[q]; }
  }
  return C;
}

// The wave reductions of the lane form: R::max over int64, R::sum over int32, and R::NONE, the
// total of a lane without a class (below every real total).  Over the whole wave, or over the first
// 16 lanes (one DPP row) for callers whose class lanes are 0..15 and whose other lanes are not live.
struct KsimReduceWave {
  static constexpr int64_t NONE = INT64_MIN;
  static __device__ __forceinline__ int64_t max(int64_t v) { return ksimw::max_i64(v); }
  static __device__ __forceinline__ int32_t sum(int32_t v) { return ksimw::sum_i32(v); }
};
struct KsimReduceRow16 {
  static constexpr int64_t NONE = INT64_MIN;
  static __device__ __forceinline__ int64_t max(int64_t v) { return ksimw::max16_i64(v); }
  static __device__ __forceinline__ int32_t sum(int32_t v) { return ksimw::sum16_i32(v); }
};

// Lane q = reduce class q.  live: the class has fit nodes; M, C: its max map score and count.
// Returns the number of nodes at the best total; win: ballot of the classes that reach it.
template <class R>
__device__ __forceinline__ int32_t ksim_decide_lanes(const KsimCtx& c, bool live, int64_t M, int32_t C, int64_t tv,
                                                     int64_t av, int64_t ad, uint64_t& win, int64_t& best) {
  const int64_t mxT = c.w[KSIM_W_TAINT_TOLERATION] ? R::max(live ? tv : 0) : 0;
  const int64_t mxA = c.w[KSIM_W_NODE_AFFINITY] ? R::max(live ? av : 0) : 0;
  const int64_t t = live ? ksim_class_total(c, M, tv, av, ad, mxT, mxA) : R::NONE;
  best = R::max(t);
  const bool w = live && t == best;
  win = __ballot(w);
  return R::sum(w ? C : 0);
}
