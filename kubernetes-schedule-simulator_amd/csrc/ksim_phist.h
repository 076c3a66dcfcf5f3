// ksim_phist.h — bookkeeping of the fast kernel's histogram sub-form (ksim_pfast.hip, HIST):
// per tree class, the number of a workgroup's rows at each score.  An evaluation is -1 (the
// row does not fit) or a score in [0, KSIM_PHIST_BUCKETS); bucket s counts the rows at score s
// and -1 is counted nowhere, so for one class
//   F = sum of the buckets, M = the highest non-empty bucket (-1: none), C = its count.
// A row is KSIM_PHIST_BUCKETS 16-bit counts (a workgroup owns < 65,536 rows); two neighbouring
// counts share a 32-bit word, low half first, so the parallel build adds `khist::unit(s)` to
// word `khist::word(s)` atomically and no add carries from one half into the other.
//
// Plain inline functions without device intrinsics: the kernel calls them per lane (lane =
// bucket, `fix`: lane = row) or from one lane, and tests/c/phist_check.cpp and
// tests/c/phist_fix_check.cpp drive them on the host against a recount.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define KSIM_PHIST_FN __host__ __device__ inline
#else
#define KSIM_PHIST_FN inline
#endif

#define KSIM_PHIST_BUCKETS 64  // one bucket per lane: scores 0..63

namespace khist {

// the 32-bit word of a row that holds bucket s, and one count of bucket s in that word
KSIM_PHIST_FN int word(int s) { return s >> 1; }
KSIM_PHIST_FN uint32_t unit(int s) { return 1u << ((s & 1) * 16); }

// Build one class's row from its cache column (n evaluations); `row` aliases
// uint16_t[KSIM_PHIST_BUCKETS] on a little-endian target.  The kernel runs the loop body in
// parallel with an atomic add on the word.
KSIM_PHIST_FN void build(uint32_t* row, const int16_t* col, int n) {
  for (int s = 0; s < KSIM_PHIST_BUCKETS / 2; ++s) row[s] = 0;
  for (int j = 0; j < n; ++j)
    if (col[j] >= 0) row[word(col[j])] += unit(col[j]);
}

// One row's evaluation moved from e_old to e_new (either may be -1).
KSIM_PHIST_FN void move(uint16_t* row, int e_old, int e_new) {
  if (e_old == e_new) return;
  if (e_old >= 0) row[e_old] -= 1;
  if (e_new >= 0) row[e_new] += 1;
}

// Bucket s's count h as it stands after one row moves from e_old to e_new, the row untouched.
KSIM_PHIST_FN int32_t adjusted(int32_t h, int s, int e_old, int e_new) {
  return h - (s == e_old ? 1 : 0) + (s == e_new ? 1 : 0);
}

// The highest non-empty bucket from the mask of non-empty buckets (bit s = bucket s), -1: none.
KSIM_PHIST_FN int top(uint64_t nonempty) { return nonempty ? 63 - __builtin_clzll(nonempty) : -1; }

// (F, M, C) of a row with one of its rows moved from e_old to e_new.
KSIM_PHIST_FN void stats(const uint16_t* row, int e_old, int e_new, int32_t* F, int32_t* M, int32_t* C) {
  uint64_t ne = 0;
  int32_t f = 0;
  for (int s = 0; s < KSIM_PHIST_BUCKETS; ++s) {
    const int32_t h = adjusted(row[s], s, e_old, e_new);
    f += h;
    ne |= (uint64_t)(h != 0) << s;
  }
  const int m = top(ne);
  *F = f;
  *M = m;
  *C = m < 0 ? 0 : adjusted(row[m], m, e_old, e_new);
}

// A test may count how often each case of `fix` below is taken (tests/c/phist_fix_check.cpp).
#ifndef KSIM_PHIST_TAKEN
#define KSIM_PHIST_TAKEN(k) ((void)0)
#endif

// The same (F, M, C) from five numbers of the row instead of the row: F0 its sum, M1 its highest
// non-empty bucket and C1 that bucket, M2 the highest non-empty bucket below M1 and C2 that one
// (M1 / M2 = -1 and C1 / C2 = 0 where there is none).  Exact: every bucket above M1 and every
// bucket strictly between M2 and M1 is empty, so after the row leaves e_old the top is M1 (rows
// left in it), else M2, else nothing, and e_new then enters above it, into it or below it.
// M = -1 whenever C = 0.  Straight-line selects: the kernel runs it per lane (lane = row).
KSIM_PHIST_FN void fix(int32_t F0, int M1, int32_t C1, int M2, int32_t C2, int e_old, int e_new, int32_t* F,
                       int32_t* M, int32_t* C) {
  const bool rem = e_old >= 0, add = e_new >= 0;
  const int32_t c1a = C1 - ((rem && e_old == M1) ? 1 : 0);
  const int mb = c1a ? M1 : (C2 ? M2 : -1);
  const int32_t cb = c1a ? c1a : C2;
  const bool up = add && (cb == 0 || e_new > mb), eq = add && !up && e_new == mb;
  KSIM_PHIST_TAKEN(c1a != C1 ? 0 : 1);                       // the row left the top bucket / another or none
  KSIM_PHIST_TAKEN(c1a ? 2 : C2 ? 3 : 4);                    // top kept / second bucket becomes the top / nothing left
  KSIM_PHIST_TAKEN(!add ? 5 : up ? (cb == 0 ? 6 : 7) : eq ? 8 : 9);  // unfit / into nothing / above / on / below the top
  *F = F0 - (rem ? 1 : 0) + (add ? 1 : 0);
  *M = up ? e_new : mb;
  *C = up ? 1 : cb + (eq ? 1 : 0);
}

}  // namespace khist
