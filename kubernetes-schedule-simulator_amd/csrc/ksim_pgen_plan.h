// ksim_pgen_plan.h — the launch geometry of the general persistent kernels (ksim_pgen.hip), decided
// from sizes alone (ksim_runtime.cpp, pgen_plan): no device include and no handle, so that a host
// program can sweep every node count against the launchers' conditions (tests/c/pgen_plan_check.cpp).
// The LDS byte count of a candidate comes from the caller (ksim_pgen_plan in ksim_pgen.hip).
#pragma once
#include <stddef.h>
#include <stdint.h>

// What the launchers accept (ksim_launch_pgen, ksim_launch_pgen2; ksim_pgen.hip asserts its own
// constants against these).
#define KSIM_PGP_MAX_GRID 256   // workgroups, either form
#define KSIM_PGP_MAX_GRID2 64   // the dual form: one granule per lane in its sweeps
#define KSIM_PGP_RT1 256        // rows per thread slot, single form (x 1, 2 or 4 rows per thread)
#define KSIM_PGP_RT2 192        // ... dual form

struct KsimPgenPlanIn {
  int64_t n;          // node rows (> 0)
  int32_t max_grid;   // the handle's workgroup cap (KSIM_MAX_GRID; <= 0 or >= 256: none)
  bool allow_dual;    // false: the single form only (KSIM_PGEN_V1, the service-affinity lender)
  bool hdense_ok;     // the dense hypothesis deltas may be staged (dual form only)
  int32_t n_st;       // pod classes whose static words are staged when they fit
  int64_t chunk_hint; // KSIM_PGEN_CHUNK (0: none): rows per workgroup to start from
  size_t budget;      // LDS bytes of a workgroup
};

struct KsimPgenPlanOut {
  bool dual;
  int32_t grid, npt;  // workgroups, rows per thread (1, 2, 4)
  int64_t chunk;      // rows per workgroup
  int32_t n_st, hdense;
  size_t lds;
};

// One form: the largest chunk of the search (from max(cmin, one thread slot) or the hint, down by
// eighths to cmin) whose bytes fit, dropping first the static words, then the dense deltas.
// bytes(chunk, dual, n_st, hdense) -> LDS bytes.  False: this form cannot hold the table.
template <class Bytes>
inline bool ksim_pgen_plan_form(const KsimPgenPlanIn& in, bool dual, Bytes bytes, KsimPgenPlanOut* out) {
  const int64_t gcap = (in.max_grid > 0 && in.max_grid < KSIM_PGP_MAX_GRID) ? in.max_grid : KSIM_PGP_MAX_GRID;
  const int64_t rt = dual ? KSIM_PGP_RT2 : KSIM_PGP_RT1;
  int64_t cmin = (in.n + gcap - 1) / gcap;
  if (dual) {
    const int64_t c2 = (in.n + KSIM_PGP_MAX_GRID2 - 1) / KSIM_PGP_MAX_GRID2;
    cmin = cmin > c2 ? cmin : c2;
  }
  if (in.n <= 0 || cmin > 4 * rt) return false;  // more rows per workgroup than four per thread
  int64_t chunk = cmin > rt ? cmin : rt;
  if (chunk > in.n) chunk = in.n;
  if (in.chunk_hint) {
    chunk = in.chunk_hint < 4 * rt ? in.chunk_hint : 4 * rt;
    if (chunk < cmin) chunk = cmin;
  }
  const int32_t hd = (dual && in.hdense_ok) ? 1 : 0;
  for (;;) {
    out->n_st = in.n_st;
    out->hdense = hd;
    size_t lds = bytes(chunk, dual, out->n_st, out->hdense);
    if (lds > in.budget) {
      out->n_st = 0;
      lds = bytes(chunk, dual, out->n_st, out->hdense);
    }
    if (lds > in.budget && out->hdense) {
      out->hdense = 0;
      lds = bytes(chunk, dual, out->n_st, out->hdense);
    }
    if (lds <= in.budget) {
      out->lds = lds;
      break;
    }
    if (chunk <= cmin) return false;
    const int64_t next = chunk * 7 / 8;
    chunk = next > cmin ? next : cmin;
  }
  out->dual = dual;
  out->chunk = chunk;
  out->grid = (int32_t)((in.n + chunk - 1) / chunk);
  out->npt = chunk <= rt ? 1 : chunk <= 2 * rt ? 2 : 4;
  return true;
}

// The dual form when it can launch the table (at most 64 workgroups of at most 768 rows under the
// cap), else the single form (256 of 1,024); false when neither holds it: the launch form then does.
template <class Bytes>
inline bool ksim_pgen_plan_geometry(const KsimPgenPlanIn& in, Bytes bytes, KsimPgenPlanOut* out) {
  if (in.allow_dual && ksim_pgen_plan_form(in, true, bytes, out)) return true;
  return ksim_pgen_plan_form(in, false, bytes, out);
}
