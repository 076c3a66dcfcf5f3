// ksim_sweep_kernels.h — the device text that both sweep units compile: the scan kernel and the general
// kernel as templates, the record helpers, the LDS words and the constants.  ksim_sweep.hip instantiates
// every kernel but the VOL ones, ksim_sweep_vol.hip those; each unit names its instantiations in its
// launcher, and the argument struct of an instantiation is built here, once, for both.
#pragma once
#include <type_traits>

#include "ksim_decide.h"
#include "ksim_sweep.h"
#include "ksim_wave.h"

using namespace kf64;

namespace {
constexpr int SB = 1024;      // threads per scenario workgroup
constexpr int SW = SB / 64;   // waves
constexpr uint16_t NOFIT = 0xFFFF;

// FitError histogram of a failed pod (the WHY instantiations): the wave's reason masks, one row per
// lane (0 = no row, an absent node, or a node that fits), into the workgroup's LDS histogram — one
// ballot, popcount and LDS atomic add per reason present in the wave.  Wave-uniform control flow.
__device__ __forceinline__ void why_add(uint32_t rm, int lane, int32_t* s_hist) {
  uint64_t b;
  while ((b = __ballot(rm != 0))) {
    const uint32_t ml = (uint32_t)__builtin_amdgcn_readlane((int)rm, __builtin_ctzll(b));
    const int r = __builtin_ctz(ml);
    const int32_t nr = (int32_t)__popcll(__ballot((rm >> r) & 1u));
    if (lane == 0) atomicAdd(&s_hist[r], nr);
    rm &= ~(1u << r);
  }
}

// the record of the scenario's k-th failed pod, pod p of the range: threads 0..31 the histogram,
// thread 0 the pod (after the barrier that ends the histogram pass)
__device__ __forceinline__ void why_store(const SwWhy& y, int s, int32_t k, int32_t p, int tid, const int32_t* s_hist) {
  const int64_t rec = (int64_t)s * y.cap + k;
  if (tid < KSIM_NREASONS) y.hist[rec * KSIM_NREASONS + tid] = s_hist[tid];
  if (tid == 0) y.pod[rec] = p;
}
}  // namespace


// WHY (ksim_sweep_explain): a pod that fits nowhere is evaluated once more for its reason masks
// while the scenario has kept fewer than cap records; nothing else differs.
template <bool ABS, bool WHY>
__global__ __launch_bounds__(SB) void ksim_sweep_kernel(std::conditional_t<WHY, SwArgsWhy, SwArgs> a) {
  extern __shared__ uint16_t sc[];  // [n] evaluations of the current pod
  __shared__ int32_t s_red[SW][3];
  __shared__ int32_t s_wtot[SW];
  int32_t nfail = 0;  // WHY: failed pods of this scenario so far (uniform)
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int s = blockIdx.x;
  const int64_t n = a.n;
  const int64_t off = (int64_t)s * n;
  const int sw = a.scen0 + s;
  const EvCfg EC = make_evcfg(a.preds, a.no_prio != 0, a.w[3 * sw], a.w[3 * sw + 1], a.w[3 * sw + 2]);
  double* const rc = a.rc + off;
  double* const rm = a.rm + off;
  double* const zc = a.zc + off;
  double* const zm = a.zm + off;
  int32_t* const cnt = a.count + off;
  const int64_t K = (n + SB - 1) / SB;  // contiguous segment per thread in the select phase
  const int64_t seg0 = (int64_t)tid * K, seg1 = (seg0 + K < n) ? seg0 + K : n;
  uint64_t counter = a.counter0;  // genericScheduler.lastNodeIndex of this scenario

  for (int32_t p = 0; p < a.n_pods; ++p) {
    const FPod P = a.pods[p];
    // ---- 1. evaluate every row ----
    int32_t f = 0, mx = -1, cm = 0;
#pragma unroll 4
    for (int64_t j = tid; j < n; j += SB) {
      FRow r;
      r.ac = a.dac[j]; r.am = a.dam[j]; r.yc = a.yc[j]; r.ym = a.ym[j];
      r.rc = rc[j]; r.rm = rm[j]; r.zc = zc[j]; r.zm = zm[j];
      r.allowed = a.allowed[j]; r.count = cnt[j]; r.fl = a.flags[j];
      uint32_t rmask;
      int32_t e = feval(EC, P, r, rmask);
      if constexpr (ABS) e = r.count < 0 ? -1 : e;  // a node this scenario does not list
      sc[j] = e < 0 ? NOFIT : (uint16_t)e;
      f += e >= 0 ? 1 : 0;
      cm = e > mx ? 1 : cm + ((e == mx && e >= 0) ? 1 : 0);
      mx = e > mx ? e : mx;
    }
    // ---- 2. block reduction: F, M, C ----
    {
      const int32_t Fw = ksimw::sum_i32(f);
      const int32_t Mw = ksimw::max_i32(mx);
      const int32_t Cw = ksimw::sum_i32((mx == Mw && mx >= 0) ? cm : 0);
      if (lane == 0) { s_red[wv][0] = Fw; s_red[wv][1] = Mw; s_red[wv][2] = Cw; }
    }
    __syncthreads();
    const bool in = lane < SW;
    const int32_t F = ksimw::sum_i32(in ? s_red[in ? lane : 0][0] : 0);
    const int32_t mw = in ? s_red[lane][1] : -1;
    const int32_t M = ksimw::max_i32(mw);
    const int32_t C = ksimw::sum_i32((in && mw == M && M >= 0) ? s_red[lane][2] : 0);
    if (F == 0) {  // FitError: no node fits
      if (tid == 0) a.out_node[(int64_t)s * a.n_pods + p] = -1;
      if constexpr (WHY) {
        __shared__ int32_t s_hist[KSIM_NREASONS];
        if (nfail < a.why.cap) {  // (uniform) one more pass over the rows, for the reason masks
          if (tid < KSIM_NREASONS) s_hist[tid] = 0;
          __syncthreads();
          for (int64_t j0 = tid - lane; j0 < n; j0 += SB) {  // j0: the wave's first row of the round
            const int64_t j = j0 + lane;
            uint32_t rmask = 0;
            if (j < n) {
              FRow r;
              r.ac = a.dac[j]; r.am = a.dam[j]; r.yc = a.yc[j]; r.ym = a.ym[j];
              r.rc = rc[j]; r.rm = rm[j]; r.zc = zc[j]; r.zm = zm[j];
              r.allowed = a.allowed[j]; r.count = cnt[j]; r.fl = a.flags[j];
              (void)feval(EC, P, r, rmask);
              if constexpr (ABS) rmask = r.count < 0 ? 0u : rmask;  // not listed: not evaluated
            }
            why_add(rmask, lane, s_hist);
          }
          __syncthreads();
          why_store(a.why, s, nfail, p, tid, s_hist);
        }
        ++nfail;
      }
      __syncthreads();  // s_red (and s_hist) are rewritten by the next pod
      continue;
    }
    const uint32_t ix = (F > 1) ? (uint32_t)ksim_select_ix(counter, (uint32_t)C) : 0u;
    counter += (F > 1) ? 1 : 0;  // generic_scheduler.go:192-195 (selectHost only when F > 1)
    // ---- 3. the ix-th row at M from the top ----
    int32_t c_t = 0;
    for (int64_t j = seg0; j < seg1; ++j) c_t += (sc[j] == (uint16_t)M) ? 1 : 0;
    const int32_t pre = ksimw::prefix_incl_i32(c_t);  // within the wave
    if (lane == 63) s_wtot[wv] = pre;
    __syncthreads();
    int32_t below = 0;  // matches in lower waves
    for (int w = 0; w < SW; ++w) below += (w < wv) ? s_wtot[w] : 0;
    const uint32_t above = (uint32_t)(C - (below + pre));  // matches in higher threads
    if (c_t > 0 && ix >= above && ix < above + (uint32_t)c_t) {
      int32_t r = (int32_t)(ix - above);
      int64_t jsel = -1;
      for (int64_t j = seg1 - 1; j >= seg0; --j) {
        if (sc[j] == (uint16_t)M) {
          if (r == 0) { jsel = j; break; }
          --r;
        }
      }
      // ---- 4. commit ----
      if (jsel >= 0) {
        rc[jsel] += P.ad_c; rm[jsel] += P.ad_m; zc[jsel] += P.nz_c; zm[jsel] += P.nz_m; cnt[jsel] += 1;
      }
      a.out_node[(int64_t)s * a.n_pods + p] = (int32_t)jsel;
    }
    __syncthreads();  // the commit (workgroup release/acquire) before the next pod's loads
  }
  if (tid == 0) a.out_counter[s] = counter;
}

// ---- the general form ----
// Per pod:
//   1. every thread evaluates rows j = tid, tid+1024, ...: a node the scenario does not list (sign
//      bit of its pod count) is NOFIT before any predicate reads the count; ksim_predicates_a, then
//      for a fit node ksim_map_score and ksim_rclass_a; the packed word goes to LDS.  With more than
//      one reduce class the class's maximum is kept by an LDS atomic max (taken only by a score
//      above the value read first); with one class (max, count) stay in registers as in the scan;
//   2. F over the workgroup; per class the nodes at its maximum (one pass over the thread's
//      contiguous LDS segment, one LDS atomic add per wave, step and class present);
//   3. every wave runs ksim_decide_lanes over the classes (lane = class) -> winning classes and
//      the nodes C at the best total; ix = lastNodeIndex % C when more than one node fits;
//   4. the ix-th node from the top of the name order among the winning classes' nodes at their
//      class maximum (the scan form's block prefix over contiguous segments); its thread commits
//      with ksim_commit into the scenario's columns.
// The per-class words are double-buffered by pod parity: the buffer of the next pod is reset
// between two barriers of this one, so no reset races the next pod's atomics.
namespace {
constexpr uint32_t GNOFIT = 0xFFFFFFFFu;

// The accessor of ksim_predicates_a / ksim_rclass_a (ksim_common.h, KsimGlobalAcc) with the pod
// class's table entries of the node loaded together up front: the predicates return at the first
// failure, so the global accessor's loads (set id, then table word, per predicate) would each wait
// for the one before.
struct SwgAcc {
  const KsimCtx& c;
  bool sel, tok, nok;
  int ttc, nac;
  __device__ __forceinline__ bool sel_ok(const ksim_pod&, int64_t) const { return sel; }
  __device__ __forceinline__ bool taint_ok(const ksim_pod&, int64_t) const { return tok; }
  __device__ __forceinline__ bool noexec_ok(const ksim_pod&, int64_t) const { return nok; }
  __device__ __forceinline__ bool port_conflict(int64_t i, uint64_t want) const { return ksim_port_conflict(c, i, want); }
  __device__ __forceinline__ uint64_t want(const ksim_pod& P, int32_t k) const { return ksim_pod_port(c, P, k); }
  __device__ __forceinline__ int tt_class(const ksim_pod&, int64_t) const { return ttc; }
  __device__ __forceinline__ int na_class(const ksim_pod&, int64_t) const { return nac; }
};

// LDS of the SPR instantiations only: countsByZone of the pod (buffer = the step's parity, the other
// one is reset between two barriers, as the class words are), and the second block reduction's words.
struct SwgSpreadLds {
  unsigned long long z[2][KSIM_SWEEP_SPREAD_MAX_ZONES];
  int32_t red[SW][2];
};
__device__ __forceinline__ SwgSpreadLds& swg_spread_lds() {
  __shared__ SwgSpreadLds l;
  return l;
}
// LDS of the IPA instantiations only: each wave's (min, max) raw InterPodAffinityPriority sum
struct SwgIpaLds {
  int64_t mm[SW][2];
};
__device__ __forceinline__ SwgIpaLds& swg_ipa_lds() {
  __shared__ SwgIpaLds l;
  return l;
}
constexpr int SWG_AGG_ZONES = 16;  // up to here a wave adds one sum per zone it holds, not one per lane
}  // namespace

// WHY (ksim_sweep_explain): as in the scan form, the reason masks from ksim_predicates_a.  The packed
// word in LDS cannot carry a mask (27 score bits + 4 class bits), so the pass re-evaluates.
//
// PRE (ksim_sweep_drain): the scenario's queue is its prefix pods, then the range.  Step q of it takes
// pod pre[off + q] for q < m and pod first + q - m after, and answers into out_pre or out_node; m
// and the pod's index are uniform (scalar loads from the kernel arguments' pointers).  The index of
// step q + 1 is fetched at the top of step q, so that a step starts with the pod record's load as
// the range's steps do, not with index -> record -> class tables in a row.  The class words'
// buffer is the parity of q: the range's own index would repeat the last prefix step's buffer at an
// odd m.  A record of why holds q.
//
// SPR (a range or prefix pod with SelectorSpread state; the tables hold nothing else): a pod whose
// class has a spread pair scores CalculateSpreadPriorityReduce (selector_spreading.go:121-174) over the
// scenario's fit nodes.  Step 1 also loads each fit row's count and zone, keeps the maximum count and
// haveZones, and adds the count to the zone's LDS word; its packed word holds the map score alone, and
// neither (M, C) nor a class maximum is taken from it.  After the block reduction of (F, maximum
// count, haveZones) every wave takes the maximum zone word, and each thread revisits its own rows
// (the same j = tid + k * 1024, so its own words: no barrier on sg), adds weight x ksim_spread_score,
// rewrites the word and only then takes (M, C) or the class maximum; one more barrier publishes them.
// The count and zone are reloaded there, not kept: the kernel has no registers to spare.  The
// committing thread also runs ksim_aff_commit_body on the scenario's counts, for every pod with an
// identity.  Barriers per pod: 3 with one reduce class and 4 with several, as ever; a pod that reads a
// spread pair takes one more (4 and 5).  A pod without a pair scores a constant: today's steps.
//
// IPA (ksim_sweep_affinity, on top of SPR: the tables hold inter-pod affinity terms): the scenario's
// KsimCtx::aff is its own descriptor, so ksim_predicates_a evaluates MatchInterPodAffinity at its place
// in predicatesOrdering, in step 1 and in the WHY pass, over the scenario's cnt and carried.  A pod
// that reads InterPodAffinityPriority (uniform: ksim_interpod_prio_work) stores each fit row's raw sum
// in the scenario's raw column and keeps the thread's (min, max), both from 0; the block reduction
// carries them as int64 words, and step 1b adds weight x ksim_interpod_score beside the spread term, if
// any, before (M, C) or the class maxima are taken.  A thread rereads only the raw words it wrote: no
// barrier.  A pod that reads either priority, or both, takes step 1b's one barrier more; a pod with
// neither identity nor class takes exactly the SPR steps.  The commit is ksim_aff_commit_body on both
// copies.
//
// VOL (ksim_sweep_volumes, beside the plain, SPR and IPA forms with ABS and WHY on: a range or prefix
// pod may mount volumes): the scenario's KsimCtx::vol is its own descriptor over its own mounts
// (ksim_sweep_volume_init_kernel), so ksim_predicates_a evaluates NoDiskConflict, the MaxPD filters and
// NoVolumeZoneConflict at their places in predicatesOrdering, in step 1 and in the WHY pass, as it does
// in every instantiation whenever vol is set.  The one difference to the parent instantiation: the
// committing thread also adds the pod's mounts to the chosen node's slots (ksim_vol_commit_body, +1) after
// ksim_commit, and the closing barrier publishes them with the columns.  A full node or a saturated
// mount count sets bit 1 of the sweep's own error word, the bit of ksim_commit's port slots.
template <bool ABS, bool WHY, bool PRE = false, bool SPR = false, bool IPA = false, bool VOL = false>
__global__ __launch_bounds__(SB) void ksim_sweep_general_kernel(
    const KsimCtx* __restrict__ ctxs,
    const std::conditional_t<IPA, SwgArgsIpa, std::conditional_t<SPR, SwgArgsSpr,
                             std::conditional_t<PRE, SwgArgsPre, std::conditional_t<WHY, SwgArgsWhy, SwgArgs>>>> a) {
  static_assert(SPR || !IPA, "the IPA instantiations extend the SPR ones");
  static_assert(!VOL || (ABS && WHY), "the VOL instantiations have ABS and WHY on");
  extern __shared__ uint32_t sg[];  // [n] evaluations of the current pod
  __shared__ int32_t s_red[SW][3];
  __shared__ int32_t s_wtot[SW];
  __shared__ int32_t s_M[2][KSIM_MAX_RCLASS];  // max map score among the class's fit nodes (-1: none)
  __shared__ int32_t s_C[2][KSIM_MAX_RCLASS];  // nodes at it
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int s = blockIdx.x;
  // the scenario's context (ksim_sweep_general_ctx_kernel): read-only here, so its fields are
  // uniform loads; a private modified copy of the kernel argument would live in scratch memory
  // (the per-pod port / scalar arrays are indexed at run time)
  const KsimCtx& c = ctxs[s];
  const int64_t n = c.n;
  const int64_t KS = (n + SB - 1) / SB;  // contiguous segment per thread in the count and select phases
  const int64_t seg0 = (int64_t)tid * KS, seg1 = (seg0 + KS < n) ? seg0 + KS : n;
  uint64_t counter = a.counter0;  // genericScheduler.lastNodeIndex of this scenario
  int32_t nfail = 0;              // WHY: failed pods of this scenario so far (uniform)
  if (tid < 2 * KSIM_MAX_RCLASS) {
    (&s_M[0][0])[tid] = -1;
    (&s_C[0][0])[tid] = 0;
  }
  // SPR: the scenario's tables, its zone row and zone count (uniform), both buffers of zone words
  const KsimAff* Ap = nullptr;
  const int32_t* zrow = nullptr;
  int32_t nz = 0;
  if constexpr (SPR) {
    Ap = a.aff + s;
    if (Ap->zone_key >= 0) {
      zrow = Ap->dom + (int64_t)Ap->zone_key * n;
      nz = Ap->n_zone;  // <= KSIM_SWEEP_SPREAD_MAX_ZONES (host-checked)
    }
    if constexpr (IPA) {  // more zones are swept when no class has a spread pair: the zone words stay unused
      if (nz > KSIM_SWEEP_SPREAD_MAX_ZONES) {
        zrow = nullptr;
        nz = 0;
      }
    }
    for (int z = tid; z < 2 * KSIM_SWEEP_SPREAD_MAX_ZONES; z += SB) (&swg_spread_lds().z[0][0])[z] = 0;
  }
  int64_t* rawc = nullptr;  // IPA: the scenario's column of raw InterPodAffinityPriority sums
  if constexpr (IPA) rawc = a.raw + (int64_t)s * n;
  __syncthreads();
  // PRE: the scenario's prefix pre[0 .. m) and the queue index of its step q (uniform)
  int32_t m = 0;
  const int64_t* pre = nullptr;
  int32_t* out_pre = nullptr;
  if constexpr (PRE) {
    const int64_t o0 = a.off[a.scen0 + s];
    m = (int32_t)(a.off[a.scen0 + s + 1] - o0);
    pre = a.pod + o0;
    out_pre = a.out_pre + o0;
  }
  const int32_t nq = m + a.n_pods;  // <= INT32_MAX (host-checked)
  // pre is written before the launch and never by a kernel: read through the constant address space,
  // a uniform index is then a scalar load whatever the loop has stored since
  typedef const int64_t __attribute__((address_space(4))) * ConstI64;
  auto index_of = [&](int32_t q) -> int64_t { return q < m ? ((ConstI64)(uintptr_t)pre)[q] : a.first + (q - m); };
  auto answer_of = [&](int32_t q) -> int32_t* {
    if constexpr (PRE) {
      if (q < m) return out_pre + q;
    }
    return a.out_node + ((int64_t)s * a.n_pods + (q - m));
  };
  int64_t inext = 0;
  if constexpr (PRE) inext = nq > 0 ? index_of(0) : 0;

  for (int32_t p = 0; p < nq; ++p) {  // p: the step q of the scenario's queue
    int64_t ip = a.first + p;
    if constexpr (PRE) {
      ip = inext;
      if (p + 1 < nq) inext = index_of(p + 1);  // in flight during this pod's rows
    }
    const ksim_pod P = c.pods[ip];
    const int k1 = (c.w[KSIM_W_TAINT_TOLERATION] != 0) ? c.n_tt[P.cls] : 1;
    const int k2 = c.use_na ? c.n_na[P.cls] : 1;
    const int K = k1 * k2;  // <= KSIM_MAX_RCLASS (host-checked)
    const int pb = p & 1;
    const bool tabs = (P.flags & (KSIM_POD_NEED_SELECTOR | KSIM_POD_NEED_TAINTS)) || K > 1;
    // the decision's per-class values, lane = class (loaded now, read after the evaluation)
    int64_t tv = 0, av = 0, ad = 0;
    if (K > 1 && lane < K) {
      tv = c.tt_val[(int64_t)P.cls * c.val_w + lane / k2];
      av = c.na_val[(int64_t)P.cls * c.val_w + lane % k2];
      ad = c.na_add ? c.na_add[(int64_t)P.cls * c.val_w + lane % k2] : 0;
    }
    // SPR: the pod's SelectorSpread pair (uniform; -1: none, a constant score), the scenario's counts
    // of it per node, the zone words of this step and the thread's maximum count / haveZones
    int32_t sp = -1, mxc = 0, hzt = 0;
    const int32_t* scnt = nullptr;
    unsigned long long* zw = nullptr;
    if constexpr (SPR) {
      if (c.w[KSIM_W_SELECTOR_SPREAD] != 0 && !c.no_prio) sp = ksim_spread_pair(*Ap, P);
      if (sp >= 0) scnt = Ap->cnt + Ap->pair_off[sp];
      zw = swg_spread_lds().z[pb];
    }
    // IPA: does the pod read InterPodAffinityPriority (uniform)?  The thread's min / max raw sum over
    // its fit rows, both from 0 (interpod_affinity.go:129-131).  two: the score is completed in step 1b
    bool ipa = false;
    int64_t rmn = 0, rmx = 0;
    if constexpr (IPA) ipa = c.w[KSIM_W_INTERPOD_AFFINITY] != 0 && !c.no_prio && ksim_interpod_prio_work(*Ap, P);
    auto two = [&]() -> bool {
      if constexpr (IPA) return sp >= 0 || ipa;
      return SPR && sp >= 0;
    };
    // ---- 1. evaluate every row ----
    int32_t f = 0, mx = -1, cm = 0;
    for (int64_t j = tid; j < n; j += SB) {
      const KsimRow r = ksim_load_row(c, j);
      SwgAcc acc{c, true, true, true, 0, 0};
      if (tabs) {  // uniform: the pod reads a class table
        const int64_t cl = P.cls;
        const int32_t ls = c.label_set[j], ts = c.taint_set[j];
        if (P.flags & KSIM_POD_NEED_SELECTOR) acc.sel = ksim_bit(c.sel_ok, cl, c.lwords, ls);
        if (P.flags & KSIM_POD_NEED_TAINTS) {
          acc.tok = ksim_bit(c.taint_ok, cl, c.twords, ts);
          acc.nok = ksim_bit(c.noexec_ok, cl, c.twords, ts);
        }
        if (k1 > 1) acc.ttc = c.tt_class[cl * c.n_taint_sets + ts];
        if (k2 > 1) acc.nac = c.na_class[cl * c.n_label_sets + ls];
      }
      int32_t cv = 0, zj = -1;  // SPR: the row's count and zone, loaded with the row (used when it fits)
      if constexpr (SPR) {
        if (sp >= 0) {
          cv = scnt[j];
          if (zrow) zj = zrow[j];
        }
      }
      bool fit = true;
      if constexpr (ABS) fit = r.count >= 0;  // a node this scenario does not list
      if (fit) fit = ksim_predicates_a<SwgAcc, true, true>(c, P, j, r, acc) == 0;
      uint32_t wd = GNOFIT;
      if (fit) {
        const int32_t e = (int32_t)ksim_map_score(c, P, r);  // < 2^27 (host-checked weights)
        int q = 0;
        if (K > 1) {
          q = ksim_rclass_a(P, j, k1, k2, acc);
          // (SPR, a spread pod: the score is incomplete, the class maximum is taken in step 1b; IPA: of
          // any pod that takes step 1b.  Kept apart: the other instantiations compile to what they were)
          bool now = !SPR || sp < 0;
          if constexpr (IPA) now = !two();
          if (now && e > __hip_atomic_load(&s_M[pb][q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))
            atomicMax(&s_M[pb][q], e);
        }
        wd = ((uint32_t)e << 4) | (uint32_t)q;
        f += 1;
        cm = e > mx ? 1 : cm + (e == mx ? 1 : 0);
        mx = e > mx ? e : mx;
        if constexpr (IPA) {
          if (ipa) {  // uniform
            const int64_t raw = ksim_interpod_raw_body(*Ap, P, j);
            rawc[j] = raw;
            rmn = raw < rmn ? raw : rmn;
            rmx = raw > rmx ? raw : rmx;
          }
        }
      }
      sg[j] = wd;
      if constexpr (SPR) {
        if (sp >= 0) {  // uniform
          mxc = (fit && cv > mxc) ? cv : mxc;
          hzt |= (fit && zj >= 0) ? 1 : 0;
          const int64_t add = (fit && zj >= 0) ? (int64_t)cv : 0;
          // the wave's rows of this round are j - lane .. j - lane + 63: all below n = every lane is here
          if (nz <= SWG_AGG_ZONES && j - lane + 64 <= n) {
            uint64_t m = __ballot(add != 0);
            while (m) {  // uniform: one step, one wave sum and one LDS add per zone among the wave's counts
              const int l = __builtin_ctzll(m);
              const int32_t zl = __builtin_amdgcn_readlane(zj, l);
              const bool mine = add != 0 && zj == zl;
              const int64_t tot = ksimw::sum_i64(mine ? add : 0);
              if (lane == l) atomicAdd(&zw[zl], (unsigned long long)tot);
              m &= ~__ballot(mine);
            }
          } else if (add != 0) {
            atomicAdd(&zw[zj], (unsigned long long)add);
          }
        }
      }
    }
    // ---- 2. block reduction: F, and for one class M, C ----
    {
      const int32_t Fw = ksimw::sum_i32(f);
      const int32_t Mw = ksimw::max_i32(mx);
      const int32_t Cw = ksimw::sum_i32((mx == Mw && mx >= 0) ? cm : 0);
      if (lane == 0) { s_red[wv][0] = Fw; s_red[wv][1] = Mw; s_red[wv][2] = Cw; }
      if constexpr (SPR) {
        if (sp >= 0) {  // a spread pod: the maximum count and haveZones in place of (M, C)
          const int32_t Xw = ksimw::max_i32(mxc), Hw = ksimw::max_i32(hzt);
          if (lane == 0) { s_red[wv][1] = Xw; s_red[wv][2] = Hw; }
        }
      }
      if constexpr (IPA) {
        if (ipa) {
          const int64_t Nw = ksimw::min_i64(rmn), Xw = ksimw::max_i64(rmx);
          if (lane == 0) { swg_ipa_lds().mm[wv][0] = Nw; swg_ipa_lds().mm[wv][1] = Xw; }
        }
      }
    }
    __syncthreads();
    if (tid < KSIM_MAX_RCLASS) {  // the next pod's class words
      s_M[pb ^ 1][tid] = -1;
      s_C[pb ^ 1][tid] = 0;
    }
    if constexpr (SPR) {
      if (tid < nz) swg_spread_lds().z[pb ^ 1][tid] = 0;  // ... and its zone words
    }
    const bool in = lane < SW;
    const int32_t F = ksimw::sum_i32(in ? s_red[in ? lane : 0][0] : 0);
    const int32_t mw = in ? s_red[lane][1] : -1;
    int32_t M = ksimw::max_i32(mw);
    int32_t C = ksimw::sum_i32((in && mw == M && M >= 0) ? s_red[lane][2] : 0);
    if (F == 0) {  // FitError: no node fits
      if (tid == 0) *answer_of(p) = -1;
      if constexpr (WHY) {
        __shared__ int32_t s_hist[KSIM_NREASONS];
        if (nfail < a.why.cap) {  // (uniform) one more pass over the rows, for the reason masks
          if (tid < KSIM_NREASONS) s_hist[tid] = 0;
          __syncthreads();
          for (int64_t j0 = tid - lane; j0 < n; j0 += SB) {  // j0: the wave's first row of the round
            const int64_t j = j0 + lane;
            uint32_t rmask = 0;
            if (j < n) {
              const KsimRow r = ksim_load_row(c, j);
              bool listed = true;
              if constexpr (ABS) listed = r.count >= 0;  // not listed: not evaluated
              if (listed) {
                SwgAcc acc{c, true, true, true, 0, 0};
                if (P.flags & (KSIM_POD_NEED_SELECTOR | KSIM_POD_NEED_TAINTS)) {
                  const int64_t cl = P.cls;
                  if (P.flags & KSIM_POD_NEED_SELECTOR) acc.sel = ksim_bit(c.sel_ok, cl, c.lwords, c.label_set[j]);
                  if (P.flags & KSIM_POD_NEED_TAINTS) {
                    const int32_t ts = c.taint_set[j];
                    acc.tok = ksim_bit(c.taint_ok, cl, c.twords, ts);
                    acc.nok = ksim_bit(c.noexec_ok, cl, c.twords, ts);
                  }
                }
                rmask = ksim_predicates_a<SwgAcc, true, true>(c, P, j, r, acc);
              }
            }
            why_add(rmask, lane, s_hist);
          }
          __syncthreads();
          why_store(a.why, s, nfail, p, tid, s_hist);
        }
        ++nfail;
      }
      __syncthreads();  // s_red (and s_hist) are rewritten by the next pod
      continue;
    }
    if constexpr (SPR) {
      if (two()) {  // ---- 1b. the spread score of the thread's own fit rows, then (M, C) or the class maxima ----
        // (IPA: and / or their InterPodAffinityPriority score, from the workgroup's min / max raw sum)
        const bool spread = !IPA || sp >= 0;
        const int64_t max_node = spread ? (int64_t)ksimw::max_i32(in ? s_red[lane][1] : 0) : 0;
        const bool have_zones = spread && ksimw::max_i32(in ? s_red[lane][2] : 0) != 0;
        unsigned long long zm = 0;  // every wave: the maximum over all zone words (zones without a fit node hold 0)
        if (spread)
          for (int z = lane; z < nz; z += 64) zm = zw[z] > zm ? zw[z] : zm;
        const int64_t max_zone = spread ? ksimw::max_i64((int64_t)zm) : 0;
        const int32_t wsp = (int32_t)c.w[KSIM_W_SELECTOR_SPREAD];
        int64_t imn = 0, imx = 0;
        int32_t wip = 0;
        if constexpr (IPA) {
          if (ipa) {
            imn = ksimw::min_i64(in ? swg_ipa_lds().mm[lane][0] : 0);
            imx = ksimw::max_i64(in ? swg_ipa_lds().mm[lane][1] : 0);
            wip = (int32_t)c.w[KSIM_W_INTERPOD_AFFINITY];
          }
        }
        mx = -1;
        cm = 0;
        for (int64_t j = tid; j < n; j += SB) {
          const uint32_t wd = sg[j];
          if (wd == GNOFIT) continue;
          const int32_t zj = (spread && zrow) ? zrow[j] : -1;
          const int64_t zs = zj >= 0 ? (int64_t)zw[zj] : 0;
          // < 2^27 with the map score (host-checked weights)
          int32_t e = (int32_t)(wd >> 4);
          if (spread) e += wsp * (int32_t)ksim_spread_score(scnt[j], max_node, have_zones, zj, zs, max_zone);
          if constexpr (IPA) {
            if (ipa) e += wip * (int32_t)ksim_interpod_score(rawc[j], imn, imx);
          }
          const uint32_t q = wd & 15u;
          sg[j] = ((uint32_t)e << 4) | q;
          if (K > 1) {
            if (e > __hip_atomic_load(&s_M[pb][q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) atomicMax(&s_M[pb][q], e);
          } else {
            cm = e > mx ? 1 : cm + (e == mx ? 1 : 0);
            mx = e > mx ? e : mx;
          }
        }
        int32_t (*red)[2] = swg_spread_lds().red;
        if (K == 1) {
          const int32_t Mw = ksimw::max_i32(mx);
          const int32_t Cw = ksimw::sum_i32((mx == Mw && mx >= 0) ? cm : 0);
          if (lane == 0) { red[wv][0] = Mw; red[wv][1] = Cw; }
        }
        __syncthreads();
        if (K == 1) {
          const int32_t mw2 = in ? red[lane][0] : -1;
          M = ksimw::max_i32(mw2);
          C = ksimw::sum_i32((in && mw2 == M && M >= 0) ? red[lane][1] : 0);
        }
      }
    }
    uint32_t win = 1u;
    if (K > 1) {
      // nodes at their class's maximum, per class
      for (int64_t k = 0; k < KS; ++k) {
        const int64_t j = seg0 + k;
        const uint32_t wd = j < seg1 ? sg[j] : GNOFIT;
        const uint32_t q = wd & 15u;
        const bool cand = wd != GNOFIT && (int32_t)(wd >> 4) == s_M[pb][q];
        uint64_t m = __ballot(cand);
        while (m) {  // uniform: one step per class present among the wave's candidates
          const int l = __builtin_ctzll(m);
          const uint32_t ql = (uint32_t)__builtin_amdgcn_readlane((int)q, l);
          const uint64_t same = __ballot(cand && q == ql);
          if (lane == l) atomicAdd(&s_C[pb][ql], (int32_t)__popcll(same));
          m &= ~same;
        }
      }
      __syncthreads();
      // ---- 3. the winning classes (every wave decides; lane = class) ----
      const int lq = lane & (KSIM_MAX_RCLASS - 1);
      const int32_t Cq = s_C[pb][lq];
      const bool live = lane < K && Cq > 0;
      uint64_t wb;
      int64_t best;
      C = ksim_decide_lanes<KsimReduceWave>(c, live, (int64_t)s_M[pb][lq], live ? Cq : 0, tv, av, ad, wb, best);
      win = (uint32_t)wb;
    }
    const uint32_t ix = (F > 1) ? (uint32_t)ksim_select_ix(counter, (uint32_t)C) : 0u;
    counter += (F > 1) ? 1 : 0;  // generic_scheduler.go:192-195 (selectHost only when F > 1)
    // ---- 4. the ix-th node at the best total from the top ----
    const uint32_t one_word = (uint32_t)M << 4;
    auto at_best = [&](uint32_t wd) -> bool {
      if (K == 1) return wd == one_word;
      return wd != GNOFIT && ((win >> (wd & 15u)) & 1u) && (int32_t)(wd >> 4) == s_M[pb][wd & 15u];
    };
    int32_t c_t = 0;
    for (int64_t j = seg0; j < seg1; ++j) c_t += at_best(sg[j]) ? 1 : 0;
    const int32_t pre = ksimw::prefix_incl_i32(c_t);  // within the wave
    if (lane == 63) s_wtot[wv] = pre;
    __syncthreads();
    int32_t below = 0;  // matches in lower waves
    for (int w = 0; w < SW; ++w) below += (w < wv) ? s_wtot[w] : 0;
    const uint32_t above = (uint32_t)(C - (below + pre));  // matches in higher threads
    if (c_t > 0 && ix >= above && ix < above + (uint32_t)c_t) {
      int32_t r = (int32_t)(ix - above);
      int64_t jsel = -1;
      for (int64_t j = seg1 - 1; j >= seg0; --j) {
        if (at_best(sg[j])) {
          if (r == 0) { jsel = j; break; }
          --r;
        }
      }
      if (jsel >= 0) ksim_commit(c, P, jsel);
      if constexpr (SPR) {  // NodeInfo.AddPod on the scenario's counts: every pod with an identity
        if (jsel >= 0) ksim_aff_commit_body(*Ap, P, jsel, +1);
      }
      if constexpr (VOL) {  // ... and on the scenario's mounts: every pod with a volume class
        if (jsel >= 0 && ksim_is_vol_pod(c, P)) ksim_vol_commit_body(*c.vol, P, jsel, +1, c.err);
      }
      *answer_of(p) = (int32_t)jsel;
    }
    __syncthreads();  // the commit (workgroup release/acquire) before the next pod's loads
  }
  if (tid == 0) a.out_counter[s] = counter;
}


// The kernel arguments of an instantiation from the launch description: Args = SwgArgsSpr takes the
// chunk's spread descriptors beside the queue's arguments, SwgArgsIpa the raw column as well.  (The plain
// instantiations take *L.args itself: a kernel keeps the base part of what it is passed.)
template <class Args>
static Args swg_args(const SwgLaunch& L) {
  Args a{};
  (SwgArgsPre&)a = *L.args;
  a.aff = L.spr->aff;
  if constexpr (std::is_same_v<Args, SwgArgsIpa>) a.raw = L.ipa->raw;
  return a;
}
