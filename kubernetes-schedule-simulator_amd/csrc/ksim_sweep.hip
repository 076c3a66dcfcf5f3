// ksim_sweep.hip — scenario sweep (BASELINE.json configs[4], SURVEY.md §8e "C5"): S independent
// copies of one cluster snapshot, each scheduling the same resource-only pod queue under its own
// map-priority weights — the capacity-planning what-if the reference answers by running the
// simulator once per policy (pkg/scheduler/simulator.go:286 New + :187 Run per
// --algorithmprovider / policy file).
//
// One 1024-thread workgroup per scenario; no cross-workgroup communication.  Per pod:
//   1. every thread evaluates rows j = tid, tid+1024, ... (coalesced), streaming the scenario's
//      dynamic columns (requested / non-zero requested cpu+mem as float64, pod count) from HBM
//      and the shared static columns (alloc, RN(1/alloc), allowed pods, flags) from L2; the
//      packed evaluation goes to LDS (uint16, 0xFFFF = does not fit);
//   2. block reduction → fit count F, max score M, count at max C (findNodesThatFit +
//      PrioritizeNodes, core/generic_scheduler.go:112-167);
//   3. selectHost (:183-198): ix = lastNodeIndex % C (no increment for a single fit node,
//      :153-156), the ix-th max-score row counted from the top of the name order, found by a
//      block prefix over contiguous LDS segments;
//   4. the owning thread commits (NodeInfo.AddPod, schedulercache/node_info.go:318-341) into the
//      scenario's columns; the barrier's workgroup fence makes it visible to the next pod.
// The node table streams from HBM every pod: the HBM-bandwidth-bound form of the scan.
//
// Node sets per scenario (ksim_sweep_nodes): once the scenario's columns are initialised, the sign
// bit of its pod-count entry is set for every node the scenario does not list, and the ABS
// instantiation of the scan maps a negative count to "does not fit".  Such a row is NOFIT in
// LDS, so F, M, C and the select prefix run over the listed nodes only, and a commit, which
// lands on a fit row, never touches the bit.  Without a node set the ABS = false instantiation
// runs.
//
// The general form (ksim_sweep_general_kernel, below the scan): the same shape for pods that are
// not resource-only.  Every column a commit writes is the scenario's own, the evaluation is the
// exact int64 one of the scheduling kernels (ksim_predicates_a, ksim_map_score, ksim_rclass_a), LDS
// holds (map score << 4) | reduce class per node, and the pod's end is ksim_decide_lanes over the
// per-class (max, count at max) of the workgroup.
//
// Explained sweeps (ksim_sweep_explain, include/ksim_whatif.h): the WHY instantiations of both
// kernels keep, per scenario, the first cap failed pods with their FitError histogram.  A pod that
// fits nowhere is evaluated once more for its reason masks — the packed evaluations in LDS have no
// room for them — and the masks of the listed nodes are counted per reason.  The WHY = false
// instantiations are the kernels as they were, kernel arguments included.
//
// The kernel templates and what they use are ksim_sweep_kernels.h's, shared with ksim_sweep_vol.hip; this
// unit holds the init, context, node-set and pod kernels and the two launchers, and instantiates every
// sweep kernel but the VOL ones.
#include "ksim_sweep_kernels.h"

// Scenario s of the chunk gets its context: k (the handle's, its dynamic columns at the chunk's
// first copy, err at the sweep's own word) rebased to the scenario's copies, nothing of the per-pod,
// affinity, volume or sharded forms, and the scenario's map weights when weights are given.
__global__ void ksim_sweep_general_ctx_kernel(const KsimCtx k, const int64_t* w, int32_t scen0, int32_t n_scen,
                                              KsimCtx* out) {
  const int32_t s = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
  if (s >= n_scen) return;
  KsimCtx& c = out[s];
  c = k;
  const int64_t off = (int64_t)s * k.n;
  c.req_cpu = k.req_cpu + off; c.req_mem = k.req_mem + off; c.req_gpu = k.req_gpu + off; c.req_eph = k.req_eph + off;
  c.nz_cpu = k.nz_cpu + off; c.nz_mem = k.nz_mem + off;
  c.pod_count = k.pod_count + off; c.port_count = k.port_count + off; c.flags = k.flags + off;
  c.req_scalar = k.req_scalar + off * k.n_scalar;
  c.ports = k.ports + off * k.port_slots;
  c.one = 0; c.aff = nullptr; c.vol = nullptr; c.collect = 0; c.no_commit = 0; c.sh_world = 0;
  if (w) {
    const int64_t* ws = w + 3 * (int64_t)(scen0 + s);
    c.w[KSIM_W_LEAST_REQUESTED] = ws[0];
    c.w[KSIM_W_MOST_REQUESTED] = ws[1];
    c.w[KSIM_W_BALANCED] = ws[2];
  }
}

// every scenario's copy of the columns a commit writes, from the handle's current node state
__global__ void ksim_sweep_general_init_kernel(SwgCols src, SwgCols d, int64_t n, int32_t n_scalar, int32_t port_slots,
                                               int64_t total) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= total) return;
  const int64_t i = k % n, s = k / n;
  d.req_cpu[k] = src.req_cpu[i]; d.req_mem[k] = src.req_mem[i]; d.req_gpu[k] = src.req_gpu[i];
  d.req_eph[k] = src.req_eph[i]; d.nz_cpu[k] = src.nz_cpu[i]; d.nz_mem[k] = src.nz_mem[i];
  d.pod_count[k] = src.pod_count[i]; d.port_count[k] = src.port_count[i]; d.flags[k] = src.flags[i];
  for (int32_t t = 0; t < n_scalar; ++t) d.req_scalar[(s * n_scalar + t) * n + i] = src.req_scalar[(int64_t)t * n + i];
  for (int32_t t = 0; t < port_slots; ++t) d.ports[(s * port_slots + t) * n + i] = src.ports[(int64_t)t * n + i];
}

// SPR: every scenario's copy of the counted pairs from the handle's current counts, and its tables:
// the handle's descriptor with cnt at the copy (nothing else of it is written by the sweep)
__global__ void ksim_sweep_spread_init_kernel(const KsimAff base, int32_t* cnt, int64_t cnt_len, int64_t total,
                                              int32_t n_scen, KsimAff* out) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < total) cnt[k] = base.cnt[k % cnt_len];
  if (k < n_scen) {
    KsimAff& A = out[k];
    A = base;
    A.cnt = cnt + k * cnt_len;
  }
}

// IPA: every scenario's copy of the carried terms from the handle's current ones; its descriptor (the
// spread init kernel's, earlier on the stream) gets carried at the copy, its context (the context
// kernel's) the descriptor
__global__ void ksim_sweep_affinity_init_kernel(const int64_t* carried0, int64_t* carried, int64_t carried_len, int64_t total,
                                                int32_t n_scen, KsimAff* aff, KsimCtx* ctx) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < total) carried[k] = carried0[k % carried_len];
  if (k < n_scen) {
    aff[k].carried = carried + k * carried_len;
    ctx[k].aff = aff + k;
  }
}

// VOL: every scenario's copy of the mount words and slot counts from the handle's current mounts, its
// descriptor (the handle's, both pointers at the copies: the slot stride stays n, the static tables are
// shared) and, after the context kernel on the stream, its context's vol
__global__ void ksim_sweep_volume_init_kernel(const KsimVol base, uint64_t* slots, int32_t* slot_count, int64_t slot_words,
                                              int32_t n_scen, KsimVol* out, KsimCtx* ctx) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < slot_words * n_scen) slots[k] = base.slots[k % slot_words];
  if (k < base.n * n_scen) slot_count[k] = base.slot_count[k % base.n];
  if (k < n_scen) {
    KsimVol& V = out[k];
    V = base;
    V.slots = slots + k * slot_words;
    V.slot_count = slot_count + k * base.n;
    ctx[k].vol = out + k;
  }
}

// IPA, after the copies: thread (scenario, resident) takes the resident's contribution out of the
// scenario's counts and carried terms when its node is absent there (NodeInfo.RemovePod of a pod that
// the reference never sees).  Node, identity and class are host-checked against the loaded tables.
__global__ void ksim_sweep_affinity_correct_kernel(const KsimAff* aff, const SwgResidents res, const uint32_t* absent,
                                                   int32_t words, int64_t total) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= total) return;
  const int64_t s = k / res.n, r = k % res.n;
  const int32_t i = res.node[r];
  if (!((absent[s * words + (i >> 5)] >> (i & 31)) & 1u)) return;
  ksim_pod P{};
  P.aff_ident = res.aff_ident[r];
  P.aff_class = res.aff_class[r];
  ksim_aff_commit_body(aff[s], P, i, -1);
}

// IPA, after the correction: a negative count means the residents are not the pods behind the
// handle's counts -> the sweep's error word, and the lowest such scenario of the whole sweep
__global__ void ksim_sweep_affinity_check_kernel(const int32_t* cnt, int64_t cnt_len, int64_t total, int32_t scen0,
                                                 int32_t* err, int32_t* bad) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= total || cnt[k] >= 0) return;
  atomicOr(err, KSIM_SWEEP_ERR_COUNTS);
  atomicMin(bad, scen0 + (int32_t)(k / cnt_len));
}

// static float64 columns, once per handle
__global__ void ksim_sweep_static_kernel(const int64_t* ac, const int64_t* am, int64_t n, double* dac, double* dam,
                                         double* yc, double* ym) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double c = (double)ac[i], m = (double)am[i];
  dac[i] = c; dam[i] = m;
  yc[i] = c != 0.0 ? 1.0 / c : 0.0;
  ym[i] = m != 0.0 ? 1.0 / m : 0.0;
}

// every scenario's dynamic columns from the handle's current node state
__global__ void ksim_sweep_init_kernel(const int64_t* rc0, const int64_t* rm0, const int64_t* zc0, const int64_t* zm0,
                                       const int32_t* c0, int64_t n, int64_t total, double* rc, double* rm, double* zc,
                                       double* zm, int32_t* c) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= total) return;
  const int64_t i = k % n;
  rc[k] = (double)rc0[i]; rm[k] = (double)rm0[i]; zc[k] = (double)zc0[i]; zm[k] = (double)zm0[i]; c[k] = c0[i];
}

// node sets: absent holds [scenarios][words] bits, bit (i & 31) of word (i >> 5) set = node i is
// not listed in that scenario -> the sign bit of its pod count in the scenario's column
__global__ void ksim_sweep_absent_kernel(const uint32_t* absent, int32_t words, int64_t n, int64_t total, int32_t* c) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= total) return;
  const int64_t i = k % n;
  if ((absent[(k / n) * words + (i >> 5)] >> (i & 31)) & 1u) c[k] |= INT32_MIN;
}

__global__ void ksim_sweep_pods_kernel(const ksim_pod* pods, int64_t count, FPod* out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) out[i] = load_fpod(pods[i]);
}

// A run-time flag as a compile-time one: f(std::true_type) or f(std::false_type), so that a launcher
// names its kernel once, <decltype(ABS)::value, ...>.  A kernel takes the argument struct of its
// instantiation by value: the launchers pass the fullest one and the call keeps the base part.
template <class F>
static void with_flag(bool on, F&& f) {
  if (on) f(std::true_type{});
  else f(std::false_type{});
}

extern "C" size_t ksim_sweep_fpod_bytes(void) { return sizeof(FPod); }

extern "C" hipError_t ksim_sweep_prepare(const int64_t* ac, const int64_t* am, int64_t n, double* dac, double* dam,
                                         double* yc, double* ym, hipStream_t st) {
  hipLaunchKernelGGL(ksim_sweep_static_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ac, am, n, dac, dam,
                     yc, ym);
  return hipGetLastError();
}

extern "C" hipError_t ksim_sweep_launch(const int64_t* rc0, const int64_t* rm0, const int64_t* zc0, const int64_t* zm0,
                                        const int32_t* c0, const ksim_pod* pods, void* fpods, const SwArgsWhy* args,
                                        int32_t n_scen, const uint32_t* absent, int32_t absent_words, hipEvent_t ev0,
                                        hipEvent_t ev1, hipStream_t st) {
  const int64_t n = args->n, total = n * (int64_t)n_scen;
  hipLaunchKernelGGL(ksim_sweep_init_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, rc0, rm0, zc0, zm0,
                     c0, n, total, args->rc, args->rm, args->zc, args->zm, args->count);
  if (absent)
    hipLaunchKernelGGL(ksim_sweep_absent_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, absent,
                       absent_words, n, total, args->count);
  hipLaunchKernelGGL(ksim_sweep_pods_kernel, dim3((unsigned)((args->n_pods + 255) / 256)), dim3(256), 0, st, pods,
                     (int64_t)args->n_pods, (FPod*)fpods);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (ev0) (void)hipEventRecord(ev0, st);
  const size_t lds = (size_t)n * sizeof(uint16_t);
  const bool why = args->why.cap > 0;  // ksim_sweep_explain keeping records
  with_flag(absent != nullptr, [&](auto ABS) {
    with_flag(why, [&](auto WHY) {
      hipLaunchKernelGGL((ksim_sweep_kernel<decltype(ABS)::value, decltype(WHY)::value>), dim3((unsigned)n_scen),
                         dim3(SB), lds, st, *args);
    });
  });
  e = hipGetLastError();
  if (ev1) (void)hipEventRecord(ev1, st);
  return e;
}

// The VOL instantiations live in a translation unit of their own (ksim_sweep_vol.hip, over the same
// ksim_sweep_kernels.h): instantiating them beside the others changes the code the compiler emits for
// every existing ksim_sweep_general_kernel, and those are kept instruction for instruction.
extern "C" hipError_t ksim_sweep_general_vol_launch(const SwgLaunch* L, size_t lds);
extern "C" hipError_t ksim_sweep_policy_ctx_launch(const int64_t* w, int32_t scen0, int32_t n_scen, KsimCtx* ctx,
                                                   hipStream_t st);

// The general form over one chunk (SwgLaunch, ksim_sweep.h): the init kernels of the state the sweep owns,
// the scenarios' contexts, then the instantiation its feature parts select.
// args->off set: the PRE instantiations (ksim_sweep_drain).
// spr set: the SPR instantiations (a SelectorSpread queue): the handle's affinity descriptor and the
// chunk's count copies and per-scenario descriptors.
// ipa set (with spr): the IPA instantiations (ksim_sweep_affinity): the chunk's carried copies and raw
// columns, the residents, and the word for the scenario whose corrected counts are negative.
// vol set (alone, with spr, or with spr and ipa): the VOL instantiations (ksim_sweep_volumes): the
// handle's volume descriptor and the chunk's mount copies and per-scenario descriptors.
// polw set (ksim_sweep_policy): the weight rows, written over the scenarios' contexts by
// ksim_sweep_policy.hip's kernel behind the context kernel.
extern "C" hipError_t ksim_sweep_general_launch(const SwgLaunch* L) {
  const KsimCtx* hc = L->hc;
  const SwgCols* cols = L->cols;
  const SwgArgsPre* args = L->args;
  const int32_t n_scen = L->n_scen;
  const hipStream_t st = L->st;
  const int64_t n = hc->n, total = n * (int64_t)n_scen;
  if (L->spr) {
    const int64_t ct = L->spr->cnt_len * (int64_t)n_scen, thr = ct > n_scen ? ct : (int64_t)n_scen;
    hipLaunchKernelGGL(ksim_sweep_spread_init_kernel, dim3((unsigned)((thr + 255) / 256)), dim3(256), 0, st, L->spr->base,
                       L->spr->cnt, L->spr->cnt_len, ct, n_scen, L->spr->aff);
  }
  SwgCols src{hc->req_cpu, hc->req_mem, hc->req_gpu, hc->req_eph, hc->nz_cpu, hc->nz_mem,
              hc->req_scalar, hc->ports, hc->pod_count, hc->port_count, hc->flags};
  hipLaunchKernelGGL(ksim_sweep_general_init_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, src, *cols, n,
                     hc->n_scalar, hc->port_slots, total);
  if (L->absent)
    hipLaunchKernelGGL(ksim_sweep_absent_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, L->absent,
                       L->absent_words, n, total, cols->pod_count);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (L->ev0) (void)hipEventRecord(L->ev0, st);
  KsimCtx k = *hc;
  k.req_cpu = cols->req_cpu; k.req_mem = cols->req_mem; k.req_gpu = cols->req_gpu; k.req_eph = cols->req_eph;
  k.nz_cpu = cols->nz_cpu; k.nz_mem = cols->nz_mem; k.req_scalar = cols->req_scalar; k.ports = cols->ports;
  k.pod_count = cols->pod_count; k.port_count = cols->port_count; k.flags = cols->flags;
  k.err = L->err;
  hipLaunchKernelGGL(ksim_sweep_general_ctx_kernel, dim3((unsigned)((n_scen + 63) / 64)), dim3(64), 0, st, k, args->w,
                     args->scen0, n_scen, args->ctx);
  if (L->polw) {
    e = ksim_sweep_policy_ctx_launch(L->polw, args->scen0, n_scen, args->ctx, st);
    if (e != hipSuccess) return e;
  }
  if (L->ipa) {
    const int64_t ct = L->ipa->carried_len * (int64_t)n_scen, thr = ct > n_scen ? ct : (int64_t)n_scen;
    hipLaunchKernelGGL(ksim_sweep_affinity_init_kernel, dim3((unsigned)((thr + 255) / 256)), dim3(256), 0, st,
                       L->spr->base.carried, L->ipa->carried, L->ipa->carried_len, ct, n_scen, L->spr->aff, args->ctx);
    if (L->absent && L->ipa->res.n > 0) {
      const int64_t rt = L->ipa->res.n * (int64_t)n_scen, kt = L->spr->cnt_len * (int64_t)n_scen;
      hipLaunchKernelGGL(ksim_sweep_affinity_correct_kernel, dim3((unsigned)((rt + 255) / 256)), dim3(256), 0, st, L->spr->aff,
                         L->ipa->res, L->absent, L->absent_words, rt);
      hipLaunchKernelGGL(ksim_sweep_affinity_check_kernel, dim3((unsigned)((kt + 255) / 256)), dim3(256), 0, st, L->spr->cnt,
                         L->spr->cnt_len, kt, args->scen0, L->err, L->ipa->bad);
    }
  }
  if (L->vol) {
    const int64_t sw = (int64_t)L->vol->base.vol_slots * n, mt = (sw > n ? sw : n) * n_scen;
    hipLaunchKernelGGL(ksim_sweep_volume_init_kernel, dim3((unsigned)((mt + 255) / 256)), dim3(256), 0, st, L->vol->base,
                       L->vol->slots, L->vol->slot_count, sw, n_scen, L->vol->vol, args->ctx);
  }
  const size_t lds = (size_t)n * sizeof(uint32_t);
  const bool why = args->why.cap > 0;  // ksim_sweep_explain keeping records
  const KsimCtx* ctx = args->ctx;
  const dim3 grid((unsigned)n_scen), block(SB);
  if (L->vol) {  // the VOL instantiations (ksim_sweep_vol.hip)
    e = ksim_sweep_general_vol_launch(L, lds);
    if (L->ev1) (void)hipEventRecord(L->ev1, st);
    return e;
  }
  with_flag(args->off != nullptr, [&](auto pre) {
    constexpr bool PRE = decltype(pre)::value;
    if (L->ipa) {  // as the SPR ones: ABS and WHY on
      hipLaunchKernelGGL((ksim_sweep_general_kernel<true, true, PRE, true, true>), grid, block, lds, st, ctx,
                         swg_args<SwgArgsIpa>(*L));
      return;
    }
    if (L->spr) {
      // two instantiations, with and without prefix queues: ABS and WHY are on in both (without node
      // sets no count is negative, without records why.cap is 0: the same answers)
      hipLaunchKernelGGL((ksim_sweep_general_kernel<true, true, PRE, true>), grid, block, lds, st, ctx,
                         swg_args<SwgArgsSpr>(*L));
      return;
    }
    with_flag(L->absent != nullptr, [&](auto ABS) {
      with_flag(why, [&](auto WHY) {
        hipLaunchKernelGGL((ksim_sweep_general_kernel<decltype(ABS)::value, decltype(WHY)::value, PRE>), grid, block,
                           lds, st, ctx, *args);
      });
    });
  });
  e = hipGetLastError();
  if (L->ev1) (void)hipEventRecord(L->ev1, st);
  return e;
}
