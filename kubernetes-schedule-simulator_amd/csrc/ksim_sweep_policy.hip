// ksim_sweep_policy.hip — the kernels of ksim_sweep_policy (include/ksim_polsweep.h) that are not the
// sweep itself: a scenario's whole weight row into its context, and its outcome record from its final
// node state.  The sweep kernels stay ksim_sweep.hip's and ksim_sweep_vol.hip's, which this unit neither
// includes nor instantiates, so their code is what it was.
#include "ksim_common.h"
#include "ksim_sweep.h"
#include "ksim_wave.h"

#include "../../include/ksim_polsweep.h"

static_assert(KSIM_SWEEP_OUTCOME_WORDS == 2 + 2 * KSIM_OUTCOME_BUCKETS, "listed, used and the two histograms");

namespace {

constexpr int OB = 256;  // outcome kernel: threads of a workgroup

// Scenario s of the chunk: all KSIM_NW weights of row scen0 + s over the context that
// ksim_sweep_general_ctx_kernel wrote earlier on the stream (the handle's, rebased).  The sweep kernel
// reads every weight from that context, so this is all a policy scenario needs.
__global__ void ksim_sweep_policy_ctx_kernel(const int64_t* __restrict__ w, int32_t scen0, int32_t n_scen,
                                             KsimCtx* __restrict__ ctx) {
  const int32_t s = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
  if (s >= n_scen) return;
  const int64_t* ws = w + (int64_t)KSIM_NW * (scen0 + s);
  for (int k = 0; k < KSIM_NW; ++k) ctx[s].w[k] = ws[k];
}

// One workgroup per scenario, after its sweep: the record of include/ksim_polsweep.h over the nodes the
// scenario lists (pod_count >= 0: the sign bit marks an absent node), from the scenario's own columns.
// A thread classifies its rows, a wave sums each of the 24 words (2 + 2 x 11) with a DPP reduction and
// adds it to the workgroup's LDS words; the first 24 threads store the record.  One launch per chunk,
// no word shared between workgroups.
__global__ __launch_bounds__(OB) void ksim_sweep_outcome_kernel(const KsimCtx* __restrict__ ctxs, int32_t* __restrict__ out) {
  __shared__ int32_t s_rec[KSIM_SWEEP_OUTCOME_WORDS];
  const int tid = threadIdx.x, lane = tid & 63;
  const KsimCtx& c = ctxs[blockIdx.x];
  const int64_t n = c.n;
  if (tid < KSIM_SWEEP_OUTCOME_WORDS) s_rec[tid] = 0;
  __syncthreads();
  // the thread's rows: bucket b of cpu in hc[b], of memory in hm[b] (registers: every index is a constant
  // once the loops are unrolled)
  int32_t listed = 0, used = 0;
  int32_t hc[KSIM_OUTCOME_BUCKETS], hm[KSIM_OUTCOME_BUCKETS];
#pragma unroll
  for (int b = 0; b < KSIM_OUTCOME_BUCKETS; ++b) hc[b] = hm[b] = 0;
  for (int64_t j = tid; j < n; j += OB) {
    const int32_t cnt = c.pod_count[j];
    if (cnt < 0) continue;  // not listed
    listed += 1;
    used += cnt > 0 ? 1 : 0;
    const int32_t fc = (int32_t)ksim_least(c.nz_cpu[j], c.alloc_cpu[j]);  // 0..10
    const int32_t fm = (int32_t)ksim_least(c.nz_mem[j], c.alloc_mem[j]);
#pragma unroll
    for (int b = 0; b < KSIM_OUTCOME_BUCKETS; ++b) {
      hc[b] += fc == b ? 1 : 0;
      hm[b] += fm == b ? 1 : 0;
    }
  }
  const int32_t L = ksimw::sum_i32(listed), U = ksimw::sum_i32(used);
  if (lane == 0) {
    atomicAdd(&s_rec[0], L);
    atomicAdd(&s_rec[1], U);
  }
#pragma unroll
  for (int b = 0; b < KSIM_OUTCOME_BUCKETS; ++b) {
    const int32_t C = ksimw::sum_i32(hc[b]), M = ksimw::sum_i32(hm[b]);
    if (lane == 0) {
      atomicAdd(&s_rec[2 + b], C);
      atomicAdd(&s_rec[2 + KSIM_OUTCOME_BUCKETS + b], M);
    }
  }
  __syncthreads();
  if (tid < KSIM_SWEEP_OUTCOME_WORDS) out[(int64_t)blockIdx.x * KSIM_SWEEP_OUTCOME_WORDS + tid] = s_rec[tid];
}

}  // namespace

// After ksim_sweep_general_ctx_kernel on st: rows scen0 .. scen0 + n_scen of w into ctx[0 .. n_scen).
extern "C" hipError_t ksim_sweep_policy_ctx_launch(const int64_t* w, int32_t scen0, int32_t n_scen, KsimCtx* ctx,
                                                   hipStream_t st) {
  hipLaunchKernelGGL(ksim_sweep_policy_ctx_kernel, dim3((unsigned)((n_scen + 63) / 64)), dim3(64), 0, st, w, scen0, n_scen,
                     ctx);
  return hipGetLastError();
}

// After the chunk's sweep kernel on st: out[n_scen][KSIM_SWEEP_OUTCOME_WORDS]; ev1 (may be null) is
// recorded again behind it, so that the chunk's device time covers it.
extern "C" hipError_t ksim_sweep_outcome_launch(const KsimCtx* ctx, int32_t n_scen, int32_t* out, hipEvent_t ev1,
                                                hipStream_t st) {
  hipLaunchKernelGGL(ksim_sweep_outcome_kernel, dim3((unsigned)n_scen), dim3(OB), 0, st, ctx, out);
  const hipError_t e = hipGetLastError();
  if (ev1) (void)hipEventRecord(ev1, st);
  return e;
}
