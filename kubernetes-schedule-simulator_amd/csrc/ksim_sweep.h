// ksim_sweep.h — kernel arguments of the scenario-sweep kernel (ksim_sweep.hip), shared with
// the host runtime.
#pragma once
#include "ksim_f64.h"

// Explained sweeps (ksim_sweep_explain, the WHY instantiations): scenario s of a chunk keeps the
// first cap failed pods of its queue, record k = (pod[s][k], hist[s][k][KSIM_NREASONS]).  Only the
// WHY instantiations take it (SwArgsWhy, SwgArgsWhy): the others keep their kernel arguments.
struct SwWhy {
  int32_t cap;
  int32_t* pod;   // [C][cap] index of the k-th failed pod, relative to the range's first
  int32_t* hist;  // [C][cap][KSIM_NREASONS] its FitError histogram
};

struct SwArgs {
  int64_t n;
  int32_t n_pods, scen0;
  const double* dac;  // static columns [n]
  const double* dam;
  const double* yc;
  const double* ym;
  const int32_t* allowed;
  const uint32_t* flags;
  double* rc;         // dynamic columns [S][n]
  double* rm;
  double* zc;
  double* zm;
  int32_t* count;
  const kf64::FPod* pods;  // [n_pods]
  const int32_t* w;        // [S][3]: LeastRequested, MostRequested, BalancedResourceAllocation
  uint32_t preds;
  int32_t no_prio;
  uint64_t counter0;
  int32_t* out_node;      // [S][n_pods]
  uint64_t* out_counter;  // [S]
};
struct SwArgsWhy : SwArgs {
  SwWhy why;  // cap == 0: an unexplained launch, of the WHY = false instantiation on the SwArgs part
};

#define KSIM_SWEEP_MAX_NODES 76800  // uint16 evaluations of one scenario in LDS (150 KiB)

// The general form (ksim_sweep_general_kernel): pods the resource-only forms do not take (host
// ports, selectors, tolerations, nodeName, gpu / ephemeral / extended requests), evaluated in exact
// int64 by the shared device code.  Scenario s of a chunk owns the s-th [n] slice of every column
// a commit writes (SwgCols; [n_scalar][n] / [port_slots][n] of the scalar / port columns) and a
// KsimCtx of its own: the handle's with those columns rebased and err at the sweep's own error word.
struct SwgCols {
  int64_t *req_cpu, *req_mem, *req_gpu, *req_eph, *nz_cpu, *nz_mem;
  int64_t* req_scalar;
  uint64_t* ports;
  int32_t *pod_count, *port_count;
  uint32_t* flags;
};

struct SwgArgs {
  int32_t n_pods, scen0;
  int64_t first;          // first pod of the range in KsimCtx::pods
  const int64_t* w;       // [S][3] LeastRequested, MostRequested, BalancedResourceAllocation; null: the handle's own
  uint64_t counter0;
  KsimCtx* ctx;           // [C] the scenarios' contexts
  int32_t* out_node;      // [C][n_pods]
  uint64_t* out_counter;  // [C]
};
struct SwgArgsWhy : SwgArgs {
  SwWhy why;
};
// Drain sweeps (ksim_sweep_drain, include/ksim_drain.h, the PRE instantiations): scenario s (of the
// whole sweep: scen0 + the workgroup) schedules pods pod[off[s] .. off[s + 1]) of KsimCtx::pods before
// the range, the answers parallel to pod in out_pre.  A record of why then holds the pod's position
// in the scenario's own queue (prefix first), and cap counts over that queue.
struct SwgArgsPre : SwgArgsWhy {
  const int64_t* off;  // [S + 1]
  const int64_t* pod;  // [off[S]]
  int32_t* out_pre;    // [off[S]]
};

// SelectorSpread queues (the SPR instantiations): a range or prefix pod with SelectorSpread state,
// on tables that hold nothing else.  Scenario s of a chunk owns the s-th [cnt_len] copy of the
// counted-pair array (made from the handle's current counts, so a schedule() of a prefix is carried)
// and a KsimAff of its own with cnt rebased to it; aff[s] is read beside the scenario's KsimCtx, whose
// aff stays null for the predicates (with spread-only tables MatchInterPodAffinity is vacuous).
struct SwgArgsSpr : SwgArgsPre {
  const KsimAff* aff;  // [C] the scenarios' tables; off == null: no prefix queues
};
// What the launcher needs for them: the handle's tables, the chunk's count copies and descriptors.
struct SwgSpread {
  KsimAff base;     // the handle's descriptor (host copy)
  int32_t* cnt;     // [C][cnt_len]
  int64_t cnt_len;
  KsimAff* aff;     // [C]
};

// Inter-pod affinity queues (ksim_sweep_affinity, include/ksim_affsweep.h, the IPA instantiations on
// top of SPR): the tables hold required, preferred or carried terms.  Scenario s of a chunk also owns
// the s-th [carried_len] copy of the carried-term array (its KsimAff's carried rebased to it), its
// KsimCtx::aff points at its own KsimAff (MatchInterPodAffinity in the shared predicate chain), and
// raw is its [n] column of InterPodAffinityPriority's sums between steps 1 and 1b of a pod.  Both
// copies are the handle's arrays minus the contribution of every resident (the placed pods behind
// the handle's counts) whose node the scenario does not list: a zone- or cluster-keyed domain counts
// pods on absent nodes, and the reference removes those pods with their nodes.
struct SwgArgsIpa : SwgArgsSpr {
  int64_t* raw;  // [C][n]
};
struct SwgResidents {
  int64_t n;
  const int32_t* node;       // [n] name rank
  const int32_t* aff_ident;  // [n] as ksim_pod.aff_ident
  const int32_t* aff_class;  // [n] as ksim_pod.aff_class
};
struct SwgAffinity {
  int64_t* carried;  // [C][carried_len]
  int64_t carried_len;
  int64_t* raw;      // [C][n]
  SwgResidents res;  // device arrays (n == 0: nothing to correct)
  int32_t* bad;      // the lowest scenario of the sweep with a negative count after the correction
};
#define KSIM_SWEEP_ERR_COUNTS 256  // the sweep's own error word: a scenario's corrected count is negative

// Volume queues (ksim_sweep_volumes, include/ksim_volsweep.h, the VOL instantiations beside the plain,
// SPR and IPA ones): a range or prefix pod may mount volumes.  Scenario s of a chunk owns the s-th
// [vol_slots][n] copy of the mount words (the slot stride stays n), the s-th [n] copy of the slot
// counts and a KsimVol of its own: the handle's with both pointers rebased, the static tables
// (key_filter, vc, vc_filter, refs, zone_ok) shared.  Its KsimCtx::vol points at that descriptor, so
// the shared predicate chain evaluates NoDiskConflict, the MaxPD filters and NoVolumeZoneConflict over
// the scenario's mounts, and the commit writes them.  Mounts are per node and an absent node is never
// evaluated: no correction.  The kernels take no argument of their own for it.
struct SwgVolumes {
  KsimVol base;         // the handle's descriptor (host copy)
  uint64_t* slots;      // [C][vol_slots][n]
  int32_t* slot_count;  // [C][n]
  KsimVol* vol;         // [C]
};

// One launch of the general form over a chunk, as ksim_sweep_general_launch takes it.  The feature parts
// say which per-scenario state the sweep owns, and so which init kernels run and which instantiation
// is launched: a null part = no such state.  ipa needs spr; vol goes with either, both or neither.
struct SwgLaunch {
  const KsimCtx* hc;       // the handle's context
  const SwgCols* cols;     // the chunk's scenario columns
  const SwgArgsPre* args;  // off set: the PRE instantiations; off / pod / out_pre indexed by scen0 + the chunk's scenario
  const SwgSpread* spr;    // SelectorSpread state: the count copies and descriptors (the SPR instantiations)
  const SwgAffinity* ipa;  // inter-pod affinity terms: carried copies, raw columns, residents (the IPA instantiations)
  const SwgVolumes* vol;   // mounts: the mount copies and descriptors (the VOL instantiations)
  const int64_t* polw;     // ksim_sweep_policy: the whole sweep's [S][KSIM_NW] weight rows (args->w is then null)
  int32_t n_scen;          // scenarios of the chunk
  const uint32_t* absent;  // [n_scen][absent_words] the chunk's node sets, or null
  int32_t absent_words;
  int32_t* err;            // the sweep's own error word (the handle's is never written)
  hipEvent_t ev0, ev1;     // recorded before and behind the sweep kernel (may be null)
  hipStream_t st;
};

// Policy sweeps (ksim_sweep_policy, include/ksim_polsweep.h, ksim_sweep_policy.hip): no instantiation
// of their own.  The sweep kernels read all seven weights from the scenario's KsimCtx, so a policy
// scenario is the handle's context with its whole weight row written over it
// (ksim_sweep_policy_ctx_kernel, after the context kernel), under whichever plain, SPR, IPA or VOL
// kernel the queue takes.  A scenario's outcome record on the device: listed, used, free_cpu[11],
// free_mem[11] (ksim_sweep_outcome_kernel).
#define KSIM_SWEEP_OUTCOME_WORDS 24

// one uint32 evaluation per node in LDS, (map score << 4) | reduce class (150 KiB)
#define KSIM_SWEEP_GENERAL_MAX_NODES 38400
#define KSIM_SWEEP_GENERAL_SCORE_BITS 27  // 0xFFFFFFFF = does not fit stays above every packed word
// countsByZone of the current and the next pod as 64-bit LDS words (2 x 512 x 8 B = 8 KiB beside the
// 150 KiB of evaluations and the 1 KiB of reduction words, within the 160 KiB of a workgroup).  A word
// sums int32 counts over at most KSIM_SWEEP_GENERAL_MAX_NODES nodes: below 2^47, no overflow.
#define KSIM_SWEEP_SPREAD_MAX_ZONES 512
static_assert(KSIM_SWEEP_GENERAL_MAX_NODES * 4 + 2 * KSIM_SWEEP_SPREAD_MAX_ZONES * 8 + 1024 <= 160 * 1024,
              "evaluations + zone words + reduction words exceed a workgroup's LDS");
static_assert(KSIM_MAX_RCLASS <= 16, "the reduce class takes the low four bits of a packed evaluation");
static_assert(sizeof(KsimCtx) + sizeof(SwgArgsWhy) <= 4096 - 64, "KsimCtx + SwgArgs exceed the kernel-argument limit");
static_assert(sizeof(KsimCtx) + sizeof(SwgArgsPre) <= 4096 - 64, "KsimCtx + SwgArgsPre exceed the kernel-argument limit");
static_assert(sizeof(KsimCtx) + sizeof(SwgArgsSpr) <= 4096 - 64, "KsimCtx + SwgArgsSpr exceed the kernel-argument limit");
static_assert(sizeof(KsimCtx) + sizeof(SwgArgsIpa) <= 4096 - 64, "KsimCtx + SwgArgsIpa exceed the kernel-argument limit");
