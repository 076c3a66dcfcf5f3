/* ksim_polsweep.h — policy what-ifs under the whole provider.  ksim_sweep and ksim_sweep_nodes
 * (include/ksim.h, include/ksim_whatif.h) take scenario weights for LeastRequested, MostRequested and
 * BalancedResourceAllocation only, and refuse them over any queue or policy that reads a reduce
 * priority, SelectorSpread or a NodePreferAvoidPods addend; ksim_sweep_drain, ksim_sweep_affinity and
 * ksim_sweep_volumes take none.  Here every scenario carries all KSIM_NW weights, over every queue the
 * other entries sweep, and can report what its policy did to the cluster without a replay of its
 * placements.
 *
 * The entry is exported from the same libksim.so and is plain C (cgo).  include/ksim.h,
 * include/ksim_whatif.h, include/ksim_drain.h, include/ksim_affsweep.h, include/ksim_volsweep.h, their
 * function lists and KSIM_ABI_VERSION are unchanged. */
#ifndef KSIM_POLSWEEP_H
#define KSIM_POLSWEEP_H

#include "ksim.h"
#include "ksim_affsweep.h"
#include "ksim_drain.h"
#include "ksim_volsweep.h"
#include "ksim_whatif.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Buckets of a free-capacity histogram: the values 0..10 of LeastRequestedPriority's per-resource
 * score (least_requested.go:36-53), ((capacity - requested) * 10) / capacity. */
#define KSIM_OUTCOME_BUCKETS 11

/* Where a sweep's outcome records go: per scenario s, all over the nodes the scenario lists and their
 * state after its last pod,
 *   listed[s]       the number of listed nodes,
 *   used[s]         listed nodes that hold at least one pod,
 *   free_cpu[s][b]  listed nodes whose free-cpu score is b: the score LeastRequestedPriority gives the
 *                   node's non-zero cpu request sum against its allocatable cpu, no pod's request
 *                   added; 0 also covers zero capacity and over-commit,
 *   free_mem[s][b]  likewise for memory.
 * They are counts of nodes: nothing can overflow.  free_cpu[s] and free_mem[s] each sum to listed[s].
 * All four arrays are required. */
typedef struct ksim_sweep_outcome {
  int32_t* listed;   /* [n_scen] */
  int32_t* used;     /* [n_scen] */
  int32_t* free_cpu; /* [n_scen][KSIM_OUTCOME_BUCKETS] */
  int32_t* free_mem; /* [n_scen][KSIM_OUTCOME_BUCKETS] */
} ksim_sweep_outcome;

/* Scenario s equals one run of the reference simulator (pkg/scheduler/simulator.go New + Run) on the
 * snapshot without the scenario's absent nodes and without the placed pods bound to them, over the
 * queue: first the scenario's prefix pods (rq, exactly as in ksim_sweep_drain; rq == NULL: no
 * prefixes, and count must then be positive), after them pods [first, first + count) of the loaded
 * queue.  The run uses the handle's predicates and the prioritizer list whose weights are row s of
 * weights ([n_scen][KSIM_NW], indexed by KSIM_W_*; 0: the priority is not configured).  absent (NULL:
 * no node is absent in any scenario), res, out_node, out_counters, out_scheduled, out_rehosted, fail
 * and stats keep their meanings from ksim_whatif.h, ksim_drain.h and ksim_affsweep.h.
 *
 * State.  A scenario owns what the other entries' scenarios own, together: the node columns a commit
 * writes, the SelectorSpread counts, the inter-pod affinity counts and carried terms (less the
 * residents of its absent nodes: res), and the volume mounts when volume tables are loaded.  The
 * handle's state, counts, mounts, counter and error word are left untouched.
 *
 * Weight rules, checked before the device is touched; a refusal names the scenario.
 *   - Every weight is at least 0.
 *   - LeastRequested, MostRequested and BalancedResourceAllocation may take any value in any scenario.
 *   - TaintToleration, NodeAffinity, InterPodAffinity and SelectorSpread may be non-zero in a scenario
 *     only where the handle's own weight is non-zero: the class tables, the spread tables and the
 *     NodeAffinity class dimension were built for the handle's policy, so a scenario rescales or drops
 *     such a priority but cannot add it.
 *   - The per-class addends (NodePreferAvoidPods, ImageLocality and the Policy's label priorities,
 *     ksim_class_tables.na_add) and the constant score stay the handle's in every scenario.
 *   - A handle created with no_priorities is refused.
 *   - Per scenario 10 x (LeastRequested + MostRequested + Balanced + SelectorSpread + InterPodAffinity
 *     weight) must fit the 27 bits of the packed score.
 * The predicates do not depend on the weights: with affinity terms loaded MatchInterPodAffinity runs in
 * every scenario whatever its inter-pod weight.
 *
 * Form.  Always the general form (stats.mode == KSIM_MODE_PERSISTENT, exact int64, at most
 * KSIM_SWEEP_GENERAL_MAX_NODES = 38,400 nodes), whatever the range holds.
 *
 * outcome (NULL: not computed): the records above, reduced on the device from each scenario's own
 * copy of the node state after its queue.
 *
 * KSIM_E_INVAL, checked before the device is touched: what ksim_sweep_affinity lists for rq, fail, the
 * range and res; weights == NULL; an outcome with a NULL array.
 *
 * KSIM_E_OVERFLOW: as ksim_sweep_volumes.
 *
 * Refusals (KSIM_E_UNSUPPORTED, under this function's name): the weight rules; auxiliary spreading or
 * CheckServiceAffinity lender tables; more than KSIM_MAX_RCLASS reduce classes in a range or prefix
 * pod's class under the handle's weights (which covers every scenario); more than
 * KSIM_SWEEP_SPREAD_MAX_ZONES (512) zones when the queue or an affinity class has a SelectorSpread
 * pair; a node-sharded handle; more than KSIM_SWEEP_GENERAL_MAX_NODES nodes; affinity or volume tables
 * that predate a node event; a pod that mounts volumes on a handle without volume tables.
 *
 * stats: as ksim_sweep_drain documents; device_ms includes the outcome kernel. */
int ksim_sweep_policy(ksim_handle* h, const int64_t* weights /* [n_scen][KSIM_NW] */,
                      const uint32_t* absent /* may be NULL */, int32_t n_scen,
                      const ksim_sweep_residents* res /* may be NULL */,
                      const ksim_sweep_requeue* rq /* may be NULL */,
                      int64_t first, int64_t count, int32_t* out_node, uint64_t* out_counters,
                      int32_t* out_scheduled, int32_t* out_rehosted,
                      const ksim_sweep_failures* fail /* may be NULL */,
                      const ksim_sweep_outcome* outcome /* may be NULL */, ksim_stats* stats);

#ifdef __cplusplus
}
#endif

#endif /* KSIM_POLSWEEP_H */
