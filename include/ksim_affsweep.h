/* ksim_affsweep.h — outage and drain what-ifs over inter-pod affinity queues.  ksim_sweep_nodes
 * (include/ksim.h) and ksim_sweep_drain (include/ksim_drain.h) sweep SelectorSpread state alone and
 * refuse tables that hold a required, preferred or carried inter-pod affinity term.  Required
 * hostname or zone anti-affinity between the replicas of a service is the commonest constraint in
 * production manifests, and the one whose answer changes most under an outage: losing a zone removes
 * the pods that repelled a replica, or the only pod a required-affinity term pointed at.  Here every
 * scenario owns its affinity state.
 *
 * The entry is exported from the same libksim.so and is plain C (cgo).  include/ksim.h,
 * include/ksim_whatif.h, include/ksim_drain.h, their function lists and KSIM_ABI_VERSION are
 * unchanged. */
#ifndef KSIM_AFFSWEEP_H
#define KSIM_AFFSWEEP_H

#include "ksim.h"
#include "ksim_drain.h"
#include "ksim_whatif.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The placed pods behind the handle's current counts (ksim_affinity_tables.cnt / carried as loaded,
 * plus every ksim_schedule / ksim_assume commit since): the snapshot's running pods and whatever an
 * earlier ksim_schedule on this handle bound.  Every placed pod with a non-zero identity or class
 * must be listed; a pod with neither contributes nothing and may be left out. */
typedef struct ksim_sweep_residents {
  int64_t n;
  const int32_t* node;       /* [n] name rank of the pod's node */
  const int32_t* aff_ident;  /* [n] as ksim_pod.aff_ident (1 + id, 0: none) */
  const int32_t* aff_class;  /* [n] as ksim_pod.aff_class */
} ksim_sweep_residents;

/* Scenario s equals one run of the reference simulator (pkg/scheduler/simulator.go New + Run) on the
 * snapshot without the scenario's absent nodes and without the placed pods bound to them, over the
 * queue: first the scenario's prefix pods (rq, exactly as in ksim_sweep_drain; rq == NULL: no
 * prefixes, as in ksim_sweep_nodes, and count must then be positive), after them pods [first,
 * first + count) of the loaded queue.  The run is under the handle's own policy, MatchInterPodAffinity,
 * InterPodAffinityPriority and SelectorSpread included.  absent, out_node, out_counters,
 * out_scheduled, out_rehosted, fail and stats keep their meanings from ksim_whatif.h and
 * ksim_drain.h.  The handle's state, counts, counter and error word are left untouched.
 *
 * Counts.  The counted pairs and carried terms are kept per topology domain, so a zone-keyed or
 * cluster-wide count includes the placed pods on nodes a scenario does not list, and the reference
 * removes those pods with their nodes.  A scenario's copy of both arrays is therefore the handle's
 * minus the contribution of every resident whose node is absent in that scenario.  res == NULL or
 * n == 0: nothing is taken out (right when no node is absent, or no placed pod has affinity state).
 * After the correction no counted pair of any scenario may be negative: a negative one means the
 * list is not the pods behind the counts, and the call fails with KSIM_E_INVAL naming the scenario.
 *
 * Form.  Always the general form (exact int64, at most KSIM_SWEEP_GENERAL_MAX_NODES = 38,400 nodes).
 * Scenario weights are not taken.  The packed score holds 10 x (LeastRequested + MostRequested +
 * Balanced + SelectorSpread + InterPodAffinity weight) in 27 bits; a larger policy is refused.
 *
 * KSIM_E_INVAL, checked before the device is touched: what ksim_sweep_drain lists for rq, fail and
 * the range; a resident's node outside [0, n_nodes), identity above the loaded n_ident, class above
 * n_aclass, or a negative one; n > 0 with a NULL array.
 *
 * Refusals (KSIM_E_UNSUPPORTED, under this function's name): no affinity tables loaded (use
 * ksim_sweep_nodes or ksim_sweep_drain); volumes on a range or prefix pod; auxiliary spreading or
 * CheckServiceAffinity lender tables; more than KSIM_MAX_RCLASS reduce classes in a pod class; more
 * than KSIM_SWEEP_SPREAD_MAX_ZONES (512) zones when an affinity class has a SelectorSpread pair; a
 * node-sharded handle; more than KSIM_SWEEP_GENERAL_MAX_NODES nodes; affinity or volume tables that
 * predate a node event (ksim_schedule refuses them too: load them again).
 *
 * stats: as ksim_sweep_drain documents. */
int ksim_sweep_affinity(ksim_handle* h, const uint32_t* absent, int32_t n_scen,
                        const ksim_sweep_residents* res, const ksim_sweep_requeue* rq /* may be NULL */,
                        int64_t first, int64_t count, int32_t* out_node, uint64_t* out_counters,
                        int32_t* out_scheduled, int32_t* out_rehosted,
                        const ksim_sweep_failures* fail, ksim_stats* stats);

#ifdef __cplusplus
}
#endif

#endif /* KSIM_AFFSWEEP_H */
