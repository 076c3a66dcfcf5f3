/* ksim_drain.h — drain what-ifs: the node-outage sweep of include/ksim.h (ksim_sweep_nodes) with the
 * pods of the lost nodes re-queued.  ksim_sweep_nodes drops the pods bound to an absent node with
 * it and reports only whether the new queue fits on the survivors; the question an operator asks
 * first of an N-1 or zone outage is whether the survivors can re-host what was running there, and
 * those pods meet other constraints (selectors, host ports, tolerations) than the queue.  Here every
 * scenario schedules a prefix queue of its own before the shared range.
 *
 * The entry is exported from the same libksim.so and is plain C (cgo).  include/ksim.h,
 * include/ksim_whatif.h, their function lists and KSIM_ABI_VERSION are unchanged. */
#ifndef KSIM_DRAIN_H
#define KSIM_DRAIN_H

#include "ksim.h"
#include "ksim_whatif.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The scenarios' prefix queues, as indices into the loaded pod queue.  The caller loads the pods to
 * re-queue with the queue (ksim_load_pods): a re-queued pod is the copy of the evicted pod a
 * controller would recreate, spec.nodeName removed, status dropped, everything else kept. */
typedef struct ksim_sweep_requeue {
  const int64_t* off;   /* [n_scen + 1], off[0] = 0, non-decreasing: scenario s re-queues pod[off[s] .. off[s+1]) */
  const int64_t* pod;   /* [off[n_scen]] indices into the loaded pod queue, in scheduling order per scenario */
  int32_t* out_node;    /* [off[n_scen]] node index or -1, parallel to pod */
} ksim_sweep_requeue;

/* ksim_sweep_nodes under the handle's own policy (weights == NULL) with a prefix queue per scenario.
 *
 * Scenario s equals one run of the reference simulator (pkg/scheduler/simulator.go New + Run) on
 * the snapshot without the scenario's absent nodes and without the running pods bound to them, over
 * the queue: first pods pod[off[s] .. off[s+1]) in the order given, after them pods [first,
 * first + count) of the loaded queue.
 *
 * Everything else is exactly ksim_sweep_nodes: absent nodes are never evaluated or counted
 * (absent == NULL: no node is absent), the name order of the remaining nodes is unchanged,
 * placements are name ranks of the loaded table, lastNodeIndex starts at the handle's value and
 * advances by selectHost's rule, over the prefix pods too, each pod is committed into the scenario's
 * own columns, and the handle's state, counter and error word are left untouched.  A scenario that
 * lists no node fails every pod, prefix included, and its counter stays at the start value.
 *
 * Form.  The call always runs in the general form (exact int64, at most 38,400 nodes,
 * KSIM_SWEEP_GENERAL_MAX_NODES), even when every pod is resource-only: the float64 scan and tree
 * forms take no prefix queues.  Scenario weights are not taken.
 *
 * count == 0 is allowed ("only re-host the evicted pods", the N-1 survivability check); out_node
 * may then be NULL.  count == 0 with an empty rq is KSIM_E_INVAL.
 *
 * Repeated indices.  The same index may appear in several scenarios (a zone outage contains its
 * nodes' outages), repeat within a scenario or lie inside [first, first + count): such a pod is
 * scheduled once per appearance.  No check is made.
 *
 * out_scheduled[s]: pods bound among the range, as in ksim_sweep_nodes.  out_rehosted[s]: pods bound
 * among the scenario's prefix.  Both are optional.
 *
 * fail: ksim_sweep_failures of ksim_whatif.h, its meaning unchanged except that pod[s][k] is the
 * failed pod's position in the scenario's own queue: with m_s = off[s+1] - off[s], positions
 * 0 .. m_s - 1 are the prefix pods and position m_s + i is range pod first + i.  count[s] counts
 * failed prefix and range pods together, listed[s] is as before, cap counts records over the whole
 * scenario queue.  cap < 0, or cap > 0 with a NULL pod or hist: KSIM_E_INVAL, checked before the
 * handle.
 *
 * Refusals (KSIM_E_UNSUPPORTED, under this function's name), for the range and for every prefix pod:
 * inter-pod affinity state (SelectorSpread state alone is swept, as ksim_sweep describes: the
 * re-queued pods of a service count in the scenario's own copy of the counted pairs; more than
 * KSIM_SWEEP_SPREAD_MAX_ZONES zones are refused), volumes, more than KSIM_MAX_RCLASS reduce classes,
 * loaded auxiliary or CheckServiceAffinity lender tables, a node-sharded handle, more than
 * KSIM_SWEEP_GENERAL_MAX_NODES nodes.
 *
 * KSIM_E_INVAL: rq == NULL, a NULL off, off[0] != 0, a decreasing off, a NULL pod or out_node with
 * off[n_scen] > 0, a pod index outside the loaded queue, m_s + count > INT32_MAX.  What needs no
 * device is checked before the handle is touched.
 *
 * stats: pods is the sum of m_s plus n_scen * count, node_evals that times n_nodes; mode, blocks and
 * kernel_launches as in the general form of ksim_sweep_nodes. */
int ksim_sweep_drain(ksim_handle* h, const uint32_t* absent, int32_t n_scen, const ksim_sweep_requeue* rq,
                     int64_t first, int64_t count, int32_t* out_node, uint64_t* out_counters,
                     int32_t* out_scheduled, int32_t* out_rehosted,
                     const ksim_sweep_failures* fail, ksim_stats* stats);

#ifdef __cplusplus
}
#endif

#endif /* KSIM_DRAIN_H */
