/* ksim_whatif.h — why the pods of a what-if failed: the scenario sweep of include/ksim.h
 * (ksim_sweep, ksim_sweep_nodes) with the FitError histogram of every failed pod, per scenario.
 * The reference tells an operator which pod failed and "0/N nodes are available: 3 Insufficient
 * cpu, 2 node(s) didn't match node selector." (core/generic_scheduler.go:51-90); a sweep that only
 * counts the failed pods of an outage cannot say whether they fail on cpu, on host ports or because
 * the only nodes their selector matches were the ones taken away.
 *
 * The entry is exported from the same libksim.so and is plain C (cgo).  include/ksim.h, its function
 * list and KSIM_ABI_VERSION are unchanged. */
#ifndef KSIM_WHATIF_H
#define KSIM_WHATIF_H

#include "ksim.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Caller-owned output of ksim_sweep_explain: per scenario the first `cap` failed pods in queue
 * order, each with its FitError histogram. */
typedef struct ksim_sweep_failures {
  int32_t  cap;     /* records kept per scenario */
  int32_t* count;   /* [n_scen] failed pods of the scenario (may exceed cap) */
  int32_t* listed;  /* [n_scen] nodes the scenario lists: N of "0/N nodes are available" */
  int32_t* pod;     /* [n_scen][cap] index (relative to first) of the k-th failed pod, queue order */
  int32_t* hist;    /* [n_scen][cap][KSIM_NREASONS] its FitError histogram */
} ksim_sweep_failures;

/* ksim_sweep_nodes that also explains its failed pods.
 *
 * Same run.  Everything ksim_sweep_nodes says holds: the accepted pods, the node caps, every refusal
 * (its message under this function's name), absent == NULL (no node absent), weights == NULL (the
 * handle's own policy), and the handle's own state, counter and error word left untouched.
 * out_node, out_counters and out_scheduled are bit for bit what ksim_sweep_nodes returns for the
 * same arguments: explaining never changes a decision.  That includes SelectorSpread queues (swept
 * when the tables hold SelectorSpread state only; inter-pod affinity state is still refused): a
 * priority never enters a histogram.
 *
 * Histogram.  A failed pod's histogram is FitError.FailedPredicates of the reference run on the
 * reduced snapshot (generic_scheduler.go:51-90): every node the scenario lists adds one to each
 * reason (KSIM_R_*) of its first failing predicate in predicatesOrdering.  A node may add to
 * several slots (GeneralPredicates reports cpu and memory together).  Absent nodes are not
 * evaluated and add nothing.
 *
 * listed[s] is n_nodes - |absent set of s| (bits at or above n_nodes are ignored).
 *
 * Records are kept in queue order, the first min(count[s], cap) of them.  count[s] is always the
 * full number of failed pods of the scenario and equals count - out_scheduled[s].  Words of pod and
 * hist past the kept records are left unwritten.
 *
 * A scenario that lists no node: every pod fails with an all-zero histogram and listed[s] = 0 (the
 * reference returns ErrNoNodesAvailable there; the caller maps it).
 *
 * fail == NULL or cap == 0: the call launches exactly what ksim_sweep_nodes launches; count and
 * listed are still filled when fail is given (either may be NULL and is then skipped).
 *
 * cap < 0, or cap > 0 with a NULL pod or hist: KSIM_E_INVAL. */
int ksim_sweep_explain(ksim_handle* h, const int64_t* weights, const uint32_t* absent, int32_t n_scen,
                       int64_t first, int64_t count, int32_t* out_node, uint64_t* out_counters,
                       int32_t* out_scheduled, const ksim_sweep_failures* fail, ksim_stats* stats);

#ifdef __cplusplus
}
#endif

#endif /* KSIM_WHATIF_H */
