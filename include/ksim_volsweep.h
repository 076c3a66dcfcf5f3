/* ksim_volsweep.h — outage and drain what-ifs over volume queues.  ksim_sweep_nodes
 * (include/ksim_whatif.h), ksim_sweep_drain (include/ksim_drain.h) and ksim_sweep_affinity
 * (include/ksim_affsweep.h) refuse a pod that mounts volumes: the mounts of a node are state that a
 * commit writes, and those entries keep none per scenario.  Outage questions about volumes are sharp
 * ones: a zone outage strands every pod whose PersistentVolume lives in the lost zone; the evicted pods
 * of a drain carry their EBS, GCE PD and Azure disks to the survivors, where they meet
 * MaxEBSVolumeCount, MaxGCEPDVolumeCount, MaxAzureDiskVolumeCount and NoDiskConflict; and the mounts of
 * a lost node go with it.  Here every scenario owns its mounts.
 *
 * The entry is exported from the same libksim.so and is plain C (cgo).  include/ksim.h,
 * include/ksim_whatif.h, include/ksim_drain.h, include/ksim_affsweep.h, their function lists and
 * KSIM_ABI_VERSION are unchanged. */
#ifndef KSIM_VOLSWEEP_H
#define KSIM_VOLSWEEP_H

#include "ksim.h"
#include "ksim_affsweep.h"
#include "ksim_drain.h"
#include "ksim_whatif.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Scenario s equals one run of the reference simulator (pkg/scheduler/simulator.go New + Run) on the
 * snapshot without the scenario's absent nodes and without the placed pods bound to them, over the
 * queue: first the scenario's prefix pods (rq, exactly as in ksim_sweep_drain; rq == NULL: no
 * prefixes, as in ksim_sweep_nodes, and count must then be positive), after them pods [first,
 * first + count) of the loaded queue.  The run is under the handle's whole policy: NoDiskConflict, the
 * three MaxPD filters and NoVolumeZoneConflict at their places in predicatesOrdering, and
 * SelectorSpread, MatchInterPodAffinity and InterPodAffinityPriority when affinity tables are loaded.
 * absent, out_node, out_counters, out_scheduled, out_rehosted, fail and stats keep their meanings from
 * ksim_whatif.h and ksim_drain.h.
 *
 * Mounts.  Every scenario starts from the handle's current mounts (ksim_volume_tables.slots /
 * slot_count as loaded, plus every ksim_schedule / ksim_assume commit since, so a sweep after a
 * ksim_schedule of a prefix carries that prefix's mounts) in a copy of its own.  The mounts are kept
 * per node and an absent node is never evaluated, so its mounts are never read: nothing has to be
 * taken out.  A range or prefix pod with a volume class that binds adds its refs to the chosen node's
 * slots in the scenario's copy, as a ksim_schedule commit does to the handle's.  The handle's slots,
 * slot counts, node state, counts, counter and error word are left untouched.
 *
 * res: used exactly as in ksim_sweep_affinity when the loaded affinity tables hold a required,
 * preferred or carried term (the scenarios' counts less the residents of their absent nodes), checked
 * against the loaded tables in every call, and otherwise ignored.  May be NULL.
 *
 * Form.  Always the general form (exact int64, at most KSIM_SWEEP_GENERAL_MAX_NODES = 38,400 nodes).
 * Scenario weights are not taken.  The packed score holds 10 x (LeastRequested + MostRequested +
 * Balanced + SelectorSpread + InterPodAffinity weight) in 27 bits; a larger policy is refused.
 *
 * KSIM_E_INVAL, checked before the device is touched: what ksim_sweep_affinity lists for rq, fail,
 * the range and res.
 *
 * KSIM_E_OVERFLOW: a commit of some scenario found the chosen node's volume slots full (the tables'
 * vol_slots) or a mount count of a key saturated, or its host-port slots full.  The bit is the sweep's
 * own (the one ksim_schedule reports for either kind of slot); the handle is untouched and the next
 * call starts from a cleared word.  The outputs are then unspecified.
 *
 * Refusals (KSIM_E_UNSUPPORTED, under this function's name): no volume tables loaded (use
 * ksim_sweep_nodes, ksim_sweep_drain or ksim_sweep_affinity); auxiliary spreading or
 * CheckServiceAffinity lender tables; more than KSIM_MAX_RCLASS reduce classes in a range or prefix
 * pod's class; more than KSIM_SWEEP_SPREAD_MAX_ZONES (512) zones when an affinity class has a
 * SelectorSpread pair; a node-sharded handle; more than KSIM_SWEEP_GENERAL_MAX_NODES nodes; affinity
 * or volume tables that predate a node event (ksim_schedule refuses them too: load them again); a
 * policy beyond the 27-bit score.
 *
 * stats: as ksim_sweep_drain documents. */
int ksim_sweep_volumes(ksim_handle* h, const uint32_t* absent, int32_t n_scen,
                       const ksim_sweep_residents* res /* may be NULL */,
                       const ksim_sweep_requeue* rq /* may be NULL */,
                       int64_t first, int64_t count, int32_t* out_node, uint64_t* out_counters,
                       int32_t* out_scheduled, int32_t* out_rehosted,
                       const ksim_sweep_failures* fail, ksim_stats* stats);

#ifdef __cplusplus
}
#endif

#endif /* KSIM_VOLSWEEP_H */
