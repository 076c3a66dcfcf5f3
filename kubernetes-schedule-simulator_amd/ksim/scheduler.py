"""Host-side mirror of the reference's ScheduleAlgorithm plugin surface and simulator loop.

- Predicate / priority key sets and weights, exactly as the algorithm providers register
  them (vendor/k8s.io/kubernetes/pkg/scheduler/algorithmprovider/defaults/defaults.go:
  113-259, the TalkintDataProvider added at :36,214-216) or as a Policy lists them.
  Every supported key maps to a kernel feature bit or weight slot; any other key raises
  Unsupported (never a silently different result).
- GenericScheduler: the batch form of genericScheduler.Schedule + Scheduler.assume over a
  device-resident cluster (core/generic_scheduler.go:112-198, scheduler.go:366).
- FitError: message format of core/generic_scheduler.go:72-90.
- ClusterCapacity: the simulator's loop (pkg/scheduler/simulator.go:108-223): pods are
  popped LIFO from the expanded pod list (pkg/framework/store/store.go:223-233), each is
  scheduled and committed before the next; unschedulable pods are recorded and the run
  continues until the queue is empty.
"""
from __future__ import annotations

import contextlib
import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import abi
from .ingest import Cluster, Unsupported, class_tables_struct

# predicates.go:129-138 keys → kernel bits
PREDICATE_BITS = {
    "CheckNodeCondition": abi.P_CHECK_NODE_CONDITION,
    "CheckNodeUnschedulable": abi.P_CHECK_NODE_UNSCHEDULABLE,
    "GeneralPredicates": abi.P_GENERAL,
    "HostName": abi.P_HOSTNAME,
    "PodFitsHostPorts": abi.P_HOST_PORTS,
    "MatchNodeSelector": abi.P_NODE_SELECTOR,
    "PodFitsResources": abi.P_RESOURCES,
    "PodToleratesNodeTaints": abi.P_TAINTS,
    "PodToleratesNodeNoExecuteTaints": abi.P_NOEXEC_TAINTS,
    "CheckNodeMemoryPressure": abi.P_MEM_PRESSURE,
    "CheckNodeDiskPressure": abi.P_DISK_PRESSURE,
    "CheckNodeLabelPresence": abi.P_LABEL_PRESENCE,   # with a Policy labelsPresence argument
    "MatchInterPodAffinity": abi.P_INTERPOD_AFFINITY,  # over the cluster's affinity tables
    "NoDiskConflict": abi.P_DISK_CONFLICT,              # over the cluster's volume tables
    "MaxEBSVolumeCount": abi.P_MAX_EBS,
    "MaxGCEPDVolumeCount": abi.P_MAX_GCE_PD,
    "MaxAzureDiskVolumeCount": abi.P_MAX_AZURE_DISK,
    "NoVolumeZoneConflict": abi.P_VOLUME_ZONE,
    "CheckServiceAffinity": abi.P_SERVICE_AFFINITY,     # with a Policy serviceAffinity argument
}
VOLUME_PREDICATE_BITS = abi.P_DISK_CONFLICT | abi.P_MAX_EBS | abi.P_MAX_GCE_PD | abi.P_MAX_AZURE_DISK | abi.P_VOLUME_ZONE
# factory/plugins.go:401-406 + defaults.go:165: part of every predicate map
MANDATORY_PREDICATES = ("CheckNodeCondition",)
# keys that are true for every pod the scheduler accepts: CheckVolumeBinding (PVCs only when
# bound to a PV without node affinity, ksim/volumes.py); "PodFitsPorts" is registered but absent
# from predicatesOrdering, so it never runs
TRIVIAL_PREDICATES = {"CheckVolumeBinding", "PodFitsPorts"}

PRIORITY_SLOTS = {"LeastRequestedPriority": abi.W_LEAST, "MostRequestedPriority": abi.W_MOST,
                  "BalancedResourceAllocation": abi.W_BALANCED, "TaintTolerationPriority": abi.W_TAINT_TOL,
                  "NodeAffinityPriority": abi.W_NODE_AFF, "InterPodAffinityPriority": abi.W_INTERPOD}
SPREAD_PRIORITIES = ("SelectorSpreadPriority", "ServiceSpreadingPriority")
# value on every node under supported inputs (no services/controllers in the simulator's store —
# with SpreadListers the spread priorities take the W_SPREAD slot —, no RC/RS-owned pods next to
# preferAvoidPods annotations)
CONST_PRIORITIES = {"SelectorSpreadPriority": 10, "ServiceSpreadingPriority": 10, "NodePreferAvoidPodsPriority": 10,
                    "EqualPriority": 1,
                    # image_locality.go:39-69: 0 on every node when no node lists status.images
                    "ImageLocalityPriority": 0}

DEFAULT_PREDICATES = ("NoVolumeZoneConflict", "MaxEBSVolumeCount", "MaxGCEPDVolumeCount", "MaxAzureDiskVolumeCount",
                      "MatchInterPodAffinity", "NoDiskConflict", "GeneralPredicates", "CheckNodeMemoryPressure",
                      "CheckNodeDiskPressure", "CheckNodeCondition", "PodToleratesNodeTaints", "CheckVolumeBinding")
DEFAULT_PRIORITIES = (("SelectorSpreadPriority", 1), ("InterPodAffinityPriority", 1), ("LeastRequestedPriority", 1),
                      ("BalancedResourceAllocation", 1), ("NodePreferAvoidPodsPriority", 10000),
                      ("NodeAffinityPriority", 1), ("TaintTolerationPriority", 1))
PROVIDERS = ("DefaultProvider", "ClusterAutoscalerProvider", "TalkintDataProvider")


def provider(name: str):
    """registerAlgorithmProvider (defaults.go:207-217)."""
    if name not in PROVIDERS:
        raise Unsupported("algorithm provider %r is not registered" % name)
    pri = list(DEFAULT_PRIORITIES)
    if name != "DefaultProvider":  # copyAndReplace(LeastRequested → MostRequested)
        pri = [("MostRequestedPriority", w) if n == "LeastRequestedPriority" else (n, w) for n, w in pri]
    return list(DEFAULT_PREDICATES), pri


def make_config(predicates, priorities, device=0, mode=abi.MODE_AUTO, collect_reasons=True, last_node_index=0,
                spread=False, configured=None):
    """spread: the cluster has SelectorSpread selectors (Cluster.spread_active): the spread priority
    scores per node (KSIM_W_SELECTOR_SPREAD) instead of being the constant MaxPriority.
    configured: the whole prioritizer list when `priorities` leaves some out (Policy priorities
    with arguments, the auxiliary priority): only an empty one means EqualPriorityMap."""
    cfg = abi.Config()
    cfg.device = device
    cfg.mode = mode
    bits = 0
    for k in list(predicates) + list(MANDATORY_PREDICATES):
        if k in PREDICATE_BITS:
            bits |= PREDICATE_BITS[k]
        elif k not in TRIVIAL_PREDICATES:
            raise Unsupported("predicate %r is outside the supported key set" % k)
    cfg.predicates = bits
    const = 0
    seen = set()
    for name, w in priorities:
        if name in seen:
            raise abi.KsimError(abi.E_INVAL, "duplicate priority %r" % name)
        seen.add(name)
        if w <= 0:
            raise abi.KsimError(abi.E_INVAL, "priority %r: weight must be positive" % name)
        if name in PRIORITY_SLOTS:
            cfg.weights[PRIORITY_SLOTS[name]] = w
        elif spread and name in SPREAD_PRIORITIES:
            if cfg.weights[abi.W_SPREAD]:
                raise Unsupported("SelectorSpreadPriority and ServiceSpreadingPriority together with spread selectors")
            cfg.weights[abi.W_SPREAD] = w
        elif name in CONST_PRIORITIES:
            const += CONST_PRIORITIES[name] * w
        else:
            raise Unsupported("priority %r is outside the supported key set" % name)
    empty = not (priorities if configured is None else configured)
    cfg.no_priorities = 1 if empty else 0
    if empty:
        const = 1
    cfg.const_score = const
    cfg.collect_reasons = 1 if collect_reasons else 0
    cfg.last_node_index = last_node_index
    return cfg


REASON_TEXT = {
    abi.R_NOT_READY: "node(s) were not ready",
    abi.R_OUT_OF_DISK: "node(s) were out of disk space",
    abi.R_NET_UNAVAIL: "node(s) had unavailable network",
    abi.R_UNSCHEDULABLE: "node(s) were unschedulable",
    abi.R_PODS: "Insufficient pods",
    abi.R_CPU: "Insufficient cpu",
    abi.R_MEMORY: "Insufficient memory",
    abi.R_GPU: "Insufficient alpha.kubernetes.io/nvidia-gpu",
    abi.R_EPHEMERAL: "Insufficient ephemeral-storage",
    abi.R_HOSTNAME: "node(s) didn't match the requested hostname",
    abi.R_HOST_PORTS: "node(s) didn't have free ports for the requested pod ports",
    abi.R_NODE_SELECTOR: "node(s) didn't match node selector",
    abi.R_TAINTS: "node(s) had taints that the pod didn't tolerate",
    abi.R_MEM_PRESSURE: "node(s) had memory pressure",
    abi.R_DISK_PRESSURE: "node(s) had disk pressure",
    abi.R_LABEL_PRESENCE: "node(s) didn't have the requested labels",
    abi.R_POD_AFFINITY: "node(s) didn't match pod affinity/anti-affinity",
    abi.R_EXISTING_ANTI: "node(s) didn't satisfy existing pods anti-affinity rules",
    abi.R_AFFINITY_RULES: "node(s) didn't match pod affinity rules",
    abi.R_ANTI_AFFINITY_RULES: "node(s) didn't match pod anti-affinity rules",
    abi.R_DISK_CONFLICT: "node(s) had no available disk",
    abi.R_MAX_VOLUME_COUNT: "node(s) exceed max volume count",
    abi.R_VOLUME_ZONE: "node(s) had no available volume zone",
    abi.R_SERVICE_AFFINITY: "node(s) didn't match service affinity",
}


def reason_strings(mask: int, scalar_names=()):
    out = []
    for r in range(abi.NREASONS):
        if (mask >> r) & 1:
            out.append(reason_text(r, scalar_names))
    return out


def reason_text(r, scalar_names=()):
    if abi.R_SCALAR0 <= r < abi.R_SCALAR0 + abi.MAX_SCALAR:
        return "Insufficient " + scalar_names[r - abi.R_SCALAR0]
    return REASON_TEXT[r]


def fit_error_message(num_nodes, hist, scalar_names=()):
    """FitError.Error (core/generic_scheduler.go:72-90)."""
    parts = sorted("%d %s" % (int(v), reason_text(r, scalar_names)) for r, v in enumerate(hist) if v)
    return "0/%d nodes are available: %s." % (num_nodes, ", ".join(parts))


def label_set_priority(spec, label_set):
    """Map score of a Policy custom priority that is a function of the node's labels alone:
    NodeLabelPriority (priorities/node_label.go:42-58) and, with no services selecting the pod, the
    ServiceAntiAffinity priority (selector_spreading.go:221-275: no first service selector, so every
    count is 0 and a node scores MaxPriority when it has the label, 0 otherwise)."""
    if spec[0] == "labelPreference":
        return 10 if (spec[1] in label_set) == spec[2] else 0
    return 10 if spec[1] in label_set else 0


def class_tables_for(tables, priorities, label_sets=(), custom=None):
    """The class tables a scheduler with these priorities loads, and the weighted per-NodeAffinity-
    class addends (ksim_class_tables.na_add) or None.

    NodePreferAvoidPodsPriority (node_prefer_avoid_pods.go:32-68) and ImageLocalityPriority
    (image_locality.go:39-88) are functions of (pod class, label set) — the label set carries the
    node's preferAvoidPods annotation and its images, the class the pod's controller and container
    images — and the Policy's labelPreference / serviceAntiAffinity priorities
    (label_set_priority) of the label set alone.
    When the policy weighs them and they differ across the nodes some pod class sees, the
    NodeAffinity class dimension is re-keyed by (preferred weight, summed addend) — by the addend
    alone if NodeAffinityPriority is not configured — and each class adds its weighted score.
    Otherwise NodePreferAvoidPods is the constant MaxPriority x weight of const_score."""
    custom = custom or {}
    w_pa = sum(int(x) for n, x in priorities if n == "NodePreferAvoidPodsPriority")
    w_im = sum(int(x) for n, x in priorities if n == "ImageLocalityPriority")
    im_s = tables.get("im_s")
    im_on = bool(w_im and im_s is not None and im_s.any())
    w_custom = [(custom[n], int(x)) for n, x in priorities if n in custom]
    L = tables["na_class"].shape[1] if tables["na_class"].ndim == 2 else len(label_sets)
    lab_add = np.zeros(L, np.int64)
    for spec, w in w_custom:
        lab_add += np.array([w * label_set_priority(spec, ls) for ls in label_sets], np.int64)
    pa_on = bool(w_pa and tables.get("pa_split"))
    if not pa_on and not im_on and not lab_add.any():
        return tables, None
    use_w = any(n == "NodeAffinityPriority" for n, _ in priorities)
    d = dict(tables)
    Cn = d["n_classes"]
    nac = np.zeros_like(tables["na_class"])
    nna = np.ones(Cn, np.int32)
    avs = []
    for k in range(Cn):
        pa = [int(p) * w_pa if pa_on else 0 for p in tables["na_p"][k]]
        if im_on:
            pa = [a + w_im * int(x) for a, x in zip(pa, im_s[k])]
        keys = list(zip((int(x) if use_w else 0 for x in tables["na_w"][k]), (a + int(b) for a, b in zip(pa, lab_add))))
        av = sorted(set(keys))
        if int(tables["n_tt"][k]) * len(av) > abi.MAX_WIDE:
            raise Unsupported("pod class needs %d x %d reduce classes (> %d)" % (int(tables["n_tt"][k]), len(av), abi.MAX_WIDE))
        nna[k] = len(av)
        avs.append(av)
        pos = {x: i for i, x in enumerate(av)}
        nac[k, :] = [pos[x] for x in keys]
    # one row width for every value array: the class table's, or wider when the addends split more classes
    W = max([tables["tt_val"].shape[1]] + [len(av) for av in avs])
    nav = np.zeros((Cn, W), np.int64)
    add = np.zeros((Cn, W), np.int64)
    for k, av in enumerate(avs):
        nav[k, :len(av)] = [w for w, _ in av]
        add[k, :len(av)] = [p for _, p in av]
    ttv = np.zeros((Cn, W), np.int64)
    ttv[:, :tables["tt_val"].shape[1]] = tables["tt_val"]
    d.update(na_class=nac, n_na=nna, na_val=nav, tt_val=ttv, pa_in_add=pa_on)
    return d, add


def service_affinity_table(class_specs, label_sets, affinity_labels):
    """CheckServiceAffinity (predicates.go:980-1016) with no service selecting the pod: per pod
    class the label sets carrying the class's nodeSelector values of `affinity_labels`
    (FindLabelsInSet, CreateSelectorFromLabels — labels.Set.AsSelector, Everything when empty or
    invalid).  Returns ([n_classes][words] bits, per-class "fails somewhere")."""
    from . import labels as L
    C, S = len(class_specs), len(label_sets)
    words = max((S + 31) // 32, 1)
    ok = np.zeros((C, words), np.uint32)
    need = np.zeros(C, bool)
    for k, spec in enumerate(class_specs):
        sel = (spec or {}).get("nodeSelector") or {}
        al = {x: sel[x] for x in affinity_labels if x in sel}
        req = L.from_set(al)
        for j, ls in enumerate(label_sets):
            if L.matches(req, dict(ls)):
                ok[k, j >> 5] |= np.uint32(1 << (j & 31))
            else:
                need[k] = True
    return ok, need


def check_volume_support(cluster, predicates):
    """Refuse inputs on which a configured volume predicate returns an error instead of a verdict
    (ksim/volumes.py): findNodesThatFit then aborts the pod's cycle (core/generic_scheduler.go:351-353)
    and the simulator's requeue path takes over, which this batch form does not restate."""
    if cluster.volume_index is None:
        return
    errs = cluster.volume_index.errors
    keys = set(predicates)
    maxpd = keys & {"MaxEBSVolumeCount", "MaxGCEPDVolumeCount", "MaxAzureDiskVolumeCount"}
    if "claim_name" in errs and (maxpd or "NoVolumeZoneConflict" in keys):
        raise Unsupported("a PersistentVolumeClaim volume without a claim name (the volume predicates err)")
    if "binding" in errs and "CheckVolumeBinding" in keys:
        raise Unsupported("CheckVolumeBinding with a PVC that is not bound to a PV without node affinity "
                          "(FindPodVolumes errs or needs the volume binder)")
    if cluster.volumes is not None and cluster.volumes["zone_err"] and "NoVolumeZoneConflict" in keys:
        raise Unsupported("NoVolumeZoneConflict with a PVC the PV / PVC listers cannot resolve on a zone-labelled node")


def label_presence_flags(label_sets, label_set_ids, label_presence):
    """KSIM_N_LABEL_PRESENCE per node: CheckNodeLabelPresence (predicates.go:875-910) fails when
    a listed label's presence differs from `presence`; a function of the node's label set."""
    labels_, presence = label_presence
    bad = np.array([any((k in ls) != presence for k in labels_) for ls in label_sets], bool)
    return np.where(bad[np.asarray(label_set_ids)], abi.N_LABEL_PRESENCE, 0).astype(np.uint32)


@dataclass
class Plan:
    """What a scheduler over `cluster` loads, derived on the host alone (no device): the config,
    the node flags, the class tables with their NodePreferAvoidPods addends, the pod queue as
    loaded (affinity / volume / service-affinity fields adjusted to the configured keys), and the
    affinity / volume tables when a configured key reads them (else None)."""
    cfg: object
    flags: object          # node flags with the CheckNodeLabelPresence verdicts, or None (the cluster's)
    tables: dict
    na_add: object
    const_score: int
    pods: object
    affinity: object
    volumes: object
    use_zone: bool


def plan(cluster: Cluster, predicates, priorities, device=0, mode=abi.MODE_AUTO, collect_reasons=True,
         last_node_index=0, label_presence=None, custom_priorities=None, service_affinity=None) -> Plan:
    """The host half of GenericScheduler's construction (also what the table-level C oracle runs
    on): validates the key sets against the cluster's inputs (Unsupported where the reference errs
    or where this restatement stops) and builds every table the library loads."""
    predicates = list(predicates)
    prioritizers = list(priorities)
    custom_priorities = dict(custom_priorities or {})
    aux = getattr(cluster, "aux", None)
    aux_active = bool(getattr(cluster, "aux_active", False))
    aux_weight, aux_const = 0, 0
    saa = [(n, int(w)) for n, w in prioritizers if n in custom_priorities and custom_priorities[n][0] == "serviceAntiAffinity"]
    if saa and aux is not None and aux[0] == "service_anti_affinity" and aux_active:
        # ServiceAntiAffinity with services: the auxiliary counted priority (the pods' single
        # selecting service; Cluster.from_objects refused two or more)
        if len(saa) > 1 or custom_priorities[saa[0][0]][1] != aux[1]:
            raise Unsupported("serviceAntiAffinity priorities other than the one the cluster was built for (%r)" % (aux[1],))
        aux_weight = saa[0][1]
        prioritizers = [(n, w) for n, w in prioritizers if n != saa[0][0]]
        custom_priorities.pop(saa[0][0])
    elif saa and getattr(cluster, "spread_active", False) and not (aux is not None and aux[0] == "service_anti_affinity"):
        raise Unsupported("a serviceAntiAffinity priority with services selecting the pods needs the cluster built "
                          "with aux=('service_anti_affinity', label)")
    names = {n for n, _ in prioritizers}
    if aux is not None and aux[0] == "service_spreading" and {"SelectorSpreadPriority", "ServiceSpreadingPriority"} <= names:
        # ServiceSpreadingPriority next to SelectorSpreadPriority: the auxiliary counted priority over
        # the services-only selectors (MaxPriority everywhere, a constant, when none selects a pod)
        w = sum(int(x) for n, x in prioritizers if n == "ServiceSpreadingPriority")
        if aux_active:
            aux_weight = w
        else:
            aux_const = 10 * w
        prioritizers = [(n, x) for n, x in prioritizers if n != "ServiceSpreadingPriority"]
    if any(n == "NodeAffinityPriority" for n, _ in prioritizers) and cluster.bad_affinity_classes:
        raise Unsupported("NodeAffinityPriority: a preferred node-affinity term does not parse")
    if (any(n == "ImageLocalityPriority" for n, _ in prioritizers) and cluster.node_images
            and not getattr(cluster, "image_locality", False)):
        raise Unsupported("ImageLocalityPriority with nodes that list status.images, on a cluster built "
                          "without image interning (Cluster.from_objects(image_locality=True))")
    if "CheckNodeLabelPresence" in predicates and label_presence is None:
        raise Unsupported("CheckNodeLabelPresence needs its labelsPresence argument")
    svc_dyn = False
    if "CheckServiceAffinity" in predicates:
        if service_affinity is None:
            raise Unsupported("CheckServiceAffinity needs its serviceAffinity argument")
        if getattr(cluster, "svc_any", getattr(cluster, "spread_active", False)):
            # services select queued pods: the lender check needs the cluster built for these labels
            if getattr(cluster, "svc_labels", None) != list(service_affinity):
                raise Unsupported("CheckServiceAffinity with services selecting the pods needs the cluster built with "
                                  "service_affinity=%r" % (list(service_affinity),))
            svc_dyn = bool(cluster.svc_active)
    cfg = make_config([k for k in predicates if k != "CheckNodeLabelPresence" or label_presence],
                      [(n, w) for n, w in prioritizers if n not in custom_priorities],
                      device, mode, collect_reasons, last_node_index,
                      spread=bool(getattr(cluster, "spread_active", False)), configured=list(priorities))
    check_volume_support(cluster, predicates)
    flags = None
    if label_presence is not None and "CheckNodeLabelPresence" in predicates:
        fl = cluster.cols["flags"] | label_presence_flags(cluster.label_sets.items, cluster.cols["label_set"],
                                                            label_presence)
        flags = np.ascontiguousarray(fl, np.uint32)
    tables, na_add = class_tables_for(cluster.tables, prioritizers, cluster.label_sets.items, custom_priorities)
    # const_score without NodePreferAvoidPods when its per-class addends carry it
    const_score = cfg.const_score - (10 * sum(int(x) for n, x in prioritizers if n == "NodePreferAvoidPodsPriority")
                                     if tables.get("pa_in_add") else 0) + aux_const
    pods = np.ascontiguousarray(cluster.pods)
    if "CheckServiceAffinity" in predicates:
        ok, need = service_affinity_table(cluster.classes.items or [{}], cluster.label_sets.items, service_affinity)
        tables = dict(tables, svc_ok=ok)
        if len(pods):
            pods = pods.copy()
            pods["flags"] |= np.where(need[pods["cls"]], abi.POD_NEED_SVC_AFFINITY, 0).astype(np.uint32)
    affinity = None
    if cluster.affinity is not None:
        if cfg.predicates & abi.P_INTERPOD_AFFINITY or svc_dyn or \
                ((cfg.weights[abi.W_INTERPOD] or cfg.weights[abi.W_SPREAD] or aux_weight) and not cfg.no_priorities):
            affinity = cluster.affinity
            if cluster.affinity.get("aux_pair") is not None or cluster.affinity.get("svc_on"):
                affinity = dict(cluster.affinity, aux_weight=aux_weight, svc_use=svc_dyn)
        elif len(pods):  # neither MatchInterPodAffinity nor its priority: the terms change nothing
            pods = pods.copy()
            pods["aff_ident"] = 0
            pods["aff_class"] = 0
    volumes = None
    if cluster.volumes is not None:
        if cfg.predicates & VOLUME_PREDICATE_BITS:
            volumes = cluster.volumes
        elif len(pods):  # no volume predicate: the pods' volumes change nothing
            pods = pods.copy()
            pods["vol_class"] = 0
    return Plan(cfg, flags, tables, na_add, const_score, pods, affinity, volumes, "NoVolumeZoneConflict" in predicates)


def _explained(explain):
    return explain is not None and explain is not False


class SweepBuffers:
    """The arrays and ctypes structs of one sweep call over S scenarios and count pods, without a handle:
    out [S][width or count], ctr / sched / rehosted [S], st; weights and absent (absent_mask) as given.
    requeue (a list of queue indices per scenario): off [S + 1] cumulative from 0, pod back to back, pre
    parallel to pod (prefix(): per scenario), rq = byref(abi.SweepRequeue).
    explain (True = the longest prefix + count, or an int cap): fails = dict(count, listed [S], pod [S][cap],
    hist [S][cap][abi.NREASONS]), pod and hist filled with -1, f = byref(abi.SweepFailures).
    residents (the cluster's (node rank, aff_ident, aff_class) rows): res = the rows, then one row per bound
    (queue index, node rank) pair whose pod has an affinity identity or class; rs = abi.SweepResidents.
    outcome: rec = dict(listed, used [S], free_cpu, free_mem [S][abi.OUTCOME_BUCKETS]), oc = byref of it.
    What was not asked for is None."""
    rs = res = rq = off = pod = pre = f = fails = oc = rec = None

    def __init__(self, S, count, weights=None, absent=None, requeue=None, explain=None, residents=None, bound=(),
                 pods=None, outcome=False, width=None):
        i32 = C.c_int32
        self.S = S
        self.weights = None if weights is None else np.ascontiguousarray(weights, np.int64)
        self.absent = absent
        if residents is not None:
            rows = [np.asarray(residents, np.int32).reshape(-1, 3)]
            for q, w in bound:
                p = pods[int(q)]
                if p["aff_ident"] > 0 or p["aff_class"] > 0:
                    rows.append(np.array([[int(w), p["aff_ident"], p["aff_class"]]], np.int32))
            self.res = np.concatenate(rows)
            self._res_cols = [np.ascontiguousarray(self.res[:, k]) for k in range(3)]
            self.rs = abi.SweepResidents(len(self.res), *(abi.ptr(c, i32) for c in self._res_cols))
        if requeue is not None:
            requeue = [np.asarray(list(r), np.int64).reshape(-1) for r in requeue]
            self.off = np.zeros(S + 1, np.int64)
            self.off[1:] = np.cumsum([len(r) for r in requeue])
            self.pod = np.ascontiguousarray(np.concatenate(requeue)) if S and self.off[-1] else np.zeros(0, np.int64)
            self.pre = np.zeros(len(self.pod), np.int32)
            self._rq = abi.SweepRequeue(abi.ptr(self.off, C.c_int64), abi.ptr(self.pod, C.c_int64), abi.ptr(self.pre, i32))
            self.rq = C.byref(self._rq)
        self.out = np.zeros((S, count if width is None else width), np.int32)
        self.ctr, self.sched, self.rehosted = np.zeros(S, np.uint64), np.zeros(S, np.int32), np.zeros(S, np.int32)
        if _explained(explain):
            longest = int(np.diff(self.off).max()) if self.off is not None and S else 0
            cap = longest + count if explain is True else int(explain)
            self.fails = dict(count=np.zeros(S, np.int32), listed=np.zeros(S, np.int32),
                              pod=np.full((S, max(cap, 0)), -1, np.int32),
                              hist=np.full((S, max(cap, 0), abi.NREASONS), -1, np.int32))
            self._f = abi.SweepFailures(cap, *(abi.ptr(self.fails[k], i32) for k in ("count", "listed", "pod", "hist")))
            self.f = C.byref(self._f)
        if outcome:
            self.rec = dict(listed=np.zeros(S, np.int32), used=np.zeros(S, np.int32),
                            free_cpu=np.zeros((S, abi.OUTCOME_BUCKETS), np.int32),
                            free_mem=np.zeros((S, abi.OUTCOME_BUCKETS), np.int32))
            self._oc = abi.SweepOutcome(*(abi.ptr(self.rec[k], i32) for k in ("listed", "used", "free_cpu", "free_mem")))
            self.oc = C.byref(self._oc)
        self.st = abi.Stats()

    def prefix(self):
        return [self.pre[self.off[k]:self.off[k + 1]] for k in range(self.S)]


class GenericScheduler:
    """Batch drop-in for genericScheduler + Scheduler.assume on one MI355X.  label_presence:
    (labels, presence) of a Policy's CheckNodeLabelPresence predicate (policy.key_sets)."""

    def __init__(self, cluster: Cluster, predicates, priorities, device=0, mode=abi.MODE_AUTO,
                 collect_reasons=True, last_node_index=0, label_presence=None, custom_priorities=None,
                 service_affinity=None):
        self.cluster = cluster
        self.predicates = list(predicates)
        self.prioritizers = list(priorities)
        # Policy priorities registered with a labelPreference / serviceAntiAffinity argument, by name
        self.custom_priorities = dict(custom_priorities or {})
        p = self.plan = plan(cluster, predicates, priorities, device, mode, collect_reasons, last_node_index,
                             label_presence, custom_priorities, service_affinity)
        self.cfg = p.cfg
        self.h = abi.Handle(self.cfg)
        table = cluster.node_table()
        if p.flags is not None:
            self._flags = p.flags
            table.flags = abi.ptr(self._flags, C.c_uint32)
        self.h.call("ksim_load_nodes", C.byref(table))
        self.tables, self.na_add, self.const_score = p.tables, p.na_add, p.const_score
        self.h.call("ksim_load_classes", C.byref(class_tables_struct(self.tables, self.na_add)))
        self.affinity = p.affinity
        if self.affinity is not None:
            from .affinity import tables_struct
            self.h.call("ksim_load_affinity", C.byref(tables_struct(self.affinity)))
        self.volumes = p.volumes
        if self.volumes is not None:
            from .volumes import tables_struct as vol_struct
            self.h.call("ksim_load_volumes", C.byref(vol_struct(self.volumes, p.use_zone)))
        pods = self._pods = p.pods
        self.h.call("ksim_load_pods", abi.vptr(pods), len(pods), abi.vptr(cluster.pod_ports), len(cluster.pod_ports),
                    abi.vptr(cluster.pod_scalars), len(cluster.pod_scalars))
        self.last_stats = None

    def volume_state(self):
        """The device's volume slots ([vol_slots][n]) and per-node slot counts."""
        d = self.volumes
        slots = np.zeros_like(d["slots"])
        cnt = np.zeros_like(d["slot_count"])
        self.h.call("ksim_read_volumes", abi.vptr(slots), abi.vptr(cnt))
        return slots, cnt

    def append_pods(self, pods, ports=None, scalars=None):
        """Append descriptors (abi.POD_DTYPE) to the loaded queue (ksim_append_pods): their port /
        scalar offsets index the `ports` / `scalars` arrays passed with them, and their classes must
        be in the loaded class tables.  schedule(first, count) then accepts the new range."""
        pods = np.ascontiguousarray(pods, abi.POD_DTYPE)
        ports = np.zeros(0, np.uint64) if ports is None else np.ascontiguousarray(ports, np.uint64)
        scalars = np.zeros(0, abi.SCALAR_DTYPE) if scalars is None else np.ascontiguousarray(scalars, abi.SCALAR_DTYPE)
        self.h.call("ksim_append_pods", abi.vptr(pods), len(pods), abi.vptr(ports), len(ports), abi.vptr(scalars),
                    len(scalars))
        self._pods = np.concatenate([self._pods, pods])

    @property
    def last_form(self):
        """ksim_last_form: abi.FORM_* bits of the last schedule call's dominant kernel, its rows per
        row thread in bits 8-15; 0 for every kernel but the specialised resource-only one."""
        v = C.c_int32()
        self.h.call("ksim_last_form", C.byref(v))
        return v.value

    def last_plan(self):
        """ksim_last_plan: the launch plan of the last schedule call that ran a general persistent
        kernel, as a dict of abi.PlanInfo's fields (kernel = abi.PLAN_*; all zero after any other path)."""
        v = abi.PlanInfo()
        self.h.call("ksim_last_plan", C.byref(v))
        return {k: getattr(v, k) for k, _ in abi.PlanInfo._fields_ if k != "reserved"}

    def schedule(self, first=0, count=None):
        """Schedule + assume pods [first, first+count) in order.
        Returns (node index per pod (-1 = FitError), reason histograms or None, stats)."""
        n = len(self._pods)
        count = n - first if count is None else count
        out = np.zeros(count, np.int32)
        reasons = np.zeros((count, abi.NREASONS), np.int32) if self.cfg.collect_reasons else None
        st = abi.Stats()
        self.h.call("ksim_schedule", first, count, abi.vptr(out), abi.vptr(reasons), C.byref(st))
        self.last_stats = st
        return out, reasons, st

    def sweep(self, scenarios, first=0, count=None, absent=None, explain=None):
        """Capacity-planning what-if (ksim_sweep): every scenario — a prioritizer list of map
        priorities, e.g. [("LeastRequestedPriority", 3), ("BalancedResourceAllocation", 1)] —
        schedules pods [first, first+count) on its own copy of the current node state, from the
        current lastNodeIndex, with this scheduler's predicates.  The scheduler's own state is
        unchanged.  Returns (placements [n_scen][count], final counters [n_scen], stats).

        absent (ksim_sweep_nodes): one entry per scenario, an iterable of node indices or a
        length-n bool array — the nodes that scenario's snapshot leaves out (node failure, zone
        drain, scale-up candidates not bought).  They are not listed at all: never evaluated,
        counted or selected, and the pods already on them are gone with them; placements stay
        indices of the loaded table.  With absent, scenarios=None runs every scenario under this
        scheduler's own policy.  self.last_scheduled then holds the pods bound per scenario.

        Queues: resource-only pods take the tree or scan form.  Any other range is swept by the
        general form (stats.mode == MODE_PERSISTENT, exact int64, at most
        abi.SWEEP_GENERAL_MAX_NODES nodes): pods with nodeName, host ports, node selectors /
        required node affinity, tolerations, gpu / ephemeral / extended requests, BestEffort pods,
        and with scenarios=None the whole configured policy (TaintToleration, NodeAffinity,
        NodePreferAvoidPods, the constants).  SelectorSpread queues are swept too: on a cluster
        built with SpreadListers whose tables hold spread state only (no pod anywhere with inter-pod
        affinity terms, at most abi.SWEEP_SPREAD_MAX_ZONES zones) every scenario counts the pods of
        a service or controller on its own copy of the counts, and SelectorSpreadPriority /
        ServiceSpreadingPriority reduce over the scenario's fit nodes; scenarios=None only, when the
        policy has a spread weight.  Still refused (KsimUnsupported): a pod in the range
        with inter-pod affinity or volume state, an auxiliary spreading priority or
        CheckServiceAffinity with services selecting the pods, more than abi.MAX_RCLASS reduce
        classes in a pod class, a node-sharded scheduler, a scenario with a reduce priority, and
        explicit scenarios over such a queue when this scheduler's own policy has a reduce
        priority or a NodePreferAvoidPods addend (pass scenarios=None with absent sets).

        explain (ksim_sweep_explain, include/ksim_whatif.h): True keeps the FitError histogram of
        every failed pod of every scenario, an int at most that many per scenario (the first in
        queue order); None or False is the unexplained call.  Placements, counters and stats are
        those of the same sweep without explain, and the return value stays (placements,
        counters, stats).  self.last_failures is then dict(count [n_scen] failed pods (may exceed
        the cap), listed [n_scen] nodes the scenario lists — the N of "0/N nodes are available" —,
        pod [n_scen][cap] index relative to first of the k-th failed pod, hist [n_scen][cap]
        [abi.NREASONS] its histogram over the listed nodes), pod and hist -1 past the
        min(count, cap) kept records; fit_error_message(listed, hist, scalar_names) is the
        reference's text.  A scenario that lists no node fails every pod with an all-zero
        histogram and listed 0 (the reference's ErrNoNodesAvailable).  Works with and without
        absent, with and without scenario weights, in every form."""
        n = len(self._pods)
        count = n - first if count is None else count
        if _explained(explain) or absent is not None:
            return self._sweep_sets(scenarios, first, count, absent, explain)
        b = SweepBuffers(len(scenarios), count, weights=self._sweep_weights(scenarios))
        self.h.call("ksim_sweep", abi.vptr(b.weights), b.S, first, count, abi.vptr(b.out), abi.vptr(b.ctr), C.byref(b.st))
        return self._swept(b, scheduled=False)

    def _sweep_weights(self, scenarios):
        w = np.zeros((len(scenarios), abi.NW), np.int64)
        for k, pri in enumerate(scenarios):
            cfg = make_config(self.predicates, pri)
            if cfg.no_priorities != self.cfg.no_priorities:
                raise Unsupported("a sweep scenario needs a non-empty prioritizer list like the scheduler's")
            w[k] = list(cfg.weights)
        return w

    def _swept(self, b, scheduled=True):
        """After a sweep call over the buffers b: the last_* attributes and the return value."""
        self.last_stats = b.st
        if scheduled:
            self.last_scheduled = b.sched
        if b.fails is not None:
            self.last_failures = b.fails
        if b.rec is not None:
            self.last_outcome = b.rec
        if b.rq is None:
            return b.out, b.ctr, b.st
        self.last_rehosted = b.rehosted
        return b.out, b.prefix(), b.ctr, b.st

    def _sweep_sets(self, scenarios, first, count, absent, explain):
        """sweep with node sets (ksim_sweep_nodes), with records (ksim_sweep_explain), or both."""
        mask = None if absent is None else absent_mask(self.cluster.n_nodes, absent)
        if mask is None and scenarios is None:
            raise abi.KsimError(abi.E_INVAL, "sweep: neither scenarios nor absent sets")
        S = len(scenarios) if mask is None else len(mask)
        if scenarios is not None and len(scenarios) != S:
            raise abi.KsimError(abi.E_INVAL, "sweep: %d scenarios but %d absent sets" % (len(scenarios), S))
        w = None if scenarios is None else self._sweep_weights(scenarios)
        b = SweepBuffers(S, count, weights=w, absent=mask, explain=explain)
        args = (abi.vptr(b.weights), abi.vptr(mask), S, first, count, abi.vptr(b.out), abi.vptr(b.ctr), abi.vptr(b.sched))
        if b.f is None:
            self.h.call("ksim_sweep_nodes", *args, C.byref(b.st))
        else:
            self.h.call("ksim_sweep_explain", *args, b.f, C.byref(b.st))
        return self._swept(b)

    def sweep_drain(self, absent, requeue, first=0, count=None, explain=None):
        """Drain what-if (ksim_sweep_drain, include/ksim_drain.h): sweep(None, absent=...) with a
        prefix queue per scenario.  requeue: one list of loaded-queue indices per scenario — the
        pods re-queued when the scenario's nodes are lost (the requeue_copy of the evicted pods,
        loaded with the queue); scenario s schedules them in that order on its own copy of the node
        state, then pods [first, first+count), all from the current lastNodeIndex.  count=0 only
        re-hosts.  absent None: no node absent in any scenario.  Always the general form
        (stats.mode == MODE_PERSISTENT, at most abi.SWEEP_GENERAL_MAX_NODES nodes) under this
        scheduler's own policy; its refusals (sweep) apply to the re-queued pods as well, and so does
        what it accepts: re-queued pods of a service or controller are swept under SelectorSpread.
        Returns (placements [n_scen][count], requeued — one int32 array per scenario, the node of
        each re-queued pod or -1 —, final counters [n_scen], stats); self.last_scheduled /
        self.last_rehosted hold the pods bound per scenario among the range / the prefix.
        explain: as in sweep; self.last_failures["pod"] then holds positions in the scenario's own
        queue (0 .. len(requeue[s])-1 the prefix, len(requeue[s]) + i range pod first + i) and
        count the failed pods of prefix and range together."""
        return self._sweep_owned("sweep_drain", "ksim_sweep_drain", absent, list(requeue), first, count, explain, None)

    def has_affinity_terms(self):
        """The loaded affinity tables hold an inter-pod affinity term — required, preferred or carried —
        and not SelectorSpread state alone: sweep / sweep_drain refuse such tables, sweep_affinity
        sweeps them."""
        a = self.affinity
        return a is not None and bool(a["n_terms"] or a["n_carry"] or a["n_carries"])

    def sweep_affinity(self, absent, requeue=None, first=0, count=None, explain=None, bound=()):
        """Outage and drain what-ifs over inter-pod affinity queues (ksim_sweep_affinity,
        include/ksim_affsweep.h): sweep(None, absent=...) when requeue is None and sweep_drain(absent,
        requeue, ...) otherwise, on tables that hold inter-pod affinity terms.  Every scenario runs
        under the whole policy — MatchInterPodAffinity, InterPodAffinityPriority and SelectorSpread
        included — on its own copy of the counted pairs and carried terms, from which the placed pods
        on its absent nodes are taken out: the cluster's running pods, and bound, the (queue index,
        node rank) pairs an earlier schedule() on this scheduler committed (every bound pod with
        affinity state must be given, or the call fails with E_INVAL once a count turns negative).
        Returns what sweep returns (requeue None) or what sweep_drain returns; last_scheduled,
        last_rehosted and last_failures as there.  Always the general form.  Refused
        (KsimUnsupported): no affinity tables, volumes on a swept pod, auxiliary or lender tables,
        more than abi.MAX_RCLASS reduce classes, more than abi.SWEEP_SPREAD_MAX_ZONES zones with
        SelectorSpread state, a node-sharded scheduler, more than abi.SWEEP_GENERAL_MAX_NODES nodes."""
        return self._sweep_owned("sweep_affinity", "ksim_sweep_affinity", absent, requeue, first, count, explain, bound)

    def sweep_volumes(self, absent, requeue=None, first=0, count=None, explain=None, bound=()):
        """Outage and drain what-ifs over volume queues (ksim_sweep_volumes, include/ksim_volsweep.h):
        sweep(None, absent=...) when requeue is None and sweep_drain(absent, requeue, ...) otherwise,
        on a scheduler with volume tables, where range and re-queued pods may mount volumes.  Every
        scenario starts from the scheduler's current mounts (as loaded, plus what an earlier schedule()
        committed) in a copy of its own; NoDiskConflict, the MaxPD filters and NoVolumeZoneConflict run
        at their places in the configured order, and a pod that binds adds its mounts to its node in
        that copy.  The mounts of an absent node are never read.  With affinity tables the scenarios
        run under SelectorSpread, MatchInterPodAffinity and InterPodAffinityPriority as in
        sweep_affinity; bound matters only when those tables hold inter-pod affinity terms (the
        residents, as there).  Returns, last_scheduled, last_rehosted and last_failures exactly as
        sweep_affinity.  Always the general form.  KsimError E_OVERFLOW: a scenario's commit found a
        node's volume slots full (the scheduler's own mounts are untouched).  Refused
        (KsimUnsupported): no volume tables, auxiliary or lender tables, more than abi.MAX_RCLASS
        reduce classes, more than abi.SWEEP_SPREAD_MAX_ZONES zones with SelectorSpread state, a
        node-sharded scheduler, more than abi.SWEEP_GENERAL_MAX_NODES nodes."""
        return self._sweep_owned("sweep_volumes", "ksim_sweep_volumes", absent, requeue, first, count, explain, bound)

    def policy_weights(self, scenarios):
        """The weight rows of sweep_policy for this scheduler (policy_rows)."""
        return policy_rows(self.cluster, self.predicates, self.prioritizers, scenarios, self.custom_priorities, self.na_add)

    def sweep_policy(self, scenarios, absent=None, requeue=None, first=0, count=None, explain=None, bound=(),
                     outcome=False):
        """Policy what-ifs under the whole provider (ksim_sweep_policy, include/ksim_polsweep.h): every
        scenario — a prioritizer list, as in sweep, that may weigh TaintToleration, NodeAffinity,
        SelectorSpread and InterPodAffinity as well as the map priorities — schedules its queue on its
        own copy of the node state, spread counts, affinity counts and mounts, under this scheduler's
        predicates.  A scenario may rescale or drop a priority this scheduler's policy has; it cannot
        add a reduce, spread or inter-pod priority the policy lacks (KsimUnsupported: the tables were
        not built), and the addend priorities stay the scheduler's (policy_weights).  absent: one node
        set per scenario (outage x policy), or None; requeue: one prefix list per scenario as in
        sweep_drain, or None; bound: as in sweep_affinity.  Returns what sweep returns, or what
        sweep_drain returns when requeue is given; last_scheduled, last_rehosted and last_failures as
        those calls set them.  outcome=True: self.last_outcome = dict(listed [n_scen], used [n_scen]
        listed nodes holding a pod, free_cpu / free_mem [n_scen][abi.OUTCOME_BUCKETS] listed nodes by
        LeastRequestedPriority's per-resource score of their final state), reduced on the device.
        Always the general form."""
        w = self.policy_weights(scenarios)
        return self._sweep_owned("sweep_policy", "ksim_sweep_policy", absent, requeue, first, count, explain, bound,
                                 weights=w, outcome=outcome)

    def _sweep_owned(self, who, entry, absent, requeue, first, count, explain, bound, weights=None, outcome=False):
        """sweep_drain / sweep_affinity / sweep_volumes / sweep_policy: the entries that take prefix queues.
        bound None (sweep_drain): the entry takes no residents.  weights (sweep_policy): the scenarios' rows,
        which then give the scenario count."""
        n = len(self._pods)
        count = n - first if count is None else count
        mask = None if absent is None else absent_mask(self.cluster.n_nodes, absent)
        if requeue is None and mask is None and weights is None:
            raise abi.KsimError(abi.E_INVAL, "%s: neither absent sets nor re-queue lists" % who)
        S = len(weights) if weights is not None else len(requeue) if requeue is not None else len(mask)
        if requeue is not None and len(requeue) != S:
            raise abi.KsimError(abi.E_INVAL, "%s: %d scenarios but %d re-queue lists" % (who, S, len(requeue)))
        if mask is not None and len(mask) != S:
            raise abi.KsimError(abi.E_INVAL, "%s: %d re-queue lists but %d absent sets" % (who, S, len(mask)))
        b = SweepBuffers(S, count, weights=weights, absent=mask, requeue=requeue, explain=explain, width=max(count, 0),
                         residents=None if bound is None else self.cluster.residents, bound=bound, pods=self._pods,
                         outcome=outcome and weights is not None)
        args = (abi.vptr(mask), S, *(() if b.rs is None else (C.byref(b.rs),)), b.rq, first, count, abi.vptr(b.out),
                abi.vptr(b.ctr), abi.vptr(b.sched), abi.vptr(b.rehosted), b.f)
        if weights is None:
            self.h.call(entry, *args, C.byref(b.st))
        else:
            self.h.call(entry, abi.vptr(b.weights), *args, b.oc, C.byref(b.st))
        return self._swept(b)

    def evaluate(self, pod):
        """Per-node (fit, reason mask, map score, reduce class) for one loaded pod (no commit)."""
        n = self.cluster.n_nodes
        fit = np.zeros(n, np.uint8)
        rs = np.zeros(n, np.uint32)
        sc = np.zeros(n, np.int64)
        rc = np.zeros(n, np.uint8)
        self.h.call("ksim_evaluate", pod, abi.vptr(fit), abi.vptr(rs), abi.vptr(sc), abi.vptr(rc))
        return fit.astype(bool), rs, sc, rc

    def priority_scores(self, pod, over=None):
        """Total priority score per node as PrioritizeNodes reports it (map + reduce + the
        constant priorities) over the node subset `over` (default: fit nodes)."""
        fit, _, sc, rc = self.evaluate(pod)
        idx = np.nonzero(fit)[0] if over is None else np.asarray(over)
        p = self.cluster.pods[pod]
        t = self.tables
        cls = int(p["cls"])
        use_na = bool(self.cfg.weights[abi.W_NODE_AFF]) or self.na_add is not None
        k2 = int(t["n_na"][cls]) if use_na else 1
        tv = t["tt_val"][cls][rc[idx] // k2]
        av = t["na_val"][cls][rc[idx] % k2]
        total = sc[idx].copy()
        if self.cfg.weights[abi.W_TAINT_TOL]:
            total += self.cfg.weights[abi.W_TAINT_TOL] * _normalize(tv, True)
        if self.cfg.weights[abi.W_NODE_AFF]:
            total += self.cfg.weights[abi.W_NODE_AFF] * _normalize(av, False)
        if self.na_add is not None:
            total += self.na_add[cls][rc[idx] % k2]
        return idx, total + self.const_score

    def node_state(self):
        n = self.cluster.n_nodes
        S = self.cluster.cols["alloc_scalar"].shape[0]
        P = self.cluster.port_slots
        out = dict(req_cpu=np.zeros(n, np.int64), req_mem=np.zeros(n, np.int64), req_gpu=np.zeros(n, np.int64),
                   req_eph=np.zeros(n, np.int64), nz_cpu=np.zeros(n, np.int64), nz_mem=np.zeros(n, np.int64),
                   pod_count=np.zeros(n, np.int32), req_scalar=np.zeros((S, n), np.int64),
                   ports=np.zeros((P, n), np.uint64), port_count=np.zeros(n, np.int32))
        st = abi.NodeState()
        for k, ct in (("req_cpu", C.c_int64), ("req_mem", C.c_int64), ("req_gpu", C.c_int64), ("req_eph", C.c_int64),
                      ("nz_cpu", C.c_int64), ("nz_mem", C.c_int64), ("pod_count", C.c_int32),
                      ("req_scalar", C.c_int64), ("ports", C.c_uint64), ("port_count", C.c_int32)):
            setattr(st, k, abi.ptr(out[k], ct))
        self.h.call("ksim_read_nodes", C.byref(st))
        return out

    @property
    def last_node_index(self):
        v = C.c_uint64()
        self.h.call("ksim_get_counter", C.byref(v))
        return v.value

    def close(self):
        self.h.close()


def policy_rows(cluster, predicates, priorities, scenarios, custom_priorities=None, na_add=None):
    """The weight rows of GenericScheduler.sweep_policy, [len(scenarios)][abi.NW], for a scheduler over
    `cluster` with these predicates and priorities (na_add: its per-class addends, Plan.na_add): each
    scenario's prioritizer list through make_config with the cluster's spread flag.  The addends the
    scheduler loaded (NodePreferAvoidPods, ImageLocality and the Policy's label priorities) stay its
    own in every scenario, so a scenario must name every priority folded into them, at the scheduler's
    weight, and none that would need addends the scheduler did not load; where they are constants on
    every node they may differ freely, as every constant may.  Unsupported otherwise, and for an empty
    scenario.  Needs no device."""
    custom = dict(custom_priorities or {})
    folding = {"NodePreferAvoidPodsPriority", "ImageLocalityPriority"} | set(custom)
    own = sorted((n, int(x)) for n, x in priorities if n in folding)
    spread = bool(getattr(cluster, "spread_active", False))
    w = np.zeros((len(scenarios), abi.NW), np.int64)
    for k, pri in enumerate(scenarios):
        pri = list(pri)
        if not pri:
            raise Unsupported("sweep_policy: scenario %d is empty (EqualPriority is no policy to compare)" % k)
        cfg = make_config(predicates, [(n, x) for n, x in pri if n not in custom], spread=spread, configured=pri)
        folded = na_add is not None
        if not folded:  # would this list, on this cluster, need addends?
            folded = class_tables_for(cluster.tables, pri, cluster.label_sets.items, custom)[1] is not None
        if folded and sorted((n, int(x)) for n, x in pri if n in folding) != own:
            raise Unsupported("sweep_policy: scenario %d: %s differ across the nodes here and are folded into the "
                              "scheduler's per-class addends; a scenario must name them at the scheduler's own weights %r"
                              % (k, ", ".join(sorted(folding)), own))
        w[k] = list(cfg.weights)
    return w


def absent_mask(n_nodes, sets):
    """The node sets of ksim_sweep_nodes, packed: uint32 [len(sets)][ceil(n_nodes / 32)], bit
    (j & 31) of word (j >> 5) set = node j (name rank) is absent in that scenario.  Each set is
    an iterable of node indices or a length-n_nodes bool array; an index outside [0, n_nodes)
    raises KsimError(E_INVAL)."""
    n_nodes = int(n_nodes)
    sets = list(sets)
    words = (n_nodes + 31) // 32
    out = np.zeros((len(sets), words), np.uint32)
    for k, a in enumerate(sets):
        a = np.asarray(a if isinstance(a, np.ndarray) else list(a))
        if a.dtype == np.bool_:
            if a.shape != (n_nodes,):
                raise abi.KsimError(abi.E_INVAL, "absent set %d: a bool array must have one entry per node" % k)
            idx = np.nonzero(a)[0]
        elif a.size == 0:
            continue
        else:
            if a.ndim != 1 or a.dtype.kind not in "iu":
                raise abi.KsimError(abi.E_INVAL, "absent set %d: node indices must be integers" % k)
            idx = a.astype(np.int64)
            if idx.min() < 0 or idx.max() >= n_nodes:
                raise abi.KsimError(abi.E_INVAL, "absent set %d: node index outside [0, %d)" % (k, n_nodes))
        np.bitwise_or.at(out[k], idx >> 5, np.uint32(1) << (idx & 31).astype(np.uint32))
    return out


def default_evictable(pod):
    """kubectl drain's rule for a running pod (a v1.Pod object): False for a DaemonSet-owned pod
    (metadata.ownerReferences[].kind == "DaemonSet"), a mirror pod (annotation
    kubernetes.io/config.mirror) and a pod whose status.phase is Succeeded or Failed.  Such pods die
    with their node and are not re-queued."""
    meta = pod.get("metadata") or {}
    if any((o or {}).get("kind") == "DaemonSet" for o in meta.get("ownerReferences") or ()):
        return False
    if "kubernetes.io/config.mirror" in (meta.get("annotations") or {}):
        return False
    return (pod.get("status") or {}).get("phase") not in ("Succeeded", "Failed")


def requeue_copy(pod):
    """The copy of an evicted running pod as a controller would recreate it: spec.nodeName removed,
    status dropped, everything else kept.  The argument is left as it is."""
    import copy
    new = copy.deepcopy({k: v for k, v in pod.items() if k != "status"})
    if isinstance(new.get("spec"), dict):
        new["spec"].pop("nodeName", None)
    return new


def outage_sets(cluster_or_nodes, by):
    """The node sets of the usual outage what-ifs, as [(name, [node indices])] sorted by name.
    by="node": one set per node, named after it; by=<label key>: one set per distinct value of
    that node label, named after the value (nodes without the label are in no set).
    cluster_or_nodes: a Cluster, or a list of v1.Node objects (indices are then their ranks in
    bytewise name order, the order a Cluster built from them loads)."""
    if isinstance(cluster_or_nodes, Cluster):
        cl = cluster_or_nodes
        names = list(cl.names) if cl.names else ["%d" % i for i in range(cl.n_nodes)]
        sets_ = cl.label_sets.items
        labels_ = [sets_[k] for k in np.asarray(cl.cols["label_set"])]
    else:
        nodes = sorted(cluster_or_nodes, key=lambda x: ((x.get("metadata") or {}).get("name", "")).encode())
        names = [(x.get("metadata") or {}).get("name", "") for x in nodes]
        labels_ = [(x.get("metadata") or {}).get("labels") or {} for x in nodes]
    if by == "node":
        return sorted(((nm, [i]) for i, nm in enumerate(names)), key=lambda t: t[0])
    groups = {}
    for i, lab in enumerate(labels_):
        if by in lab:
            groups.setdefault(lab[by], []).append(i)
    return sorted(groups.items(), key=lambda t: t[0])


class ShardedScheduler(GenericScheduler):
    """Rank `rank` of a node-sharded scheduler: loads the contiguous
    name-rank shard [rank*n/world, (rank+1)*n/world) of `cluster` and the whole pod queue;
    all ranks call schedule() with the same ranges.  Connect the ranks first: connect_local
    (ranks driven from this process) or export_handle / connect (one process per device)."""

    def __init__(self, cluster: Cluster, predicates, priorities, rank, world, device=0, collect_reasons=False,
                 last_node_index=0, custom_priorities=None):
        """collect_reasons: each rank's schedule() returns, for every pod no node of the world fits,
        the reason histogram of its own shard; merge_sharded_reasons sums the ranks' into the
        FitError histogram over every node (generic_scheduler.go:51-90 builds FitError from the
        failedPredicateMap of all nodes, :289-378, and every node lies in exactly one shard)."""
        n = cluster.n_nodes
        self.lo, self.hi = rank * n // world, (rank + 1) * n // world
        self.rank, self.world = rank, world
        super().__init__(cluster.shard(self.lo, self.hi), predicates, priorities, device=device,
                         mode=abi.MODE_PERSISTENT, collect_reasons=collect_reasons, last_node_index=last_node_index,
                         custom_priorities=custom_priorities)
        self.full_cluster = cluster
        self.h.call("ksim_shard_setup", rank, world, self.lo)

    def export_handle(self) -> bytes:
        buf = (C.c_uint8 * abi.IPC_HANDLE_BYTES)()
        self.h.call("ksim_shard_export", buf)
        return bytes(buf)

    def connect(self, peer, handle: bytes):
        buf = (C.c_uint8 * abi.IPC_HANDLE_BYTES).from_buffer_copy(handle)
        self.h.call("ksim_shard_connect", peer, buf)

    def connect_local(self, peer, other: "ShardedScheduler"):
        self.h.call("ksim_shard_connect_local", peer, other.h.h)

    def connect_torch(self, dist):
        """Exchange IPC handles with every rank of an initialised torch.distributed group."""
        hs = [None] * self.world
        dist.all_gather_object(hs, self.export_handle())
        for r, hb in enumerate(hs):
            if r != self.rank:
                self.connect(r, hb)


def connect_local_world(scheds):
    """Connect the ranks of a node-sharded scheduler driven from this process."""
    for s in scheds:
        for t in scheds:
            if s is not t:
                s.connect_local(t.rank, t)


def merge_sharded(outs):
    """Per-rank ksim_schedule outputs (-2 = another rank's node) → global placements."""
    return np.max(np.stack(outs), axis=0)


def merge_sharded_reasons(reasons):
    """Per-rank FitError histograms ([pods][KSIM_NREASONS], each over its own shard) → the
    histogram over every node: their sum.  Host-side, once per call (a torch.distributed
    all_reduce(SUM) of the same arrays between processes)."""
    return np.sum(np.stack([np.asarray(r, np.int64) for r in reasons]), axis=0).astype(np.int32)


def _normalize(vals, reverse):
    """NormalizeReduce over a value vector (priorities/reduce.go:29-64)."""
    vals = np.asarray(vals, np.int64)
    mx = int(vals.max()) if len(vals) else 0
    if mx == 0:
        return np.full(len(vals), 10, np.int64) if reverse else vals.copy()
    s = (10 * vals) // mx
    return 10 - s if reverse else s


# ----------------------------------------------------------------------------- simulator
def expand_simulation_pods(spec_list, namespace="", uid=None):
    """ParseSimulationPod (cmd/app/options/options.go:73-99): each SimulationPod's pod deep-copied
    `num` times with UID = name = a fresh uuid, labels replaced by {SimulationName: name} and the
    namespace set.  uid: None → deterministic "<SimulationName>-<i>" (so runs are reproducible);
    "uuid" → uuid4 strings as the reference makes them; or a callable (sp name, i) → str."""
    import copy
    import uuid as _uuid
    out = []
    for sp in spec_list:
        for i in range(int(sp.get("num", 0))):
            if uid is None:
                u = "%s-%d" % (sp["name"], i)
            elif uid == "uuid":
                u = str(_uuid.uuid4())
            else:
                u = uid(sp["name"], i)
            pod = copy.deepcopy(sp.get("pod") or {})
            meta = pod.setdefault("metadata", {})
            meta.update({"uid": u, "name": u, "namespace": namespace, "labels": {"SimulationName": sp["name"]}})
            pod.setdefault("spec", {})
            out.append(pod)
    return out


def load_podspec(path):
    """The --podspec file: a YAML or JSON list of SimulationPod{name, num, pod}
    (pkg/api/api.go:79-83, cmd/app/options/options.go:73-99)."""
    import yaml
    with open(path) as f:
        return yaml.safe_load(f)


def load_checkpoint(nodes_path, pods_path=None):
    """The offline snapshot (pkg/main.go:147-179 getNodeCheckPoint / getPodsCheckPoint): JSON
    arrays of v1.Node and v1.Pod.  Returns (nodes, pods)."""
    import json
    with open(nodes_path) as f:
        nodes = json.load(f)
    pods = []
    if pods_path:
        with open(pods_path) as f:
            pods = json.load(f)
    if not isinstance(nodes, list) or not isinstance(pods, list):
        raise abi.KsimError(abi.E_INVAL, "checkpoint files must hold JSON arrays of v1.Node / v1.Pod")
    return nodes, pods


@dataclass
class Report:
    """The simulation's outcome: (pod, node) in bind order, (pod, FitError text) for failed pods,
    the framework.Status the reference reports from (report.status, pod objects as the
    simulator leaves them) and GetReport's review (report.review)."""
    successful: list = field(default_factory=list)   # (pod name, node name) in bind order
    failed: list = field(default_factory=list)       # (pod name, FitError message)
    stop_reason: str = ""
    stats: object = None
    last_node_index: int = 0
    status: object = None
    review: object = None

    def text(self) -> str:
        """ClusterCapacityReviewPrint's output."""
        from .report import review_text
        return review_text(self.review)


def _placements(cluster, pod_names, row):
    """[(pod name, node name or None)] of a what-if record: row holds a node rank or -1 per pod."""
    names = cluster.names
    return [(pn, names[w] if w >= 0 else None) for pn, w in zip(pod_names, row)]


def _fit_errors(cluster, fails, s, pod_name):
    """listed, explained and fit_errors of scenario s's what-if record from a sweep's last_failures;
    pod_name maps a record's position in the scenario's queue to the pod's name."""
    from .report import ERR_NO_NODES
    listed = int(fails["listed"][s])
    kept = min(int(fails["count"][s]), fails["pod"].shape[1])
    scal = cluster.scalar_names.items
    return dict(listed=listed, explained=kept, fit_errors=[
        (pod_name(int(fails["pod"][s, k])),
         fit_error_message(listed, fails["hist"][s, k], scal) if listed else ERR_NO_NODES)
        for k in range(kept)])


class ClusterCapacity:
    """The simulator (pkg/scheduler/simulator.go:286-342 New, :187-213 Run): nodes and running
    pods of a snapshot, the simulation pods popped LIFO from the expanded podspec list
    (pkg/framework/store/store.go:223-233), each scheduled and committed before the next; a
    provider name, explicit key lists or a Policy (policy.key_sets) configure the algorithm."""

    def __init__(self, nodes, running_pods, simulation_pods, provider_name="DefaultProvider",
                 predicates=None, priorities=None, device=0, mode=abi.MODE_AUTO, collect_reasons=True,
                 policy_obj=None, pvs=(), pvcs=(), storage_classes=(), spread=None):
        label_presence = None
        custom = None
        svc_aff = None
        if policy_obj is not None:
            from .policy import key_sets, priority_arguments, service_affinity_labels
            predicates, priorities, label_presence = key_sets(policy_obj)
            custom = priority_arguments(policy_obj)
            svc_aff = service_affinity_labels(policy_obj)
        if predicates is None or priorities is None:
            p, q = provider(provider_name)
            predicates = p if predicates is None else predicates
            priorities = q if priorities is None else priorities
        self.order = list(reversed(simulation_pods))   # PodQueue.Pop takes the last element
        self.running = list(running_pods)
        self.nodes = list(nodes)
        # pvs / pvcs / storage_classes: the simulator's listers are empty; other callers may fill them
        names = {n for n, _ in priorities}
        both = {"SelectorSpreadPriority", "ServiceSpreadingPriority"} <= names
        saa = [custom[n][1] for n in names if custom and n in custom and custom[n][0] == "serviceAntiAffinity"]
        if both and saa and spread:
            raise Unsupported("ServiceSpreadingPriority next to SelectorSpreadPriority and a serviceAntiAffinity "
                              "priority, with spread listers (one auxiliary spreading priority)")
        # a second spreading priority over the services (include/ksim.h ksim_affinity_tables.aux_*)
        aux = ("service_spreading",) if both else (("service_anti_affinity", saa[0]) if len(saa) == 1 else None)
        # the listers / policy keywords of the cluster, kept for drain_what_if's second cluster
        self._cluster_args = dict(pvs=pvs, pvcs=pvcs, storage_classes=storage_classes, spread=spread,
                                  spread_services_only="ServiceSpreadingPriority" in names and not both,
                                  aux=aux if spread else None,
                                  service_affinity=svc_aff if "CheckServiceAffinity" in predicates else None)
        self.cluster = Cluster.from_objects(nodes, running_pods, self.order, **self._cluster_args)
        self._sched_args = (predicates, priorities, dict(device=device, mode=mode, label_presence=label_presence,
                                                         custom_priorities=custom, service_affinity=svc_aff))
        self.scheduler = GenericScheduler(self.cluster, predicates, priorities, collect_reasons=collect_reasons,
                                          **self._sched_args[2])

    def run(self) -> Report:
        from .report import ERR_NO_NODES, get_report, simulation_status
        rep = Report()
        names = self.cluster.names
        scal = self.cluster.scalar_names.items
        try:
            nodes, reasons, st = self.scheduler.schedule()
            rep.stats = st
            msgs = [None if w >= 0 else (fit_error_message(len(names), reasons[k], scal) if reasons is not None
                                         else "unschedulable") for k, w in enumerate(nodes)]
        except abi.NoNodesAvailable:
            # ErrNoNodesAvailable (generic_scheduler.go:63-64,124-125) for every pod: nothing is
            # ever bound, so each pod in turn fails the same way and goes through Update
            nodes, msgs = np.full(len(self.order), -1, np.int32), [ERR_NO_NODES] * len(self.order)
        rep.last_node_index = self.scheduler.last_node_index
        outcomes = [(names[w] if w >= 0 else None, m) for w, m in zip(nodes, msgs)]
        for k, (node, msg) in enumerate(outcomes):
            name = self.cluster.pod_names[k]
            if node is not None:
                rep.successful.append((name, node))
            else:
                rep.failed.append((name, msg))
        rep.status = simulation_status(self.order, self.running, outcomes)
        rep.stop_reason = rep.status.stop_reason
        rep.review = get_report(rep.status)
        return rep

    @contextlib.contextmanager
    def _own_scheduler(self, cluster):
        """A scheduler of its own over cluster for one what-if sweep, closed afterwards."""
        predicates, priorities, kw = self._sched_args
        g = GenericScheduler(cluster, predicates, priorities, collect_reasons=False, **kw)
        try:
            yield g
        finally:
            g.close()

    def _outage_ranks(self, outages):
        """The sorted node ranks of every (name, node names or indices) outage."""
        cl = self.cluster
        sets_ = []
        for name, members in outages:
            idx = []
            for m in members:
                if isinstance(m, str):
                    if m not in cl.index:
                        raise abi.KsimError(abi.E_INVAL, "outage %r: no node named %r" % (name, m))
                    m = cl.index[m]
                idx.append(int(m))
            sets_.append(sorted(set(idx)))
        return sets_

    def what_if(self, outages, first=0, count=None, explain=False):
        """Node-outage what-ifs over the snapshot (ksim_sweep_nodes): for every outage — (name, node
        names or indices), or the output of outage_sets — the whole queue is scheduled on the
        snapshot without those nodes, under the simulator's own provider or policy, all outages in
        one sweep.  An absent node is not listed at all, and the running pods bound to it disappear
        with it: nothing is re-queued.  The sweep starts from the snapshot as loaded (not from the
        state a run() left), on a scheduler of its own.  Queues with node selectors, tolerations,
        host ports, nodeName and gpu / ephemeral / extended requests are swept under the whole
        provider or policy, and with spread= listers under SelectorSpreadPriority /
        ServiceSpreadingPriority, reduced over each outage's own fit nodes.  A snapshot with inter-pod
        affinity terms (required, preferred, or carried by a running pod) is swept through
        GenericScheduler.sweep_affinity: every outage evaluates MatchInterPodAffinity and
        InterPodAffinityPriority on its own counts, without the running pods of its lost nodes.
        A snapshot with volume state (pods with EBS, GCE PD, Azure disk or PVC volumes under a volume
        predicate; pvs= / pvcs= listers) is swept through GenericScheduler.sweep_volumes: every outage
        evaluates NoDiskConflict, the MaxPD filters and NoVolumeZoneConflict on its own mounts, which
        its binds extend; the mounts of a lost node go with it.  check_volume_support still refuses
        what the reference errs on.
        Returns one record per outage: dict(name, absent (node count), scheduled, failed,
        placements [(pod name, node name or None)] in queue order).
        explain (ksim_sweep_explain): True, or an int cap per outage — each record gains listed (the
        nodes the outage leaves), fit_errors [(pod name, message)] of its failed pods in queue order,
        the message the reference's FitError text over the listed nodes ("0/N nodes are available:
        ...") or report.ERR_NO_NODES when the outage leaves no node, and explained, how many of the
        failed pods fit_errors holds (all of them, or the cap)."""
        cl = self.cluster
        outages = list(outages)
        sets_ = self._outage_ranks(outages)
        if not outages:
            return []
        with self._own_scheduler(cl) as g:
            if g.volumes is not None:  # volume tables: every outage owns its mounts (and its affinity state)
                out, _, _ = g.sweep_volumes(sets_, None, first, count, explain=explain if explain else None)
            elif g.has_affinity_terms():  # inter-pod affinity terms: every outage owns its affinity state
                out, _, _ = g.sweep_affinity(sets_, None, first, count, explain=explain if explain else None)
            else:
                out, _, _ = g.sweep(None, first, count, absent=sets_, explain=explain if explain else None)
            fails = g.last_failures if explain else None
        pod_names = cl.pod_names[first:first + out.shape[1]]
        recs = []
        for s, ((name, _), idx, row) in enumerate(zip(outages, sets_, out)):
            bound = int((row >= 0).sum())
            recs.append(dict(name=name, absent=len(idx), scheduled=bound, failed=len(row) - bound,
                             placements=_placements(cl, pod_names, row)))
            if fails is not None:
                recs[-1].update(_fit_errors(cl, fails, s, lambda k: pod_names[k]))
        return recs

    def policy_what_if(self, policies, outages=None, first=0, count=None, explain=False):
        """Policy what-ifs over the snapshot (ksim_sweep_policy, GenericScheduler.sweep_policy): for
        every policy — (name, prioritizer list) — the whole queue is scheduled on the snapshot under
        the simulator's own predicates and that list, all policies in one sweep, on a scheduler of its
        own that starts from the snapshot as loaded.  A policy may rescale or drop what the
        simulator's provider or policy weighs (TaintToleration, NodeAffinity, SelectorSpread,
        InterPodAffinity and the map priorities at will); what sweep_policy refuses is refused here.
        outages: as in what_if — then one record per (policy, outage) pair, policy-major, still in one
        sweep; an absent node vanishes with its running pods and nothing is re-queued.
        Returns the records of what_if — dict(name (the outage's, None without outages), absent,
        scheduled, failed, placements) and with explain listed, explained, fit_errors — plus policy
        (its name) and the outcome of its final state over the listed nodes: listed, used (nodes
        holding a pod), free_cpu / free_mem (11 counts of nodes by LeastRequestedPriority's
        per-resource score 0..10: how many nodes stay empty or nearly so, and how evenly)."""
        cl = self.cluster
        policies = [(name, list(pri)) for name, pri in policies]
        if not policies:
            return []
        outages = None if outages is None else list(outages)
        if outages is not None and not outages:
            return []
        sets_ = None if outages is None else self._outage_ranks(outages)
        cases = [(pn, pri, None, None) for pn, pri in policies] if outages is None else \
            [(pn, pri, on, idx) for pn, pri in policies for (on, _), idx in zip(outages, sets_)]
        with self._own_scheduler(cl) as g:
            out, _, _ = g.sweep_policy([c[1] for c in cases], None if outages is None else [c[3] for c in cases],
                                       None, first, count, explain=explain if explain else None, outcome=True)
            fails = g.last_failures if explain else None
            oc = g.last_outcome
        pod_names = cl.pod_names[first:first + out.shape[1]]
        recs = []
        for s, ((pn, _, on, idx), row) in enumerate(zip(cases, out)):
            bound = int((row >= 0).sum())
            recs.append(dict(policy=pn, name=on, absent=len(idx or ()), scheduled=bound, failed=len(row) - bound,
                             placements=_placements(cl, pod_names, row),
                             listed=int(oc["listed"][s]), used=int(oc["used"][s]),
                             free_cpu=[int(v) for v in oc["free_cpu"][s]], free_mem=[int(v) for v in oc["free_mem"][s]]))
            if fails is not None:  # (listed stays the outcome's)
                recs[-1].update((k, v) for k, v in _fit_errors(cl, fails, s, lambda k: pod_names[k]).items() if k != "listed")
        return recs

    def drain_what_if(self, outages, first=0, count=None, explain=False, evictable=None):
        """what_if with the pods of the lost nodes re-queued (ksim_sweep_drain): for every outage the
        evictable running pods bound to its nodes are scheduled first, as the copies a controller
        would recreate (requeue_copy) and in the order of running_pods, then the queue — one run of
        the simulator per outage on the snapshot without the outage's nodes and the pods bound to
        them, all outages in one sweep.  evictable: a predicate over a running pod (default
        default_evictable, kubectl drain's rule); a pod it rejects vanishes with its node, as every
        pod does in what_if.  The sweep runs on a cluster of its own — the snapshot's nodes and
        running pods, the queue followed by the copy of every evictable pod on a node of any outage,
        built with the constructor's listers and policy — and on a scheduler of its own.  With spread=
        listers the evicted pods of a service or controller are re-hosted under the spread priority, as
        the queue is, and with inter-pod affinity terms in the snapshot both are swept through
        GenericScheduler.sweep_affinity, as in what_if.  With volume state in the snapshot both are swept
        through GenericScheduler.sweep_volumes: an evicted pod carries its disks to the survivor that
        takes it, where they count for MaxPD and NoDiskConflict against the pods after it.
        first / count select the queue's range as in what_if (count=0: only re-host).
        Returns one record per outage: dict(name, absent (node count), evicted, rehosted, stranded,
        requeued [(pod name, node name or None)] in eviction order, scheduled, failed, placements
        [(pod name, node name or None)] of the queue's range).
        explain: True, or an int cap per outage — each record gains listed, fit_errors [(pod name,
        message)] over the outage's whole queue (evicted pods first, under their original names;
        report.ERR_NO_NODES when the outage leaves no node) and explained, as in what_if."""
        cl = self.cluster
        outages = list(outages)
        if not outages:
            return []
        evictable = default_evictable if evictable is None else evictable
        sets_ = self._outage_ranks(outages)
        nq = len(self.order)
        count = nq - first if count is None else count
        lost = set().union(*sets_)
        evicted = []  # (its node's index, the running pod) of every pod some outage re-queues
        for pod in self.running:
            node = cl.index.get((pod.get("spec") or {}).get("nodeName"))
            if node is not None and node in lost and evictable(pod):
                evicted.append((node, pod))
        copies = [requeue_copy(pod) for _, pod in evicted]
        dcl = Cluster.from_objects(self.nodes, self.running, self.order + copies, **self._cluster_args)
        requeue = [[nq + k for k, (node, _) in enumerate(evicted) if node in set(idx)] for idx in sets_]
        with self._own_scheduler(dcl) as g:
            drain = (g.sweep_volumes if g.volumes is not None else
                     g.sweep_affinity if g.has_affinity_terms() else g.sweep_drain)
            out, pre, _, _ = drain(sets_, requeue, first, count, explain=explain if explain else None)
            fails = g.last_failures if explain else None
        pod_names = dcl.pod_names
        recs = []
        for s, ((name, _), idx, row, rq, got) in enumerate(zip(outages, sets_, out, requeue, pre)):
            bound, back = int((row >= 0).sum()), int((got >= 0).sum())
            recs.append(dict(name=name, absent=len(idx), evicted=len(rq), rehosted=back, stranded=len(rq) - back,
                             requeued=_placements(dcl, [pod_names[q] for q in rq], got),
                             scheduled=bound, failed=len(row) - bound,
                             placements=_placements(dcl, pod_names[first:first + len(row)], row)))
            if fails is not None:
                queue = list(rq) + list(range(first, first + len(row)))  # the outage's own queue, by loaded index
                recs[-1].update(_fit_errors(dcl, fails, s, lambda k: pod_names[queue[k]]))
        return recs
