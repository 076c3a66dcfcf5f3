"""The per-pod path's table-level reference and inputs (no device needed to build them).

Mirror steps the C oracle (oracle/cpu_ref.c) one pod per call with carried state, which is what
ksim_schedule_one + the cache-event entry points of include/ksim.h promise to compute; Dut is the
same surface over a GenericScheduler handle; record() runs a step script on the Mirror and keeps
what every call must answer, replay() runs the recorded script on the Dut and compares after every
call; check() is both.  Every comparison is exact.

Steps (tuples; a script may be a generator that reads mirror.placed, it is pulled lazily):
  ("one", k, assume)        ksim_schedule_one of queue pod k (SCHEDULE_ASSUME / SCHEDULE_ONLY)
  ("adapter", k, read)      SCHEDULE_ONLY, then ksim_pod_add onto the answer (Scheduler.assume); read:
                            a ksim_get_counter in between, which undoes the tentative commit first
  ("pod_add", node, k) / ("pod_remove", node, k) / ("node_add", rank, row) / ("node_remove", rank)
  ("counter", v)            ksim_set_counter
  ("sleep", seconds)        the Dut sleeps (the resident kernel's idle leave); the Mirror does nothing
  ("env", name, value)      the Dut's process environment (KSIM_PICK_NPT is read per call); None unsets

The workloads at the bottom return a Case: the ingested cluster, the policy and (where a case has
one) a restatement of how many nodes fit, evaluated on the Mirror's state before the call."""
import ctypes as C
import os
import time

import numpy as np

import cpu_ref
from ksim import abi, ingest, scheduler, spread as kspread, synth
from workloads import rnd_spread_workload, sixteen_class_workload, uniform_selector_workload

DYNAMIC = ("req_cpu", "req_mem", "req_gpu", "req_eph", "nz_cpu", "nz_mem", "pod_count", "req_scalar", "port_count")
STATIC = ("alloc_cpu", "alloc_mem", "alloc_gpu", "alloc_eph", "allowed_pods", "flags", "label_set", "taint_set",
          "alloc_scalar")
ZONE = "failure-domain.beta.kubernetes.io/zone"
REGION = "failure-domain.beta.kubernetes.io/region"
ROW_KEYS = ("alloc_cpu", "alloc_mem", "allowed_pods", "req_cpu", "req_mem", "nz_cpu", "nz_mem", "pod_count")


class Case:
    """One workload: cluster, policy, the fit-count restatement (None: not checked), listers."""

    def __init__(self, cl, preds, prios, fit=None, n_calls=None):
        self.cl, self.preds, self.prios, self.fit = cl, list(preds), list(prios), fit
        self.n_calls = len(cl.pods) if n_calls is None else n_calls


def node_row(alloc_cpu, alloc_mem, allowed_pods, req_cpu=0, req_mem=0, nz_cpu=0, nz_mem=0, pod_count=0):
    """A resource-only node row (no labels, taints, scalars or ports) for node_add."""
    return dict(zip(ROW_KEYS, (alloc_cpu, alloc_mem, allowed_pods, req_cpu, req_mem, nz_cpu, nz_mem, pod_count)))


class Mirror:
    """The reference: a cluster's columns in numpy, lastNodeIndex, the affinity `extra` dict, and
    one cpu_ref.run call per Schedule."""

    def __init__(self, cl, preds, prios, counter=0):
        self.cl, self.preds, self.prios = cl, list(preds), list(prios)
        self.counter = int(counter)
        self.state = cpu_ref._state(cl)
        self.placed = {}            # queue index -> node of the last commit of that pod
        self._replan()
        self.extra = {}
        a = self.plan.affinity
        if a is not None:
            self.extra = {"cnt": np.ascontiguousarray(a["cnt"]).copy(), "carried": np.ascontiguousarray(a["carried"]).copy()}

    def _replan(self):
        self.plan = scheduler.plan(self.cl, self.preds, self.prios)
        self.threads = 1 if self.cl.n_nodes < 20000 else 8

    @property
    def n(self):
        return self.cl.n_nodes

    def schedule(self, k, assume):
        """(node, reasons[32]) of queue pod k; SCHEDULE_ONLY runs on copies, so only the counter moves."""
        assert 0 <= k < len(self.plan.pods)
        st, ex = self.state, self.extra
        if not assume:
            st = {key: v.copy() for key, v in st.items()}
            ex = {key: v.copy() for key, v in ex.items()}
        out, reasons, _, ctr, _ = cpu_ref.run(self.cl, None, first=k, count=1, threads=self.threads, state=st,
                                              counter=self.counter, plan=self.plan, extra=ex)
        self.counter = int(ctr)
        node = int(out[0])
        if assume and node >= 0:
            self.placed[k] = node
        return node, reasons[0].copy()

    def _delta(self, node, k, sign):
        """NodeInfo.AddPod / RemovePod (schedulercache/node_info.go:318-398) of queue pod k."""
        p, s = self.plan.pods[k], self.state
        assert not p["aff_ident"] and not p["aff_class"] and not p["vol_class"] and not p["scalar_cnt"]
        for col, f in (("req_cpu", "add_cpu"), ("req_mem", "add_mem"), ("req_gpu", "add_gpu"), ("req_eph", "add_eph"),
                       ("nz_cpu", "nz_cpu"), ("nz_mem", "nz_mem")):
            s[col][node] += sign * int(p[f])
        s["pod_count"][node] += sign
        keys = [int(x) for x in self.cl.pod_ports[int(p["port_off"]):int(p["port_off"]) + int(p["port_cnt"])]]
        have = [int(x) for x in s["ports"][:s["port_count"][node], node]]
        have = have + [x for x in dict.fromkeys(keys) if x not in have] if sign > 0 else [x for x in have if x not in keys]
        s["ports"][:, node] = 0
        s["ports"][:len(have), node] = have
        s["port_count"][node] = len(have)

    def pod_add(self, node, k):
        self._delta(node, k, 1)
        self.placed[k] = node

    def pod_remove(self, node, k):
        self._delta(node, k, -1)
        self.placed.pop(k, None)

    def _rebuild(self, cols, names):
        """The Cluster again from the edited columns (resource-only nodes), the queue kept."""
        old = self.cl
        cl = synth.resource_cluster(names, cols["alloc_cpu"], cols["alloc_mem"], cols["allowed_pods"], [], [])
        for key in STATIC:
            cl.cols[key] = np.ascontiguousarray(cols[key])
        for key, v in self.state.items():
            cl.cols[key] = v.copy()
        cl.pods, cl.pod_ports, cl.pod_scalars, cl.port_slots = old.pods, old.pod_ports, old.pod_scalars, old.port_slots
        self.cl = cl
        self._replan()

    def node_add(self, rank, row, name=None):
        old = self.cl
        assert not self.extra and not old.cols["label_set"].any() and not old.cols["taint_set"].any()
        cols = {}
        for key in STATIC:
            a = old.cols[key]
            cols[key] = np.insert(a, rank, row.get(key, 0), axis=a.ndim - 1)
        for key, a in self.state.items():
            self.state[key] = np.ascontiguousarray(np.insert(a, rank, row.get(key, 0), axis=a.ndim - 1))
        names = None
        if old.names is not None:
            names = list(old.names)
            names.insert(rank, name)
        self.placed = {k: w + (w >= rank) for k, w in self.placed.items()}
        self._rebuild(cols, names)

    def node_remove(self, rank):
        old = self.cl
        assert not self.extra
        cols = {key: np.delete(old.cols[key], rank, axis=old.cols[key].ndim - 1) for key in STATIC}
        for key, a in self.state.items():
            self.state[key] = np.ascontiguousarray(np.delete(a, rank, axis=a.ndim - 1))
        names = None
        if old.names is not None:
            names = list(old.names)
            del names[rank]
        self.placed = {k: w - (w > rank) for k, w in self.placed.items() if w != rank}
        self._rebuild(cols, names)

    def set_counter(self, v):
        self.counter = int(v)

    def queue(self, desc):
        """Append one descriptor (see resource_desc) to the queue; its index."""
        self.cl.pods = np.concatenate([self.cl.pods, np.asarray(desc, abi.POD_DTYPE).reshape(1)])
        self._replan()
        return len(self.cl.pods) - 1

    def node_state(self):
        return {key: self.state[key] for key in DYNAMIC}


def resource_desc(pod):
    """The descriptor of a pod object that has requests only (class 0, no ports or scalars)."""
    pred, add, nzc, nzm = ingest.container_requests(pod)
    assert not pred.scalar and not ingest.host_ports(pod)
    row = np.zeros(1, abi.POD_DTYPE)
    r = row[0]
    r["req_cpu"], r["req_mem"], r["req_gpu"], r["req_eph"] = pred.cpu, pred.mem, pred.gpu, pred.eph
    r["add_cpu"], r["add_mem"], r["add_gpu"], r["add_eph"] = add.cpu, add.mem, add.gpu, add.eph
    r["nz_cpu"], r["nz_mem"], r["host"] = nzc, nzm, -1
    r["flags"] = (abi.POD_ANY_REQUEST if pred.cpu or pred.mem or pred.gpu or pred.eph else 0) | \
        (abi.POD_BEST_EFFORT if ingest.best_effort(pod) else 0)
    return row


class Dut:
    """The same surface over ksim_schedule_one and the cache-event entry points on one handle."""

    def __init__(self, cl, preds, prios, counter=0):
        self.cl = cl
        self.g = scheduler.GenericScheduler(cl, preds, prios, mode=abi.MODE_LAUNCH, last_node_index=counter)
        self.pods = self.g._pods
        self.S = cl.cols["alloc_scalar"].shape[0]

    def _args(self, k):
        cl = self.cl
        self._pod = abi.Pod.from_buffer_copy(self.pods[k].tobytes())
        return (C.byref(self._pod), abi.vptr(cl.pod_ports), len(cl.pod_ports), abi.vptr(cl.pod_scalars),
                len(cl.pod_scalars))

    def schedule(self, k, assume):
        """(node, lastNodeIndex, reasons[32], fit_nodes)."""
        res = abi.Result()
        self.g.h.call("ksim_schedule_one", *self._args(k), abi.SCHEDULE_ASSUME if assume else abi.SCHEDULE_ONLY,
                      C.byref(res))
        return int(res.node), int(res.last_node_index), np.array(res.reasons[:], np.int32), int(res.fit_nodes)

    def pod_add(self, node, k):
        self.g.h.call("ksim_pod_add", int(node), *self._args(k))

    def pod_remove(self, node, k):
        self.g.h.call("ksim_pod_remove", int(node), *self._args(k))

    def node_add(self, rank, row):
        """The row as ksim/cache.py::_node_row builds it (no labels, taints, scalars or ports)."""
        r = abi.NodeRow()
        for key in ROW_KEYS:
            setattr(r, key, int(row.get(key, 0)))
        z = np.zeros(max(self.S, 1), np.int64)
        r.alloc_scalar, r.req_scalar = abi.ptr(z, C.c_int64), abi.ptr(z, C.c_int64)
        self.g.h.call("ksim_node_add", int(rank), C.byref(r))

    def node_remove(self, rank):
        self.g.h.call("ksim_node_remove", int(rank))

    def set_counter(self, v):
        self.g.h.call("ksim_set_counter", C.c_uint64(int(v)))

    @property
    def counter(self):
        return self.g.last_node_index

    def node_count(self):
        v = C.c_int64()
        self.g.h.call("ksim_node_count", C.byref(v))
        return int(v.value)

    def node_state(self):
        """The dynamic columns but the port keys (their slot count grows inside the library; the
        per-node port count is compared, and what the ports refuse shows in the decisions)."""
        n = self.node_count()
        out = {key: np.zeros((self.S, n) if key == "req_scalar" else n, np.int32 if key in ("pod_count", "port_count")
                             else np.int64) for key in DYNAMIC}
        st = abi.NodeState()
        for key in DYNAMIC:
            setattr(st, key, abi.ptr(out[key], C.c_int32 if out[key].dtype == np.int32 else C.c_int64))
        self.g.h.call("ksim_read_nodes", C.byref(st))
        return out

    def close(self):
        self.g.close()


def record(mirror, steps, fit=None):
    """Run the script on the Mirror: [(step, expectation)] and the final dynamic columns.
    expectation of a Schedule: (node, lastNodeIndex, reasons, fit nodes or None)."""
    out = []
    for st in steps:
        kind = st[0]
        exp = None
        if kind in ("one", "adapter"):
            k = st[1]
            want_fit = None if fit is None else int(fit(mirror, k))
            node, reasons = mirror.schedule(k, kind == "one" and bool(st[2]))
            exp = (node, mirror.counter, reasons, want_fit)
            if kind == "adapter" and node >= 0:
                mirror.pod_add(node, k)
        elif kind == "counter":
            mirror.set_counter(st[1])
        elif kind not in ("sleep", "env"):
            getattr(mirror, kind)(*st[1:])
        out.append((st, exp))
    final = {key: v.copy() for key, v in mirror.node_state().items()}
    final["counter"] = mirror.counter
    return out, final


def replay(dut, recorded, final=None):
    """Run a recorded script on the Dut; after every Schedule the node, lastNodeIndex, the reasons of
    a FitError and (where recorded) fit_nodes must equal the reference's; then the node state."""
    saved = {}  # environment variables the script's "env" steps touched: put back whatever happens
    try:
        for i, (st, exp) in enumerate(recorded):
            kind = st[0]
            if kind in ("one", "adapter"):
                k = st[1]
                node, lni, reasons, fit = dut.schedule(k, kind == "one" and bool(st[2]))
                where = "call %d (%s pod %d)" % (i, kind, k)
                assert node == exp[0], "%s: node %d, reference %d" % (where, node, exp[0])
                assert lni == exp[1], "%s: lastNodeIndex %d, reference %d" % (where, lni, exp[1])
                if node < 0:
                    assert reasons.tolist() == exp[2].tolist(), "%s: FitError reasons" % where
                if exp[3] is not None:
                    assert fit == exp[3], "%s: fit_nodes %d, reference %d" % (where, fit, exp[3])
                if kind == "adapter" and node >= 0:
                    if st[2]:
                        assert dut.counter == exp[1], "%s: ksim_get_counter" % where
                    dut.pod_add(node, k)
            elif kind == "counter":
                dut.set_counter(st[1])
            elif kind == "sleep":
                time.sleep(st[1])
            elif kind == "env":
                saved.setdefault(st[1], os.environ.get(st[1]))
                if st[2] is None:
                    os.environ.pop(st[1], None)
                else:
                    os.environ[st[1]] = st[2]
            else:
                getattr(dut, kind)(*st[1:])
    finally:
        for name, v in saved.items():
            if v is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = v
    if final is not None:
        got = dut.node_state()
        for key in DYNAMIC:
            assert np.array_equal(got[key], final[key]), "node state: %s differs at %s" % (
                key, np.argwhere(got[key] != final[key])[:4].tolist() if got[key].shape == final[key].shape else "shape")
        assert dut.counter == final["counter"], "lastNodeIndex %d, reference %d" % (dut.counter, final["counter"])


def check(dut, mirror, steps, fit=None):
    recorded, final = record(mirror, steps, fit)
    replay(dut, recorded, final)
    return recorded


def assume_all(case, first=0, count=None):
    count = case.n_calls - first if count is None else count
    return [("one", k, True) for k in range(first, first + count)]


# ----------------------------------------------------------------------------- workloads
MI, GI = 1 << 20, 1 << 30
PREDS = list(scheduler.DEFAULT_PREDICATES)
LR_BRA = [("LeastRequestedPriority", 1), ("BalancedResourceAllocation", 1)]


def rotation(n, n_pods=None):
    """n identical nodes (64 cpu, 256Gi, 110 pods), pods of 10m / 1Mi, no priorities: every node
    fits and ties, so call k lands on node (n - 1 - k) mod n and the counter moves every call
    (n > 1).  fit_nodes: n."""
    m = n + 3 if n_pods is None else n_pods
    cl = synth.resource_cluster(None, np.full(n, 64000, np.int64), np.full(n, 256 * GI, np.int64),
                                np.full(n, 110, np.int32), np.full(m, 10, np.int64), np.full(m, MI, np.int64))
    return Case(cl, PREDS, [], fit=lambda mirror, k: mirror.n)


FIXED_RANKS = (0, 1, 62, 63, 64, 65, 255, 256, 257, 511, 512, 513)


def probe_ranks(n, chunk):
    """Ranks from the top (node n - 1 - rank) selectHost's index is aimed at: the fixed wave / block
    edges counted from the top and from the bottom, and both sides of every block boundary (node
    chunk * b) and, inside fat blocks, of every 256-node segment boundary (up to 20,000 nodes)."""
    nodes = set(FIXED_RANKS) | {n - 1 - r for r in FIXED_RANKS} | {0, 1, n - 2, n - 1}
    for b in range(0, (n + chunk - 1) // chunk + 1):
        nodes |= {chunk * b - 1, chunk * b, chunk * b + 1}
    if chunk > 256 and n <= 20000:
        for seg in range(256, n, 256):
            nodes |= {seg - 1, seg, seg + 1}
    return sorted(n - 1 - w for w in nodes if 0 <= w < n)


def probes(n, chunk, wrap_every=1):
    """The rotation cluster with lastNodeIndex set before every call so that selectHost's index
    (lastNodeIndex mod fits, counted from the top: node n - 1 - index) lands on each of
    probe_ranks(n, chunk) — once with the counter equal to the rank, and (every wrap_every-th rank,
    the fixed ranks always) with the largest counter below 2^32 and the smallest one from 2^32 up
    that reach the same index.  Calls alternate SCHEDULE_ASSUME and SCHEDULE_ONLY (all assumed
    from 100,000 nodes up).  Returns (case, steps)."""
    ranks = probe_ranks(n, chunk)
    fixed = set(FIXED_RANKS) | {n - 2, n - 1}
    vals = []
    for j, r in enumerate(ranks):
        vals.append(r)
        if r in fixed or j % wrap_every == 0:
            lo = (2 ** 32 - 1) - ((2 ** 32 - 1 - r) % n)       # the largest v < 2^32 with v mod n == r
            vals += [lo, lo + n]
    case = rotation(n, len(vals))
    steps = []
    for k, v in enumerate(vals):
        steps += [("counter", v), ("one", k, k % 2 == 0 or n >= 100000)]
    return case, steps


def saturate_fit(mirror, k):
    """Nodes with a free pod slot that hold the request (PodFitsResources, predicates.go:709-773)."""
    c, s, p = mirror.cl.cols, mirror.state, mirror.plan.pods[k]
    return int(((s["pod_count"] < c["allowed_pods"]) & (c["alloc_cpu"] - s["req_cpu"] >= p["req_cpu"])
                & (c["alloc_mem"] - s["req_mem"] >= p["req_mem"])).sum())


def saturate(n, seed=31, names=False, n_pods=None, allowed=2):
    """C3-shaped nodes that take 2 pods each and 2n + 40 C3 pods under LeastRequested +
    BalancedResourceAllocation: ties among same-shape nodes in every block, blocks that fit nothing
    while others fit, single-fit calls, then FitErrors whose reasons sum over every block.
    n_pods / allowed: another queue length / pods per node (the revisit cases, which never fill up)."""
    cpu, mem = synth.c3_nodes(n, seed)
    pc, pm = synth.c3_pods(2 * n + 40 if n_pods is None else n_pods, seed)
    nm = ["s-%07d" % (2 * i + 2) for i in range(n)] if names else None
    cl = synth.resource_cluster(nm, cpu.astype(np.int64), mem.astype(np.int64), np.full(n, allowed, np.int32), pc, pm)
    return Case(cl, PREDS, LR_BRA, fit=saturate_fit)


def _default():
    return scheduler.provider("DefaultProvider")


def sixteen(n):
    """workloads.sixteen_class_workload(n): every pod has exactly 16 reduce classes (4 taint counts
    x 4 preferred-affinity weights), selector decoys at both ends; it overflows the cluster."""
    nodes, pods = sixteen_class_workload(n)
    preds, prios = _default()
    return Case(ingest.Cluster.from_objects(nodes, (), pods), preds, prios)


def _tolerating(pod, keys):
    q = {"metadata": dict(pod["metadata"]), "spec": dict(pod["spec"])}
    q["spec"]["tolerations"] = [{"key": k, "operator": "Exists"} if k else {"operator": "Exists"} for k in keys]
    return q


def selector(n, per_kind=1000):
    """Record widths 1 + 2K for K = 2, 1 and 16 on one handle.  The node table is the sixteen-class
    one (0..3 PreferNoSchedule taints taint-0.., four tiers, pool=b decoys at both ends) so that the
    three pod kinds can share it:
      - workloads.uniform_selector_workload's pods (nodeSelector pool=a), tolerating taint-1 and
        taint-2: the intolerable taints number 0 or 1, so 2 reduce classes;
      - rotation-style pods (10m / 1Mi) tolerating everything: 1 reduce class;
      - the sixteen-class pods: 16.
    The queue alternates the three (index 3j, 3j + 1, 3j + 2); selector_order picks from it."""
    nodes, k16 = sixteen_class_workload(n)
    _, sel = uniform_selector_workload(4, per_kind)
    sel = [_tolerating(p, ["taint-1", "taint-2"]) for p in sel]
    plain = [_tolerating({"metadata": {"name": "r-pod-%d" % k, "namespace": "default"},
                          "spec": {"containers": [{"resources": {"requests": {"cpu": "10m", "memory": "1Mi"}}}]}}, [""])
             for k in range(per_kind)]
    pods = [x for t in zip(sel, plain, k16) for x in t]
    preds, prios = _default()
    return Case(ingest.Cluster.from_objects(nodes, (), pods), preds, prios)


def selector_order(alternating=540, cycles=3):
    """Queue indices of the selector mix: `alternating` calls that change the width call by call
    (two tag cycles of 254), then `cycles` times one 16-class pod followed by 253 one-class pods —
    the wide record's words beyond the narrow one's are then read exactly one tag cycle after they
    were last needed, with no wide call of the other 253 in between."""
    order = list(range(alternating))
    wide = (k for k in range(alternating, 10 ** 6) if k % 3 == 2)
    narrow = (k for k in range(alternating, 10 ** 6) if k % 3 == 1)
    for _ in range(cycles):
        order.append(next(wide))
        order += [next(narrow) for _ in range(253)]
    order.append(next(wide))
    return order


def reduce_classes(case):
    """n_tt x n_na of every queue pod (the decision record is 1 + 2K words wide)."""
    t = scheduler.plan(case.cl, case.preds, case.prios).tables
    return (np.asarray(t["n_tt"]) * np.asarray(t["n_na"]))[np.asarray(case.cl.pods["cls"])]


def spread(n, Z, n_pods=200, extra_pods=()):
    """workloads.rnd_spread_workload(3) on n nodes, every node in zone z{i % Z} and no region, with
    its services / RCs / RSs / StatefulSets (SelectorSpread's zone sums: Z of them).  extra_pods
    are queued first (pods no lister selects have no pass A)."""
    nodes, running, pods, objs = rnd_spread_workload(3, n_nodes=n, n_pods=n_pods, n_running=80)
    for i, x in enumerate(nodes):
        lab = x["metadata"]["labels"]
        lab.pop(REGION, None)
        lab[ZONE] = "z%d" % (i % Z)
    preds, prios = _default()
    cl = ingest.Cluster.from_objects(nodes, running, list(extra_pods) + list(reversed(pods)),
                                     spread=kspread.SpreadListers(**objs))
    return Case(cl, preds, prios)


def ports_late(n=2048, m=900, first_block=256, per_node=3):
    """A block that is late by its data: every node from rank `first_block` up runs `per_node` pods
    of 16 host ports each, the nodes below none, and every queued pod brings 16 other host ports —
    so a thread of the first block evaluates PodFitsHostPorts over nothing and a thread of any
    other block over 16 x 48 port pairs, and the first block publishes its record and reads the
    others' before they are written.  No priorities: the pods rotate over the fit nodes, and a node
    that took one refuses the next (its ports), so every block's fit count keeps changing.
    fit_nodes: the nodes that hold no queued pod yet."""
    nodes = [{"metadata": {"name": "l-%05d" % i}, "spec": {},
              "status": {"allocatable": {"cpu": "64", "memory": "256Gi", "pods": "110"},
                         "conditions": [{"type": "Ready", "status": "True"}]}} for i in range(n)]
    running = [{"metadata": {"name": "run-%d-%d" % (i, j), "namespace": "none"},
                "spec": {"nodeName": "l-%05d" % i,
                         "containers": [{"ports": [{"hostPort": 20000 + 16 * j + q, "protocol": "TCP"} for q in range(16)]}]}}
               for i in range(first_block, n) for j in range(per_node)]
    pods = plain_pods(m)
    for p in pods:
        p["spec"]["containers"][0]["ports"] = [{"hostPort": 9000 + q, "protocol": "TCP"} for q in range(16)]
    return Case(ingest.Cluster.from_objects(nodes, running, pods), PREDS, [],
                fit=lambda mirror, k: mirror.n - len(set(mirror.placed.values())))


def zone_count(case):
    """SelectorSpread's zones in the plan's affinity tables (the pass-A record holds 60)."""
    a = scheduler.plan(case.cl, case.preds, case.prios).affinity
    return int(a["n_dom"][a["zone_key"]]) if a is not None and a["zone_key"] >= 0 else 0


def plain_pods(m, prefix="plain"):
    return [{"metadata": {"name": "%s-%d" % (prefix, k), "namespace": "none"},
             "spec": {"containers": [{"resources": {"requests": {"cpu": "10m", "memory": "1Mi"}}}]}} for k in range(m)]


def ports17(n=600, m=60, at=(20, 40)):
    """The rotation cluster's shape as objects with m pods, of which those at `at` carry 17 distinct
    host ports (one more than the resident kernel's message holds): the first lands on the node the
    rotation gives it; nothing else distinguishes nodes, so the second must skip exactly that node."""
    nodes = [{"metadata": {"name": "p-%05d" % i}, "spec": {},
              "status": {"allocatable": {"cpu": "64", "memory": "256Gi", "pods": "110"},
                         "conditions": [{"type": "Ready", "status": "True"}]}} for i in range(n)]
    pods = plain_pods(m)
    for k in at:
        pods[k]["spec"]["containers"][0]["ports"] = [{"hostPort": 9000 + j, "protocol": "TCP"} for j in range(17)]
    def fit(mirror, k):  # a 17-port pod is refused where its ports are taken (PodFitsHostPorts)
        return mirror.n - (int((mirror.state["port_count"] > 0).sum()) if mirror.plan.pods[k]["port_cnt"] else 0)
    return Case(ingest.Cluster.from_objects(nodes, (), pods), PREDS, [], fit=fit)
