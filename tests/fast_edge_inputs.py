"""Input builders for the float64 fast path's edge tests (pure numpy, no device): clusters whose
nodes sit exactly on a LeastRequested / MostRequested score boundary, on a
BalancedResourceAllocation truncation boundary that one ulp of either quotient decides, or on a
degenerate row (zero capacity, request == capacity, capacity 1).

Every pod requests (1, 1) unless stated; the node pre-state is written straight into the cluster's
req / nz columns.  Every quantity and every sum a run reaches stays below 2^48, so the float64
kernels (csrc/ksim_f64.h) never hand over to the int64 ones.

The score expressions restated (reference: priorities/least_requested.go:44-53,
most_requested.go:45-55, balanced_resource_allocation.go:39-61):
  LR  = (floor((cap_c - t_c) * 10 / cap_c) + floor((cap_m - t_m) * 10 / cap_m)) / 2
  MR  = (floor(t_c * 10 / cap_c) + floor(t_m * 10 / cap_m)) / 2
  BRA = int((1 - |t_c / cap_c - t_m / cap_m|) * 10) in float64, 0 when a fraction is >= 1
with t = the node's non-zero requested + the pod's."""
import numpy as np

from ksim import abi, scheduler, synth

PREDS = list(scheduler.DEFAULT_PREDICATES)
LR = [("LeastRequestedPriority", 1)]
MR = [("MostRequestedPriority", 1)]
BRA = [("BalancedResourceAllocation", 1)]
LR_BRA = [("LeastRequestedPriority", 1), ("BalancedResourceAllocation", 1)]
LR_MR_BRA = [("LeastRequestedPriority", 2), ("MostRequestedPriority", 1), ("BalancedResourceAllocation", 3)]

EDGE_CAPS = [20, 999, 1000, 1001, 2 ** 20 + 1, 3 * 2 ** 30, 10 ** 12 + 39, 2 ** 47 - 1, 2 ** 47 + 12345, 2 ** 48 - 1]
ULP_CAPS = [10, 1000, 10 * (2 ** 20 + 1), 30 * 2 ** 30, 10 * (10 ** 11 + 3), 10 * ((2 ** 47 - 1) // 10),
            10 * ((2 ** 48 - 1) // 10)]
# Multiples of 10 at which, for some k, RN(float(k * cap) * RN(1 / cap)) falls below the exact
# quotient k: the truncated estimate is k - 1 and only the remainder correction of the float64
# floor division (kf64::div_floor) restores k.  The EDGE_CAPS totals never need that correction.
EXACT_POOL = [850, 1370, 1450, 1470, 1530, 1700, 1790, 3630, 3770, 4090, 7260, 8130, 16260, 32520, 61130,
              1728531940, 1809709250, 1827183590, 1978980090, 2123195060, 2132348380,
              1596574513930, 1950865809940, 1986698047550, 2116335607100, 2157645398800,
              163012329274030, 223350937846450, 257492359786250, 269178734737690, 273775071924090, 278946300213390]
STATE_KEYS = ("req_cpu", "req_mem", "nz_cpu", "nz_mem", "pod_count")


def _cluster(prefix, cpu, mem, allowed, n_pods, pre_cpu, pre_mem):
    """Resource cluster of (1, 1) pods whose nodes start at req = nz = (pre_cpu, pre_mem)."""
    n = len(cpu)
    names = ["%s-%04d" % (prefix, i) for i in range(n)]
    cl = synth.resource_cluster(names, np.asarray(cpu, np.int64), np.asarray(mem, np.int64),
                                np.full(n, allowed, np.int32), np.ones(n_pods, np.int64), np.ones(n_pods, np.int64))
    for k, v in (("req_cpu", pre_cpu), ("nz_cpu", pre_cpu), ("req_mem", pre_mem), ("nz_mem", pre_mem)):
        cl.cols[k][:] = np.asarray(v, np.int64)
    return cl


def truncates_low(cap, k):
    """The float64 estimate of (k * cap) / cap truncates to k - 1."""
    return int(float(k * cap) * (1.0 / float(cap))) == k - 1


def _edge_caps(seed, n, exact_k=None):
    """Capacities per node from EDGE_CAPS; with exact_k, every second node from the EXACT_POOL
    entries that truncate low at k instead (the others keep the tie set honest)."""
    r = synth.splitmix64(seed, 2 * n)
    cpu, mem = synth._pick(r[:n], EDGE_CAPS).astype(np.int64), synth._pick(r[n:], EDGE_CAPS).astype(np.int64)
    if exact_k is not None:
        low = [c for c in EXACT_POOL if truncates_low(c, exact_k)]
        cpu[0::2] = synth._pick(r[:n] >> np.uint64(9), low)[0::2]
        mem[0::2] = synth._pick(r[n:] >> np.uint64(9), low)[0::2]
    return cpu, mem


def _ceil_tenths(k, cap):
    return -((-k * cap) // 10)  # ceil(k * cap / 10), exact in int64 (9 * 2^48 < 2^63)


def lr_edge_cluster(k, n=130, n_pods=390, exact=False):
    """Every node one unit below the largest total that still scores k under LeastRequested: with
    the (1, 1) pod it scores exactly k, with one more unit k - 1.  All n nodes tie at the maximum
    and each commit takes exactly one node out of the tie set.  exact: every second node on
    capacities where (cap - t) * 10 is exactly k * cap and the float64 estimate truncates low."""
    cpu, mem = _edge_caps((300 if exact else 100) + k, n, k if exact else None)
    tc, tm = cpu - _ceil_tenths(k, cpu), mem - _ceil_tenths(k, mem)
    return _cluster(("lx%d" if exact else "lr%d") % k, cpu, mem, 110, n_pods, tc - 1, tm - 1)


def mr_edge_cluster(k, n=130, n_pods=390, exact=False):
    """Every node one unit below the smallest total that scores k under MostRequested (exact: as
    lr_edge_cluster)."""
    cpu, mem = _edge_caps((400 if exact else 200) + k, n, k if exact else None)
    return _cluster(("mx%d" if exact else "mr%d") % k, cpu, mem, 5, n_pods, _ceil_tenths(k, cpu) - 1,
                    _ceil_tenths(k, mem) - 1)


def bra_score(tc, cc, tm, cm):
    """BalancedResourceAllocation's expression in float64 (Python floats), capacities non-zero."""
    fc, fm = float(tc) / float(cc), float(tm) / float(cm)
    return 0 if fc >= 1.0 or fm >= 1.0 else int((1.0 - abs(fc - fm)) * 10.0)


def ulp_family():
    """(cc, cm, tc, tm) with the pod added: tc = cc/10 * p and tm = cm/10 * (p + j), and the same
    with cpu and memory swapped, p = 1..9, j = 0..9-p: the fractions differ by exactly j/10 as
    rationals, so float rounding alone decides between a score of 10 - j and 9 - j."""
    out = []
    for cc in ULP_CAPS:
        for cm in ULP_CAPS:
            for p in range(1, 10):
                for j in range(0, 10 - p):
                    out.append((cc, cm, cc // 10 * p, cm // 10 * (p + j)))
                    if j:
                        out.append((cc, cm, cc // 10 * (p + j), cm // 10 * p))
    return out


def _ulp_cluster(prefix, rows, n_pods=None):
    cc, cm, tc, tm = (np.array([r[k] for r in rows], np.int64) for k in range(4))
    return _cluster(prefix, cc, cm, 110, 3 * len(rows) if n_pods is None else n_pods, tc - 1, tm - 1)


def bra_ulp_clusters(max_nodes=260):
    """The ulp family grouped by true score, one cluster per (score, chunk of <= max_nodes
    combinations), each at least 65 nodes (combinations repeated to fill): [(score, cluster)].
    Within a cluster every node ties for the first pod."""
    groups = {}
    for r in ulp_family():
        groups.setdefault(bra_score(r[2], r[0], r[3], r[1]), []).append(r)
    out = []
    for s in sorted(groups):
        g = groups[s]
        for c0 in range(0, len(g), max_nodes):
            rows = g[c0:c0 + max_nodes]
            while len(rows) < 65:
                rows = rows + g[:65 - len(rows)]
            out.append((s, _ulp_cluster("u%02d-%02d" % (s, c0 // max_nodes), rows)))
    return out


def ulp_mixed_clusters(n=300):
    """LR + BRA parity runs over the family across its score groups: two strided samples of the
    union (offsets 0 and half a stride), n nodes each."""
    fam = ulp_family()
    step = len(fam) // n
    return [_ulp_cluster("um%d" % k, fam[off::step][:n]) for k, off in enumerate((0, step // 2))]


def degenerate_cluster(n=120):
    """Zero cpu / memory / both capacities, capacity 1, request == capacity after the pod, a few
    memory-pressure and NotReady nodes, 3 pods per node at most so the cluster fills; the queue
    alternates a BestEffort class (no requests, the non-zero defaults) with the (1, 1) class."""
    cpu, mem = synth.c3_nodes(n, 41)
    cpu, mem = cpu.astype(np.int64), mem.astype(np.int64)
    pre_c, pre_m = np.zeros(n, np.int64), np.zeros(n, np.int64)
    cpu[0::12] = 0
    mem[1::12] = 0
    cpu[2::12] = 0
    mem[2::12] = 0
    cpu[3::12] = 1          # capacity 1 = the pod's request
    mem[3::12] = 1
    cpu[4::12] = 1000       # request == capacity once the pod is added
    pre_c[4::12] = 999
    mem[5::12] = 2 ** 47 + 12345
    pre_m[5::12] = 2 ** 47 + 12344
    cl = _cluster("dg", cpu, mem, 3, 3 * n, pre_c, pre_m)
    be = np.arange(3 * n) % 2 == 0
    for f in ("req_cpu", "req_mem", "add_cpu", "add_mem"):
        cl.pods[f][be] = 0
    cl.pods["flags"][be] = abi.POD_BEST_EFFORT
    cl.pods["nz_cpu"][be] = 100
    cl.pods["nz_mem"][be] = 200 * 2 ** 20
    cl.cols["flags"][6::24] |= abi.N_MEM_PRESSURE
    cl.cols["flags"][7::36] |= abi.N_NOT_READY
    return cl


def all_edge_cases():
    """[(id, cluster, priorities)] — every cluster of this module with the policy it is built for."""
    out = [("lr%d" % k, lr_edge_cluster(k), LR) for k in range(1, 10)]
    out += [("mr%d" % k, mr_edge_cluster(k), MR) for k in range(1, 10)]
    out += [("lx%d" % k, lr_edge_cluster(k, exact=True), LR) for k in range(1, 10)]
    out += [("mx%d" % k, mr_edge_cluster(k, exact=True), MR) for k in range(1, 10)]
    out += [(cl.names[0][:-5], cl, BRA) for _, cl in bra_ulp_clusters()]
    out += [(cl.names[0][:-5], cl, LR_BRA) for cl in ulp_mixed_clusters()]
    out.append(("degenerate", degenerate_cluster(), LR_MR_BRA))
    return out
