"""CPU-only tests of the node-outage what-if's host side (ksim_sweep_nodes): the C ABI entry, the
node-set packing, the outage sets and the command line's flags."""
import os
import re

import numpy as np
import pytest

from ksim import abi, cli, ingest, scheduler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sweep_nodes_is_declared_exported_and_listed():
    src = open(os.path.join(ROOT, "include", "ksim.h")).read()
    assert re.search(r"^\s*int\s+ksim_sweep_nodes\(", src, re.M)
    L = abi.lib()
    assert hasattr(L, "ksim_sweep_nodes")
    assert "ksim_sweep_nodes" in abi.EXPORTS
    assert L.ksim_abi_version() == abi.ABI_VERSION == 7


@pytest.mark.parametrize("n", [1, 31, 32, 33, 1500])
def test_absent_mask_bit_layout(n):
    words = (n + 31) // 32
    every = scheduler.absent_mask(n, [range(n), [], [n - 1], np.ones(n, bool), np.zeros(n, bool)])
    assert every.dtype == np.uint32 and every.shape == (5, words)
    # every node: all bits below n, the last word's unused bits zero
    want = np.full(words, 0xFFFFFFFF, np.uint64)
    if n % 32:
        want[-1] = (1 << (n % 32)) - 1
    assert np.array_equal(every[0].astype(np.uint64), want)
    assert np.array_equal(every[3], every[0])
    assert not every[1].any() and not every[4].any()
    last = np.zeros(words, np.uint32)
    last[(n - 1) >> 5] = np.uint32(1) << np.uint32((n - 1) & 31)
    assert np.array_equal(every[2], last)
    for j in (0, 30, 31, 32, 1023, 1024, n - 1):
        if j < n:
            m = scheduler.absent_mask(n, [[j]])[0]
            assert int(m[j >> 5]) == 1 << (j & 31) and int(m.astype(np.uint64).sum()) == 1 << (j & 31)


def test_absent_mask_word_boundary():
    m = scheduler.absent_mask(33, [[31], [32], [31, 32, 31], {0, 32}])
    assert m.tolist() == [[1 << 31, 0], [0, 1], [1 << 31, 1], [1, 1]]


def test_absent_mask_empty_sets_and_no_scenarios():
    assert scheduler.absent_mask(70, [[], (), set(), np.array([], np.int64)]).tolist() == [[0, 0, 0]] * 4
    assert scheduler.absent_mask(70, []).shape == (0, 3)


@pytest.mark.parametrize("bad", [[-1], [40], [0, 40], np.array([2 ** 40]), np.ones(39, bool), [1.5]])
def test_absent_mask_refuses_what_is_not_a_node(bad):
    with pytest.raises(abi.KsimError) as e:
        scheduler.absent_mask(40, [[3], bad])
    assert e.value.code == abi.E_INVAL


def _node(name, labels=None):
    md = {"name": name}
    if labels is not None:
        md["labels"] = labels
    return {"metadata": md, "status": {"allocatable": {"cpu": "4", "memory": "8Gi", "pods": "10"},
                                       "conditions": [{"type": "Ready", "status": "True"}]}}


ZONE = "failure-domain.beta.kubernetes.io/zone"
# given out of name order: indices are ranks in bytewise name order (b-0, b-1, b-10, b-2, b-3)
NODES = [_node("b-2", {ZONE: "z2"}), _node("b-10", {ZONE: "z1", "rack": "r1"}), _node("b-0", {ZONE: "z1"}),
         _node("b-3"), _node("b-1", {"rack": "r1"})]


def _as_cluster(nodes):
    return ingest.Cluster.from_objects(nodes, [], [])


@pytest.mark.parametrize("src", [lambda: NODES, lambda: _as_cluster(NODES)], ids=["objects", "cluster"])
def test_outage_sets(src):
    assert scheduler.outage_sets(src(), "node") == [("b-0", [0]), ("b-1", [1]), ("b-10", [2]), ("b-2", [3]), ("b-3", [4])]
    assert scheduler.outage_sets(src(), ZONE) == [("z1", [0, 2]), ("z2", [3])]
    assert scheduler.outage_sets(src(), "rack") == [("r1", [1, 2])]
    assert scheduler.outage_sets(src(), "no-such-label") == []


def test_outage_sets_feed_absent_mask():
    sets_ = scheduler.outage_sets(NODES, ZONE)
    assert scheduler.absent_mask(len(NODES), [s for _, s in sets_]).tolist() == [[0b00101], [0b01000]]


BASE = ["--podspec", "pod.yaml", "--nodes", "nodes.json"]


def test_cli_accepts_the_what_if_flags():
    a = cli.parse_args(BASE + ["--what-if-outage", ZONE, "--what-if-json"])
    assert a.what_if_outage == ZONE and a.what_if_json is True
    assert cli.parse_args(BASE + ["--what-if-outage", "node"]).what_if_outage == "node"


def test_cli_namespace_without_the_flags_is_the_earlier_one():
    a = vars(cli.parse_args(BASE + ["--pods", "pods.json", "--json"]))
    assert a.pop("what_if_outage") is None and a.pop("what_if_json") is False
    assert a == dict(podspec="pod.yaml", nodes="nodes.json", pods="pods.json", algorithmprovider="DefaultProvider",
                     policy_config_file=None, namespace="", kubeconfig=None, uuid_names=False, json=True, device=0)
