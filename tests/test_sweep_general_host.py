"""CPU-only tests of the scenario sweep's general form: the node cap mirrored in the binding, the
header's account of which pods ksim_sweep / ksim_sweep_nodes take, and the unchanged C ABI."""
import os
import re

from ksim import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ksim.h")
SWEEP_H = os.path.join(ROOT, "kubernetes-schedule-simulator_amd", "csrc", "ksim_sweep.h")


def _comment_before(src, decl):
    """The block comment that ends right before the declaration."""
    end = src.index(decl)
    start = src.rindex("/*", 0, end)
    assert src[start:end].rstrip().endswith("*/")
    return " ".join(src[start:end].replace("*", " ").split())


def test_node_cap_is_mirrored():
    m = re.search(r"^#define\s+KSIM_SWEEP_GENERAL_MAX_NODES\s+(\d+)", open(SWEEP_H).read(), re.M)
    assert m and int(m.group(1)) == abi.SWEEP_GENERAL_MAX_NODES == 38400
    # one uint32 per node within 150 KiB of LDS
    assert abi.SWEEP_GENERAL_MAX_NODES * 4 == 150 * 1024
    text = _comment_before(open(HEADER).read(), "int ksim_sweep(")
    assert "38,400" in text and "KSIM_SWEEP_GENERAL_MAX_NODES" in text


def test_header_no_longer_requires_resource_only_pods():
    src = open(HEADER).read()
    for decl in ("int ksim_sweep(", "int ksim_sweep_nodes("):
        text = _comment_before(src, decl)
        assert "must be resource-only" not in text, decl
    sweep = _comment_before(src, "int ksim_sweep(")
    for word in ("host ports", "tolerations", "nodeName", "inter-pod affinity", "volume", "node-sharded",
                 "KSIM_MAX_RCLASS", "NodePreferAvoidPods"):
        assert word in sweep, word
    assert "general form" in _comment_before(src, "int ksim_sweep_nodes(")


def test_abi_is_unchanged():
    L = abi.lib()
    assert L.ksim_abi_version() == abi.ABI_VERSION == 7
    assert "ksim_sweep" in abi.EXPORTS and "ksim_sweep_nodes" in abi.EXPORTS
    assert not any("general" in name for name in abi.EXPORTS)
    assert len(abi.EXPORTS) == len(set(abi.EXPORTS)) == 32
    for name in abi.EXPORTS:
        assert hasattr(L, name), name
