"""k8s-scheduler-simulator's command line over the HIP path.

    python -m ksim.cli --podspec etc/pod.yaml --nodes nodes.json [--pods pods.json]
                       [--algorithmprovider DefaultProvider | --policy-config-file policy.json]
                       [--namespace NS] [--uuid-names] [--json]
                       [--what-if-outage node|LABEL-KEY [--what-if-json]]
                       [--what-if-policy FILE [--what-if-json]]

Reference: cmd/app/server.go:40-110 (flags from cmd/app/options/options.go:64-69, podspec parsing
:73-99, run + ClusterCapacityReviewPrint) and the offline checkpoint path of pkg/main.go:134-179
(nodes.json / pods.json arrays of v1.Node / v1.Pod).  The snapshot comes from the checkpoint
files: listing a live cluster through --kubeconfig needs an API server and is out of scope
(SURVEY.md §8), so that flag is refused rather than ignored.  Pods in pods.json are the
already-running pods (getCheckpoints lists status.phase=Running; here the file is taken as it
is, like anaCheckPoint).  Exit status 1 with a message on every error, like glog.Fatalf.

--what-if-outage KEY adds, after the normal report, the node-outage what-ifs of the snapshot
(ClusterCapacity.what_if): KEY = node removes each node in turn (N-1), any other KEY removes the
nodes of each value of that node label in turn (a zone or rack drain).  One line per outage with
its name, the nodes removed and the pods scheduled and failed; --what-if-json prints the records
as JSON instead.  Snapshots and podspecs with node selectors, tolerations, host ports, nodeName
and extended resources are swept under the whole provider or policy; inter-pod affinity, spread
listers and volumes are refused there (the normal report is printed first either way).

--what-if-policy FILE adds the policy what-ifs of the snapshot (ClusterCapacity.policy_what_if): FILE is
JSON, [{"name": ..., "priorities": [{"name": ..., "weight": ...}]}] — each entry's priorities in the Policy
file's own shape.  Every policy schedules the whole queue under the simulator's predicates and its own
priorities, all in one sweep.  One line per policy with the pods scheduled and failed, the nodes used and
how many nodes end with no more than a tenth, and with at least nine tenths, of their cpu free;
--what-if-json prints the records as JSON instead.
"""
from __future__ import annotations

import argparse
import json
import sys


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="k8s-scheduler-simulator",
                                 description="Simulate kube-scheduler placement of a pod spec on a cluster snapshot (MI355X).")
    ap.add_argument("--podspec", required=True, help="Path to JSON or YAML file containing pod definition.")
    ap.add_argument("--nodes", required=True, help="nodes.json checkpoint: JSON array of v1.Node.")
    ap.add_argument("--pods", default=None, help="pods.json checkpoint: JSON array of running v1.Pod.")
    ap.add_argument("--algorithmprovider", default="DefaultProvider", help="Kubernetes scheduler algorithm provider.")
    ap.add_argument("--policy-config-file", default=None, help="Scheduler Policy file (overrides the provider).")
    ap.add_argument("--namespace", default="", help="Namespace given to the simulation pods.")
    ap.add_argument("--kubeconfig", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--uuid-names", action="store_true", help="Name simulation pods with uuid4s as the reference does.")
    ap.add_argument("--json", action="store_true", help="Print GetReport's review as JSON instead of the tables.")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--what-if-outage", default=None, metavar="KEY",
                    help="After the report, schedule the queue once per outage: KEY = node (each node in turn) or a "
                         "node label key (the nodes of each value in turn).")
    # (absent from the namespace unless given: callers that compare the parsed namespace see the earlier one)
    ap.add_argument("--what-if-policy", default=argparse.SUPPRESS, metavar="FILE",
                    help="After the report, schedule the queue once per policy of FILE: JSON "
                         "[{\"name\": ..., \"priorities\": [{\"name\": ..., \"weight\": ...}]}].")
    ap.add_argument("--what-if-json", action="store_true", help="Print the what-if records as JSON.")
    return ap.parse_args(argv)


def _json_default(o):
    return str(o)


def load_policies(path):
    """The --what-if-policy file as [(name, [(priority name, weight)])]."""
    with open(path) as f:
        doc = json.load(f)
    if not isinstance(doc, list):
        raise ValueError("%s: a JSON list of {name, priorities} is expected" % path)
    out = []
    for k, ent in enumerate(doc):
        if not isinstance(ent, dict) or not isinstance(ent.get("priorities"), list):
            raise ValueError("%s: entry %d: {name, priorities: [...]} is expected" % (path, k))
        pri = []
        for p in ent["priorities"]:
            if not isinstance(p, dict) or "name" not in p or "weight" not in p:
                raise ValueError("%s: entry %d: a priority is {name, weight}" % (path, k))
            if p.get("argument"):
                raise ValueError("%s: entry %d: priority %r carries an argument; policy what-ifs take the "
                                 "priorities of the simulator's own policy by name" % (path, k, p["name"]))
            pri.append((str(p["name"]), int(p["weight"])))
        out.append((str(ent.get("name", "policy-%d" % k)), pri))
    return out


def main(argv=None) -> int:
    a = parse_args(argv)
    from . import scheduler
    from .report import review_text
    if a.kubeconfig:
        print("--kubeconfig: listing a live cluster is not supported; pass --nodes/--pods checkpoint files",
              file=sys.stderr)
        return 1
    try:
        spec = scheduler.load_podspec(a.podspec)
        sim = scheduler.expand_simulation_pods(spec or [], a.namespace, uid="uuid" if a.uuid_names else None)
        nodes, running = scheduler.load_checkpoint(a.nodes, a.pods)
        pol = None
        if a.policy_config_file:
            from . import policy
            pol = policy.load(a.policy_config_file)
        cc = scheduler.ClusterCapacity(nodes, running, sim, provider_name=a.algorithmprovider, policy_obj=pol,
                                       device=a.device)
        rep = cc.run()
        what = None
        if a.what_if_outage:
            what = cc.what_if(scheduler.outage_sets(cc.cluster, a.what_if_outage))
        what_pol = None
        if getattr(a, "what_if_policy", None):
            what_pol = cc.policy_what_if(load_policies(a.what_if_policy))
    except Exception as e:  # glog.Fatalf("Failed to start scheduler simulator: %v", err)
        print("Failed to start scheduler simulator: %s" % e, file=sys.stderr)
        return 1
    if a.json:
        print(json.dumps(rep.review, default=_json_default, indent=1))
    else:
        sys.stdout.write(review_text(rep.review))
    if what is not None:
        if a.what_if_json:
            print(json.dumps(what, default=_json_default, indent=1))
        else:
            for r in what:
                print("what-if outage %s: nodes removed %d, scheduled %d, failed %d"
                      % (r["name"], r["absent"], r["scheduled"], r["failed"]))
    if what_pol is not None:
        if a.what_if_json:
            print(json.dumps(what_pol, default=_json_default, indent=1))
        else:
            for r in what_pol:
                print("what-if policy %s: scheduled %d, failed %d, nodes used %d of %d, cpu nearly full %d, nearly empty %d"
                      % (r["policy"], r["scheduled"], r["failed"], r["used"], r["listed"], sum(r["free_cpu"][:2]),
                         sum(r["free_cpu"][9:])))
    return 0


if __name__ == "__main__":
    sys.exit(main())
