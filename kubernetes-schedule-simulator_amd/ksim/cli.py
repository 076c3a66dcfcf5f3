"""k8s-scheduler-simulator's command line over the HIP path.

    python -m ksim.cli --podspec etc/pod.yaml --nodes nodes.json [--pods pods.json]
                       [--algorithmprovider DefaultProvider | --policy-config-file policy.json]
                       [--namespace NS] [--uuid-names] [--json]
                       [--what-if-outage node|LABEL-KEY [--what-if-json]]

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
    ap.add_argument("--what-if-json", action="store_true", help="Print the what-if records as JSON.")
    return ap.parse_args(argv)


def _json_default(o):
    return str(o)


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
    return 0


if __name__ == "__main__":
    sys.exit(main())
