"""The step between a stage and the next iteration's graph: host order and outputs against the
device ones (pipeline.run's resident=True sequence against resident="device").

    python tools/resident_loop.py [out.json] [--workloads c4,c3] [--order-only c4]

On this box, host clock around a device synchronise (every step synchronises inside), median of
5 after one warm run:
  * gtf.pipeline.run on the committed vol-7 event (tests/golden/kat134), three iterations, with
    resident=False, True and "device": the whole loop, and per iteration the median of the
    host-visible seconds pipeline.run records (stage / extract / next). resident=True is the code
    of the parent commit, unchanged, so its figure here is the comparison base on this box.
  * per synthetic workload (C4, C3, seed 3 -- tools/graph_subset.py's inputs and seeded mask, the
    nodes renumbered subgraph by subgraph as the extraction needs them, node ids that repeat
    replaced by 0 .. N - 1 as the device order needs them), after one fused pass
    has left an activation mask: from the finished stage to a ready child DeviceGraph,
      old: download, extract.candidate_order, extract.run, extract.outputs, DeviceGraph.subset of
           the host mask + refresh_send_mw, to_host;
      new: extract.candidate_order_dev, run_dev, outputs_dev, DeviceGraph.subset of the device
           mask with vivl carried + refresh_send_mw;
    whole and per call. extract.outputs compares every node with every subgraph and every
    extracted candidate (a Python loop of O(N) NumPy calls): where that is over 5e10 element
    compares it is not run, and the old sequence is reported without it (the JSON says so).
  * what gtf_candidate_order_device met on the workload: components, set-ordered ones and the
    largest (each walked by one thread), with the call's time.
--order-only NAME: just the order call on that workload, ten times (to run under a kernel trace,
which gives the one-thread walk kernel k_ord_walk's own time).
Prints one JSON line (times in milliseconds)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gnn-track-finding_amd"), os.path.join(ROOT, "tools")]
import torch  # noqa: E402
from gtf import device as dev, extract, graph, pipeline, synth  # noqa: E402
from gtf.params import Params  # noqa: E402
from graph_subset import PREFIX, seeded_mask  # noqa: E402

RUNS = 5
OUTPUTS_LIMIT = 5e10


def _ms(fn, runs=RUNS):
    fn()
    ts = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "runs": runs}


def pipeline_vol7():
    g, vivl = pipeline.build_event(PREFIX, 7, 7, Params())
    out = {"n_nodes": g.n_nodes, "n_slots": g.n_slots}
    for name, mode in (("host", False), ("resident", True), ("device", "device")):
        recs = []

        def loop():
            recs.append(pipeline.run(g.copy(), vivl, iterations=3, resident=mode))
        r = _ms(loop)
        per_it = []
        for i in range(3):
            runs = [x[i].seconds for x in recs[1:]]
            per_it.append({k: statistics.median(s[k] for s in runs) * 1e3 for k in ("stage", "extract", "next")})
            per_it[-1]["total"] = statistics.median(sum(s.values()) for s in runs) * 1e3
        out[name] = {"loop": r, "iterations": per_it}
    return out


def staged(name):
    """the workload on the device after one fused pass, its vivl and the seeded mask"""
    g = synth.workload(name, seed=3)
    # the extraction wants the nodes grouped by subgraph, as pack() numbers them (the synthetic
    # event is not): the same graph renumbered
    g, _ = graph.renumber(g, np.argsort(g.node["sub_id"], kind="stable"))
    graph.refresh_send_mw(g)
    keep = seeded_mask(g)
    # the device order wants distinct node ids (as the event builder); a synthetic event whose
    # ids repeat gets 0 .. N - 1
    renumbered = np.unique(g.node["node_id"]).size < g.n_nodes
    if renumbered:
        g.node["node_id"] = np.arange(g.n_nodes, dtype=np.int64)
    d = dev.DeviceGraph(g, "cuda:0", tables="device")
    d.fresh_node_ids = bool(renumbered)
    d.clear_errors()
    d.full_pass(Params())
    torch.cuda.synchronize()
    vivl = np.stack([np.full(g.n_nodes, 8.0), np.nan_to_num(g.node["layer"].astype(np.float64))], 1)
    return g, d, vivl, keep


def workload(name):
    g, d, vivl, keep = staged(name)
    ex = extract.Params()
    scratch = g.copy()
    keep_dev = d._dev_from(keep.astype(np.uint8))
    vivl_dev = d._dev_from(vivl)
    d.node_id_dev()
    s = {}       # what one call leaves for the next

    def download():
        d.download(scratch)

    def host_order():
        s["order"] = extract.candidate_order(scratch)

    def host_run():
        s["res"] = extract.run(scratch, vivl, ex, order_key=s["order"], d=d)

    def host_outputs():
        s["out"] = extract.outputs(scratch, s["res"], ex.numhits, s["order"])

    def host_subset():
        s["child"] = d.subset(keep, gnn=s["res"]["gnn"])
        s["child"].refresh_send_mw()

    def to_host():
        s["child"].to_host(scratch)

    def dev_order():
        s["cnt"] = {}
        s["order_dev"] = extract.candidate_order_dev(d, s["cnt"])

    def dev_run():
        s["res_dev"] = extract.run_dev(d, vivl_dev, ex, s["order_dev"])

    def dev_outputs():
        s["out_dev"] = extract.outputs_dev(d, s["res_dev"], ex.numhits, ids=True)

    def dev_subset():
        s["child_dev"] = d.subset(keep_dev, gnn=s["res_dev"]["gnn"], carry={"vivl": vivl_dev})
        s["child_dev"].refresh_send_mw()

    r = {"n_nodes": g.n_nodes, "n_slots": g.n_slots, "n_edges": g.n_edges, "n_sub": d.n_sub,
         "kept_nodes": int(keep.sum()), "node_ids_replaced": d.fresh_node_ids}
    new = [("order", dev_order), ("extraction", dev_run), ("outputs", dev_outputs), ("subset", dev_subset)]
    r["new_parts"] = {k: _ms(f) for k, f in new}
    r["new"] = _ms(lambda: [f() for _, f in new])
    r["order_counts"] = s["cnt"]
    n_ext = len(s["out_dev"]["extracted"])
    r["extraction"] = {"n_candidates": int(d._np(s["res_dev"]["ncand"])[0]), "n_extracted": n_ext,
                       "n_remaining": len(s["out_dev"]["remaining"]), "n_fragments": len(s["out_dev"]["fragments"])}
    work = float(g.n_nodes) * (d.n_sub + n_ext)
    old = [("download", download), ("order", host_order), ("extraction", host_run), ("outputs", host_outputs),
           ("subset", host_subset), ("to_host", to_host)]
    if work > OUTPUTS_LIMIT:
        old = [x for x in old if x[0] != "outputs"]
        r["old_outputs_skipped"] = "extract.outputs: %.1e element compares (nodes x (subgraphs + extracted))" % work
    r["old_parts"] = {k: _ms(f) for k, f in old}
    r["old"] = _ms(lambda: [f() for _, f in old])
    if "out" in s:
        same = all(len(s["out"][k]) == len(s["out_dev"][k]) for k in ("extracted", "remaining", "fragments"))
        r["same_output_counts"] = bool(same and np.array_equal(s["order"], d._np(s["order_dev"])[:g.n_nodes]))
    r["old_over_new"] = r["old"]["median_ms"] / r["new"]["median_ms"]
    return r


def order_only(name):
    _, d, _, _ = staged(name)
    cnt = {}
    for _ in range(10):
        extract.candidate_order_dev(d, cnt)
    torch.cuda.synchronize()
    return {"workload": name, "order_counts": cnt}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--workloads", default="c4,c3")
    ap.add_argument("--order-only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resident_loop.py needs the MI355X")
    if a.order_only:
        print(json.dumps(order_only(a.order_only)))
        return
    res = {"tool": "resident_loop", "device": torch.cuda.get_device_name(0), "pipeline_vol7": pipeline_vol7(),
           "workloads": {}}
    for name in [w for w in a.workloads.split(",") if w]:
        res["workloads"][name] = workload(name)
    s = json.dumps(res)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
