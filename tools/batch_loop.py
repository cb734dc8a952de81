"""The resident loop on a batch of events against the same events one after another.

    python tools/batch_loop.py [out.json] [--copies 1,8,64] [--runs 5]

K copies of the committed vol-7 event (tests/golden/kat134), each built in GPU memory as
pipeline.build_event_dev builds it (the CSV files are parsed once, on the host, outside every timed
window). Timed from K resident events to the last iteration's records, three iterations, host clock
around a device synchronise (every step synchronises inside), one warm round and then the median of
`runs` rounds; a round times both modes, one after the other, on the same box:
  * sequential: pipeline.run(d, None, resident="device") on each of the K events in turn -- the loop
    of the parent commit, unchanged. run() works on the event itself, so every round gets K freshly
    built events (built before the clock starts).
  * batch: pipeline.run_batch(ds) -- DeviceGraph.concat, ONE loop on the fused graph, gtf_event_split
    per iteration. run_batch does not modify its inputs: the same K events serve every round.
Both give every event's 1,055 / 110 / 2 candidates (checked on every round). Also timed on their
own, between device synchronises: DeviceGraph.concat of the K events (gtf_graph_concat,
gtf_concat_columns, gtf_graph_prepare and the Python around them) and extract.split_dev
(gtf_event_split and its small download) on the first iteration's outputs of the fused graph.
Prints one JSON line (times in milliseconds)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gnn-track-finding_amd")]
import torch  # noqa: E402
from gtf import extract, io, pipeline  # noqa: E402
from gtf.device import DeviceGraph  # noqa: E402
from gtf.params import Params  # noqa: E402

PREFIX = os.path.join(ROOT, "tests", "golden", "kat134", "event_1_filtered_graph_")
EXPECT = [1055, 110, 2]


def _stats(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "runs": len(ts)}


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def columns():
    ids, x, y, z, r, layer = io.read_nodes(PREFIX + "nodes.csv", 7, 7)
    n2, n1 = io.read_edges(PREFIX + "edges.csv")
    return ids, x, y, z, r, layer, n1, n2


def build(cols, p):
    """pipeline.build_event_dev from the parsed columns"""
    d = DeviceGraph.from_event(*cols)
    d.clear_errors()
    d.track_state_estimates(p)
    d.node_ops(["priors_tse", "mw_tse", "degree"], p)
    d.raise_errors()
    d.refresh_send_mw()
    return d


def _check(records):
    for recs in records:
        got = [r.counts["n_extracted"] for r in recs]
        if got != EXPECT:
            raise SystemExit("batch_loop.py: an event gave %r candidates, not %r" % (got, EXPECT))


def measure(K, cols, runs):
    p = Params()
    resident = [build(cols, p) for _ in range(K)]      # the batch's inputs, never modified
    seq, bat = [], []
    for rnd in range(runs + 1):
        fresh = [build(cols, p) for _ in range(K)]
        t, recs = _timed(lambda: [pipeline.run(d, None, iterations=3, resident="device") for d in fresh])
        _check(recs)
        del fresh
        tb, recs = _timed(lambda: pipeline.run_batch(resident, iterations=3))
        _check(recs)
        if rnd:      # (round 0 warms both)
            seq.append(t)
            bat.append(tb)
    # the two new calls on their own
    concat, split = [], []
    ex = extract.Params()
    for rnd in range(runs + 1):
        t, fused = _timed(lambda: DeviceGraph.concat(resident))
        fused.clear_errors()
        fused.cluster("tse", *pipeline.CLUSTER_FIRST, p)
        order = extract.candidate_order_dev(fused)
        res = extract.run_dev(fused, fused.carried["vivl"], ex, order)
        o = extract.outputs_dev(fused, res, ex.numhits, ids=True, lists=False, members=True)
        ts, sp = _timed(lambda: extract.split_dev(fused, o, K))
        if [c["n_extracted"] for c in sp["counts"]] != [EXPECT[0]] * K:
            raise SystemExit("batch_loop.py: the split gave %r" % [c["n_extracted"] for c in sp["counts"]])
        if rnd:
            concat.append(t)
            split.append(ts)
    out = {"copies": K, "n_nodes": fused.n_nodes, "n_slots": fused.n_slots, "n_sub": fused.n_sub,
           "sequential": _stats(seq), "batch": _stats(bat), "concat": _stats(concat), "split": _stats(split)}
    out["sequential_over_batch"] = out["sequential"]["median_ms"] / out["batch"]["median_ms"]
    out["per_event_ms"] = {"sequential": out["sequential"]["median_ms"] / K, "batch": out["batch"]["median_ms"] / K}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--copies", default="1,8,64")
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("batch_loop.py needs the MI355X")
    cols = columns()
    res = {"tool": "batch_loop", "device": torch.cuda.get_device_name(0), "event": "tests/golden/kat134, volume 7",
           "iterations": 3, "batches": [measure(int(k), cols, a.runs) for k in a.copies.split(",") if k]}
    s = json.dumps(res)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
