"""A batch of events built in one call against the same events built one after another and fused.

    python tools/batch_build.py [out.json] [--copies 1,8,64] [--runs 5]

K copies of the committed vol-7 event (tests/golden/kat134). The CSV files are parsed once, on the host,
outside every timed window: a side starts from the parsed host columns and ends with a fused graph ready
for stage 1 (states, priors, mixture weights, degrees and send weights computed). Host clock around a
device synchronise, one warm round and then the median and the minimum of `runs` rounds; a round times
both sides, one after the other, on the same box:
  * per_event (side A, the parent commit's sequence): K times pipeline.build_event_dev's body --
    DeviceGraph.from_event (gtf_build_event_csr_device, gtf_event_pack, gtf_fill_columns,
    gtf_graph_prepare), the states and the send weights -- then DeviceGraph.concat;
  * batch (side B): pipeline.build_events_dev's body -- DeviceGraph.from_events
    (gtf_build_events_csr_device once, then pack, fill and prepare once), the states and the send weights
    once on the fused graph.
Every round also runs side B with marks -- a synchronise and a clock read after the upload, the CSR, pack +
fill, prepare, the states and the send weights, as tools/resident_event.py marks from_event -- and both
sides followed by the loop (pipeline.run_batch on the list / on the fused graph, three iterations; every
event's 1,055 / 110 / 2 candidates are checked). Prints one JSON line (times in milliseconds)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gnn-track-finding_amd")]
import torch  # noqa: E402
from gtf import io, pipeline  # noqa: E402
from gtf.device import DeviceGraph  # noqa: E402
from gtf.params import Params  # noqa: E402

PREFIX = os.path.join(ROOT, "tests", "golden", "kat134", "event_1_filtered_graph_")
EXPECT = [1055, 110, 2]
PARTS = ("upload", "csr", "pack_fill", "prepare", "states", "send_mw")


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


def _states(d, p, mark=lambda part: None):
    d.clear_errors()
    d.track_state_estimates(p)
    d.node_ops(["priors_tse", "mw_tse", "degree"], p)
    d.raise_errors()
    mark("states")
    d.refresh_send_mw()
    mark("send_mw")
    return d


def per_event(cols, K, p):
    """side A: the events one after another, then the concat; returns the list too (run_batch's input)"""
    ds = [_states(DeviceGraph.from_event(*cols), p) for _ in range(K)]
    return ds, DeviceGraph.concat(ds)


def batch(cols, K, p, mark=lambda part: None):
    """side B: one build"""
    return _states(DeviceGraph._from_events([cols] * K, "cuda", "torch", mark), p, mark)


def _check(records):
    for recs in records:
        got = [r.counts["n_extracted"] for r in recs]
        if got != EXPECT:
            raise SystemExit("batch_build.py: an event gave %r candidates, not %r" % (got, EXPECT))


def measure(K, cols, runs):
    p = Params()
    a, b, a_loop, b_loop = [], [], [], []
    parts = {k: [] for k in PARTS}
    for rnd in range(runs + 1):
        ta, (_, fa) = _timed(lambda: per_event(cols, K, p))
        tb, fb = _timed(lambda: batch(cols, K, p))
        if (fa.n_nodes, fa.n_slots, fa.n_sub) != (fb.n_nodes, fb.n_slots, fb.n_sub):
            raise SystemExit("batch_build.py: the two sides built different graphs")
        sizes = {"n_nodes": fb.n_nodes, "n_slots": fb.n_slots, "n_sub": fb.n_sub}
        del fa, fb
        marks = []

        def mark(part):
            torch.cuda.synchronize()
            marks.append((part, time.perf_counter()))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        batch(cols, K, p, mark)
        tal, recs = _timed(lambda: pipeline.run_batch(per_event(cols, K, p)[0], iterations=3))
        _check(recs)
        tbl, recs = _timed(lambda: pipeline.run_batch(batch(cols, K, p), iterations=3))
        _check(recs)
        if rnd:      # (round 0 warms both sides)
            a.append(ta)
            b.append(tb)
            a_loop.append(tal)
            b_loop.append(tbl)
            for part, t in marks:
                parts[part].append((t - t0) * 1e3)
                t0 = t
    out = {"copies": K, **sizes, "per_event": _stats(a), "batch": _stats(b),
           "batch_parts": {k: _stats(v) for k, v in parts.items()},
           "per_event_and_loop": _stats(a_loop), "batch_and_loop": _stats(b_loop)}
    out["batch_median_below_per_event_min"] = out["batch"]["median_ms"] < out["per_event"]["min_ms"]
    out["per_event_over_batch"] = out["per_event"]["median_ms"] / out["batch"]["median_ms"]
    out["per_event_ms"] = {"per_event": out["per_event"]["median_ms"] / K, "batch": out["batch"]["median_ms"] / K}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--copies", default="1,8,64")
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("batch_build.py needs the MI355X")
    cols = columns()
    res = {"tool": "batch_build", "device": torch.cuda.get_device_name(0), "event": "tests/golden/kat134, volume 7",
           "iterations": 3, "batches": [measure(int(k), cols, a.runs) for k in a.copies.split(",") if k]}
    s = json.dumps(res)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
