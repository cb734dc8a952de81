"""The CSV front end of a batch in one call per kind against the same files parsed one after another.

    python tools/batch_parse.py [out.json] [--copies 1,8,64] [--runs 5]

K copies of the committed vol-7 event (tests/golden/kat134). The bytes of nodes.csv and edges.csv are read
once, outside every timed window: a side starts from those bytes in host memory and ends with a fused graph
ready for stage 1 (states, priors, mixture weights, degrees and send weights computed). Host clock around a
device synchronise, one warm round and then the median and the minimum of `runs` rounds; a round times both
sides, one after the other, on the same box:
  * per_file (side A, pipeline.build_events_dev(parse="device")'s body): per event io.read_nodes_dev
    (upload, gtf_csv_parse, gtf_event_window, the ambiguous list down, edge_length_xy, up,
    gtf_event_radius_patch) and io.read_edges_dev, then DeviceGraph.from_events (a gather, one build) and
    the states;
  * batch (side B, batch_parse=True's body): io.read_nodes_batch_dev (one buffer, one upload, one
    gtf_csv_parse_ev, one gtf_event_window_ev, one patch), io.read_edges_batch_dev, DeviceGraph.from_fused
    (no gather, one build) and the states.
The same comparison for the truth files (particles, mapping, truth.csv written from the committed tables to
a temporary directory, so they come from the page cache) up to a DeviceTruthBatch:
metrics.truth_files_batch_dev with batch_parse False / True.
Before anything is timed the two sides' outputs are compared at every size, bit for bit. Every round also
runs side B with marks -- a synchronise and a clock read after each part -- and once more with device events
around gtf_csv_parse_ev and gtf_event_window_ev of the node files. Prints one JSON line (times in ms)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gnn-track-finding_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from gtf import io, metrics, pipeline  # noqa: E402
from gtf.device import DeviceGraph  # noqa: E402
from gtf.params import Params  # noqa: E402

KAT = os.path.join(ROOT, "tests", "golden", "kat134")
PREFIX = os.path.join(KAT, "event_1_filtered_graph_")
MAPPING = "full-mapping-minCurv-0.3-134.csv"
PARTS = ("upload", "parse", "window", "patch", "edges", "build", "states")


def _stats(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "runs": len(ts)}


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def per_file(nodes, edges, K, p):
    """side A"""
    parts = []
    for _ in range(K):
        nd = io.read_nodes_dev(nodes, 7, 7)
        n2, n1, _ = io.read_edges_dev(edges)
        parts.append((nd.ids, nd.x, nd.y, nd.z, nd.r, nd.layer_id, n1, n2))
    return pipeline._event_states(DeviceGraph.from_events(parts), p)


def batch(nodes, edges, K, p, mark=None):
    """side B"""
    done = mark or (lambda part: None)
    nd = io.read_nodes_batch_dev([nodes] * K, 7, 7, mark=mark)
    n2, n1, row_off, _ = io.read_edges_batch_dev([edges] * K)
    done("edges")
    d = DeviceGraph.from_fused((nd.ids, nd.x, nd.y, nd.z, nd.r, nd.layer_id, n1, n2), nd.node_off, row_off)
    done("build")
    d = pipeline._event_states(d, p)
    done("states")
    return d


def _same_graph(a, b):
    (ga, va), (gb, vb) = a.host_graph(), b.host_graph()
    same = (ga.n_nodes, ga.n_slots, ga.n_subgraphs) == (gb.n_nodes, gb.n_slots, gb.n_subgraphs) and va.tobytes() == vb.tobytes()
    for x, y in ((ga.slot_ptr, gb.slot_ptr), (ga.out_ptr, gb.out_ptr), (ga.out_slot, gb.out_slot)):
        same = same and np.array_equal(x, y)
    for da, db in ((ga.node, gb.node), (ga.slot, gb.slot)):
        same = same and sorted(da) == sorted(db) and all(da[k].dtype == db[k].dtype and da[k].tobytes() == db[k].tobytes() for k in da)
    return same and np.array_equal(a._np(a.carried["event"]), b._np(b.carried["event"]))


def _same_truth(a, b):
    ha, hb = vars(a.host()), vars(b.host())
    return sorted(ha) == sorted(hb) and all(np.asarray(ha[k]).tobytes() == np.asarray(hb[k]).tobytes() for k in ha) \
        and a.n_reference == b.n_reference


def truth_dir(tmp):
    """the truth files of the vol-7 fixture, with a truth.csv"""
    import pandas as pd
    z = np.load(os.path.join(ROOT, "tests", "golden", "metrics_vol7.npz"), allow_pickle=False)
    m = pd.DataFrame({c: z["map__" + c] for c in metrics.MAPPING_COLUMNS})
    m.to_csv(os.path.join(tmp, "event000001000-" + MAPPING), index=False)
    pd.DataFrame({c: z["particles__" + c] for c in ("particle_id", "px", "py")}).to_csv(
        os.path.join(tmp, "event000001000-particles.csv"), index=False)
    m[["hit_id", "particle_id"]].drop_duplicates("hit_id").to_csv(os.path.join(tmp, "event000001000-truth.csv"), index=False)
    return os.path.join(tmp, "event000001000-")


def measure(K, nodes, edges, truth, runs):
    p = Params()
    fa, fb = per_file(nodes, edges, K, p), batch(nodes, edges, K, p)
    if not _same_graph(fa, fb):
        raise SystemExit("batch_parse.py: the two sides built different graphs at K = %d" % K)
    sizes = {"n_nodes": fb.n_nodes, "n_slots": fb.n_slots, "text_bytes": K * (len(nodes) + len(edges))}
    del fa, fb
    if truth:
        ta = metrics.truth_files_batch_dev([truth] * K, MAPPING, 7, 7)[0]
        tb = metrics.truth_files_batch_dev([truth] * K, MAPPING, 7, 7, batch_parse=True)[0]
        if not _same_truth(ta, tb):
            raise SystemExit("batch_parse.py: the two sides built different truth tables at K = %d" % K)
        del ta, tb
    a, b, ta_, tb_, dev_parse, dev_window = [], [], [], [], [], []
    parts = {k: [] for k in PARTS}
    for rnd in range(runs + 1):
        t_a, _ = _timed(lambda: per_file(nodes, edges, K, p))
        t_b, _ = _timed(lambda: batch(nodes, edges, K, p))
        marks = []

        def mark(part):
            torch.cuda.synchronize()
            marks.append((part, time.perf_counter()))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        batch(nodes, edges, K, p, mark)
        events = {}

        def record(part):
            events[part] = torch.cuda.Event(enable_timing=True)
            events[part].record()
        io.read_nodes_batch_dev([nodes] * K, 7, 7, mark=record)
        torch.cuda.synchronize()
        if truth:
            t_ta, _ = _timed(lambda: metrics.truth_files_batch_dev([truth] * K, MAPPING, 7, 7))
            t_tb, _ = _timed(lambda: metrics.truth_files_batch_dev([truth] * K, MAPPING, 7, 7, batch_parse=True))
        if rnd:      # (round 0 warms both sides)
            a.append(t_a)
            b.append(t_b)
            dev_parse.append(events["upload"].elapsed_time(events["parse"]))
            dev_window.append(events["parse"].elapsed_time(events["window"]))
            for part, t in marks:
                parts[part].append((t - t0) * 1e3)
                t0 = t
            if truth:
                ta_.append(t_ta)
                tb_.append(t_tb)
    out = {"copies": K, **sizes, "per_file": _stats(a), "batch": _stats(b),
           "batch_parts": {k: _stats(v) for k, v in parts.items()},
           "gtf_csv_parse_ev_nodes_device_ms": _stats(dev_parse), "gtf_event_window_ev_device_ms": _stats(dev_window)}
    out["batch_median_below_per_file_min"] = out["batch"]["median_ms"] < out["per_file"]["min_ms"]
    out["per_file_over_batch"] = out["per_file"]["median_ms"] / out["batch"]["median_ms"]
    if truth:
        out["truth_per_file"], out["truth_batch"] = _stats(ta_), _stats(tb_)
        out["truth_batch_median_below_per_file_min"] = out["truth_batch"]["median_ms"] < out["truth_per_file"]["min_ms"]
        out["truth_per_file_over_batch"] = out["truth_per_file"]["median_ms"] / out["truth_batch"]["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--copies", default="1,8,64")
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("batch_parse.py needs the MI355X")
    nodes, edges = (open(PREFIX + f, "rb").read() for f in ("nodes.csv", "edges.csv"))
    with tempfile.TemporaryDirectory() as tmp:
        truth = truth_dir(tmp)
        res = {"tool": "batch_parse", "device": torch.cuda.get_device_name(0), "event": "tests/golden/kat134, volume 7",
               "truth_files": bool(truth),
               "batches": [measure(int(k), nodes, edges, truth, a.runs) for k in a.copies.split(",") if k]}
    s = json.dumps(res)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
