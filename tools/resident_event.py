"""Event conversion into a resident DeviceGraph (pipeline.build_event_dev: DeviceGraph.from_event,
then the states on that object) against the sequence it replaces: pipeline.build_event followed by
the DeviceGraph(g) that pipeline.run constructs for iteration 1.

    python tools/resident_event.py [out.json] [--events vol7,c4]

On this box, host clock around a device synchronise, one warm run, median of 5:
  * the vol-7 event (tests/golden/kat134) and a C4-sized one -- the undirected edges of
    synth.workload("c4") as shuffled rows with random 40-bit node ids, the way
    bench.py:bench_event_build makes them, with that event's coordinates and layers -- each from
    PARSED COLUMNS (the CSV readers are replaced by the cached columns, so no file is read inside a
    timed window) to a graph ready for stage 1:
      old: io.build_event_csr(device) (CSR on the GPU, downloaded, NumPy assembly), DeviceGraph(g),
           clear_errors / track_state_estimates / node_ops / error read, download, host
           refresh_send_mw, and the second DeviceGraph(g) of pipeline.run -- with tables="host" (the
           default of both) and with tables="device";
      new: from_event (upload, CSR build, pack + fill, prepare -- each timed to a synchronise through
           DeviceGraph._from_event's mark callback), the same state calls and refresh_send_mw on the device;
    whole and per part. The error word is read, not raised (a synthetic event may hold a node whose
    reference code would raise); the JSON records it for both paths.
  * the three-iteration vol-7 loop end to end FROM THE CSV FILES: build_event + run(resident="device")
    against build_event_dev + run(d, None, resident="device").
Prints one JSON line (times in milliseconds) and writes it to out.json."""
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
from gtf import graph, io, pipeline, synth  # noqa: E402
from gtf.device import DeviceGraph  # noqa: E402
from gtf.params import Params  # noqa: E402

PREFIX = os.path.join(ROOT, "tests", "golden", "kat134", "event_1_filtered_graph_")
RUNS = 5
OPS = ["priors_tse", "mw_tse", "degree"]


def _stats(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "runs": len(ts)}


def _ms(fn, runs=RUNS):
    fn()
    ts = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return _stats(ts)


def columns(name):
    """(ids, x, y, z, r, layer_id, row_a, row_b) of the event"""
    if name == "vol7":
        ids, x, y, z, r, layer = io.read_nodes(PREFIX + "nodes.csv", 7, 7)
        n2, n1 = io.read_edges(PREFIX + "edges.csv")
        return ids, x, y, z, r, layer, n1, n2
    g = synth.workload(name, seed=3)
    rng = np.random.default_rng(5)                       # bench.py:bench_event_build's rows
    dst = np.repeat(np.arange(g.n_nodes), np.diff(g.slot_ptr))
    src = g.slot["slot_src"]
    keep = (src >= 0) & (src < dst)
    a, b = src[keep], dst[keep]
    perm = rng.permutation(a.size)
    ids = rng.choice(2 ** 40, size=g.n_nodes, replace=False).astype(np.int64)
    gnn = g.node["gnn"]
    layer = 7000 + np.nan_to_num(g.node["layer"]).astype(np.int64)
    return (ids, gnn[:, 0].copy(), gnn[:, 1].copy(), gnn[:, 2].copy(), gnn[:, 3].copy(), layer,
            ids[a[perm]], ids[b[perm]])


def _states(d, p):
    d.clear_errors()
    d.track_state_estimates(p)
    d.node_ops(OPS, p)
    return d.errors()


def event(name):
    cols = columns(name)
    p = Params()
    # the CSV readers hand out the cached columns: every timed window starts from parsed columns
    io.read_nodes = lambda path, lo, hi: cols[:6]
    io.read_edges = lambda path: (cols[7], cols[6])
    s = {}

    def old(tables, parts=None):
        def step(k, fn):
            if parts is None:
                return fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            parts.setdefault(k, []).append((time.perf_counter() - t0) * 1e3)
            return out
        g, vivl = step("csr_build_download_assemble", lambda: io.build_event_csr("", 7, 7, device="cuda"))
        d = step("device_graph_1", lambda: DeviceGraph(g, "cuda", tables=tables))
        s["old_err"] = step("states", lambda: _states(d, p))
        step("download", lambda: d.download(g))
        step("host_send_mw", lambda: graph.refresh_send_mw(g))
        s["old"] = step("device_graph_2", lambda: DeviceGraph(g, "cuda", tables=tables))
        s["g"] = g

    def new(parts=None):
        t = [0.0]

        def mark(k):
            torch.cuda.synchronize()
            now = time.perf_counter()
            parts.setdefault(k, []).append((now - t[0]) * 1e3)
            t[0] = now
        if parts is not None:
            torch.cuda.synchronize()
            t[0] = time.perf_counter()
        d = (DeviceGraph.from_event(*cols) if parts is None
             else DeviceGraph._from_event(*cols, "cuda", "torch", mark))
        s["new_err"] = _states(d, p)
        if parts is not None:
            mark("states")
        d.refresh_send_mw()
        if parts is not None:
            mark("send_mw")
        s["new"] = d

    r = {}
    for tables in ("host", "device"):
        parts = {}
        old(tables)
        for _ in range(RUNS):
            old(tables, parts)
        r["old_tables_" + tables] = {"whole": _ms(lambda: old(tables)), "parts": {k: _stats(v) for k, v in parts.items()}}
    parts = {}
    new()
    for _ in range(RUNS):
        new(parts)
    r["new"] = {"whole": _ms(new), "parts": {k: _stats(v) for k, v in parts.items()}}
    d, g = s["new"], s["g"]
    h, _ = d.host_graph()
    same = all(np.array_equal(h.node[k], g.node[k], equal_nan=True) for k in graph.NODE_FIELDS) and \
        all(np.array_equal(h.slot[k], g.slot[k], equal_nan=True) for k in graph.SLOT_FIELDS)
    r.update(n_nodes=d.n_nodes, n_edges=d.n_edges, n_sub=d.n_sub, rows=int(cols[6].size),
             error_word_old=int(s["old_err"]), error_word_new=int(s["new_err"]), same_graph=bool(same))
    for tables in ("host", "device"):
        r["old_tables_%s_over_new" % tables] = r["old_tables_" + tables]["whole"]["median_ms"] / \
            r["new"]["whole"]["median_ms"]
    return r


def loop_vol7():
    """three iterations from the CSV files, parsing included"""
    p = Params()
    s = {}

    def old():
        g, vivl = pipeline.build_event(PREFIX, 7, 7, p)
        s["old"] = pipeline.run(g, vivl, iterations=3, p=p, resident="device")

    def new():
        s["new"] = pipeline.run(pipeline.build_event_dev(PREFIX, 7, 7, p), None, iterations=3, p=p, resident="device")

    r = {"old": _ms(old), "new": _ms(new)}
    r["candidates"] = [len(i.candidates) for i in s["new"]]
    r["same_candidates"] = [len(i.candidates) for i in s["old"]] == r["candidates"]
    r["old_over_new"] = r["old"]["median_ms"] / r["new"]["median_ms"]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--events", default="vol7,c4")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resident_event.py needs the MI355X")
    res = {"tool": "resident_event", "device": torch.cuda.get_device_name(0), "loop_vol7": loop_vol7(), "events": {}}
    read_nodes, read_edges = io.read_nodes, io.read_edges
    for name in [e for e in a.events.split(",") if e]:
        io.read_nodes, io.read_edges = read_nodes, read_edges
        res["events"][name] = event(name)
    s = json.dumps(res)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
