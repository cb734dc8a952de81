"""Host builders against gtf_graph_prepare: what the graph-static schedules and slot tables cost.

    python tools/graph_prepare.py [out.json] [--workloads c4,c3] [--runs 25]

Per workload (synthetic C4 and C3, seed 3), on this box:
  * the NumPy builders of gtf/device.py, by group (schedules; slot_classes; slot_static_words +
    slot_sender_xzr; the inline tables of DeviceGraph.__init__), host clock, median of 5;
  * the whole DeviceGraph construction with tables="host" (classes on) and tables="device", host
    clock around a device synchronise, median of 5 after one warm construction of each;
  * gtf_graph_prepare alone on a resident graph: HIP events around the call (it synchronises
    once inside), warm, median of --runs (>= 20) calls.
Prints one JSON line (times in milliseconds, and the host / device ratio)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gnn-track-finding_amd")]
import torch  # noqa: E402
from gtf import device as dev, synth, _native as nat  # noqa: E402

HOST_RUNS = 5


def _ms(fn, runs=HOST_RUNS):
    ts = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def host_builders(g):
    """the NumPy builders DeviceGraph(tables="host", classes=True) runs, timed by group"""
    out = {}

    def schedules():
        sched, _, _, _ = dev.node_schedule(g.slot_ptr)
        dev.sched_segments(g.slot_ptr, sched)
        q, n = dev.sender_schedule(g.out_ptr)
        od = g.slot_dst()[g.out_slot].astype(np.int32) if g.n_edges else np.zeros(0, np.int32)
        dev.sender_lanes(g.out_slot, od, q, n)

    def inline():   # slot_dst, out_dst, slot_layer, slot_outpos, slot_outidx as DeviceGraph.__init__ computes them
        g.slot_dst().astype(np.int32)
        g.slot_dst()[g.out_slot].astype(np.int32)
        src = g.slot["slot_src"].astype(np.int64)
        np.where(src >= 0, g.node["layer"][np.maximum(src, 0)], np.nan).astype(np.float64)
        owner = np.repeat(np.arange(g.n_nodes, dtype=np.int64), np.diff(g.out_ptr.astype(np.int64)))
        outpos = np.full(g.n_slots, -1, np.int32)
        outpos[g.out_slot] = (np.arange(g.n_edges) - g.out_ptr[owner]).astype(np.int32)
        oidx = np.full(g.n_slots, -1, np.int32)
        oidx[g.out_slot] = np.arange(g.n_edges, dtype=np.int32)

    cls, sfl, _ = dev.slot_classes(g)
    out["schedules_ms"] = _ms(schedules)
    out["slot_classes_ms"] = _ms(lambda: dev.slot_classes(g))
    out["static_sxzr_ms"] = _ms(lambda: (dev.slot_static_words(g, cls, sfl), dev.slot_sender_xzr(g)))
    out["inline_tables_ms"] = _ms(inline)
    out["total_ms"] = sum(out.values())
    return out


def construction(g, **kw):
    def build():
        d = dev.DeviceGraph(g, "cuda:0", **kw)
        torch.cuda.synchronize()
        return d
    build()
    return _ms(build)


def prepare_alone(g, runs):
    d = dev.DeviceGraph(g, "cuda:0", tables="device")
    L = d.lib
    N, S, E = g.n_nodes, g.n_slots, g.n_edges
    ws = torch.empty(int(L.gtf_graph_prepare_workspace_bytes(N, S, E)), dtype=torch.uint8, device="cuda:0")
    p = d.ptr
    names = [f for f, _ in nat.GtfGraphTables._fields_]
    tb = nat.GtfGraphTables(**{n: p(n) for n in names})   # rewrites the graph's own tables with the same values

    def call():
        cg = nat.GtfGraph(n_nodes=N, n_slots=S, n_edges=E, slot_ptr=p("slot_ptr"), slot_src=p("slot_src"),
                          out_ptr=p("out_ptr"), out_slot=p("out_slot"), is_edge=p("is_edge"), rev_edge=p("rev_edge"),
                          gnn=p("gnn"), layer=p("layer"))
        nat.check(L.gtf_graph_prepare(ctypes.byref(cg), ctypes.byref(tb), ctypes.c_void_p(ws.data_ptr()),
                                      ctypes.c_size_t(ws.numel()), d.stream))
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "runs": runs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--workloads", default="c4,c3")
    ap.add_argument("--runs", type=int, default=25)
    a = ap.parse_args()
    if a.runs < 20:
        ap.error("--runs must be at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("graph_prepare.py needs the MI355X")
    res = {"tool": "graph_prepare", "device": torch.cuda.get_device_name(0), "workloads": {}}
    for name in a.workloads.split(","):
        g = synth.workload(name, seed=3)
        h = host_builders(g)
        r = {"n_nodes": g.n_nodes, "n_slots": g.n_slots, "n_edges": g.n_edges, "host_builders": h,
             "device_graph_host_tables_ms": construction(g, classes=True),
             "device_graph_device_tables_ms": construction(g, tables="device"),
             "gtf_graph_prepare": prepare_alone(g, a.runs)}
        r["host_over_device"] = h["total_ms"] / r["gtf_graph_prepare"]["median_ms"]
        res["workloads"][name] = r
    s = json.dumps(res)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
