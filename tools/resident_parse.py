"""The CSV front end on the GPU (pipeline.build_event_dev(parse="device"): gtf_csv_parse,
gtf_event_window, gtf_event_radius_patch; metrics.truth_files_dev) against the sequence it replaces: the
host readers (io.read_nodes: pandas, io.read_edges: np.loadtxt; three pd.read_csv for the truth files)
in front of the same resident build.

    python tools/resident_parse.py [out.json] [--tiles 40]

On this box, one build, host clock around a device synchronise, one warm run, median of 5. Both
sequences start from the files in a temporary directory (in the page cache after the warm run) and end
with a graph ready for stage 1 (build_event_dev, states included) or with the scorer's tables:
  * the vol-7 fixture (tests/golden/kat134) and the same files tiled `tiles` times with shifted ids,
    written at run time;
  * the device sequence split at DeviceGraph-free marks, each closed by a synchronise: upload of the
    bytes (with the allocation of the outputs), gtf_csv_parse per file (host clock, and between device
    events), the window, the host radius patch with its node count, and the rest (the event build);
  * the truth files of the golden vol-7 event (mapping, truth, particles), tiled the same way:
    pd.read_csv x 3 + truth_tables_dev against truth_files_dev.
Prints one JSON line (times in milliseconds) and writes it to out.json."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gnn-track-finding_amd")]
import torch  # noqa: E402
from gtf import csvdev, io, metrics, pipeline  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
PREFIX = os.path.join(GOLDEN, "kat134", "event_1_filtered_graph_")
RUNS = 5
MAPPING = "full-mapping-minCurv-0.3-134.csv"


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


def write_event(d, tiles):
    """the vol-7 files `tiles` times over, node ids shifted per tile; returns the prefix"""
    import pandas as pd
    nodes = pd.read_csv(PREFIX + "nodes.csv", dtype=str)
    lines = open(PREFIX + "edges.csv").read().split("\n")
    edges = [ln.split(",") for ln in lines[2:] if ln]
    ids = nodes["node_idx"].astype(np.int64)
    shift = int(max(ids.max(), max(int(e[0]) for e in edges), max(int(e[1]) for e in edges))) + 1
    pre = os.path.join(d, "event_1_filtered_graph_")
    with open(pre + "nodes.csv", "w") as f:
        f.write(",".join(nodes.columns) + "\n")
        rest = nodes[[c for c in nodes.columns if c != "node_idx"]].agg(",".join, axis=1).tolist()
        for k in range(tiles):
            f.write("".join("%d,%s\n" % (i + k * shift, r) for i, r in zip(ids.tolist(), rest)))
    with open(pre + "edges.csv", "w") as f:
        f.write(lines[0] + "\n" + lines[1] + "\n")
        for k in range(tiles):
            f.write("".join("%d,%d,%s\n" % (int(e[0]) + k * shift, int(e[1]) + k * shift, e[2]) for e in edges))
    return pre


def write_truth(d, tiles):
    """the golden vol-7 truth tables as the three files, `tiles` times over with shifted ids"""
    import pandas as pd
    z = np.load(os.path.join(GOLDEN, "metrics_vol7.npz"), allow_pickle=False)
    m = pd.DataFrame({c: z["map__" + c] for c in metrics.MAPPING_COLUMNS})
    p = pd.DataFrame({c: z["particles__" + c] for c in ("particle_id", "px", "py")})
    sh = {c: int(m[c].max()) + 1 for c in ("node_idx", "hit_id")}
    known = set(p["particle_id"].tolist()) | set(m["particle_id"].tolist())
    ms, ps = [], []
    for k in range(tiles):
        a, b = m.copy(), p.copy()
        for c in sh:
            a[c] += k * sh[c]
        if k:      # (TrackML particle ids are sparse 18-digit codes: + k names a new particle; 0 stays the noise id)
            a.loc[a["particle_id"] != 0, "particle_id"] += k
            b.loc[b["particle_id"] != 0, "particle_id"] += k
            b = b[b["particle_id"] != 0]
            new = set(b["particle_id"].tolist())
            assert not (new & known), "particle ids collide between tiles"
            known |= new
        ms.append(a)
        ps.append(b)
    m, p = pd.concat(ms, ignore_index=True), pd.concat(ps, ignore_index=True)
    pre = os.path.join(d, "event000001000-")
    m.to_csv(pre + MAPPING)
    p.to_csv(pre + "particles.csv", index=False)
    m[["hit_id", "particle_id"]].drop_duplicates("hit_id").to_csv(pre + "truth.csv", index=False)
    return pre


def event(pre):
    r = {"bytes": {k: os.path.getsize(pre + k + ".csv") for k in ("nodes", "edges")}}
    s = {}

    def old():
        s["old"] = pipeline.build_event_dev(pre, 7, 7, parse="host")

    def new():
        s["new"] = pipeline.build_event_dev(pre, 7, 7, parse="device")

    def readers():
        io.read_nodes(pre + "nodes.csv", 7, 7)
        io.read_edges(pre + "edges.csv")

    r["host_readers"] = _ms(readers)
    r["old"] = _ms(old)
    r["new"] = _ms(new)
    assert s["new"].parse_info == {"nodes": "device", "edges": "device"}, s["new"].parse_info
    (ga, _), (gb, _) = s["old"].host_graph(), s["new"].host_graph()
    r["same_graph"] = bool(all(np.array_equal(ga.node[k], gb.node[k], equal_nan=True) for k in ga.node) and
                           all(np.array_equal(ga.slot[k], gb.slot[k], equal_nan=True) for k in ga.slot))
    r.update(n_nodes=gb.n_nodes, n_edges=gb.n_edges)
    # the parts of the device readers
    parts, dev_ms, info = {}, {}, {}
    for _ in range(RUNS + 1):
        t = [0.0]
        ev = {}

        def mark(k, name="nodes"):
            if k == "upload":
                ev[name] = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                torch.cuda.synchronize()
                ev[name][0].record()
            if k == "parse":
                ev[name][1].record()
            torch.cuda.synchronize()
            now = time.perf_counter()
            parts.setdefault(name + "_" + k, []).append((now - t[0]) * 1e3)
            t[0] = now
        torch.cuda.synchronize()
        t[0] = time.perf_counter()
        nd = io.read_nodes_dev(pre + "nodes.csv", 7, 7, mark=mark)
        csvdev.parse_dev(pre + "edges.csv", ((0, "int64"), (1, "int64")), 2, mark=lambda k: mark(k, "edges"))
        for name, (a, b) in ev.items():
            dev_ms.setdefault(name + "_parse_device_events", []).append(a.elapsed_time(b))
        info = {"rows": nd.n_rows, "kept": nd.n, "patched_nodes": nd.n_ambiguous,
                "patched_share": nd.n_ambiguous / max(nd.n, 1)}
    r["new_parts"] = {k: _stats(v[1:]) for k, v in {**parts, **dev_ms}.items()}      # (the first run is the warm one)
    r["new_parts"]["rest"] = r["new"]["median_ms"] - sum(r["new_parts"][k]["median_ms"] for k in parts)
    r["radius_patch"] = info
    r["old_over_new"] = r["old"]["median_ms"] / r["new"]["median_ms"]
    return r


def truth(pre):
    import pandas as pd
    s = {}

    def old():
        particles = pd.read_csv(pre + "particles.csv")
        m = metrics.HitMapping.from_frame(pd.read_csv(pre + MAPPING))
        t = pd.read_csv(pre + "truth.csv", usecols=["hit_id", "particle_id"])
        s["old"] = metrics.truth_tables_dev(m, particles.particle_id.to_numpy(), particles.px.to_numpy(),
                                            particles.py.to_numpy(), 7, 7, t.hit_id.to_numpy(np.int64),
                                            t.particle_id.to_numpy(np.int64))

    def new():
        s["new"], s["info"] = metrics.truth_files_dev(pre, MAPPING, 7, 7)

    r = {"bytes": {k: os.path.getsize(pre + k) for k in (MAPPING, "truth.csv", "particles.csv")}}
    r["old"] = _ms(old)
    r["new"] = _ms(new)
    a, b = s["old"].host(), s["new"].host()
    r["same_tables"] = bool(all(np.array_equal(getattr(a, k), getattr(b, k)) for k, _ in metrics._TABLE_FIELDS))
    r["parsers"] = {k: v for k, v in s["info"].items() if not k.endswith("_reason")}
    r.update(T=s["new"].n_nodes, P=s["new"].n_entries, R=s["new"].n_particles, reference=s["new"].n_reference)
    r["old_over_new"] = r["old"]["median_ms"] / r["new"]["median_ms"]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--tiles", type=int, default=40)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resident_parse.py needs the MI355X")
    res = {"tool": "resident_parse", "device": torch.cuda.get_device_name(0), "tiles": a.tiles, "events": {}, "truth": {}}
    with tempfile.TemporaryDirectory() as d:
        for name, tiles in (("vol7", 1), ("vol7_x%d" % a.tiles, a.tiles)):
            sub = os.path.join(d, name)
            os.makedirs(sub)
            res["events"][name] = event(write_event(sub, tiles))
            res["truth"][name] = truth(write_truth(sub, tiles))
    s = json.dumps(res)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
