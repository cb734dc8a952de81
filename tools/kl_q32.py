"""GPU box: config 5's parabolic KL launch through its three input paths -- f64, f32 (fp64
coordinates and int64 truth ids both) and q32 (gtf_parabolic_kl_q32: 32-bit fixed-point
coordinates, int32 ids) -- on the 256-event batch of the committed vol-7 134 event in the
ordered layout, cold as bench.py's bench_c5 measures it: 8 resident replicas (jitter seeds
0..7) launched in rotation, so no launch finds its inputs in the caches.

    python tools/kl_q32.py [--events 256] [--batches 8] [--rounds 3] [--launches 200]
                           [--dump DIR] [--pmc]

Prints one JSON line: per path the HIP-event time per launch (median and minimum over the
rounds; the paths alternate inside a round), the algorithmic byte model
(gtf.roofline.parabolic_kl_bytes) and its fraction of 8 TB/s at the median, the device
footprint per batch, and q32's error against f64 on batch 0.
--dump DIR: batch 0's kl / truth / emp_var of every path as .npy (to compare two builds).
--pmc: a counter run -- one warm-up and one rotation per path, no timing; run it under
rocprofv3 --pmc FETCH_SIZE and again under rocprofv3 --pmc WRITE_SIZE (counters only, no
tracing; one counter per run: the two together exceed what the hardware collects at once, and
rocprofv3 aborts), each into its own directory under one parent, then

    python tools/kl_q32.py --pmc-summary <parent dir>

prints the median FETCH_SIZE / WRITE_SIZE (KiB per launch) of each path's kernel -- the
kernel names carry the path (PathD<double>, PathD<float>, PathQ) -- and the q32 / f64 and
q32 / f32 ratios, as one JSON line (needs no GPU)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gnn-track-finding_amd")]
import torch  # noqa: E402
from gtf import io, parabolic, roofline as rf  # noqa: E402

PATHS = ("f64", "f32", "q32")
KERNEL_OF = {"f64": "PathD<double>", "f32": "PathD<float>", "q32": "PathQ"}


def pmc_summary(d):
    import collections
    import csv
    import glob
    vals = collections.defaultdict(list)
    files = sorted(glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True))
    for f in files:
        for r in csv.DictReader(open(f)):
            for dt, tag in KERNEL_OF.items():
                if "k_parabolic_kl<" in r["Kernel_Name"] and tag in r["Kernel_Name"]:
                    vals[dt, r["Counter_Name"]].append(float(r["Counter_Value"]))
    res = {"files": [os.path.relpath(f, d) for f in files], "unit": "KiB per launch, median over the launches"}
    for dt in PATHS:
        res[dt] = {c: float(np.median(vals[dt, c])) for c in ("FETCH_SIZE", "WRITE_SIZE") if vals[dt, c]}
        res[dt]["launches"] = max(len(vals[dt, c]) for c in ("FETCH_SIZE", "WRITE_SIZE"))
    for c in ("FETCH_SIZE", "WRITE_SIZE"):
        if all(c in res[dt] for dt in PATHS):
            res["q32_over_f64_" + c] = res["q32"][c] / res["f64"][c]
            res["q32_over_f32_" + c] = res["q32"][c] / res["f32"][c]
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=256)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--dump")
    ap.add_argument("--pmc", action="store_true")
    ap.add_argument("--pmc-summary")
    a = ap.parse_args()
    if a.pmc_summary:
        return pmc_summary(a.pmc_summary)
    assert torch.cuda.is_available(), "needs the GPU"
    kat = os.path.join(ROOT, "tests", "golden", "kat134")
    g = io.load_event(os.path.join(kat, "event_1_filtered_graph_"), 7, 7)
    truth = io.read_truth(os.path.join(kat, "truth_vol7.csv"), g.node["node_id"])
    ptr0, src0 = parabolic.in_edge_csr(g)
    ptr, src, gnn, tr = parabolic.batch(ptr0, src0, g.node["gnn"], truth, a.events)
    k = parabolic.ParabolicKL(ptr, src, gnn, tr, "cuda", ordered=True, compact=True)
    ks = [k] + [k.replica(gnn=parabolic.batch(ptr0, src0, g.node["gnn"], truth, a.events, seed=e)[2])
                for e in range(1, a.batches)]
    outs = {dt: [kk.alloc(dt, emp="var") for kk in ks] for dt in PATHS}

    def rotate(dt, n):
        for i in range(n):
            ks[i % len(ks)].run(outs[dt][i % len(ks)], dt)

    for dt in PATHS:   # warm-up: code objects loaded, every buffer touched
        rotate(dt, len(ks))
    torch.cuda.synchronize()
    res = {"workload": "%d x committed vol-7 134 event (jittered copies), ordered layout" % a.events,
           "nodes": k.n_nodes, "in_edges": k.n_slots, "pairs": k.n_pairs, "listed_nodes": k.n_listed,
           "batches_rotated": len(ks), "scale_log2": int(np.log2(k.scale))}
    if a.pmc:
        for dt in PATHS:
            rotate(dt, len(ks))
        torch.cuda.synchronize()
        res["pmc_launches_per_path"] = 2 * len(ks)
    else:
        launches = max(a.launches, len(ks)) // len(ks) * len(ks)
        times = {dt: [] for dt in PATHS}
        for _ in range(a.rounds):
            for dt in PATHS:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                rotate(dt, launches)
                e1.record()
                torch.cuda.synchronize()
                times[dt].append(e0.elapsed_time(e1) / launches * 1e3)
        for dt in PATHS:
            nb = rf.parabolic_kl_bytes(k.n_nodes, k.n_listed, k.n_slots, k.n_pairs, dt)
            us = float(np.median(times[dt]))
            res[dt] = {"cold_us_median": us, "cold_us_min": float(min(times[dt])), "cold_us_rounds": times[dt],
                       "launches_per_round": launches, "algorithmic_bytes_per_launch": nb,
                       "frac_of_8TBs": nb / (us * 1e-6) / 8e12,
                       "footprint_bytes_per_batch": k.footprint_bytes(outs[dt][0], dt)}
        res["q32_over_f32_time"] = res["q32"]["cold_us_median"] / res["f32"]["cold_us_median"]
        res["q32_over_f64_time"] = res["q32"]["cold_us_median"] / res["f64"]["cold_us_median"]
    res["device_error_flags"] = max(kk.errors() for kk in ks)
    a64 = outs["f64"][0]["kl"].double().cpu().numpy()
    b = outs["q32"][0]["kl"].double().cpu().numpy()
    rel = np.abs(b - a64) / np.maximum(np.abs(a64), 1e-300)
    res["q32_vs_f64"] = {"median_rel": float(np.median(rel)), "p99_rel": float(np.percentile(rel, 99)),
                         "flips": {str(t): int(((a64 < t) != (b < t)).sum()) for t in (1, 2, 10, 100)},
                         "truth_equal": bool(torch.equal(outs["f64"][0]["truth"], outs["q32"][0]["truth"]))}
    if a.dump:
        os.makedirs(a.dump, exist_ok=True)
        for dt in PATHS:
            for f in ("kl", "truth", "emp_var"):
                np.save(os.path.join(a.dump, "%s_%s.npy" % (dt, f)), outs[dt][0][f].cpu().numpy())
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
