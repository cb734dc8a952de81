"""Scoring the extracted candidates: host lists against the device stage.

    python tools/resident_metrics.py [out.json] [--workloads c4,c3] [--score-only NAME]

On this box, host clock around a device synchronise, one warm run, then the median of 5, one run on
one box. After a stage and run_dev have left their result on a DeviceGraph:
  old: extract.outputs_dev(lists=True) -- every candidate, remaining and fragment group sliced into
       a Python list -- then the candidates concatenated again and scored on the host;
  new: extract.outputs_dev(lists=False), metrics.DeviceScorer.add on its device arrays, result().
Both whole and per part, with the candidates' sizes and whether both give the same Result.
  * vol-7 (tests/golden/kat134, iteration 1's stage) with the event's real truth
    (tests/golden/metrics_vol7.npz): the host scoring is metrics.reconstruction_efficiency itself
    ("host_full": it rebuilds the reference tracks and hit_dissociation on every call) and its
    per-candidate part on prebuilt tables ("host_tables": candidate_particles, majority and the
    match, what a caller that scores more than once would keep);
  * the C4- and C3-sized synthetic workloads (tools/resident_loop.py's staged inputs, seed 3) with
    seeded fabricated truth tables of the fixture's shape: 1-6 hits per node, the first one of the
    particle that 8 consecutive nodes of the packed order share and the others of particles up to
    3 blocks away, so candidates have a majority with noise around it. There is no mapping to hand
    to reconstruction_efficiency, so the host column is "host_tables".
--score-only NAME: just DeviceScorer.add on that workload ("vol7", "c4", "c3"), ten times: to run
under a kernel trace, which gives the score launches (k_members, the exclusive sum, k_vote,
k_winners) their own times.
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
from gtf import extract, metrics, pipeline  # noqa: E402
from gtf.params import Params  # noqa: E402
from graph_subset import PREFIX  # noqa: E402
from resident_loop import staged  # noqa: E402

RUNS = 5
GOLDEN = os.path.join(ROOT, "tests", "golden", "metrics_vol7.npz")


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


def host_tables(t, cand_ptr, cand_ids):
    """metrics.reconstruction_efficiency's per-candidate part (:125-171) on prebuilt tables"""
    n = len(cand_ptr) - 1
    cand_of, part = metrics.candidate_particles(cand_ptr, cand_ids, t.node_id, t.node_ptr.astype(np.int64), t.node_part)
    pid, n_good, total = metrics.majority(n, cand_of, part)
    R = t.part_id.size
    r = np.minimum(np.searchsorted(t.part_id, pid), max(R - 1, 0))
    is_ref = (t.part_id[r] == pid) & (t.part_ref[r] != 0) if R else np.zeros(n, bool)
    hits = np.where(is_ref, t.part_hits[r] if R else 0, 1)
    good = n_good * 1.0
    with np.errstate(divide="ignore", invalid="ignore"):
        tpur, ppur = good / total, good / hits
    ok = is_ref & (good >= 0.5 * hits) & (tpur >= 0.5) & (ppur >= 0.5)
    idx = np.flatnonzero(ok)
    _, first = np.unique(pid[idx], return_index=True)
    first = np.sort(idx[first])
    matched = np.zeros(n, bool)
    matched[first] = True
    return metrics.Result(int(first.size), t.n_reference, tpur[first], ppur[first], pid, n_good, matched)


def fabricated_tables(g, seed=3):
    """truth tables of the fixture's shape for a synthetic graph: every node 1-6 hits; hit 0 belongs
    to the particle of the node's block of 8 consecutive packed nodes, the others to particles of
    blocks up to 3 away"""
    rng = np.random.default_rng(seed)
    node_id = g.node["node_id"].astype(np.int64)
    order = np.argsort(node_id, kind="stable")
    block = (np.arange(node_id.size) // 8)[order]
    n_hits = rng.choice(np.arange(1, 7), size=node_id.size, p=[0.62, 0.26, 0.08, 0.02, 0.01, 0.01])
    ptr = np.zeros(node_id.size + 1, np.int64)
    ptr[1:] = np.cumsum(n_hits)
    owner = np.repeat(np.arange(node_id.size), n_hits)
    first = np.arange(ptr[-1]) == ptr[owner]
    shift = np.where(first, 0, rng.integers(-3, 4, ptr[-1]))
    part = (1 << 59) + 2 * np.maximum(block[owner] + shift, 0) + 1
    ids, hits = np.unique(part, return_counts=True)
    ref = (hits >= 4).astype(np.uint8)
    return metrics.TruthTables(node_id[order], ptr.astype(np.int32), part.astype(np.int64), ids.astype(np.int64),
                               hits.astype(np.int32), ref, int(ref.sum()))


def _flat(lists):
    ptr = np.zeros(len(lists) + 1, np.int64)
    ptr[1:] = np.cumsum([len(c) for c in lists])
    return ptr, np.concatenate(lists) if lists else np.zeros(0, np.int64)


def _same(a, b):
    return bool(a.n_reconstructed == b.n_reconstructed and np.array_equal(a.track_purities, b.track_purities)
                and np.array_equal(a.particle_purities, b.particle_purities))


def measure(d, res, ex, t, full=None):
    """d: the DeviceGraph after its stage; res: run_dev's result; t: TruthTables; full: the host function
    on candidate lists, where the event has a real mapping"""
    scorer = metrics.DeviceScorer(t, d.device)
    s = {}
    # candidates beyond 64 entries take the vote's chunked loop, quadratic in the entries: a workload
    # with a giant candidate is reported, not timed
    longest = max([len(c) for c in extract.outputs_dev(d, res, ex.numhits, ids=True)["extracted"]] or [0])
    if longest > 2000:
        return {"skipped": "a candidate of %d members (the vote's long path is quadratic)" % longest}, scorer, s

    def old_outputs():
        s["o"] = extract.outputs_dev(d, res, ex.numhits, ids=True)

    def old_score_tables():
        s["host"] = host_tables(t, *_flat(s["o"]["extracted"]))

    def old_score_full():
        s["host_full"] = full(*_flat(s["o"]["extracted"]))

    def new_outputs():
        s["b"] = extract.outputs_dev(d, res, ex.numhits, ids=True, lists=False)

    def new_add():
        c = s["b"]["counts"]
        scorer.reset()
        scorer.add(s["b"]["cand_ptr"], s["b"]["cand_ids"], c["n_extracted"], 0, n_members=c["n_extracted_nodes"])

    def new_result():
        s["dev"] = scorer.result()

    old = [("outputs_lists", old_outputs), ("score_tables", old_score_tables)]
    new = [("outputs_no_lists", new_outputs), ("add", new_add), ("result", new_result)]
    r = {"old_parts": {k: _ms(f) for k, f in old}, "new_parts": {k: _ms(f) for k, f in new}}
    r["old"] = _ms(lambda: [f() for _, f in old])
    r["new"] = _ms(lambda: [f() for _, f in new])
    r["old_over_new"] = r["old"]["median_ms"] / r["new"]["median_ms"]
    r["same_result"] = _same(s["host"], s["dev"])
    if full is not None:
        r["old_parts"]["score_full"] = _ms(old_score_full)
        r["old_full"] = _ms(lambda: [old_outputs(), old_score_full()])
        r["old_full_over_new"] = r["old_full"]["median_ms"] / r["new"]["median_ms"]
        r["same_result"] = r["same_result"] and _same(s["host_full"], s["dev"])
    c = s["b"]["counts"]
    ptr, ids = _flat(s["o"]["extracted"])
    total = np.zeros(1, np.int64)
    if c["n_extracted"]:
        total = metrics.majority(len(ptr) - 1, *metrics.candidate_particles(ptr, ids, t.node_id,
                                                                            t.node_ptr.astype(np.int64), t.node_part))[2]
    r.update({"counts": c, "n_reconstructed": s["dev"].n_reconstructed, "n_reference": t.n_reference,
              "truth": {"nodes": int(t.node_id.size), "entries": int(t.node_part.size), "particles": int(t.part_id.size)},
              "candidate_entries": {"min": int(total.min()), "median": float(np.median(total)), "max": int(total.max())}})
    return r, scorer, s


def vol7():
    z = np.load(GOLDEN, allow_pickle=False)
    m = metrics.HitMapping(*(z["map__" + c] for c in ("node_idx", "hit_id", "particle_id", "volume_id", "layer_id",
                                                       "module_id")))
    part = (z["particles__particle_id"], z["particles__px"], z["particles__py"])
    t = metrics.truth_tables(m, *part, 7, 7)
    p, ex = Params(), extract.Params()
    d = pipeline.build_event_dev(PREFIX, 7, 7, p)
    d.clear_errors()
    d.cluster("tse", pipeline.CLUSTER_FIRST[0], pipeline.CLUSTER_FIRST[1], p)
    d.raise_errors()
    res = extract.run_dev(d, d.carried["vivl"], ex, extract.candidate_order_dev(d))
    return d, res, ex, t, lambda ptr, ids: metrics.reconstruction_efficiency(ptr, ids, m, *part, 7, 7)


def synthetic(name):
    g, d, vivl, _ = staged(name)
    ex = extract.Params()
    d.node_id_dev()
    res = extract.run_dev(d, d._dev_from(vivl), ex, extract.candidate_order_dev(d))
    return d, res, ex, fabricated_tables(g), None


def setup(name):
    return vol7() if name == "vol7" else synthetic(name)


def score_only(name):
    d, res, ex, t, _ = setup(name)
    scorer = metrics.DeviceScorer(t, d.device)
    b = extract.outputs_dev(d, res, ex.numhits, ids=True, lists=False)
    c = b["counts"]
    for _ in range(10):
        scorer.reset()
        scorer.add(b["cand_ptr"], b["cand_ids"], c["n_extracted"], 0, n_members=c["n_extracted_nodes"])
    r = scorer.result()
    return {"workload": name, "counts": c, "n_reconstructed": r.n_reconstructed}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--workloads", default="c4,c3")
    ap.add_argument("--score-only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resident_metrics.py needs the MI355X")
    if a.score_only:
        print(json.dumps(score_only(a.score_only)))
        return
    out = {"tool": "resident_metrics", "device": torch.cuda.get_device_name(0), "workloads": {}}
    for name in ["vol7"] + [w for w in a.workloads.split(",") if w]:
        out["workloads"][name] = measure(*setup(name))[0]
    s = json.dumps(out)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
