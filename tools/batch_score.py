"""Scoring a batch of events: one BatchScorer against one DeviceScorer per event.

    python tools/batch_score.py [out.json] [--copies 1,8,64] [--runs 5]

K copies of the committed vol-7 event (tests/golden/kat134) with its golden truth
(tests/golden/metrics_vol7.npz), resident in GPU memory (tools/batch_loop.py's build; files and truth
columns are read once, on the host, outside every timed window). Timed from the loop's start to the last
Result: pipeline.run_batch(resident, iterations=3, lists=False) and then every event's Result, host
clock around a device synchronise, one warm round and then the median (and the minimum) of `runs`
rounds; a round times all three sides, one after the other, on the same box:
  * none:      no scorer -- the loop alone;
  * per_event: K metrics.DeviceScorer, the code path of the parent commit, unchanged: K adds per
               iteration and K result() calls;
  * batch:     ONE metrics.BatchScorer: one add per iteration, one results().
The scorers are made before the clock starts (their tables are on the device already) and reset
between rounds. Every Result is checked: 133 / 163. "scoring" is a scored side minus the unscored one.
Also timed on their own, between device synchronises: K x metrics.truth_tables_dev from the uploaded
columns (what every side pays today), and the one metrics.truth_concat_dev of the K device tables that
the batch side adds -- what a batched truth build could still win is the first of the two.
Prints one JSON line (times in milliseconds)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gnn-track-finding_amd"), os.path.dirname(os.path.abspath(__file__))]
import torch  # noqa: E402
from batch_loop import build, columns  # noqa: E402
from gtf import metrics, pipeline  # noqa: E402
from gtf.params import Params  # noqa: E402

EXPECT = (133, 163)


def _stats(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "runs": len(ts)}


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def truth_columns():
    z = np.load(os.path.join(ROOT, "tests", "golden", "metrics_vol7.npz"), allow_pickle=False)
    m = metrics.HitMapping(*(torch.from_numpy(z["map__" + c].astype(np.int64)).cuda() for c in metrics.MAPPING_COLUMNS))
    part = [torch.from_numpy(np.ascontiguousarray(z["particles__" + c], dt)).cuda()
            for c, dt in (("particle_id", np.int64), ("px", np.float64), ("py", np.float64))]
    return m, part


def _check(results):
    for r in results:
        if (r.n_reconstructed, r.n_reference) != EXPECT:
            raise SystemExit("batch_score.py: an event gave %d / %d, not %d / %d"
                             % ((r.n_reconstructed, r.n_reference) + EXPECT))


def measure(K, cols, truth, runs):
    p = Params()
    m, part = truth
    resident = [build(cols, p) for _ in range(K)]      # run_batch does not modify them
    tables, t_build, t_concat = None, [], []
    for rnd in range(runs + 1):
        t, tables = _timed(lambda: [metrics.truth_tables_dev(m, *part, 7, 7) for _ in range(K)])
        tc, batch = _timed(lambda: metrics.truth_concat_dev(tables))
        if rnd:
            t_build.append(t)
            t_concat.append(tc)
    per = [metrics.DeviceScorer(t) for t in tables]
    one = metrics.BatchScorer(batch)
    sides = {"none": [], "per_event": [], "batch": []}

    def per_event():
        pipeline.run_batch(resident, iterations=3, scorers=per, lists=False)
        return [s.result() for s in per]

    def batched():
        pipeline.run_batch(resident, iterations=3, scorers=one, lists=False)
        return one.results()

    for rnd in range(runs + 1):
        for s in per:
            s.reset()
        one.reset()
        t0, _ = _timed(lambda: pipeline.run_batch(resident, iterations=3, lists=False))
        t1, res = _timed(per_event)
        _check(res)
        t2, res = _timed(batched)
        _check(res)
        if rnd:      # (round 0 warms every side)
            for k, t in zip(("none", "per_event", "batch"), (t0, t1, t2)):
                sides[k].append(t)
    out = {"copies": K, "truth_rows": int(m.node_idx.numel()), "n_particles_sum": one.R}
    out.update({k: _stats(v) for k, v in sides.items()})
    out["truth_tables_dev_x_K"], out["truth_concat_dev"] = _stats(t_build), _stats(t_concat)
    none = out["none"]["median_ms"]
    out["scoring_ms"] = {"per_event": out["per_event"]["median_ms"] - none, "batch": out["batch"]["median_ms"] - none}
    out["scoring_per_event_ms"] = {k: v / K for k, v in out["scoring_ms"].items()}
    out["per_event_over_batch"] = out["per_event"]["median_ms"] / out["batch"]["median_ms"]
    out["batch_median_below_per_event_min"] = out["batch"]["median_ms"] < out["per_event"]["min_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--copies", default="1,8,64")
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("batch_score.py needs the MI355X")
    cols, truth = columns(), truth_columns()
    res = {"tool": "batch_score", "device": torch.cuda.get_device_name(0), "event": "tests/golden/kat134, volume 7",
           "iterations": 3, "batches": [measure(int(k), cols, truth, a.runs) for k in a.copies.split(",") if k]}
    s = json.dumps(res)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
