"""The truth tables of a batch of events: one batched build against one build per event and a concat.

    python tools/batch_truth.py [out.json] [--copies 1,8,64] [--runs 5]

K copies of the golden vol-7 truth columns (tests/golden/metrics_vol7.npz: 13,129 mapping rows, 1,934
particles), uploaded once, outside every timed window. Both sides start from those device columns and end
with a DeviceTruthBatch that a BatchScorer takes; host clock around a device synchronise, one warm round
and then the median (and the minimum) of `runs` rounds; a round times both sides, one after the other:
  * per_event: K x metrics.truth_tables_dev and one metrics.truth_concat_dev -- the code path of the
               parent commit, unchanged;
  * batch:     ONE metrics.truth_tables_batch_dev: the columns gathered end to end (gtf_graph_concat's
               offsets, gtf_concat_columns) and one gtf_truth_build_ev. "build_device" is that library
               call alone, between two device events.
The two results are compared once per K (the nine arrays, array_equal) and every event's counts are
checked: T = 8,748, P = 13,129, R = 246, 163 reference tracks. Prints one JSON line (times in
milliseconds)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gnn-track-finding_amd")]
import torch  # noqa: E402
from gtf import metrics  # noqa: E402

EXPECT = (8748, 13129, 246, 163)
FIELDS = ("node_id", "node_ptr", "node_part", "part_id", "part_hits", "part_ref", "node_off", "entry_off", "part_off")


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


def _check(K, a, b):
    ha, hb = a.host(), b.host()
    for f in FIELDS:
        if not np.array_equal(getattr(ha, f), getattr(hb, f)):
            raise SystemExit("batch_truth.py: %s differs between the two sides at K = %d" % (f, K))
    for e in range(K):
        got = tuple(int(getattr(hb, f)[e + 1] - getattr(hb, f)[e]) for f in ("node_off", "entry_off", "part_off")) + \
            (b.n_reference[e],)
        if got != EXPECT or a.n_reference[e] != EXPECT[3]:
            raise SystemExit("batch_truth.py: event %d gave %r, not %r" % (e, got, EXPECT))


def measure(K, truth, runs):
    m, part = truth
    parts = [(m,) + tuple(part)] * K
    marks = []

    def mark(what):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        marks.append(ev)

    sides = {"per_event": [], "batch": [], "build_device": []}
    for rnd in range(runs + 1):
        t0, a = _timed(lambda: metrics.truth_concat_dev([metrics.truth_tables_dev(m, *part, 7, 7) for _ in range(K)]))
        del marks[:]
        t1, b = _timed(lambda: metrics._truth_tables_batch_dev(parts, 7, 7, "cuda", "torch", mark))
        if rnd == 0:      # (round 0 warms both sides)
            _check(K, a, b)
            continue
        sides["per_event"].append(t0)
        sides["batch"].append(t1)
        sides["build_device"].append(marks[0].elapsed_time(marks[1]))
    out = {"copies": K, "rows": K * int(m.node_idx.numel()), "particles": K * int(part[0].numel())}
    out.update({k: _stats(v) for k, v in sides.items()})
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
        raise SystemExit("batch_truth.py needs the MI355X")
    truth = truth_columns()
    res = {"tool": "batch_truth", "device": torch.cuda.get_device_name(0), "event": "tests/golden/metrics_vol7.npz, volume 7",
           "batches": [measure(int(k), truth, a.runs) for k in a.copies.split(",") if k]}
    s = json.dumps(res)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
