"""What run_batch's error policy costs, and what it saves when one event of a batch raises.

    python tools/batch_errors.py [out.json] [--copies 1,8,64] [--runs 5]

Clean batches: K copies of the committed vol-7 event (tests/golden/kat134), built in GPU memory as
pipeline.build_event_dev builds them (the CSV files are parsed once, on the host, outside every timed
window). Timed from K resident events to the last iteration's records, three iterations, host clock around
a device synchronise, one warm round and then `runs` rounds; a round times both modes one after the other
on the same resident events (run_batch does not modify a list's parts):
  * raise:   pipeline.run_batch(ds) -- the parent commit's path, unchanged;
  * isolate: pipeline.run_batch(ds, on_error="isolate") on a batch in which nothing raises: per stage one
    zero fill of 4 N bytes and the registration (DeviceGraph.track_node_errors), nothing else.
Both give every event's 1,055 / 110 / 2 candidates (checked on every round). "registration" is one
track_node_errors() on the fused graph between two synchronises (three stages and one update() make four
of them per run).

One raising event: the committed 800' event (tests/golden/kat800, volumes 7-14, raises in iteration 1)
at index 3 among K - 1 vol-7 events, K = 8 and 64:
  * isolate: run_batch(ds, on_error="isolate"): the whole batch, 800' cut out in iteration 1;
  * today:   run_batch(ds) until it raises, then the K - 1 survivors one by one with
    pipeline.run(d, None, resident="device") (freshly built before the clock starts: run() works on its
    input) -- what a user of the parent commit does after the batch died;
  * the failing iteration's extra work on its own: DeviceGraph.event_errors (gtf_event_errors and its one
    copy back) between device events, and the subset(keep) that cuts the event out, host clock around a
    synchronise.
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
from gtf import io, pipeline  # noqa: E402
from gtf.device import DeviceGraph  # noqa: E402
from gtf.params import Params  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
VOL7 = (os.path.join(GOLDEN, "kat134", "event_1_filtered_graph_"), 7, 7)
KAT800 = (os.path.join(GOLDEN, "kat800", "event_1_filtered_graph_"), 7, 14)
EXPECT = [1055, 110, 2]
AT = 3   # where the raising event stands


def _stats(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "runs": len(ts)}


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def columns(prefix, lo, hi):
    ids, x, y, z, r, layer = io.read_nodes(prefix + "nodes.csv", lo, hi)
    n2, n1 = io.read_edges(prefix + "edges.csv")
    return ids, x, y, z, r, layer, n1, n2


def build(cols, p):
    """pipeline.build_event_dev from the parsed columns"""
    return pipeline._event_states(DeviceGraph.from_event(*cols), p)


def _check(records, skip=()):
    for e, recs in enumerate(records):
        got = [r.counts["n_extracted"] for r in recs]
        if got != ([] if e in skip else EXPECT):
            raise SystemExit("batch_errors.py: event %d gave %r candidates" % (e, got))


def clean(K, cols, runs):
    p = Params()
    ds = [build(cols, p) for _ in range(K)]
    t = {"raise": [], "isolate": []}
    for rnd in range(runs + 1):
        for mode in ("raise", "isolate"):
            ms, recs = _timed(lambda: pipeline.run_batch(ds, iterations=3, on_error=mode))
            _check(recs)
            if mode == "isolate" and recs.errors:
                raise SystemExit("batch_errors.py: a clean batch reported %r" % recs.errors)
            if rnd:      # (round 0 warms both)
                t[mode].append(ms)
    # what isolate adds per stage, on its own: the allocation, the zero fill and the 64-byte registration
    fused, reg, idle = DeviceGraph.concat(ds), [], []
    for rnd in range(runs + 1):
        ms, _ = _timed(fused.track_node_errors)
        ms0, _ = _timed(lambda: None)     # (the clock and the two synchronises alone)
        if rnd:
            reg.append(ms)
            idle.append(ms0)
    out = {"copies": K, "n_nodes": sum(d.n_nodes for d in ds), "raise": _stats(t["raise"]), "isolate": _stats(t["isolate"]),
           "registration": _stats(reg), "empty_window": _stats(idle), "registrations_per_run": 4}
    out["isolate_over_raise"] = out["isolate"]["median_ms"] / out["raise"]["median_ms"]
    out["isolate_median_above_raise_max"] = out["isolate"]["median_ms"] > out["raise"]["max_ms"]
    return out


def one_raising(K, cols7, cols800, runs):
    p = Params()
    ds = [build(cols800 if e == AT else cols7, p) for e in range(K)]
    iso, today, died, reduce_ms, subset_ms = [], [], [], [], []

    def as_today(fresh):
        try:
            pipeline.run_batch(ds, iterations=3)
        except ValueError:
            pass
        else:
            raise SystemExit("batch_errors.py: the batch with the 800' event did not raise")
        t_died = time.perf_counter()
        return t_died, [pipeline.run(d, None, iterations=3, resident="device") for d in fresh]

    for rnd in range(runs + 1):
        ms, recs = _timed(lambda: pipeline.run_batch(ds, iterations=3, on_error="isolate"))
        _check(recs, skip=(AT,))
        if set(recs.errors) != {AT} or recs.errors[AT].flags != 8:
            raise SystemExit("batch_errors.py: expected the 800' event alone to raise, got %r" % recs.errors)
        fresh = [build(cols7, p) for _ in range(K - 1)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ms2, (t_died, recs2) = _timed(lambda: as_today(fresh))
        _check(recs2)
        del fresh
        # the failing iteration's extra work, on a fused graph after its stage
        fused = DeviceGraph.concat(ds)
        fused.clear_errors()
        fused.track_node_errors()
        fused.cluster("tse", *pipeline.CLUSTER_FIRST, p)
        if fused.errors() != 8:
            raise SystemExit("batch_errors.py: the fused graph's error word is not GTF_ERR_TIE_EMPTIED")
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        r = fused.event_errors()
        b.record()
        torch.cuda.synchronize()
        ms3, child = _timed(lambda: fused.subset(r["keep"], carry={"vivl": fused.carried["vivl"],
                                                                   "event": fused.carried["event"]}, keep_fresh=True))
        if [int(e) for e in r["err_ev"].nonzero()[0]] != [AT] or child.n_nodes != fused.n_nodes - ds[AT].n_nodes:
            raise SystemExit("batch_errors.py: event_errors / subset did not cut the 800' event")
        if rnd:
            iso.append(ms)
            today.append(ms2)
            died.append((t_died - t0) * 1e3)
            reduce_ms.append(a.elapsed_time(b))
            subset_ms.append(ms3)
    out = {"events": K, "raising_event_at": AT, "n_nodes": sum(d.n_nodes for d in ds), "isolate": _stats(iso),
           "today": _stats(today), "today_until_the_batch_died": _stats(died), "event_errors": _stats(reduce_ms),
           "subset_cut": _stats(subset_ms)}
    out["today_over_isolate"] = out["today"]["median_ms"] / out["isolate"]["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--copies", default="1,8,64")
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("batch_errors.py needs the MI355X")
    cols7, cols800 = columns(*VOL7), columns(*KAT800)
    res = {"tool": "batch_errors", "device": torch.cuda.get_device_name(0), "iterations": 3,
           "clean": [clean(int(k), cols7, a.runs) for k in a.copies.split(",") if k],
           "one_raising": [one_raising(K, cols7, cols800, a.runs) for K in (8, 64)]}
    s = json.dumps(res)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
