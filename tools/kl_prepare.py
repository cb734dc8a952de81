"""The host constructor of gtf.parabolic.ParabolicKL against gtf_kl_prepare, and pair_index() + gather
against gtf_kl_pair_rows: what building the parabolic-KL graph costs on either side.

    python tools/kl_prepare.py [out.json] [--copies 1,8,64,256] [--rounds 5]

Per input (the golden vol-7 event and parabolic.batch copies of it) and layout (plain, ordered,
ordered + compact), both sides in every round, after one warm round, median of --rounds:
  * host:        ParabolicKL(..., prepare="host") -- the NumPy build and the upload of what it built;
  * device:      ParabolicKL(..., prepare="device") -- the upload of the raw arrays and gtf_kl_prepare;
  * from_device: ParabolicKL.from_device on arrays that are resident already;
    each by the host clock around a device synchronise;
  * call:        gtf_kl_prepare alone between device events (it synchronises once inside);
  * rows_host:   pair_index() and the emp_var[node] gather (emp_var downloaded), rows_device: rows_dev(),
    host clock around a synchronise.
The outputs are compared first at every size (structure arrays as bytes; the rows exactly); a
difference ends the run. Prints one JSON line (times in milliseconds)."""
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
from gtf import io, parabolic  # noqa: E402
from gtf.parabolic import ParabolicKL  # noqa: E402

LAYOUTS = {"plain": dict(ordered=False, compact=False), "ordered": dict(ordered=True, compact=False),
           "ordered_compact": dict(ordered=True, compact=True)}


def _sync_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def _same(kd, kh):
    for f in ("slot_ptr", "slot_src", "gnn", "truth", "pair_ptr", "q", "truth32"):
        a, b = getattr(kd, f), getattr(kh, f)
        if (a is None) != (b is None) or (a is not None and not torch.equal(a, b)):
            raise SystemExit("kl_prepare: %s differs between the device and the host build" % f)
    if (kd.n_slots, kd.n_pairs, kd.n_listed, kd.scale) != (kh.n_slots, kh.n_pairs, kh.n_listed, kh.scale):
        raise SystemExit("kl_prepare: the counts differ")
    if kh.node_of is not None and not (np.array_equal(kd.node_of, kh.node_of) and np.array_equal(kd.slot_of, kh.slot_of)):
        raise SystemExit("kl_prepare: node_of / slot_of differ")


def _raw_call(res, kw):
    """gtf_kl_prepare on resident inputs and outputs and a workspace allocated once: a function that makes the call"""
    import ctypes
    from gtf import _native as nat
    L = nat.lib()
    sp, ss, gnn, tr = res
    N, S = int(sp.numel()) - 1, int(ss.numel())
    z = lambda n, dt: torch.empty(max(n, 1), dtype=dt, device="cuda")  # noqa: E731
    bufs = [z(N + 1, torch.int32), z(S, torch.int32), z(2 * N, torch.float64), z(N, torch.int64), z(N + 1, torch.int64),
            z(N, torch.int32), z(N, torch.int64), z(S, torch.int64), z(2 * N, torch.int32), z(N, torch.int32)]
    nb = int(L.gtf_kl_prepare_workspace_bytes(N, S))
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    pin = nat.GtfKlPrepareIn(n_nodes=N, n_slots=S, slot_ptr=sp.data_ptr(), slot_src=ss.data_ptr(), gnn=gnn.data_ptr(),
                             truth=tr.data_ptr(), gnn_stride=int(gnn.shape[1]), layout=int(kw["ordered"]),
                             compact=int(kw["compact"]))
    buf = nat.GtfKlPrepareBuf(*[b.data_ptr() for b in bufs])
    g, q, c = nat.GtfKlGraph(), nat.GtfKlQ32(), nat.GtfKlCounts()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run(_keep=(bufs, ws, res)):
        nat.check(L.gtf_kl_prepare(ctypes.byref(pin), ctypes.byref(buf), ctypes.byref(g), ctypes.byref(q), ctypes.byref(c),
                                   ws.data_ptr(), nb, stream))
    return run


def measure(ptr, src, gnn, truth, kw, rounds):
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    res = (up(ptr), up(src), up(gnn), up(truth))
    host = lambda: ParabolicKL(ptr, src, gnn, truth, **kw)  # noqa: E731
    device = lambda: ParabolicKL(ptr, src, gnn, truth, prepare="device", **kw)  # noqa: E731
    resident = lambda: ParabolicKL.from_device(*res, **kw)  # noqa: E731
    kh, kd = host(), device()
    _same(kd, kh)
    _same(resident(), kh)
    dtype = "q32" if kw["compact"] else "f64"
    out = kh.run(kh.alloc(dtype, emp="var"), dtype)

    def rows_host():
        node, i, j = kh.pair_index()
        return node, i, j, out["emp_var"].cpu().numpy()[kh.pair_index(device_nodes=True)[0]]

    rows_device = lambda: kd.rows_dev(out)  # noqa: E731
    a, b = rows_host(), rows_device()
    for x, y in zip(a, (b["node"], b["i"], b["j"], b["emp_var"])):
        if x.tobytes() != y.cpu().numpy().tobytes():
            raise SystemExit("kl_prepare: the pair rows differ")
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    raw = _raw_call(res, kw)

    def call():   # the library call alone, on buffers allocated once (it synchronises once inside)
        ev0.record()
        raw()
        ev1.record()
        ev1.synchronize()
        return ev0.elapsed_time(ev1)

    names = ("host", "device", "from_device", "call_events", "rows_host", "rows_device")
    ts = {n: [] for n in names}
    for r in range(rounds + 1):   # (round 0 warms every path)
        t = {"host": _sync_ms(host)[0], "device": _sync_ms(device)[0], "from_device": _sync_ms(resident)[0],
             "call_events": call(), "rows_host": _sync_ms(rows_host)[0], "rows_device": _sync_ms(rows_device)[0]}
        if r:
            for n in names:
                ts[n].append(t[n])
    o = {n + "_ms": statistics.median(v) for n, v in ts.items()}
    o.update({n + "_min_ms": min(v) for n, v in ts.items()})
    o["host_over_device"] = o["host_ms"] / o["device_ms"]
    o["host_over_from_device"] = o["host_ms"] / o["from_device_ms"]
    o["rows_host_over_device"] = o["rows_host_ms"] / o["rows_device_ms"]
    o["n_pairs"] = kh.n_pairs
    return o


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--copies", default="1,8,64,256")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kl_prepare: no GPU (the device side cannot be measured without one)")
    kat = os.path.join(ROOT, "tests", "golden", "kat134")
    g = io.load_event(os.path.join(kat, "event_1_filtered_graph_"), 7, 7)
    truth = np.asarray(io.read_truth(os.path.join(kat, "truth_vol7.csv"), g.node["node_id"]), np.int64)
    ptr0, src0 = parabolic.in_edge_csr(g)
    res = {"tool": "kl_prepare", "device": torch.cuda.get_device_name(0), "rounds": a.rounds, "inputs": {}}
    for c in [int(x) for x in a.copies.split(",")]:
        ptr, src, gnn, tr = (ptr0, src0, np.asarray(g.node["gnn"], np.float64), truth) if c == 1 else \
            parabolic.batch(ptr0, src0, g.node["gnn"], truth, c)
        e = {"n_nodes": int(ptr.size - 1), "n_in_edges": int(src.size)}
        for name, kw in LAYOUTS.items():
            e[name] = measure(ptr, src, gnn, tr, kw, a.rounds)
        res["inputs"]["vol7_x%d" % c] = e
        print("vol7_x%d" % c, json.dumps(e), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
