"""The directed a2 cases (tse_cases.py, pinned to the reference by test_tse_cases.py) on the GPU.

All cases, their padded variants and the fillers form one graph (tse_cases.everything()), uploaded
once per allocator and run in one gtf_track_state_estimates_ws call:

  * against the oracle on every node, and against the record of the reference's own
    helper.compute_track_state_estimates on the own nodes of every recorded case, padded variants
    included: the bar of test_gpu_tse.py (1e-6 relative plus 1e-12 of the row's largest entry),
    non-finite entries equal in kind and not compared in value, tse_xyzr and the keys' layout exact;
  * xy_mean_var and zr_mean_var equal the record (and, for the oracle-only cases, the oracle) bit for
    bit at every key count: the gradients are single IEEE operations and the order of the sums is
    numpy's, beyond 128 terms too;
  * GTF_ERR_SINGULAR_H is in the error word and in gtf_diag.node_err at exactly the nodes that hold
    a singular key; those keys' outputs are not compared, every other key and node is;
  * through the C-ABI between guard bytes, with and without a workspace: the same bits, no error
    word without one, nothing written outside the outputs.

The largest relative error per field is printed.
"""
import ctypes
import functools
import os

import numpy as np
import pytest

import tse_cases as TC
from fixtures import GOLDEN
from gtf import _native as nat

pytestmark = pytest.mark.gpu

SINGULAR_H = 128
GUARD = 64   # doubles before and after every output


@functools.lru_cache(maxsize=1)
def world():
    g, comps = TC.everything()
    out, node, sing = TC.run_oracle(g)
    skip = np.zeros(g.n_slots, bool)
    skip[[k for _, k in sing]] = True
    err = np.zeros(g.n_nodes, np.uint32)
    err[[v for v, _ in sing]] = SINGULAR_H
    return dict(g=g, comps=comps, out=out, node=node, skip=skip, err=err,
                record=np.load(os.path.join(GOLDEN, "tse_cases.npz"), allow_pickle=False))


def blank(g):
    h = g.copy()
    for f in TC.FIELDS:
        h.slot[f][:] = np.nan
    return h


@functools.lru_cache(maxsize=None)
def device_run(mem):
    from gtf.device import DeviceGraph
    w = world()
    h = blank(w["g"])
    d = DeviceGraph(h, mem=mem)
    # the schedule is the one the cases were sized for
    cg = d.cg_sched
    assert [cg.n_g4 + cg.n_g8, cg.n_g16, cg.n_g32, cg.n_g64, cg.n_big] == [
        int(sum(1 for s in np.diff(w["g"].slot_ptr) if TC.bucket(s) == b)) for b in (8, 16, 32, 64, 65)]
    node_err = None
    if mem == "torch":
        d.set_diagnostics(node_err=True, edge_chi2=False)
    d.clear_errors()
    x = d.track_state_estimates(TC.P)
    flags = d.errors()
    if mem == "torch":
        node_err = d.diagnostics()["node_err"].copy()
    d.download(h)
    return dict(d=d, got=h, flags=flags, node_err=node_err,
                node={k: (v if isinstance(v, np.ndarray) else v.cpu().numpy()) for k, v in x.items()})


def check(got, exp, rows, name, worst):
    """the bar of test_gpu_tse.py on the rows `rows`, kinds equal, values where exp is finite"""
    a, b = np.asarray(got)[rows], np.asarray(exp)[rows]
    if a.ndim == 1:
        a, b = a[:, None], b[:, None]
    assert np.array_equal(np.isnan(a), np.isnan(b)), (name, "NaN", np.argwhere(np.isnan(a) != np.isnan(b))[:5])
    inf = np.isinf(b) | np.isinf(a)
    assert np.array_equal(a[inf], b[inf]), (name, "inf")
    fin = np.isfinite(b)
    a0, b0 = np.where(fin, a, 0.0), np.where(fin, b, 0.0)
    scale = np.abs(b0).max(axis=1, keepdims=True) if b0.size else b0
    ok = np.abs(a0 - b0) <= 1e-6 * np.abs(b0) + 1e-12 * scale
    rel = np.where(np.abs(b0) > 1e-12 * scale, np.abs(a0 - b0) / np.maximum(np.abs(b0), 1e-300), 0.0)
    worst[name] = max(worst.get(name, 0.0), float(rel.max()) if rel.size else 0.0)
    assert ok.all(), (name, np.argwhere(~ok)[:5], a[~ok][:5], b[~ok][:5])


@pytest.mark.parametrize("mem", ["torch", "hip"])
def test_cases_match_the_oracle(mem):
    w, r = world(), device_run(mem)
    g = w["g"]
    assert r["flags"] == SINGULAR_H
    if r["node_err"] is not None:
        assert np.array_equal(r["node_err"], w["err"]), np.nonzero(r["node_err"] != w["err"])[0][:10]
    rows = (g.slot["tse_rank"] >= 0) & ~w["skip"]
    worst = {}
    for f in TC.FIELDS:
        check(r["got"].slot[f], w["out"].slot[f], rows, f, worst)
    assert np.array_equal(r["got"].slot["tse_xyzr"][rows], w["out"].slot["tse_xyzr"][rows])
    absent = g.slot["tse_rank"] < 0          # nothing is written for an absent key
    for f in TC.FIELDS:
        assert np.isnan(r["got"].slot[f][absent]).all(), f
    allnodes = np.ones(g.n_nodes, bool)
    for f in TC.NODE_FIELDS:
        check(r["node"][f], w["node"][f], allnodes, f, worst)
    for f in ("xy_mean_var", "zr_mean_var"):   # numpy's order of summation: bit for bit
        bad = ~((r["node"][f] == w["node"][f]) | (np.isnan(r["node"][f]) & np.isnan(w["node"][f])))
        assert not bad.any(), (f, [c["case"].name for c in w["comps"]
                                   if bad[c["nodes"][0]:c["nodes"][1]].any()][:8])
    print("a2 cases vs oracle (%s), max rel: %s" % (mem, ", ".join("%s %.3g" % kv for kv in worst.items())))


def test_cases_match_the_reference_record():
    w, r = world(), device_run("torch")
    g, rec = w["g"], w["record"]
    worst, seen = {}, 0
    for c in w["comps"]:
        name = c["case"].name
        if name + "__slot__tse_sv" not in rec.files:
            continue
        n0, own = c["nodes"][0], c["own"]
        nodes = np.arange(n0, n0 + own)
        assert np.array_equal(g.node["node_id"][nodes] % 8192, rec[name + "__node_id"] % 8192)
        # the own nodes' own slots are the record's, in its order (the padding's slots follow them)
        sl = np.concatenate([np.arange(g.slot_ptr[v], g.slot_ptr[v + 1])[g.slot["tse_rank"][g.slot_ptr[v]:g.slot_ptr[v + 1]] >= 0]
                             for v in nodes]).astype(np.int64) if own else np.zeros(0, np.int64)
        assert np.array_equal(g.slot["slot_key"][sl] % 8192, rec[name + "__slot_key"] % 8192), name
        assert np.array_equal(g.slot["tse_rank"][sl], rec[name + "__slot__tse_rank"]), (name, "dict order")
        allrows = np.ones(sl.size, bool)
        for f in TC.FIELDS:
            check(r["got"].slot[f][sl], rec["%s__slot__%s" % (name, f)], allrows, f, worst)
        assert np.array_equal(r["got"].slot["tse_xyzr"][sl], rec[name + "__slot__tse_xyzr"]), name
        for f in TC.NODE_FIELDS:
            check(r["node"][f][nodes], rec["%s__node__%s" % (name, f)], np.ones(own, bool), f, worst)
        for f in ("xy_mean_var", "zr_mean_var"):
            assert np.array_equal(r["node"][f][nodes], rec["%s__node__%s" % (name, f)], equal_nan=True), (name, c["slots"], f)
        seen += 1
    assert seen >= 45 * 2
    print("a2 cases vs reference record, max rel: %s" % ", ".join("%s %.3g" % kv for kv in worst.items()))


def test_allocators_are_bit_equal():
    a, b = device_run("torch"), device_run("hip")
    assert a["flags"] == b["flags"]
    for f in TC.FIELDS:
        assert np.array_equal(a["got"].slot[f], b["got"].slot[f], equal_nan=True), f
    for f in TC.NODE_FIELDS:
        assert np.array_equal(a["node"][f], b["node"][f], equal_nan=True), f


def _guarded(torch, n, dev):
    t = torch.full((n + 2 * GUARD,), -7.25, dtype=torch.float64, device=dev)
    return t, t[GUARD:GUARD + n]


@pytest.mark.parametrize("workspace", [True, False])
def test_c_abi_between_guard_bytes(workspace):
    """gtf_track_state_estimates_ws / gtf_track_state_estimates on outputs of the caller's own,
    each between guard doubles"""
    import torch
    w, r = world(), device_run("torch")
    d, g = r["d"], w["g"]
    N, S = g.n_nodes, g.n_slots
    sizes = dict(sv=3 * S, tau=S, cov=5 * S, xyzr=4 * S, theta=3 * S, var_ms=S, xy=2 * N, zr=2 * N, angle=N, trans=2 * N)
    buf = {k: _guarded(torch, n, d.device) for k, n in sizes.items()}
    vp = lambda k: ctypes.c_void_p(buf[k][1].data_ptr())  # noqa: E731
    st = nat.GtfStates()
    ctypes.memmove(ctypes.byref(st), ctypes.byref(d.ctse), ctypes.sizeof(st))
    st.sv, st.tau, st.cov, st.xyzr = vp("sv"), vp("tau"), vp("cov"), vp("xyzr")
    ex = nat.GtfTseExtra(vp("theta"), vp("var_ms"), vp("xy"), vp("zr"), vp("angle"), vp("trans"))
    cp = d.cparams(TC.P)
    d.clear_errors()
    if workspace:
        nat.check(d.lib.gtf_track_state_estimates_ws(ctypes.byref(d.cg_sched), ctypes.byref(st), ctypes.byref(ex),
                                                     ctypes.byref(cp), d.ptr("ws"), d.stream))
    else:
        nat.check(d.lib.gtf_track_state_estimates(ctypes.byref(d.cg_sched), ctypes.byref(st), ctypes.byref(ex),
                                                  ctypes.byref(cp), d.stream))
    assert d.errors() == (SINGULAR_H if workspace else 0)
    d.clear_errors()
    for k, (whole, _) in buf.items():
        h = whole.cpu().numpy()
        assert (h[:GUARD] == -7.25).all() and (h[-GUARD:] == -7.25).all(), k
    have = np.repeat(g.slot["tse_rank"] >= 0, 1)
    host = {k: v[1].cpu().numpy() for k, v in buf.items()}
    for k, f, width in (("sv", "tse_sv", 3), ("tau", "tse_tau", 1), ("cov", "tse_cov", 5), ("xyzr", "tse_xyzr", 4),
                        ("theta", "tse_theta", 3), ("var_ms", "tse_var_ms", 1)):
        a = host[k].reshape(S, width)
        assert (a[~have] == -7.25).all(), k          # absent keys: untouched
        assert np.array_equal(a[have], r["got"].slot[f].reshape(S, width)[have], equal_nan=True), k
    for k, f in (("xy", "xy_mean_var"), ("zr", "zr_mean_var"), ("angle", "angle_of_rotation"), ("trans", "translation")):
        assert np.array_equal(host[k], r["node"][f].reshape(-1), equal_nan=True), k


def test_device_build_names_the_event_with_a_singular_key(tmp_path):
    """two hits at one (x, y) joined by an edge (x_B == 0): the reference's event conversion stops at
    helper.py:384, and so does the device build, naming or cutting out that event alone. A self loop
    (a node as its own key) is singular too but is not reported (gtf.h): that event converts as ever"""
    from gtf import pipeline
    from test_build import _write_event
    pre = _write_event(str(tmp_path), 21, 400, 300, 10 ** 6, 0.0)    # (random local edges, self loops among them)
    with open(pre + "edges.csv") as f:
        rows = [ln.split(",")[:2] for ln in f.read().splitlines()[2:]]
    assert any(a == b for a, b in rows)
    vol7 = os.path.join(GOLDEN, "kat134", "event_1_filtered_graph_")
    d = pipeline.build_events_dev([vol7, pre], 7, 8, on_error="isolate")
    assert d.event_error_records == {} and d.event_nodes[1] > 0
    # move one end of an edge onto the other end's (x, y)
    with open(pre + "nodes.csv") as f:
        head, *nodes = f.read().splitlines()
    at = {ln.split(",")[0]: i for i, ln in enumerate(nodes)}
    a, b = next((a, b) for a, b in rows if a != b and a in at and b in at)
    fa, fb = nodes[at[a]].split(","), nodes[at[b]].split(",")
    assert fa[4] != fb[4]
    nodes[at[b]] = ",".join(fb[:2] + fa[2:4] + fb[4:])
    with open(pre + "nodes.csv", "w") as f:
        f.write("\n".join([head] + nodes) + "\n")
    with pytest.raises(ValueError, match=r"LinAlgError.*helper\.py:384"):
        pipeline.build_events_dev([vol7, pre], 7, 8)
    with pytest.raises(pipeline.BatchError, match=r"event 1: LinAlgError.*helper\.py:384") as ei:
        pipeline.build_events_dev([vol7, pre], 7, 8, on_error="name")
    assert set(ei.value.events) == {1} and ei.value.events[1] & SINGULAR_H
    d = pipeline.build_events_dev([vol7, pre], 7, 8, on_error="isolate")
    assert set(d.event_error_records) == {1} and d.event_error_records[1].flags & SINGULAR_H
    assert d.event_error_records[1].iteration == 0 and d.event_nodes[1] == 0 and d.event_nodes[0] > 0
    assert d.event_error_records[1].n_raising == 2      # both ends of that edge
    clean = pipeline.build_events_dev([vol7], 7, 8, on_error="isolate")
    assert clean.event_error_records == {} and clean.event_nodes[0] == d.event_nodes[0]
