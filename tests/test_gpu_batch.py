"""A batch of resident events (gtf_graph_concat, gtf_concat_columns, gtf_candidate_order_device_ev,
gtf_event_split, DeviceGraph.concat, pipeline.run_batch, run_pipeline.py --batch) against what it
replaces: gtf.graph.concat of the parts' host graphs, the parts' own order keys, per-event slicing and
pipeline.run(d, None, resident="device") event by event. Everything is compared bit for bit: the batch
moves values and shifts indices, and every candidate's fit runs on the same data in the same order."""
import ctypes
import os
import shutil

import numpy as np
import pytest

import batch_cases as bc
import subset_cases as sc
from gtf import _native as nat
from gtf import graph
from gtf.graph import NODE_FIELDS, SLOT_FIELDS
from test_build import _write_event
from test_gpu_event_pack import _graphs_equal, _same
from test_gpu_graph_subset import _assert_tables_equal

pytestmark = pytest.mark.gpu

GUARD = 64
PREFIX = bc.PREFIX
SYNTHETIC = {21: (400, 300, 10 ** 6, 0.0), 22: (300, 420, 5000, 0.3), 23: (520, 450, 2 ** 40, 0.6)}


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _with_states(d):
    """the states pipeline.build_event_dev computes on a from_event graph"""
    from gtf.params import Params
    if d.n_nodes:
        p = Params()
        d.clear_errors()
        d.track_state_estimates(p)
        d.node_ops(["priors_tse", "mw_tse", "degree"], p)
        d.raise_errors()
        d.refresh_send_mw()
    return d


def _device_part(spec, mem):
    """(DeviceGraph, its host graph, vivl or None) of a batch_cases part"""
    from gtf import pipeline
    from gtf.device import DeviceGraph
    if spec[0] == "subset":
        g, keep = sc.case(spec[1])[:2]
        c = DeviceGraph(g, mem=mem).subset(keep)
        return c, c.to_host(g), None
    if spec[0] == "vol7":      # with its states, priors and weights
        d = pipeline.build_event_dev(PREFIX, 7, 7, mem=mem)
    else:
        d = DeviceGraph.from_event(*bc.columns(spec), mem=mem)
    h, v = d.host_graph()
    if spec[0] != "vol7":
        _graphs_equal(h, bc.host_part(spec)[0], spec)
    return d, h, v


def _resident_equal(c, exp, event):
    """every array the fused DeviceGraph holds against the host concat (an orphan's -1 kept)"""
    assert (c.n_nodes, c.n_slots, c.n_edges, c.n_sub) == (exp.n_nodes, exp.n_slots, exp.n_edges, exp.n_subgraphs)
    for k in ("slot_ptr", "out_ptr", "out_slot"):
        assert _same(c._np(c.t[k]), getattr(exp, k).astype(np.int32)), k
    for fields, host, n in ((NODE_FIELDS, exp.node, exp.n_nodes), (SLOT_FIELDS, exp.slot, exp.n_slots)):
        for f, (dt, shape, _) in fields.items():
            if f in c.t:
                got = c._np(c.t[f]).reshape((n,) + shape)
                if f == "uts_fresh":
                    got = got & 1
                assert _same(got, host[f]), f
    assert _same(c._np(c.carried["event"]), event)


# ---------------------------------------------------------------- 1. DeviceGraph.concat
CONCAT_RUNS = [(n, "torch") for n in bc.CONCAT] + [(n, "hip") for n in ("hand4", "empty_middle", "k65", "orphans")]


@pytest.mark.parametrize("name,mem", CONCAT_RUNS)
def test_concat_equals_host_concat(name, mem):
    from gtf.device import DeviceGraph
    built = [_device_part(s, mem) for s in bc.CONCAT[name]]
    parts = [b[0] for b in built]
    exp = graph.concat([b[1] for b in built])
    event = np.repeat(np.arange(len(parts), dtype=np.int32), [d.n_nodes for d in parts])
    c = DeviceGraph.concat(parts, mem=mem)
    assert c.tables == "device" and c.layout == "natural" and c.mem == mem and c.n_events == len(parts)
    _resident_equal(c, exp, event)
    _assert_tables_equal(c, exp, mem=mem)
    if name == "orphans":
        assert (exp.slot["slot_src"] < 0).sum() > 200 and "vivl" not in c.carried
        with pytest.raises(ValueError, match="node_id|orphan"):
            c.host_graph()
    else:
        h, v = c.host_graph()
        _graphs_equal(h, exp, name)
        assert _same(v, np.concatenate([b[2] for b in built]).reshape(-1, 2))
        assert _same(c._np(c.node_id_dev()), exp.node["node_id"])
    for d, (_, h0, _) in zip(parts, built):   # the parts are read, not changed
        assert _same(d._np(d.t["slot_src"]), h0.slot["slot_src"])


def test_concat_refusals():
    from gtf.device import DeviceGraph
    g = sc.case("tiny200")[0]
    a = DeviceGraph.from_event(*bc.columns(("hand", "two")))
    for kw in (dict(layout="schedule"), dict(pack=True)):
        with pytest.raises(NotImplementedError, match="layout='natural'"):
            DeviceGraph.concat([a, DeviceGraph(g, **kw)])
    with pytest.raises(ValueError, match="allocator"):
        DeviceGraph.concat([a, DeviceGraph.from_event(*bc.columns(("hand", "one")), mem="hip")])
    with pytest.raises(ValueError, match="mem="):
        DeviceGraph.concat([a], mem="hip")
    e = DeviceGraph.concat([])
    assert (e.n_nodes, e.n_slots, e.n_edges, e.n_sub, e.n_events) == (0, 0, 0, 0, 0)


# ---------------------------------------------------------------- 2. the C-ABI between guard bytes
def _guarded(nbytes):
    import torch
    return torch.full((GUARD + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")


def _payload(t, nbytes, dtype):
    h = t.cpu().numpy()
    assert bool((h[:GUARD] == 0xA5).all()) and bool((h[GUARD + nbytes:] == 0xA5).all()), "guard bytes"
    return h[GUARD:GUARD + nbytes].view(dtype)


ABI_COLUMNS = [(0, "gnn"), (0, "layer"), (0, "has_tse"), (0, "degree"), (0, "merged_cov"), (1, "act"),
               (1, "tse_cov"), (1, "tse_rank"), (1, "uts_xyzr"), (1, "edge_mw"), (1, "tse_theta")]


@pytest.mark.parametrize("name", ["midwave", "empty_middle", "k65", "k2050"])
def test_concat_abi_guards(name):
    """gtf_graph_concat + gtf_concat_columns on raw buffers: 34 columns (two launches) of 1-, 4-, 8-, 24-, 32- and
    40-byte rows. k2050: more offsets than the LDS stage holds -- three real parts among 2,048 empty ones."""
    import torch
    L = nat.lib()
    if name == "k2050":
        real = [_device_part(s, "torch") for s in bc.CONCAT["midwave"]]
        where = [0, 1025, 2049]
        built = [(None, bc.empty_graph(), None)] * 2050
        for i, b in zip(where, real):
            built[i] = b
    else:
        built = [_device_part(s, "torch") for s in bc.CONCAT[name]]
    K = len(built)
    hosts = [b[1] for b in built]
    exp = graph.concat(hosts)
    N, S, E = exp.n_nodes, exp.n_slots, exp.n_edges
    adr = lambda d, k: (d.t[k].data_ptr() if d is not None and d.t[k].numel() else 0)  # noqa: E731
    sizes = (nat.GtfConcatSizes * K)(*[nat.GtfConcatSizes(h.n_nodes, h.n_slots, h.n_edges, h.n_subgraphs) for h in hosts])
    ptab = (nat.GtfConcatPart * K)(*[nat.GtfConcatPart(h.n_nodes, h.n_slots, h.n_edges, h.n_subgraphs,
                                                       *[adr(d, k) for k in ("slot_ptr", "slot_src", "out_ptr", "out_slot",
                                                                             "sub_id")]) for (d, h, _) in built])
    cols = ABI_COLUMNS * 3 + [(0, "gnn")]
    assert len(cols) == 34 > nat.CONCAT_MAX_COLUMNS
    srcs = np.array([[adr(d, f) for (d, _, _) in built] for _, f in cols], np.int64)
    tab = torch.from_numpy(np.concatenate([np.frombuffer(ptab, np.int64), srcs.reshape(-1)])).cuda()
    src0 = tab.data_ptr() + ctypes.sizeof(ptab)
    out = {k: _guarded(4 * n) for k, n in (("slot_ptr", N + 1), ("slot_src", S), ("out_ptr", N + 1), ("out_slot", E),
                                           ("sub_id", N), ("event", N))}
    nb = int(L.gtf_graph_concat_workspace_bytes(K))
    ws = _guarded(nb + 192)                 # (GUARD + payload stays 256-byte aligned: torch allocations are)
    wsp = ctypes.c_void_p(ws.data_ptr() + 256)
    co = nat.GtfConcatOut(**{k: ctypes.c_void_p(t.data_ptr() + GUARD) for k, t in out.items()})
    vp = ctypes.c_void_p
    assert L.gtf_graph_concat(sizes, vp(tab.data_ptr()), K, ctypes.byref(co), wsp, nb - 1, _stream()) == -2
    nat.check(L.gtf_graph_concat(sizes, vp(tab.data_ptr()), K, ctypes.byref(co), wsp, nb, _stream()))
    bufs, cc = [], []
    for i, (axis, f) in enumerate(cols):
        dt, shape, _ = (NODE_FIELDS if axis == 0 else SLOT_FIELDS)[f]
        rb = int(np.prod(shape, dtype=np.int64)) * np.dtype(dt).itemsize
        t = _guarded((N if axis == 0 else S) * rb)
        bufs.append(t)
        cc.append(nat.GtfConcatColumn(src0 + 8 * K * i, t.data_ptr() + GUARD, rb, axis))
    nat.check(L.gtf_concat_columns(wsp, K, N, S, (nat.GtfConcatColumn * len(cc))(*cc), len(cc), _stream()))
    event = np.repeat(np.arange(K, dtype=np.int32), [h.n_nodes for h in hosts])
    want = {"slot_ptr": exp.slot_ptr, "slot_src": exp.slot["slot_src"], "out_ptr": exp.out_ptr, "out_slot": exp.out_slot,
            "sub_id": exp.node["sub_id"], "event": event}
    for k, t in out.items():
        assert _same(_payload(t, 4 * want[k].size, np.int32), want[k].astype(np.int32)), k
    h = ws.cpu().numpy()
    assert bool((h[:256] == 0xA5).all()) and bool((h[256 + nb:] == 0xA5).all()), "workspace guard"
    for (axis, f), t in zip(cols, bufs):
        e = (exp.node if axis == 0 else exp.slot)[f]
        assert _same(_payload(t, e.nbytes, e.dtype).reshape(e.shape), e), f
    # refused on the host, nothing written: a bad axis, a row of 0 bytes, a misaligned destination
    t = _guarded(8 * max(N, 1))
    for bad in (nat.GtfConcatColumn(src0, t.data_ptr() + GUARD, 8, 2), nat.GtfConcatColumn(src0, t.data_ptr() + GUARD, 0, 0),
                nat.GtfConcatColumn(src0, t.data_ptr() + GUARD + 4, 8, 0), nat.GtfConcatColumn(0, t.data_ptr() + GUARD, 8, 0)):
        assert L.gtf_concat_columns(wsp, K, N, S, (nat.GtfConcatColumn * 1)(bad), 1, _stream()) == -2
    assert bool((t.cpu().numpy() == 0xA5).all())


# ---------------------------------------------------------------- 3. candidate order on a batch
def _order(d, event=None, ev_call=True):
    """gtf_candidate_order_device[_ev] on d's arrays, through ctypes"""
    from gtf import extract
    sp, nid = extract.sub_ptr_dev(d), d.node_id_dev()
    order = d._dev_empty(max(d.n_nodes, 1), np.int32)
    nb = int(d.lib.gtf_candidate_order_workspace_bytes(d.n_nodes, d.n_slots, d.n_sub))
    ws = d._dev_empty(nb, np.uint8)
    cnt = nat.GtfOrderCounts()
    vp = extract._vp
    a = [ctypes.byref(d.cg_sched), ctypes.byref(d.ce), d.ptr("sub_id"), vp(sp), d.n_sub, vp(nid)]
    b = [vp(order), vp(ws), ctypes.c_size_t(nb), ctypes.byref(cnt), d.stream]
    if ev_call:
        rc = d.lib.gtf_candidate_order_device_ev(*a, vp(event), *b)
    else:
        rc = d.lib.gtf_candidate_order_device(*a, *b)
    return rc, d._np(order)[:d.n_nodes], (cnt.n_components, cnt.n_set_ordered, cnt.max_set_ordered)


def _staged_vol7():
    """the vol-7 event after iteration 1's stage (its activation mask decides the order)"""
    from gtf import pipeline
    from gtf.params import Params
    d = pipeline.build_event_dev(PREFIX, 7, 7)
    d.clear_errors()
    d.cluster("tse", *pipeline.CLUSTER_FIRST, Params())
    d.raise_errors()
    return d


def test_order_ev_null_is_the_existing_call():
    d = _staged_vol7()
    rc0, o0, c0 = _order(d, ev_call=False)
    rc1, o1, c1 = _order(d, None)
    assert rc0 == rc1 == 0 and c0 == c1 and c0[1] > 0 and _same(o0, o1)
    zero = d._dev_zeros(d.n_nodes, np.int32)             # one event: the same rule, the other code path
    rc2, o2, c2 = _order(d, zero)
    assert rc2 == 0 and c2 == c0 and _same(o2, o0)


def test_order_on_the_fused_graph_is_the_parts_orders():
    from gtf.device import DeviceGraph
    parts = [_staged_vol7(), _with_states(DeviceGraph.from_event(*bc.columns(("hand", "perm257")))), _staged_vol7()]
    own = [_order(d, ev_call=False) for d in parts]
    assert all(rc == 0 for rc, _, _ in own) and own[0][2][1] > 0
    c = DeviceGraph.concat(parts)
    rc, o, cnt = _order(c, c.carried["event"])
    assert rc == 0 and _same(o, np.concatenate([x[1] for x in own]))
    assert cnt[0] == sum(x[2][0] for x in own) and cnt[1] == sum(x[2][1] for x in own)
    rc, _, _ = _order(c, None)                           # without the event column the ids collide
    assert rc == -2 and b"duplicate node id" in c.lib.gtf_last_error()
    from gtf import extract
    assert _same(c._np(extract.candidate_order_dev(c))[:c.n_nodes], o)   # (the binding passes the column)


def test_order_refuses_a_duplicate_inside_an_event():
    import torch
    from gtf.device import DeviceGraph
    parts = [DeviceGraph.from_event(*bc.columns(("hand", n))) for n in ("chain65", "two", "chain65")]
    c = DeviceGraph.concat(parts)
    assert _order(c, c.carried["event"])[0] == 0
    ids = c._np(c.t["node_id"]).copy()
    ids[66] = ids[65]                                   # the two nodes of event 1
    c.t["node_id"] = torch.from_numpy(ids).cuda()
    rc, _, _ = _order(c, c.carried["event"])
    assert rc == -2 and b"duplicate node id" in c.lib.gtf_last_error()
    ids[66] = -5
    c.t["node_id"] = torch.from_numpy(ids).cuda()
    assert _order(c, c.carried["event"])[0] == -2 and b"2^61" in c.lib.gtf_last_error()


# ---------------------------------------------------------------- 4. gtf_event_split
def _split(case):
    """gtf_event_split on a batch_cases split case, every output between guard bytes"""
    import torch
    L = nat.lib()
    K, N, lists = case["K"], case["N"], case["lists"]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    dev = {k: (up(p), up(m)) for k, (p, m) in lists.items()}
    event = up(case["event"])
    vp = lambda t: ctypes.c_void_p(t.data_ptr() if t.numel() else 0)  # noqa: E731
    cnt = nat.GtfExtractOutCounts(*bc.counts_of(lists))
    n_pev = cnt.n_extracted + K
    out = {"cand": _guarded(4 * (K + 1)), "rem": _guarded(4 * (K + 1)), "frag": _guarded(4 * (K + 1)),
           "counts": _guarded(24 * K), "pev": _guarded(4 * n_pev)}
    sin = nat.GtfSplitIn(**{f: vp(t) for k, fs in (("cand", ("cand_ptr", "cand_members")), ("rem", ("rem_ptr", "rem_nodes")),
                                                   ("frag", ("frag_ptr", "frag_nodes"))) for f, t in zip(fs, dev[k])})
    sout = nat.GtfSplitOut(*[ctypes.c_void_p(out[k].data_ptr() + GUARD) for k in ("cand", "rem", "frag", "counts", "pev")])
    nb = int(L.gtf_event_split_workspace_bytes(K))
    ws = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    rc = L.gtf_event_split(vp(event), N, K, ctypes.byref(cnt), ctypes.byref(sin), ctypes.byref(sout), vp(ws), nb, _stream())
    got = {k: _payload(out[k], 4 * (K + 1), np.int32) for k in ("cand", "rem", "frag")}
    return rc, got, _payload(out["counts"], 24 * K, np.int32).reshape(K, 6), _payload(out["pev"], 4 * n_pev, np.int32)


@pytest.mark.parametrize("name", list(bc.SPLIT) + ["k257"])
def test_split_equals_the_rule(name):
    case = bc.split_case(name)
    first, counts, pev = bc.split_rule(case["event"], case["K"], case["lists"])
    rc, gfirst, gcounts, gpev = _split(case)
    assert rc == 0, nat.lib().gtf_last_error()
    for k in ("cand", "rem", "frag"):
        assert _same(gfirst[k], first[k]), k
    assert _same(gcounts, counts) and _same(gpev, pev)


@pytest.mark.parametrize("name", ["spanning", "decreasing", "empty_group", "member_range"])
def test_split_refuses_what_breaks_the_rule(name):
    rc, _, _, _ = _split(bc.bad_split_case(name))      # (the guard bytes are checked whatever the status)
    assert rc == -2 and b"gtf_event_split" in nat.lib().gtf_last_error()


def test_split_host_refusals():
    L = nat.lib()
    cnt, sin, sout = nat.GtfExtractOutCounts(), nat.GtfSplitIn(), nat.GtfSplitOut()
    fake = ctypes.c_void_p(256)
    assert L.gtf_event_split(None, 0, 0, ctypes.byref(cnt), ctypes.byref(sin), ctypes.byref(sout), None, 0, None) == 0
    assert L.gtf_event_split(None, 0, 2, None, ctypes.byref(sin), ctypes.byref(sout), fake, 256, None) == -2
    assert L.gtf_event_split(None, 0, 2, ctypes.byref(cnt), ctypes.byref(sin), ctypes.byref(sout), fake, 256, None) == -2
    assert b"output" in L.gtf_last_error()
    full = nat.GtfSplitOut(fake, fake, fake, fake, fake)
    assert L.gtf_event_split(None, 0, 2, ctypes.byref(cnt), ctypes.byref(sin), ctypes.byref(full), fake, 8, None) == -2
    assert b"workspace" in L.gtf_last_error()
    other = nat.GtfSplitIn()
    other.abi_version = nat.ABI_VERSION - 1
    assert L.gtf_event_split(None, 0, 2, ctypes.byref(cnt), ctypes.byref(other), ctypes.byref(full), fake, 256, None) == -3
    assert b"gtf_split_in ABI mismatch" in L.gtf_last_error()
    assert L.gtf_event_split(None, 0, 2, ctypes.byref(cnt), None, ctypes.byref(full), fake, 256, None) == -2
    cnt.n_remaining = 1
    assert L.gtf_event_split(fake, 5, 2, ctypes.byref(cnt), ctypes.byref(sin), ctypes.byref(full), fake, 256, None) == -2
    assert b"missing array" in L.gtf_last_error()


# ---------------------------------------------------------------- 5. the loop
@pytest.fixture(scope="module")
def synthetic_dirs(tmp_path_factory):
    """{seed: an --eventNetwork directory} of the seeded synthetic events"""
    out = {}
    for seed, (n, rows, space, chain) in SYNTHETIC.items():
        d = str(tmp_path_factory.mktemp("ev%d" % seed))
        pre = _write_event(d, seed, n, rows, space, chain)
        for f in ("nodes.csv", "edges.csv"):
            shutil.move(pre + f, os.path.join(d, "event_1_filtered_graph_" + f))
        out[seed] = d
    return out


def _build(spec, dirs=None):
    from gtf import pipeline
    from gtf.device import DeviceGraph
    if spec[0] == "vol7":
        return pipeline.build_event_dev(PREFIX, 7, 7)
    if spec[0] == "synthetic":
        return pipeline.build_event_dev(os.path.join(dirs[spec[1]], "event_1_filtered_graph_"), 7, 8)
    return _with_states(DeviceGraph.from_event(*bc.columns(spec)))


_ALONE = {}


def _alone(spec, dirs=None):
    """pipeline.run on the event alone, computed once: treat as read-only"""
    from gtf import pipeline
    if spec not in _ALONE:
        _ALONE[spec] = pipeline.run(_build(spec, dirs), None, iterations=3, resident="device")
    return _ALONE[spec]


def _records_equal(got, exp, what, lists=True):
    assert [r.index for r in got] == [r.index for r in exp], what
    for a, b in zip(got, exp):
        assert a.stage == b.stage and set(a.seconds) == set(b.seconds) and a.counts == b.counts, (what, a.index)
        for k in ("candidates", "remaining", "fragments"):
            p, q = getattr(a, k), getattr(b, k)
            if not lists:
                assert p is None
                continue
            assert len(p) == len(q) and all(_same(np.asarray(x), np.asarray(y)) for x, y in zip(p, q)), (what, a.index, k)
        for k in ("pval_xy", "pval_zr"):      # bit for bit
            p, q = np.asarray(getattr(a, k), np.float64), np.asarray(getattr(b, k), np.float64)
            assert p.shape == q.shape and np.array_equal(p.view(np.int64), q.view(np.int64)), (what, a.index, k)


def test_run_batch_equals_run_per_event():
    from gtf import metrics, pipeline
    from test_gpu_score import golden
    specs = [("vol7",), ("hand", "perm257"), ("empty",), ("vol7",)]
    ds = [_build(s) for s in specs]
    before = [d._np(d.t["act"]).copy() for d in ds]
    scorers = [metrics.DeviceScorer(golden()[3]) if s == ("vol7",) else None for s in specs]
    its = pipeline.run_batch(ds, iterations=3, scorers=scorers)
    assert len(its) == 4 and its[2] == []
    for e, s in enumerate(specs):
        _records_equal(its[e], _alone(s), s)
    for e in (0, 3):
        assert [len(r.candidates) for r in its[e]] == [1055, 110, 2]
        r = scorers[e].result()
        assert (r.n_reconstructed, r.n_reference, r.efficiency_str) == (133, 163, "81.595")
    assert all(_same(d._np(d.t["act"]), b) for d, b in zip(ds, before))     # the inputs are not modified


@pytest.mark.parametrize("lists", [True, False])
def test_run_batch_synthetic(synthetic_dirs, lists):
    from gtf import pipeline
    specs = [("synthetic", s) for s in SYNTHETIC]
    its = pipeline.run_batch([_build(s, synthetic_dirs) for s in specs], iterations=3, lists=lists)
    for e, s in enumerate(specs):
        exp = _alone(s, synthetic_dirs)
        assert len(exp) >= 1 and exp[0].counts["n_extracted"] + exp[0].counts["n_remaining"] > 0
        _records_equal(its[e], exp, s, lists)
    with pytest.raises(ValueError, match="per event"):
        pipeline.run_batch([_build(specs[0], synthetic_dirs)], scorers=[None, None])
    assert pipeline.run_batch([]) == []


# ---------------------------------------------------------------- 6. the CLI
def test_gpu_pipeline_cli_batch(tmp_path, synthetic_dirs):
    """run_pipeline.py --batch A B writes under ROOTDIR/0 and ROOTDIR/1 the files two single runs write"""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cli = os.path.join(root, "gnn-track-finding_amd", "run_pipeline.py")
    dirs = [os.path.join(bc.GOLDEN, "kat134"), synthetic_dirs[21]]
    common = ["-a", "7", "-z", "8"]
    both = str(tmp_path / "both")
    subprocess.check_call([sys.executable, cli, "--batch"] + dirs + ["-o", both] + common)
    for i, dn in enumerate(dirs):
        one = str(tmp_path / ("one%d" % i))
        subprocess.check_call([sys.executable, cli, "-n", dn, "-o", one, "--resident-event"] + common)
        got = os.path.join(both, str(i))
        files = sorted(os.path.relpath(os.path.join(r, f), one) for r, _, fs in os.walk(one) for f in fs)
        assert files == sorted(os.path.relpath(os.path.join(r, f), got) for r, _, fs in os.walk(got) for f in fs)
        assert sum(f.endswith(".npz") for f in files) >= 1 + 4
        for f in files:
            a, b = os.path.join(one, f), os.path.join(got, f)
            if f.endswith(".npz"):
                with np.load(a) as za, np.load(b) as zb:
                    assert sorted(za.files) == sorted(zb.files), f
                    for k in za.files:
                        assert za[k].dtype == zb[k].dtype and za[k].shape == zb[k].shape and \
                            np.array_equal(za[k], zb[k], equal_nan=za[k].dtype.kind == "f"), (i, f, k)
            elif f.endswith(".csv"):
                assert open(a).read() == open(b).read(), f
            else:
                assert f == "timings.json", f
                assert sorted(json.load(open(a))) == sorted(json.load(open(b)))
    rc = subprocess.run([sys.executable, cli, "--batch"] + dirs + ["-o", str(tmp_path / "x"), "--start", "2"],
                        capture_output=True, text=True)
    assert rc.returncode == 2 and "--start 1" in rc.stderr
