"""The device subset on the GPU (DeviceGraph.subset / refresh_send_mw / to_host over
gtf_graph_subset_plan / _apply, gtf_subset_gather and gtf_refresh_send_mw) against the host
definition gtf.graph.subset / refresh_send_mw, which tests/test_subset.py pins to pack() of the
reduced networkx graphs. Every comparison is exact. The inputs are tests/subset_cases.py's
(checked on the CPU by tests/test_subset_cases.py)."""
import ctypes

import numpy as np
import pytest

import subset_cases as sc
from gtf import _native as nat
from gtf import graph
from gtf.graph import NODE_FIELDS, SLOT_FIELDS
from gtf.params import Params
from test_gpu_graph_prepare import COUNTS, TABLES

pytestmark = pytest.mark.gpu
GUARD = 64


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(a, b, equal_nan=a.dtype.kind == "f"))


def _assert_graphs_equal(got, exp, what=""):
    assert (got.n_nodes, got.n_slots, got.n_edges, got.n_subgraphs) == \
        (exp.n_nodes, exp.n_slots, exp.n_edges, exp.n_subgraphs), what
    for k in ("slot_ptr", "out_ptr", "out_slot"):
        assert _same(getattr(got, k), getattr(exp, k)), (what, k)
    for k in NODE_FIELDS:
        assert _same(got.node[k], exp.node[k]), (what, k)
    for k in SLOT_FIELDS:
        assert _same(got.slot[k], exp.slot[k]), (what, k)


def _assert_tables_equal(child, h, **kw):
    """the child's solo, tables and counts against DeviceGraph(h, tables="device") of the host-made h"""
    from gtf.device import DeviceGraph
    ref = DeviceGraph(h, tables="device", **kw)
    assert child.tables == "device"
    n_o = [ref.cg_sched.n_o4, ref.cg_sched.n_o8, ref.cg_sched.n_o16]
    written = {"out_sched": 4 * sum(n_o), "out_lanes": 2 * (4 * n_o[0] + 8 * n_o[1])}   # (capacities)
    for name in ("solo",) + TABLES:
        assert (name in ref.t) == (name in child.t), name
        if name in ref.t:
            a, b = ref._np(ref.t[name]), child._np(child.t[name])
            n = min(written.get(name, a.size), a.size)
            assert a.size == b.size and _same(a[:n], b[:n]), name
    for f in COUNTS:
        assert getattr(ref.cg, f) == getattr(child.cg, f), f
        assert getattr(ref.cg_sched, f) == getattr(child.cg_sched, f), f
    for f in TABLES:
        assert bool(getattr(ref.cg, f)) == bool(getattr(child.cg, f)), f


@pytest.mark.parametrize("name,mem", [(n, "torch") for n in sc.NAMES] + [("boundary", "hip"), ("tiny200", "hip")])
def test_subset_equals_host(name, mem):
    from gtf.device import DeviceGraph
    g, keep, h, nm, sm = sc.case(name)
    d = DeviceGraph(g, mem=mem)
    c = d.subset(keep)
    assert (c.n_nodes, c.n_slots, c.n_edges, c.n_sub) == (h.n_nodes, h.n_slots, h.n_edges, h.n_subgraphs)
    assert _same(c._np(c.t["node_map"]), nm.astype(np.int32)) and _same(c._np(c.t["slot_map"]), sm.astype(np.int32))
    got = c.to_host(g)
    graph.check_layout(got)
    _assert_graphs_equal(got, h, "subset")
    _assert_tables_equal(c, h, mem=mem)
    c.refresh_send_mw()   # the input's send_mw is consistent, so the refresh changes nothing
    _assert_graphs_equal(c.to_host(g), h, "refreshed")
    if name == "all":
        assert _same(c._np(c.t["node_map"]), np.arange(g.n_nodes, dtype=np.int32))
        assert _same(c._np(c.t["slot_map"]), np.arange(g.n_slots, dtype=np.int32))
        _assert_graphs_equal(got, graph.subset(g, np.ones(g.n_nodes, bool)), "all")
    if name == "none":
        assert c.n_nodes == 0 and c.n_slots == 0 and c.n_edges == 0
        p = Params()
        c.clear_errors()
        c.extrapolate(p)
        c.update(p)
        c.cluster("uts", 1000.0, 100.0, p)
        c.cluster("tse", 1.0, 2.0, p)
        c.full_pass(p)
        c.refresh_send_mw()
        assert c.errors() == 0
        e = c.subset(np.zeros(0, bool))   # and an empty graph cuts to an empty graph
        assert e.n_nodes == 0 and e.to_host(got).n_nodes == 0


def test_device_mask_and_replaced_coordinates():
    import torch
    from gtf.device import DeviceGraph
    g, keep, _, _, _ = sc.case("tiny200")
    rng = np.random.default_rng(3)
    gnn = g.node["gnn"] + rng.normal(0, 1, g.node["gnn"].shape)
    g2 = g.copy()
    g2.node["gnn"] = gnn
    h = graph.refresh_send_mw(graph.subset(g2, keep))
    d = DeviceGraph(g)
    kd = torch.from_numpy(keep.astype(np.uint8)).to(d.device)
    c = d.subset(kd, gnn=torch.from_numpy(gnn).to(d.device))
    _assert_graphs_equal(c.to_host(g), h, "device arrays")
    _assert_tables_equal(c, h)   # (the sender coordinates of the tables are the replaced ones)
    c = d.subset(keep, gnn=gnn)
    _assert_graphs_equal(c.to_host(g), h, "host arrays")
    assert _same(d._np(d.t["gnn"]).reshape(-1, 4), g.node["gnn"])   # the parent keeps its own
    with pytest.raises(ValueError, match="keep"):
        d.subset(keep[:-1])
    with pytest.raises(ValueError, match="gnn"):
        d.subset(keep, gnn=gnn[:-1])


def test_other_layouts_are_refused():
    from gtf.device import DeviceGraph
    g, keep, _, _, _ = sc.case("tiny200")
    for kw in (dict(layout="schedule"), dict(layout="tiled", tile=64), dict(layout="padded", tile=64), dict(pack=True)):
        with pytest.raises(NotImplementedError, match="layout='natural'"):
            DeviceGraph(g, **kw).subset(keep)
    with pytest.raises(ValueError, match="subset"):
        DeviceGraph(g).to_host(g)


# ---- through ctypes: bounds, optional outputs, column shapes ----
class Raw:
    """a parent on the device, its plan in a workspace, and guarded output buffers"""

    def __init__(self, name):
        import torch
        from gtf.device import DeviceGraph
        self.torch = torch
        self.g, self.keep, self.h, self.nm, self.sm = sc.case(name)
        self.d = DeviceGraph(self.g)
        self.L = self.d.lib
        g, d = self.g, self.d
        self.cg = d._base_graph()
        nb = int(self.L.gtf_graph_subset_workspace_bytes(g.n_nodes, g.n_slots, g.n_edges, d.n_sub))
        self.ws = torch.empty(nb + GUARD, dtype=torch.uint8, device="cuda")
        self.ws[nb:] = 0xA5
        self.nb = nb
        self.keep_t = torch.from_numpy(self.keep.astype(np.uint8)).cuda()
        self.counts = nat.GtfSubsetCounts()
        rc = self.L.gtf_graph_subset_plan(ctypes.byref(self.cg), d.ptr("tse_rank"), d.ptr("uts_rank"), d.ptr("sub_id"),
                                          d.n_sub, ctypes.c_void_p(self.keep_t.data_ptr()),
                                          ctypes.c_void_p(self.ws.data_ptr()), ctypes.c_size_t(nb),
                                          ctypes.byref(self.counts), d.stream)
        assert rc == 0, self.L.gtf_last_error()

    def buf(self, nbytes):
        return self.torch.full((nbytes + GUARD,), 0xA5, dtype=self.torch.uint8, device="cuda")

    def gather(self, axis, cols):
        arr = (nat.GtfColumn * len(cols))(*cols)
        rc = self.L.gtf_subset_gather(ctypes.c_void_p(self.ws.data_ptr()), axis, arr, len(cols), self.d.stream)
        self.torch.cuda.synchronize()
        return rc


@pytest.fixture(scope="module")
def raw():
    return Raw("boundary")


def _guard_ok(b):
    return bool((b[-GUARD:] == 0xA5).all())


def test_plan_counts_and_workspace_guard(raw):
    c, h = raw.counts, raw.h
    assert (c.n_nodes, c.n_slots, c.n_edges, c.n_sub) == (h.n_nodes, h.n_slots, h.n_edges, h.n_subgraphs)
    raw.torch.cuda.synchronize()
    assert _guard_ok(raw.ws)


def test_apply_guard_bytes_and_optional_outputs(raw):
    h = raw.h
    N2, S2, E2 = h.n_nodes, h.n_slots, h.n_edges
    exp = {"node_map": raw.nm.astype(np.int32), "slot_map": raw.sm.astype(np.int32), "slot_ptr": h.slot_ptr,
           "slot_src": h.slot["slot_src"], "out_ptr": h.out_ptr, "out_slot": h.out_slot, "sub_id": h.node["sub_id"]}
    sub = h.node["sub_id"]
    exp["solo"] = (np.bincount(sub)[sub] == 1).astype(np.uint8)
    assert exp["solo"].sum() >= 1
    for names in (tuple(exp), ("slot_src", "out_slot"), ("node_map",)):
        bufs = {n: raw.buf(exp[n].nbytes) for n in names}
        out = nat.GtfSubsetOut(**{n: ctypes.c_void_p(b.data_ptr()) for n, b in bufs.items()})
        assert raw.L.gtf_graph_subset_apply(ctypes.byref(raw.cg), ctypes.c_void_p(raw.ws.data_ptr()), ctypes.byref(out),
                                            raw.d.stream) == 0
        raw.torch.cuda.synchronize()
        for n, b in bufs.items():
            assert _guard_ok(b), n
            assert _same(b[:-GUARD].cpu().numpy().view(exp[n].dtype), exp[n]), n
    assert (N2, S2, E2) == (exp["node_map"].size, exp["slot_map"].size, exp["out_slot"].size)
    assert _guard_ok(raw.ws)


def test_gather_every_graph_column_with_guards(raw):
    g, h, d = raw.g, raw.h, raw.d
    for axis, rows, fields, names in ((0, h.n_nodes, NODE_FIELDS, [f for f in NODE_FIELDS if f in d.t and f != "sub_id"]),
                                      (1, h.n_slots, SLOT_FIELDS, [f for f in SLOT_FIELDS if f in d.t and f != "slot_src"])):
        bufs, cols = {}, []
        for f in names:
            dt, shape, _ = fields[f]
            rb = int(np.prod(shape, dtype=np.int64)) * np.dtype(dt).itemsize
            bufs[f] = raw.buf(rows * rb)
            cols.append(nat.GtfColumn(d.ptr(f), ctypes.c_void_p(bufs[f].data_ptr()), rb,
                                      d.SUBSET_FILL.get(f, nat.COL_COPY) if axis else nat.COL_COPY))
        assert raw.gather(axis, cols) == 0
        for f in names:
            dt, shape, _ = fields[f]
            exp = (h.node if axis == 0 else h.slot)[f]
            if f == "send_mw":   # (h's was refreshed; the gather copies the parent's, which is consistent)
                exp = graph.subset(g, raw.keep).slot[f]
            assert _guard_ok(bufs[f]), f
            assert _same(bufs[f][:-GUARD].cpu().numpy().view(dt).reshape((rows,) + shape), exp), f


@pytest.mark.parametrize("axis", [0, 1])
def test_gather_column_shapes_and_fills(raw, axis):
    """1-, 4-, 8-, 24- and 40-byte rows with every fill kind in one call (and 40 more columns, so
    the table goes over in two launches), misaligned single bytes included, against NumPy"""
    torch = raw.torch
    rng = np.random.default_rng(9)
    old = raw.g.n_slots if axis else raw.g.n_nodes
    idx = raw.sm if axis else raw.nm
    orphan = raw.h.slot["slot_src"] < 0 if axis else np.zeros(idx.size, bool)
    assert not axis or (orphan.sum() > 100 and (~orphan).sum() > 100)
    rows = idx.size
    cols, checks, hold = [], [], []
    kinds = [(rb, fill) for fill in (nat.COL_COPY, nat.COL_ZERO_ORPHAN, nat.COL_NAN_ORPHAN, nat.COL_ZERO_ALL)
             for rb in (1, 4, 8, 24, 40) if fill != nat.COL_NAN_ORPHAN or rb % 8 == 0]
    kinds += [(8, nat.COL_COPY)] * 40 + [(3, nat.COL_COPY), (12, nat.COL_ZERO_ORPHAN), (1000, nat.COL_COPY)]
    for i, (rb, fill) in enumerate(kinds):
        off = 1 if rb in (1, 3) and i % 2 else 0   # (a byte column need not be aligned)
        src = rng.integers(1, 255, (old, rb), dtype=np.uint8)
        s = torch.zeros(old * rb + 8, dtype=torch.uint8, device="cuda")
        s[off:off + old * rb] = torch.from_numpy(src.reshape(-1)).cuda()
        b = raw.buf(rows * rb + 8)
        hold += [s, b]
        cols.append(nat.GtfColumn(ctypes.c_void_p(s.data_ptr() + off) if fill != nat.COL_ZERO_ALL or i % 2 else None,
                                  ctypes.c_void_p(b.data_ptr() + off), rb, fill))
        exp = src[idx].copy()
        if fill == nat.COL_ZERO_ALL:
            exp[:] = 0
        elif fill == nat.COL_ZERO_ORPHAN:
            exp[orphan] = 0
        elif fill == nat.COL_NAN_ORPHAN:
            exp[orphan] = np.frombuffer(np.full(rb // 8, np.nan).tobytes(), np.uint8)
        checks.append((b, off, exp))
    assert raw.gather(axis, cols) == 0
    for i, (b, off, exp) in enumerate(checks):
        got = b.cpu().numpy()
        assert np.all(got[:off] == 0xA5) and np.all(got[off + exp.size:] == 0xA5), kinds[i]
        assert np.array_equal(got[off:off + exp.size].reshape(exp.shape), exp), kinds[i]


# ---- send weights ----
@pytest.mark.parametrize("name", ["boundary", "tiny200", "dropin_extract_input_again"])
def test_refresh_send_mw_equals_host(name):
    from gtf.device import DeviceGraph
    g = sc.case(name)[0].copy()
    rng = np.random.default_rng(4)
    g.slot["tse_mw"] = rng.uniform(0, 1, g.n_slots)
    edges = np.nonzero(g.slot["is_edge"] == 1)[0]
    clear = rng.choice(g.n_slots, g.n_slots // 5, replace=False)   # some senders lose the entry
    g.slot["tse_rank"][clear] = -1
    g.slot["send_mw"][:] = 7.0
    exp = graph.refresh_send_mw(g.copy()).slot["send_mw"]
    if name != "boundary":   # (the boundary graph's senders hold no slot: every weight is absent there)
        assert np.isfinite(exp[edges]).sum() > 20 and np.isnan(exp[edges]).sum() > 20
    assert np.all(np.isnan(exp[g.slot["is_edge"] == 0]))
    for kw in (dict(), dict(schedule=False, classes=False)):   # with slot_dst from the tables, and the same struct
        d = DeviceGraph(g, **kw)
        d.refresh_send_mw()
        assert _same(d._np(d.t["send_mw"]), exp)
    # without slot_dst in the struct: the receiver by binary search
    cg = d._base_graph()
    d.t["send_mw"].fill_(3.0)
    assert d.lib.gtf_refresh_send_mw(ctypes.byref(cg), d.ptr("tse_rank"), d.ptr("tse_mw"), d.ptr("send_mw"),
                                     d.stream) == 0
    assert _same(d._np(d.t["send_mw"]), exp)


# ---- the stages see the same graph ----
def test_stages_bit_equal_on_the_child():
    from gtf.device import DeviceGraph
    g, keep, h, _, _ = sc.case("tiny200")
    p = Params()

    def stages(d):
        d.clear_errors()
        d.extrapolate(p)
        d.update(p)
        d.cluster("uts", 1000.0, 100.0, p)
        return d.errors()

    c = DeviceGraph(g).subset(keep)
    ref = DeviceGraph(h)
    fa, fb = stages(c), stages(ref)
    assert fa == fb
    exp = ref.download(h.copy())
    assert int((exp.slot["uts_rank"] >= 0).sum()) > 100   # the stages did something
    _assert_graphs_equal(c.to_host(g), exp, "stages")


# ---- the pipeline ----
def test_gpu_pipeline_resident():
    from gtf import pipeline
    from test_pipeline import PREFIX, _check, _fixture
    exp = _fixture()
    g, vivl = pipeline.build_event(PREFIX, 7, 7)
    ia = pipeline.run(g.copy(), vivl, iterations=3, keep_graphs=True)
    ib = pipeline.run(g.copy(), vivl, iterations=3, keep_graphs=True, resident=True)
    assert [i.index for i in ia] == [i.index for i in ib] == [1, 2, 3]
    for i in ib:
        _check(i.index, i.candidates, i.pval_xy, i.pval_zr, i.remaining, i.fragments, exp, 1e-7)
    assert [(len(i.candidates), len(i.remaining), len(i.fragments)) for i in ib] == \
        [(1055, 160, 491), (110, 129, 10), (2, 129, 0)]
    for x, y in zip(ia, ib):
        _assert_graphs_equal(y.remaining_graph, x.remaining_graph, "remaining graph of iteration %d" % x.index)
        _assert_graphs_equal(y.network, x.network, "network of iteration %d" % x.index)
        assert np.array_equal(x.remaining_vivl, y.remaining_vivl)


def test_gpu_pipeline_cli_resident(tmp_path):
    """run_pipeline.py --resident writes the reference run's candidates, fragments and remaining graphs"""
    import os
    import subprocess
    import sys
    from fixtures import GOLDEN
    from gtf import store
    from test_pipeline import _check, _fixture
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cli = os.path.join(root, "gnn-track-finding_amd", "run_pipeline.py")
    out = str(tmp_path / "out")
    subprocess.check_call([sys.executable, cli, "-n", os.path.join(GOLDEN, "kat134"), "-o", out, "-a", "7", "-z", "7",
                           "--resident"])
    exp = _fixture()
    for it in (1, 2, 3):
        d = os.path.join(out, "iteration_%d" % it)
        cands, pv = store.load_groups(os.path.join(d, "candidates", "candidates.npz"))
        frag, _ = store.load_groups(os.path.join(d, "fragments", "fragments.npz"))
        rem_g, _ = store.load_graph(os.path.join(d, "remaining", "graph.npz"))
        graph.check_layout(rem_g)
        sub, nid = rem_g.node["sub_id"], rem_g.node["node_id"]
        rem = [nid[sub == s] for s in range(rem_g.n_subgraphs)]
        _check(it, cands, pv["pval_xy"], pv["pval_zr"], rem, frag, exp, 1e-7)
