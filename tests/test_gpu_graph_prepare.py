"""gtf_graph_prepare on the GPU: the schedules and slot tables it builds are, array for array,
the ones gtf.device's NumPy builders upload (DeviceGraph(tables="host")), the kernels see the
same graph through either, and the optional-field rules of include/gtf.h hold.

The boundary graph is hand-built because the synthetic workloads top out at 41 (c2) and 48 (c4)
slots per receiver: it has receivers at both ends of every schedule class and lane group, beyond
64 slots (one wavefront per node, several steps), partial last wavefronts in every bucket, and
equal / signed-zero / NaN values inside single segments. Counts of 6- and 12-slot receivers:
11 of 6 slots is a wavefront of the node kernel's 6-lane groups (10) plus one and, with the 5-,
7- and 8-slot ones, two and a half wavefronts of prepare's own 8-lane groups; 4 of 12 slots is
one group short of a wavefront of 12-lane groups (5), and the 9..16-slot bucket (13 receivers)
ends one 16-lane group after its third full wavefront."""
import ctypes

import numpy as np
import pytest

from gtf import _native as nat
from gtf import graph, synth
from gtf.params import Params

pytestmark = pytest.mark.gpu

TABLES = ("slot_dst", "out_dst", "slot_layer", "slot_outpos", "slot_outidx", "slot_class", "slot_sflags",
          "slot_xclass", "slot_sxzr", "slot_static", "sched", "sched_seg", "out_sched", "out_lanes")
COUNTS = ("n_g2", "n_g4", "n_g6", "n_g8", "n_g12", "n_g16", "n_g32", "n_g64", "n_big", "n_o4", "n_o8", "n_o16")
DEGREES = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13, 16, 17, 32, 33, 63, 64, 65, 100)
RESERVED = (1, 4, 5, 8, 9)   # senders with exactly this many out-edges
POOL = 112                   # the other senders


def boundary_graph(seed=5):
    rng = np.random.default_rng(seed)
    degs = [d for d in DEGREES for _ in range(3)] + [6] * 8 + [12]
    R = len(degs)
    N = R + len(RESERVED) + POOL
    # receivers 0..R-1, reserved senders R.., the pool after them; then shuffled
    senders = [[] for _ in range(R)]
    roomy = [v for v in range(R) if degs[v] >= 13]
    for i, k in enumerate(RESERVED):
        for v in rng.choice(roomy, k, replace=False):
            senders[v].append(R + i)
    pool = np.arange(R + len(RESERVED), N)
    src, dst = [], []
    for v in range(R):
        s = senders[v] + list(rng.choice(pool, degs[v] - len(senders[v]), replace=False))
        assert len(s) == degs[v]
        src += s
        dst += [v] * len(s)
    perm = rng.permutation(N)
    src, dst = perm[np.array(src, np.int64)], perm[np.array(dst, np.int64)]
    r = np.empty(N)
    r[perm[:R]] = rng.uniform(100, 200, R)        # receivers inside, senders outside
    r[perm[R:]] = rng.uniform(300, 900, N - R)
    phi = rng.uniform(-np.pi, np.pi, N)
    with np.errstate(divide="ignore"):   # (the pure senders have no slot: their send_mw is 1 / 0, unused here)
        g = synth._assemble(N, src, dst, r * np.cos(phi), r * np.sin(phi), rng.uniform(-500, 500, N), r,
                            rng.integers(1, 9, N), Params())
    # few distinct layers and x values, so every larger segment repeats them; signed zeros in both;
    # NaN layers on real senders
    idx = np.arange(N)
    layer = (idx % 4).astype(np.float64)
    layer[idx % 8 == 4] = -0.0
    layer[idx % 8 == 0] = 0.0
    layer[idx % 23 == 5] = np.nan
    x = (idx % 7 - 2) * 1.5
    x[idx % 14 == 2] = 0.0
    x[idx % 14 == 9] = -0.0
    g.node["layer"] = layer
    g.node["gnn"][:, 0] = x
    return g


def _segments(g):
    sp = g.slot_ptr.astype(np.int64)
    src = g.slot["slot_src"].astype(np.int64)
    for v in range(g.n_nodes):
        if sp[v + 1] - sp[v] >= 2:
            yield sp[v + 1] - sp[v], src[sp[v]:sp[v + 1]]


@pytest.fixture(scope="module")
def boundary():
    return boundary_graph()


def test_boundary_graph_is_what_it_says(boundary):
    g = boundary
    deg = np.diff(g.slot_ptr.astype(np.int64))
    for d in DEGREES:
        assert int((deg == d).sum()) >= 3, d
    assert int((deg == 6).sum()) == 11 and int((deg == 12).sum()) == 4
    od = np.diff(g.out_ptr.astype(np.int64))
    for k in (0,) + RESERVED:
        assert int((od == k).sum()) >= 1, k
    assert int((od > 16).sum()) >= 1
    seen = dict(layer=0, x=0, zero=0, nan=0)
    for d, s in _segments(g):
        lay, x = g.node["layer"][s], g.node["gnn"][s, 0]
        seen["layer"] += np.unique(lay[~np.isnan(lay)]).size < (~np.isnan(lay)).sum()
        seen["x"] += np.unique(x).size < x.size
        z = x[x == 0.0]
        seen["zero"] += d <= 32 and z.size >= 2 and np.signbit(z).any() and not np.signbit(z).all()
        seen["nan"] += d <= 64 and np.isnan(lay).sum() >= 2
    assert all(n >= 3 for n in seen.values()), seen


def _compare(g, **kw):
    """every table and count of DeviceGraph(tables="device") against the host builders' upload"""
    from gtf.device import DeviceGraph
    host = DeviceGraph(g, classes=True, **kw)
    dev = DeviceGraph(g, tables="device", **kw)
    assert dev.use_classes and dev.use_sxzr and dev.use_static32
    for name in TABLES:
        a = host._np(host.t[name])
        b = dev._np(dev.t[name])
        assert b.size >= a.size and a.dtype == b.dtype, name
        assert np.array_equal(a, b[:a.size], equal_nan=a.dtype.kind == "f"), name
    for f in COUNTS:
        assert getattr(host.cg, f) == getattr(dev.cg, f), f
        assert getattr(host.cg_sched, f) == getattr(dev.cg_sched, f), f
    for f in TABLES:   # every table reaches the kernels' struct
        assert bool(getattr(host.cg, f)) and bool(getattr(dev.cg, f)), f
    return host, dev


def test_boundary_graph_tables(boundary):
    host, dev = _compare(boundary)
    assert host.cg.n_big >= 6 and host.cg.n_g64 >= 9 and host.cg.n_g6 == 14 and host.cg.n_g12 == 7


@pytest.mark.parametrize("layout", ["schedule", "tiled"])
def test_boundary_graph_tables_renumbered(boundary, layout):
    _compare(boundary, layout=layout, tile=64)


def test_orphan_graph_tables():
    g = synth.workload("tiny200", seed=1)
    keep = np.ones(g.n_nodes, bool)
    keep[::3] = False
    h = graph.subset(g, keep)
    assert h.n_slots == 1837 and int((h.slot["slot_src"] < 0).sum()) == 643
    _compare(h)


def test_c2_tables():
    g = synth.workload("c2", seed=3)
    deg = np.diff(g.slot_ptr.astype(np.int64))
    assert int(((deg >= 33) & (deg <= 64)).sum()) == 17 and int((deg == 0).sum()) == 1482
    _compare(g)


# ---- bounds and optional fields, through ctypes ----
SIZES = dict(slot_dst=lambda N, S, E: 4 * S, out_dst=lambda N, S, E: 4 * E, slot_layer=lambda N, S, E: 8 * S,
             slot_outpos=lambda N, S, E: 4 * S, slot_outidx=lambda N, S, E: 4 * S, slot_class=lambda N, S, E: 8 * S,
             slot_sflags=lambda N, S, E: S, slot_xclass=lambda N, S, E: 8 * S, slot_sxzr=lambda N, S, E: 24 * S,
             slot_static=lambda N, S, E: 4 * S, sched=lambda N, S, E: 4 * N, sched_seg=lambda N, S, E: 8 * N,
             out_sched=lambda N, S, E: 16 * N, out_lanes=lambda N, S, E: 64 * N)
OPTIONAL = tuple(n for n in TABLES if n not in ("slot_dst", "slot_outpos"))
GUARD = 64


class Raw:
    """the base arrays of a graph on the device and a gtf_graph of them, nothing else"""

    def __init__(self, g):
        import torch
        from gtf.device import DeviceGraph
        self.torch = torch
        self.d = DeviceGraph(g, schedule=False, classes=False)   # (its uploads are the base arrays)
        self.lib = self.d.lib
        self.N, self.S, self.E = g.n_nodes, g.n_slots, g.n_edges

    def graph(self, **over):
        p = self.d.ptr
        f = dict(n_nodes=self.N, n_slots=self.S, n_edges=self.E, slot_ptr=p("slot_ptr"), slot_src=p("slot_src"),
                 out_ptr=p("out_ptr"), out_slot=p("out_slot"), is_edge=p("is_edge"), rev_edge=p("rev_edge"),
                 gnn=p("gnn"), layer=p("layer"))
        f.update(over)
        return nat.GtfGraph(**f)

    def tables(self, names, sizes=None):
        N, S, E = sizes or (self.N, self.S, self.E)
        buf = {n: self.torch.full((SIZES[n](N, S, E) + GUARD,), 0xA5, dtype=self.torch.uint8, device="cuda")
               for n in names}
        return buf, nat.GtfGraphTables(**{n: ctypes.c_void_p(b.data_ptr()) for n, b in buf.items()})

    def prepare(self, cg, t):
        need = self.lib.gtf_graph_prepare_workspace_bytes(cg.n_nodes, cg.n_slots, cg.n_edges)
        ws = self.torch.empty(need, dtype=self.torch.uint8, device="cuda")
        rc = self.lib.gtf_graph_prepare(ctypes.byref(cg), ctypes.byref(t), ctypes.c_void_p(ws.data_ptr()),
                                        ctypes.c_size_t(need), self.d.stream)
        self.torch.cuda.synchronize()
        return rc


@pytest.fixture(scope="module")
def raw(boundary):
    return Raw(boundary)


def _guards_intact(buf):
    for n, b in buf.items():
        assert bool((b[-GUARD:] == 0xA5).all()), n


def test_guard_bytes_and_contents(raw, boundary):
    from gtf.device import DeviceGraph
    buf, t = raw.tables(TABLES)
    cg = raw.graph()
    assert raw.prepare(cg, t) == 0
    _guards_intact(buf)
    host = DeviceGraph(boundary, classes=True)
    for n in TABLES:
        a = host._np(host.t[n])
        b = buf[n][:-GUARD].cpu().numpy().view(a.dtype)
        assert np.array_equal(a, b[:a.size], equal_nan=a.dtype.kind == "f"), n
        assert getattr(cg, n) == buf[n].data_ptr(), n
        # past the written part of the two capacity tables nothing was touched
        assert bool((buf[n][a.nbytes:] == 0xA5).all()), n
    for f in COUNTS:
        assert getattr(cg, f) == getattr(host.cg, f), f


def test_schedule_only(raw):
    buf, t = raw.tables(("sched", "sched_seg"))
    stale = ctypes.c_void_p(256)
    cg = raw.graph(n_o4=5, n_o8=6, n_o16=7, **{n: stale for n in OPTIONAL})
    assert raw.prepare(cg, t) == 0
    _guards_intact(buf)
    for n in OPTIONAL:
        assert bool(getattr(cg, n)) == (n in ("sched", "sched_seg")), n
    assert (cg.n_o4, cg.n_o8, cg.n_o16) == (0, 0, 0)
    assert cg.n_g4 + cg.n_g8 + cg.n_g16 + cg.n_g32 + cg.n_g64 + cg.n_big == raw.N
    assert cg.n_g2 > 0 and cg.n_g6 > 0 and cg.n_g12 > 0 and cg.n_big > 0


def test_partial_class_set_is_dropped(raw):
    buf, t = raw.tables(("slot_class", "slot_sflags", "slot_static", "out_lanes", "sched_seg"))
    cg = raw.graph()
    assert raw.prepare(cg, t) == 0
    for n in ("slot_class", "slot_sflags", "slot_xclass", "slot_static"):
        assert not getattr(cg, n), n
    assert not cg.out_lanes and not cg.out_sched      # out_lanes needs out_sched
    assert not cg.sched_seg and not cg.sched and cg.n_g4 == 0 and cg.n_big == 0   # sched_seg needs sched
    for b in buf.values():   # and none of them was written
        assert bool((b == 0xA5).all())


def test_empty_graphs(raw):
    stale = ctypes.c_void_p(256)
    junk = {f: 3 for f in COUNTS}
    buf, t = raw.tables(TABLES, sizes=(0, 0, 0))
    cg = nat.GtfGraph(n_nodes=0, **junk, **{n: stale for n in OPTIONAL})
    assert raw.prepare(cg, t) == 0
    assert all(getattr(cg, f) == 0 for f in COUNTS) and not any(getattr(cg, n) for n in OPTIONAL)
    # nodes only
    buf2, t2 = raw.tables(TABLES, sizes=(raw.N, 0, 0))
    zeros = raw.torch.zeros(raw.N + 1, dtype=raw.torch.int32, device="cuda")
    z = ctypes.c_void_p(zeros.data_ptr())
    cg = nat.GtfGraph(n_nodes=raw.N, slot_ptr=z, out_ptr=z, **junk, **{n: stale for n in OPTIONAL})
    assert raw.prepare(cg, t2) == 0
    assert all(getattr(cg, f) == 0 for f in COUNTS) and not any(getattr(cg, n) for n in OPTIONAL)
    for b in list(buf.values()) + list(buf2.values()):
        assert bool((b == 0xA5).all())


# ---- the kernels see the same graph ----
def _bit_equal(a, b, what):
    for kind in ("node", "slot"):
        da, db = getattr(a, kind), getattr(b, kind)
        for k in da:
            x, y = da[k], db[k]
            assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), (what, kind, k)


def _run(g, fn, **kw):
    from gtf.device import DeviceGraph
    d = DeviceGraph(g, **kw)
    d.clear_errors()
    fn(d)
    flags = d.errors()
    return d.download(g.copy()), flags


@pytest.fixture(scope="module")
def event():
    return synth.event(seed=7, n_tracks=1000, fake_mean=synth.C4_FAKE), Params()


@pytest.mark.parametrize("kw", [dict(layout="natural"), dict(layout="tiled", tile=256)], ids=["natural", "tiled"])
def test_two_passes_bit_equal(event, kw):
    g, p = event

    def two(d):
        d.full_pass(p)
        d.full_pass(p)

    a, fa = _run(g, two, classes=True, **kw)
    b, fb = _run(g, two, tables="device", **kw)
    assert fa == fb
    _bit_equal(a, b, kw["layout"])


def test_extrapolate_bit_equal_on_plain_allocations(event):
    g, p = event
    a, fa = _run(g, lambda d: d.extrapolate(p), classes=True, mem="hip")
    b, fb = _run(g, lambda d: d.extrapolate(p), tables="device", mem="hip")
    assert fa == fb
    _bit_equal(a, b, "mem=hip")


def test_degenerate_graphs_take_the_host_tables(event):
    """no slots and no edges: prepare has nothing to build (zero counts by contract), so the
    device mode's structs are the host mode's"""
    from gtf.device import DeviceGraph
    g, _ = event
    h = graph.subset(g, (np.diff(g.slot_ptr) == 0) & (np.diff(g.out_ptr) == 0))
    assert h.n_nodes > 0 and h.n_slots == 0 and h.n_edges == 0
    a, b = DeviceGraph(h), DeviceGraph(h, tables="device")
    for f in COUNTS:
        assert getattr(a.cg, f) == getattr(b.cg, f), f


def test_unsupported_combinations_raise(event):
    from gtf.device import DeviceGraph
    g, _ = event
    with pytest.raises(ValueError, match="padded"):
        DeviceGraph(g, tables="device", layout="padded")
    with pytest.raises(ValueError, match="pack"):
        DeviceGraph(g, tables="device", pack=True)
    with pytest.raises(ValueError, match="tables"):
        DeviceGraph(g, tables="gpu")


# ---- the pipeline ----
def test_pipeline_with_device_tables():
    from gtf import pipeline
    from test_pipeline import PREFIX

    def sets(groups):
        return sorted(sorted(int(x) for x in c) for c in groups)

    ga, va = pipeline.build_event(PREFIX, 7, 7)
    gb, vb = pipeline.build_event(PREFIX, 7, 7, tables="device")
    assert np.array_equal(va, vb)
    _bit_equal(ga, gb, "build_event")
    ia = pipeline.run(ga, va, iterations=3)
    ib = pipeline.run(gb, vb, iterations=3, tables="device")
    assert [i.index for i in ia] == [i.index for i in ib] == [1, 2, 3]
    for x, y in zip(ia, ib):
        assert [list(c) for c in x.candidates] == [list(c) for c in y.candidates], x.index
        assert np.array_equal(x.pval_xy, y.pval_xy) and np.array_equal(x.pval_zr, y.pval_zr), x.index
        assert sets(x.remaining) == sets(y.remaining) and sets(x.fragments) == sets(y.fragments), x.index
