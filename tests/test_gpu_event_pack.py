"""Event conversion into a resident DeviceGraph (gtf_event_pack, gtf_fill_columns,
DeviceGraph.from_event / host_graph, pipeline.build_event_dev, run on a DeviceGraph, run_pipeline.py
--resident-event) against the host path it replaces: io.build_event_csr, pipeline.build_event and
pipeline.run on host graphs. Everything is compared bit for bit (NaN meeting NaN): the new path moves
and initialises values, it computes none of its own."""
import ctypes
import functools
import os

import numpy as np
import pytest

from fixtures import GOLDEN
from gtf import _native as nat
from gtf import io
from gtf.graph import NODE_FIELDS, SLOT_FIELDS, TrackGraph, check_layout, empty_arrays
from test_build import _write_event
from test_gpu_graph_subset import _assert_tables_equal

pytestmark = pytest.mark.gpu

PREFIX = os.path.join(GOLDEN, "kat134", "event_1_filtered_graph_")
SYNTHETIC = {0: (400, 300, 10 ** 6, 0.0), 1: (3000, 4000, 5000, 0.0), 2: (2000, 1500, 10 ** 6, 0.7),
             3: (5000, 9000, 2 ** 40, 0.3)}   # test_build.py's four events (seed: n, rows, id space, chain)


def _same(a, b):
    """dtype, shape and bits (NaN meeting NaN)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind == "f":
        return bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))
    return bool(np.array_equal(a, b))


def _graphs_equal(got, exp, what):
    assert (got.n_nodes, got.n_slots, got.n_edges, got.n_subgraphs) == \
        (exp.n_nodes, exp.n_slots, exp.n_edges, exp.n_subgraphs), what
    for k in ("slot_ptr", "out_ptr", "out_slot"):
        assert _same(getattr(got, k), getattr(exp, k)), (what, k)
    for k in NODE_FIELDS:
        assert _same(got.node[k], exp.node[k]), (what, k)
    for k in SLOT_FIELDS:
        assert _same(got.slot[k], exp.slot[k]), (what, k)


def _host_event(ids, x, y, z, r, layer, a, b):
    """io.build_event_csr from columns instead of files (the host builder, NumPy assembly)"""
    N = int(ids.size)
    o, E, n_sub = io.csr_from_rows(ids, a, b)
    order = o["order"][:N].astype(np.int64)
    node, slot = empty_arrays(NODE_FIELDS, N), empty_arrays(SLOT_FIELDS, E)
    node["gnn"] = np.stack([x, y, z, r], axis=1)[order]
    node["xyzr"] = node["gnn"].copy()
    node["layer"] = (layer[order] % 100).astype(np.float64)
    node["has_tse"][:] = 1
    node["tag"] = ids[order]
    node["node_id"] = ids[order]
    node["sub_id"] = o["sub_id"][:N].copy()
    slot["slot_src"] = o["slot_src"][:E].copy()
    slot["slot_key"] = ids[order][slot["slot_src"]] if E else np.zeros(0, np.int64)
    for k in ("is_edge", "rev_edge", "act"):
        slot[k][:] = 1
    slot["tse_rank"] = o["tse_rank"][:E].copy()
    g = TrackGraph(N, E, o["slot_ptr"].copy(), o["out_ptr"].copy(), o["out_slot"][:E].copy(), node, slot, n_sub)
    check_layout(g)
    lay = layer[order]
    return g, np.stack([lay // 1000, lay % 100], 1).astype(np.float64).reshape(N, 2)


def _columns(prefix, lo, hi):
    ids, x, y, z, r, layer = io.read_nodes(prefix + "nodes.csv", lo, hi)
    n2, n1 = io.read_edges(prefix + "edges.csv")
    return ids, x, y, z, r, layer, n1, n2


def _check_event(cols, g, vivl, mem):
    """from_event(cols) against the host event (g, vivl): the downloaded graph, vivl, solo, the tables"""
    from gtf.device import DeviceGraph
    d = DeviceGraph.from_event(*cols, mem=mem)
    assert d.layout == "natural" and d.tables == "device" and d.mem == mem
    assert (d.n_nodes, d.n_slots, d.n_edges, d.n_sub) == (g.n_nodes, g.n_slots, g.n_edges, g.n_subgraphs)
    h, v = d.host_graph()
    _graphs_equal(h, g, "from_event")
    assert _same(v, vivl)
    assert _same(d._np(d.node_id_dev()), g.node["node_id"])
    sub = g.node["sub_id"].astype(np.int64)
    solo = (np.bincount(sub - sub.min())[sub - sub.min()] == 1).astype(np.uint8) if g.n_nodes else np.zeros(0, np.uint8)
    assert _same(d._np(d.t["solo"]), solo)
    _assert_tables_equal(d, g, mem=mem)
    return d


# ---------------------------------------------------------------- 1. pack against the host
@pytest.fixture(scope="module")
def csv_events(tmp_path_factory):
    out = {"kat134": (PREFIX, 7, 7)}
    for seed, (n, rows, space, chain) in SYNTHETIC.items():
        d = tmp_path_factory.mktemp("ev%d" % seed)
        out["seed%d" % seed] = (_write_event(str(d), seed, n, rows, space, chain), 7, 8)
    d = tmp_path_factory.mktemp("empty")
    out["empty"] = (_write_event(str(d), 4, 50, 40, 1000, 0.0), 20, 21)   # test_native_build_empty's window
    return out


@pytest.mark.parametrize("name,mem", [("seed0", "torch"), ("seed1", "torch"), ("seed2", "torch"), ("seed3", "torch"),
                                      ("kat134", "torch"), ("seed0", "hip"), ("seed3", "hip"), ("kat134", "hip")])
def test_from_event_equals_host_event(csv_events, name, mem):
    prefix, lo, hi = csv_events[name]
    g, vivl = io.build_event_csr(prefix, lo, hi)
    cols = _columns(prefix, lo, hi)
    g2, vivl2 = _host_event(*cols)            # (the helper the hand-made events below rely on)
    _graphs_equal(g2, g, "helper")
    assert _same(vivl2, vivl)
    assert g.n_nodes > 200 and g.n_edges > 0
    _check_event(cols, g, vivl, mem)


# ---------------------------------------------------------------- 2. edges of the kernels
def _handmade(name):
    rng = np.random.default_rng(11)
    if name == "one":          # one isolated node
        ids, rows = np.array([5], np.int64), np.zeros((0, 2), np.int64)
    elif name == "two":        # two nodes and one row
        ids, rows = np.array([9, 4], np.int64), np.array([[4, 9]], np.int64)
    elif name == "chain65":    # one wavefront plus one
        ids = np.arange(100, 165, dtype=np.int64)
        rows = np.stack([ids[:-1], ids[1:]], 1)
    else:                      # "perm257": small components of far-apart ids, so set orders permute the nodes
        ids = rng.choice(2 ** 40, 257, replace=False).astype(np.int64)
        cut = np.sort(rng.choice(np.arange(1, 257), 40, replace=False))
        rows = np.array([(ids[i], ids[i + 1]) for i in range(256) if i + 1 not in cut], np.int64)
        rows = rows[rng.permutation(rows.shape[0])]
    N = ids.size
    x, y, z = (rng.normal(0, 300, N).round(4) for _ in range(3))
    layer = (rng.integers(7, 10, N) * 1000 + rng.integers(2, 14, N)).astype(np.int64)
    return ids, x, y, z, io.edge_length_xy(x, y), layer, rows[:, 0].copy(), rows[:, 1].copy()


@pytest.mark.parametrize("name,mem", [(n, m) for n in ("one", "two", "chain65", "perm257") for m in ("torch", "hip")])
def test_from_event_handmade(name, mem):
    cols = _handmade(name)
    g, vivl = _host_event(*cols)
    assert g.n_nodes == {"one": 1, "two": 2, "chain65": 65, "perm257": 257}[name]
    assert g.n_edges == {"one": 0, "two": 2, "chain65": 128}.get(name, g.n_edges)
    if name == "perm257":
        assert not np.array_equal(g.node["node_id"], cols[0]) and g.n_subgraphs > 10
    d = _check_event(cols, g, vivl, mem)
    if name == "one":
        assert d._np(d.t["solo"]).tolist() == [1]


@pytest.mark.parametrize("mem", ["torch", "hip"])
def test_from_event_empty_window(csv_events, mem):
    prefix, lo, hi = csv_events["empty"]
    g, vivl = io.build_event_csr(prefix, lo, hi)
    cols = _columns(prefix, lo, hi)
    assert g.n_nodes == 0 and cols[0].size == 0 and cols[6].size > 0     # rows, but no node
    d = _check_event(cols, g, vivl, mem)
    assert d.n_nodes == 0 and d.host_graph()[1].shape == (0, 2)


def test_from_event_refuses_bad_columns():
    from gtf.device import DeviceGraph
    ids, x, y, z, r, layer, a, b = _handmade("two")
    with pytest.raises(ValueError, match="negative layer_id"):
        DeviceGraph.from_event(ids, x, y, z, r, np.array([7002, -1]), a, b)
    with pytest.raises(ValueError, match="per node"):
        DeviceGraph.from_event(ids, x[:1], y, z, r, layer, a, b)
    with pytest.raises(ValueError, match="mem"):
        DeviceGraph.from_event(ids, x, y, z, r, layer, a, b, mem="cpu")


def test_host_graph_needs_the_node_id_column():
    from gtf.device import DeviceGraph
    cols = _handmade("chain65")
    g, _ = _host_event(*cols)
    with pytest.raises(ValueError, match="node_id"):
        DeviceGraph(g).host_graph()
    d = DeviceGraph.from_event(*cols)
    with pytest.raises(ValueError, match="subset"):        # to_host(parent) keeps its refusals
        d.to_host(g)
    # a subset() child of the resident loop holds node_id and vivl too, and with every node kept no
    # orphan slot either: still no from_event graph
    child = d.subset(np.ones(d.n_nodes, bool), carry={"vivl": d.carried["vivl"]})
    assert "node_id" in child.t and "vivl" in child.carried and child.n_slots == d.n_slots
    with pytest.raises(ValueError, match="from_event"):
        child.host_graph()
    assert _same(child.to_host(g).node["node_id"], g.node["node_id"])


GUARD = 64
NAN, M1 = 0x7ff8000000000000, 0xffffffffffffffff
ROWS = (0, 1, 63, 64, 65, 1000)
PATTERNS = {1: (0xff, 0, 1, 0xff, 0, 1), 4: (0xffffffff, 0, 1, M1, 0xffffffff, 1),
            8: (NAN, NAN, 0, NAN, 0x0102030405060708, NAN), 24: (NAN,) * 6, 40: (NAN, NAN, NAN, 0, NAN, NAN)}


def test_fill_columns_guards_and_patterns():
    """every row size x every row count in ONE call of 32 columns: 1-, 4- and 8-byte words, buffers with
    guard bytes on both sides, payload preset to a value no pattern holds"""
    import torch
    L = nat.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    spec = [(rb, rows, PATTERNS[rb][i]) for rb in (1, 4, 8, 24, 40) for i, rows in enumerate(ROWS)]
    spec += [(32, 65, NAN), (1, 257, 1)]
    assert len(spec) == nat.FILL_MAX_COLUMNS
    bufs, cols = [], []
    for rb, rows, pat in spec:
        t = torch.full((GUARD + rows * rb + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        t[GUARD:GUARD + rows * rb] = 0x5A
        bufs.append(t)
        cols.append(nat.GtfFillColumn(ctypes.c_void_p(t.data_ptr() + GUARD if rows else 0), rows, rb, 0, pat))
    nat.check(L.gtf_fill_columns((nat.GtfFillColumn * len(cols))(*cols), len(cols), stream))
    for (rb, rows, pat), t in zip(spec, bufs):
        h = t.cpu().numpy()
        assert bool((h[:GUARD] == 0xA5).all()) and bool((h[GUARD + rows * rb:] == 0xA5).all()), (rb, rows)
        wb = rb if rb in (1, 4) else 8
        word = np.array([pat], np.uint64).view(np.uint8)[:wb]       # (little endian: the low bytes)
        assert np.array_equal(h[GUARD:GUARD + rows * rb], np.tile(word, rows * rb // wb)), (rb, rows)
    # the values event conversion asks for, read back as their types
    payload = lambda i: bufs[i].cpu().numpy()[GUARD:-GUARD]  # noqa: E731
    assert spec[21] == (24, 64, NAN) and np.isnan(payload(21).view(np.float64)).all()
    assert spec[10] == (4, 65, 0xffffffff) and (payload(10).view(np.int32) == -1).all()
    assert spec[3] == (1, 64, 0xff) and (payload(3).view(np.int8) == -1).all()
    assert spec[5] == (1, 1000, 1) and (payload(5) == 1).all()
    # 33 columns are refused, and nothing is written
    t = torch.full((GUARD + 8 + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    c33 = [nat.GtfFillColumn(ctypes.c_void_p(t.data_ptr() + GUARD), 1, 8, 0, 0)] * 33
    assert L.gtf_fill_columns((nat.GtfFillColumn * 33)(*c33), 33, stream) == -2 and b"n_cols" in L.gtf_last_error()
    assert bool((t.cpu().numpy() == 0xA5).all())


def test_event_pack_skips_null_outputs():
    """gtf_event_pack through ctypes: NULL outputs are skipped, the wanted ones are written and
    nothing beyond them"""
    import torch
    L = nat.lib()
    ids, x, y, z, r, layer, a, b = _handmade("perm257")
    g, vivl = _host_event(ids, x, y, z, r, layer, a, b)
    N = ids.size
    o, _, n_sub = io.csr_from_rows(ids, a, b)
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()  # noqa: E731
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    t_ids, t_order, t_sub, t_x, t_y, t_z, t_r, t_l = (up(v) for v in (ids, o["order"][:N], o["sub_id"][:N], x, y, z,
                                                                      r, layer))
    ev = nat.GtfEventCsr(N, a.size, vp(t_ids), None, None, vp(t_order), vp(t_sub), None, None, None, None, None,
                         g.n_edges, n_sub, 0)
    cols = nat.GtfEventCols(vp(t_x), vp(t_y), vp(t_z), vp(t_r), vp(t_l))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def guarded(nbytes):
        return torch.full((GUARD + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")

    exp = {"gnn": g.node["gnn"], "xyzr": g.node["xyzr"], "layer": g.node["layer"], "node_id": g.node["node_id"],
           "vivl": vivl}
    # solo reads sub_id alone: wanted by itself it needs neither order, node_id nor the input columns
    ev_sub = nat.GtfEventCsr(N, a.size, None, None, None, None, vp(t_sub), None, None, None, None, None,
                             g.n_edges, n_sub, 0)
    for wanted, ev_w, cols_w in ((("gnn",), ev, cols), (("xyzr", "vivl"), ev, cols), (("solo",), ev, cols),
                                 (("solo",), ev_sub, None), (("layer", "node_id", "solo"), ev, cols),
                                 (tuple(exp) + ("solo",), ev, cols)):
        sub = g.node["sub_id"].astype(np.int64)
        e = dict(exp, solo=(np.bincount(sub)[sub] == 1).astype(np.uint8))
        bufs = {k: guarded(e[k].nbytes) for k in wanted}
        out = nat.GtfEventOut(*[ctypes.c_void_p(bufs[k].data_ptr() + GUARD) if k in bufs else None
                                for k in ("gnn", "xyzr", "layer", "node_id", "vivl", "solo")])
        nat.check(L.gtf_event_pack(ctypes.byref(ev_w), ctypes.byref(cols_w) if cols_w is not None else None,
                                   ctypes.byref(out), stream))
        for k, t in bufs.items():
            h = t.cpu().numpy()
            assert bool((h[:GUARD] == 0xA5).all()) and bool((h[GUARD + e[k].nbytes:] == 0xA5).all()), k
            assert _same(h[GUARD:GUARD + e[k].nbytes].view(e[k].dtype).reshape(e[k].shape), e[k]), (wanted, k)


# ---------------------------------------------------------------- 3. states
@functools.lru_cache(maxsize=None)
def _host_built():
    from gtf import pipeline
    return pipeline.build_event(PREFIX, 7, 7)


@pytest.mark.parametrize("mem", ["torch", "hip"])
def test_build_event_dev_equals_build_event(mem):
    from gtf import pipeline
    g, vivl = _host_built()
    d = pipeline.build_event_dev(PREFIX, 7, 7, mem=mem)
    h, v = d.host_graph()
    _graphs_equal(h, g, "build_event_dev")
    assert _same(v, vivl)
    assert np.isfinite(h.slot["tse_mw"]).any() and np.isfinite(h.slot["send_mw"]).any() and (h.node["degree"] >= 0).all()


# ---------------------------------------------------------------- 4. the loop
@functools.lru_cache(maxsize=None)
def _host_loop():
    from gtf import pipeline
    g, vivl = _host_built()
    return pipeline.run(g.copy(), vivl, iterations=3, keep_graphs=True)


@pytest.mark.parametrize("keep", [True, False])
def test_run_on_a_resident_event(keep):
    from gtf import pipeline
    ia = _host_loop()
    ib = pipeline.run(pipeline.build_event_dev(PREFIX, 7, 7), None, iterations=3, keep_graphs=keep, resident="device")
    assert [i.index for i in ia] == [i.index for i in ib] == [1, 2, 3]
    assert [len(i.candidates) for i in ib] == [1055, 110, 2]
    for x, y in zip(ia, ib):
        assert y.stage == x.stage and set(y.seconds) == set(x.seconds)
        for k in ("candidates", "remaining", "fragments"):
            a, b = getattr(x, k), getattr(y, k)
            assert len(a) == len(b) and all(_same(np.asarray(p, np.int64), q) for p, q in zip(a, b)), (x.index, k)
        assert _same(np.asarray(y.pval_xy, np.float64), np.asarray(x.pval_xy, np.float64))
        assert _same(np.asarray(y.pval_zr, np.float64), np.asarray(x.pval_zr, np.float64))
        if keep:
            _graphs_equal(y.network, x.network, "network of iteration %d" % x.index)
            _graphs_equal(y.remaining_graph, x.remaining_graph, "remaining graph of iteration %d" % x.index)
            assert _same(y.remaining_vivl, x.remaining_vivl)
        else:
            assert y.network is None and y.remaining_graph is None and y.remaining_vivl is None


def test_run_refuses_a_device_graph_outside_the_device_mode():
    from gtf import pipeline
    d = pipeline.build_event_dev(PREFIX, 7, 7)
    for resident in (False, True):
        with pytest.raises(ValueError, match="resident='device'"):
            pipeline.run(d, None, iterations=1, resident=resident)
    with pytest.raises(ValueError, match="vivl"):
        pipeline.run(d, _host_built()[1], iterations=1, resident="device")
    g, vivl = _host_built()
    with pytest.raises(ValueError, match="host"):          # a caller's download goes with a DeviceGraph input only
        pipeline.run(g, vivl, iterations=1, resident="device", host=g)


# ---------------------------------------------------------------- 5. the CLI
def test_gpu_pipeline_cli_resident_event(tmp_path):
    """run_pipeline.py --resident-event writes the files --resident-outputs writes"""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cli = os.path.join(root, "gnn-track-finding_amd", "run_pipeline.py")
    outs = []
    for flag in ("--resident-outputs", "--resident-event"):
        out = str(tmp_path / flag.strip("-"))
        subprocess.check_call([sys.executable, cli, "-n", os.path.join(GOLDEN, "kat134"), "-o", out, "-a", "7", "-z", "7",
                               flag])
        outs.append(out)
    files = sorted(os.path.relpath(os.path.join(r, f), outs[0]) for r, _, fs in os.walk(outs[0]) for f in fs)
    assert files == sorted(os.path.relpath(os.path.join(r, f), outs[1]) for r, _, fs in os.walk(outs[1]) for f in fs)
    assert sum(f.endswith(".npz") for f in files) >= 1 + 3 * 4
    for f in files:
        a, b = os.path.join(outs[0], f), os.path.join(outs[1], f)
        if f.endswith(".npz"):
            with np.load(a) as za, np.load(b) as zb:
                assert sorted(za.files) == sorted(zb.files), f
                for k in za.files:
                    assert za[k].dtype == zb[k].dtype and np.array_equal(za[k], zb[k], equal_nan=za[k].dtype.kind == "f"), \
                        (f, k)
        elif f.endswith(".csv"):
            assert open(a).read() == open(b).read(), f
        else:
            assert f == "timings.json", f
            import json
            assert sorted(json.load(open(a))) == sorted(json.load(open(b)))
    rc = subprocess.run([sys.executable, cli, "-o", str(tmp_path / "x"), "--start", "2", "--resident-event"],
                        capture_output=True, text=True)
    assert rc.returncode == 2 and "--start 1" in rc.stderr
