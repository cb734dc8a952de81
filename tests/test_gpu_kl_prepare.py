"""gtf_kl_prepare, gtf_kl_coords and gtf_kl_pair_rows on the GPU against the host constructor
(gtf.parabolic.ParabolicKL, tile = 0), over tests/kl_prepare_cases.py: every array, count and the
scale through the C-ABI between guard bytes; run() of the device-prepared object bit for bit; the pair
rows; the Python entry points."""
import ctypes

import numpy as np
import pytest

import kl_prepare_cases as kc
from guard_mem import FILL, GUARD, Mem, at

pytestmark = pytest.mark.gpu

def _np(t):
    return t.cpu().numpy() if t is not None else None


# ---------------------------------------------------------------- 1. the C-ABI between guard bytes
def _abi(c, mode):
    """gtf_kl_prepare on the case in guarded buffers: (rc, message, payloads, graph, q32, counts, buffers)"""
    from gtf import _native as nat
    L = nat.lib()
    mem = Mem("torch")
    ordered, with_single, compact = mode
    N, S = c["ptr"].size - 1, c["src"].size
    up = lambda a: mem.up(a) if a is not None and a.size else None  # noqa: E731
    d_ptr, d_src, d_gnn = mem.up(c["ptr"]), up(c["src"]), up(c["gnn"])
    d_truth, d_ise = (mem.up(c["truth"]) if c["truth"] is not None else None), up(c["is_edge"])
    if d_truth is not None and N == 0:
        d_truth = mem.up(np.zeros(1, np.int64))
    sizes = {"slot_ptr": 4 * (N + 1), "slot_src": 4 * S, "xy": 16 * N, "truth": 8 * N, "pair_ptr": 8 * (N + 1),
             "list": 4 * N, "node_of": 8 * N, "slot_of": 8 * S, "q": 8 * N, "truth32": 4 * N}
    nb = int(L.gtf_kl_prepare_workspace_bytes(N, S))
    g = {k: mem.guarded(v) for k, v in sizes.items()}
    ws = mem.guarded(nb)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    pin = nat.GtfKlPrepareIn(n_nodes=N, n_slots=S, slot_ptr=p(d_ptr), slot_src=p(d_src), is_edge=p(d_ise), gnn=p(d_gnn),
                             truth=p(d_truth), gnn_stride=4, with_single=int(with_single), layout=int(ordered),
                             compact=int(compact), scale=c["scale"] or 0.0)
    buf = nat.GtfKlPrepareBuf(**{k: at(v) for k, v in g.items()})
    kg, q, cnt = nat.GtfKlGraph(), nat.GtfKlQ32(), nat.GtfKlCounts()
    rc = L.gtf_kl_prepare(ctypes.byref(pin), ctypes.byref(buf), ctypes.byref(kg), ctypes.byref(q), ctypes.byref(cnt),
                          at(ws), nb, mem.stream)
    msg = L.gtf_last_error().decode() if rc else ""
    import torch
    torch.cuda.synchronize()
    dt = {"slot_ptr": np.int32, "slot_src": np.int32, "xy": np.float64, "truth": np.int64, "pair_ptr": np.int64,
          "list": np.int32, "node_of": np.int64, "slot_of": np.int64, "q": np.int32, "truth32": np.int32}
    got = {k: mem.payload(g[k], sizes[k], dt[k]) for k in sizes}   # (asserts the guards)
    mem.payload(ws, nb, np.uint8)
    return rc, msg, got, kg, q, cnt, g


def _untouched(a):
    return bool((a.view(np.uint8) == FILL).all())


@pytest.mark.parametrize("name", kc.NAMES)
def test_abi_equals_the_host_constructor(name):
    c = kc.case(name)
    N = c["ptr"].size - 1
    for mode in c["modes"]:
        ordered, with_single, compact = mode
        rc, msg, got, kg, q, cnt, g = _abi(c, mode)
        if c["error"] is not None:
            assert rc == -2 and c["error"] in msg, (mode, rc, msg)
            assert cnt.error != 0
            continue
        assert rc == 0, (mode, msg)
        k = kc.host(c, mode)
        S = k.n_slots
        what = (name, mode)
        assert cnt.error == 0 and cnt.n_kept == S and cnt.n_pairs == k.n_pairs and cnt.n_listed == k.n_listed, what
        assert np.array_equal(got["slot_ptr"], _np(k.slot_ptr)), what
        assert np.array_equal(got["slot_src"][:S], _np(k.slot_src)) and _untouched(got["slot_src"][S:]), what
        assert got["xy"].tobytes() == _np(k.gnn).tobytes(), what
        assert np.array_equal(got["pair_ptr"], _np(k.pair_ptr)), what
        if c["truth"] is not None:
            assert np.array_equal(got["truth"], _np(k.truth)), what
        else:
            assert _untouched(got["truth"]) and not kg.truth, what
        hg = k._g
        assert list(cnt.count) == list(hg.count) and list(cnt.first) == list(hg.first) and cnt.n_d1 == hg.n_d1, what
        assert list(cnt.n_deg) == list(hg.n_deg), what
        assert (kg.n_nodes, kg.n_slots, kg.gnn_stride, kg.slot0, kg.pair0, kg.n_blk, kg.deg_runs) == \
            (N, S, 2, 0, 0, 0, hg.deg_runs) and not kg.blk, what
        assert list(kg.count) == list(hg.count) and list(kg.first) == list(hg.first) and kg.n_d1 == hg.n_d1, what
        assert list(kg.n_deg) == list(hg.n_deg), what
        if N:
            assert (kg.slot_ptr, kg.slot_src, kg.gnn, kg.pair_ptr) == tuple(
                g[f].data_ptr() + GUARD for f in ("slot_ptr", "slot_src", "xy", "pair_ptr")), what
        if ordered:
            assert np.array_equal(got["node_of"], k.node_of) and np.array_equal(got["slot_of"][:S], k.slot_of), what
            assert _untouched(got["slot_of"][S:]) and _untouched(got["list"]) and not any(kg.list), what
        else:
            first = 0
            for b in range(4):
                n_b = int(k.lists[b].numel())
                assert cnt.count[b] == n_b and np.array_equal(got["list"][first:first + n_b], _np(k.lists[b])), what
                assert (kg.list[b] or 0) == (g["list"].data_ptr() + GUARD + 4 * first if n_b else 0), what
                first += n_b
            assert _untouched(got["node_of"]) and _untouched(got["slot_of"]), what
        if compact:
            assert cnt.scale == k.scale == q.scale, what
            assert np.array_equal(got["q"].reshape(-1, 2), _np(k.q)), what
            if c["truth"] is not None:
                assert np.array_equal(got["truth32"], _np(k.truth32)), what
            else:
                assert _untouched(got["truth32"]) and not q.truth32, what
        else:
            assert cnt.scale == 0.0 and _untouched(got["q"]) and _untouched(got["truth32"]) and not q.xy, what


def test_abi_refuses_a_short_workspace_without_writing():
    from gtf import _native as nat
    c = kc.case("n255")
    L = nat.lib()
    mem = Mem("torch")
    N, S = c["ptr"].size - 1, c["src"].size
    nb = int(L.gtf_kl_prepare_workspace_bytes(N, S))
    out = mem.guarded(8 * (N + S + 1))
    d = [mem.up(c[f]) for f in ("ptr", "src", "gnn")]
    pin = nat.GtfKlPrepareIn(n_nodes=N, n_slots=S, slot_ptr=d[0].data_ptr(), slot_src=d[1].data_ptr(),
                             gnn=d[2].data_ptr(), gnn_stride=4)
    buf = nat.GtfKlPrepareBuf(*[at(out)] * 10)
    rc = L.gtf_kl_prepare(ctypes.byref(pin), ctypes.byref(buf), ctypes.byref(nat.GtfKlGraph()), None,
                          ctypes.byref(nat.GtfKlCounts()), at(out), nb - 1, mem.stream)
    assert rc == -2 and "workspace" in L.gtf_last_error().decode()
    assert _untouched(mem.payload(out, 8 * (N + S + 1), np.uint8))


# ---------------------------------------------------------------- 2. run() of the device-prepared object
def _device_object(c, mode):
    """the case through the Python entry points: from_device where it has is_edge or a given scale,
    else ParabolicKL(prepare="device")"""
    import torch
    from gtf.parabolic import ParabolicKL
    ordered, with_single, compact = mode
    if c["is_edge"] is None and c["scale"] is None:
        return ParabolicKL(c["ptr"], c["src"], c["gnn"], c["truth"], with_single=with_single, ordered=ordered,
                           compact=compact, prepare="device")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda() if a is not None else None  # noqa: E731
    return ParabolicKL.from_device(t(c["ptr"]), t(c["src"]), t(c["gnn"]), t(c["truth"]), t(c["is_edge"]),
                                   with_single=with_single, ordered=ordered, compact=compact, scale=c["scale"])


def _same_outputs(a, b, what):
    assert sorted(a) == sorted(b), what
    for f in a:
        if f.startswith("_"):   # (the padded buffers "kl" and "truth" are views of: one unwritten element without pairs)
            continue
        assert _np(a[f]).tobytes() == _np(b[f]).tobytes(), what + (f,)


def _structure_equal(kd, kh, what):
    for f in ("slot_ptr", "slot_src", "gnn", "truth", "pair_ptr", "q", "truth32"):
        a, b = getattr(kd, f), getattr(kh, f)
        assert (a is None) == (b is None) and (a is None or _np(a).tobytes() == _np(b).tobytes()), what + (f,)
    assert (kd.n_nodes, kd.n_slots, kd.n_pairs, kd.n_listed, kd.scale) == \
        (kh.n_nodes, kh.n_slots, kh.n_pairs, kh.n_listed, kh.scale), what
    for f in ("node_of", "slot_of", "degree", "slot_ptr_host", "pair_ptr_host"):   # the lazy downloads
        a, b = getattr(kd, f), getattr(kh, f)
        assert (a is None) == (b is None) and (a is None or (a.dtype == b.dtype and np.array_equal(a, b))), what + (f,)
    if kh.node_of is None:   # (the ordered layout reads no list: a device-prepared object holds none)
        assert all(np.array_equal(_np(x), _np(y)) for x, y in zip(kd.lists, kh.lists)), what


@pytest.mark.parametrize("name", [n for n in kc.NAMES if kc.case(n)["error"] is None])
def test_run_is_bit_equal_and_rows_match(name):
    """kl, truth, emp_var, emp_mean, sv and cov of the device-prepared object against the
    host-prepared one as bytes (f64, f32 and, compact, q32); gtf_kl_pair_rows against pair_index() + gather"""
    c = kc.case(name)
    for mode in c["modes"]:
        kh, kd = kc.host(c, mode, device="cuda"), _device_object(c, mode)
        what = (name, mode)
        _structure_equal(kd, kh, what)
        if kh.n_nodes == 0:
            assert kd.rows_dev({})["node"].numel() == 0
            continue
        for dtype in ("f64", "f32") + (("q32",) if mode[2] else ()):
            args = dict(truth=True, emp=True, states=dtype == "f64")
            oh, od = kh.run(kh.alloc(dtype, **args), dtype), kd.run(kd.alloc(dtype, **args), dtype)
            _same_outputs(od, oh, what + (dtype,))
            assert kd.errors() == kh.errors(), what
            node, i, j = kh.pair_index()
            ev = _np(oh["emp_var"])[kh.pair_index(device_nodes=True)[0]]
            for k in (kd, kh):   # (kh: a host-prepared object uploads its node_of once)
                rows = k.rows_dev(od)
                assert rows["node"].dtype == rows["i"].dtype == rows["j"].dtype
                assert np.array_equal(_np(rows["node"]), node) and np.array_equal(_np(rows["i"]), i), what + (dtype,)
                assert np.array_equal(_np(rows["j"]), j), what + (dtype,)
                assert rows["emp_var"].dtype == od["emp_var"].dtype, what
                assert _np(rows["emp_var"]).tobytes() == ev.tobytes(), what + (dtype,)


@pytest.mark.parametrize("name", [n for n in kc.NAMES if kc.case(n)["error"] is not None])
def test_python_raises_value_error(name):
    c = kc.case(name)
    for mode in c["modes"]:
        with pytest.raises(ValueError) as e:
            _device_object(c, mode)
        assert c["error"] in str(e.value), (mode, str(e.value))
        assert str(e.value).startswith("quantise_xy: ") == name.startswith(("err_nan", "err_inf", "err_scale")), name
    if "fit" in c["error"]:   # quantise_xy's wording, figures included
        from gtf.parabolic import quantise_xy
        with pytest.raises(ValueError) as h:
            quantise_xy(c["gnn"], c["scale"])
        assert str(h.value) == str(e.value)


# ---------------------------------------------------------------- 3. the Python entry points
@pytest.mark.parametrize("dtype", ["f64", "f32", "q32"])
def test_training_rows_csr_device_equals_default(dtype):
    from gtf import parabolic
    ptr, src, gnn, truth = kc.vol7()
    a = parabolic.training_rows_csr(ptr, src, gnn, truth, dtype)
    b = parabolic.training_rows_csr(ptr, src, gnn, truth, dtype, prepare="device")
    assert len(a) == len(b) == 6 and a[0].size == 7574
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
    c = kc.case("every_degree")
    a = parabolic.training_rows_csr(c["ptr"], c["src"], c["gnn"], None, dtype)
    b = parabolic.training_rows_csr(c["ptr"], c["src"], c["gnn"], None, dtype, prepare="device")
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()


def test_training_rows_device_equals_default():
    from gtf import parabolic
    from test_kat_parabolic import kat_event
    g, truth = kat_event()
    for x, y in zip(parabolic.training_rows(g, truth), parabolic.training_rows(g, truth, prepare="device")):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()


def test_tile_with_device_prepare_is_refused():
    from gtf.parabolic import ParabolicKL
    c = kc.case("n255")
    with pytest.raises(ValueError, match="tiled layout"):
        ParabolicKL(c["ptr"], c["src"], c["gnn"], tile=64, prepare="device")


@pytest.mark.parametrize("specs", [[("vol7",)], [("vol7",), ("hand", "perm257"), ("empty",), ("vol7",)]],
                         ids=["from_event", "from_events"])
def test_from_device_graph(specs):
    """a resident event, and the fused graph of a batch, against from_graph(host_graph())"""
    import batch_cases as bc
    from gtf.device import DeviceGraph
    from gtf.parabolic import ParabolicKL
    cols = [bc.columns(s) for s in specs]
    d = DeviceGraph.from_event(*cols[0]) if len(specs) == 1 else DeviceGraph.from_events(cols)
    h = d.host_graph()[0]
    assert h.n_nodes == sum(x[0].size for x in cols)
    truth = np.random.default_rng(3).integers(0, 500, h.n_nodes)
    for tr, with_single in ((None, False), (truth, True)):
        kh = ParabolicKL.from_graph(h, tr, with_single=with_single)
        kd = ParabolicKL.from_device_graph(d, tr, with_single=with_single)
        _structure_equal(kd, kh, (len(specs), with_single))
        args = dict(truth=True, emp=True, states=True)
        _same_outputs(kd.run(kd.alloc("f64", **args)), kh.run(kh.alloc("f64", **args)), (len(specs), with_single))
    ko = ParabolicKL.from_device_graph(d, truth, ordered=True, compact=True)
    from gtf import parabolic
    ptr, src = parabolic.in_edge_csr(h)
    kh = ParabolicKL(ptr, src, h.node["gnn"], truth, ordered=True, compact=True)
    _structure_equal(ko, kh, (len(specs), "ordered"))
    _same_outputs(ko.run(ko.alloc("q32"), "q32"), kh.run(kh.alloc("q32"), "q32"), (len(specs), "q32"))


@pytest.mark.parametrize("prepare", ["host", "device"])
@pytest.mark.parametrize("ordered,compact", [(False, False), (True, True)])
def test_replica_from_a_device_tensor(prepare, ordered, compact):
    """replica(gnn=device tensor), [N, 4] and [N, 2], against the host replica of the same coordinates"""
    import torch
    from gtf import parabolic
    ptr, src, gnn, truth = kc.vol7()
    bptr, bsrc, g0, btr = parabolic.batch(ptr, src, gnn, truth, 2, seed=0)
    g1 = parabolic.batch(ptr, src, gnn, truth, 2, seed=1)[2]
    k = parabolic.ParabolicKL(bptr, bsrc, g0, btr, ordered=ordered, compact=compact, prepare=prepare)
    rh = k.replica(gnn=g1)
    for cols in (4, 2):
        rd = k.replica(gnn=torch.from_numpy(np.ascontiguousarray(g1[:, :cols])).cuda())
        assert torch.equal(rd.gnn, rh.gnn) and rd.gnn.data_ptr() != k.gnn.data_ptr()
        if compact:
            assert torch.equal(rd.q, rh.q) and rd.scale == rh.scale == k.scale and rd.q.data_ptr() != k.q.data_ptr()
        for dtype in ("f64",) + (("q32",) if compact else ()):
            _same_outputs(rd.run(rd.alloc(dtype), dtype), rh.run(rh.alloc(dtype), dtype), (prepare, ordered, dtype))
        assert rd.errors() == 0
    if compact:
        far = torch.from_numpy(g1 * 2.0).cuda()   # max |xy| ~ 351 >= 2^8: beyond the parent's scale
        with pytest.raises(ValueError, match="quantise_xy"):
            k.replica(gnn=far)
        bad = torch.from_numpy(g1).cuda()
        bad[5, 1] = float("nan")
        with pytest.raises(ValueError, match="non-finite coordinate"):
            k.replica(gnn=bad)
