"""The compact (32-bit fixed-point) input mode of the parabolic KL stage on the GPU:
gtf_parabolic_kl_q32 through gtf.parabolic.ParabolicKL(compact=True) / run(out, "q32").

The accuracy bar is the project's own fp32 bar (test_gpu_batches.py::
test_c5_fp32_envelope_256_events): median relative KL error < 1e-5, 99th percentile < 1e-3,
no decision flip at k in {1, 2, 10, 100}, identical truth flags."""
import numpy as np
import pytest

from test_kat_parabolic import kat_event, kat_rows, sorted_rows

pytestmark = pytest.mark.gpu

KS = (1.0, 2.0, 10.0, 100.0)
MEDIAN_BAR, P99_BAR = 1e-5, 1e-3


def _rel(a, b):
    return np.abs(a - b) / np.maximum(np.abs(b), 1e-300)


def _envelope(name, got, ref):
    """print and return (median, p99, flips) of got against ref"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    r = _rel(got, ref)
    p50, p99 = np.percentile(r, 50), np.percentile(r, 99)
    flips = {t: int(((ref < t) != (got < t)).sum()) for t in KS}
    err = np.abs(got - ref)
    small, near0 = ref < 1e-3, np.abs(ref) < 1e-3     # (the formula's values can be negative)
    print("%s over %d pairs: median %.3g, p99 %.3g, max %.3g, max abs err where kl < 1e-3 %.3g (%d pairs), "
          "where |kl| < 1e-3 %.3g (%d pairs), flips %s"
          % (name, ref.size, p50, p99, r.max(), err[small].max() if small.any() else 0.0, int(small.sum()),
             err[near0].max() if near0.any() else 0.0, int(near0.sum()), flips))
    return p50, p99, flips


def _assert_envelope(name, got, ref):
    p50, p99, flips = _envelope(name, got, ref)
    assert np.isfinite(got).all()
    assert p50 < MEDIAN_BAR and p99 < P99_BAR, (name, p50, p99)
    assert all(v == 0 for v in flips.values()), (name, flips)


def _dequantised(gnn):
    """(gnn with x, y replaced by q * scale -- exact in fp64 --, scale)"""
    from gtf.parabolic import quantise_xy
    q, scale = quantise_xy(gnn)
    out = np.array(gnn, np.float64)
    out[:, :2] = q.astype(np.float64) * scale
    return out, scale


def _rows(k, out):
    """pair rows and per-node moments of a run in the caller's order (pairs by node, i, j)"""
    node, i, j = k.pair_index()
    key = np.lexsort((j, i, node))
    r = {"rows": np.stack([node, i, j], 1)[key], "kl": out["kl"].cpu().numpy()[key],
         "emp_var": k.host_nodes(out["emp_var"].cpu().numpy())}
    if "truth" in out:
        r["truth"] = out["truth"].cpu().numpy()[key]
    if "emp_mean" in out:
        r["emp_mean"] = k.host_nodes(out["emp_mean"].cpu().numpy())
    return r


# ---------------------------------------------------------------- 1. every bucket at its edges
DEGREES = {1: 40, 2: 40, 3: 40, 4: 40, 5: 9, 8: 9, 9: 3, 63: 2, 64: 2, 65: 2, 130: 2}


def bucket_edge_graph(seed=11):
    """receivers of in-degree 1, 2, 3, 4, 5, 8, 9, 63, 64, 65 and 130 (DEGREES: how many of
    each -- more than one 64-thread block of the thread-per-node buckets, more than one
    block of 8 groups of the 8-lane bucket, two or three wavefront nodes of each size), each
    with senders of its own (in-degree 0), node numbers shuffled. Receivers 30..1000 mm from
    the origin, senders 5..80 mm from their receiver in any direction."""
    rng = np.random.default_rng(seed)
    deg = np.concatenate([np.full(n, d) for d, n in DEGREES.items()])
    n_recv, n_send = deg.size, int(deg.sum())
    r, phi = rng.uniform(30.0, 1000.0, n_recv), rng.uniform(-np.pi, np.pi, n_recv)
    recv = np.stack([r * np.cos(phi), r * np.sin(phi)], 1)
    owner = np.repeat(np.arange(n_recv), deg)
    dr, dphi = rng.uniform(5.0, 80.0, n_send), rng.uniform(-np.pi, np.pi, n_send)
    send = recv[owner] + np.stack([dr * np.cos(dphi), dr * np.sin(dphi)], 1)
    n = n_recv + n_send
    perm = rng.permutation(n)                    # new number of receiver a: perm[a]; of sender b: perm[n_recv + b]
    xy = np.empty((n, 2))
    xy[perm] = np.concatenate([recv, send])
    d_all = np.zeros(n, np.int64)
    d_all[perm[:n_recv]] = deg
    ptr = np.zeros(n + 1, np.int32)
    np.cumsum(d_all, out=ptr[1:])
    src = np.empty(n_send, np.int32)
    first = np.concatenate([[0], np.cumsum(deg)[:-1]])
    for a in range(n_recv):
        s = np.sort(perm[n_recv + first[a]:n_recv + first[a] + deg[a]])   # slot order = sender index order
        src[ptr[perm[a]]:ptr[perm[a]] + deg[a]] = s
    gnn = np.concatenate([xy, np.zeros((n, 1)), np.hypot(xy[:, 0], xy[:, 1])[:, None]], 1)
    truth = rng.integers(0, 3, n).astype(np.int64)
    return ptr, src, gnn, truth


LAYOUTS = {"listed": {}, "ordered": {"ordered": True},
           "tile4": {"tile": 4}, "tile4_list_b1": {"tile": 4, "tile_b1": False},
           "tile256": {"tile": 256}, "tile256_list_b1": {"tile": 256, "tile_b1": False}}


def test_q32_every_bucket_and_layout():
    """every in-degree bucket at its edges through the listed, ordered and tiled (T = 4 and
    256, the 3- / 4-edge nodes in the tiles or by list) layouts: the q32 layouts agree bit for
    bit in kl, truth, emp_var and emp_mean (every layout runs the same per-node code on the
    same values: pkl_b0_finish for d <= 2, pkl_node4_core for d <= 4, pkl_node_core on 8 or 64
    lanes beyond, so no summation order differs), the truth flags equal the f64 kernel's, and
    the distances sit inside the fp32 envelope against the f64 kernel on the de-quantised
    coordinates"""
    from gtf.parabolic import ParabolicKL
    ptr, src, gnn, truth = bucket_edge_graph()
    d = np.diff(ptr)
    for deg, n in DEGREES.items():
        assert int((d == deg).sum()) == n >= 2
    deq, scale = _dequantised(gnn)
    assert scale == 2.0 ** -20                   # (this seed: max |xy| in [512, 1024))
    kr = ParabolicKL(ptr, src, deq, truth, with_single=True)
    ref = _rows(kr, kr.run(kr.alloc("f64"), "f64"))
    assert kr.errors() == 0
    res = {}
    for name, kw in LAYOUTS.items():
        k = ParabolicKL(ptr, src, gnn, truth, with_single=True, compact=True, **kw)
        assert k.scale == scale
        res[name] = _rows(k, k.run(k.alloc("q32"), "q32"))
        assert k.errors() == 0, name
    a = res["listed"]
    assert a["kl"].dtype == a["emp_var"].dtype == a["emp_mean"].dtype == np.float32
    assert np.array_equal(a["rows"], ref["rows"]) and np.array_equal(a["truth"], ref["truth"])
    listed = d >= 1
    assert np.isfinite(a["emp_var"][listed]).all() and np.isnan(a["emp_var"][~listed]).all()
    assert (a["emp_var"][d == 1] == 0.0).all()
    for name, b in res.items():
        for f in a:
            assert np.array_equal(a[f], b[f], equal_nan=a[f].dtype.kind == "f"), (name, f)
    _assert_envelope("bucket-edge graph, q32 vs f64 on the de-quantised coordinates", a["kl"], ref["kl"])
    # the moments against the f64 kernel's: float stores of fp64 sums of float gradients
    for f in ("emp_mean", "emp_var"):
        r = _rel(a[f][listed].astype(np.float64), ref[f][listed])
        print("bucket-edge graph %s: median %.3g, p99 %.3g" % (f, np.median(r), np.percentile(r, 99)))


# ---------------------------------------------------------------- 2. envelope on the KAT event
@pytest.fixture(scope="module")
def kat4():
    """4 jittered copies of the committed vol-7 134 event (seed 0: 30,296 pairs), the q32 run
    and the f64 runs on the original and on the de-quantised coordinates, all in the ordered
    layout (the same pair order)"""
    import torch
    from gtf import parabolic
    g, truth = kat_event()
    ptr, src = parabolic.in_edge_csr(g)
    bptr, bsrc, bgnn, btr = parabolic.batch(ptr, src, g.node["gnn"], truth, 4, seed=0)
    k = parabolic.ParabolicKL(bptr, bsrc, bgnn, btr, ordered=True, compact=True)
    assert k.n_pairs == 30296 and k.scale == 2.0 ** -22
    deq, _ = _dequantised(bgnn)
    kd = parabolic.ParabolicKL(bptr, bsrc, deq, btr, ordered=True)
    q32 = k.run(k.alloc("q32"), "q32")
    f64 = k.run(k.alloc("f64"), "f64")
    f64d = kd.run(kd.alloc("f64"), "f64")
    torch.cuda.synchronize()
    return {"k": k, "kd": kd, "q32": q32, "f64": f64, "f64d": f64d, "csr": (bptr, bsrc, deq), "errors": k.errors()}


def test_q32_envelope_kat(kat4):
    """q32 against f64 on the de-quantised coordinates (the arithmetic alone) and against f64
    on the original coordinates (what a user sees): the fp32 bar, no flips, identical truth
    flags, no error word"""
    import torch
    assert kat4["errors"] == 0 and kat4["kd"].errors() == 0
    q = kat4["q32"]["kl"].cpu().numpy()
    _assert_envelope("KAT x4, q32 vs f64 on the de-quantised coordinates", q, kat4["f64d"]["kl"].cpu().numpy())
    _assert_envelope("KAT x4, q32 vs f64 on the original coordinates", q, kat4["f64"]["kl"].cpu().numpy())
    assert torch.equal(kat4["q32"]["truth"], kat4["f64"]["truth"])
    assert torch.equal(kat4["q32"]["truth"], kat4["f64d"]["truth"])


def test_q32_moments_kat(kat4):
    """emp_mean / emp_var against the f64 kernel on the de-quantised coordinates. The
    gradient variance is ill-conditioned where dx -> 0, so the bar is relative to the shipped
    fp32-precision computation of the same quantity -- the fp64 gradients cast to float, the
    moments formed from those in fp64 and stored as float: q32 (one more rounding of each
    difference, then the float division) must stay within 4x of its median and 99th-percentile
    relative error."""
    k = kat4["k"]
    bptr, bsrc, deq = kat4["csr"]
    d = np.diff(bptr).astype(np.int64)
    v = np.repeat(np.arange(d.size), d)
    u = bsrc.astype(np.int64)
    grad = ((deq[v, 1] - deq[u, 1]) / (deq[v, 0] - deq[u, 0])).astype(np.float32).astype(np.float64)
    lst = d >= 2
    mean_all = np.bincount(v, grad, d.size) / np.maximum(d, 1)
    var_all = np.bincount(v, (grad - mean_all[v]) ** 2, d.size) / np.maximum(d, 1)
    mean, var = mean_all[lst], var_all[lst]
    base = {"emp_mean": mean.astype(np.float32).astype(np.float64), "emp_var": var.astype(np.float32).astype(np.float64)}
    for f in ("emp_mean", "emp_var"):
        ref = kat4["kd"].host_nodes(kat4["f64d"][f].cpu().numpy())[lst]
        got = k.host_nodes(kat4["q32"][f].cpu().numpy())[lst].astype(np.float64)
        assert np.isfinite(ref).all() and np.isfinite(got).all()
        ok = ref != 0.0
        rq, rb = _rel(got[ok], ref[ok]), _rel(base[f][ok], ref[ok])
        mq, pq, mb, pb = np.median(rq), np.percentile(rq, 99), np.median(rb), np.percentile(rb, 99)
        print("%s over %d nodes: q32 median %.3g p99 %.3g; fp64 gradients cast to float median %.3g p99 %.3g"
              % (f, int(ok.sum()), mq, pq, mb, pb))
        assert mq <= 4 * mb and pq <= 4 * pb, (f, mq, mb, pq, pb)


# ---------------------------------------------------------------- 3. KAT-1 through the compact path
def test_q32_rows_match_committed_training_csv():
    """KAT-1 through training_rows_csr(dtype="q32"): truth flags exact and the distances
    inside the fp32 envelope (median and 99th percentile over the 7,574 rows, no flips)
    relative to the committed CSV. The 1e-8 bar of test_gpu_parabolic.py belongs to the fp64
    path only. Rows are matched to the CSV's by pair: the f64 run of the same event has the
    same pair order and is known to match the CSV row for row once both are sorted
    (sorted_rows), so its sorting permutation places the q32 rows too -- sorting the q32
    rows by their own fp32 distances could swap near-equal rows of different truth."""
    from gtf import parabolic
    g, truth = kat_event()
    ptr, src = parabolic.in_edge_csr(g)
    n64, i64, j64, kl64, ev64, tr64 = parabolic.training_rows_csr(ptr, src, g.node["gnn"], truth, "f64")
    node, i, j, kl, ev, tr = parabolic.training_rows_csr(ptr, src, g.node["gnn"], truth, "q32")
    assert kl.dtype == np.float32 and ev.dtype == np.float32 and kl.size == 7574
    assert np.array_equal(node, n64) and np.array_equal(i, i64) and np.array_equal(j, j64)
    kat = kat_rows()
    o = np.lexsort((tr64.astype(np.float64), ev64, kl64))     # sorted_rows' order
    b = sorted_rows(kat["kl_dist"], kat["emp_var"], kat["truth"])
    assert (np.abs(kl64[o] - b[0]) <= 1e-8 * np.abs(b[0])).all() and (tr64[o] == b[2]).all()   # the pairing holds
    assert (tr[o] == b[2]).all() and int(tr.sum()) == 5231
    _assert_envelope("KAT-1, q32 vs the committed CSV", kl[o], b[0])
    r = _rel(ev[o].astype(np.float64), b[1])
    print("KAT-1 emp_var vs the CSV: median %.3g, p99 %.3g" % (np.median(r), np.percentile(r, 99)))


# ---------------------------------------------------------------- 4. singular input, no pairs
@pytest.mark.parametrize("ordered", [False, True])
def test_q32_singular_sets_the_error_word(ordered):
    """test_gpu_parabolic.py's singular case: node 1 at (10, 0), neighbour 0 at the same x
    after rotation (x_B = 0; the integer difference is exactly 0)"""
    from gtf import parabolic
    gnn = np.array([[10.0, 5.0, 0, 11.18], [10.0, 0.0, 0, 10.0], [20.0, 1.0, 0, 20.0]])
    ptr = np.array([0, 0, 2, 2], np.int32)
    src = np.array([0, 2], np.int32)
    k = parabolic.ParabolicKL(ptr, src, gnn, ordered=ordered, compact=True)
    k.run(k.alloc("q32"), "q32")
    assert k.errors() & 128
    if not ordered:
        with pytest.raises(np.linalg.LinAlgError):
            parabolic.training_rows_csr(ptr, src, gnn, dtype="q32")


@pytest.mark.parametrize("ordered", [False, True])
def test_q32_isolated_node_and_no_pairs(ordered):
    """an isolated node, a one-edge node and no pairs: the pair outputs hold one dummy
    element, the launch returns 0 and the error word stays clear"""
    from gtf.parabolic import ParabolicKL
    gnn = np.array([[10.0, 1.0, 0, 10.05], [20.0, 2.0, 0, 20.1]])
    k = ParabolicKL(np.array([0, 0, 1], np.int32), np.array([0], np.int32), gnn, np.array([3, 3], np.int64),
                    with_single=True, ordered=ordered, compact=True)
    out = k.run(k.alloc("q32"), "q32")
    assert k.n_pairs == 0 and out["kl"].numel() == 0 and out["_kl"].numel() == 1
    assert k.errors() == 0
    ev, em = k.host_nodes(out["emp_var"].cpu().numpy()), k.host_nodes(out["emp_mean"].cpu().numpy())
    assert ev[1] == 0.0 and em[1] == np.float32(0.1) and np.isnan(ev[0])
    k0 = ParabolicKL(np.array([0, 0, 1], np.int32), np.array([0], np.int32), gnn, ordered=ordered, compact=True)
    k0.run(k0.alloc("q32"), "q32")              # nothing listed: no launch at all
    assert k0.n_listed == 0 and k0.errors() == 0


# ---------------------------------------------------------------- 5. replica
def test_q32_replica_requantises_with_the_parents_scale():
    """a replica with other jittered coordinates gives the rows of a fresh compact object
    built from those coordinates (same scale); coordinates beyond the scale's range raise"""
    import torch
    from gtf import parabolic
    g, truth = kat_event()
    ptr, src = parabolic.in_edge_csr(g)
    bptr, bsrc, g0, btr = parabolic.batch(ptr, src, g.node["gnn"], truth, 2, seed=0)
    g1 = parabolic.batch(ptr, src, g.node["gnn"], truth, 2, seed=1)[2]
    assert not np.array_equal(g0, g1)
    k = parabolic.ParabolicKL(bptr, bsrc, g0, btr, ordered=True, compact=True)
    r = k.replica(gnn=g1)
    fresh = parabolic.ParabolicKL(bptr, bsrc, g1, btr, ordered=True, compact=True)
    assert r.scale == k.scale == fresh.scale and torch.equal(r.q, fresh.q) and not torch.equal(r.q, k.q)
    assert r.q.data_ptr() != k.q.data_ptr() and r.truth32.data_ptr() != k.truth32.data_ptr()
    a, b = r.run(r.alloc("q32"), "q32"), fresh.run(fresh.alloc("q32"), "q32")
    same = k.replica()
    c, d = same.run(same.alloc("q32"), "q32"), k.run(k.alloc("q32"), "q32")
    for f in ("kl", "truth", "emp_var", "emp_mean"):
        assert torch.equal(a[f].nan_to_num(7.0), b[f].nan_to_num(7.0)), f
        assert torch.equal(c[f].nan_to_num(7.0), d[f].nan_to_num(7.0)), f
    assert not torch.equal(a["kl"], d["kl"])
    assert r.errors() == 0 and fresh.errors() == 0 and same.errors() == 0
    # the replica's fp64 path still works beside it
    assert torch.equal(r.run(r.alloc("f64"), "f64")["kl"], fresh.run(fresh.alloc("f64"), "f64")["kl"])
    far = np.array(g1)
    far[:, :2] *= 2.0                           # max |xy| ~ 351 >= 2^8: beyond scale 2^-22
    with pytest.raises(ValueError):
        k.replica(gnn=far)
