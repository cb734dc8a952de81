"""gtf_parabolic_kl (§8 a17) on the GPU, through the C-ABI.

* KAT: the rows the GPU produces for the committed volume-7 134 event equal the
  reference's committed training CSV as a multiset (kl 1e-8 rel, emp_var 1e-9 rel,
  truth exact) -- the same bar the oracle meets (test_kat_parabolic.py).
* Row by row against the oracle (np.linalg.inv restatement) on the KAT event and on
  a synthetic event with nodes of up to ~60 in-edges (the one-wavefront path and
  its beyond-LDS recompute path).
* States: edge_state_vector / edge_covariance per in-edge vs the oracle.
* fp32: the config-5 sweep's fp32 mode stays within its stated envelope.
* Singular H: the geometric rule raises GTF_ERR_SINGULAR_H (see test_gpu_singular_raises).

The exact-arithmetic distance that _check_rows_vs_oracle falls back on is kl_cases.exact_kl (50-digit
decimal), shared with the directed cases of test_gpu_kl_cases.py.
"""
import os
import numpy as np
import pytest

import gtf_oracle as O
from gtf import synth
from gtf.graph import TrackGraph
from kl_cases import exact_kl as _true_kl
from test_kat_parabolic import kat2_event, kat2_match, kat_event, kat_rows, sorted_rows

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return np.abs(a - b) / np.maximum(np.abs(b), 1e-300)


def test_gpu_rows_match_committed_training_csv():
    from gtf import parabolic
    g, truth = kat_event()
    node, i, j, kl, ev, tr = parabolic.training_rows(g, truth)
    kat = kat_rows()
    assert kl.size == kat.size == 7574
    a = sorted_rows(kl, ev, tr.astype(np.float64))
    b = sorted_rows(kat["kl_dist"], kat["emp_var"], kat["truth"])
    assert _rel(a[0], b[0]).max() < 1e-8
    assert (np.abs(a[1] - b[1]) <= 1e-9 * np.abs(b[1])).all()
    assert (a[2] == b[2]).all()
    assert int(tr.sum()) == 5231


def test_gpu_rows_match_kat2():
    """KAT-2: the GPU's rows for volume 7 of the committed 800' event are
    rows of the reference's 3_events_training_data.csv, 1,054 of 1,055 (the one not found
    is the oracle's and the survey's too: test_kat_parabolic.test_parabolic_rows_match_kat2)"""
    from gtf import parabolic
    g, truth = kat2_event()
    node, i, j, kl, ev, tr = parabolic.training_rows(g, truth)
    assert kl.size == 1055
    missing = kat2_match(kl, ev, tr.astype(np.float64))
    assert len(missing) == 1 and g.node["node_id"][node[missing[0]]] == 1635, missing


def _check_rows_vs_oracle(g, truth, tol):
    """rows equal the oracle's; distances within tol, or -- where the oracle's
    np.linalg.inv of an ill-conditioned covariance is itself off -- no further from
    the exact value than the oracle (printed counts)"""
    from gtf import parabolic
    got = parabolic.training_rows(g, truth)
    ref = O.parabolic_training_rows(g, truth)
    for a, b in zip(got[:3], ref[:3]):
        assert (a == b).all()
    r = _rel(got[3], ref[3])
    gnn, src, ptr = g.node["gnn"], g.slot["slot_src"], g.slot_ptr
    bad = np.nonzero(r >= tol)[0]
    for n in bad:
        v, i, j = got[0][n], got[1][n], got[2][n]
        t = _true_kl(gnn[v], gnn[src[ptr[v] + i]], gnn[src[ptr[v] + j]])
        eg, eo = abs(got[3][n] - t), abs(ref[3][n] - t)
        assert eg <= max(10 * eo, tol * abs(t)), (n, got[3][n], ref[3][n], t)
    print("pairs %d: %d beyond %g of the oracle, each no further from the exact value" % (r.size, bad.size, tol))
    assert (np.abs(got[4] - ref[4]) <= 1e-9 * np.abs(ref[4]) + 1e-300).all()
    assert (got[5] == ref[5]).all()
    return got


def test_gpu_rows_match_oracle_kat_event():
    g, truth = kat_event()
    _check_rows_vs_oracle(g, truth, 1e-8)


def _dense_event():
    g = synth.event(seed=5, n_tracks=400, fake_mean=synth.C4_FAKE)
    return g, np.random.default_rng(5).integers(0, 50, g.n_nodes)


def test_gpu_rows_match_oracle_wavefront_path():
    g, truth = _dense_event()
    d = np.diff(g.slot_ptr)
    assert d.max() > 8, "need nodes on the one-wavefront path"
    got = _check_rows_vs_oracle(g, truth, 1e-8)
    print("pairs %d, max degree %d" % (got[3].size, d.max()))


def test_gpu_states_match_oracle():
    from gtf import parabolic
    g, _ = kat_event()
    sv, cov, gm, gv = parabolic.compute_track_state_estimates(g)
    gnn, src = g.node["gnn"], g.slot["slot_src"]
    for v in range(0, g.n_nodes, 7):
        lo, hi = g.slot_ptr[v], g.slot_ptr[v + 1]
        if hi == lo:
            continue
        for k, (s, c) in zip(range(lo, hi), O.parabolic_states(gnn[v], gnn[src[lo:hi]])):
            assert np.allclose(sv[k], s, rtol=1e-8, atol=1e-12 * np.abs(s).max())
            assert np.allclose(cov[k], c, rtol=1e-8, atol=1e-12 * np.abs(c).max())
        grads = (gnn[v][1] - gnn[src[lo:hi], 1]) / (gnn[v][0] - gnn[src[lo:hi], 0])
        assert np.isclose(gm[v], np.mean(grads), rtol=1e-12, atol=1e-15)
        assert np.isclose(gv[v], np.var(grads), rtol=1e-9, atol=1e-18)


def test_gpu_fp32_envelope():
    """fp32 mode: states and distances in fp32 after fp64 geometry. Envelope measured
    on the KAT event: median rel err < 1e-5, 99th pct < 1e-3."""
    from gtf.parabolic import ParabolicKL
    g, truth = kat_event()
    k = ParabolicKL.from_graph(g, truth)
    a = k.run(k.alloc("f64"), "f64")["kl"].cpu().numpy()
    b = k.run(k.alloc("f32"), "f32")["kl"].cpu().numpy().astype(np.float64)
    r = _rel(b, a)
    assert np.isfinite(b).all()
    assert np.median(r) < 1e-5 and np.percentile(r, 99) < 1e-3, (np.median(r), np.percentile(r, 99))


def test_gpu_singular_raises():
    """The flag is raised wherever the reference raises, and additionally at exact geometric singularity
    (x_B == 0, x_B == x_0 or x_0 == 0 in the kernel's rotation), where the reference returns unbounded
    values. This input, node (10, 0) with neighbour (10, 5), is of the second kind: the reference's
    rotation by cos / sin(2 pi - atan2) leaves x_B a few ulp from 0, np.linalg.inv does not raise and the
    state it returns has sv ~ 2.8e14 and cov[0][0] ~ 6e25 (recorded as sing_perp_axis_0 in
    tests/golden/kl_cases.npz; its image (-10, 0) / (-10, 5) raises in the reference too)."""
    from gtf import parabolic
    # node 1 at (10, 0); neighbour 0 at the same x after rotation (x_B = 0)
    gnn = np.array([[10.0, 5.0, 0, 11.18], [10.0, 0.0, 0, 10.0], [20.0, 1.0, 0, 20.0]])
    ptr = np.array([0, 0, 2, 2], np.int32)
    src = np.array([0, 2], np.int32)
    k = parabolic.ParabolicKL(ptr, src, gnn)
    k.run(k.alloc("f64"), "f64")
    assert k.errors() & 128
    # training_rows turns the flag into the LinAlgError np.linalg.inv raises at the singular images (utils.py:285)
    with pytest.raises(np.linalg.LinAlgError):
        parabolic.training_rows_csr(ptr, src, gnn)


@pytest.mark.parametrize("ordered", [False, True])
def test_gpu_empty_and_single(ordered):
    from gtf.parabolic import ParabolicKL
    gnn = np.array([[10.0, 1.0, 0, 10.05], [20.0, 2.0, 0, 20.1]])
    k = ParabolicKL(np.array([0, 0, 1], np.int32), np.array([0], np.int32), gnn, with_single=True, ordered=ordered)
    out = k.run(k.alloc("f64", states=True), "f64")
    assert k.n_pairs == 0 and out["kl"].numel() == 0
    assert np.isfinite(out["sv"].cpu().numpy()).all()
    assert k.host_nodes(out["emp_var"].cpu().numpy())[1] == 0.0


def test_gpu_beyond_lds_recompute_path():
    """a node with 70 in-edges (> the 64 states a wavefront stages in LDS)"""
    from gtf import parabolic
    rng = np.random.default_rng(3)
    n = 71
    phi = rng.uniform(0.2, 0.4, n)
    r = np.concatenate([[300.0], rng.uniform(100, 600, n - 1)])
    gnn = np.stack([r * np.cos(phi), r * np.sin(phi), np.zeros(n), r], 1)
    ptr = np.array([0] + [n - 1] * n, np.int32)
    src = np.arange(1, n, dtype=np.int32)
    k = parabolic.ParabolicKL(ptr, src, gnn)
    kl = k.run(k.alloc("f64"), "f64")["kl"].cpu().numpy()
    st = O.parabolic_states(gnn[0], gnn[1:])
    ref = np.asarray(O.parabolic_kl_pairs([s for s, _ in st], [c for _, c in st]))
    assert kl.size == ref.size == 70 * 69 // 2
    assert _rel(kl, ref).max() < 1e-6


@pytest.mark.parametrize("tile", [0, 256, 100, -256])
@pytest.mark.parametrize("with_single", [False, True])
def test_gpu_ordered_layout_equals_lists(with_single, tile):
    """ParabolicKL(ordered=True) (bucket node ranges, the two-edge bucket by arithmetic) and
    ParabolicKL(tile=T) (tiles of T one- to four-edge nodes with their LDS windows, one
    256-thread block each, the larger buckets by list; -T: tiles of T one- / two-edge nodes,
    the 3- / 4-edge bucket by list too) give the list layout's pair rows, truth flags,
    gradient moments and states bit for bit once mapped back to the caller's order (16
    jittered copies of the vol-7 event)"""
    from gtf import io, parabolic
    kat = os.path.join(GOLDEN, "kat134")
    g = io.load_event(os.path.join(kat, "event_1_filtered_graph_"), 7, 7)
    truth = io.read_truth(os.path.join(kat, "truth_vol7.csv"), g.node["node_id"])
    ptr, src = parabolic.in_edge_csr(g)
    ptr, src, gnn, tr = parabolic.batch(ptr, src, g.node["gnn"], truth, 16)
    res = []
    for ordered in (False, True):
        k = parabolic.ParabolicKL(ptr, src, gnn, tr, with_single=with_single, ordered=ordered,
                                  tile=abs(tile) if ordered else 0, tile_b1=tile > 0)
        out = k.run(k.alloc("f64", emp=True, states=with_single), "f64")
        node, i, j = k.pair_index()
        key = np.lexsort((j, i, node))
        r = {"rows": np.stack([node, i, j], 1)[key], "kl": out["kl"].cpu().numpy()[key],
             "truth": out["truth"].cpu().numpy()[key],
             "emp_var": k.host_nodes(out["emp_var"].cpu().numpy()),
             "emp_mean": k.host_nodes(out["emp_mean"].cpu().numpy())}
        if with_single:
            r["sv"] = k.host_slots(out["sv"].cpu().numpy())
            r["cov"] = k.host_slots(out["cov"].cpu().numpy())
        assert k.errors() == 0
        res.append(r)
    a, b = res
    for f in a:
        x, y = a[f], b[f]
        assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), f


@pytest.mark.parametrize("stride", [0, 4])
def test_gpu_four_field_rows_equal_compact(stride):
    """gtf_kl_graph.gnn_stride 0 / 4 (the GNN_Measurement x, y, z, r rows themselves)
    gives the compact x, y copy's (gnn_stride 2, what ParabolicKL uploads) results bit
    for bit, in both layouts"""
    import ctypes
    import torch
    from gtf import io, parabolic
    kat = os.path.join(GOLDEN, "kat134")
    g = io.load_event(os.path.join(kat, "event_1_filtered_graph_"), 7, 7)
    truth = io.read_truth(os.path.join(kat, "truth_vol7.csv"), g.node["node_id"])
    ptr, src = parabolic.in_edge_csr(g)
    for ordered in (False, True):
        k = parabolic.ParabolicKL(ptr, src, g.node["gnn"], truth, ordered=ordered)
        a = k.run(k.alloc("f64", emp=True), "f64")
        rows = g.node["gnn"] if k.node_of is None else g.node["gnn"][k.node_of]
        full = torch.from_numpy(np.ascontiguousarray(rows, np.float64)).to(k.device)
        k._g.gnn, k._g.gnn_stride = ctypes.c_void_p(full.data_ptr()), stride
        b = k.run(k.alloc("f64", emp=True), "f64")
        for f in ("kl", "truth", "emp_var", "emp_mean"):
            assert torch.equal(a[f], b[f]) or (a[f].dtype.is_floating_point and
                                               torch.equal(a[f].nan_to_num(7.0), b[f].nan_to_num(7.0))), f
        assert k.errors() == 0
