"""The fused node kernel's 6- and 12-lane groups (5..6- and 9..12-slot receivers: 10 and 5
nodes per wavefront, gtf_graph.n_g6 / n_g12) on the GPU.

  * oracle parity of one and two full passes on a small event that populates every slot-count
    class, in the tiled layout with a small tile (several tiles, partial last waves in both
    new buckets), at the bar of test_gpu_synthetic.py; the same passes with n_g6 = n_g12 = 0
    forced in the C struct (every node on its power-of-two group) are bit-equal, array for array;
  * hand-built star graphs with exact counts: 11 receivers of 6 slots and 6 of 12 (one full
    wave plus one group each), exactly one full wave of either, and none of either class;
  * 5-slot receivers whose present keys tie in the pairwise chi2 (cut from the reference's
    own tie fixture, cluster_tie): bit for bit the C++ restatement's result.
"""
import numpy as np
import pytest

import cpu_ref
import gtf_oracle as O
from compare import compare, compare_noise, noise_envelope
from fixtures import load
from gtf import graph, synth
from gtf.params import Params
from pass_cases import distances as _tse_distances, tied as _tied   # (the pairwise chi2 matrix of a node's dict)

pytestmark = pytest.mark.gpu

TILE = 256
CLASSES = ((5, 6), (7, 8), (9, 12), (13, 16))


def _bit_equal(a, b, what):
    for kind in ("node", "slot"):
        da, db = getattr(a, kind), getattr(b, kind)
        for k in da:
            x, y = da[k], db[k]
            assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), (what, kind, k)


def _gpu(g, fn, classes, groups=True, layout="tiled"):
    """fn(d) on a fresh DeviceGraph; groups=False: every node on its power-of-two lane group"""
    from gtf.device import DeviceGraph
    d = DeviceGraph(g, layout=layout, tile=TILE, classes=classes)
    if not groups:
        d.cg.n_g6 = 0
        d.cg.n_g12 = 0
    d.clear_errors()
    fn(d)
    flags = d.errors()
    return d, d.download(g.copy()), flags


def _passes(p, n):
    def fn(d):
        for _ in range(n):
            d.full_pass(p)
    return fn


@pytest.fixture(scope="module")
def event():
    """the event and the oracle's outputs with their noise envelopes after one and two passes
    (the second envelope continues the first one's runs instead of repeating their first pass:
    noise_envelope calls run() on the same inputs in the same order)"""
    g = synth.event(seed=7, n_tracks=1000, fake_mean=synth.C4_FAKE)
    p = Params()
    firsts = []

    def run1(x):
        O.full_pass(x, p, tie_policy="stop")
        firsts.append(x.copy())
        return x

    one = noise_envelope(run1, g)
    nxt = iter(firsts)

    def run2(_):
        x = next(nxt)
        O.full_pass(x, p, tie_policy="stop")
        return x

    return g, p, {1: one, 2: noise_envelope(run2, g)}


def test_event_covers_every_class(event):
    g, _, _ = event
    deg = np.diff(g.slot_ptr)
    for lo, hi in CLASSES:
        assert int(((deg >= lo) & (deg <= hi)).sum()) >= 50, (lo, hi)
    assert g.n_nodes > 4 * TILE


@pytest.mark.parametrize("classes", [False, True], ids=["kernel_classes", "static_classes"])
@pytest.mark.parametrize("passes", [1, 2])
def test_passes_match_oracle_and_the_power_of_two_groups(event, passes, classes):
    g, p, refs = event
    ref, noise, flips = refs[passes]
    d, got, flags = _gpu(g, _passes(p, passes), classes)
    deg = np.diff(g.slot_ptr)
    assert d.cg.n_g6 == int(((deg >= 5) & (deg <= 6)).sum()) and d.cg.n_g12 == int(((deg >= 9) & (deg <= 12)).sum())
    errs, stats = compare_noise(got, ref, noise, flips)
    print("%d pass(es): %s, device flags %d" % (passes, stats, flags))
    assert errs == [], "\n".join(errs)
    assert stats["mask_undetermined"] == 0 and stats["mask_ill_differs"] == 0 and stats["ill_nodes"] == 0, stats
    assert stats["float_ill"] <= 2e-6 * stats["float_checked"] + 1, stats
    assert flags == 0, flags
    d0, got0, flags0 = _gpu(g, _passes(p, passes), classes, groups=False)
    assert d0.cg.n_g6 == 0 and d0.cg.n_g12 == 0 and flags0 == flags
    _bit_equal(got, got0, "6/12-lane groups vs 8/16-lane groups")


def star_graph(counts, seed=7, n_tracks=400):
    """hits of a seeded synthetic event, its edges replaced by stars: counts[k] hub hits joined
    (both directions) to the k hits closest in azimuth on the two neighbouring layers, no hit
    used twice -- exactly counts[k] receivers of k slots, every other hit has at most 1"""
    p = Params()
    g = synth.event(seed=seed, n_tracks=n_tracks, fake_mean=synth.C4_FAKE)
    x, y, z, r = (g.node["gnn"][:, i].copy() for i in range(4))
    layer = g.node["layer"].copy()
    phi = np.arctan2(y, x)
    levels = np.unique(layer)
    mid = np.nonzero((layer > levels[0]) & (layer < levels[-1]))[0]
    rng = np.random.default_rng(seed)
    used = np.zeros(g.n_nodes, bool)
    src, dst = [], []
    for k, n in sorted(counts.items()):
        made = 0
        for h in rng.permutation(mid):
            if made == n:
                break
            if used[h]:
                continue
            li = np.searchsorted(levels, layer[h])
            near = np.nonzero(((layer == levels[li - 1]) | (layer == levels[li + 1])) & ~used)[0]
            near = near[near != h]
            if near.size < k:
                continue
            dphi = np.abs(np.angle(np.exp(1j * (phi[near] - phi[h]))))
            leaves = near[np.argsort(dphi)[:k]]
            used[h] = True
            used[leaves] = True
            for v in leaves:
                src += [h, v]
                dst += [v, h]
            made += 1
        assert made == n, (k, n)
    out = synth._assemble(g.n_nodes, np.array(src, np.int64), np.array(dst, np.int64), x, y, z, r, layer, p)
    deg = np.diff(out.slot_ptr)
    for k, n in counts.items():
        assert int((deg == k).sum()) == n
    assert int((deg > 1).sum()) == sum(counts.values())
    return out, p


@pytest.mark.parametrize("counts", [{6: 11, 12: 6}, {6: 10, 12: 5}, {8: 3, 16: 2}, {6: 1}, {12: 1, 3: 2}],
                         ids=["wave_plus_group", "one_full_wave", "neither_class", "one_6", "one_12"])
def test_exact_counts(counts):
    g, p = star_graph(counts)

    def run(x):
        O.full_pass(x, p, tie_policy="stop")
        return x

    ref, noise, flips = noise_envelope(run, g)
    for layout in ("natural", "tiled"):
        d, got, flags = _gpu(g, _passes(p, 1), None, layout=layout)
        assert d.cg.n_g6 == counts.get(6, 0) and d.cg.n_g12 == counts.get(12, 0)
        errs, stats = compare_noise(got, ref, noise, flips)
        assert errs == [], "\n".join(errs)
        assert stats["mask_undetermined"] == 0 and stats["mask_ill_differs"] == 0, stats
        assert flags == 0, flags
        _, got0, flags0 = _gpu(g, _passes(p, 1), None, groups=False, layout=layout)
        assert flags0 == 0
        _bit_equal(got, got0, layout)


def _params(meta):
    return Params(sigma0xy=meta["sigma0xy"], sigma0rz=meta["sigma0rz"], sigma0rz2=meta["sigma0rz2"],
                  endcap_boundary=meta["endcap_boundary"], chi2_cut=meta.get("chi2_cut", 2.0),
                  cluster_chi2=meta.get("chi2", 1000.0), cluster_kl=meta.get("kl", 100.0))


def five_slot_ties():
    """the tie fixture with one key that takes no part in the tie removed from every tied
    6-slot receiver (its dict entry cleared and its sender cut from the graph): tied receivers
    of 5 slots. Returns (graph, their node ids, meta)."""
    g, _, extra, meta = load("cluster_tie")
    p = _params(meta)
    deg = np.diff(g.slot_ptr)
    tied = np.nonzero(np.isin(g.node["node_id"], extra["tie_nodes"]) & (deg == 6))[0]
    keep = np.ones(g.n_nodes, bool)
    want = []
    for v in tied:
        order, D = _tse_distances(g, v, p)
        if len(order) != 6 or not _tied(D):
            continue
        nz = D[np.nonzero(D)]
        rows, cols = np.where(D == nz.min())
        free = [k for i, k in enumerate(order) if i not in set(rows.tolist() + cols.tolist())]
        free = [k for k in free if g.slot["slot_src"][k] >= 0 and g.slot["slot_src"][k] not in tied]
        if not free:
            continue
        k = free[-1]
        g.slot["tse_rank"][k] = -1
        g.slot["uts_rank"][k] = -1
        keep[g.slot["slot_src"][k]] = False
        want.append(int(g.node["node_id"][v]))
    keep[tied] = True
    return graph.subset(g, keep), np.array(want), meta


def test_five_slot_ties_bit_exact():
    g, ids, meta = five_slot_ties()
    p = _params(meta)
    deg = np.diff(g.slot_ptr)
    five = np.nonzero(np.isin(g.node["node_id"], ids) & (deg == 5))[0]
    five = [v for v in five if _tied(_tse_distances(g, v, p)[1])]
    assert len(five) >= 5, len(five)
    exp = g.copy()
    assert cpu_ref.cluster(exp, "tse", meta["chi2"], meta["kl"], p, 2) == 0
    assert exp.node["has_merged"][five].sum() >= 3
    for classes in (False, True):
        run = lambda d: d.cluster("tse", meta["chi2"], meta["kl"], p)   # noqa: E731
        d, got, flags = _gpu(g, run, classes, layout="natural")
        assert d.cg.n_g6 >= len(five) and flags == 0
        errs = compare(got, exp, rtol=0.0, atol=0.0)
        assert errs == [], "\n".join(errs)
        _, got0, flags0 = _gpu(g, run, classes, groups=False, layout="natural")
        assert flags0 == 0
        _bit_equal(got, got0, "ties")
