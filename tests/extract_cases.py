"""Directed events for the extraction kernel (gtf_extract_candidates), shared by
test_extract_cases.py (CPU: every case reaches the branch it exists for, on the oracle
alone) and test_gpu_extract_cases.py (GPU against the oracle on the same events).

A case is a list of candidates; a candidate is a list of hits (x, y, z, volume, layer).
:func:`build` numbers the nodes candidate by candidate, chains each candidate's hits
with edges in both directions and joins candidates by deactivated edges; :func:`graph`
is the layer below it (explicit nodes, edges and deactivated directions).
"""
import functools

import numpy as np

import gtf_oracle as O
from gtf import synth
from gtf.params import Params as PassParams

CODE = {"fragment": 0, "bad": 1, "rejected": 2, "extracted": 3}


# --------------------------------------------------------------------------- builder
def graph(hits, edges, inactive=(), sub_id=None):
    """hits: [N, 5] (x, y, z, volume, layer) in node order; edges: undirected (u, v)
    pairs, stored in both directions; inactive: directed (u, v) pairs -- the slot k in
    [slot_ptr[v], slot_ptr[v+1]) with slot_src[k] == u gets act = 0; sub_id: override
    of the subgraph ids (default: the connected components of all edges).
    Returns (TrackGraph, vivl [N, 2])."""
    h = np.asarray(hits, np.float64).reshape(-1, 5)
    N = len(h)
    e = np.asarray(list(edges), np.int64).reshape(-1, 2)
    assert len(e) == 0 or (e.min() >= 0 and e.max() < N and (e[:, 0] != e[:, 1]).all())
    src = np.concatenate([e[:, 0], e[:, 1]])
    dst = np.concatenate([e[:, 1], e[:, 0]])
    x, y, z = h[:, 0].copy(), h[:, 1].copy(), h[:, 2].copy()
    r = np.sqrt(x * x + y * y)
    g = synth._assemble(N, src, dst, x, y, z, r, h[:, 4].copy(), PassParams())
    for u, v in inactive:
        lo, hi = int(g.slot_ptr[v]), int(g.slot_ptr[v + 1])
        k = lo + np.nonzero(g.slot["slot_src"][lo:hi] == u)[0]
        assert len(k) == 1, "no edge %d -> %d" % (u, v)
        g.slot["act"][k[0]] = 0
    if sub_id is not None:
        g.node["sub_id"] = np.asarray(sub_id, np.int32).copy()
        g.n_subgraphs = int(g.node["sub_id"].max()) + 1 if N else 0
    sub = g.node["sub_id"]
    assert N == 0 or (sub[0] == 0 and np.isin(np.diff(sub), (0, 1)).all()), "nodes not grouped by subgraph"
    return g, h[:, 3:5].copy()


def offsets(cands):
    """first node of every candidate (and N at the end)"""
    return np.concatenate([[0], np.cumsum([len(c) for c in cands])]).astype(np.int64)


def wire(cands, start=0, joins=(), one_way=False, cut=()):
    """edges and deactivated directions of candidates numbered from node `start` on: a
    chain inside each candidate, the joins and the cuts (see build)"""
    off = offsets(cands) + start
    edges = [(int(off[c]) + i, int(off[c]) + i + 1) for c in range(len(cands)) for i in range(len(cands[c]) - 1)]
    inactive = []
    for a, b in joins:
        u, v = int(off[a + 1] - 1), int(off[b])
        edges.append((u, v))
        inactive.append((u, v))
        if not one_way:
            inactive.append((v, u))
    for c, i in cut:
        u = int(off[c]) + i
        inactive += [(u, u + 1), (u + 1, u)]
    return edges, inactive


def build(cands, joins=(), one_way=False, sub_id=None, cut=()):
    """cands: list of hit lists. joins: pairs (a, b) of candidate indices: the last hit
    of a and the first hit of b get an edge that is deactivated (one_way: only the
    direction a -> b, the way back stays active). cut: (candidate, i) pairs: the chain
    edge between hits i and i + 1 of that candidate is deactivated in both directions.
    sub_id: per-candidate subgraph override (list, one entry per candidate)."""
    edges, inactive = wire(cands, 0, joins, one_way, cut)
    sub = None if sub_id is None else np.repeat(np.asarray(sub_id), [len(c) for c in cands])
    return graph([h for c in cands for h in c], edges, inactive, sub)


def track(seed, n=6, r0=32.0, dr=40.0, curv=2e-4, tanl=0.3, scatter=0.1, layers=None, volume=8.0, phi0=None,
          z0=0.0, radii=None):
    """n hits of a circle through the origin with curvature `curv` (1/mm) starting at
    azimuth phi0 (seeded when None), at radii r0 + i dr (or `radii`), z = z0 + tanl * arc
    length, each coordinate scattered by a seeded Gaussian of `scatter` mm. layers: the
    in-volume layer id of every hit (default 2, 4, 6, ...), or (volume, layer) pairs."""
    rng = np.random.default_rng(seed)
    rr = np.asarray(radii, np.float64) if radii is not None else r0 + dr * np.arange(n)
    n = len(rr)
    if phi0 is None:
        phi0 = rng.uniform(-np.pi, np.pi)
    half = np.arcsin(0.5 * curv * rr)
    s = 2.0 * half / curv if curv else rr
    phi = phi0 + half
    x = rr * np.cos(phi) + rng.normal(0, scatter, n)
    y = rr * np.sin(phi) + rng.normal(0, scatter, n)
    z = z0 + tanl * s + rng.normal(0, scatter, n)
    if layers is None:
        layers = 2.0 * (1 + np.arange(n))
    out = []
    for i in range(n):
        vl = layers[i] if np.ndim(layers[i]) else (volume, layers[i])
        out.append((float(x[i]), float(y[i]), float(z[i]), float(vl[0]), float(vl[1])))
    return out


def reverse(cands):
    return [list(c[::-1]) for c in cands]


def order_map(cands):
    """node of build(cands) -> node of build(reverse(cands)) holding the same hit; as an
    order_key it is the reversed rank inside each candidate"""
    off = offsets(cands)
    return np.concatenate([np.arange(off[c + 1] - 1, off[c] - 1, -1) for c in range(len(cands))]).astype(np.int32)


# --------------------------------------------------------------------------- oracle side
def extract_params(scale=1.0):
    from gtf import extract
    p = extract.Params()
    p.sigma0xy *= scale
    p.sigma0rz *= scale
    return p


def oracle(g, vivl, p):
    with np.errstate(all="ignore"):
        return O.extract_candidates(g, vivl, p.pval, p.numhits, p.separation, p.merge, p.sigma0xy, p.sigma0rz,
                                    p.endcap)


def fit_inputs(g, vivl, rec, p):
    """what the oracle fits for one candidate record, recomputed from its own helpers:
    (assessed nodes, coordinates sorted by radius, rotated coordinates, merged flag)"""
    an, ac, merged = O.check_close_proximity_nodes(rec["nodes"], vivl, g.node["xyzr"], g.node["gnn"].copy(), p.merge)
    coords = sorted([ac[v] for v in an], key=lambda c: c[3], reverse=True)
    return an, coords, O.rotate_track(coords, p.separation), merged


def pdist(a, b):
    """distance of two p-values in _pclose's metric (test_extract.py): relative error, or
    relative error in log p, whichever is smaller; 0 for two zeros"""
    a, b = np.asarray(a, float), np.asarray(b, float)
    with np.errstate(all="ignore"):
        rel = np.abs(a - b) / np.abs(b)
        rlog = np.abs(np.log(a) - np.log(b)) / np.abs(np.log(b))
        d = np.fmin(rel, rlog)
    return np.where((a == 0) & (b == 0), 0.0, d)


def ulp_noise(g, vivl, p, base=None, draws=5, frozen=()):
    """conditioning of every fit: the oracle's p-values with every coordinate (x, y, z, r)
    moved by +-1 ulp, over `draws` seeded draws, against its own unperturbed ones, in
    pdist's metric. frozen: nodes whose x, y, r stay put (bit-equal radii and a zero
    denominator are the point of those hits; one ulp would remove the case, not measure
    its conditioning). Returns {first node of the candidate: noise} for fitted candidates."""
    base = base or oracle(g, vivl, p)
    fitted = [r for r in base["records"] if r["status"] in ("rejected", "extracted")]
    noise = {int(r["nodes"][0]): 0.0 for r in fitted}
    keep = np.zeros((g.n_nodes, 4), bool)
    keep[list(frozen)] = (True, True, False, True)
    for d in range(draws):
        rng = np.random.default_rng(1000 + d)
        h = g.copy()
        c = h.node["xyzr"]
        moved = np.nextafter(c, np.where(rng.random(c.shape) < 0.5, -np.inf, np.inf))
        h.node["xyzr"] = np.where(keep, c, moved)
        h.node["gnn"] = h.node["xyzr"].copy()
        got = {int(r["nodes"][0]): r for r in oracle(h, vivl, p)["records"]}
        for r in fitted:
            k = int(r["nodes"][0])
            q = got[k]
            for key in ("pval_xy", "pval_zr"):
                if np.isnan(r[key]) and np.isnan(q[key]):
                    continue
                noise[k] = max(noise[k], float(pdist(q[key], r[key])))
    return noise


# --------------------------------------------------------------------------- set order
GRID = [(float(v), float(l)) for v in (7, 8, 9, 12, 13, 14, 16, 17, 18) for l in range(2, 15, 2)]


def grid_pairs():
    """entry k of the (volume, layer) grid paired with entry (7k + 3) mod 63: the distinct
    unordered pairs of two different tuples, in order of k"""
    seen, out = set(), []
    for k in range(len(GRID)):
        a, b = GRID[k], GRID[(7 * k + 3) % len(GRID)]
        if a != b and frozenset((a, b)) not in seen:
            seen.add(frozenset((a, b)))
            out.append((a, b))
    return out


def set_order_cands(swap=False):
    """one candidate per grid pair: hits A, B, A', B' and two clean hits; A's duplicate
    1.8 mm away (merges), B's 30 mm away (does not): the candidate ends bad either way,
    and A's GNN_Measurement keeps the midpoint exactly when set() yields A before B"""
    cands = []
    for i, (a, b) in enumerate(grid_pairs()):
        if swap:
            a, b = b, a
        t = track(100 + i, n=4, scatter=0.05, layers=[a, b, (20.0, 2.0), (20.0, 4.0)])
        a2 = (t[0][0] + 1.8, t[0][1], t[0][2]) + a
        b2 = (t[1][0], t[1][1] + 30.0, t[1][2]) + b
        cands.append([t[0], t[1], a2, b2, t[2], t[3]])
    return cands


# --------------------------------------------------------------------------- branch cases
def branch_cases():
    """name -> hits of the per-branch candidates, in event order, and the joins"""
    c = {}
    c["barrel"] = track(1, tanl=0.2, scatter=0.1)
    c["endcap"] = track(2, tanl=-2.0, z0=-700.0, scatter=0.1)
    c["mixed"] = track(3, tanl=-1.0, z0=-250.0, scatter=0.1)
    # two hits on different layers with bit-equal r: (x, y) and (y, x) across the 45 degree line
    t = track(4, n=6, scatter=0.1, phi0=np.pi / 4 - np.arcsin(0.5 * 2e-4 * 112.0))
    x, y, z = t[2][:3]
    t.insert(3, (y, x, z + 0.05, 8.0, 20.0))
    c["tie"] = t
    # the two innermost hits 3.5 mm apart: rotate_track takes the third-innermost
    c["sep"] = track(5, radii=[28.5, 32.0, 72.0, 112.0, 152.0, 192.0, 232.0], scatter=0.1)
    # two hits with identical (x, y): zero parabola denominator, NaN p-values
    t = track(6, scatter=0.1)
    t.insert(3, (t[2][0], t[2][1], t[2][2] + 7.0, 8.0, 20.0))
    c["samexy"] = t
    t = track(7, scatter=0.1)
    c["triple"] = t[:3] + [(t[2][0] + 1.0, t[2][1], t[2][2], 8.0, 6.0), (t[2][0], t[2][1] + 1.0, t[2][2], 8.0, 6.0)] + t[3:]
    t = track(8, scatter=0.1)
    c["merge1"] = t[:4] + [(t[3][0] + 1.2, t[3][1] - 1.2, t[3][2] + 0.6, 8.0, 8.0)] + t[4:]
    t = track(9, scatter=0.1)
    c["merge2"] = ([t[0], (t[0][0] - 1.0, t[0][1] + 1.0, t[0][2] + 0.5, 8.0, 2.0)] + t[1:5] +
                   [(t[4][0] + 1.3, t[4][1] + 0.4, t[4][2] - 1.0, 8.0, 10.0), t[5]])
    t = track(10, n=3, scatter=0.1)
    c["merge_short"] = t + [(t[1][0] + 1.0, t[1][1] + 1.0, t[1][2], 8.0, 4.0)]
    c["four"] = track(11, n=4, scatter=0.1)
    c["three"] = track(12, n=3, scatter=0.1)
    c["single"] = track(13, n=1)
    names = list(c)
    joins = [(names.index(a), names.index(b)) for a, b in
             (("barrel", "endcap"), ("endcap", "mixed"), ("tie", "sep"), ("merge1", "merge2"), ("four", "three"))]
    return c, joins


def branch_frozen(cases):
    """nodes of the branch event whose x, y, r the conditioning check leaves alone"""
    names = list(cases)
    off = offsets(list(cases.values()))
    return [int(off[names.index("tie")]) + 2, int(off[names.index("tie")]) + 3,
            int(off[names.index("samexy")]) + 2, int(off[names.index("samexy")]) + 3]


# --------------------------------------------------------------------------- p-value regimes
REGIME_HITS = (4, 5, 6, 8, 12, 20, 40)
REGIME_SCATTER = (0.1, 0.3, 3.0, 30.0)
REGIME_SCALES = (0.3, 1.0, 3.0, 10.0)


def regime_cands():
    out = []
    for n in REGIME_HITS:
        for j, sc in enumerate(REGIME_SCATTER):
            out.append(track(1000 * n + j, n=n, scatter=sc, tanl=0.3))
    return out


@functools.lru_cache(maxsize=None)
def regime_admission(scale):
    """the regime event at sigma0 x scale: (oracle result, {first node: (xy admitted, zr
    admitted)}, {first node: +-1 ulp noise}). A p-value is admitted for the GPU comparison
    when its candidate's noise is <= 1e-8, it is not a subnormal-range value in (0, 1e-290),
    and, if it is 0, its chi2 / 2 is beyond 800 (far past cephes' MAXLOG = 709.78, where
    every igamc gives exactly 0)."""
    g, vivl = cached("regimes")
    p = extract_params(scale)
    o = oracle(g, vivl, p)
    noise = ulp_noise(g, vivl, p, o)
    adm = {}
    for r in o["records"]:
        k = int(r["nodes"][0])
        adm[k] = tuple(noise[k] <= 1e-8 and not 0 < r[key] < 1e-290 and (r[key] > 0 or r[c2] / 2 > 800)
                       for key, c2 in (("pval_xy", "chi2_xy"), ("pval_zr", "chi2_zr")))
    return o, adm, noise


# --------------------------------------------------------------------------- components
def components_event(seed=5):
    """one subgraph of 2048 + 900 + 1023 nodes numbered by a seeded permutation: a path, a
    star and a binary tree, chained by two deactivated edges (three components), every
    hit on one layer (bad after the O(n^2) scan); then the small connectivity subgraphs.
    Returns (g, vivl, number of nodes of the big subgraph)."""
    rng = np.random.default_rng(seed)
    n_path, n_star, n_tree = 2048, 900, 1023
    M = n_path + n_star + n_tree
    perm = rng.permutation(M)
    e = [(i, i + 1) for i in range(n_path - 1)]
    s0 = n_path
    e += [(s0, s0 + i) for i in range(1, n_star)]
    t0 = n_path + n_star
    e += [(t0 + (i - 1) // 2, t0 + i) for i in range(1, n_tree)]
    dead = [(n_path - 1, s0), (s0 + n_star - 1, t0)]
    e += dead
    phi = rng.uniform(-np.pi, np.pi, M)
    zz = rng.uniform(-400, 400, M)
    hits = [(100.0 * np.cos(phi[i]), 100.0 * np.sin(phi[i]), zz[i], 8.0, 2.0) for i in range(M)]
    big_hits = [None] * M
    for i in range(M):
        big_hits[perm[i]] = hits[i]
    edges = [(int(perm[u]), int(perm[v])) for u, v in e]
    inactive = [(int(perm[u]), int(perm[v])) for u, v in dead] + [(int(perm[v]), int(perm[u])) for u, v in dead]
    sub = [0] * M

    def add(cands, sub_id, **kw):
        e2, dead2 = wire(cands, len(big_hits), **kw)
        edges.extend(e2)
        inactive.extend(dead2)
        for hs in cands:
            big_hits.extend(hs)
            sub.extend([sub_id] * len(hs))

    lay = lambda a: [2.0 * (a + i) for i in range(5)]     # noqa: E731
    # an edge active in one direction only joins its two chains and marks the subgraph as
    # split: the third, disjoint chain of the subgraph is a candidate of its own
    add([track(21, n=5, layers=lay(1)), track(21, n=5, r0=232.0, layers=lay(6)), track(22, n=5)], 1,
        joins=[(0, 1)], one_way=True)
    # two disjoint chains, no deactivated edge: one candidate
    add([track(23, n=5, layers=lay(1)), track(23, n=5, r0=232.0, layers=lay(6))], 2)
    # the same with one chain edge deactivated: a 2-hit and a 3-hit fragment and the other chain
    add([track(23, n=5, layers=lay(1)), track(23, n=5, r0=232.0, layers=lay(6))], 3, cut=[(0, 1)])
    g, vivl = graph(big_hits, edges, inactive, sub)
    return g, vivl, M


@functools.lru_cache(maxsize=None)
def cached(name):
    """the shared, unchanged events: name -> (g, vivl, ...)"""
    if name == "branch":
        cases, joins = branch_cases()
        return build(list(cases.values()), joins) + (cases,)
    if name == "regimes":
        return build(regime_cands())
    if name == "components":
        return components_event()
    raise KeyError(name)
