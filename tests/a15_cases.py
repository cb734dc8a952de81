"""Directed components for the distances between updated track states (a15, csrc/gtf_a15.hip),
shared by tests/golden/make_golden_a15_cases.py (the reference's own mahalanobis_distance on every
pair of every visited node), test_a15_cases.py (CPU: the oracle against that record, and that every
case reaches its branch) and test_gpu_a15_cases.py (GPU against the oracle and the record).

A case is one star in the reference's schema: a node "v" with in-neighbours, its
``updated_track_states`` dict written by hand (well-conditioned states: these are inputs of a15),
``activated`` on the edges, ``xyzr`` and ``truth_particle`` on the nodes. ``Case.claim`` says which
branch it is there for and ``Case.check(info)`` asserts it on the oracle's output.
``Case.hold`` lists what the conditioning check keeps of the inputs that sit ON a comparison, as
("freeze" | "tie", node indices in the star (0: "v", 1..: the neighbours as made), columns of
x y z r): a frozen coordinate stays (|x| == 600), tied ones move by one common factor per column
(two coordinates that must stay equal); every other coordinate of every node moves on its own.

:func:`expected` is the oracle's pair loop with the reference's exceptions kept per pair: a pair
whose C_i + C_j is exactly singular (np.linalg.inv raises, :37) gets NaN in all four columns and is
listed; the device must leave a non-finite chi2 there and nowhere else.
"""
import dataclasses
import functools
import math

import networkx as nx
import numpy as np

import gtf_oracle as O
from gtf import graph

F = np.float64
X600 = 600.0
BELOW = float(np.nextafter(600.0, 0.0))
COLS = ("chi2", "avg_tau", "avg_theta", "delta_theta")
ERR_PAIR_COUNT, ERR_NEIGHBOUR_MISSING, ERR_TOO_MANY_STATES = 256, 512, 1024
BIG_CAP = 2048


class Meas:
    def __init__(self, x, y, z, r, node):
        self.x, self.y, self.z, self.r, self.node = x, y, z, r, node


def state(i):
    """the i-th hand-made state: (a, b), a 2x2 block with c01 == c10 and a positive determinant"""
    a, b = 1e-3 * (1.0 + 0.37 * (i % 11)) * (-1.0) ** i, 0.05 + 0.013 * (i % 17) - 0.004 * (i % 5)
    c00, c11 = 1e-6 * (1.0 + 0.25 * (i % 7)), 1e-3 * (1.0 + 0.2 * (i % 3))
    c01 = 0.3 * math.sqrt(c00 * c11) * (1.0 if i % 2 else -1.0)
    return (a, b), (c00, c01, c01, c11)


def entry(ab, blk, xyzr, tau=0.3):
    cov = np.array([[blk[0], blk[1], 0.0], [blk[2], blk[3], 0.0], [0.0, 0.0, 1e-3]])
    return {"xyzr": tuple(F(c) for c in xyzr), "edge_state_vector": np.array([ab[0], ab[1], 0.0]),
            "edge_covariance": cov, "joint_vector": [F(ab[0]), F(ab[1]), F(tau)], "joint_vector_covariance": cov,
            "likelihood": F(1.0), "mixture_weight": F(1.0), "prior": F(1.0)}


def nb_xyz(i, n=1):
    """the i-th neighbour of a star at V0: dr = 40 + i step, dz = 10 + 6 i step; tau rises with i"""
    step = 1.0 if n <= 130 else 0.1
    r, z = 300.0 + 40.0 + 0.5 * step * i, 100.0 + 10.0 + 3.0 * step * i
    phi = 0.30 + 0.01 * math.sin(i)
    return (r * math.cos(phi), r * math.sin(phi), z, r)


V0 = (300.0 * math.cos(0.30), 300.0 * math.sin(0.30), 100.0, 300.0)


class Star:
    """node "v" (id base) and its in-neighbours (ids base + 1 ..), in the reference's schema"""

    def __init__(self, base, v=V0, has_uts=True, truth=7):
        self.G = nx.DiGraph()
        self.base = base
        self.v = base
        self._node(base, v, truth)
        if has_uts:
            self.G.nodes[base]["updated_track_states"] = {}
        self.keys = []
        self.made = 0

    def _node(self, n, xyzr, truth):
        x, y, z, r = (F(c) for c in xyzr)
        self.G.add_node(n, GNN_Measurement=Meas(x, y, z, r, n), xyzr=(x, y, z, r), truth_particle=int(truth))

    def nb(self, xyzr=None, edge=True, act=1, key=True, st=None, truth=7, orphan=False):
        i = self.made
        self.made += 1
        n = self.base + 1 + i
        if not orphan:
            self._node(n, nb_xyz(i) if xyzr is None else xyzr, truth)
            if edge:
                self.G.add_edge(n, self.v, activated=act)
        if key:
            self.keys.append((n, st if st is not None else state(i)))
        return n

    def finish(self, order=None):
        """the dict in the order `order` (a permutation of the keys' indices; default: as made)"""
        keys = self.keys if order is None else [self.keys[i] for i in order]
        if keys or "updated_track_states" in self.G.nodes[self.v]:
            d = self.G.nodes[self.v].setdefault("updated_track_states", {})
            for n, (ab, blk) in keys:
                d[n] = entry(ab, blk, self.G.nodes[n]["xyzr"] if n in self.G else (0.0, 0.0, 0.0, 0.0))
        return self.G


@dataclasses.dataclass
class Case:
    name: str
    build: object          # build(base) -> nx.DiGraph
    claim: str
    check: object          # check(info)
    hold: tuple = ()
    copies: int = 1        # instances in everything() (the 2- and 4-lane groups need more than a block)
    err: int = 0           # the error bit the case raises (it is then run in a call of its own group)
    sparse: bool = False   # ranks made sparse (3 r + 1) after packing
    singular: int = 0      # pairs whose C_i + C_j is singular


CASES = []


def case(name, build, claim, check, **kw):
    CASES.append(Case(name, build, claim, check, **kw))


def pairs_of(info, name="v"):
    v = info["v"]
    return int(info["ptr"][v + 1] - info["ptr"][v])


def _npairs(n):
    return lambda info: np.testing.assert_equal(pairs_of(info), n)


# ---- the visit rule (:139-143)
def _visit(has_uts, n_active, n_keys=3, keyless_active=0, inactive_keys=0):
    def build(base):
        s = Star(base, has_uts=has_uts)
        for i in range(n_keys):
            s.nb(act=1 if i < n_active else 0, key=has_uts)
        for _ in range(keyless_active):
            s.nb(act=1, key=False)
        for _ in range(inactive_keys):
            s.nb(act=0, key=True)
        return s.finish()
    return build


case("no_uts_dict", _visit(False, 2), "has_uts == 0 with two active in-edges: not visited", _npairs(0))
case("active_0", _visit(True, 0), "a dict of 3 keys and no active in-edge: not visited", _npairs(0))
case("active_1", _visit(True, 1), "a dict of 3 keys and one active in-edge: nact > 1 fails", _npairs(0))
case("active_2", _visit(True, 2), "a dict of 3 keys and two active in-edges: visited, all 3 pairs", _npairs(3))
case("keys_on_inactive_edges", _visit(True, 0, n_keys=0, keyless_active=2, inactive_keys=3),
     "the active edges carry no key and the keys' edges are inactive: visited, pairs among the keys", _npairs(3))
case("visited_d0", _visit(True, 0, n_keys=0, keyless_active=2), "visited with an empty dict", _npairs(0))
case("visited_d1", _visit(True, 0, n_keys=0, keyless_active=2, inactive_keys=1), "visited with one key", _npairs(0))


# ---- pair order: dict order against slot order
def shuffled(d):
    """a dict order that is neither the slot order nor its reverse (from 3 keys on)"""
    if d < 8:
        return list(range(d // 2, d)) + list(range(d // 2))
    return [(i * 7 + 3) % d for i in range(d)] if d % 7 else [(i * 5 + 3) % d for i in range(d)]


def _order(d, extra_slots=0):
    def build(base):
        s = Star(base)
        for i in range(d):
            s.nb()
        for _ in range(extra_slots):
            s.nb(key=False)
        return s.finish(order=shuffled(d))
    return build


def _order_check(d, slots=None):
    def check(info):
        g, v = info["g"], info["v"]
        lo, hi = int(g.slot_ptr[v]), int(g.slot_ptr[v + 1])
        assert hi - lo == (d if slots is None else slots) and pairs_of(info) == d * (d - 1) // 2
        rk = g.slot["uts_rank"][lo:hi]
        if d > 2:
            assert not np.array_equal(rk[rk >= 0], np.sort(rk[rk >= 0]))     # dict order is not slot order
        # theta rises with the slot index: delta_theta's sign tells which of a pair came first
        dt = info["cols"]["delta_theta"][info["ptr"][v]:info["ptr"][v + 1]]
        assert (dt != 0).all() and ((dt > 0).any() and (dt < 0).any() if d > 2 else True)
    return check


for d in (2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 130):
    case("order_%d" % d, _order(d), "%d keys, all pairs, the dict in another order than the slots%s" % (
        d, "; the wave path and its position -> slot map" if d > 64 else ""), _order_check(d),
        sparse=d in (5, 17, 65), copies={2: 130, 3: 33, 4: 34}.get(d, 1))
case("keys_3_slots_9", _order(3, extra_slots=6), "fewer keys than slots: the group width comes from the slot count",
     _order_check(3, slots=9))
case("keys_3_slots_70", _order(3, extra_slots=67), "3 keys in a 70-slot node: the wave path with few keys",
     _order_check(3, slots=70))


# ---- the 600 test (:66-74), on x, independently for the node and both neighbours
def _x600(vx, bx, cx):
    def build(base):
        s = Star(base, v=(vx, 80.0, 100.0, 620.0))
        s.nb(xyzr=(bx, 90.0, 130.0, 660.0))
        s.nb(xyzr=(cx, 70.0, 190.0, 700.0))
        return s.finish()
    return build


def _x600_check(flags):
    def check(info):
        g, v = info["g"], info["v"]
        lo = int(g.slot_ptr[v])
        xs = [g.node["xyzr"][v][0]] + [g.node["xyzr"][g.slot["slot_src"][lo + i]][0] for i in (0, 1)]
        assert [bool(abs(x) >= 600.0) for x in xs] == list(flags)
        assert all(abs(x) in (X600, BELOW) for x in xs) and pairs_of(info) == 1
    return check


for m in range(8):
    fl = (bool(m & 1), bool(m & 2), bool(m & 4))
    for sg, stag in ((1.0, "p"), (-1.0, "m")):
        xs = [sg * (X600 if f else BELOW) for f in fl]
        case("x600_%d%d%d_%s" % (fl + (stag,)), _x600(*xs),
             "|x| %s 600 for node / neighbour 1 / neighbour 2 at %sx" % (
                 "/".join("==" if f else "one ulp below" for f in fl), "+" if sg > 0 else "-"),
             _x600_check(fl), hold=(("freeze", (0, 1, 2), (0,)),))


# ---- arithmetic
def _two(st0=None, st1=None, xyz0=None, xyz1=None):
    def build(base):
        s = Star(base)
        s.nb(st=st0, xyzr=xyz0)
        s.nb(st=st1, xyzr=xyz1)
        s.nb()               # a clean third key: two clean pairs beside the special one
        return s.finish()
    return build


def _pair(info, t=0):
    return {c: info["cols"][c][info["ptr"][info["v"]] + t] for c in COLS}


case("c01_ne_c10", _two(st0=((1e-3, 0.06), (1e-6, 9e-6, -4e-6, 1e-3))),
     "a stored block with c01 != c10", lambda info: np.testing.assert_equal(np.isfinite(_pair(info)["chi2"]), True))
case("equal_states", _two(st0=state(4), st1=state(4)), "two identical states: chi2 is the tau term alone",
     lambda info: np.testing.assert_array_less(0.0, _pair(info)["chi2"]))
case("equal_coordinates", _two(xyz0=nb_xyz(5), xyz1=nb_xyz(5)),
     "two neighbours with identical coordinates: delta tau and delta theta are zero",
     lambda info: np.testing.assert_equal((_pair(info)["delta_theta"], np.isfinite(_pair(info)["chi2"])), (0.0, True)), hold=(("tie", (1, 2), (0, 1, 2, 3)),))
case("rb_equals_ra", _two(xyz0=(310.0 * math.cos(0.31), 310.0 * math.sin(0.31), 150.0, 300.0)),
     "r_b == r_a: tau_1 is infinite (kinds)",
     lambda info: np.testing.assert_equal(np.isinf(_pair(info)["avg_tau"]) and not np.isfinite(_pair(info)["chi2"]), True), hold=(("tie", (0, 1), (3,)),))
ONES = (1.0, 1.0, 1.0, 1.0)
case("singular_sum", _two(st0=((1e-3, 0.05), ONES), st1=((2e-3, 0.07), ONES)),
     "C_i + C_j exactly singular: the reference's inv raises (:37); non-finite chi2 for that pair and no other",
     lambda info: np.testing.assert_equal((info["singular"], bool(np.isfinite(info["cols"]["chi2"][info["ptr"][info["v"]] + 1:
                                                                               info["ptr"][info["v"] + 1]]).all())),
                                          ([int(info["ptr"][info["v"]])], True)), singular=1)


# ---- truth (:190-193)
def _truth(tv, t0, t1):
    def build(base):
        s = Star(base, truth=tv)
        s.nb(truth=t0)
        s.nb(truth=t1)
        return s.finish()
    return build


def _truth_is(want):
    return lambda info: np.testing.assert_equal(int(info["cols"]["truth"][info["ptr"][info["v"]]]), want)


BIGID = 3 * 2 ** 32 + 11
case("truth_equal", _truth(5, 5, 5), "node and both neighbours share a particle", _truth_is(1))
case("truth_node_differs", _truth(6, 5, 5), "the node differs", _truth_is(0))
case("truth_nb1_differs", _truth(5, 6, 5), "neighbour 1 differs", _truth_is(0))
case("truth_nb2_differs", _truth(5, 5, 6), "neighbour 2 differs", _truth_is(0))
case("truth_beyond_int32_equal", _truth(BIGID, BIGID, BIGID), "ids beyond int32, equal", _truth_is(1))
case("truth_equal_modulo_2_32", _truth(BIGID, BIGID + 2 ** 32, BIGID), "ids equal modulo 2^32 only", _truth_is(0))


# ---- error bits, in a group-path node and in a wave-path node
def _orphan(d):
    def build(base):
        s = Star(base)
        for i in range(d):
            s.nb(orphan=(i == d // 2), edge=True)
        return s.finish()
    return build


def _orphan_check(info):
    g, v = info["g"], info["v"]
    assert (g.slot["slot_src"][g.slot_ptr[v]:g.slot_ptr[v + 1]] < 0).sum() == 1 and info["raised"] == [v]


case("orphan_key_group", _orphan(4), "a present key with slot_src = -1 (KeyError :182-183), group path", _orphan_check,
     err=ERR_NEIGHBOUR_MISSING)
case("orphan_key_wave", _orphan(66), "a present key with slot_src = -1, wave path", _orphan_check, err=ERR_NEIGHBOUR_MISSING)

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# --------------------------------------------------------------------------- building and the oracle
@functools.lru_cache(maxsize=None)
def _everything(errs):
    subs, comps = [], []
    base = 0
    for c in CASES:
        if bool(c.err) != errs and not (errs and c.name in ("order_5", "order_65", "active_2")):
            continue
        for i in range(c.copies if not errs else 1):
            G = c.build(base)
            subs.append(G)
            comps.append(dict(case=c, v=None, base=base))
            base += 4096
    g = graph.pack(subs)
    n0 = 0
    for c, G in zip(comps, subs):
        c["v"] = n0
        c["nodes"] = (n0, n0 + G.number_of_nodes())
        if c["case"].sparse:
            lo, hi = int(g.slot_ptr[n0]), int(g.slot_ptr[n0 + 1])
            rk = g.slot["uts_rank"][lo:hi]
            rk[rk >= 0] = rk[rk >= 0] * 3 + 1
        n0 += G.number_of_nodes()
    truth = np.concatenate([[G.nodes[n]["truth_particle"] for n in G.nodes] for G in subs]).astype(np.int64)
    return g, comps, truth


def everything(errs=False):
    """(graph, components, node truth): errs=False: every clean case (with its copies) in one graph;
    errs=True: the cases that raise an error bit, beside three clean ones that must stay exact"""
    return _everything(bool(errs))


def expected(g, truth=None):
    """the oracle's pair loop (O.updated_state_pairs' rule and order, O.mahalanobis_distance_updated
    per pair) with the reference's exceptions kept apart: returns (pair_ptr, columns, pair indices
    whose inv raised (NaN rows), nodes whose pair loop raises KeyError (no rows compared))"""
    S, sp = g.slot, g.slot_ptr
    ptr = np.zeros(g.n_nodes + 1, np.int64)
    rows, sing, raised = [], [], []
    for v in range(g.n_nodes):
        lo, hi = int(sp[v]), int(sp[v + 1])
        nact = int(np.sum((S["is_edge"][lo:hi] == 1) & (S["act"][lo:hi] == 1)))
        if g.node["has_uts"][v] == 1 and nact > 1:
            keys = O._dict_order(g, "uts", v)
            bad = any(S["slot_src"][k] < 0 for k in keys) and len(keys) >= 2
            if bad:
                raised.append(v)
            for i in range(len(keys)):
                for j in range(i):
                    ki, kj = keys[i], keys[j]
                    ui, uj = S["slot_src"][ki], S["slot_src"][kj]
                    if bad:
                        rows.append((np.nan,) * 4 + (0,))
                        continue
                    mi = np.array([S["uts_sv"][ki][0], S["uts_sv"][ki][1], S["uts_tau"][ki]])
                    mj = np.array([S["uts_sv"][kj][0], S["uts_sv"][kj][1], S["uts_tau"][kj]])
                    try:
                        with np.errstate(all="ignore"):
                            r = O.mahalanobis_distance_updated(mi, O.mat_from_cov5(S["uts_cov"][ki]), mj,
                                                               O.mat_from_cov5(S["uts_cov"][kj]), g.node["xyzr"][v],
                                                               g.node["xyzr"][ui], g.node["xyzr"][uj])
                    except np.linalg.LinAlgError:
                        sing.append(len(rows))
                        r = (np.nan,) * 4
                    t = 0 if truth is None else int(truth[v] == truth[ui] and truth[ui] == truth[uj] and truth[v] == truth[uj])
                    rows.append(tuple(r) + (t,))
        ptr[v + 1] = len(rows)
    a = np.array(rows, dtype=np.float64).reshape(-1, 5)
    cols = {c: a[:, i].copy() for i, c in enumerate(COLS)}
    cols["truth"] = a[:, 4].astype(np.int8)
    return ptr, cols, sing, raised


def info_of(case):
    G = case.build(0)
    g = graph.pack([G])
    truth = np.array([G.nodes[n]["truth_particle"] for n in G.nodes], np.int64)
    ptr, cols, sing, raised = expected(g, truth)
    return dict(g=g, v=0, ptr=ptr, cols=cols, singular=sing, raised=raised, truth=truth)


def perturbed(g, comps, seed):
    """g with every xyzr coordinate moved by +-2^-46 relative, each on its own, but for the components'
    Case.hold: frozen coordinates stay, tied ones share one factor per column"""
    rng = np.random.default_rng(seed)
    h = g.copy()
    f = 1.0 + rng.choice([-1.0, 1.0], size=h.node["xyzr"].shape) * 2.0 ** -46
    for c in comps:
        for how, who, cols in c["case"].hold:
            rows = [c["nodes"][0] + i for i in who]
            for col in cols:
                f[rows, col] = 1.0 if how == "freeze" else f[rows[0], col]
    h.node["xyzr"] = h.node["xyzr"] * f
    return h


def big_star(d, beside=()):
    """one node with d keys on active edges (d = 2048: the most the wave path takes; 2049: refused),
    and after it the clean cases named in `beside`, one star each, in the same graph"""
    s = Star(0)
    for i in range(d):
        s.nb(xyzr=nb_xyz(i, d))
    subs = [s.finish(order=shuffled(d))] + [BY_NAME[n].build(4096 * (k + 1)) for k, n in enumerate(beside)]
    return graph.pack(subs)


def pair_of(g, v, t, truth=None):
    """the oracle's columns of pair t (= i (i - 1) / 2 + j) of node v alone"""
    keys = O._dict_order(g, "uts", v)
    i = int((1 + math.isqrt(1 + 8 * t)) // 2)
    j = t - i * (i - 1) // 2
    S = g.slot
    ki, kj = keys[i], keys[j]
    ui, uj = S["slot_src"][ki], S["slot_src"][kj]
    mi = np.array([S["uts_sv"][ki][0], S["uts_sv"][ki][1], S["uts_tau"][ki]])
    mj = np.array([S["uts_sv"][kj][0], S["uts_sv"][kj][1], S["uts_tau"][kj]])
    return O.mahalanobis_distance_updated(mi, O.mat_from_cov5(S["uts_cov"][ki]), mj, O.mat_from_cov5(S["uts_cov"][kj]),
                                          g.node["xyzr"][v], g.node["xyzr"][ui], g.node["xyzr"][uj])
