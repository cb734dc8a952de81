"""Directed components for the initial track-state estimates (a2, csrc/gtf_tse.hip), shared by
tests/golden/make_golden_tse_cases.py (the reference's own helper.compute_track_state_estimates on
every case), test_tse_cases.py (CPU: the oracle against that record, and that every case reaches
the branch it is there for) and test_gpu_tse_cases.py (GPU against the oracle and the record).

A case is one weakly connected component in the reference's schema: a networkx DiGraph whose nodes
carry a ``GNN_Measurement`` with numpy float64 coordinates (as helper.py:486 makes them, so that a
zero divisor gives inf / NaN and no ZeroDivisionError). The dict order of a node's
track_state_estimates is the reference's: reversed(set(nx.all_neighbors)), computed by CPython at
build time from the case's own node ids and stored as placeholder dicts, from which gtf.graph.pack
takes ``tse_rank``. Ids are spread over 4096 values so that the set order is not ascending.

``Case.claim`` says which branch the case is there for and ``Case.check(info)`` asserts, on the
oracle's output, that it got there. ``Case.hold`` lists what the conditioning
check must keep of the inputs that sit ON a comparison: ("freeze", names, columns) leaves those
coordinates of those nodes alone (|z| at the endcap boundary), ("tie", names, columns) moves them by
one common factor per column (two coordinates that must stay equal). Every other coordinate of every
node, the other coordinates of these nodes included, is perturbed on its own. ``Case.ref`` is None for a case pinned to the
reference, else the reason it stays oracle-only (``Case.post`` then edits the packed graph: absent
keys and rank patterns that the reference's dicts cannot hold).

:func:`everything` packs all cases into one graph, adds for every case whose node "v" has at most 8
slots the variants in which "v" is padded with absent-key slots into the 16-, 32-, 64-lane and > 64-slot buckets
(the padding: in-edges without a dict key from nodes of their own; the record of the unpadded case
stays the expectation of the case's own nodes), and fills every bucket of the schedule to one node
more than a whole number of blocks, so that the last block of each is partial.
"""
import dataclasses
import functools
import math

import networkx as nx
import numpy as np

import gtf_oracle as O
from gtf import graph
from gtf.params import Params

P = Params()
EB = float(P.endcap_boundary)
F = np.float64
BELOW = float(np.nextafter(EB, 0.0))
GROUPS_PER_BLOCK = {8: 32, 16: 16, 32: 8, 64: 4, 65: 4}   # gtf_tse.hip: BLOCK 256 over the group width
PAD_SLOTS = (16, 32, 64, 65)


class Meas:
    """the attributes of the reference's GNN_Measurement that the stage reads"""

    def __init__(self, x, y, z, r, node):
        self.x, self.y, self.z, self.r, self.node = x, y, z, r, node


def _id(base, k):
    return base + 1 + (k * 7919) % 4096


class Net:
    """one component under construction; the k-th node made gets the id base + 1 + 7919 k mod 4096"""

    def __init__(self, base):
        self.G = nx.DiGraph()
        self.base = base
        self.names = {}
        self.pads = []

    def node(self, name, x, y, z, r=None):
        n = _id(self.base, self.G.number_of_nodes())
        x, y, z = F(x), F(y), F(z)
        r = np.sqrt(x * x + y * y) if r is None else F(r)
        self.G.add_node(n, GNN_Measurement=Meas(x, y, z, r, n))
        self.names[name] = n
        return n

    def polar(self, name, r, phi, z):
        return self.node(name, r * math.cos(phi), r * math.sin(phi), z, r)

    def move(self, name, x, y, z, r=None):
        n = self.names[name]
        x, y, z = F(x), F(y), F(z)
        r = np.sqrt(x * x + y * y) if r is None else F(r)
        self.G.nodes[n]["GNN_Measurement"] = Meas(x, y, z, r, n)

    def edge(self, a, b, kind=2):
        """kind 0: a -> b, 1: b -> a, 2: both"""
        a, b = self.names[a], self.names[b]
        if kind in (0, 2):
            self.G.add_edge(a, b)
        if kind in (1, 2):
            self.G.add_edge(b, a)

    def dict_order(self, name):
        """the keys of the node's track_state_estimates in dict order (helper.py:280, :350-374)"""
        n = self.names[name]
        return list(reversed(list(set(nx.all_neighbors(self.G, n)))))

    def name_of(self, n):
        return next(k for k, v in self.names.items() if v == n)

    def finish(self):
        for n in self.G.nodes:
            order = list(reversed(list(set(nx.all_neighbors(self.G, n)))))
            self.G.nodes[n]["track_state_estimates"] = {k: {} for k in order}
        return self

    def pad(self, name, slots):
        """after finish(): bring the node to `slots` slots with in-edges that carry no dict key"""
        v = self.names[name]
        m = self.G.nodes[v]["GNN_Measurement"]
        have = len(set(self.G.predecessors(v)) | set(self.G.nodes[v]["track_state_estimates"]))
        phi = math.atan2(m.y, m.x)
        for i in range(slots - have):
            r = float(m.r) + 41.0 + 0.5 * i
            n = _id(self.base, self.G.number_of_nodes())
            x, y = F(r * math.cos(phi + 0.04 + 0.001 * i)), F(r * math.sin(phi + 0.04 + 0.001 * i))
            self.G.add_node(n, GNN_Measurement=Meas(x, y, F(m.z + 33.0 + i), F(r), n), track_state_estimates={})
            self.G.add_edge(n, v)
            self.pads.append(n)
        return self


@dataclasses.dataclass
class Case:
    name: str
    build: object                 # build(net): fills the component, names its nodes ("v": the node the case is about)
    claim: str
    check: object = None          # check(info): asserts the claim on the oracle's output of the case
    hold: tuple = ()              # ("freeze" | "tie", node names, columns of x y z r = 0 1 2 3) entries
    ref: object = None            # None: pinned to the reference; else the reason it stays oracle-only
    post: object = None           # post(g, lo, hi): edits tse_rank of v's slots [lo, hi) of the packed graph
    raises: tuple = ()            # names of the nodes that hold a singular key
    keys: int = 0                 # keys of "v" (hub cases)


# --------------------------------------------------------------------------- geometry
V0 = (300.0, 0.30, 100.0)   # the hub of the clean cases: r, phi, z


def clean_nb(i):
    """the i-th neighbour of a clean hub: |dr| >= 20, |dz| >= 15, |dphi| >= 0.01, all in the barrel"""
    s = 1.0 if i % 2 == 0 else -1.0
    t = 1.0 if (i // 2) % 2 == 0 else -1.0
    return (300.0 + s * (20.0 + i), 0.30 + t * (0.011 + 0.0007 * i), 100.0 + s * t * (15.0 + 1.3 * i))


def hub(n, v=V0, special=None):
    """build(net) of a hub "v" with n neighbours "n0".. in-only, out-only and both in turn;
    special(net): moves nodes afterwards"""
    def build(net):
        net.polar("v", *v)
        for i in range(n):
            net.polar("n%d" % i, *clean_nb(i))
            net.edge("n%d" % i, "v", i % 3)
        if special:
            special(net)
    return build


def pair(v, nb, w=None):
    """build(net) of "v" at cartesian/explicit coordinates with the neighbour "nb" and a clean "w";
    v, nb, w: (x, y, z) or (x, y, z, r)"""
    def build(net):
        net.node("v", *v)
        net.node("nb", *nb)
        net.edge("nb", "v", 2)
        if w is not None:
            net.node("w", *w)
            net.edge("v", "w", 0)
    return build


def pol(r, phi, z):
    return (r * math.cos(phi), r * math.sin(phi), z, r)


W0 = pol(340.0, 0.33, 160.0)
W_EC = pol(340.0, 0.33, 760.0)


def slot_of(info, node, key):
    g = info["g"]
    v = info["ix"][node]
    lo, hi = int(g.slot_ptr[v]), int(g.slot_ptr[v + 1])
    k = lo + int(np.nonzero(g.slot["slot_key"][lo:hi] == info["names"][key])[0][0])
    return v, k


def val(info, field, node="v", key="nb"):
    return info["out"].slot[field][slot_of(info, node, key)[1]]


def partner(info, node, key):
    """the key whose tau / del_tau / theta the reference stores at `key` (dict position n - 1 - i)"""
    g = info["g"]
    v, k = slot_of(info, node, key)
    lo, hi = int(g.slot_ptr[v]), int(g.slot_ptr[v + 1])
    rk = g.slot["tse_rank"][lo:hi]
    ks = [lo + int(j) for j in np.argsort(rk, kind="stable") if rk[j] >= 0]
    return ks[len(ks) - 1 - ks.index(k)]


CASES = []


def case(name, build, claim, **kw):
    CASES.append(Case(name, build, claim, **kw))


# ---- endcap tests: node x neighbour in barrel / endcap
def _sig(info, node_ec, nb_ec):
    """del_tau of the key that carries nb's zr terms is the J S2 J^T of exactly these sigmas"""
    g = info["g"]
    v, k = slot_of(info, "v", "nb")
    kp = partner(info, "v", "nb")      # the key at which nb's zr terms are stored is nb's partner ...
    x1 = g.node["gnn"][v]
    x2 = g.node["gnn"][g.slot["slot_src"][k]]
    sz, sr = (P.sigma0rz, P.sigma0rz2) if node_ec else (P.sigma0rz2, P.sigma0rz)
    szn, srn = (P.sigma0rz, P.sigma0rz2) if nb_ec else (P.sigma0rz2, P.sigma0rz)
    dr, dz = x1[3] - x2[3], x1[2] - x2[2]
    want = (sz ** 2 + szn ** 2) / dr ** 2 + (sr ** 2 + srn ** 2) * dz ** 2 / dr ** 4
    got = info["out"].slot["tse_cov"][kp][4] - info["out"].slot["tse_var_ms"][kp]
    assert abs(math.sqrt(got) - want) <= 1e-6 * want and P.sigma0rz != P.sigma0rz2, (got, want)


for vz, nz, tag in ((100.0, 200.0, "bb"), (100.0, 800.0, "be"), (700.0, 200.0, "eb"), (700.0, 800.0, "ee")):
    case("ec_" + tag, pair(pol(300.0, 0.30, vz), pol(360.0, 0.32, nz), W_EC if vz > EB else W0),
         "node %s, neighbour %s of the endcap boundary" % ("beyond" if vz > EB else "inside", "beyond" if nz > EB else "inside"),
         check=functools.partial(_sig, node_ec=vz >= EB, nb_ec=nz >= EB))

for who in ("node", "nb"):
    for sgn, stag in ((1.0, "p"), (-1.0, "m")):
        for z, ztag in ((EB, "at"), (BELOW, "below")):
            vz, nz = (sgn * z, sgn * 480.0) if who == "node" else (sgn * 480.0, sgn * z)
            case("zb_%s_%s_%s" % (who, stag, ztag), pair(pol(300.0, 0.30, vz), pol(360.0, 0.32, nz), pol(340.0, 0.33, sgn * 420.0)),
                 "|z| of the %s %s endcap_boundary at %sz: the >= of gtf_tse.hip:%s" % (
                     "node" if who == "node" else "neighbour", "exactly" if ztag == "at" else "one ulp below",
                     "+" if sgn > 0 else "-", "85, 196" if who == "node" else "53"),
                 check=functools.partial(_sig, node_ec=(who == "node" and ztag == "at"), nb_ec=(who == "nb" and ztag == "at")),
                 hold=(("freeze", ("v",) if who == "node" else ("nb",), (2,)),))


def _kind(field, want, node="v", key="nb", col=None):
    def check(info):
        x = val(info, field, node, key)
        x = x if col is None else x[col]
        if want == "nan":
            assert np.isnan(x), (field, x)
        elif want == "+inf":
            assert x == np.inf, (field, x)
        elif want == "-inf":
            assert x == -np.inf, (field, x)
        else:
            assert x == want and math.copysign(1.0, x) == math.copysign(1.0, want), (field, x)
    return check


def _all(*checks):
    def check(info):
        for c in checks:
            c(info)
    return check


def _partner_kind(field, want, col=None):
    """as _kind, on the key that holds nb's zr terms"""
    def check(info):
        kp = partner(info, "v", "nb")
        x = info["out"].slot[field][kp]
        x = x if col is None else x[col]
        if want == "nan":
            assert np.isnan(x), (field, x)
        elif isinstance(want, str):
            assert x == float(want), (field, x)
        else:
            assert x == want and math.copysign(1.0, x) == math.copysign(1.0, want), (field, x, want)
    return check


case("ec_same_z", pair(pol(300.0, 0.30, 700.0), pol(360.0, 0.32, 700.0), W_EC),
     "an endcap node whose neighbour has its z: |dr / dz| is infinite and so is var_ms",
     check=_kind("tse_var_ms", "+inf"), hold=(("tie", ("v", "nb"), (2,)),))
case("ec_same_z_a0", pair((300.0, 0.0, 700.0), (360.0, 0.0, 700.0), (340.0, 9.0, 760.0)),
     "the same with a == 0: var_ms is 0 * inf = NaN",
     check=_all(_kind("tse_var_ms", "nan"), _kind("tse_sv", 0.0, col=0)), hold=(("tie", ("v", "nb"), (2,)),))

# ---- degenerate geometry: kinds
for dy, tag, want in ((25.0, "pos", "+inf"), (-25.0, "neg", "-inf")):
    case("dx0_" + tag, pair((290.0, 80.0, 100.0), (290.0, 80.0 + dy, 160.0), W0),
         "dx == 0: the xy gradient is %s, its mean infinite and its variance NaN" % want,
         check=lambda info, want=want: (
             np.testing.assert_equal(info["node"]["xy_mean_var"][info["ix"]["v"]][0], float(want)),
             np.testing.assert_equal(np.isnan(info["node"]["xy_mean_var"][info["ix"]["v"]][1]), True)),
         hold=(("tie", ("v", "nb"), (0,)),))
case("dr0", pair(pol(300.0, 0.30, 100.0), pol(300.0, 0.33, 160.0), W0),
     "dr == 0 with dz != 0: tau infinite; the dense J S2 J^T gives NaN for del_tau",
     check=_all(_partner_kind("tse_tau", "inf"), _partner_kind("tse_cov", "nan", col=4), _partner_kind("tse_theta", 0.0, col=0)),
     hold=(("tie", ("v", "nb"), (3,)),))
case("dz0_dr_pos", pair(pol(300.0, 0.30, 100.0), pol(360.0, 0.32, 100.0), W0),
     "dz == 0 with dr > 0: tau = +0 and arctan(1 / tau) = +pi / 2",
     check=_all(_partner_kind("tse_tau", 0.0), _partner_kind("tse_theta", math.pi / 2, col=0)), hold=(("tie", ("v", "nb"), (2,)),))
case("dz0_dr_neg", pair(pol(300.0, 0.30, 100.0), pol(240.0, 0.32, 100.0), W0),
     "dz == 0 with dr < 0: tau = -0 and arctan(1 / tau) = -pi / 2",
     check=_all(_partner_kind("tse_tau", -0.0), _partner_kind("tse_theta", -math.pi / 2, col=0)), hold=(("tie", ("v", "nb"), (2,)),))
case("dr0_dz0", pair(pol(300.0, 0.30, 100.0), pol(300.0, 0.34, 100.0), W0),
     "dr == dz == 0 at another azimuth: tau = 0 / 0", check=_partner_kind("tse_tau", "nan"), hold=(("tie", ("v", "nb"), (2, 3)),))
case("collinear", pair((300.0, 0.0, 100.0), (360.0, 0.0, 150.0), (340.0, 9.0, 160.0)),
     "a neighbour collinear with the origin and the node: m_B == 0, so a == b == 0 and var_ms == 0",
     check=_all(_kind("tse_sv", 0.0, col=0), _kind("tse_sv", 0.0, col=1), _kind("tse_var_ms", 0.0)))
case("curv_pos", pair(pol(300.0, 0.30, 100.0), pol(360.0, 0.33, 150.0), W0), "curvature a > 0",
     check=lambda info: np.testing.assert_array_less(0.0, val(info, "tse_sv")[0]))
case("curv_neg", pair(pol(300.0, 0.30, 100.0), pol(360.0, 0.27, 150.0), W0), "curvature a < 0",
     check=lambda info: np.testing.assert_array_less(val(info, "tse_sv")[0], 0.0))


# ---- singular H: the raising key first, in the middle and last in the dict, beside clean keys and a clean node
def _singular(kind, pos):
    def special(net):
        order = net.dict_order("v")
        nb = net.name_of(order[pos])
        m = net.G.nodes[net.names["v"]]["GNN_Measurement"]
        if kind == "xb0":
            net.move(nb, m.x, m.y, m.z + 60.0, m.r)
        else:
            net.move(nb, 0.0, 0.0, 40.0, 0.0)
        net.names["nb"] = net.names[nb]
    return special


def _raises_at(pos):
    def check(info):
        v = info["ix"]["v"]
        at = [k for (n, k) in info["singular"] if n == v]
        assert len(at) == 1 and at[0] == slot_of(info, "v", "nb")[1]
        g = info["g"]
        lo, hi = int(g.slot_ptr[v]), int(g.slot_ptr[v + 1])
        rk = g.slot["tse_rank"][lo:hi]
        assert int((rk[rk >= 0] < g.slot["tse_rank"][at[0]]).sum()) == pos
        # the node that mirrors the key raises too; every other node is clean
        assert sorted(set(n for n, _ in info["singular"])) == sorted([v, info["ix"]["nb"]])
    return check


for kind, what in (("xb0", "x_B == 0: a neighbour with the node's own x, y and another z"),
                   ("xbx0", "x_B == x_0: a neighbour at the origin")):
    for pos, ptag in ((0, "first"), (1, "mid"), (2, "last")):
        case("sing_%s_%s" % (kind, ptag), hub(3, special=_singular(kind, pos)),
             what + "; the raising key %s in the dict" % ptag, check=_raises_at(pos), raises=("v", "nb"), keys=3,
             hold=(("tie", ("v", "nb"), (0, 1, 3)),) if kind == "xb0" else ())   # (r follows x, y)


def _origin_node(info):
    v = info["ix"]["v"]
    assert sorted(k for n, k in info["singular"] if n == v) == list(range(int(info["g"].slot_ptr[v]), int(info["g"].slot_ptr[v + 1])))
    assert sorted(set(n for n, _ in info["singular"])) == sorted(info["ix"][k] for k in ("v", "n0", "n1"))


def _origin_build(net):
    net.node("v", 0.0, 0.0, 10.0, 0.0)
    for i in range(2):
        net.polar("n%d" % i, *clean_nb(i))
        net.edge("n%d" % i, "v", i)
    net.polar("w", 340.0, 0.33, 160.0)
    net.edge("n0", "w", 2)


case("sing_x0_0", _origin_build, "x_0 == 0: the node at the origin, every key of it raises; w two hops away is clean",
     check=_origin_node, raises=("v", "n0", "n1"))


# ---- key counts and dict order
def _count(n):
    def check(info):
        g, v = info["g"], info["ix"]["v"]
        lo, hi = int(g.slot_ptr[v]), int(g.slot_ptr[v + 1])
        rk = g.slot["tse_rank"][lo:hi]
        assert hi - lo == n and int((rk >= 0).sum()) == n
        if n >= 3:
            # the set order is not ascending in the ids, and the dict position is not the slot index:
            # the partner n - 1 - i is then not the mirror slot
            keys = g.slot["slot_key"][lo:hi][np.argsort(rk)]
            assert not np.array_equal(keys, np.sort(keys)[::-1]) and not np.array_equal(rk, np.arange(n))
            assert not np.array_equal(rk, np.arange(n)[::-1])
        e, r = g.slot["is_edge"][lo:hi], g.slot["rev_edge"][lo:hi]
        if n >= 3:
            assert (e & ~r.astype(bool)).any() and (~e.astype(bool) & r.astype(bool)).any() and (e & r).any()
        mv = info["node"]["xy_mean_var"][v]
        assert np.isnan(mv).all() if n == 0 else np.isfinite(mv).all()
    return check


COUNTS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 32, 33, 64, 65, 70, 127, 128, 129, 130, 257)
for n in COUNTS:
    case("keys_%d" % n, hub(n), "%d keys%s" % (n, {0: ": np.mean([]) is NaN", 3: ": the middle key is its own partner"}.get(n, "")
                                                + (": numpy's pairwise sum recurses" if n > 128 else "")),
         check=_count(n), keys=n)


# ---- oracle-only: what the reference's dicts cannot hold
def _absent(which):
    def post(g, lo, hi):
        rk = g.slot["tse_rank"][lo:hi]
        rk[list(which)] = -1
    return post


def _ranks(fn):
    def post(g, lo, hi):
        g.slot["tse_rank"][lo:hi] = fn(hi - lo)
    return post


def _present(n):
    def check(info):
        g, v = info["g"], info["ix"]["v"]
        rk = g.slot["tse_rank"][int(g.slot_ptr[v]):int(g.slot_ptr[v + 1])]
        assert int((rk >= 0).sum()) == n and np.isfinite(info["node"]["zr_mean_var"][v]).all()
    return check


NOT_A_DICT = "a dict of the reference holds every neighbour, at dense ranks in reversed set order"
case("absent_staged", hub(5), "absent keys (rank < 0) between present ones in a staged node (d <= G)", check=_present(3),
     ref=NOT_A_DICT, post=_absent((1, 3)), keys=3)
case("absent_65_slots", hub(65), "absent keys between present ones in a 65-slot node", check=_present(60),
     ref=NOT_A_DICT, post=_absent((0, 7, 31, 40, 64)), keys=60)
case("sparse_ranks", hub(7), "sparse ranks: 3 i + 1 of a permutation", check=_present(7), ref=NOT_A_DICT,
     post=_ranks(lambda n: (np.arange(n) * 5 % n) * 3 + 1), keys=7)
case("ranks_in_slot_order", hub(6), "ranks in slot order (no set gives it for these ids)", check=_present(6), ref=NOT_A_DICT,
     post=_ranks(lambda n: np.arange(n)), keys=6)
case("ranks_against_slot_order", hub(9), "ranks against the slot order, in a 16-lane group", check=_present(9), ref=NOT_A_DICT,
     post=_ranks(lambda n: np.arange(n)[::-1] * 2), keys=9)

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
FIELDS = ("tse_sv", "tse_tau", "tse_cov", "tse_xyzr", "tse_theta", "tse_var_ms")
NODE_FIELDS = ("xy_mean_var", "zr_mean_var", "angle_of_rotation", "translation")


# --------------------------------------------------------------------------- building
def build(case, base=None, slots=None):
    """the case's component (nx.DiGraph), its names and its padding nodes"""
    net = Net(8192 * CASES.index(case) if base is None else base)
    case.build(net)
    net.finish()
    if slots is not None:
        net.pad("v", slots)
    return net.G, dict(net.names), list(net.pads)


def _post(case, g, names, first=0):
    """the case's edit of v's own slots (the padding's slots follow them and hold no key)"""
    if case.post:
        v = first + int(np.nonzero(g.node["node_id"][first:] == names["v"])[0][0])
        lo, hi = int(g.slot_ptr[v]), int(g.slot_ptr[v + 1])
        case.post(g, lo, lo + int((g.slot["tse_rank"][lo:hi] >= 0).sum()))


@functools.lru_cache(maxsize=None)
def _packed(name):
    case = BY_NAME[name]
    G, names, _ = build(case)
    g = graph.pack([G])
    _post(case, g, names)
    return g, names


def packed(case):
    """the unpadded case as a TrackGraph of its own (a copy), and its names"""
    g, names = _packed(case.name)
    return g.copy(), names


def run_oracle(g):
    """(output graph, node arrays, singular (node, slot) list) of the oracle's a2 on g"""
    out = g.copy()
    for f in FIELDS:
        out.slot[f][:] = np.nan
    sing = []
    with np.errstate(all="ignore"):
        node = O.compute_track_state_estimates(out, P, singular=sing)
    return out, node, sing


def info_of(case):
    g, names = packed(case)
    out, node, sing = run_oracle(g)
    ix = {k: int(np.nonzero(g.node["node_id"] == v)[0][0]) for k, v in names.items()}
    return dict(g=g, out=out, node=node, singular=sing, names=names, ix=ix)


def v_slots(case):
    g, names = _packed(case.name)
    v = int(np.nonzero(g.node["node_id"] == names["v"])[0][0])
    return int(g.slot_ptr[v + 1] - g.slot_ptr[v])


def bucket(slots):
    return 8 if slots <= 8 else 16 if slots <= 16 else 32 if slots <= 32 else 64 if slots <= 64 else 65


@functools.lru_cache(maxsize=1)
def everything():
    """(graph, components): every case, the padded variants of the cases whose "v" has at most 8
    slots, and the fillers that leave every bucket of the schedule with a partial last block. A
    component: dict(case, slots, names, nodes (index range), own (how many of its first nodes are
    the case's own; the padding follows), ix (name -> node index))"""
    subs, comps = [], []
    base = [8192 * len(CASES)]

    def add(case, slots, fresh=True):
        G, names, pads = build(case, base[0] if fresh else None, slots)
        base[0] += 8192 if fresh else 0
        subs.append(G)
        comps.append(dict(case=case, slots=slots, names=names, own=G.number_of_nodes() - len(pads)))

    for case in CASES:
        add(case, None, fresh=False)
    for case in CASES:
        if v_slots(case) <= 8:
            for s in PAD_SLOTS:
                add(case, s)

    def need(b):
        deg = [d for G in subs for _, d in _slot_counts(G)]
        return (1 - sum(1 for d in deg if bucket(d) == b)) % GROUPS_PER_BLOCK[b]

    for b in (65, 64, 32, 16):
        for _ in range(need(b)):
            add(BY_NAME["keys_3"], b)
    for _ in range(need(8)):
        add(BY_NAME["keys_0"], None)
    g = graph.pack(subs)
    n0 = 0
    for c, G in zip(comps, subs):
        c["nodes"] = (n0, n0 + G.number_of_nodes())
        _post(c["case"], g, c["names"], n0)
        c["ix"] = {k: n0 + list(G.nodes).index(v) for k, v in c["names"].items()}
        n0 += G.number_of_nodes()
    return g, comps


def _slot_counts(G):
    return [(n, len(set(G.predecessors(n)) | set(G.nodes[n]["track_state_estimates"]))) for n in G.nodes]


def perturbed(g, hold, names, seed):
    """g with every coordinate moved by +-2^-46 relative, each on its own, but for `hold`
    (Case.hold): frozen coordinates stay, tied ones share one factor per column"""
    rng = np.random.default_rng(seed)
    h = g.copy()
    f = 1.0 + rng.choice([-1.0, 1.0], size=h.node["gnn"].shape) * 2.0 ** -46
    for how, who, cols in hold:
        rows = [int(np.nonzero(g.node["node_id"] == names[k])[0][0]) for k in who]
        for c in cols:
            f[rows, c] = 1.0 if how == "freeze" else f[rows[0], c]
    h.node["gnn"] = h.node["gnn"] * f
    return h
