"""Directed inputs for the parabolic-model states and pairwise KL distances (a17, csrc/gtf_kl.hip),
shared by tests/golden/make_golden_kl_cases.py (the reference's own compute_track_state_estimates,
KLDistance and calc_pairwise_distances on every case: tests/golden/kl_cases.npz), test_kl_cases.py
(CPU: the oracle against that record, every claim, the singular classes, the conditioning shares) and
test_gpu_kl_cases.py (every case through every node layout and arithmetic path of ParabolicKL).

A case is a CSR ``(ptr, src, gnn[N, 4], truth or None)``: receivers (nodes with in-edges) and senders
(nodes with none). A receiver has no out-edge -- the reference takes nx.all_neighbors, predecessors
then successors, for the gradients and reshapes the states to (num_in_edges, 3, 3) -- so its
neighbours are exactly its in-edges, in slot order. ``Case.claim`` says which branch the case is
there for and ``Case.check(case, rec)`` asserts it on the record. ``Case.kind``:

  value     finite geometry: distances are held to the exact value (exact_kl)
  singular  a receiver at which the reference, the kernel's rule, or both raise; ``Case.singular``
            is the expected class ("both", "reference", "kernel", or "none" for the near-singular one)
  moments   a gradient with dx == 0 (inf / NaN moments): classes of non-finite values
  shape     launch shapes (bucket populations, block interleaving, degree runs): values as "value"
  tile      tiled-layout directed cases (``tile_only``: run in the tiled layouts alone)
  truth     the truth flag's three-way equality

The exact-arithmetic definitions are here too (50-digit Decimal for the states and distances, Fraction
for the gradient moments), all computed from the fp64 inputs: exact_state, exact_kl, exact_moments.
The kernel's singular rule and the q32 geometry are restated in NumPy (kernel_singular,
q32_singular): csrc/gtf_kl.hip is compiled with -ffp-contract=off, so the fp64 restatement is the
kernel's arithmetic operation for operation.
"""
import dataclasses
import decimal
import functools
import math
import zlib
from decimal import Decimal as D
from fractions import Fraction

import numpy as np

CTX = decimal.Context(prec=50)
ERR_SINGULAR_H = 128
WELL = 1e-9          # ref_err at or below which a value case is well-conditioned
FP32_SENS = 1e-4     # sensitivity at or below which a value case is fp32-checked
WIN_NODES, WIN_MARGIN = 1024, 128   # gtf.parabolic's (asserted equal in test_kl_cases)


# --------------------------------------------------------------------------- exact arithmetic
def _geometry(node, nb):
    """(X0, XB, MB) of neighbour nb in the frame of node: rotation by the exact cos / sin of
    2 pi - atan2(y, x), i.e. x / h and -y / h, then translation to the node (utils.py:197-270)"""
    x, y = D(float(node[0])), D(float(node[1]))
    h = CTX.sqrt(CTX.add(CTX.multiply(x, x), CTX.multiply(y, y)))
    with decimal.localcontext(CTX):
        ca, sa = x / h, -y / h
        xt, yt = x * ca - y * sa, x * sa + y * ca
        xb, yb = D(float(nb[0])), D(float(nb[1]))
        return -xt, xb * ca - yb * sa - xt, xb * sa + yb * ca - yt


def _state(X0, XB, MB):
    """the closed-form state of (X0, XB, MB): the columns of H^-1 are the Lagrange basis on
    {X0, 0, XB}; returns (a2 MB, b2 MB, c00, c11, i00, i01, i11, L0, L1, L2)"""
    with decimal.localcontext(CTX):
        s0, s1 = D(16), D(0.1) * D(0.1)
        r0, r1, r2 = 1 / (X0 * (X0 - XB)), 1 / (X0 * XB), 1 / (XB * (XB - X0))
        a0, b0, a1, b1, a2, b2 = r0, -XB * r0, r1, -(X0 + XB) * r1, r2, -X0 * r2
        return (MB * a2, MB * b2, s0 * a0 * a0 + s1 * a1 * a1 + s1 * a2 * a2,
                s0 * b0 * b0 + s1 * b1 * b1 + s1 * b2 * b2,
                X0 ** 4 / s0 + XB ** 4 / s1, X0 ** 3 / s0 + XB ** 3 / s1, X0 ** 2 / s0 + XB ** 2 / s1,
                (a0, b0, D(0)), (a1, b1, D(1)), (a2, b2, D(0)))


def _kl(p, q):
    """KLDistance of two states (extract_metadata_trackml_parabolic_model.py:15-17): component 2 of
    every state is (0, s1), so its terms vanish"""
    with decimal.localcontext(CTX):
        tr = (p[2] - q[2]) * (q[4] - p[4]) + (p[3] - q[3]) * (q[6] - p[6])
        d0, d1 = p[0] - q[0], p[1] - q[1]
        S00, S01, S11 = p[4] + q[4], p[5] + q[5], p[6] + q[6]
        return tr + d0 * (d0 * S00 + d1 * S01) + d1 * (d0 * S01 + d1 * S11)


def exact_state(node, nb):
    """(sv [3], cov [3, 3]) of the edge from nb in exact arithmetic, rounded to fp64 once"""
    s = _state(*_geometry(node, nb))
    with decimal.localcontext(CTX):
        s0, s1 = D(16), D(0.1) * D(0.1)
        cov = [[s0 * s[7][i] * s[7][j] + s1 * s[8][i] * s[8][j] + s1 * s[9][i] * s[9][j] for j in range(3)]
               for i in range(3)]
    return np.array([float(s[0]), float(s[1]), 0.0]), np.array([[float(c) for c in r] for r in cov])


def exact_kl(node, a, b):
    """KLDistance of the exact-arithmetic parabolic states of neighbours a, b of node
    (50-digit decimal; the rotation with exact cos/sin of atan2)."""
    return float(_kl(_state(*_geometry(node, a)), _state(*_geometry(node, b))))


def exact_moments(node, nbs):
    """(mean, population variance) of dy / dx over the neighbours (utils.py:248-251, :297), exact
    rationals of the fp64 inputs rounded once; None where a dx is zero"""
    x, y = Fraction(float(node[0])), Fraction(float(node[1]))
    g = []
    for nb in nbs:
        dx = x - Fraction(float(nb[0]))
        if dx == 0:
            return None
        g.append((y - Fraction(float(nb[1]))) / dx)
    m = sum(g) / len(g)
    return float(m), float(sum((v - m) ** 2 for v in g) / len(g))


# --------------------------------------------------------------------------- the kernel's rules in NumPy
def kernel_geometry(node, nbs):
    """(x0, xB [d], mB [d]) as node_frame_xy and pstate (csrc/gtf_kl.hip) form them in fp64"""
    x, y = np.float64(node[0]), np.float64(node[1])
    nbs = np.asarray(nbs, np.float64).reshape(-1, nbs.shape[-1] if hasattr(nbs, "shape") else 2)
    with np.errstate(all="ignore"):
        h = np.sqrt(x * x + y * y)
        rh = np.float64(1.0) / h
        ca, sa = (x * rh, -y * rh) if h > 0.0 else (np.float64(1.0), np.float64(0.0))
        xt, yt = x * ca - y * sa, x * sa + y * ca
        xB = (nbs[:, 0] * ca - nbs[:, 1] * sa) - xt
        mB = (nbs[:, 0] * sa + nbs[:, 1] * ca) - yt
    return np.float64(0.0) - xt, xB, mB


def kernel_singular(node, nbs):
    """per neighbour: the kernel's stated rule, xB == 0, xB == x0 or x0 == 0 in its own rotation"""
    x0, xB, _ = kernel_geometry(node, nbs)
    return (xB == 0.0) | (xB == x0) | (x0 == 0.0)


def q32_geometry(qnode, qnbs, scale):
    """(x0, xB [d], mB [d]) of PathQ::frame / PathQ::state in fp32 from the fixed-point coordinates"""
    f = np.float32
    s = f(scale)
    with np.errstate(all="ignore"):
        x, y = f(qnode[0]) * s, f(qnode[1]) * s
        h = np.sqrt(x * x + y * y, dtype=f)
        ca, sa = (x / h, -y / h) if h > 0 else (f(1), f(0))
        q = np.asarray(qnbs, np.int64).reshape(-1, 2)
        dx = (q[:, 0] - int(qnode[0])).astype(f) * s
        dy = (q[:, 1] - int(qnode[1])).astype(f) * s
        return -h, dx * ca - dy * sa, dx * sa + dy * ca


def q32_singular(qnode, qnbs, scale):
    x0, xB, _ = q32_geometry(qnode, qnbs, scale)
    return (xB == 0) | (xB == x0) | (x0 == 0)


# --------------------------------------------------------------------------- cases
@dataclasses.dataclass
class Case:
    name: str
    claim: str
    kind: str
    ptr: np.ndarray
    src: np.ndarray
    gnn: np.ndarray
    truth: object = None
    with_single: bool = False
    singular: str = None       # expected class of a singular case
    states: bool = True        # sv / cov recorded and compared (False: the large launch-shape cases)
    tile_only: bool = False
    tile: int = 0              # the tile size at which a tile case's claim holds
    sort_window: int = 8192
    check: object = None       # check(case, rec): the claim on the record

    @property
    def n_nodes(self):
        return int(self.ptr.size - 1)

    @property
    def degree(self):
        return np.diff(self.ptr.astype(np.int64))

    def listed(self):
        return np.nonzero(self.degree >= (1 if self.with_single else 2))[0]

    def nbs(self, v):
        return self.gnn[self.src[self.ptr[v]:self.ptr[v + 1]], :2]

    def pair_ptr(self):
        d = self.degree
        p = np.zeros(d.size + 1, np.int64)
        np.cumsum(np.where(d >= 2, d * (d - 1) // 2, 0), out=p[1:])
        return p


class Graph:
    """receivers and senders as they are added; slot order is the order given"""

    def __init__(self):
        self.xy, self.tr, self.into = [], [], {}

    def node(self, xy, t=0):
        self.xy.append((float(xy[0]), float(xy[1])))
        self.tr.append(int(t))
        return len(self.xy) - 1

    def recv(self, xy, senders, t=0):
        """a receiver at xy whose in-edges come from `senders`: coordinates (new nodes) or node numbers"""
        v = self.node(xy, t)
        self.into[v] = [s if isinstance(s, (int, np.integer)) else self.node(s, t) for s in senders]
        return v

    def finish(self, truth=True):
        n = len(self.xy)
        d = np.array([len(self.into.get(v, ())) for v in range(n)], np.int64)
        ptr = np.zeros(n + 1, np.int32)
        np.cumsum(d, out=ptr[1:])
        src = np.array([s for v in range(n) for s in self.into.get(v, ())], np.int32)
        xy = np.array(self.xy, np.float64).reshape(n, 2)
        gnn = np.concatenate([xy, np.zeros((n, 1)), np.hypot(xy[:, 0], xy[:, 1])[:, None]], 1)
        for v, s in self.into.items():
            assert all(u not in self.into for u in s), "a receiver has no out-edge"
        return dict(ptr=ptr, src=src, gnn=gnn, truth=np.array(self.tr, np.int64) if truth else None)


CASES = []
ILL = {}     # the named ill-conditioned cases: name -> why the reference's own distance is far from exact there


def case(name, claim, kind, g, **kw):
    if isinstance(g, Graph):
        g = g.finish()
    CASES.append(Case(name, claim, kind, **g, **kw))


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def fillers(rng, xy, k, rmin=5.0, rmax=80.0):
    """k senders rmin..rmax mm from the receiver at xy in any direction (bucket_edge_graph's
    geometry), away from the singular lines (xB = 0: perpendicular to the radius through the node;
    xB = x0: the perpendicular through the origin) and from dx = 0"""
    x, y = xy
    h = math.hypot(x, y)
    out = []
    while len(out) < k:
        dr, a = rng.uniform(rmin, rmax), rng.uniform(-math.pi, math.pi)
        dx, dy = dr * math.cos(a), dr * math.sin(a)
        along = (dx * x + dy * y) / h          # = xB
        if abs(along) < 0.25 * dr or abs(along + h) < 0.25 * h or abs(dx) < 0.1 * dr:
            continue
        out.append((x + dx, y + dy))
    return out


BUCKET_D = (2, 4, 8, 9)    # one in-degree of each bucket (thread-per-node d <= 2 and d <= 4, 8 lanes, a wavefront)


def polar(r, phi):
    return (r * math.cos(phi), r * math.sin(phi))


def finite_no_raise(case, rec):
    assert rec["raised_nodes"].size == 0 and np.isfinite(rec["kl"]).all() and rec["kl"].size > 0


# ---- geometry: the special neighbours alone (when they are two or more) and first among the
# ---- slots of a receiver of every bucket
def geometry(name, claim, node, special, check=finite_no_raise, kind="value", **kw):
    rng, g = _rng(name), Graph()
    ds = sorted(d for d in set(BUCKET_D) | {max(len(special), 2)} if d >= len(special))
    for d in ds:
        g.recv(node, list(special) + fillers(rng, node, max(d - len(special), 0)))
    case(name, claim, kind, g, check=check, **kw)


for nm, xy in (("px", (250.0, 0.0)), ("mx", (-250.0, 0.0)), ("py", (0.0, 250.0)), ("my", (0.0, -250.0)),
               ("q1", polar(300.0, 0.7)), ("q2", polar(300.0, 2.3)), ("q3", polar(300.0, -2.3)), ("q4", polar(300.0, -0.7)),
               ("px_y_plus0", (120.0, 0.0)), ("px_y_minus0", (120.0, -0.0)), ("mx_y_plus0", (-120.0, 0.0)),
               ("mx_y_minus0", (-120.0, -0.0)), ("r30", polar(30.0, 1.1)), ("r1000", polar(1000.0, -1.9))):
    geometry("node_" + nm, "the node at (%r, %r): the frame's rotation in this quadrant / on this axis" % xy, xy,
             [])


def _check_geo(cond):
    def check(case, rec):
        finite_no_raise(case, rec)
        v = int(case.listed()[0])
        x0, xB, mB = kernel_geometry(case.gnn[v], case.nbs(v))
        assert cond(x0, xB, mB), (x0, xB, mB)
    return check


NODE_A = polar(400.0, 0.6)
U, V = (math.cos(0.6), math.sin(0.6)), (-math.sin(0.6), math.cos(0.6))     # radial and transverse unit vectors


def at(xB, mB, node=NODE_A, u=U, v=V):
    """the point with node-frame coordinates (xB, mB) up to rounding (the frame rotates by -phi)"""
    return (node[0] + xB * u[0] + mB * v[0], node[1] + xB * u[1] + mB * v[1])


geometry("nb_collinear_inside", "a neighbour on the line origin-node, between them: mB = 0, sv = 0", NODE_A,
         [(NODE_A[0] * 0.875, NODE_A[1] * 0.875)], _check_geo(lambda x0, xB, mB: abs(mB[0]) < 1e-9 and xB[0] < 0))
geometry("nb_collinear_beyond", "a neighbour on the line origin-node, beyond the node", NODE_A,
         [(NODE_A[0] * 1.125, NODE_A[1] * 1.125)], _check_geo(lambda x0, xB, mB: abs(mB[0]) < 1e-9 and xB[0] > 0))
geometry("nb_xB_minus_x0", "a neighbour at xB = -x0 (x0 + xB = 0: b1 vanishes)", NODE_A, [at(400.0, 9.0)],
         _check_geo(lambda x0, xB, mB: abs(xB[0] + x0) < 1e-9 and abs(mB[0]) > 1))
geometry("nb_xB_2x0", "a neighbour at xB = 2 x0, beyond the old origin", NODE_A, [at(-800.0, 11.0)],
         _check_geo(lambda x0, xB, mB: abs(xB[0] - 2 * x0) < 1e-9 and abs(mB[0]) > 1))
NB1 = at(-30.0, 4.0)


def _check_equal(case, rec):
    finite_no_raise(case, rec)
    assert rec["kl"][0] == 0.0 and exact_kl(case.gnn[0], NB1, NB1) == 0.0


geometry("nb_equal_pair", "two equal neighbours: their KL is exactly 0 in closed form", NODE_A, [NB1, NB1], _check_equal)
geometry("nb_one_ulp_pair", "two neighbours one ulp apart in x", NODE_A, [NB1, (float(np.nextafter(NB1[0], 1e9)), NB1[1])])
ILL["nb_one_ulp_pair"] = "two states one ulp apart: the distance is a difference of nearly equal numbers"
geometry("nb_dy0", "a neighbour with dy == 0: gradient 0", NODE_A, [(NODE_A[0] - 20.0, NODE_A[1])],
         lambda c, r: (finite_no_raise(c, r), np.testing.assert_equal(np.isfinite(r["gmean"][c.listed()]).all(), True)))


def _check_moments(mean_class, d=None):
    def check(case, rec):
        assert rec["raised_nodes"].size == 0 and np.isfinite(rec["kl"]).all()
        for v in case.listed():
            m, var = rec["gmean"][v], rec["gvar"][v]
            assert np.isnan(var) and (np.isnan(m) if mean_class == "nan" else np.isinf(m)), (v, m, var)
    return check


geometry("nb_dx0_above", "a neighbour with dx == 0 above the node: gradient -inf, mean inf, variance NaN", NODE_A,
         [(NODE_A[0], NODE_A[1] + 20.0)], _check_moments("inf"), kind="moments")
geometry("nb_dx0_below", "a neighbour with dx == 0 below the node: gradient +inf", NODE_A,
         [(NODE_A[0], NODE_A[1] - 20.0)], _check_moments("inf"), kind="moments")
geometry("nb_dx0_both", "dx == 0 above and below: +inf and -inf, mean and variance NaN", NODE_A,
         [(NODE_A[0], NODE_A[1] + 20.0), (NODE_A[0], NODE_A[1] - 25.0)], _check_moments("nan"), kind="moments")


def _single_inf():
    g = Graph()
    g.recv(NODE_A, [(NODE_A[0], NODE_A[1] - 20.0)])
    g.recv(polar(200.0, 2.0), fillers(_rng("single_inf"), polar(200.0, 2.0), 1))
    return g


def _check_single_inf(case, rec):
    assert rec["kl"].size == 0 and np.isinf(rec["gmean"][0]) and np.isnan(rec["gvar"][0])
    assert np.isfinite(rec["gmean"][2]) and rec["gvar"][2] == 0.0


case("single_edge_inf_gradient", "a one-edge node whose gradient is inf (with_single): the variance is 0 * (inf - inf) "
     "= NaN, beside a one-edge node with variance 0", "moments", _single_inf(), with_single=True, check=_check_single_inf)


# ---- singular geometries: the raising edge first, in the middle and last among the slots of a
# ---- d = 2, 4, 8 and 9 receiver, beside a clean receiver of each bucket
SING_D = (2, 4, 8, 9)


def singular(name, claim, node, nb, cls):
    rng, g = _rng(name), Graph()
    for d in SING_D:
        for pos in sorted({0, d // 2, d - 1}):
            f = fillers(rng, node, d - 1) if math.hypot(*node) > 0 else fillers(rng, (40.0, 30.0), d - 1)
            g.recv(node, f[:pos] + [nb] + f[pos:])
    for d in SING_D:
        c = polar(350.0, -1.0 + 0.1 * d)
        g.recv(c, fillers(rng, c, d))
    case(name, claim, "singular", g, singular=cls)


def mirrors(p):
    """p and its images under x -> -x, y -> -y and x <-> y"""
    out = []
    for sw in (False, True):
        for sx in (1.0, -1.0):
            for sy in (1.0, -1.0):
                q = (p[1], p[0]) if sw else p
                out.append((sx * q[0] if q[0] != 0 else q[0], sy * q[1] if q[1] != 0 else q[1]))
    return out


SINGULAR_GEOMETRIES = (
    ("perp_axis", "neighbour on the perpendicular through a node on an axis (xB = 0)", (10.0, 0.0), (10.0, 5.0)),
    ("origin_nb", "the neighbour is the origin (xB = x0)", (10.0, 5.0), (0.0, 0.0)),
    ("perp_diag", "neighbour on the perpendicular through a node on the diagonal (xB = 0)", (8.0, 8.0), (10.0, 6.0)),
)
# The class of every image as the record has it (test_kl_cases.test_singular_classes holds each to the
# record): "kernel" where the kernel's geometric rule raises and the reference's rotation by
# cos / sin(2 pi - atan2) leaves a pivot of a few ulp, so that it returns unbounded values; every
# image not named here is "both"
SINGULAR_CLASSES = dict.fromkeys(["sing_perp_axis_0", "sing_perp_axis_6", "sing_perp_diag_6"] +
                                 ["sing_origin_nb_%d" % m for m in range(8)], "kernel")
for _key, _claim, _node, _nb in SINGULAR_GEOMETRIES:
    for _m, (_n, _b) in enumerate(zip(mirrors(_node), mirrors(_nb))):
        singular("sing_%s_%d" % (_key, _m), "%s: node %r, neighbour %r" % (_claim, _n, _b), _n, _b,
                 SINGULAR_CLASSES.get("sing_%s_%d" % (_key, _m), "both"))
singular("sing_node_at_origin", "the node at the origin (x0 = 0)", (0.0, 0.0), (12.0, 7.0), "both")
singular("sing_node_at_minus_zero", "the node at (-0.0, -0.0)", (-0.0, -0.0), (-12.0, 7.0), "both")
for _m, _n in enumerate(((10.0, 5.0), (-250.0, 0.0), polar(300.0, -2.3))):
    singular("sing_nb_equals_node_%d" % _m, "the neighbour equal to the node %r (xB = 0, mB = 0, dx = 0)" % (_n,), _n, _n, "both")
singular("near_singular_one_ulp", "xB one ulp (of the node's x) from 0: no exact singularity", (10.0, 0.0),
         (float(np.nextafter(10.0, 11.0)), 5.0), "none")


# ---- in-degrees
def _degree(d, name):
    rng, g = _rng(name), Graph()
    for k in range(2 if d <= 17 else 1):
        c = polar(rng.uniform(30.0, 1000.0), rng.uniform(-math.pi, math.pi))
        g.recv(c, fillers(rng, c, d))
    return g


def _check_degree(d, listed):
    def check(case, rec):
        assert (case.degree[case.listed()] == d).all() and case.listed().size == listed
        assert rec["kl"].size == listed * d * (d - 1) // 2 and np.isfinite(rec["kl"]).all()
    return check


WHY_D = {4: "the last thread-per-node count", 5: "the first 8-lane count", 8: "the last 8-lane count",
         9: "the first wavefront count", 16: "120 pairs: the last count read from the pair table",
         17: "136 pairs: the first solved by pair_ij", 63: "below the LDS stage of 64 states", 64: "the LDS stage exactly full",
         65: "one state beyond the LDS stage: pair lanes recompute both states", 130: "three rounds of lanes over the in-edges"}
for d in (2, 3, 4, 5, 6, 7, 8, 9, 16, 17, 63, 64, 65, 130):
    case("deg_%d" % d, "in-degree %d%s" % (d, ": " + WHY_D[d] if d in WHY_D else ""), "value", _degree(d, "deg_%d" % d),
         check=_check_degree(d, 2 if d <= 17 else 1))
case("deg_1", "in-degree 1 without with_single: a graph with no listed node", "shape", _degree(1, "deg_1"),
     check=_check_degree(1, 0))
case("deg_1_single", "in-degree 1 with with_single: states and moments, no pair", "shape", _degree(1, "deg_1"),
     with_single=True, check=_check_degree(1, 2))


def _one_each(name):
    rng, g = _rng(name), Graph()
    for d in BUCKET_D:
        c = polar(200.0 + 90 * d, 0.3 * d)
        g.recv(c, fillers(rng, c, d))
    return g


case("bucket_of_one", "each bucket holds exactly one node", "value", _one_each("bucket_of_one"),
     check=lambda c, r: np.testing.assert_equal(sorted(c.degree[c.listed()]), list(BUCKET_D)))
case("n0", "N = 0", "shape", dict(ptr=np.zeros(1, np.int32), src=np.zeros(0, np.int32), gnn=np.zeros((0, 4)),
                                   truth=np.zeros(0, np.int64)), check=lambda c, r: np.testing.assert_equal(r["kl"].size, 0))
case("senders_only", "nodes and no edge: no listed node", "shape",
     dict(ptr=np.zeros(6, np.int32), src=np.zeros(0, np.int32), gnn=np.array([[10.0 * i, 3.0, 0, 0] for i in range(1, 6)]),
          truth=np.arange(5, dtype=np.int64)), check=lambda c, r: np.testing.assert_equal(r["kl"].size, 0))


# ---- bucket populations and the block interleaving: clusters of receivers sharing a pool of senders
PER_BLOCK = (64, 64, 8, 1)      # nodes per 64-thread block of the four buckets (gtf_kl.hip BLOCK / BG)
BUCKET_DEGREES = ((2,), (3, 4), (5, 6, 7, 8), (9, 10, 11, 12))


def population(name, counts, degrees=BUCKET_DEGREES, cluster=16):
    """counts[b] receivers of bucket b, their in-degrees cycling through degrees[b], node numbers
    shuffled; receivers come in clusters within 1 mm that draw from one pool of 14 senders"""
    rng, g = _rng(name), Graph()
    want = [degrees[b][i % len(degrees[b])] for b in range(4) for i in range(counts[b])]
    order = rng.permutation(len(want))
    pool, centre = [], None
    for n, k in enumerate(order):
        if n % cluster == 0:
            centre = polar(rng.uniform(60.0, 1000.0), rng.uniform(-math.pi, math.pi))
            pool = [g.node(p, n % 3) for p in fillers(rng, centre, 14, 12.0, 80.0)]
        d = want[k]
        c = (centre[0] + rng.uniform(-0.5, 0.5), centre[1] + rng.uniform(-0.5, 0.5))
        g.recv(c, [pool[(n + i) % 14] for i in range(d)], t=n % 3)
    return g


def blocks_of(case):
    """nodes per bucket of the listed nodes"""
    d = case.degree[case.listed()]
    return [int(((d >= lo) & (d <= hi)).sum()) for lo, hi in ((1, 2), (3, 4), (5, 8), (9, 1 << 30))]


def _check_blocks(raw):
    def check(case, rec):
        n = blocks_of(case)
        assert [-(-c // p) for c, p in zip(n, PER_BLOCK)] == list(raw), (n, raw)
        assert np.isfinite(rec["kl"]).all() and rec["raised_nodes"].size == 0
    return check


for b in range(4):
    for nb_, cnt in ((7, 6 * PER_BLOCK[b] + 1), (8, 8 * PER_BLOCK[b]), (9, 8 * PER_BLOCK[b] + 1)):
        counts = [1, 1, 1, 1]
        counts[b] = cnt
        raw = [1, 1, 1, 1]
        raw[b] = nb_
        case("pop_b%d_%dblocks" % (b, nb_), "bucket %d holds %d nodes: %d blocks (%s), the other buckets one node each"
             % (b, cnt, nb_, "the last one partial" if cnt % PER_BLOCK[b] else "all full"), "shape",
             population("pop_b%d_%d" % (b, nb_), counts), states=False, check=_check_blocks(raw))
case("b0_empty", "bucket 0 empty, the others populated: the interleaving has tot = rest", "shape",
     population("b0_empty", [0, 70, 20, 9]), states=False, check=_check_blocks([0, 2, 3, 9]))
case("b0_only", "only bucket 0 populated: the interleaving has rest = 0", "shape",
     population("b0_only", [130, 0, 0, 0]), states=False, check=_check_blocks([3, 0, 0, 0]))
case("b0_8_vs_40", "bucket 0 of 8 blocks against 40 blocks of the others (16 + 8 + 16)", "shape",
     population("b0_8_vs_40", [500, 600, 10, 9]), states=False, check=_check_blocks([8, 10, 2, 9]))
case("b0_40_vs_8", "bucket 0 of 40 blocks (33 before padding) against 8 of the others", "shape",
     population("b0_40_vs_8", [2049, 0, 0, 2], cluster=64), states=False, check=_check_blocks([33, 0, 0, 2]))
for absent in (5, 6, 7, 8):
    degs = (BUCKET_DEGREES[0], BUCKET_DEGREES[1], tuple(d for d in (5, 6, 7, 8) if d != absent), BUCKET_DEGREES[3])
    case("runs_without_%d" % absent, "degree runs with no %d-edge node: that run is empty, the next starts where it would"
         % absent, "shape", population("runs_without_%d" % absent, [5, 7, 11, 1], degs),
         check=lambda c, r, a=absent: np.testing.assert_equal((a in c.degree, np.isfinite(r["kl"]).all()), (False, True)))


# ---- the tiled layout: nodes on a ring at rising azimuth, so that the azimuth sort keeps their order
def ring(n_recv, per, r_recv=500.0, d=2, phi0=-3.0, phi1=3.0, singles=False):
    """n_recv receivers, each followed by `per` senders, at azimuth running from phi0 to phi1;
    receiver k takes the d senders that follow it on the ring (the last ones: that precede it);
    singles: in-degrees 1, 2, 3, 4 in turn. Returns (graph, receivers, senders)"""
    g = Graph()
    n = n_recv * (1 + per)
    step = (phi1 - phi0) / n
    recv, send, after = [], [], []
    for k in range(n_recv):
        i = k * (1 + per)
        recv.append(g.node(polar(r_recv, phi0 + step * i), k % 3))
        after.append(len(send))
        send += [g.node(polar(r_recv - 25.0 - 9.0 * ((k + q) % 5), phi0 + step * (i + 1 + q)), (k + q) % 3) for q in range(per)]
    for k, v in enumerate(recv):
        dk = 1 + k % 4 if singles else d
        lo = min(after[k], len(send) - dk)
        g.into[v] = send[lo:lo + dk]
    return g, recv, send


def tiled_layout(c, tile, tile_b1=True):
    """the ParabolicKL of a case in a tiled layout on the host, with its block records [n_blk, 12]"""
    from gtf.parabolic import ParabolicKL
    k = ParabolicKL(c.ptr, c.src, c.gnn, c.truth, device="cpu", with_single=c.with_single, tile=tile, tile_b1=tile_b1,
                    sort_window=c.sort_window)
    return k, k.blk.numpy().reshape(-1, 12).astype(np.int64)


def _edge_targets(blk, tile):
    """(device node of a two-edge receiver, device node it takes as its second sender) for wlo - 1,
    wlo, whi - 1 and whi: all four in the middle tile, or (tile < 4) one each in four tiles"""
    t = blk.shape[0] // 2
    out = []
    for q in range(4):
        r = blk[t + q] if tile < 4 else blk[t]
        out.append((int(r[0]) + (0 if tile < 4 else q), int((r[9] - 1, r[9], r[10] - 1, r[10])[q]), int(r[9]), int(r[10])))
    return out


def _window_edges(tile, n_recv, per):
    g, recv, _ = ring(n_recv, per)
    c = Case("probe", "", "tile", **g.finish())
    k, blk = tiled_layout(c, tile)
    for v, u, wlo, whi in _edge_targets(blk, tile):
        assert wlo > 0 and whi < c.n_nodes, "the window is clipped"
        v, u = int(k.node_of[v]), int(k.node_of[u])
        assert v in g.into and u not in g.into, "the window edge is a receiver: choose another ring"
        g.into[v][1] = u
    return g


def _check_window(case, rec):
    k, blk = tiled_layout(case, case.tile)
    src, ptr = k.slot_src.numpy(), k.slot_ptr_host
    for v, u, wlo, whi in _edge_targets(blk, case.tile):
        assert int(src[ptr[v] + 1]) == u and wlo > 0 and whi < case.n_nodes, (v, u, wlo, whi)
    assert np.isfinite(rec["kl"]).all()


for _tile, _nr, _per in ((4, 260, 4), (256, 581, 1), (1, 260, 4)):
    case("tile%d_window_edges" % _tile, "tile = %d: senders exactly at wlo - 1, wlo, whi - 1 and whi of a tile's window "
         "(WSrc::in on both sides of both ends)" % _tile, "tile", _window_edges(_tile, _nr, _per), tile=_tile,
         tile_only=True, states=False, check=_check_window)


def _wide():
    g, recv, send = ring(4, 350)
    g.into[recv[2]] = [send[2 * 350], send[3 * 350 - 1]]   # one sender inside the window; the tile's own last node, beyond it
    return g                                                # (the last receiver's senders follow it: in the next tile)


def _check_wide(case, rec):
    k, blk = tiled_layout(case, case.tile)
    assert blk.shape[0] == 2 and blk[1, 0] - blk[0, 0] > WIN_NODES and blk[0, 10] - blk[0, 9] == WIN_NODES, blk
    src, ptr = k.slot_src.numpy(), k.slot_ptr_host
    s = src[ptr[0]:ptr[4]]
    assert (s >= blk[0, 10]).sum() == 3 and (s < blk[0, 10]).sum() == 5, "the tile's senders on both sides of the window's end"
    assert blk[0, 10] <= s[5] < blk[1, 0], "a node of the tile itself beyond the window"
    assert np.isfinite(rec["kl"]).all()


def _check_clipped(case, rec):
    blk = tiled_layout(case, 4)[1]
    assert (blk[:, 9] == 0).all() and (blk[:, 10] == case.n_nodes).all() and blk.shape[0] >= 10


def _check_sort_window(case, rec):
    k, _ = tiled_layout(case, 4)
    # azimuth falls with the node number: one sort over the event would put the last nodes first
    assert case.n_nodes > 4 * 64 and (k.node_of[:16] < 128).all(), k.node_of[:16]


case("tile_wider_than_window", "a tile of 4 two-edge nodes and 1,050 senders: its span exceeds WIN_NODES, the clamp "
     "min(whi, wlo + WWIN) cuts the window and the tile's own later nodes are read from global memory", "tile",
     _wide(), tile=4, tile_only=True, states=False, check=_check_wide)
case("tile_window_clipped", "a small event: every window is clipped at node 0 and at N", "tile", ring(40, 2)[0], tile=4,
     tile_only=True, check=_check_clipped)
case("tile_sort_window_64", "sort_window = 64 smaller than the event: azimuth order inside windows of 64 nodes", "tile",
     ring(100, 2, phi0=3.0, phi1=-3.0)[0], tile=4, tile_only=True, sort_window=64, check=_check_sort_window)
case("tile_256_full", "300 one- to four-edge nodes (with_single): a tile with exactly 256 of them, one per thread", "tile",
     ring(300, 3, singles=True)[0], tile=256, tile_only=True, with_single=True, states=False,
     check=lambda c, r: np.testing.assert_equal(int(tiled_layout(c, 256)[1][0, [1, 3, 4]].sum()), 256))


# ---- the truth flag: node, neighbour i and neighbour j all equal (script :95)
def truth_case(name, claim, tn, ids, want):
    rng, g = _rng(name), Graph()
    for d in BUCKET_D:
        c = polar(300.0 + 10 * d, 0.2 * d)
        v = g.recv(c, fillers(rng, c, d), t=tn)
        for q, u in enumerate(g.into[v]):
            g.tr[u] = ids[q % len(ids)]

    def check(case, rec):
        assert rec["truth"][0] == want and set(np.unique(rec["truth"])) <= {0, 1}
    case(name, claim, "truth", g, check=check)


BIG = 3 * 2 ** 32 + 11
truth_case("truth_all_equal", "node = i = j", 5, (5,), 1)
truth_case("truth_node_differs", "node != i = j", 6, (5,), 0)
truth_case("truth_i_differs", "node = j != i (pair (1, 0): i is slot 1)", 5, (5, 6), 0)
truth_case("truth_j_differs", "node = i != j", 5, (6, 5), 0)
truth_case("truth_all_differ", "three different ids", 5, (6, 7), 0)
truth_case("truth_beyond_int32_equal", "ids beyond int32, equal", BIG, (BIG,), 1)
truth_case("truth_equal_modulo_2_32", "ids equal modulo 2^32 but different: 0 in f64, and q32 relabels instead of truncating",
           BIG, (BIG + 2 ** 32, BIG), 0)
truth_case("truth_negative_equal", "negative ids, equal", -3, (-3,), 1)
truth_case("truth_negative_vs_positive", "-3 against 3", -3, (3, -3), 0)
_g = Graph()
for _d in BUCKET_D:
    _c = polar(320.0, 0.3 * _d)
    _g.recv(_c, fillers(_rng("truth_none"), _c, _d))
case("truth_none", "truth = None: no truth input, no truth output", "truth", _g.finish(truth=False),
     check=lambda c, r: np.testing.assert_equal(int(r["truth"].sum()), 0))

# ---- the case the output-selection, stride and C-ABI tests run on: every bucket, both kinds of flag
case("mix_all_buckets", "every bucket with several nodes and mixed truth: the input of the output-selection cases", "value",
     population("mix_all_buckets", [70, 70, 20, 5]), check=finite_no_raise)

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
VALUE_KINDS = ("value", "shape", "tile", "truth")


# --------------------------------------------------------------------------- the record and what follows from it
@functools.lru_cache(maxsize=None)
def record():
    import os
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kl_cases.npz")) as z:
        out = {}
        for k in z.files:
            name, f = k.split("__")
            out.setdefault(name, {})[f] = z[k]
    for c in CASES:
        r = out[c.name]
        r.setdefault("raised_nodes", np.zeros(0, np.int64))
        r.setdefault("raised", np.zeros(0, "U1"))
    return out


def kernel_raising(c):
    """(nodes, slot mask): the listed nodes at which the kernel's rule raises, and the slots it names"""
    mask = np.zeros(int(c.ptr[-1]), bool)
    nodes = []
    for v in c.listed():
        m = kernel_singular(c.gnn[v], c.nbs(v))
        mask[c.ptr[v]:c.ptr[v + 1]] = m
        if m.any():
            nodes.append(int(v))
    return np.array(nodes, np.int64), mask


def singular_class(c, rec):
    """"both", "reference" or "kernel" by the listed nodes at which the record and the kernel's rule raise
    ("none": neither anywhere; "mixed": the two differ in more than one direction)"""
    ref = set(int(v) for v in rec["raised_nodes"]) & set(int(v) for v in c.listed())
    ker = set(int(v) for v in kernel_raising(c)[0])
    if not ref and not ker:
        return "none"
    if ref == ker:
        return "both"
    if ker < ref or (not ker and ref):
        return "reference" if not ker else "mixed"
    if ref < ker:
        return "kernel" if not ref else "mixed"
    return "mixed"


def compared_pairs(c, rec):
    """bool per pair: its distance is compared -- its node raises neither in the record nor by the
    kernel's rule, or (a kernel-only node) neither of its slots is one the rule names"""
    pp, d = c.pair_ptr(), c.degree
    ok = np.ones(int(pp[-1]), bool)
    _, mask = kernel_raising(c)
    for v in rec["raised_nodes"]:
        ok[pp[v]:pp[v + 1]] = False
    for v in np.nonzero(d >= 2)[0]:
        m = mask[c.ptr[v]:c.ptr[v + 1]]
        if m.any():
            i, j = np.tril_indices(int(d[v]), -1)
            ok[pp[v]:pp[v + 1]] &= ~(m[i] | m[j])
    return ok


def pair_rows(c):
    """(node, i, j) of every pair in node order, row-major lower triangle"""
    d = c.degree
    node, ii, jj = [], [], []
    for v in np.nonzero(d >= 2)[0]:
        i, j = np.tril_indices(int(d[v]), -1)
        node.append(np.full(i.size, v))
        ii.append(i)
        jj.append(j)
    z = np.zeros(0, np.int64)
    return (np.concatenate(node) if node else z, np.concatenate(ii) if ii else z, np.concatenate(jj) if jj else z)


def _bump(t, k, sign):
    e = D(1) + D(sign) * D(2) ** -24
    return tuple(CTX.multiply(x, e) if q == k else x for q, x in enumerate(t))


def exact_pairs(c, rec, geometry_of=None, sensitivity=True):
    """per pair: exact_kl (NaN where the pair is not compared) and, with `sensitivity`, the relative
    change of exact_kl when each of the two states' (X0, XB, MB) moves by a factor 1 +- 2^-24: the
    sum over the six numbers of the larger of the two one-sided changes (the worst combination of
    signs to first order), relative to |exact|. geometry_of(v, k) -> (X0, XB, MB) replaces the fp64
    inputs' exact geometry (the q32 path's de-quantised coordinates)."""
    pp, d = c.pair_ptr(), c.degree
    ok = compared_pairs(c, rec)
    ex = np.full(ok.size, np.nan)
    sens = np.full(ok.size, np.nan)
    for v in np.nonzero(d >= 2)[0]:
        if not ok[pp[v]:pp[v + 1]].any():
            continue
        nbs = c.nbs(v)
        geo = [geometry_of(v, k) if geometry_of else _geometry(c.gnn[v], nbs[k]) for k in range(int(d[v]))]
        bad = [g[0] == 0 or g[1] == 0 or g[0] == g[1] for g in geo]
        st = [None if b else _state(*g) for g, b in zip(geo, bad)]
        var = [None if b or not sensitivity else [(_state(*_bump(g, k, 1)), _state(*_bump(g, k, -1))) for k in range(3)]
               for g, b in zip(geo, bad)]
        i, j = np.tril_indices(int(d[v]), -1)
        for t, (a, b) in enumerate(zip(i, j)):
            p = int(pp[v]) + t
            if not ok[p] or bad[a] or bad[b]:
                continue
            e = _kl(st[a], st[b])
            ex[p] = float(e)
            if sensitivity:
                tot = D(0)
                for k in range(3):
                    tot += max(abs(_kl(var[a][k][0], st[b]) - e), abs(_kl(var[a][k][1], st[b]) - e))
                    tot += max(abs(_kl(st[a], var[b][k][0]) - e), abs(_kl(st[a], var[b][k][1]) - e))
                sens[p] = float(tot / abs(e)) if e != 0 else 0.0   # (an exact 0 -- two equal states -- is held exactly)
    return ex, sens


def rel_to_exact(a, ex):
    """|a - exact| / |exact| per pair (0 where both are 0), over the pairs with an exact value"""
    m = np.isfinite(ex)
    with np.errstate(all="ignore"):
        r = np.abs(np.asarray(a, np.float64)[m] - ex[m]) / np.abs(ex[m])
    r[(ex[m] == 0) & (np.asarray(a)[m] == 0)] = 0.0
    return r


@functools.lru_cache(maxsize=None)
def conditioning(name):
    """dict(exact [P], ref_err, sens): the record's largest distance from exact_kl relative to |exact|
    and the case's largest fp32 sensitivity; well = ref_err <= WELL, fp32 = sens <= FP32_SENS"""
    c, rec = BY_NAME[name], record()[name]
    ex, sens = exact_pairs(c, rec)
    r = rel_to_exact(rec["kl"], ex)
    ref_err = float(r.max()) if r.size else 0.0
    s = float(np.nanmax(sens)) if np.isfinite(ex).any() else 0.0
    return dict(exact=ex, ref_err=ref_err, sens=s, well=ref_err <= WELL, fp32=s <= FP32_SENS, n=int(np.isfinite(ex).sum()))


def value_cases():
    """the cases whose distances are held to exact_kl: every kind but the singular and moments ones,
    with at least one pair"""
    return [c for c in CASES if c.kind in VALUE_KINDS and record()[c.name]["kl"].size > 0]


def oracle_graph(c):
    """the fields of a TrackGraph that gtf_oracle.parabolic_training_rows reads, for a case"""
    import types
    dst = np.repeat(np.arange(c.n_nodes), c.degree)
    order = np.argsort(c.src, kind="stable")
    out_ptr = np.zeros(c.n_nodes + 1, np.int64)
    np.cumsum(np.bincount(c.src, minlength=c.n_nodes), out=out_ptr[1:])
    return types.SimpleNamespace(n_nodes=c.n_nodes, node={"gnn": c.gnn}, slot={"slot_src": c.src}, slot_ptr=c.ptr,
                                 slot_dst=lambda: dst, out_ptr=out_ptr, out_slot=order)
