"""Directed components for the fused pass (extrapolate -> update -> KL clustering), shared by
tests/golden/make_golden_pass_cases.py (the reference's own stage functions on every case),
test_pass_cases.py (CPU: the oracle and the C++ restatement against that record) and
test_gpu_pass_cases.py (GPU against the oracle, in every node-kernel configuration).

A case is one weakly connected component of a few nodes, built directly in the reference's
schema (a networkx DiGraph whose nodes carry ``track_state_estimates`` /
``updated_track_states`` / ``merged_state`` and whose edges carry ``activated``) by
:class:`Net`; ``gtf.graph.pack`` turns a list of them into a TrackGraph. Every case names the
stage it is for, the Params that differ from the defaults, and what it must reach: an error
bit at a named node, or a predicate on the oracle's output. States are set by hand where a
branch needs it (equal states, NaNs, dyadic numbers whose differences are exact); elsewhere the
numbers are physical, coordinates in mm on the layer radii of gtf.synth.

:func:`variants` instantiates a case unpadded and, for the node-kernel cases, with its
receiver ``v`` padded to every slot count of SIZES above its own: extra in-edges that are
inactive and carry no dict key, from senders without a merged state. The padding changes
nothing the reference computes, so the record of the unpadded case is the expectation of every
variant; it moves the receiver through the 4-, 6-, 8-, 12-, 16-, 32- and 64-lane groups and the
thread-per-node tail of the node kernel.
"""
import dataclasses
import functools
import math
import re

import networkx as nx
import numpy as np

import gtf_oracle as O
from gtf import graph
from gtf.params import Params

SIZES = (4, 6, 8, 12, 16, 32, 64, 65)
NAN = float("nan")
# the update stage as node ops (remove_state_metadata.py:31-53)
UPDATE_OPS = ("prune", "priors_tse", "priors_uts", "reweight_uts")


class Meas:
    """the attributes of the reference's GNN_Measurement that the stages read"""

    def __init__(self, x, y, z, r, node):
        self.x, self.y, self.z, self.r, self.node = x, y, z, r, node


def entry(sv, tau, cov5, xyzr, prior=None, mw=None, lik=None, lr=None, side=None):
    """one state-dict entry in the reference's schema; the parabolic and the joint covariance
    are one object, as the reference aliases them (helper.py:422-425)"""
    cov = graph.mat_from_cov5(cov5)
    x, y, z, r = (np.float64(c) for c in xyzr)   # (new objects: every NaN its own, as set() sees them)
    e = {"xy": (x, y), "zr": (z, r), "xyzr": (x, y, z, r),
         "edge_state_vector": np.array(sv, dtype=np.float64), "edge_covariance": cov,
         "joint_vector": [np.float64(sv[0]), np.float64(sv[1]), np.float64(tau)], "joint_vector_covariance": cov}
    if lik is not None:
        e["likelihood"] = np.float64(lik)
    if mw is not None:
        e["mixture_weight"] = np.float64(mw)
    if prior is not None:
        e["prior"] = np.float64(prior)
    if lr is not None:
        e["lr_layer_norm"] = lr
    if side is not None:
        e["side"] = side
    return e


SV0, COV0 = (1e-4, 0.02, 0.1), (1e-8, -4e-7, -4e-7, 1e-4, 1e-3)
KEYS = {"tse": "track_state_estimates", "uts": "updated_track_states"}


class Net:
    """one component under construction; node ids are base + the order of creation"""

    def __init__(self, base=0):
        self.G = nx.DiGraph()
        self.base = base
        self.names = {}
        self.pads = []
        self.no_send_mw = set()

    def hit_xyz(self, x, y, z, layer, name=None):
        n = self.base + self.G.number_of_nodes()
        x, y, z = np.float64(x), np.float64(y), np.float64(z)
        r = np.sqrt(x * x + y * y)
        self.G.add_node(n, GNN_Measurement=Meas(x, y, z, r, n), xyzr=(x, y, z, r), in_volume_layer_id=layer,
                        vivl_id=(8, layer), truth_particle=(n - self.base) % 2, translation=(x, y), tags=[n])
        if name:
            self.names[name] = n
        return n

    def hit(self, r, phi, z, layer, name=None):
        return self.hit_xyz(r * math.cos(phi), r * math.sin(phi), z, layer, name)

    def xyzr(self, n):
        return self.G.nodes[n]["xyzr"]

    def edge(self, u, v, act=1, back=True, back_act=1):
        """u -> v with 'activated' = act, and (back) v -> u"""
        self.G.add_edge(u, v, activated=act)
        if back:
            self.G.add_edge(v, u, activated=back_act)

    def merged(self, u, state, cov5, prior=1.0):
        a = self.G.nodes[u]
        a["merged_state"] = np.array(state, dtype=np.float64)
        a["merged_cov"] = graph.mat_from_cov5(cov5)
        a["merged_prior"] = prior

    def state(self, v, u, key, sv=SV0, tau=0.3, cov5=COV0, xyzr=None, **kw):
        """entry for key u in v's dict; xyzr: the stored coordinates (default: u's own)"""
        d = self.G.nodes[v].setdefault(KEYS[key], {})
        if key == "uts":
            kw.setdefault("lik", 1.0)
        kw.setdefault("mw", 1.0)
        kw.setdefault("prior", 1.0)
        d[u] = entry(sv, tau, cov5, self.xyzr(u) if xyzr is None else xyzr, **kw)

    def empty_dict(self, v, key):
        self.G.nodes[v].setdefault(KEYS[key], {})

    def pad(self, v, slots):
        """bring receiver v to `slots` slots with inactive, keyless in-edges from new senders
        that have no merged state (each holds one track_state_estimates key, v)"""
        a = self.G.nodes[v]
        have = set(self.G.predecessors(v))
        for k in KEYS.values():
            have |= set(a.get(k, {}))
        x, y, z, r = self.xyzr(v)
        phi = math.atan2(y, x)
        for i in range(slots - len(have)):
            p = self.hit(r - 40.0, phi + 0.05 + 0.002 * i, z - 20.0 - i, 2.0)
            self.G.add_edge(p, v, activated=0)
            self.state(p, v, "tse")
            self.pads.append(p)
        return self

    def finish(self):
        """every node without a state dict of its own (unless a case wants exactly that: see
        `bare`) gets one track_state_estimates key per neighbour: what a sender holds for its
        receivers (the mixture weight extrapolate_merged_states.py:384 reads)"""
        for n, a in self.G.nodes(data=True):
            if a.get("bare"):
                continue
            if "merged_state" in a or not any(k in a for k in KEYS.values()):
                nb = list(self.G.successors(n)) or list(self.G.predecessors(n))
                for w in nb:
                    d = a.setdefault(KEYS["tse"], {})
                    if w not in d and (n, w) not in self.no_send_mw:
                        self.state(n, w, "tse", mw=0.5)
            a.setdefault("degree", sum(1 for u in self.G.predecessors(n) if self.G[u][n]["activated"] == 1))
        return self.G


@dataclasses.dataclass
class Case:
    name: str
    stage: object                 # "extrapolate" | "update" | "cluster_uts" | "cluster_tse" | "full_pass" | tuple of node ops
    build: object                 # build(net): fills the component, names its nodes
    params: object = None         # Params overrides: dict, or callable(unpadded packed graph, names) -> dict
    err: object = None            # (bit, name of the raising node)
    check: object = None          # check(out, inp, ix, info): asserts what the case must reach on the oracle's output
    pad: bool = False             # instantiate at every slot count of SIZES
    ref: object = None            # None: pinned to the reference; else the reason it stays oracle-only
    tie_stop: bool = False        # raises GTF_ERR_TIE_EMPTIED and keeps the merged state formed so far
    exact: bool = False           # an input sits on a decision boundary on purpose: no noise envelope
    post: object = None           # post(g, ix): edit of the packed graph that the schema cannot express
    running: bool = False         # a running-covariance case (the chi2 sensitivity check)


def stage_key(case):
    return case.stage if isinstance(case.stage, str) else "ops:" + ",".join(case.stage)


# --------------------------------------------------------------------------- geometry
RL = {2.0: 32.0, 4.0: 72.0, 6.0: 116.0, 8.0: 172.0}   # layer id -> radius (mm)
PHI0 = 0.30


def on_parabola(net, u, state, s, dy=0.0, z=None, layer=6.0, name=None):
    """a hit at distance s along sender u's radial direction, on the parabola y' = a x'^2 + b x' + c
    of `state` in u's frame, moved dy mm across it"""
    x, y, zu, _ = net.xyzr(u)
    phi = math.atan2(y, x)
    a, b, c = state
    yp = a * s * s + b * s + c + dy
    gx = x + s * math.cos(phi) - yp * math.sin(phi)
    gy = y + s * math.sin(phi) + yp * math.cos(phi)
    return net.hit_xyz(gx, gy, zu + 0.45 * s if z is None else z, layer, name)


# the default regime
MS0, MC0 = (2e-3, 0.09, 0.0), (1e-10, 0.0, 0.0, 1e-6, 1e-2)
# the scattering regime: sigma0xy and the sender's covariance so small that one edge's var_ms
# (~6e-12 at a = 2e-4) moves the chi2 of every later out-edge by about a percent
SCAT = dict(sigma0xy=1e-3)
MS1, MC1 = (2e-4, 9e-3, 0.0), (1e-16, 0.0, 0.0, 1e-12, 1e-8)
ACCEPT, REJECT = 0.5, 20.0   # the chi2 a case gives its accepted and rejected edges (chi2_cut = 2)


def _solve(f, x0, h, target):
    """x above the minimum of the near-quadratic f with f(x) = target: the vertex from two rounds of
    three probes, then the secant on sqrt(f)"""
    A = 1.0
    for step in (h, 0.05 * h):
        q = [f(x0 - step), f(x0), f(x0 + step)]
        A = (q[0] + q[2] - 2.0 * q[1]) / (2.0 * step * step)
        x0 -= (q[2] - q[0]) / (2.0 * step) / (2.0 * A)
    x = x0 + math.sqrt(target / A)
    for _ in range(6):
        x = x0 + (x - x0) * math.sqrt(target / f(x))
    assert abs(f(x) - target) < 0.02 * target, (f(x), target)   # (near enough: the case states the side of the cut)
    return x


def _chi2(gu, gv, state, cov5, sig):
    """the xy chi2 of extrapolating `state` from coordinates gu to gv: the oracle's own function"""
    r = O.extrapolate_validate(np.asarray(gu, float), np.asarray(gv, float), np.array(state, float),
                               graph.mat_from_cov5(cov5), -1.0, sig, 0.4, 0.6, 550.0)[2]
    return float(np.ravel(r)[0])


def place(net, u, state, cov5, chi2, sig=0.3, z=None, layer=6.0, name=None, dy=0.3):
    """a hit along sender u's radial direction (dy mm across it), so far out that the extrapolation of
    `state` (covariance cov5) from u has the xy chi2 `chi2`. The extrapolated offset F.state hardly
    sees where the hit lies across the track; it is about -a s (s - b / a) at distance s, so MS0 and MS1
    put its zero near s = 45 mm and the distance sets the chi2."""
    x, y, zu, _ = net.xyzr(u)
    phi = math.atan2(y, x)

    def at(s):
        return x + s * math.cos(phi) - dy * math.sin(phi), y + s * math.sin(phi) + dy * math.cos(phi)

    def f(s):
        gx, gy = at(s)
        return _chi2(net.xyzr(u), (gx, gy, zu + 0.45 * s if z is None else z, math.hypot(gx, gy)), state, cov5, sig)
    s = _solve(f, state[1] / state[0], 1.0, chi2)
    gx, gy = at(s)
    return net.hit_xyz(gx, gy, zu + 0.45 * s if z is None else z, layer, name)


def aim(net, u, v, chi2, a=2e-4, c=0.0, cov5=MC0, sig=0.3):
    """the merged state (a, b, c) of sender u whose extrapolation to the existing hit v has the xy chi2
    `chi2`: b solved the same way"""
    b = _solve(lambda b: _chi2(net.xyzr(u), net.xyzr(v), (a, b, c), cov5, sig), 0.0, 1e-2, chi2)
    net.merged(u, (a, b, c), cov5)


def _slot(g, v, u):
    lo, hi = int(g.slot_ptr[v]), int(g.slot_ptr[v + 1])
    k = lo + np.nonzero(g.slot["slot_src"][lo:hi] == u)[0]
    assert k.size == 1, (v, u)
    return int(k[0])


# --------------------------------------------------------------------------- extrapolation cases
def _ex_pair(net, merged=True, act=1, state=MS0, cov=MC0, chi2=ACCEPT, zu=30.0, zv=None, sig=0.3):
    u = net.hit(72.0, PHI0, zu, 4.0, "u")
    if chi2 is None or np.isnan(state).any():
        v = on_parabola(net, u, MS0, 44.0, 0.7, z=zv, name="v")
    else:
        v = place(net, u, state, cov, chi2, sig, z=zv, name="v")
    net.edge(u, v, act=act)
    if merged:
        net.merged(u, state, cov)
    return u, v


def _b_not_merged(net):
    _ex_pair(net, merged=False)


def _c_nothing_sent(out, inp, ix, info):
    v, u = ix("v"), ix("u")
    assert out.node["has_uts"][v] == 0 and out.slot["act"][_slot(out, v, u)] == inp.slot["act"][_slot(inp, v, u)]
    assert np.array_equal(out.node["merged_cov"][u], inp.node["merged_cov"][u], equal_nan=True)


def _b_inactive_edge(net):
    _ex_pair(net, act=0)


def _b_accept_reject(net):
    u = net.hit(72.0, PHI0, 30.0, 4.0, "u")
    v = place(net, u, MS0, MC0, ACCEPT, name="v")
    w = place(net, u, MS0, MC0, REJECT, name="w", dy=-0.4)
    net.edge(u, v)
    net.edge(u, w)
    net.merged(u, MS0, MC0)


def _c_accept_reject(out, inp, ix, info):
    u, v, w = ix("u"), ix("v"), ix("w")
    kv, kw = _slot(out, v, u), _slot(out, w, u)
    assert out.slot["act"][kv] == 1 and out.slot["uts_rank"][kv] == 0 and out.node["has_uts"][v] == 1
    assert out.slot["act"][kw] == 0 and out.slot["uts_rank"][kw] < 0 and out.node["has_uts"][w] == 0
    assert info["chi2"][kv] < 2.0 < info["chi2"][kw]
    assert out.node["merged_cov"][u][3] > inp.node["merged_cov"][u][3]


def _b_zero_state(net):
    _ex_pair(net, state=(0.0, 0.0, 0.0), chi2=None)


def _c_zero_state(out, inp, ix, info):
    k = _slot(out, ix("v"), ix("u"))
    assert info["chi2"][k] == 0.0 and out.slot["act"][k] == 1 and out.slot["uts_rank"][k] == 0


def _b_nan_state(net):
    _ex_pair(net, state=(2e-4, NAN, 0.0))


def _c_nan_state(out, inp, ix, info):
    k = _slot(out, ix("v"), ix("u"))
    assert np.isnan(info["chi2"][k]) and out.slot["act"][k] == 0 and out.slot["uts_rank"][k] < 0


def _b_send_mw_accept(net):
    u, v = _ex_pair(net)
    net.no_send_mw.add((u, v))
    net.empty_dict(u, "tse")   # (the sender holds a dict, without the receiver's key)


def _b_send_mw_reject(net):
    u, v = _ex_pair(net, chi2=REJECT)
    net.no_send_mw.add((u, v))
    net.empty_dict(u, "tse")


def _c_rejected(out, inp, ix, info):
    k = _slot(out, ix("v"), ix("u"))
    assert info["chi2"][k] > 2.0 and out.slot["act"][k] == 0 and np.isnan(inp.slot["send_mw"][k])


BOUNDARY = 550.0
ZS = {"below": 549.99, "at": BOUNDARY, "above": 550.01}


def _b_endcap(zu, zv):
    def build(net):
        _ex_pair(net, state=MS1, cov=MC1, zu=-zu, zv=zv, sig=1e-3)   # (|z|: the sender sits on the negative side)
    return build


def _c_endcap(su, sv):
    def check(out, inp, ix, info):
        u, v = ix("u"), ix("v")
        k = _slot(out, v, u)
        assert out.slot["act"][k] == 1 and out.slot["uts_rank"][k] == 0
        gu, gv = inp.node["gnn"][u], inp.node["gnn"][v]
        assert (abs(gu[2]) >= BOUNDARY) == (su != "below") and (abs(gv[2]) >= BOUNDARY) == (sv != "below")
        # the sender's swap and tan_t, the neighbour's swap: each visible far above 1e-6 in c22 or merged_cov[1, 1]
        dr, dz = gv[3] - gu[3], gv[2] - gu[2]
        s = {False: (0.4, 0.6), True: (0.6, 0.4)}   # (sigma_r, sigma_z) barrel / endcap
        (sr, sz), (srn, szn) = s[su != "below"], s[sv != "below"]
        vt = (sz * sz + szn * szn) / dr ** 2 + (dz / dr ** 2) ** 2 * (sr * sr + srn * srn)
        var_ms = out.node["merged_cov"][u][3] - inp.node["merged_cov"][u][3]
        assert abs(out.slot["uts_cov"][k][4] - (vt + var_ms)) <= 1e-9 * vt
        other = (sr * sr + szn * szn) / dr ** 2 + (dz / dr ** 2) ** 2 * (sz * sz + srn * srn)
        assert abs(other - vt) > 1e-2 * vt
    return check


def _b_running(n):
    """one sender with n out-edges: active and accepted, inactive, active and rejected, in turn"""
    def build(net):
        u = net.hit(72.0, PHI0, 30.0, 4.0, "u")
        net.merged(u, MS1, MC1)
        for i in range(n):
            kind = i % 3 if n > 1 else 0
            w = place(net, u, MS1, MC1, 15.0 + i % 5 if kind == 2 else 0.3 + (i % 7) / 14.0, 1e-3, z=50.0 + 2.0 * i,
                      name="w%d" % i, dy=0.01 * i)
            net.edge(u, w, act=0 if kind == 1 else 1)
    return build


def _c_running(n):
    def check(out, inp, ix, info):
        u = ix("u")
        for i in range(n):
            kind = i % 3 if n > 1 else 0
            k = _slot(out, ix("w%d" % i), u)
            if kind == 1:
                assert np.isnan(info["chi2"][k]) and out.slot["act"][k] == 0
            else:
                assert (info["chi2"][k] <= 2.0) == (kind == 0), (i, info["chi2"][k])
                assert out.slot["act"][k] == (1 if kind == 0 else 0)
    return check


def _b_ranks_gap(net):
    """receiver v already holds keys A and B (ranks 0 and 3 after `post`); A's sender extrapolates
    again (rewritten), C and D are new, B's sender has no merged state. B's stored x is D's
    live x: one class of equal x across a snapshot and a live coordinate."""
    v = net.hit(116.0, PHI0, 50.0, 6.0, "v")
    su = []
    for i, nm in enumerate("ABCD"):
        u = net.hit(72.0, PHI0 + 0.002 * (i - 1.5), 30.0 + i, 4.0, nm)
        su.append(u)
    for i, (nm, u) in enumerate(zip("ABCD", su)):
        if nm != "B":
            aim(net, u, v, 0.3 * (i + 1))
        net.edge(u, v)
    net.state(v, su[0], "uts", sv=(1e-4, 0.03, 0.0), prior=0.5, mw=0.4, lik=0.9, lr=1, side="left")
    xd = net.xyzr(su[3])
    net.state(v, su[1], "uts", sv=(3e-4, 0.01, 0.0), xyzr=(xd[0], 20.0, 31.0, 70.0), prior=0.5, mw=0.6, lik=0.8, lr=1,
              side="left")


def _p_ranks_gap(g, ix):
    k = _slot(g, ix("v"), ix("B"))
    assert g.slot["uts_rank"][k] == 1
    g.slot["uts_rank"][k] = 3


def _c_ranks_gap(out, inp, ix, info):
    v = ix("v")
    r = {nm: int(out.slot["uts_rank"][_slot(out, v, ix(nm))]) for nm in "ABCD"}
    assert r == {"A": 0, "B": 3, "C": 4, "D": 5}, r
    f = {nm: int(out.slot["uts_fresh"][_slot(out, v, ix(nm))]) for nm in "ABCD"}
    assert f == {"A": 1, "B": 0, "C": 1, "D": 1}, f
    kb, kd = _slot(out, v, ix("B")), _slot(out, v, ix("D"))
    assert out.slot["uts_xyzr"][kb][0] == out.slot["uts_xyzr"][kd][0]


# --------------------------------------------------------------------------- priors, side norm, reweight, prune
def _uts_star(net, keys, node_x=None):
    """receiver v and one sender per key, in dict order. A key is a dict: layer (4 inner / 8 outer),
    act (1), edge (True: sender -> v exists), rev (True: v -> sender exists), x (stored x override),
    and entry fields (mw, lik, prior, ...)"""
    v = net.hit(116.0, PHI0, 50.0, 6.0, "v")
    for i, kd in enumerate(keys):
        kd = dict(kd)
        layer = kd.pop("layer", 4.0)
        act, edge, rev, x = kd.pop("act", 1), kd.pop("edge", True), kd.pop("rev", True), kd.pop("x", None)
        u = net.hit(RL[layer], PHI0 + 0.003 * (i - len(keys) / 2.0), 50.0 + (RL[layer] - 116.0) * 0.45 + i, layer, "k%d" % i)
        assert edge or rev, "a key without either edge would leave the component"
        if edge:
            net.edge(u, v, act=act, back=rev)
        else:
            net.G.add_edge(v, u, activated=1)
        xyzr = list(net.xyzr(u))
        if x is not None:
            xyzr[0] = x
        kd.setdefault("mw", 0.5 + 0.05 * i)
        kd.setdefault("lik", 0.8 - 0.03 * i)
        net.state(v, u, "uts", sv=(1e-4 * (1 + i), 0.02, 0.1), xyzr=xyzr, **kd)
    return v


def _keys(out, ix, n, f):
    v = ix("v")
    return [out.slot[f][_slot(out, v, ix("k%d" % i))] for i in range(n)]


def _b_one_layer(net):
    _uts_star(net, [{}, {}, {"act": 0, "prior": 0.77}, {}])


def _c_one_layer(out, inp, ix, info):
    assert _keys(out, ix, 4, "uts_prior") == [1 / 3, 1 / 3, 0.77, 1 / 3]
    lr = _keys(out, ix, 4, "uts_lr")
    assert lr[0] == lr[1] == lr[3] == 3.0 and np.isnan(lr[2])


def _b_two_layers(net):
    _uts_star(net, [{}, {"layer": 8.0}, {}, {"layer": 8.0}, {"layer": 8.0, "act": 0, "prior": 0.6}, {}])


def _c_two_layers(out, inp, ix, info):
    assert _keys(out, ix, 6, "uts_prior") == [1 / 3, 0.5, 1 / 3, 0.5, 0.6, 1 / 3]
    assert _keys(out, ix, 6, "uts_side")[:4] == [0, 1, 0, 1]
    assert _keys(out, ix, 6, "uts_lr")[:4] == [3.0, 2.0, 3.0, 2.0]


def _b_repeated_x(net):
    _uts_star(net, [{"x": 60.0}, {"layer": 8.0}, {"x": 60.0}, {"x": 61.0}, {"x": 60.0}])


def _c_repeated_x(out, inp, ix, info):
    assert _keys(out, ix, 5, "uts_lr") == [2.0, 1.0, 2.0, 2.0, 2.0]


def _b_last_inactive(net):
    _uts_star(net, [{}, {"layer": 8.0}, {}, {"act": 0}])


def _c_last_inactive(out, inp, ix, info):
    assert _keys(out, ix, 4, "uts_lr")[:3] == [1.0, 1.0, 1.0]
    assert _keys(out, ix, 4, "uts_side")[:3] == [0, 1, 0]


def _b_last_no_edge(net):
    _uts_star(net, [{}, {"layer": 8.0}, {"edge": False}])


def _b_last_no_edge_right(net):
    _uts_star(net, [{"layer": 8.0}, {"layer": 8.0}, {"edge": False}])


def _b_none_active_last_no_edge(net):
    _uts_star(net, [{"act": 0}, {"layer": 8.0, "act": 0}, {"edge": False}])


def _c_unchanged_mw(out, inp, ix, info):
    v = ix("v")
    lo, hi = int(out.slot_ptr[v]), int(out.slot_ptr[v + 1])
    assert np.array_equal(out.slot["uts_mw"][lo:hi], inp.slot["uts_mw"][lo:hi], equal_nan=True)
    assert np.array_equal(out.slot["act"][lo:hi], inp.slot["act"][lo:hi])


def _b_x_equal(net):
    _uts_star(net, [{}, {"x": 116.0 * math.cos(PHI0)}, {}])


def _c_x_equal(out, inp, ix, info):
    assert inp.slot["uts_xyzr"][_slot(inp, ix("v"), ix("k1"))][0] == inp.node["gnn"][ix("v")][0]
    assert _keys(out, ix, 3, "uts_side") == [0, 1, 0] and _keys(out, ix, 3, "uts_lr") == [2.0, 1.0, 2.0]


def _b_nan_x(net):
    _uts_star(net, [{}, {"x": NAN}, {"x": NAN}, {"layer": 8.0}, {"layer": 8.0, "x": 150.0}])


def _c_nan_x(out, inp, ix, info):
    assert _keys(out, ix, 5, "uts_side") == [0, 1, 1, 1, 1] and _keys(out, ix, 5, "uts_lr") == [1.0, 4.0, 4.0, 4.0, 4.0]


def _b_thr_tenth(net):
    """ten active keys, each alone on its layer (prior 1), one stored x, mw = lik = 1: the denominator is
    exactly 10 and every w exactly 1 / 10 = 0.1, the reference's own hard-coded threshold (helper.py:145)"""
    v = net.hit(116.0, PHI0, 50.0, 6.0, "v")
    for i in range(10):
        u = net.hit(72.0, PHI0 + 0.003 * (i - 5), 30.0 + i, 100.0 + i, "k%d" % i)
        net.edge(u, v)
        xyzr = list(net.xyzr(u))
        xyzr[0] = 60.0
        net.state(v, u, "uts", xyzr=xyzr, mw=1.0, lik=1.0)


def _c_thr_tenth(out, inp, ix, info):
    assert _keys(out, ix, 10, "uts_mw") == [0.1] * 10 and _keys(out, ix, 10, "act") == [1] * 10


def _b_thr_one(net):
    _uts_star(net, [{"mw": 0.3, "lik": 0.7}, {"act": 0}])


def _c_thr_one(out, inp, ix, info):
    assert _keys(out, ix, 2, "uts_mw")[0] == 1.0 and _keys(out, ix, 2, "act") == [1, 0]


def _b_thr_quarter(net):
    _uts_star(net, [{"mw": 1.0, "lik": 1.0, "x": 60.0}, {"mw": 1.0, "lik": 1.0, "x": 60.0}])


def _c_thr_quarter(active):
    def check(out, inp, ix, info):
        assert _keys(out, ix, 2, "uts_mw") == [0.25, 0.25] and _keys(out, ix, 2, "act") == [active] * 2
    return check


def _b_prune(net):
    _uts_star(net, [{}, {"rev": False}, {"layer": 8.0}])


def _c_prune(out, inp, ix, info):
    assert [r >= 0 for r in _keys(out, ix, 3, "uts_rank")] == [True, False, True]
    assert _keys(out, ix, 3, "uts_prior")[0] == 1.0     # (the pruned key's edge is still active: it takes no prior)
    assert _keys(out, ix, 3, "uts_lr")[0] == 1.0


def _b_prune_last(net):
    """the last key has an in-edge but no way back: the first reweight is clean and caches it as the
    last key; pruning removes it, and the new last key has a way back but no in-edge"""
    _uts_star(net, [{}, {"layer": 8.0}, {"edge": False}, {"rev": False}])


def _b_no_dict(net):
    v = _uts_star(net, [{}, {"layer": 8.0}])
    b = net.hit(172.0, PHI0 + 0.01, 80.0, 8.0, "bare")
    net.G.nodes[b]["bare"] = True
    net.edge(b, v, act=0)


def _b_empty_uts(solo):
    def build(net):
        v = net.hit(116.0, PHI0, 50.0, 6.0, "v")
        net.empty_dict(v, "uts")
        net.empty_dict(v, "tse")
        if not solo:
            net.edge(net.hit(72.0, PHI0, 30.0, 4.0), v)
    return build


def _c_solo(out, inp, ix, info):
    assert out.n_nodes == 1 and out.node["has_uts"][0] == 1 and out.node["has_merged"][0] == 0


# --------------------------------------------------------------------------- clustering cases
def _dyadic_cov():
    return (2.0 ** -20, 0.0, 0.0, 2.0 ** -10, 2.0 ** -8)


def _cl_star(net, key, states, same_xyzr=False):
    """receiver v with one key per state in dict `key`; a state is a dict of entry fields (sv, tau, cov5,
    prior). same_xyzr: every key stores one coordinate tuple (the tau term of every pair is exactly 0)"""
    v = net.hit(116.0, PHI0, 50.0, 6.0, "v")
    d = len(states)
    shared = None
    for i, st in enumerate(states):
        st = dict(st)
        layer = 4.0 if i % 2 == 0 else 8.0
        u = net.hit(RL[layer], PHI0 + 0.003 * (i - d / 2.0), 50.0 + (RL[layer] - 116.0) * 0.45 + 0.3 * i, layer, "k%d" % i)
        net.edge(u, v)
        xyzr = st.pop("xyzr", None)
        if same_xyzr:
            shared = shared or net.xyzr(u)
            xyzr = shared
        st.setdefault("prior", 1.0 / d)
        net.state(v, u, key, xyzr=xyzr, **st)
    return v


def _distinct(d):
    return [dict(sv=(1e-4 * (1 + 0.3 * i), 0.02 * (1 + 0.1 * i), 0.05 * i), tau=0.45 + 0.01 * i,
                 cov5=(1e-8 * (1 + i / 8.0), -4e-7, -4e-7, 1e-4 * (1 + i / 16.0), 1e-3 * (1 + i / 4.0))) for i in range(d)]


def _b_count(key, d):
    return lambda net: _cl_star(net, key, _distinct(d))


def _c_count(d):
    def check(out, inp, ix, info):
        assert int(out.node["has_merged"][ix("v")]) == (1 if 2 < d < 16 else 0)
    return check


def _b_identical(key):
    return lambda net: _cl_star(net, key, [_distinct(1)[0]] * 3, same_xyzr=True)


def _b_zero_pair(key):
    """keys 0 and 1 are one state at one stored coordinate (distance exactly 0, far below every other);
    the merged pair is the closest of the others"""
    def build(net):
        st = _distinct(5)
        st[1] = dict(st[0])
        v = _cl_star(net, key, st)
        e = net.G.nodes[v][KEYS[key]]
        k0, k1 = net.names["k0"], net.names["k1"]
        e[k1]["xyzr"] = e[k0]["xyzr"]
        e[k1]["xy"], e[k1]["zr"] = e[k0]["xy"], e[k0]["zr"]
    return build


def _c_zero_pair(pfx):
    def check(out, inp, ix, info):
        order, D = distances(inp, ix("v"), Params(), pfx)
        assert D[1][0] == 0.0 and np.count_nonzero(D) == 9
        assert out.node["has_merged"][ix("v")] == 1
        # merged with a threshold that lets nothing else in: the merged pair alone stays active
        act = _keys(out, ix, 5, "act")
        nz = D[np.nonzero(D)]
        r, c = np.where(D == nz.min())
        assert sorted(np.nonzero(act)[0].tolist()) == sorted([int(r[0]), int(c[0])]) and {int(r[0]), int(c[0])} != {0, 1}
    return check


def _b_nan_cov(key):
    def build(net):
        st = _distinct(4)
        st[2]["cov5"] = (1e-8, NAN, -4e-7, 1e-4, 1e-3)
        _cl_star(net, key, st)
    return build


def _c_no_merge(out, inp, ix, info):
    v = ix("v")
    assert out.node["has_merged"][v] == 0
    lo, hi = int(out.slot_ptr[v]), int(out.slot_ptr[v + 1])
    assert np.array_equal(out.slot["act"][lo:hi], inp.slot["act"][lo:hi])


def _b_nan_c22(key):
    """the closest pair is (0, 1); key 3's c22 is NaN: its pairwise distances read only the [a, b] block"""
    def build(net):
        st = _distinct(4)
        st[1]["sv"] = tuple(np.array(st[0]["sv"]) * (1 + 1e-3))
        st[3]["cov5"] = st[3]["cov5"][:4] + (NAN,)
        _cl_star(net, key, st, same_xyzr=True)
    return build


def _dy(a, prior=0.125):
    return dict(sv=(a * 2.0 ** -10, 0.0, 0.0), tau=0.5, cov5=_dyadic_cov(), prior=prior)


def _b_tie(key, avals):
    return lambda net: _cl_star(net, key, [_dy(a) for a in avals], same_xyzr=True)


def _c_tie(rows, cols, merged_rest):
    """the minimum is reached at exactly (rows[i], cols[i]); every listed key leaves the list"""
    def check(out, inp, ix, info, pfx=None):
        v = ix("v")
        pfx = "uts" if inp.node["has_uts"][v] else "tse"
        order, D = distances(inp, v, Params(), pfx)
        nz = D[np.nonzero(D)]
        r, c = np.where(D == nz.min())
        assert r.tolist() == rows and c.tolist() == cols, (r, c)
        assert out.node["has_merged"][v] == 1
        if merged_rest is not None:
            assert _keys(out, ix, len(order), "act") == merged_rest
    return check


def _b_kl_all(key):
    return lambda net: _cl_star(net, key, _distinct(7))


def _c_kl_all(out, inp, ix, info):
    assert out.node["has_merged"][ix("v")] == 1 and _keys(out, ix, 7, "act") == [1] * 7
    assert abs(out.node["merged_prior"][ix("v")] - 1.0) < 1e-12


def _b_kl_equal(key):
    """keys 2 and 3 are one state (every key stores one coordinate): after (0, 1) merge, their KL distances to the
    merged state are equal and the first of them is taken"""
    def build(net):
        st = _distinct(4)
        st[1]["sv"] = tuple(np.array(st[0]["sv"]) * (1 + 1e-3))
        st[3] = dict(st[2])
        _cl_star(net, key, st, same_xyzr=True)
    return build


def _p_kl_equal(g, names):
    """cluster_kl between the first KL minimum (twice in the list) and the next round's"""
    tr = trace(g, names["v"])
    assert tr["kl"][0].count(min(tr["kl"][0])) == 2 and len(tr["kl"]) >= 2
    a, b = min(tr["kl"][0]), min(tr["kl"][1])
    assert b > a * 1.01
    return dict(cluster_kl=0.5 * (a + b))


def _c_kl_equal(out, inp, ix, info):
    assert _keys(out, ix, 4, "act") == [1, 1, 1, 0]


def _p_chi2(f):
    return lambda g, names: dict(cluster_chi2=f * trace(g, names["v"])["chi2"], cluster_kl=1e-30)


def _p_kl(f):
    return lambda g, names: dict(cluster_kl=f * min(trace(g, names["v"])["kl"][0]))


def _c_merged(lo, hi):
    """the number of v's five in-edges that stay active is in [lo, hi]; 5 and no merged state: no merge"""
    def check(out, inp, ix, info):
        n = sum(_keys(out, ix, 5, "act"))
        assert lo <= n <= hi, n
        assert out.node["has_merged"][ix("v")] == (0 if lo == 5 else 1)
    return check


# --------------------------------------------------------------------------- full pass
def _b_full(net):
    """two layers of merged senders into a middle layer of receivers that hold earlier keys: every
    stage of the pass has work, and v ends with three keys to cluster"""
    v = net.hit(116.0, PHI0, 50.0, 6.0, "v")
    for i in range(4):
        layer = 4.0 if i % 2 == 0 else 8.0
        u = net.hit(RL[layer], PHI0 + 0.0015 * (i - 1.5), 50.0 + 0.45 * (RL[layer] - 116.0) + 0.2 * i, layer, "k%d" % i)
        aim(net, u, v, (0.2, 0.5, 0.9, REJECT)[i])
        net.edge(u, v)


def _c_full(out, inp, ix, info):
    v = ix("v")
    assert [r >= 0 for r in _keys(out, ix, 4, "uts_rank")] == [True, True, True, False]
    assert out.node["has_merged"][v] == 1


def _b_full_prune_last(net):
    """the pass's own reweights cache v's last key (it has an in-edge, no way back); the update stage
    prunes it and the key before it has no in-edge: the last reweight raises"""
    v = _uts_star(net, [{}, {"layer": 8.0}, {"edge": False}, {"rev": False}])
    u = net.names["k0"]   # (its key is rewritten in place: the dict's last key stays the one pruning removes)
    aim(net, u, v, ACCEPT)


# --------------------------------------------------------------------------- the list
def _cases():
    C = []
    X = "extrapolate"
    C += [Case("ex_not_merged", X, _b_not_merged, check=_c_nothing_sent),
          Case("ex_inactive_edge", X, _b_inactive_edge, check=_c_nothing_sent),
          Case("ex_accept_reject", X, _b_accept_reject, check=_c_accept_reject),
          Case("ex_zero_state_cut0", X, _b_zero_state, params=dict(chi2_cut=0.0), check=_c_zero_state),
          Case("ex_nan_state", X, _b_nan_state, check=_c_nan_state),
          Case("ex_send_mw_nan_accepted", X, _b_send_mw_accept, err=(1, "v")),
          Case("ex_send_mw_nan_rejected", X, _b_send_mw_reject, check=_c_rejected)]
    for su, zu in ZS.items():
        for sv, zv in ZS.items():
            C.append(Case("ex_endcap_%s_%s" % (su, sv), X, _b_endcap(zu, zv), params=SCAT, check=_c_endcap(su, sv),
                          exact="at" in (su, sv)))
    for n in (1, 8, 9, 16, 17, 64, 65):
        C.append(Case("ex_running_%d" % n, X, _b_running(n), params=SCAT, check=_c_running(n), running=True))
    C.append(Case("ex_ranks_gap", X, _b_ranks_gap, check=_c_ranks_gap, post=_p_ranks_gap, pad=True, exact=True))

    U = "update"
    no_thr = "the reference hard-codes reweight_threshold = 0.1 (helper.py:145)"
    C += [Case("rw_one_layer", U, _b_one_layer, check=_c_one_layer, pad=True),
          Case("rw_two_layers", U, _b_two_layers, check=_c_two_layers, pad=True),
          Case("rw_repeated_x_left", U, _b_repeated_x, check=_c_repeated_x, pad=True),
          Case("rw_last_inactive", U, _b_last_inactive, check=_c_last_inactive, pad=True),
          Case("rw_last_no_edge", U, _b_last_no_edge, err=(2, "v"), pad=True),
          Case("rw_last_no_edge_right_side", U, _b_last_no_edge_right, err=(2, "v"), pad=True),
          Case("rw_none_active_last_no_edge", U, _b_none_active_last_no_edge, check=_c_unchanged_mw, pad=True),
          Case("rw_x_equal_node_x", U, _b_x_equal, check=_c_x_equal, pad=True, exact=True),
          Case("rw_nan_x", U, _b_nan_x, check=_c_nan_x, pad=True),
          Case("rw_w_equals_reference_threshold", U, _b_thr_tenth, check=_c_thr_tenth, pad=True),
          Case("rw_w_one_threshold_one", U, _b_thr_one, params=dict(reweight_threshold=1.0), check=_c_thr_one,
               pad=True, ref=no_thr),
          Case("rw_w_quarter_threshold_quarter", U, _b_thr_quarter, params=dict(reweight_threshold=0.25),
               check=_c_thr_quarter(1), pad=True, ref=no_thr),
          Case("rw_w_quarter_threshold_ulp_above", U, _b_thr_quarter,
               params=dict(reweight_threshold=float(np.nextafter(0.25, 1.0))), check=_c_thr_quarter(0), pad=True,
               ref=no_thr),
          Case("prune_no_rev_edge", U, _b_prune, check=_c_prune, pad=True),
          Case("prune_last_key_then_stale", ("reweight_uts",) + UPDATE_OPS, _b_prune_last, err=(2, "v"), pad=True),
          Case("no_state_dict", U, _b_no_dict, err=(64, "bare")),
          Case("empty_uts_dict_two_nodes", "cluster_uts", _b_empty_uts(False), err=(16, "v"), pad=True),
          Case("empty_uts_dict_solo", "cluster_uts", _b_empty_uts(True), check=_c_solo)]

    for key in ("uts", "tse"):
        S = "cluster_" + key
        nm = lambda s: "cl_%s_%s" % (key, s)   # noqa: E731
        for d in (2, 3, 15, 16):
            C.append(Case(nm("d%d" % d), S, _b_count(key, d), check=_c_count(d), pad=True))
        C += [Case(nm("three_identical"), S, _b_identical(key), err=(4, "v"), pad=True),
              Case(nm("zero_pair"), S, _b_zero_pair(key), params=dict(cluster_kl=1e-30), check=_c_zero_pair(key), pad=True),
              Case(nm("nan_pair_distance"), S, _b_nan_cov(key), check=_c_no_merge, pad=True),
              Case(nm("nan_kl"), S, _b_nan_c22(key), err=(32, "v"), pad=True),
              # |a1 - a0| = |a3 - a2|: rows (1, 3), cols (0, 2); keys 4 and 5 stay in the list
              Case(nm("tie_two_way"), S, _b_tie(key, (0, 0.25, 1, 1.25, 4, 8)), params=dict(cluster_kl=1e-30),
                   check=_c_tie([1, 3], [0, 2], [1, 1, 1, 1, 0, 0]), pad=True),
              # |a2 - a0| = |a2 - a1|: rows (2, 2): key 2 merges with itself
              Case(nm("tie_shared_row"), S, _b_tie(key, (-0.25, 0.25, 0, 4, 8)), params=dict(cluster_kl=1e-30),
                   check=_c_tie([2, 2], [0, 1], [1, 1, 1, 0, 0]), pad=True),
              Case(nm("tie_empties_list"), S, _b_tie(key, (0, 0.25, 1, 1.25)), err=(8, "v"), tie_stop=True, pad=True),
              Case(nm("kl_merges_all"), S, _b_kl_all(key), params=dict(cluster_kl=1e30), check=_c_kl_all, pad=True),
              Case(nm("kl_equal_minima"), S, _b_kl_equal(key), params=_p_kl_equal, check=_c_kl_equal, pad=True)]
        for side, f in (("below", 1 - 1e-3), ("above", 1 + 1e-3)):
            C.append(Case(nm("chi2_threshold_" + side), S, lambda net, key=key: _cl_star(net, key, _distinct(5)),
                          params=_p_chi2(f), check=_c_merged(*((5, 5) if side == "below" else (2, 2))), pad=True))
            C.append(Case(nm("kl_threshold_" + side), S, lambda net, key=key: _cl_star(net, key, _distinct(5)),
                          params=_p_kl(f), check=_c_merged(*((2, 2) if side == "below" else (3, 5))), pad=True))
    C += [Case("full_pass_three_keys", "full_pass", _b_full, check=_c_full, pad=True),
          Case("full_pass_prune_last_key", "full_pass", _b_full_prune_last, err=(2, "v"), pad=True)]
    assert len(set(c.name for c in C)) == len(C)
    return C


# --------------------------------------------------------------------------- distances of a node's dict
def distances(g, v, p, pfx="tse"):
    """the pairwise chi2 matrix of node v's dict (clustering.py:80-86) and its keys in dict order"""
    S = g.slot
    order = O._dict_order(g, pfx, v)
    jsv = np.array([[S[pfx + "_sv"][k][0], S[pfx + "_sv"][k][1], S[pfx + "_tau"][k]] for k in order])
    jcov = np.array([O.mat_from_cov5(S[pfx + "_cov"][k]) for k in order])
    xyzr = np.array([S[pfx + "_xyzr"][k] for k in order])
    D = np.zeros((len(order), len(order)))
    for i in range(len(order)):
        for j in range(i):
            D[i][j] = O.mahalanobis_distance(jsv[i], jcov[i], jsv[j], jcov[j], g.node["xyzr"][v], xyzr[i], xyzr[j],
                                             p.sigma0rz, p.sigma0rz2, p.endcap_boundary)
    return order, D


def tied(D):
    nz = D[np.nonzero(D)]
    return nz.size > 0 and int((D == nz.min()).sum()) >= 2


def trace(g, v_id):
    """the oracle's smallest pairwise distance of the node with id v_id and every KL list of its greedy
    loop, run with thresholds that merge everything"""
    g = g.copy()
    v = int(np.nonzero(g.node["node_id"] == v_id)[0][0])
    pfx = "uts" if g.node["has_uts"][v] else "tse"
    rec = {"chi2": None, "kl": []}
    orig = O.get_smallest_dist_idx

    def spy(d):
        sm, idx = orig(d)
        if isinstance(d, list):
            rec["kl"].append([float(x) for x in d])
        else:
            rec["chi2"] = float(sm)
        return sm, idx
    O.get_smallest_dist_idx = spy
    try:
        O.cluster_node(g, pfx, v, np.inf, np.inf, Params(), "stop")
    finally:
        O.get_smallest_dist_idx = orig
    return rec


# --------------------------------------------------------------------------- instances
CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


def build(case, base=0, slots=None):
    """the component of `case` with node ids from `base`, its receiver padded to `slots` slots.
    Returns (list of subgraphs, names -> node id, ids of the padding nodes)."""
    net = Net(base)
    case.build(net)
    if slots is not None:
        net.pad(net.names["v"], slots)
    G = net.finish()
    for a in G.nodes.values():
        a.pop("bare", None)
    comps = list(nx.weakly_connected_components(G))
    assert len(comps) == 1, (case.name, "not one component")
    return [G], dict(net.names), list(net.pads)


def packed(case, base=0, slots=None):
    subs, names, pads = build(case, base, slots)
    g = graph.pack(subs)
    if case.post:
        case.post(g, lambda nm: int(np.nonzero(g.node["node_id"] == names[nm])[0][0]))
    return g, names, pads


@functools.lru_cache(maxsize=None)
def own_slots(name):
    g, names, _ = packed(BY_NAME[name])
    if "v" not in names:
        return 0
    v = int(np.nonzero(g.node["node_id"] == names["v"])[0][0])
    return int(g.slot_ptr[v + 1] - g.slot_ptr[v])


@functools.lru_cache(maxsize=None)
def params_of(name):
    """the Params of a case (thresholds that depend on the oracle's distances come from the unpadded build)"""
    c = BY_NAME[name]
    over = c.params
    if callable(over):
        g, names, _ = packed(c)
        over = over(g, names)
    return Params(**(over or {}))


def variants(case):
    """the slot counts a case is instantiated at: None (as built) and, for a padded case, every
    entry of SIZES above its receiver's own count"""
    if not case.pad:
        return [None]
    return [None] + [s for s in SIZES if s > own_slots(case.name)]


def line_of(text):
    """(file or None, line) of the source position a ReferenceError_ names: '(clustering.py:120)', '(:384)'"""
    m = re.search(r"\((\w+\.py)?:(\d+)", text)
    return (m.group(1), int(m.group(2)))


# --------------------------------------------------------------------------- the oracle on a case
def run_oracle(g, case, p, tie_policy="raise"):
    """the case's stage on a copy of g through the oracle; returns (output graph, info)"""
    g = g.copy()
    info = {}
    st = case.stage
    if st == "extrapolate":
        info = O.extrapolate_stage(g, p)
    elif st == "update":
        O.update_stage(g, p)
    elif st in ("cluster_uts", "cluster_tse"):
        O.cluster_stage(g, st[-3:], p.cluster_chi2, p.cluster_kl, p, tie_policy)
    elif st == "full_pass":
        info = O.full_pass(g, p, tie_policy)
    else:
        fn = {"priors_tse": lambda: O.compute_prior_probabilities(g, "tse"),
              "priors_uts": lambda: O.compute_prior_probabilities(g, "uts"),
              "reweight_uts": lambda: O.reweight(g, "uts", p.reweight_threshold),
              "degree": lambda: O.query_node_degree_in_edges(g), "prune": lambda: O.prune_states(g),
              "mw_tse": lambda: O.compute_mixture_weights(g, "tse"), "mw_uts": lambda: O.compute_mixture_weights(g, "uts")}
        for op in st:
            fn[op]()
    return g, info


# --------------------------------------------------------------------------- every case in one graph
@functools.lru_cache(maxsize=1)
def everything():
    """every variant of every case as one packed graph, one component (sub_id) each. Returns (graph,
    comps): per component its case, slot count, `ix` (name -> node index), `nodes` (its node indices,
    a contiguous range), `pad` (bool over those: the padding senders) and `group`, the (stage, Params)
    it runs under."""
    subs, comps = [], []
    for case in CASES:
        for slots in variants(case):
            s, names, pads = build(case, 1000 * len(subs), slots)
            subs += s
            comps.append(dict(case=case, slots=slots, names=names, pads=set(pads)))
    g = graph.pack(subs)
    index = {int(n): i for i, n in enumerate(g.node["node_id"])}
    bounds = np.searchsorted(g.node["sub_id"], np.arange(len(comps) + 1))
    for s, c in enumerate(comps):
        c["sub"] = s
        c["ix"] = {nm: index[n] for nm, n in c["names"].items()}
        c["nodes"] = np.arange(bounds[s], bounds[s + 1])
        c["pad"] = np.isin(g.node["node_id"][c["nodes"]], list(c["pads"]))
        c["group"] = (stage_key(c["case"]), dataclasses.astuple(params_of(c["case"].name)))
        if c["case"].post:
            c["case"].post(g, c["ix"].__getitem__)
    return g, comps


def groups(comps):
    """components by the (stage, Params) they run under, in first-seen order"""
    out = {}
    for c in comps:
        out.setdefault(c["group"], []).append(c)
    return out


def node_mask(g, comps):
    m = np.zeros(g.n_nodes, bool)
    for c in comps:
        m[c["nodes"]] = True
    return m


def is_clean(case):
    """compared on its outputs: no error, or the tie that keeps the merged state formed so far"""
    return case.err is None or case.tie_stop
