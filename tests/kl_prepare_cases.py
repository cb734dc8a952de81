"""Directed inputs for gtf_kl_prepare, gtf_kl_coords and gtf_kl_pair_rows (tests/test_gpu_kl_prepare.py),
with gtf.parabolic.ParabolicKL(device="cpu") -- after in_edge_csr's cut where a case has is_edge -- as
the definition. tests/test_kl_prepare_cases.py checks on the CPU that each case holds what it is
there to exercise.

A case is a dict: ptr int32 [N + 1], src int32 [S], gnn float64 [N, 4], truth int64 [N] or None,
is_edge uint8 [S] or None (ptr / src are then the slot CSR with the non-edges in it), scale (None:
derived), modes: the (ordered, with_single, compact) triples it runs in, error: None or a piece of
the message the device path raises, claim: what test_kl_prepare_cases asserts about it.
"""
import functools

import numpy as np

from gtf import parabolic

ALL = ((False, False, False), (True, False, False), (False, True, True), (True, True, True), (True, False, True))
COMPACT = ((False, False, True), (True, True, True))


def _gnn(rng, n):
    g = rng.normal(0.0, 300.0, (n, 4)).round(4)
    g[:, 3] = np.hypot(g[:, 0], g[:, 1])
    return g


def _csr(degrees, rng=None):
    """ptr, src of nodes with the given in-degrees; a node's senders are distinct and not itself"""
    d = np.asarray(degrees, np.int64)
    n = d.size
    ptr = np.zeros(n + 1, np.int32)
    np.cumsum(d, out=ptr[1:])
    src = np.zeros(int(ptr[-1]), np.int32)
    for v in range(n):
        k = np.arange(1, d[v] + 1)
        if rng is not None:
            k = np.sort(rng.choice(np.arange(1, max(n, d[v] + 1)), d[v], replace=False))
        src[ptr[v]:ptr[v + 1]] = (v + k) % max(n, 1)
    return ptr, src


def _case(ptr, src, gnn, truth=None, is_edge=None, scale=None, modes=ALL, error=None, claim=None):
    return dict(ptr=np.asarray(ptr, np.int32), src=np.asarray(src, np.int32), gnn=np.asarray(gnn, np.float64).reshape(-1, 4),
                truth=None if truth is None else np.asarray(truth, np.int64),
                is_edge=None if is_edge is None else np.asarray(is_edge, np.uint8), scale=scale, modes=tuple(modes),
                error=error, claim=claim)


def _seeded(n, seed, truth="small"):
    rng = np.random.default_rng(seed)
    ptr, src = _csr(rng.integers(0, 11, n) if n > 12 else rng.integers(0, min(n, 11), n), rng)
    return ptr, src, _gnn(rng, n), _truth(rng, n, truth)


def _truth(rng, n, kind):
    if kind is None:
        return None
    if kind == "small":
        return rng.integers(0, max(n // 3, 2), n)
    if kind == "wide":   # 60-bit ids with repeats
        pool = rng.integers(1 << 58, 1 << 60, max(n // 3, 2), dtype=np.int64)
        return pool[rng.integers(0, pool.size, n)]
    if kind == "signed":   # negative and positive ids beyond int32, with repeats
        pool = rng.integers(-(1 << 60), 1 << 60, max(n // 3, 2), dtype=np.int64)
        return pool[rng.integers(0, pool.size, n)]
    raise KeyError(kind)


def _with_edges(ptr, src, rng, keep=0.5, minus=1.0):
    """is_edge at random; a dropped slot's source becomes -1 with probability `minus`"""
    ise = (rng.random(src.size) < keep).astype(np.uint8)
    src = src.copy()
    src[(ise == 0) & (rng.random(src.size) < minus)] = -1
    return src, ise


def _coords(values, n=6):
    """n nodes in a ring of two-edge nodes; `values` laid into x, y from node 0 on"""
    ptr, src = _csr([2] * n)
    g = np.zeros((n, 4))
    v = np.asarray(values, np.float64)
    g.reshape(-1)[np.arange(v.size) // 2 * 4 + np.arange(v.size) % 2] = v
    return ptr, src, g


@functools.lru_cache(maxsize=None)
def vol7():
    from test_kat_parabolic import kat_event
    g, truth = kat_event()
    ptr, src = parabolic.in_edge_csr(g)
    return ptr, src, np.asarray(g.node["gnn"], np.float64), np.asarray(truth, np.int64)


def _build():
    c = {}
    rng = np.random.default_rng(2024)
    # ---- shape and degree
    c["n0"] = _case([0], [], np.zeros((0, 4)), np.zeros(0, np.int64), claim="empty")
    c["n1"] = _case([0, 0], [], [[3.0, 4.0, 0.0, 5.0]], [7], claim="no_slots")
    ptr, src = _csr(list(range(11)) + [65] + [0] * 68)
    c["every_degree"] = _case(ptr, src, _gnn(rng, 80), _truth(rng, 80, "small"), claim="every_degree")
    ptr, src = _csr([8, 9, 9, 8, 0, 0, 0, 0, 0, 0])
    c["deg8_9"] = _case(ptr, src, _gnn(rng, 10), None, claim="deg8_9")
    ptr, src = _csr([1] * 5)
    c["single_only"] = _case(ptr, src, _gnn(rng, 5), [5, 5, 6, 6, 5], claim="single_only")
    for n in (255, 256, 257, 1025):
        c["n%d" % n] = _case(*_seeded(n, n), claim="seeded")
    # ---- is_edge
    ptr, src, g, tr = _seeded(300, 31)
    s2, ise = _with_edges(ptr, src, rng, 0.5, 0.0)
    c["edge_interleaved"] = _case(ptr, s2, g, tr, ise, claim="interleaved")
    s2, ise = _with_edges(ptr, src, rng, 0.6, 1.0)
    c["edge_minus1"] = _case(ptr, s2, g, tr, ise, claim="minus1")
    ise = np.ones(src.size, np.uint8)
    v = int(np.argmax(np.diff(ptr) >= 3))
    ise[ptr[v]:ptr[v + 1]] = 0
    c["edge_node_dropped"] = _case(ptr, src, g, tr, ise, claim=("node_dropped", v))
    s2, ise = _with_edges(ptr, src, rng, 0.5, 1.0)
    s2[np.nonzero(ise)[0][7]] = 300
    c["err_source_n"] = _case(ptr, s2, g, tr, ise, error="source outside [0, n_nodes)", claim="source_n")
    p2 = ptr.copy()
    p2[100] = p2[99] - 1 if p2[99] > 0 else p2[101] + 1
    c["err_ptr_decreases"] = _case(p2, src, g, tr, error="slot_ptr", claim="ptr_decreases")
    # ---- truth ids
    ptr, src, g, _ = _seeded(40, 41)
    lim = np.array([-(1 << 31), (1 << 31) - 1], np.int64)
    c["truth_int32"] = _case(ptr, src, g, np.concatenate([lim, lim, rng.integers(-9, 9, 36)]), modes=COMPACT,
                             claim="truth_plain")
    t = rng.integers(-9, 9, 40)
    t[17] = 1 << 31
    c["truth_2p31"] = _case(ptr, src, g, t, modes=COMPACT, claim="truth_relabel")
    t = rng.integers(-9, 9, 40)
    t[3] = -(1 << 31) - 1
    c["truth_below"] = _case(ptr, src, g, t, modes=COMPACT, claim="truth_relabel")
    c["truth_60bit"] = _case(ptr, src, g, _truth(rng, 40, "wide"), modes=COMPACT, claim="truth_relabel")
    c["truth_signed"] = _case(ptr, src, g, _truth(rng, 40, "signed"), modes=COMPACT, claim="truth_signed")
    c["truth_absent"] = _case(ptr, src, g, None, modes=COMPACT, claim="truth_absent")
    # ---- coordinates
    c["xy_pow2"] = _case(*_coords([256.0, -3.5, 17.25, 100.0, -255.0, 1.0]), modes=COMPACT, claim=("scale", 9))
    c["xy_ulp_below"] = _case(*_coords([np.nextafter(256.0, 0.0), -3.5, 17.25, -100.0]), modes=COMPACT,
                              claim=("bump", 9))
    c["xy_zero"] = _case(*_coords([]), modes=COMPACT, claim=("scale", 0))
    s = 2.0 ** -23   # max 100: e = 7
    ties = [(k + 0.5) * s * sg for k in range(6) for sg in (1.0, -1.0)]
    c["xy_ties"] = _case(*_coords([100.0] + ties, 8), modes=COMPACT, claim=("ties", s))
    c["err_nan"] = _case(*_coords([1.0, 2.0, np.nan, 4.0]), modes=COMPACT, error="non-finite coordinate", claim="nonfinite")
    c["err_inf"] = _case(*_coords([1.0, 2.0, 3.0, -np.inf]), modes=COMPACT, error="non-finite coordinate", claim="nonfinite")
    c["scale_given"] = _case(*_coords([300.0, -17.3, 0.1, 250.0]), scale=2.0 ** -20, modes=COMPACT, claim=("given", True))
    c["err_scale_small"] = _case(*_coords([300.0, -17.3, 0.1, 250.0]), scale=2.0 ** -22, modes=COMPACT,
                                 error="does not fit scale", claim=("given", False))
    # ---- larger inputs
    for k in range(20):
        r = np.random.default_rng(9000 + k)
        n = int(r.integers(1, 400))
        ptr, src, g, tr = _seeded(n, 9100 + k, (None, "small", "wide", "signed")[k % 4])
        ise = None
        if k % 3 == 0 and src.size:
            src, ise = _with_edges(ptr, src, r, 0.7, 0.5)
        c["rand%02d" % k] = _case(ptr, src, g, tr, ise, modes=(ALL[k % 5], ALL[(k + 2) % 5]), claim="random")
    return c


CASES = _build()
NAMES = sorted(CASES) + ["vol7x3"]


def case(name):
    if name == "vol7x3":   # three vol-7 copies (the largest input)
        return _case(*parabolic.batch(*vol7(), 3, seed=5), modes=ALL, claim="vol7x3")
    return CASES[name]


def cut(c):
    """in_edge_csr (parabolic.py:66-75) on the case's arrays: the in-edge CSR the host constructor takes"""
    if c["is_edge"] is None:
        return c["ptr"], c["src"]
    ise = c["is_edge"].astype(bool)
    n = c["ptr"].size - 1
    dst = np.repeat(np.arange(n), np.diff(c["ptr"]))
    ptr = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(dst[ise], minlength=n), out=ptr[1:])
    return ptr, c["src"][ise].astype(np.int32)


def host(c, mode, device="cpu"):
    """the definition: the host constructor on the cut CSR (a given scale goes through quantise_xy as
    a replica's does)"""
    ordered, with_single, compact = mode
    ptr, src = cut(c)
    k = parabolic.ParabolicKL(ptr, src, c["gnn"], c["truth"], device=device, with_single=with_single, ordered=ordered,
                              compact=compact and c["scale"] is None)
    if compact and c["scale"] is not None:
        g = c["gnn"] if k.node_of is None else c["gnn"][k.node_of]
        t = c["truth"] if c["truth"] is None or k.node_of is None else c["truth"][k.node_of]
        k._set_compact(g, t, c["scale"])
    return k
