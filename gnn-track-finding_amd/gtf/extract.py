"""Track-candidate extraction on the GPU: host side of ``gtf_extract_candidates``.

Mirrors src/extract/extract_track_candidates.py (:349-467): CCA over the activated
edges, close-proximity merging, the one-hit-per-layer check and the xy / rz Kalman
fits with chi-square p-values, per candidate on the device. This module turns the
per-candidate device results into the stage's outputs (extracted candidates in the
reference's order with their p-values, the remaining and fragment subgraphs) and, in
:func:`extract_graphs`, into the reference's networkx objects.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native as nat
from .graph import TrackGraph

FRAGMENT, BAD, REJECTED, EXTRACTED = 0, 1, 2, 3


class Params:
    """extract_track_candidates.py flags -p -n -s -t -e -z -b (run_gnn_trackml_mod.sh defaults)."""

    def __init__(self, pval=0.01, numhits=4, separation_3d_threshold=10.0, threshold_distance_node_merging=8.0,
                 sigma0xy=0.3, sigma0rz=0.4, endcap_boundary=550.0):
        self.pval, self.numhits = float(pval), int(numhits)
        self.separation = float(separation_3d_threshold)
        self.merge = float(threshold_distance_node_merging)
        self.sigma0xy, self.sigma0rz, self.endcap = float(sigma0xy), float(sigma0rz), float(endcap_boundary)

    def c(self):
        return nat.GtfExtractParams(self.pval, self.numhits, 0, self.separation, self.merge, self.sigma0xy,
                                    self.sigma0rz, self.endcap)


def run(g: TrackGraph, vivl, params: Params, order_key=None, device="cuda", d=None):
    """Run the extraction on the device for a packed graph (the pass's output).
    vivl: [N, 2] (volume_id, in_volume_layer_id); order_key: optional [N] member order
    inside a candidate (default node order); d: the DeviceGraph of ``g`` already in HBM
    (a stage just ran on it: its activation mask is read in place), else ``g`` is
    uploaded. Returns a dict of host arrays."""
    from .device import DeviceGraph
    if params.numhits < 3:
        raise ValueError("numhits must be >= 3 (rotate_track reads three hits)")
    if d is None:
        from .devmem import default_mem
        d = DeviceGraph(g, device, mem=default_mem())
    elif d.n_nodes != g.n_nodes or d.n_slots != g.n_slots:
        raise ValueError("DeviceGraph does not hold this graph")
    N = g.n_nodes
    sub = g.node["sub_id"].astype(np.int32)
    if N and (np.any(np.diff(sub) < 0) or sub[0] != 0 or np.any(np.diff(sub) > 1)):
        raise ValueError("extraction needs nodes grouped by subgraph (sub_id 0, 1, 2, ... non-decreasing), "
                         "as pack() numbers them")
    n_sub = int(sub.max()) + 1 if N else 0
    sub_ptr = np.searchsorted(sub, np.arange(n_sub + 1)).astype(np.int32)
    n1 = max(N, 1)
    up = lambda a, dt=None: _up(d, np.asarray(a) if dt is None else np.asarray(a).astype(dt))  # noqa: E731
    t = {"xyzr": up(g.node["xyzr"], np.float64), "vivl": up(np.asarray(vivl), np.float64), "sub": up(sub),
         "sub_ptr": up(sub_ptr), "gnn": up(g.node["gnn"], np.float64),
         "order": up(np.asarray(order_key), np.int32) if order_key is not None else None,
         "label": up(np.zeros(n1, np.int32)),
         "status": up(np.full(n1, -1, np.int8)),
         "pxy": up(np.full(n1, np.nan)),
         "pzr": up(np.full(n1, np.nan)),
         "ext": up(np.zeros(n1, np.uint8)),
         "ncand": up(np.zeros(1, np.int32))}
    ws = _zeros(d, int(d.lib.gtf_extract_workspace_bytes(N, n_sub)))
    vp = lambda x: ctypes.c_void_p(x.data_ptr() if x is not None and x.numel() else 0)  # noqa: E731
    io = nat.GtfExtractIO(vp(t["xyzr"]), vp(t["vivl"]), vp(t["sub"]), vp(t["sub_ptr"]), n_sub, 0, vp(t["order"]),
                          vp(t["gnn"]), vp(t["label"]), vp(t["status"]), vp(t["pxy"]), vp(t["pzr"]),
                          vp(t["ext"]), vp(t["ncand"]))
    cp = params.c()
    nat.check(d.lib.gtf_extract_candidates(ctypes.byref(d.cg), ctypes.byref(d.ce), ctypes.byref(io),
                                           ctypes.byref(cp), vp(ws), d.stream))
    out = {k: d._np(t[k])[:N] for k in ("label", "status", "pxy", "pzr", "ext")}
    out["gnn"] = d._np(t["gnn"]).reshape(-1, 4)[:N]
    out["n_candidates"] = int(d._np(t["ncand"])[0])
    return out


def _up(d, a):
    """a host array as a device array of d's allocator (torch tensor or gtf.devmem)"""
    a = np.ascontiguousarray(a).reshape(-1)
    if d.torch is None:
        from .devmem import HipArray
        return HipArray.from_numpy(a)
    return d.torch.from_numpy(a).to(d.device)


def _zeros(d, nbytes):
    if d.torch is None:
        from .devmem import HipArray
        return HipArray.zeros(nbytes, np.uint8)
    return d.torch.zeros(nbytes, dtype=d.torch.uint8, device=d.device)


# ---------------------------------------------------------------- on a DeviceGraph's own buffers
def _vp(x):
    return ctypes.c_void_p(x.data_ptr() if x is not None and x.numel() else 0)


def sub_ptr_dev(d):
    """the first node of every subgraph ([n_sub + 1] int32 on the device) from d's sub_id, by
    gtf_subgraph_ptr_device; built once per DeviceGraph"""
    if "sub_ptr" not in d.t:
        if d.layout != "natural":
            raise NotImplementedError("the device extraction needs layout='natural'")
        t = d._dev_empty(d.n_sub + 1, np.int32)
        nat.check(d.lib.gtf_subgraph_ptr_device(d.ptr("sub_id"), d.n_nodes, d.n_sub, _vp(t), d.stream))
        d.t["sub_ptr"] = t
    return d.t["sub_ptr"]


def candidate_order_dev(d, counts=None):
    """candidate_order() on the device (gtf_candidate_order_device), from the DeviceGraph's own
    arrays: the activation mask a stage just left, sub_id, and the resident node_id column
    (uploaded on first need). Returns the order keys as a device int32 [N] array; counts: an
    optional dict that receives gtf_order_counts (components, set-ordered ones, the largest).
    A graph that carries an event column (``carried["event"]``: DeviceGraph.concat and its subset()
    children) goes through gtf_candidate_order_device_ev: node ids distinct within an event."""
    N = d.n_nodes
    sp, nid = sub_ptr_dev(d), d.node_id_dev()
    order = d._dev_empty(max(N, 1), np.int32)
    nb = int(d.lib.gtf_candidate_order_workspace_bytes(N, d.n_slots, d.n_sub))
    ws = d._dev_empty(nb, np.uint8)
    cnt = nat.GtfOrderCounts()
    ev = getattr(d, "carried", {}).get("event")
    if ev is not None:   # a batch (DeviceGraph.concat): ids are distinct within an event only
        nat.check(d.lib.gtf_candidate_order_device_ev(ctypes.byref(d.cg_sched), ctypes.byref(d.ce), d.ptr("sub_id"),
                                                      _vp(sp), d.n_sub, _vp(nid), _vp(ev), _vp(order), _vp(ws),
                                                      ctypes.c_size_t(nb), ctypes.byref(cnt), d.stream))
    else:
        nat.check(d.lib.gtf_candidate_order_device(ctypes.byref(d.cg_sched), ctypes.byref(d.ce), d.ptr("sub_id"),
                                                   _vp(sp), d.n_sub, _vp(nid), _vp(order), _vp(ws),
                                                   ctypes.c_size_t(nb), ctypes.byref(cnt), d.stream))
    if counts is not None:
        counts.update(n_components=cnt.n_components, n_set_ordered=cnt.n_set_ordered,
                      max_set_ordered=cnt.max_set_ordered)
    return order


def run_dev(d, vivl_dev, params: Params, order_dev=None):
    """run() on the DeviceGraph's own buffers: xyzr, sub_id and the activation mask are read
    where they lie, the merge mutation goes into a device copy of gnn, nothing is uploaded from
    a host graph. vivl_dev: device float64 [N * 2]; order_dev: device int32 [N] (candidate_order_dev)
    or None. Returns device arrays: label, status, pxy, pzr, ext, gnn, ncand, and the workspace
    ("ws") that outputs_dev reads the sorted member list from."""
    if params.numhits < 3:
        raise ValueError("numhits must be >= 3 (rotate_track reads three hits)")
    N, n1 = d.n_nodes, max(d.n_nodes, 1)
    if vivl_dev.numel() != 2 * N:
        raise ValueError("vivl must have one (volume, layer) row per node")
    sp = sub_ptr_dev(d)
    gnn = d._dev_empty(4 * N, np.float64)
    if N:
        nat.check(d.lib.gtf_memcpy_dtod(_vp(gnn), d.ptr("gnn"), ctypes.c_size_t(32 * N), d.stream))
    t = {"gnn": gnn, "label": d._dev_zeros(n1, np.int32), "status": d._dev_empty(n1, np.int8),
         "pxy": d._dev_empty(n1, np.float64), "pzr": d._dev_empty(n1, np.float64),
         "ext": d._dev_zeros(n1, np.uint8), "ncand": d._dev_zeros(1, np.int32)}
    nat.check(d.lib.gtf_memset(_vp(t["status"]), 0xFF, ctypes.c_size_t(n1), d.stream))          # -1
    for k in ("pxy", "pzr"):
        nat.check(d.lib.gtf_memset(_vp(t[k]), 0xFF, ctypes.c_size_t(8 * n1), d.stream))         # NaN
    t["ws"] = d._dev_empty(int(d.lib.gtf_extract_workspace_bytes(N, d.n_sub)), np.uint8)
    io = nat.GtfExtractIO(d.ptr("xyzr"), _vp(vivl_dev), d.ptr("sub_id"), _vp(sp), d.n_sub, 0, _vp(order_dev),
                          _vp(gnn), _vp(t["label"]), _vp(t["status"]), _vp(t["pxy"]), _vp(t["pzr"]), _vp(t["ext"]),
                          _vp(t["ncand"]))
    cp = params.c()
    nat.check(d.lib.gtf_extract_candidates(ctypes.byref(d.cg), ctypes.byref(d.ce), ctypes.byref(io),
                                           ctypes.byref(cp), _vp(t["ws"]), d.stream))
    t["io"] = io
    return t


def _groups(ptr, members):
    return [members[ptr[i]:ptr[i + 1]] for i in range(len(ptr) - 1)]


def outputs_dev(d, res, fragment, ids=True, lists=True, members=False):
    """outputs() on the device (gtf_extract_outputs) from run_dev's result, which must not have
    been reused since. Returns the dict outputs() returns -- the lists as host arrays: of node
    ids (int64) with ids=True, of node indices with ids=False -- plus "keep", the device uint8
    [N] mask DeviceGraph.subset takes, and "left" [n_sub] on the device. Only the counts, the
    pointers, the p-values and the lists asked for cross to the host.
    lists=False: no list crosses and no Python group is built. The dict then carries the device
    arrays as gtf_extract_outputs wrote them, at their upper-bound sizes -- "cand_ptr", "rem_ptr",
    "frag_ptr" (int32), "cand_ids", "rem_ids", "frag_ids" (int64 node ids; "cand_members",
    "rem_nodes", "frag_nodes", int32 indices, with ids=False), "pval_xy", "pval_zr" -- and
    "counts", the six host counts that say how much of each is filled (n_extracted,
    n_extracted_nodes, n_remaining, n_remaining_nodes, n_fragments, n_fragment_nodes): what
    metrics.DeviceScorer.add and DeviceGraph.subset consume without a host copy.
    members=True (with ids=True): the index lists "cand_members", "rem_nodes", "frag_nodes" are written
    beside the id lists -- what split_dev reads a batch's events from."""
    N, n1, S = d.n_nodes, max(d.n_nodes, 1), d.n_sub
    both = bool(ids and members)
    o = {"left": d._dev_empty(max(S, 1), np.int32), "keep": d._dev_empty(n1, np.uint8),
         "pval_xy": d._dev_empty(n1, np.float64), "pval_zr": d._dev_empty(n1, np.float64)}
    for k in ("cand", "rem", "frag"):
        o[k + "_ptr"] = d._dev_empty(n1 + 1, np.int32)
        o[k + "_list"] = d._dev_empty(n1, np.int64 if ids else np.int32)
        if both:
            o[k + "_idx"] = d._dev_empty(n1, np.int32)
    z = ctypes.c_void_p(0)
    lp = [_vp(o[k + "_list"]) for k in ("cand", "rem", "frag")]
    ip = [_vp(o[k + "_idx"]) for k in ("cand", "rem", "frag")] if both else ([z, z, z] if ids else lp)
    out = nat.GtfExtractOut(_vp(o["left"]), _vp(o["keep"]), _vp(o["cand_ptr"]), ip[0],
                            _vp(o["pval_xy"]), _vp(o["pval_zr"]), _vp(o["rem_ptr"]), ip[1],
                            _vp(o["frag_ptr"]), ip[2], _vp(d.node_id_dev()) if ids else z,
                            *(lp if ids else (z, z, z)))
    nb = int(d.lib.gtf_extract_outputs_workspace_bytes(N, S))
    ws = d._dev_empty(nb, np.uint8)
    cnt = nat.GtfExtractOutCounts()
    nat.check(d.lib.gtf_extract_outputs(ctypes.byref(d.cg), ctypes.byref(res["io"]), int(fragment), _vp(res["ws"]),
                                        ctypes.byref(out), _vp(ws), ctypes.c_size_t(nb), ctypes.byref(cnt),
                                        d.stream))
    r = {"keep": o["keep"], "left": o["left"], "pval_xy": o["pval_xy"], "pval_zr": o["pval_zr"]}
    for k in ("cand", "rem", "frag"):
        r[k + "_ptr"], r[_LIST_KEYS[k][0 if ids else 1]] = o[k + "_ptr"], o[k + "_list"]
        if both:
            r[_LIST_KEYS[k][1]] = o[k + "_idx"]
    r["counts"] = {f: int(getattr(cnt, f)) for f, _ in nat.GtfExtractOutCounts._fields_}
    return outputs_host(d, r) if lists else r


_LIST_KEYS = {"cand": ("cand_ids", "cand_members"), "rem": ("rem_ids", "rem_nodes"), "frag": ("frag_ids", "frag_nodes")}


def outputs_host(d, r):
    """the dict outputs_dev(lists=True) returns from the one outputs_dev(lists=False) returned:
    the filled part of every list and of the p-values copied to the host, the lists cut into
    one array per group"""
    c = r["counts"]

    def host(t, n):   # the first n elements on the host
        if n == 0:
            return np.empty(0, t.dtype if d.torch is None else t.cpu().numpy().dtype)
        return d._np(t[:n] if d.torch is not None else t.view(0, n, t.dtype))

    h = {"keep": r["keep"], "left": r["left"]}
    for k, key, n, m in (("cand", "extracted", c["n_extracted"], c["n_extracted_nodes"]),
                         ("rem", "remaining", c["n_remaining"], c["n_remaining_nodes"]),
                         ("frag", "fragments", c["n_fragments"], c["n_fragment_nodes"])):
        lst = r[_LIST_KEYS[k][0]] if _LIST_KEYS[k][0] in r else r[_LIST_KEYS[k][1]]
        h[key] = _groups(host(r[k + "_ptr"], n + 1), host(lst, m)) if d.n_nodes else []
    h["pval_xy"], h["pval_zr"] = host(r["pval_xy"], c["n_extracted"]), host(r["pval_zr"], c["n_extracted"])
    return h


def split_dev(d, o, n_events=None):
    """One extraction's outputs on a fused graph (DeviceGraph.concat, or a subset() child that carries
    its event column) taken apart per event by gtf_event_split. o: outputs_dev(d, res, fragment,
    ids=True, lists=False, members=True). Returns {"first": {"cand" | "rem" | "frag": host int32
    [K + 1], the first group of every event in that list}, "counts": K dicts of the six counts,
    "cand_ptr_ev": the device array of every event's candidate pointers rebased to 0, event e's at
    first["cand"][e] + e, "cand_first_dev": a device view of first["cand"], the K + 1 words the call
    wrote (metrics.BatchScorer.add's cand_first)}. One small download after the call's own synchronisation. Raises
    RuntimeError (rc -2) when a group spans two events or the events do not ascend."""
    K = int(getattr(d, "n_events", 0) if n_events is None else n_events)
    ev = d.carried["event"]
    c = o["counts"]
    cnt = nat.GtfExtractOutCounts(*[c[f] for f, _ in nat.GtfExtractOutCounts._fields_])
    small = d._dev_empty(3 * (K + 1) + 6 * K, np.int32)   # the three first arrays, then the counts
    pev = d._dev_empty(c["n_extracted"] + K, np.int32)
    base = small.data_ptr() if small.numel() else 0
    at = lambda words: ctypes.c_void_p(base + 4 * words if base else 0)  # noqa: E731
    sin = nat.GtfSplitIn(**{k: _vp(o[k]) for k in ("cand_ptr", "cand_members", "rem_ptr", "rem_nodes", "frag_ptr",
                                                   "frag_nodes")})
    sout = nat.GtfSplitOut(at(0), at(K + 1), at(2 * (K + 1)), at(3 * (K + 1)), _vp(pev))
    nb = int(d.lib.gtf_event_split_workspace_bytes(K))
    ws = d._dev_empty(nb, np.uint8)
    nat.check(d.lib.gtf_event_split(_vp(ev), d.n_nodes, K, ctypes.byref(cnt), ctypes.byref(sin), ctypes.byref(sout),
                                    _vp(ws), ctypes.c_size_t(nb), d.stream))
    h = d._np(small).astype(np.int32, copy=False) if K else np.zeros(3, np.int32)
    first = {k: h[i * (K + 1):(i + 1) * (K + 1)] for i, k in enumerate(("cand", "rem", "frag"))}
    names = [f for f, _ in nat.GtfExtractOutCounts._fields_]
    counts = [dict(zip(names, (int(x) for x in h[3 * (K + 1) + 6 * e:3 * (K + 1) + 6 * e + 6]))) for e in range(K)]
    return {"first": first, "counts": counts, "cand_ptr_ev": pev,
            "cand_first_dev": small[:K + 1] if d.torch is not None else small.view(0, K + 1, small.dtype)}


def candidate_order(g: TrackGraph) -> np.ndarray:
    """Each node's position inside its candidate in the reference's member order
    (gtf_candidate_order: networkx CCA + subgraph-copy orders, :332-346), for run()'s
    order_key. Host function on the packed graph's activation mask."""
    N = g.n_nodes
    a = {k: np.ascontiguousarray(v) for k, v in (
        ("slot_ptr", g.slot_ptr.astype(np.int32)), ("slot_src", g.slot["slot_src"].astype(np.int32)),
        ("is_edge", g.slot["is_edge"].astype(np.uint8)), ("act", g.slot["act"].astype(np.uint8)),
        ("out_ptr", g.out_ptr.astype(np.int32)), ("out_slot", g.out_slot.astype(np.int32)),
        ("sub_id", g.node["sub_id"].astype(np.int32)), ("node_id", g.node["node_id"].astype(np.int64)))}
    vp = lambda x: ctypes.c_void_p(x.ctypes.data if x.size else 0)  # noqa: E731
    cg = nat.GtfCandidateGraph(N, g.n_slots, g.n_edges, 0, vp(a["slot_ptr"]), vp(a["slot_src"]), vp(a["is_edge"]),
                               vp(a["act"]), vp(a["out_ptr"]), vp(a["out_slot"]), vp(a["sub_id"]), vp(a["node_id"]))
    out = np.zeros(max(N, 1), np.int32)
    nat.check(nat.lib(lean=True).gtf_candidate_order(ctypes.byref(cg), vp(out)))   # host code: no torch needed
    return out[:N]


def outputs(g: TrackGraph, res, fragment, order_key=None):
    """The stage's outputs from the device results: extracted candidates (node index
    arrays, in the reference's order), their p-values, remaining and fragment node
    sets per subgraph (:423-430). order_key: member order inside each candidate (as
    given to run()); default node order."""
    label, status, ext = res["label"], res["status"], res["ext"].astype(bool)
    roots = np.unique(label)                          # candidate order = first-node order
    extracted = [np.nonzero(label == r)[0] for r in roots if status[r] == EXTRACTED]
    if order_key is not None:
        extracted = [c[np.argsort(order_key[c], kind="stable")] for c in extracted]
    pxy = np.array([res["pxy"][r] for r in roots if status[r] == EXTRACTED])
    pzr = np.array([res["pzr"][r] for r in roots if status[r] == EXTRACTED])
    sub = g.node["sub_id"]
    remaining, fragments = [], []
    for s in range(int(sub.max()) + 1 if g.n_nodes else 0):
        left = np.nonzero((sub == s) & ~ext)[0]
        if 0 < len(left) < fragment:
            fragments.append(left)
        elif len(left) >= fragment:
            remaining.append(left)
    return {"extracted": extracted, "pval_xy": pxy, "pval_zr": pzr, "remaining": remaining,
            "fragments": fragments}
