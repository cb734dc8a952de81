"""Directed inputs for the batch of resident events (tests/test_gpu_batch.py): the part lists
DeviceGraph.concat / gtf_graph_concat are given, with gtf.graph.concat as the definition, and
hand-made extraction outputs for gtf_event_split, with per-event slicing as the definition.
tests/test_batch_cases.py checks on the CPU that each input holds what it claims.

A part is named by a spec: ("hand", name) one of test_gpu_event_pack's hand-made events, ("empty",)
the event whose volume window holds no node (its edge rows stay), ("tiny", i) a one-node (even i) or
two-node (odd i) event with ids of its own, ("vol7",) the golden volume-7 event, ("subset", name) the
subset() child of a subset_cases case -- orphan keys, scattered sub_id.
"""
import functools
import os

import numpy as np

import subset_cases as sc
from fixtures import GOLDEN
from gtf import graph, io
from gtf.graph import NODE_FIELDS, SLOT_FIELDS, TrackGraph, empty_arrays
from test_gpu_event_pack import _handmade, _host_event

PREFIX = os.path.join(GOLDEN, "kat134", "event_1_filtered_graph_")

CONCAT = {
    "hand4": [("hand", "one"), ("hand", "two"), ("hand", "chain65"), ("hand", "perm257")],
    "empty_first": [("empty",), ("hand", "two"), ("hand", "chain65")],
    "empty_middle": [("hand", "chain65"), ("empty",), ("empty",), ("hand", "two")],
    "empty_last": [("hand", "perm257"), ("hand", "one"), ("empty",)],
    "all_empty": [("empty",), ("empty",)],
    "k1": [("hand", "perm257")],
    "k65": [("tiny", i) for i in range(65)],              # more parts than a wavefront
    "k257": [("tiny", i) for i in range(257)],            # ... than a block of offsets
    "vol7_twice": [("vol7",), ("vol7",)],                 # every node id twice
    "orphans": [("subset", "tiny200"), ("subset", "boundary")],
    "midwave": [("hand", "chain65"), ("hand", "two"), ("hand", "perm257")],   # boundaries at nodes 65 and 67
}


def tiny_columns(i):
    """a one-node (even i) or two-node (odd i) event; the ids of different i differ"""
    rng = np.random.default_rng(1000 + i)
    n = 1 + (i & 1)
    ids = np.array([7 * i + 3, 7 * i + 1][:n], np.int64)
    rows = np.array([[7 * i + 1, 7 * i + 3]], np.int64) if n == 2 else np.zeros((0, 2), np.int64)
    x, y, z = (rng.normal(0, 300, n).round(4) for _ in range(3))
    layer = (rng.integers(7, 10, n) * 1000 + rng.integers(2, 14, n)).astype(np.int64)
    return ids, x, y, z, io.edge_length_xy(x, y), layer, rows[:, 0].copy(), rows[:, 1].copy()


def empty_columns():
    """no node in the window, but edge rows: what from_event gets for test_from_event_empty_window's event"""
    e, f = np.zeros(0, np.int64), np.zeros(0, np.float64)
    return e, f, f, f, f, e, np.array([4, 9], np.int64), np.array([9, 5], np.int64)


def columns(spec):
    """the from_event columns of a "hand", "tiny", "empty" or "vol7" part"""
    if spec[0] == "hand":
        return _handmade(spec[1])
    if spec[0] == "tiny":
        return tiny_columns(spec[1])
    if spec[0] == "empty":
        return empty_columns()
    if spec[0] == "vol7":
        ids, x, y, z, r, layer = io.read_nodes(PREFIX + "nodes.csv", 7, 7)
        n2, n1 = io.read_edges(PREFIX + "edges.csv")
        return ids, x, y, z, r, layer, n1, n2
    raise KeyError(spec)


def empty_graph():
    z = np.zeros(1, np.int32)
    return TrackGraph(0, 0, z, z.copy(), np.zeros(0, np.int32), empty_arrays(NODE_FIELDS, 0),
                      empty_arrays(SLOT_FIELDS, 0), 0)


@functools.lru_cache(maxsize=None)
def host_part(spec):
    """(graph, vivl or None) of a part as the host builds it: treat as read-only. ("vol7",) is the event
    without states here (the host builder alone); the GPU tests build it with them."""
    if spec[0] == "empty":
        return empty_graph(), np.zeros((0, 2))
    if spec[0] == "subset":
        return sc.case(spec[1])[2], None
    return _host_event(*columns(spec))


def host_concat(name):
    """(parts, fused graph, event column) of a named case on the host"""
    parts = [host_part(s)[0] for s in CONCAT[name]]
    event = np.repeat(np.arange(len(parts), dtype=np.int32), [g.n_nodes for g in parts])
    return parts, graph.concat(parts), event


# ---------------------------------------------------------------- split
def _groups(rng, lo, hi, n_groups, size):
    """n_groups disjoint groups of `size` node indices of [lo, hi), each ascending, groups by first member"""
    if n_groups == 0:
        return []
    pick = rng.choice(np.arange(lo, hi), n_groups * size, replace=False)
    g = [np.sort(pick[i * size:(i + 1) * size]) for i in range(n_groups)]
    return sorted(g, key=lambda a: int(a[0]))


def _event_lists(rng, lo, hi, n_cand, n_rem, n_frag):
    """one event's three lists over its nodes [lo, hi): candidates of 4 members in any member order (the order
    key's), remaining groups of 5, fragments of 1..3"""
    cand = [rng.permutation(c) for c in _groups(rng, lo, hi, n_cand, 4)]
    cand = sorted(cand, key=lambda a: int(a.min()))   # candidates ascend by their smallest node
    return cand, _groups(rng, lo, hi, n_rem, 5), _groups(rng, lo, hi, n_frag, int(rng.integers(1, 4)))


SPLIT = {   # name: per event (nodes, candidates, remaining groups, fragment groups)
    "no_candidate": [(40, 3, 2, 1), (30, 0, 2, 2), (40, 2, 1, 0)],
    "only_fragments": [(30, 2, 1, 1), (12, 0, 0, 3), (30, 1, 2, 1)],
    "last_empty": [(40, 3, 2, 2), (30, 1, 1, 1), (0, 0, 0, 0)],
    "first_empty_nodes_no_groups": [(0, 0, 0, 0), (25, 0, 0, 0), (40, 4, 3, 2)],
    "nothing": [(10, 0, 0, 0), (10, 0, 0, 0)],
}


def _csr(groups):
    ptr = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int32)
    mem = np.concatenate(groups).astype(np.int32) if groups else np.zeros(0, np.int32)
    return ptr, mem


@functools.lru_cache(maxsize=None)
def split_case(name):
    """{"event", "K", "N", "lists": {"cand" | "rem" | "frag": (ptr, members)}, "per_event": K x {list: groups}}:
    the fused lists as gtf_extract_outputs leaves them, made event by event (the definition of the split).
    Candidates take the node indices a remaining or fragment group may take too: the split does not care."""
    if name == "k257":
        rng = np.random.default_rng(257)
        spec = [(int(n), int(c), int(r), int(f)) for n, c, r, f in
                zip(rng.choice([0, 9, 20, 33], 257), rng.integers(0, 3, 257), rng.integers(0, 3, 257),
                    rng.integers(0, 3, 257))]
        spec = [(n, c if n >= 9 else 0, r if n >= 20 else 0, f if n >= 9 else 0) for n, c, r, f in spec]
    else:
        spec = SPLIT[name]
    rng = np.random.default_rng(5)
    per, lo = [], 0
    for n, c, r, f in spec:
        cand, rem, frag = _event_lists(rng, lo, lo + n, c, r, f)
        per.append({"cand": cand, "rem": rem, "frag": frag})
        lo += n
    event = np.repeat(np.arange(len(spec), dtype=np.int32), [s[0] for s in spec])
    lists = {k: _csr([g for e in per for g in e[k]]) for k in ("cand", "rem", "frag")}
    return {"event": event, "K": len(spec), "N": lo, "lists": lists, "per_event": per}


def bad_split_case(name):
    """a list gtf_event_split must refuse: "spanning" -- a remaining group with members of two events;
    "decreasing" -- the candidates of two events swapped; "empty_group" -- a fragment group without members;
    "member_range" -- a member beyond the nodes"""
    c = split_case("no_candidate")
    lists = {k: (p.copy(), m.copy()) for k, (p, m) in c["lists"].items()}
    if name == "spanning":
        p, m = lists["rem"]
        m[p[1] - 1] = 45     # the last member of event 0's first remaining group moves into event 1
    elif name == "decreasing":
        per = c["per_event"]
        lists["cand"] = _csr(per[2]["cand"] + per[0]["cand"])
    elif name == "empty_group":
        p, m = lists["frag"]
        lists["frag"] = (np.concatenate([p[:1], p]).astype(np.int32), m)
    elif name == "member_range":
        lists["cand"][1][0] = c["N"]
    else:
        raise KeyError(name)
    return dict(c, lists=lists)


def counts_of(lists):
    """gtf_extract_out_counts of the fused lists, in the struct's order"""
    return [int(x) for k in ("cand", "rem", "frag") for x in (lists[k][0].size - 1, lists[k][1].size)]


def split_rule(event, K, lists):
    """The split as gtf_event_split states it, in NumPy: per list the first group of every event = the lower
    bound of the event among the events of the groups' first members; the six counts of every event; every
    event's candidate pointers rebased to 0, event e's at first[e] + e."""
    first, counts = {}, np.zeros((K, 6), np.int32)
    for j, k in enumerate(("cand", "rem", "frag")):
        ptr, mem = lists[k]
        ev = event[mem[ptr[:-1]]] if ptr.size > 1 else np.zeros(0, np.int32)
        first[k] = np.searchsorted(ev, np.arange(K + 1), side="left").astype(np.int32)
        counts[:, 2 * j] = np.diff(first[k])
        counts[:, 2 * j + 1] = np.diff(ptr[first[k]])
    ptr, fc = lists["cand"][0], first["cand"]
    pev = np.zeros(ptr.size - 1 + K, np.int32)
    for e in range(K):
        pev[fc[e] + e:fc[e + 1] + e + 1] = ptr[fc[e]:fc[e + 1] + 1] - ptr[fc[e]]
    return first, counts, pev
