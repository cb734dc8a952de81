"""Directed inputs for the device subset (tests/test_gpu_graph_subset.py), with the host
gtf.graph.subset as the definition; tests/test_subset_cases.py checks on the CPU that each
input holds what it claims.

The reference stage graphs (tests/golden/dropin_*.pkl) under test_subset.py's masks never put
more than 3 orphans in a segment, never exceed 4 slots a segment and have no orphan with only
an updated_track_states key, so the hard branches come from a hand-built graph:

  boundary   test_gpu_graph_prepare.boundary_graph (segments of 0..100 slots) with every
             segment's track_state_estimates order permuted, a third of the slots moved to an
             updated_track_states-only key, some slots in both dicts, some edges in neither,
             some dict keys without an edge, scattered sub_id; the mask keeps every receiver
             beyond 64 slots, removes one subgraph whole and reduces one to a single node
  dropin_*   the four reference graphs under test_subset.py's masks, and each result cut again
             with keep[1::4] = False, so old and new orphans share segments
  tiny200    synth.workload("tiny200", seed=1) with keep[::3] = False (1,837 slots, 643 orphans)
  all / none keep everything, keep nothing
"""
import copy
import functools
import os
import pickle
import random

import numpy as np

from fixtures import GOLDEN
from gtf import graph, synth

BOUNDARY_SEED = 11
DROPIN = (("extract", "input", 1), ("extrapolate", "out", 2), ("update", "in", 3), ("update", "out", 4))


def host_subset(g, keep):
    """(h, node_map, slot_map): graph.subset(g, keep) with send_mw refreshed, and the old node /
    slot of every new one -- read off a run whose node_id / slot_key are the old indices"""
    t = g.copy()
    t.node["node_id"] = np.arange(g.n_nodes, dtype=np.int64)
    t.slot["slot_key"] = np.arange(g.n_slots, dtype=np.int64)
    t = graph.subset(t, keep)
    h = graph.refresh_send_mw(graph.subset(g, keep))
    return h, t.node["node_id"].copy(), t.slot["slot_key"].copy()


def _segments(ptr):
    ptr = np.asarray(ptr, np.int64)
    return [(int(ptr[v]), int(ptr[v + 1])) for v in range(ptr.size - 1)]


def boundary(seed=BOUNDARY_SEED):
    from test_gpu_graph_prepare import boundary_graph
    g = boundary_graph()
    rng = np.random.default_rng(seed)
    N, S = g.n_nodes, g.n_slots
    tr = np.full(S, -1, np.int32)
    ur = np.full(S, -1, np.int32)
    kind = rng.choice(4, S, p=[0.42, 0.33, 0.15, 0.10])   # tse only, uts only, both, neither (edge only)
    for lo, hi in _segments(g.slot_ptr):
        k = np.arange(lo, hi)
        t = k[(kind[k] == 0) | (kind[k] == 2)]
        u = k[(kind[k] == 1) | (kind[k] == 2)]
        tr[t] = rng.permutation(t.size)
        ur[u] = rng.permutation(u.size)
    g.slot["tse_rank"], g.slot["uts_rank"] = tr, ur
    g.node["has_uts"][:] = 1
    # dict keys without an edge: clear is_edge on some keyed slots and take them out of the out view
    unedge = (kind != 3) & (rng.random(S) < 0.08)
    g.slot["is_edge"][unedge] = 0
    g.slot["act"][unedge] = 0
    op = g.out_ptr.astype(np.int64)
    owner = np.repeat(np.arange(N), np.diff(op))
    ok = g.slot["is_edge"][g.out_slot] == 1
    g.out_slot = g.out_slot[ok].astype(np.int32)
    g.out_ptr = np.concatenate([[0], np.cumsum(np.bincount(owner[ok], minlength=N))]).astype(np.int32)
    # scattered subgraph ids (the synthetic events' ids are not monotone either)
    n_sub = 40
    sub = rng.integers(0, n_sub, N).astype(np.int32)
    g.node["sub_id"] = sub
    g.n_subgraphs = n_sub
    graph.refresh_send_mw(g)
    graph.check_layout(g)
    deg = np.diff(g.slot_ptr.astype(np.int64))
    big = deg >= 65
    keep = big | (rng.random(N) > 0.4)
    free = [s for s in range(n_sub) if (sub == s).sum() >= 2 and not big[sub == s].any()]
    keep[sub == free[0]] = False                       # a subgraph removed whole
    keep[sub == free[1]] = False                       # a subgraph reduced to one node
    keep[np.nonzero(sub == free[1])[0][0]] = True
    return g, keep


def _dropin(name, key, seed):
    """test_subset.py's input and mask for this fixture"""
    with open(os.path.join(GOLDEN, "dropin_%s.pkl" % name), "rb") as f:
        subs = copy.deepcopy(pickle.load(f)[key])
    rng = random.Random(seed)
    g = graph.pack(subs)
    keep = np.zeros(g.n_nodes, bool)
    i = 0
    for G in subs:
        whole = rng.random() < 0.1
        for _ in G.nodes:
            keep[i] = not whole and rng.random() > 0.2
            i += 1
    return g, keep


def _second(name, key, seed):
    g, keep = _dropin(name, key, seed)
    h = graph.refresh_send_mw(graph.subset(g, keep))
    keep2 = np.ones(h.n_nodes, bool)
    keep2[1::4] = False
    return h, keep2


def tiny200():
    g = synth.workload("tiny200", seed=1)
    graph.refresh_send_mw(g)
    keep = np.ones(g.n_nodes, bool)
    keep[::3] = False
    return g, keep


def _all():
    g, _ = tiny200()
    return g, np.ones(g.n_nodes, bool)


def _none():
    g, _ = tiny200()
    return g, np.zeros(g.n_nodes, bool)


BUILDERS = {"boundary": boundary, "tiny200": tiny200, "all": _all, "none": _none}
for _n, _k, _s in DROPIN:
    BUILDERS["dropin_%s_%s" % (_n, _k)] = functools.partial(_dropin, _n, _k, _s)
    BUILDERS["dropin_%s_%s_again" % (_n, _k)] = functools.partial(_second, _n, _k, _s)
NAMES = tuple(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    """(g, keep, h, node_map, slot_map) of a named case, built once and shared: treat as read-only"""
    g, keep = BUILDERS[name]()
    h, nm, sm = host_subset(g, keep)
    return g, keep, h, nm, sm


def census(name):
    """what the case's subset contains, counted on the host result"""
    g, keep, h, nm, sm = case(name)
    tr, ur, src = h.slot["tse_rank"], h.slot["uts_rank"], h.slot["slot_src"]
    orph = src < 0
    out = {"orphans": int(orph.sum()), "tse_only": int((orph & (tr >= 0) & (ur < 0)).sum()),
           "uts_only": int((orph & (tr < 0) & (ur >= 0)).sum()), "both": int((orph & (tr >= 0) & (ur >= 0)).sum()),
           "inside_non_edge": int((~orph & (h.slot["is_edge"] == 0)).sum())}
    reordered = most = big_seg = 0
    for lo, hi in _segments(h.slot_ptr):
        o = sm[lo:hi][orph[lo:hi]]
        reordered += bool(np.any(np.diff(o) < 0))
        most = max(most, o.size)
        big_seg += hi - lo > 64 and o.size > 32
    out.update(reordered_segments=reordered, most_orphans=most, big_segments=big_seg,
               largest_segment=int(np.diff(h.slot_ptr).max()) if h.n_nodes else 0)
    # old slots of kept receivers that were an edge and in neither dict, and are gone
    kr = keep[g.slot_dst()] if g.n_slots else np.zeros(0, bool)
    gone = np.ones(g.n_slots, bool)
    gone[sm] = False
    out["vanished_edge_only"] = int((kr & gone & (g.slot["is_edge"] == 1) & (g.slot["tse_rank"] < 0) &
                                     (g.slot["uts_rank"] < 0)).sum())
    out["slot_free_nodes"] = int((np.diff(h.slot_ptr) == 0).sum())
    od_old = np.diff(g.out_ptr.astype(np.int64))[nm]
    out["senders_losing_all"] = int(((od_old > 0) & (np.diff(h.out_ptr) == 0)).sum())
    sub = g.node["sub_id"]
    kept = np.bincount(sub[keep], minlength=int(sub.max()) + 1 if g.n_nodes else 0)
    had = np.bincount(sub, minlength=kept.size)
    out["subgraphs_removed"] = int(((had > 0) & (kept == 0)).sum())
    out["solo_subgraphs"] = int((kept == 1).sum())
    out["sub_id_monotone"] = not bool(np.any(np.diff(sub) < 0))
    return out
