"""Batches of events for the batched candidate scoring (gtf.metrics.concat_tables / BatchScorer on the
host side, gtf_truth_concat / gtf_score_*_ev on the device): lists of events, most of them taken from
tests/score_cases.py (each is a complete event: mapping, particles, calls). World starts every event at
node 10 and reuses small particle ids, so node ids and particle ids collide across the events of almost
every batch: the lookups must stay inside the event's own segment.

A batch is a list of events. An event is a score_cases case; {"unscored": True, "calls": ...} is an
event without truth (its tables are None). The definition of every event's result is
metrics.reconstruction_efficiency / metrics.truth_tables on that event alone.
tests/test_score_batch_cases.py checks on the host that every batch reaches the branch it is named for;
tests/test_gpu_score_batch.py runs them on the device."""
import functools

import numpy as np

import score_cases as SC
from gtf import metrics

SIZES = (1, 2, 16, 17, 63, 64, 65, 200)


# ------------------------------------------------------------------ events
def _case(name):
    return SC.CASES[name]()


def _track_event(pid=1, n=4, take=None, node0=10, stride=3):
    """one particle on n nodes, one candidate of its first `take` nodes"""
    w = SC.World(node0=node0, stride=stride)
    a = w.track(pid, n)
    return w.build([(0, [a[:take or n]])], {})


def _no_match():
    w = SC.World()
    e = w.track(8, 4, pt=0.5)     # below the pT cut: not in the region
    return w.build([(0, [e])], {})


def _all_matched():
    w = SC.World()
    a, b = w.track(1, 4), w.track(2, 5)
    return w.build([(0, [b, a])], {})


def _negative_ids():
    w = SC.World()
    a, b, c = w.track(-5, 4), w.track(-SC.B60 - 3, 5), w.track(SC.B60 + 5, 4)
    return w.build([(0, [c, a, b])], {})


def _empty_tables():
    """an event whose mapping has no row: T = P = R = 0, no candidate"""
    z = np.zeros(0, np.int64)
    t = metrics.TruthTables(z, np.zeros(1, np.int32), z, z, np.zeros(0, np.int32), np.zeros(0, np.uint8), 0)
    host = metrics.Result(0, 0, np.zeros(0), np.zeros(0), z, z, np.zeros(0, bool))
    return {"calls": [(0, [])], "tables": t, "host": host}


def _unscored():
    return {"unscored": True, "calls": [(0, [[999, 1000, 10], [5]]), (1, [[13]])]}


def _sized(sizes, first_pid):
    """one candidate per size: odd positions a dense candidate (nodes of up to 6 hits), even ones a
    track of one hit per node (score_cases._sizes)"""
    w = SC.World()
    cands = []
    for i, n in enumerate(sizes):
        if i % 2:
            cands.append(SC._dense(w, first_pid + i, n, first_pid + 1000 + 10 * i)[0])
        else:
            cands.append(w.track(first_pid + i, n))
    return w.build([(0, cands)], {"sizes": list(sizes)})


def _random_event(seed):
    """tests/test_gpu_score.py's random events, smaller: nodes of 1-6 hits, every particle in several
    candidates (duplicates), half-and-half candidates (ties), repeated members, 1-3 calls"""
    rng = np.random.default_rng(seed)
    w = SC.World(node0=int(rng.integers(0, 20)), stride=int(rng.integers(1, 4)))
    tracks = []
    n_part = int(rng.integers(8, 20))
    for p in range(n_part):
        pid = SC.B60 + int(rng.integers(0, 1 << 40)) * 2 + 1 if p else 0
        tracks.append((pid, w.track(pid, int(rng.integers(2, 13)), pt=float(rng.choice([0.5, 2.0, 2.0, 2.0])))))
    for pid, ns in tracks:
        for v in ns:
            for _ in range(int(rng.choice([0, 0, 0, 1, 2, 5]))):
                w.hit(v, tracks[int(rng.integers(0, n_part))][0], int(rng.integers(1, 40)) * 2 + 1)
    cands = []
    n_cand = int(rng.integers(20, 60))
    while len(cands) < n_cand:
        kind = rng.integers(0, 6)
        pid, ns = tracks[int(rng.integers(0, n_part))]
        if kind == 0:               # a tie by construction
            _, other = tracks[int(rng.integers(0, n_part))]
            k = int(rng.integers(1, min(len(ns), len(other)) + 1))
            c = list(ns[:k]) + list(other[:k])
        elif kind == 1:             # a repeated member, a long list
            c = [ns[int(i)] for i in rng.integers(0, len(ns), int(rng.integers(1, 40)))]
        elif kind == 2:
            c = []
        else:
            c = [v for v in ns if rng.random() < 0.8]
        cands.append(c)
    cuts = sorted(int(x) for x in rng.integers(0, n_cand + 1, int(rng.integers(0, 3))))
    edges = [0] + cuts + [n_cand]
    return w.build([(g, cands[a:b]) for g, (a, b) in enumerate(zip(edges[:-1], edges[1:]))], {})


def _random_batch(seed):
    rng = np.random.default_rng(1000 + seed)
    return [_random_event(100 * seed + i) for i in range(int(rng.integers(3, 10)))]


def _large(K):
    """K one-candidate events, three kinds in turn (built once each; the list repeats the objects)"""
    kinds = [_track_event(1, 4), _no_match(), _track_event(2, 6, take=3)]
    return [kinds[i % 3] for i in range(K)]


def _boundaries():
    # candidates per event 1, 1, 1, 2, 1, 2, 3, 1, 2: the events start at candidates 0, 1, 2, 3, 5, 6, 8, 11, 12
    sizes = [(1,), (17,), (63,), (64, 2), (65,), (200, 16), (16, 17, 1), (2,), (64, 65)]
    return [_sized(s, 100 * (i + 1)) for i, s in enumerate(sizes)]


_NEIGHBOUR = functools.partial(_track_event, 1, 12, None, 10, 1)   # nodes 10 .. 21: holds missing_id's id 20

BATCHES = {
    "twice": lambda: [_case("thresholds")] * 2,
    "same_node_other_particles": lambda: [_track_event(1, 4), _track_event(2, 5), _track_event(1, 6, take=3)],
    "missing_middle": lambda: [_NEIGHBOUR(), _case("missing_id"), _NEIGHBOUR()],
    "missing_first": lambda: [_case("missing_id"), _NEIGHBOUR()],
    "missing_last": lambda: [_NEIGHBOUR(), _case("thresholds"), _case("missing_id")],
    "empty_events": lambda: [_case("no_candidates"), _case("thresholds"), _case("no_candidates"), _empty_tables(),
                             _case("ids_60bit"), _case("no_candidates")],
    "unscored_between": lambda: [_case("thresholds"), _unscored(), _case("dup_in_call")],
    "boundaries": _boundaries,
    "group_orders": lambda: [_case("dup_across_short_first"), _case("thresholds"), _case("dup_across_full_first")],
    "finish": lambda: [_all_matched(), _no_match(), _case("ids_60bit"), _negative_ids()],
    "large_65": lambda: _large(65),
    "large_257": lambda: _large(257),
    "large_2049": lambda: _large(2049),
}
BATCHES.update({"singleton_" + n: (lambda n=n: [_case(n)]) for n in SC.CASES})
BATCHES.update({"random_%d" % s: (lambda s=s: _random_batch(s)) for s in range(5)})
MISSING = {"missing_middle": 1, "missing_first": 0, "missing_last": 2, "singleton_missing_id": 0}   # the event named


# ------------------------------------------------------------------ the definition, per event
def event_tables(ev):
    """the event's TruthTables (None: an event without truth); computed once per event object"""
    if ev.get("unscored"):
        return None
    if "tables" not in ev:
        ev["tables"] = SC.tables(ev)
    return ev["tables"]


def event_host(ev):
    """metrics.reconstruction_efficiency on the event alone (None: without truth); raises ValueError for
    an event with a missing id"""
    if ev.get("unscored"):
        return None
    if "host" not in ev:
        ev["host"] = SC.host_result(ev)
    return ev["host"]


def batch_calls(events):
    """-> [(group, cand_first [K + 1], candidates of all events)] by ascending group: the call of a group
    holds the candidates every event has in it (none where the event has no such call), so cand_first
    differs from call to call"""
    groups = sorted({g for ev in events for g, _ in ev["calls"]})
    out = []
    for g in groups:
        per = [[c for gg, cs in ev["calls"] if gg == g for c in cs] for ev in events]
        first = np.zeros(len(events) + 1, np.int32)
        first[1:] = np.cumsum([len(p) for p in per])
        out.append((g, first, [c for p in per for c in p]))
    return out


def csr(cands):
    ptr = np.zeros(len(cands) + 1, np.int32)
    ptr[1:] = np.cumsum([len(c) for c in cands])
    return ptr, np.array([v for c in cands for v in c], np.int64)
