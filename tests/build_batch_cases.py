"""Hand-made batches of events for the batch build (io.csr_from_rows_batch, gtf_build_events_csr_device):
each case is a list of parts (ids, a, b) as io.csr_from_rows takes one event -- node ids in CSV order,
edge rows add_edge(a, b) then add_edge(b, a). tests/test_build_batch_cases.py checks on the CPU that every
case reaches the branch it is named for; tests/test_gpu_build_batch.py sends every case through the C-ABI.

The yardstick is io.csr_from_rows_batch(parts) with device=None: the host builder once per event and
gtf.graph.concat's offsets. reference() caches it per case: treat what it returns as read-only."""
import numpy as np

from gtf import io
from gtf.graph import NODE_FIELDS, SLOT_FIELDS, TrackGraph, check_layout, empty_arrays

I64 = np.int64
NO = np.zeros(0, I64)


def part(ids, rows=()):
    """(ids, a, b) from a list of ids and a list of (a, b) rows"""
    rows = list(rows)
    return (np.array(ids, I64).reshape(-1), np.array([r[0] for r in rows], I64), np.array([r[1] for r in rows], I64))


def chain(ids):
    return [(ids[i], ids[i + 1]) for i in range(len(ids) - 1)]


def random_event(seed, n, rows, id_space, chain_frac):
    """test_build._write_event's event as columns: a chain over the first chain_frac of the nodes, random local
    rows, repeated rows, self loops and two rows with an unknown end, shuffled"""
    rng = np.random.default_rng(seed)
    ids = rng.choice(id_space, size=n, replace=False).astype(I64)
    m = int(n * chain_frac)
    e = [(ids[i], ids[i + 1]) for i in range(m - 1)]
    for _ in range(rows):
        i = int(rng.integers(0, n))
        j = int(min(n - 1, max(0, i + rng.integers(-6, 7))))
        e.append((ids[i], ids[j]))
    e += e[:: max(1, len(e) // 50)]
    e += [(ids[0], id_space + 5), (id_space + 6, ids[min(1, n - 1)])]
    order = rng.permutation(len(e))
    return part(ids, [e[k] for k in order])


def tiny(i):
    """1 to 3 nodes, chained; the ids of different i overlap on purpose"""
    n = 1 + i % 3
    ids = [(7 * i + 11 * k) % 23 + 100 * k for k in range(n)]
    return part(ids, chain(ids)[::-1])


def deep_chain(n, seed):
    """one component whose labels need several hook rounds: a chain through the nodes in an order unrelated to
    their CSV order, ids shuffled as well"""
    rng = np.random.default_rng(seed)
    ids = rng.choice(10 ** 6, size=n, replace=False).astype(I64)
    walk = ids[rng.permutation(n)]
    rows = chain(list(walk))
    return part(ids, [rows[k] for k in rng.permutation(len(rows))])


def sized(n, rows, base):
    """n nodes and exactly `rows` rows: self loops first (one node: nothing else exists), then a ring"""
    ids = [base + 3 * k for k in range(n)]
    r = [(ids[k % n], ids[(k + 1) % n]) for k in range(rows)]
    return part(ids, r)


# the half-size rule. HALF: 8 nodes, the component of the first four is exactly half of its event and keeps
# CSV order, although CPython's set order of {40, 13, 21, 8} is 40, 8, 13, 21. THIRD: 8 nodes, a component
# of three, under half: set order 50, 43, 45 against CSV order 45, 43, 50. The ids of BIG, HALF and THIRD are
# disjoint, so the three can also be merged into one event (the self-check does).
HALF = part([40, 13, 21, 8, 1000, 1001, 1002, 1003], chain([40, 13, 21, 8]))
THIRD = part([45, 43, 50, 2000, 2001, 2002, 2003, 2004], chain([45, 43, 50]))
BIG = random_event(31, 200, 260, 10 ** 5, 0.5)
BIG = (BIG[0] + 10 ** 4, BIG[1] + 10 ** 4, BIG[2] + 10 ** 4)

A60 = random_event(32, 60, 70, 500, 0.3)
A60_OTHER_ROWS = (A60[0], A60[2][::-1].copy(), np.roll(A60[1], 3))
EMPTY = part([])
ROWS_ONLY = part([], [(4, 9), (9, 5)])
TOP = (1 << 61) - 2   # the largest legal id


def _random_batch(seed):
    rng = np.random.default_rng(900 + seed)
    k = int(rng.integers(3, 7))
    return [random_event(1000 * seed + e, int(rng.integers(50, 401)), int(rng.integers(40, 500)),
                         int(rng.choice([600, 10 ** 6, 2 ** 40])), float(rng.choice([0.0, 0.3, 0.7])))
            for e in range(k)]


CASES = {
    "half_size": [BIG, HALF, THIRD],
    "same_twice": [A60, A60],
    "same_ids_other_rows": [A60, A60_OTHER_ROWS],
    "foreign_end": [part([1, 2, 3], [(1, 2), (2, 7)]), part([7, 8], [(7, 8)])],
    "dup_across": [part([1, 2], [(1, 2)]), part([5]), part([1, 3], [(3, 1)])],
    "empty_first": [EMPTY, A60, HALF],
    "empty_middle": [HALF, EMPTY, EMPTY, A60],
    "empty_last": [A60, THIRD, EMPTY],
    "all_empty": [EMPTY, ROWS_ONLY, EMPTY],
    "nodes_no_rows": [HALF, part([9, 3, 4]), THIRD],
    "rows_no_nodes": [HALF, ROWS_ONLY, THIRD],
    "k1": [A60],
    "tiny65": [tiny(i) for i in range(65)],
    "tiny257": [tiny(i) for i in range(257)],
    "tiny2049": [tiny(i) for i in range(2049)],
    "block_boundary": [sized(255, 255, 10), sized(1, 1, 10), sized(257, 257, 10)],
    "loops_repeats": [HALF, part([5, 6, 7, 8], [(5, 5), (5, 6), (6, 5), (5, 6), (7, 7), (6, 7), (6, 7), (8, 8)]), A60],
    "deep_chain": [part([1, 2], [(2, 1)]), deep_chain(300, 33), part([4, 5, 6], [(4, 5)])],
    "dense_ids": [part([TOP, TOP - 8, TOP - 16, 3, TOP - 1, TOP - 2, TOP - 3, TOP - 5],
                       chain([TOP, TOP - 8, TOP - 16]) + [(3, TOP - 1)]),
                  part([TOP - 8, TOP, 5], [(TOP, TOP - 8)])],
}
for _s in range(5):
    CASES["random%d" % _s] = _random_batch(_s)

# a repeated id inside event 1 of 3 (an error naming event 1); events 0 and 2 share an id, which is fine
DUP_INSIDE = [part([1, 2, 3], [(1, 2)]), part([4, 5, 4], [(4, 5)]), part([1, 9], [(1, 9)])]

_REF = {}


def reference(name):
    """(arrays incl. "event", n_edges, n_subgraphs) of io.csr_from_rows_batch(CASES[name]) on the host"""
    if name not in _REF:
        _REF[name] = io.csr_from_rows_batch(CASES[name])
    return _REF[name]


def track_graph(ids, a, b):
    """the structure of one event's TrackGraph, assembled from io.csr_from_rows as io.build_event_csr does
    (no coordinates: the payload is not the builder's)"""
    N = int(ids.size)
    o, E, n_sub = io.csr_from_rows(ids, a, b)
    order = o["order"][:N].astype(np.int64)
    node, slot = empty_arrays(NODE_FIELDS, N), empty_arrays(SLOT_FIELDS, E)
    node["has_tse"][:] = 1
    for k in ("is_edge", "rev_edge", "act"):
        slot[k][:] = 1
    node["tag"] = ids[order]
    node["node_id"] = ids[order]
    node["sub_id"] = o["sub_id"][:N].copy()
    src = o["slot_src"][:E].copy()
    slot["slot_src"] = src
    slot["slot_key"] = ids[order][src] if E else np.zeros(0, np.int64)
    slot["tse_rank"] = o["tse_rank"][:E].copy()
    g = TrackGraph(N, E, o["slot_ptr"].copy(), o["out_ptr"].copy(), o["out_slot"][:E].copy(), node, slot, n_sub)
    check_layout(g)
    return g, order
