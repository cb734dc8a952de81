"""tests/build_batch_cases.py on the CPU: io.csr_from_rows_batch(parts) -- the host definition of the batch
build -- equals the structure arrays and the event column of gtf.graph.concat of the events' own
TrackGraphs, and every hand-made case really reaches the branch it is named for. No GPU."""
import numpy as np
import pytest

import build_batch_cases as bb
from gtf import graph, io


def _offsets(parts):
    return np.concatenate([[0], np.cumsum([p[0].size for p in parts])]).astype(np.int64)


def _event_slice(name, e, key="order"):
    """event e's piece of a node array of the case's reference"""
    off = _offsets(bb.CASES[name])
    return bb.reference(name)[0][key][off[e]:off[e + 1]]


@pytest.mark.parametrize("name", list(bb.CASES))
def test_batch_definition_is_concat_of_the_events(name):
    parts = bb.CASES[name]
    o, E, B = bb.reference(name)
    built = [bb.track_graph(*p) for p in parts]
    off = _offsets(parts)
    N = int(off[-1])
    exp_event = np.repeat(np.arange(len(parts), dtype=np.int32), [p[0].size for p in parts])
    assert np.array_equal(o["event"], exp_event) and o["event"].dtype == np.int32
    order = [b[1] + off[e] for e, b in enumerate(built)]
    assert np.array_equal(o["order"], np.concatenate(order) if order else np.zeros(0))
    if not any(g.n_nodes for g, _ in built):
        assert (E, B, N) == (0, 0, 0) and o["slot_ptr"].tolist() == [0] and o["out_ptr"].tolist() == [0]
        return
    exp = graph.concat([g for g, _ in built])
    assert (exp.n_nodes, exp.n_slots, exp.n_edges, exp.n_subgraphs) == (N, E, E, B)
    for k, want in (("slot_ptr", exp.slot_ptr), ("out_ptr", exp.out_ptr), ("out_slot", exp.out_slot),
                    ("slot_src", exp.slot["slot_src"]), ("tse_rank", exp.slot["tse_rank"]),
                    ("sub_id", exp.node["sub_id"])):
        assert o[k].dtype == np.int32 and np.array_equal(o[k], want), k
    assert sorted(o["order"].tolist()) == list(range(N))
    for e in range(len(parts)):   # event e's packed nodes are the positions [off[e], off[e + 1])
        piece = o["order"][off[e]:off[e + 1]]
        assert piece.size == 0 or (piece.min() >= off[e] and piece.max() < off[e + 1])


def test_half_size_rule_counts_the_components_own_event():
    off = _offsets(bb.CASES["half_size"])
    half, third = _event_slice("half_size", 1) - off[1], _event_slice("half_size", 2) - off[2]
    assert half[:4].tolist() == [0, 1, 2, 3]                       # 2|c| == |G_e|: CSV order
    assert sorted(third[:3].tolist()) == [0, 1, 2] and third[:3].tolist() != [0, 1, 2]   # under half: set order
    # the same three events as ONE event (disjoint ids): both components are far below half of the 216 nodes
    # and the four-node one leaves CSV order -- what a batch build that compares with N would give
    merged = tuple(np.concatenate([p[i] for p in bb.CASES["half_size"]]) for i in range(3))
    assert np.unique(merged[0]).size == merged[0].size == 216
    om = io.csr_from_rows(*merged)[0]["order"][:216]
    where = {int(v): i for i, v in enumerate(om)}
    four = sorted(where[int(off[1]) + k] for k in range(4))
    assert four == list(range(four[0], four[0] + 4))               # still one component, contiguous
    assert [int(om[i]) - int(off[1]) for i in four] != [0, 1, 2, 3]


def test_same_event_twice_and_shared_ids():
    o, E, B = bb.reference("same_twice")
    one, e1, b1 = io.csr_from_rows(*bb.A60)
    assert (E, B) == (2 * e1, 2 * b1)
    assert np.array_equal(o["order"][60:] - 60, o["order"][:60]) and np.array_equal(o["tse_rank"][e1:], o["tse_rank"][:e1])
    o2, E2, _ = bb.reference("same_ids_other_rows")
    assert np.array_equal(bb.CASES["same_ids_other_rows"][0][0], bb.CASES["same_ids_other_rows"][1][0])
    assert not np.array_equal(o2["slot_src"][e1:] - 60, o2["slot_src"][:e1]) or E2 != 2 * e1
    # dup_across: event 0 and event 2 both hold id 1
    ids0, ids2 = bb.CASES["dup_across"][0][0], bb.CASES["dup_across"][2][0]
    assert np.intersect1d(ids0, ids2).tolist() == [1] and bb.reference("dup_across")[1] == 4


def test_foreign_row_end_is_dropped():
    parts = bb.CASES["foreign_end"]
    o, E, B = bb.reference("foreign_end")
    assert E == 4 and B == 3                                       # (1, 2) and (7, 8) only; node 3 alone
    merged = tuple(np.concatenate([p[i] for p in parts]) for i in range(3))
    assert io.csr_from_rows(*merged)[1] == 6                       # one event: the row (2, 7) is kept


def test_duplicate_id_names_its_event():
    with pytest.raises(RuntimeError, match=r"duplicate node id.*event 1"):
        io.csr_from_rows_batch(bb.DUP_INSIDE)
    assert np.intersect1d(bb.DUP_INSIDE[0][0], bb.DUP_INSIDE[2][0]).size == 1
    ok = [bb.DUP_INSIDE[0], bb.part([4, 5], [(4, 5)]), bb.DUP_INSIDE[2]]
    assert io.csr_from_rows_batch(ok)[1] == 6


def test_empty_and_one_sided_events():
    for name, empty in (("empty_first", [0]), ("empty_middle", [1, 2]), ("empty_last", [2]), ("all_empty", [0, 1, 2])):
        sizes = [p[0].size for p in bb.CASES[name]]
        assert [i for i, n in enumerate(sizes) if n == 0] == empty, name
    assert bb.CASES["all_empty"][1][1].size == 2 and bb.reference("all_empty")[1:] == (0, 0)
    parts = bb.CASES["nodes_no_rows"]
    assert parts[1][0].size == 3 and parts[1][1].size == 0
    assert bb.reference("nodes_no_rows")[2] == sum(io.csr_from_rows(*p)[2] for p in parts)
    parts = bb.CASES["rows_no_nodes"]
    assert parts[1][0].size == 0 and parts[1][1].size == 2
    for k in bb.io.BATCH_CSR:
        assert np.array_equal(bb.reference("rows_no_nodes")[0][k], io.csr_from_rows_batch([parts[0], parts[2]])[0][k]), k
    assert len(bb.CASES["k1"]) == 1


def test_many_tiny_parts_and_block_boundaries():
    for name, k in (("tiny65", 65), ("tiny257", 257), ("tiny2049", 2049)):
        parts = bb.CASES[name]
        assert len(parts) == k and {p[0].size for p in parts} == {1, 2, 3}
        assert bb.reference(name)[2] == k                          # every tiny event is one component
    parts = bb.CASES["block_boundary"]
    assert [p[0].size for p in parts] == [255, 1, 257] and [p[1].size for p in parts] == [255, 1, 257]
    assert _offsets(parts)[1] // 256 == (_offsets(parts)[2] - 1) // 256 == 0   # two boundaries inside block 0


def test_loops_repeats_deep_chain_and_dense_ids():
    ids, a, b = bb.CASES["loops_repeats"][1]
    assert (a == b).sum() == 3 and len(set(zip(a.tolist(), b.tolist()))) < a.size
    assert io.csr_from_rows(ids, a, b)[1] == 7       # (5, 6), (6, 7) in both directions, one edge per self loop
    ids, a, b = bb.CASES["deep_chain"][1]
    o, E, B = io.csr_from_rows(ids, a, b)
    assert (ids.size, E, B) == (300, 598, 1)
    # a chain in an order unrelated to the CSV order: the minimum label needs more than one hook round
    lab = np.arange(300)
    idx = {int(v): i for i, v in enumerate(ids)}
    u, v = np.array([idx[int(x)] for x in a]), np.array([idx[int(x)] for x in b])
    lo = np.minimum(lab[u], lab[v])
    np.minimum.at(lab, u, lo)
    np.minimum.at(lab, v, lo)
    assert lab.max() > 0
    assert all(io.csr_from_rows(*p)[2] <= 2 for i, p in enumerate(bb.CASES["deep_chain"]) if i != 1)
    ids = bb.CASES["dense_ids"][0][0]
    assert ids.max() == (1 << 61) - 2 and bb.reference("dense_ids")[1] == 8
    third = _event_slice("dense_ids", 0)[:3].tolist()
    assert sorted(third) == [0, 1, 2]


def test_random_batches_have_the_asked_shape():
    for s in range(5):
        parts = bb.CASES["random%d" % s]
        assert 3 <= len(parts) <= 6 and all(50 <= p[0].size <= 400 for p in parts)
