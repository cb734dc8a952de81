"""The directed inputs of tests/subset_cases.py hold what they claim (CPU): the branches of
gtf.graph.subset that the device version has to reproduce are all present, counted on the
host result."""
import numpy as np
import pytest

import subset_cases as sc
from gtf import graph


@pytest.mark.parametrize("name", sc.NAMES)
def test_case_is_well_formed(name):
    g, keep, h, nm, sm = sc.case(name)
    graph.check_layout(g)
    graph.check_layout(h)
    assert keep.shape == (g.n_nodes,) and keep.dtype == bool
    assert np.array_equal(nm, np.nonzero(keep)[0])
    assert sm.shape == (h.n_slots,) and np.unique(sm).size == sm.size
    for f in ("slot_key", "tse_rank", "uts_rank", "tse_mw", "uts_xyzr"):   # slot_map is the gather map
        assert np.array_equal(g.slot[f][sm], h.slot[f], equal_nan=True), f
    # the invariant gtf_refresh_send_mw searches by: non-orphan slots ascend by sender, orphans last
    for t in (g, h):
        src = t.slot["slot_src"].astype(np.int64)
        key = np.where(src >= 0, src, t.n_nodes)
        inner = np.ones(t.n_slots, bool)
        inner[t.slot_ptr[:-1][np.diff(t.slot_ptr) > 0]] = False
        assert np.all((np.diff(key, prepend=0) > 0)[inner & (src >= 0)])
        assert np.all((np.diff(key, prepend=0) >= 0)[inner])
    # the input's send_mw is what refresh_send_mw gives, so a subset keeps it consistent
    assert np.array_equal(graph.refresh_send_mw(g.copy()).slot["send_mw"], g.slot["send_mw"], equal_nan=True)
    assert np.array_equal(graph.subset(g, keep).slot["send_mw"], h.slot["send_mw"], equal_nan=True)


def test_boundary_case_has_every_branch():
    c = sc.census("boundary")
    g, keep, h, _, _ = sc.case("boundary")
    assert np.all(keep[np.diff(g.slot_ptr) >= 65]) and 0.45 < keep.mean() < 0.75
    assert c["tse_only"] >= 20 and c["uts_only"] >= 20 and c["both"] >= 20, c
    assert c["reordered_segments"] >= 10, c
    assert c["big_segments"] >= 1 and c["largest_segment"] > 64, c
    assert c["vanished_edge_only"] >= 20, c
    assert c["inside_non_edge"] >= 5, c
    assert c["slot_free_nodes"] >= 1 and c["senders_losing_all"] >= 1, c
    assert c["subgraphs_removed"] >= 1 and c["solo_subgraphs"] >= 1 and not c["sub_id_monotone"], c
    assert int(h.node["sub_id"].max()) + 1 == h.n_subgraphs < g.n_subgraphs


def test_second_round_mixes_old_and_new_orphans():
    both = [sc.census("dropin_%s_%s_again" % (n, k))["both"] for n, k, _ in sc.DROPIN]
    assert sum(b >= 6 for b in both) >= 3, both
    for n, k, _ in sc.DROPIN:
        g, keep, h, _, _ = sc.case("dropin_%s_%s_again" % (n, k))
        assert int((g.slot["slot_src"] < 0).sum()) > 0 and int((h.slot["slot_src"] < 0).sum()) > 0


def test_tiny200_and_the_trivial_masks():
    c = sc.census("tiny200")
    assert sc.case("tiny200")[2].n_slots == 1837 and c["orphans"] == 643
    g, keep, h, nm, sm = sc.case("all")
    assert h.n_nodes == g.n_nodes and np.array_equal(nm, np.arange(g.n_nodes)) and np.array_equal(sm, np.arange(g.n_slots))
    g, keep, h, nm, sm = sc.case("none")
    assert h.n_nodes == 0 and h.n_slots == 0 and h.n_edges == 0
