"""The directed candidate-order inputs of order_cases.py on the CPU: the host function
gtf_candidate_order equals the reference's networkx orders on them (so it is the yardstick the
GPU tests compare gtf_candidate_order_device with), and the cases reach what they exist for."""
import numpy as np

import order_cases as oc


def _components():
    """(order key from networkx, per candidate: subgraph, members in candidate order, set-ordered?)"""
    subs, g, names = oc.event()
    key, cands = oc.expected_nx(subs)
    sizes = [len(s) for s in subs]
    cut = [any(d["activated"] == 0 for _, _, d in s.edges(data=True)) for s in subs]
    return subs, g, names, key, [(si, m, cut[si] and 2 * len(m) < sizes[si]) for si, m in cands]


def test_host_order_equals_networkx():
    from gtf.extract import candidate_order
    subs, g, _, key, _ = _components()
    assert g.n_nodes == sum(len(s) for s in subs) > 256
    assert np.array_equal(candidate_order(g), key)


def test_cases_reach_their_branches():
    subs, g, names, key, comps = _components()
    nid = g.node["node_id"]
    by_sub = lambda name: [(m, so) for si, m, so in comps if si == names[name]]   # noqa: E731
    # no deactivated edge: one candidate whatever the connectivity, in node order
    (m, so), = by_sub("whole")
    assert not so and m == sorted(m) and len(m) == 6
    # exactly half: rank order; one fewer than half and the singleton: set order
    h = {len(m): (m, so) for m, so in by_sub("halves")}
    assert set(h) == {4, 3, 1} and not h[4][1] and h[3][1] and h[1][1] and h[4][0] == sorted(h[4][0])
    assert any(so and len(m) == 5 for m, so in by_sub("five"))
    assert any(so and len(m) == 25 for m, so in by_sub("twentyfive"))
    assert sorted(len(m) for m, so in by_sub("big") if so) == [20] * 7
    assert sorted(len(m) for m, _ in by_sub("one_way")) == [2, 2, 6]
    # the ids: collisions modulo 8 and modulo 32, and ids next to 2^61 - 1
    for name, step in (("mod8", 8), ("twentyfive", 32)):
        ids = np.array([nid[v] for m, _ in by_sub(name) for v in m])
        assert len(set(ids % step)) == 1 and (ids > oc.TOP - 64 * step).sum() >= 3
    assert nid.min() >= 0 and nid.max() < oc.TOP
    # a sorted order would not pass: set-ordered components whose order is neither ascending
    # node index nor ascending node id
    mixed = [m for _, m, so in comps if so and m != sorted(m) and m != sorted(m, key=lambda v: nid[v])]
    assert len(mixed) >= 3
    assert max(len(m) for m in mixed) >= 20
    # the members of a component are not contiguous in node order
    assert any(so and max(m) - min(m) >= 2 * len(m) for _, m, so in comps)
