"""gtf_extract_candidates against the oracle on the directed events of extract_cases.py
(test_extract_cases.py shows on the CPU that every case reaches its branch and that every
compared fit is well conditioned): labels, statuses, the candidate count, the extracted
flags, the outputs() groups and the GNN_Measurement mutations exact, p-values within 1e-7
in _pclose's metric, NaN meeting NaN.

Largest GPU-against-oracle p-value distance measured on an MI355X (every run prints it):
branch cases 7.3e-12, regimes 1.6e-10 / 2.0e-11 / 1.5e-11 / 8.3e-13 at sigma0 x 0.3 / 1 /
3 / 10, components 7.2e-12, order_key 7.4e-12, no slots 0 (the fixture: 2.2e-8)."""
import numpy as np
import pytest

import extract_cases as X
from test_extract import _pclose

pytestmark = pytest.mark.gpu

RTOL = 1e-7


def _same(a, b):
    return np.array_equal(a, b, equal_nan=np.asarray(a).dtype.kind == "f")


def _compare(g, p, res, orc, admitted=None, order_key=None, node_map=None):
    """res (extract.run on g) against the oracle's result orc. node_map: orc ran on another
    numbering of the same hits (node v of g is node node_map[v] there; candidates keep
    their first node). Returns the largest p-value distance."""
    from gtf import extract
    N = g.n_nodes
    m = np.arange(N) if node_map is None else np.asarray(node_map)
    inv = np.empty(N, np.int64)
    inv[m] = np.arange(N)
    assert res["n_candidates"] == len(orc["records"])
    label = np.full(N, -1)
    ext = np.zeros(N, np.uint8)
    worst = 0.0
    for rec in orc["records"]:
        nodes = inv[rec["nodes"]]
        root = int(nodes.min())
        assert root == int(rec["nodes"][0])
        label[nodes] = root
        assert res["status"][root] == X.CODE[rec["status"]], (root, rec["status"], res["status"][root])
        ext[nodes] = rec["status"] == "extracted"
        adm = (True, True) if admitted is None else admitted[root]
        for k, kk, ok in (("pval_xy", "pxy", adm[0]), ("pval_zr", "pzr", adm[1])):
            got, exp = res[kk][root], rec[k]
            if np.isnan(exp):
                assert np.isnan(got), (root, k, got)
            elif exp == 0:
                # an underflowed p: _pclose takes anything against 0, so exactly 0 here. Not
                # asked of a zero that is not admitted (chi2 / 2 short of 800: a subnormal
                # from one igamc may be a 0 from another)
                assert got == 0 or not ok, (root, k, got)
            elif ok:
                assert not np.isnan(got) and _pclose(got, exp, RTOL), (root, k, got, exp)
                worst = max(worst, float(X.pdist(got, exp)))
    assert np.array_equal(res["label"], label)
    assert np.array_equal(res["ext"], ext)
    assert _same(res["gnn"], orc["gnn_after"][m])
    out = extract.outputs(g, res, p.numhits, order_key)
    for k in ("extracted", "remaining", "fragments"):
        exp = [inv[c] for c in orc[k]]
        if order_key is None:
            exp = [np.sort(c) for c in exp]
        assert len(out[k]) == len(exp), k
        for a, b in zip(out[k], exp):
            assert np.array_equal(a if k == "extracted" else np.sort(a), b if k == "extracted" else np.sort(b)), k
    for k in ("pval_xy", "pval_zr"):
        assert out[k].shape == orc[k].shape
        if admitted is None:
            assert (orc[k] > 0).all() and _pclose(out[k], orc[k], RTOL).all(), k
    assert np.isfinite(worst)
    return worst


def _run(g, vivl, p, **kw):
    from gtf import extract
    return extract.run(g, vivl, p, **kw)


@pytest.mark.parametrize("swap", [False, True])
def test_set_order_decides_the_mutation(swap):
    """every candidate ends bad; the merging tuple's node keeps the midpoint exactly where
    CPython's set() yields that tuple first (23 of 60 candidates, 33 with the tuples
    swapped). No p-value is computed."""
    cands = X.set_order_cands(swap)
    g, vivl = X.build(cands)
    p = X.extract_params()
    orc = X.oracle(g, vivl, p)
    res = _run(g, vivl, p)
    _compare(g, p, res, orc)
    changed = (res["gnn"] != g.node["gnn"]).any(1)
    assert (res["status"][X.offsets(cands)[:-1]] == X.CODE["bad"]).all()
    assert 20 <= changed.sum() <= len(cands) - 20
    print("set order (swap=%s): %d of %d candidates mutated" % (swap, changed.sum(), len(cands)))


def test_branch_cases():
    """barrel / end-cap / mixed var_ms arms, a radius tie, the separation_3d fallback, a
    zero denominator (NaN, rejected), a triple, one and two merges, a merge below numhits,
    numhits and numhits - 1 hits and an isolated node, in one event."""
    g, vivl, _ = X.cached("branch")
    p = X.extract_params()
    worst = _compare(g, p, _run(g, vivl, p), X.oracle(g, vivl, p))
    print("branch cases: largest p-value distance %.2e" % worst)


@pytest.mark.parametrize("scale", X.REGIME_SCALES)
def test_p_value_regimes(scale):
    """4 to 40 hits (dof 2 to 38) at four scatter levels, sigma0 scaled: p from exactly 0
    through the deep tail to the igam series arm next to 1."""
    g, vivl = X.cached("regimes")
    p = X.extract_params(scale)
    orc, adm, _ = X.regime_admission(scale)
    worst = _compare(g, p, _run(g, vivl, p), orc, admitted=adm)
    print("regimes, sigma0 x %g: largest p-value distance %.2e over %d admitted p-values" % (
        scale, worst, sum(map(sum, adm.values()))))


def test_components():
    """a 2048-node path, a 900-node star and a 1023-node binary tree in one subgraph under a
    permuted numbering (several hooking rounds), a one-way deactivated edge, a sub_id
    override with and without a deactivated edge."""
    g, vivl, _ = X.cached("components")
    p = X.extract_params()
    worst = _compare(g, p, _run(g, vivl, p), X.oracle(g, vivl, p))
    print("components: largest p-value distance %.2e" % worst)


@pytest.mark.parametrize("one_subgraph", [False, True])
def test_event_without_slots(one_subgraph):
    g, vivl = X.graph(X.track(31), [], sub_id=[0] * 6 if one_subgraph else None)
    assert g.n_slots == 0
    p = X.extract_params()
    orc = X.oracle(g, vivl, p)
    assert [r["status"] for r in orc["records"]] == (["extracted"] if one_subgraph else ["fragment"] * 6)
    worst = _compare(g, p, _run(g, vivl, p), orc)
    print("no slots: largest p-value distance %.2e" % worst)


def test_order_key():
    """order_key = arange(N) is bit-equal to None; the reversed rank inside each candidate
    gives what the oracle gives on the event with every hit list reversed, under the node
    mapping (the mutated row of a merged pair moves to the pair's other node)."""
    g, vivl, cases = X.cached("branch")
    cands, joins = list(cases.values()), X.branch_cases()[1]
    p = X.extract_params()
    plain = _run(g, vivl, p)
    ident = _run(g, vivl, p, order_key=np.arange(g.n_nodes, dtype=np.int32))
    for k in plain:
        assert _same(plain[k], ident[k]), k
    m = X.order_map(cands)
    gb, vb = X.build(X.reverse(cands), joins)
    orc = X.oracle(gb, vb, p)
    res = _run(g, vivl, p, order_key=m)
    worst = _compare(g, p, res, orc, order_key=m, node_map=m)
    assert not _same(res["gnn"], plain["gnn"])
    print("order_key: largest p-value distance %.2e" % worst)
