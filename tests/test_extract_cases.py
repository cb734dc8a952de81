"""The directed extraction events of extract_cases.py, checked on the oracle alone: every
case reaches the branch it exists for (recomputed from the oracle's own helpers), every
fit whose p-value the GPU test compares is well conditioned (+-1 ulp on every coordinate
moves the oracle's own p-value by <= 1e-8 in _pclose's metric, a tenth of the GPU bar),
and the kernel's emulation of CPython's set order, restated here, is CPython's."""
import numpy as np
import pytest

import extract_cases as X
import gtf_oracle as O

NOISE_BAR = 1e-8
M64 = (1 << 64) - 1


# ------------------------------------------------------------------ the kernel's set order, restated
def kernel_tuple_hash(a, b):
    """py_tuple_hash2 of gtf_extract.hip"""
    P1, P2, P5 = 11400714785074694791, 14029467366897019727, 2870177450012600261
    acc = P5
    for it in (a, b):
        hv = int(it)
        lane = (-2 if hv == -1 else hv) & M64
        acc = (acc + lane * P2) & M64
        acc = ((acc << 31) | (acc >> 33)) & M64
        acc = (acc * P1) & M64
    acc = (acc + (2 ^ (P5 ^ 3527539))) & M64
    return 1546275796 if acc == M64 else acc


def kernel_set_slot(h, occupied):
    """py_set_slot: the minimum 8-slot table, no linear probes (i + 9 > mask)"""
    i, perturb = h & 7, h
    while i == occupied:
        perturb >>= 5
        i = (i * 5 + 1 + perturb) & 7
    return i


def kernel_order(a, b):
    sa = kernel_set_slot(kernel_tuple_hash(*a), -1)
    sb = kernel_set_slot(kernel_tuple_hash(*b), sa)
    return [b, a] if sb < sa else [a, b]


def test_set_order_grid_matches_cpython():
    pairs = X.grid_pairs()
    a_first = collisions = 0
    for a, b in pairs:
        for u, v in ((a, b), (b, a)):
            assert kernel_tuple_hash(*u) == hash(u) & M64
            assert kernel_order(u, v) == list(set([u, u, v, v])), (u, v)
            # the reference builds the set from numpy scalars in candidate order
            assert kernel_order(u, v) == list(set([tuple(np.array(t)) for t in (u, v, u, v)]))
        a_first += kernel_order(a, b) == [a, b]
        collisions += (kernel_tuple_hash(*a) & 7) == (kernel_tuple_hash(*b) & 7)
    print("grid: %d pairs, A first %d, B first %d, same home slot %d" % (len(pairs), a_first, len(pairs) - a_first,
                                                                         collisions))
    assert len(pairs) >= 59
    assert a_first >= 20 and len(pairs) - a_first >= 20        # both orders
    assert collisions >= 8                                      # the probe path


@pytest.mark.parametrize("swap", [False, True])
def test_set_order_event_mutates_where_the_merging_tuple_comes_first(swap):
    cands = X.set_order_cands(swap)
    g, vivl = X.build(cands)
    p = X.extract_params()
    o = X.oracle(g, vivl, p)
    assert len(o["records"]) == len(cands)
    changed = np.nonzero((o["gnn_after"] != g.node["gnn"]).any(1))[0]
    expect = []
    for rec, c in zip(o["records"], cands):
        assert rec["status"] == "bad" and len(rec["nodes"]) == 6
        a, b = tuple(c[0][3:]), tuple(c[1][3:])
        d = lambda i, j: np.sqrt(sum((c[i][k] - c[j][k])**2 for k in range(3)))   # noqa: E731
        assert tuple(c[2][3:]) == a and tuple(c[3][3:]) == b and d(0, 2) <= p.merge < d(1, 3)
        if list(set([a, b, a, b])) == [a, b]:
            expect.append(int(rec["nodes"][0]))
    assert changed.tolist() == expect
    assert 20 <= len(expect) <= len(cands) - 20
    print("set-order event (swap=%s): %d of %d candidates mutated" % (swap, len(expect), len(cands)))


# ------------------------------------------------------------------ branch cases
def _by_name(cases, orc):
    names, off = list(cases), X.offsets(list(cases.values()))
    return {names[int(np.searchsorted(off, r["nodes"][0], "right")) - 1]: r for r in orc["records"]}


def test_branch_cases_reach_their_branches():
    g, vivl, cases = X.cached("branch")
    p = X.extract_params()
    o = X.oracle(g, vivl, p)
    rec = _by_name(cases, o)
    assert list(rec) == list(cases), "every case is one candidate"
    for name, r in rec.items():
        assert len(r["nodes"]) == len(cases[name]), name
    assert len(np.unique(g.node["sub_id"])) < len(cases), "joined candidates share a subgraph"
    assert [(int(s), len(n)) for s, n in O.active_components(g)] == [(r["sub"], len(r["nodes"])) for r in o["records"]]
    fit = {n: X.fit_inputs(g, vivl, r, p) for n, r in rec.items() if r["status"] in ("rejected", "extracted")}
    zabs = lambda n: np.abs([c[2] for c in fit[n][2][1:]])      # |z'| of every hit the endcap branch reads  # noqa: E731
    assert zabs("barrel").max() < p.endcap
    assert zabs("endcap").min() >= p.endcap
    assert zabs("mixed").min() < p.endcap <= zabs("mixed").max()
    for n in fit:
        rr = [c[3] for c in fit[n][1]]
        d = np.sqrt(sum((fit[n][1][-1][i] - fit[n][1][-2][i])**2 for i in range(3)))
        assert (len(rr) != len(set(rr))) == (n in ("tie", "samexy")), n
        assert (d < p.separation) == (n == "sep"), n
        assert fit[n][3] == (n in ("merge1", "merge2")), n
    rr = [c[3] for c in fit["tie"][1]]
    i = [k for k in range(len(rr) - 1) if rr[k] == rr[k + 1]]
    assert len(i) == 1 and fit["tie"][1][i[0]][0] == fit["tie"][1][i[0] + 1][1]      # (x, y) and (y, x)
    assert 3.0 <= np.sqrt(sum((fit["sep"][1][-1][k] - fit["sep"][1][-2][k])**2 for k in range(3))) <= 4.0
    status = {n: r["status"] for n, r in rec.items()}
    assert status == {"barrel": "extracted", "endcap": "extracted", "mixed": "extracted", "tie": "extracted",
                      "sep": "extracted", "samexy": "rejected", "triple": "bad", "merge1": "extracted",
                      "merge2": "extracted", "merge_short": "bad", "four": "extracted", "three": "fragment",
                      "single": "fragment"}
    assert np.isnan(rec["samexy"]["pval_xy"]) and np.isnan(rec["samexy"]["pval_zr"])
    # merges: the fit runs on the midpoint with its recomputed r, and the first node keeps it
    changed = np.nonzero((o["gnn_after"] != g.node["gnn"]).any(1))[0]
    first = lambda n: int(rec[n]["nodes"][0])                   # noqa: E731
    assert changed.tolist() == [first("merge1") + 3, first("merge2"), first("merge2") + 5, first("merge_short") + 1]
    an, coords, _, _ = fit["merge1"]
    assert len(an) == 6 and tuple(o["gnn_after"][first("merge1") + 3]) in coords
    m = o["gnn_after"][first("merge1") + 3]
    assert m[3] == np.sqrt(m[0]**2 + m[1]**2) and m[3] != g.node["xyzr"][first("merge1") + 3, 3]
    assert len(fit["merge2"][0]) == 6
    assert len(rec["four"]["nodes"]) == p.numhits and len(rec["three"]["nodes"]) == p.numhits - 1


def test_rotate_track_fallback_and_radius_order_decide_the_p_values():
    """the sep and tie cases are not vacuous: without the fallback, or with the tied pair
    in the other order, the oracle's own p-values move by far more than the GPU bar"""
    g, vivl, cases = X.cached("branch")
    p = X.extract_params()
    rec = _by_name(cases, X.oracle(g, vivl, p))
    _, coords, _, _ = X.fit_inputs(g, vivl, rec["sep"], p)
    pv = O.kf_track_fit_moliere(p.sigma0xy, p.sigma0rz, O.rotate_track(coords, 0.0), p.endcap)
    assert X.pdist(pv[0], rec["sep"]["pval_xy"]) > 1e-4 or X.pdist(pv[1], rec["sep"]["pval_zr"]) > 1e-4
    _, coords, _, _ = X.fit_inputs(g, vivl, rec["tie"], p)
    i = [k for k in range(len(coords) - 1) if coords[k][3] == coords[k + 1][3]][0]
    coords[i], coords[i + 1] = coords[i + 1], coords[i]
    pv = O.kf_track_fit_moliere(p.sigma0xy, p.sigma0rz, O.rotate_track(coords, p.separation), p.endcap)
    assert X.pdist(pv[0], rec["tie"]["pval_xy"]) > 1e-4 or X.pdist(pv[1], rec["tie"]["pval_zr"]) > 1e-4


def test_branch_fits_are_well_conditioned():
    g, vivl, cases = X.cached("branch")
    noise = X.ulp_noise(g, vivl, X.extract_params(), frozen=X.branch_frozen(cases))
    print("branch event: largest +-1 ulp noise %.2e" % max(noise.values()))
    assert len(noise) == 9 and max(noise.values()) <= NOISE_BAR, noise
    # the same hits in reversed candidate order (the order_key test's event B)
    cands, joins = list(cases.values()), X.branch_cases()[1]
    gb, vb = X.build(X.reverse(cands), joins)
    mapped = [int(X.order_map(cands)[v]) for v in X.branch_frozen(cases)]
    noise = X.ulp_noise(gb, vb, X.extract_params(), frozen=mapped)
    assert len(noise) == 9 and max(noise.values()) <= NOISE_BAR, noise


def test_tie_fit_is_well_conditioned_in_the_tied_hits():
    """ulp_noise leaves x, y, r of the tied pair alone (one ulp on either hit removes the
    tie); here the pair moves together, (x, y) -> (x', y') and its mirror to (y', x'), so
    the radii stay bit-equal and the fit's sensitivity to those hits is measured too"""
    g, vivl, cases = X.cached("branch")
    p = X.extract_params()
    a = int(X.offsets(list(cases.values()))[list(cases).index("tie")]) + 2
    base = {int(r["nodes"][0]): r for r in X.oracle(g, vivl, p)["records"]}[a - 2]
    worst = 0.0
    for d in range(5):
        rng = np.random.default_rng(2000 + d)
        h = g.copy()
        x, y = np.nextafter(h.node["xyzr"][a, :2], np.where(rng.random(2) < 0.5, -np.inf, np.inf))
        r = np.sqrt(x * x + y * y)
        h.node["xyzr"][a, [0, 1, 3]] = x, y, r
        h.node["xyzr"][a + 1, [0, 1, 3]] = y, x, r
        h.node["gnn"] = h.node["xyzr"].copy()
        got = {int(q["nodes"][0]): q for q in X.oracle(h, vivl, p)["records"]}[a - 2]
        _, coords, _, _ = X.fit_inputs(h, vivl, got, p)
        assert len({c[3] for c in coords}) == len(coords) - 1, "still tied"
        worst = max(worst, float(X.pdist(got["pval_xy"], base["pval_xy"])), float(X.pdist(got["pval_zr"], base["pval_zr"])))
    print("tie case, tied hits moved together: noise %.2e" % worst)
    assert worst <= NOISE_BAR


def test_components_and_no_slot_fits_are_well_conditioned():
    g, vivl, _ = X.cached("components")
    noise = X.ulp_noise(g, vivl, X.extract_params())
    print("components event: largest +-1 ulp noise %.2e" % max(noise.values()))
    assert len(noise) == 4 and max(noise.values()) <= NOISE_BAR, noise
    g, vivl = X.graph(X.track(31), [], sub_id=[0] * 6)
    noise = X.ulp_noise(g, vivl, X.extract_params())
    print("no-slot event: +-1 ulp noise %.2e" % max(noise.values()))
    assert len(noise) == 1 and max(noise.values()) <= NOISE_BAR, noise


def test_chi2_sums_on_the_record_give_the_p_values():
    from scipy.stats import chi2
    g, vivl = X.cached("regimes")
    o = X.oracle(g, vivl, X.extract_params())
    for r in o["records"]:
        dof = len(r["nodes"]) - 2
        assert chi2.sf(r["chi2_xy"], dof) == r["pval_xy"] and chi2.sf(r["chi2_zr"], dof) == r["pval_zr"]


# ------------------------------------------------------------------ p-value regimes
def test_regime_cases_are_admitted_and_cover_every_regime():
    g, vivl = X.cached("regimes")
    assert g.n_nodes < 5000
    ps, statuses, dofs = [], set(), set()
    for scale in X.REGIME_SCALES:
        o, adm, noise = X.regime_admission(scale)
        assert len(o["records"]) == len(X.REGIME_HITS) * len(X.REGIME_SCATTER)
        print("sigma0 x %g: largest +-1 ulp noise %.2e, admitted p-values %d of %d" % (
            scale, max(noise.values()), sum(map(sum, adm.values())), 2 * len(adm)))
        for r in o["records"]:
            k = int(r["nodes"][0])
            assert r["status"] in ("rejected", "extracted")
            # a condition on the inputs: every candidate of the event is well conditioned
            assert noise[k] <= NOISE_BAR, (scale, len(r["nodes"]), noise[k])
            for key, c2, ok in (("pval_xy", "chi2_xy", adm[k][0]), ("pval_zr", "chi2_zr", adm[k][1])):
                if not ok:
                    continue
                assert not 0 < r[key] < 1e-290
                assert r[key] > 0 or r[c2] / 2 > 800        # an admitted zero is far past MAXLOG
                ps.append(r[key])
                dofs.add(len(r["nodes"]) - 2)
            if all(adm[k]):
                statuses.add(r["status"])
    ps = np.array(ps)
    for lo, hi, name in ((1e-290, 1e-30, "deep tail"), (1e-30, 0.01, "tail")):
        assert ((ps > lo) & (ps < hi)).any(), name
    assert (ps == 0).any() and ((ps >= 0.01) & (ps <= 0.99)).any() and ((ps > 0.99) & (ps <= 1)).any()
    assert statuses == {"rejected", "extracted"}                # both sides of p_accept
    assert dofs == {n - 2 for n in X.REGIME_HITS}
    assert (ps[ps > 0.99] < 1).any()                            # the igam series arm, short of 1


# ------------------------------------------------------------------ components
def test_components_event_splits_as_intended():
    g, vivl, M = X.cached("components")
    assert 3900 <= g.n_nodes < 5000
    comps = O.active_components(g)
    big = [(s, n) for s, n in comps if s == 0]
    assert sorted(len(n) for _, n in big) == [900, 1023, 2048]
    assert all(np.ptp(n) > M // 2 for _, n in big), "components interleave under the permuted numbering"
    assert [(s, len(n)) for s, n in comps if s > 0] == [(1, 10), (1, 5), (2, 10), (3, 2), (3, 3), (3, 5)]
    o = X.oracle(g, vivl, X.extract_params())
    assert [r["status"] for r in o["records"]][:3] == ["bad"] * 3
    # subgraph 1: the one-way edge is its only deactivated slot
    dst = g.slot_dst()
    dead = np.nonzero(g.slot["act"] == 0)[0]
    s1 = [k for k in dead if g.node["sub_id"][dst[k]] == 1]
    assert len(s1) == 1
    u, v = int(g.slot["slot_src"][s1[0]]), int(dst[s1[0]])
    back = [k for k in range(g.slot_ptr[u], g.slot_ptr[u + 1]) if g.slot["slot_src"][k] == v]
    assert len(back) == 1 and g.slot["act"][back[0]] == 1
    assert not (g.node["sub_id"][dst[dead]] == 2).any()
    # the empty-slot events
    for sub in (None, [0] * 6):
        h, _ = X.graph(X.track(31), [], sub_id=sub)
        assert h.n_slots == 0 and h.n_nodes == 6


# ------------------------------------------------------------------ order_key
def test_reversed_event_moves_the_merged_rows():
    g, vivl, cases = X.cached("branch")
    cands, joins = list(cases.values()), X.branch_cases()[1]
    m = X.order_map(cands)
    gb, vb = X.build(X.reverse(cands), joins)
    assert np.array_equal(gb.node["xyzr"][m], g.node["xyzr"]) and np.array_equal(vb[m], vivl)
    p = X.extract_params()
    oa, ob = X.oracle(g, vivl, p), X.oracle(gb, vb, p)
    assert [r["status"] for r in oa["records"]] == [r["status"] for r in ob["records"]]
    moved = (ob["gnn_after"][m] != oa["gnn_after"]).any(1)
    assert moved.sum() == 8, "each of the four merged pairs keeps the midpoint on its other node"
