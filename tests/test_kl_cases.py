"""The directed parabolic-KL cases (kl_cases.py) on the CPU, against the record of the reference's
own functions (tests/golden/kl_cases.npz, made by tests/golden/make_golden_kl_cases.py):

  * every case's claim holds on the record;
  * gtf_oracle.parabolic_states, parabolic_kl_pairs and parabolic_training_rows reproduce the record at
    the bars the oracle meets against the committed training CSV (kl 1e-8, emp_var 1e-9 relative, truth
    exact; states rtol 1e-8, atol 1e-12 max), and raise LinAlgError at the same nodes;
  * every singular case is classified from the record and from the kernel's stated rule, both in NumPy,
    and the class equals the one written in the case: "both", "kernel" (the rule raises where the
    reference returns unbounded values) or "reference" (a bug: there is none);
  * at least two thirds of the value cases are well-conditioned (the record within 1e-9 of exact_kl),
    the others are the named ill-conditioned ones; at least half are fp32-checked (exact_kl moves by at
    most 1e-4 when the states' (X0, XB, MB) move by 1 +- 2^-24).
"""
import numpy as np
import pytest

import gtf_oracle as O
import kl_cases as KC

NAMES = [c.name for c in KC.CASES]
BY = KC.BY_NAME


def rec_of(name):
    return KC.record()[name]


def test_record_covers_the_cases():
    from gtf import parabolic
    assert set(KC.record()) == set(NAMES)
    assert (KC.WIN_NODES, KC.WIN_MARGIN) == (parabolic.WIN_NODES, parabolic.WIN_MARGIN)
    for c in KC.CASES:
        r = rec_of(c.name)
        assert r["kl"].shape == r["truth"].shape == (int(c.pair_ptr()[-1]),) and r["gmean"].shape == (c.n_nodes,)
        assert ("sv" in r) == c.states and len(r["raised"]) == len(r["raised_nodes"])
        lo, hi = c.ptr[:-1], c.ptr[1:]
        assert not any(u in set(np.nonzero(c.degree)[0]) for u in set(c.src.tolist())), "a receiver has no out-edge"
        assert (lo <= hi).all() and c.n_nodes <= 2600


@pytest.mark.parametrize("name", NAMES)
def test_claim_holds_on_the_record(name):
    c = BY[name]
    assert c.check is not None or c.kind == "singular"
    if c.check is not None:
        c.check(c, rec_of(name))
    raised = set(rec_of(name)["raised_nodes"].tolist())
    assert np.isnan(rec_of(name)["kl"][~KC.compared_pairs(c, rec_of(name))]).sum() == sum(
        int(c.pair_ptr()[v + 1] - c.pair_ptr()[v]) for v in raised)
    if c.kind != "singular":
        assert not raised


def _close(a, b, rtol):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    with np.errstate(all="ignore"):
        return bool((same | (np.abs(a - b) <= rtol * np.abs(b))).all())


@pytest.mark.parametrize("name", NAMES)
def test_oracle_reproduces_the_record(name):
    c, r = BY[name], rec_of(name)
    pp = c.pair_ptr()
    raised = []
    for v in np.nonzero(c.degree > 0)[0]:
        lo, hi = int(c.ptr[v]), int(c.ptr[v + 1])
        try:
            with np.errstate(all="ignore"):
                st = O.parabolic_states(c.gnn[v], c.nbs(v))
                kl = O.parabolic_kl_pairs([s for s, _ in st], [cv for _, cv in st]) if hi - lo > 1 else []
        except np.linalg.LinAlgError:
            raised.append(int(v))
            continue
        if c.states:
            for k, (s, cv) in zip(range(lo, hi), st):
                assert np.allclose(s, r["sv"][k], rtol=1e-8, atol=1e-12 * np.abs(r["sv"][k]).max(), equal_nan=True), (v, k)
                assert np.allclose(cv, r["cov"][k], rtol=1e-8, atol=1e-12 * np.abs(r["cov"][k]).max(), equal_nan=True), (v, k)
        assert _close(kl, r["kl"][pp[v]:pp[v + 1]], 1e-8), v
    assert raised == r["raised_nodes"].tolist()
    if not raised:
        with np.errstate(all="ignore"):
            node, i, j, kl, ev, tr = O.parabolic_training_rows(KC.oracle_graph(c), c.truth)
        rows = KC.pair_rows(c)
        assert all(np.array_equal(a, b) for a, b in zip((node, i, j), rows))
        assert _close(kl, r["kl"], 1e-8) and _close(ev, r["gvar"][rows[0]], 1e-9)
        assert np.array_equal(tr, r["truth"])


def test_singular_classes():
    """per singular case: what the record and the kernel's rule do at its receivers"""
    table = {}
    for c in KC.CASES:
        cls = KC.singular_class(c, rec_of(c.name))
        if c.kind == "singular":
            table[c.name] = cls
            print("%-26s %-9s %s" % (c.name, cls, sorted(set(rec_of(c.name)["raised"].tolist()))))
            assert cls == c.singular, (c.name, cls, c.singular)
            # the raising edge first, in the middle and last in a d = 2, 4, 8 and 9 receiver: 11 receivers
            if cls != "none":
                nodes = np.union1d(rec_of(c.name)["raised_nodes"], KC.kernel_raising(c)[0])
                assert sorted(c.degree[nodes]) == [2, 2, 4, 4, 4, 8, 8, 8, 9, 9, 9]
        else:
            assert cls == "none", c.name
    assert "reference" not in table.values() and "mixed" not in table.values()
    assert set(k for k, v in table.items() if v == "kernel") == set(KC.SINGULAR_CLASSES)
    # the issue's table: (10, 0) / (10, 5) and (10, 5) / origin do not raise in the reference
    assert table["sing_perp_axis_0"] == table["sing_origin_nb_0"] == "kernel"
    assert table["sing_perp_axis_2"] == table["sing_perp_diag_0"] == "both"     # (-10, 0) / (-10, 5); (8, 8) / (10, 6)


def test_kernel_only_cases_are_unbounded_in_the_record():
    """where only the kernel's rule raises, the reference's state of the raising edge is garbage: a
    covariance entry beyond 1e14 (the exact value is infinite)"""
    for name in KC.SINGULAR_CLASSES:
        c, r = BY[name], rec_of(name)
        _, mask = KC.kernel_raising(c)
        assert mask.sum() == 11 and (np.abs(r["cov"][mask, 0, 0]) > 1e14).all(), name


def test_conditioning_shares():
    vc = KC.value_cases()
    k = {c.name: KC.conditioning(c.name) for c in vc}
    for n, v in k.items():
        print("%-28s pairs %5d ref_err %.2e sensitivity %.2e %s %s" % (
            n, v["n"], v["ref_err"], v["sens"], "well" if v["well"] else "ILL-CONDITIONED", "fp32-checked" if v["fp32"] else ""))
    well = [n for n, v in k.items() if v["well"]]
    fp32 = [n for n, v in k.items() if v["fp32"]]
    assert 3 * len(well) >= 2 * len(vc), (len(well), len(vc))
    assert 2 * len(fp32) >= len(vc), (len(fp32), len(vc))
    assert set(k) - set(well) == set(KC.ILL)


def test_exact_definitions():
    """exact_state / exact_kl / exact_moments against the record on a well-conditioned case, and the closed
    forms they rest on: sv[2] = 0, cov[2][2] = s1, equal states at distance 0"""
    c, r = BY["deg_9"], rec_of("deg_9")
    v = int(c.listed()[0])
    nbs = c.nbs(v)
    for k in range(nbs.shape[0]):
        sv, cov = KC.exact_state(c.gnn[v], nbs[k])
        assert sv[2] == 0.0 and cov[2, 2] == float(KC.D(0.1) * KC.D(0.1)) and np.array_equal(cov, cov.T)
        assert np.allclose(sv, r["sv"][c.ptr[v] + k], rtol=1e-9, atol=1e-20)
        assert np.allclose(cov, r["cov"][c.ptr[v] + k], rtol=1e-9, atol=1e-12 * np.abs(cov).max())
    assert KC.exact_kl(c.gnn[v], nbs[3], nbs[3]) == 0.0
    assert abs(KC.exact_kl(c.gnn[v], nbs[1], nbs[0]) - r["kl"][c.pair_ptr()[v]]) <= 1e-9 * abs(r["kl"][c.pair_ptr()[v]])
    m, var = KC.exact_moments(c.gnn[v], nbs)
    assert abs(m - r["gmean"][v]) <= 1e-12 * abs(m) and abs(var - r["gvar"][v]) <= 1e-9 * var
    assert KC.exact_moments((1.0, 2.0), [(1.0, 5.0)]) is None


@pytest.mark.parametrize("name", ["n0", "senders_only", "deg_1"])
@pytest.mark.parametrize("kw", [{}, {"ordered": True}, {"tile": 4}], ids=["listed", "ordered", "tile4"])
def test_empty_arrays_are_not_null(name, kw):
    """an event without nodes or without edges: the structs ParabolicKL hands to the C-ABI hold no null
    pointer for an array that is merely empty (the entry points refuse null as a missing array)"""
    from gtf.parabolic import ParabolicKL
    c = BY[name]
    k = ParabolicKL(c.ptr, c.src, c.gnn, c.truth, device="cpu", compact=True, **kw)
    g = k._g
    assert all((g.slot_ptr, g.slot_src, g.gnn, g.truth, g.pair_ptr, k._q.xy, k._q.truth32))
    assert k.n_pairs == 0 and k.n_slots == int(c.ptr[-1])
