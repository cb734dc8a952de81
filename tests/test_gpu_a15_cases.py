"""The directed a15 cases (a15_cases.py, pinned to the reference by test_a15_cases.py) on the GPU,
called through the C-ABI (gtf_updated_state_pair_counts, gtf_updated_state_distances) with every
output between guard bytes.

All clean cases and their copies form one graph, uploaded once; it runs with the node schedule
(the 2- to 64-lane groups and the wave path) and with sched = NULL (every node on the wave path):

  * pair counts, pair_ptr, the truth flags and the error word exact;
  * the four columns against the oracle at the bar of test_a15_matches_oracle_with_hubs (1e-10
    relative, 1e-15 absolute) and against the record of the reference's mahalanobis_distance at the
    bar of test_a15_matches_reference_pairs (1e-6, 1e-12 absolute on the angle and tau columns),
    non-finite entries equal in kind;
  * the pair whose C_i + C_j is singular holds a non-finite chi2, and no other pair does that the
    oracle has finite;
  * each optional output NULL, truth NULL with and without a truth output;
  * GTF_ERR_PAIR_COUNT, GTF_ERR_NEIGHBOUR_MISSING and GTF_ERR_TOO_MANY_STATES, each in a group-path
    and in a wave-path node where the bit can arise there: the raising node's pairs are untouched,
    every other node of the call is exact;
  * 2,048 keys are processed (chi2 alone; first, last and 2,000 sampled pairs against the oracle's
    per-pair function), 2,049 are refused.
"""
import ctypes
import functools
import os

import numpy as np
import pytest

import a15_cases as AC
from fixtures import GOLDEN
from gtf import _native as nat

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = -7.25
ALL = AC.COLS + ("truth",)


@functools.lru_cache(maxsize=None)
def world(errs=False):
    from gtf.device import DeviceGraph
    g, comps, truth = AC.everything(errs)
    ptr, cols, sing, raised = AC.expected(g, truth)
    return dict(g=g, comps=comps, truth=truth, ptr=ptr, cols=cols, sing=sing, raised=raised, d=DeviceGraph(g))


def graph_arg(d, sched):
    if sched:
        return d.cg_sched
    cg = nat.GtfGraph()
    ctypes.memmove(ctypes.byref(cg), ctypes.byref(d.cg_sched), ctypes.sizeof(cg))
    cg.sched = None
    cg.sched_seg = None
    return cg


def counts(d, sched=True):
    import torch
    c = torch.full((d.n_nodes + 2 * GUARD,), -3, dtype=torch.int64, device=d.device)
    nat.check(d.lib.gtf_updated_state_pair_counts(ctypes.byref(graph_arg(d, sched)), ctypes.byref(d.cn), ctypes.byref(d.cuts),
                                                  ctypes.byref(d.ce), ctypes.c_void_p(c[GUARD:].data_ptr()), d.stream))
    h = c.cpu().numpy()
    assert (h[:GUARD] == -3).all() and (h[-GUARD:] == -3).all()
    return h[GUARD:-GUARD]


def distances(d, pair_ptr, n_out, truth=None, outputs=ALL, sched=True, want_rc=0):
    """one gtf_updated_state_distances call on guarded outputs of n_out pairs; returns (columns, error word)"""
    import torch
    dev = d.device
    bufs = {}
    for k in outputs:
        dt = torch.int8 if k == "truth" else torch.float64
        bufs[k] = torch.full((n_out + 2 * GUARD,), -7 if k == "truth" else FILL, dtype=dt, device=dev)
    vp = lambda k: ctypes.c_void_p(bufs[k][GUARD:].data_ptr()) if k in bufs else ctypes.c_void_p(0)  # noqa: E731
    err = torch.zeros(1 + 2 * GUARD, dtype=torch.int32, device=dev)
    tr = None if truth is None else torch.as_tensor(np.asarray(truth, np.int64), device=dev)
    pp = torch.as_tensor(np.asarray(pair_ptr, np.int64), device=dev)
    po = nat.GtfPairOut(vp("chi2"), vp("avg_tau"), vp("avg_theta"), vp("delta_theta"), vp("truth"),
                        ctypes.c_void_p(err[GUARD:].data_ptr()))
    rc = d.lib.gtf_updated_state_distances(ctypes.byref(graph_arg(d, sched)), ctypes.byref(d.cn), ctypes.byref(d.cuts),
                                           ctypes.byref(d.ce), ctypes.c_void_p(tr.data_ptr() if tr is not None else 0),
                                           ctypes.c_void_p(pp.data_ptr()), ctypes.byref(po), d.stream)
    assert rc == want_rc, (rc, d.lib.gtf_last_error())
    if rc:
        return None, None
    out = {}
    for k, t in bufs.items():
        h = t.cpu().numpy()
        fill = -7 if k == "truth" else FILL
        assert (h[:GUARD] == fill).all() and (h[-GUARD:] == fill).all(), k
        out[k] = h[GUARD:-GUARD]
    e = err.cpu().numpy()
    assert (e[:GUARD] == 0).all() and (e[GUARD + 1:] == 0).all()
    return out, int(e[GUARD])


def untouched(out, lo, hi):
    return all((out[k][lo:hi] == (-7 if k == "truth" else FILL)).all() for k in out)


def against_oracle(out, exp, rows, sing=()):
    """the bar of test_a15_matches_oracle_with_hubs on the pairs `rows` (a bool mask)"""
    m = rows.copy()
    m[list(sing)] = False
    for c in AC.COLS:
        if c in out:
            np.testing.assert_allclose(out[c][m], exp[c][m], rtol=1e-10, atol=1e-15, err_msg=c)
    if "truth" in out:
        assert np.array_equal(out["truth"][rows], exp["truth"][rows])
    for t in sing:
        assert not np.isfinite(out["chi2"][t]), "a singular C_i + C_j must leave a non-finite chi2"


@functools.lru_cache(maxsize=None)
def clean_run(sched):
    w = world()
    return distances(w["d"], w["ptr"], int(w["ptr"][-1]), truth=w["truth"], sched=sched)


@pytest.mark.parametrize("sched", [True, False], ids=["schedule", "sched_null"])
def test_cases_match_the_oracle(sched):
    w = world()
    d, g = w["d"], w["g"]
    if sched:   # the buckets the cases were sized for
        deg = np.diff(g.slot_ptr)
        cg = d.cg_sched
        assert cg.n_g2 == int((deg <= 2).sum()) > 128 and cg.n_g4 - cg.n_g2 == int(((deg > 2) & (deg <= 4)).sum()) > 64
        assert cg.n_big == int((deg > 64).sum()) >= 3
    assert np.array_equal(np.cumsum(counts(d, sched)), w["ptr"][1:])
    out, err = clean_run(sched)
    assert err == 0
    P = int(w["ptr"][-1])
    against_oracle(out, w["cols"], np.ones(P, bool), w["sing"])
    assert len(w["sing"]) == 1 and int(np.isfinite(w["cols"]["chi2"]).sum()) == int(np.isfinite(out["chi2"]).sum())
    worst = {c: float(np.nanmax(np.where(np.isfinite(w["cols"][c]) & (w["cols"][c] != 0),
                                         np.abs(out[c] - w["cols"][c]) / np.abs(w["cols"][c]), 0.0))) for c in AC.COLS}
    print("a15 cases vs oracle (%s), max rel: %s" % ("sched" if sched else "sched NULL", ", ".join("%s %.3g" % kv for kv in worst.items())))


def test_schedule_and_sched_null_are_bit_equal():
    a, b = clean_run(True)[0], clean_run(False)[0]
    for k in ALL:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_cases_match_the_reference_record():
    w = world()
    out, _ = clean_run(True)
    rec = np.load(os.path.join(GOLDEN, "a15_cases.npz"), allow_pickle=False)
    seen = 0
    for c in w["comps"]:
        name, v = c["case"].name, c["v"]
        lo, hi = int(w["ptr"][v]), int(w["ptr"][v + 1])
        assert hi - lo == int(rec[name + "__pair_ptr"][-1]), name      # (the node "v" is the only one with pairs)
        raised = rec[name + "__raised_pairs"].tolist() if name + "__raised_pairs" in rec.files else []
        m = np.ones(hi - lo, bool)
        m[raised] = False
        for col in AC.COLS:
            atol = 1e-12 if col in ("avg_theta", "delta_theta", "avg_tau") else 0.0
            np.testing.assert_allclose(out[col][lo:hi][m], rec[name + "__" + col][m], rtol=1e-6, atol=atol, err_msg=name + " " + col)
        for t in raised:
            assert not np.isfinite(out["chi2"][lo + t]), name
        seen += hi > lo
    assert seen >= 40


@pytest.mark.parametrize("drop", AC.COLS[1:] + ("truth",))
def test_each_optional_output_null(drop):
    w = world()
    full, _ = clean_run(True)
    out, err = distances(w["d"], w["ptr"], int(w["ptr"][-1]), truth=w["truth"], outputs=tuple(k for k in ALL if k != drop))
    assert err == 0 and drop not in out
    for k in out:
        assert np.array_equal(out[k], full[k], equal_nan=True), k


def test_truth_null():
    w = world()
    full, _ = clean_run(True)
    out, err = distances(w["d"], w["ptr"], int(w["ptr"][-1]), truth=None, outputs=AC.COLS)
    assert err == 0
    for k in AC.COLS:
        assert np.array_equal(out[k], full[k], equal_nan=True), k
    distances(w["d"], w["ptr"], int(w["ptr"][-1]), truth=None, outputs=ALL, want_rc=-2)   # a truth output needs node truth
    assert b"truth" in w["d"].lib.gtf_last_error()


@pytest.mark.parametrize("sched", [True, False], ids=["schedule", "sched_null"])
def test_pair_count_error(sched):
    """one node's pair_ptr span off by one, in a group-path node and in a wave-path node"""
    w = world()
    full, _ = clean_run(True)
    vs = [next(c["v"] for c in w["comps"] if c["case"].name == n) for n in ("order_5", "order_65")]
    ptr = w["ptr"].copy()
    for v in vs:
        ptr[v + 1:] += 1
    out, err = distances(w["d"], ptr, int(ptr[-1]), truth=w["truth"], sched=sched)
    assert err == AC.ERR_PAIR_COUNT
    for v in range(w["g"].n_nodes):
        lo, hi = int(ptr[v]), int(ptr[v + 1])
        if v in vs:
            assert untouched(out, lo, hi), v
        else:
            for k in ALL:
                assert np.array_equal(out[k][lo:hi], full[k][int(w["ptr"][v]):int(w["ptr"][v + 1])], equal_nan=True), (v, k)


@pytest.mark.parametrize("sched", [True, False], ids=["schedule", "sched_null"])
def test_neighbour_missing_error(sched):
    w = world(True)
    d = w["d"]
    assert len(w["raised"]) == 2
    assert np.array_equal(np.cumsum(counts(d, sched)), w["ptr"][1:])
    out, err = distances(d, w["ptr"], int(w["ptr"][-1]), truth=w["truth"], sched=sched)
    assert err == AC.ERR_NEIGHBOUR_MISSING
    rows = np.ones(int(w["ptr"][-1]), bool)
    for v in w["raised"]:
        lo, hi = int(w["ptr"][v]), int(w["ptr"][v + 1])
        assert hi > lo and untouched(out, lo, hi), v
        rows[lo:hi] = False
    assert rows.sum() >= 10 + 3 + 2080
    against_oracle(out, w["cols"], rows)


BESIDE = ("order_5", "order_65", "active_2")      # a group-path star, a wave-path star and a 3-key one


@pytest.mark.parametrize("sched", [True, False], ids=["schedule", "sched_null"])
def test_too_many_states(sched):
    """d = 2,049 is refused and d = 2,048 is processed, in a call that also holds clean stars of the
    group and of the wave path: their pairs equal the oracle's whichever way the big node goes"""
    from gtf.device import DeviceGraph
    for n in (AC.BIG_CAP + 1, AC.BIG_CAP):
        g = AC.big_star(n, BESIDE)
        d = DeviceGraph(g)
        P = n * (n - 1) // 2
        small = AC.big_star(2, BESIDE)              # the same clean stars behind a 2-key node: the oracle's rows
        sp, scols, _, _ = AC.expected(small)
        rest = int(sp[-1]) - 1
        assert rest == 10 + 2080 + 3
        cnt = counts(d, sched)
        assert cnt[0] == P and cnt[1:].sum() == rest
        ptr = np.concatenate([[0], np.cumsum(cnt)])
        out, err = distances(d, ptr, P + rest, outputs=("chi2",), sched=sched)
        # the clean stars of the same call: exact
        np.testing.assert_allclose(out["chi2"][P:], scols["chi2"][1:], rtol=1e-10, atol=1e-15)
        assert np.array_equal(np.diff(ptr)[n + 1:], np.diff(sp)[3:])
        if n > AC.BIG_CAP:
            assert err == AC.ERR_TOO_MANY_STATES and untouched(out, 0, P)
            full, err = distances(d, ptr, P + rest, outputs=AC.COLS, sched=sched)       # and with all four columns
            assert err == AC.ERR_TOO_MANY_STATES and untouched(full, 0, P)
            for c in AC.COLS:
                np.testing.assert_allclose(full[c][P:], scols[c][1:], rtol=1e-10, atol=1e-15, err_msg=c)
            continue
        assert err == 0 and np.isfinite(out["chi2"][:P]).all()
        ts = [0, P - 1] + np.random.default_rng(2048).integers(0, P, 2000).tolist()
        exp = np.array([AC.pair_of(g, 0, t)[0] for t in ts])
        np.testing.assert_allclose(out["chi2"][ts], exp, rtol=1e-10, atol=1e-15)
