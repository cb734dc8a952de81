"""Candidate scoring on the device (gtf_score_reset / _candidates / _finish, gtf.metrics.DeviceScorer)
against gtf.metrics.reconstruction_efficiency / majority, which tests/test_metrics.py pins to the
reference script's own outputs and tests/test_score_cases.py to the oracle. Everything is exact
(array_equal): the device counts integers and the purities are the host's fp64 divisions.

  * tests/score_cases.py through the C-ABI, guard bytes around every output, the calls in every order;
  * the golden vol-7 candidates: "script" 1 / 163 = 0.613 %, "cumulative" 133 / 163 = 81.595 %, as one
    call and as three calls cut at 2 / 110 / 1,055 candidates, in both orders;
  * 20 seeded random events with forced duplicates and ties;
  * extract.outputs_dev(lists=False), pipeline.run(scorer=..., lists=False) and
    run_pipeline.py --resident-metrics on kat134."""
import ctypes
import functools
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import score_cases as SC
from fixtures import GOLDEN, load
from gtf import _native as nat
from gtf import extract, metrics

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREFIX = os.path.join(GOLDEN, "kat134", "event_1_filtered_graph_")
GUARD, FILL = 256, 0xA5


# ------------------------------------------------------------------ the C-ABI with guard bytes
class Guarded:
    """n elements of dtype on the device between two GUARD-byte fences"""

    def __init__(self, n, dtype, init=None):
        import torch
        self.n, self.dtype = n, np.dtype(dtype)
        host = np.full(2 * GUARD + max(n, 1) * self.dtype.itemsize, FILL, np.uint8)
        if init is not None:
            host[GUARD:GUARD + n * self.dtype.itemsize] = np.ascontiguousarray(init, self.dtype).view(np.uint8)
        self.t = torch.from_numpy(host).cuda()

    @property
    def p(self):
        return ctypes.c_void_p(self.t.data_ptr() + GUARD)

    def get(self):
        """the payload, after checking that both fences (and the slack of an empty array) are untouched"""
        raw = self.t.cpu().numpy()
        end = GUARD + self.n * self.dtype.itemsize
        assert np.all(raw[:GUARD] == FILL) and np.all(raw[end:] == FILL), "guard bytes overwritten"
        return raw[GUARD:end].view(self.dtype).copy()


def _csr(cands):
    ptr = np.zeros(len(cands) + 1, np.int32)
    ptr[1:] = np.cumsum([len(c) for c in cands])
    return ptr, np.array([v for c in cands for v in c], np.int64)


class Raw:
    """one event's tables and state on the device, through ctypes only"""

    def __init__(self, t):
        import torch
        self.L, self.t, self.torch = nat.lib(), t, torch
        self.R = R = int(t.part_id.size)
        self.dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in
                    (t.node_id, t.node_ptr, t.node_part, t.part_id, t.part_hits, t.part_ref)]
        vp = lambda x: ctypes.c_void_p(x.data_ptr() if x.numel() else 0)   # noqa: E731
        self.truth = nat.GtfTruth(n_nodes=int(t.node_id.size), n_entries=int(t.node_part.size), n_particles=R,
                                  node_id=vp(self.dev[0]), node_ptr=vp(self.dev[1]), node_part=vp(self.dev[2]),
                                  part_id=vp(self.dev[3]), part_hits=vp(self.dev[4]), part_ref=vp(self.dev[5]))
        self.key, self.good, self.total = Guarded(R, np.uint64), Guarded(R, np.int32), Guarded(R, np.int32)
        self.err = Guarded(1, np.uint32)
        self.state = nat.GtfScoreState(R, 0, self.key.p, self.good.p, self.total.p, self.err.p)
        assert self.L.gtf_score_reset(ctypes.byref(self.state), None) == 0
        assert np.all(self.key.get() == np.uint64(2 ** 64 - 1)) and self.err.get()[0] == 0

    def add(self, cands, group):
        """-> (pid, n_good, total, passes) of one gtf_score_candidates call"""
        ptr, ids = _csr(cands)
        n = len(cands)
        dptr, dids = Guarded(n + 1, np.int32, ptr), Guarded(ids.size, np.int64, ids)
        outs = [Guarded(n, d) for d in (np.int64, np.int32, np.int32, np.uint8)]
        nb = int(self.L.gtf_score_workspace_bytes(n, ids.size))
        ws = Guarded(nb, np.uint8)
        out = nat.GtfScoreOut(*(o.p for o in outs))
        rc = self.L.gtf_score_candidates(ctypes.byref(self.truth), dptr.p, dids.p, n, group, ctypes.byref(out),
                                         ctypes.byref(self.state), ws.p, ctypes.c_size_t(nb), None)
        assert rc == 0, self.L.gtf_last_error()
        self.torch.cuda.synchronize()
        ws.get(), dptr.get(), dids.get()
        return [o.get() for o in outs]

    def finish(self):
        """-> (rc, n_reconstructed, error, key, pid, good, total, hits)"""
        R = self.R
        outs = [Guarded(R, d) for d in (np.uint64, np.int64, np.int32, np.int32, np.int32)]
        nb = int(self.L.gtf_score_finish_workspace_bytes(R))
        ws = Guarded(nb, np.uint8)
        cnt = nat.GtfScoreCounts(-1, 0)
        rc = self.L.gtf_score_finish(ctypes.byref(self.truth), ctypes.byref(self.state), *(o.p for o in outs),
                                     ctypes.byref(cnt), ws.p, ctypes.c_size_t(nb), None)
        ws.get(), self.key.get(), self.good.get(), self.total.get(), self.err.get()
        n = max(cnt.n_reconstructed, 0)
        return (rc, cnt.n_reconstructed, cnt.error) + tuple(o.get()[:n] for o in outs)


def _majority(t, cands):
    ptr, ids = _csr(cands)
    cand_of, part = metrics.candidate_particles(ptr, ids, t.node_id, t.node_ptr.astype(np.int64), t.node_part)
    return metrics.majority(len(cands), cand_of, part)


def _check_against_host(t, calls, order, host, passes_of=None):
    """the calls (group, candidates) fed in `order` through the C-ABI against the host Result of the
    candidates concatenated by ascending group"""
    raw = Raw(t)
    per = {}
    for i in order:
        group, cands = calls[i]
        per[group] = raw.add(cands, group)
        pid, good, total = _majority(t, cands)
        assert np.array_equal(per[group][0], pid) and np.array_equal(per[group][1], good), (group, "majority")
        assert np.array_equal(per[group][2], total), (group, "total")
        if passes_of is not None:
            assert np.array_equal(per[group][3], passes_of(cands)), (group, "passes")
    rc, n, err, key, pid, good, total, hits = raw.finish()
    assert (rc, err) == (0, 0)
    assert n == host.n_reconstructed
    start, at = {}, 0
    for group, cands in sorted(calls, key=lambda x: x[0]):
        start[group] = at
        at += len(cands)
    where = np.array([start[int(k >> np.uint64(32))] + int(k & np.uint64(0xffffffff)) for k in key], np.int64)
    assert np.array_equal(where, np.flatnonzero(host.matched))            # match order = candidate order
    assert np.array_equal(pid, host.reconstructed_pid[host.matched])
    assert np.array_equal(good, host.n_good[host.matched])
    assert np.array_equal(hits, t.part_hits[np.searchsorted(t.part_id, pid)])
    assert np.array_equal(good * 1.0 / total, host.track_purities)
    assert np.array_equal(good * 1.0 / hits, host.particle_purities)
    allp = np.concatenate([per[g][3] for g in sorted(per)]) if per else np.zeros(0, np.uint8)
    assert np.all(allp[host.matched] == 1)


def _alone(case):
    """each candidate scored by the host function on its own: matched = it passes the three tests"""
    pid, px, py = case["particles"]

    def f(cands):
        out = np.zeros(len(cands), np.uint8)
        for i, c in enumerate(cands):
            r = metrics.reconstruction_efficiency(np.array([0, len(c)]), np.array(c, np.int64), case["m"], pid, px, py, 7, 7)
            out[i] = r.matched[0]
        return out
    return f


NAMES = sorted(n for n in SC.CASES if n != "missing_id")


@pytest.mark.parametrize("name", NAMES)
def test_cases_through_the_c_abi(name):
    case = SC.CASES[name]()
    t, host = SC.tables(case), SC.host_result(case)
    for order in itertools.permutations(range(len(case["calls"]))):
        _check_against_host(t, case["calls"], order, host, _alone(case))


@pytest.mark.parametrize("name", NAMES)
def test_cases_through_the_scorer(name):
    """DeviceScorer.result() equals the host Result in every field, the calls in every order"""
    import torch
    case = SC.CASES[name]()
    host = SC.host_result(case)
    s = metrics.DeviceScorer(SC.tables(case))
    for order in itertools.permutations(range(len(case["calls"]))):
        s.reset()
        for i in order:
            group, cands = case["calls"][i]
            ptr, ids = _csr(cands)
            s.add(torch.from_numpy(ptr).cuda(), torch.from_numpy(ids).cuda(), len(cands), group, per_candidate=True)
        _results_equal(s.result(), host)


def _results_equal(a, b, per_candidate=True):
    assert (a.n_reconstructed, a.n_reference) == (b.n_reconstructed, b.n_reference)
    assert a.n_reference == 0 or a.efficiency_str == b.efficiency_str
    assert a.track_purities.dtype == b.track_purities.dtype == np.float64
    assert np.array_equal(a.track_purities, b.track_purities) and np.array_equal(a.particle_purities, b.particle_purities)
    if per_candidate:
        for k in ("reconstructed_pid", "n_good", "matched"):
            x, y = getattr(a, k), getattr(b, k)
            assert x.dtype == y.dtype and np.array_equal(x, y), k


def test_missing_id_is_the_references_key_error():
    import torch
    case = SC.CASES["missing_id"]()
    t = SC.tables(case)
    raw = Raw(t)
    pid, good, total, passes = raw.add(case["calls"][0][1], 0)
    assert list(total) == [4, 2] and list(passes) == [1, 1]      # the missing member contributes nothing
    rc, n, err = raw.finish()[:3]
    assert rc == -2 and err == nat.SCORE_ERR_MISSING and b"no hit_dissociation" in raw.L.gtf_last_error()
    s = metrics.DeviceScorer(t)
    ptr, ids = _csr(case["calls"][0][1])
    s.add(torch.from_numpy(ptr).cuda(), torch.from_numpy(ids).cuda(), 2, 0)
    with pytest.raises(ValueError, match="a candidate node has no hit_dissociation"):
        s.result()
    s.reset()                                                     # and the scorer is usable again
    s.add(torch.from_numpy(ptr[:2].copy()).cuda(), torch.from_numpy(ids[:4].copy()).cuda(), 1, 0)
    assert s.result().n_reconstructed == 1


def test_small_workspace_is_reported_not_overrun():
    """more members than the workspace was sized for: the error word, nothing written outside"""
    case = SC.CASES["sizes"]()
    raw = Raw(SC.tables(case))
    cands = case["calls"][0][1]
    ptr, ids = _csr(cands)
    assert ids.size > 400     # (far beyond the few dozen that the rounding of a zero-member workspace leaves room for)
    dptr, dids = Guarded(ptr.size, np.int32, ptr), Guarded(ids.size, np.int64, ids)
    nb = int(raw.L.gtf_score_workspace_bytes(len(cands), 0))
    ws = Guarded(nb, np.uint8)
    assert raw.L.gtf_score_candidates(ctypes.byref(raw.truth), dptr.p, dids.p, len(cands), 0, None,
                                      ctypes.byref(raw.state), ws.p, ctypes.c_size_t(nb), None) == 0
    raw.torch.cuda.synchronize()
    ws.get()
    rc, n, err = raw.finish()[:3]
    assert rc == -2 and err & nat.SCORE_ERR_WORKSPACE and b"workspace" in raw.L.gtf_last_error()


# ------------------------------------------------------------------ the golden event
@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(os.path.join(GOLDEN, "metrics_vol7.npz"), allow_pickle=False)
    m = metrics.HitMapping(*(z["map__" + c] for c in ("node_idx", "hit_id", "particle_id", "volume_id", "layer_id",
                                                       "module_id")))
    part = (z["particles__particle_id"], z["particles__px"], z["particles__py"])
    return z, m, part, metrics.truth_tables(m, *part, 7, 7)


def _golden_host(layout):
    z, m, part, _ = golden()
    return metrics.reconstruction_efficiency(z[layout + "__cand_ptr"], z[layout + "__cand_ids"], m, *part, 7, 7)


def _golden_cands(layout):
    z = golden()[0]
    ptr, ids = z[layout + "__cand_ptr"], z[layout + "__cand_ids"]
    return [ids[ptr[i]:ptr[i + 1]] for i in range(len(ptr) - 1)]


def _expect(layout):
    z = golden()[0]
    return (int(z[layout + "__counts"][0]), int(z[layout + "__counts"][1]), str(z[layout + "__efficiency"]),
            z[layout + "__track_purity"], z[layout + "__particle_purity"])


def _score(calls, order):
    import torch
    s = metrics.DeviceScorer(golden()[3])
    for i in order:
        group, cands = calls[i]
        ptr, ids = _csr(cands)
        s.add(torch.from_numpy(ptr).cuda(), torch.from_numpy(ids).cuda(), len(cands), group, per_candidate=True)
    return s.result()


@pytest.mark.parametrize("layout,n_reco,eff", [("script", 1, "0.613"), ("cumulative", 133, "81.595")])
def test_golden_event_one_call(layout, n_reco, eff):
    e = _expect(layout)
    assert e[:3] == (n_reco, 163, eff)
    r = _score([(0, _golden_cands(layout))], [0])
    assert (r.n_reconstructed, r.n_reference, r.efficiency_str) == e[:3]
    assert np.array_equal(r.track_purities, e[3]) and np.array_equal(r.particle_purities, e[4])   # bit-equal, in order
    _results_equal(r, _golden_host(layout))
    _check_against_host(golden()[3], [(0, _golden_cands(layout))], [0], _golden_host(layout))


@pytest.mark.parametrize("order", [(0, 1, 2), (2, 1, 0)])
def test_golden_event_three_calls(order):
    """the cumulative list cut where the iterations meet (3, 2, 1: 2 + 110 + 1,055 candidates)"""
    cands = _golden_cands("cumulative")
    assert len(cands) == 2 + 110 + 1055
    calls = [(0, cands[:2]), (1, cands[2:112]), (2, cands[112:])]
    e = _expect("cumulative")
    r = _score(calls, order)
    assert (r.n_reconstructed, r.n_reference, r.efficiency_str) == (133, 163, "81.595")
    assert np.array_equal(r.track_purities, e[3]) and np.array_equal(r.particle_purities, e[4])
    _results_equal(r, _golden_host("cumulative"))


def test_scorer_on_plain_allocations():
    """mem="hip": the same calls on gtf.devmem arrays (no torch tensor involved)"""
    from gtf.devmem import HipArray
    s = metrics.DeviceScorer(golden()[3], mem="hip")
    cands = _golden_cands("cumulative")
    for group, part in ((1, cands[2:]), (0, cands[:2])):
        ptr, ids = _csr(part)
        s.add(HipArray.from_numpy(ptr), HipArray.from_numpy(ids), len(part), group, per_candidate=True)
    _results_equal(s.result(), _golden_host("cumulative"))


# ------------------------------------------------------------------ random events
def _random_event(seed):
    """<= 300 candidates over ~60 particles: nodes of 1-6 hits, every particle in several candidates
    (duplicates), half-and-half candidates (ties), repeated members, 1-3 calls"""
    rng = np.random.default_rng(seed)
    w = SC.World(node0=int(rng.integers(0, 50)), stride=int(rng.integers(1, 5)))
    tracks = []
    n_part = int(rng.integers(20, 60))
    for p in range(n_part):
        pid = SC.B60 + int(rng.integers(0, 1 << 40)) * 2 + 1 if p else 0      # (id 0 is a particle here)
        tracks.append((pid, w.track(pid, int(rng.integers(2, 13)), pt=float(rng.choice([0.5, 2.0, 2.0, 2.0])))))
    for pid, ns in tracks:          # extra hits of other particles on the same nodes, up to 6 per node
        for v in ns:
            for _ in range(int(rng.choice([0, 0, 0, 1, 2, 5]))):
                w.hit(v, tracks[int(rng.integers(0, n_part))][0], int(rng.integers(1, 40)) * 2 + 1)
    cands = []
    n_cand = int(rng.integers(100, 301))
    while len(cands) < n_cand:
        kind = rng.integers(0, 6)
        pid, ns = tracks[int(rng.integers(0, n_part))]
        if kind == 0:               # a tie by construction: as many nodes of one particle as of another
            _, other = tracks[int(rng.integers(0, n_part))]
            k = int(rng.integers(1, min(len(ns), len(other)) + 1))
            c = list(ns[:k]) + list(other[:k])
        elif kind == 1:             # a repeated member, a long list
            c = [ns[int(i)] for i in rng.integers(0, len(ns), int(rng.integers(1, 40)))]
        elif kind == 2:
            c = []
        else:                       # most of one particle's nodes (the same particle comes again and again)
            c = [v for v in ns if rng.random() < 0.8]
        cands.append(c)
    cuts = sorted(int(x) for x in rng.integers(0, n_cand + 1, int(rng.integers(0, 3))))
    edges = [0] + cuts + [n_cand]
    calls = [(g, cands[a:b]) for g, (a, b) in enumerate(zip(edges[:-1], edges[1:]))]
    return w.build(calls, {})


def _has_tie(t, case):
    """a candidate whose two most frequent ids have the same count"""
    ptr, ids, cands = SC.flatten(case)
    cand_of, part = metrics.candidate_particles(ptr, ids, t.node_id, t.node_ptr.astype(np.int64), t.node_part)
    for c in range(len(cands)):
        n = np.sort(np.unique(part[cand_of == c], return_counts=True)[1])
        if n.size >= 2 and n[-1] == n[-2]:
            return True
    return False


def test_random_events():
    seen_dup = seen_tie = 0
    for seed in range(20):
        case = _random_event(seed)
        t, host = SC.tables(case), SC.host_result(case)
        order = list(range(len(case["calls"])))
        if seed % 2:
            order.reverse()
        _check_against_host(t, case["calls"], order, host)
        ok_pid = host.reconstructed_pid[host.matched]
        seen_dup += host.n_reconstructed > 0 and np.isin(host.reconstructed_pid[~host.matched], ok_pid).any()
        seen_tie += _has_tie(t, case)
    assert seen_dup >= 15 and seen_tie >= 15


# ------------------------------------------------------------------ the loop
def test_outputs_dev_without_lists():
    """lists=False: the device arrays hold what lists=True returns as lists (vol-7 stage output)"""
    from gtf.device import DeviceGraph
    g, _, x, m = load("extract_it1")
    p = extract.Params(m["p"], m["n"], m["s"], m["t"], m["sigma0xy"], m["sigma0rz"], m["endcap_boundary"])
    d = DeviceGraph(g)
    res = extract.run_dev(d, d._dev_from(np.asarray(x["vivl"], np.float64)), p, extract.candidate_order_dev(d))
    for ids, keys in ((True, ("cand_ids", "rem_ids", "frag_ids")), (False, ("cand_members", "rem_nodes", "frag_nodes"))):
        a = extract.outputs_dev(d, res, p.numhits, ids=ids)
        b = extract.outputs_dev(d, res, p.numhits, ids=ids, lists=False)
        assert set(b) == {"keep", "left", "pval_xy", "pval_zr", "counts", "cand_ptr", "rem_ptr", "frag_ptr"} | set(keys)
        assert not any(k in b for k in ("extracted", "remaining", "fragments"))
        c = b["counts"]
        assert c["n_extracted"] == len(a["extracted"]) > 0
        for name, lst, (n, m_) in zip(("cand", "rem", "frag"), keys, (("n_extracted", "n_extracted_nodes"),
                                                                     ("n_remaining", "n_remaining_nodes"),
                                                                     ("n_fragments", "n_fragment_nodes"))):
            groups = a[{"cand": "extracted", "rem": "remaining", "frag": "fragments"}[name]]
            ptr = d._np(b[name + "_ptr"])[:c[n] + 1]
            flat = d._np(b[lst])[:c[m_]]
            assert c[n] == len(groups) and c[m_] == sum(len(q) for q in groups)
            assert flat.dtype == (np.int64 if ids else np.int32)
            assert np.array_equal(np.diff(ptr), [len(q) for q in groups])
            assert np.array_equal(flat, np.concatenate(groups) if groups else flat[:0])
        for k in ("pval_xy", "pval_zr"):
            assert np.array_equal(d._np(b[k])[:c["n_extracted"]].view(np.int64), a[k].view(np.int64))
        assert np.array_equal(d._np(b["keep"]), d._np(a["keep"]))


def test_pipeline_scores_without_lists():
    from gtf import pipeline
    z, m, part, t = golden()
    scorer = metrics.DeviceScorer(t)
    its = pipeline.run(pipeline.build_event_dev(PREFIX, 7, 7), None, iterations=3, resident="device", scorer=scorer,
                       lists=False)
    assert [i.counts["n_extracted"] for i in its] == [1055, 110, 2]
    assert all(i.candidates is None and i.remaining is None and i.fragments is None for i in its)
    assert [len(i.pval_xy) for i in its] == [1055, 110, 2]
    got = scorer.result()
    ref = pipeline.run(pipeline.build_event_dev(PREFIX, 7, 7), None, iterations=3, resident="device")
    assert [i.counts["n_extracted"] for i in ref] == [len(i.candidates) for i in ref] == [1055, 110, 2]
    lists = ref[2].candidates + ref[1].candidates + ref[0].candidates
    ptr = np.concatenate([[0], np.cumsum([len(c) for c in lists])])
    host = metrics.reconstruction_efficiency(ptr, np.concatenate(lists), m, *part, 7, 7)
    _results_equal(got, host, per_candidate=False)
    e = _expect("cumulative")
    assert (got.n_reconstructed, got.n_reference, got.efficiency_str) == e[:3] == (133, 163, "81.595")
    # with the per-candidate outputs every field of Result is the host's
    scorer.reset()
    import torch
    for k, it in enumerate(ref):
        p_, i_ = _csr(it.candidates)
        scorer.add(torch.from_numpy(p_).cuda(), torch.from_numpy(i_).cuda(), len(it.candidates), 2 - k, per_candidate=True)
    _results_equal(scorer.result(), host)
    for kw in ({"scorer": scorer}, {"lists": False}):      # (refused before the graph is looked at)
        for resident in (False, True):
            with pytest.raises(ValueError, match="resident='device'"):
                pipeline.run(None, None, iterations=1, resident=resident, **kw)


def test_run_pipeline_resident_metrics(tmp_path):
    """run_pipeline.py --resident-metrics --truth writes the metrics.json the plain run writes"""
    import pandas as pd
    z = golden()[0]
    tdir = str(tmp_path / "truth")
    os.makedirs(tdir)
    cols = ("node_idx", "hit_id", "particle_id", "volume_id", "layer_id", "module_id")
    pd.DataFrame({c: z["map__" + c] for c in cols}).to_csv(
        os.path.join(tdir, "event000001000-full-mapping-minCurv-0.3-134.csv"), index=False)
    pd.DataFrame({c: z["particles__" + c] for c in ("particle_id", "px", "py")}).to_csv(
        os.path.join(tdir, "event000001000-particles.csv"), index=False)
    cli = os.path.join(ROOT, "gnn-track-finding_amd", "run_pipeline.py")
    got = []
    for flags in ([], ["--resident-metrics"]):
        out = str(tmp_path / ("out%d" % len(got)))
        subprocess.check_call([sys.executable, cli, "-n", os.path.join(GOLDEN, "kat134"), "-o", out, "-a", "7", "-z", "7",
                               "--truth", tdir, "--mapping", "full-mapping-minCurv-0.3-134.csv"] + flags)
        with open(os.path.join(out, "metrics.json")) as f:
            got.append(json.load(f))
    assert got[0] == got[1]
    assert (got[1]["cumulative"]["reconstructed"], got[1]["cumulative"]["efficiency_pct"]) == (133, "81.595")
    assert (got[1]["last_iteration"]["reconstructed"], got[1]["last_iteration"]["efficiency_pct"]) == (1, "0.613")
