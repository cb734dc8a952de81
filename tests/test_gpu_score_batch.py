"""The batched scoring on the device (gtf_truth_concat, gtf_score_reset_ev / _candidates_ev / _finish_ev,
gtf.metrics.truth_concat_dev / BatchScorer, pipeline.run_batch(scorers=BatchScorer), run_pipeline.py
--batch-metrics) against what it replaces: gtf_score_candidates / gtf_score_finish and DeviceScorer once
per event, both sides on the GPU, and metrics.reconstruction_efficiency / concat_tables on the host.
Everything is exact (array_equal). The batches are tests/score_batch_cases.py's."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import score_batch_cases as BC
from fixtures import GOLDEN
from gtf import _native as nat
from gtf import metrics
from test_gpu_build_batch import _prefixes, event_dirs  # noqa: F401  (the golden batch's directories)
from test_gpu_score import Guarded, Raw, _results_equal, golden

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = np.uint64(2 ** 64 - 1)
INT32_MAX = 2 ** 31 - 1
NAMES = sorted(BC.BATCHES)
FIELDS = [f for f, _ in metrics._TABLE_FIELDS]


def _sync():
    import torch
    torch.cuda.synchronize()


# ------------------------------------------------------------------ the C-ABI with guard bytes
class RawBatch:
    """a batch's tables, concatenated by gtf_truth_concat into guarded arrays, and a guarded state"""

    def __init__(self, events):
        import torch
        self.L, self.events = nat.lib(), events
        self.tables = [BC.event_tables(ev) for ev in events]
        self.host = h = metrics.concat_tables(self.tables)
        K = self.K = len(events)
        T, P, R = int(h.node_off[-1]), int(h.entry_off[-1]), int(h.part_off[-1])
        self.R = R
        sizes, parts = (nat.GtfTruthSizes * max(K, 1))(), (nat.GtfTruthPart * max(K, 1))()
        self._up = {}
        for i, t in enumerate(self.tables):
            if t is None:
                continue
            if id(t) not in self._up:
                self._up[id(t)] = [torch.from_numpy(np.ascontiguousarray(getattr(t, f))).cuda() for f in FIELDS]
            n = (t.node_id.size, t.node_part.size, t.part_id.size)
            sizes[i].n_nodes, sizes[i].n_entries, sizes[i].n_particles = n
            parts[i].n_nodes, parts[i].n_entries, parts[i].n_particles = n
            for f, a in zip(FIELDS, self._up[id(t)]):
                setattr(parts[i], f, a.data_ptr() if a.numel() else None)
        self.d_parts = Guarded(ctypes.sizeof(parts), np.uint8, np.frombuffer(bytes(parts), np.uint8))
        dts = [dt for _, dt in metrics._TABLE_FIELDS]
        self.arr = [Guarded(n, dt) for n, dt in zip((T, T + 1, P, R, R, R), dts)]
        self.off = [Guarded(K + 1, np.int32) for _ in range(3)]
        scored = h.scored
        self.d_scored = Guarded(K, np.uint8, scored) if K and not scored.all() else None
        buf = nat.GtfTruthBatchBuf(*[g.p for g in self.off + self.arr])
        self.batch = nat.GtfTruthBatch(scored=self.d_scored.p if self.d_scored else None)
        nb = int(self.L.gtf_truth_concat_workspace_bytes(K))
        ws = Guarded(nb, np.uint8)
        rc = self.L.gtf_truth_concat(sizes, self.d_parts.p, K, ctypes.byref(buf), ctypes.byref(self.batch), ws.p,
                                     ctypes.c_size_t(nb), None)
        assert rc == 0, self.L.gtf_last_error()
        _sync()
        assert ws.get()[:4].view(np.int32)[0] == 0       # the device table agrees with the host's sizes
        self.d_parts.get()
        assert (self.batch.n_events, self.batch.n_nodes, self.batch.n_entries, self.batch.n_particles) == (K, T, P, R)
        self.new_state()

    def check_tables(self):
        h = self.host
        for g, name in zip(self.off + self.arr, list(metrics._OFFSET_FIELDS) + FIELDS):
            assert np.array_equal(g.get(), getattr(h, name)), name

    def new_state(self):
        R = self.R
        self.key, self.good, self.total = Guarded(R, np.uint64), Guarded(R, np.int32), Guarded(R, np.int32)
        self.err = Guarded(2, np.uint32)
        self.state = nat.GtfScoreStateEv(n_particles=R, best_key=self.key.p, best_good=self.good.p,
                                         best_total=self.total.p, error=self.err.p)
        self.reset(None)
        assert np.all(self.key.get() == NONE) and self.err.get().tolist() == [0, INT32_MAX]

    def reset(self, mask):
        m = Guarded(self.K, np.uint8, np.asarray(mask, np.uint8)) if mask is not None else None
        rc = self.L.gtf_score_reset_ev(ctypes.byref(self.state), ctypes.byref(self.batch), m.p if m else None, None)
        assert rc == 0, self.L.gtf_last_error()
        _sync()
        if m:
            m.get()

    def add(self, group, first, cands, first_override=None, ws_members=None):
        """-> (pid, n_good, total, passes) of one gtf_score_candidates_ev call"""
        ptr, ids = BC.csr(cands)
        n = len(cands)
        dptr, dids = Guarded(n + 1, np.int32, ptr), Guarded(ids.size, np.int64, ids)
        dfirst = Guarded(self.K + 1, np.int32, first if first_override is None else first_override)
        outs = [Guarded(n, d) for d in (np.int64, np.int32, np.int32, np.uint8)]
        nb = int(self.L.gtf_score_ev_workspace_bytes(n, ids.size if ws_members is None else ws_members, self.K))
        ws = Guarded(nb, np.uint8)
        out = nat.GtfScoreOut(*(o.p for o in outs))
        rc = self.L.gtf_score_candidates_ev(ctypes.byref(self.batch), dptr.p, dids.p, dfirst.p, n, group,
                                            ctypes.byref(out), ctypes.byref(self.state), ws.p, ctypes.c_size_t(nb), None)
        assert rc == 0, self.L.gtf_last_error()
        _sync()
        ws.get(), dptr.get(), dids.get(), dfirst.get()
        for g in self.off + self.arr + [self.d_parts] + ([self.d_scored] if self.d_scored else []):
            g.get()
        return [o.get() for o in outs] if n else [np.zeros(0, d) for d in (np.int64, np.int32, np.int32, np.uint8)]

    def finish(self):
        """-> (rc, n_reconstructed [K], error [2], rec_first, key, pid, good, total, hits)"""
        R, K = self.R, self.K
        outs = [Guarded(R, d) for d in (np.uint64, np.int64, np.int32, np.int32, np.int32)]
        first = Guarded(K + 1, np.int32)
        nb = int(self.L.gtf_score_finish_ev_workspace_bytes(R, K))
        ws = Guarded(nb, np.uint8)
        n_rec, err = np.full(max(K, 1), -1, np.int32), np.zeros(2, np.uint32)
        rc = self.L.gtf_score_finish_ev(ctypes.byref(self.batch), ctypes.byref(self.state), *(o.p for o in outs), first.p,
                                        ctypes.c_void_p(n_rec.ctypes.data), ctypes.c_void_p(err.ctypes.data), ws.p,
                                        ctypes.c_size_t(nb), None)
        ws.get(), self.key.get(), self.good.get(), self.total.get(), self.err.get()
        n = int(n_rec[:K].sum())
        return (rc, n_rec[:K], err, first.get()) + tuple(o.get()[:n] for o in outs)


def _event_reference(events, order):
    """every distinct event scored alone through gtf_score_candidates, its calls in `order` (the batch's
    groups) -> {id(ev): (key, good, total, error, {group: outputs})}"""
    ref = {}
    for ev in events:
        if id(ev) in ref or ev.get("unscored"):
            continue
        raw = Raw(BC.event_tables(ev))
        per = {}
        for g in order:
            cands = [c for gg, cs in ev["calls"] if gg == g for c in cs]
            if any(gg == g for gg, _ in ev["calls"]) and cands:
                per[g] = raw.add(cands, g)
        _sync()
        ref[id(ev)] = (raw.key.get(), raw.good.get(), raw.total.get(), int(raw.err.get()[0]), per, raw)
    return ref


def _empty_outputs(n):
    return [np.zeros(n, d) for d in (np.int64, np.int32, np.int32, np.uint8)]


def _expected_state(events, ref):
    key = [ref[id(ev)][0] for ev in events if not ev.get("unscored")]
    good = [ref[id(ev)][1] for ev in events if not ev.get("unscored")]
    total = [ref[id(ev)][2] for ev in events if not ev.get("unscored")]
    cat = lambda xs, dt: np.concatenate(xs) if xs else np.zeros(0, dt)   # noqa: E731
    errs = [0 if ev.get("unscored") else ref[id(ev)][3] for ev in events]
    word = int(np.bitwise_or.reduce(errs)) if errs else 0
    where = min([e for e, x in enumerate(errs) if x], default=INT32_MAX)
    return cat(key, np.uint64), cat(good, np.int32), cat(total, np.int32), [word, where]


@pytest.mark.parametrize("name", NAMES)
def test_batches_through_the_c_abi(name):
    events = BC.BATCHES[name]()
    rb = RawBatch(events)
    rb.check_tables()                                   # gtf_truth_concat against concat_tables
    calls = BC.batch_calls(events)
    groups = [g for g, _, _ in calls]
    for order in ([groups, groups[::-1]] if len(groups) > 1 else [groups]):
        ref = _event_reference(events, order)
        rb.new_state()
        for g in order:
            _, first, cands = calls[groups.index(g)]
            got = rb.add(g, first, cands)
            exp = [ref[id(ev)][4].get(g, _empty_outputs(0)) if not ev.get("unscored")
                   else _empty_outputs(int(first[e + 1] - first[e])) for e, ev in enumerate(events)]
            for i in range(4):                          # the per-candidate outputs, concatenated
                assert np.array_equal(got[i], np.concatenate([x[i] for x in exp])), (g, i)
        key, good, total, err = _expected_state(events, ref)
        assert np.array_equal(rb.key.get(), key)        # word for word, the unclaimed words included
        assert np.array_equal(rb.good.get(), good) and np.array_equal(rb.total.get(), total)
        assert rb.err.get().tolist() == err
    # finish: against the per-event gtf_score_finish and against the host
    rc, n_rec, err, first, key, pid, good, total, hits = rb.finish()
    if name in BC.MISSING:
        assert rc == -2 and err[0] == nat.SCORE_ERR_MISSING and err[1] == BC.MISSING[name]
        assert b"event %d: a candidate node has no hit_dissociation" % BC.MISSING[name] in rb.L.gtf_last_error()
        return
    assert rc == 0 and err.tolist() == [0, INT32_MAX], rb.L.gtf_last_error()
    assert first[0] == 0 and np.array_equal(np.diff(first), n_rec)
    done = {}
    for e, ev in enumerate(events):
        a, b = int(first[e]), int(first[e + 1])
        if ev.get("unscored"):
            assert a == b
            continue
        if id(ev) not in done:
            done[id(ev)] = ref[id(ev)][5].finish()
        r = done[id(ev)]
        assert (r[0], r[2]) == (0, 0) and r[1] == b - a
        for x, y in zip((key, pid, good, total, hits), r[3:]):
            assert np.array_equal(x[a:b], y), e
        host = BC.event_host(ev)
        assert b - a == host.n_reconstructed
        assert np.array_equal(pid[a:b], host.reconstructed_pid[host.matched])
        assert np.array_equal(good[a:b] * 1.0 / total[a:b], host.track_purities)
        assert np.array_equal(good[a:b] * 1.0 / hits[a:b], host.particle_purities)


def test_partial_reset_keeps_the_other_events():
    events = BC.BATCHES["group_orders"]()
    rb = RawBatch(events)
    calls = BC.batch_calls(events)
    for g, first, cands in calls:
        rb.add(g, first, cands)
    before = rb.key.get()
    po = rb.host.part_off
    rb.reset([1, 0, 1])
    after = rb.key.get()
    assert np.all(after[po[0]:po[1]] == NONE) and np.all(after[po[2]:po[3]] == NONE)
    assert np.array_equal(after[po[1]:po[2]], before[po[1]:po[2]]) and np.any(before[po[1]:po[2]] != NONE)
    _, first, cands = calls[1]
    rb.add(0, first, cands)
    key, good, total = rb.key.get(), rb.good.get(), rb.total.get()
    for e, ev in enumerate(events):        # events 0 and 2: their group-1 candidates alone, as group 0
        raw = Raw(BC.event_tables(ev))
        for g, cs in (ev["calls"] if e == 1 else [(0, [c for gg, x in ev["calls"] if gg == 1 for c in x])]):
            raw.add(cs, g)
        k = raw.key.get()
        assert np.array_equal(key[po[e]:po[e + 1]], k), e
        hit = k != NONE
        assert np.array_equal(good[po[e]:po[e + 1]][hit], raw.good.get()[hit])
        assert np.array_equal(total[po[e]:po[e + 1]][hit], raw.total.get()[hit])
    # a masked reset leaves the error words alone
    rb = RawBatch(BC.BATCHES["missing_middle"]())
    for g, first, cands in BC.batch_calls(rb.events):
        rb.add(g, first, cands)
    rb.reset([1, 1, 1])
    assert rb.err.get().tolist() == [nat.SCORE_ERR_MISSING, 1] and np.all(rb.key.get() == NONE)
    rb.reset(None)
    assert rb.err.get().tolist() == [0, INT32_MAX]


@pytest.mark.parametrize("how", ["first_not_zero", "decreasing", "last_not_n_cand", "beyond"])
def test_broken_cand_first_is_reported_not_followed(how):
    events = BC.BATCHES["boundaries"]()
    rb = RawBatch(events)
    g, first, cands = BC.batch_calls(events)[0]
    bad = first.copy()
    if how == "first_not_zero":
        bad[0] = 1
    elif how == "decreasing":
        bad[3], bad[4] = bad[4] + 2, bad[3]
    elif how == "last_not_n_cand":
        bad[-1] -= 1
    else:
        bad[2:] = [1 << 30, -5, 1 << 30, 7, 7, 7, -(1 << 31), len(cands)]
    rb.add(g, first, cands, first_override=bad)       # (every guard is checked in there)
    err = rb.err.get()
    assert err[0] & nat.SCORE_ERR_RANGE
    assert rb.finish()[0] == -2                       # (a candidate counted to a wrong event may miss its ids as well)
    if how != "decreasing" and how != "beyond":       # no candidate changes its event: RANGE alone
        assert err[0] == nat.SCORE_ERR_RANGE and b"cand_first" in rb.L.gtf_last_error()


def test_small_workspace_and_other_abi():
    events = BC.BATCHES["boundaries"]()
    rb = RawBatch(events)
    g, first, cands = BC.batch_calls(events)[0]
    rb.add(g, first, cands, ws_members=0)             # far more members than a zero-member workspace holds
    assert rb.err.get()[0] & nat.SCORE_ERR_WORKSPACE
    assert rb.finish()[0] == -2 and b"workspace" in rb.L.gtf_last_error()
    rb.new_state()
    a = Guarded(64, np.int32)
    key_before = rb.key.get()
    rb.batch.abi_version = 7
    assert rb.L.gtf_score_candidates_ev(ctypes.byref(rb.batch), a.p, a.p, a.p, 4, 0, None, ctypes.byref(rb.state), a.p,
                                        ctypes.c_size_t(1 << 20), None) == -3
    rb.batch.abi_version = 8
    for n, grp, nb in ((-1, 0, 1 << 20), (4, -1, 1 << 20), (4, 0, 16)):
        assert rb.L.gtf_score_candidates_ev(ctypes.byref(rb.batch), a.p, a.p, a.p, n, grp, None, ctypes.byref(rb.state),
                                            a.p, ctypes.c_size_t(nb), None) == -2
    _sync()
    a.get()
    assert np.array_equal(rb.key.get(), key_before)   # nothing was launched


def test_concat_of_nothing_and_of_empty_parts():
    for events in ([], [BC._empty_tables()], [BC._unscored(), BC._unscored()]):
        rb = RawBatch(events)
        rb.check_tables()
        for g, first, cands in BC.batch_calls(events):
            rb.add(g, first, cands)
        rc, n_rec, err = rb.finish()[:3]
        assert rc == 0 and n_rec.tolist() == [0] * len(events) and err.tolist() == [0, INT32_MAX]


# ------------------------------------------------------------------ BatchScorer
def _dev(mem, a):
    if mem == "hip":
        from gtf.devmem import HipArray
        return HipArray.from_numpy(a)
    import torch
    return torch.from_numpy(a).cuda()


def _scorer_reference(events, cache):
    """[DeviceScorer(...).result() ...], computed once per distinct event"""
    out = []
    for ev in events:
        if ev.get("unscored"):
            out.append(None)
            continue
        if id(ev) not in cache:
            s = metrics.DeviceScorer(BC.event_tables(ev))
            for g, cands in ev["calls"]:
                ptr, ids = BC.csr(cands)
                s.add(_dev("torch", ptr), _dev("torch", ids), len(cands), g, per_candidate=True)
            cache[id(ev)] = s.result()
        out.append(cache[id(ev)])
    return out


HIP_NAMES = ("unscored_between", "group_orders", "large_257", "random_0", "missing_middle")


@pytest.mark.parametrize("name,mem", [(n, "torch") for n in NAMES] + [(n, "hip") for n in HIP_NAMES])
def test_batch_scorer_equals_the_device_scorers(name, mem):
    events = BC.BATCHES[name]()
    s = metrics.BatchScorer([BC.event_tables(ev) for ev in events], mem=mem)
    for g, first, cands in reversed(BC.batch_calls(events)):
        ptr, ids = BC.csr(cands)
        s.add(_dev(mem, ptr), _dev(mem, ids if ids.size else np.zeros(1, np.int64)), _dev(mem, first), len(cands), g,
              per_candidate=True)
    if name in BC.MISSING:
        with pytest.raises(ValueError, match="^event %d: a candidate node has no hit_dissociation" % BC.MISSING[name]):
            s.results()
        s.reset()                                       # and the scorer is usable again
        assert all(r.n_reconstructed == 0 for r in s.results() if r is not None)
        return
    got = s.results()
    exp = _scorer_reference(events, {})
    assert len(got) == len(exp) == len(events)
    for a, b, ev in zip(got, exp, events):
        if b is None:
            assert a is None
            continue
        _results_equal(a, b)
        _results_equal(a, BC.event_host(ev))


@pytest.mark.parametrize("mem", ["torch", "hip"])
def test_truth_concat_dev_takes_host_device_and_no_tables(mem):
    import score_cases as SC
    cases = [SC.CASES["thresholds"](), SC.CASES["ids_60bit"]()]
    host = [SC.tables(c) for c in cases]
    pid, px, py = cases[1]["particles"]
    on_dev = metrics.truth_tables_dev(cases[1]["m"], pid, px, py, 7, 7, mem=mem)
    got = metrics.truth_concat_dev([host[0], None, on_dev, host[0]], mem=mem)
    exp = metrics.concat_tables([host[0], None, host[1], host[0]])
    h = got.host()
    for f in FIELDS + list(metrics._OFFSET_FIELDS) + ["scored"]:
        x, y = getattr(h, f), getattr(exp, f)
        assert x.dtype == y.dtype and np.array_equal(x, y), f
    assert h.n_reference == exp.n_reference and got.n_events == 4
    other = "hip" if mem == "torch" else "torch"
    if other == "torch":      # (one direction is enough)
        return
    with pytest.raises(ValueError, match="one allocator"):
        metrics.truth_concat_dev([on_dev, metrics.truth_tables_dev(cases[1]["m"], pid, px, py, 7, 7, mem=other)])


# ------------------------------------------------------------------ the loop
def _golden_tables():
    return [golden()[3], None, None, golden()[3]]


def _run_both(make):
    from gtf import pipeline
    per = [metrics.DeviceScorer(t) if t is not None else None for t in _golden_tables()]
    exp = pipeline.run_batch(make(), iterations=3, scorers=per, lists=False)
    one = metrics.BatchScorer(_golden_tables())
    got = pipeline.run_batch(make(), iterations=3, scorers=one, lists=False)
    assert [[r.counts for r in x] for x in got] == [[r.counts for r in x] for x in exp]
    res = one.results()
    assert res[1] is None and res[2] is None
    for e in (0, 3):
        r = res[e]
        assert (r.n_reconstructed, r.n_reference, r.efficiency_str) == (133, 163, "81.595")
        _results_equal(r, per[e].result(), per_candidate=False)


def test_run_batch_with_one_batch_scorer(event_dirs):  # noqa: F811
    """vol-7, the 257-node hand-made event, an empty window, vol-7"""
    from gtf import pipeline
    _run_both(lambda: [pipeline.build_event_dev(p, 7, 8) for p in _prefixes(event_dirs)])


def test_run_batch_on_the_fused_graph_with_one_batch_scorer(event_dirs):  # noqa: F811
    from gtf import pipeline
    _run_both(lambda: pipeline.build_events_dev(_prefixes(event_dirs), 7, 8))


def test_run_pipeline_batch_metrics(tmp_path):
    """--batch A B --truth T --batch-metrics writes the metrics.json files of the run without the flag"""
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
    ev = os.path.join(GOLDEN, "kat134")
    got = []
    for flags in ([], ["--batch-metrics"]):
        out = str(tmp_path / ("out%d" % len(got)))
        subprocess.check_call([sys.executable, cli, "--batch", ev, ev, "-o", out, "-a", "7", "-z", "7", "--truth", tdir,
                               "--mapping", "full-mapping-minCurv-0.3-134.csv"] + flags)
        got.append([open(os.path.join(out, str(i), "metrics.json"), "rb").read() for i in (0, 1)])
    assert got[0] == got[1] and got[0][0] == got[0][1]
    m = json.loads(got[1][0])
    assert (m["cumulative"]["reconstructed"], m["cumulative"]["efficiency_pct"]) == (133, "81.595")
    assert (m["last_iteration"]["reconstructed"], m["last_iteration"]["efficiency_pct"]) == (1, "0.613")
