"""The batched scoring (gtf_truth_concat, gtf_score_*_ev, gtf.metrics.BatchScorer) without a GPU:
metrics.concat_tables against its per-event inputs; a pure-NumPy restatement of the batch rule --
segment lookups, keys rebased to the event, per-event match order -- that reproduces, per event,
metrics.reconstruction_efficiency's Result for every batch of tests/score_batch_cases.py; every batch
reaches the branch it is named for; the header, the library's exports and gtf._native agree on the new
symbols and structs; the refusals the header promises come back before any launch."""
import collections
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import score_batch_cases as BC
import score_cases as SC
from gtf import _native as nat
from gtf import metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "gtf.h")
NEW_SYMBOLS = ("gtf_truth_concat_workspace_bytes", "gtf_truth_concat", "gtf_score_reset_ev",
               "gtf_score_ev_workspace_bytes", "gtf_score_candidates_ev", "gtf_score_finish_ev_workspace_bytes",
               "gtf_score_finish_ev")
STRUCTS = {"gtf_truth_batch": "GtfTruthBatch", "gtf_truth_sizes": "GtfTruthSizes", "gtf_truth_part": "GtfTruthPart",
           "gtf_truth_batch_buf": "GtfTruthBatchBuf", "gtf_score_state_ev": "GtfScoreStateEv"}
NONE = (1 << 64) - 1
NAMES = sorted(BC.BATCHES)


# ------------------------------------------------------------------ concat_tables
@pytest.mark.parametrize("name", NAMES)
def test_concat_tables_against_its_inputs(name):
    events = BC.BATCHES[name]()
    tables = [BC.event_tables(ev) for ev in events]
    b = metrics.concat_tables(tables)
    K = len(events)
    for off, field in ((b.node_off, "node_id"), (b.entry_off, "node_part"), (b.part_off, "part_id")):
        sizes = [0 if t is None else getattr(t, field).size for t in tables]
        assert off.dtype == np.int32 and off.shape == (K + 1,) and off[0] == 0 and np.array_equal(np.diff(off), sizes)
        assert getattr(b, field).size == off[-1]
    assert b.node_ptr.size == b.node_off[-1] + 1 and b.node_ptr[-1] == b.entry_off[-1]
    assert np.array_equal(b.scored, [t is not None for t in tables]) and b.scored.dtype == np.uint8
    assert b.n_reference == [None if t is None else t.n_reference for t in tables]
    for e, t in enumerate(tables):
        got = b.event(e)
        if t is None:
            assert got is None and b.node_off[e] == b.node_off[e + 1] and b.part_off[e] == b.part_off[e + 1]
            continue
        for f, dt in metrics._TABLE_FIELDS:   # every event's slice, shifted back, is its own table
            x, y = getattr(got, f), getattr(t, f)
            assert x.dtype == np.dtype(dt) and np.array_equal(x, y), (e, f)
        assert got.n_reference == t.n_reference


def test_concat_tables_of_nothing():
    b = metrics.concat_tables([])
    assert b.node_ptr.tolist() == [0] and b.node_off.tolist() == [0] and b.scored.size == 0 and b.n_reference == []
    b = metrics.concat_tables([None, None])
    assert b.node_ptr.tolist() == [0] and b.part_off.tolist() == [0, 0, 0] and b.scored.tolist() == [0, 0]


# ------------------------------------------------------------------ the batch rule in NumPy
class Rule:
    """gtf_score_reset_ev / _candidates_ev / _finish_ev restated on the host arrays of a BatchTables"""

    def __init__(self, b):
        self.b = b
        R = int(b.part_off[-1])
        self.key = np.full(R, NONE, np.uint64)
        self.good, self.total = np.zeros(R, np.int64), np.zeros(R, np.int64)
        self.error = None     # the smallest event with a missing id

    def reset(self, events):
        for e in np.flatnonzero(events):
            self.key[self.b.part_off[e]:self.b.part_off[e + 1]] = NONE

    def add(self, group, first, cands):
        """-> (pid, n_good, total, passes) per candidate"""
        b = self.b
        out = np.zeros((4, len(cands)), np.int64)
        claims = []
        for c, members in enumerate(cands):
            e = int(np.searchsorted(first, c, side="right")) - 1
            if not b.scored[e]:
                continue
            ids = b.node_id[b.node_off[e]:b.node_off[e + 1]]          # the event's own segment
            parts = []
            for v in members:
                k = int(np.searchsorted(ids, v))
                if k >= ids.size or ids[k] != v:
                    self.error = e if self.error is None else min(self.error, e)
                    continue
                k += int(b.node_off[e])
                parts += b.node_part[b.node_ptr[k]:b.node_ptr[k + 1]].tolist()
            if not parts:
                continue
            count = collections.Counter(parts)
            pid = max(count, key=count.get)                           # ties to the id seen first
            n_good, total = count[pid], len(parts)
            seg = b.part_id[b.part_off[e]:b.part_off[e + 1]]
            r = int(np.searchsorted(seg, pid))
            ok = r < seg.size and seg[r] == pid
            if ok:
                r += int(b.part_off[e])
                ok = bool(b.part_ref[r]) and 2 * n_good >= b.part_hits[r] and 2 * n_good >= total
            out[:, c] = pid, n_good, total, ok
            if ok:
                key = (group << 32) | (c - int(first[e]))             # rebased to the event
                claims.append((r, key, n_good, total))
                self.key[r] = min(int(self.key[r]), key)
        for r, key, n_good, total in claims:
            if int(self.key[r]) == key:
                self.good[r], self.total[r] = n_good, total
        return out

    def results(self):
        b, out = self.b, []
        for e in range(b.scored.size):
            if not b.scored[e]:
                out.append(None)
                continue
            lo, hi = int(b.part_off[e]), int(b.part_off[e + 1])
            rows = lo + np.argsort(self.key[lo:hi], kind="stable")
            rows = rows[self.key[rows] != NONE]                        # match order: ascending key
            g = self.good[rows] * 1.0
            out.append((rows.size, b.n_reference[e], g / self.total[rows], g / b.part_hits[rows], self.key[rows]))
        return out


def _run_rule(events):
    """the batch through the rule, the calls by descending group -> (Rule, per call the per-candidate
    outputs, the calls)"""
    rule = Rule(metrics.concat_tables([BC.event_tables(ev) for ev in events]))
    calls = BC.batch_calls(events)
    per = {g: rule.add(g, first, cands) for g, first, cands in reversed(calls)}
    return rule, per, calls


def _check_event(e, ev, got, per, calls):
    host = BC.event_host(ev)
    if host is None:
        assert got is None
        return
    n, n_ref, tpur, ppur, keys = got
    assert (n, n_ref) == (host.n_reconstructed, host.n_reference), e
    assert np.array_equal(tpur, host.track_purities) and np.array_equal(ppur, host.particle_purities), e
    # the per-candidate outputs of the event, by ascending group, and the matched candidates from the keys
    mine = [per[g][:, first[e]:first[e + 1]] for g, first, _ in calls]
    start = np.cumsum([0] + [m.shape[1] for m in mine])
    pid, good = (np.concatenate([m[i] for m in mine]) if mine else np.zeros(0, np.int64) for i in (0, 1))
    assert np.array_equal(pid, host.reconstructed_pid) and np.array_equal(good, host.n_good), e
    where = [int(start[[g for g, _, _ in calls].index(int(k) >> 32)]) + (int(k) & 0xffffffff) for k in keys]
    assert np.array_equal(where, np.flatnonzero(host.matched)), e


@pytest.mark.parametrize("name", [n for n in NAMES if n not in BC.MISSING])
def test_batch_rule_reproduces_every_events_result(name):
    events = BC.BATCHES[name]()
    rule, per, calls = _run_rule(events)
    assert rule.error is None
    res = rule.results()
    seen = {}
    for e, ev in enumerate(events):
        if id(ev) in seen and name.startswith("large"):      # (the same object again: the same answer)
            assert res[e][0] == res[seen[id(ev)]][0] and np.array_equal(res[e][2], res[seen[id(ev)]][2])
            continue
        seen[id(ev)] = e
        _check_event(e, ev, res[e], per, calls)


@pytest.mark.parametrize("name", sorted(BC.MISSING))
def test_missing_names_its_event(name):
    events = BC.BATCHES[name]()
    e = BC.MISSING[name]
    with pytest.raises(ValueError, match="no hit_dissociation"):
        BC.event_host(events[e])
    missing = events[e]["calls"][0][1][1][-1]
    assert missing not in BC.event_tables(events[e]).node_id
    for other in (e - 1, e + 1):     # ... but the neighbours know the id
        if 0 <= other < len(events) and name != "missing_last":
            assert missing in BC.event_tables(events[other]).node_id
    if name == "missing_middle":
        assert len(events) == 3
    assert _run_rule(events)[0].error == e


# ------------------------------------------------------------------ every batch reaches its branch
def _matched(ev):
    return BC.event_host(ev).n_reconstructed


def test_batches_reach_their_branches():
    B = {n: f() for n, f in BC.BATCHES.items() if not n.startswith(("singleton_", "random_"))}
    assert set("singleton_" + n for n in SC.CASES) <= set(BC.BATCHES) and len(SC.CASES) == 17
    a, b = B["twice"]
    assert a is b and _matched(a) >= 2
    ev = B["same_node_other_particles"]
    t = [BC.event_tables(x) for x in ev]
    assert t[0].node_id[0] == t[1].node_id[0] == t[2].node_id[0] == ev[0]["calls"][0][1][0][0]
    assert t[0].node_part[0] != t[1].node_part[0] and t[0].part_id[0] == t[2].part_id[0]
    assert t[0].part_hits[0] != t[2].part_hits[0] and all(_matched(x) == 1 for x in ev)
    ev = B["empty_events"]
    n_cand = [sum(len(cs) for _, cs in x["calls"]) for x in ev]
    assert n_cand[0] == n_cand[2] == n_cand[-1] == 0 and n_cand[1] > 0 and n_cand[4] > 0
    t = BC.event_tables(ev[3])
    assert t.node_id.size == t.part_id.size == t.node_part.size == 0
    ev = B["unscored_between"]
    assert BC.event_tables(ev[1]) is None and BC.event_tables(ev[0]) is not None and BC.event_tables(ev[2]) is not None
    known = set(BC.event_tables(ev[0]).node_id) | set(BC.event_tables(ev[2]).node_id)
    assert any(v not in known for c in ev[1]["calls"][0][1] for v in c)
    # event boundaries inside a wavefront's four candidates, every size on both sides of one
    ev = B["boundaries"]
    first = BC.batch_calls(ev)[0][1]
    assert {1, 2, 3} <= set(int(x) % 4 for x in first[1:-1])
    before = {x["expect"]["sizes"][-1] for x in ev[:-1]}
    after = {x["expect"]["sizes"][0] for x in ev[1:]}
    sizes = {s for x in ev for s in x["expect"]["sizes"]}
    assert sizes == set(BC.SIZES) and {1, 2, 16, 17, 63, 65} <= before | after
    for x in ev:
        ptr, ids, _ = SC.flatten(x)
        tt = BC.event_tables(x)
        cand_of, _ = metrics.candidate_particles(ptr, ids, tt.node_id, tt.node_ptr.astype(np.int64), tt.node_part)
        assert np.array_equal(np.bincount(cand_of, minlength=len(ptr) - 1), x["expect"]["sizes"])
    # a neighbour with fewer groups: the calls have different cand_first
    calls = BC.batch_calls(B["group_orders"])
    assert [g for g, _, _ in calls] == [0, 1] and not np.array_equal(calls[0][1], calls[1][1])
    assert calls[1][1][1] == calls[1][1][2]       # (the middle event has no candidate in group 1)
    ev = B["finish"]
    assert [_matched(x) for x in ev] == [2, 0, 2, 3]
    assert BC.event_tables(ev[0]).part_id.size == 2                      # every region particle matched
    assert BC.event_tables(ev[3]).part_id.min() < -SC.B60 and BC.event_tables(ev[2]).part_id.max() > SC.B60
    for K in (65, 257, 2049):
        ev = B["large_%d" % K]
        assert len(ev) == K and all(sum(len(cs) for _, cs in x["calls"]) == 1 for x in ev[:3])
        assert [_matched(x) for x in ev[:3]] == [1, 0, 1]
    assert 2049 + 1 > 2048          # (the offsets of the largest no longer fit the LDS staging)
    ties = dups = 0
    for s in range(5):
        ev = BC.BATCHES["random_%d" % s]()
        assert 3 <= len(ev) <= 9
        for x in ev:
            h = BC.event_host(x)
            dups += bool(h.n_reconstructed and np.isin(h.reconstructed_pid[~h.matched], h.reconstructed_pid[h.matched]).any())
            ptr, ids, cands = SC.flatten(x)
            tt = BC.event_tables(x)
            cand_of, part = metrics.candidate_particles(ptr, ids, tt.node_id, tt.node_ptr.astype(np.int64), tt.node_part)
            for c in range(len(cands)):
                n = np.sort(np.unique(part[cand_of == c], return_counts=True)[1])
                if n.size >= 2 and n[-1] == n[-2]:
                    ties += 1
                    break
    assert ties >= 15 and dups >= 15


def test_partial_reset_keeps_the_other_events():
    """score, reset a mask of events, add again with group 0: the unmasked events keep their claims"""
    events = BC.BATCHES["group_orders"]()
    rule, _, calls = _run_rule(events)
    before = rule.key.copy()
    mask = np.array([1, 0, 1], bool)
    rule.reset(mask)
    b = rule.b
    assert np.all(rule.key[b.part_off[0]:b.part_off[1]] == NONE) and np.array_equal(
        rule.key[b.part_off[1]:b.part_off[2]], before[b.part_off[1]:b.part_off[2]])
    assert np.any(before[b.part_off[1]:b.part_off[2]] != NONE)
    g, first, cands = calls[1]
    rule.add(0, first, cands)
    res = rule.results()
    assert res[1][0] == BC.event_host(events[1]).n_reconstructed
    # events 0 and 2 now hold their group-1 candidates alone, scored as group 0
    for e in (0, 2):
        only = dict(events[e], calls=[(0, [c for gg, cs in events[e]["calls"] if gg == 1 for c in cs])])
        only.pop("host", None)
        h = SC.host_result(only)
        assert res[e][0] == h.n_reconstructed and np.array_equal(res[e][2], h.track_purities)


# ------------------------------------------------------------------ header, exports, _native
def test_symbols_declared_exported_and_listed():
    src = open(HDR).read()
    declared = set(re.findall(r"^\s*(?:int|size_t|const char\*)\s+(gtf_\w+)\s*\(", src, re.M))
    nat.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", nat.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (gtf_\w+)", out))
    for s in NEW_SYMBOLS:
        assert s in declared and s in exported and s in nat.SYMBOLS, s
    ver = re.search(r"#define GTF_ABI_VERSION (\d+)u", src)
    assert ver and int(ver.group(1)) == nat.ABI_VERSION == 8


def test_structs_match_header():
    py = {t: getattr(nat, c) for t, c in STRUCTS.items()}
    lines = []
    for t, cls in py.items():
        lines += ['  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (t, f, t, f) for f, _ in cls._fields_]
        lines.append('  printf("sizeof.%s %%zu\\n", sizeof(%s));' % (t, t))
    probe = "#include <stdio.h>\n#include <stddef.h>\n#include \"gtf.h\"\nint main(void) {\n%s\n  return 0;\n}\n" % \
        "\n".join(lines)
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "p.c")
        open(c, "w").write(probe)
        exe = os.path.join(d, "p")
        subprocess.check_call(["gcc", "-I", os.path.dirname(HDR), c, "-o", exe])
        got = dict(l.rsplit(" ", 1) for l in subprocess.check_output([exe], text=True).split("\n") if l)
    assert len(got) == sum(len(c._fields_) + 1 for c in py.values())
    for k, v in got.items():
        t, f = k.split(".")
        if t == "sizeof":
            assert ctypes.sizeof(py[f]) == int(v), k
        else:
            assert getattr(py[t], f).offset == int(v), k
    for cls in (nat.GtfTruthBatch, nat.GtfScoreStateEv):
        assert cls().struct_size == ctypes.sizeof(cls) and cls().abi_version == 8


def test_workspace_sizes():
    L = nat.lib()
    ws, fin, cat = L.gtf_score_ev_workspace_bytes, L.gtf_score_finish_ev_workspace_bytes, L.gtf_truth_concat_workspace_bytes
    assert ws(0, 0, 0) > 0 and fin(0, 0) > 0 and cat(0) > 0 and ws(-5, -5, -5) == ws(0, 0, 0) and fin(-1, -1) == fin(0, 0)
    last = [0, 0, 0, 0]
    for n in (0, 1, 3, 255, 256, 257, 1000, 4097, 100000, 1 << 20):
        now = [ws(n, 1000, 8), ws(1000, n, 8), fin(n, 8), fin(1000, n)]
        assert all(x >= y for x, y in zip(now, last)), n
        last = now
    assert ws(1000, 6000, 8) == ws(1000, 6000, 4096)                       # (nothing is sized by K)
    assert ws(1000, 6000, 8) >= L.gtf_score_workspace_bytes(1000, 6000) + 4 * 1000   # one word per candidate more
    assert fin(1000, 64) >= 16 * 1000 + 4 * 65


def test_refusals_come_before_any_launch():
    """host buffers and a NULL stream: only for calls the library must refuse on the host"""
    L = nat.lib()
    buf = (ctypes.c_uint8 * 4096)()
    a, null = ctypes.cast(buf, ctypes.c_void_p), ctypes.c_void_p(0)
    big = ctypes.c_size_t(1 << 20)

    def batch(**kw):
        f = dict(n_events=2, n_nodes=4, n_entries=4, n_particles=2,
                 **{k: a for k in ("node_off", "entry_off", "part_off", "node_id", "node_ptr", "node_part", "part_id",
                                   "part_hits", "part_ref")})
        f.update(kw)
        return nat.GtfTruthBatch(**f)

    def state(**kw):
        f = dict(n_particles=2, best_key=a, best_good=a, best_total=a, error=a)
        f.update(kw)
        return nat.GtfScoreStateEv(**f)

    def cand(b=None, s=None, ptr=a, ids=a, first=a, n=4, group=0, ws=a, nb=big):
        b, s = b or batch(), s or state()
        return L.gtf_score_candidates_ev(ctypes.byref(b), ptr, ids, first, n, group, None, ctypes.byref(s), ws, nb, None)

    old = batch()
    old.abi_version = 7
    assert cand(b=old) == -3 and b"gtf_truth_batch ABI mismatch" in L.gtf_last_error()
    old = state()
    old.struct_size -= 8
    assert cand(s=old) == -3 and b"gtf_score_state_ev ABI mismatch" in L.gtf_last_error()
    assert L.gtf_score_candidates_ev(None, a, a, a, 4, 0, None, ctypes.byref(state()), a, big, None) == -2
    assert cand(b=batch(n_events=-1)) == -2 and cand(b=batch(part_off=null)) == -2 and cand(b=batch(node_id=null)) == -2
    assert cand(s=state(n_particles=3)) == -2 and b"differs" in L.gtf_last_error()
    assert cand(s=state(error=null)) == -2 and cand(s=state(best_key=null)) == -2
    assert cand(n=-1) == -2 and cand(group=-1) == -2
    assert cand(ptr=null) == -2 and cand(ids=null) == -2 and cand(first=null) == -2 and cand(ws=null) == -2
    assert cand(nb=ctypes.c_size_t(L.gtf_score_ev_workspace_bytes(4, 0, 2) - 1)) == -2 and b"workspace" in L.gtf_last_error()
    assert cand(n=0, ptr=null, ids=null, first=null, ws=null) == 0            # nothing launched
    # reset and finish
    b, s = batch(), state()
    assert L.gtf_score_reset_ev(None, ctypes.byref(b), None, None) == -2
    assert L.gtf_score_reset_ev(ctypes.byref(s), None, None, None) == -2
    assert L.gtf_score_reset_ev(ctypes.byref(old), ctypes.byref(b), None, None) == -3
    n_rec, err = (ctypes.c_int32 * 2)(), (ctypes.c_uint32 * 2)()
    fin = lambda b=b, s=s, first=a, n=n_rec, e=err, ws=a, nb=big: L.gtf_score_finish_ev(   # noqa: E731
        ctypes.byref(b), ctypes.byref(s), a, a, a, a, a, first, n, e, ws, nb, None)
    assert fin(first=null) == -2 and fin(n=None) == -2 and fin(e=None) == -2 and fin(ws=null) == -2
    assert fin(nb=ctypes.c_size_t(L.gtf_score_finish_ev_workspace_bytes(2, 2) - 1)) == -2
    assert fin(s=old) == -3 and fin(s=state(n_particles=5)) == -2
    # concat
    sizes = (nat.GtfTruthSizes * 2)()
    bb = nat.GtfTruthBatchBuf(*([a] * 9))
    out = nat.GtfTruthBatch()
    cc = lambda sizes=sizes, parts=a, k=2, bb=bb, out=out, ws=a, nb=big: L.gtf_truth_concat(   # noqa: E731
        sizes, parts, k, ctypes.byref(bb) if bb is not None else None, ctypes.byref(out) if out is not None else None,
        ws, nb, None)
    assert cc(out=None) == -2 and cc(bb=None) == -2 and cc(k=-1) == -2 and cc(sizes=None) == -2 and cc(parts=null) == -2
    assert cc(ws=null) == -2 and cc(nb=ctypes.c_size_t(L.gtf_truth_concat_workspace_bytes(2) - 1)) == -2
    stale = nat.GtfTruthBatch()
    stale.abi_version = 9
    assert cc(out=stale) == -3
    neg = (nat.GtfTruthSizes * 2)()
    neg[1].n_entries = -1
    assert cc(sizes=neg) == -2 and b"negative" in L.gtf_last_error()
    huge = (nat.GtfTruthSizes * 2)()
    huge[0].n_particles = huge[1].n_particles = 1 << 30
    assert cc(sizes=huge) == -2 and b"2^31" in L.gtf_last_error()
    bad = nat.GtfTruthBatchBuf(*([a] * 9))
    bad.entry_off = None
    assert cc(bb=bad) == -2 and b"missing" in L.gtf_last_error()


def test_run_pipeline_refuses_batch_metrics_alone(tmp_path):
    import sys
    cli = os.path.join(ROOT, "gnn-track-finding_amd", "run_pipeline.py")
    for extra in ([], ["--batch", "a", "b"], ["--truth", "t", "-n", "x"]):
        r = subprocess.run([sys.executable, cli, "-o", str(tmp_path), "--batch-metrics"] + extra, capture_output=True,
                           text=True)
        assert r.returncode == 2 and "--batch-metrics" in r.stderr
