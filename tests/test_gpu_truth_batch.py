"""A batch's truth tables in one call (gtf_truth_build_ev, gtf.metrics.truth_tables_batch_dev) against
gtf.metrics.truth_tables_batch, which tests/test_truth_batch_cases.py pins to concat_tables of the
per-event tables, and against the per-event path on the device (truth_concat_dev of truth_tables_dev).
Everything is an integer, so every comparison is array_equal.

  * tests/truth_batch_cases.py through the C-ABI, guard bytes around the six arrays, the three offset
    arrays and the workspace, nothing written past the sums; the raising batches name their event;
  * the golden batch [vol-7, a 257-node event, no truth, vol-7] and BatchScorer on it: 133 / 163 twice;
  * both allocators with host columns, device columns and a mix; truth_files_batch_dev on files;
    run_pipeline.py --batch-truth."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import truth_batch_cases as BC
from fixtures import GOLDEN
from gtf import _native as nat
from gtf import metrics
from test_gpu_score import FILL, Guarded, _csr, _golden_cands, _golden_host, _results_equal, golden
from test_truth_batch_cases import ARRAYS, batches_equal, host_batch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLUMNS = metrics.MAPPING_COLUMNS + ("truth_hit", "truth_part", "part_id", "px", "py")
ERR = {"missing": nat.TRUTH_ERR_MISSING, "range": nat.TRUTH_ERR_RANGE}
TEXT = {"missing": b"a mapped hit has no truth row", "range": b"a volume_id, layer_id or module_id outside [0, 2^21)"}


# ------------------------------------------------------------------ the C-ABI with guard bytes
class Raw:
    """one gtf_truth_build_ev call through ctypes only: the events' columns laid end to end and uploaded
    as they are, the outputs at their bounds (sum of rows (+ 1), K + 1) between fences, pre-filled with FILL"""

    def __init__(self, batch, ws_bytes=None, **change):
        import torch
        self.L = nat.lib()
        parts = BC.parts(batch)
        K = self.K = len(parts)
        per = [[] for _ in range(11)]
        sizes = np.zeros((3, K), np.int64)
        for e, p in enumerate(parts):
            if p is None:
                continue
            cols = [getattr(p[0], c) for c in metrics.MAPPING_COLUMNS] + (list(p[4:6]) if len(p) == 6 else [None, None]) + \
                list(p[1:4])
            for i, a in enumerate(cols):
                if a is not None:
                    per[i].append(np.ascontiguousarray(a, np.float64 if i > 8 else np.int64))
            sizes[:, e] = [cols[0].size, 0 if cols[6] is None else cols[6].size, cols[8].size]
        host = [np.concatenate(c) if c else np.zeros(0, np.float64 if i > 8 else np.int64) for i, c in enumerate(per)]
        self.offs = [np.ascontiguousarray(np.concatenate([[0], np.cumsum(s)]), np.int32) for s in sizes]
        N, NT, NP = (int(o[-1]) for o in self.offs)
        self.n = N
        self.dev = [torch.from_numpy(a).cuda() for a in host]
        vp = lambda x: ctypes.c_void_p(x.data_ptr() if x.numel() else 0)   # noqa: E731
        fields = dict(n_events=K, num_layers=metrics.NUM_DISTINCT_LAYERS, min_volume=batch["window"][0],
                      max_volume=batch["window"][1], pt_cut=metrics.PT_CUT, row_off=self.offs[0].ctypes.data,
                      truth_off=self.offs[1].ctypes.data, particle_off=self.offs[2].ctypes.data,
                      **{k: vp(a) for k, a in zip(COLUMNS, self.dev)})
        fields.update(change)
        self.tin = nat.GtfTruthInEv(**fields)
        self.out = [Guarded(N + (name == "node_ptr"), dt) for name, dt in ARRAYS[:6]] + \
            [Guarded(K + 1, np.int32) for _ in range(3)]
        self.nb = int(self.L.gtf_truth_build_ev_workspace_bytes(N, NT, NP, K)) if ws_bytes is None else ws_bytes
        self.ws = Guarded(self.nb, np.uint8)
        self.buf = nat.GtfTruthBatchBuf(*(o.p for o in self.out[6:] + self.out[:6]))
        self.scored = np.array([p is not None for p in parts], np.uint8)
        self.d_scored = torch.from_numpy(self.scored).cuda() if K else None
        self.batch = nat.GtfTruthBatch(scored=vp(self.d_scored) if K else None)
        self.cnt = (nat.GtfTruthCounts * max(K, 1))(*[nat.GtfTruthCounts(-1, -1, -1, -1, 0, 0) for _ in range(max(K, 1))])

    def run(self, ws=True):
        import torch
        rc = self.L.gtf_truth_build_ev(ctypes.byref(self.tin), ctypes.byref(self.buf), ctypes.byref(self.batch), self.cnt,
                                       self.ws.p if ws else None, ctypes.c_size_t(self.nb if ws else 0), None)
        torch.cuda.synchronize()
        self.ws.get()
        return rc

    def untouched(self):
        """every output still holds its fill"""
        return all(np.all(o.get().view(np.uint8) == FILL) for o in self.out)

    def guards_intact(self):
        for o in self.out + [self.ws]:
            o.get()
        return True

    def tables(self):
        """the nine arrays trimmed to the sums, after checking that nothing was written past them"""
        c, K = self.cnt, self.K
        T, P, R = (sum(getattr(c[e], f) for e in range(K)) for f in ("n_nodes", "n_entries", "n_particles"))
        got = []
        for o, k, (name, _) in zip(self.out, (T, T + 1, P, R, R, R, K + 1, K + 1, K + 1), ARRAYS):
            a = o.get()
            assert 0 <= k <= a.size and np.all(a[k:].view(np.uint8) == FILL), "written past the end of " + name
            got.append(a[:k])
        b = self.batch
        assert (b.n_events, b.n_nodes, b.n_entries, b.n_particles) == (K, T, P, R)
        assert (b.struct_size, b.abi_version) == (ctypes.sizeof(nat.GtfTruthBatch), nat.ABI_VERSION)
        assert [getattr(b, name) for name, _ in ARRAYS] == [o.p.value for o in self.out]
        assert (b.scored or 0) == (self.d_scored.data_ptr() if K else 0)
        return metrics.BatchTables(*got, self.scored, [int(c[e].n_reference) if self.scored[e] else None for e in range(K)])


def _per_event_dev(batch, **kw):
    """the parent path: one truth_tables_dev per event, then truth_concat_dev"""
    tables = []
    for p in BC.parts(batch):
        tables.append(None if p is None else metrics.truth_tables_dev(p[0], p[1], p[2], p[3], *batch["window"], *p[4:6], **kw))
    return metrics.truth_concat_dev(tables, **kw)


@pytest.mark.parametrize("name", BC.NON_RAISING)
def test_batches_through_the_c_abi(name):
    batch = BC.BATCHES[name]()
    host = host_batch(batch)
    raw = Raw(batch)
    assert raw.run() == 0, raw.L.gtf_last_error()
    got = raw.tables()
    batches_equal(got, host)
    for e in range(raw.K):
        c = raw.cnt[e]
        assert (c.n_nodes, c.n_entries, c.n_particles) == tuple(int(o[e + 1] - o[e]) for o in (
            host.node_off, host.entry_off, host.part_off)), e
        assert c.n_reference == (host.n_reference[e] or 0) and c.error == 0, e
    assert raw.guards_intact()


@pytest.mark.parametrize("name", BC.NON_RAISING)
def test_both_sides_on_the_gpu(name):
    batch = BC.BATCHES[name]()
    one = metrics.truth_tables_batch_dev(BC.parts(batch), *batch["window"])
    per = _per_event_dev(batch)
    assert (one.n_events, one.n_nodes, one.n_entries, one.n_particles) == (per.n_events, per.n_nodes, per.n_entries,
                                                                           per.n_particles)
    for name_, _ in ARRAYS:     # byte for byte, at the same lengths
        a, b = getattr(one, name_), getattr(per, name_)
        assert a.dtype == b.dtype and a.numel() == b.numel(), name_
    batches_equal(one.host(), per.host())
    batches_equal(one.host(), host_batch(batch))


@pytest.mark.parametrize("name", BC.RAISING)
def test_raising_batches_name_their_event(name):
    batch = BC.BATCHES[name]()
    e, kind = batch["raises"]
    raw = Raw(batch)
    assert raw.run() == -2
    msg = raw.L.gtf_last_error()
    assert b"event %d: " % e + TEXT[kind] in msg, msg
    assert raw.cnt[e].error == ERR[kind]
    assert all(raw.cnt[k].error == 0 for k in range(raw.K) if k != e)
    assert raw.guards_intact()
    text = r"^event %d: a mapped hit has no truth row" if kind == "missing" else r"^event %d: a volume_id, layer_id or " \
        r"module_id outside \[0, 2097152\)"
    with pytest.raises(ValueError, match=text % e):
        metrics.truth_tables_batch_dev(BC.parts(batch), *batch["window"])


def test_an_explicit_empty_truth_beside_rows_is_refused_on_the_host():
    batch = BC.BATCHES["truth_beside_own"]()
    parts = BC.parts(batch)
    empty = np.zeros(0, np.int64)
    parts[1] = parts[1][:4] + (empty, empty)
    with pytest.raises(ValueError, match="^event 1: a mapped hit has no truth row"):
        metrics.truth_tables_batch_dev(parts, *batch["window"])
    parts[1] = parts[1][:4] + (empty, np.zeros(1, np.int64))
    with pytest.raises(ValueError, match="^event 1: truth columns of different lengths"):
        metrics.truth_tables_batch_dev(parts, *batch["window"])
    with pytest.raises(ValueError, match="min_volume > max_volume"):
        metrics.truth_tables_batch_dev(BC.parts(batch), 8, 7)


def test_refusals_on_the_host_write_nothing():
    batch = BC.BATCHES["truth_beside_own"]()
    need = Raw(batch).nb
    bad_off = np.array([0, 3, 2, 5, 6], np.int32)
    for kw, text in (({"min_volume": 9}, b"min_volume > max_volume"), ({"ws_bytes": need - 1}, b"workspace"),
                     ({"layer_id": None}, b"mapping column"), ({"px": None}, b"part_id / px / py"),
                     ({"truth_hit": None}, b"truth_hit"), ({"n_events": -1}, b"negative"),
                     ({"row_off": bad_off.ctypes.data}, b"row_off is negative or decreases"),
                     ({"particle_off": None}, b"particle_off")):
        raw = Raw(batch, **kw)
        assert raw.run() == -2 and text in raw.L.gtf_last_error(), kw
        assert raw.untouched() and all(c.error == 0 for c in raw.cnt), kw
    raw = Raw(batch)
    raw.tin.abi_version += 1
    assert raw.run() == -3 and raw.untouched()
    raw = Raw(batch)
    raw.batch.struct_size += 8
    assert raw.run() == -3 and raw.untouched()
    raw = Raw(batch)
    raw.buf.part_off = None
    assert raw.run() == -2 and b"missing array" in raw.L.gtf_last_error() and raw.untouched()
    raw = Raw(batch)                       # ... and the same object goes through untouched by all that
    assert raw.run() == 0
    batches_equal(raw.tables(), host_batch(batch))


@pytest.mark.parametrize("name", ["only_empty", "none_only", "no_events"])
def test_no_rows_writes_the_offsets_and_node_ptr_only(name):
    batch = BC.BATCHES[name]()
    raw = Raw(batch)
    assert not raw.tin.node_idx and not raw.tin.module_id      # no column is needed, nor the workspace
    assert raw.run(ws=False) == 0, raw.L.gtf_last_error()
    got = raw.tables()
    assert list(got.node_ptr) == [0]
    for f in ("node_off", "entry_off", "part_off"):
        assert list(getattr(got, f)) == [0] * (raw.K + 1)
    assert np.all(raw.ws.get() == FILL)
    batches_equal(got, host_batch(batch))
    d = metrics.truth_tables_batch_dev(BC.parts(batch), *batch["window"])
    batches_equal(d.host(), host_batch(batch))
    assert [r is None or (r.n_reconstructed, r.n_reference) == (0, 0) for r in metrics.BatchScorer(d).results()] == \
        [True] * raw.K


# ------------------------------------------------------------------ the golden batch
def _golden_parts():
    z, m, part, _ = golden()
    hand = BC.chain(257, extra_truth=3)                # a 257-node event with truth columns of its own
    return [(m,) + tuple(part), BC.part(hand), None, (m,) + tuple(part)], hand


def test_golden_batch_and_its_scores():
    import torch
    parts, hand = _golden_parts()
    d = metrics.truth_tables_batch_dev(parts, 7, 7)
    host = metrics.truth_tables_batch(parts, 7, 7)
    batches_equal(d.host(), host)
    sizes = [tuple(int(o[e + 1] - o[e]) for o in (host.node_off, host.entry_off, host.part_off)) for e in range(4)]
    assert sizes[0] == sizes[3] == (8748, 13129, 246) and sizes[1][0] == 257 and sizes[2] == (0, 0, 0)
    assert d.n_reference[0] == d.n_reference[3] == 163 and d.n_reference[2] is None and list(d.scored) == [1, 1, 0, 1]
    cands = _golden_cands("cumulative")
    ptr, ids = _csr(cands + cands)
    n = len(cands)
    first = np.array([0, n, n, n, 2 * n], np.int32)
    s = metrics.BatchScorer(d)
    assert s.tables is d
    s.add(torch.from_numpy(ptr).cuda(), torch.from_numpy(ids).cuda(), torch.from_numpy(first).cuda(), 2 * n, 0,
          per_candidate=True)
    res = s.results()
    assert res[2] is None and res[1].n_reconstructed == 0
    exp = _golden_host("cumulative")
    for e in (0, 3):
        assert (res[e].n_reconstructed, res[e].n_reference, res[e].efficiency_str) == (133, 163, "81.595")
        _results_equal(res[e], exp)


# ------------------------------------------------------------------ allocators; host, device and mixed columns
def _on_device(parts, mem):
    if mem == "hip":
        from gtf.devmem import HipArray
        up = HipArray.from_numpy
    else:
        import torch
        up = lambda a: torch.from_numpy(a).cuda()    # noqa: E731
    out = []
    for p in parts:
        if p is None:
            out.append(None)
            continue
        cols = [np.ascontiguousarray(getattr(p[0], c), np.int64) for c in metrics.MAPPING_COLUMNS] + \
            [np.ascontiguousarray(p[1], np.int64), np.ascontiguousarray(p[2], np.float64), np.ascontiguousarray(p[3], np.float64)] + \
            [np.ascontiguousarray(a, np.int64) for a in p[4:6]]
        cols = [up(a) for a in cols]
        out.append((metrics.HitMapping(*cols[:6]),) + tuple(cols[6:]))
    return out


@pytest.mark.parametrize("mem", ["torch", "hip"])
def test_both_allocators_host_and_device_columns(mem):
    from gtf.devmem import HipArray
    for name in ("truth_beside_own", "none_between", "runs_beside_one_row", "random_0", "one_row_x257",
                 "alone_truth_selects", "alone_runs"):       # (one event on the device: its columns are used where they are)
        batch = BC.BATCHES[name]()
        host = host_batch(batch)
        parts = [p for p in BC.parts(batch)]
        a = metrics.truth_tables_batch_dev(parts, *batch["window"], mem=mem)
        assert isinstance(a.node_id, HipArray) == (mem == "hip") and a.mem == mem
        batches_equal(a.host(), host)
        b = metrics.truth_tables_batch_dev(_on_device(parts, mem), *batch["window"], mem=mem)
        batches_equal(b.host(), host)
    parts, _ = _golden_parts()
    batches_equal(metrics.truth_tables_batch_dev(_on_device(parts, mem), 7, 7, mem=mem).host(),
                  metrics.truth_tables_batch(parts, 7, 7))
    mixed = _on_device(parts[:1], mem) + parts[1:]
    with pytest.raises(ValueError, match="all host arrays or all device arrays"):
        metrics.truth_tables_batch_dev(mixed, 7, 7, mem=mem)
    dev = _on_device(parts[:1], mem)[0]
    with pytest.raises(ValueError, match="all host arrays or all device arrays"):
        metrics.truth_tables_batch_dev([(dev[0], parts[0][1], dev[2], dev[3])], 7, 7, mem=mem)


@pytest.mark.parametrize("mem", ["torch", "hip"])
def test_truth_files_batch_dev(tmp_path, mem):
    """the files of three events (one with a truth.csv, one without truth at all) parsed per file on the
    device, then one build: the tables of the host columns"""
    import pandas as pd
    batch = BC.BATCHES["truth_beside_own"]()
    cases = batch["events"][:2]
    pres = []
    for i, c in enumerate(cases):
        pre = str(tmp_path / ("ev%d-" % i))
        pd.DataFrame({k: getattr(c["m"], k) for k in metrics.MAPPING_COLUMNS}).to_csv(pre + "map.csv", index=False)
        pid, px, py = c["particles"]
        pd.DataFrame({"particle_id": pid, "px": px, "py": py}).to_csv(pre + "particles.csv", index=False)
        if c["truth"] is not None:
            pd.DataFrame({"hit_id": c["truth"][0], "particle_id": c["truth"][1]}).to_csv(pre + "truth.csv", index=False)
        pres.append(pre)
    assert os.path.isfile(pres[0] + "truth.csv") and not os.path.isfile(pres[1] + "truth.csv")
    got, infos = metrics.truth_files_batch_dev([pres[0], None, pres[1]], "map.csv", *batch["window"], mem=mem)
    assert infos[1] is None and infos[0]["truth"] == infos[0]["mapping"] == infos[2]["particles"] == "device"
    assert "truth" not in infos[2] and got.mem == mem
    batches_equal(got.host(), metrics.truth_tables_batch([BC.part(cases[0]), None, BC.part(cases[1])], *batch["window"]))


# ------------------------------------------------------------------ the CLI
def test_run_pipeline_batch_truth(tmp_path):
    """--batch A B --truth T --batch-metrics --batch-truth writes the metrics.json files of the run without
    --batch-truth, byte for byte; the flag without --batch-metrics is an argument error"""
    import pandas as pd
    z = golden()[0]
    tdir = str(tmp_path / "truth")
    os.makedirs(tdir)
    pd.DataFrame({c: z["map__" + c] for c in metrics.MAPPING_COLUMNS}).to_csv(
        os.path.join(tdir, "event000001000-full-mapping-minCurv-0.3-134.csv"), index=False)
    pd.DataFrame({c: z["particles__" + c] for c in ("particle_id", "px", "py")}).to_csv(
        os.path.join(tdir, "event000001000-particles.csv"), index=False)
    cli = os.path.join(ROOT, "gnn-track-finding_amd", "run_pipeline.py")
    ev = os.path.join(GOLDEN, "kat134")
    common = ["-a", "7", "-z", "7", "--truth", tdir, "--mapping", "full-mapping-minCurv-0.3-134.csv"]
    got = []
    for flags in (["--batch-metrics"], ["--batch-metrics", "--batch-truth"]):
        out = str(tmp_path / ("out%d" % len(got)))
        subprocess.check_call([sys.executable, cli, "--batch", ev, ev, "-o", out] + common + flags)
        got.append([open(os.path.join(out, str(i), "metrics.json"), "rb").read() for i in (0, 1)])
    assert got[0] == got[1] and got[1][0] == got[1][1]
    assert b'"81.595"' in got[1][0] and b'"0.613"' in got[1][0]
    r = subprocess.run([sys.executable, cli, "--batch", ev, ev, "-o", str(tmp_path / "x"), "--batch-truth"] + common,
                       capture_output=True, text=True)
    assert r.returncode == 2 and "--batch-metrics" in r.stderr
