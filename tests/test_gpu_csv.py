"""The CSV front end on the device (gtf_csv_parse, gtf_event_window, gtf_event_radius_patch; gtf.csvdev,
gtf.io.read_nodes_dev / read_edges_dev, pipeline.build_event_dev(parse="device"),
gtf.metrics.truth_files_dev, run_pipeline.py --resident-parse) against the host readers, which
tests/test_csv_cases.py pins to the rule of tests/csv_cases.py. Every comparison is of bit patterns.

  * every case of tests/csv_cases.py and 20 seeded random files through the C-ABI, the outputs at their
    bound max_rows between guard bytes: the columns, the counts, the error bits, the first bad
    (row, field) and its bit; nothing written past n_rows;
  * the window cases through the C-ABI against NumPy, the ambiguous list against the exact rule;
  * kat134 and kat800: read_nodes_dev / read_edges_dev equal read_nodes / read_edges array for array,
    r included; the ambiguous list holds every node where pow and x * x differ, and the patch changes r;
  * build_event_dev(parse="device") equals parse="host" under both allocators; a 16-digit coordinate
    falls back to the host reader, visibly; truth_files_dev equals truth_tables; the CLI."""
import ctypes
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import csv_cases as CC
from fixtures import GOLDEN
from gtf import _native as nat
from gtf import csvdev, metrics
from gtf import io as gio
from test_gpu_event_pack import _graphs_equal, _same
from test_gpu_score import FILL, Guarded, golden

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "gnn-track-finding_amd", "run_pipeline.py")
KATS = {"kat134": (7, 7), "kat800": (7, 9)}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else a.dtype)


# ------------------------------------------------------------------ the C-ABI with guard bytes
class Raw:
    """one gtf_csv_parse call through ctypes only: the text uploaded as it is, one output per column
    at its bound max_rows between fences, pre-filled with FILL"""

    def __init__(self, case, max_rows=None):
        import torch
        self.L, self.case = nat.lib(), case
        n = len(case.data)
        self.max_rows = case.data.count(b"\n") + 1 if max_rows is None else max_rows
        self.text = torch.from_numpy(np.frombuffer(bytearray(case.data), np.uint8)).cuda() if n else None
        self.out = [Guarded(self.max_rows, np.int64 if t == CC.INT64 else np.float64) for _, t in case.columns]
        self.cin = nat.GtfCsvIn(text=self.text.data_ptr() if n else None, n_bytes=n, skip_lines=case.skip,
                                n_fields=case.n_fields, max_rows=self.max_rows, n_columns=len(case.columns),
                                delimiter=ord(","))
        for k, ((f, t), o) in enumerate(zip(case.columns, self.out)):
            self.cin.columns[k] = nat.GtfCsvColumn(f, t, o.p)
        self.nb = int(self.L.gtf_csv_parse_workspace_bytes(n))
        self.ws = Guarded(self.nb, np.uint8)
        self.cnt = nat.GtfCsvCounts(-1, 0, 0, 0, 0, 0)

    def run(self):
        import torch
        rc = self.L.gtf_csv_parse(ctypes.byref(self.cin), ctypes.byref(self.cnt), self.ws.p, ctypes.c_size_t(self.nb), None)
        torch.cuda.synchronize()
        self.ws.get()
        return rc

    def columns(self):
        """the columns trimmed to n_rows, after checking that nothing was written past it"""
        got = []
        for o in self.out:
            a = o.get()
            k = self.cnt.n_rows
            assert 0 <= k <= a.size and np.all(a[k:].view(np.uint8) == FILL), "written past n_rows"
            got.append(a[:k])
        return got


def check_case(case):
    n, cols, error, first = case.rule()
    raw = Raw(case)
    rc = raw.run()
    c = raw.cnt
    assert c.n_rows == n, (c.n_rows, n)
    if error:
        assert rc == -2 and b"exact domain" in raw.L.gtf_last_error()
        assert c.error == error and (c.first_bad_row, c.first_bad_field, c.first_bad_error) == first
        for o in raw.out:
            o.get()          # (the fences)
        return
    assert rc == 0, raw.L.gtf_last_error()
    assert (c.error, c.first_bad_row, c.first_bad_field, c.first_bad_error) == (0, -1, -1, 0)
    got = raw.columns()
    assert len(got) == len(cols)
    for a, b in zip(got, cols):
        assert a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("name", sorted(CC.CASES))
def test_cases_through_the_c_abi(name):
    case = CC.CASES[name]
    check_case(case)
    if case.err:         # the stated error, not only the rule's
        raw = Raw(case)
        raw.run()
        bit, row, field = case.err
        assert raw.cnt.first_bad_error == bit and raw.cnt.first_bad_field == field
        assert row is None or raw.cnt.first_bad_row == row


def test_random_files_through_the_c_abi():
    for seed in range(CC.N_RANDOM):
        check_case(CC.random_file(seed))


def test_more_rows_than_max_rows():
    case = CC.CASES["blank_lines"]            # two rows
    raw = Raw(case, max_rows=1)
    assert raw.run() == -2 and raw.cnt.error == CC.ERR_ROWS
    assert (raw.cnt.n_rows, raw.cnt.first_bad_row, raw.cnt.first_bad_field) == (1, 1, 0)
    got = raw.columns()                       # the one row that fits, nothing past it
    assert got[0].tolist() == [1] and got[1].tolist() == [2.0]


def test_parse_dev_by_header_name():
    data = b",,x,id,x\n0,9,1.5,7,8\n1,9,-2.5,8,8\n"       # two unnamed leading columns, "x" twice: the first one
    for mem in ("torch", "hip"):
        c = csvdev.parse_dev(data, (("id", "int64"), ("x", "float64")), mem=mem)
        assert c.n_rows == 2 and c.mem == mem
        m = c._m
        assert m.host(c["id"], 2, np.int64).tolist() == [7, 8] and m.host(c["x"], 2, np.float64).tolist() == [1.5, -2.5]
    with pytest.raises(KeyError):
        csvdev.parse_dev(data, (("y", "float64"),))
    with pytest.raises(csvdev.OutOfDomain) as e:
        csvdev.parse_dev(b"a,b\n1,2\n3,1234567890123456\n", (("b", "float64"),))
    assert (e.value.row, e.value.field, e.value.bit) == (1, 1, nat.CSV_ERR_DIGITS)
    assert csvdev.parse_dev(b"", (("a", "int64"),)).n_rows == 0


# ------------------------------------------------------------------ the window
def _window(ids, lay, x, y, z, lo, hi):
    import torch
    L = nat.lib()
    n = int(ids.size)
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (ids, lay, x, y, z)]
    vp = lambda t: ctypes.c_void_p(t.data_ptr() if t.numel() else 0)   # noqa: E731
    out = [Guarded(n, dt) for dt in (np.int64, np.int64, np.float64, np.float64, np.float64, np.float64, np.int32,
                                     np.float64, np.float64)]
    win = nat.GtfWindowIn(n_rows=n, lo=lo, hi=hi, node_idx=vp(dev[0]), layer_id=vp(dev[1]), x=vp(dev[2]), y=vp(dev[3]),
                          z=vp(dev[4]))
    nb = int(L.gtf_event_window_workspace_bytes(n))
    ws = Guarded(nb, np.uint8)
    cnt = nat.GtfWindowCounts(-1, -1)
    rc = L.gtf_event_window(ctypes.byref(win), ctypes.byref(nat.GtfWindowOut(*(o.p for o in out))), ctypes.byref(cnt),
                            ws.p, ctypes.c_size_t(nb), None)
    torch.cuda.synchronize()
    assert rc == 0, L.gtf_last_error()
    ws.get()
    got = []
    for o, k in zip(out, [cnt.n_kept] * 6 + [cnt.n_ambiguous] * 3):
        a = o.get()
        assert np.all(a[k:].view(np.uint8) == FILL), "written past the count"
        got.append(a[:k])
    return got, out


@pytest.mark.parametrize("name", sorted(CC.window_cases()))
def test_window_through_the_c_abi(name):
    ids, lay, x, y, z, lo, hi = CC.window_cases()[name]
    got, out = _window(ids, lay, x, y, z, lo, hi)
    e_ids, e_x, e_y, e_z, e_r, e_lay = CC.window_rule(ids, lay, x, y, z, lo, hi)
    for a, b in zip(got[:6], (e_ids, e_lay, e_x, e_y, e_z, e_r)):
        assert a.dtype == b.dtype and np.array_equal(bits(a), bits(b))
    amb = [i for i in range(e_ids.size) if CC.ambiguous(float(e_x[i])) or CC.ambiguous(float(e_y[i]))]
    assert got[6].tolist() == amb
    assert np.array_equal(bits(got[7]), bits(e_x[amb])) and np.array_equal(bits(got[8]), bits(e_y[amb]))
    if name == "ends_inclusive":
        assert e_lay.tolist() == [7000, 7001, 7999, 8000, 7002]
    # the patch: the listed nodes get the given values, nobody else, nothing outside r
    if amb:
        import torch
        val = torch.arange(1, len(amb) + 1, dtype=torch.float64).cuda()
        assert nat.lib().gtf_event_radius_patch(out[5].p, e_ids.size, out[6].p, ctypes.c_void_p(val.data_ptr()), len(amb),
                                                None) == 0
        torch.cuda.synchronize()
        r = out[5].get()[:e_ids.size]
        exp = e_r.copy()
        exp[amb] = np.arange(1, len(amb) + 1)
        assert np.array_equal(bits(r), bits(exp))


# ------------------------------------------------------------------ the fixtures
@pytest.mark.parametrize("kat", sorted(KATS))
def test_readers_equal_the_host_readers(kat):
    pre = os.path.join(GOLDEN, kat, "event_1_filtered_graph_")
    lo, hi = KATS[kat]
    host = gio.read_nodes(pre + "nodes.csv", lo, hi)
    d = gio.read_nodes_dev(pre + "nodes.csv", lo, hi, keep_unpatched=True)
    got = d.host()
    assert d.n == host[0].size > 0
    for a, b, name in zip(got, host, ("ids", "x", "y", "z", "r", "layer_id")):
        assert a.dtype == b.dtype and np.array_equal(bits(a), bits(b)), name
    # where pow and x * x differ the node is on the list, and the patch is what makes r right there
    x, y = host[1], host[2]
    differ = [i for i in range(x.size) if math.pow(x[i], 2.0) != x[i] * x[i] or math.pow(y[i], 2.0) != y[i] * y[i]]
    amb = {i for i in range(x.size) if CC.ambiguous(float(x[i])) or CC.ambiguous(float(y[i]))}
    assert differ and set(differ) <= amb and d.n_ambiguous == len(amb)
    changed = np.nonzero(bits(d.r_unpatched) != bits(host[4]))[0]
    assert changed.size >= 1 and set(changed.tolist()) <= set(differ)
    n2, n1 = gio.read_edges(pre + "edges.csv")
    g2, g1, rows = gio.read_edges_dev(pre + "edges.csv")
    assert rows == n2.size and np.array_equal(g2.cpu().numpy(), n2) and np.array_equal(g1.cpu().numpy(), n1)


def test_edge_ids_written_as_floats_are_out_of_domain():
    with pytest.raises(csvdev.OutOfDomain) as e:
        gio.read_edges_dev(b"2 1\nnode2,node1,weight\n960,13,1.0\n961.0,9,1.0\n")
    assert (e.value.row, e.value.field, e.value.bit) == (1, 0, nat.CSV_ERR_INT_FORM)


@pytest.mark.parametrize("mem", ["torch", "hip"])
def test_build_event_dev_parse_device(mem):
    from gtf import pipeline
    pre = os.path.join(GOLDEN, "kat134", "event_1_filtered_graph_")
    a = pipeline.build_event_dev(pre, 7, 7, mem=mem, parse="host")
    b = pipeline.build_event_dev(pre, 7, 7, mem=mem, parse="device")
    assert a.parse_info == {"nodes": "host", "edges": "host"} and b.parse_info == {"nodes": "device", "edges": "device"}
    (ga, va), (gb, vb) = a.host_graph(), b.host_graph()
    _graphs_equal(gb, ga, "parse=device")
    assert _same(vb, va) and ga.n_nodes == 8748
    with pytest.raises(ValueError, match="parse"):
        pipeline.build_event_dev(pre, 7, 7, parse="gpu")


def test_out_of_domain_file_falls_back_to_the_host_reader(tmp_path):
    from gtf import pipeline
    src = os.path.join(GOLDEN, "kat134", "event_1_filtered_graph_")
    pre = str(tmp_path / "event_1_filtered_graph_")
    shutil.copy(src + "edges.csv", pre + "edges.csv")
    lines = open(src + "nodes.csv", "rb").read().split(b"\n")
    f = lines[101].split(b",")
    f[2] = b"-64.30570000000001"          # 16 digits: outside the device parser's domain, fine for pandas
    lines[101] = b",".join(f)
    open(pre + "nodes.csv", "wb").write(b"\n".join(lines))
    a = pipeline.build_event_dev(pre, 7, 7, parse="host")
    b = pipeline.build_event_dev(pre, 7, 7, parse="device")
    assert b.parse_info["nodes"] == "host" and b.parse_info["edges"] == "device"
    assert "row 100, field 2" in b.parse_info["nodes_reason"] and "more digits" in b.parse_info["nodes_reason"]
    (ga, va), (gb, vb) = a.host_graph(), b.host_graph()
    _graphs_equal(gb, ga, "fallback")
    assert _same(vb, va)


# ------------------------------------------------------------------ the truth files, the CLI
def _truth_dir(tmp_path, extra_columns=False, with_truth=False):
    import pandas as pd
    z = golden()[0]
    tdir = str(tmp_path / "truth")
    os.makedirs(tdir, exist_ok=True)
    cols = ("node_idx", "hit_id", "particle_id", "volume_id", "layer_id", "module_id")
    m = pd.DataFrame({c: z["map__" + c] for c in cols})
    if extra_columns:     # as the reference's mapping files: leading index columns, one without a name
        m.insert(0, "Unnamed: 0.1", np.arange(len(m)))
        m.to_csv(os.path.join(tdir, "event000001000-full-mapping-minCurv-0.3-134.csv"), index=True)
    else:
        m.to_csv(os.path.join(tdir, "event000001000-full-mapping-minCurv-0.3-134.csv"), index=False)
    pd.DataFrame({c: z["particles__" + c] for c in ("particle_id", "px", "py")}).to_csv(
        os.path.join(tdir, "event000001000-particles.csv"), index=False)
    if with_truth:
        m[["hit_id", "particle_id"]].drop_duplicates("hit_id").to_csv(os.path.join(tdir, "event000001000-truth.csv"),
                                                                       index=False)
    return tdir


@pytest.mark.parametrize("extra,with_truth", [(False, False), (True, True)])
def test_truth_files_dev(tmp_path, extra, with_truth):
    from test_gpu_truth import _equal
    host = golden()[3]
    tdir = _truth_dir(tmp_path, extra, with_truth)
    d, info = metrics.truth_files_dev(os.path.join(tdir, "event000001000-"), "full-mapping-minCurv-0.3-134.csv", 7, 7)
    assert info == dict({"particles": "device", "mapping": "device"}, **({"truth": "device"} if with_truth else {}))
    assert (d.n_nodes, d.n_entries, d.n_particles, d.n_reference) == (8748, 13129, 246, 163)
    _equal(d.host(), host)


def test_run_pipeline_resident_parse(tmp_path):
    """--resident-parse --resident-truth writes the files and the metrics.json of --resident-event
    --resident-truth, and says which parser read each file"""
    tdir = _truth_dir(tmp_path)
    outs, texts = [], []
    for flags in (["--resident-event", "--resident-truth"], ["--resident-parse", "--resident-truth"]):
        out = str(tmp_path / ("out%d" % len(outs)))
        r = subprocess.run([sys.executable, CLI, "-n", os.path.join(GOLDEN, "kat134"), "-o", out, "-a", "7", "-z", "7",
                            "--truth", tdir, "--mapping", "full-mapping-minCurv-0.3-134.csv"] + flags,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        outs.append(out)
        texts.append(r.stdout)
    assert "parse" not in texts[0]
    for key in ("nodes", "edges", "particles", "mapping"):
        assert "parse %s: device" % key in texts[1]
    files = sorted(os.path.relpath(os.path.join(r, f), outs[0]) for r, _, fs in os.walk(outs[0]) for f in fs)
    assert files == sorted(os.path.relpath(os.path.join(r, f), outs[1]) for r, _, fs in os.walk(outs[1]) for f in fs)
    assert "metrics.json" in files and sum(f.endswith(".npz") for f in files) >= 1 + 3 * 4
    for f in files:
        a, b = os.path.join(outs[0], f), os.path.join(outs[1], f)
        if f.endswith(".npz"):
            with np.load(a) as za, np.load(b) as zb:
                assert sorted(za.files) == sorted(zb.files), f
                for k in za.files:
                    assert za[k].dtype == zb[k].dtype and np.array_equal(za[k], zb[k], equal_nan=za[k].dtype.kind == "f"), (f, k)
        elif f != "timings.json":
            assert open(a, "rb").read() == open(b, "rb").read(), f
    assert b'"81.595"' in open(os.path.join(outs[1], "metrics.json"), "rb").read()
    r = subprocess.run([sys.executable, CLI, "-o", str(tmp_path / "x"), "--resident-parse", "--start", "2"],
                       capture_output=True, text=True)
    assert r.returncode == 2 and "only with --start 1" in r.stderr
