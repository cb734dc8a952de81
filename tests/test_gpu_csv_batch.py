"""The CSV front end of a batch in one call (gtf_csv_parse_ev, gtf_event_window_ev; csvdev.parse_batch_dev,
io.read_nodes_batch_dev / read_edges_batch_dev, DeviceGraph.from_fused, pipeline.build_events_dev(batch_parse=True),
metrics.truth_files_batch_dev(batch_parse=True), run_pipeline.py --batch-parse) against what it replaces:
the single-file calls, one per file, their results laid end to end. Every comparison is of bit patterns.

  * every batch of tests/csv_batch_cases.py and five seeded random ones through the C-ABI, under both
    allocators, the text's padding filled with digits, commas, quotes and line ends, every output and the
    workspace between guard bytes: the columns against K gtf_csv_parse calls, row_off, the K counts, the
    first bad file in the message; nothing written past the last row;
  * the host refusals write nothing;
  * gtf_event_window_ev against gtf_event_window per event: the kept columns, n_kept per event, the
    ambiguous list rebased;
  * build_events_dev(parse="device", batch_parse=True) equals parse="host" graph for graph, with an event that
    keeps no node but has edge rows, with a nodes.csv outside the exact domain and with headers that differ;
  * truth_files_batch_dev(batch_parse=True) equals batch_parse=False word for word and scores 133 / 163; the CLI."""
import ctypes
import functools
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import csv_batch_cases as BC
import csv_cases as CC
from fixtures import GOLDEN
from guard_mem import FILL, Mem, at
from gtf import _native as nat
from gtf import csvdev, metrics
from gtf import io as gio

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "gnn-track-finding_amd", "run_pipeline.py")
VOL7 = os.path.join(GOLDEN, "kat134", "event_1_filtered_graph_")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else a.dtype)


def dtype_of(t):
    return np.int64 if t == CC.INT64 else np.float64


# ------------------------------------------------------------------ 1. the parse through the C-ABI
@functools.lru_cache(maxsize=None)
def _single(data, columns, n_fields, skip):
    """gtf_csv_parse on one file alone -> parse_rule's tuple (n_rows, columns or None, error, first)"""
    import torch
    L = nat.lib()
    n, max_rows = len(data), data.count(b"\n") + 1
    text = torch.from_numpy(np.frombuffer(bytearray(data), np.uint8)).cuda() if n else None
    out = [torch.empty(max_rows, dtype=torch.int64 if t == CC.INT64 else torch.float64, device="cuda") for _, t in columns]
    cin = nat.GtfCsvIn(text=text.data_ptr() if n else None, n_bytes=n, skip_lines=skip, n_fields=n_fields,
                       max_rows=max_rows, n_columns=len(columns), delimiter=ord(","))
    for k, ((f, t), o) in enumerate(zip(columns, out)):
        cin.columns[k] = nat.GtfCsvColumn(f, t, o.data_ptr())
    nb = int(L.gtf_csv_parse_workspace_bytes(n))
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    cnt = nat.GtfCsvCounts()
    rc = L.gtf_csv_parse(ctypes.byref(cin), ctypes.byref(cnt), ws.data_ptr(), ctypes.c_size_t(nb),
                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    if cnt.error:
        assert rc == -2
        return cnt.n_rows, None, cnt.error, (cnt.first_bad_row, cnt.first_bad_field, cnt.first_bad_error)
    assert rc == 0, L.gtf_last_error()
    return cnt.n_rows, [o[:cnt.n_rows].cpu().numpy() for o in out], 0, None


@functools.lru_cache(maxsize=None)
def _expected(name):
    """K single calls laid end to end (computed once, shared by both allocators)"""
    b = BC.BATCHES[name] if isinstance(name, str) else BC.random_batch(name)
    per = [_single(f, tuple(b.columns), b.n_fields, b.skip) for f in b.files]
    return b, per, BC.assemble(per, b.columns, b.bound())


def _abi(b, mem, tamper=None, ws_short=0, with_row_off=True, fill=BC.GARBAGE):
    """gtf_csv_parse_ev on raw buffers -> (status, columns at max_rows, row_off, counts)"""
    L, m, K = nat.lib(), Mem(mem), b.K
    buf, table = b.layout(fill=fill)
    max_rows = b.bound()
    text = m.up(np.frombuffer(bytearray(buf) if buf else bytearray(1), np.uint8))
    out = [m.guarded(8 * max_rows) for _ in b.columns]
    off = m.guarded(4 * (K + 1))
    tab = (nat.GtfCsvFile * max(K, 1))(*[nat.GtfCsvFile(s, n) for s, n in table])
    cin = nat.GtfCsvInEv(text=text.data_ptr(), files=ctypes.cast(tab, ctypes.c_void_p), n_files=K, skip_lines=b.skip,
                         n_fields=b.n_fields, max_rows=max_rows, n_columns=len(b.columns), delimiter=ord(","),
                         row_off=at(off) if with_row_off else None)
    for k, ((f, t), o) in enumerate(zip(b.columns, out)):
        cin.columns[k] = nat.GtfCsvColumn(f, t, at(o))
    nb = int(L.gtf_csv_parse_ev_workspace_bytes(len(buf), K))
    assert nb > 0
    ws = m.guarded(nb)
    cnt = (nat.GtfCsvCounts * max(K, 1))(*[nat.GtfCsvCounts(-7, 7, 7, 7, 7, 7) for _ in range(max(K, 1))])
    if tamper:
        tamper(cin, tab)
    rc = L.gtf_csv_parse_ev(ctypes.byref(cin), cnt, at(ws), ctypes.c_size_t(nb - ws_short), m.stream)
    cols = [m.payload(o, 8 * max_rows, dtype_of(t)) for o, (_, t) in zip(out, b.columns)]
    m.payload(ws, nb, np.uint8)
    return rc, cols, m.payload(off, 4 * (K + 1), np.int32), cnt


def _check(name, mem):
    b, per, (cut, counts, cols, exact) = _expected(name)
    rc, got, off, cnt = _abi(b, mem)
    L = nat.lib()
    bad = [e for e, c in enumerate(counts) if c[1]]
    if bad:
        assert rc == -2 and (b"file %d: " % bad[0]) in L.gtf_last_error(), L.gtf_last_error()
    else:
        assert rc == 0, L.gtf_last_error()
    for e, (n, error, first) in enumerate(counts):
        c = cnt[e]
        assert (c.n_rows, c.error) == (n, error), (e, c.n_rows, c.error, n, error)
        assert (c.first_bad_row, c.first_bad_field, c.first_bad_error) == (first or (-1, -1, 0)), e
    if any(len(f) for f in b.files):          # (no byte at all: the offsets are zeroed, nothing else happens)
        assert off.tolist() == np.concatenate([[0], np.cumsum([p[0] for p in per])]).tolist()
    else:
        assert not off.any()
    total = int(cut[-1])
    for a, x in zip(got, cols):
        assert a.dtype == x.dtype and np.array_equal(bits(a[:total])[exact], bits(x)[exact])
        assert bool((a[total:].view(np.uint8) == FILL).all()), "written past the last row"


@pytest.mark.parametrize("mem", ["torch", "hip"])
@pytest.mark.parametrize("name", sorted(BC.BATCHES))
def test_batches_through_the_c_abi(name, mem):
    _check(name, mem)


@pytest.mark.parametrize("mem", ["torch", "hip"])
def test_random_batches_through_the_c_abi(mem):
    for seed in range(BC.N_RANDOM):
        _check(seed, mem)


def test_single_calls_are_the_rule():
    """the reference of this file is the definition of tests/csv_batch_cases.py"""
    for name in ("bad_file_2_of_4", "two_bad_files", "fewer_lines_than_skip_between", "no_newline_before_garbage",
                 "max_rows_runs_out_in_file_1", "65_one_row_files"):
        b, per, (cut, counts, cols, exact) = _expected(name)
        d_cut, d_counts, d_cols, d_exact = b.definition()
        assert cut.tolist() == d_cut.tolist() and counts == d_counts and exact.tolist() == d_exact.tolist()
        for x, y in zip(cols, d_cols):
            assert np.array_equal(bits(x)[exact], bits(y)[exact])


def test_row_off_is_optional_and_padding_is_dont_care():
    b = BC.BATCHES["ends_one_short_of_chunk_boundary"]
    total = int(_expected("ends_one_short_of_chunk_boundary")[2][0][-1])
    rc, got, off, cnt = _abi(b, "torch", with_row_off=False)
    assert rc == 0 and bool((off.view(np.uint8) == FILL).all())
    for fill in (b"\n", b"\0", b'"', b"1", b"\r"):
        assert fill in b.layout(fill=fill)[0][4095:4097]
        rc, got2, off2, _ = _abi(b, "torch", fill=fill)
        assert rc == 0 and off2[-1] == total
        for x, y in zip(got, got2):
            assert np.array_equal(bits(x), bits(y))


def test_host_refusals_write_nothing():
    b = BC.BATCHES["bad_file_2_of_4"]
    L = nat.lib()
    C = CC.chunk()

    def refused(text, tamper=None, ws_short=0, status=-2):
        rc, got, off, cnt = _abi(b, "torch", tamper, ws_short)
        assert rc == status and text in L.gtf_last_error(), (rc, L.gtf_last_error())
        assert all(bool((a.view(np.uint8) == FILL).all()) for a in got) and bool((off.view(np.uint8) == FILL).all())

    def field(name, value):
        def tamper(cin, tab):
            setattr(cin, name, value)
        return tamper

    def entry(e, start=None, n_bytes=None):
        def tamper(cin, tab):
            if start is not None:
                tab[e].start = start
            if n_bytes is not None:
                tab[e].n_bytes = n_bytes
        return tamper

    refused(b"workspace", ws_short=1)
    refused(b"file 1 does not start on a multiple", entry(1, start=C + 16))
    refused(b"file 1 does not start on a multiple", entry(1, start=-C))
    refused(b"file 2 starts before the end", entry(2, start=C))             # overlapping: file 1 is there
    refused(b"file 2 starts before the end", entry(2, start=0))             # descending
    refused(b"file 1 starts before the end", entry(0, n_bytes=C + 1))       # file 0 grows into file 1's chunk
    refused(b"file 3 has a negative size", entry(3, n_bytes=-1))
    refused(b"null files", field("files", None))
    refused(b"negative sizes", field("n_files", -1))
    refused(b"negative sizes", field("max_rows", -1))
    refused(b"n_fields", field("n_fields", 65))
    refused(b"delimiter", field("delimiter", ord("5")))
    refused(b"2^31", entry(3, start=(2 ** 31 // C - 1) * C))
    refused(b"ABI mismatch", field("abi_version", nat.ABI_VERSION + 1), status=-3)

    def twice(cin, tab):
        cin.columns[1].field = cin.columns[0].field
    refused(b"requested twice", twice)

    def misaligned(cin, tab):
        cin.row_off = ctypes.c_void_p(cin.row_off + 2)
    refused(b"row_off", misaligned)
    rc = L.gtf_csv_parse_ev(ctypes.byref(nat.GtfCsvInEv(n_fields=1, delimiter=ord(","))), None, None, 0, None)
    assert rc == 0                                                           # K = 0: nothing to do, nothing needed
    assert int(L.gtf_csv_parse_ev_workspace_bytes(0, 0)) > 0
    assert int(L.gtf_csv_parse_ev_workspace_bytes(10 * C, 3)) <= int(L.gtf_csv_parse_ev_workspace_bytes(11 * C, 4))


# ------------------------------------------------------------------ 2. the window of a batch
def _columns(layers, rng):
    n = len(layers)
    return (np.arange(100, 100 + n, dtype=np.int64), np.array(layers, np.int64), rng.normal(0, 300, n),
            rng.normal(0, 300, n), rng.normal(0, 1000, n))


def window_batches():
    """name -> (events: [(ids, layer, x, y, z)], lo, hi)"""
    rng = np.random.default_rng(11)
    cases = CC.window_cases()
    ev = lambda name: cases[name][:5]   # noqa: E731
    keep, drop = 7002, 9500
    out = {"nothing_kept_in_the_middle": ([ev("ends_inclusive"), ev("none_kept"), ev("all_kept")], 7000, 8000),
           "all_rows_kept": ([ev("all_kept"), ev("all_kept")], 7000, 8000),
           "no_rows_events": ([ev("no_rows"), ev("many_blocks"), ev("no_rows"), ev("zeros_and_extremes"), ev("no_rows")],
                              7000, 9000),
           "one_event": ([ev("many_blocks")], 7000, 9000),
           "no_events": ([], 7000, 8000),
           "only_empty_events": ([ev("no_rows")] * 3, 7000, 8000)}
    for n in (255, 256, 257):       # an event boundary at a block boundary of the scan, one short of it, one past it
        layers = [keep if i % 3 else drop for i in range(n)]
        out["boundary_at_row_%d" % n] = ([_columns(layers, rng), _columns([keep] * 300, rng), _columns(layers[::-1], rng)],
                                         7000, 8000)
    return out


def _window_single(ids, lay, x, y, z, lo, hi):
    from test_gpu_csv import _window
    got, _ = _window(ids, lay, x, y, z, lo, hi)
    return got


def _window_ev(events, lo, hi, mem):
    L, m, K = nat.lib(), Mem(mem), len(events)
    row_off = np.concatenate([[0], np.cumsum([e[0].size for e in events])]).astype(np.int32)
    n = int(row_off[-1])
    cat = [np.concatenate([e[i] for e in events] + [np.zeros(1, events[0][i].dtype if K else np.int64)]) for i in range(5)]
    dev = [m.up(a) for a in cat]
    dts = (np.int64, np.int64, np.float64, np.float64, np.float64, np.float64, np.int32, np.float64, np.float64)
    out = [m.guarded(max(n, 1) * np.dtype(dt).itemsize) for dt in dts]
    win = nat.GtfWindowIn(n_rows=n, lo=lo, hi=hi, node_idx=dev[0].data_ptr(), layer_id=dev[1].data_ptr(),
                          x=dev[2].data_ptr(), y=dev[3].data_ptr(), z=dev[4].data_ptr())
    nb = int(L.gtf_event_window_ev_workspace_bytes(n, K))
    ws = m.guarded(nb)
    cnt = nat.GtfWindowCounts(-1, -1)
    kept = np.full(K + 1, -5, np.int32)
    rc = L.gtf_event_window_ev(ctypes.byref(win), row_off.ctypes.data, K, ctypes.byref(nat.GtfWindowOut(*(at(o) for o in out))),
                               kept.ctypes.data, ctypes.byref(cnt), at(ws), ctypes.c_size_t(nb), m.stream)
    assert rc == 0, L.gtf_last_error()
    assert kept[K] == -5
    m.payload(ws, nb, np.uint8)
    got = []
    for o, dt, k in zip(out, dts, [cnt.n_kept] * 6 + [cnt.n_ambiguous] * 3):
        a = m.payload(o, max(n, 1) * np.dtype(dt).itemsize, dt)
        assert bool((a[k:].view(np.uint8) == FILL).all()), "written past the count"
        got.append(a[:k])
    return got, kept[:K].tolist(), cnt


@pytest.mark.parametrize("mem", ["torch", "hip"])
@pytest.mark.parametrize("name", sorted(window_batches()))
def test_window_of_a_batch_equals_the_windows_of_its_events(name, mem):
    events, lo, hi = window_batches()[name]
    got, kept, cnt = _window_ev(events, lo, hi, mem)
    singles = [_window_single(*e, lo, hi) for e in events]
    assert kept == [s[0].size for s in singles] and cnt.n_kept == sum(kept)
    base = np.concatenate([[0], np.cumsum(kept)]).astype(np.int64)
    for i in range(6):
        exp = np.concatenate([s[i] for s in singles]) if singles else np.zeros(0, got[i].dtype)
        assert got[i].dtype == exp.dtype and np.array_equal(bits(got[i]), bits(exp)), i
    amb = np.concatenate([s[6].astype(np.int64) + base[e] for e, s in enumerate(singles)]) if singles else np.zeros(0)
    assert got[6].tolist() == amb.tolist() and cnt.n_ambiguous == amb.size     # positions among the batch's kept rows
    for i in (7, 8):
        exp = np.concatenate([s[i] for s in singles]) if singles else np.zeros(0)
        assert np.array_equal(bits(got[i]), bits(exp))
    if name == "nothing_kept_in_the_middle":
        assert kept[1] == 0 and kept[0] == 5 and kept[2] == 700
    if name == "all_rows_kept":
        assert kept == [700, 700]
    if name.startswith("boundary_at_row_"):
        rule = [CC.window_rule(*e, lo, hi)[0].size for e in events]
        assert kept == rule and kept[1] == 300


def test_window_ev_refusals():
    L = nat.lib()
    import torch
    n = 4
    cols = [torch.zeros(n, dtype=torch.int64 if i < 2 else torch.float64, device="cuda") for i in range(5)]
    out = [torch.zeros(n, dtype=torch.float64, device="cuda") for _ in range(9)]
    win = nat.GtfWindowIn(n_rows=n, lo=0, hi=1, node_idx=cols[0].data_ptr(), layer_id=cols[1].data_ptr(),
                          x=cols[2].data_ptr(), y=cols[3].data_ptr(), z=cols[4].data_ptr())
    wout = nat.GtfWindowOut(*(o.data_ptr() for o in out))
    nb = int(L.gtf_event_window_ev_workspace_bytes(n, 2))
    ws = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    kept = np.zeros(2, np.int32)
    cnt = nat.GtfWindowCounts()

    def call(off, K=2, kept_p=kept.ctypes.data, size=nb):
        off = np.asarray(off, np.int32)
        return L.gtf_event_window_ev(ctypes.byref(win), off.ctypes.data if off.size else None, K, ctypes.byref(wout), kept_p,
                                     ctypes.byref(cnt), ws.data_ptr(), ctypes.c_size_t(size), None)

    assert call([0, 2, 4]) == 0
    for off, text in (([1, 2, 4], b"from 0 to n_rows"), ([0, 2, 3], b"from 0 to n_rows"), ([0, 5, 4], b"decreases")):
        assert call(off) == -2 and text in L.gtf_last_error()
    assert call([], 2) == -2 and b"null row_off" in L.gtf_last_error()
    assert call([0, 2, 4], -1) == -2 and b"negative n_events" in L.gtf_last_error()
    assert call([0, 2, 4], kept_p=None) == -2 and b"n_kept" in L.gtf_last_error()
    assert call([0, 2, 4], size=nb - 1) == -2 and b"gtf_event_window_ev_workspace_bytes" in L.gtf_last_error()
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 3. the binding, the readers
@pytest.mark.parametrize("mem", ["torch", "hip"])
def test_parse_batch_dev(mem, tmp_path):
    cols = (("id", "int64"), ("x", "float64"))
    files = [b"id,x\n1,2.5\n2,3.5", b"", b"id,x\n", b"id,x\r\n3,4.5\r\n"]
    path = str(tmp_path / "f.csv")
    open(path, "wb").write(files[3])
    c = csvdev.parse_batch_dev(files[:3] + [path], cols, mem=mem)
    m = c._m
    assert c.info == {"mode": "batch"} and c.row_off.tolist() == [0, 2, 2, 2, 3] and c.n_rows == 3 and c.mem == mem
    assert m.host(c["id"], 3, np.int64).tolist() == [1, 2, 3] and m.host(c["x"], 3, np.float64).tolist() == [2.5, 3.5, 4.5]
    # another header layout: every file alone, the same columns
    d = csvdev.parse_batch_dev(files[:3] + [b"x,id\n4.5,3\n"], cols, mem=mem)
    assert d.info["mode"] == "per-file" and d.info["file"] == 3 and "file 3" in d.info["reason"]
    assert d.row_off.tolist() == [0, 2, 2, 2, 3] and d.files == ["device"] * 4
    assert m.host(d["id"], 3, np.int64).tolist() == [1, 2, 3] and m.host(d["x"], 3, np.float64).tolist() == [2.5, 3.5, 4.5]
    # a field outside the domain: OutOfDomain, or the host reader for that file alone
    bad = files[:1] + [b"id,x\n7,1234567890123456\n"] + files[3:]
    with pytest.raises(csvdev.OutOfDomain) as e:
        csvdev.parse_batch_dev(bad, cols, mem=mem)
    assert (e.value.row, e.value.field, e.value.bit) == (0, 1, nat.CSV_ERR_DIGITS)
    d = csvdev.parse_batch_dev(bad, cols, mem=mem, host_reader=lambda f: ([7], [1234567890123456.0]))
    assert d.info["mode"] == "per-file" and d.info["file"] == 1 and "row 0, field 1" in d.info["reason"]
    assert d.files == ["device", "host", "device"] and "more digits" in d.reasons[1] and d.row_off.tolist() == [0, 2, 3, 4]
    assert m.host(d["x"], 4, np.float64).tolist() == [2.5, 3.5, 1234567890123456.0, 4.5]
    for empty in ([], [b"", b""]):
        z = csvdev.parse_batch_dev(empty, cols, mem=mem)
        assert z.n_rows == 0 and z.row_off.tolist() == [0] * (len(empty) + 1) and z.info == {"mode": "batch"}


def test_batch_readers_equal_the_single_readers():
    k800 = os.path.join(GOLDEN, "kat800", "event_1_filtered_graph_")
    files = [VOL7, k800, VOL7]
    d = gio.read_nodes_batch_dev([f + "nodes.csv" for f in files], 7, 9, keep_unpatched=True)
    singles = [gio.read_nodes(f + "nodes.csv", 7, 9) for f in files]
    assert d.parse == {"mode": "batch"} and d.files == ["device"] * 3
    assert d.node_off.tolist() == np.concatenate([[0], np.cumsum([s[0].size for s in singles])]).tolist() and d.n == d.node_off[-1]
    for a, i, what in zip(d.host(), range(6), ("ids", "x", "y", "z", "r", "layer_id")):
        exp = np.concatenate([s[i] for s in singles])
        assert a.dtype == exp.dtype and np.array_equal(bits(a), bits(exp)), what
    assert d.n_ambiguous > 0 and (bits(d.r_unpatched) != bits(d.host()[4])).any()        # the one patch did its work
    n2, n1, row_off, c = gio.read_edges_batch_dev([f + "edges.csv" for f in files])
    es = [gio.read_edges(f + "edges.csv") for f in files]
    assert row_off.tolist() == np.concatenate([[0], np.cumsum([e[0].size for e in es])]).tolist() and c.info == {"mode": "batch"}
    assert np.array_equal(n2.cpu().numpy(), np.concatenate([e[0] for e in es]))
    assert np.array_equal(n1.cpu().numpy(), np.concatenate([e[1] for e in es]))


# ------------------------------------------------------------------ 4. the graph builds
def _write_event(d, ids, layer, x, y, z, a, b, header="node_idx,layer_id,x,y,z"):
    order = {"node_idx": ids, "layer_id": layer, "x": x, "y": y, "z": z}
    names = header.split(",")
    with open(os.path.join(d, "event_1_filtered_graph_nodes.csv"), "w") as f:
        f.write(header + "\n")
        for k in range(ids.size):
            f.write(",".join(repr(float(order[c][k])) if c in "xyz" else "%d" % order[c][k] for c in names) + "\n")
    with open(os.path.join(d, "event_1_filtered_graph_edges.csv"), "w") as f:
        f.write("%d %d\nnode2,node1,weight\n" % (ids.size, a.size))
        for k in range(a.size):
            f.write("%d,%d,1.0\n" % (b[k], a[k]))
    return os.path.join(d, "event_1_filtered_graph_")


@pytest.fixture(scope="module")
def prefixes(tmp_path_factory):
    """vol-7; the 257-node event; an event with an empty window; an event outside the window that has edge rows"""
    import batch_cases as bc
    out = {"vol7": VOL7}
    for name, spec in (("257", ("hand", "perm257")), ("empty", ("empty",))):
        ids, x, y, z, r, layer, a, b = bc.columns(spec)
        out[name] = _write_event(str(tmp_path_factory.mktemp(name)), ids, layer, x, y, z, a, b)
    ids, x, y, z, r, layer, a, b = bc.columns(("hand", "perm257"))
    out["outside"] = _write_event(str(tmp_path_factory.mktemp("outside")), ids, np.full(ids.size, 12001), x, y, z, a, b)
    out["reordered"] = _write_event(str(tmp_path_factory.mktemp("reordered")), ids, layer, x, y, z, a, b,
                                    header="layer_id,node_idx,z,y,x")
    return out


def _same_graph(got, exp, what):
    from test_gpu_event_pack import _graphs_equal, _same
    (ga, va), (gb, vb) = exp.host_graph(), got.host_graph()
    _graphs_equal(gb, ga, what)
    assert _same(vb, va), what
    assert got.n_events == exp.n_events and got.event_nodes == exp.event_nodes
    assert np.array_equal(got._np(got.carried["event"]), exp._np(exp.carried["event"]))


@pytest.mark.parametrize("mem", ["torch", "hip"])
def test_build_events_dev_batch_parse_equals_parse_host(prefixes, mem):
    from gtf import pipeline
    pre = [prefixes[k] for k in ("vol7", "257", "empty", "vol7")]
    a = pipeline.build_events_dev(pre, 7, 9, mem=mem, parse="host")
    b = pipeline.build_events_dev(pre, 7, 9, mem=mem, parse="device", batch_parse=True)
    assert [(i["nodes"], i["edges"]) for i in b.parse_info] == [("device", "device")] * 4
    assert b.parse_info[0]["batch"] == {"nodes": {"mode": "batch"}, "edges": {"mode": "batch"}}
    assert a.event_nodes == [8748, 257, 0, 8748]
    _same_graph(b, a, "batch_parse")
    with pytest.raises(ValueError, match="parse='device'"):
        pipeline.build_events_dev(pre, 7, 8, parse="host", batch_parse=True)


def test_an_event_that_keeps_no_node_but_has_edge_rows(prefixes):
    """from_events drops such an event's rows; from_fused leaves them in the row columns and the builder drops
    them: the same graph, byte for byte, wherever the event stands"""
    from gtf import pipeline
    for keys in (("257", "outside", "vol7"), ("outside", "257"), ("257", "outside"), ("outside",)):
        pre = [prefixes[k] for k in keys]
        a = pipeline.build_events_dev(pre, 7, 8, parse="host")
        b = pipeline.build_events_dev(pre, 7, 8, parse="device", batch_parse=True)
        assert a.event_nodes[keys.index("outside")] == 0
        _same_graph(b, a, keys)


def test_out_of_domain_nodes_file_falls_back(prefixes, tmp_path):
    from gtf import pipeline
    pre = str(tmp_path / "event_1_filtered_graph_")
    shutil.copy(VOL7 + "edges.csv", pre + "edges.csv")
    lines = open(VOL7 + "nodes.csv", "rb").read().split(b"\n")
    f = lines[101].split(b",")
    f[2] = b"-64.30570000000001"          # 16 digits: outside the device parser's domain, fine for pandas
    lines[101] = b",".join(f)
    open(pre + "nodes.csv", "wb").write(b"\n".join(lines))
    batch = [prefixes["257"], pre, prefixes["vol7"]]
    a = pipeline.build_events_dev(batch, 7, 8, parse="host")
    b = pipeline.build_events_dev(batch, 7, 8, parse="device", batch_parse=True)
    assert [i["nodes"] for i in b.parse_info] == ["device", "host", "device"] and [i["edges"] for i in b.parse_info] == ["device"] * 3
    assert "row 100, field 2" in b.parse_info[1]["nodes_reason"] and "more digits" in b.parse_info[1]["nodes_reason"]
    info = b.parse_info[0]["batch"]
    assert info["nodes"]["mode"] == "per-file" and info["nodes"]["file"] == 1 and info["edges"] == {"mode": "batch"}
    _same_graph(b, a, "fallback")


def test_headers_that_differ_fall_back(prefixes):
    from gtf import pipeline
    batch = [prefixes["257"], prefixes["reordered"], prefixes["vol7"]]
    a = pipeline.build_events_dev(batch, 7, 8, parse="host")
    b = pipeline.build_events_dev(batch, 7, 8, parse="device", batch_parse=True)
    info = b.parse_info[0]["batch"]["nodes"]
    assert info["mode"] == "per-file" and info["file"] == 1 and "file 1 resolves" in info["reason"]
    assert [i["nodes"] for i in b.parse_info] == ["device"] * 3
    _same_graph(b, a, "headers")


def test_from_fused_refusals():
    import torch
    from gtf.device import DeviceGraph
    z = lambda n, dt: torch.zeros(n, dtype=dt, device="cuda")   # noqa: E731
    cols = [z(2, torch.int64)] + [z(2, torch.float64)] * 4 + [z(2, torch.int64)] + [z(1, torch.int64)] * 2
    for node_off, row_off, text in (([0, 1], [0, 1], "node_off"), ([0, 2], [0, 2], "row_off"), ([0, 2, 1, 2], [0, 0, 0, 1], "node_off"),
                                    ([0, 2], [0, 0, 1], "one entry per event")):
        with pytest.raises(ValueError, match=text):
            DeviceGraph.from_fused(cols, node_off, row_off)
    with pytest.raises(ValueError, match="eight columns"):
        DeviceGraph.from_fused(cols[:7], [0, 2], [0, 1])


# ------------------------------------------------------------------ 5. the truth files, the CLI
@pytest.fixture(scope="module")
def truth_dirs(tmp_path_factory):
    """the vol-7 truth files without and with a truth.csv"""
    from test_gpu_csv import _truth_dir
    return _truth_dir(tmp_path_factory.mktemp("plain")), _truth_dir(tmp_path_factory.mktemp("full"), True, True)


@pytest.mark.parametrize("mem", ["torch", "hip"])
def test_truth_files_batch_parse_equals_per_file(truth_dirs, mem):
    from test_truth_batch_cases import batches_equal
    plain, full = (os.path.join(t, "event000001000-") for t in truth_dirs)
    name = "full-mapping-minCurv-0.3-134.csv"
    for pres in ([plain, None, full, plain], [full, full], [None, plain], [None, None], []):
        a, ia = metrics.truth_files_batch_dev(pres, name, 7, 7, mem=mem)
        b, ib = metrics.truth_files_batch_dev(pres, name, 7, 7, mem=mem, batch_parse=True)
        assert ia == ib and b.mem == mem
        batches_equal(b.host(), a.host())
        assert list(b.scored) == list(a.scored) and b.n_reference == a.n_reference
        if any(pres):
            assert b.parse_info["particles"] == {"mode": "batch"} and ("truth" in b.parse_info) == (full in pres)
            if plain in pres and full in pres:      # the mapping with leading index columns is another layout: per file
                info = b.parse_info["mapping"]
                assert info["mode"] == "per-file" and info["file"] == 1 and "[2, 3, 4, 5, 6, 7] of 8" in info["reason"]
            else:
                assert b.parse_info["mapping"] == {"mode": "batch"}


def test_batch_scorer_on_batch_parsed_tables(truth_dirs):
    import torch
    from test_gpu_score import _csr, _golden_cands
    plain, full = (os.path.join(t, "event000001000-") for t in truth_dirs)
    d, _ = metrics.truth_files_batch_dev([plain, None, full], "full-mapping-minCurv-0.3-134.csv", 7, 7, batch_parse=True)
    cands = _golden_cands("cumulative")
    ptr, ids = _csr(cands + cands)
    n = len(cands)
    s = metrics.BatchScorer(d)
    s.add(torch.from_numpy(ptr).cuda(), torch.from_numpy(ids).cuda(), torch.from_numpy(np.array([0, n, n, 2 * n], np.int32)).cuda(),
          2 * n, 0, per_candidate=True)
    res = s.results()
    assert res[1] is None
    for e in (0, 2):
        assert (res[e].n_reconstructed, res[e].n_reference) == (133, 163)


def test_run_pipeline_batch_parse(tmp_path, truth_dirs, prefixes):
    """--batch ... --batch-build --resident-parse --batch-metrics --batch-truth writes the same files with and
    without --batch-parse, metrics.json included, byte for byte"""
    ev = os.path.join(GOLDEN, "kat134")
    common = ["-a", "7", "-z", "8", "--truth", truth_dirs[0], "--mapping", "full-mapping-minCurv-0.3-134.csv",
              "--batch-build", "--resident-parse", "--batch-metrics", "--batch-truth"]
    outs, texts = [], []
    for flags in ([], ["--batch-parse"]):
        out = str(tmp_path / ("out%d" % len(outs)))
        r = subprocess.run([sys.executable, CLI, "--batch", ev, os.path.dirname(prefixes["257"]), "-o", out] + common + flags,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        outs.append(out)
        texts.append(r.stdout)
    assert [ln for ln in texts[0].splitlines() if "parse " in ln] == [ln for ln in texts[1].splitlines() if "parse " in ln]
    files = sorted(os.path.relpath(os.path.join(r, f), outs[0]) for r, _, fs in os.walk(outs[0]) for f in fs)
    assert files == sorted(os.path.relpath(os.path.join(r, f), outs[1]) for r, _, fs in os.walk(outs[1]) for f in fs)
    assert sum(f.endswith("metrics.json") for f in files) == 2 and sum(f.endswith(".npz") for f in files) >= 2 * 5
    for f in files:
        a, b = os.path.join(outs[0], f), os.path.join(outs[1], f)
        if f.endswith(".npz"):
            with np.load(a) as za, np.load(b) as zb:
                assert sorted(za.files) == sorted(zb.files), f
                for k in za.files:
                    assert za[k].dtype == zb[k].dtype and za[k].shape == zb[k].shape and \
                        za[k].tobytes() == zb[k].tobytes(), (f, k)
        elif not f.endswith("timings.json"):
            assert open(a, "rb").read() == open(b, "rb").read(), f
    assert b'"81.595"' in open(os.path.join(outs[1], "0", "metrics.json"), "rb").read()
    r = subprocess.run([sys.executable, CLI, "--batch", ev, "-o", str(tmp_path / "x"), "--batch-build", "--batch-parse"],
                       capture_output=True, text=True)
    assert r.returncode == 2 and "--resident-parse" in r.stderr
