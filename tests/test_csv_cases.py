"""The pure-Python statement of gtf_csv_parse's rules (tests/csv_cases.py) against the host readers it
has to reproduce, without a GPU: pandas.read_csv and np.loadtxt bit for bit on every in-domain case,
on 20 seeded random files and on the two fixtures; every error case rejected where it is stated; the
ctypes mirrors of the new structs against the header; and the band of gtf_event_window around the
rounding midpoints: on kat134 and kat800 every x or y whose math.pow(v, 2.0) differs from v * v
lies inside it.

Measured (glibc 2.35): pow(v, 2) differs from v * v for 61 of the 76,676 x / y values of kat134 and
kat800 together; the largest distance of such a square from its rounding midpoint is 0.00352 ulp,
against the band's 0.0625; the band itself takes 9,612 of the values (12.5 %) and 23-24 % of the nodes
(2,046 of kat134's 8,748; 2,967 of the 12,361 of kat800's volumes 7-9)."""
import ctypes
import io as pyio
import math
import os
import subprocess
import tempfile

import numpy as np
import pandas as pd
import pytest

import csv_cases as CC
from fixtures import GOLDEN
from gtf import _native as nat
from gtf import csvdev
from gtf import io as gio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "gtf.h")
GOOD = sorted(n for n, c in CC.CASES.items() if not c.err)
BAD = sorted(n for n, c in CC.CASES.items() if c.err)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else a.dtype)


def host_columns(case):
    """the case's columns as the host readers give them: pandas for one header line (the dtype of a
    column forced, as an all-integer float column would be read as int64 and lose the sign of -0),
    np.loadtxt as io.read_edges for two"""
    dts = [np.int64 if t == CC.INT64 else np.float64 for _, t in case.columns]
    if case.loadtxt:
        f = pyio.BytesIO(case.data)
        for _ in range(case.skip):
            f.readline()
        e = np.loadtxt(f, delimiter=",", dtype=np.float64, ndmin=2)
        return [e[:, c].astype(dt) for (c, _), dt in zip(case.columns, dts)]
    try:
        a = pd.read_csv(pyio.BytesIO(case.data), dtype={c: dt for (c, _), dt in zip(case.columns, dts)}, header=0)
    except pd.errors.EmptyDataError:
        return [np.zeros(0, dt) for dt in dts]
    return [a.iloc[:, c].to_numpy(dt) for (c, _), dt in zip(case.columns, dts)]


def check_against_host(case):
    n, cols, error, first = case.rule()
    assert error == 0 and first is None
    host = host_columns(case)
    assert len(cols) == len(host)
    for a, b in zip(cols, host):
        assert a.dtype == b.dtype and a.size == b.size == n
        assert np.array_equal(bits(a), bits(b))
    return cols


@pytest.mark.parametrize("name", GOOD)
def test_rule_is_the_host_readers(name):
    case = CC.CASES[name]
    cols = check_against_host(case)
    if case.cols is not None:   # ... and what the case states by hand
        for a, b in zip(cols, case.cols):
            assert np.array_equal(bits(a), bits(np.array(b, a.dtype)))


def test_zero_mantissa_with_a_large_exponent_through_read_nodes():
    """pandas reads such a column as text; io.read_nodes' to_numpy(float64) makes the zeros of the rule"""
    case = CC.CASES["zero_mantissa_exponent_400"]
    a = pd.read_csv(pyio.BytesIO(case.data))
    assert a["b"].dtype == object
    assert np.array_equal(bits(a["b"].to_numpy(np.float64)), bits(case.rule()[1][1]))


@pytest.mark.parametrize("name", BAD)
def test_rule_rejects_every_error_case(name):
    case = CC.CASES[name]
    n, cols, error, first = case.rule()
    bit, row, field = case.err
    assert cols is None and error & bit and first[2] == bit and first[1] == field
    assert row is None or first[0] == row


def test_random_files():
    n_bad = 0
    for seed in range(CC.N_RANDOM):
        case = CC.random_file(seed)
        assert len(CC.lines_of(case.data)) - 1 <= 3000
        if case.rule()[2]:
            n_bad += 1
            assert seed % 5 == 4
        else:
            check_against_host(case)
    assert n_bad == CC.N_RANDOM // 5


@pytest.mark.parametrize("kat", ["kat134", "kat800"])
def test_fixtures(kat):
    """every field of the fixtures' node and edge files lies in the domain and the rule gives what
    io.read_nodes (before its window) and io.read_edges read"""
    pre = os.path.join(GOLDEN, kat, "event_1_filtered_graph_")
    data = open(pre + "nodes.csv", "rb").read()
    names = csvdev.header_fields(data, 1)
    assert names == ["node_idx", "layer_id", "x", "y", "z"]
    n, cols, error, _ = CC.parse_rule(data, 1, 5, [(0, CC.INT64), (1, CC.INT64), (2, CC.DOUBLE), (3, CC.DOUBLE), (4, CC.DOUBLE)])
    a = pd.read_csv(pre + "nodes.csv")
    assert error == 0 and n == len(a)
    for got, name in zip(cols, names):
        assert np.array_equal(bits(got), bits(a[name].to_numpy(got.dtype))), name
    data = open(pre + "edges.csv", "rb").read()
    assert csvdev.header_fields(data, 2) == ["node2", "node1", "weight"]
    n, cols, error, _ = CC.parse_rule(data, 2, 3, [(0, CC.INT64), (1, CC.INT64)])
    n2, n1 = gio.read_edges(pre + "edges.csv")
    assert error == 0 and np.array_equal(cols[0], n2) and np.array_equal(cols[1], n1)


def test_radius_band_holds_every_pow_difference():
    """the docstring's figures: where the C library's pow(v, 2) is not v * v, the exact square lies
    well inside the band gtf_event_window marks"""
    worst, n_diff, n_band, n_all = 0.0, 0, 0, 0
    for kat in ("kat134", "kat800"):
        a = pd.read_csv(os.path.join(GOLDEN, kat, "event_1_filtered_graph_nodes.csv"))
        for v in np.concatenate([a["x"].to_numpy(np.float64), a["y"].to_numpy(np.float64)]).tolist():
            n_all += 1
            amb = CC.ambiguous(v)
            n_band += amb
            if math.pow(v, 2.0) != v * v:
                n_diff += 1
                assert amb, v
                worst = max(worst, float(CC.band_distance(v)))
    print("pow(v, 2) != v * v for %d of %d values; largest distance from the midpoint %.5f ulp; %d in the band"
          % (n_diff, n_all, worst, n_band))
    assert n_diff > 0 and worst < 1.0 / 16


def test_ambiguity_rule_on_known_values():
    assert not CC.ambiguous(0.0) and not CC.ambiguous(3.0) and not CC.ambiguous(-0.5)     # exact squares
    assert CC.ambiguous(1e200) and CC.ambiguous(1e-200)                                   # not a normal square
    v = 1.0 + 2.0 ** -27          # v * v = 1 + 2^-26 + 2^-54: the residual 2^-54 is a quarter of ulp(1) = 2^-52
    assert CC.band_distance(v) == 0.25 and not CC.ambiguous(v)
    v = 1.0 + 2.0 ** -26 + 2.0 ** -52   # square 1 + 2^-25 + 2^-51 + 2^-52 + ...: residual just under half an ulp
    assert CC.ambiguous(v) == (CC.band_distance(v) < 1.0 / 16)


def test_header_resolution():
    h = csvdev.header_fields
    assert h(b"a,b\n1,2", 1) == ["a", "b"] and h(b"\n\r\na,,b\r\n1,2", 1) == ["a", "", "b"]
    assert h(b"3 2\nn2,n1,w\n", 2) == ["n2", "n1", "w"] and h(b"a,b", 1) == ["a", "b"]
    assert h(b"", 1) is None and h(b"\n\n", 1) is None and h(b"a\n", 2) is None
    e = csvdev.OutOfDomain(3, 1, nat.CSV_ERR_DIGITS, nat.CSV_ERR_DIGITS | nat.CSV_ERR_TEXT, "f.csv")
    assert (e.row, e.field, e.bit) == (3, 1, 1) and "more digits" in e.reason and "f.csv: row 3, field 1" in str(e)
    assert isinstance(e, ValueError)
    assert [getattr(nat, "CSV_ERR_" + k) for k in ("DIGITS", "EXPONENT", "TEXT", "EMPTY", "QUOTE", "SPACE", "INT_FORM",
                                                   "FIELDS", "ROW_LONG", "ROWS")] == \
        [CC.ERR_DIGITS, CC.ERR_EXPONENT, CC.ERR_TEXT, CC.ERR_EMPTY, CC.ERR_QUOTE, CC.ERR_SPACE, CC.ERR_INT_FORM,
         CC.ERR_FIELDS, CC.ERR_ROW_LONG, CC.ERR_ROWS]


def test_new_structs_match_the_header():
    """offsetof / sizeof of the structs of gtf_csv_parse and gtf_event_window against their ctypes
    mirrors, and the constants"""
    py = {"gtf_csv_column": nat.GtfCsvColumn, "gtf_csv_in": nat.GtfCsvIn, "gtf_csv_counts": nat.GtfCsvCounts,
          "gtf_window_in": nat.GtfWindowIn, "gtf_window_out": nat.GtfWindowOut, "gtf_window_counts": nat.GtfWindowCounts}
    lines = []
    for t, cls in py.items():
        lines += ['  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (t, f, t, f) for f, *_ in cls._fields_]
        lines.append('  printf("sizeof.%s %%zu\\n", sizeof(%s));' % (t, t))
    for c in ("GTF_CSV_MAX_COLUMNS", "GTF_CSV_MAX_FIELDS", "GTF_CSV_MAX_ROW_BYTES", "GTF_CSV_INT64", "GTF_CSV_DOUBLE",
              "GTF_CSV_ERR_DIGITS", "GTF_CSV_ERR_ROWS", "GTF_ABI_VERSION"):
        lines.append('  printf("const.%s %%zu\\n", (size_t)%s);' % (c, c))
    probe = "#include <stdio.h>\n#include <stddef.h>\n#include \"gtf.h\"\nint main(void) {\n%s\n  return 0;\n}\n" % "\n".join(lines)
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "p.c")
        with open(c, "w") as f:
            f.write(probe)
        exe = os.path.join(d, "p")
        subprocess.check_call(["gcc", "-I", os.path.dirname(HDR), c, "-o", exe])
        got = dict(ln.rsplit(" ", 1) for ln in subprocess.check_output([exe], text=True).split("\n") if ln)
    consts = {"GTF_CSV_MAX_COLUMNS": nat.CSV_MAX_COLUMNS, "GTF_CSV_MAX_FIELDS": nat.CSV_MAX_FIELDS,
              "GTF_CSV_MAX_ROW_BYTES": nat.CSV_MAX_ROW_BYTES, "GTF_CSV_INT64": nat.CSV_INT64, "GTF_CSV_DOUBLE": nat.CSV_DOUBLE,
              "GTF_CSV_ERR_DIGITS": nat.CSV_ERR_DIGITS, "GTF_CSV_ERR_ROWS": nat.CSV_ERR_ROWS, "GTF_ABI_VERSION": nat.ABI_VERSION}
    for k, v in got.items():
        t, f = k.split(".")
        if t == "sizeof":
            assert ctypes.sizeof(py[f]) == int(v), k
        elif t == "const":
            assert consts[f] == int(v), k
        else:
            assert getattr(py[t], f).offset == int(v), k
    assert nat.GtfCsvIn().struct_size == ctypes.sizeof(nat.GtfCsvIn) and nat.GtfWindowIn().abi_version == nat.ABI_VERSION


def test_host_refusals_without_a_gpu():
    """the argument checks of gtf_csv_parse and gtf_event_window run before any device work"""
    if not os.path.exists(nat.LIB_PATH):
        pytest.skip("libgtf.so not built")
    L = nat.lib()
    assert L.gtf_csv_chunk_bytes() == CC.chunk() == 4096
    assert 0 < L.gtf_csv_parse_workspace_bytes(0) <= L.gtf_csv_parse_workspace_bytes(1 << 20)
    assert 0 < L.gtf_event_window_workspace_bytes(0) <= L.gtf_event_window_workspace_bytes(1000)
    cnt = nat.GtfCsvCounts()

    def call(**kw):
        f = dict(n_bytes=0, skip_lines=1, n_fields=2, max_rows=1, n_columns=0, delimiter=ord(","))
        f.update(kw)
        return L.gtf_csv_parse(ctypes.byref(nat.GtfCsvIn(**f)), ctypes.byref(cnt), None, 0, None)

    assert call() == 0 and (cnt.n_rows, cnt.error, cnt.first_bad_row) == (0, 0, -1)      # an empty text: no launch
    for kw, text in (({"n_fields": 0}, b"n_fields"), ({"n_fields": 65}, b"n_fields"), ({"n_columns": 17}, b"n_columns"),
                     ({"delimiter": ord("e")}, b"delimiter"), ({"delimiter": ord('"')}, b"delimiter"),
                     ({"n_bytes": -1}, b"negative"), ({"n_bytes": 5}, b"null text"), ({"text": 24, "n_bytes": 5}, b"aligned"),
                     ({"skip_lines": -1}, b"negative"), ({"n_bytes": 2 ** 31 - 1}, b"2^31"),
                     ({"text": 4096, "n_bytes": 5}, b"workspace")):
        assert call(**kw) == -2 and text in L.gtf_last_error(), kw
    cin = nat.GtfCsvIn(n_bytes=0, skip_lines=1, n_fields=2, max_rows=1, n_columns=2, delimiter=ord(","))
    for cols, text in ((((2, 0, 8), (1, 1, 8)), b"field 2 of 2"), (((0, 0, 8), (0, 1, 8)), b"twice"),
                       (((0, 7, 8), (1, 1, 8)), b"type"), (((0, 0, 0), (1, 1, 8)), b"null output"),
                       (((0, 0, 12), (1, 1, 8)), b"8 bytes")):
        for k, c in enumerate(cols):
            cin.columns[k] = nat.GtfCsvColumn(*c)
        assert L.gtf_csv_parse(ctypes.byref(cin), ctypes.byref(cnt), None, 0, None) == -2 and text in L.gtf_last_error()
    cin.abi_version += 1
    assert L.gtf_csv_parse(ctypes.byref(cin), ctypes.byref(cnt), None, 0, None) == -3
    wc = nat.GtfWindowCounts(-1, -1)
    w = nat.GtfWindowIn(n_rows=0)
    assert L.gtf_event_window(ctypes.byref(w), ctypes.byref(nat.GtfWindowOut()), ctypes.byref(wc), None, 0, None) == 0
    assert (wc.n_kept, wc.n_ambiguous) == (0, 0)
    w = nat.GtfWindowIn(n_rows=4)
    assert L.gtf_event_window(ctypes.byref(w), ctypes.byref(nat.GtfWindowOut()), ctypes.byref(wc), None, 0, None) == -2
    assert b"missing input column" in L.gtf_last_error()
    w.abi_version += 1
    assert L.gtf_event_window(ctypes.byref(w), ctypes.byref(nat.GtfWindowOut()), ctypes.byref(wc), None, 0, None) == -3
    assert L.gtf_event_radius_patch(None, 0, None, None, 0, None) == 0
    assert L.gtf_event_radius_patch(None, 4, None, None, 2, None) == -2
