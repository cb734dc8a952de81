"""CSV files parsed on the GPU (gtf_csv_parse, csrc/gtf_csv.hip): the bytes of a file go up once
and the requested columns stay in device memory as int64 / float64 arrays in row order, bit for
bit what pandas.read_csv and np.loadtxt return on these files -- for every field inside the exact
domain of include/gtf.h (a sign and at most 18 digits for an integer; at most 15 mantissa digit
characters and a net decimal exponent within +-22 for a float). A field outside it raises
:class:`OutOfDomain` with its row, field and reason: nothing is guessed, and the callers here
(gtf.io.read_nodes_dev / read_edges_dev, gtf.metrics.truth_files_dev, pipeline.build_event_dev)
then read that file with the host parser, which stays the definition."""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native as nat

TYPES = {"int64": nat.CSV_INT64, "float64": nat.CSV_DOUBLE}


class OutOfDomain(ValueError):
    """a field gtf_csv_parse does not take: ``row`` (from 0, after the skipped lines), ``field``,
    ``reason`` (the text of the first error's GTF_CSV_ERR_* bit), ``error`` (every bit found)"""

    def __init__(self, row, field, bit, error, what=""):
        self.row, self.field, self.bit, self.error = int(row), int(field), int(bit), int(error)
        self.reason = nat.CSV_ERRORS.get(self.bit, "error bit 0x%x" % self.bit)
        super().__init__("%srow %d, field %d: %s (outside the exact domain of gtf_csv_parse)"
                         % (what + ": " if what else "", self.row, self.field, self.reason))


class Parsed(dict):
    """parse_dev's result: {column name: device array of n_rows elements}, with ``n_rows``, the
    allocator ``mem`` ("torch" / "hip") and ``device``"""
    n_rows = 0


def read_bytes(data_or_path) -> bytes:
    if isinstance(data_or_path, (bytes, bytearray, memoryview)):
        return bytes(data_or_path)
    with open(data_or_path, "rb") as f:
        return f.read()


def header_fields(data, skip_lines: int, delimiter: bytes = b","):
    """the fields of the last of the first ``skip_lines`` non-blank lines (the header), as the
    device counts lines: blank ones (nothing, or a lone "\\r") are not lines. None when the
    text has fewer lines."""
    pos, line = 0, None
    n = len(data)
    for _ in range(skip_lines):
        while True:
            if pos >= n:
                return None
            end = data.find(b"\n", pos)
            end = n if end < 0 else end
            line = bytes(data[pos:end])
            pos = end + 1
            if line.endswith(b"\r"):
                line = line[:-1]
            if line:
                break
    return None if line is None else [f.decode("utf-8", "replace") for f in line.split(delimiter)]


def parse_dev(data_or_path, columns, skip_lines: int = 1, device="cuda", mem: str = "torch", delimiter: str = ",",
              fields=None, mm=None, mark=None) -> Parsed:
    """The columns of one CSV file as device arrays. ``columns``: (name, "int64" | "float64")
    pairs, resolved against the header -- the last skipped line; of a name that occurs twice the
    first field, as pandas keeps it -- or (field index, type) pairs. ``fields``: the number of
    fields of a row when there is no header line (skip_lines == 0). Raises OutOfDomain for a field
    outside the exact domain, KeyError for a column the header lacks. mark: called with "upload" and
    "parse" as each part has been issued (tools/resident_parse.py reads the clock there)."""
    from .metrics import _Mem
    mm = mm or _Mem(device, mem)
    data = read_bytes(data_or_path)
    delim = delimiter.encode()
    names = header_fields(data, skip_lines, delim) if skip_lines else None
    if skip_lines and names is None:    # fewer lines than skip_lines: no row, whatever the fields are
        names = [name for name, _ in columns] or [""]
    n_fields = len(names) if names is not None else fields
    if n_fields is None:
        raise ValueError("parse_dev: no header line; give fields=")
    want = []
    for name, typ in columns:
        if isinstance(name, str):
            if names is None or name not in names:
                raise KeyError("column %r not in the header %r" % (name, names))
            want.append((name, names.index(name), TYPES[typ]))
        else:
            want.append((name, int(name), TYPES[typ]))
    if len(want) > nat.CSV_MAX_COLUMNS:
        raise ValueError("parse_dev: more than %d columns" % nat.CSV_MAX_COLUMNS)
    n = len(data)
    max_rows = data.count(b"\n") + 1
    text = mm.from_host(np.frombuffer(bytearray(data), np.uint8)) if n else None
    out = [mm.empty(max_rows, np.int64 if t == nat.CSV_INT64 else np.float64) for _, _, t in want]
    cin = nat.GtfCsvIn(text=mm.p(text), n_bytes=n, skip_lines=int(skip_lines), n_fields=int(n_fields), max_rows=max_rows,
                       n_columns=len(want), delimiter=delim[0])
    for k, ((_, f, t), o) in enumerate(zip(want, out)):
        cin.columns[k] = nat.GtfCsvColumn(f, t, mm.p(o))
    nb = int(mm.lib.gtf_csv_parse_workspace_bytes(n))
    ws = mm.empty(nb, np.uint8)
    cnt = nat.GtfCsvCounts()
    if mark:
        mark("upload")
    rc = mm.lib.gtf_csv_parse(ctypes.byref(cin), ctypes.byref(cnt), mm.p(ws), ctypes.c_size_t(nb), mm.stream)
    if rc == -2 and cnt.error:
        raise OutOfDomain(cnt.first_bad_row, cnt.first_bad_field, cnt.first_bad_error, cnt.error,
                          data_or_path if isinstance(data_or_path, str) else "")
    nat.check(rc)
    if mark:
        mark("parse")
    res = Parsed((name, mm.first(o, int(cnt.n_rows))) for (name, _, _), o in zip(want, out))
    res.n_rows, res.mem, res.device, res._m = int(cnt.n_rows), mm.mem, mm.device, mm
    return res
