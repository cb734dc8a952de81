"""CSV files parsed on the GPU (gtf_csv_parse, csrc/gtf_csv.hip): the bytes of a file go up once
and the requested columns stay in device memory as int64 / float64 arrays in row order, bit for
bit what pandas.read_csv and np.loadtxt return on these files -- for every field inside the exact
domain of include/gtf.h (a sign and at most 18 digits for an integer; at most 15 mantissa digit
characters and a net decimal exponent within +-22 for a float). A field outside it raises
:class:`OutOfDomain` with its row, field and reason: nothing is guessed, and the callers here
(gtf.io.read_nodes_dev / read_edges_dev, gtf.metrics.truth_files_dev, pipeline.build_event_dev)
then read that file with the host parser, which stays the definition.

parse_batch_dev does the same for the K files of one kind of a batch of events in one call
(gtf_csv_parse_ev): the files are read into one host buffer at chunk-aligned offsets, go up once
and come back as fused columns, file after file, with the host row offsets."""
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


def header_fields(data, skip_lines: int, delimiter: bytes = b",", start: int = 0, end: int = None):
    """the fields of the last of the first ``skip_lines`` non-blank lines (the header), as the
    device counts lines: blank ones (nothing, or a lone "\\r") are not lines. None when the
    text has fewer lines. start, end: the text is data[start:end]."""
    pos, line = start, None
    n = len(data) if end is None else end
    for _ in range(skip_lines):
        while True:
            if pos >= n:
                return None
            end = data.find(b"\n", pos, n)
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
    n_fields, resolved = resolve_columns(names, columns, fields)
    want = [(name, f, t) for (name, _), (f, t) in zip(columns, resolved)]
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


# ------------------------------------------------------------------ a batch's files of one kind
class ParsedBatch(dict):
    """parse_batch_dev's result: {column name: device array of n_rows elements}, the files' rows end
    to end; ``row_off`` (host int32 [K + 1]: file e's rows are row_off[e] .. row_off[e + 1]),
    ``n_rows`` = row_off[K], ``info`` and ``files``:

    info   {"mode": "batch"} after one gtf_csv_parse_ev, or {"mode": "per-file", "file": e,
           "reason": text} when file e made the batch impossible (another header layout, a field
           outside the exact domain) and every file went through parse_dev on its own;
    files  per file "device", or "host" where ``host_reader`` read it (with ``reasons[e]``)."""
    n_rows = 0


def batch_layout(sizes, chunk: int = None):
    """where the files of a batch lie in its one buffer: every start a multiple of the chunk
    (gtf_csv_chunk_bytes), ascending, a file of 0 bytes taking no room -> (starts, total bytes)"""
    chunk = chunk or int(nat.lib().gtf_csv_chunk_bytes())
    starts, pos = [], 0
    for n in sizes:
        if n < 0:
            raise ValueError("batch_layout: negative size")
        starts.append(pos)
        pos += -(-int(n) // chunk) * chunk
    return starts, pos


def read_batch(files, chunk: int = None, fill: bytes = None):
    """the files (paths, or bytes-like texts) in one host buffer at batch_layout's offsets, each
    read straight into its place -> (bytearray, starts, sizes). The padding behind a file is
    whatever the buffer held (zeros; ``fill``: that pattern repeated, for the tests)."""
    import os
    sizes = [len(f) if isinstance(f, (bytes, bytearray, memoryview)) else os.path.getsize(f) for f in files]
    starts, total = batch_layout(sizes, chunk)
    buf = bytearray(total) if fill is None else bytearray((fill * (total // len(fill) + 1))[:total])
    view = memoryview(buf)
    for f, s, n in zip(files, starts, sizes):
        if isinstance(f, (bytes, bytearray, memoryview)):
            view[s:s + n] = f
        elif n:
            with open(f, "rb") as fh:
                if fh.readinto(view[s:s + n]) != n:
                    raise IOError("%s: shorter than its size" % f)
    return buf, starts, sizes


def resolve_columns(names, columns, fields=None):
    """the (n_fields, ((field index, type code), ...)) a header gives a column request, as parse_dev
    resolves it; names None: no header line"""
    n_fields = len(names) if names is not None else fields
    if n_fields is None:
        raise ValueError("parse_dev: no header line; give fields=")
    want = []
    for name, typ in columns:
        if isinstance(name, str):
            if names is None or name not in names:
                raise KeyError("column %r not in the header %r" % (name, names))
            want.append((names.index(name), TYPES[typ]))
        else:
            want.append((int(name), TYPES[typ]))
    return int(n_fields), tuple(want)


def batch_request(buf, starts, sizes, columns, skip_lines, delim=b",", fields=None):
    """one layout for all the files of the buffer, or the first file that has another:
    -> ((n_fields, fields), None, None) or (None, file, reason). A file with fewer lines than
    skip_lines has no row and takes any layout."""
    layout, first = None, None
    for e, (s, n) in enumerate(zip(starts, sizes)):
        names = header_fields(buf, skip_lines, delim, s, s + n) if skip_lines else None
        if skip_lines and names is None:
            continue
        got = resolve_columns(names, columns, fields)
        if layout is None:
            layout, first = got, e
        elif got != layout:
            return None, e, ("file %d resolves the columns to fields %r of %d, file %d to %r of %d"
                             % (e, [f for f, _ in got[1]], got[0], first, [f for f, _ in layout[1]], layout[0]))
    if layout is None:      # no file has a row
        layout = (max(len(columns), 1), tuple((k, TYPES[t]) for k, (_, t) in enumerate(columns)))
    return layout, None, None


def parse_batch_dev(files, columns, skip_lines: int = 1, device="cuda", mem: str = "torch", delimiter: str = ",",
                    fields=None, mm=None, mark=None, host_reader=None) -> ParsedBatch:
    """The columns of K CSV files of one kind as fused device arrays: one host buffer (read_batch),
    one upload, one gtf_csv_parse_ev. ``columns`` as parse_dev's. When the headers do not all resolve
    the request to the same fields, or a file holds a field outside the exact domain, every file is
    parsed on its own with parse_dev instead and the columns are put end to end (``info`` names the
    file and the reason); the offending file then raises OutOfDomain unless ``host_reader(file) ->
    one host array per column`` is given, which reads it. mark: as parse_dev's."""
    from .metrics import _Mem
    mm = mm or _Mem(device, mem)
    files = list(files)
    K = len(files)
    delim = delimiter.encode()
    if len(columns) > nat.CSV_MAX_COLUMNS:
        raise ValueError("parse_batch_dev: more than %d columns" % nat.CSV_MAX_COLUMNS)
    dts = [np.int64 if TYPES[t] == nat.CSV_INT64 else np.float64 for _, t in columns]
    buf, starts, sizes = read_batch(files)
    layout, bad, reason = batch_request(buf, starts, sizes, columns, skip_lines, delim, fields)
    res = ParsedBatch()
    res.mem, res.device, res._m = mm.mem, mm.device, mm
    res.files, res.reasons = ["device"] * K, [None] * K
    if bad is None and len(buf):
        n_fields, want = layout
        max_rows = buf.count(b"\n") + K
        text = mm.from_host(np.frombuffer(buf, np.uint8))
        out = [mm.empty(max(max_rows, 1), dt) for dt in dts]
        tab = (nat.GtfCsvFile * max(K, 1))(*[nat.GtfCsvFile(s, n) for s, n in zip(starts, sizes)])
        cin = nat.GtfCsvInEv(text=mm.p(text), files=ctypes.cast(tab, ctypes.c_void_p), n_files=K,
                             skip_lines=int(skip_lines), n_fields=n_fields, max_rows=max_rows, n_columns=len(want),
                             delimiter=delim[0])
        for k, ((f, t), o) in enumerate(zip(want, out)):
            cin.columns[k] = nat.GtfCsvColumn(f, t, mm.p(o))
        nb = int(mm.lib.gtf_csv_parse_ev_workspace_bytes(len(buf), K))
        ws = mm.empty(nb, np.uint8)
        cnt = (nat.GtfCsvCounts * max(K, 1))()
        if mark:
            mark("upload")
        rc = mm.lib.gtf_csv_parse_ev(ctypes.byref(cin), cnt, mm.p(ws), ctypes.c_size_t(nb), mm.stream)
        first = next((e for e in range(K) if cnt[e].error), None) if rc == -2 else None
        if first is None:
            nat.check(rc)
            if mark:
                mark("parse")
            res.row_off = np.concatenate([[0], np.cumsum([cnt[e].n_rows for e in range(K)])]).astype(np.int32)
            res.n_rows = int(res.row_off[-1])
            res.update((name, mm.first(o, res.n_rows)) for (name, _), o in zip(columns, out))
            res.info = {"mode": "batch"}
            return res
        c = cnt[first]
        bad, reason = first, str(OutOfDomain(c.first_bad_row, c.first_bad_field, c.first_bad_error, c.error,
                                             files[first] if isinstance(files[first], str) else "file %d" % first))
    elif bad is None:       # no byte at all
        res.row_off, res.info = np.zeros(K + 1, np.int32), {"mode": "batch"}
        res.update((name, mm.first(mm.empty(1, dt), 0)) for (name, _), dt in zip(columns, dts))
        return res
    # per file, as before the batch call existed
    parts, rows = [], []
    for e, f in enumerate(files):
        try:
            c = parse_dev(f, columns, skip_lines, mm=mm, delimiter=delimiter, fields=fields)
            parts.append([c[name] for name, _ in columns])
            rows.append(c.n_rows)
        except OutOfDomain as err:
            if host_reader is None:
                raise
            host = [np.ascontiguousarray(a, dt).reshape(-1) for a, dt in zip(host_reader(f), dts)]
            res.files[e], res.reasons[e] = "host", str(err)
            parts.append([mm.from_host(a) if a.size else None for a in host])
            rows.append(int(host[0].size) if host else 0)
    res.row_off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int32)
    res.n_rows = int(res.row_off[-1])
    res.info = {"mode": "per-file", "file": int(bad), "reason": reason}
    res.update((name, _cat(mm, [p[k] for p in parts], rows, dt)) for k, ((name, _), dt) in enumerate(zip(columns, dts)))
    return res


def _cat(mm, parts, rows, dtype):
    """device arrays end to end (the per-file path only: one copy per part)"""
    total = int(sum(rows))
    if mm.torch is not None:
        keep = [p[:n] for p, n in zip(parts, rows) if n]
        return mm.torch.cat(keep) if keep else mm.empty(0, dtype)
    out = mm.first(mm.empty(max(total, 1), dtype), total)
    size, pos = np.dtype(dtype).itemsize, 0
    for p, n in zip(parts, rows):
        if n:
            nat.check(mm.lib.gtf_memcpy_dtod(ctypes.c_void_p(out.data_ptr() + pos * size), ctypes.c_void_p(p.data_ptr()),
                                             ctypes.c_size_t(n * size), mm.stream))
            pos += n
    if total:
        nat.check(mm.lib.gtf_stream_synchronize(None))
    return out
