"""Batches of CSV texts for gtf_csv_parse_ev, built from tests/csv_cases.py, with the definition and
a restatement of the batch rule of include/gtf.h.

The definition: every file parsed alone by csv_cases.parse_rule, the results laid end to end.

The rule (batch_rule), as the device applies it to ONE buffer and a table of (start, n_bytes):
  * the buffer is cut into chunks; a chunk belongs to the one file whose bytes it holds, a file of
    0 bytes owns none;
  * a byte in front of a file's first or behind its last reads as "\\n", whatever the buffer holds
    there (padding, or the next file);
  * a line belongs to the chunk its first byte lies in; the exclusive sum of the chunks' line counts is
    global, and file e's lines are the difference of the sum at its first chunk and at its successor's;
  * rows[e] = max(lines[e] - skip, 0), clamped per file; row_off is their exclusive sum; row r of
    file e is row row_off[e] + r of every column;
  * errors are per file, the first bad row counted inside the file.

GARBAGE is what the tests put between the files: digits, commas, quotes and line ends.
"""
import numpy as np

import csv_cases as CC

GARBAGE = b'7,8.5,"9"\n12,"3.5,4\r\n,,1e5'
DEFAULT = ((0, CC.INT64), (1, CC.DOUBLE))


class Batch:
    """files: the texts; gaps[e]: whole chunks of padding in front of file e; max_rows: the outputs'
    size (None: a bound of the batch's rows)"""

    def __init__(self, files, columns=DEFAULT, n_fields=3, skip=1, gaps=None, max_rows=None):
        self.files, self.columns, self.n_fields, self.skip = [bytes(f) for f in files], list(columns), n_fields, skip
        self.gaps = list(gaps) if gaps is not None else [0] * len(self.files)
        self.max_rows = max_rows

    @property
    def K(self):
        return len(self.files)

    def bound(self):
        return self.max_rows if self.max_rows is not None else sum(f.count(b"\n") + 1 for f in self.files)

    def layout(self, chunk=None, fill=GARBAGE):
        """(the buffer, [(start, n_bytes)]): every start a multiple of the chunk, ascending; the
        padding filled with `fill` repeated"""
        C = chunk or CC.chunk()
        table, pos = [], 0
        for f, gap in zip(self.files, self.gaps):
            pos += gap * C
            table.append((pos, len(f)))
            pos += -(-len(f) // C) * C
        buf = bytearray((fill * (pos // len(fill) + 1))[:pos])
        for f, (s, n) in zip(self.files, table):
            buf[s:s + n] = f
        return bytes(buf), table

    def definition(self):
        """per file csv_cases.parse_rule -> (row_off [K + 1] with max_rows applied, per file (n_rows,
        error, first), columns: one array per column of the rows of the files WITHOUT an error laid at
        their offsets, and `exact`: the mask of the rows that are specified)"""
        per = [CC.parse_rule(f, self.skip, self.n_fields, self.columns) for f in self.files]
        return assemble(per, self.columns, self.bound())


def assemble(per, columns, max_rows):
    """per-file (n_rows, cols, error, first) -> the batch: see Batch.definition"""
    off = np.concatenate([[0], np.cumsum([p[0] for p in per])]).astype(np.int64)
    cut = np.minimum(off, max_rows)
    counts = []
    total = int(cut[-1])
    cols = [np.zeros(total, np.int64 if t == CC.INT64 else np.float64) for _, t in columns]
    exact = np.zeros(total, bool)
    for e, (n, c, error, first) in enumerate(per):
        kept = int(cut[e + 1] - cut[e])
        if kept < n:        # the file's row `kept` is the batch's row max_rows, or lies behind it
            error |= CC.ERR_ROWS
            if first is None or (kept, 0) < first[:2]:
                first = (kept, 0, CC.ERR_ROWS)
        counts.append((kept, error, first))
        if c is not None:
            for dst, src in zip(cols, c):
                dst[cut[e]:cut[e + 1]] = src[:kept]
            exact[cut[e]:cut[e + 1]] = True
    return cut.astype(np.int32), counts, cols, exact


# ------------------------------------------------------------------ the rule, restated on the buffer
def batch_rule(buf: bytes, table, skip, n_fields, columns, max_rows, chunk=None):
    """The same four results as Batch.definition, from the buffer and the table alone, the way the
    device goes about it: chunk ownership, masked bytes, global line ordinals, per-file clamps."""
    C = chunk or CC.chunk()
    K = len(table)
    # chunk offsets: the files' chunks end to end; the owner of every chunk
    coff = np.concatenate([[0], np.cumsum([-(-n // C) for _, n in table])]).astype(np.int64)
    owner = np.repeat(np.arange(K), np.diff(coff))
    assert all(s % C == 0 for s, _ in table)

    def line_starts(e):   # the bytes of file e a non-blank line starts on; outside the file a line end
        s, n = table[e]
        m = np.frombuffer(buf, np.uint8, n, s)
        prev, nxt = np.concatenate([[0x0A], m[:-1]]), np.concatenate([m[1:], [0x0A]])
        return np.nonzero((prev == 0x0A) & (m != 0x0A) & ~((m == 0x0D) & (nxt == 0x0A)))[0]

    first = [[] for _ in range(coff[-1])]       # per chunk: the line starts, as offsets into its file
    for e in range(K):
        if table[e][1]:
            for i in line_starts(e).tolist():
                first[coff[e] + i // C].append(i)
    assert all(len(first[b]) == 0 or owner[b] == e for e in range(K) for b in range(coff[e], coff[e + 1]))
    cnt = np.array([len(f) for f in first] + [0], np.int64)
    total = np.concatenate([[0], np.cumsum(cnt)])[:-1]          # the exclusive sum, one past the end included
    lines = np.array([total[coff[e + 1]] - total[coff[e]] for e in range(K)], np.int64)
    rows = np.maximum(lines - skip, 0)
    row_off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    per = []
    for e in range(K):
        s, n = table[e]
        text = []
        for b in range(coff[e], coff[e + 1]):
            for k, i in enumerate(first[b]):
                r = total[b] - total[coff[e]] + k - skip
                if r < 0:
                    continue
                j = buf.find(b"\n", s + i, s + n)
                j = s + n if j < 0 else j
                assert r == len(text)
                text.append(buf[s + i:j - 1] if buf[j - 1] == 0x0D else buf[s + i:j])
        per.append(CC.parse_rule(b"\n".join(text), 0, n_fields, columns) if text else
                   (0, [np.zeros(0, np.int64 if t == CC.INT64 else np.float64) for _, t in columns], 0, None))
        assert per[-1][0] == rows[e]
    return assemble(per, columns, max_rows)


# ------------------------------------------------------------------ the batches
def _rows(k, first=1, eol=b"\n", last_eol=True):
    """a three-field file of k rows numbered from `first`"""
    body = eol.join(b"%d,%d.25,w" % (first + i, first + i) for i in range(k))
    return CC.H3 + body + (eol if last_eol and k else b"")


EDGES = [b"3 2\nnode2,node1,weight\n960,13,1.0\n961,9,1.0\n", b"1 1\nnode2,node1,weight\n5,6,0.5",
         b"4 3\r\nnode2,node1,weight\r\n1,2,1.0\r\n3,4,1.0\r\n5,6,1.0\r\n"]
E_COLS = ((0, CC.INT64), (1, CC.INT64))


def _layout():
    C = CC.chunk()
    A, B, D = _rows(3), _rows(5, 100), _rows(2, 1000, b"\r\n")
    c = {}
    for name, case in CC.CASES.items():        # every clean single-file case as a batch of one
        if case.rule()[2] == 0:
            c["one_" + name] = Batch([case.data], case.columns, case.n_fields, case.skip)
    c["same_file_twice"] = Batch([CC.CASES["three_chunks"].data] * 2)
    c["empty_files_first_middle_last"] = Batch([b"", A, b"", b"", B, b""])
    c["only_empty_files"] = Batch([b"", b"", b""])
    c["no_files"] = Batch([])
    c["header_only_between"] = Batch([A, CC.H3, B])
    c["header_without_newline_between"] = Batch([A, b"a,b,c", B])
    c["fewer_lines_than_skip_between"] = Batch([EDGES[0], b"3 2\n", EDGES[2]], E_COLS, 3, 2)
    c["fewer_lines_than_skip_first_and_last"] = Batch([b"9 9", EDGES[0], b"\n\n"], E_COLS, 3, 2)
    c["blank_lines_only_between"] = Batch([A, b"\n\n\r\n\n", B])
    # no header: the next file starts with digits, the padding in between is garbage
    c["no_newline_before_garbage"] = Batch([b"1,2.5,z\n5,6.5,z", b"77,8.5,z\n78,9.5,z\n"], skip=0)
    c["no_newline_at_chunk_end_next_starts_with_digits"] = Batch([CC.filler(C + 1, b"")[:-1], b"77,8.5,z\n"], skip=0)
    c["ends_on_chunk_boundary"] = Batch([CC.filler(C), B, CC.filler(2 * C), D])
    c["ends_one_short_of_chunk_boundary"] = Batch([CC.filler(C - 1), B, CC.filler(C)[:-1], D])
    c["ends_one_past_chunk_boundary"] = Batch([CC.filler(C + 1), B, CC.filler(C + 2)[:-1], D])
    c["row_starts_in_last_bytes_of_last_chunk"] = Batch([CC.filler(C - 8) + b"5,6.5,z", B,
                                                         CC.filler(2 * C - 6) + b"5,6.5,z", _rows(1, 7)])
    c["row_on_last_byte_then_next_chunk"] = Batch([CC.CASES["row_starts_on_last_byte"].data, A])
    c["crlf_across_chunks"] = Batch([CC.filler(C + 1, eol=b"\r\n") + b"3,4.5,z\r\n", CC.CASES["crlf_across_chunks"].data,
                                     CC.filler(C, eol=b"\r\n")[:-1], A])
    c["long_row_into_the_halo"] = Batch([CC.CASES["row_1024_at_chunk_end_crlf"].data, A,
                                         CC.filler(C - 500) + b"1,2.5," + b"x" * 1018, B])
    c["edges_form"] = Batch(EDGES, E_COLS, 3, 2)
    c["gaps_of_whole_chunks"] = Batch([A, B, D], gaps=[1, 2, 0])
    bad = CC.CASES["bad_float_00"].data
    c["bad_file_2_of_4"] = Batch([A, B, bad, D])
    c["two_bad_files"] = Batch([A, CC.CASES["too_few_fields"].data, B, bad, D])
    c["bad_row_long_into_next_file"] = Batch([CC.CASES["row_1025"].data, A])
    c["max_rows_runs_out_in_file_1"] = Batch([_rows(2), _rows(3, 10), _rows(2, 20)], max_rows=4)
    c["max_rows_exactly_at_a_file_end"] = Batch([_rows(2), _rows(3, 10), b"", _rows(2, 20)], max_rows=5)
    c["max_rows_zero"] = Batch([CC.H3, _rows(1)], max_rows=0)
    for k in (65, 257, 2049):
        c["%d_one_row_files" % k] = Batch([_rows(1, i) for i in range(k)])
    return c


def random_batch(seed: int) -> Batch:
    """2 to 6 files: clean csv_cases.random_file texts, empty files and header-only ones, with gaps"""
    rng = np.random.default_rng(77 + seed)
    files = []
    for _ in range(int(rng.integers(2, 7))):
        u = rng.random()
        if u < 0.15:
            files.append(b"")
        elif u < 0.25:
            files.append(b"id,x,y,name,k\n")
        else:
            s = int(rng.integers(0, CC.N_RANDOM))
            files.append(CC.random_file(s + 1 if s % 5 == 4 else s).data)
    cols = ((0, CC.INT64), (1, CC.DOUBLE), (2, CC.DOUBLE), (4, CC.INT64))
    return Batch(files, cols, 5, 1, gaps=[int(g) for g in rng.integers(0, 2, len(files))])


N_RANDOM = 5
BATCHES = _layout()
