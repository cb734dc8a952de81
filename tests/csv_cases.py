"""Hand-made CSV texts for gtf_csv_parse and gtf_event_window, with a pure-Python statement of the
rules of include/gtf.h that the device must reproduce (tests/test_csv_cases.py pins that statement
to pandas.read_csv / np.loadtxt; tests/test_gpu_csv.py runs every case through the C-ABI).

The rules:
  * lines end in "\\n" or "\\r\\n", the last may lack it; a line that is empty or a lone "\\r" is
    blank: neither a row nor one of the skipped lines;
  * a row of more than 1,024 bytes is ERR_ROW_LONG at field 0 and nothing else of it is looked at;
  * every row has exactly n_fields fields: ERR_FIELDS at the first missing or the first extra field;
  * a '"' in any field is ERR_QUOTE; fields no column asks for are otherwise not read;
  * a requested field: empty -> ERR_EMPTY; a space or tab -> ERR_SPACE; not
    [+-]digits[.digits][(e|E)[+-]digits] with a mantissa digit -> ERR_TEXT; an int64 field with a
    point or exponent -> ERR_INT_FORM, with more than 18 digits -> ERR_DIGITS; a float field with
    more than 15 mantissa digit characters -> ERR_DIGITS, with a nonzero mantissa and a net exponent
    e = written exponent - fraction digits beyond +-22 -> ERR_EXPONENT;
  * the value: M * 10^e (e >= 0) or M / 10^-e, one rounding; the sign by negation;
  * error = the bits of every offending field; first = the lowest (row, field) and its bit.
"""
import math
import re
from fractions import Fraction

import numpy as np

INT64, DOUBLE = 0, 1
(ERR_DIGITS, ERR_EXPONENT, ERR_TEXT, ERR_EMPTY, ERR_QUOTE, ERR_SPACE, ERR_INT_FORM, ERR_FIELDS, ERR_ROW_LONG,
 ERR_ROWS) = (1 << k for k in range(10))
MAX_ROW = 1024
NUMBER = re.compile(rb"([+-]?)(\d*)(\.?)(\d*)(?:[eE]([+-]?\d+))?\Z")


def chunk() -> int:
    """the bytes one block takes (gtf_csv_chunk_bytes), 4096 without the library"""
    try:
        from gtf import _native as nat
        return int(nat.lib().gtf_csv_chunk_bytes())
    except Exception:   # noqa: BLE001  (no library built: the documented value)
        return 4096


# ------------------------------------------------------------------ the rule
def field_rule(f: bytes, typ):
    """one field: (value, 0) or (None, error bit); typ None = not requested"""
    if b'"' in f:
        return None, ERR_QUOTE
    if typ is None:
        return None, 0
    if not f:
        return None, ERR_EMPTY
    if b" " in f or b"\t" in f:
        return None, ERR_SPACE
    m = NUMBER.match(f)
    if not m or not (m.group(2) or m.group(4)):
        return None, ERR_TEXT
    sign, ip, point, fp, ex = m.groups()
    if fp and not point:
        return None, ERR_TEXT
    digits = ip + fp
    if typ == INT64:
        if point or ex is not None:
            return None, ERR_INT_FORM
        if len(digits) > 18:
            return None, ERR_DIGITS
        return np.int64(int(sign + digits)), 0
    if len(digits) > 15:
        return None, ERR_DIGITS
    mant, e = int(digits), int(ex or 0) - len(fp)
    if mant == 0:
        v = 0.0
    elif abs(e) > 22:
        return None, ERR_EXPONENT
    else:
        v = float(mant) * float(10 ** e) if e >= 0 else float(mant) / float(10 ** -e)
    return np.float64(-v if sign == b"-" else v), 0


def lines_of(data: bytes):
    """the non-blank lines, without their line ends"""
    out = []
    for ln in data.split(b"\n"):
        if ln.endswith(b"\r"):
            ln = ln[:-1]
        if ln:
            out.append(ln)
    return out


def parse_rule(data: bytes, skip: int, n_fields: int, columns, delim: bytes = b","):
    """columns: [(field, INT64 | DOUBLE)]. Returns (n_rows, [one array per column] or None on an
    error, error bits, (row, field, bit) of the first error or None)."""
    rows = lines_of(data)[skip:]
    want = dict(columns)
    vals = {f: [] for f, _ in columns}
    error, first = 0, None
    for r, ln in enumerate(rows):
        bad = []
        if len(ln) > MAX_ROW:
            bad.append((0, ERR_ROW_LONG))
        else:
            fields = ln.split(delim)
            for i, f in enumerate(fields):
                if i < n_fields:
                    v, e = field_rule(f, want.get(i))
                    if e:
                        bad.append((i, e))
                    elif i in want:
                        vals[i].append(v)
                elif i == n_fields:
                    bad.append((i, ERR_FIELDS))
            if len(fields) < n_fields:
                bad.append((len(fields), ERR_FIELDS))
        for i, e in bad:
            error |= e
            if first is None or (r, i) < first[:2]:
                first = (r, i, e)
    if error:
        return len(rows), None, error, first
    cols = [np.array(vals[f], np.int64 if t == INT64 else np.float64) for f, t in columns]
    return len(rows), cols, 0, None


# ------------------------------------------------------------------ the cases
class Case:
    def __init__(self, data, columns=((0, INT64), (1, DOUBLE)), n_fields=None, skip=1, cols=None, err=None,
                 loadtxt=False):
        self.data, self.columns, self.skip = data, list(columns), skip
        self.loadtxt = loadtxt or skip == 2   # the host reader to compare with: np.loadtxt, else pandas
        hdr = lines_of(data)[:skip]
        self.n_fields = n_fields if n_fields is not None else (len(hdr[-1].split(b",")) if len(hdr) == skip and skip else 2)
        self.cols = cols      # stated by hand: [[...], [...]]; None: the rule's
        self.err = err        # stated by hand: (bit, row, field)

    def rule(self):
        return parse_rule(self.data, self.skip, self.n_fields, self.columns)


H2, H3 = b"a,b\n", b"a,b,c\n"


def filler(target: int, head: bytes = H3, eol: bytes = b"\n") -> bytes:
    """head and three-field rows "i,i.5,z" of exactly `target` bytes; the last row's numbers carry
    leading zeros to land there"""
    out, i = bytearray(head), 1
    while target - len(out) >= 30 + len(eol):
        out += b"%d,%d.5,z" % (i, i) + eol
        i += 1
    pad = target - len(out) - len(b"7,1.5,z" + eol)
    assert 0 <= pad <= 28, pad
    a, b = min(pad, 15), pad - min(pad, 15)
    out += b"0" * a + b"7," + b"0" * b + b"1.5,z" + eol
    assert len(out) == target
    return bytes(out)


FLOAT_FORMS = [b"-0", b"-0.0", b"+.5", b"5.", b"007.50", b"1e3", b"1E-3", b"1.5e+2", b"123456789012345",
               b"0.12345678901234", b"-12345678.9012345", b"1e22", b"123.45e24", b"1e-22", b"123456789012345e-22",
               b"0.000e-400", b"9007199254740.99", b"3.14159", b"-55.2492", b"0.620091", b"-1502.5",
               b"+0", b"00000000000000.1", b"999999999999999e22", b"1e-7", b"4.35e-5"]
INT_FORMS = [b"0", b"-0", b"+7", b"007", b"123456789012345678", b"+999999999999999999", b"-999999999999999999",
             b"-123456789012345678", b"22525763437723648", b"954766419537428480", b"000000000000000001"]
# (text of field 1 of a float column or field 0 of an int column, the bit); each is row 2 of its file
BAD_FLOATS = [(b"1234567890123456", ERR_DIGITS), (b"0.123456789012345", ERR_DIGITS),
              (b"0.000000000000000000001", ERR_DIGITS), (b"1e23", ERR_EXPONENT), (b"1.5e24", ERR_EXPONENT),
              (b"1e-23", ERR_EXPONENT), (b"12345e-28", ERR_EXPONENT), (b"1e400", ERR_EXPONENT),
              (b"1e99999999999999999999", ERR_EXPONENT), (b"nan", ERR_TEXT), (b"inf", ERR_TEXT), (b"-inf", ERR_TEXT),
              (b"NaN", ERR_TEXT), (b"abc", ERR_TEXT), (b"0x10", ERR_TEXT), (b"1_000", ERR_TEXT), (b"1e", ERR_TEXT),
              (b"1e+", ERR_TEXT), (b".", ERR_TEXT), (b"+", ERR_TEXT), (b".e5", ERR_TEXT), (b"--1", ERR_TEXT), (b"1.2.3", ERR_TEXT),
              (b"1e5.0", ERR_TEXT), (b"1d5", ERR_TEXT), (b"", ERR_EMPTY), (b'"2.5"', ERR_QUOTE), (b" 2.5", ERR_SPACE),
              (b"2.5 ", ERR_SPACE), (b"2\t5", ERR_SPACE), (b"1\r5", ERR_TEXT)]
BAD_INTS = [(b"1234567890123456789", ERR_DIGITS), (b"-1000000000000000000", ERR_DIGITS), (b"960.0", ERR_INT_FORM),
            (b"1e3", ERR_INT_FORM), (b"5.", ERR_INT_FORM), (b"", ERR_EMPTY), (b"x", ERR_TEXT), (b'"1"', ERR_QUOTE),
            (b" 1", ERR_SPACE)]


def _layout():
    C = chunk()
    c = {}
    c["empty"] = Case(b"", cols=[[], []])
    c["header_only"] = Case(H2, cols=[[], []])
    c["header_only_no_newline"] = Case(b"a,b", cols=[[], []])
    c["one_row"] = Case(H2 + b"1,2.5\n", cols=[[1], [2.5]])
    c["one_row_no_newline"] = Case(H2 + b"1,2.5", cols=[[1], [2.5]])
    c["crlf"] = Case(b"a,b\r\n1,2.5\r\n\r\n3,4", cols=[[1, 3], [2.5, 4.0]])
    c["crlf_last_cr_only"] = Case(b"a,b\r\n1,2.5\r\n3,4\r", cols=[[1, 3], [2.5, 4.0]])
    c["blank_lines"] = Case(H2 + b"\n1,2\n\n\n3,4\n\n\n", cols=[[1, 3], [2.0, 4.0]])
    c["blank_before_header"] = Case(b"\n\r\na,b\n1,2\n", cols=[[1], [2.0]])
    c["only_blank_lines"] = Case(b"\n\n\r\n\n", cols=[[], []])
    c["edges_two_lines"] = Case(b"3 2\nnode2,node1,weight\n960,13,1.0\n961,9,1.0\n", columns=((0, INT64), (1, INT64)),
                                skip=2, cols=[[960, 961], [13, 9]])
    c["long_header"] = Case(b"a,b," + b"x" * (C + 100) + b"\n1,2.5,0\n-2,-3.5,1\n", cols=[[1, -2], [2.5, -3.5]])
    c["header_two_chunks_blank"] = Case(b"a,b," + b"x" * (2 * C) + b"\r\n\r\n" + b"\n" * 40 + b"1,2.5,0\r\n",
                                        cols=[[1], [2.5]])
    c["reordered_columns"] = Case(b"a,b,c,d\n1,2,3,4\n5,6,7,8\n", columns=((3, DOUBLE), (0, INT64), (2, INT64)),
                                  cols=[[4.0, 8.0], [1, 5], [3, 7]])
    c["no_columns"] = Case(H2 + b"1,2\n3,4\n", columns=(), cols=[])
    c["text_in_unrequested"] = Case(b"a,b,c\n1,2.5,hello world\n2,3.5,\n3,4.5,nan\n", cols=[[1, 2, 3], [2.5, 3.5, 4.5]])
    # chunk boundaries
    c["newline_last_byte_of_chunk"] = Case(filler(C) + b"5,6.5,z\n")
    c["newline_first_byte_of_next_chunk"] = Case(filler(C + 1) + b"5,6.5,z\n")
    c["row_starts_on_last_byte"] = Case(filler(C - 1) + b"5,6.5,z\n8,9.5,z")
    c["crlf_across_chunks"] = Case(filler(C - 8) + b"5,6.5,z\r\n3,4.5,z\n")
    c["blank_crlf_across_chunks"] = Case(filler(C - 1) + b"\r\n9,9.5,z\n")
    c["row_1024_across_chunks"] = Case(filler(C - 500) + b"1,2.5," + b"x" * 1018 + b"\n4,5.5,z\n")
    c["row_1024_at_chunk_end_crlf"] = Case(filler(2 * C - 1) + b"1,2.5," + b"x" * 1018 + b"\r\n4,5.5,z")
    c["row_1025"] = Case(filler(C - 500) + b"1,2.5," + b"x" * 1019 + b"\n4,5.5,z\n", err=(ERR_ROW_LONG, None, 0))
    c["row_5000_hides_its_fields"] = Case(H3 + b"1,2.5,z\n" + b'9,"",' + b"x," * 2500 + b"\n4,5.5,z\n", err=(ERR_ROW_LONG, 1, 0))
    c["three_chunks"] = Case(filler(3 * C + 17) + b"5,6.5,z")
    # numbers
    c["float_forms"] = Case(H2 + b"".join(b"%d,%s\n" % (i, t) for i, t in enumerate(FLOAT_FORMS)),
                            cols=[list(range(len(FLOAT_FORMS))), [float(t) for t in FLOAT_FORMS]])
    # pandas' tokenizer takes an exponent beyond its range for text even under a zero mantissa (the column
    # becomes strings, which read_nodes' to_numpy(float64) converts with Python's float): np.loadtxt is the
    # reader to compare with
    c["zero_mantissa_exponent_400"] = Case(H2 + b"1,0e400\n2,-0.0e400\n3,0E+400\n4,-0e-400\n", loadtxt=True,
                                           cols=[[1, 2, 3, 4], [0.0, -0.0, 0.0, -0.0]])
    c["int_forms"] = Case(H2 + b"".join(b"%s,%d\n" % (t, i) for i, t in enumerate(INT_FORMS)),
                          cols=[[int(t) for t in INT_FORMS], [float(i) for i in range(len(INT_FORMS))]])
    for k, (t, bit) in enumerate(BAD_FLOATS):
        c["bad_float_%02d" % k] = Case(H3 + b"1,2.5,z\n2,3.5,z\n3," + t + b",z\n4,5.5,z\n", err=(bit, 2, 1))
    for k, (t, bit) in enumerate(BAD_INTS):
        c["bad_int_%02d" % k] = Case(H3 + b"1,2.5,z\n2,3.5,z\n" + t + b",4.5,z\n4,5.5,z\n", err=(bit, 2, 0))
    c["empty_last_field"] = Case(H2 + b"1,2\n3,\n", err=(ERR_EMPTY, 1, 1))
    c["quote_in_unrequested"] = Case(H3 + b'1,2.5,"z"\n', err=(ERR_QUOTE, 0, 2))
    c["too_few_fields"] = Case(H3 + b"1,2.5,z\n2,3.5\n", err=(ERR_FIELDS, 1, 2))
    c["one_field_of_three"] = Case(H3 + b"1,2.5,z\n7\n", err=(ERR_FIELDS, 1, 1))
    c["too_many_fields"] = Case(H3 + b"1,2.5,z\n2,3.5,z,9,9\n", err=(ERR_FIELDS, 1, 3))
    # the first of several: rows in three chunks, given out of order; two in one row
    body = filler(2 * C + 100).split(b"\n")
    n = len(body) - 2           # (the header in front, the empty piece behind)
    r0, r1, r2 = 5, n // 2, n - 3
    body[1 + r2] = b"1,nan,z"
    body[1 + r1] = b'x,"2.5",z'
    body[1 + r0] = b"1,2.5"
    c["first_of_several"] = Case(b"\n".join(body), err=(ERR_FIELDS, r0, 2))
    body[1 + r0] = b"1,2.5,z"
    c["first_of_two_in_a_row"] = Case(b"\n".join(body), err=(ERR_TEXT, r1, 0))
    return c


CASES = _layout()
N_RANDOM = 20


def _random_float(rng):
    nd = int(rng.integers(1, 16))
    digits = "".join(str(d) for d in rng.integers(0, 10, nd))
    if rng.random() < 0.2:
        digits = ("0" * int(rng.integers(1, 4)) + digits)[:15]
    k = int(rng.integers(0, len(digits) + 1)) if rng.random() < 0.8 else None
    s, frac = (digits, 0) if k is None else (digits[:k] + "." + digits[k:], len(digits) - k)
    if rng.random() < 0.3:
        net = int(rng.integers(-22, 23))
        s += ("e", "E")[int(rng.integers(2))] + ("%+d" if rng.random() < 0.5 else "%d") % (net + frac)
    return ("", "-", "+")[int(rng.choice(3, p=[0.5, 0.4, 0.1]))] + s


def random_file(seed: int) -> Case:
    """at most 3,000 rows of (int, float, float, text, int), mixed number forms, "\\n" or "\\r\\n", blank
    lines, with or without the last newline; every fifth file has one field outside the domain"""
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(1, 3001)) if seed else 3000
    eol = "\r\n" if seed % 3 == 1 else "\n"
    rows = []
    for i in range(n):
        rows.append("%d,%s,%s,%s,%d" % (int(rng.integers(-10 ** 6, 10 ** 6)) if rng.random() < 0.9 else int(rng.integers(-2 ** 59, 2 ** 59)),
                                        _random_float(rng), _random_float(rng), "t%d" % i if rng.random() < 0.5 else "",
                                        int(rng.integers(0, 20000))))
        if rng.random() < 0.02:
            rows.append("")
    if seed % 5 == 4:
        i = int(rng.integers(0, len(rows)))
        while not rows[i]:
            i = (i + 1) % len(rows)
        f = rows[i].split(",")
        f[2] = ("nan", "1e300", "12345678901234567", "")[seed % 4]
        rows[i] = ",".join(f)
    text = eol.join(["id,x,y,name,k"] + rows) + (eol if seed % 2 else "")
    return Case(text.encode(), columns=((0, INT64), (1, DOUBLE), (2, DOUBLE), (4, INT64)))


# ------------------------------------------------------------------ the window, the radius band
def window_cases():
    """name -> (node_idx, layer_id, x, y, z, lo, hi)"""
    rng = np.random.default_rng(7)

    def ev(layers):
        n = len(layers)
        return (np.arange(100, 100 + n, dtype=np.int64), np.array(layers, np.int64), rng.normal(0, 300, n),
                rng.normal(0, 300, n), rng.normal(0, 1000, n))

    big = rng.integers(6000, 10000, 3001).tolist()
    return {"ends_inclusive": ev([6999, 7000, 7001, 7999, 8000, 8001, 7002]) + (7000, 8000),
            "none_kept": ev([1, 2, 3, 9000]) + (7000, 8000),
            "all_kept": ev([7002] * 700) + (7000, 8000),
            "no_rows": ev([]) + (7000, 8000),
            "many_blocks": ev(big) + (7000, 9000),
            "zeros_and_extremes": (np.arange(6, dtype=np.int64), np.full(6, 7002, np.int64),
                                   np.array([0.0, -0.0, 1e-200, 1e200, 3.0, -55.2492]), np.array([0.0, 5.0, 0.0, 1.0, 4.0, 0.620091]),
                                   np.zeros(6), 7000, 8000)}


def window_rule(ids, lay, x, y, z, lo, hi):
    """io.read_nodes after the parse, with r = sqrt(x*x + y*y): (ids, x, y, z, r, layer)"""
    keep = (lay >= lo) & (lay <= hi)
    with np.errstate(over="ignore", under="ignore"):
        r = np.sqrt(x[keep] * x[keep] + y[keep] * y[keep])
    return ids[keep], x[keep], y[keep], z[keep], r, lay[keep]


def band_distance(v: float):
    """| |e| - ulp(p) / 2 | / ulp(p) for p = v * v rounded and e the exact residual, exactly (None
    for a square that is zero or not a normal number)"""
    p = v * v
    if v == 0.0 or not math.isfinite(p) or p < 2.0 ** -959:
        return None
    e = Fraction(v) ** 2 - Fraction(p)
    ulp = Fraction(math.ulp(p))
    return abs(abs(e) - ulp / 2) / ulp


def ambiguous(v: float) -> bool:
    """gtf_event_window's test for one coordinate"""
    if v == 0.0:
        return False
    d = band_distance(v)
    return d is None or d < Fraction(1, 16)
