"""tests/csv_batch_cases.py checks itself, without a device: the restated batch rule (chunk ownership,
bytes outside a file read as line ends, per-file clamped row counts and offsets) gives what the
definition gives -- every file parsed alone by csv_cases.parse_rule, laid end to end; a naive
"concatenate and parse once" does not; gtf.csvdev lays the files out as the library demands and sees
a header mismatch before anything goes to a device."""
import numpy as np
import pytest

import csv_batch_cases as BC
import csv_cases as CC
from gtf import csvdev


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else a.dtype)


def same(got, exp):
    (off_a, cnt_a, cols_a, ok_a), (off_b, cnt_b, cols_b, ok_b) = got, exp
    assert off_a.tolist() == off_b.tolist() and cnt_a == cnt_b and ok_a.tolist() == ok_b.tolist()
    for a, b in zip(cols_a, cols_b):
        assert a.dtype == b.dtype and np.array_equal(bits(a)[ok_a], bits(b)[ok_b])


@pytest.mark.parametrize("name", sorted(BC.BATCHES))
def test_rule_equals_the_definition(name):
    b = BC.BATCHES[name]
    buf, table = b.layout(4096)
    same(BC.batch_rule(buf, table, b.skip, b.n_fields, b.columns, b.bound(), 4096), b.definition())


def test_rule_equals_the_definition_on_random_batches():
    for seed in range(BC.N_RANDOM):
        b = BC.random_batch(seed)
        buf, table = b.layout(4096)
        same(BC.batch_rule(buf, table, b.skip, b.n_fields, b.columns, b.bound(), 4096), b.definition())


def test_the_stated_results_of_a_few_batches():
    off, cnt, cols, ok = BC.BATCHES["fewer_lines_than_skip_between"].definition()
    assert off.tolist() == [0, 2, 2, 5] and cols[0].tolist() == [960, 961, 1, 3, 5] and cols[1].tolist() == [13, 9, 2, 4, 6]
    off, cnt, cols, ok = BC.BATCHES["no_newline_before_garbage"].definition()
    assert off.tolist() == [0, 2, 4] and cols[0].tolist() == [1, 5, 77, 78] and cols[1].tolist() == [2.5, 6.5, 8.5, 9.5]
    off, cnt, cols, ok = BC.BATCHES["bad_file_2_of_4"].definition()
    assert [c[1] for c in cnt] == [0, 0, CC.ERR_DIGITS, 0] and cnt[2][2] == (2, 1, CC.ERR_DIGITS)   # file-local row
    assert off.tolist() == [0, 3, 8, 12, 14] and ok.tolist() == [True] * 8 + [False] * 4 + [True] * 2
    off, cnt, cols, ok = BC.BATCHES["two_bad_files"].definition()
    assert [e for e, c in enumerate(cnt) if c[1]] == [1, 3]
    off, cnt, cols, ok = BC.BATCHES["max_rows_runs_out_in_file_1"].definition()
    assert off.tolist() == [0, 2, 4, 4] and cnt == [(2, 0, None), (2, CC.ERR_ROWS, (2, 0, CC.ERR_ROWS)),
                                                    (0, CC.ERR_ROWS, (0, 0, CC.ERR_ROWS))]
    off, cnt, cols, ok = BC.BATCHES["max_rows_exactly_at_a_file_end"].definition()
    assert [c[1] for c in cnt] == [0, 0, 0, CC.ERR_ROWS] and cnt[3][2] == (0, 0, CC.ERR_ROWS)
    assert BC.BATCHES["2049_one_row_files"].definition()[0].tolist() == list(range(2050))


@pytest.mark.parametrize("name", ["no_newline_before_garbage", "fewer_lines_than_skip_between", "header_only_between"])
def test_concatenate_and_parse_once_is_not_the_batch(name):
    """what a batch call must not be: gtf_csv_parse's rule on the files' bytes joined, or on the buffer
    with its padding, gives other rows than the files give one by one"""
    b = BC.BATCHES[name]
    off, cnt, cols, ok = b.definition()
    assert not any(c[1] for c in cnt)
    for text in (b"".join(b.files), b.layout(4096)[0]):
        n, naive, error, _ = CC.parse_rule(text, b.skip, b.n_fields, b.columns)
        assert error or n != off[-1] or any(not np.array_equal(bits(x), bits(y)) for x, y in zip(naive, cols))
    # the clamp is per file: the lines a short file lacks are not taken from its neighbour
    if name == "fewer_lines_than_skip_between":
        n, naive, error, _ = CC.parse_rule(b"".join(f if f.endswith(b"\n") else f + b"\n" for f in b.files), 0, 3, b.columns)
        lines = [len(CC.lines_of(f)) for f in b.files]
        assert lines == [4, 1, 5] and sum(max(k - 2, 0) for k in lines) == 5 != max(sum(lines) - 2 * 3, 0)


# ------------------------------------------------------------------ the host side of gtf.csvdev
def test_batch_layout():
    sizes = [0, 1, 4095, 4096, 4097, 0, 0, 10000, 0]
    starts, total = csvdev.batch_layout(sizes, 4096)
    assert all(s % 4096 == 0 and s % 16 == 0 for s in starts) and starts == sorted(starts)
    assert starts == [0, 0, 4096, 8192, 12288, 20480, 20480, 20480, 32768] and total == 32768
    for (s, n), nxt in zip(zip(starts, sizes), starts[1:] + [total]):
        assert s + n <= nxt                                    # a chunk belongs to one file
    assert csvdev.batch_layout([], 4096) == ([], 0)
    with pytest.raises(ValueError):
        csvdev.batch_layout([3, -1], 4096)


def test_read_batch_reads_into_place(tmp_path):
    files = [b"a,b\n1,2\n", b"", CC.filler(4096), b"a,b\n3,4"]
    paths = []
    for k, f in enumerate(files):
        paths.append(str(tmp_path / ("f%d.csv" % k)))
        open(paths[-1], "wb").write(f)
    for given in (files, paths, [files[0], paths[1], paths[2], bytearray(files[3])]):
        buf, starts, sizes = csvdev.read_batch(given, 4096, fill=BC.GARBAGE)
        assert isinstance(buf, bytearray) and sizes == [len(f) for f in files] and starts == [0, 4096, 4096, 8192]
        poison = (BC.GARBAGE * (len(buf) // len(BC.GARBAGE) + 1))[:len(buf)]
        owned = np.zeros(len(buf), bool)
        for f, s in zip(files, starts):
            assert bytes(buf[s:s + len(f)]) == f
            owned[s:s + len(f)] = True
        a, p = np.frombuffer(bytes(buf), np.uint8), np.frombuffer(poison, np.uint8)
        assert np.array_equal(a[~owned], p[~owned])            # the padding is nobody's: left as it was
    assert len(csvdev.read_batch(files, 4096)[0]) == 12288
    # the test batches lie the same way, and their padding is the poison
    b = BC.BATCHES["empty_files_first_middle_last"]
    buf, table = b.layout(4096)
    assert [s for s, _ in table] == csvdev.batch_layout([len(f) for f in b.files], 4096)[0]
    assert b'"' in buf and all(b'"' not in f for f in b.files)


def test_headers_that_resolve_differently_are_seen_on_the_host():
    cols = (("id", "int64"), ("x", "float64"))
    files = [b"id,x\n1,2.5\n", b"", b"id,x\n", b"x,id\n2.5,1\n", b"id,x\n3,4.5\n"]
    buf, starts, sizes = csvdev.read_batch(files, 4096)
    layout, bad, reason = csvdev.batch_request(buf, starts, sizes, cols, 1)
    assert layout is None and bad == 3 and "file 3" in reason and "[1, 0]" in reason and "file 0" in reason
    layout, bad, reason = csvdev.batch_request(*csvdev.read_batch(files[:3] + files[4:], 4096), cols, 1)
    assert layout == (2, ((0, 0), (1, 1))) and bad is None and reason is None
    # another number of fields is another layout, even where the wanted fields agree
    layout, bad, _ = csvdev.batch_request(*csvdev.read_batch([files[0], b"id,x,y\n1,2.5,3\n"], 4096), cols, 1)
    assert layout is None and bad == 1
    # a file with fewer lines than skip_lines has no row and fits any layout; by index no header is read
    layout, bad, _ = csvdev.batch_request(*csvdev.read_batch([b"3 2\n", b"3 2\na,b,c\n1,2,3\n"], 4096),
                                          ((0, "int64"), (1, "int64")), 2)
    assert layout == (3, ((0, 0), (1, 0))) and bad is None
    with pytest.raises(KeyError):
        csvdev.batch_request(*csvdev.read_batch([b"id,y\n1,2\n"], 4096), cols, 1)
    assert csvdev.header_fields(bytearray(b"zzz\na,b\nq"), 1, b",", 4, 8) == ["a", "b"]
