"""gtf_event_pack / gtf_fill_columns without a GPU: the entry points are declared, exported and
bound, the new structs match their ctypes mirrors, the ABI version is unchanged, and every bad
argument is refused on the host (-2 with a message) before any device work."""
import ctypes
import os
import re
import subprocess
import tempfile

import pytest

from gtf import _native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "gtf.h")
NEW = ("gtf_event_pack", "gtf_fill_columns")
Z = ctypes.c_void_p(0)
PTR = ctypes.c_void_p(4096)   # never dereferenced: every call below is refused before any device work


def _lib():
    if not os.path.exists(nat.LIB_PATH):
        pytest.fail("libgtf.so not built (run __graft_entry__.build())")
    return nat.lib()


def test_symbols_declared_exported_and_listed():
    src = open(HDR).read()
    declared = set(re.findall(r"^\s*(?:int|size_t|const char\*)\s+(gtf_\w+)\s*\(", src, re.M))
    _lib()
    out = subprocess.run(["nm", "-D", "--defined-only", nat.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (gtf_\w+)", out))
    for s in NEW:
        assert s in declared and s in exported and s in nat.SYMBOLS, s


def test_declarations_cite_the_reference():
    """every new declaration names the reference lines it replaces, as the rest of the header does"""
    src = open(HDR).read()
    for decl in ("typedef struct gtf_event_cols", "typedef struct gtf_event_out", "int gtf_event_pack(",
                 "typedef struct gtf_fill_column", "int gtf_fill_columns("):
        at = src.index(decl)
        comment = src[src.rindex("/*", 0, at):at]
        assert "event_conversion.py:53-101" in comment or "helper.py:" in comment, decl


def test_abi_version_unchanged():
    ver = re.search(r"#define GTF_ABI_VERSION (\d+)u", open(HDR).read())
    assert ver and int(ver.group(1)) == nat.ABI_VERSION == 8
    cap = re.search(r"#define GTF_FILL_MAX_COLUMNS (\d+)", open(HDR).read())
    assert cap and int(cap.group(1)) == nat.FILL_MAX_COLUMNS == 32


def test_new_structs_match_header():
    """the offsetof() / sizeof() probe of test_capi.py on the new structs, and gtf_event_csr (which
    gtf_event_pack reads) still at its layout"""
    py = {"gtf_event_cols": nat.GtfEventCols, "gtf_event_out": nat.GtfEventOut,
          "gtf_fill_column": nat.GtfFillColumn, "gtf_event_csr": nat.GtfEventCsr}
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


def _col(dst=PTR, rows=1, row_bytes=8, pattern=0):
    return nat.GtfFillColumn(dst, rows, row_bytes, 0, pattern)


@pytest.mark.parametrize("cols,n,msg", [
    ([_col()], -1, b"n_cols"),
    ([_col()] * 33, 33, b"n_cols"),
    (None, 1, b"null column table"),
    ([_col(rows=-1)], 1, b"negative rows"),
    ([_col(row_bytes=0)], 1, b"row_bytes"),
    ([_col(row_bytes=-8)], 1, b"row_bytes"),
    ([_col(row_bytes=2)], 1, b"row_bytes"),
    ([_col(row_bytes=12)], 1, b"row_bytes"),
    ([_col(), _col(row_bytes=3, rows=0)], 2, b"row_bytes"),
    ([_col(dst=Z, rows=5)], 1, b"null destination"),
    ([_col(dst=ctypes.c_void_p(4100), row_bytes=24)], 1, b"aligned"),
    ([_col(dst=ctypes.c_void_p(4098), row_bytes=4)], 1, b"aligned"),
])
def test_fill_columns_refuses_bad_arguments(cols, n, msg):
    L = _lib()
    arr = (nat.GtfFillColumn * len(cols))(*cols) if cols is not None else None
    rc = L.gtf_fill_columns(arr, n, Z)
    assert rc == -2 and b"gtf_fill_columns" in L.gtf_last_error() and msg in L.gtf_last_error(), L.gtf_last_error()


def test_fill_columns_nothing_to_do_is_fine_without_a_device():
    L = _lib()
    assert L.gtf_fill_columns(None, 0, Z) == 0
    cols = [_col(dst=Z, rows=0, row_bytes=rb) for rb in (1, 4, 8, 24, 32, 40)]
    assert L.gtf_fill_columns((nat.GtfFillColumn * len(cols))(*cols), len(cols), Z) == 0


def _ev(n_nodes=4, n_rows=0, n_edges=0, n_sub=4, order=PTR, node_id=PTR, sub_id=PTR):
    return nat.GtfEventCsr(n_nodes, n_rows, node_id, Z, Z, order, sub_id, PTR, Z, Z, PTR, Z, n_edges, n_sub, 0)


ALL_IN = nat.GtfEventCols(PTR, PTR, PTR, PTR, PTR)
ALL_OUT = nat.GtfEventOut(PTR, PTR, PTR, PTR, PTR, PTR)


@pytest.mark.parametrize("ev,cols,out,msg", [
    (None, ALL_IN, ALL_OUT, b"null gtf_event_csr"),
    (_ev(), ALL_IN, None, b"null gtf_event_out"),
    (_ev(n_nodes=-1), ALL_IN, ALL_OUT, b"negative sizes"),
    (_ev(n_rows=-1), ALL_IN, ALL_OUT, b"negative sizes"),
    (_ev(n_edges=-1), ALL_IN, ALL_OUT, b"negative sizes"),
    (_ev(n_sub=-1), ALL_IN, ALL_OUT, b"negative sizes"),
    (_ev(n_nodes=2 ** 31), ALL_IN, ALL_OUT, b"too large"),
    (_ev(order=Z), ALL_IN, ALL_OUT, b"order"),
    (_ev(node_id=Z), ALL_IN, ALL_OUT, b"node_id"),
    (_ev(sub_id=Z), ALL_IN, ALL_OUT, b"sub_id"),
    (_ev(order=Z, node_id=Z, sub_id=Z), None, nat.GtfEventOut(Z, Z, Z, Z, Z, PTR), b"sub_id"),   # solo alone
    (_ev(order=Z), None, nat.GtfEventOut(Z, Z, Z, PTR, Z, PTR), b"order"),
    (_ev(), None, ALL_OUT, b"null gtf_event_cols"),
    (_ev(), nat.GtfEventCols(PTR, PTR, PTR, Z, PTR), ALL_OUT, b"(x, y, z, r)"),
    (_ev(), nat.GtfEventCols(PTR, PTR, PTR, PTR, Z), ALL_OUT, b"layer_id"),
    (_ev(), nat.GtfEventCols(PTR, PTR, PTR, PTR, Z), nat.GtfEventOut(Z, Z, Z, Z, PTR, Z), b"layer_id"),
])
def test_event_pack_refuses_bad_arguments(ev, cols, out, msg):
    L = _lib()
    ref = lambda s: ctypes.byref(s) if s is not None else None  # noqa: E731
    rc = L.gtf_event_pack(ref(ev), ref(cols), ref(out), Z)
    assert rc == -2 and b"gtf_event_pack" in L.gtf_last_error() and msg in L.gtf_last_error(), L.gtf_last_error()


def test_event_pack_nothing_to_do_is_fine_without_a_device():
    L = _lib()
    assert L.gtf_event_pack(ctypes.byref(_ev(n_nodes=0, n_sub=0)), ctypes.byref(ALL_IN), ctypes.byref(ALL_OUT), Z) == 0
    none = nat.GtfEventOut(Z, Z, Z, Z, Z, Z)
    assert L.gtf_event_pack(ctypes.byref(_ev()), None, ctypes.byref(none), Z) == 0
