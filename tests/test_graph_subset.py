"""The device subset (gtf_graph_subset_plan / _apply, gtf_subset_gather, gtf_refresh_send_mw)
without a GPU: the header declares the five entry points and the library exports them, the
ctypes mirrors of the three new structs match the header, the workspace size behaves, and
every refusal that the header promises on the host really comes back before any launch."""
import ctypes
import os
import re
import subprocess
import tempfile

import pytest

from gtf import _native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "gtf.h")
NAMES = ("gtf_graph_subset_workspace_bytes", "gtf_graph_subset_plan", "gtf_graph_subset_apply",
         "gtf_subset_gather", "gtf_refresh_send_mw")
SIZES = (0, 1, 255, 256, 257, 1000, 4097, 100000, 1 << 20)


def _lib():
    if not os.path.exists(nat.LIB_PATH):
        pytest.skip("libgtf.so not built (run __graft_entry__.build())")
    return nat.lib()


def test_header_declares_and_library_exports():
    src = open(HDR).read()
    declared = set(re.findall(r"^\s*(?:int|size_t|const char\*)\s+(gtf_\w+)\s*\(", src, re.M))
    assert set(NAMES) <= declared
    assert set(NAMES) <= set(nat.SYMBOLS)
    _lib()
    out = subprocess.run(["nm", "-D", "--defined-only", nat.LIB_PATH], capture_output=True, text=True).stdout
    assert set(NAMES) <= set(re.findall(r" T (gtf_\w+)", out))
    # every declaration cites the reference lines and the host definition it restates
    for name in NAMES:
        at = src.index(" %s(" % name)
        comment = src[src.rindex("/*", 0, at):at]
        assert "extract_track_candidates.py:459-467" in comment and "gtf/graph.py" in comment, name
    assert "#define GTF_ABI_VERSION 8u" in src and nat.ABI_VERSION == 8


def test_structs_match_header():
    """offsetof()/sizeof() of the three new structs from a C probe against the ctypes mirrors"""
    py = {"gtf_subset_counts": nat.GtfSubsetCounts, "gtf_subset_out": nat.GtfSubsetOut, "gtf_column": nat.GtfColumn}
    lines = []
    for t, cls in py.items():
        lines += ['  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (t, f, t, f) for f, _ in cls._fields_]
        lines.append('  printf("sizeof.%s %%zu\\n", sizeof(%s));' % (t, t))
    for i, k in enumerate(("COPY", "ZERO_ORPHAN", "NAN_ORPHAN", "ZERO_ALL")):
        lines.append('  printf("fill.%s %%d\\n", GTF_COL_%s);' % (k, k))
    probe = "#include <stdio.h>\n#include <stddef.h>\n#include \"gtf.h\"\nint main(void) {\n%s\n  return 0;\n}\n" % \
        "\n".join(lines)
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "p.c")
        open(c, "w").write(probe)
        exe = os.path.join(d, "p")
        subprocess.check_call(["gcc", "-I", os.path.dirname(HDR), c, "-o", exe])
        got = dict(l.rsplit(" ", 1) for l in subprocess.check_output([exe], text=True).split("\n") if l)
    assert len(got) == sum(len(c._fields_) + 1 for c in py.values()) + 4 == 4 + 1 + 8 + 1 + 4 + 1 + 4
    for k, v in got.items():
        t, f = k.split(".")
        if t == "sizeof":
            assert ctypes.sizeof(py[f]) == int(v), k
        elif t == "fill":
            assert getattr(nat, "COL_" + f) == int(v), k
        else:
            assert getattr(py[t], f).offset == int(v), k


def test_workspace_size():
    L = _lib()
    ws = L.gtf_graph_subset_workspace_bytes
    assert ws(0, 0, 0, 0) > 0
    base = (1000, 6000, 5000, 40)
    for axis in range(4):
        last = 0
        for n in SIZES:
            a = list(base)
            a[axis] = n
            assert ws(*a) >= last, (axis, n)
            last = ws(*a)
    # both node maps, both slot maps and the per-node offsets live there
    assert ws(1000, 6000, 5000, 40) >= 8 * 6000 + 16 * 1000


def _plan(L, g, ws_bytes=None, keep=True, n_sub=1, ranks=True, sub=True, counts=None):
    """gtf_graph_subset_plan with host buffers and a NULL stream: only for calls that the library
    must refuse, or finish, on the host (nothing may be launched, so nothing reads the buffers)"""
    need = L.gtf_graph_subset_workspace_bytes(max(g.n_nodes, 0), max(g.n_slots, 0), max(g.n_edges, 0), max(n_sub, 0))
    n = need if ws_bytes is None else ws_bytes(need)
    buf = ctypes.create_string_buffer(max(n, 1))
    arr = ctypes.create_string_buffer(64)
    a = ctypes.cast(arr, ctypes.c_void_p)
    null = ctypes.c_void_p(0)
    counts = counts if counts is not None else nat.GtfSubsetCounts(7, 7, 7, 7)
    rc = L.gtf_graph_subset_plan(ctypes.byref(g), a if ranks else null, a if ranks else null, a if sub else null,
                                 n_sub, a if keep else null, ctypes.cast(buf, ctypes.c_void_p), ctypes.c_size_t(n),
                                 ctypes.byref(counts), null)
    return rc, counts


def test_abi_mismatch_is_refused_on_the_host():
    L = _lib()
    g = nat.GtfGraph(n_nodes=0)
    g.abi_version = nat.ABI_VERSION + 1
    assert _plan(L, g)[0] == -3 and b"ABI mismatch" in L.gtf_last_error()
    g = nat.GtfGraph(n_nodes=0)
    g.struct_size -= 8
    assert _plan(L, g)[0] == -3 and b"ABI mismatch" in L.gtf_last_error()
    out = nat.GtfSubsetOut()
    buf = ctypes.create_string_buffer(4096)
    ws = ctypes.cast(buf, ctypes.c_void_p)
    assert L.gtf_graph_subset_apply(ctypes.byref(g), ws, ctypes.byref(out), None) == -3
    assert L.gtf_refresh_send_mw(ctypes.byref(g), ws, ws, ws, None) == -3


@pytest.mark.parametrize("sizes", [(-1, 0, 0, 1), (4, -1, 0, 1), (4, 0, -2, 1), (4, 0, 0, -1)])
def test_negative_sizes_are_refused_on_the_host(sizes):
    L = _lib()
    g = nat.GtfGraph(n_nodes=sizes[0], n_slots=sizes[1], n_edges=sizes[2])
    assert _plan(L, g, n_sub=sizes[3])[0] == -2
    assert L.gtf_last_error() and b"negative" in L.gtf_last_error()


def test_missing_arrays_are_refused_on_the_host():
    L = _lib()
    g = nat.GtfGraph(n_nodes=3)   # slot_ptr NULL with N > 0
    assert _plan(L, g)[0] == -2
    assert L.gtf_last_error() and b"slot_ptr" in L.gtf_last_error()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    g = nat.GtfGraph(n_nodes=3, slot_ptr=p, out_ptr=p)
    assert _plan(L, g, keep=False)[0] == -2
    assert L.gtf_last_error() and b"keep" in L.gtf_last_error()
    assert _plan(L, g, sub=False)[0] == -2 and b"sub_id" in L.gtf_last_error()
    g = nat.GtfGraph(n_nodes=3, n_slots=2, slot_ptr=p, out_ptr=p, slot_src=p, is_edge=p)
    assert _plan(L, g, ranks=False)[0] == -2 and b"tse_rank" in L.gtf_last_error()
    g = nat.GtfGraph(n_nodes=0, n_slots=2, slot_src=p, is_edge=p)
    assert _plan(L, g)[0] == -2 and b"without nodes" in L.gtf_last_error()


def test_short_workspace_is_refused_and_an_empty_graph_plans_to_nothing():
    L = _lib()
    g = nat.GtfGraph(n_nodes=0)
    assert _plan(L, g, ws_bytes=lambda need: need - 1)[0] == -2
    assert L.gtf_last_error() and b"workspace" in L.gtf_last_error()
    rc, c = _plan(L, g)
    assert rc == 0 and (c.n_nodes, c.n_slots, c.n_edges, c.n_sub) == (0, 0, 0, 0)
    rc, c = _plan(L, g, n_sub=0, keep=False, ranks=False, sub=False)   # nothing is needed of an empty graph
    assert rc == 0 and (c.n_nodes, c.n_slots, c.n_edges, c.n_sub) == (0, 0, 0, 0)


def test_gather_refusals_on_the_host():
    L = _lib()
    buf = ctypes.create_string_buffer(4096)
    ws = ctypes.cast(buf, ctypes.c_void_p)
    p = ctypes.c_void_p(ctypes.addressof(buf) + 256)
    assert L.gtf_subset_gather(ws, 0, None, 0, None) == 0
    assert L.gtf_subset_gather(ws, 1, None, 0, None) == 0

    def gather(axis, *cols):
        arr = (nat.GtfColumn * len(cols))(*cols)
        return L.gtf_subset_gather(ws, axis, arr, len(cols), None)

    good = nat.GtfColumn(p, p, 8, nat.COL_COPY)
    for rb in (0, -8):
        assert gather(1, good, nat.GtfColumn(p, p, rb, nat.COL_COPY)) == -2
        assert b"row_bytes" in L.gtf_last_error()
    assert gather(2, good) == -2 and b"axis" in L.gtf_last_error()
    assert gather(1, nat.GtfColumn(p, p, 8, 4)) == -2 and b"fill" in L.gtf_last_error()
    assert gather(1, nat.GtfColumn(p, None, 8, nat.COL_COPY)) == -2
    assert gather(1, nat.GtfColumn(None, p, 8, nat.COL_COPY)) == -2
    assert gather(1, nat.GtfColumn(p, p, 12, nat.COL_NAN_ORPHAN)) == -2 and b"NAN_ORPHAN" in L.gtf_last_error()


def test_refresh_send_mw_refusals_on_the_host():
    L = _lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.gtf_refresh_send_mw(ctypes.byref(nat.GtfGraph(n_nodes=0)), None, None, None, None) == 0
    g = nat.GtfGraph(n_nodes=2, n_slots=-1)
    assert L.gtf_refresh_send_mw(ctypes.byref(g), p, p, p, None) == -2 and b"negative" in L.gtf_last_error()
    g = nat.GtfGraph(n_nodes=2, n_slots=2, slot_src=p, is_edge=p)
    assert L.gtf_refresh_send_mw(ctypes.byref(g), p, p, p, None) == -2 and b"slot_ptr" in L.gtf_last_error()
    g = nat.GtfGraph(n_nodes=2, n_slots=2, slot_ptr=p, slot_src=p, is_edge=p)
    assert L.gtf_refresh_send_mw(ctypes.byref(g), p, None, p, None) == -2
    assert L.gtf_refresh_send_mw(ctypes.byref(g), p, p, p, None) == -2 and b"aliases" in L.gtf_last_error()
