"""gtf_graph_prepare (the schedules and slot tables built on the GPU) without a GPU: the
header declares the two entry points and the library exports them, the ctypes mirror of
gtf_graph_tables matches the header, the workspace size behaves, and every rejection that
the header promises "before any launch" really comes back from the host."""
import ctypes
import os
import re
import subprocess
import tempfile

import pytest

from gtf import _native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "gtf.h")
NAMES = ("gtf_graph_prepare_workspace_bytes", "gtf_graph_prepare")
COUNTS = ("n_g2", "n_g4", "n_g6", "n_g8", "n_g12", "n_g16", "n_g32", "n_g64", "n_big", "n_o4", "n_o8", "n_o16")


def _lib():
    if not os.path.exists(nat.LIB_PATH):
        pytest.skip("libgtf.so not built (run __graft_entry__.build())")
    return nat.lib()


def test_header_declares_and_library_exports():
    # the pattern tests/test_capi.py finds declarations with
    declared = set(re.findall(r"^\s*(?:int|size_t|const char\*)\s+(gtf_\w+)\s*\(", open(HDR).read(), re.M))
    assert set(NAMES) <= declared
    assert set(NAMES) <= set(nat.SYMBOLS)
    _lib()
    out = subprocess.run(["nm", "-D", "--defined-only", nat.LIB_PATH], capture_output=True, text=True).stdout
    assert set(NAMES) <= set(re.findall(r" T (gtf_\w+)", out))


def test_tables_struct_matches_header():
    """offsetof()/sizeof() of gtf_graph_tables from a C probe against the ctypes mirror"""
    cls = nat.GtfGraphTables
    lines = ['  printf("%s %%zu\\n", offsetof(gtf_graph_tables, %s));' % (f, f) for f, _ in cls._fields_]
    lines.append('  printf("sizeof %zu\\n", sizeof(gtf_graph_tables));')
    probe = "#include <stdio.h>\n#include <stddef.h>\n#include \"gtf.h\"\nint main(void) {\n%s\n  return 0;\n}\n" % \
        "\n".join(lines)
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "p.c")
        open(c, "w").write(probe)
        exe = os.path.join(d, "p")
        subprocess.check_call(["gcc", "-I", os.path.dirname(HDR), c, "-o", exe])
        got = dict(l.rsplit(" ", 1) for l in subprocess.check_output([exe], text=True).split("\n") if l)
    assert len(got) == len(cls._fields_) + 1 == 15
    assert ctypes.sizeof(cls) == int(got.pop("sizeof"))
    for f, off in got.items():
        assert getattr(cls, f).offset == int(off), f


def test_workspace_size():
    L = _lib()
    ws = L.gtf_graph_prepare_workspace_bytes
    assert ws(0, 0, 0) > 0
    base = (1000, 6000, 5000)
    for axis in range(3):
        last = 0
        for n in (0, 1, 255, 256, 257, 1000, 4097, 100000, 1 << 20):
            a = list(base)
            a[axis] = n
            assert ws(*a) >= last, (axis, n)
            last = ws(*a)
    assert ws(1000, 6000, 5000) >= 4 * 6000 + 12 * 1000   # a slot_dst and a schedule of its own


def _call(L, g, t=None, ws_bytes=None):
    """gtf_graph_prepare with a host buffer as `workspace`: only for calls that the library must
    refuse, or finish, on the host (nothing may be launched, so nothing reads the buffer)"""
    need = L.gtf_graph_prepare_workspace_bytes(max(g.n_nodes, 0), max(g.n_slots, 0), max(g.n_edges, 0))
    n = need if ws_bytes is None else ws_bytes(need)
    buf = ctypes.create_string_buffer(max(n, 1))
    t = t or nat.GtfGraphTables()
    return L.gtf_graph_prepare(ctypes.byref(g), ctypes.byref(t), ctypes.cast(buf, ctypes.c_void_p), ctypes.c_size_t(n),
                               ctypes.c_void_p(0))


def test_abi_mismatch_is_refused_on_the_host():
    L = _lib()
    g = nat.GtfGraph(n_nodes=0)
    g.abi_version = nat.ABI_VERSION + 1
    assert _call(L, g) == -3 and b"ABI mismatch" in L.gtf_last_error()
    g = nat.GtfGraph(n_nodes=0)
    g.struct_size -= 8
    assert _call(L, g) == -3 and b"ABI mismatch" in L.gtf_last_error()


@pytest.mark.parametrize("sizes", [(-1, 0, 0), (4, -1, 0), (4, 0, -2)])
def test_negative_sizes_are_refused_on_the_host(sizes):
    L = _lib()
    g = nat.GtfGraph(n_nodes=sizes[0], n_slots=sizes[1], n_edges=sizes[2])
    assert _call(L, g) == -2
    assert L.gtf_last_error() and b"negative" in L.gtf_last_error()


def test_missing_base_array_is_refused_on_the_host():
    L = _lib()
    g = nat.GtfGraph(n_nodes=3)   # slot_ptr NULL with N > 0
    assert _call(L, g) == -2
    assert L.gtf_last_error() and b"slot_ptr" in L.gtf_last_error()


def test_short_workspace_is_refused_on_the_host():
    L = _lib()
    g = nat.GtfGraph(n_nodes=0)
    assert _call(L, g, ws_bytes=lambda need: need - 1) == -2
    assert L.gtf_last_error() and b"workspace" in L.gtf_last_error()
    # the full size: an empty graph returns 0 with zero counts and NULL tables, nothing launched
    for f in COUNTS:
        setattr(g, f, 7)
    g.sched = ctypes.c_void_p(64)
    assert _call(L, g) == 0
    assert all(getattr(g, f) == 0 for f in COUNTS) and not g.sched
